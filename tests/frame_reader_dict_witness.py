"""The witness for the incremental frame readers with a dictionary set (k4lz4_frame_read_dictset_batch):
frame_reader_witness.WitnessReader with three things changed --

  _read_header    a DictID resolves against the call's id table (the first entry whose id equals it) instead of being refused;
                  no set, or no entry under that id, is K4LZ4_FRAME_DICTIONARY where the plain reader reports it
  independent     LZ4BlockDecoder whose Decode is the engine's LZ4_decompress_safe_usingDict with the entry's kept bytes (the last
                  64 KiB of the dictionary) somewhere else in memory
  chained         LZ4ChainDecoder after one Inject(kept bytes): the injected bytes are the history and are never delivered

The engine stays the reference's compiled one (frame_reader_witness.engine()).  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import struct

import xxhash

import frame_reader_witness as W
from frame_reader_witness import BLOCK, BLOCK_SIZE, DICTIONARY, HEADER_SUM, K64, MAGIC, VERSION, BAD_MAGIC, Defect


class DictBlockDecoder(W.BlockDecoder):
    """LZ4BlockDecoder over LZ4_decompress_safe_usingDict: every block sees the kept bytes and never another block"""

    def __init__(self, block_size: int, kept: bytes):
        super().__init__(block_size)
        self.kept = (C.c_uint8 * max(len(kept), 1)).from_buffer_copy(kept or b"\0")
        self.kept_len = len(kept)

    def decode(self, src: bytes) -> int:
        decoded = 0 if len(src) <= 0 else W.engine().decompress_using_dict(src, self.base, self.output_length, C.addressof(self.kept),
                                                                             self.kept_len)
        if len(src) > 0 and decoded <= 0:
            decoded = -1
        if decoded < 0:
            raise Defect(BLOCK)
        self.output_index = decoded
        return decoded


class DictWitnessReader(W.WitnessReader):
    """entries: the set's dictionaries (whole; the last 64 KiB are kept), ids: entry e answers to DictID ids[e]; entries None: no set"""

    def __init__(self, source: bytes, entries=None, ids=None, max_block_size: int = 4 << 20):
        super().__init__(source, max_block_size)
        self.kept = None if entries is None else [bytes(e)[-K64:] for e in entries]
        self.ids = None if entries is None else [int(i) for i in ids]
        self.entry = None                   # the open frame's entry (None: none)
        self.entries_seen = []              # per frame opened, in order
        self.block_len = 0                  # what the last block read decoded to (read plans look at it)

    def _read_block(self) -> int:
        self.block_len = super()._read_block()
        return self.block_len

    def _read_header(self) -> bool:                                       # WitnessReader._read_header, the DictID resolved
        m = self._take(4, optional=True)
        if m is None:
            return False
        if struct.unpack("<I", m)[0] != MAGIC:
            raise Defect(BAD_MAGIC)
        head = self._take(2)
        flg, bd = head[0], head[1]
        if (flg >> 6) & 0x11 != 1:
            raise Defect(VERSION)
        chaining, bsum = ((flg >> 5) & 1) == 0, ((flg >> 4) & 1) != 0
        has_size, csum, has_dict = ((flg >> 3) & 1) != 0, ((flg >> 2) & 1) != 0, (flg & 1) != 0
        clen, dict_id = None, None
        if has_size:
            w = self._take(8); head += w
            clen = struct.unpack("<Q", w)[0]
        if has_dict:
            w = self._take(4); head += w
            dict_id = struct.unpack("<I", w)[0]
        actual = (xxhash.xxh32(head, seed=0).intdigest() >> 8) & 0xFF
        if self._take(1)[0] != actual:
            raise Defect(HEADER_SUM)
        block_size = {7: 4 << 20, 6: 1 << 20, 5: 256 << 10, 4: 64 << 10}.get((bd >> 4) & 7, 64 << 10)
        entry = None
        if has_dict:
            if self.ids is None or dict_id not in self.ids:
                raise Defect(DICTIONARY)
            entry = self.ids.index(dict_id)                               # the first entry whose id equals it
        if block_size > self.max_block_size:
            raise Defect(BLOCK_SIZE)
        if csum:
            self.checksum = xxhash.xxh32(seed=0)
        self.descriptor = (clen, csum, chaining, bsum, block_size)
        kept = self.kept[entry] if entry is not None else b""
        if chaining:
            self.decoder = W.ChainDecoder(block_size, 0)
            if kept:
                self.decoder.inject(kept)                                 # the history; not delivered, not hashed, not counted
        else:
            self.decoder = DictBlockDecoder(block_size, kept) if kept else W.BlockDecoder(block_size)
        self.decoded = 0
        self.entry = entry
        self.entries_seen.append(entry)
        return True
