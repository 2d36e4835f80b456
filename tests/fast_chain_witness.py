"""The witness for chained fast streams: the system liblz4 (1.9.3) driven through hc_chain_witness's transcription of
LZ4EncoderBase's ring buffer (RingEncoder) with LZ4FastChainEncoder's calls (Encoders/LZ4FastChainEncoder.cs: a zeroed LZ4_stream_t,
LZ4_compress_fast_continue(..., 1), LZ4_saveDict).  Test infrastructure only.

`Lz4FastChainCodec` gives real bytes and reads the stream context (hashTable, currentOffset, dictSize) out of liblz4's LZ4_stream_t --
1.9.3's internal layout, no header for it is installed, so the version is asserted and the layout checked by hand (check_layout).
`FastTableCodec` follows only the context's fields the way LL64.fast.cs:582-667 and LL.tools.cs:195-213 do and records, per block,
(start, length, dictSize, dictSmall) in content coordinates and the arm taken -- what encoders.fast_chain_blocks has to reproduce."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

import hc_chain_witness as HW
from hc_chain_witness import RingEncoder, encode_stream, compress_bound, decode_chain, frame_from_blocks  # noqa: F401

K64 = 65536
STATE_BYTES = 16416                     # sizeof(LZ4_stream_t), LZ4_STREAMSIZE in 1.9.3
OFF_CURRENT, OFF_TABLETYPE, OFF_DICTSIZE = 16384, 16388, 16408    # hashTable[4096]; currentOffset; tableType; dictionary; dictCtx; dictSize


class FastTableCodec:
    """the stream context's fields of LZ4_compress_fast_continue / LZ4_saveDict, no bytes (offsets into the ring stand in for addresses)"""

    def __init__(self, current_offset: int = 0):
        self.cur = current_offset
        self.dictionary: Optional[int] = None     # NULL
        self.dict_size = 0
        self.consumed = 0
        self.blocks: List[Tuple[int, int, int, bool]] = []
        self.arms: List[str] = []
        self.ring_index: List[int] = []

    def encode_block(self, buf, at: int, n: int, cap: int):
        dict_end = None if self.dictionary is None else self.dictionary + self.dict_size
        assert self.cur + n <= 1 << 31, "LZ4_renormDictT is not modelled"
        if ((self.dict_size - 1) & 0xffffffff) < 3 and dict_end != at:            # invalidate tiny dictionaries
            self.dict_size, self.dictionary, dict_end = 0, at, at
        if self.dictionary is not None and self.dictionary < at + n < dict_end:    # overlapping input / dictionary
            d = min(dict_end - (at + n), K64)
            self.dict_size = 0 if d < 4 else d
            self.dictionary = dict_end - self.dict_size
        small = self.dict_size < K64 and self.dict_size < self.cur
        self.blocks.append((self.consumed, n, self.dict_size, small))
        self.ring_index.append(at)
        if dict_end == at:
            self.arms.append("withPrefix64k")
            self.dict_size += n
        else:
            self.arms.append("usingExtDict")
            self.dictionary, self.dict_size = at, n
        self.cur += n
        self.consumed += n
        return 1, b""

    def copy_dict(self, buf, ptr: int) -> int:                                      # LZ4_saveDict(ctx, buf, ptr)
        d = min(ptr, K64, self.dict_size)
        self.dictionary, self.dict_size = 0, d
        return d

    def close(self):
        pass


class Lz4FastChainCodec:
    """LZ4FastChainEncoder over liblz4's LZ4_stream_t"""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            L = HW.Lz4HcCodec.lib()
            L.LZ4_createStream.restype = C.c_void_p
            L.LZ4_freeStream.argtypes = [C.c_void_p]
            L.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
            L.LZ4_saveDict.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            assert L.LZ4_versionNumber() == 10903, "the LZ4_stream_t layout read here is liblz4 1.9.3's"
            cls._lib = L
        return cls._lib

    def __init__(self):
        self.L = Lz4FastChainCodec.lib()
        self.ctx = self.L.LZ4_createStream()

    def encode_block(self, buf, at: int, n: int, cap: int):
        dst = (C.c_uint8 * cap)()
        r = self.L.LZ4_compress_fast_continue(self.ctx, C.addressof(buf) + at, dst, n, cap, 1)
        return r, bytes(dst[:max(r, 0)])

    def copy_dict(self, buf, ptr: int) -> int:
        return self.L.LZ4_saveDict(self.ctx, buf, ptr)

    def state(self) -> dict:
        raw = (C.c_uint8 * STATE_BYTES).from_address(self.ctx)
        b = np.frombuffer(bytes(raw), np.uint8)
        return {"hashTable": b[:16384].view("<u4").copy(), "currentOffset": int(b[OFF_CURRENT:OFF_CURRENT + 4].view("<u4")[0]),
                "tableType": int(b[OFF_TABLETYPE:OFF_TABLETYPE + 4].view("<u4")[0]), "dictSize": int(b[OFF_DICTSIZE:OFF_DICTSIZE + 4].view("<u4")[0])}

    def close(self):
        if self.ctx:
            self.L.LZ4_freeStream(self.ctx)
            self.ctx = None


def check_layout() -> None:
    """the word after the table is currentOffset, tableType is byU32 (2), dictSize where 1.9.3 keeps it: one call of a fresh stream"""
    codec = Lz4FastChainCodec()
    enc = RingEncoder(codec, 4096)
    data = np.frombuffer(b"layout check " * 300, np.uint8)[:3000].copy()
    enc.topup(data, 0, data.size)
    enc.encode(False)
    st = codec.state()
    codec.close()
    assert st["currentOffset"] == 3000 and st["tableType"] == 2 and st["dictSize"] == 3000, st
    assert np.count_nonzero(st["hashTable"]) > 10


def witness_stream(content: np.ndarray, block_size: int, extra_blocks: int = 0, allow_copy: bool = True, topups=None):
    """[(outLen as k4lz4_encode_fast_chain_batch reports it, payload)] per block, and the context after the last block (and the ring's
    save behind it).  topups: sizes of the Topup calls (ragged feeding: the blocks are what the ring cuts all the same)."""
    content = np.ascontiguousarray(content, np.uint8)
    codec = Lz4FastChainCodec()
    enc = RingEncoder(codec, block_size, extra_blocks)
    out, pos, k = [], 0, 0
    while pos < content.size:
        want = content.size - pos if topups is None else min(topups[k % len(topups)], content.size - pos)
        k += 1
        pos += enc.topup(content, pos, want)
        if enc.bytes_ready >= enc.block_size:
            out.append(enc.encode(allow_copy))
    if enc.bytes_ready:
        out.append(enc.encode(allow_copy))
    st = codec.state()
    codec.close()
    return out, st


def witness_table(length: int, block_size: int, extra_blocks: int = 0):
    codec = FastTableCodec()
    encode_stream(codec, np.zeros(length, np.uint8), block_size, extra_blocks, allow_copy=False)
    return codec
