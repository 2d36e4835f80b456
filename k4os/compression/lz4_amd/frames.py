"""LZ4 frame format over batched blocks, backed by libk4lz4.so.

Mirrors (K4os.Compression.LZ4.Streams):
  LZ4EncoderSettings / LZ4Descriptor                 LZ4EncoderSettings.cs:8-47, Frames/LZ4Descriptor.cs
  LZ4Frame.Encode / LZ4Frame.Decode                  LZ4Frame.cs (span / buffer-writer overloads)
  frame writer   magic, FLG/BD, header checksum byte, block length with raw bit, block checksum,
                 EndMark, content checksum           Frames/LZ4FrameWriter.cs:57-108,:159-189,
                                                     Frames/LZ4FrameWriter.async.cs:15-27,:75-90
  frame reader                                       Frames/LZ4FrameReader.async.cs:52-136
What runs where: splitting into blocks, the header and the block table are host index work; block
encoding (with the allowCopy rule), block decoding (independent blocks as one batch, chained blocks as
one in-order stream per wavefront) and every XXH32 -- header byte included -- run in the HIP kernels.

Chained frames (ChainBlocks=True) are written at L03_HC and up: LZ4HighChainEncoder's blocks
(k4lz4_encode_hc_chain_batch), every block of every frame of the batch side by side -- the HC tables
depend on the data alone, so a block needs the 64 KiB before it and not the parse of the block before
it.  ExtraMemory sets the encoder's extra blocks as the reference's writer does.

Chained frames below L03_HC -- LZ4FastChainEncoder's, whose hash table holds only the positions its parse
visited, so a stream's blocks are serial -- are written by `encode_fast_chain_frames`
(k4lz4_encode_fast_chain_batch: one wavefront per stream, many streams side by side).

Frames that sit in device memory are read by `decode_frames_device` (k4lz4_decode_frames_device): header walk,
block table, checksums and decoding all on the device, with one wait for the batch's block count.

Differences from the reference, all deliberate:
  * ChainBlocks defaults to False here (the reference: True).  LZ4Frame.Encode / EncodeBatch and
    encode_frames_device still raise NotImplementedException for chained frames at L00_FAST; the
    chained fast writer is encode_fast_chain_frames.  The READER takes both kinds.
  * ContentLength in the header is written when asked for (the reference's writer throws
    NotImplemented, LZ4FrameWriter.cs:86-88) and verified by the reader, like the reference's reader.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from .codec import LZ4Codec, LZ4Level, _ro_view, pack_blocks, make_arena, _batch_args
from .encoders import encode_blocks_packed, encode_hc_chain_packed, encode_fast_chain_packed, hc_chain_blocks, _round_block_size

MAGIC = 0x184D2204
K64, K256, M1, M4 = 64 << 10, 256 << 10, 1 << 20, 4 << 20


class InvalidDataException(Exception):
    """System.IO.InvalidDataException (magic number, header checksum, block / content checksum)"""


class NotImplementedException(Exception):
    """System.NotImplementedException (predefined dictionaries)"""


FAST_CHAIN_REFUSED = ("chained blocks at L00_FAST are not offered: LZ4_compress_fast_continue's hash table holds only the positions "
                      "its parse visited, so every block depends on the parse of the one before it (serial per stream); use "
                      "ChainBlocks=False, or CompressionLevel L03_HC and up")


def _extra_blocks(block_size: int, extra_memory: int) -> int:
    """Streams/Extensions.cs:18-19"""
    return max(block_size if extra_memory > 0 else 0, extra_memory) // block_size


@dataclass
class LZ4EncoderSettings:                     # LZ4EncoderSettings.cs (ChainBlocks default differs, see module docstring)
    ContentLength: Optional[int] = None
    ChainBlocks: bool = False
    BlockSize: int = K64
    ContentChecksum: bool = False
    BlockChecksum: bool = False
    CompressionLevel: LZ4Level = LZ4Level.L00_FAST
    ExtraMemory: int = 0

    @property
    def Dictionary(self):
        return None


@dataclass
class LZ4Descriptor:                          # Frames/LZ4Descriptor.cs
    ContentLength: Optional[int]
    ContentChecksum: bool
    Chaining: bool
    BlockChecksum: bool
    Dictionary: Optional[int]
    BlockSize: int


@dataclass
class FrameInfo:
    """what the reader learns from walking a frame (no payload is touched)"""
    descriptor: LZ4Descriptor
    header: bytes                 # FLG .. before HC: the bytes the header checksum covers
    header_checksum: int
    block_off: List[int] = field(default_factory=list)     # payload offsets inside the frame
    block_len: List[int] = field(default_factory=list)     # payload lengths, bit 31 = raw
    block_checksum: List[int] = field(default_factory=list)
    content_checksum: Optional[int] = None
    consumed: int = 0


def max_block_size_code(block_size: int) -> int:          # LZ4FrameWriter.cs:184-189
    if block_size <= K64:
        return 4
    if block_size <= K256:
        return 5
    if block_size <= M1:
        return 6
    if block_size <= M4:
        return 7
    raise ValueError(f"Invalid block size ${block_size} for this operation")


def max_block_size(code: int) -> int:                     # LZ4FrameReader.cs:56-59
    return {7: M4, 6: M1, 5: K256, 4: K64}.get(code, K64)


def frame_header(d: LZ4Descriptor, dictionary: bool = False) -> bytes:
    """FLG, BD [, content size] [, DictID] -- the bytes covered by the header checksum (LZ4FrameWriter.cs:65-100).  A descriptor's
    Dictionary is written (FLG bit 0, the id after the content size) only for the writer with a DictionarySet (dictionary=True,
    DESIGN.md 4.24); otherwise it is refused as the reference refuses it."""
    if d.Dictionary is not None and not dictionary:
        raise NotImplementedException("Predefined dictionaries feature is not implemented")
    flg = (1 << 6) | ((0 if d.Chaining else 1) << 5) | ((1 if d.BlockChecksum else 0) << 4) | \
          ((1 if d.ContentLength is not None else 0) << 3) | ((1 if d.ContentChecksum else 0) << 2) | (1 if d.Dictionary is not None else 0)
    bd = max_block_size_code(d.BlockSize) << 4
    out = bytes([flg & 0xFF, bd & 0xFF])
    if d.ContentLength is not None:
        out += struct.pack("<Q", d.ContentLength)
    if d.Dictionary is not None:
        out += struct.pack("<I", d.Dictionary)
    return out


def parse_frame(frame, start: int = 0) -> FrameInfo:
    """walks one frame: header fields, block table, checksums as stored (LZ4FrameReader.async.cs:52-136).
    Checksums are NOT verified here -- that is batch work for the device."""
    buf = _ro_view(frame, "source")
    pos, end = int(start), buf.size

    def need(n):
        if end - pos < n:
            raise EOFError("Unexpected end of stream")               # EndOfStream()
    need(4)
    if struct.unpack_from("<I", buf, pos)[0] != MAGIC:
        raise InvalidDataException("LZ4 frame magic number expected")
    pos += 4
    hdr0 = pos
    need(2)
    flg, bd = int(buf[pos]), int(buf[pos + 1])
    pos += 2
    version = (flg >> 6) & 0x11                                     # as written at LZ4FrameReader.async.cs:72
    if version != 1:
        raise InvalidDataException(f"LZ4 frame version unknown: {version}")
    chaining = ((flg >> 5) & 1) == 0
    bsum = ((flg >> 4) & 1) != 0
    has_size = ((flg >> 3) & 1) != 0
    csum = ((flg >> 2) & 1) != 0
    has_dict = (flg & 1) != 0
    content_length = None
    if has_size:
        need(8)
        content_length = struct.unpack_from("<Q", buf, pos)[0]
        pos += 8
    dict_id = None
    if has_dict:
        need(4)
        dict_id = struct.unpack_from("<I", buf, pos)[0]
        pos += 4
    header = buf[hdr0:pos].tobytes()
    need(1)
    hc = int(buf[pos])
    pos += 1
    info = FrameInfo(LZ4Descriptor(content_length, csum, chaining, bsum, dict_id, max_block_size((bd >> 4) & 7)), header, hc)
    while True:
        need(4)
        lc = struct.unpack_from("<I", buf, pos)[0]
        pos += 4
        if lc == 0:
            break
        n = lc & 0x7FFFFFFF
        need(n + (4 if bsum else 0))
        info.block_off.append(pos)
        info.block_len.append(lc)
        pos += n
        if bsum:
            info.block_checksum.append(struct.unpack_from("<I", buf, pos)[0])
            pos += 4
    if csum:
        need(4)
        info.content_checksum = struct.unpack_from("<I", buf, pos)[0]
        pos += 4
    info.consumed = pos - int(start)
    return info


def assemble_frame(d: LZ4Descriptor, header_hash: int, payloads: Sequence[bytes], raw: Sequence[bool],
                   block_hashes: Optional[Sequence[int]], content_hash: Optional[int], dictionary: bool = False) -> bytes:
    """lays the pieces out as the writer does (LZ4FrameWriter.async.cs:15-27,:75-90); dictionary: as frame_header"""
    parts = [struct.pack("<I", MAGIC), frame_header(d, dictionary), bytes([(header_hash >> 8) & 0xFF])]
    for i, p in enumerate(payloads):
        parts.append(struct.pack("<I", len(p) | (0x80000000 if raw[i] else 0)))     # BlockLengthCode
        parts.append(p)
        if d.BlockChecksum:
            parts.append(struct.pack("<I", block_hashes[i]))
    parts.append(struct.pack("<I", 0))                                                  # EndMark
    if d.ContentChecksum:
        parts.append(struct.pack("<I", content_hash))
    return b"".join(parts)


def xxh32_many(buffers: Sequence, ctx: Optional[_native.Context] = None) -> np.ndarray:
    """XXH32.DigestOf of every buffer, one kernel launch (seed 0, as every call site of the reference)"""
    ctx = ctx or _native.default_context()
    views = [_ro_view(b, "buffer") for b in buffers]
    if not views:
        return np.zeros(0, np.uint32)
    data, off, _ = pack_blocks(views)
    lens = np.array([v.size for v in views], dtype=np.uint64)
    out = np.zeros(len(views), dtype=np.uint32)
    ctx.check(ctx.lib.k4lz4_xxh32_batch(ctx.handle, data.ctypes.data, off.ctypes.data, lens.ctypes.data, out.ctypes.data,
                                        len(views), 0))
    return out


def _assemble_frames(s: "LZ4EncoderSettings", contents, out, arena, aoff, owner, ctx, dict_ids=None) -> List[bytes]:
    """the frames of a batch from its encoded blocks (outLen per block, negative: stored raw; arena slots; owning frame per block):
    header, block records with their checksums, EndMark, content checksum -- every XXH32 in one launch.  dict_ids: per frame the
    DictID its header names (the writer with a DictionarySet)"""
    bs = int(s.BlockSize)
    payloads, raw = [], []
    for n, o in zip(out, aoff if len(out) else []):
        if n == 0:
            raise RuntimeError("Failed to encode chunk. Target buffer too small.")       # LZ4EncoderBase.cs:75-77
        payloads.append(arena[int(o):int(o) + abs(int(n))])
        raw.append(n < 0)
    with_id = dict_ids is not None
    descs = [LZ4Descriptor(s.ContentLength, s.ContentChecksum, bool(s.ChainBlocks), s.BlockChecksum, int(dict_ids[f]) if with_id else None, bs)
             for f, _ in enumerate(contents)]
    # every XXH32 of the batch in one launch: headers, then block payloads, then contents
    to_hash = [np.frombuffer(frame_header(d, with_id), np.uint8) for d in descs]
    if s.BlockChecksum:
        to_hash += payloads
    if s.ContentChecksum:
        to_hash += contents
    hashes = xxh32_many(to_hash, ctx)
    nf, nb = len(contents), len(payloads)
    bh = hashes[nf:nf + nb] if s.BlockChecksum else None
    ch = hashes[nf + (nb if s.BlockChecksum else 0):] if s.ContentChecksum else None
    frames = []
    k = 0
    for f, d in enumerate(descs):
        k0 = k
        while k < nb and owner[k] == f:
            k += 1
        frames.append(assemble_frame(d, int(hashes[f]), [payloads[i].tobytes() for i in range(k0, k)], raw[k0:k],
                                     None if bh is None else [int(x) for x in bh[k0:k]],
                                     None if ch is None else int(ch[f]), with_id))
    return frames


class LZ4Frame:
    """LZ4Frame.Encode / Decode for whole buffers, plus their batch forms."""

    # ---- encode -----------------------------------------------------------------------------------
    @staticmethod
    def Encode(source, settings: Optional[LZ4EncoderSettings] = None, level: Optional[LZ4Level] = None, dictionary=None,
               dict_index: int = -1) -> bytes:
        return LZ4Frame.EncodeBatch([source], settings, level, dictionary=dictionary,
                                    dict_index=None if dictionary is None else [dict_index])[0]

    @staticmethod
    def EncodeBatch(sources: Sequence, settings: Optional[LZ4EncoderSettings] = None, level: Optional[LZ4Level] = None,
                    ctx: Optional[_native.Context] = None, dictionary=None, dict_index=None) -> List[bytes]:
        """dictionary=(DictionarySet, ids) with dict_index[f] (an entry of the set, -1: a plain frame): frame f names the entry's id
        as its DictID and its blocks are encoded against the entry (_encode_frames_dictset)"""
        s = settings or LZ4EncoderSettings()
        if level is not None:
            s = LZ4EncoderSettings(**{**s.__dict__, "CompressionLevel": LZ4Level(level)})
        if dictionary is not None:
            return _encode_frames_dictset(sources, s, ctx, dictionary, dict_index)
        if s.ChainBlocks and int(s.CompressionLevel) < int(LZ4Level.L03_HC):
            raise NotImplementedException(FAST_CHAIN_REFUSED)
        max_block_size_code(s.BlockSize)
        ctx = ctx or _native.default_context()
        contents = [_ro_view(x, "source") for x in sources]
        bs = int(s.BlockSize)
        for c in contents:
            if s.ContentLength is not None and s.ContentLength != c.size:
                raise ValueError("ContentLength does not match the source length")
        blocks, owner = [], []
        if s.ChainBlocks:
            # LZ4HighChainEncoder per frame (Streams/Extensions.cs:28-36): its blocks are the ring buffer's, rounded to a whole KiB
            nonempty = [f for f, c in enumerate(contents) if c.size]
            if nonempty:
                out, arena, aoff, nblk = encode_hc_chain_packed([contents[f] for f in nonempty], bs,
                                                                _extra_blocks(bs, int(s.ExtraMemory)), s.CompressionLevel, True, ctx)
                owner = list(np.repeat(np.array(nonempty), nblk))
            else:
                out, arena, aoff = np.zeros(0, np.int32), None, None
        else:
            for f, c in enumerate(contents):
                for p in range(0, c.size, bs):
                    blocks.append(c[p:p + bs])
                    owner.append(f)
            out, arena, aoff = encode_blocks_packed(blocks, s.CompressionLevel, True, ctx) if blocks else (np.zeros(0, np.int32), None, None)
        return _assemble_frames(s, contents, out, arena, aoff, owner, ctx)

    # ---- decode -----------------------------------------------------------------------------------
    @staticmethod
    def Decode(source, settings=None, dictionary=None) -> bytes:
        return LZ4Frame.DecodeBatch([source], dictionary=dictionary)[0]

    @staticmethod
    def DecodeBatch(sources: Sequence, ctx: Optional[_native.Context] = None, dictionary=None) -> List[bytes]:
        """every element holds one frame (bytes after it are ignored, as a reader that stops at EndMark does).
        dictionary=(DictionarySet, ids): frames with a DictID are decoded against the first entry whose id equals it
        (k4lz4_decode_frames_dictset); without it such a frame raises NotImplementedException as before."""
        if dictionary is not None:
            return _decode_frames_dictset_host(sources, ctx, dictionary)
        ctx = ctx or _native.default_context()
        bufs = [_ro_view(x, "source") for x in sources]
        infos = [parse_frame(b) for b in bufs]
        for i in infos:
            if i.descriptor.Dictionary is not None:
                raise NotImplementedException("Predefined dictionaries feature is not implemented")
        # header and block checksums: one launch
        to_hash = [np.frombuffer(i.header, np.uint8) for i in infos]
        for b, i in zip(bufs, infos):
            if i.descriptor.BlockChecksum:
                to_hash += [b[o:o + (l & 0x7FFFFFFF)] for o, l in zip(i.block_off, i.block_len)]
        hashes = xxh32_many(to_hash, ctx)
        k = len(infos)
        for f, i in enumerate(infos):
            if ((int(hashes[f]) >> 8) & 0xFF) != i.header_checksum:
                raise InvalidDataException("Invalid LZ4 frame header checksum")
            if i.descriptor.BlockChecksum:
                for want in i.block_checksum:
                    if int(hashes[k]) != want:
                        raise InvalidDataException("Invalid block checksum")
                    k += 1
        outs = LZ4Frame._decode_streams(bufs, infos, ctx)
        with_sum = [f for f, i in enumerate(infos) if i.descriptor.ContentChecksum]
        if with_sum:
            got = xxh32_many([outs[f] for f in with_sum], ctx)
            for f, g in zip(with_sum, got):
                if int(g) != infos[f].content_checksum:
                    raise InvalidDataException("Invalid content checksum")
        for f, i in enumerate(infos):
            if i.descriptor.ContentLength is not None and i.descriptor.ContentLength != outs[f].size:
                raise InvalidDataException("Content length does not match the frame header")
        return [o.tobytes() for o in outs]

    # What a frame's metadata may make the decoder allocate.  The reference's reader holds ONE block-sized buffer at a time
    # (LZ4FrameReader.async.cs:108-136); a batch decoder sizes an arena up front, so the size must come from what the input
    # can actually produce, not from what the header claims: an LZ4 block never decodes to more than 255 bytes per input
    # byte (a match costs at least 3 bytes + 1 per 255 bytes of length), and launches are cut at an arena budget.
    ARENA_BUDGET = 1 << 30

    @staticmethod
    def _block_cap(block_size: int, stored: int) -> int:
        return int(min(block_size, 255 * stored + 32))

    @staticmethod
    def _decode_streams(bufs, infos, ctx) -> List[np.ndarray]:
        """frames of independent blocks: all their blocks as batches (LZ4BlockDecoder per block, parallel) of at most
        ARENA_BUDGET bytes of output slots each; frames of chained blocks: one in-order stream per frame (LZ4ChainDecoder,
        k4lz4_decode_chain_batch)"""
        res: List[Optional[np.ndarray]] = [None] * len(infos)
        indep = [f for f, i in enumerate(infos) if not i.descriptor.Chaining]
        chain = [f for f, i in enumerate(infos) if i.descriptor.Chaining]
        if indep:
            blocks, caps, where = [], [], []
            for f in indep:
                i, b = infos[f], bufs[f]
                for k, (o, l) in enumerate(zip(i.block_off, i.block_len)):
                    if not (l & 0x80000000):
                        blocks.append(b[o:o + l])
                        caps.append(LZ4Frame._block_cap(i.descriptor.BlockSize, l))
                        where.append((f, k))
            decoded = {}
            lo = 0
            while lo < len(blocks):
                hi, room = lo, LZ4Frame.ARENA_BUDGET
                while hi < len(blocks) and (hi == lo or caps[hi] <= room):
                    room -= caps[hi]
                    hi += 1
                src, soff, slen = pack_blocks(blocks[lo:hi])
                cap = np.array(caps[lo:hi], np.int32)
                dst, doff = make_arena(cap)
                out = LZ4Codec.DecodeBatchPacked(src, soff, slen, dst, doff, cap, ctx=ctx)
                for (f, k), n, o in zip(where[lo:hi], out, doff):
                    if n < 0:
                        raise InvalidDataException("LZ4 block does not decode")      # LZ4BlockDecoder.cs:50-52
                    decoded[(f, k)] = dst[int(o):int(o) + int(n)].copy()             # (the arena goes away with this launch)
                lo = hi
            for f in indep:
                i, b = infos[f], bufs[f]
                parts = [decoded[(f, k)] if not (l & 0x80000000) else b[o:o + (l & 0x7FFFFFFF)]
                         for k, (o, l) in enumerate(zip(i.block_off, i.block_len))]
                res[f] = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        if chain:
            cb = [bufs[f] for f in chain]
            ci = [infos[f] for f in chain]
            nf = len(ci)
            src, foff, _ = pack_blocks(cb)
            blk_off, blk_len, first, nblk = [], [], np.zeros(nf, np.uint64), np.zeros(nf, np.uint32)
            for f, i in enumerate(ci):
                first[f] = len(blk_off)
                nblk[f] = len(i.block_off)
                blk_off += [int(foff[f]) + o for o in i.block_off]
                blk_len += i.block_len
            bsize = np.array([i.descriptor.BlockSize for i in ci], np.int32)
            chained = np.ones(nf, np.uint8)
            produced = [sum(LZ4Frame._block_cap(i.descriptor.BlockSize, l & 0x7FFFFFFF) if not (l & 0x80000000) else (l & 0x7FFFFFFF)
                            for l in i.block_len) for i in ci]          # what the blocks can produce, not what the header claims
            caps = np.array([p if i.descriptor.ContentLength is None else min(i.descriptor.ContentLength, p)
                             for i, p in zip(ci, produced)], np.uint64)
            doff = np.zeros(nf, np.uint64)
            if nf > 1:
                doff[1:] = np.cumsum(caps[:-1])
            dst = np.zeros(max(int(caps.sum()), 1), np.uint8)
            out = np.zeros(nf, np.int64)
            bo = np.array(blk_off if blk_off else [0], np.uint64)
            bl = np.array(blk_len if blk_len else [0], np.uint32)
            ctx.check(ctx.lib.k4lz4_decode_chain_batch(ctx.handle, src.ctypes.data, bo.ctypes.data, bl.ctypes.data, len(blk_off),
                                                       first.ctypes.data, nblk.ctypes.data, bsize.ctypes.data, chained.ctypes.data,
                                                       dst.ctypes.data, doff.ctypes.data, caps.ctypes.data, out.ctypes.data, nf))
            for k, f in enumerate(chain):
                if out[k] < 0:
                    raise InvalidDataException("LZ4 block does not decode" if out[k] == -6
                                               else "Decoded frame does not fit its declared size")
                res[f] = dst[int(doff[k]):int(doff[k]) + int(out[k])]
        return res


def encode_frames_device(dc, data, off: np.ndarray, length: np.ndarray, settings: Optional[LZ4EncoderSettings] = None, dictionary=None,
                         dict_index=None):
    """LZ4Frame.EncodeBatch on HBM-resident contents, nothing leaves the device: `data` is a uint8 torch tensor holding
    the contents, content f = data[off[f] : off[f]+length[f]] (off / length: host arrays -- the block split is host index
    work).  Returns (frames, frame_off, frame_len): frame f = frames[frame_off[f] : frame_off[f] + frame_len[f]], with
    frame_off a host array of (worst-case spaced) positions and frame_len a device tensor.  Asynchronous on the current
    torch stream; `dc` is a device.DeviceCodec.
    dictionary=(DictionarySet, ids) with dict_index[f] (a host array; an entry of the set, -1: a plain frame): frame f names the
    entry's id as its DictID; its independent blocks are k4lz4_encode_dictset_batch_device's with the allowCopy rule behind them
    (k4lz4_allow_copy_batch_device), its chained blocks those of a ChainEncoderDevice opened from the entry, one record (Topup and a
    forced Encode) per block.  Levels 10 - 12 and Enforce32 are refused when a frame names an entry."""
    import ctypes as C
    import torch
    from ._native import FLAG_ALLOW_COPY
    from .device import DeviceBatch, ChainEncoderDevice, _dp
    s = settings or LZ4EncoderSettings()
    off = np.asarray(off, dtype=np.int64)
    length = np.asarray(length, dtype=np.int64)
    nf = len(off)
    entry = np.full(nf, -1, np.int64)
    ids = None
    if dictionary is not None:
        dset, ids = _dictionary_ids(dictionary)
        entry = np.asarray(dict_index if dict_index is not None else [], np.int64)
        if entry.shape != (nf,):
            raise ValueError("dict_index must have one entry per content")
        if nf and (int(entry.min()) < -1 or int(entry.max()) >= dset.n):
            raise ValueError("a dict_index outside the DictionarySet")
    named = entry >= 0
    if named.any() and (int(s.CompressionLevel) >= int(LZ4Level.L10_OPT) or LZ4Codec.Enforce32):
        raise NotImplementedException(DICT_WRITER_REFUSED)
    fast_chain = s.ChainBlocks and int(s.CompressionLevel) < int(LZ4Level.L03_HC)
    if fast_chain and (dictionary is None or not named.all()):
        raise NotImplementedException(FAST_CHAIN_REFUSED)
    bs = int(s.BlockSize)
    max_block_size_code(bs)
    eb = _round_block_size(bs) if s.ChainBlocks else bs          # (the chained encoder's blocks: its ring buffer's, whole KiB)
    nblk = (length + eb - 1) // eb
    first = np.concatenate(([0], np.cumsum(nblk)))[:-1]
    nb = int(nblk.sum())
    owner = np.repeat(np.arange(nf), nblk)
    bound = LZ4Codec.MaximumOutputSize(eb)
    dev = dc.device
    k_in = np.arange(nb) - first[owner]
    boff = off[owner] + k_in * eb
    blen = np.minimum(eb, length[owner] - k_in * eb).astype(np.int32)
    stream = C.c_void_p(dc._stream())
    out_len = torch.zeros(nb, dtype=torch.int32, device=dev)
    if not s.ChainBlocks:
        arena = DeviceBatch.empty_slots(np.full(nb, bound, np.int64), dev)
        slot_off = arena.off
        for which in (np.flatnonzero(~named[owner]), np.flatnonzero(named[owner])):
            if not which.size:
                continue
            sel = torch.from_numpy(which).to(dev)
            src = DeviceBatch(data, torch.from_numpy(boff[which]).to(dev), torch.from_numpy(blen[which]).to(dev))
            dst = DeviceBatch(arena.data, arena.off[sel], arena.length[sel])
            if named[owner[which[0]]]:
                got = dc.encode_dictset(src, dst, torch.from_numpy(entry[owner[which]].astype(np.int32)).to(dev), dset, level=s.CompressionLevel)
                dc.ctx.check(dc.lib.k4lz4_allow_copy_batch_device(dc.ctx.handle, _dp(src.data), _dp(src.off), _dp(src.length), _dp(dst.data),
                                                                  _dp(dst.off), _dp(dst.length), _dp(got), src.n, stream))
            else:
                got = dc.encode(src, dst, level=s.CompressionLevel, flags=FLAG_ALLOW_COPY)
            out_len[sel] = got
    else:
        # every frame one stream whose blocks' slots lie behind each other
        frame_slots = np.zeros(nf, np.int64)
        if nf > 1:
            frame_slots[1:] = np.cumsum((nblk * bound + 15) // 16 * 16)[:-1]
        arena = DeviceBatch(torch.empty(int(((nblk * bound + 15) // 16 * 16).sum()) + 64, dtype=torch.uint8, device=dev), None, None)
        slot_off = torch.from_numpy(frame_slots[owner] + k_in * bound).to(dev)          # the whole-stream call: `bound` bytes apart
        plain, pb = np.flatnonzero(~named), np.flatnonzero(~named[owner])
        if pb.size:
            got = torch.empty(pb.size, dtype=torch.int32, device=dev)
            c_off, c_len, c_dst = off[plain].astype(np.uint64), np.ascontiguousarray(length[plain]), frame_slots[plain].astype(np.uint64)
            bsz = np.full(plain.size, bs, np.int32)
            ext = np.full(plain.size, _extra_blocks(bs, int(s.ExtraMemory)), np.int32)
            dc.ctx.check(dc.lib.k4lz4_encode_hc_chain_batch_device(dc.ctx.handle, _dp(data), c_off.ctypes.data, c_len.ctypes.data, bsz.ctypes.data,
                                                                   ext.ctypes.data, None, plain.size, _dp(arena.data), c_dst.ctypes.data, _dp(got),
                                                                   pb.size, int(s.CompressionLevel), FLAG_ALLOW_COPY, stream))
            out_len[torch.from_numpy(pb).to(dev)] = got
        mine = np.flatnonzero(named & (nblk > 0))
        if mine.size:
            # open encoders primed from the entries; one record per block, each a Topup and a forced Encode: the blocks lie packed
            from .encoders import CENC_FORCE, CENC_ALLOW_COPY
            enc = ChainEncoderDevice([(True, s.CompressionLevel, bs, _extra_blocks(bs, int(s.ExtraMemory)))] * mine.size, dc)
            enc.open(entry[mine].astype(np.int32), dset)
            mb = np.flatnonzero(named[owner])
            sel = torch.from_numpy(mb).to(dev)
            rec_first = np.concatenate(([0], np.cumsum(nblk[mine])))[:-1]
            got = torch.zeros(mb.size, dtype=torch.int32, device=dev)
            loaded = torch.zeros(mb.size, dtype=torch.int32, device=dev)
            total = torch.zeros(mine.size, dtype=torch.int64, device=dev)
            enc.run(data, boff[mb], blen[mb], np.full(mb.size, CENC_FORCE | CENC_ALLOW_COPY, np.uint32), rec_first, nblk[mine], arena.data,
                    frame_slots[mine], nblk[mine] * bound, loaded, got, total)
            out_len[sel] = got
            size = got.abs().to(torch.int64)
            excl = torch.cumsum(size, 0) - size
            start = excl[torch.from_numpy(rec_first).to(dev)]
            rank = torch.from_numpy(np.repeat(np.arange(mine.size), nblk[mine])).to(dev)
            slot_off[sel] = torch.from_numpy(frame_slots[owner[mb]]).to(dev) + excl - start[rank]
    stored = out_len.abs().to(torch.int64)
    # header bytes (host: two to fourteen bytes per frame) and every XXH32 of the batch
    hdrs = [frame_header(LZ4Descriptor(int(length[f]) if s.ContentLength is not None else None, s.ContentChecksum, bool(s.ChainBlocks),
                                       s.BlockChecksum, int(ids[entry[f]]) if named[f] else None, bs), bool(named[f])) for f in range(nf)]
    hl = np.array([len(h) for h in hdrs] if nf else [2], np.int64)
    hdr_h = np.zeros((max(nf, 1), 16), np.uint8)
    for f, h in enumerate(hdrs):
        hdr_h[f, :len(h)] = np.frombuffer(h, np.uint8)
    hdr_d = torch.from_numpy(hdr_h.reshape(-1)).to(dev)
    hdr_len = torch.from_numpy(hl).to(dev)
    hdr_sum = dc.xxh32(hdr_d, torch.arange(max(nf, 1), dtype=torch.int64, device=dev) * 16, hdr_len)
    blk_sum = dc.xxh32(arena.data, slot_off, stored) if (s.BlockChecksum and nb) else None
    con_sum = dc.xxh32(data, torch.from_numpy(off).to(dev), torch.from_numpy(length).to(dev)) if (s.ContentChecksum and nf) else None
    # layout: frames sit at worst-case spaced bases (known without a sync), records are packed inside each frame
    head = 4 + hl[:nf] + 1
    per_block = 4 + bound + (4 if s.BlockChecksum else 0)
    frame_cap = head + nblk * per_block + 8
    frame_off = np.concatenate(([0], np.cumsum(frame_cap)))[:-1].astype(np.int64)
    rec_size = stored + (8 if s.BlockChecksum else 4)
    excl = torch.cumsum(rec_size, 0) - rec_size if nb else rec_size
    owner_d = torch.from_numpy(owner).to(dev)
    first_d = torch.from_numpy(np.minimum(first, max(nb - 1, 0))).to(dev)
    base_d = torch.from_numpy(frame_off + head).to(dev)          # behind the header
    start_of_frame = excl[first_d] if nb else torch.zeros(nf, dtype=torch.int64, device=dev)
    rec_off = (base_d[owner_d] + excl - start_of_frame[owner_d]) if nb else torch.zeros(0, dtype=torch.int64, device=dev)
    total = torch.zeros(nf, dtype=torch.int64, device=dev)
    if nb:
        total.index_add_(0, owner_d, rec_size)
    tail_off = base_d + total
    frames = torch.empty(int(frame_cap.sum()) + 64, dtype=torch.uint8, device=dev)
    frame_len = torch.zeros(max(nf, 1), dtype=torch.int64, device=dev)
    hdr_len32 = hdr_len.to(torch.int32)
    rc = dc.lib.k4lz4_frame_assemble_device(dc.ctx.handle, _dp(arena.data), _dp(slot_off), _dp(out_len), _dp(blk_sum), _dp(rec_off), nb,
                                            _dp(hdr_d), _dp(hdr_len32), _dp(hdr_sum), _dp(torch.from_numpy(frame_off).to(dev)), _dp(tail_off),
                                            _dp(con_sum), _dp(frames), _dp(frame_len), nf, stream)
    dc.ctx.check(rc)
    return frames, frame_off, frame_len[:nf]


# per-frame codes of the device reader (include/k4lz4.h K4LZ4_FRAME_*) and what the reference's reader raises for each
FRAME_EOF, FRAME_MAGIC, FRAME_VERSION, FRAME_HEADER_SUM, FRAME_DICTIONARY = -1, -2, -3, -4, -5
FRAME_BLOCK, FRAME_BLOCK_SUM, FRAME_CONTENT_SUM, FRAME_CAPACITY, FRAME_LENGTH = -6, -7, -8, -9, -10
FRAME_BLOCK_SIZE = -11          # the incremental reader's: a block size above its maxBlockSize


def frame_exception(code: int) -> Exception:
    """the exception LZ4FrameReader raises for a K4LZ4_FRAME_* code"""
    return {FRAME_EOF: lambda: EOFError("Unexpected end of stream"),
            FRAME_MAGIC: lambda: InvalidDataException("LZ4 frame magic number expected"),
            FRAME_VERSION: lambda: InvalidDataException("LZ4 frame version unknown: 0"),      # (FLG >> 6) & 0x11 is 0 or 1
            FRAME_HEADER_SUM: lambda: InvalidDataException("Invalid LZ4 frame header checksum"),
            FRAME_DICTIONARY: lambda: NotImplementedException("Predefined dictionaries feature is not implemented"),
            FRAME_BLOCK: lambda: InvalidDataException("LZ4 block does not decode"),
            FRAME_BLOCK_SUM: lambda: InvalidDataException("Invalid block checksum"),
            FRAME_CONTENT_SUM: lambda: InvalidDataException("Invalid content checksum"),
            FRAME_CAPACITY: lambda: InvalidDataException("Decoded frame does not fit its target"),
            FRAME_LENGTH: lambda: InvalidDataException("Content length does not match the frame header"),
            FRAME_BLOCK_SIZE: lambda: InvalidDataException("LZ4 frame block size is above the reader's maxBlockSize"),
            }.get(int(code), lambda: RuntimeError(f"unknown frame result {int(code)}"))()


def _dev_i64(x, dev):
    """host array or device tensor -> contiguous int64 device tensor (uint64 offsets / lengths)"""
    import torch
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=torch.int64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64))).to(dev)


def _dictionary_ids(dictionary):
    """dictionary=(DictionarySet, ids) -> (the set, its ids as a uint32 host array: entry e answers to DictID ids[e])"""
    dset, ids = dictionary
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32))
    if ids.ndim != 1 or ids.size != dset.n:
        raise ValueError("dictionary=(DictionarySet, ids): one id per entry of the set")
    return dset, ids


def _reader_dictionary(dictionary):
    """the incremental readers' dictionary=(DictionarySet, ids), or None -> (the set and the id array, kept alive by the reader; the two
    arguments the _dictset calls take behind their counterparts')"""
    if dictionary is None:
        return None, []
    dset, ids = _dictionary_ids(dictionary)
    return (dset, ids), [dset.handle, ids.ctypes.data if ids.size else None]


DICT_WRITER_REFUSED = ("frames with a predefined dictionary are written at L00_FAST .. L09_HC by the 64-bit engine: the dictionary "
                       "encoders have no witness at L10_OPT and above, nor under Enforce32")


def _encode_frames_dictset(sources: Sequence, s: "LZ4EncoderSettings", ctx, dictionary, dict_index) -> List[bytes]:
    """LZ4Frame.EncodeBatch(dictionary=..., dict_index=...).  Frame f with dict_index[f] = e >= 0 carries DictID ids[e]; its blocks are
    independent frames: the blocks k4lz4_encode_dictset_batch writes for entry e (each block one message), with the allowCopy rule
                        (a block that does not shrink is stored raw);
    chained frames:     the blocks of an encoder opened from entry e (k4lz4_chain_encoder_open_dictset: LZ4FastChainEncoder below
                        L03_HC, LZ4HighChainEncoder from there), fed the whole content and flushed, block size and ExtraMemory as
                        the chained writers have them.
    Frames with dict_index -1 are the plain writers' (LZ4Frame.EncodeBatch, encode_fast_chain_frames)."""
    from .encoders import LZ4EncoderBatch
    dset, ids = _dictionary_ids(dictionary)
    ctx = ctx or dset.ctx
    contents = [_ro_view(x, "source") for x in sources]
    idx = np.asarray(dict_index if dict_index is not None else [], np.int64)
    if idx.shape != (len(contents),):
        raise ValueError("dict_index must have one entry per source")
    if idx.size and (int(idx.min()) < -1 or int(idx.max()) >= dset.n):
        raise ValueError("a dict_index outside the DictionarySet")
    if (idx >= 0).any() and (int(s.CompressionLevel) >= int(LZ4Level.L10_OPT) or LZ4Codec.Enforce32):
        raise NotImplementedException(DICT_WRITER_REFUSED)          # (a batch of plain frames is the plain writers' at any level)
    bs = int(s.BlockSize)
    max_block_size_code(bs)
    for c in contents:
        if s.ContentLength is not None and s.ContentLength != c.size:
            raise ValueError("ContentLength does not match the source length")
    res: List[Optional[bytes]] = [None] * len(contents)
    plain = [f for f in range(len(contents)) if idx[f] < 0]
    if plain:
        fast_chain = s.ChainBlocks and int(s.CompressionLevel) < int(LZ4Level.L03_HC)
        made = encode_fast_chain_frames([contents[f] for f in plain], s, ctx) if fast_chain else LZ4Frame.EncodeBatch([contents[f] for f in plain], s, ctx=ctx)
        for f, fr in zip(plain, made):
            res[f] = fr
    named = [f for f in range(len(contents)) if idx[f] >= 0]
    if named:
        mine = [contents[f] for f in named]
        payloads, out, owner = [], [], []
        if s.ChainBlocks:
            enc = LZ4EncoderBatch([(True, s.CompressionLevel, bs, _extra_blocks(bs, int(s.ExtraMemory)))] * len(named), ctx)
            enc.open(idx[named].astype(np.int32), dset)
            written = enc.Write(mine, force=False, allowCopy=True)
            for k, last in enumerate(enc.Flush(allowCopy=True)):
                for n, b in written[k] + last:
                    payloads.append(np.frombuffer(b, np.uint8))
                    out.append(int(n))
                    owner.append(k)
        else:
            blocks = [c[p:p + bs] for c in mine for p in range(0, c.size, bs)]
            owner = [k for k, c in enumerate(mine) for _ in range(0, c.size, bs)]
            if blocks:
                src, soff, slen = pack_blocks(blocks)
                caps = np.array([LZ4Codec.MaximumOutputSize(b.size) for b in blocks], np.int32)
                dst, doff = make_arena(caps)
                got = LZ4Codec.EncodeDictBatchPacked(src, soff, slen, dst, doff, caps, idx[named][owner].astype(np.int32), dset,
                                                     level=s.CompressionLevel, ctx=ctx)
                for b, n, o in zip(blocks, got, doff):                   # LZ4EncoderBase.Encode(allowCopy: true), LZ4EncoderBase.cs:66-88
                    if n <= 0:
                        raise RuntimeError("Failed to encode chunk. Target buffer too small.")
                    raw = int(n) >= b.size
                    payloads.append(b if raw else dst[int(o):int(o) + int(n)])
                    out.append(-b.size if raw else int(n))
        arena, aoff = (np.concatenate(payloads), np.concatenate(([0], np.cumsum([p.size for p in payloads])))[:-1]) if payloads else (None, [])
        frames = _assemble_frames(s, mine, np.array(out, np.int64), arena, aoff, owner, ctx, dict_ids=[int(ids[idx[f]]) for f in named])
        for f, fr in zip(named, frames):
            res[f] = fr
    return res


def _decode_frames_dictset_host(sources: Sequence, ctx, dictionary) -> List[bytes]:
    """LZ4Frame.DecodeBatch(dictionary=...): k4lz4_frame_sizes_dictset sizes the targets, k4lz4_decode_frames_dictset reads the
    frames; the lowest-index failing frame raises what LZ4FrameReader raises"""
    dset, ids = _dictionary_ids(dictionary)
    ctx = ctx or dset.ctx
    bufs = [_ro_view(x, "source") for x in sources]
    n = len(bufs)
    if not n:
        return []
    src, foff, flen = pack_blocks(bufs)
    flen = flen.astype(np.uint64)
    size, status, idx = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.int32)
    ip = ids.ctypes.data if ids.size else None
    ctx.check(ctx.lib.k4lz4_frame_sizes_dictset(ctx.handle, src.ctypes.data_as(_native._u8p), foff.ctypes.data, flen.ctypes.data, n,
                                                size.ctypes.data, status.ctypes.data, idx.ctypes.data, dset.handle, ip))
    doff = np.zeros(n, np.uint64)
    doff[1:] = np.cumsum(size[:-1])
    dst = np.zeros(max(int(size.sum()), 1), np.uint8)
    out = np.zeros(n, np.int64)
    ctx.check(ctx.lib.k4lz4_decode_frames_dictset(ctx.handle, src.ctypes.data_as(_native._u8p), foff.ctypes.data, flen.ctypes.data, n,
                                                  dst.ctypes.data_as(_native._u8p), doff.ctypes.data, size.ctypes.data, out.ctypes.data,
                                                  dset.handle, ip))
    bad = np.flatnonzero(out < 0)
    if bad.size:
        raise frame_exception(int(out[bad[0]]))
    return [dst[int(o):int(o) + int(k)].tobytes() for o, k in zip(doff, out)]


def frame_sizes_device(dc, frames, off, length, dictionary=None):
    """k4lz4_frame_sizes_device: frame f = frames[off[f] : off[f]+length[f]] (frames: uint8 device tensor; off / length: host arrays or
    device tensors).  Returns (size, status), int64 / int32 device tensors: the most frame f can decode to without trusting its
    header (per block min(blockSize, 255 * stored + 32), stored if raw; capped by ContentLength), and 0 or the walk's K4LZ4_FRAME_*
    code.  Asynchronous on the current torch stream.
    dictionary=(DictionarySet, ids): k4lz4_frame_sizes_dictset_device -- a DictID that one of the ids answers to is no defect, and a
    third tensor comes back: dict_index (int32), the entry every frame resolved to, -1 for none."""
    import ctypes as C
    import torch
    from .device import _dp
    dev = dc.device
    off_d, len_d = _dev_i64(off, dev), _dev_i64(length, dev)
    n = off_d.numel()
    size = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    if dictionary is not None:
        dset, ids = _dictionary_ids(dictionary)
        idx = torch.full((n,), -1, dtype=torch.int32, device=dev)
        dc.ctx.check(dc.lib.k4lz4_frame_sizes_dictset_device(dc.ctx.handle, _dp(frames), _dp(off_d), _dp(len_d), n, _dp(size), _dp(status),
                                                             _dp(idx), dset.handle, ids.ctypes.data if ids.size else None,
                                                             C.c_void_p(dc._stream())))
        return size, status, idx
    dc.ctx.check(dc.lib.k4lz4_frame_sizes_device(dc.ctx.handle, _dp(frames), _dp(off_d), _dp(len_d), n, _dp(size), _dp(status),
                                                 C.c_void_p(dc._stream())))
    return size, status


def decode_frames_device(dc, frames, off, length, out=None, raise_errors: bool = True, dictionary=None):
    """LZ4Frame.DecodeBatch on HBM-resident frames, nothing goes through the host: frame f = frames[off[f] : off[f]+length[f]]
    (off / length: host arrays or device tensors, e.g. encode_frames_device's frame_off and frame_len as they are).
    out: None, or (buffer, out_off, out_cap) -- a uint8 device tensor and per-frame positions / capacities (host arrays or device
    tensors).  Without it the output is sized by frame_sizes_device, which costs one synchronisation, and out_off is a host array.
    Returns (out, out_off, out_len): frame f decoded = out[out_off[f] : out_off[f]+out_len[f]], out_len an int64 device tensor
    holding a negative K4LZ4_FRAME_* code for a frame that does not decode.  k4lz4_decode_frames_device waits for the stream once
    (it reads the batch's block count back).  raise_errors: raise what LZ4FrameReader raises for the lowest-index failing frame
    (reads out_len back); otherwise the caller reads out_len.
    dictionary=(DictionarySet, ids): k4lz4_decode_frames_dictset_device -- frames with a DictID are decoded against the first entry of
    the set whose id equals it; a DictID none of the ids answers to is FRAME_DICTIONARY, as every DictID is without it."""
    import ctypes as C
    import torch
    from .device import _dp
    dev = dc.device
    off_d, len_d = _dev_i64(off, dev), _dev_i64(length, dev)
    n = off_d.numel()
    if out is None:
        size = frame_sizes_device(dc, frames, off_d, len_d, dictionary=dictionary)[0]
        cap = size.cpu().numpy() if n else np.zeros(0, np.int64)
        out_off = np.zeros(n, np.int64)
        if n > 1:
            out_off[1:] = np.cumsum((cap + 15) // 16 * 16)[:-1]
        buf = torch.empty(int(((cap + 15) // 16 * 16).sum()) + 64, dtype=torch.uint8, device=dev)
        off_o, cap_o = torch.from_numpy(out_off).to(dev), size
    else:
        buf, out_off, out_cap = out
        off_o, cap_o = _dev_i64(out_off, dev), _dev_i64(out_cap, dev)
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    if n and dictionary is not None:
        dset, ids = _dictionary_ids(dictionary)
        dc.ctx.check(dc.lib.k4lz4_decode_frames_dictset_device(dc.ctx.handle, _dp(frames), _dp(off_d), _dp(len_d), n, _dp(buf), _dp(off_o),
                                                               _dp(cap_o), _dp(out_len), dset.handle, ids.ctypes.data if ids.size else None,
                                                               C.c_void_p(dc._stream())))
    elif n:
        dc.ctx.check(dc.lib.k4lz4_decode_frames_device(dc.ctx.handle, _dp(frames), _dp(off_d), _dp(len_d), n, _dp(buf), _dp(off_o),
                                                       _dp(cap_o), _dp(out_len), C.c_void_p(dc._stream())))
    if raise_errors and n:
        got = out_len.cpu().numpy()
        bad = np.flatnonzero(got < 0)
        if bad.size:
            raise frame_exception(int(got[bad[0]]))
    return buf, out_off, out_len


def encode_fast_chain_frames(sources: Sequence, settings: Optional[LZ4EncoderSettings] = None,
                             ctx: Optional[_native.Context] = None) -> List[bytes]:
    """the frames LZ4FrameWriter writes with ChainBlocks=True below L03_HC (Streams/Extensions.cs:28-36 -> LZ4FastChainEncoder(blockSize,
    extraBlocks)): header, blocks with the allowCopy rule, block checksums, EndMark, content checksum, ContentLength when asked for.
    Every frame is one stream of one k4lz4_encode_fast_chain_batch call; the assembly is LZ4Frame.EncodeBatch's."""
    s = settings or LZ4EncoderSettings(ChainBlocks=True)
    if int(s.CompressionLevel) >= int(LZ4Level.L03_HC):
        raise ValueError("encode_fast_chain_frames writes the fast levels' frames (below L03_HC)")
    s = LZ4EncoderSettings(**{**s.__dict__, "ChainBlocks": True})
    max_block_size_code(s.BlockSize)
    ctx = ctx or _native.default_context()
    contents = [_ro_view(x, "source") for x in sources]
    bs = int(s.BlockSize)
    for c in contents:
        if s.ContentLength is not None and s.ContentLength != c.size:
            raise ValueError("ContentLength does not match the source length")
    nonempty = [f for f, c in enumerate(contents) if c.size]
    if nonempty:
        out, arena, aoff, nblk, _ = encode_fast_chain_packed([contents[f] for f in nonempty], bs, _extra_blocks(bs, int(s.ExtraMemory)),
                                                             True, ctx)
        owner = list(np.repeat(np.array(nonempty), nblk))
    else:
        out, arena, aoff, owner = np.zeros(0, np.int32), None, None, []
    return _assemble_frames(s, contents, out, arena, aoff, owner, ctx)


# ---- incremental frame writer: many LZ4FrameWriters, one Write / OpenFrame / CloseFrame each per call (k4lz4_frame_write_batch*,
# DESIGN.md 4.13) ------------------------------------------------------------------------------------------------------------
import ctypes as _C

FWRITE_WRITE, FWRITE_OPEN, FWRITE_CLOSE = 0, 1, 2
FWRITE_TARGET, FWRITE_CLOSED, FWRITE_LENGTH = -1, -2, -3          # per-stream codes (include/k4lz4.h K4LZ4_FWRITE_*)


class _WriterSettings(_C.Structure):          # k4lz4_frame_writer_settings
    _fields_ = [("contentLength", _C.c_int64), ("blockSize", _C.c_int32), ("level", _C.c_int32), ("chainBlocks", _C.c_int32),
                ("blockChecksum", _C.c_int32), ("contentChecksum", _C.c_int32), ("extraMemory", _C.c_int32)]


class FrameWriterRecord(_C.Structure):        # k4lz4_frame_writer: settings and counters, host memory
    _fields_ = [("settings", _WriterSettings), ("kind", _C.c_int32), ("encBlock", _C.c_int32), ("extraBlocks", _C.c_int32),
                ("ringBytes", _C.c_int32), ("written", _C.c_int64), ("index", _C.c_int32), ("pointer", _C.c_int32),
                ("currentOffset", _C.c_uint32), ("dictSize", _C.c_uint32), ("phase", _C.c_int32), ("reserved", _C.c_int32)]


def _writer_records(n: int, settings, lib):
    """n k4lz4_frame_writer records from one LZ4EncoderSettings or a list of n; their stores' offsets and total size"""
    lst = list(settings) if isinstance(settings, (list, tuple)) else [settings or LZ4EncoderSettings()] * n
    if len(lst) != n:
        raise ValueError("one settings object, or one per stream")
    recs = (FrameWriterRecord * max(n, 1))()
    store_off = np.zeros(n, np.uint64)
    at = 0
    for i, s in enumerate(lst):
        max_block_size_code(int(s.BlockSize))
        ws = _WriterSettings(-1 if s.ContentLength is None else int(s.ContentLength), int(s.BlockSize), int(s.CompressionLevel),
                             int(bool(s.ChainBlocks)), int(bool(s.BlockChecksum)), int(bool(s.ContentChecksum)), int(s.ExtraMemory))
        if lib.k4lz4_frame_writer_init(_C.byref(recs[i]), _C.byref(ws)) != 0:
            raise ValueError(f"Invalid block size ${s.BlockSize} for this operation")
        store_off[i] = at
        at += int(lib.k4lz4_frame_writer_store_bytes(_C.byref(recs[i])))
    return recs, store_off, at


class LZ4FrameWriterBatch:
    """n LZ4FrameWriters (Frames/LZ4FrameWriter*.cs) advanced together: Write(chunks) is one WriteManyBytes per stream, Open() one
    OpenFrame, Close() one CloseFrame; each returns, per stream, the bytes the reference's writer pushes to its inner stream during
    that call (None where a chunk is None).  The streams' encoder state lives in device memory; the data goes up and the bytes come
    back in one host-pointer call (k4lz4_frame_write_batch).  A stream the call refuses reports None and its K4LZ4_FWRITE_* code in
    LastCodes."""

    def __init__(self, n: int, settings=None, ctx: Optional[_native.Context] = None):
        import torch
        self.ctx = ctx or _native.default_context()
        self.n = int(n)
        self.records, self.store_off, size = _writer_records(self.n, settings, self.ctx.lib)
        dev = int(self.ctx.lib.k4lz4_ctx_device(self.ctx.handle))
        self.store = torch.empty(max(size, 1) + 64, dtype=torch.uint8, device=f"cuda:{dev}")
        self.LastCodes = np.zeros(self.n, np.int64)

    def _call(self, chunks, op: int, dst_cap=None) -> List[Optional[bytes]]:
        if len(chunks) != self.n:
            raise ValueError("one chunk (or None) per stream")
        views = [None if c is None else _ro_view(c, "source") for c in chunks]
        lens = np.array([-1 if v is None else v.size for v in views], np.int64)
        src, soff, _ = pack_blocks([v if v is not None else np.zeros(0, np.uint8) for v in views])
        caps = np.array([self.ctx.lib.k4lz4_frame_write_bound(_C.byref(self.records[i]), int(lens[i]), int(op == FWRITE_CLOSE))
                         for i in range(self.n)], np.uint64) if dst_cap is None else np.asarray(dst_cap, np.uint64)
        doff = np.zeros(self.n, np.uint64)
        if self.n > 1:
            doff[1:] = np.cumsum(caps[:-1])
        dst = np.zeros(max(int(caps.sum()), 1), np.uint8)
        out = np.zeros(self.n, np.int64)
        self.ctx.check(self.ctx.lib.k4lz4_frame_write_batch(self.ctx.handle, self.records, self.store.data_ptr(), self.store_off.ctypes.data,
                                                            src.ctypes.data, soff.ctypes.data, lens.ctypes.data, dst.ctypes.data,
                                                            doff.ctypes.data, caps.ctypes.data, out.ctypes.data, self.n, op, 0))
        self.LastCodes = np.minimum(out, 0)
        return [None if (lens[i] < 0 or out[i] < 0) else dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() for i in range(self.n)]

    def Write(self, chunks) -> List[Optional[bytes]]:
        return self._call(chunks, FWRITE_WRITE)

    def Open(self, streams=None) -> List[Optional[bytes]]:
        return self._call([b"" if streams is None or i in streams else None for i in range(self.n)], FWRITE_OPEN)

    def Close(self, streams=None) -> List[Optional[bytes]]:
        return self._call([b"" if streams is None or i in streams else None for i in range(self.n)], FWRITE_CLOSE)

    def Bound(self, stream: int, length: int, closing: bool = False) -> int:
        return int(self.ctx.lib.k4lz4_frame_write_bound(_C.byref(self.records[stream]), int(length), int(closing)))


class FrameWriterDevice:
    """n LZ4FrameWriters over HBM-resident data (k4lz4_frame_write_batch_device): write(data, off, length) takes stream s's bytes
    from data[off[s] : off[s] + length[s]] (data a uint8 torch tensor, off / length host arrays, length < 0: untouched) and returns
    (out, out_off, out_len) like encode_frames_device: stream s's bytes of this call are out[out_off[s] : out_off[s] + out_len[s]],
    out_off a host array, out_len an int64 device tensor (negative: a K4LZ4_FWRITE_* code).  Asynchronous on the current torch
    stream; `dc` is a device.DeviceCodec."""

    def __init__(self, dc, n: int, settings=None):
        import torch
        self.dc = dc
        self.n = int(n)
        self.records, self.store_off, size = _writer_records(self.n, settings, dc.lib)
        self.store = torch.empty(max(size, 1) + 64, dtype=torch.uint8, device=dc.device)

    def bound(self, length, closing: bool = False) -> np.ndarray:
        length = np.broadcast_to(np.asarray(length, np.int64), (self.n,))
        return np.array([self.dc.lib.k4lz4_frame_write_bound(_C.byref(self.records[i]), int(length[i]), int(closing)) for i in range(self.n)],
                        np.uint64)

    def _call(self, data, off, length, op: int, dst_cap=None):
        import torch
        from .device import _dp
        length = np.ascontiguousarray(np.broadcast_to(np.asarray(length, np.int64), (self.n,)))
        off = np.ascontiguousarray(np.broadcast_to(np.asarray(off, np.int64), (self.n,))).astype(np.uint64)
        caps = self.bound(length, op == FWRITE_CLOSE) if dst_cap is None else np.ascontiguousarray(dst_cap, np.uint64)
        out_off = np.zeros(self.n, np.uint64)
        if self.n > 1:
            out_off[1:] = np.cumsum((caps[:-1] + 15) // 16 * 16)
        out = torch.empty(int(((caps + 15) // 16 * 16).sum()) + 64, dtype=torch.uint8, device=self.dc.device)
        out_len = torch.zeros(max(self.n, 1), dtype=torch.int64, device=self.dc.device)
        self.dc.ctx.check(self.dc.lib.k4lz4_frame_write_batch_device(
            self.dc.ctx.handle, self.records, _dp(self.store), self.store_off.ctypes.data, _dp(data), off.ctypes.data, length.ctypes.data,
            _dp(out), out_off.ctypes.data, caps.ctypes.data, _dp(out_len), self.n, op, 0, _C.c_void_p(self.dc._stream())))
        return out, out_off.astype(np.int64), out_len[:self.n]

    def write(self, data, off, length, dst_cap=None):
        return self._call(data, off, length, FWRITE_WRITE, dst_cap)

    def open(self, streams=None):
        return self._call(None, 0, [0 if streams is None or i in streams else -1 for i in range(self.n)], FWRITE_OPEN)

    def close(self, data=None, off=0, length=None, dst_cap=None):
        """CloseFrame; with data, the bytes are written first (Write then CloseFrame in one call)"""
        return self._call(data, off, 0 if length is None else length, FWRITE_CLOSE, dst_cap)


# ---- incremental frame reader: many LZ4FrameReaders, one ReadManyBytes / OpenFrame each per call (k4lz4_frame_read_batch*,
# DESIGN.md 4.14) ------------------------------------------------------------------------------------------------------------
FREAD_READ, FREAD_OPEN, FREAD_RESET = 0, 1, 2
FREAD_INTERACTIVE = 1
FRQ_BYTES_READ, FRQ_FRAME_LENGTH, FRQ_PHASE, FRQ_CODE, FRQ_BLOCKS, FRQ_DIRECT, FRQ_FAST, FRQ_HANDED_BACK, FRQ_WORDS = 0, 1, 2, 3, 4, 5, 6, 7, 8


class FrameReaderRecord(_C.Structure):        # k4lz4_frame_reader: the settings and the per-stream store size, host memory
    _fields_ = [("maxBlockSize", _C.c_int32), ("flags", _C.c_int32), ("storeBytes", _C.c_int64)]


FREADER_FED = 1


def frame_reader_record(max_block_size: int, lib, fed: bool = False) -> FrameReaderRecord:
    """fed: a record for the fed calls (k4lz4_frame_read_fed_batch[_device]); its store has a stash behind the buffer"""
    rec = FrameReaderRecord()
    settings = (_C.c_int32 * 2)(int(max_block_size), FREADER_FED if fed else 0)
    if lib.k4lz4_frame_reader_init(_C.byref(rec), settings) != 0:
        raise ValueError(f"maxBlockSize {max_block_size} is above 4 MiB")
    return rec


def _store_offsets(n: int, rec: FrameReaderRecord):
    return (np.arange(n, dtype=np.uint64) * np.uint64(rec.storeBytes)).astype(np.uint64)


class LZ4FrameReaderBatch:
    """n LZ4FrameReaders (Frames/LZ4FrameReader*.cs, what LZ4DecoderStream.Read drives) advanced together over sources held in host
    memory: Read(counts) is one ReadManyBytes(count) per stream and returns, per stream, the bytes it delivers (b"" at the end of a
    frame and at the end of the source, None where the count is None or negative); Open() is one OpenFrame.  The readers' state lives
    in device memory; every call sends the sources up and brings the bytes back (k4lz4_frame_read_batch).  A stream that fails raises
    the reader's exception (the lowest-index one) when raise_errors, else reports None and its K4LZ4_FRAME_* code in LastCodes; it
    stays failed.  maxBlockSize: the largest block size a frame may declare (the stores are sized by it).
    dictionary=(DictionarySet, ids): k4lz4_frame_read_dictset_batch -- frames with a DictID are read against the first entry of the set
    whose id equals it; without it every DictID is FRAME_DICTIONARY."""

    def __init__(self, sources, maxBlockSize: int = 4 << 20, ctx: Optional[_native.Context] = None, raise_errors: bool = True,
                 dictionary=None):
        import torch
        self.ctx = ctx or _native.default_context()
        self.dictionary, self._dict_args = _reader_dictionary(dictionary)
        self.views = [_ro_view(s, "source") for s in sources]
        self.n = len(self.views)
        self.raise_errors = raise_errors
        self.record = frame_reader_record(maxBlockSize, self.ctx.lib)
        self.store_off = _store_offsets(self.n, self.record)
        dev = int(self.ctx.lib.k4lz4_ctx_device(self.ctx.handle))
        self.store = torch.empty(max(self.n, 1) * int(self.record.storeBytes) + 64, dtype=torch.uint8, device=f"cuda:{dev}")
        self.src, soff, _ = pack_blocks(self.views) if self.n else (np.zeros(16, np.uint8), np.zeros(0, np.uint64), None)
        self.src_off = np.ascontiguousarray(soff, np.uint64)
        self.src_len = np.array([v.size for v in self.views], np.uint64)
        self.LastCodes = np.zeros(self.n, np.int64)
        self._call(FREAD_RESET, np.zeros(self.n, np.int64), False)

    def _call(self, op: int, counts: np.ndarray, interactive: bool):
        caps = np.maximum(counts, 0).astype(np.uint64) if op == FREAD_READ else np.zeros(self.n, np.uint64)
        doff = np.zeros(self.n, np.uint64)
        if self.n > 1:
            doff[1:] = np.cumsum(caps[:-1])
        dst = np.zeros(max(int(caps.sum()), 1), np.uint8)
        out = np.zeros(max(self.n, 1), np.int64)
        call = self.ctx.lib.k4lz4_frame_read_dictset_batch if self.dictionary else self.ctx.lib.k4lz4_frame_read_batch
        self.ctx.check(call(
            self.ctx.handle, _C.byref(self.record), self.store.data_ptr(), self.store_off.ctypes.data, self.src.ctypes.data,
            self.src_off.ctypes.data, self.src_len.ctypes.data, dst.ctypes.data, doff.ctypes.data, counts.ctypes.data, out.ctypes.data,
            self.n, op, FREAD_INTERACTIVE if interactive else 0, *self._dict_args))
        out = out[:self.n]
        self.LastCodes = np.where(counts >= 0, np.minimum(out, 0), 0)
        bad = np.flatnonzero(self.LastCodes < 0)
        if self.raise_errors and bad.size:
            raise frame_exception(int(self.LastCodes[bad[0]]))
        return out, dst, doff

    @staticmethod
    def _counts(counts, n):
        if len(counts) != n:
            raise ValueError("one count (or None) per stream")
        return np.array([-1 if c is None else int(c) for c in counts], np.int64)

    def Read(self, counts, interactive: bool = False) -> List[Optional[bytes]]:
        counts = self._counts(counts, self.n)
        out, dst, doff = self._call(FREAD_READ, counts, interactive)
        return [None if (counts[i] < 0 or out[i] < 0) else dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() for i in range(self.n)]

    def Open(self, streams=None) -> List[Optional[bool]]:
        """OpenFrame per stream: True a frame is open, False the source is at its end, None untouched or failed"""
        counts = np.array([0 if streams is None or i in streams else -1 for i in range(self.n)], np.int64)
        out, _, _ = self._call(FREAD_OPEN, counts, False)
        return [None if (counts[i] < 0 or out[i] < 0) else bool(out[i]) for i in range(self.n)]

    def Query(self) -> np.ndarray:
        """(n, FRQ_WORDS) int64: bytes read, the open frame's ContentLength or -1, phase, code, blocks read, blocks decoded in place"""
        q = np.zeros(max(self.n, 1) * FRQ_WORDS, np.int64)
        self.ctx.check(self.ctx.lib.k4lz4_frame_reader_query(self.ctx.handle, self.store.data_ptr(), self.store_off.ctypes.data, self.n,
                                                             q.ctypes.data))
        return q[:self.n * FRQ_WORDS].reshape(self.n, FRQ_WORDS)

    @property
    def BytesRead(self) -> List[int]:
        return [int(v) for v in self.Query()[:, FRQ_BYTES_READ]]

    @property
    def FrameLength(self) -> List[Optional[int]]:
        """GetFrameLength per stream: opens a frame where none is open, then its ContentLength or None"""
        self.Open()
        return [None if v < 0 else int(v) for v in self.Query()[:, FRQ_FRAME_LENGTH]]


class FrameReaderDevice:
    """n LZ4FrameReaders over HBM-resident sources (k4lz4_frame_read_batch_device): stream s is data[off[s] : off[s] + length[s]]
    (data a uint8 torch tensor; off / length host arrays or device tensors).  read(counts) delivers up to counts[s] bytes per stream
    (host array or device tensor; negative: the stream sits the call out) and returns (out, out_off, out_len): stream s's bytes of
    this call are out[out_off[s] : out_off[s] + out_len[s]], out_len an int64 device tensor (negative: a K4LZ4_FRAME_* code).  With
    out=(buffer, out_off) the bytes go to buffer[out_off[s] : out_off[s] + counts[s]] (host array or device tensor), and with
    device tensors throughout the call touches no host memory.  Asynchronous on the current torch stream: one kernel, no
    synchronisation; `dc` is a device.DeviceCodec.  dictionary=(DictionarySet, ids): k4lz4_frame_read_dictset_batch_device, as
    LZ4FrameReaderBatch; the ids are a host array and go up with every call."""

    def __init__(self, dc, data, off, length, maxBlockSize: int = 4 << 20, dictionary=None):
        import torch
        self.dc = dc
        self.dictionary, self._dict_args = _reader_dictionary(dictionary)
        self.data = data
        self.off, self.length = _dev_i64(off, dc.device), _dev_i64(length, dc.device)
        self.n = int(self.off.numel())
        self.record = frame_reader_record(maxBlockSize, dc.lib)
        self.store_off = torch.from_numpy(_store_offsets(self.n, self.record).astype(np.int64)).to(dc.device)
        self.store = torch.empty(max(self.n, 1) * int(self.record.storeBytes) + 64, dtype=torch.uint8, device=dc.device)
        self._zero = torch.zeros(max(self.n, 1), dtype=torch.int64, device=dc.device)
        self._call(FREAD_RESET, self._zero, None, None, False)

    def _call(self, op, counts, buf, out_off, interactive, max_count=0):
        import torch
        from .device import _dp
        out_len = torch.zeros(max(self.n, 1), dtype=torch.int64, device=self.dc.device)
        if self.n:
            call = self.dc.lib.k4lz4_frame_read_dictset_batch_device if self.dictionary else self.dc.lib.k4lz4_frame_read_batch_device
            self.dc.ctx.check(call(
                self.dc.ctx.handle, _C.byref(self.record), _dp(self.store), _dp(self.store_off), _dp(self.data), _dp(self.off),
                _dp(self.length), _dp(buf), _dp(out_off), _dp(counts), _dp(out_len), self.n, op, FREAD_INTERACTIVE if interactive else 0,
                int(max_count), *self._dict_args,
                _C.c_void_p(self.dc._stream())))
        return out_len[:self.n]

    def read(self, counts, out=None, interactive: bool = False, max_count: Optional[int] = None):
        """max_count: an upper bound of the counts (it sizes the fast path's block table); None: taken from host counts, and for
        device counts 0, which leaves every stream to the general reader"""
        import torch
        if max_count is None and not isinstance(counts, torch.Tensor):
            max_count = int(np.max(np.asarray(counts, np.int64), initial=0))
        if out is None:
            c = np.ascontiguousarray(np.broadcast_to(np.asarray(counts.cpu().numpy() if isinstance(counts, torch.Tensor) else counts,
                                                                np.int64), (self.n,)))
            caps = (np.maximum(c, 0) + 15) // 16 * 16
            out_off = np.zeros(self.n, np.int64)
            if self.n > 1:
                out_off[1:] = np.cumsum(caps[:-1])
            buf = torch.empty(int(caps.sum()) + 64, dtype=torch.uint8, device=self.dc.device)
            counts_d, off_d = _dev_i64(c, self.dc.device), _dev_i64(out_off, self.dc.device)
        else:
            buf, out_off = out
            counts_d, off_d = _dev_i64(counts, self.dc.device), _dev_i64(out_off, self.dc.device)
        return buf, out_off, self._call(FREAD_READ, counts_d, buf, off_d, interactive, max_count or 0)

    def open(self, streams=None):
        """OpenFrame per stream: an int64 device tensor of 1 / 0 / K4LZ4_FRAME_* codes"""
        counts = self._zero if streams is None else _dev_i64([0 if i in streams else -1 for i in range(self.n)], self.dc.device)
        return self._call(FREAD_OPEN, counts, None, None, False)

    def query(self):
        """(n, FRQ_WORDS) int64 device tensor, see LZ4FrameReaderBatch.Query"""
        import torch
        from .device import _dp
        q = torch.zeros(max(self.n, 1) * FRQ_WORDS, dtype=torch.int64, device=self.dc.device)
        if self.n:
            self.dc.ctx.check(self.dc.lib.k4lz4_frame_reader_query_device(self.dc.ctx.handle, _dp(self.store), _dp(self.store_off), self.n,
                                                                          _dp(q), _C.c_void_p(self.dc._stream())))
        return q[:self.n * FRQ_WORDS].reshape(self.n, FRQ_WORDS)


class LZ4FrameFedReaderBatch:
    """n LZ4FrameReaders whose sources arrive in pieces (k4lz4_frame_read_fed_batch): what LZ4DecoderStream does
    over a socket or a pipe.  Feed(pieces, final) appends to a per-stream host queue; Read(counts) presents each stream's unconsumed
    bytes to one ReadManyBytes per stream, drops what was consumed and returns the bytes delivered; Need[s] > 0 then says that the
    read is starved: the field it stands at wants that many further bytes, and the same read is to be issued again with the count
    reduced by what it delivered once more has been fed.  ReadAll(counts) does that over what is queued.  Every source byte goes up
    once.  Errors and dictionary=(DictionarySet, ids) (k4lz4_frame_read_fed_dictset_batch) as LZ4FrameReaderBatch."""

    def __init__(self, n: int, maxBlockSize: int = 4 << 20, ctx: Optional[_native.Context] = None, raise_errors: bool = True,
                 dictionary=None):
        import torch
        self.ctx = ctx or _native.default_context()
        self.dictionary, self._dict_args = _reader_dictionary(dictionary)
        self.n = int(n)
        self.raise_errors = raise_errors
        self.record = frame_reader_record(maxBlockSize, self.ctx.lib, fed=True)
        self.store_off = _store_offsets(self.n, self.record)
        dev = int(self.ctx.lib.k4lz4_ctx_device(self.ctx.handle))
        self.store = torch.empty(max(self.n, 1) * int(self.record.storeBytes) + 64, dtype=torch.uint8, device=f"cuda:{dev}")
        self.queue = [bytearray() for _ in range(self.n)]
        self.final = np.zeros(self.n, np.int64)
        self.LastCodes = np.zeros(self.n, np.int64)
        self.Need = np.zeros(self.n, np.int64)
        self.Consumed = np.zeros(self.n, np.int64)
        self.call(FREAD_RESET, [b""] * self.n, self.final, np.zeros(self.n, np.int64), False)

    def call(self, op: int, pieces, final, counts, interactive: bool):
        """the raw call: pieces[s] is the part of stream s's source that has not been consumed yet -> (outLen, [bytes], consumed, need)"""
        n = self.n
        counts = np.ascontiguousarray(counts, np.int64)
        final = np.ascontiguousarray(final, np.int64)
        views = [_ro_view(p, "piece") for p in pieces]
        src, soff, _ = pack_blocks(views) if n else (np.zeros(16, np.uint8), np.zeros(0, np.uint64), None)
        src_off = np.ascontiguousarray(soff, np.uint64)
        src_len = np.array([v.size for v in views], np.uint64)
        caps = np.maximum(counts, 0).astype(np.uint64) if op == FREAD_READ else np.zeros(n, np.uint64)
        doff = np.zeros(n, np.uint64)
        if n > 1:
            doff[1:] = np.cumsum(caps[:-1])
        dst = np.zeros(max(int(caps.sum()), 1), np.uint8)
        out, consumed, need = (np.zeros(max(n, 1), np.int64) for _ in range(3))
        call = self.ctx.lib.k4lz4_frame_read_fed_dictset_batch if self.dictionary else self.ctx.lib.k4lz4_frame_read_fed_batch
        self.ctx.check(call(
            self.ctx.handle, _C.byref(self.record), self.store.data_ptr(), self.store_off.ctypes.data, src.ctypes.data,
            src_off.ctypes.data, src_len.ctypes.data, final.ctypes.data, dst.ctypes.data, doff.ctypes.data, counts.ctypes.data,
            out.ctypes.data, consumed.ctypes.data, need.ctypes.data, n, op, FREAD_INTERACTIVE if interactive else 0, *self._dict_args))
        out = out[:n]
        data = [dst[int(doff[i]):int(doff[i]) + max(int(out[i]), 0)].tobytes() if op == FREAD_READ else b"" for i in range(n)]
        return out, data, consumed[:n], need[:n]

    def Feed(self, pieces, final=None) -> None:
        """pieces[s]: the next bytes of stream s's source (None: none now); final[s]: no byte follows them"""
        if len(pieces) != self.n or (final is not None and len(final) != self.n):
            raise ValueError("one piece (or None) per stream")
        for i, p in enumerate(pieces):
            if p is not None and len(p):
                if self.final[i]:
                    raise ValueError(f"stream {i} was fed its final piece already")
                self.queue[i] += bytes(p)
            if final is not None and final[i]:
                self.final[i] = 1

    def _queued(self, op, counts, interactive):
        out, data, consumed, need = self.call(op, [bytes(q) for q in self.queue], self.final, counts, interactive)
        for i in range(self.n):
            if counts[i] >= 0 and out[i] >= 0:
                del self.queue[i][:int(consumed[i])]
        self.Consumed, self.Need = consumed.copy(), np.where(out >= 0, need, 0)
        self.LastCodes = np.where(counts >= 0, np.minimum(out, 0), 0)
        bad = np.flatnonzero(self.LastCodes < 0)
        if self.raise_errors and bad.size:
            raise frame_exception(int(self.LastCodes[bad[0]]))
        return out, data

    def Read(self, counts, interactive: bool = False) -> List[Optional[bytes]]:
        counts = LZ4FrameReaderBatch._counts(counts, self.n)
        out, data = self._queued(FREAD_READ, counts, interactive)
        return [None if (counts[i] < 0 or out[i] < 0) else data[i] for i in range(self.n)]

    def ReadAll(self, counts, interactive: bool = False) -> List[Optional[bytes]]:
        """a logical read over what is queued: a starved stream is read again while its queue holds the bytes it needs"""
        left = LZ4FrameReaderBatch._counts(counts, self.n)
        acc: List[Optional[bytearray]] = [None if c < 0 else bytearray() for c in left]
        while (left >= 0).any():
            got = self.Read([None if c < 0 else int(c) for c in left], interactive)
            for i in range(self.n):
                if left[i] < 0:
                    continue
                if got[i] is None:
                    acc[i], left[i] = None, -1
                    continue
                acc[i] += got[i]
                again = self.Need[i] > 0 and len(self.queue[i]) > 0
                left[i] = left[i] - len(got[i]) if again else -1
        return [None if a is None else bytes(a) for a in acc]

    def Open(self, streams=None) -> List[Optional[bool]]:
        """OpenFrame per stream: True a frame is open, False the source is at its end or (Need[s] > 0) the header is not all there"""
        counts = np.array([0 if streams is None or i in streams else -1 for i in range(self.n)], np.int64)
        out, _ = self._queued(FREAD_OPEN, counts, False)
        return [None if (counts[i] < 0 or out[i] < 0) else bool(out[i]) for i in range(self.n)]

    def Query(self) -> np.ndarray:
        q = np.zeros(max(self.n, 1) * FRQ_WORDS, np.int64)
        self.ctx.check(self.ctx.lib.k4lz4_frame_reader_query(self.ctx.handle, self.store.data_ptr(), self.store_off.ctypes.data, self.n,
                                                             q.ctypes.data))
        return q[:self.n * FRQ_WORDS].reshape(self.n, FRQ_WORDS)

    @property
    def BytesRead(self) -> List[int]:
        return [int(v) for v in self.Query()[:, FRQ_BYTES_READ]]


class FrameFedReaderDevice:
    """n fed LZ4FrameReaders over pieces in HBM (k4lz4_frame_read_fed_batch_device).  Per call stream s is given
    data[off[s] : off[s] + length[s]], the part of its source it has not consumed yet, and final[s] (None: none is final); read()
    returns (out, out_off, out_len, consumed, need), the last three int64 device tensors.  Arguments as FrameReaderDevice.read;
    asynchronous on the current torch stream, nothing is read back.  dictionary=(DictionarySet, ids):
    k4lz4_frame_read_fed_dictset_batch_device, as FrameReaderDevice."""

    def __init__(self, dc, n: int, maxBlockSize: int = 4 << 20, dictionary=None):
        import torch
        self.dc = dc
        self.dictionary, self._dict_args = _reader_dictionary(dictionary)
        self.n = int(n)
        self.record = frame_reader_record(maxBlockSize, dc.lib, fed=True)
        self.store_off = torch.from_numpy(_store_offsets(self.n, self.record).astype(np.int64)).to(dc.device)
        self.store = torch.empty(max(self.n, 1) * int(self.record.storeBytes) + 64, dtype=torch.uint8, device=dc.device)
        self._zero = torch.zeros(max(self.n, 1), dtype=torch.int64, device=dc.device)
        self._call(FREAD_RESET, None, self._zero, self._zero, None, self._zero, None, None, False)

    def _call(self, op, data, off, length, final, counts, buf, out_off, interactive, max_count=0):
        import torch
        from .device import _dp
        out_len, consumed, need = (torch.zeros(max(self.n, 1), dtype=torch.int64, device=self.dc.device) for _ in range(3))
        if self.n:
            call = self.dc.lib.k4lz4_frame_read_fed_dictset_batch_device if self.dictionary else self.dc.lib.k4lz4_frame_read_fed_batch_device
            self.dc.ctx.check(call(
                self.dc.ctx.handle, _C.byref(self.record), _dp(self.store), _dp(self.store_off), _dp(data), _dp(off), _dp(length),
                _dp(final), _dp(buf), _dp(out_off), _dp(counts), _dp(out_len), _dp(consumed), _dp(need), self.n, op,
                FREAD_INTERACTIVE if interactive else 0, int(max_count), *self._dict_args, _C.c_void_p(self.dc._stream())))
        return out_len[:self.n], consumed[:self.n], need[:self.n]

    def _pieces(self, off, length, final):
        dev = self.dc.device
        return _dev_i64(off, dev), _dev_i64(length, dev), None if final is None else _dev_i64(final, dev)

    def read(self, data, off, length, final, counts, out=None, interactive: bool = False, max_count: Optional[int] = None):
        import torch
        off_d, len_d, fin_d = self._pieces(off, length, final)
        if max_count is None and not isinstance(counts, torch.Tensor):
            max_count = int(np.max(np.asarray(counts, np.int64), initial=0))
        if out is None:
            c = np.ascontiguousarray(np.broadcast_to(np.asarray(counts.cpu().numpy() if isinstance(counts, torch.Tensor) else counts,
                                                                np.int64), (self.n,)))
            caps = (np.maximum(c, 0) + 15) // 16 * 16
            out_off = np.zeros(self.n, np.int64)
            if self.n > 1:
                out_off[1:] = np.cumsum(caps[:-1])
            buf = torch.empty(int(caps.sum()) + 64, dtype=torch.uint8, device=self.dc.device)
            counts_d, ooff_d = _dev_i64(c, self.dc.device), _dev_i64(out_off, self.dc.device)
        else:
            buf, out_off = out
            counts_d, ooff_d = _dev_i64(counts, self.dc.device), _dev_i64(out_off, self.dc.device)
        return (buf, out_off) + self._call(FREAD_READ, data, off_d, len_d, fin_d, counts_d, buf, ooff_d, interactive, max_count or 0)

    def open(self, data, off, length, final, streams=None):
        """-> (out_len, consumed, need): out_len 1 / 0 / a K4LZ4_FRAME_* code"""
        off_d, len_d, fin_d = self._pieces(off, length, final)
        counts = self._zero if streams is None else _dev_i64([0 if i in streams else -1 for i in range(self.n)], self.dc.device)
        return self._call(FREAD_OPEN, data, off_d, len_d, fin_d, counts, None, None, False)

    def query(self):
        import torch
        from .device import _dp
        q = torch.zeros(max(self.n, 1) * FRQ_WORDS, dtype=torch.int64, device=self.dc.device)
        if self.n:
            self.dc.ctx.check(self.dc.lib.k4lz4_frame_reader_query_device(self.dc.ctx.handle, _dp(self.store), _dp(self.store_off), self.n,
                                                                          _dp(q), _C.c_void_p(self.dc._stream())))
        return q[:self.n * FRQ_WORDS].reshape(self.n, FRQ_WORDS)
