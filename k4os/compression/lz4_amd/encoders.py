"""Host-side mirror of the independent-block stream encoder / decoder, backed by
libk4lz4.so.

Mirrors:
  ILZ4Encoder  (Topup / Encode / BlockSize / BytesReady)      Encoders/ILZ4Encoder.cs
  LZ4EncoderBase                                              Encoders/LZ4EncoderBase.cs:28-97
  LZ4BlockEncoder(level, blockSize)                           Encoders/LZ4BlockEncoder.cs:7-23
  LZ4HighChainEncoder(level, blockSize, extraBlocks)          Encoders/LZ4HighChainEncoder.cs (-> LZ4_compress_HC_continue,
                                                              LZ4_saveDictHC over LZ4EncoderBase's ring buffer)
  ILZ4Decoder  (Decode / Inject / Drain / Peek / BytesReady)  Encoders/ILZ4Decoder.cs
  LZ4BlockDecoder(blockSize)                                  Encoders/LZ4BlockDecoder.cs:11-106
  LZ4ChainDecoder(blockSize, extraBlocks)                     Encoders/LZ4ChainDecoder.cs
  LZ4Decoder.Create(chaining, blockSize, extraBlocks)         Encoders/LZ4Decoder.cs
  LZ4EncoderExtensions.TopupAndEncode / FlushAndEncode /
      DecodeAndDrain, EncoderAction                           Encoders/LZ4EncoderExtensions.cs:8-205, EncoderAction.cs
  LZ4FastChainEncoder(blockSize, extraBlocks)                 Encoders/LZ4FastChainEncoder.cs (-> LZ4_compress_fast_continue,
                                                              LZ4_saveDict over LZ4EncoderBase's ring buffer)
Chained HC blocks batch like independent ones: the HC tables are a function of the data alone, so a
block needs the bytes before it (at most 64 KiB of them), not the parse of the block before it
(k4lz4_encode_hc_chain_batch).  The chained FAST encoder's hash table holds only the
positions its parse visited, so every block depends on the parse of the one before it: one wavefront
encodes a stream's blocks in order with the table in LDS, many streams side by side
(k4lz4_encode_fast_chain_batch); the table and indices travel between calls as a state blob
(k4lz4_fast_chain_state).  Chained *decoding* of a stream that is all there is frames.py's (k4lz4_decode_chain_batch); of
blocks that arrive over time it is LZ4ChainDecoder's here: the decoder's state and ring buffer live in a device store and every call
applies a run of Decode / Inject records (k4lz4_chain_decode_batch) -- `LZ4ChainDecoderBatch` for many open
decoders, `LZ4ChainDecoder` the single ILZ4Decoder over a batch of one, `LZ4Decoder.Create` the reference's factory.

`LZ4BlockEncoder.EncodeBlocks` is the batching front-end the frame writer uses: K blocks, one launch,
with the reference's allowCopy rule applied on the device; `encode_hc_chain_packed` / `encode_fast_chain_packed`
are the same for whole chained streams, `LZ4HighChainEncoder.EncodeBlocks` / `LZ4FastChainEncoder.EncodeBlocks`
for the blocks of one.
"""
from __future__ import annotations

import ctypes as _C
import enum
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from ._native import FLAG_ALLOW_COPY
from .codec import LZ4Codec, LZ4Level, _ro_view, _rw_view, _batch_args, pack_blocks, make_arena

K1 = 1024


class InvalidOperationException(Exception):
    """System.InvalidOperationException"""


class EncoderAction(enum.IntEnum):          # Encoders/EncoderAction.cs
    None_ = 0
    Loaded = 1
    Encoded = 2
    Copied = 3


def _round_block_size(block_size: int) -> int:
    block_size = max(int(block_size), K1)
    return (block_size + K1 - 1) // K1 * K1                      # Mem.RoundUp(Math.Max(blockSize, Mem.K1), Mem.K1)


class LZ4BlockEncoder:
    """Independent block encoder (LZ4BlockEncoder.cs): every block is LZ4Codec.Encode of its own bytes."""

    def __init__(self, level: LZ4Level = LZ4Level.L00_FAST, blockSize: int = 65536):
        self._level = LZ4Level(level)
        self._block_size = _round_block_size(blockSize)
        self._input = np.zeros(self._block_size + 32 + 8, np.uint8)   # LZ4EncoderBase.cs:34-37, no dictionary part
        self._index = 0
        self._pointer = 0

    @property
    def BlockSize(self) -> int:
        return self._block_size

    @property
    def BytesReady(self) -> int:
        return self._pointer - self._index

    def Topup(self, source, offset: int = 0, length: Optional[int] = None) -> int:
        """copies up to the free space of the current block; returns bytes taken (LZ4EncoderBase.cs:46-62)"""
        src = _ro_view(source, "source")
        length = src.size - offset if length is None else int(length)
        if length == 0:
            return 0
        space = self._index + self._block_size - self._pointer
        if space <= 0:
            return 0
        chunk = min(space, length)
        self._input[self._pointer:self._pointer + chunk] = src[offset:offset + chunk]
        self._pointer += chunk
        return chunk

    def Encode(self, target, offset: int = 0, length: Optional[int] = None, allowCopy: bool = False) -> int:
        """encodes the pending bytes as one block into target; with allowCopy a block that does not shrink
        is stored raw and -length is returned (LZ4EncoderBase.cs:66-88)"""
        dst = _rw_view(target, "target")
        length = dst.size - offset if length is None else int(length)
        n = self._pointer - self._index
        if n <= 0:
            return 0
        encoded = LZ4Codec.Encode(self._input, self._index, n, dst, offset, length, self._level)
        if encoded <= 0:
            raise InvalidOperationException("Failed to encode chunk. Target buffer too small.")
        if allowCopy and encoded >= n:
            dst[offset:offset + n] = self._input[self._index:self._index + n]
            encoded = -n
        self._index = self._pointer = 0                              # Commit(): CopyDict returns 0 for independent blocks
        return encoded

    # ---- batching front-end ---------------------------------------------------------------------
    def EncodeBlocks(self, sources: Sequence, allowCopy: bool = True,
                     ctx: Optional[_native.Context] = None) -> List[Tuple[EncoderAction, bytes]]:
        """each element (at most BlockSize bytes) as Topup + Encode(allowCopy) would produce it, one launch"""
        blocks = [_ro_view(s, "source") for s in sources]
        for b in blocks:
            if b.size > self._block_size:
                raise InvalidOperationException("block larger than BlockSize")
        out, dst, doff = encode_blocks_packed(blocks, self._level, allowCopy, ctx)
        res = []
        for n, o, b in zip(out, doff, blocks):
            if b.size == 0:
                res.append((EncoderAction.None_, b""))
            elif n == 0:
                raise InvalidOperationException("Failed to encode chunk. Target buffer too small.")
            elif n < 0:
                res.append((EncoderAction.Copied, dst[int(o):int(o) - int(n)].tobytes()))
            else:
                res.append((EncoderAction.Encoded, dst[int(o):int(o) + int(n)].tobytes()))
        return res


def encode_blocks_packed(blocks, level: LZ4Level, allow_copy: bool, ctx: Optional[_native.Context] = None):
    """-> (outLen int32 (negative: stored raw), arena, arena offsets)"""
    ctx = ctx or _native.default_context()
    src, soff, slen = pack_blocks(blocks)
    caps = np.array([LZ4Codec.MaximumOutputSize(b.size) for b in blocks], dtype=np.int32)
    dst, doff = make_arena(caps)
    out = np.empty(len(blocks), dtype=np.int32)
    a = _batch_args(src, soff, slen, dst, doff, caps, out)
    ctx.check(ctx.lib.k4lz4_encode_batch(ctx.handle, *a, int(level), FLAG_ALLOW_COPY if allow_copy else 0))
    return out, dst, doff


# ---- chained HC streams ---------------------------------------------------------------------------------
HC_CHAIN_LIMIT = (1 << 31) - 65536      # LZ4_compressHC_continue_generic renormalises a block that starts beyond this (LL64.high.cs:1271-1276)


def hc_chain_blocks(length: int, blockSize: int, extraBlocks: int = 0, dictLen: int = 0) -> List[Tuple[int, int, int]]:
    """LZ4HighChainEncoder's blocks of a content in content coordinates: (start, length, dictLimit) per block -- the model
    LZ4EncoderBase's ring buffer reduces to (Topup / Encode / Commit -> LZ4_saveDictHC).  dictLen: the content's first bytes are
    what the ring buffer already holds (no block for them).  The library builds the same table (k4lz4_capi.hip,
    hc_chain_table: the stream's block lengths through k4lz4_chain_encoder.hpp's ce_hc_rows)."""
    B = _round_block_size(blockSize)
    L = 65536 + (1 + max(int(extraBlocks), 0)) * B + 32
    ptr = s = int(dictLen)
    dl = 0
    out = []
    while s < length:
        n = min(B, length - s)
        out.append((s, n, dl))
        s += n
        ptr += n
        if ptr + B > L:                                  # Commit -> LZ4_saveDictHC(ctx, buf, ptr), LL.high.cs:168
            d = min(65536, ptr, s - dl)
            d = 0 if d < 4 else d
            dl, ptr = s - d, d
    return out


def encode_hc_chain_packed(contents: Sequence, blockSize: Union[int, Sequence[int]], extraBlocks: Union[int, Sequence[int]],
                           level: LZ4Level, allow_copy: bool, ctx: Optional[_native.Context] = None, dictLen=None):
    """chained HC streams, one call (k4lz4_encode_hc_chain_batch) -> (outLen int32 per block, streams in order (negative: stored
    raw), arena, arena offset per block, blocks per stream)"""
    ctx = ctx or _native.default_context()
    views = [_ro_view(c, "source") for c in contents]
    ns = len(views)
    bs = np.broadcast_to(np.asarray(blockSize, np.int64), (ns,)).astype(np.int32)
    ex = np.broadcast_to(np.asarray(extraBlocks, np.int64), (ns,)).astype(np.int32)
    dlen = np.zeros(ns, np.int32) if dictLen is None else np.asarray(dictLen, np.int32).reshape(ns)
    src, soff, _ = pack_blocks(views)
    slen = np.array([v.size for v in views], np.int64)
    B = np.array([_round_block_size(int(b)) for b in bs], np.int64)
    nblk = (slen - dlen + B - 1) // B
    slot = B + B // 255 + 16                                   # LZ4Codec.MaximumOutputSize(B)
    doff = np.zeros(ns, np.uint64)
    if ns > 1:
        doff[1:] = np.cumsum((nblk * slot)[:-1]).astype(np.uint64)
    nb = int(nblk.sum())
    dst = np.empty(max(int((nblk * slot).sum()), 1), np.uint8)
    out = np.zeros(max(nb, 1), np.int32)
    ctx.check(ctx.lib.k4lz4_encode_hc_chain_batch(ctx.handle, src.ctypes.data, soff.ctypes.data, slen.ctypes.data, bs.ctypes.data,
                                                  ex.ctypes.data, dlen.ctypes.data, ns, dst.ctypes.data, doff.ctypes.data,
                                                  out.ctypes.data, nb, int(level), FLAG_ALLOW_COPY if allow_copy else 0))
    boff = np.concatenate([doff[f] + np.arange(nblk[f], dtype=np.uint64) * np.uint64(slot[f]) for f in range(ns)]) if nb else np.zeros(0, np.uint64)
    return out[:nb], dst, boff, nblk


class LZ4HighChainEncoder:
    """Chained HC encoder (LZ4HighChainEncoder.cs over LZ4EncoderBase.cs): every block is LZ4_compress_HC_continue with the
    blocks before it as history.  The ring buffer is the reference's, byte for byte (Topup / Encode / Commit); a block is encoded
    on the device with what the buffer holds in front of it.  `EncodeBlocks` hands many blocks of the stream to one call."""

    def __init__(self, level: LZ4Level = LZ4Level.L09_HC, blockSize: int = 65536, extraBlocks: int = 0):
        level = int(level)
        self._level = LZ4Level(min(max(level, int(LZ4Level.L03_HC)), int(LZ4Level.L12_MAX)))   # LZ4HighChainEncoder.cs:19-20
        self._block_size = _round_block_size(blockSize)
        self._extra = max(int(extraBlocks), 0)
        self._length = 65536 + (1 + self._extra) * self._block_size + 32                      # LZ4EncoderBase.cs:25
        self._input = np.zeros(self._length + 8, np.uint8)
        self._index = 0
        self._pointer = 0
        self._position = 0                       # stream bytes encoded so far (the 2 GB renormalisation is not offered)

    @property
    def BlockSize(self) -> int:
        return self._block_size

    @property
    def BytesReady(self) -> int:
        return self._pointer - self._index

    def Topup(self, source, offset: int = 0, length: Optional[int] = None) -> int:
        """LZ4EncoderBase.cs:46-62"""
        src = _ro_view(source, "source")
        length = src.size - offset if length is None else int(length)
        if length == 0:
            return 0
        space = self._index + self._block_size - self._pointer
        if space <= 0:
            return 0
        chunk = min(space, length)
        self._input[self._pointer:self._pointer + chunk] = src[offset:offset + chunk]
        self._pointer += chunk
        return chunk

    def _commit(self) -> None:
        """LZ4EncoderBase.Commit -> LZ4_saveDictHC(ctx, buffer, pointer)"""
        self._index = self._pointer
        if self._index + self._block_size <= self._length:
            return
        d = min(65536, self._pointer)
        d = 0 if d < 4 else d
        self._input[:d] = self._input[self._pointer - d:self._pointer].copy()
        self._index = self._pointer = d

    def Encode(self, target, offset: int = 0, length: Optional[int] = None, allowCopy: bool = False) -> int:
        """encodes the pending bytes as one block into target; with allowCopy a block that does not shrink is stored raw and
        -length is returned (LZ4EncoderBase.cs:66-88)"""
        dst = _rw_view(target, "target")
        length = dst.size - offset if length is None else int(length)
        n = self._pointer - self._index
        if n <= 0:
            return 0
        if self._position > HC_CHAIN_LIMIT:
            raise NotImplementedError("a chained HC stream beyond 2 GB (the encoder's renormalisation) is not supported")
        out, arena, boff, _ = encode_hc_chain_packed([self._input[:self._pointer]], self._block_size, self._extra, self._level,
                                                     allowCopy, dictLen=[self._index])
        encoded = int(out[0])
        if encoded == 0 or abs(encoded) > length:
            raise InvalidOperationException("Failed to encode chunk. Target buffer too small.")
        dst[offset:offset + abs(encoded)] = arena[int(boff[0]):int(boff[0]) + abs(encoded)]
        self._position += n
        self._commit()
        return encoded

    def EncodeBlocks(self, sources: Sequence, allowCopy: bool = True,
                     ctx: Optional[_native.Context] = None) -> List[Tuple[EncoderAction, bytes]]:
        """the next blocks of the stream, as Topup + Encode(allowCopy) per element would produce them, in one call.  Every
        element but the last is BlockSize bytes (the encoder's blocks are what the ring buffer cuts), the last at most that;
        nothing may be pending."""
        blocks = [_ro_view(s, "source") for s in sources]
        if self.BytesReady:
            raise InvalidOperationException("bytes are pending: Encode them first")
        for i, b in enumerate(blocks):
            if b.size > self._block_size or (i < len(blocks) - 1 and b.size != self._block_size):
                raise InvalidOperationException("every block but the last must be BlockSize bytes")
        blocks = [b for b in blocks if b.size]
        if not blocks:
            return [(EncoderAction.None_, b"") for _ in sources]
        total = sum(b.size for b in blocks)
        if self._position + total - blocks[-1].size > HC_CHAIN_LIMIT:
            raise NotImplementedError("a chained HC stream beyond 2 GB (the encoder's renormalisation) is not supported")
        content = np.concatenate([self._input[:self._index]] + blocks)
        out, arena, boff, _ = encode_hc_chain_packed([content], self._block_size, self._extra, self._level, allowCopy, ctx,
                                                     dictLen=[self._index])
        res = []
        for n, o in zip(out, boff):
            if n == 0:
                raise InvalidOperationException("Failed to encode chunk. Target buffer too small.")
            res.append((EncoderAction.Copied if n < 0 else EncoderAction.Encoded, arena[int(o):int(o) + abs(int(n))].tobytes()))
        # the ring buffer as the blocks one by one would have left it
        for b in blocks:
            self.Topup(b)
            self._position += b.size
            self._commit()
        return res + [(EncoderAction.None_, b"")] * (len(sources) - len(res))


# ---- chained fast streams ------------------------------------------------------------------------------
FAST_CHAIN_LIMIT = 1 << 31       # LZ4_renormDictT rescales the table once currentOffset + inputSize passes this (LL64.tools.cs:157-173)
FAST_CHAIN_STATE = np.dtype([("hashTable", "<u4", (4096,)), ("currentOffset", "<u4"), ("dictSize", "<u4"), ("reserved", "<u4", (2,))])
"""k4lz4_fast_chain_state: LZ4_stream_t's hashTable and indices, word for word"""


def fast_chain_blocks(length: int, blockSize: int, extraBlocks: int = 0, dictLen: int = 0,
                      currentOffset: Optional[int] = None) -> List[Tuple[int, int, int, bool]]:
    """LZ4FastChainEncoder's blocks of a content in content coordinates: (start, length, dictSize, dictSmall) per block -- the
    model LZ4EncoderBase's ring buffer reduces to (Topup / Encode / Commit -> LZ4_saveDict).  dictLen: the content's first bytes are
    what the ring buffer already holds (= the stream context's dictSize); currentOffset: the context's index at that point (default:
    dictLen, a stream from its start).  dictSize is what the ring holds in front of the block, dictSmall LZ4_compress_fast_continue's
    choice of dictIssue (LL64.fast.cs:617, :650).  The library builds the same table (k4lz4_capi.hip, fast_chain_table:
    the stream's block lengths through k4lz4_chain_encoder.hpp's ce_fast_rows)."""
    B = _round_block_size(blockSize)
    L = 65536 + (1 + max(int(extraBlocks), 0)) * B + 32
    s = ptr = d = int(dictLen)
    cur = d if currentOffset is None else int(currentOffset)
    out = []
    while s < length:
        n = min(B, length - s)
        if cur + n > FAST_CHAIN_LIMIT:
            raise NotImplementedError("a chained fast stream beyond 2 GB (the encoder's renormalisation) is not supported")
        out.append((s, n, d, d < 65536 and d < cur))
        s += n
        ptr += n
        d += n                                           # LZ4_compress_generic: dictSize += inputSize (the first call's extDict arm: = inputSize)
        cur += n
        if ptr + B > L:                                  # Commit -> LZ4_saveDict(ctx, buf, ptr): ptr == dictSize
            d = ptr = min(65536, d)
    return out


def _fast_chain_args(contents, blockSize, extraBlocks, state_in, dictLen):
    views = [_ro_view(c, "source") for c in contents]
    ns = len(views)
    bs = np.broadcast_to(np.asarray(blockSize, np.int64), (ns,)).astype(np.int32)
    ex = np.broadcast_to(np.asarray(extraBlocks, np.int64), (ns,)).astype(np.int32)
    if state_in is not None:
        state_in = np.ascontiguousarray(state_in, FAST_CHAIN_STATE).reshape(ns)
    if dictLen is None:
        dlen = state_in["dictSize"].astype(np.int32) if state_in is not None else np.zeros(ns, np.int32)
    else:
        dlen = np.asarray(dictLen, np.int32).reshape(ns)
    slen = np.array([v.size for v in views], np.int64)
    B = np.array([_round_block_size(int(b)) for b in bs], np.int64)
    nblk = np.maximum(slen - dlen + B - 1, 0) // B
    slot = B + B // 255 + 16                                   # LZ4Codec.MaximumOutputSize(B)
    doff = np.zeros(ns, np.uint64)
    if ns > 1:
        doff[1:] = np.cumsum((nblk * slot)[:-1]).astype(np.uint64)
    return views, bs, ex, state_in, dlen, slen, nblk, slot, doff


def _fast_chain_flags(allow_copy: bool) -> int:
    if LZ4Codec.Enforce32:
        raise NotImplementedError("the 32-bit engine's chained fast encoder (LZ4Codec.Enforce32) is not supported")
    return FLAG_ALLOW_COPY if allow_copy else 0


def encode_fast_chain_packed(contents: Sequence, blockSize: Union[int, Sequence[int]], extraBlocks: Union[int, Sequence[int]] = 0,
                             allow_copy: bool = True, ctx: Optional[_native.Context] = None, state_in=None, want_state: bool = False,
                             dictLen=None):
    """chained fast streams, one call (k4lz4_encode_fast_chain_batch) -> (outLen int32 per block, streams in order (negative: stored
    raw), arena, arena offset per block, blocks per stream, state after each stream (FAST_CHAIN_STATE) or None).  state_in: one state
    per stream (None: fresh streams); the content's first state.dictSize bytes are then the ring buffer's (dictLen)."""
    flags = _fast_chain_flags(allow_copy)
    ctx = ctx or _native.default_context()
    views, bs, ex, state_in, dlen, slen, nblk, slot, doff = _fast_chain_args(contents, blockSize, extraBlocks, state_in, dictLen)
    ns = len(views)
    src, soff, _ = pack_blocks(views)
    nb = int(nblk.sum())
    dst = np.empty(max(int((nblk * slot).sum()), 1), np.uint8)
    out = np.zeros(max(nb, 1), np.int32)
    st_out = np.zeros(ns, FAST_CHAIN_STATE) if want_state else None
    ctx.check(ctx.lib.k4lz4_encode_fast_chain_batch(ctx.handle, src.ctypes.data, soff.ctypes.data, slen.ctypes.data, bs.ctypes.data,
                                                    ex.ctypes.data, dlen.ctypes.data, ns,
                                                    None if state_in is None else state_in.ctypes.data,
                                                    None if st_out is None else st_out.ctypes.data,
                                                    dst.ctypes.data, doff.ctypes.data, out.ctypes.data, nb, flags))
    boff = np.concatenate([doff[f] + np.arange(nblk[f], dtype=np.uint64) * np.uint64(slot[f]) for f in range(ns)]) if nb else np.zeros(0, np.uint64)
    return out[:nb], dst, boff, nblk, st_out


def encode_fast_chain_device(dc, data, off, length, blockSize, extraBlocks=0, allow_copy: bool = True, state_in=None,
                             want_state: bool = False, dictLen=None):
    """encode_fast_chain_packed on HBM-resident contents (k4lz4_encode_fast_chain_batch_device): `data` a uint8 torch tensor, content s =
    data[off[s] : off[s] + length[s]] (off / length host arrays).  state_in: a uint8 torch tensor of one state per stream on the device,
    or None.  Returns (outLen, arena, arena offset per block (host), blocks per stream, states after the streams (uint8 tensor) or None),
    asynchronous on the current torch stream; `dc` is a device.DeviceCodec."""
    import torch
    from .device import _dp
    flags = _fast_chain_flags(allow_copy)
    off = np.ascontiguousarray(off, np.uint64)
    length = np.ascontiguousarray(length, np.int64)
    ns = len(off)
    bs = np.broadcast_to(np.asarray(blockSize, np.int64), (ns,)).astype(np.int32)
    ex = np.broadcast_to(np.asarray(extraBlocks, np.int64), (ns,)).astype(np.int32)
    dlen = np.zeros(ns, np.int32) if dictLen is None else np.asarray(dictLen, np.int32).reshape(ns)
    B = np.array([_round_block_size(int(b)) for b in bs], np.int64)
    nblk = np.maximum(length - dlen + B - 1, 0) // B
    slot = B + B // 255 + 16
    doff = np.zeros(ns, np.uint64)
    if ns > 1:
        doff[1:] = np.cumsum((nblk * slot)[:-1]).astype(np.uint64)
    nb = int(nblk.sum())
    dev = dc.device
    arena = torch.empty(max(int((nblk * slot).sum()), 1) + 64, dtype=torch.uint8, device=dev)
    out = torch.zeros(max(nb, 1), dtype=torch.int32, device=dev)
    st_out = torch.zeros(ns * FAST_CHAIN_STATE.itemsize, dtype=torch.uint8, device=dev) if want_state else None
    import ctypes as C
    dc.ctx.check(dc.lib.k4lz4_encode_fast_chain_batch_device(dc.ctx.handle, _dp(data), off.ctypes.data, length.ctypes.data, bs.ctypes.data,
                                                             ex.ctypes.data, dlen.ctypes.data, ns, _dp(state_in), _dp(st_out), _dp(arena),
                                                             doff.ctypes.data, _dp(out), nb, flags, C.c_void_p(dc._stream())))
    boff = np.concatenate([doff[f] + np.arange(nblk[f], dtype=np.uint64) * np.uint64(slot[f]) for f in range(ns)]) if nb else np.zeros(0, np.uint64)
    return out[:nb], arena, boff, nblk, st_out


class LZ4FastChainEncoder:
    """Chained fast encoder (LZ4FastChainEncoder.cs over LZ4EncoderBase.cs): every block is LZ4_compress_fast_continue with the
    blocks before it as history.  The ring buffer is the reference's, byte for byte (Topup / Encode / Commit -> LZ4_saveDict); the
    stream context (hash table, currentOffset, dictSize) lives in a k4lz4_fast_chain_state blob that every call hands to the device
    and takes back.  `EncodeBlocks` hands many blocks of the stream to one call."""

    def __init__(self, blockSize: int = 65536, extraBlocks: int = 0):
        self._block_size = _round_block_size(blockSize)
        self._extra = max(int(extraBlocks), 0)
        self._length = 65536 + (1 + self._extra) * self._block_size + 32                      # LZ4EncoderBase.cs:25
        self._input = np.zeros(self._length + 8, np.uint8)
        self._index = 0
        self._pointer = 0
        self._state = np.zeros(1, FAST_CHAIN_STATE)                                            # Mem.AllocZero(sizeof(LZ4_stream_t))

    @property
    def BlockSize(self) -> int:
        return self._block_size

    @property
    def BytesReady(self) -> int:
        return self._pointer - self._index

    @property
    def State(self) -> np.ndarray:
        """the stream context as it stands (FAST_CHAIN_STATE, a copy)"""
        return self._state.copy()

    def Topup(self, source, offset: int = 0, length: Optional[int] = None) -> int:
        """LZ4EncoderBase.cs:46-62"""
        src = _ro_view(source, "source")
        length = src.size - offset if length is None else int(length)
        if length == 0:
            return 0
        space = self._index + self._block_size - self._pointer
        if space <= 0:
            return 0
        chunk = min(space, length)
        self._input[self._pointer:self._pointer + chunk] = src[offset:offset + chunk]
        self._pointer += chunk
        return chunk

    def _commit(self) -> None:
        """LZ4EncoderBase.Commit -> LZ4_saveDict(ctx, buffer, pointer)"""
        self._index = self._pointer
        if self._index + self._block_size <= self._length:
            return
        d = min(65536, self._pointer, int(self._state["dictSize"][0]))
        self._input[:d] = self._input[self._pointer - d:self._pointer].copy()
        self._state["dictSize"] = d
        self._index = self._pointer = d

    def _run(self, content: np.ndarray, allowCopy: bool, ctx=None):
        if int(self._state["currentOffset"][0]) + content.size - self._index > FAST_CHAIN_LIMIT:
            raise NotImplementedError("a chained fast stream beyond 2 GB (the encoder's renormalisation) is not supported")
        out, arena, boff, _, st = encode_fast_chain_packed([content], self._block_size, self._extra, allowCopy, ctx, state_in=self._state,
                                                           want_state=True)
        return out, arena, boff, st

    def Encode(self, target, offset: int = 0, length: Optional[int] = None, allowCopy: bool = False) -> int:
        """encodes the pending bytes as one block into target; with allowCopy a block that does not shrink is stored raw and
        -length is returned (LZ4EncoderBase.cs:66-88)"""
        dst = _rw_view(target, "target")
        length = dst.size - offset if length is None else int(length)
        n = self._pointer - self._index
        if n <= 0:
            return 0
        out, arena, boff, st = self._run(self._input[:self._pointer], allowCopy)
        encoded = int(out[0])
        if encoded == 0 or abs(encoded) > length:
            raise InvalidOperationException("Failed to encode chunk. Target buffer too small.")
        dst[offset:offset + abs(encoded)] = arena[int(boff[0]):int(boff[0]) + abs(encoded)]
        self._state = st
        self._commit()
        return encoded

    def EncodeBlocks(self, sources: Sequence, allowCopy: bool = True,
                     ctx: Optional[_native.Context] = None) -> List[Tuple[EncoderAction, bytes]]:
        """the next blocks of the stream, as Topup + Encode(allowCopy) per element would produce them, in one call.  Every
        element but the last is BlockSize bytes (the encoder's blocks are what the ring buffer cuts), the last at most that;
        nothing may be pending."""
        blocks = [_ro_view(s, "source") for s in sources]
        if self.BytesReady:
            raise InvalidOperationException("bytes are pending: Encode them first")
        for i, b in enumerate(blocks):
            if b.size > self._block_size or (i < len(blocks) - 1 and b.size != self._block_size):
                raise InvalidOperationException("every block but the last must be BlockSize bytes")
        blocks = [b for b in blocks if b.size]
        if not blocks:
            return [(EncoderAction.None_, b"") for _ in sources]
        content = np.concatenate([self._input[:self._index]] + blocks)
        out, arena, boff, st = self._run(content, allowCopy, ctx)
        res = []
        for n, o in zip(out, boff):
            if n == 0:
                raise InvalidOperationException("Failed to encode chunk. Target buffer too small.")
            res.append((EncoderAction.Copied if n < 0 else EncoderAction.Encoded, arena[int(o):int(o) + abs(int(n))].tobytes()))
        # the ring buffer as the blocks one by one would have left it; the device's state is the last block's (and its save)
        for b in blocks:
            self.Topup(b)
            self._state["dictSize"] += b.size
            self._commit()
        assert int(self._state["dictSize"][0]) == int(st["dictSize"][0])
        self._state = st
        return res + [(EncoderAction.None_, b"")] * (len(sources) - len(res))


class LZ4BlockDecoder:
    """Decoder for independent blocks (LZ4BlockDecoder.cs)."""

    def __init__(self, blockSize: int = 65536):
        self._block_size = _round_block_size(blockSize)
        self._output_length = self._block_size + 8
        self._output = np.zeros(self._output_length + 8, np.uint8)
        self._output_index = 0

    @property
    def BlockSize(self) -> int:
        return self._block_size

    @property
    def BytesReady(self) -> int:
        return self._output_index

    def Decode(self, source, offset: int = 0, length: Optional[int] = None, blockSize: int = 0) -> int:
        src = _ro_view(source, "source")
        length = src.size - offset if length is None else int(length)
        if blockSize <= 0:
            blockSize = self._block_size
        if blockSize > self._block_size:
            raise InvalidOperationException()
        decoded = LZ4Codec.Decode(src, offset, length, self._output, 0, self._output_length)
        if decoded < 0:
            raise InvalidOperationException()
        self._output_index = decoded
        return decoded

    def Inject(self, source, offset: int = 0, length: Optional[int] = None) -> int:
        src = _ro_view(source, "source")
        length = src.size - offset if length is None else int(length)
        if length <= 0:
            self._output_index = 0
            return 0
        if length > self._output_length:
            raise InvalidOperationException()
        self._output[:length] = src[offset:offset + length]
        self._output_index = length
        return length

    def Drain(self, target, offset: int, length: int, targetOffset: int = 0) -> None:
        """offset is relative to the end of the decoded data (negative), LZ4BlockDecoder.cs:75-85"""
        dst = _rw_view(target, "target")
        start = self._output_index + int(offset)
        if start < 0 or length < 0 or start + length > self._output_index:
            raise InvalidOperationException()
        dst[targetOffset:targetOffset + length] = self._output[start:start + length]

    def Peek(self, offset: int) -> np.ndarray:
        start = self._output_index + int(offset)
        if start < 0 or start > self._output_index:
            raise InvalidOperationException()
        return self._output[start:self._output_index]


# ---- LZ4EncoderExtensions ---------------------------------------------------------------------------
def TopupAndEncode(encoder: Union[LZ4BlockEncoder, LZ4HighChainEncoder, LZ4FastChainEncoder], source, target, forceEncode: bool, allowCopy: bool):
    """-> (action, loaded, encoded)   (LZ4EncoderExtensions.cs:117-133, :183-205)"""
    src = _ro_view(source, "source")
    loaded = encoder.Topup(src) if src.size > 0 else 0
    action, encoded = FlushAndEncode(encoder, target, forceEncode, allowCopy, loaded)
    return action, loaded, encoded


def FlushAndEncode(encoder: Union[LZ4BlockEncoder, LZ4HighChainEncoder, LZ4FastChainEncoder], target, forceEncode: bool = True, allowCopy: bool = True, loaded: int = 0):
    """-> (action, encoded)"""
    if encoder.BytesReady < (1 if forceEncode else encoder.BlockSize):
        return (EncoderAction.Loaded if loaded > 0 else EncoderAction.None_), 0
    encoded = encoder.Encode(target, allowCopy=allowCopy)
    if not allowCopy or encoded >= 0:
        return EncoderAction.Encoded, encoded
    return EncoderAction.Copied, -encoded


def DecodeAndDrain(decoder: Union[LZ4BlockDecoder, "LZ4ChainDecoder"], source, target):
    """-> (ok, decoded): decodes one block and copies it to the start of target
    (LZ4EncoderExtensions.cs:288-305: false for an empty source, a failed decode or a target too small)"""
    src = _ro_view(source, "source")
    if src.size <= 0:
        return False, 0
    decoded = decoder.Decode(src)
    dst = _rw_view(target, "target")
    if decoded <= 0 or dst.size < decoded:
        return False, decoded
    decoder.Drain(dst, -decoded, decoded)
    return True, decoded


# ---- many open ILZ4Decoders advanced per call (k4lz4_chain_decode_batch) ---------------------------------
CDEC_RUN, CDEC_RESET = 0, 1
CDEC_DRAIN = 1
CDEC_DECODE, CDEC_INJECT, CDEC_BLOCK_SIZE, CDEC_TARGET, CDEC_NOT_RUN, CDEC_RANGE, CDEC_NO_DECODER = -1, -2, -3, -4, -5, -6, -7
CDEC_DICT_INDEX = -8
CDQ_BYTES_READY, CDQ_BLOCK_SIZE, CDQ_RECORDS, CDQ_BYTES, CDQ_CODE, CDQ_CHAINING, CDQ_EXTRA_BLOCKS, CDQ_MOVES, CDQ_WORDS = range(9)
CDEC_INJECT_BIT = 0x80000000


class ChainDecoderSettings(_C.Structure):
    """k4lz4_chain_decoder_settings"""
    _fields_ = [("blockSize", _C.c_int32), ("extraBlocks", _C.c_int32), ("chaining", _C.c_int32)]


class ChainDecoderRecord(_C.Structure):
    """k4lz4_chain_decoder"""
    _fields_ = [("blockSize", _C.c_int32), ("extraBlocks", _C.c_int32), ("chaining", _C.c_int32), ("reserved", _C.c_int32),
                ("storeBytes", _C.c_int64)]


def chain_decoder_record(chaining, blockSize: int, extraBlocks: int = 0, lib=None) -> ChainDecoderRecord:
    """k4lz4_chain_decoder_init: host arithmetic, no device"""
    lib = lib or _native.load_library()
    rec = ChainDecoderRecord()
    _native._check_plain(lib, lib.k4lz4_chain_decoder_init(_C.byref(rec), _C.byref(ChainDecoderSettings(int(blockSize), int(extraBlocks),
                                                                                                     1 if chaining else 0))))
    return rec


def chain_record_table(records):
    """per-stream lists of (inject, bytes, blockSize) -> (src, recOff, recLen, recBlockSize, firstRec, nRec), the record table of
    k4lz4_chain_decode_batch"""
    flat = [r for rs in records for r in rs]
    n_rec = np.array([len(rs) for rs in records], np.uint32)
    first = np.zeros(len(records), np.uint64)
    if len(records) > 1:
        first[1:] = np.cumsum(n_rec[:-1].astype(np.uint64))
    views = [_ro_view(r[1], "source") for r in flat]
    src, off, _ = pack_blocks(views) if views else (np.zeros(1, np.uint8), np.zeros(0, np.uint64), None)
    rec_len = np.array([v.size | (CDEC_INJECT_BIT if r[0] else 0) for v, r in zip(views, flat)], np.uint32)
    rec_bs = np.array([int(r[2]) if len(r) > 2 else 0 for r in flat], np.int32)
    return src, np.ascontiguousarray(off, np.uint64), rec_len, rec_bs, first, n_rec


class LZ4ChainDecoderBatch:
    """Many open ILZ4Decoders over host arrays (k4lz4_chain_decode_batch / k4lz4_chain_drain_batch / k4lz4_chain_decoder_query):
    settings is one (chaining, blockSize, extraBlocks) per decoder, as LZ4Decoder.Create takes them.  The stores live in device
    memory (a torch tensor); every call is synchronous."""

    def __init__(self, settings, ctx: Optional[_native.Context] = None):
        import torch
        self.ctx = ctx or _native.default_context()
        self.lib = self.ctx.lib
        self.settings = [(1 if c else 0, int(b), int(e)) for c, b, e in settings]
        self.n = len(self.settings)
        self.records = (ChainDecoderRecord * max(self.n, 1))(*[chain_decoder_record(c, b, e, self.lib) for c, b, e in self.settings])
        sizes = np.array([r.storeBytes for r in self.records[:self.n]], np.int64)
        self.store_off = np.concatenate(([0], np.cumsum(sizes[:-1]))).astype(np.uint64) if self.n else np.zeros(0, np.uint64)
        self.store = torch.empty(int(sizes.sum()) + 256, dtype=torch.uint8, device=torch.device("cuda", self.ctx.device))
        self._base = (self.store.data_ptr() + 255) // 256 * 256
        self.Reset()

    def _subset(self, which):
        idx = np.arange(self.n) if which is None else np.asarray(list(which), np.int64)
        return idx, np.ascontiguousarray(self.store_off[idx])

    def Reset(self, which=None) -> None:
        """the stores of `which` (default: all) become fresh decoders"""
        idx, off = self._subset(which)
        if idx.size == 0:
            return
        recs = (ChainDecoderRecord * idx.size)(*[self.records[int(i)] for i in idx])
        out = np.zeros(idx.size, np.int64)
        self.ctx.check(self.lib.k4lz4_chain_decode_batch(self.ctx.handle, recs, _C.c_void_p(self._base), off.ctypes.data, None, None, None, None, 0,
                                                         None, None, None, None, None, None, out.ctypes.data, idx.size, CDEC_RESET, 0))

    def open(self, dict_idx, dictionaries) -> List[int]:
        """k4lz4_chain_decoder_open_dictset: every store becomes a fresh decoder, and decoder s with dict_idx[s] = e >= 0 one after
        Inject(the bytes entry e of `dictionaries`, a DictionarySet, keeps); -1: no dictionary.  -> per decoder the bytes injected, or
        CDEC_INJECT (an independent decoder shorter than the entry)"""
        idx = np.ascontiguousarray(dict_idx, np.int32)
        if idx.size != self.n:
            raise ValueError("dict_idx must have one entry per decoder")
        out = np.zeros(max(self.n, 1), np.int64)
        self.ctx.check(self.lib.k4lz4_chain_decoder_open_dictset(self.ctx.handle, self.records, _C.c_void_p(self._base), self.store_off.ctypes.data,
                                                                 idx.ctypes.data, dictionaries.handle, out.ctypes.data, self.n))
        return out[:self.n].tolist()

    def Run(self, records, drain: bool = False, caps=None):
        """records[s]: the run of decoder s, a list of (inject, bytes, blockSize) -- Decode(source, length, blockSize), or Inject where
        the first word is true; an empty list leaves the decoder untouched.  With drain the bytes of every record are appended to a
        target of caps[s] bytes, as DecodeAndDrain does.  -> (recOut per decoder, outLen, the drained bytes per decoder)"""
        n = self.n
        assert len(records) == n
        src, roff, rlen, rbs, first, nrec = chain_record_table(records)
        nr = int(rlen.size)
        caps = np.zeros(n, np.uint64) if caps is None else np.ascontiguousarray(caps, np.uint64)
        doff = np.concatenate(([0], np.cumsum(caps[:-1]))).astype(np.uint64) if n else np.zeros(0, np.uint64)
        dst = np.zeros(max(int(caps.sum()), 1), np.uint8)
        rec_out = np.zeros(max(nr, 1), np.int32)
        out = np.zeros(max(n, 1), np.int64)
        p = lambda a: a.ctypes.data  # noqa: E731
        self.ctx.check(self.lib.k4lz4_chain_decode_batch(self.ctx.handle, None, _C.c_void_p(self._base), p(self.store_off), p(src), p(roff), p(rlen),
                                                         p(rbs), nr, p(first), p(nrec), p(dst) if drain else None, p(doff) if drain else None,
                                                         p(caps) if drain else None, p(rec_out), p(out), n, CDEC_RUN, CDEC_DRAIN if drain else 0))
        ro = [rec_out[int(f):int(f) + int(k)].tolist() for f, k in zip(first, nrec)]
        given = [sum(r[:next((j for j, g in enumerate(r) if g < 0), len(r))]) if drain else 0 for r in ro]
        return ro, out[:n].tolist(), [dst[int(doff[i]):int(doff[i]) + given[i]].tobytes() for i in range(n)]

    def Drain(self, offsets, lengths):
        """Drain(target, offset, length) per decoder: offset relative to BytesReady (<= 0).  -> per decoder the bytes, or CDEC_RANGE"""
        n = self.n
        offsets, lengths = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(lengths, np.int64)
        # a decoder holds less than its store: a longer range takes no room, the device answers it with CDEC_RANGE
        held = np.array([r.storeBytes for r in self.records[:n]], np.int64)
        caps = np.where((lengths > 0) & (lengths <= held), lengths, 0).astype(np.uint64)
        doff = np.concatenate(([0], np.cumsum(caps[:-1]))).astype(np.uint64) if n else np.zeros(0, np.uint64)
        dst = np.zeros(max(int(caps.sum()), 1), np.uint8)
        out = np.zeros(max(n, 1), np.int64)
        self.ctx.check(self.lib.k4lz4_chain_drain_batch(self.ctx.handle, _C.c_void_p(self._base), self.store_off.ctypes.data, offsets.ctypes.data,
                                                        lengths.ctypes.data, dst.ctypes.data, doff.ctypes.data, out.ctypes.data, n))
        return [int(out[i]) if out[i] < 0 else dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() for i in range(n)]

    def Query(self) -> np.ndarray:
        """(n, CDQ_WORDS) int64: BytesReady, BlockSize, records applied, bytes decoded, the last code, ..."""
        q = np.zeros(max(self.n, 1) * CDQ_WORDS, np.int64)
        self.ctx.check(self.lib.k4lz4_chain_decoder_query(self.ctx.handle, _C.c_void_p(self._base), self.store_off.ctypes.data, self.n, q.ctypes.data))
        return q[:self.n * CDQ_WORDS].reshape(self.n, CDQ_WORDS)


class LZ4ChainDecoder:
    """Decoder for dependent blocks (LZ4ChainDecoder.cs): the ILZ4Decoder of one stream, a batch of one underneath.  With
    chaining=False the same store is an LZ4BlockDecoder on the device (LZ4Decoder.Create uses the host class for that)."""

    def __init__(self, blockSize: int = 65536, extraBlocks: int = 0, ctx: Optional[_native.Context] = None, chaining: bool = True,
                 dictionary=None):
        """dictionary: (DictionarySet, index) -- the decoder starts as one that was given Inject(the entry's kept bytes)"""
        self._batch = LZ4ChainDecoderBatch([(chaining, blockSize, extraBlocks)], ctx)
        self._block_size = int(self._batch.records[0].blockSize)
        if dictionary is not None:
            code = self._batch.open([int(dictionary[1])], dictionary[0])[0]
            if code < 0:
                raise InvalidOperationException(f"code {code}")

    @property
    def BlockSize(self) -> int:
        return self._block_size

    @property
    def BytesReady(self) -> int:
        return int(self._batch.Query()[0, CDQ_BYTES_READY])

    def _one(self, inject, source, offset, length, blockSize=0) -> int:
        src = _ro_view(source, "source")
        length = src.size - offset if length is None else int(length)
        rec_out, _, _ = self._batch.Run([[(inject, src[offset:offset + max(length, 0)], blockSize)]])
        if rec_out[0][0] < 0:
            raise InvalidOperationException(f"code {rec_out[0][0]}")
        return rec_out[0][0]

    def Decode(self, source, offset: int = 0, length: Optional[int] = None, blockSize: int = 0) -> int:
        return self._one(False, source, offset, length, blockSize)

    def Inject(self, source, offset: int = 0, length: Optional[int] = None) -> int:
        return self._one(True, source, offset, length)

    def Drain(self, target, offset: int, length: int, targetOffset: int = 0) -> None:
        """offset is relative to the end of the decoded data (negative), LZ4ChainDecoder.cs:96-103"""
        dst = _rw_view(target, "target")
        got = self._batch.Drain([int(offset)], [int(length)])[0]
        if isinstance(got, int):
            raise InvalidOperationException()
        dst[targetOffset:targetOffset + length] = np.frombuffer(got, np.uint8)

    def Peek(self, offset: int) -> np.ndarray:
        """the bytes from BytesReady + offset to BytesReady (LZ4ChainDecoder.cs:106-115): a drain without a length"""
        ready, offset = self.BytesReady, int(offset)
        if ready + offset < 0 or offset > 0:
            raise InvalidOperationException()
        return np.frombuffer(self._batch.Drain([offset], [-offset])[0], np.uint8)


class LZ4Decoder:
    """Encoders/LZ4Decoder.cs"""

    @staticmethod
    def Create(chaining: bool, blockSize: int, extraBlocks: int = 0, dictionary=None):
        """dictionary: (DictionarySet, index): the decoder after one Inject of the entry's kept bytes, taken from the set on the
        device (an independent decoder then lives on the device too)"""
        if dictionary is not None:
            return LZ4ChainDecoder(blockSize, extraBlocks, getattr(dictionary[0], "ctx", None), bool(chaining), dictionary)
        return LZ4ChainDecoder(blockSize, extraBlocks) if chaining else LZ4BlockDecoder(blockSize)


# ---- many open ILZ4Encoders advanced per call (k4lz4_chain_encode_batch) ---------------------------------
CENC_RUN, CENC_RESET = 0, 1
CENC_FORCE, CENC_ALLOW_COPY = 1, 2
CENC_TARGET = -1


class ChainEncoderSettings(_C.Structure):
    """k4lz4_chain_encoder_settings"""
    _fields_ = [("chaining", _C.c_int32), ("level", _C.c_int32), ("blockSize", _C.c_int32), ("extraBlocks", _C.c_int32)]


class ChainEncoderRecord(_C.Structure):
    """k4lz4_chain_encoder"""
    _fields_ = [("kind", _C.c_int32), ("level", _C.c_int32), ("blockSize", _C.c_int32), ("extraBlocks", _C.c_int32),
                ("ringBytes", _C.c_int32), ("index", _C.c_int32), ("pointer", _C.c_int32), ("currentOffset", _C.c_uint32),
                ("dictSize", _C.c_uint32), ("reserved", _C.c_int32), ("taken", _C.c_int64), ("blocks", _C.c_int64),
                ("storeBytes", _C.c_int64)]


def chain_encoder_record(chaining, level, blockSize: int, extraBlocks: int = 0, lib=None) -> ChainEncoderRecord:
    """k4lz4_chain_encoder_init: host arithmetic, no device"""
    lib = lib or _native.load_library()
    rec = ChainEncoderRecord()
    _native._check_plain(lib, lib.k4lz4_chain_encoder_init(_C.byref(rec), _C.byref(ChainEncoderSettings(1 if chaining else 0, int(level), int(blockSize),
                                                                                                     int(extraBlocks)))))
    return rec


def encoder_record_table(records):
    """per-stream lists of (bytes, force, allowCopy) -> (src, recOff, recLen, recFlags, firstRec, nRec), the record table of
    k4lz4_chain_encode_batch"""
    flat = [r for rs in records for r in rs]
    n_rec = np.array([len(rs) for rs in records], np.uint32)
    first = np.zeros(len(records), np.uint64)
    if len(records) > 1:
        first[1:] = np.cumsum(n_rec[:-1].astype(np.uint64))
    views = [_ro_view(r[0], "source") for r in flat]
    src, off, _ = pack_blocks(views) if views else (np.zeros(1, np.uint8), np.zeros(0, np.uint64), None)
    rec_len = np.array([v.size for v in views], np.uint32)
    rec_flags = np.array([(CENC_FORCE if r[1] else 0) | (CENC_ALLOW_COPY if r[2] else 0) for r in flat], np.uint32)
    return src, np.ascontiguousarray(off, np.uint64), rec_len, rec_flags, first, n_rec


def _ring_at(rec: ChainEncoderRecord) -> int:
    """a store's layout: a chained fast stream's k4lz4_fast_chain_state (rounded to 256 bytes), then the ring"""
    return (FAST_CHAIN_STATE.itemsize + 255) // 256 * 256 if rec.kind == 2 else 0


class LZ4EncoderBatch:
    """Many open ILZ4Encoders over host arrays (k4lz4_chain_encode_batch): settings is one (chaining, level, blockSize, extraBlocks)
    per encoder, as LZ4Encoder.Create takes them.  The rings (and the fast chains' states) live in device memory (a torch tensor), the
    counters in the host records; every call is synchronous."""

    def __init__(self, settings, ctx: Optional[_native.Context] = None):
        import torch
        self.ctx = ctx or _native.default_context()
        self.lib = self.ctx.lib
        self.n = len(settings)
        self.records = (ChainEncoderRecord * max(self.n, 1))(*[chain_encoder_record(c, int(l), b, e, self.lib) for c, l, b, e in settings])
        sizes = np.array([r.storeBytes for r in self.records[:self.n]], np.int64)
        self.store_off = np.concatenate(([0], np.cumsum(sizes[:-1]))).astype(np.uint64) if self.n else np.zeros(0, np.uint64)
        self.store = torch.empty(int(sizes.sum()) + 256, dtype=torch.uint8, device=torch.device("cuda", self.ctx.device))
        self._base = (self.store.data_ptr() + 255) // 256 * 256

    def BlockSize(self, i: int = 0) -> int:
        return int(self.records[i].blockSize)

    def BytesReady(self, i: int = 0) -> int:
        return int(self.records[i].pointer - self.records[i].index)

    def Reset(self) -> None:
        """every encoder becomes a fresh one"""
        if self.n:
            self.ctx.check(self.lib.k4lz4_chain_encode_batch(self.ctx.handle, self.records, _C.c_void_p(self._base), self.store_off.ctypes.data,
                                                             None, None, None, None, 0, None, None, None, None, None, None, None, None, self.n,
                                                             CENC_RESET, 0))

    def open(self, dict_idx, dictionaries) -> None:
        """k4lz4_chain_encoder_open_dictset: every encoder becomes a fresh one, and encoder s with dict_idx[s] = e >= 0 starts with
        the bytes entry e of `dictionaries` (a DictionarySet) keeps as its prefix -- LZ4_loadDict / LZ4_loadDictHC on the ring; -1: no
        dictionary"""
        idx = np.ascontiguousarray(dict_idx, np.int32)
        if idx.size != self.n:
            raise ValueError("dict_idx must have one entry per encoder")
        self.ctx.check(self.lib.k4lz4_chain_encoder_open_dictset(self.ctx.handle, self.records, _C.c_void_p(self._base), self.store_off.ctypes.data,
                                                                 idx.ctypes.data, dictionaries.handle, self.n))

    def Bound(self, records) -> List[int]:
        out = []
        for i, rs in enumerate(records):
            _, _, rlen, rflags, _, _ = encoder_record_table([rs])
            out.append(int(self.lib.k4lz4_chain_encode_bound(_C.byref(self.records[i]), rlen.ctypes.data, rflags.ctypes.data, len(rs))))
        return out

    def Run(self, records, caps=None, flags: int = 0):
        """records[s]: the run of encoder s, a list of (bytes, forceEncode, allowCopy) -- one TopupAndEncode each (no bytes with
        forceEncode: FlushAndEncode); an empty list leaves the encoder untouched.  caps[s]: the target's room (default: the bound).
        -> (recLoaded per encoder, recOut per encoder, outLen, the bytes written per encoder)"""
        n = self.n
        assert len(records) == n
        src, roff, rlen, rflags, first, nrec = encoder_record_table(records)
        nr = int(rlen.size)
        caps = np.array(self.Bound(records), np.uint64) if caps is None else np.ascontiguousarray(caps, np.uint64)
        doff = np.concatenate(([0], np.cumsum(caps[:-1]))).astype(np.uint64) if n else np.zeros(0, np.uint64)
        dst = np.zeros(max(int(caps.sum()), 1), np.uint8)
        loaded = np.zeros(max(nr, 1), np.int32)
        rec_out = np.zeros(max(nr, 1), np.int32)
        out = np.zeros(max(n, 1), np.int64)
        p = lambda a: a.ctypes.data  # noqa: E731
        flags |= _native.FLAG_X32 if LZ4Codec.Enforce32 else 0
        self.ctx.check(self.lib.k4lz4_chain_encode_batch(self.ctx.handle, self.records, _C.c_void_p(self._base), p(self.store_off), p(src), p(roff),
                                                         p(rlen), p(rflags), nr, p(first), p(nrec), p(dst), p(doff), p(caps), p(loaded), p(rec_out),
                                                         p(out), n, CENC_RUN, flags))
        cut = lambda a: [a[int(f):int(f) + int(k)].tolist() for f, k in zip(first, nrec)]  # noqa: E731
        return cut(loaded), cut(rec_out), out[:n].tolist(), [dst[int(doff[i]):int(doff[i]) + max(int(out[i]), 0)].tobytes() for i in range(n)]

    def write_records(self, i: int, piece, force: bool = False, allowCopy: bool = True):
        """the writer's loop for one piece -- TopupAndEncode(forceEncode) until the piece is in -- as records: each offers what is left
        (up to a block) and the library's model (k4lz4_chain_encode_plan) says what Topup takes and where the record leaves the ring"""
        v = _ro_view(piece, "source")
        cur, nxt = ChainEncoderRecord.from_buffer_copy(self.records[i]), ChainEncoderRecord()
        flags = np.array([(CENC_FORCE if force else 0) | (CENC_ALLOW_COPY if allowCopy else 0)], np.uint32)
        loaded = np.zeros(1, np.int32)
        recs, pos = [], 0
        while pos < v.size:
            offer = np.array([min(v.size - pos, cur.blockSize)], np.uint32)
            _native._check_plain(self.lib, self.lib.k4lz4_chain_encode_plan(_C.byref(cur), offer.ctypes.data, flags.ctypes.data, 1, _C.byref(nxt),
                                                                           loaded.ctypes.data, None))
            take = int(loaded[0])
            recs.append((v[pos:pos + take], force, allowCopy))     # (a full block that was topped up but not encoded: no bytes, it encodes)
            pos += take
            cur, nxt = nxt, cur
        return recs

    def Write(self, pieces, force: bool = False, allowCopy: bool = True):
        """pieces[s]: bytes for encoder s (None or empty: it sits the call out) -> per encoder the blocks the call wrote, [(recOut, bytes)]"""
        records = [self.write_records(i, p, force, allowCopy) if p is not None and len(p) else [] for i, p in enumerate(pieces)]
        return self.blocks_of(*self.Run(records)[1:])

    def Flush(self, allowCopy: bool = True):
        """FlushAndEncode for every encoder"""
        return self.blocks_of(*self.Run([[(b"", True, allowCopy)] for _ in range(self.n)])[1:])

    @staticmethod
    def blocks_of(rec_out, out_len, data):
        res = []
        for ro, total, d in zip(rec_out, out_len, data):
            if total < 0:
                raise InvalidOperationException(f"code {total}")
            at, blocks = 0, []
            for o in ro:
                if o:
                    blocks.append((o, d[at:at + abs(o)]))
                    at += abs(o)
            res.append(blocks)
        return res

    def Ring(self, i: int) -> bytes:
        """the ring of encoder i as the store holds it, from 0 to _inputPointer"""
        r = self.records[i]
        at = int(self._base - self.store.data_ptr() + self.store_off[i]) + _ring_at(r)
        return self.store[at:at + int(r.pointer)].cpu().numpy().tobytes()

    def State(self, i: int) -> np.ndarray:
        """a chained fast encoder's stream context as the store holds it (FAST_CHAIN_STATE)"""
        at = int(self._base - self.store.data_ptr() + self.store_off[i])
        return np.frombuffer(self.store[at:at + FAST_CHAIN_STATE.itemsize].cpu().numpy().tobytes(), FAST_CHAIN_STATE).copy()


class LZ4ChainEncoder:
    """The ILZ4Encoder of one stream over a batch of one (k4lz4_chain_encode_batch): what LZ4Encoder.Create returns.  Topup keeps its
    bytes on the host until the Encode that takes them -- one record, Topup and a forced Encode -- so the two work as separate calls."""

    def __init__(self, chaining: bool, level: LZ4Level, blockSize: int, extraBlocks: int = 0, ctx: Optional[_native.Context] = None,
                 dictionary=None):
        """dictionary: (DictionarySet, index) -- the stream starts with the entry's kept bytes as its prefix"""
        self._batch = LZ4EncoderBatch([(chaining, level, blockSize, extraBlocks)], ctx or getattr(dictionary and dictionary[0], "ctx", None))
        self._pending: List[np.ndarray] = []
        if dictionary is not None:
            self._batch.open([int(dictionary[1])], dictionary[0])

    @property
    def BlockSize(self) -> int:
        return self._batch.BlockSize(0)

    @property
    def BytesReady(self) -> int:
        return self._batch.BytesReady(0) + sum(p.size for p in self._pending)

    def Topup(self, source, offset: int = 0, length: Optional[int] = None) -> int:
        """LZ4EncoderBase.cs:46-62"""
        src = _ro_view(source, "source")
        length = src.size - offset if length is None else int(length)
        if length == 0:
            return 0
        space = self.BlockSize - self.BytesReady
        if space <= 0:
            return 0
        chunk = min(space, length)
        self._pending.append(src[offset:offset + chunk].copy())
        return chunk

    def Encode(self, target, offset: int = 0, length: Optional[int] = None, allowCopy: bool = False) -> int:
        """LZ4EncoderBase.cs:66-88: the pending bytes as one block into target; negative: stored raw under allowCopy.  A target below
        the library's bound for the block (its length under allowCopy, MaximumOutputSize otherwise) is refused before anything runs
        (K4LZ4_CENC_TARGET): the exception is the reference's, and the encoder keeps the block for a retry with a larger target"""
        dst = _rw_view(target, "target")
        length = dst.size - offset if length is None else int(length)
        if self.BytesReady <= 0:
            return 0
        piece = np.concatenate(self._pending) if self._pending else np.zeros(0, np.uint8)
        run = [[(piece, True, allowCopy)]]
        cap = min(max(length, 0), self._batch.Bound(run)[0])
        _, rec_out, out_len, data = self._batch.Run(run, caps=[cap])
        if out_len[0] < 0:
            raise InvalidOperationException("Failed to encode chunk. Target buffer too small.")
        self._pending = []
        encoded = rec_out[0][0]
        dst[offset:offset + abs(encoded)] = np.frombuffer(data[0], np.uint8)
        return encoded


class LZ4Encoder:
    """Encoders/LZ4Encoder.cs"""

    @staticmethod
    def Create(chaining: bool, level: LZ4Level, blockSize: int, extraBlocks: int = 0, ctx: Optional[_native.Context] = None,
               dictionary=None) -> LZ4ChainEncoder:
        return LZ4ChainEncoder(chaining, level, blockSize, extraBlocks, ctx, dictionary)
