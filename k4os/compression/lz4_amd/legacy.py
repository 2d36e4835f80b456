"""lz4net's legacy formats (K4os.Compression.LZ4.Legacy), backed by libk4lz4.so.

Mirrors:
  LZ4Legacy.Wrap / WrapHC / Unwrap      LZ4Wrapper.cs:50-145   [u32 U][u32 C][block], or [u32 U][u32 U][bytes]
  LZ4Legacy.Encode / Decode             LZ4Stream.cs           chunks `varint(flags) varint(U) [varint(C)] payload`,
                                                               written whole and disposed / read to the end
What runs where: the encoders write every block straight into its place (wraps) or into an arena (streams); the stream's
record sizes, their scan and the assembly, the reader's walk over the varints and every check of AcquireNextChunk, the
batch decode of the compressed chunks / payloads and the raw copies all run in the HIP kernels (k4lz4_legacy.hpp).

Batches are whole buffers: LZ4Stream's interactive reads and incremental Read / Write are not offered.  Chunks with
passes are refused as the reference refuses them (NotSupportedException).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .codec import _ro_view, pack_blocks
from .frames import InvalidDataException, _dev_i64

INT_MAX = 0x7FFFFFFF


class EndOfStreamException(EOFError):
    """System.IO.EndOfStreamException (a truncated chunk, a compressed length larger than the original)"""


class OverflowException(ArithmeticError):
    """System.OverflowException (a negative length reaches new byte[])"""


class NotSupportedException(Exception):
    """System.NotSupportedException (chunks with multiple passes)"""


class ArgumentException(ValueError):
    """System.ArgumentException (Wrap / Unwrap arguments, a wrapped buffer whose sizes do not fit it)"""


class CapacityError(ValueError):
    """not the reference's: a caller's target is too small (K4LZ4_LEGACY_CAPACITY)"""


# per-item codes (include/k4lz4.h K4LZ4_LEGACY_*)
LEGACY_END_OF_STREAM, LEGACY_OVERFLOW, LEGACY_NOT_SUPPORTED, LEGACY_INVALID_DATA = -1, -2, -3, -4
LEGACY_ARGUMENT, LEGACY_CAPACITY, LEGACY_NOT_ENCODED = -5, -6, -7


def legacy_exception(code: int) -> Exception:
    """the exception the reference throws for a K4LZ4_LEGACY_* code"""
    return {LEGACY_END_OF_STREAM: lambda: EndOfStreamException("Unexpected end of stream"),
            LEGACY_OVERFLOW: lambda: OverflowException("Arithmetic operation resulted in an overflow."),
            LEGACY_NOT_SUPPORTED: lambda: NotSupportedException("Chunks with multiple passes are not supported."),
            LEGACY_INVALID_DATA: lambda: InvalidDataException("Compressed data corrupted"),
            LEGACY_ARGUMENT: lambda: ArgumentException("inputBuffer size is invalid or has been corrupted"),
            LEGACY_CAPACITY: lambda: CapacityError("the target is too small"),
            LEGACY_NOT_ENCODED: lambda: MemoryError("HC scratch reserved with k4lz4_ctx_reserve_hc was too small"),
            }.get(int(code), lambda: RuntimeError(f"unknown legacy result {int(code)}"))()


def _first_error(codes):
    bad = np.flatnonzero(np.asarray(codes) < 0)
    if bad.size:
        raise legacy_exception(int(np.asarray(codes)[bad[0]]))


class LZ4Legacy:
    """LZ4Legacy (LZ4Legacy.cs): Wrap / WrapHC / Unwrap and the legacy stream, with batch forms."""

    # ---- LZ4Wrapper ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _slice(inputBuffer, inputOffset: int, inputLength: int) -> np.ndarray:
        src = _ro_view(inputBuffer, "inputBuffer")
        inputLength = min(src.size - int(inputOffset), int(inputLength))          # LZ4Wrapper.cs:53
        if inputLength < 0 or inputOffset < 0:
            raise ArgumentException("inputBuffer size of inputLength is invalid")
        return src[int(inputOffset):int(inputOffset) + inputLength]

    @staticmethod
    def Wrap(inputBuffer, inputOffset: int = 0, inputLength: int = INT_MAX) -> bytes:
        return LZ4Legacy.WrapBatch([LZ4Legacy._slice(inputBuffer, inputOffset, inputLength)])[0]

    @staticmethod
    def WrapHC(inputBuffer, inputOffset: int = 0, inputLength: int = INT_MAX) -> bytes:
        return LZ4Legacy.WrapBatch([LZ4Legacy._slice(inputBuffer, inputOffset, inputLength)], high=True)[0]

    @staticmethod
    def WrapBatch(sources: Sequence, high: bool = False, ctx: Optional[_native.Context] = None) -> List[bytes]:
        """Wrap (high: WrapHC) of every source, in one k4lz4_wrap_batch call (LZ4Codec.Enforce32 applies)"""
        ctx = ctx or _native.default_context()
        blocks = [_ro_view(s, "inputBuffer") for s in sources]
        if not blocks:
            return []
        src, soff, slen = pack_blocks(blocks)
        caps = np.array([ctx.lib.k4lz4_wrap_bound(b.size) for b in blocks], dtype=np.int32)
        doff = np.zeros(len(blocks), np.uint64)
        if len(blocks) > 1:
            doff[1:] = np.cumsum(caps[:-1].astype(np.uint64))
        dst = np.empty(int(caps.astype(np.int64).sum()) + 1, np.uint8)
        out = np.empty(len(blocks), dtype=np.int32)
        ctx.check(ctx.lib.k4lz4_wrap_batch(ctx.handle, src.ctypes.data, soff.ctypes.data, slen.ctypes.data, dst.ctypes.data,
                                           doff.ctypes.data, caps.ctypes.data, out.ctypes.data, len(blocks), 1 if high else 0, 0))
        if (out < 0).any():
            raise _native.NativeLibraryError("wrap kernel reported a slot too small (internal error)")
        return [dst[int(o):int(o) + int(n)].tobytes() for n, o in zip(out, doff)]

    @staticmethod
    def UnwrappedSize(inputBuffer, inputOffset: int = 0) -> int:
        """the length Unwrap returns, or the exception it throws (host arithmetic, k4lz4_unwrap_size)"""
        src = _ro_view(inputBuffer, "inputBuffer")
        if inputOffset < 0 or inputOffset > src.size:
            raise ArgumentException("inputBuffer size is invalid")
        rest = src[int(inputOffset):]
        r = _native.load_library().k4lz4_unwrap_size(rest.ctypes.data if rest.size else None, rest.size)
        if r < 0:
            raise legacy_exception(r)
        return r

    @staticmethod
    def Unwrap(inputBuffer, inputOffset: int = 0) -> bytes:
        src = _ro_view(inputBuffer, "inputBuffer")
        if inputOffset < 0 or inputOffset > src.size:
            raise ArgumentException("inputBuffer size is invalid")
        out, _ = LZ4Legacy.UnwrapBatch([src[int(inputOffset):]])
        return out[0]

    @staticmethod
    def UnwrapBatch(buffers: Sequence, ctx: Optional[_native.Context] = None) -> Tuple[List[bytes], np.ndarray]:
        """Unwrap of every buffer -> (results, decode_ok).  decode_ok[i] is False where LZ4Codec.Decode did not return the
        wrapped length (a corrupt payload): Unwrap ignores that and returns outLen bytes all the same, and so does this.
        Raises what Unwrap throws for the lowest-index buffer that fails."""
        ctx = ctx or _native.default_context()
        bufs = [_ro_view(b, "inputBuffer") for b in buffers]
        if not bufs:
            return [], np.zeros(0, bool)
        sizes = np.array([ctx.lib.k4lz4_unwrap_size(b.ctypes.data if b.size else None, b.size) for b in bufs], np.int64)
        _first_error(sizes)
        src, soff, slen = pack_blocks(bufs)
        caps = sizes.astype(np.int32)
        doff = np.zeros(len(bufs), np.uint64)
        if len(bufs) > 1:
            doff[1:] = np.cumsum(caps[:-1].astype(np.uint64))
        dst = np.empty(int(sizes.sum()) + 1, np.uint8)
        out = np.empty(len(bufs), np.int32)
        dec = np.empty(len(bufs), np.int32)
        ctx.check(ctx.lib.k4lz4_unwrap_batch(ctx.handle, src.ctypes.data, soff.ctypes.data, slen.ctypes.data, dst.ctypes.data,
                                             doff.ctypes.data, caps.ctypes.data, out.ctypes.data, dec.ctypes.data, len(bufs)))
        _first_error(out)
        return [dst[int(o):int(o) + int(n)].tobytes() for n, o in zip(out, doff)], dec == out

    # ---- LZ4Stream -----------------------------------------------------------------------------------------------------
    @staticmethod
    def Encode(content, highCompression: bool = False, blockSize: int = 1 << 20) -> bytes:
        return LZ4Legacy.EncodeBatch([content], highCompression, blockSize)[0]

    @staticmethod
    def EncodeBatch(contents: Sequence, highCompression: bool = False, blockSize: int = 1 << 20,
                    ctx: Optional[_native.Context] = None) -> List[bytes]:
        """what LZ4Legacy.Encode(stream, highCompression, blockSize) writes for each content written whole, then disposed"""
        ctx = ctx or _native.default_context()
        blocks = [_ro_view(s, "buffer") for s in contents]
        if not blocks:
            return []
        src, soff, _ = pack_blocks(blocks)
        slen = np.array([b.size for b in blocks], np.uint64)
        caps = np.array([ctx.lib.k4lz4_legacy_stream_bound(b.size, int(blockSize)) for b in blocks], np.uint64)
        doff = np.zeros(len(blocks), np.uint64)
        if len(blocks) > 1:
            doff[1:] = np.cumsum(caps[:-1])
        dst = np.empty(int(caps.sum()) + 1, np.uint8)
        out = np.empty(len(blocks), np.int64)
        ctx.check(ctx.lib.k4lz4_encode_legacy_streams(ctx.handle, src.ctypes.data, soff.ctypes.data, slen.ctypes.data, len(blocks),
                                                      int(blockSize), 1 if highCompression else 0, 0, dst.ctypes.data, doff.ctypes.data,
                                                      caps.ctypes.data, out.ctypes.data))
        _first_error(out)
        return [dst[int(o):int(o) + int(n)].tobytes() for n, o in zip(out, doff)]

    @staticmethod
    def Decode(stream) -> bytes:
        return LZ4Legacy.DecodeBatch([stream])[0]

    @staticmethod
    def DecodeBatch(streams: Sequence, ctx: Optional[_native.Context] = None) -> List[bytes]:
        """what reading LZ4Legacy.Decode(stream) to its end returns for each stream; raises what the reader throws for the
        lowest-index stream that fails"""
        ctx = ctx or _native.default_context()
        bufs = [_ro_view(s, "stream") for s in streams]
        if not bufs:
            return []
        src, soff, _ = pack_blocks(bufs)
        slen = np.array([b.size for b in bufs], np.uint64)
        n = len(bufs)
        size = np.empty(n, np.uint64)
        status = np.empty(n, np.int32)
        ctx.check(ctx.lib.k4lz4_legacy_stream_sizes(ctx.handle, src.ctypes.data, soff.ctypes.data, slen.ctypes.data, n,
                                                    size.ctypes.data, status.ctypes.data))
        doff = np.zeros(n, np.uint64)
        if n > 1:
            doff[1:] = np.cumsum(size[:-1])
        dst = np.empty(int(size.sum()) + 1, np.uint8)
        out = np.empty(n, np.int64)
        ctx.check(ctx.lib.k4lz4_decode_legacy_streams(ctx.handle, src.ctypes.data, soff.ctypes.data, slen.ctypes.data, n,
                                                      dst.ctypes.data, doff.ctypes.data, size.ctypes.data, out.ctypes.data))
        _first_error(out)
        return [dst[int(o):int(o) + int(k)].tobytes() for k, o in zip(out, doff)]


# ---- device-resident forms (torch tensors on the context's device; asynchronous on the current torch stream unless noted) ----
def _slots(dev, caps: np.ndarray):
    import torch
    caps = np.asarray(caps, np.int64).clip(min=0)
    off = np.zeros(len(caps), np.int64)
    if len(caps) > 1:
        off[1:] = np.cumsum((caps + 15) // 16 * 16)[:-1]
    return torch.empty(int(((caps + 15) // 16 * 16).sum()) + 64, dtype=torch.uint8, device=dev), off


def _dev_i32(x, dev):
    import torch
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int32))).to(dev)


def wrap_device(dc, data, off, length, high: bool = False, out=None, flags: int = 0):
    """k4lz4_wrap_batch_device: message i = data[off[i] : off[i]+length[i]] (int32 lengths).  out: None, or (buffer, out_off,
    out_cap) with out_cap[i] >= 8 + length[i].  Returns (buffer, out_off, out_len): wrapped i = buffer[out_off[i] : +out_len[i]]."""
    import torch
    from .device import _dp
    dev = dc.device
    off_d, len_d = _dev_i64(off, dev), _dev_i32(length, dev)
    n = off_d.numel()
    if out is None:
        lens = len_d.cpu().numpy().astype(np.int64)
        buf, o = _slots(dev, lens + 8)
        off_o, cap_o = torch.from_numpy(o).to(dev), torch.from_numpy((lens + 8).astype(np.int32)).to(dev)
        out_off = o
    else:
        buf, out_off, out_cap = out
        off_o, cap_o = _dev_i64(out_off, dev), _dev_i32(out_cap, dev)
    out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    if n:
        dc.ctx.check(dc.lib.k4lz4_wrap_batch_device(dc.ctx.handle, _dp(data), _dp(off_d), _dp(len_d), _dp(buf), _dp(off_o), _dp(cap_o),
                                                    _dp(out_len), n, 1 if high else 0, flags, C.c_void_p(dc._stream())))
    return buf, out_off, out_len


def unwrap_device(dc, data, off, length, out=None):
    """k4lz4_unwrap_batch_device: buffer i = data[off[i] : off[i]+length[i]].  Without `out` the targets are sized by
    k4lz4_unwrap_sizes_device (one synchronisation).  Returns (buffer, out_off, out_len, decoded): out_len[i] = Unwrap's length or
    a K4LZ4_LEGACY_* code, decoded[i] = what LZ4Codec.Decode returned (== out_len[i]: the bytes are the payload's)."""
    import torch
    from .device import _dp
    dev = dc.device
    off_d, len_d = _dev_i64(off, dev), _dev_i32(length, dev)
    n = off_d.numel()
    if out is None:
        sizes = torch.zeros(n, dtype=torch.int32, device=dev)
        if n:
            dc.ctx.check(dc.lib.k4lz4_unwrap_sizes_device(dc.ctx.handle, _dp(data), _dp(off_d), _dp(len_d), _dp(sizes), n,
                                                          C.c_void_p(dc._stream())))
        caps = sizes.cpu().numpy().astype(np.int64).clip(min=0)
        buf, out_off = _slots(dev, caps)
        off_o, cap_o = torch.from_numpy(out_off).to(dev), torch.from_numpy(caps.astype(np.int32)).to(dev)
    else:
        buf, out_off, out_cap = out
        off_o, cap_o = _dev_i64(out_off, dev), _dev_i32(out_cap, dev)
    out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    decoded = torch.zeros(n, dtype=torch.int32, device=dev)
    if n:
        dc.ctx.check(dc.lib.k4lz4_unwrap_batch_device(dc.ctx.handle, _dp(data), _dp(off_d), _dp(len_d), _dp(buf), _dp(off_o), _dp(cap_o),
                                                      _dp(out_len), _dp(decoded), n, C.c_void_p(dc._stream())))
    return buf, out_off, out_len, decoded


def encode_legacy_streams_device(dc, data, off, length, high: bool = False, block_size: int = 1 << 20, out=None, flags: int = 0):
    """k4lz4_encode_legacy_streams_device: content i = data[off[i] : off[i]+length[i]].  out: None (slots of
    k4lz4_legacy_stream_bound), or (buffer, out_off, out_cap).  Returns (buffer, out_off, out_len), out_len an int64 device tensor.
    The call waits for the stream once (the chunk count)."""
    import torch
    from .device import _dp
    dev = dc.device
    off_d, len_d = _dev_i64(off, dev), _dev_i64(length, dev)
    n = off_d.numel()
    if out is None:
        lens = len_d.cpu().numpy()
        caps = np.array([dc.lib.k4lz4_legacy_stream_bound(int(x), int(block_size)) for x in lens], np.int64)
        buf, out_off = _slots(dev, caps)
        off_o, cap_o = torch.from_numpy(out_off).to(dev), torch.from_numpy(caps).to(dev)
    else:
        buf, out_off, out_cap = out
        off_o, cap_o = _dev_i64(out_off, dev), _dev_i64(out_cap, dev)
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    if n:
        dc.ctx.check(dc.lib.k4lz4_encode_legacy_streams_device(dc.ctx.handle, _dp(data), _dp(off_d), _dp(len_d), n, int(block_size),
                                                               1 if high else 0, flags, _dp(buf), _dp(off_o), _dp(cap_o), _dp(out_len),
                                                               C.c_void_p(dc._stream())))
    return buf, out_off, out_len


def legacy_stream_sizes_device(dc, streams, off, length):
    """k4lz4_legacy_stream_sizes_device -> (size int64, status int32) device tensors: the bytes of the chunks before the first
    structural defect (U of a compressed chunk trusted up to 255 * C + 32), and 0 or that defect's K4LZ4_LEGACY_* code"""
    import torch
    from .device import _dp
    dev = dc.device
    off_d, len_d = _dev_i64(off, dev), _dev_i64(length, dev)
    n = off_d.numel()
    size = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    if n:
        dc.ctx.check(dc.lib.k4lz4_legacy_stream_sizes_device(dc.ctx.handle, _dp(streams), _dp(off_d), _dp(len_d), n, _dp(size),
                                                             _dp(status), C.c_void_p(dc._stream())))
    return size, status


def decode_legacy_streams_device(dc, streams, off, length, out=None, raise_errors: bool = True):
    """LZ4Legacy.DecodeBatch on HBM-resident streams: stream i = streams[off[i] : off[i]+length[i]].  out: None (sized by
    legacy_stream_sizes_device, one synchronisation), or (buffer, out_off, out_cap).  Returns (buffer, out_off, out_len), out_len an
    int64 device tensor holding the content's length or a K4LZ4_LEGACY_* code.  The call waits for the stream once (the chunk
    count).  raise_errors: raise what the reader throws for the lowest-index failing stream."""
    import torch
    from .device import _dp
    dev = dc.device
    off_d, len_d = _dev_i64(off, dev), _dev_i64(length, dev)
    n = off_d.numel()
    if out is None:
        size, _ = legacy_stream_sizes_device(dc, streams, off_d, len_d)
        caps = size.cpu().numpy() if n else np.zeros(0, np.int64)
        buf, out_off = _slots(dev, caps)
        off_o, cap_o = torch.from_numpy(out_off).to(dev), size
    else:
        buf, out_off, out_cap = out
        off_o, cap_o = _dev_i64(out_off, dev), _dev_i64(out_cap, dev)
    out_len = torch.zeros(n, dtype=torch.int64, device=dev)
    if n:
        dc.ctx.check(dc.lib.k4lz4_decode_legacy_streams_device(dc.ctx.handle, _dp(streams), _dp(off_d), _dp(len_d), n, _dp(buf),
                                                               _dp(off_o), _dp(cap_o), _dp(out_len), C.c_void_p(dc._stream())))
    if raise_errors and n:
        _first_error(out_len.cpu().numpy())
    return buf, out_off, out_len
