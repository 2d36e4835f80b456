"""lz4net's legacy formats (K4os.Compression.LZ4.Legacy), backed by libk4lz4.so.

Mirrors:
  LZ4Legacy.Wrap / WrapHC / Unwrap      LZ4Wrapper.cs:50-145   [u32 U][u32 C][block], or [u32 U][u32 U][bytes]
  LZ4Legacy.Encode / Decode             LZ4Stream.cs           chunks `varint(flags) varint(U) [varint(C)] payload`,
                                                               written whole and disposed / read to the end
What runs where: the encoders write every block straight into its place (wraps) or into an arena (streams); the stream's
record sizes, their scan and the assembly, the reader's walk over the varints and every check of AcquireNextChunk, the
batch decode of the compressed chunks / payloads and the raw copies all run in the HIP kernels (k4lz4_legacy.hpp).

LZ4Legacy's batches are whole buffers.  LZ4Stream's incremental Write / Flush / Dispose and Read (interactive reads too) over
many open streams are LZ4StreamWriterBatch / LegacyWriterDevice and LZ4StreamReaderBatch / LegacyReaderDevice below
(k4lz4_legacy_stream.hpp).  Chunks with passes are refused as the reference refuses them
(NotSupportedException).
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
    """not the reference's: a caller's target is too small (K4LZ4_LEGACY_CAPACITY), or a chunk is larger than the reader's
    maxBlockSize (K4LZ4_LEGACY_BLOCK_SIZE)"""


class ObjectDisposedException(Exception):
    """System.ObjectDisposedException (a call on a stream that was closed)"""


# per-item codes (include/k4lz4.h K4LZ4_LEGACY_*)
LEGACY_END_OF_STREAM, LEGACY_OVERFLOW, LEGACY_NOT_SUPPORTED, LEGACY_INVALID_DATA = -1, -2, -3, -4
LEGACY_ARGUMENT, LEGACY_CAPACITY, LEGACY_NOT_ENCODED = -5, -6, -7
LEGACY_BLOCK_SIZE, LEGACY_CLOSED = -8, -9


def legacy_exception(code: int) -> Exception:
    """the exception the reference throws for a K4LZ4_LEGACY_* code"""
    return {LEGACY_END_OF_STREAM: lambda: EndOfStreamException("Unexpected end of stream"),
            LEGACY_OVERFLOW: lambda: OverflowException("Arithmetic operation resulted in an overflow."),
            LEGACY_NOT_SUPPORTED: lambda: NotSupportedException("Chunks with multiple passes are not supported."),
            LEGACY_INVALID_DATA: lambda: InvalidDataException("Compressed data corrupted"),
            LEGACY_ARGUMENT: lambda: ArgumentException("inputBuffer size is invalid or has been corrupted"),
            LEGACY_CAPACITY: lambda: CapacityError("the target is too small"),
            LEGACY_NOT_ENCODED: lambda: MemoryError("HC scratch reserved with k4lz4_ctx_reserve_hc was too small"),
            LEGACY_BLOCK_SIZE: lambda: CapacityError("a chunk is larger than the reader's maxBlockSize"),
            LEGACY_CLOSED: lambda: ObjectDisposedException("the stream is closed"),
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


# ---- LZ4Stream piece by piece: many open streams, one Write / Flush / Dispose or one Read each per call (k4lz4_legacy_write_batch*,
# k4lz4_legacy_read_batch*) -----------------------------------------------------------------------------------
LWRITE_WRITE, LWRITE_FLUSH, LWRITE_CLOSE = 0, 1, 2
LREAD_READ, LREAD_RESET = 0, 1
LREAD_INTERACTIVE = 1
LREADER_FED = 1
LSQ_POSITION, LSQ_BYTES_READ, LSQ_PENDING, LSQ_CODE, LSQ_CHUNKS, LSQ_DIRECT, LSQ_BATCHED, LSQ_HANDED_BACK, LSQ_WORDS = 0, 1, 2, 3, 4, 5, 6, 7, 8


class LegacyWriterRecord(C.Structure):        # k4lz4_legacy_writer: settings and the pending count, host memory
    _fields_ = [("blockSize", C.c_int32), ("high", C.c_int32), ("pending", C.c_int32), ("closed", C.c_int32)]


class LegacyReaderRecord(C.Structure):        # k4lz4_legacy_reader
    _fields_ = [("maxBlockSize", C.c_int32), ("flags", C.c_int32), ("storeBytes", C.c_int64)]


def _per_stream(value, n):
    lst = list(value) if isinstance(value, (list, tuple, np.ndarray)) else [value] * n
    if len(lst) != n:
        raise ValueError("one value, or one per stream")
    return lst


def _legacy_writer_records(n: int, highCompression, blockSize, lib):
    recs = (LegacyWriterRecord * max(n, 1))()
    store_off = np.zeros(n, np.uint64)
    at = 0
    for i, (h, b) in enumerate(zip(_per_stream(highCompression, n), _per_stream(blockSize, n))):
        if lib.k4lz4_legacy_writer_init(C.byref(recs[i]), int(b), int(bool(h))) != 0:
            raise ArgumentException(f"blockSize {b} is too large")
        store_off[i] = at
        at += (int(lib.k4lz4_legacy_writer_store_bytes(C.byref(recs[i]))) + 255) // 256 * 256
    return recs, store_off, at


class LZ4StreamWriterBatch:
    """n LZ4Streams in Compress mode (LZ4Stream.cs) advanced together: Write(chunks) is one Write per stream, Flush() one Flush,
    Close() one Dispose (with chunks: the bytes are written first); each returns, per stream, the bytes the reference's stream
    pushes to its inner stream during that call (None where a chunk is None).  The reference flushes lazily: a buffer that a Write
    fills exactly goes out with the next byte, or at Flush / Dispose.  The pending bytes live in device memory; the data goes up
    and the bytes come back in one host-pointer call (k4lz4_legacy_write_batch).  A stream the call refuses reports None and its
    K4LZ4_LEGACY_* code in LastCodes.  highCompression, blockSize: one value, or one per stream."""

    def __init__(self, n: int, highCompression=False, blockSize=1 << 20, ctx: Optional[_native.Context] = None):
        import torch
        self.ctx = ctx or _native.default_context()
        self.n = int(n)
        self.records, self.store_off, size = _legacy_writer_records(self.n, highCompression, blockSize, self.ctx.lib)
        dev = int(self.ctx.lib.k4lz4_ctx_device(self.ctx.handle))
        self.store = torch.empty(max(size, 1) + 64, dtype=torch.uint8, device=f"cuda:{dev}")
        self.LastCodes = np.zeros(self.n, np.int64)

    def Bound(self, stream: int, length: int, op: int = LWRITE_WRITE) -> int:
        return int(self.ctx.lib.k4lz4_legacy_write_bound(C.byref(self.records[stream]), int(length), int(op)))

    def _call(self, chunks, op: int, dst_cap=None) -> List[Optional[bytes]]:
        if len(chunks) != self.n:
            raise ValueError("one chunk (or None) per stream")
        views = [None if c is None else _ro_view(c, "buffer") for c in chunks]
        lens = np.array([-1 if v is None else v.size for v in views], np.int64)
        src, soff, _ = pack_blocks([v if v is not None else np.zeros(0, np.uint8) for v in views])
        caps = np.array([self.Bound(i, int(lens[i]), op) for i in range(self.n)], np.uint64) if dst_cap is None else \
            np.ascontiguousarray(dst_cap, np.uint64)
        doff = np.zeros(self.n, np.uint64)
        if self.n > 1:
            doff[1:] = np.cumsum(caps[:-1])
        dst = np.zeros(max(int(caps.sum()), 1), np.uint8)
        out = np.zeros(max(self.n, 1), np.int64)
        self.ctx.check(self.ctx.lib.k4lz4_legacy_write_batch(self.ctx.handle, self.records, self.store.data_ptr(), self.store_off.ctypes.data,
                                                             src.ctypes.data, soff.ctypes.data, lens.ctypes.data, dst.ctypes.data,
                                                             doff.ctypes.data, caps.ctypes.data, out.ctypes.data, self.n, op, 0))
        out = out[:self.n]
        self.LastCodes = np.minimum(out, 0)
        return [None if (lens[i] < 0 or out[i] < 0) else dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() for i in range(self.n)]

    def Write(self, chunks, dst_cap=None) -> List[Optional[bytes]]:
        return self._call(chunks, LWRITE_WRITE, dst_cap)

    def Flush(self, streams=None) -> List[Optional[bytes]]:
        return self._call([b"" if streams is None or i in streams else None for i in range(self.n)], LWRITE_FLUSH)

    def Close(self, chunks=None, streams=None) -> List[Optional[bytes]]:
        if chunks is None:
            chunks = [b"" if streams is None or i in streams else None for i in range(self.n)]
        return self._call(chunks, LWRITE_CLOSE)


class LegacyWriterDevice:
    """n LZ4Streams in Compress mode over HBM-resident data (k4lz4_legacy_write_batch_device): write(data, off, length) takes stream
    s's bytes from data[off[s] : off[s] + length[s]] (data a uint8 torch tensor, off / length host arrays, length < 0: untouched)
    and returns (out, out_off, out_len): stream s's bytes of this call are out[out_off[s] : out_off[s] + out_len[s]], out_off a host
    array, out_len an int64 device tensor (negative: a K4LZ4_LEGACY_* code).  Asynchronous on the current torch stream, nothing is
    read back; `dc` is a device.DeviceCodec."""

    def __init__(self, dc, n: int, highCompression=False, blockSize=1 << 20):
        import torch
        self.dc = dc
        self.n = int(n)
        self.records, self.store_off, size = _legacy_writer_records(self.n, highCompression, blockSize, dc.lib)
        self.store = torch.empty(max(size, 1) + 64, dtype=torch.uint8, device=dc.device)

    def bound(self, length, op: int = LWRITE_WRITE) -> np.ndarray:
        length = np.broadcast_to(np.asarray(length, np.int64), (self.n,))
        return np.array([self.dc.lib.k4lz4_legacy_write_bound(C.byref(self.records[i]), int(length[i]), int(op)) for i in range(self.n)],
                        np.uint64)

    def _call(self, data, off, length, op: int, dst_cap=None, out=None):
        import torch
        from .device import _dp
        length = np.ascontiguousarray(np.broadcast_to(np.asarray(length, np.int64), (self.n,)))
        off = np.ascontiguousarray(np.broadcast_to(np.asarray(off, np.int64), (self.n,))).astype(np.uint64)
        caps = self.bound(length, op) if dst_cap is None else np.ascontiguousarray(dst_cap, np.uint64)
        if out is None:
            out_off = np.zeros(self.n, np.uint64)
            if self.n > 1:
                out_off[1:] = np.cumsum((caps[:-1] + 15) // 16 * 16)
            buf = torch.empty(int(((caps + 15) // 16 * 16).sum()) + 64, dtype=torch.uint8, device=self.dc.device)
        else:
            buf, out_off = out
            out_off = np.ascontiguousarray(out_off, np.uint64)
        out_len = torch.zeros(max(self.n, 1), dtype=torch.int64, device=self.dc.device)
        if self.n:
            self.dc.ctx.check(self.dc.lib.k4lz4_legacy_write_batch_device(
                self.dc.ctx.handle, self.records, _dp(self.store), self.store_off.ctypes.data, _dp(data), off.ctypes.data, length.ctypes.data,
                _dp(buf), out_off.ctypes.data, caps.ctypes.data, _dp(out_len), self.n, op, 0, C.c_void_p(self.dc._stream())))
        return buf, out_off.astype(np.int64), out_len[:self.n]

    def write(self, data, off, length, dst_cap=None, out=None):
        return self._call(data, off, length, LWRITE_WRITE, dst_cap, out)

    def flush(self, streams=None):
        return self._call(None, 0, [0 if streams is None or i in streams else -1 for i in range(self.n)], LWRITE_FLUSH)

    def close(self, data=None, off=0, length=None, dst_cap=None, out=None):
        """Dispose; with data, the bytes are written first (Write then Dispose in one call)"""
        return self._call(data, off, 0 if length is None else length, LWRITE_CLOSE, dst_cap, out)


def legacy_reader_record(max_block_size: int, lib, fed: bool = False) -> LegacyReaderRecord:
    """fed: a record for the _fed calls (k4lz4_legacy_reader_init_fed: the store has a stash behind it)"""
    rec = LegacyReaderRecord()
    if (lib.k4lz4_legacy_reader_init_fed if fed else lib.k4lz4_legacy_reader_init)(C.byref(rec), int(max_block_size)) != 0:
        raise ArgumentException(f"maxBlockSize {max_block_size} is too large")
    return rec


class LZ4StreamReaderBatch:
    """n LZ4Streams in Decompress mode advanced together over sources held in host memory: Read(counts) is one Read(count) per
    stream and returns, per stream, the bytes it delivers (b"" at the end of the source, None where the count is None or negative);
    interactive=True is LZ4StreamFlags.InteractiveRead (the read returns after the first copy); ReadByte is a read of 1.  The
    readers' state lives in device memory; every call sends the sources up and brings the bytes back (k4lz4_legacy_read_batch).
    A stream that fails raises the reference's exception (the lowest-index one) when raise_errors, else reports None and its
    K4LZ4_LEGACY_* code in LastCodes; it stays failed.  maxBlockSize: the largest chunk a stream may hold."""

    def __init__(self, sources, maxBlockSize: int = 1 << 20, ctx: Optional[_native.Context] = None, raise_errors: bool = True):
        import torch
        self.ctx = ctx or _native.default_context()
        self.views = [_ro_view(s, "stream") for s in sources]
        self.n = len(self.views)
        self.raise_errors = raise_errors
        self.record = legacy_reader_record(maxBlockSize, self.ctx.lib)
        self.store_off = (np.arange(self.n, dtype=np.uint64) * np.uint64(self.record.storeBytes)).astype(np.uint64)
        dev = int(self.ctx.lib.k4lz4_ctx_device(self.ctx.handle))
        self.store = torch.empty(max(self.n, 1) * int(self.record.storeBytes) + 64, dtype=torch.uint8, device=f"cuda:{dev}")
        self.src, soff, _ = pack_blocks(self.views) if self.n else (np.zeros(16, np.uint8), np.zeros(0, np.uint64), None)
        self.src_off = np.ascontiguousarray(soff, np.uint64)
        self.src_len = np.array([v.size for v in self.views], np.uint64)
        self.LastCodes = np.zeros(self.n, np.int64)
        self._call(LREAD_RESET, np.zeros(self.n, np.int64), False)

    def _call(self, op: int, counts: np.ndarray, interactive: bool):
        caps = np.maximum(counts, 0).astype(np.uint64) if op == LREAD_READ else np.zeros(self.n, np.uint64)
        doff = np.zeros(self.n, np.uint64)
        if self.n > 1:
            doff[1:] = np.cumsum(caps[:-1])
        dst = np.zeros(max(int(caps.sum()), 1), np.uint8)
        out = np.zeros(max(self.n, 1), np.int64)
        self.ctx.check(self.ctx.lib.k4lz4_legacy_read_batch(
            self.ctx.handle, C.byref(self.record), self.store.data_ptr(), self.store_off.ctypes.data, self.src.ctypes.data,
            self.src_off.ctypes.data, self.src_len.ctypes.data, dst.ctypes.data, doff.ctypes.data, counts.ctypes.data, out.ctypes.data,
            self.n, op, LREAD_INTERACTIVE if interactive else 0))
        out = out[:self.n]
        self.LastCodes = np.where(counts >= 0, np.minimum(out, 0), 0)
        if self.raise_errors:
            _first_error(self.LastCodes)
        return out, dst, doff

    def Read(self, counts, interactive: bool = False) -> List[Optional[bytes]]:
        if len(counts) != self.n:
            raise ValueError("one count (or None) per stream")
        counts = np.array([-1 if c is None else int(c) for c in counts], np.int64)
        out, dst, doff = self._call(LREAD_READ, counts, interactive)
        return [None if (counts[i] < 0 or out[i] < 0) else dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() for i in range(self.n)]

    def ReadByte(self, streams=None) -> List[Optional[int]]:
        """-1 at the end of the stream, None where the stream sits the call out or fails"""
        got = self.Read([1 if streams is None or i in streams else None for i in range(self.n)])
        return [None if g is None else (g[0] if g else -1) for g in got]

    def Query(self) -> np.ndarray:
        """(n, LSQ_WORDS) int64: source position, bytes delivered, bytes pending, code, chunks, made in dst, batched, handed back"""
        q = np.zeros(max(self.n, 1) * LSQ_WORDS, np.int64)
        self.ctx.check(self.ctx.lib.k4lz4_legacy_reader_query(self.ctx.handle, self.store.data_ptr(), self.store_off.ctypes.data, self.n,
                                                              q.ctypes.data))
        return q[:self.n * LSQ_WORDS].reshape(self.n, LSQ_WORDS)


class LegacyReaderDevice:
    """n LZ4Streams in Decompress mode over HBM-resident sources (k4lz4_legacy_read_batch_device): stream s is
    data[off[s] : off[s] + length[s]] (data a uint8 torch tensor; off / length host arrays or device tensors).  read(counts)
    delivers up to counts[s] bytes per stream (host array or device tensor; negative: the stream sits the call out) and returns
    (out, out_off, out_len): stream s's bytes of this call are out[out_off[s] : out_off[s] + out_len[s]], out_len an int64 device
    tensor (negative: a K4LZ4_LEGACY_* code).  With out=(buffer, out_off) the bytes go to buffer[out_off[s] : out_off[s] + counts[s]],
    and with device tensors throughout the call touches no host memory.  Asynchronous on the current torch stream, no
    synchronisation; `dc` is a device.DeviceCodec."""

    def __init__(self, dc, data, off, length, maxBlockSize: int = 1 << 20):
        import torch
        self.dc = dc
        self.data = data
        self.off, self.length = _dev_i64(off, dc.device), _dev_i64(length, dc.device)
        self.n = int(self.off.numel())
        self.record = legacy_reader_record(maxBlockSize, dc.lib)
        so = np.arange(self.n, dtype=np.int64) * int(self.record.storeBytes)
        self.store_off = torch.from_numpy(so).to(dc.device)
        self.store = torch.empty(max(self.n, 1) * int(self.record.storeBytes) + 64, dtype=torch.uint8, device=dc.device)
        self._zero = torch.zeros(max(self.n, 1), dtype=torch.int64, device=dc.device)
        self._call(LREAD_RESET, self._zero, None, None, False)

    def _call(self, op, counts, buf, out_off, interactive, max_count=0):
        import torch
        from .device import _dp
        out_len = torch.zeros(max(self.n, 1), dtype=torch.int64, device=self.dc.device)
        if self.n:
            self.dc.ctx.check(self.dc.lib.k4lz4_legacy_read_batch_device(
                self.dc.ctx.handle, C.byref(self.record), _dp(self.store), _dp(self.store_off), _dp(self.data), _dp(self.off),
                _dp(self.length), _dp(buf), _dp(out_off), _dp(counts), _dp(out_len), self.n, op, LREAD_INTERACTIVE if interactive else 0,
                int(max_count), C.c_void_p(self.dc._stream())))
        return out_len[:self.n]

    def read(self, counts, out=None, interactive: bool = False, max_count: Optional[int] = None):
        """max_count: an upper bound of the counts (it sizes the direct path's chunk table); None: taken from host counts, and for
        device counts 0, which leaves every stream to the general kernel"""
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
        return buf, out_off, self._call(LREAD_READ, counts_d, buf, off_d, interactive, max_count or 0)

    def query(self):
        """(n, LSQ_WORDS) int64 device tensor, see LZ4StreamReaderBatch.Query"""
        import torch
        from .device import _dp
        q = torch.zeros(max(self.n, 1) * LSQ_WORDS, dtype=torch.int64, device=self.dc.device)
        if self.n:
            self.dc.ctx.check(self.dc.lib.k4lz4_legacy_reader_query_device(self.dc.ctx.handle, _dp(self.store), _dp(self.store_off), self.n,
                                                                           _dp(q), C.c_void_p(self.dc._stream())))
        return q[:self.n * LSQ_WORDS].reshape(self.n, LSQ_WORDS)


# ---- the incremental LZ4Stream reader fed its source in pieces (k4lz4_legacy_read_fed_batch*) ---------------
class LZ4StreamFedReaderBatch:
    """n LZ4Streams in Decompress mode whose sources arrive in pieces (sockets, pipes, files read as they grow).  Feed(pieces,
    final) hands stream s its next bytes (appended behind what it has not consumed yet; final[s]: nothing follows); Read(counts)
    is one k4lz4_legacy_read_fed_batch over what is held and returns (bytes, consumed, need) per stream: the bytes delivered (None
    where the count is None or negative, or the stream failed), the source bytes the call consumed, and need > 0 where the read is
    starved -- it wants that many further bytes before it can go on; issue it again with the count reduced by what it delivered
    once they are fed.  The bytes, total and code of such a sequence are those of one LZ4Stream.Read(count) over the whole source.
    Only the pieces travel to the device; the readers' state and stash live there.  Errors as LZ4StreamReaderBatch."""

    def __init__(self, n: int, maxBlockSize: int = 1 << 20, ctx: Optional[_native.Context] = None, raise_errors: bool = True):
        import torch
        self.ctx = ctx or _native.default_context()
        self.n = int(n)
        self.raise_errors = raise_errors
        self.record = legacy_reader_record(maxBlockSize, self.ctx.lib, fed=True)
        self.store_off = (np.arange(self.n, dtype=np.uint64) * np.uint64(self.record.storeBytes)).astype(np.uint64)
        dev = int(self.ctx.lib.k4lz4_ctx_device(self.ctx.handle))
        self.store = torch.empty(max(self.n, 1) * int(self.record.storeBytes) + 64, dtype=torch.uint8, device=f"cuda:{dev}")
        self.held = [bytearray() for _ in range(self.n)]
        self.final = np.zeros(self.n, np.int64)
        self.LastCodes = np.zeros(self.n, np.int64)
        self._call(LREAD_RESET, np.zeros(self.n, np.int64), False)

    def Feed(self, pieces, final=None) -> None:
        if len(pieces) != self.n:
            raise ValueError("one piece (or None) per stream")
        for i, p in enumerate(pieces):
            if p is not None and len(p):
                if self.final[i]:
                    raise ArgumentException(f"stream {i} was fed its final piece already")
                self.held[i] += bytes(p)
        if final is not None:
            self.final |= np.asarray([1 if f else 0 for f in final], np.int64)

    def _call(self, op: int, counts: np.ndarray, interactive: bool):
        n = self.n
        lens = np.array([len(h) for h in self.held], np.uint64)
        soff = np.zeros(n, np.uint64)
        if n > 1:
            soff[1:] = np.cumsum(lens[:-1])
        src = np.frombuffer(b"".join(bytes(h) for h in self.held) + bytes(16), np.uint8)
        caps = np.maximum(counts, 0).astype(np.uint64) if op == LREAD_READ else np.zeros(n, np.uint64)
        doff = np.zeros(n, np.uint64)
        if n > 1:
            doff[1:] = np.cumsum(caps[:-1])
        dst = np.zeros(max(int(caps.sum()), 1), np.uint8)
        out, consumed, need = (np.zeros(max(n, 1), np.int64) for _ in range(3))
        self.ctx.check(self.ctx.lib.k4lz4_legacy_read_fed_batch(
            self.ctx.handle, C.byref(self.record), self.store.data_ptr(), self.store_off.ctypes.data, src.ctypes.data, soff.ctypes.data,
            lens.ctypes.data, self.final.ctypes.data, dst.ctypes.data, doff.ctypes.data, counts.ctypes.data, out.ctypes.data,
            consumed.ctypes.data, need.ctypes.data, n, op, LREAD_INTERACTIVE if interactive else 0))
        out, consumed, need = out[:n], consumed[:n], need[:n]
        for i in range(n):
            if out[i] >= 0 and consumed[i] > 0:
                del self.held[i][:int(consumed[i])]
        self.LastCodes = np.where(counts >= 0, np.minimum(out, 0), 0)
        if self.raise_errors:
            _first_error(self.LastCodes)
        return out, dst, doff, consumed, need

    def Read(self, counts, interactive: bool = False):
        """-> ([bytes or None], consumed, need)"""
        if len(counts) != self.n:
            raise ValueError("one count (or None) per stream")
        counts = np.array([-1 if c is None else int(c) for c in counts], np.int64)
        out, dst, doff, consumed, need = self._call(LREAD_READ, counts, interactive)
        got = [None if (counts[i] < 0 or out[i] < 0) else dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() for i in range(self.n)]
        return got, consumed, need

    def Query(self) -> np.ndarray:
        """(n, LSQ_WORDS) int64, see LZ4StreamReaderBatch.Query; the position is the sum of consumed"""
        q = np.zeros(max(self.n, 1) * LSQ_WORDS, np.int64)
        self.ctx.check(self.ctx.lib.k4lz4_legacy_reader_query(self.ctx.handle, self.store.data_ptr(), self.store_off.ctypes.data, self.n,
                                                              q.ctypes.data))
        return q[:self.n * LSQ_WORDS].reshape(self.n, LSQ_WORDS)


class LegacyFedReaderDevice:
    """n LZ4Streams in Decompress mode fed HBM-resident pieces (k4lz4_legacy_read_fed_batch_device).  read(data, off, length, final,
    counts) takes stream s's unconsumed source from data[off[s] : off[s] + length[s]] (data a uint8 torch tensor; off / length /
    final / counts host arrays or device tensors; final may be None) and returns (out, out_off, out_len, consumed, need): stream s's
    bytes of this call are out[out_off[s] : out_off[s] + out_len[s]]; out_len (negative: a K4LZ4_LEGACY_* code), consumed and need
    are int64 device tensors.  With out=(buffer, out_off) and device tensors throughout the call touches no host memory.
    Asynchronous on the current torch stream, no synchronisation; `dc` is a device.DeviceCodec."""

    def __init__(self, dc, n: int, maxBlockSize: int = 1 << 20):
        import torch
        self.dc = dc
        self.n = int(n)
        self.record = legacy_reader_record(maxBlockSize, dc.lib, fed=True)
        so = np.arange(self.n, dtype=np.int64) * int(self.record.storeBytes)
        self.store_off = torch.from_numpy(so).to(dc.device)
        self.store = torch.empty(max(self.n, 1) * int(self.record.storeBytes) + 64, dtype=torch.uint8, device=dc.device)
        self._zero = torch.zeros(max(self.n, 1), dtype=torch.int64, device=dc.device)
        self._call(LREAD_RESET, None, self._zero, self._zero, None, self._zero, None, None, False, 0)

    def _call(self, op, data, off, length, final, counts, buf, out_off, interactive, max_count):
        import torch
        from .device import _dp
        out_len, consumed, need = (torch.zeros(max(self.n, 1), dtype=torch.int64, device=self.dc.device) for _ in range(3))
        if self.n:
            self.dc.ctx.check(self.dc.lib.k4lz4_legacy_read_fed_batch_device(
                self.dc.ctx.handle, C.byref(self.record), _dp(self.store), _dp(self.store_off), _dp(data), _dp(off), _dp(length),
                _dp(final), _dp(buf), _dp(out_off), _dp(counts), _dp(out_len), _dp(consumed), _dp(need), self.n, op,
                LREAD_INTERACTIVE if interactive else 0, int(max_count), C.c_void_p(self.dc._stream())))
        return out_len[:self.n], consumed[:self.n], need[:self.n]

    def read(self, data, off, length, final, counts, out=None, interactive: bool = False, max_count: Optional[int] = None):
        """max_count: an upper bound of the counts (it sizes the direct path's chunk table); None: taken from host counts, and for
        device counts 0, which leaves every stream to the general reader"""
        import torch
        dev = self.dc.device
        if max_count is None and not isinstance(counts, torch.Tensor):
            max_count = int(np.max(np.asarray(counts, np.int64), initial=0))
        off_d, len_d = _dev_i64(off, dev), _dev_i64(length, dev)
        fin_d = None if final is None else _dev_i64(final, dev)
        if out is None:
            c = np.ascontiguousarray(np.broadcast_to(np.asarray(counts.cpu().numpy() if isinstance(counts, torch.Tensor) else counts,
                                                                np.int64), (self.n,)))
            caps = (np.maximum(c, 0) + 15) // 16 * 16
            out_off = np.zeros(self.n, np.int64)
            if self.n > 1:
                out_off[1:] = np.cumsum(caps[:-1])
            buf = torch.empty(int(caps.sum()) + 64, dtype=torch.uint8, device=dev)
            counts_d, oo_d = _dev_i64(c, dev), _dev_i64(out_off, dev)
        else:
            buf, out_off = out
            counts_d, oo_d = _dev_i64(counts, dev), _dev_i64(out_off, dev)
        res = self._call(LREAD_READ, data, off_d, len_d, fin_d, counts_d, buf, oo_d, interactive, max_count or 0)
        return (buf, out_off) + res

    def query(self):
        """(n, LSQ_WORDS) int64 device tensor, see LZ4StreamReaderBatch.Query"""
        import torch
        from .device import _dp
        q = torch.zeros(max(self.n, 1) * LSQ_WORDS, dtype=torch.int64, device=self.dc.device)
        if self.n:
            self.dc.ctx.check(self.dc.lib.k4lz4_legacy_reader_query_device(self.dc.ctx.handle, _dp(self.store), _dp(self.store_off), self.n,
                                                                           _dp(q), C.c_void_p(self.dc._stream())))
        return q[:self.n * LSQ_WORDS].reshape(self.n, LSQ_WORDS)
