"""The witness for the incremental frame reader: a transcription of LZ4FrameReader's read path, one object per stream --
ReadManyBytes (Frames/LZ4FrameReader.async.cs:150-172), EnsureHeader / ReadHeader (:46-108), ReadBlock (:110-137), Drain,
VerifyBlockChecksum, the content checksum (Frames/LZ4FrameReader.cs:98-134), TryReadBlock's EndOfStream rule
(Internal/ReaderExtensions.cs:10-28) -- over transcriptions of LZ4BlockDecoder (Encoders/LZ4BlockDecoder.cs) and LZ4ChainDecoder
(Encoders/LZ4ChainDecoder.cs, with its ring buffer and LZ4_streamDecode_t as LL64.LZ4_decompress_safe_continue keeps it,
Engine/x64/LL64.dec.cs:558-608).  Blocks are decoded by the reference's own engine compiled here (oracle/_ref/libk4ref.so:
k4ref_decompress_safe, k4ref_decompress_safe_using_dict with the prefix really in front of the target, so that the engine takes
its prefix modes); where that library is absent, by the C oracle's same two entry points.  XXH32 is the xxhash module's.

A read answers with bytes, or with the K4LZ4_FRAME_* code of the exception the reference throws; after a code the stream is
failed and every later call answers with the same code (the library's rule; the reference's caller would stop).  One deliberate
difference: a stored block length above the frame's block size overruns the reference's pooled block buffer in a way that depends
on the pool; it is a block defect (-6) here.  max_block_size: a frame whose block size is above it is -11 (the library's own
code).  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import struct

import xxhash

K1, K64 = 1024, 65536
MAGIC = 0x184D2204
EOF, BAD_MAGIC, VERSION, HEADER_SUM, DICTIONARY, BLOCK, BLOCK_SUM, CONTENT_SUM, BLOCK_SIZE = -1, -2, -3, -4, -5, -6, -7, -8, -11
_u8p = C.POINTER(C.c_uint8)


class Defect(Exception):
    def __init__(self, code):
        self.code = code


class Engine:
    """LLxx.LZ4_decompress_safe / LZ4_decompress_safe_usingDict on raw addresses"""

    def __init__(self):
        from oracle_lib import RefEngine, Oracle
        try:
            lib = RefEngine().lib
            self.safe, self.using_dict, self.name = lib.k4ref_decompress_safe, lib.k4ref_decompress_safe_using_dict, "k4ref"
        except (FileNotFoundError, OSError):
            lib = Oracle().lib
            self.safe, self.using_dict, self.name = lib.k4o_decompress_safe, lib.k4o_decompress_safe_using_dict, "oracle"

    @staticmethod
    def _p(addr):
        return C.cast(C.c_void_p(addr), _u8p)

    def decompress_safe(self, src: bytes, dst_addr: int, cap: int) -> int:
        s = (C.c_uint8 * max(len(src), 1)).from_buffer_copy(src or b"\0")
        return self.safe(s, self._p(dst_addr), len(src), cap)

    def decompress_using_dict(self, src: bytes, dst_addr: int, cap: int, dict_addr: int, dict_size: int) -> int:
        s = (C.c_uint8 * max(len(src), 1)).from_buffer_copy(src or b"\0")
        return self.using_dict(s, self._p(dst_addr), len(src), cap, self._p(dict_addr), dict_size)


_engine = None


def engine() -> Engine:
    global _engine
    if _engine is None:
        _engine = Engine()
    return _engine


def _round_up(v, m):
    return (v + m - 1) // m * m


class BlockDecoder:
    """Encoders/LZ4BlockDecoder.cs"""

    def __init__(self, block_size: int):
        self.block_size = _round_up(max(block_size, K1), K1)             # :25
        self.output_length = self.block_size + 8                          # :27
        self.output_index = 0
        self.buf = (C.c_uint8 * (self.output_length + 8))()               # :29
        self.base = C.addressof(self.buf)

    def decode(self, src: bytes) -> int:                                  # :39-55 (blockSize = 0 -> _blockSize)
        # LZ4Codec.Decode (LZ4Codec.cs:104-115): empty source 0, engine result <= 0 is -1
        decoded = 0 if len(src) <= 0 else engine().decompress_safe(src, self.base, self.output_length)
        if len(src) > 0 and decoded <= 0:
            decoded = -1
        if decoded < 0:
            raise Defect(BLOCK)                                           # :50-51 InvalidOperationException
        self.output_index = decoded
        return decoded

    def inject(self, src: bytes) -> int:                                  # :58-71
        if len(src) <= 0:
            self.output_index = 0
            return 0
        if len(src) > self.output_length:
            raise Defect(BLOCK)
        C.memmove(self.base, src, len(src))
        self.output_index = len(src)
        return len(src)

    def peek(self, offset: int, length: int) -> bytes:                    # Drain / Peek: offset is negative
        at = self.output_index + offset
        assert at >= 0 and length >= 0 and at + length <= self.output_index
        return C.string_at(self.base + at, length)


class ChainDecoder:
    """Encoders/LZ4ChainDecoder.cs over LZ4_streamDecode_t (prefixSize, prefixEnd, extDictSize)"""

    def __init__(self, block_size: int, extra_blocks: int = 0):
        self.block_size = _round_up(max(block_size, K1), K1)              # :28
        self.output_length = K64 + (1 + max(extra_blocks, 0)) * self.block_size + 32   # :32
        self.output_index = 0
        self.buf = (C.c_uint8 * (self.output_length + 8))()               # :35
        self.base = C.addressof(self.buf)
        self.prefix_size, self.prefix_end, self.ext_dict_size = 0, 0, 0   # the context, zeroed by PinnedMemory.Alloc

    def _set_stream_decode(self, dict_addr: int, dict_size: int):         # LL.tools.cs LZ4_setStreamDecode
        self.prefix_size, self.prefix_end, self.ext_dict_size = dict_size, dict_addr + dict_size, 0

    def _continue(self, src: bytes, dest: int, cap: int) -> int:          # LL64.dec.cs:558-608
        e = engine()
        if self.prefix_size == 0:
            result = e.decompress_safe(src, dest, cap)
            if result <= 0:
                return result
            self.prefix_size, self.prefix_end = result, dest + result
        elif self.prefix_end == dest:
            if self.prefix_size >= K64 - 1 or self.ext_dict_size == 0:
                # withPrefix64k / withSmallPrefix: what LZ4_decompress_safe_usingDict picks for a dictionary that ends at dest
                # (LL64.dec.cs:530-541), told min(prefixSize, 64 KiB) -- at 64 KiB - 1 and above the mode ignores the size
                size = min(self.prefix_size, K64)
                result = e.decompress_using_dict(src, dest, cap, dest - size, size)
            else:
                raise NotImplementedError("LZ4_decompress_safe_doubleDict: LZ4ChainDecoder never gets there")
            if result <= 0:
                return result
            self.prefix_size += result
            self.prefix_end += result
        else:
            raise NotImplementedError("external dictionary: LZ4ChainDecoder always decodes at the prefix's end")
        return result

    def _copy_dict(self, index: int) -> int:                              # :125-132
        start = max(index - K64, 0)
        size = index - start
        C.memmove(self.base, self.base + start, size)
        self._set_stream_decode(self.base, size)
        return size

    def _apply_dict(self, index: int) -> int:                             # :134-140
        start = max(index - K64, 0)
        self._set_stream_decode(self.base + start, index - start)
        return index

    def decode(self, src: bytes) -> int:                                  # :45-61
        block_size = self.block_size
        if self.output_index + block_size > self.output_length:           # Prepare :117-123
            self.output_index = self._copy_dict(self.output_index)
        decoded = self._continue(src, self.base + self.output_index, block_size)
        if decoded < 0:
            raise Defect(BLOCK)
        self.output_index += decoded
        return decoded

    def inject(self, src: bytes) -> int:                                  # :64-93
        length = len(src)
        if length <= 0:
            return 0
        if length > max(self.block_size, K64):
            raise Defect(BLOCK)
        if self.output_index + length < self.output_length:
            C.memmove(self.base + self.output_index, src, length)
            self.output_index = self._apply_dict(self.output_index + length)
        elif length >= K64:
            C.memmove(self.base, src, length)
            self.output_index = self._apply_dict(length)
        else:
            tail = min(K64 - length, self.output_index)
            C.memmove(self.base, self.base + self.output_index - tail, tail)
            C.memmove(self.base + tail, src, length)
            self.output_index = self._apply_dict(tail + length)
        return length

    peek = BlockDecoder.peek


class WitnessReader:
    """one LZ4FrameReader over a source that is all there (the ReadOnlyMemory adapter's case)"""

    def __init__(self, source: bytes, max_block_size: int = 4 << 20):
        self.src = bytes(source)
        self.pos = 0
        self.max_block_size = max_block_size
        self.decoder = None
        self.descriptor = None              # (contentLength | None, contentChecksum, chaining, blockChecksum, blockSize)
        self.decoded = 0
        self.bytes_read = 0
        self.checksum = None
        self.failed = None

    # ---- the inner stream: TryReadBlock (ReaderExtensions.cs:10-28)
    def _take(self, n: int, optional: bool = False):
        left = len(self.src) - self.pos
        if left < n:
            if left == 0 and optional:
                return None
            self.pos = len(self.src)
            raise Defect(EOF)
        b = self.src[self.pos:self.pos + n]
        self.pos += n
        return b

    def _read_header(self) -> bool:                                       # .async.cs:50-108
        m = self._take(4, optional=True)
        if m is None:
            return False
        if struct.unpack("<I", m)[0] != MAGIC:
            raise Defect(BAD_MAGIC)
        head = self._take(2)
        flg, bd = head[0], head[1]
        if (flg >> 6) & 0x11 != 1:                                        # :69-72, as written
            raise Defect(VERSION)
        chaining, bsum = ((flg >> 5) & 1) == 0, ((flg >> 4) & 1) != 0
        has_size, csum, has_dict = ((flg >> 3) & 1) != 0, ((flg >> 2) & 1) != 0, (flg & 1) != 0
        clen = None
        if has_size:
            w = self._take(8); head += w
            clen = struct.unpack("<Q", w)[0]
        if has_dict:
            head += self._take(4)
        actual = (xxhash.xxh32(head, seed=0).intdigest() >> 8) & 0xFF     # _stash.Digest(headerOffset) >> 8
        if self._take(1)[0] != actual:
            raise Defect(HEADER_SUM)
        block_size = {7: 4 << 20, 6: 1 << 20, 5: 256 << 10, 4: 64 << 10}.get((bd >> 4) & 7, 64 << 10)
        if has_dict:
            raise Defect(DICTIONARY)
        if block_size > self.max_block_size:
            raise Defect(BLOCK_SIZE)                                      # the library's own refusal, where the decoder is created
        if csum:
            self.checksum = xxhash.xxh32(seed=0)                          # InitializeContentChecksum
        self.descriptor = (clen, csum, chaining, bsum, block_size)
        self.decoder = ChainDecoder(block_size, 0) if chaining else BlockDecoder(block_size)   # LZ4Decoder.Create
        self.decoded = 0
        return True

    def _ensure_header(self) -> bool:
        return self.decoder is not None or self._read_header()

    def _read_block(self) -> int:                                         # .async.cs:110-137
        clen, csum, chaining, bsum, block_size = self.descriptor
        lc = struct.unpack("<I", self._take(4))[0]
        if lc == 0:
            if csum:
                expected = struct.unpack("<I", self._take(4))[0]
                if expected != self.checksum.intdigest():
                    raise Defect(CONTENT_SUM)
            self.decoder = self.descriptor = None                         # CloseFrame
            return 0
        uncompressed = (lc & 0x80000000) != 0
        n = lc & 0x7FFFFFFF
        if n > block_size:
            raise Defect(BLOCK)                                           # the deliberate difference above
        payload = self._take(n)
        if bsum:
            if struct.unpack("<I", self._take(4))[0] != xxhash.xxh32(payload, seed=0).intdigest():
                raise Defect(BLOCK_SUM)
        read = self.decoder.inject(payload) if uncompressed else self.decoder.decode(payload)
        if csum:
            self.checksum.update(self.decoder.peek(-read, read))          # UpdateContentChecksum: the whole block, now
        return read

    def _guard(self, fn):
        if self.failed is not None:
            return self.failed
        try:
            return fn()
        except Defect as d:
            self.failed = d.code
            return d.code

    def open(self):
        """OpenFrame(): 1, 0 or a code"""
        return self._guard(lambda: 1 if self._ensure_header() else 0)

    def read(self, count: int, interactive: bool = False):
        """ReadManyBytes: bytes, or a code"""
        def run():
            if not self._ensure_header():
                return b""
            out = bytearray()
            left = count
            while left > 0:
                if self.decoded <= 0:
                    self.decoded = self._read_block()
                    if self.decoded == 0:
                        break
                n = min(left, self.decoded)                                # Drain
                out += self.decoder.peek(-self.decoded, n)
                self.bytes_read += n
                self.decoded -= n
                left -= n
                if interactive:
                    break
            return bytes(out)
        return self._guard(run)

    @property
    def frame_length(self):
        """the open frame's ContentLength, None when no frame is open or it declares none"""
        return self.descriptor[0] if self.descriptor is not None else None

    @property
    def phase(self):
        return 2 if self.failed is not None else 1 if self.decoder is not None else 0
