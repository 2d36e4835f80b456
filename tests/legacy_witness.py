"""A line-by-line transcription of K4os.Compression.LZ4.Legacy's LZ4Wrapper (Wrap / Unwrap) and LZ4Stream (the writer with
Write / Flush / Dispose, the reader's AcquireNextChunk / TryReadVarInt with its exception order), run over the reference's own
block engine compiled into oracle/_ref (oracle_lib.RefEngine).  The checker of the legacy tests: it never touches libk4lz4.

LZ4Codec.Encode / Decode (LZ4Codec.cs) are transcribed too: Encode returns -1 for a failed encode (<= 0), Decode returns 0 for
an empty source without decoding and -1 for a result <= 0."""
from __future__ import annotations

import struct
from typing import List, Optional, Tuple

import numpy as np

from oracle_lib import RefEngine

# the exceptions, by the names the reference throws (compared by code with include/k4lz4.h K4LZ4_LEGACY_*)
END_OF_STREAM, OVERFLOW, NOT_SUPPORTED, INVALID_DATA, ARGUMENT = -1, -2, -3, -4, -5


class Thrown(Exception):
    def __init__(self, code: int):
        super().__init__(code)
        self.code = code


def _i32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


class Witness:
    def __init__(self, ref: Optional[RefEngine] = None, x32: bool = False):
        self.ref = ref or RefEngine()
        self.x32 = x32                       # LZ4Codec.Enforce32

    # ---- LZ4Codec.Encode(source, target of targetLength, level) / Decode ----------------------------------------------
    def encode(self, src: np.ndarray, cap: int, high: bool) -> Tuple[int, bytes]:
        if src.size <= 0:
            return 0, b""
        if high:
            r, d = (self.ref.compress_hc_x32 if self.x32 else self.ref.compress_hc)(src, 9, cap)
        else:
            r, d = (self.ref.compress_fast_x32 if self.x32 else self.ref.compress_fast)(src, cap)
        return (-1 if r <= 0 else r), d[:max(r, 0)].tobytes()

    def decode(self, src: bytes, cap: int) -> Tuple[int, bytes]:
        if len(src) <= 0:
            return 0, b""
        r, d = self.ref.decompress_safe(np.frombuffer(src, np.uint8), cap, fill=0, x32=self.x32)
        return (-1 if r <= 0 else r), d.tobytes()

    # ---- LZ4Wrapper.cs ------------------------------------------------------------------------------------------------------
    def wrap(self, buf: bytes, high: bool = False, offset: int = 0, length: int = 0x7FFFFFFF) -> bytes:
        length = min(len(buf) - offset, length)
        if length < 0:
            raise Thrown(ARGUMENT)
        if length == 0:
            return bytes(8)
        src = np.frombuffer(bytes(buf[offset:offset + length]), np.uint8)
        out_len, out = self.encode(src, length, high)
        if out_len >= length or out_len <= 0:
            return struct.pack("<II", length, length) + src.tobytes()
        return struct.pack("<II", length, out_len) + out[:out_len]

    def unwrap(self, buf: bytes, offset: int = 0) -> Tuple[bytes, bool]:
        """-> (result, LZ4Codec.Decode returned outputLength); the reference ignores the second"""
        input_length = len(buf) - offset
        if input_length < 8:
            raise Thrown(ARGUMENT)
        output_length = _i32(struct.unpack_from("<I", buf, offset)[0])
        input_length = _i32(struct.unpack_from("<I", buf, offset + 4)[0])
        if input_length > len(buf) - offset - 8:
            raise Thrown(ARGUMENT)
        if input_length >= output_length:
            if input_length < 0:
                raise Thrown(OVERFLOW)                               # new byte[inputLength]
            return bytes(buf[offset + 8:offset + 8 + input_length]), True
        if output_length < 0:
            raise Thrown(OVERFLOW)                                   # new byte[outputLength]
        if input_length < 0:
            raise Thrown(ARGUMENT)                                   # Validate
        r, d = self.decode(bytes(buf[offset + 8:offset + 8 + input_length]), output_length)
        result = bytearray(output_length)
        if r > 0:
            result[:r] = d[:r]
        return bytes(result), r == output_length

    # ---- LZ4Stream.cs: the writer ---------------------------------------------------------------------------------------
    class Writer:
        def __init__(self, w: "Witness", high: bool = False, block_size: int = 1 << 20):
            self.w, self.high = w, high
            self.block_size = max(16, block_size)
            self.buffer: Optional[bytearray] = None
            self.offset = 0
            self.length = 0
            self.out = bytearray()

        def _varint(self, value: int):
            while True:
                b = value & 0x7F
                value >>= 7
                self.out.append(b | (0 if value == 0 else 0x80))
                if value == 0:
                    break

        def _flush_chunk(self):
            if self.offset <= 0:
                return
            n = self.offset
            src = np.frombuffer(bytes(self.buffer[:n]), np.uint8)
            clen, comp = self.w.encode(src, n, self.high)
            if clen <= 0 or clen >= n:
                comp, clen = bytes(self.buffer[:n]), n
            is_compressed = clen < n
            flags = (1 if is_compressed else 0) | (2 if self.high else 0)
            self._varint(flags)
            self._varint(n)
            if is_compressed:
                self._varint(clen)
            self.out += comp[:clen]
            self.offset = 0

        def write(self, data: bytes):
            if self.buffer is None:
                self.buffer = bytearray(self.block_size)
                self.length = self.block_size
                self.offset = 0
            pos, count = 0, len(data)
            while count > 0:
                chunk = min(count, self.length - self.offset)
                if chunk > 0:
                    self.buffer[self.offset:self.offset + chunk] = data[pos:pos + chunk]
                    pos += chunk
                    count -= chunk
                    self.offset += chunk
                else:
                    self._flush_chunk()

        def flush(self):
            if self.offset > 0:
                self._flush_chunk()

        def dispose(self) -> bytes:
            self.flush()
            return bytes(self.out)

    def encode_stream(self, content: bytes, high: bool = False, block_size: int = 1 << 20, pieces: Optional[List[int]] = None,
                      flush_after: bool = False) -> bytes:
        """content written whole (or in `pieces`, with a Flush after each when flush_after), then disposed"""
        wr = Witness.Writer(self, high, block_size)
        if pieces is None:
            wr.write(content)
        else:
            pos = 0
            for p in pieces:
                wr.write(content[pos:pos + p])
                pos += p
                if flush_after:
                    wr.flush()
            wr.write(content[pos:])
        return wr.dispose()

    # ---- LZ4Stream.cs: the reader -------------------------------------------------------------------------------------
    def read_chunks(self, stream: bytes):
        """-> (chunks, code): chunks = [(flags, U, C, payload_offset)] of the chunks AcquireNextChunk accepted that produce
        bytes, code = 0 or the exception of the first defect (decoding included)"""
        pos = 0
        chunks = []

        def try_read_varint():
            nonlocal pos
            count, result = 0, 0
            while True:
                if pos >= len(stream):
                    if count == 0:
                        return None
                    raise Thrown(END_OF_STREAM)
                b = stream[pos]
                pos += 1
                result = (result + ((b & 0x7F) << count)) & 0xFFFFFFFFFFFFFFFF
                count += 7
                if (b & 0x80) == 0 or count >= 64:
                    break
            return result

        def read_varint():
            v = try_read_varint()
            if v is None:
                raise Thrown(END_OF_STREAM)
            return v

        try:
            while True:
                varint = try_read_varint()
                if varint is None:
                    return chunks, 0
                flags = _i32(varint)                                         # (ChunkFlags) varint, an int enum
                is_compressed = (flags & 1) != 0
                original_length = _i32(read_varint())
                compressed_length = _i32(read_varint()) if is_compressed else original_length
                if compressed_length > original_length:
                    raise Thrown(END_OF_STREAM)
                if compressed_length < 0:
                    raise Thrown(OVERFLOW)                                   # new byte[compressedLength]
                if len(stream) - pos < compressed_length:
                    raise Thrown(END_OF_STREAM)
                at = pos
                pos += compressed_length
                if is_compressed:
                    if (flags >> 2) != 0:
                        raise Thrown(NOT_SUPPORTED)
                    r, _ = self.decode(stream[at:at + compressed_length], original_length)
                    if r != original_length:
                        raise Thrown(INVALID_DATA)
                if original_length > 0:
                    chunks.append((flags, original_length, compressed_length, at))
        except Thrown as e:
            return chunks, e.code

    def decode_stream(self, stream: bytes) -> bytes:
        """the content, or Thrown"""
        chunks, code = self.read_chunks(stream)
        if code:
            raise Thrown(code)
        out = bytearray()
        for flags, U, Cl, at in chunks:
            if flags & 1:
                r, d = self.decode(stream[at:at + Cl], U)
                out += d[:U]
            else:
                out += stream[at:at + U]
        return bytes(out)

    def walk(self, stream: bytes):
        """what the device walk sees: chunks before the first STRUCTURAL defect (no decoding; a compressed chunk's U is trusted up to
        255 * C + 32, C == 0 only for U == 0) -> (chunks, code)"""
        class NoDecode(Witness):
            def decode(s, src, cap):
                if len(src) <= 0:
                    return 0, b""
                return (cap if cap <= 255 * len(src) + 32 and cap > 0 else -1), b""
        nd = NoDecode.__new__(NoDecode)
        nd.ref, nd.x32 = self.ref, self.x32
        return nd.read_chunks(stream)
