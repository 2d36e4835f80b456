"""The incremental side of K4os.Compression.LZ4.Legacy's LZ4Stream, transcribed line by line in the style of legacy_witness.py:
the reader's Read / ReadByte over AcquireNextChunk / TryReadVarInt (LZ4Stream.cs:133-191, :248-294, :332-377) in both modes, with
the reference's exception order, over an in-memory inner stream and the reference's own block engine (legacy_witness.Witness).
For the writer, legacy_witness.Witness.Writer is driven call by call and the bytes each call appends are recorded.  The checker
of the legacy stream tests: it never touches libk4lz4.

Not the reference's: max_block_size.  The library refuses a chunk whose original length is above the reader's maxBlockSize
(BLOCK_SIZE) where the reference would allocate a buffer of that size; the witness does the same when a limit is given."""
from __future__ import annotations

from typing import List, Optional, Tuple

from legacy_witness import Witness, Thrown, END_OF_STREAM, OVERFLOW, NOT_SUPPORTED, INVALID_DATA, _i32

BLOCK_SIZE, CLOSED, CAPACITY = -8, -9, -6


class Reader:
    """LZ4Stream(inner, LZ4StreamMode.Decompress, interactiveRead)"""

    def __init__(self, w: Witness, stream: bytes, interactive: bool = False, max_block_size: Optional[int] = None):
        self.w, self.inner, self.pos = w, bytes(stream), 0
        self.interactive = interactive
        self.max_block_size = max_block_size
        self.buffer = b""
        self.buffer_length = 0
        self.buffer_offset = 0
        self.failed: Optional[int] = None
        self.chunks = 0                       # chunks acquired that produce bytes (a statistic the tests compare)

    # ---- the inner stream --------------------------------------------------------------------------------------------------
    def _inner_read(self, n: int) -> bytes:
        got = self.inner[self.pos:self.pos + n]
        self.pos += len(got)
        return got

    def _try_read_varint(self) -> Optional[int]:                  # :133-155
        count, result = 0, 0
        while True:
            b = self._inner_read(1)
            if len(b) == 0:
                if count == 0:
                    return None
                raise Thrown(END_OF_STREAM)
            result = (result + ((b[0] & 0x7F) << count)) & 0xFFFFFFFFFFFFFFFF
            count += 7
            if (b[0] & 0x80) == 0 or count >= 64:
                break
        return result

    def _read_varint(self) -> int:                                # :161-167
        v = self._try_read_varint()
        if v is None:
            raise Thrown(END_OF_STREAM)
        return v

    def _acquire_next_chunk(self) -> bool:                        # :248-294
        while True:
            varint = self._try_read_varint()
            if varint is None:
                return False
            flags = _i32(varint)
            is_compressed = (flags & 1) != 0
            original_length = _i32(self._read_varint())
            compressed_length = _i32(self._read_varint()) if is_compressed else original_length
            if compressed_length > original_length:
                raise Thrown(END_OF_STREAM)
            if compressed_length < 0:
                raise Thrown(OVERFLOW)                            # new byte[compressedLength]
            compressed = self._inner_read(compressed_length)      # ReadBlock
            if len(compressed) != compressed_length:
                raise Thrown(END_OF_STREAM)
            if not is_compressed:
                if self.max_block_size is not None and original_length > self.max_block_size:
                    raise Thrown(BLOCK_SIZE)
                self.buffer = compressed
                self.buffer_length = compressed_length
            else:
                passes = flags >> 2
                if passes != 0:
                    raise Thrown(NOT_SUPPORTED)
                if self.max_block_size is not None and original_length > self.max_block_size:
                    # refused before its bytes are looked at, but behind what no payload can satisfy (4.12's walk: C bytes never
                    # decode to more than 255 * C + 32, nothing decodes to nothing)
                    if original_length > 255 * compressed_length + 32 or compressed_length == 0:
                        raise Thrown(INVALID_DATA)
                    raise Thrown(BLOCK_SIZE)
                r, d = self.w.decode(compressed, original_length)
                if r != original_length:
                    raise Thrown(INVALID_DATA)
                self.buffer = d[:original_length]
                self.buffer_length = original_length
            self.buffer_offset = 0
            if self.buffer_length != 0:                           # :291 skip empty block
                self.chunks += 1
                return True

    # ---- Read / ReadByte ---------------------------------------------------------------------------------------------------
    def read(self, count: int) -> bytes:
        """the bytes Read(buffer, 0, count) delivers, or Thrown; a stream that has thrown stays failed (the library's rule)"""
        if self.failed is not None:
            raise Thrown(self.failed)
        try:
            out = bytearray()
            while count > 0:                                      # :355-374
                chunk = min(count, self.buffer_length - self.buffer_offset)
                if chunk <= 0:
                    if not self._acquire_next_chunk():
                        break
                else:
                    out += self.buffer[self.buffer_offset:self.buffer_offset + chunk]
                    self.buffer_offset += chunk
                    if self.interactive:
                        break
                    count -= chunk
            return bytes(out)
        except Thrown as e:
            self.failed = e.code
            raise

    def read_byte(self) -> int:                                   # :332-342
        if self.failed is not None:
            raise Thrown(self.failed)
        try:
            if self.buffer_offset >= self.buffer_length and not self._acquire_next_chunk():
                return -1
            self.buffer_offset += 1
            return self.buffer[self.buffer_offset - 1]
        except Thrown as e:
            self.failed = e.code
            raise


def read_calls(w: Witness, stream: bytes, counts, interactive: bool = False, max_block_size: Optional[int] = None):
    """one Read per count -> [bytes, or the thrown code]; after a throw every later call reports the same code"""
    r = Reader(w, stream, interactive, max_block_size)
    out = []
    for c in counts:
        if c is None or c < 0:
            out.append(None)
            continue
        try:
            out.append(r.read(int(c)))
        except Thrown as e:
            out.append(e.code)
    return out


class WriterCalls:
    """Witness.Writer driven call by call: write / flush / dispose return the bytes the call pushed to the inner stream"""

    def __init__(self, w: Witness, high: bool = False, block_size: int = 1 << 20):
        self.wr = Witness.Writer(w, high, block_size)
        self.closed = False

    def _delta(self, fn) -> bytes:
        before = len(self.wr.out)
        fn()
        return bytes(self.wr.out[before:])

    @property
    def pending(self) -> int:
        return self.wr.offset

    def write(self, data: bytes) -> bytes:
        return self._delta(lambda: self.wr.write(bytes(data)))

    def flush(self) -> bytes:
        return self._delta(self.wr.flush)

    def dispose(self, data: bytes = b"") -> bytes:
        """Write(data) then Dispose"""
        def both():
            self.wr.write(bytes(data))
            self.wr.flush()
        self.closed = True
        return self._delta(both)


def chunk_count(stream_bytes: bytes) -> int:
    """records in a well-formed piece of a stream (what one writer call emitted)"""
    pos, n = 0, 0

    def varint():
        nonlocal pos
        v, s = 0, 0
        while True:
            b = stream_bytes[pos]
            pos += 1
            v |= (b & 0x7F) << s
            s += 7
            if not b & 0x80:
                return v
    while pos < len(stream_bytes):
        flags = varint()
        u = varint()
        payload = varint() if flags & 1 else u
        pos += payload
        n += 1
    assert pos == len(stream_bytes)
    return n


def lazy_flush(B: int, p: int, L: int, op: str) -> Tuple[int, int]:
    """the issue's formula: (chunks emitted, bytes pending afterwards) for a call with p pending bytes and L new ones"""
    if op == "flush":
        return (1, 0) if p > 0 else (0, 0)
    e = max(0, -(-(p + L) // B) - 1) if L > 0 else 0
    rest = p + L - B * e
    if op == "close":
        return e + (1 if rest > 0 else 0), 0
    return e, rest
