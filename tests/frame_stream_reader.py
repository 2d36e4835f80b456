"""A transcription of the reference's blocking frame reader (Frames/LZ4FrameReader.blocking.cs ReadHeader / ReadBlock) for one
frame held in host memory: it meets defects in stream order -- header fields, header checksum, dictionary, then per block
truncation, block checksum, decoding, then the EndMark's content checksum -- and checks ContentLength at the end, as
k4lz4_decode_frames does.  LZ4Frame.DecodeBatch walks the whole frame first and checks data afterwards, so for a frame with
several defects the two may name different ones.  Blocks are decoded by the system liblz4 (LZ4_decompress_safe_usingDict with
the output so far as the prefix of a chained block).  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import struct
from typing import Optional, Tuple

import xxhash

MAGIC = 0x184D2204
_lz4 = None


def lz4():
    global _lz4
    if _lz4 is None:
        lib = C.CDLL("liblz4.so.1")
        lib.LZ4_decompress_safe_usingDict.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
        lib.LZ4_decompress_safe_usingDict.restype = C.c_int
        _lz4 = lib
    return _lz4


class _Defect(Exception):
    def __init__(self, code):
        self.code = code


def read_frame(frame) -> Tuple[int, Optional[bytes]]:
    """-> (0, decoded bytes) or (K4LZ4_FRAME_* code, None)"""
    buf = bytes(frame)
    end = len(buf)
    pos = 0

    def need(n):
        if end - pos < n:
            raise _Defect(-1)
    try:
        need(4)
        if struct.unpack_from("<I", buf, 0)[0] != MAGIC:
            raise _Defect(-2)
        pos = 4
        need(2)
        flg, bd = buf[4], buf[5]
        pos = 6
        if (flg >> 6) & 0x11 != 1:
            raise _Defect(-3)
        chained, bsum, has_size, csum, has_dict = not (flg >> 5) & 1, (flg >> 4) & 1, (flg >> 3) & 1, (flg >> 2) & 1, flg & 1
        clen = None
        if has_size:
            need(8)
            clen = struct.unpack_from("<Q", buf, pos)[0]
            pos += 8
        if has_dict:
            need(4)
            pos += 4
        hc = (xxhash.xxh32(buf[4:pos], seed=0).intdigest() >> 8) & 0xFF
        need(1)
        if buf[pos] != hc:
            raise _Defect(-4)
        pos += 1
        if has_dict:
            raise _Defect(-5)
        bs = {7: 4 << 20, 6: 1 << 20, 5: 256 << 10, 4: 64 << 10}.get((bd >> 4) & 7, 64 << 10)
        out = bytearray()
        while True:
            need(4)
            lc = struct.unpack_from("<I", buf, pos)[0]
            pos += 4
            if lc == 0:
                if csum:
                    need(4)
                    if xxhash.xxh32(bytes(out), seed=0).intdigest() != struct.unpack_from("<I", buf, pos)[0]:
                        raise _Defect(-8)
                break
            n = lc & 0x7FFFFFFF
            need(n)
            payload = buf[pos:pos + n]
            pos += n
            if bsum:
                need(4)
                if xxhash.xxh32(payload, seed=0).intdigest() != struct.unpack_from("<I", buf, pos)[0]:
                    raise _Defect(-7)
                pos += 4
            if lc & 0x80000000:
                out += payload
                continue
            d = bytes(out[-65536:]) if chained else b""
            dst = C.create_string_buffer(bs)
            r = lz4().LZ4_decompress_safe_usingDict(payload, dst, n, bs, d, len(d))
            if r < 0:
                raise _Defect(-6)
            out += dst.raw[:r]
        if clen is not None and len(out) != clen:
            raise _Defect(-10)
        return 0, bytes(out)
    except _Defect as e:
        return e.code, None
