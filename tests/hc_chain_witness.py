"""The witness for chained HC streams: the system liblz4 (1.9.3) driven through a literal transcription of
LZ4EncoderBase's ring buffer (Encoders/LZ4EncoderBase.cs: Topup / Encode / Commit) and LZ4HighChainEncoder
(Encoders/LZ4HighChainEncoder.cs: LZ4_initStreamHC + LZ4_resetStreamHC_fast, LZ4_compress_HC_continue,
LZ4_saveDictHC).  Test infrastructure only.

`RingEncoder` is the transcription; its codec is either liblz4 (`Lz4HcCodec`, real bytes) or `TableCodec`,
which only follows the stream context's indices the way LL.high.cs does (LZ4HC_init_internal, LZ4_saveDictHC)
and records (start, length, dictLimit) per block in stream coordinates -- what the block-table model
(encoders.hc_chain_blocks) has to reproduce."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

K1, K64 = 1024, 65536


def compress_bound(n: int) -> int:
    return n + n // 255 + 16


class RingEncoder:
    """LZ4EncoderBase(chaining=True, blockSize, extraBlocks), line by line"""

    def __init__(self, codec, block_size: int, extra_blocks: int = 0):
        block_size = (max(block_size, K1) + K1 - 1) // K1 * K1        # Mem.RoundUp(Math.Max(blockSize, Mem.K1), Mem.K1)
        extra_blocks = max(extra_blocks, 0)
        self.block_size = block_size
        self.input_length = K64 + (1 + extra_blocks) * block_size + 32
        self.buf = (C.c_uint8 * (self.input_length + 8))()            # a fixed address: the codec keeps pointers into it
        self.index = self.pointer = 0
        self.codec = codec

    @property
    def bytes_ready(self) -> int:
        return self.pointer - self.index

    def topup(self, src: np.ndarray, off: int, n: int) -> int:
        if n == 0:
            return 0
        space = self.index + self.block_size - self.pointer
        if space <= 0:
            return 0
        chunk = min(space, n)
        C.memmove(C.addressof(self.buf) + self.pointer, src[off:off + chunk].ctypes.data, chunk)
        self.pointer += chunk
        return chunk

    def encode(self, allow_copy: bool) -> Tuple[int, bytes]:
        n = self.pointer - self.index
        if n <= 0:
            return 0, b""
        encoded, data = self.codec.encode_block(self.buf, self.index, n, compress_bound(self.block_size))
        if encoded <= 0:
            raise RuntimeError("Failed to encode chunk. Target buffer too small.")
        if allow_copy and encoded >= n:
            data = bytes(self.buf[self.index:self.index + n])
            encoded = -n
        self.commit()
        return encoded, data

    def commit(self) -> None:
        self.index = self.pointer
        if self.index + self.block_size <= self.input_length:
            return
        self.index = self.pointer = self.codec.copy_dict(self.buf, self.pointer)


def encode_stream(codec, content: np.ndarray, block_size: int, extra_blocks: int = 0, allow_copy: bool = True) -> List[Tuple[int, bytes]]:
    """the frame writer's loop: TopupAndEncode(forceEncode=false) until the content is in, then FlushAndEncode"""
    enc = RingEncoder(codec, block_size, extra_blocks)
    out, pos = [], 0
    while pos < content.size:
        pos += enc.topup(content, pos, content.size - pos)
        if enc.bytes_ready >= enc.block_size:
            out.append(enc.encode(allow_copy))
    if enc.bytes_ready:
        out.append(enc.encode(allow_copy))
    codec.close()
    return out


class TableCodec:
    """the indices of an LZ4_streamHC_t (LL.high.cs:142-190), no bytes: block k -> (start, length, dictLimit) in stream coordinates"""

    def __init__(self):
        self.base_addr = None          # address of stream position 0 minus the initial 64 KiB offset, per LZ4HC_init_internal
        self.end = None                # index (relative to base) of the end of what has been consumed
        self.dict_limit = self.low_limit = 0
        self.consumed = 0
        self.blocks: List[Tuple[int, int, int]] = []

    def encode_block(self, buf, at: int, n: int, cap: int):
        if self.base_addr is None:                              # LZ4HC_init_internal(start): startingOffset 64 KiB
            self.base_addr = at - K64                           # (buffer offsets stand in for addresses)
            self.end = K64
            self.dict_limit = self.low_limit = K64
        assert at - self.base_addr == self.end, "blocks follow each other in the buffer (no extDict)"
        assert self.low_limit == self.dict_limit
        self.blocks.append((self.consumed, n, self.dict_limit - K64))
        self.end += n
        self.consumed += n
        return 1, b""

    def copy_dict(self, buf, ptr: int) -> int:                 # LZ4_saveDictHC(ctx, buf, ptr)
        prefix = self.end - self.dict_limit
        d = min(ptr, K64)
        d = 0 if d < 4 else d
        d = min(d, prefix)
        end_index = self.end
        self.base_addr = d - end_index                          # the buffer's start now holds the last d bytes
        self.dict_limit = self.low_limit = end_index - d
        return d

    def close(self):
        pass


class Lz4HcCodec:
    """LZ4HighChainEncoder over liblz4's LZ4_streamHC_t"""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            L = C.CDLL("liblz4.so.1")
            L.LZ4_createStreamHC.restype = C.c_void_p
            L.LZ4_freeStreamHC.argtypes = [C.c_void_p]
            L.LZ4_resetStreamHC_fast.argtypes = [C.c_void_p, C.c_int]
            L.LZ4_compress_HC_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            L.LZ4_saveDictHC.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            L.LZ4_decompress_safe_usingDict.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
            L.LZ4_versionNumber.restype = C.c_int
            cls._lib = L
        return cls._lib

    def __init__(self, level: int):
        level = min(max(int(level), 3), 12)                    # LZ4HighChainEncoder.cs:19-20
        self.L = Lz4HcCodec.lib()
        self.ctx = self.L.LZ4_createStreamHC()                  # (LZ4_initStreamHC inside)
        self.L.LZ4_resetStreamHC_fast(self.ctx, level)

    def encode_block(self, buf, at: int, n: int, cap: int):
        dst = (C.c_uint8 * cap)()
        r = self.L.LZ4_compress_HC_continue(self.ctx, C.addressof(buf) + at, dst, n, cap)
        return r, bytes(dst[:max(r, 0)])

    def copy_dict(self, buf, ptr: int) -> int:
        return self.L.LZ4_saveDictHC(self.ctx, buf, ptr)

    def close(self):
        if self.ctx:
            self.L.LZ4_freeStreamHC(self.ctx)
            self.ctx = None


def witness_blocks(content: np.ndarray, level: int, block_size: int, extra_blocks: int = 0, allow_copy: bool = True) -> List[Tuple[int, bytes]]:
    """[(outLen as k4lz4_encode_hc_chain_batch reports it, payload)] per block"""
    return encode_stream(Lz4HcCodec(level), np.ascontiguousarray(content, np.uint8), block_size, extra_blocks, allow_copy)


def witness_table(length: int, block_size: int, extra_blocks: int = 0) -> List[Tuple[int, int, int]]:
    codec = TableCodec()
    encode_stream(codec, np.zeros(length, np.uint8), block_size, extra_blocks, allow_copy=False)
    return codec.blocks


def decode_chain(blocks: List[Tuple[int, bytes]], block_size: int) -> bytes:
    """LZ4ChainDecoder's way: every block decoded with the output so far (its last 64 KiB) as the dictionary"""
    L = Lz4HcCodec.lib()
    out = bytearray()
    for n, data in blocks:
        if n < 0:
            out += data
            continue
        d = bytes(out[-K64:])
        dst = (C.c_uint8 * block_size)()
        r = L.LZ4_decompress_safe_usingDict(data, dst, len(data), block_size, d, len(d))
        if r < 0:
            raise ValueError("block does not decode")
        out += bytes(dst[:r])
    return bytes(out)


def frame_from_blocks(blocks: List[Tuple[int, bytes]], block_size: int, content: np.ndarray, block_checksum: bool,
                      content_checksum: bool, xxh32) -> bytes:
    """LZ4FrameWriter's layout of a chained frame (FLG bit 5 clear) from witness blocks"""
    import struct
    bd = {65536: 4, 262144: 5, 1 << 20: 6, 4 << 20: 7}
    code = next(v for k, v in sorted(bd.items()) if block_size <= k)
    hdr = bytes([(1 << 6) | (int(block_checksum) << 4) | (int(content_checksum) << 2), code << 4])
    parts = [struct.pack("<I", 0x184D2204), hdr, bytes([(xxh32(hdr) >> 8) & 0xFF])]
    for n, data in blocks:
        parts.append(struct.pack("<I", len(data) | (0x80000000 if n < 0 else 0)))
        parts.append(data)
        if block_checksum:
            parts.append(struct.pack("<I", xxh32(data)))
    parts.append(struct.pack("<I", 0))
    if content_checksum:
        parts.append(struct.pack("<I", xxh32(content.tobytes())))
    return b"".join(parts)
