"""The witness for the incremental frame writer: a line-by-line transcription of LZ4FrameWriter (Frames/LZ4FrameWriter.cs:57-108
TryStashFrame, :159-189 block records; Frames/LZ4FrameWriter.async.cs:29-47 WriteManyBytes, :59-90 CloseFrame / WriteFrameTail) over
LZ4EncoderBase's ring buffer (Encoders/LZ4EncoderBase.cs) and, per frame kind, the engine that produces the reference's bytes:
the C oracle's blocks (compress_fast_x32 under Enforce32) for independent blocks, liblz4's LZ4_compress_HC_continue for chained HC
(hc_chain_witness.Lz4HcCodec) and LZ4_compress_fast_continue for chained fast (fast_chain_witness.Lz4FastChainCodec); XXH32 is the
oracle's.  Every call returns the bytes the writer pushed during it.  Test infrastructure only.

Deliberate differences, as in LZ4Frame.EncodeBatch: the content size is written when asked for, and independent blocks are cut at
BlockSize (the reference's encoder rounds its block up to a whole KiB; every size the frame format names is one)."""
from __future__ import annotations

import ctypes as C
import struct
from typing import Optional

import numpy as np

from oracle_lib import Oracle, FrameOracle
import hc_chain_witness as HW
import fast_chain_witness as FW
from k4os.compression.lz4_amd.frames import LZ4Descriptor, frame_header, _extra_blocks

K1, K64 = 1024, 65536


class _BlockCodec:
    """LZ4BlockEncoder.EncodeBlock: every block on its own; CopyDict keeps nothing"""

    def __init__(self, oracle: Oracle, level: int, x32: bool):
        self.o, self.level, self.x32 = oracle, int(level), x32

    def encode_block(self, buf, at: int, n: int, cap: int):
        src = np.frombuffer(bytes(buf[at:at + n]), np.uint8)
        if self.level >= 3:
            r, d = self.o.compress_hc(src, self.level, cap)
        elif self.x32:
            r, d = self.o.compress_fast_x32(src, cap)
        else:
            r, d = self.o.compress_fast(src, cap)
        return r, d[:max(r, 0)].tobytes()

    def copy_dict(self, buf, ptr: int) -> int:
        return 0

    def close(self):
        pass


class _BlockRing(HW.RingEncoder):
    """LZ4EncoderBase(chaining: false) for LZ4BlockEncoder: no dictionary part, the ring is one block + 32 bytes (the block cut at
    BlockSize, see above); Topup / Encode / Commit are hc_chain_witness.RingEncoder's"""

    def __init__(self, codec, block_size: int):
        self.block_size = block_size
        self.input_length = block_size + 32
        self.buf = (C.c_uint8 * (self.input_length + 8))()
        self.index = self.pointer = 0
        self.codec = codec


class WitnessWriter:
    """LZ4FrameWriter for one stream; write / open / close return the bytes each call pushes"""

    def __init__(self, settings, x32: bool = False, oracle: Optional[Oracle] = None):
        self.s = settings
        self.x32 = x32
        self.o = oracle or Oracle()
        self.fo = FrameOracle(self.o)
        self.enc: Optional[HW.RingEncoder] = None
        self.content = bytearray()
        self.blocks = []                                   # the last call's blocks: (encoded as outLen reports it, payload, source length)

    def _create_encoder(self) -> HW.RingEncoder:                    # Streams/Extensions.cs:18-36
        s = self.s
        bs, level = int(s.BlockSize), int(s.CompressionLevel)
        extra = _extra_blocks(bs, int(s.ExtraMemory))
        if not s.ChainBlocks:
            return _BlockRing(_BlockCodec(self.o, level, self.x32), bs)
        if level >= 3:
            return HW.RingEncoder(HW.Lz4HcCodec(level), bs, extra)
        return HW.RingEncoder(FW.Lz4FastChainCodec(), bs, extra)

    def _stash_frame(self) -> bytes:                       # TryStashFrame
        if self.enc is not None:
            return b""
        s = self.s
        d = LZ4Descriptor(s.ContentLength, s.ContentChecksum, bool(s.ChainBlocks), s.BlockChecksum, None, int(s.BlockSize))
        h = frame_header(d)
        self.content = bytearray()                         # InitializeContentChecksum
        self.enc = self._create_encoder()
        return struct.pack("<I", 0x184D2204) + h + bytes([(self.fo.xxh32(h) >> 8) & 0xFF])

    def _encode(self) -> bytes:                           # Encode(allowCopy: true) -> WriteBlock
        n = self.enc.bytes_ready
        encoded, data = self.enc.encode(True)
        self.blocks.append((encoded, data, n))
        return self._block(encoded, data)

    def _block(self, encoded: int, data: bytes) -> bytes:  # WriteBlock: BlockLengthCode, payload, block checksum
        out = struct.pack("<I", len(data) | (0x80000000 if encoded < 0 else 0)) + data
        if self.s.BlockChecksum:
            out += struct.pack("<I", self.fo.xxh32(data))
        return out

    def write(self, data) -> bytes:                        # WriteManyBytes
        self.blocks = []
        out = self._stash_frame()
        src = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
        if self.s.ContentChecksum:
            self.content += src.tobytes()
        offset, count = 0, src.size
        while count > 0:                                   # TopupAndEncode(forceEncode: false, allowCopy: true)
            loaded = self.enc.topup(src, offset, count)
            offset += loaded
            count -= loaded
            if self.enc.bytes_ready >= self.enc.block_size:
                out += self._encode()
        return out

    def open(self) -> bytes:                               # OpenFrame
        self.blocks = []
        return self._stash_frame()

    def close(self) -> bytes:                              # CloseFrame -> WriteFrameTail
        self.blocks = []
        if self.enc is None:
            return b""
        out = b""
        if self.enc.bytes_ready >= 1:                      # FlushAndEncode(forceEncode: true)
            out += self._encode()
        out += struct.pack("<I", 0)
        if self.s.ContentChecksum:
            out += struct.pack("<I", self.fo.xxh32(bytes(self.content)))
        self.enc.codec.close()
        self.enc = None
        return out

    def write_close(self, data) -> bytes:                  # a CLOSE call that carries bytes: Write, then CloseFrame
        out = self.write(data)
        blocks = self.blocks
        out += self.close()
        self.blocks = blocks + self.blocks
        return out
