"""The witness for ILZ4Encoder as LZ4Encoder.Create makes it (Encoders/LZ4Encoder.cs): hc_chain_witness.RingEncoder -- the literal
transcription of LZ4EncoderBase -- over liblz4 1.9.3's _continue streams (Lz4HcCodec, Lz4FastChainCodec) and, for independent
encoders, the oracle's block encoder as frame_writer_witness wraps it (LL32 under Enforce32), with TopupAndEncode / FlushAndEncode
transcribed from Encoders/LZ4EncoderExtensions.cs:117-210.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

import hc_chain_witness as HW
import fast_chain_witness as FW

K1, K64 = 1024, 65536


class BlockRing(HW.RingEncoder):
    """LZ4BlockEncoder(level, blockSize): base(false, blockSize, 0) -- no dictionary part"""

    def __init__(self, codec, block_size: int):
        super().__init__(codec, block_size, 0)
        self.input_length = self.block_size + 32
        self.buf = (C.c_uint8 * (self.input_length + 8))()


class CountingCodec:
    """the indices alone, for any kind: records (block length, dictSize before the block) and what CopyDict keeps"""

    def __init__(self, kind: int):
        self.kind, self.dict_size, self.cur = kind, 0, 0
        self.blocks: List[Tuple[int, int]] = []
        self.saves: List[int] = []                       # the move distance of every save: pointer - kept

    def encode_block(self, buf, at, n, cap):
        self.blocks.append((n, self.dict_size))
        self.dict_size += n
        self.cur += n
        return 1, b""

    def copy_dict(self, buf, ptr):
        if self.kind == 0:
            return 0
        d = min(ptr, K64)
        if self.kind == 1:
            d = 0 if d < 4 else d
        else:
            d = min(d, self.dict_size)
        self.dict_size = d
        self.saves.append(ptr - d)
        return d

    def close(self):
        pass


class Tap:
    """a codec with every EncodeBlock result kept: (encoded, bytes) before LZ4EncoderBase applies the allowCopy rule"""

    def __init__(self, codec):
        self.codec, self.raw = codec, []

    def encode_block(self, buf, at, n, cap):
        r, d = self.codec.encode_block(buf, at, n, cap)
        self.raw.append((r, d))
        return r, d

    def __getattr__(self, name):
        return getattr(self.codec, name)


def kind_of(chaining, level) -> int:
    """Encoders/LZ4Encoder.cs: Create"""
    return 0 if not chaining else (2 if int(level) < 3 else 1)


class WitnessEncoder:
    """one ILZ4Encoder; run(records) applies TopupAndEncode records and returns what k4lz4_chain_encode_batch reports"""

    def __init__(self, chaining, level, block_size, extra_blocks=0, x32=False, oracle=None, counting=False):
        self.kind = kind_of(chaining, level)
        if counting:
            codec = CountingCodec(self.kind)
        elif self.kind == 0:
            from frame_writer_witness import _BlockCodec
            from oracle_lib import Oracle
            codec = _BlockCodec(oracle or Oracle(), int(level), x32)
        elif self.kind == 1:
            codec = HW.Lz4HcCodec(level)
        else:
            codec = FW.Lz4FastChainCodec()
        self.codec = codec = Tap(codec)
        self.enc = BlockRing(codec, block_size) if self.kind == 0 else HW.RingEncoder(codec, block_size, extra_blocks)

    def topup_and_encode(self, src: np.ndarray, force: bool, allow_copy: bool):
        """-> (loaded, encoded before the sign is dropped, bytes)   LZ4EncoderExtensions.cs:117-132, :190-210"""
        loaded = self.enc.topup(src, 0, src.size) if src.size > 0 else 0
        if self.enc.bytes_ready < (1 if force else self.enc.block_size):
            return loaded, 0, b""
        encoded, data = self.enc.encode(allow_copy)
        return loaded, encoded, data

    def run(self, records):
        loaded, out, data = [], [], b""
        for src, force, allow in records:
            l, e, d = self.topup_and_encode(np.ascontiguousarray(np.frombuffer(bytes(src), np.uint8)), bool(force), bool(allow))
            loaded.append(l); out.append(e); data += d
        return loaded, out, data

    def ring(self) -> bytes:
        return bytes(self.enc.buf[:self.enc.pointer])

    def close(self):
        self.codec.close()
