"""The incremental frame writer's host side (k4lz4_frame_writer_init, k4lz4_frame_writer_store_bytes, k4lz4_frame_write_bound) against
the witness (frame_writer_witness.py: LZ4FrameWriter transcribed over the oracle's engine).  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from frame_writer_witness import WitnessWriter
from k4os.compression.lz4_amd import LZ4Level, corpus
from k4os.compression.lz4_amd import _native
from k4os.compression.lz4_amd.frames import LZ4EncoderSettings, _writer_records, FWRITE_CLOSE

K64 = 65536


@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


SETTINGS = [LZ4EncoderSettings(BlockSize=bs, BlockChecksum=bc, ContentChecksum=cc) for bs in (K64, 256 << 10, 1 << 20, 4 << 20)
            for bc, cc in ((False, False), (True, True))] + \
           [LZ4EncoderSettings(ChainBlocks=True, CompressionLevel=LZ4Level.L09_HC, ExtraMemory=em, BlockChecksum=True) for em in (0, 1, 200000)] + \
           [LZ4EncoderSettings(ChainBlocks=True, ExtraMemory=em, ContentChecksum=True) for em in (0, 300000)] + \
           [LZ4EncoderSettings(ContentLength=12345, BlockSize=1000)]


def test_init_follows_the_encoders_ring(lib):
    recs, off, total = _writer_records(len(SETTINGS), SETTINGS, lib)
    for i, s in enumerate(SETTINGS):
        ring = WitnessWriter(s)._create_encoder()
        r = recs[i]
        assert r.encBlock == ring.block_size
        assert r.ringBytes == (ring.input_length if s.ChainBlocks else ring.block_size)
        assert r.kind == (0 if not s.ChainBlocks else 1 if int(s.CompressionLevel) >= 3 else 2)
        assert lib.k4lz4_frame_writer_store_bytes(C.byref(r)) >= r.ringBytes + 64
        assert r.phase == 0 and r.written == 0 and r.index == r.pointer == 0
    assert total == int(sum(lib.k4lz4_frame_writer_store_bytes(C.byref(recs[i])) for i in range(len(SETTINGS))))


def test_init_refuses_block_sizes_past_4_mib(lib):
    with pytest.raises(ValueError):
        _writer_records(1, LZ4EncoderSettings(BlockSize=(4 << 20) + 1), lib)


def test_bound_covers_what_the_witness_writes(lib):
    """a never-opened stream: the first call's bytes, for writes of every shape, never pass the bound (and a close that writes
    nothing has bound 0); stored blocks (random bytes) come within a few bytes of it"""
    rng = np.random.default_rng(5)
    data = corpus.silesia_like_blocks(2, 1 << 20, seed=1).reshape(-1)
    noise = rng.integers(0, 256, 9 << 20, dtype=np.uint8)
    recs, _, _ = _writer_records(len(SETTINGS), SETTINGS, lib)
    for i, s in enumerate(SETTINGS):
        r = recs[i]
        assert lib.k4lz4_frame_write_bound(C.byref(r), 0, 1) == 0                     # CloseFrame of a frame never opened
        for n in (0, 1, 15, r.encBlock - 1, r.encBlock, 2 * r.encBlock + 7):
            if s.ContentLength is not None and n != s.ContentLength:
                continue
            for src in (data, noise):
                for closing in (False, True):
                    w = WitnessWriter(s)
                    # a CLOSE call of n bytes is Write + CloseFrame; of none, on a frame never opened, CloseFrame alone
                    got = w.close() if closing and n == 0 else w.write(src[:n]) + (w.close() if closing else b"")
                    b = lib.k4lz4_frame_write_bound(C.byref(r), n, int(closing))
                    assert len(got) <= b, (i, n, closing)
                    if src is noise and n >= 16:
                        assert b - len(got) <= 16, (i, n, closing, b, len(got))
