"""The incremental frame writer without a GPU: its kernels under the host wave emulator (frame_write_emu.py) and its host model
(k4lz4_frame_write.hpp: fw_model / fw_code / fw_advance, what k4lz4_frame_write_batch runs) against the witness (frame_writer_witness.py:
LZ4FrameWriter over LZ4EncoderBase's ring, hc_chain_witness.RingEncoder, the oracle's engine and liblz4)."""
import ctypes as C

import numpy as np
import pytest

import frame_write_emu as E
from frame_writer_witness import WitnessWriter
from oracle_lib import Oracle, FrameOracle
from k4os.compression.lz4_amd import LZ4Level, corpus
from k4os.compression.lz4_amd import _native
from k4os.compression.lz4_amd.frames import LZ4EncoderSettings, _writer_records, FWRITE_WRITE, FWRITE_OPEN, FWRITE_CLOSE

K64 = 65536
XXH_STATE = 48
p = lambda a: a.ctypes.data  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def pool():
    rng = np.random.default_rng(3)
    return np.concatenate([corpus.silesia_like_blocks(64, K64, seed=9).reshape(-1), rng.integers(0, 256, 2 << 20, dtype=np.uint8)])


def test_resumable_xxh32_equals_one_shot(oracle, pool):
    """k4_fw_xxh32_kernel + the digest over random splits (empty writes, 1-15 bytes, stripes, long runs) equals XXH32 of the prefix"""
    fo = FrameOracle(oracle)
    rng = np.random.default_rng(7)
    n = 24
    state = np.zeros(n * XXH_STATE, np.uint8)
    digest = np.zeros(n, np.uint32)
    starts = rng.integers(0, pool.size // 2, n)
    done = np.zeros(n, np.int64)
    for call in range(10):
        lens = np.array([int(rng.choice([0, 1, 3, 15, 16, 17, 31, 64, 1000, 65537, 300001])) for _ in range(n)], np.uint64)
        off = (starts + done).astype(np.uint64)
        fresh = np.full(n, 1 if call == 0 else 0, np.uint32)
        E.lib().k4emu_fw_xxh32(p(pool), p(off), p(lens), p(fresh), p(state), p(digest), n, 4)
        done += lens.astype(np.int64)
        for i in range(n):
            assert int(digest[i]) == fo.xxh32(pool[int(starts[i]):int(starts[i] + done[i])]), (call, i)


MODEL_SETTINGS = [LZ4EncoderSettings(BlockSize=bs) for bs in (K64, 256 << 10, 1 << 20, 4 << 20)] + \
    [LZ4EncoderSettings(ChainBlocks=True, CompressionLevel=LZ4Level.L03_HC, BlockSize=bs, ExtraMemory=em)
     for bs, em in ((K64, 0), (256 << 10, 1), (K64, 300000), (1 << 20, 0), (4 << 20, 0))] + \
    [LZ4EncoderSettings(ChainBlocks=True, BlockSize=bs, ExtraMemory=em) for bs, em in ((K64, 0), (K64, 200000), (256 << 10, 0), (1 << 20, 1))]


@pytest.mark.parametrize("k", range(len(MODEL_SETTINGS)))
def test_model_follows_the_witness_ring(lib, oracle, pool, k):
    """per call: the blocks fw_model cuts (their lengths), the ring's index and pointer after the call, and for chained fast streams
    LZ4_stream_t's currentOffset / dictSize, against the reference's ring buffer and liblz4's context"""
    s = MODEL_SETTINGS[k]
    recs, _, _ = _writer_records(1, s, lib)
    B = recs[0].encBlock
    w = WitnessWriter(s, oracle=oracle)
    rng = np.random.default_rng(100 + k)
    pos = written = 0
    sizes = [0, 1, B, 2 * B, 3 << 20, B - 1, 15, int(rng.integers(1, 3 * B)), 5 << 20, 0, int(rng.integers(1, 100000))]
    for call, n in enumerate(sizes + [None]):
        closing = n is None
        n = 0 if closing else min(n, pool.size - pos)
        chunk = pool[pos:pos + n]
        pos = (pos + n) % (pool.size // 2)
        written += n
        got_bytes = w.close() if closing else w.write(chunk)
        code, nblk = np.zeros(1, np.int32), np.zeros(1, np.uint32)
        bs_, bl = np.zeros(4096, np.int64), np.zeros(4096, np.int64)
        ln, cap = np.array([n], np.int64), np.array([1 << 40], np.uint64)        # (kept alive across the call)
        nb = E.lib().k4emu_fw_plan(C.byref(recs[0]), p(ln), p(cap), 1, FWRITE_CLOSE if closing else FWRITE_WRITE, p(code), p(nblk), p(bs_),
                                   p(bl), 4096)
        assert code[0] == 0 and nb == len(w.blocks), (call, n, nb, len(w.blocks))
        assert [int(x) for x in bl[:nb]] == [b[2] for b in w.blocks], call
        assert len(got_bytes) <= 15 + nb * (8 + B) + 8
        if closing:
            assert recs[0].phase == 2
            break
        assert (recs[0].index, recs[0].pointer) == (w.enc.index, w.enc.pointer), call
        assert recs[0].written == written
        if recs[0].kind == 2:
            st = w.enc.codec.state()
            assert (recs[0].currentOffset, recs[0].dictSize) == (st["currentOffset"], st["dictSize"]), call


def test_refusals_leave_the_record(lib):
    s = LZ4EncoderSettings(ContentLength=10)
    recs, _, _ = _writer_records(3, s, lib)
    code, nblk = np.zeros(3, np.int32), np.zeros(3, np.uint32)
    bs_, bl = np.zeros(8, np.int64), np.zeros(8, np.int64)

    def plan(lens, caps, op):
        ln, cap = np.array(lens, np.int64), np.array(caps, np.uint64)
        E.lib().k4emu_fw_plan(recs, p(ln), p(cap), 3, op, p(code), p(nblk), p(bs_), p(bl), 8)
        return list(code)
    assert plan([4, 4, 4], [1 << 40, 1 << 40, 3], FWRITE_WRITE) == [0, 0, -1]
    assert recs[2].phase == 0 and recs[0].phase == 1
    assert plan([2, 6, -1], [1 << 40] * 3, FWRITE_CLOSE) == [-3, 0, 1]
    assert recs[0].phase == 1 and recs[0].written == 4 and recs[1].phase == 2
    assert plan([0, 0, 0], [1 << 40] * 3, FWRITE_OPEN) == [0, -2, 0] and recs[2].phase == 1


EMIT_SETTINGS = [LZ4EncoderSettings(), LZ4EncoderSettings(BlockChecksum=True, ContentChecksum=True),
                 LZ4EncoderSettings(BlockSize=256 << 10, ContentChecksum=True, CompressionLevel=LZ4Level.L09_HC),
                 LZ4EncoderSettings(ChainBlocks=True, CompressionLevel=LZ4Level.L09_HC, BlockChecksum=True, ContentChecksum=True),
                 LZ4EncoderSettings(ChainBlocks=True, CompressionLevel=LZ4Level.L03_HC, ExtraMemory=1),
                 LZ4EncoderSettings(ContentLength=None, BlockSize=1 << 20, BlockChecksum=True)]


def test_emitted_records_and_rings_equal_the_witness(lib, oracle, pool):
    """k4emu_fw_call (the writer's kernels: hash, staging, write-back, record sizes, block checksums, scan, places, records, edges) with
    the witness's encoded blocks standing in for the encoder: every call's bytes per stream equal the witness's, and every stream's ring
    in its store holds what the reference's ring buffer holds"""
    n = 12
    settings = [EMIT_SETTINGS[i % len(EMIT_SETTINGS)] for i in range(n)]
    recs, soff, size = _writer_records(n, settings, lib)
    store = np.zeros(size + 64, np.uint8)
    wit = [WitnessWriter(s, oracle=oracle) for s in settings]
    rng = np.random.default_rng(5)
    ops = [FWRITE_OPEN] + [FWRITE_WRITE] * 6 + [FWRITE_CLOSE]
    for call, op in enumerate(ops):
        lens = np.array([0 if op == FWRITE_OPEN else -1 if rng.random() < 0.15 else
                         int(rng.choice([0, 1, 15, K64, 2 * K64, 100000, 2 << 20])) for _ in range(n)], np.int64)
        if op == FWRITE_CLOSE:
            lens = np.where(np.arange(n) % 2 == 0, 0, 70000)          # half of the closes carry bytes
        starts = rng.integers(0, pool.size // 2, n)
        src = np.concatenate([pool[int(starts[i]):int(starts[i]) + max(int(lens[i]), 0)] for i in range(n)] + [np.zeros(16, np.uint8)])
        srcoff = np.concatenate(([0], np.cumsum(np.maximum(lens, 0))))[:-1].astype(np.uint64)
        want = []
        for i in range(n):
            chunk = src[int(srcoff[i]):int(srcoff[i]) + max(int(lens[i]), 0)]
            if lens[i] < 0:
                want.append(b""); wit[i].blocks = []
            elif op == FWRITE_OPEN:
                want.append(wit[i].open())
            elif op == FWRITE_CLOSE:
                want.append(wit[i].write_close(chunk) if lens[i] > 0 else wit[i].close())
            else:
                want.append(wit[i].write(chunk))
        blocks = [b for i in range(n) for b in wit[i].blocks]
        enc_len = np.array([b[0] for b in blocks] + [0], np.int32)
        enc_off = np.zeros(len(blocks) + 1, np.uint64)
        enc_off[1:] = np.cumsum([len(b[1]) for b in blocks])
        arena = np.frombuffer(b"".join(b[1] for b in blocks) + bytes(16), np.uint8).copy()
        dcap = np.array([len(x) + 64 for x in want], np.uint64)
        doff = np.concatenate(([0], np.cumsum(dcap)))[:-1].astype(np.uint64)
        dst = np.zeros(int(dcap.sum()) + 64, np.uint8)
        out = np.zeros(n, np.int64)
        nb = E.lib().k4emu_fw_call(recs, p(store), p(soff), p(src), p(srcoff), p(lens), n, op, p(enc_len), p(arena), p(enc_off), len(blocks),
                                   p(dst), p(doff), p(out), 4)
        assert nb == len(blocks), (call, nb, len(blocks))
        for i in range(n):
            assert dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() == want[i], (call, i, settings[i])
            if op != FWRITE_CLOSE and wit[i].enc is not None:
                ring = store[int(soff[i]) + 64 + 0:][:recs[i].pointer]
                assert (recs[i].index, recs[i].pointer) == (wit[i].enc.index, wit[i].enc.pointer), (call, i)
                assert ring.tobytes() == bytes(wit[i].enc.buf[:recs[i].pointer]), (call, i)
