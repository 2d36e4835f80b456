"""LZ4Stream piece by piece: the new kernels (k4lz4_legacy_stream.hpp) and the host plan under the host wave emulator
(legacy_stream_emu.py), call by call against the witness (legacy_stream_witness.py).  No GPU."""
import numpy as np
import pytest

from legacy_witness import Witness
from legacy_stream_witness import WriterCalls, read_calls
from legacy_stream_emu import EmuWriters, EmuReaders
from test_legacy_host import valid_streams, damaged_streams
from k4os.compression.lz4_amd import corpus

WRITE, FLUSH, CLOSE = 0, 1, 2
LSQ_BATCHED, LSQ_HANDED_BACK = 6, 7


@pytest.fixture(scope="module")
def w():
    return Witness()


def _drive(w, blocks, steps):
    """steps: [(op, pieces)] -> every call's bytes equal the witness's"""
    em = EmuWriters(blocks)
    wcs = [WriterCalls(w, False, b) for b in blocks]
    for op, pieces in steps:
        out, got = em.call(op, pieces)
        for i, p in enumerate(pieces):
            if p is None:
                assert out[i] == 0 and got[i] is None
                continue
            want = wcs[i].write(p) if op == WRITE else wcs[i].flush() if op == FLUSH else wcs[i].dispose(p)
            assert got[i] == want, (op, i, blocks[i], len(p))
            assert em.recs[i].pending == wcs[i].pending
    return em


def test_writer_random_writes(w):
    rng = np.random.default_rng(21)
    blocks = [16, 16, 100, 4096, 4096, 65536, 1000, 16]
    text = corpus.class_bytes("xml", 300000, 1).tobytes()
    noise = rng.integers(0, 256, 300000, dtype=np.uint8).tobytes()
    steps = []
    for k in range(10):
        op = WRITE if k < 2 else int(rng.choice([WRITE, WRITE, FLUSH]))
        pieces = []
        for B in blocks:
            if rng.random() < 0.15:
                pieces.append(None)
            elif op == FLUSH:
                pieces.append(b"")
            else:
                size = int(rng.choice([0, int(rng.integers(1, 16)), B - 1, B, B + 1, 2 * B, 3 * B + 7]))
                src = noise if rng.random() < 0.2 else text
                at = int(rng.integers(0, len(src) - size))
                pieces.append(src[at:at + size])
        steps.append((op, pieces))
    steps.append((CLOSE, [b"end"[:i % 4] for i in range(len(blocks))]))
    em = _drive(w, blocks, steps)
    out, got = em.call(WRITE, [b"x"] * len(blocks))
    assert (out == -9).all()                                                          # closed streams refuse


@pytest.mark.parametrize("B", [16, 4096])
def test_writer_corner_cases_one_by_one(w, B):
    data = corpus.class_bytes("dickens", 3 * B + 7, 2).tobytes()
    for n in (0, 1, 15, 16, B - 1, B, B + 1, 2 * B, 3 * B + 7):
        for first in (0, 1, B - 1, B):                                                # what is pending when the write arrives
            _drive(w, [B], [(WRITE, [data[:first]]), (WRITE, [data[:n]]), (WRITE, [data[:1]]), (FLUSH, [b""]), (FLUSH, [b""]),
                            (CLOSE, [data[:n]])])


def test_writer_short_target_is_refused_and_retried(w):
    B = 4096
    data = corpus.class_bytes("xml", 3 * B + 7, 3).tobytes()
    em = EmuWriters([B, B])
    wc = WriterCalls(w, False, B)
    em.call(WRITE, [data[:100], data[:100]])
    wc.write(data[:100])
    out, got = em.call(WRITE, [data, data], short=[0])
    want = wc.write(data)
    assert out[0] == -6 and got[0] is None and got[1] == want and em.recs[0].pending == 100
    out, got = em.call(WRITE, [data, None])
    assert got[0] == want and em.recs[0].pending == em.recs[1].pending


def _compare(w, srcs, calls, interactive, max_block, direct=True):
    want = [read_calls(w, s, [c[i] for c in calls], interactive, max_block) for i, s in enumerate(srcs)]
    em = EmuReaders(srcs, max_block, direct=direct)
    for k, counts in enumerate(calls):
        got = em.read(counts, interactive)
        for i in range(len(srcs)):
            assert got[i] == want[i][k], (k, i, counts[i], got[i] if isinstance(got[i], int) else len(got[i] or b""),
                                          want[i][k] if isinstance(want[i][k], int) else len(want[i][k] or b""))
    return em


def _calls(rng, n, k, scale):
    return [[None if rng.random() < 0.07 else int(rng.choice([0, 1, 15, 16, 17, 1000, 4096, int(rng.integers(1, scale)), scale]))
             for _ in range(n)] for _ in range(k)]


@pytest.mark.parametrize("interactive", [False, True])
def test_reader_valid_streams_in_random_counts(w, interactive):
    srcs = valid_streams(w)
    em = _compare(w, srcs, _calls(np.random.default_rng(22), len(srcs), 14, 30000), interactive, 65536)
    q = em.query()
    if not interactive:
        assert (q[:, LSQ_BATCHED] > 0).any()
        _compare(w, srcs, _calls(np.random.default_rng(23), len(srcs), 8, 30000), False, 65536, direct=False)     # the general kernel alone


@pytest.mark.parametrize("interactive", [False, True])
def test_reader_mutants_and_truncations_in_random_counts(w, interactive):
    """the code equals the witness's, in the call in which the witness throws it -- never later than its last byte"""
    srcs = damaged_streams(w)
    base = w.encode_stream(corpus.class_bytes("dickens", 20000, 6).tobytes(), False, 4096)
    rng = np.random.default_rng(24)
    for _ in range(16):
        m = bytearray(base)
        m[int(rng.integers(4, len(m)))] ^= 1 << int(rng.integers(0, 8))
        srcs.append(bytes(m))
    _compare(w, srcs, _calls(rng, len(srcs), 10, 9000), interactive, 4096)


def test_reader_corner_cases_and_both_ways_in_one_call(w):
    text = corpus.class_bytes("xml", 40000, 7).tobytes()
    good = w.encode_stream(text, False, 4096)
    chunks, _ = w.read_chunks(good)
    bad = bytearray(good)
    at = chunks[4][3]
    bad[at:at + 3] = b"\xff\xff\xff"
    srcs = [good, bytes(bad), good, bytes(bad), w.encode_stream(text, False, 16)]
    em = _compare(w, srcs, [[8192] * 5, [20000] * 5, [1] * 5, [0] * 5, [50000] * 5, [5] * 5], False, 4096)
    assert list(em.plans[1][:4]) == [2, 1, 2, 1]                                      # served directly / handed back, in one call
    q = em.query()
    assert q[1, LSQ_HANDED_BACK] == 1 and q[0, LSQ_HANDED_BACK] == 0 and q[0, LSQ_BATCHED] >= 7
    # a chunk above maxBlockSize, ReadByte to the end, empty chunks between good ones
    _compare(w, [good], [[10], [10]], False, 4095)
    a, b = w.encode_stream(text[:100], False, 100), w.encode_stream(text[100:300], False, 100)
    _compare(w, [a + b, a + b"\x00\x00" + b"\x01\x00\x00" + b], [[1, 1]] * 40 + [[400, 400]] * 2, False, 100)
