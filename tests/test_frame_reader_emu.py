"""The incremental frame reader's kernel (k4_fr_read_kernel, k4lz4_frame_reader.hpp) and its wave-wide resumable XXH32 under the
host wave emulator (frame_reader_emu.py), against the witness (frame_reader_witness.py) on a reduced set of the GPU test's cases:
valid sources of every kind read in random pieces, the reference's corner cases, structural mutations, and the queries.  Guard
bytes around every slot and every store are checked at every call."""
import numpy as np
import pytest
import xxhash

import frame_reader_cases as K
import frame_reader_emu as E
from frame_reader_witness import WitnessReader
from test_frame_layer import LZ4F

K64 = 65536


def test_wave_xxh32_update_equals_one_shot():
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 400_000, dtype=np.uint8)
    state = np.zeros(64, np.uint8)
    at = 0
    for k, n in enumerate([0, 1, 15, 16, 17, 0, 255, 256, 65536, 3, 100_001, 31]):
        got = E.lib().k4emu_fr_xxh(state.ctypes.data, data[at:].ctypes.data, n, int(k == 0))
        at += n
        assert got == xxhash.xxh32(data[:at].tobytes(), seed=0).intdigest(), (k, n)


@pytest.mark.parametrize("fast", [False, True], ids=["general", "fast"])
def test_valid_sources_in_random_pieces(fast):
    srcs = [s for s in K.valid_sources(LZ4F(), big=False) if not s[0].startswith(("indep-b7", "linked-b7", "linked-raw-b7", "linked-b6"))]
    names = [s[0] for s in srcs]
    sources = [s[1] for s in srcs]
    bs_of = [K64 if not n.startswith(("indep-b", "linked-b")) else K.BLOCK_SIZES[int(n.split("-b")[1][0])] for n in names]
    rd = E.EmuReaders(sources, fast=fast)
    wit = K.check_reads(rd, sources, K.read_plan(np.random.default_rng(5), len(sources), bs_of, calls=6, top=400_000), names)
    q = rd.query()
    for i, w in enumerate(wit):
        assert (int(q[i, 0]), int(q[i, 2])) == (w.bytes_read, w.phase) and w.bytes_read == len(srcs[i][2]), names[i]
    assert q[:, 5].sum() > 0 and (q[:, 4] - q[:, 5] - q[:, 6]).sum() > 0  # the general reader: in place and through the buffer
    if fast:
        served = np.array(rd.plans)
        assert (served == 2).any() and (served == 1).any() and (served == 0).any() and q[:, 6].sum() > 0 and q[:, 7].sum() > 0
    else:
        assert q[:, 6].sum() == 0


def test_corner_cases_follow_the_witness():
    qs = K.quirk_sources()
    names, sources = [n for n, _ in qs], [s for _, s in qs]
    for counts in ([2 * K64, 1, 1, 5 * K64, 7], [K64, 3 * K64, 3 * K64, 10, 10], [5 * K64, 5 * K64, 5 * K64, 1], [0, 1, K64 - 1, K64 + 8, K64, 1 << 20, 3]):
        plan = [(np.full(len(sources), c, np.int64), False) for c in counts]
        K.check_reads(E.EmuReaders(sources, max_block=K64), sources, plan, names, max_block=K64)
        K.check_reads(E.EmuReaders(sources, max_block=K64, fast=True), sources, plan, names, max_block=K64)


def test_fast_path_serves_full_blocks_and_hands_back_the_rest():
    """the walk-ahead, the batch decoder, verify / commit and the resumable checksum against the witness: a regular frame is served
    by the fast path (straddling reads included), a frame with a short middle block is planned and handed back to the general reader
    in the same call, a chained frame is never planned, and a frame whose block checksum fails is handed back and then refused"""
    c = K.corpus.class_bytes("dickens", 6 * K64 + 100, 6).tobytes()
    rnd = K.corpus.random_bytes(2 * K64, 1).tobytes()
    regular = K.indep_frame(c, K64, True, True)
    with_raw = K.indep_frame(c[:K64] + rnd + c[K64:3 * K64], K64, False, True, raw_every=0)
    with_raw = K.frame_of([K.compress(c[:K64]), rnd[:K64], rnd[K64:], K.compress(c[K64:2 * K64])], [False, True, True, False],
                          c[:K64] + rnd + c[K64:2 * K64], K64, False, True, True)
    short_mid = K.frame_of([K.compress(c[:K64]), K.compress(c[K64:K64 + 5000]), K.compress(c[2 * K64:3 * K64])], [False] * 3,
                           c[:K64] + c[K64:K64 + 5000] + c[2 * K64:3 * K64], K64, False, True, True)
    chained = LZ4F().compress(np.frombuffer(c, np.uint8), 4, True, True, False, False)
    bad = bytearray(regular); bad[K64 + 3000] ^= 4
    over = K.frame_of([K.rle_block(K64 + 8), K.compress(c[:K64])], [False, False], bytes([0x42]) * (K64 + 8) + c[:K64], K64, False, False, True)
    sources = [regular, with_raw, short_mid, chained, bytes(bad), over, regular + regular]
    names = ["regular", "raw", "short-middle", "chained", "bad-block-sum", "over8", "two"]
    rd = E.EmuReaders(sources, max_block=K64, fast=True)
    plan = [(np.full(len(sources), n, np.int64), False) for n in (2 * K64, K64 + 1000, K64, 3 * K64, 1 << 20, 1 << 20, 1 << 20)]
    wit = K.check_reads(rd, sources, plan, names, max_block=K64)
    p0, p1 = rd.plans[0], rd.plans[1]
    assert p0.tolist() == [2, 2, 1, 0, 1, 1, 2], p0.tolist()          # served, served, handed back, not planned, handed back x 2, served
    assert p1[0] == 2 and p1[1] == 2                                   # a read that ends inside a block: the straddling block
    assert rd.plans[2][0] == 0                                         # ... leaves bytes pending: the next read is the general reader's
    q = rd.query()
    assert q[0, 6] > 0 and q[2, 7] >= 1 and q[3, 6] == 0 and wit[4].failed == -7 and q[4, 3] == -7
    assert E.lib().k4emu_fr_table_rows(1) == 2 and E.lib().k4emu_fr_table_rows(8 * K64) == 10 and E.lib().k4emu_fr_table_rows(0) == 0


def test_open_frame_length_and_block_size_refusal():
    a = K.indep_frame(b"abc" * 1000, K64, clen=True)
    big = K.indep_frame(b"x" * 1000, 1 << 20)
    sources = [a, big, b"", a[:3], a + a]
    rd = E.EmuReaders(sources, max_block=256 << 10)
    wit = [WitnessReader(s, 256 << 10) for s in sources]
    assert rd.query()[:, 1].tolist() == [-1] * 5
    assert rd.open() == [w.open() for w in wit] == [1, -11, 0, -1, 1]
    assert rd.query()[:, 1].tolist() == [3000, -1, -1, -1, 3000] and rd.query()[:, 3].tolist() == [0, -11, 0, -1, 0]
    assert rd.open([0, 1]) == [1, -11, None, None, None]
    got = rd.read(np.array([5000, 5, 5, 5, -1], np.int64))
    assert got == [w.read(c) if c >= 0 else None for w, c in zip(wit, (5000, 5, 5, 5, -1))]
    assert rd.read(np.full(5, 5000, np.int64))[4] == b"abc" * 1000


def test_structural_mutations_fail_at_the_same_call_with_the_same_code():
    rng = np.random.default_rng(3)
    c = K.corpus.class_bytes("xml", 150_000, 2).tobytes()
    lz4f = LZ4F()
    bases = [K.indep_frame(c, K64, True, True, True), lz4f.compress(np.frombuffer(c, np.uint8), 4, True, True, False, False)]
    for base in bases:
        muts = K.structural_mutants(base)
        names, sources = [n for n, _ in muts], [s for _, s in muts]
        plan = [(np.array([int(rng.choice([0, 7, K64 - 1, K64, K64 + 1, 100_000])) for _ in sources], np.int64), False) for _ in range(4)]
        plan += [(np.full(len(sources), 1 << 20, np.int64), False)] * 3
        wit = K.check_reads(E.EmuReaders(sources, max_block=K64), sources, plan, names, max_block=K64)
        assert sum(w.failed is not None for w in wit) > len(wit) // 2
