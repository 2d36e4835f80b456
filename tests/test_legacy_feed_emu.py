"""The fed LZ4Stream reader's kernels (k4lz4_legacy_feed.hpp: k4_ls_feed_kernel and the direct path's top-up / plan / commit for
pieces) under the host wave emulator (legacy_feed_emu.py).  Every test drives logical reads (frame_feed_cases.FedDriver) and compares
them with legacy_stream_witness.Reader over the WHOLE source with max_block_size set; the driver holds every raw call to the contract
(consumed, need, final), and guard bytes around every slot, store and piece are checked at every call.  No GPU."""
import numpy as np
import pytest

import legacy_feed_cases as LC
import legacy_feed_emu as E
from legacy_witness import Witness
from test_legacy_host import valid_streams, damaged_streams
from k4os.compression.lz4_amd import corpus

B = 300


@pytest.fixture(scope="module")
def w():
    return Witness()


@pytest.mark.parametrize("count,interactive,direct", [(1 << 20, False, False), (1 << 20, False, True), (100, False, False), (100, False, True),
                                                      (7, False, False), (1, False, False), (100, True, False), (1 << 20, True, False)],
                         ids=["whole", "whole-direct", "100", "100-direct", "7", "1", "100-interactive", "whole-interactive"])
def test_every_single_cut(w, count, interactive, direct):
    """the small stream cut at every byte position k into [0, k) and [k, end) final, one reader per k, read to its end by logical
    reads of `count` bytes.  Whenever the call over [0, k) starves, consumed == srcLen and need == field_end(k) - k (FedDriver asserts
    both from the layout)."""
    src, content = LC.small_stream(w, B)
    ks = list(range(len(src) + 1))
    sources = [src] * len(ks)
    rd = E.EmuFedReaders(len(ks), max_block=B, threads=8, direct=direct)
    drv = LC.driver(rd, sources, [[k, len(src)] for k in ks])
    n_reads = len(LC.layout(src)) + 3 if interactive else len(LC.reads_to_the_end(len(content), count))
    if interactive and count < B:
        n_reads = sum(-(-c[3] // count) for c in LC.layout(src)) + 3
    wit = LC.check_reads(drv, w, sources, [[count] * len(ks)] * n_reads, interactive, B, [f"k{k}" for k in ks])
    q = rd.query()
    LC.check_query(q, wit)
    assert all(x.pos == len(src) and x.failed is None for x in wit) and (q[:, LC.LSQ_BYTES_READ] == len(content)).all()
    # every cut that lies inside the source starved once at k with everything in front of it consumed
    at_k = {u for i, u, _ in drv.starved if u == ks[i]}
    assert at_k >= set(range(1, len(src))), sorted(set(range(1, len(src))) - at_k)[:10]
    if direct:
        assert (np.array(rd.plans) == 2).any() and q[:, LC.LSQ_BATCHED].sum() > 0


def test_byte_by_byte(w):
    src, content = LC.small_stream(w, B)
    for count, interactive in ((1 << 20, False), (100, False), (7, True)):
        rd = E.EmuFedReaders(1, max_block=B, threads=1, direct=not interactive)
        drv = LC.driver(rd, [src], [list(range(1, len(src) + 1))])
        reads = (len(content) // min(count, 40) + 8) if interactive else len(LC.reads_to_the_end(len(content), count))
        wit = LC.check_reads(drv, w, [src], [[count]] * reads, interactive, B)
        LC.check_query(rd.query(), wit)
        assert wit[0].pos == len(src) and drv.calls > len(src) and rd.query()[0, LC.LSQ_BYTES_READ] == len(content)


def _counts(rng, n, calls, scale):
    return [[None if rng.random() < 0.07 else int(rng.choice([0, 1, 15, 16, 17, 1000, 4096, int(rng.integers(1, scale)), scale]))
             for _ in range(n)] for _ in range(calls)]


def _chunk_len(s):
    """a typical compressed chunk's length, for the cuts around C +- 8"""
    try:
        lay = LC.layout(s)
    except (AssertionError, IndexError):
        return 64
    return max([c[2] for c in lay] + [16])


@pytest.mark.parametrize("interactive,direct", [(False, False), (False, True), (True, False)], ids=["general", "direct", "interactive"])
def test_valid_streams_in_random_pieces(w, interactive, direct):
    rng = np.random.default_rng(31)
    srcs = valid_streams(w)
    rd = E.EmuFedReaders(len(srcs), max_block=65536, threads=8, direct=direct)
    drv = LC.driver(rd, srcs, [LC.random_ends(rng, len(s), _chunk_len(s)) for s in srcs])
    wit = LC.check_reads(drv, w, srcs, _counts(rng, len(srcs), 14, 30000) + [[1 << 20] * len(srcs)] * (0 if interactive else 2), interactive, 65536)
    q = rd.query()
    LC.check_query(q, wit)
    LC.check_code_timing(drv, wit)
    assert len(drv.starved) > len(srcs)
    if direct:
        assert (np.array(rd.plans) == 2).any() and np.array(rd.heads).any() and q[:, LC.LSQ_BATCHED].sum() > 0
    else:
        assert q[:, LC.LSQ_BATCHED].sum() == 0


@pytest.mark.parametrize("interactive,direct", [(False, False), (False, True), (True, False)], ids=["general", "direct", "interactive"])
def test_mutants_and_truncations_cut_at_random_places(w, interactive, direct):
    """the code equals the witness's, no later than the call that hands over the last byte the witness consumed; END_OF_STREAM from
    running out only with final"""
    rng = np.random.default_rng(32)
    srcs = damaged_streams(w)
    base = w.encode_stream(corpus.class_bytes("dickens", 20000, 6).tobytes(), False, 4096)
    for _ in range(16):
        m = bytearray(base)
        m[int(rng.integers(4, len(m)))] ^= 1 << int(rng.integers(0, 8))
        srcs.append(bytes(m))
    srcs += [base[:int(k)] for k in rng.integers(1, len(base), 8)]
    rd = E.EmuFedReaders(len(srcs), max_block=4096, threads=8, direct=direct)
    drv = LC.driver(rd, srcs, [LC.random_ends(rng, len(s), 1500) for s in srcs], with_layout=False)
    wit = LC.check_reads(drv, w, srcs, _counts(rng, len(srcs), 10, 9000) + [[1 << 20] * len(srcs)] * 2, interactive, 4096)
    LC.check_query(rd.query(), wit)
    LC.check_code_timing(drv, wit)
    assert sum(x.failed is not None for x in wit) > len(wit) // 3
    ran_out = [i for i, x in enumerate(wit) if x.failed == -1 and x.short_last]
    assert ran_out and all(drv.code_final[i] for i in ran_out)


def test_refused_chunk_spanning_several_pieces(w):
    """a chunk with U > maxBlockSize whose payload spans several pieces: BLOCK_SIZE in the call with the payload's last byte (its bytes
    are counted, not kept: the stash has no room for them), END_OF_STREAM if final comes first; the same for passes != 0"""
    text = corpus.class_bytes("xml", 9000, 3).tobytes()
    good = w.encode_stream(text[:1000], False, 1000)
    big = w.encode_stream(text, False, 16384)                     # one compressed chunk, U = 9000 > 1000
    raw = LC.varint(0) + LC.varint(5000) + bytes(5000)           # a stored one
    lay = LC.layout(good + big)
    passes = LC.varint(1 | 4) + LC.varint(900) + LC.varint(600) + bytes(600)
    for tail, code in ((big, -8), (raw, -8), (passes, -3)):
        src = good + tail
        p0 = len(good) + (LC.layout(tail)[0][1])                  # where the refused payload begins
        cuts = [len(good) // 2, p0 - 1, p0 + 10, p0 + 11, p0 + 300, len(src) - 1]
        srcs = [src, src, src[:len(src) - 5]]
        ends = [cuts + [len(src)], cuts + [len(src), len(src)], cuts[:-1] + [len(src) - 5]]
        for direct in (False, True):
            rd = E.EmuFedReaders(3, max_block=1000, threads=3, direct=direct)
            drv = LC.driver(rd, srcs, ends, with_layout=False)
            wit = LC.check_reads(drv, w, srcs, [[600] * 3, [5000] * 3, [10] * 3], False, 1000)
            assert [x.failed for x in wit] == [code, code, -1]
            assert drv.code_at[:2] == [len(src), len(src)] and drv.code_final == [True, False, True]
            # while the payload went by, need was what was left of it and nothing was delivered
            assert (0, len(src) - 1, 1) in drv.starved and (0, p0 + 300, len(src) - p0 - 300) in drv.starved
    assert lay


def _pin(w, nstreams, k, Bsz, topup=True):
    pairs = LC.full_chunk_streams(w, nstreams, k, Bsz, seed=5)
    srcs = [s for s, _ in pairs]
    ends = [LC.ends_inside_chunks(s, 1.5) for s in srcs]
    lays = [LC.layout(s) for s in srcs]
    for e, lay in zip(ends, lays):                                  # every piece but the last ends inside a chunk's payload
        assert len(e) >= 3 and all(any(p < x < p + c for _, p, c, _, _ in lay) for x in e[:-1])
    rd = E.EmuFedReaders(nstreams, max_block=Bsz, threads=4, direct=True, topup=topup, max_count=k * Bsz + 100)
    drv = LC.driver(rd, srcs, ends)
    wit = LC.check_reads(drv, w, srcs, [[k * Bsz + 100] * nstreams, [10] * nstreams], False, Bsz)
    assert all(x.pos == len(s) for x, s in zip(wit, srcs))
    return rd, drv, wit


def test_direct_path_pin(w):
    """streams of k full chunks fed in pieces of about 1.5 chunks that each end inside a chunk, read with one large count: every chunk
    goes through the batch decoder -- the chunk a piece cuts as row 0 of the next call, from the stash that piece's head completes"""
    rd, drv, wit = _pin(w, 3, 7, 4096)
    q = rd.query()
    LC.check_query(q, wit)
    assert (q[:, LC.LSQ_CHUNKS] == 7).all()
    assert (q[:, LC.LSQ_BATCHED] == q[:, LC.LSQ_CHUNKS]).all() and (q[:, LC.LSQ_HANDED_BACK] == 0).all() and (q[:, LC.LSQ_DIRECT] == 0).all()
    heads = np.array(rd.heads)
    assert (heads[1:len(drv.ends[0]) - 1] > 0).all()              # every call after the first began with a top-up


def test_without_the_top_up_the_general_reader_takes_the_cut_chunks(w):
    """the same streams with the top-up step left out: everything still reads correctly, but the chunks that a piece cuts are decoded
    by one wavefront per stream -- what test_direct_path_pin rules out"""
    rd, drv, wit = _pin(w, 2, 7, 4096, topup=False)
    q = rd.query()
    assert (q[:, LC.LSQ_BATCHED] < q[:, LC.LSQ_CHUNKS]).all()


def test_payload_flip_in_a_planned_chunk_and_both_ways_in_one_call(w):
    (good, content), = LC.full_chunk_streams(w, 1, 6, 4096, seed=9)
    lay = LC.layout(good)
    bad = bytearray(good)
    at = lay[2][1]
    bad[at:at + 3] = b"\xff\xff\xff"
    bad = bytes(bad)
    srcs = [good, bad, good, bad]
    cut = lay[4][1] + 5                                             # the first piece holds four whole chunks and a cut one
    ends = [[cut, len(s)] for s in srcs]
    rd = E.EmuFedReaders(4, max_block=4096, threads=4, direct=True)
    drv = LC.driver(rd, srcs, ends, with_layout=False)
    wit = LC.check_reads(drv, w, srcs, [[5 * 4096] * 4, [4096] * 4], False, 4096)
    assert [x.failed for x in wit] == [None, -4, None, -4]
    assert list(rd.plans[0]) == [2, 1, 2, 1]                        # served directly / handed back, in one call
    assert drv.code_at[1] == cut                                    # ... and the code came in that call
    q = rd.query()
    assert list(q[:, LC.LSQ_HANDED_BACK]) == [0, 1, 0, 1] and q[0, LC.LSQ_BATCHED] == 6 and q[1, LC.LSQ_BATCHED] == 0
    assert q[1, LC.LSQ_CODE] == -4 and q[1, LC.LSQ_CHUNKS] == 2    # the general reader delivered the two good chunks' bytes' chunks


def test_fed_and_whole_readers_agree_on_query(w):
    """fed readers against whole-source readers (k4_ls_read_kernel) on the same streams: Query() words 0-4 after every completed
    logical read"""
    import ctypes as C
    rng = np.random.default_rng(33)
    srcs = valid_streams(w)[::2]
    n = len(srcs)
    rd = E.EmuFedReaders(n, max_block=65536, threads=8, direct=True)
    drv = LC.driver(rd, srcs, [LC.random_ends(rng, len(s), _chunk_len(s)) for s in srcs])
    lib = E.lib()
    sb = int(lib.k4emu_lf_store_bytes(65536, 0))
    store = np.zeros(n * sb + 256, np.uint8)
    soff = (np.arange(n, dtype=np.uint64) * sb).astype(np.uint64)
    lens = np.array([len(s) for s in srcs], np.uint64)
    off = np.concatenate(([0], np.cumsum(lens[:-1]))).astype(np.uint64)
    src = np.frombuffer(b"".join(srcs), np.uint8).copy()
    p = lambda a: a.ctypes.data  # noqa: E731
    wit = [LC.TrackedReader(w, s, False, 65536) for s in srcs]
    for counts in _counts(rng, n, 10, 30000):
        c = np.array([-1 if x is None else x for x in counts], np.int64)
        got = drv.read(c, False)
        caps = np.maximum(c, 0)
        doff = np.concatenate(([0], np.cumsum(caps[:-1]))).astype(np.uint64)
        dst = np.zeros(int(caps.sum()) + 16, np.uint8)
        out = np.zeros(n, np.int64)
        lib.k4emu_lf_whole_call(65536, p(store), p(soff), p(src), p(off), p(lens), p(dst), p(doff), p(c), p(out), n, 0, 0, 4)
        for i in range(n):
            if c[i] >= 0:
                assert got[i] == wit[i].call(c[i]) == dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes()
        qw = np.zeros(n * 8, np.int64)
        lib.k4emu_lf_query(p(store), p(soff), p(qw), n, 1)
        LC.check_query(rd.query(), wit, qw.reshape(n, 8))
    assert C.sizeof(C.c_int64) == 8
