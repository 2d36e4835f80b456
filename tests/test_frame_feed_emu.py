"""The fed frame reader's kernels (k4lz4_frame_feed.hpp: k4_fr_feed_kernel and the fast path's plan / commit for pieces) under the
host wave emulator (frame_feed_emu.py).  Every test drives logical reads (frame_feed_cases.FedDriver) and compares them with
frame_reader_witness.WitnessReader over the WHOLE source; the driver holds every raw call to the contract (consumed, need, final),
and guard bytes around every slot, store and piece are checked at every call."""
import numpy as np
import pytest

import frame_feed_cases as FC
import frame_feed_emu as E
import frame_reader_cases as K
from test_frame_layer import LZ4F

K64 = 65536


@pytest.mark.parametrize("count,near,fast", [(1 << 20, None, False), (1 << 20, None, True), (100, 250, False), (100, 250, True),
                                             (7, 40, False), (1, 16, False)],
                         ids=["whole", "whole-fast", "100", "100-fast", "7", "1"])
def test_every_single_cut(count, near, fast):
    """the small source cut at every byte position k into [0, k) and [k, end) final, one stream per k, read to its end by logical
    reads of `count` bytes.  Whenever the call over [0, k) starves, consumed == srcLen and need == e - k, e the end of the field that
    holds byte k (FedDriver asserts both from the layout).  Under the emulator a stream-call costs about 0.2 ms, so the small reads
    cross the middle of the two 64 KiB blocks' content with one large read each (reads_to_the_end, near); every read within `near`
    bytes of a block's ends, an EndMark or a frame boundary has the stated count."""
    src, content = FC.small_source()
    ks = list(range(len(src) + 1))
    sources = [src] * len(ks)
    rd = E.EmuFedReaders(len(ks), max_block=K64, threads=8, fast=fast)
    drv = FC.FedDriver(rd, sources, [[k, len(src)] for k in ks], FC.field_end_fn(sources))
    plan = FC.reads_to_the_end(src, count, len(ks), near, FC.small_content_ends())
    wit = K.check_reads(drv, sources, plan, [f"k{k}" for k in ks], max_block=K64)
    q = rd.query()
    for i, w in enumerate(wit):
        assert (int(q[i, 0]), int(q[i, 2])) == (w.bytes_read, w.phase) == (len(content), 0), ks[i]
    # every cut that lies inside the source starved once at k with everything in front of it consumed
    at_k = {k for i, k, _ in [(i, u, n) for i, u, n in drv.starved] if k == ks[i]}
    assert at_k >= set(range(1, len(src))), sorted(set(range(1, len(src))) - at_k)[:10]
    if fast:
        served = np.array(rd.plans)
        assert (served == 2).any() and q[:, 6].sum() > 0


def test_byte_by_byte():
    src, content = FC.small_source()
    for count in (1 << 20, 70_000):
        rd = E.EmuFedReaders(1, max_block=K64, threads=1)
        drv = FC.FedDriver(rd, [src], [list(range(1, len(src) + 1))], FC.field_end_fn([src]))
        wit = K.check_reads(drv, [src], FC.reads_to_the_end(src, count, 1))
        assert rd.query()[0, 0] == wit[0].bytes_read == len(content) and drv.calls > len(src)


@pytest.mark.parametrize("fast", [False, True], ids=["general", "fast"])
def test_random_pieces(fast):
    rng = np.random.default_rng(11)
    srcs = [s for s in K.valid_sources(LZ4F(), big=False) if not s[0].startswith(("indep-b7", "linked-b7", "linked-raw-b7", "linked-b6"))]
    srcs += [(n, s, None) for n, s in K.quirk_sources()]
    names, sources = [s[0] for s in srcs], [s[1] for s in srcs]
    bs_of = [FC.block_size_of(n) for n in names]
    rd = E.EmuFedReaders(len(sources), threads=8, fast=fast)
    drv = FC.FedDriver(rd, sources, [FC.random_ends(rng, len(s), b) for s, b in zip(sources, bs_of)])
    plan = K.read_plan(np.random.default_rng(5), len(sources), bs_of, calls=6, top=400_000)
    wit = K.check_reads(FC.OpenMixer(drv, sources, rng), sources, plan, names)
    q = rd.query()
    for i, w in enumerate(wit):
        assert (int(q[i, 0]), int(q[i, 2]), int(q[i, 3])) == (w.bytes_read, w.phase, w.failed or 0), names[i]
        if srcs[i][2] is not None:
            assert w.bytes_read == len(srcs[i][2]), names[i]
    FC.check_code_timing(drv, wit, names)
    assert len(drv.starved) > len(sources)
    if fast:
        served = np.array(rd.plans)
        assert (served == 2).any() and (served == 1).any() and q[:, 6].sum() > 0 and q[:, 7].sum() > 0
    else:
        assert q[:, 6].sum() == 0


def test_fast_path_takes_whole_records_and_stashes_the_tail():
    """full 64 KiB blocks fed in pieces of 2 records plus 1000 bytes: the fast path serves the whole records of each piece and leaves
    the read starved with the tail in the stash; the general reader finishes that record; a short block inside a piece is handed back"""
    c = K.corpus.class_bytes("dickens", 6 * K64, 6).tobytes()
    regular = K.indep_frame(c, K64, True, True)
    short_mid = K.frame_of([K.compress(c[:K64]), K.compress(c[K64:K64 + 5000]), K.compress(c[2 * K64:3 * K64])], [False] * 3,
                           c[:K64] + c[K64:K64 + 5000] + c[2 * K64:3 * K64], K64, False, True, True)
    sources = [regular, short_mid]
    info = K.F.parse_frame(regular)
    two = info.block_off[2] - 4                                    # the header and two records
    ends = [[two + 1000, len(regular)], [len(short_mid)]]
    rd = E.EmuFedReaders(2, max_block=K64, threads=2, fast=True)
    drv = FC.FedDriver(rd, sources, ends, FC.field_end_fn(sources))
    wit = K.check_reads(drv, sources, [(np.array([1 << 20, 2 * K64], np.int64), False)] + [(np.full(2, 1 << 20, np.int64), False)] * 3,
                        ["regular", "short-middle"], max_block=K64)
    assert rd.plans[0].tolist() == [2, 1] and drv.starved[0] == (0, two + 1000, FC.field_end_fn(sources)(0, two + 1000) - two - 1000)
    q = rd.query()
    assert q[0, 6] >= 2 and q[0, 7] == 0 and q[1, 7] >= 1 and [w.bytes_read for w in wit] == [6 * K64, 2 * K64 + 5000]


def test_defects_come_when_their_bytes_do():
    rng = np.random.default_rng(3)
    c = K.corpus.class_bytes("xml", 150_000, 2).tobytes()
    bases = [K.indep_frame(c, K64, True, True, True), LZ4F().compress(np.frombuffer(c, np.uint8), 4, True, True, False, False)]
    for base in bases:
        muts = K.structural_mutants(base) + [(n, s) for n, s, _ in K.payload_mutants(base, rng)]
        names, sources = [n for n, _ in muts], [s for _, s in muts]
        loose = [None] * len(sources)
        if base is bases[1]:                                       # no block checksums: a flipped payload byte may decode to other bytes
            info = K.F.parse_frame(base)
            for i, (n, s) in enumerate(muts):
                if n.startswith("flip@"):
                    at = int(n[5:])
                    loose[i] = max(k for k, off in enumerate(info.block_off) if off <= at) * K64
        rd = E.EmuFedReaders(len(sources), max_block=K64, threads=8)
        drv = FC.FedDriver(rd, sources, [FC.random_ends(rng, len(s), K64) for s in sources])
        plan = [(np.array([int(rng.choice([0, 7, K64 - 1, K64, K64 + 1, 100_000])) for _ in sources], np.int64), False) for _ in range(4)]
        plan += [(np.full(len(sources), 1 << 20, np.int64), False)] * 3
        wit = K.check_reads(drv, sources, plan, names, max_block=K64, loose_from=loose)
        assert sum(w.failed is not None for w in wit) > len(wit) // 2
        FC.check_code_timing(drv, wit, names)
        # truncated sources starve before the final piece and fail in it
        cuts = [i for i, n in enumerate(names) if n.startswith("cut@") and wit[i].failed == -1]
        assert cuts and all(drv.code_final[i] for i in cuts)
