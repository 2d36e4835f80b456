"""The incremental frame readers against a dictionary set under the host wave emulator (no GPU): k4lz4_frame_reader_dict.hpp,
DESIGN.md 4.25.  The witness (tests/frame_reader_dict_witness.py: the reference's reader over the reference's compiled engine) is
pinned to tests/golden/frame_dict_cases.json first; then the emulated kernels are compared with it byte for byte and code for code.
Guard bytes surround every slot, store, source, piece and the set (tests/frame_reader_dict_emu.py checks them after every call)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import frame_dict_cases as FC                      # noqa: E402
import frame_feed_cases as FF                      # noqa: E402
import frame_reader_dict_cases as RC               # noqa: E402
import frame_reader_dict_emu as RE                 # noqa: E402
from frame_reader_dict_witness import DictWitnessReader   # noqa: E402

K64 = FC.K64
FRQ_FAST, FRQ_HANDED_BACK, FRQ_BYTES_READ, FRQ_PHASE = 6, 7, 0, 2


@pytest.fixture(scope="module")
def E():
    return FC.entries()


# ---- the witness ---------------------------------------------------------------------------------------------------------------
def test_witness_reads_every_case_as_the_golden_file_records_it(E):
    """one read of the whole content per frame: all 43 frames, the ten entries of lengths 0, 1, 3, 4, 100, 65535, 65536 and 70000.
    What liblz4 rejects is a code here, but for a wrong ContentLength, which the reference's reader (and so this one) does not compare;
    a target one byte short has no meaning for a reader that is asked for counts."""
    golden = FC.load()["cases"]
    assert len(FC.cases()) == 43 and len(golden) == 43
    assert sorted(set(e.size for e in E)) == [0, 1, 3, 4, 100, 4000, 65535, 65536, 70000] and len(E) == 10
    for c in FC.cases():
        w = DictWitnessReader(c.frame, None if c.null_set else E, FC.IDS, K64)
        got = w.read(RC.WHOLE)
        want = golden[c.name]["decoded"]
        if c.null_set or c.expect == FC.DICTIONARY:
            assert got == FC.DICTIONARY, c.name
        elif c.expect == FC.LENGTH:
            assert want == "rejected" and isinstance(got, bytes), c.name
        elif want == "rejected":
            assert got == c.expect and got in (FC.EOF, FC.HEADER_SUM, FC.BLOCK), (c.name, got)
        else:
            assert isinstance(got, bytes) and [len(got), FC.xxh32(got)] == want, (c.name, got if isinstance(got, int) else len(got))
            assert c.content is None or got == c.content, c.name
            assert w.read(1) == b"" and w.phase == 0 and w.bytes_read == want[0], c.name
        if FC.liblz4() is not None and not c.null_set and c.expect not in (FC.DICTIONARY, FC.LENGTH):
            live = FC.lz4f_decode(c.frame, E[c.entry].tobytes() if c.entry >= 0 else b"", RC.WHOLE)
            assert (live if live is not None else "rejected") == (got if isinstance(got, bytes) else "rejected"), c.name


# ---- counts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 7, 100, K64 - 1, K64, K64 + 1, RC.WHOLE])
def test_every_case_read_to_its_end(E, count):
    """every frame of the case list, one stream each, in reads of `count` bytes with every third read interactive and OPENs in
    between; the entry word follows the witness's frame"""
    src = [s for s in RC.case_sources() if s[2]]
    near = None if count >= 1000 else max(3 * count, 16)
    plans = [RC.plan_reads(s, True, E, count, near, mix=True) for _, s, _ in src]
    rd = RE.EmuDictReaders([s for _, s, _ in src], E, FC.IDS)
    RC.check_reads(rd, [RC.witness(s, True, E) for _, s, _ in src], RC.batch_plan(plans), [n for n, _, _ in src],
                   opens=np.random.default_rng(count), state=rd.entries)
    q = rd.query()
    for i, (name, s, _) in enumerate(src):
        w = RC.witness(s, True, E)
        while isinstance(w.read(RC.WHOLE), bytes) and not (w.pos == len(s) and w.phase == 0):
            pass
        assert q[i, FRQ_BYTES_READ] == w.bytes_read, name          # the kept bytes are never counted


def test_several_frames_per_source(E):
    """dictionary / plain / another entry / the same id twice, chained next to independent: the entry word follows the frames"""
    src = RC.multi_frame_sources()
    for count in (7, 50000, RC.WHOLE):
        plans = [RC.plan_reads(s, True, E, count, 24 if count == 7 else None) for _, s in src]
        rd = RE.EmuDictReaders([s for _, s in src], E, FC.IDS, fast=count == 50000)
        wits = [RC.witness(s, True, E) for _, s in src]
        RC.check_reads(rd, wits, RC.batch_plan(plans), [n for n, _ in src], state=rd.entries)
        assert wits[0].entries_seen == [6, None, 0] and wits[1].entries_seen == [0, 0] and wits[4].entries_seen == [6, 1, 7]
        assert all(w.failed is None and w.pos == len(s) for w, (_, s) in zip(wits, src))


# ---- defects -------------------------------------------------------------------------------------------------------------------
def test_header_defects_are_reported_by_open_and_by_read(E):
    src = RC.header_defects()
    names = [n for n, _ in src]
    for opens in (True, False):
        rd = RE.EmuDictReaders([s for _, s in src], E, FC.IDS)
        wits = [RC.witness(s, True, E) for _, s in src]
        if opens:
            got = rd.open()
            assert got == [w.open() for w in wits]
            assert got[names.index("unknown-id")] == FC.DICTIONARY
        RC.check_reads(rd, wits, [(np.full(len(src), 100, np.int64), False)] * 2, names, state=rd.entries)
        codes = {n: w.failed for n, w in zip(names, wits)}
        assert codes["unknown-id"] == FC.DICTIONARY and all(codes[f"dictid-byte{k}-flipped"] == FC.HEADER_SUM for k in range(4))
        assert codes["cut@0"] is None and all(codes[f"cut@{k}"] == FC.EOF for k in range(1, 20))


def test_an_offset_before_the_first_kept_byte_is_a_block_defect(E):
    src = RC.reach_sources(E)
    rd = RE.EmuDictReaders([s for _, s in src], E, FC.IDS)
    wits = [RC.witness(s, True, E) for _, s in src]
    RC.check_reads(rd, wits, [(np.full(len(src), 1000, np.int64), False)] * 3, [n for n, _ in src])
    for (name, _), w in zip(src, wits):
        assert w.failed == (FC.BLOCK if "before" in name else None), (name, w.failed)
    assert len(src) == 5 * 6 - 2                           # the entry of no bytes has no first kept byte from a first block


def test_a_null_set_is_the_plain_reader(E):
    """the same sources through the kernels of the plain calls and through frame_reader_emu's: bytes, codes and query words"""
    import frame_reader_emu as PE
    src = [s for _, s, _ in RC.case_sources()] + [s for _, s in RC.multi_frame_sources()]
    for fast in (False, True):
        a, b = RE.EmuDictReaders(src, None, None, fast=fast), PE.EmuReaders(src, K64, fast=fast)
        for counts in ([70000] * len(src), [K64] * len(src), [RC.WHOLE] * len(src)):
            c = np.array(counts, np.int64)
            assert a.read(c) == b.read(c)
        assert (a.query() == b.query()).all() and (a.entries() == -1).all()
        has_id = [len(s) > 4 and s[4] & 1 for s in src]
        assert sum(1 for i, h in enumerate(has_id) if h and a.query()[i, 3] == FC.DICTIONARY) >= 30


@pytest.mark.parametrize("fed", [False, True])
@pytest.mark.parametrize("fast", [False, True])
def test_a_set_without_the_stored_entry_fails_the_stream(E, fed, fast):
    """frames are opened on entry 9; the next call brings a set of two entries: K4LZ4_FRAME_DICTIONARY on both ways through a READ (the
    independent frame of full blocks would be planned), while a frame on entry 0 reads on"""
    src = [RC.by_name("hand-chain-first-kept-byte-second-block").frame, RC.fast_path_sources(E)[3][1], RC.by_name("lz4-indep-1blk-b0c0s0-e0").frame]
    zero, one, counts = np.zeros(3, np.int64), np.ones(3, np.int64), np.full(3, 3 * K64, np.int64)
    if fed:
        rd = RE.EmuDictFedReaders(3, E, FC.IDS, fast=fast)
        out, _, consumed, _ = rd.call(1, src, one, zero, False)
    else:
        rd = RE.EmuDictReaders(src, E, FC.IDS, fast=fast)
        out, _ = rd._call(1, zero, False)
    assert list(out) == [1, 1, 1] and list(rd.entries()) == [9, 9, 0]
    rd.dset = RE.EmuSet(E[:2], FC.IDS[:2])
    out = rd.call(0, [s[int(c):] for s, c in zip(src, consumed)], one, counts, False)[0] if fed else rd._call(0, counts, False)[0]
    assert list(out) == [FC.DICTIONARY, FC.DICTIONARY, 40000]
    assert list(rd.query()[:, FRQ_PHASE]) == [2, 2, 0] and list(rd.entries()) == [-1, -1, -1]


# ---- the fast path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fed", [False, True])
def test_fast_path_serves_full_dictionary_blocks_and_hands_back_a_short_one(E, fed):
    src = RC.fast_path_sources(E)
    names = [n for n, _, _ in src]
    n = len(src)
    count = 2 * K64 + K64 // 2
    wits = [RC.witness(s, True, E) for _, s, _ in src]
    if fed:
        raw = RE.EmuDictFedReaders(n, E, FC.IDS, fast=True)
        rd = FF.FedDriver(raw, [s for _, s, _ in src], [[len(s)] for _, s, _ in src])
    else:
        raw = rd = RE.EmuDictReaders([s for _, s, _ in src], E, FC.IDS, fast=True)
    RC.check_reads(rd, wits, [(np.full(n, count, np.int64), False)] * 4, names, state=raw.entries)
    q = raw.query()
    first = raw.plans[0]
    for i, (name, _, served) in enumerate(src):
        assert wits[i].failed is None and wits[i].pos == len(src[i][1]), name
        if served:
            assert first[i] == 2 and q[i, FRQ_FAST] >= 3 and q[i, FRQ_HANDED_BACK] == 0, (name, first[i], q[i])
        else:
            assert first[i] == 1 and q[i, FRQ_HANDED_BACK] >= 1, (name, first[i], q[i])


# ---- the fed readers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [RC.WHOLE, 100, 7, 1])
def test_fed_source_cut_at_every_byte(E, count):
    """one stream per cut of a two-frame source (chained on the hundred-byte entry, independent on entry 0; block checksums, content
    checksum, ContentLength): whenever the call over [0, k) starves, need == e - k, e the end of the field that holds byte k"""
    source, content, ends = RC.small_fed_source(E)
    import bisect
    cuts = list(range(len(source) + 1))
    n = len(cuts)
    raw = RE.EmuDictFedReaders(n, E, FC.IDS, fast=count == RC.WHOLE)
    drv = FF.FedDriver(raw, [source] * n, [[k, len(source)] for k in cuts], lambda i, u: ends[bisect.bisect_right(ends, u)])
    wits = [RC.witness(source, True, E) for _ in cuts]
    plan = RC.batch_plan([RC.plan_reads(source, True, E, count)] * n)
    RC.check_reads(drv, wits, plan, state=raw.entries)
    assert wits[0].failed is None and wits[0].bytes_read == len(content) and wits[0].entries_seen == [9, 0]
    starved_at = set(u for _, u, _ in drv.starved)
    assert set(range(1, 19)) <= starved_at                # every cut inside the first header starved there (0: nothing to stash)
    assert any(u == 16 and need == 3 for _, u, need in drv.starved)       # inside the DictID: the bytes that complete the header


def test_fed_defects_cut_at_random_places(E):
    rng = np.random.default_rng(41)
    src = [(n, s) for n, s, with_set in RC.case_sources() if with_set and [c for c in FC.cases() if c.name == n][0].expect is not None]
    src += RC.header_defects() + [x for x in RC.reach_sources(E) if "before" in x[0]]
    names, sources = [n for n, _ in src], [s for _, s in src]
    for interactive in (False, True):
        raw = RE.EmuDictFedReaders(len(src), E, FC.IDS)
        drv = FF.FedDriver(raw, sources, [FF.random_ends(rng, len(s), 64) if len(s) else [0] for s in sources])
        wits = [RC.witness(s, True, E) for s in sources]
        plan = [(np.full(len(src), c, np.int64), interactive) for c in (10, 1000, RC.WHOLE, RC.WHOLE, 5)]
        RC.check_reads(drv, wits, plan, names)
        FF.check_code_timing(drv, wits, names)
        assert sum(1 for w in wits if w.failed is not None) >= 40
