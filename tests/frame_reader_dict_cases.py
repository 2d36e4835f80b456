"""What the tests of the incremental frame readers with a dictionary set share, without a GPU and with one: the
sources -- the frames of tests/frame_dict_cases.py one per stream, sources of several frames made of them, header defects, frames of
full blocks for the fast path, a small two-frame source for the fed readers --, read plans that reach every block boundary with
small counts, and the comparison with frame_reader_dict_witness.DictWitnessReader.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import frame_dict_cases as FC
from frame_reader_dict_witness import DictWitnessReader

K64 = FC.K64
IDS = FC.IDS
WHOLE = 4 * K64 + 4096                          # above every content of the case list


def case_sources():
    """[(name, source, with a set)] -- every frame of the case list, one per stream"""
    return [(c.name, c.frame, not c.null_set) for c in FC.cases()]


def by_name(name):
    return [c for c in FC.cases() if c.name == name][0]


def multi_frame_sources():
    """[(name, source)]: two and three frames per source -- dictionary / plain / another entry / the same id twice, chained and
    independent next to each other, an entry of no bytes"""
    f = lambda n: by_name(n).frame  # noqa: E731
    a6, l0, p = f("lz4-indep-2blk-b1c1s1-e6"), f("lz4-linked-1blk-b0c1s0-e0"), f("plain-frame-in-dictset-call")
    h9, i5 = f("hand-chain-first-kept-byte-second-block"), f("lz4-indep-4blk-b1c0s0-e5")
    e1, l7 = f("hand-indep-empty-dictionary"), f("lz4-linked-same-bytes-entry7")
    return [("dict-plain-other", a6 + p + l0), ("same-id-twice", l0 + l0), ("plain-first", p + a6), ("chain-indep-chain", h9 + i5 + h9),
            ("empty-entry-between", a6 + e1 + l7), ("two-chained-entries", l7 + h9), ("plain-plain-dict", p + p + h9)]


def header_defects():
    """[(name, source)]: an unknown id, every DictID byte flipped (the checksum as it was), the source cut at every byte of the header
    -- of a header with ContentLength and DictID, 19 bytes"""
    good = by_name("lz4-indep-2blk-b1c1s1-e6").frame
    assert good[4] & 0x09 == 0x09
    out = [("unknown-id", by_name("hostile-unknown-dictid").frame)]
    for k in range(4):
        b = bytearray(good); b[14 + k] ^= 0x10
        out.append((f"dictid-byte{k}-flipped", bytes(b)))
    out += [(f"cut@{k}", good[:k]) for k in range(0, 20)]
    return out


def all_sources(E):
    """[(name, source)]: everything above that is read with the set, for the GPU tests"""
    return [(n, s) for n, s, with_set in case_sources() if with_set] + multi_frame_sources() + header_defects() + reach_sources(E)


def check_query(rd, wits, names):
    """bytes read, phase and code of rd.query() against the witnesses"""
    q = rd.query()
    for i, w in enumerate(wits):
        assert (int(q[i, 0]), int(q[i, 2]), int(q[i, 3])) == (w.bytes_read, w.phase, w.failed or 0), names[i]


def reach_sources(E):
    """[(name, source)]: per dictionary length (entries of 0, 1, 3, 4 and 100 bytes; with 65535 kept bytes and more no offset reaches
    further) and block mode, an offset at the first kept byte and one before it -- from the first block, and for chained frames from a
    second block behind 30 bytes of output"""
    rng = np.random.default_rng(17)
    fresh = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    out = []
    for entry in (1, 2, 3, 4, 9):
        kept = min(E[entry].size, K64)
        for indep in (True, False):
            for before in (0, 1):
                if kept + before == 0:
                    continue
                blocks = [(FC.seq(fresh(20), 20 + kept + before, 8) + FC.seq(fresh(12)), False)]
                model = FC.decode_model(blocks, E[entry].tobytes(), indep)
                assert (model is None) == bool(before)
                out.append((f"reach-len{kept}-{'indep' if indep else 'chain'}-{'before' if before else 'first'}",
                            FC.frame(blocks, IDS[entry], indep, bsum=True, content=model)))
        for before in (0, 1):
            blocks = [(FC.seq(fresh(30)), False), (FC.seq(fresh(10), 10 + 30 + kept + before, 8) + FC.seq(fresh(12)), False)]
            model = FC.decode_model(blocks, E[entry].tobytes(), False)
            assert (model is None) == bool(before)
            out.append((f"reach-len{kept}-chain-second-{'before' if before else 'first'}", FC.frame(blocks, IDS[entry], False, content=model)))
    assert len({n for n, _ in out}) == len(out)
    return out


def full_block(rng, back, lit=16):
    """a compressed block of exactly 64 KiB: `lit` fresh bytes, one match `back` bytes before them that runs to 12 bytes from the end"""
    fresh = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    return FC.seq(fresh(lit), lit + back, K64 - lit - 12) + FC.seq(fresh(12))


def fast_path_sources(E):
    """[(name, source, served)]: independent dictionary frames of full 64 KiB blocks, three and more each, every block reaching into
    the dictionary; served False: a short block inside the first read of 2.5 blocks (the fast path hands the stream back)"""
    rng = np.random.default_rng(23)
    out = []
    for k, (entry, nblk, bsum, csum) in enumerate(((0, 4, True, True), (6, 3, False, True), (5, 5, True, False), (9, 3, False, False))):
        kept = min(E[entry].size, K64)
        blocks = [(full_block(rng, int(rng.integers(1, kept + 1))), False) for _ in range(nblk)]
        model = FC.decode_model(blocks, E[entry].tobytes(), True)
        out.append((f"full-e{entry}-{nblk}blk", FC.frame(blocks, IDS[entry], True, bsum=bsum, content=model if csum else None), True))
    blocks = [(full_block(rng, 500), False), (FC.seq(b"short block" * 9), False), (full_block(rng, 900), False), (full_block(rng, 70), False)]
    out.append(("short-block-inside", FC.frame(blocks, IDS[0], True, bsum=True, content=FC.decode_model(blocks, E[0].tobytes(), True)), False))
    raw = [(full_block(rng, 300), False), (rng.integers(0, 256, K64, dtype=np.uint8).tobytes(), True), (full_block(rng, 40), False)]
    out.append(("raw-full-block", FC.frame(raw, IDS[7], True, bsum=True, content=FC.decode_model(raw, E[7].tobytes(), True)), True))
    return out


def small_fed_source(E):
    """(source, content, field ends): a chained frame on the hundred-byte entry and an independent one on entry 0, both with block
    checksums, content checksum and ContentLength, two blocks each, a few hundred bytes in all"""
    rng = np.random.default_rng(29)
    fresh = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    frames, content, ends, at = [], b"", [], 0
    for entry, indep, blocks in ((9, False, [(FC.seq(fresh(20), 20 + 60, 30) + FC.seq(fresh(12)), False),
                                             (FC.seq(fresh(8), 8 + 62 + 90, 25) + FC.seq(fresh(12)), False)]),
                                 (0, True, [(FC.seq(fresh(10), 10 + 3000, 50) + FC.seq(fresh(12)), False), (fresh(40), True)])):
        model = FC.decode_model(blocks, E[entry].tobytes(), indep)
        f = FC.frame(blocks, IDS[entry], indep, clen=len(model), bsum=True, content=model)
        ends += [at + 4, at + 6, at + 19]
        p = at + 19
        for payload, _ in blocks:
            ends += [p + 4, p + 4 + len(payload) + 4]
            p += 4 + len(payload) + 4
        ends += [p + 4, p + 8]
        assert p + 8 == at + len(f)
        at += len(f)
        frames.append(f)
        content += model
    ends.append(at + 4)                                    # the magic of a frame that might follow
    source = b"".join(frames)
    assert len(source) < 1024
    return source, content, ends


# ---- read plans and the comparison ---------------------------------------------------------------------------------------------
def witness(source, with_set, E, max_block=K64):
    return DictWitnessReader(source, E if with_set else None, IDS, max_block)


def plan_reads(source, with_set, E, count, near=None, mix=False):
    """[(count, interactive)] that reads `source` to its end with reads of `count` bytes (two more behind the end).  near: content
    more than `near` bytes from both ends of its block is crossed by one large read, so that small counts reach every block boundary,
    EndMark and frame boundary without tens of thousands of calls.  mix: every third read is interactive."""
    w = witness(source, with_set, E)
    plan = []
    while len(plan) < 4000:
        c = count
        if near is not None and w.decoded > near and w.block_len - w.decoded >= near:
            c = w.decoded - near
        inter = mix and len(plan) % 3 == 2
        r = w.read(c, inter)
        plan.append((c, inter))
        if isinstance(r, int) or (not r and w.pos == len(source) and w.phase == 0):
            break
    return plan + [(count, False), (count, False)]


def batch_plan(plans):
    """per-stream plans -> [(counts per stream, interactive)] of one batch: calls are grouped by their flag, a stream whose next read
    has the other flag, or whose plan is over, sits the call out"""
    at = [0] * len(plans)
    out = []
    while any(a < len(p) for a, p in zip(at, plans)):
        flag = next(p[a][1] for a, p in zip(at, plans) if a < len(p))
        counts = np.full(len(plans), -1, np.int64)
        for i, (a, p) in enumerate(zip(at, plans)):
            if a < len(p) and p[a][1] == flag:
                counts[i] = p[a][0]
                at[i] += 1
        out.append((counts, flag))
    return out


def check_reads(reader, wits, plan, names=None, opens=None, state=None):
    """drives reader.read(counts, interactive) -> [bytes | code | None] and the witnesses through the plan and compares every call byte
    for byte and code for code.  opens: a random generator -- an OPEN on a random subset of the streams in front of every fourth call,
    compared too.  state(): the readers' entry per stream (-1: none), compared with the witnesses' after every call."""
    for call, (counts, interactive) in enumerate(plan):
        if opens is not None and call % 4 == 1:
            which = set(int(i) for i in np.flatnonzero(opens.random(len(wits)) < 0.4))
            got = reader.open(which)
            assert got == [w.open() if i in which else None for i, w in enumerate(wits)], call
        got = reader.read(counts, interactive)
        for i, w in enumerate(wits):
            tag = (call, i, names[i] if names else None, int(counts[i]), interactive)
            if counts[i] < 0:
                assert got[i] is None, tag
                continue
            want = w.read(int(counts[i]), interactive)
            if isinstance(want, int):
                assert got[i] == want, (tag, want, got[i] if isinstance(got[i], int) else len(got[i]))
                continue
            assert not isinstance(got[i], int), (tag, got[i], len(want))
            assert got[i] == want, (tag, len(got[i]), len(want))
        if state is not None:
            have = state()
            for i, w in enumerate(wits):
                want = -1 if (w.phase != 1 or w.entry is None) else w.entry
                assert have[i] == want, (call, i, names[i] if names else None, int(have[i]), want)
