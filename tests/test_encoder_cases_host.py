"""The encoder case set of tests/encoder_cases.py, proven on the CPU before a GPU sees it: the oracle stays inside every slot, its
verdicts and bytes are the compiled reference's, the set holds enough accepted and enough rejected cases in every mode to show a
failure, and the kernel source under the wave emulator gives exactly what tests/test_gpu_encoder_routes.py asserts of the device
(the same `check`)."""
import numpy as np
import pytest

import encoder_cases as ec
from oracle_lib import REFERENCE_PRESENT, RefEngine

ROUNDS = [(m, f) for m in ec.MODES for f in ec.ROUNDS[m]]
ROUND_IDS = [f"{m}-{f}" for m, f in ROUNDS]


@pytest.fixture(scope="module")
def ref():
    try:
        return RefEngine()
    except FileNotFoundError as e:
        assert not REFERENCE_PRESENT, "the reference is here, so oracle/_ref must build"
        pytest.skip(str(e))


@pytest.fixture(scope="module")
def emu():
    from emu_lib import Emu
    return Emu()


def slot_mask(lay):
    off, cap = lay.dst_off.astype(np.int64), lay.dst_cap.astype(np.int64)
    return ec._mask(lay.arena.size, off, off + cap)


@pytest.mark.parametrize("mode,flags", ROUNDS, ids=ROUND_IDS)
def test_the_oracle_stays_inside_every_slot(oracle, mode, flags):
    """check(expect(oracle)) holds, and the expectation is itself what the contract promises: outside all slots the arena is the
    fill -- both guards of every slot, rejected ones included -- and so is an accepted slot behind its bytes (but for what an
    ALLOW_COPY raw copy leaves of the encoder's longer output, which the reference leaves too)"""
    cs, lay, exp = ec.prepared(mode, flags, oracle)
    ec.check(lay, exp, exp.want.copy(), exp.arena.copy(), f"{mode} oracle", src_after=lay.src.copy())
    assert (exp.arena[~slot_mask(lay)] == ec.FILL).all()
    for i in np.flatnonzero(~exp.rejected):
        a, cap, w = int(lay.dst_off[i]), int(lay.dst_cap[i]), int(exp.want[i])
        if w >= 0:
            assert (exp.arena[a + w:a + cap] == ec.FILL).all(), ec.describe(lay, int(i))
    assert exp.want.min() >= (-1 if not flags & ec.FLAG_ALLOW_COPY or ec.call_of(mode) != "encode" else -int(lay.src_len.max()))


@pytest.mark.parametrize("mode,flags", ROUNDS, ids=ROUND_IDS)
def test_the_case_set_cannot_hide_a_failure(oracle, mode, flags):
    """conditions on the inputs, from the oracle's results alone.  At least one case in eight is accepted (its bytes and slack are
    compared) and at least half are rejected (their guards are); every block has an accepted case and -- where its result leaves
    room for one: r >= 2, an envelope of a message that is not empty -- a rejected one with a capacity of at least 1; every tag
    occurs; what `comparable` masks beyond the inside of rejected slots -- the little the contract leaves open behind accepted
    ones -- is at most 2 % of the arena, the slots of blocks that segments may cut apart.  (Of the WHOLE arena the mask takes more
    than half: seven of the ladder's capacities lie just below r, so most of the arena is the inside of rejected slots; that
    share is printed, a small one cannot be asked of this ladder.)"""
    cs, lay, exp = ec.prepared(mode, flags, oracle)
    n, acc, rej = lay.n, int((~exp.rejected).sum()), int(exp.rejected.sum())
    masked = ~exp.keep
    inside_rejected = ec._mask(lay.arena.size, lay.dst_off[exp.rejected].astype(np.int64), (lay.dst_off.astype(np.int64) + lay.dst_cap)[exp.rejected])
    print(f"{mode} flags {flags}: {len(cs.blocks)} blocks, {n} cases: {acc} accepted ({acc / n:.2f}), {rej} rejected ({rej / n:.2f}); arena "
          f"{lay.arena.size} bytes, {masked.mean():.3f} of them masked, {(masked & ~inside_rejected).mean():.4f} outside rejected slots")
    assert acc * 8 >= n and rej * 2 >= n, (mode, acc, rej, n)
    assert not (masked & ~slot_mask(lay)).any(), "the mask reaches outside the slots"
    big = (lay.src_len >= ec.SEG_MIN) & ec.cuts_by_default(mode, flags)     # (blocks that segments may cut leave their whole slot open: counted apart)
    may_cut = ec._mask(lay.arena.size, lay.dst_off[big].astype(np.int64), (lay.dst_off.astype(np.int64) + lay.dst_cap)[big])
    assert (masked & ~inside_rejected & ~may_cut).mean() <= 0.02
    for b in range(len(cs.blocks)):
        mine = lay.block == b
        assert (mine & ~exp.rejected).any(), (mode, b, cs.block_tag[b])
        room = cs.blocks[b].size > 0 if ec.call_of(mode) != "encode" else ec.unlimited(mode, oracle, cs.blocks[b]) >= 2
        assert not room or (mine & exp.rejected & (lay.dst_cap >= 1)).any(), (mode, b, cs.block_tag[b])
    want_tags = {"edge", "text", "binary", "noise", "64k", "repeat", "ll-code", "ml-code", "search-limit", "dense", "big"} | \
                ({"cut"} if mode == "fast-seg" or ec.call_of(mode) != "encode" else set())
    assert set(cs.block_tag) == want_tags
    sizes = {b.size for b in cs.blocks}
    assert {0, 128, 65535, 65536, 65546, ec.LIMIT_64K} <= sizes                   # the thresholds every mode reaches
    assert ec.call_of(mode) == "encode" or any(ec.LIMIT_64K < n < ec.SEG_MIN for n in sizes)      # an envelope with byU32 tables that is not cut
    if flags & ec.FLAG_ALLOW_COPY and ec.call_of(mode) == "encode":      # U <= cap < r gives 0, and a raw copy happens
        u, cap = lay.src_len.astype(np.int64), lay.dst_cap.astype(np.int64)
        assert ((exp.want == 0) & (cap >= u) & (u > 0)).any() and (exp.want < 0).any()


BLOCK_MODES = ("fast", "fast-x32", "hc3", "hc9", "opt10")


@pytest.mark.parametrize("mode", BLOCK_MODES)
def test_oracle_verdicts_and_bytes_are_the_compiled_references(oracle, ref, mode):
    """the oracle travels to the GPU machine, the compiled reference does not: here compress_fast, compress_fast_x32 and
    compress_hc of the reference encode every (block, capacity) into the same arena -- equal returns for every case, equal
    bytes for every accepted one, and the reference too leaves everything outside the slots alone"""
    flags = ec.ROUNDS[mode][0]
    cs, lay, exp = ec.prepared(mode, flags, oracle)
    got = ec.expect(lay, oracle, flags, lib=ref.lib, prefix="k4ref_")
    ec.check(lay, exp, got.want, got.arena, f"{mode} compiled reference")


@pytest.mark.parametrize("high", [0, 1])
def test_wrap_expectation_is_the_transcribed_wrappers(oracle, ref, high):
    from legacy_witness import Witness
    w = Witness(ref)
    cs = ec.prepared("wrap", high, oracle)[0]
    for b in cs.blocks:
        assert ec.wrap_expected(oracle, b, bool(high)) == w.wrap(b.tobytes(), bool(high)), b.size


def emulate(emu, lay, run):
    arena, src = lay.arena.copy(), lay.src.copy()
    out = run(src, lay.src_off, lay.src_len, arena, lay.dst_off, lay.dst_cap)
    return out, arena, src


FAST_BUILDS = {
    "lds-table": lambda e, *a: e.encode_batch(*a, flags=ec.FLAG_RAW),
    "global-table": lambda e, *a: e.encode_batch(*a, flags=ec.FLAG_RAW, gtab=True),
    "28-known-bytes": lambda e, *a: e.encode_batch(*a, flags=ec.FLAG_RAW, more=True),
    "parse+emit": lambda e, *a: e.encode_parse_batch(*a, flags=ec.FLAG_RAW)[0],
    "parse inline+migrate+slots": lambda e, *a: e.encode_parse_batch(*a, flags=ec.FLAG_RAW, inline_emit=True, migrate=True, slot_recs=True)[0],
    "parse inline+queue+slots": lambda e, *a: e.encode_parse_batch(*a, flags=ec.FLAG_RAW, inline_emit=True, queue=True, slot_recs=True)[0],
}


@pytest.mark.parametrize("build", list(FAST_BUILDS))
def test_emulated_fast_kernels_on_the_case_set(emu, oracle, build):
    """the proof that the case set and its expectation are right for the kernel source: the three one-kernel encoders and three
    configurations of parse + emit under the wave emulator, held to the assertions of the GPU tests -- rejected slots included"""
    cs, lay, exp = ec.prepared("fast", ec.FLAG_RAW, oracle)
    out, arena, src = emulate(emu, lay, lambda *a: FAST_BUILDS[build](emu, *a))
    ec.check(lay, exp, out, arena, f"fast emulated {build}", src_after=src)


def test_emulated_allow_copy_on_the_case_set(emu, oracle):
    """k4_allow_copy_kernel behind the LDS-table encoder (LZ4Codec's mapping, as the launcher runs it) on the fast-copy set"""
    cs, lay, exp = ec.prepared("fast-copy", ec.FLAG_ALLOW_COPY, oracle)

    def run(src, soff, slen, arena, doff, dcap):
        out = emu.encode_batch(src, soff, slen, arena, doff, dcap, flags=ec.FLAG_ALLOW_COPY)
        return emu.allow_copy(src, soff, slen, arena, doff, dcap, out)
    out, arena, src = emulate(emu, lay, run)
    ec.check(lay, exp, out, arena, "fast-copy emulated", src_after=src)


def test_emulated_pickle_kernel_on_the_case_set(emu, oracle):
    """k4_pickle_kernel on the pickle set: -1 and an untouched neighbourhood below 5 + U, the oracle's envelope from there"""
    cs, lay, exp = ec.prepared("pickle", 0, oracle, cuts=False)           # (one wave per message: nothing is cut)
    out, arena, src = emulate(emu, lay, lambda *a: emu.pickle_batch(*a))
    ec.check(lay, exp, out, arena, "pickle emulated", src_after=src)


HC_EMU_FLAGS = {"hc3": (1 << 30) | (2 << 27), "hc9": 0, "opt10": 0}      # level 3 as the launcher runs it: records, four waves per block


@pytest.mark.parametrize("flags", [0, ec.FLAG_ALLOW_COPY], ids=["plain", "allow-copy"])
@pytest.mark.parametrize("mode", list(HC_EMU_FLAGS))
def test_emulated_hc_kernels_on_a_subset(emu, oracle, mode, flags):
    """the HC kernels under the emulator on the blocks of at most 4 KiB (every ninth of the search-limit blocks, which are the fast
    search's corner): chain, candidates and parse as the launcher runs them for such a batch, then k4_allow_copy_kernel in its round"""
    cs = ec.prepared(mode, flags, oracle)[0]
    nth = {b: k for k, b in enumerate(i for i, t in enumerate(cs.block_tag) if t == "search-limit")}
    sub = cs.subset([i for i, (b, _) in enumerate(cs.cases) if cs.blocks[b].size <= 4096 and nth.get(b, 0) % 9 == 0])
    lay = ec.layout(sub)
    exp = ec.expect(lay, oracle, flags)

    def run(src, soff, slen, arena, doff, dcap):
        out = emu.encode_hc_batch(src, soff, slen, arena, doff, dcap, level=ec.LEVEL[mode], flags=flags | HC_EMU_FLAGS[mode])
        return emu.allow_copy(src, soff, slen, arena, doff, dcap, out) if flags & ec.FLAG_ALLOW_COPY else out
    out, arena, src = emulate(emu, lay, run)
    print(f"{mode}: {lay.n} cases emulated")
    ec.check(lay, exp, out, arena, f"{mode} emulated", src_after=src)


def test_check_notices_what_it_is_there_for(oracle):
    """`check` on doctored copies of the oracle's own run: one byte in the front guard of a rejected slot, in the back guard of a
    zero-capacity slot, in the slack of an accepted slot, in an accepted block's bytes; one result never written, one wrong; one
    source byte changed -- each is reported, with the slot and the offset relative to it; a byte inside a rejected slot is not"""
    cs, lay, exp = ec.prepared("fast", ec.FLAG_RAW, oracle)
    off, cap = lay.dst_off.astype(np.int64), lay.dst_cap.astype(np.int64)
    rejected = int(np.flatnonzero(exp.rejected & (cap > 8))[0])
    empty = int(np.flatnonzero(cap == 0)[0])
    roomy = int(np.flatnonzero(~exp.rejected & (cap > exp.want + 4) & (exp.want > 4))[0])

    def doctored(at=None, result=None, source=None):
        got, arena, src = exp.want.copy(), exp.arena.copy(), lay.src.copy()
        if at is not None: arena[at] ^= 0x40
        if result is not None: got[result[0]] = result[1]
        if source is not None: src[source] ^= 1
        ec.check(lay, exp, got, arena, "doctored", src_after=src)

    doctored(at=off[rejected] + 3)                                     # undefined on failure: not compared
    for at, slot, rel in ((off[rejected] - 1, rejected, -1), (off[rejected] - ec.GUARD, rejected, -ec.GUARD), (off[rejected] + cap[rejected], rejected, cap[rejected]),
                          (off[empty], empty, 0), (off[empty] + ec.GUARD - 1, empty, ec.GUARD - 1), (off[roomy] + exp.want[roomy], roomy, exp.want[roomy]),
                          (off[roomy] + cap[roomy] - 1, roomy, cap[roomy] - 1), (off[roomy] + 2, roomy, 2)):
        with pytest.raises(AssertionError, match=rf"slot {slot} \(.*at offset {int(rel)} of the slot"):
            doctored(at=int(at))
    with pytest.raises(AssertionError, match="never written"):
        doctored(result=(rejected, ec.UNWRITTEN))
    with pytest.raises(AssertionError, match=f"results differ, first slot {roomy} "):
        doctored(result=(roomy, exp.want[roomy] - 1))
    with pytest.raises(AssertionError, match="source buffer changed"):
        doctored(source=17)


def test_route_witness_names_are_the_headers():
    """the binding's ENCODE_ROUTE_* constants and their names are enum k4lz4_encode_route of include/k4lz4.h, bit for bit, and a
    NULL context reports no route"""
    import os
    import re
    from k4os.compression.lz4_amd import _native as K
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "k4lz4.h")).read()
    enum = re.search(r"enum k4lz4_encode_route \{(.*?)\};", header, re.S).group(1)
    bits = dict((n, int(b)) for n, b in re.findall(r"K4LZ4_ENCODE_ROUTE_(\w+) = 1 << (\d+)", enum))
    assert len(bits) == len(K.ENCODE_ROUTE_NAMES) == 30 and "K4LZ4_ENCODE_ROUTE_NONE = 0" in enum
    for i, name in enumerate(K.ENCODE_ROUTE_NAMES):
        assert bits[name] == i and getattr(K, "ENCODE_ROUTE_" + name) == 1 << i, name
    assert K.encode_route_names(K.ENCODE_ROUTE_PARSE | K.ENCODE_ROUTE_CHUNKS) == "parse+chunks" and K.encode_route_names(0) == "none"
    assert K.load_library().k4lz4_last_encode_route(None) == K.ENCODE_ROUTE_NONE
