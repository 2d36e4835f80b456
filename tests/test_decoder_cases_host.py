"""The decoder case set of tests/decoder_cases.py, proven on the CPU before a GPU sees it: the oracle's verdicts are the compiled
reference's, the set holds enough accepted, rejected and long streams in every mode to show a failure, and the kernel source
under the wave emulator -- one wave per block and the two-waves-per-block route -- gives exactly what
tests/test_gpu_decoder_variants.py asserts of the device (the same `check`)."""
import ctypes as C

import numpy as np
import pytest

import decoder_cases as dc
from oracle_lib import REFERENCE_PRESENT, RefEngine


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


def _ref_unpickle(ref, lay):
    """LZ4Pickler.Unpickle(source, output) put together from the reference's own pieces: its header reader
    (LZ4Pickler.unpickle.cs:131-148) and its LZ4_decompress_safe behind LZ4Codec.Decode's mapping (LZ4Codec.cs:104-115)"""
    arena = lay.arena.copy()
    out = np.zeros(lay.n, np.int32)
    u8p = C.POINTER(C.c_uint8)
    for i in range(lay.n):
        a, n, cap = int(lay.src_off[i]), int(lay.src_len[i]), int(lay.dst_cap[i])
        p = lay.src[a:a + n]
        if n == 0:
            continue
        rc, off, rl, compressed, _ = ref.unpickle_header(p.tobytes())
        if rc < 0 or rl < 0 or rl != cap:
            out[i] = -1
            continue
        d = int(lay.dst_off[i])
        if not compressed:
            arena[d:d + n - off] = p[off:]
            out[i] = rl
            continue
        r = -1
        if n - off > 0:
            r = ref.lib.k4ref_decompress_safe(C.cast(lay.src.ctypes.data + a + off, u8p), C.cast(arena.ctypes.data + d, u8p), n - off, cap)
            r = -1 if r <= 0 else r
        else:
            r = 0
        out[i] = r if r == rl else -1
    return out, arena


@pytest.mark.parametrize("mode", dc.MODES)
def test_oracle_verdicts_are_the_compiled_references(oracle, ref, mode):
    """The oracle travels to the GPU machine, the compiled reference does not: here the case set is pinned to the reference
    itself.  Both decode every case into its slot of the same 0xCD-filled arena: the return values are equal for every stream and
    the decoded bytes for every accepted one whose bytes are defined.  Defined is: the oracle decodes the same bytes into a target
    that held zeros (a match at offset 0 leaves what the target held; the reference's copy loops and the oracle's differ there)."""
    cs, lay, want, want_arena = dc.prepared(mode, oracle)
    got, got_arena = _ref_unpickle(ref, lay) if mode == "unpickle" else dc.expect(lay, ref.lib, "k4ref_")
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (mode, bad[:5], got[bad[:5]], want[bad[:5]])
    zeroed = dc.layout(cs, fill=0)
    other, other_arena = dc.expect(zeroed, oracle.lib)
    assert np.array_equal(other, want)
    compared = 0
    for i in np.flatnonzero(want > 0):
        a = int(lay.dst_off[i])
        if np.array_equal(other_arena[a:a + want[i]], want_arena[a:a + want[i]]):
            compared += 1
            assert np.array_equal(got_arena[a:a + want[i]], want_arena[a:a + want[i]]), (mode, int(i))
    print(f"{mode}: {int((want > 0).sum())} accepted streams, the bytes of {compared} are defined and equal the reference's")
    assert compared >= 0.9 * (want > 0).sum()
    outside = ~lay.inside
    assert np.array_equal(want_arena[outside], lay.arena[outside]) and np.array_equal(got_arena[outside], lay.arena[outside])


@pytest.mark.parametrize("mode", dc.MODES)
def test_the_case_set_cannot_hide_a_failure(oracle, mode):
    """a condition on the inputs, from the oracle alone: enough mutants the oracle accepts (their bytes are compared), enough it
    rejects (their guards and error positions are), enough streams that wrap the pair kernels' four pipe slots"""
    cs, lay, want, _ = dc.prepared(mode, oracle)
    mutant = cs.mutant
    accepted, rejected = int((mutant & (want > 0)).sum()), int((mutant & (want < 0)).sum())
    long_streams = sum(1 for c, _, _ in cs.cases if c.size > dc.LONG_SEQUENCES * 3 and dc.sequences_parsed(c) > dc.LONG_SEQUENCES)
    print(f"{mode}: {len(cs.cases)} cases, {int(mutant.sum())} mutants: {accepted} accepted / {rejected} rejected; "
          f"{long_streams} streams of more than {dc.LONG_SEQUENCES} sequences; arena {lay.arena.size} bytes")
    assert accepted >= 60 and rejected >= 400 and long_streams >= 20, (mode, accepted, rejected, long_streams)
    for kind in dc.MUTATIONS:
        assert cs.tags.count(kind) > 0, (mode, kind)


def run_emulated(emu, lay):
    arena = lay.arena.copy()
    flags = dc.FLAGS[lay.mode]
    if lay.mode in ("plain", "partial"):
        out = emu.decode_batch(lay.src, lay.src_off, lay.src_len, arena, lay.dst_off, lay.dst_cap, flags=flags)
    elif lay.mode == "dict":
        out = emu.decode_dict_batch(lay.src, lay.src_off, lay.src_len, arena, lay.dst_off, lay.dst_cap, arena, lay.dict_off, lay.dict_len, flags=flags)
    else:
        out = emu.unpickle_batch(lay.src, lay.src_off, lay.src_len, arena, lay.dst_off, lay.dst_cap)
    return out, arena


@pytest.mark.parametrize("pair", [False, True], ids=["one-wave", "pair"])
@pytest.mark.parametrize("mode", dc.MODES)
def test_emulated_kernels_on_the_case_set(emu, oracle, mode, pair):
    """the proof that the case set and its expectations are right for the kernel source: k4_decode_kernel / k4_unpickle_kernel and
    k4_decode_pair_kernel / k4_unpickle_pair_kernel under the wave emulator, held to the assertions of the GPU tests"""
    cs, lay, want, want_arena = dc.prepared(mode, oracle)
    emu.pair = pair
    try:
        got, got_arena = run_emulated(emu, lay)
    finally:
        emu.pair = False
    dc.check(lay, want, want_arena, got, got_arena, f"{mode} emulated pair={pair}")
