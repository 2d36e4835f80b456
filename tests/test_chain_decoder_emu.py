"""Many open ILZ4Decoders (k4lz4_chain_decoder.hpp) under the host wave emulator against the witness: the whole case list and the
mutants, with guard bytes around every store, every drain slot and every source (chain_decoder_emu.EmuDecoders checks them after
every launch).  What runs is the kernel the library launches: the pair form, two waves per stream."""
import pytest

import chain_decoder_cases as K
import chain_decoder_witness as W
from chain_decoder_emu import EmuDecoders


@pytest.mark.parametrize("k", range(len(K.BUILDERS)), ids=K.case_ids())
def test_case_against_the_witness(k):
    _, settings, calls = K.case(k)
    K.same(K.play(W.WitnessDecoders(settings), calls), K.play(EmuDecoders(settings), calls))


def undefined_mutants(settings, calls):
    """the witness's transcripts, and the mutants whose bytes depend on what lay behind the decoder's index (a match with offset 0,
    SURVEY.md 8a): the reference leaves those bytes undefined"""
    a = K.play(W.WitnessDecoders(settings), calls, fill=0x00)
    b = K.play(W.WitnessDecoders(settings), calls, fill=0xFF)
    K.same(a, b, skip_bytes=range(len(settings)))                       # results and codes never depend on it
    skip = {i for x, y in zip(a, b) for i in range(len(settings)) if x[3][i] != y[3][i] or x[4][i] != y[4][i]}
    assert len(skip) <= 0.02 * len(settings), f"{len(skip)} of {len(settings)} mutants left out of the byte comparison"
    return a, skip


def test_mutants_against_the_witness():
    settings, calls = K.mutants()
    want, skip = undefined_mutants(settings, calls)
    codes = [c for c in want[1][2] if c < 0]
    assert 30 < len(codes) < K.N_MUTANTS - 30                           # the mutations reach both outcomes
    K.same(want, K.play(EmuDecoders(settings), calls), skip_bytes=skip)


def test_a_store_that_was_never_reset():
    e = EmuDecoders([(1, 1024, 0), (0, 1024, 0)])
    at = int(e.store_off[0])
    e.store[at:at + 256] = 0xA5                                          # as allocated
    rec_out, out_len, _ = e.run([[(False, b"\x00", 0), (False, b"\x00", 0)], [(True, b"abc", 0)]])
    assert rec_out == [[W.NO_DECODER, W.NOT_RUN], [3]] and out_len == [W.NO_DECODER, 3]
    assert e.drain([0, -3], [0, 3]) == [W.NO_DECODER, b"abc"] and e.query()[0, 4] == W.NO_DECODER
