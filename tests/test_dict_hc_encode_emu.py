"""The HC dictionary encoder's kernels (k4lz4_dict_encode_hc.hpp) under the host wave emulator, on the whole shared list of cases
(tests/dict_hc_encode_cases.py) except the 4096-message call, at every level a case names: blocks byte for byte against the witness
(the system liblz4's LZ4_loadDictHC + LZ4_compress_HC_continue) and against the goldens recorded from it, the loaded tables against
liblz4's LZ4_streamHC_t and against their definition written down in Python, a seeded random set at levels 3, 4 and 9, and the
goldens themselves against a fresh recording."""
import functools
import os
import sys

import numpy as np
import pytest

import dict_hc_encode_cases as HC
import dict_hc_encode_emu as E
import dict_hc_encode_witness as W

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import record_dict_hc_goldens as G     # noqa: E402

PAIRS = [(c.name, lv) for c in HC.calls() if not c.big for lv in c.levels]
CALLS = [c.name for c in HC.calls() if not c.big]
needs_witness = pytest.mark.skipif(not W.available(), reason="liblz4 1.9.3 not present: the goldens stand in for it")


@functools.lru_cache(maxsize=None)
def golden(name):
    return next(c for c in G.load()["calls"] if c["name"] == name)


def call_of(name):
    return next(c for c in HC.calls() if c.name == name)


@functools.lru_cache(maxsize=None)
def emulated(name, level):
    """one run of the kernels per call and level, shared by the tests: (outLen, arena, dstOff, caps, heads, chain, kept, status)"""
    call = call_of(name)
    src, soff, slen, cap, doff, asz, idx, dct, dcoff, dclen = HC.pack(call, golden(name)["levels"][str(level)]["size"])
    dst = np.full(asz, 0xCD, np.uint8)
    out, heads, chain, kept, status = E.encode(src, soff, slen, dst, doff, cap, level, idx, dct, dcoff, dclen)
    return out, dst, doff, cap, heads, chain, kept, status


def test_every_call_has_a_golden_with_the_same_inputs():
    """a changed case is a failure until the goldens are recorded again, never a skip"""
    assert [c["name"] for c in G.load()["calls"]] == [c.name for c in HC.calls()]
    for c in HC.calls():
        g = golden(c.name)
        assert g["inputs_xxh32"] == G.inputs_hash(c), c.name
        assert sorted(g["levels"]) == sorted(str(lv) for lv in c.levels) and len(g["keptLen"]) == len(c.dicts)
        assert all(len(g["levels"][lv]["outLen"]) == len(c.msgs) for lv in g["levels"])


@needs_witness
def test_goldens_equal_a_fresh_recording():
    assert G.load() == G.record()


def test_case_list_covers_the_issue():
    assert [m.size for m in call_of("message_lengths").msgs] == list(HC.MESSAGE_LENGTHS)
    assert [d.size for d in call_of("dictionary_lengths").dicts] == list(HC.DICT_LENGTHS)
    assert call_of("long_message").msgs[0].size == 70000 and call_of("long_message").levels == (3, 9)
    assert "minus1" in call_of("caps").caps and "exact" in call_of("caps").caps
    assert len(call_of("ticket_rounds").msgs) == 4096 and len(set(call_of("interleaved").idx)) == 4
    assert len(call_of("periods").msgs) == 2 * len(HC.PERIODS)


@pytest.mark.parametrize("name,level", PAIRS)
def test_blocks_equal_goldens(name, level):
    call, g = call_of(name), golden(name)["levels"][str(level)]
    out, dst, doff, *_, status = emulated(name, level)
    assert status == 0
    assert out.tolist() == g["outLen"]
    for i in range(len(call.msgs)):
        if out[i] > 0:
            got = dst[int(doff[i]):int(doff[i]) + int(out[i])]
            assert G.xxh32(got) == g["xxh32"][i], (name, level, i)
            if str(i) in g["bytes"]:
                assert got.tobytes().hex() == g["bytes"][str(i)], (name, level, i)


@needs_witness
@pytest.mark.parametrize("name,level", PAIRS)
def test_blocks_equal_witness(name, level):
    call = call_of(name)
    out, dst, doff, cap, *_ = emulated(name, level)
    for i, (m, d) in enumerate(zip(call.msgs, call.idx)):
        r, want = W.encode(m, call.dicts[d], int(cap[i]), level)
        assert int(out[i]) == W.codec_result(m.size, r), (name, level, i)
        if out[i] > 0:
            assert dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() == want, (name, level, i)


@pytest.mark.parametrize("name,level", PAIRS)
def test_slots_are_written_up_to_outlen_only(name, level):
    """the guard bytes between the slots are intact, and so is everything behind outLen in a slot that was encoded"""
    call = call_of(name)
    out, dst, doff, cap, *_ = emulated(name, level)
    used = np.zeros(dst.size, bool)
    for i in range(len(call.msgs)):
        o = int(doff[i])
        used[o:o + (int(out[i]) if out[i] > 0 else int(cap[i]) if out[i] < 0 else 0)] = True
    assert (dst[~used] == 0xCD).all()


@pytest.mark.parametrize("name", CALLS)
def test_loaded_tables(name):
    """hashTable: all 32768 words; chainTable: the written slots k < D - 3 (unwritten ones are 0xFFFF in the reference, 0 in liblz4)"""
    call, g = call_of(name), golden(name)
    *_, heads, chain, kept, _ = emulated(name, call.levels[0])
    assert kept.tolist() == g["keptLen"]
    for d, dictionary in enumerate(call.dicts):
        want_heads, want_chain, written = W.reference_tables(dictionary)
        assert np.array_equal(heads[d], want_heads), (name, d)
        assert np.array_equal(chain[d][written], want_chain[written]) and (chain[d][~written] == 0xFFFF).all(), (name, d)
        assert list(G.table_hashes(heads[d], chain[d], int(kept[d]))) == [g["heads_xxh32"][d], g["chain_xxh32"][d]]
        if W.available():
            st = W.load_state(dictionary)
            assert np.array_equal(heads[d], st["hashTable"]) and np.array_equal(chain[d][written], st["chainTable"][written]), (name, d)


@pytest.mark.parametrize("name,level", PAIRS)
def test_blocks_decode_with_the_dictionary(name, level, oracle):
    call = call_of(name)
    out, dst, doff, *_ = emulated(name, level)
    for i, (m, d) in enumerate(zip(call.msgs, call.idx)):
        if out[i] > 0:
            r, back = oracle.decompress_using_dict(dst[int(doff[i]):int(doff[i]) + int(out[i])], m.size, call.dicts[d])
            assert r == m.size and back[:r].tobytes() == m.tobytes(), (name, level, i)


@needs_witness
@pytest.mark.parametrize("level", HC.LEVELS)
def test_cases_tell_the_external_arm_from_a_dictionary_in_front(level):
    """seam, tail3, zeros and the one- and two-byte periods: liblz4 writes other bytes when the same dictionary lies directly in front
    of the message, so an encoder that treats the dictionary as a prefix fails these cases"""
    picks = [("seam", 0), ("tail3", 0), ("zeros", 0), ("periods", 0), ("periods", 2)]
    for name, i in picks:
        call = call_of(name)
        m, d = call.msgs[i], call.dicts[call.idx[i]]
        ext = W.encode(m, d, HC.DC.bound(m.size), level)
        pre = W.encode(m, d, HC.DC.bound(m.size), level, prefix=True)
        assert ext != pre, (name, i, level)


def random_inputs():
    """240 seeded (dictionary, message) pairs: text, xml and runs, dictionary lengths 0 .. 9000, message lengths 13 .. 3000"""
    rng = np.random.default_rng(2024)
    text, xml = HC.synthetic("dickens", 120000, 5), HC.synthetic("xml", 120000, 5)
    out = []
    for k in range(240):
        base = (text, xml)[k % 2]
        dn = int(rng.choice([0, 2, 5, 40, 300, 2000, 9000]))
        ds = int(rng.integers(0, 60000))
        d = base[ds:ds + dn].copy()
        mn = int(rng.integers(13, 3000))
        m = HC.mix(d, base[70000:], mn, 5000 + k)
        if k % 5 == 0 and dn >= 40:        # a run of one byte across the seam
            run = int(rng.integers(3, 30))
            d[-run:] = 0x61
            m[:int(rng.integers(1, 200))] = 0x61
        out.append((d, m))
    return out


@needs_witness
@pytest.mark.parametrize("level", (3, 4, 9))
def test_random_inputs_equal_witness(level):
    pairs = random_inputs()
    call = HC.HcCall("random", [d for d, _ in pairs])
    for k, (_, m) in enumerate(pairs):
        call.add(m, k)
    src, soff, slen, cap, doff, asz, idx, dct, dcoff, dclen = HC.pack(call)
    dst = np.full(asz, 0xCD, np.uint8)
    out, *_, status = E.encode(src, soff, slen, dst, doff, cap, level, idx, dct, dcoff, dclen, workgroups=3)
    assert status == 0
    for i, (d, m) in enumerate(pairs):
        r, want = W.encode(m, d, int(cap[i]), level)
        assert int(out[i]) == r and dst[int(doff[i]):int(doff[i]) + r].tobytes() == want, (level, i, d.size, m.size)


def test_dictionary_index_outside_the_list_reports_minus_one():
    call = call_of("tile")
    src, soff, slen, cap, doff, asz, idx, dct, dcoff, dclen = HC.pack(call)
    idx = np.array([2, 1], np.int32)
    dst = np.full(asz, 0xCD, np.uint8)
    out, *_, status = E.encode(src, soff, slen, dst, doff, cap, 3, idx, dct, dcoff, dclen)
    assert out[0] == -1 and status == 4
    assert (dst[int(doff[0]):int(doff[1])] == 0xCD).all()
    assert out[1] == golden("tile")["levels"]["3"]["outLen"][1]
