"""The dictionary encoder's kernels (k4lz4_dict_encode.hpp) under the host wave emulator, on the whole shared list of cases
(tests/dict_encode_cases.py) except the 4096-message call: blocks byte for byte against the witness (the system liblz4's LZ4_loadDict +
LZ4_compress_fast_continue) and against the goldens recorded from it, the loaded tables word for word against liblz4's LZ4_stream_t
and against the definition written down in Python; and the goldens themselves against a fresh recording."""
import functools
import os
import sys

import numpy as np
import pytest

import dict_encode_cases as DC
import dict_encode_emu as E
import dict_encode_witness as W

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import record_dict_goldens as G     # noqa: E402

CALLS = [c.name for c in DC.calls() if not c.big]


@functools.lru_cache(maxsize=None)
def golden(name):
    return next(c for c in G.load()["calls"] if c["name"] == name)


def call_of(name):
    return next(c for c in DC.calls() if c.name == name)


@functools.lru_cache(maxsize=None)
def emulated(name):
    """one run of the three kernels per call, shared by the tests: (outLen, arena, dstOff, caps, tables, dictSize, status)"""
    call = call_of(name)
    src, soff, slen, cap, doff, asz, idx, dct, dcoff, dclen = DC.pack(call, golden(name)["size"])
    dst = np.full(asz, 0xCD, np.uint8)
    out, tables, kept, status = E.encode(src, soff, slen, dst, doff, cap, idx, dct, dcoff, dclen)
    return out, dst, doff, cap, tables, kept, status


def test_every_call_has_a_golden_with_the_same_inputs():
    """a changed case is a failure until the goldens are recorded again, never a skip"""
    names = [c["name"] for c in G.load()["calls"]]
    assert names == [c.name for c in DC.calls()]
    for c in DC.calls():
        assert golden(c.name)["inputs_xxh32"] == G.inputs_hash(c), c.name
        assert len(golden(c.name)["outLen"]) == len(c.msgs) and len(golden(c.name)["dictSize"]) == len(c.dicts)


def test_goldens_equal_a_fresh_recording():
    if not W.available():
        pytest.skip("liblz4 1.9.3 not present: the goldens stand in for it everywhere else")
    assert G.load() == G.record()


def test_case_list_covers_the_lengths():
    assert [m.size for m in call_of("message_lengths").msgs] == list(DC.MESSAGE_LENGTHS)
    assert [d.size for d in call_of("dictionary_lengths").dicts] == list(DC.DICT_LENGTHS)
    assert "minus1" in call_of("caps").caps and "exact" in call_of("caps").caps
    assert len(call_of("ticket_rounds").msgs) == 4096 and len(set(call_of("interleaved").idx)) == 4


@pytest.mark.parametrize("name", CALLS)
def test_blocks_equal_goldens(name):
    call, g = call_of(name), golden(name)
    out, dst, doff, cap, *_ , status = emulated(name)
    assert status == 0
    assert out.tolist() == g["outLen"]
    for i in range(len(call.msgs)):
        if out[i] > 0:
            got = dst[int(doff[i]):int(doff[i]) + int(out[i])]
            assert G.xxh32(got) == g["xxh32"][i], (name, i)
            if str(i) in g["bytes"]:
                assert got.tobytes().hex() == g["bytes"][str(i)], (name, i)
    assert sum(1 for o in g["outLen"] if 0 < o < 128) == len(g["bytes"])


@pytest.mark.parametrize("name", CALLS)
def test_blocks_equal_witness(name):
    if not W.available():
        pytest.skip("liblz4 1.9.3 not present: test_blocks_equal_goldens checks the same bytes")
    call = call_of(name)
    out, dst, doff, cap, *_ = emulated(name)
    for i, (m, d) in enumerate(zip(call.msgs, call.idx)):
        r, want = W.encode(m, call.dicts[d], int(cap[i]))
        assert int(out[i]) == W.codec_result(m.size, r), (name, i)
        if out[i] > 0:
            assert dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() == want, (name, i)


@pytest.mark.parametrize("name", CALLS)
def test_slots_are_written_up_to_outlen_only(name):
    """the guard bytes between the slots are intact, and so is everything behind outLen in a slot that was encoded"""
    call = call_of(name)
    out, dst, doff, cap, *_ = emulated(name)
    used = np.zeros(dst.size, bool)
    for i in range(len(call.msgs)):
        o = int(doff[i])
        used[o:o + (int(out[i]) if out[i] > 0 else int(cap[i]) if out[i] < 0 else 0)] = True
    assert (dst[~used] == 0xCD).all()


@pytest.mark.parametrize("name", CALLS)
def test_loaded_tables(name):
    call, g = call_of(name), golden(name)
    *_, tables, kept, _ = emulated(name)
    assert kept.tolist() == g["dictSize"]
    for d, dictionary in enumerate(call.dicts):
        assert np.array_equal(tables[d], DC.reference_table(dictionary)), (name, d)
        assert G.xxh32(tables[d].view(np.uint8)) == g["table_xxh32"][d]
        if W.available():
            st = W.load_state(dictionary)
            assert np.array_equal(tables[d], st["hashTable"]) and st["dictSize"] == int(kept[d]) and st["currentOffset"] == DC.K64


@pytest.mark.parametrize("name", CALLS)
def test_blocks_decode_with_the_dictionary(name, oracle):
    call = call_of(name)
    out, dst, doff, *_ = emulated(name)
    for i, (m, d) in enumerate(zip(call.msgs, call.idx)):
        if out[i] > 0:
            r, back = oracle.decompress_using_dict(dst[int(doff[i]):int(doff[i]) + int(out[i])], m.size, call.dicts[d])
            assert r == m.size and back[:r].tobytes() == m.tobytes(), (name, i)


def test_seam_block_is_the_external_arms():
    out, dst, doff, *_ = emulated("seam")
    block = dst[int(doff[0]):int(doff[0]) + int(out[0])].tobytes()
    assert block.startswith(DC.SEAM_BLOCK_START)
    if W.available():     # and not what the same bytes give as a contiguous prefix
        from oracle_lib import SystemLZ4
        both = np.concatenate([DC.u8(DC.SEAM_DICTIONARY), DC.u8(DC.SEAM_MESSAGE)])
        L = SystemLZ4().lib
        import ctypes as C
        st = L.LZ4_createStream()
        tmp = np.zeros(200, np.uint8)
        u8p = C.POINTER(C.c_uint8)
        L.LZ4_loadDict(C.c_void_p(st), both.ctypes.data_as(u8p), len(DC.SEAM_DICTIONARY))
        r = L.LZ4_compress_fast_continue(C.c_void_p(st), C.cast(both.ctypes.data + len(DC.SEAM_DICTIONARY), u8p), tmp.ctypes.data_as(u8p),
                                         len(DC.SEAM_MESSAGE), 200, 1)
        L.LZ4_freeStream(C.c_void_p(st))
        assert tmp[:r].tobytes().startswith(bytes([0xc9]) + b"ABCDEFGHIJKL" + bytes([0x0d, 0x00, 0xff, 0x01])) and tmp[:r].tobytes() != block


def test_dictionary_index_outside_the_list_reports_minus_one():
    call = call_of("seam")
    src, soff, slen, cap, doff, asz, idx, dct, dcoff, dclen = DC.pack(call)
    idx = idx.copy()
    idx[1], idx[2] = 3, -1
    dst = np.full(asz, 0xCD, np.uint8)
    out, _, _, status = E.encode(src, soff, slen, dst, doff, cap, idx, dct, dcoff, dclen)
    assert out[1] == -1 and out[2] == -1 and status == 4
    assert (dst[int(doff[1]):int(doff[3])] == 0xCD).all()
    assert out[0] == golden("seam")["outLen"][0] and out[3] == golden("seam")["outLen"][3]
