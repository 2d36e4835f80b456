"""Chained encoders opened from a dictionary, the host half without a GPU: k4lz4_chain_encoder_open_plan against the
witness's counters for every dictionary length and kind, the record model and the block tables continued from the primed record
against the table codecs (LZ4_loadDict / LZ4_loadDictHC transcribed onto them), and the committed goldens against the live witness."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from k4os.compression.lz4_amd import _native, encoders as E
import chain_prime_cases as PC
import chain_prime_witness as PW
from chain_encoder_witness import kind_of
from test_chain_encoder_host import plan, table_rows, model_rows, random_records

K1, K64 = 1024, 65536
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_prime_cases.json")


def open_plan(rec, dict_len):
    lib = _native.load_library()
    out = E.ChainEncoderRecord.from_buffer_copy(rec)
    return lib.k4lz4_chain_encoder_open_plan(C.byref(out), int(dict_len)), out


def counters(enc, codec, kind):
    return (enc.index, enc.pointer, codec.dict_size if kind == 2 else 0, codec.cur if kind == 2 else 0)


@pytest.mark.parametrize("level", PC.LEVELS)
@pytest.mark.parametrize("dict_len", PC.DICT_LENGTHS)
def test_open_plan_equals_the_witness_counters(dict_len, level):
    for B, extra in ((K1, 0), (K1, 2), (K64, 0)):
        rec = E.chain_encoder_record(True, level, B, extra)
        # a record that has run is opened like a fresh one
        used = plan(rec, [(np.zeros(3 * K1 + 5, np.uint8), True, True)])[0]
        enc, codec = PW.counting_encoder(True, level, B, extra, dict_len)
        for start in (rec, used):
            rc, got = open_plan(start, dict_len)
            if level >= 10:                     # the optimal parser's levels are not opened from a dictionary: the record stays
                assert rc == _native.E_ARG and bytes(got) == bytes(start)
                continue
            assert rc == 0
            assert (got.index, got.pointer, got.dictSize, got.currentOffset) == counters(enc, codec, rec.kind)
            assert got.index == PW.primed_length(rec.kind, dict_len) and (got.taken, got.blocks) == (0, 0)
            assert (got.kind, got.level, got.blockSize, got.extraBlocks, got.ringBytes, got.storeBytes) == \
                (rec.kind, rec.level, rec.blockSize, rec.extraBlocks, rec.ringBytes, rec.storeBytes)
        if rec.kind == 2:
            assert got.currentOffset == K64 and got.dictSize == (min(dict_len, K64) if dict_len >= 8 else 0)
        # no dictionary: the fresh record
        rc, got = open_plan(used, -1)
        assert rc == 0 and bytes(got) == bytes(rec)


def test_open_plan_refusals():
    lib = _native.load_library()
    ind = E.chain_encoder_record(False, 0, K1, 0)
    assert open_plan(ind, 0)[0] == _native.E_ARG and open_plan(ind, 4096)[0] == _native.E_ARG
    rc, got = open_plan(ind, -1)
    assert rc == 0 and bytes(got) == bytes(ind)
    assert lib.k4lz4_chain_encoder_open_plan(None, 5) == _native.E_ARG
    bad = E.chain_encoder_record(True, 0, K1, 0)
    bad.ringBytes += 1
    before = bytes(bad)
    assert lib.k4lz4_chain_encoder_open_plan(C.byref(bad), 100) == _native.E_ARG and bytes(bad) == before


def apply(enc, rec):
    """TopupAndEncode on the counting ring -> (loaded, the block's length or 0)"""
    data, force, _ = rec
    loaded = enc.topup(np.zeros(len(data), np.uint8), 0, len(data)) if len(data) else 0
    n = enc.bytes_ready
    if n < (1 if force else enc.block_size):
        return loaded, 0
    enc.encode(False)
    return loaded, n


@pytest.mark.parametrize("level", [0, 9])
@pytest.mark.parametrize("B,extra", [(K1, 0), (K1, 2), (4 * K1, 1), (K64, 0)])
@pytest.mark.parametrize("dict_len", PC.DICT_LENGTHS)
def test_model_continues_from_the_primed_record(dict_len, B, extra, level):
    rng = np.random.default_rng(dict_len + B + extra + level)
    rec0 = E.chain_encoder_record(True, level, B, extra)
    rc, rec = open_plan(rec0, dict_len)
    assert rc == 0
    kind = kind_of(True, level)
    d = PW.primed_length(kind, dict_len)
    enc, codec = PW.counting_encoder(True, level, B, extra, dict_len)
    records = random_records(rng, B, max(24, 6 * (K64 + 3 * B) // B))
    # the blocks the model yields for the whole run, and the table built from their lengths, are the codec's rows
    rows = model_rows(rec, records)
    cur = rec
    blens = []
    for r in records:
        nb = len(codec.blocks)
        loaded, blen = apply(enc, r)
        cur, got_loaded, got_blen, _ = plan(cur, [r])
        assert got_loaded == [loaded] and got_blen == [blen]
        assert (cur.index, cur.pointer, cur.dictSize, cur.currentOffset) == counters(enc, codec, kind)
        assert len(codec.blocks) == nb + (1 if blen else 0)
        if blen:
            blens.append(blen)
    want = [tuple(b) for b in codec.blocks]
    assert len(want) >= 6 and enc.pointer < cur.taken + d, "the run is long enough to save at least once"
    assert rows == want
    assert table_rows(blens, B, extra, d, kind, cur=K64 if kind == 2 else None) == want
    if kind == 2:
        # the tables' invariant: dictSize is what the ring holds in front of the next block, for every stream -- the empty ones too
        assert rec.dictSize == rec.index == d and rec.currentOffset == K64
        assert codec.arms[0] == ("withPrefix64k" if d else "usingExtDict") and set(codec.arms[1:]) <= {"withPrefix64k"}
    assert (cur.taken, cur.blocks) == (sum(blens) + enc.bytes_ready, len(blens))


@pytest.mark.skipif(not PW.available(), reason="liblz4 1.9.3 is the witness")
@pytest.mark.parametrize("name", PC.NAMES)
def test_goldens_equal_the_live_witness(name):
    with open(GOLDEN) as f:
        golden = {c["name"]: c for c in json.load(f)["cases"]}
    case = PC.case(name)
    assert json.loads(json.dumps(PW.summary(case, PW.play(case)))) == golden[name]


def test_goldens_cover_the_case_list():
    with open(GOLDEN) as f:
        golden = json.load(f)["cases"]
    assert [c["name"] for c in golden] == list(PC.NAMES)
    for c in golden:
        assert c["inputs_crc32"] == PW.inputs_crc(PC.case(c["name"])), c["name"]


@pytest.mark.skipif(not PW.available(), reason="liblz4 1.9.3 is the witness")
def test_witness_takes_the_prefix_arm_and_uses_the_dictionary():
    """the two conditions on the witness alone: the seam block opens as a contiguous prefix's does, and the gain case's first block
    is below half of the unprimed stream's at L00 and L03"""
    seam = PW.play(PC.case("seam"))
    for row in seam:
        assert row["calls"][0][2].startswith(PC.SEAM_PREFIX_START)
    case = PC.case("gain")
    first = [row["calls"][0][1][0] for row in PW.play(case)]
    for s in (0, 2):
        assert case.idx[s] == 0 and case.idx[s + 1] == -1 and case.settings[s] == case.settings[s + 1]
        assert 0 < first[s] < first[s + 1] / 2, (case.settings[s], first)
