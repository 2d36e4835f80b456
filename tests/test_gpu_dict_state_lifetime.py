"""How long the dictionary encoders' state queries answer (k4lz4_encode_dict_state, k4lz4_encode_dict_hc_state), all on one
DeviceCodec: the fast levels and the HC levels keep what they loaded apart from each other; the load step of a per-call call runs
without messages; a call against a k4lz4_dict_set takes its family's answer away and leaves the other family's, and with no
messages it takes nothing away; the host form loads only the entries its messages use.  The smallest committed cases: `seam` of
tests/dict_encode_cases.py at level 0 (three dictionaries), `seam` of tests/dict_hc_encode_cases.py at level 3 (one dictionary, the
fast list's first), and the empty dictionary of both `dictionary_lengths` calls; the tables are checked against the goldens' hashes."""
import os
import sys

import numpy as np
import pytest
import torch

import dict_encode_cases as DC
import dict_hc_encode_cases as HC
from k4os.compression.lz4_amd import DictionarySet, LZ4Codec, LZ4Level
from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import record_dict_goldens as G          # noqa: E402
import record_dict_hc_goldens as GH      # noqa: E402

pytestmark = pytest.mark.gpu


def named(module, goldens, name):
    return next(c for c in module.calls() if c.name == name), next(c for c in goldens.load()["calls"] if c["name"] == name)


FAST, FAST_G = named(DC, G, "seam")
HCS, HCS_G = named(HC, GH, "seam")
EMPTY_FAST_G, EMPTY_HC_G = named(DC, G, "dictionary_lengths")[1], named(HC, GH, "dictionary_lengths")[1]
assert DC.DICT_LENGTHS[0] == HC.DICT_LENGTHS[0] == 0 and FAST.dicts[0].tobytes() == HCS.dicts[0].tobytes()
EMPTY = np.zeros(0, np.uint8)

# what a state query answers per entry: fast (dictSize, xxh32 of the table), HC (kept length, xxh32 of the heads, of the written chain slots)
FAST_STATES = [(FAST_G["dictSize"][k], FAST_G["table_xxh32"][k]) for k in range(3)]
HC_STATES = [(HCS_G["keptLen"][0], HCS_G["heads_xxh32"][0], HCS_G["chain_xxh32"][0])]
EMPTY_FAST_STATE = (EMPTY_FAST_G["dictSize"][0], EMPTY_FAST_G["table_xxh32"][0])
EMPTY_HC_STATE = (EMPTY_HC_G["keptLen"][0], EMPTY_HC_G["heads_xxh32"][0], EMPTY_HC_G["chain_xxh32"][0])


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


@pytest.fixture(scope="module")
def ds(dc):
    with DictionarySet(FAST.dicts, owner=dc) as s:          # both families
        yield s


def encode(dc, level, dicts, msgs, idx, form="device"):
    """one call: against the list `dicts`, or against a DictionarySet; returns outLen"""
    call = DC.Call("lifetime", [] if isinstance(dicts, DictionarySet) else list(dicts))
    for m, d in zip(msgs, idx):
        call.add(m, d)
    src, soff, slen, cap, doff, asz, idx, dct, dcoff, dclen = DC.pack(call)
    per_call = () if isinstance(dicts, DictionarySet) else (dcoff, dclen)
    if form == "host":
        dst = np.zeros(asz, np.uint8)
        return LZ4Codec.EncodeDictBatchPacked(src, soff, slen, dst, doff, cap, idx, dicts if not per_call else dct, *per_call,
                                              level=LZ4Level(level), ctx=dc.ctx).tolist()
    dev = dc.device
    s = DeviceBatch.from_host(src, soff, slen, dev)
    d = DeviceBatch(torch.zeros(asz, dtype=torch.uint8, device=dev), torch.from_numpy(doff.view(np.int64)).to(dev), torch.from_numpy(cap).to(dev))
    t_idx = torch.from_numpy(idx).to(dev)
    if per_call:
        out = dc.encode_dict(s, d, t_idx, torch.from_numpy(dct if dct.size else np.zeros(1, np.uint8)).to(dev), dcoff, dclen, level=LZ4Level(level))
    else:
        out = dc.encode_dictset(s, d, t_idx, dicts, level=LZ4Level(level))
    dc.ctx.synchronize(dc._stream())
    return out.cpu().numpy().tolist()


def fast_call(dc, form="device"):
    assert encode(dc, 0, FAST.dicts, FAST.msgs, FAST.idx, form) == FAST_G["outLen"]


def hc_call(dc, form="device"):
    assert encode(dc, 3, HCS.dicts, HCS.msgs, HCS.idx, form) == HCS_G["levels"]["3"]["outLen"]


def fast_states(dc, want):
    for k, (size, table) in enumerate(want):
        st = dc.dict_state(k)
        assert int(st["currentOffset"][0]) == DC.K64 and int(st["dictSize"][0]) == size, k
        assert G.xxh32(st["hashTable"][0].view(np.uint8)) == table, k


def hc_states(dc, want):
    for k, (kept_len, heads_hash, chain_hash) in enumerate(want):
        heads, chain, kept = dc.dict_hc_state(k)
        assert kept == kept_len and list(GH.table_hashes(heads, chain, kept)) == [heads_hash, chain_hash], k


def refused(query, k=0):
    with pytest.raises(ValueError, match="no such dictionary"):
        query(k)


@pytest.mark.parametrize("first", ["fast", "hc"])
def test_the_families_keep_their_answers_apart(first, dc):
    for call in (fast_call, hc_call) if first == "fast" else (hc_call, fast_call):
        call(dc)
    fast_states(dc, FAST_STATES)
    hc_states(dc, HC_STATES)
    refused(dc.dict_state, 3)
    refused(dc.dict_hc_state, 1)


def test_the_load_step_runs_without_messages(dc):
    """lists the calls before them did not load: the fast one reversed behind an empty dictionary, the HC one behind an empty dictionary"""
    fast_call(dc)
    hc_call(dc)
    assert encode(dc, 0, [EMPTY] + FAST.dicts[::-1], [], []) == []
    assert encode(dc, 3, [EMPTY] + HCS.dicts, [], []) == []
    fast_states(dc, [EMPTY_FAST_STATE] + FAST_STATES[::-1])
    hc_states(dc, [EMPTY_HC_STATE] + HC_STATES)


def test_a_set_call_takes_its_familys_answer_and_leaves_the_other(dc, ds):
    fast_call(dc)
    hc_call(dc)
    assert encode(dc, 0, ds, FAST.msgs, FAST.idx) == FAST_G["outLen"]
    refused(dc.dict_state)
    hc_states(dc, HC_STATES)
    assert encode(dc, 3, ds, HCS.msgs, HCS.idx) == HCS_G["levels"]["3"]["outLen"]
    refused(dc.dict_hc_state)
    refused(dc.dict_state)
    fast_call(dc)                                           # and the other way round
    assert encode(dc, 3, ds, HCS.msgs, HCS.idx, "host") == HCS_G["levels"]["3"]["outLen"]
    fast_states(dc, FAST_STATES)
    refused(dc.dict_hc_state)


@pytest.mark.parametrize("form", ["device", "host"])
def test_a_set_call_without_messages_takes_nothing(form, dc, ds):
    fast_call(dc)
    hc_call(dc)
    for level in (0, 3):
        assert encode(dc, level, ds, [], [], form) == []
    fast_states(dc, FAST_STATES)
    hc_states(dc, HC_STATES)


def test_the_host_form_loads_only_the_entries_in_use(dc):
    """the fast list's first and last entries at both levels: the query refuses the one in between, and what lies beyond the list"""
    assert encode(dc, 0, FAST.dicts, [FAST.msgs[0], FAST.msgs[2]], [0, 2], "host") == [FAST_G["outLen"][0], FAST_G["outLen"][2]]
    assert encode(dc, 3, FAST.dicts, HCS.msgs, [0], "host") == HCS_G["levels"]["3"]["outLen"]
    fast_states(dc, FAST_STATES[:1])
    hc_states(dc, HC_STATES)
    st = dc.dict_state(2)
    assert (int(st["dictSize"][0]), G.xxh32(st["hashTable"][0].view(np.uint8))) == FAST_STATES[2]
    for query in (dc.dict_state, dc.dict_hc_state):
        refused(query, 1)
        refused(query, 3)
    refused(dc.dict_hc_state, 2)
