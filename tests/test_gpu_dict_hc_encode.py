"""k4lz4_encode_dict_hc_batch and k4lz4_encode_dict_hc_batch_device on the GPU, on the whole shared list of cases
(tests/dict_hc_encode_cases.py) at every level a case names: blocks against the goldens recorded from liblz4
(tests/golden/dict_hc_encode_cases.json: nothing is left out where the machine has no liblz4) and against liblz4 itself where it is
present, the loaded tables (k4lz4_encode_dict_hc_state) against the recorded table hashes, every block decoded again with
k4lz4_decode_dict_batch_device, and in the device form the 0xCD guard bytes around every output slot and the slot's bytes behind
outLen."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import dict_hc_encode_cases as HC
import dict_hc_encode_witness as W
from k4os.compression.lz4_amd import LZ4Codec, LZ4Level, encode_dict_device
from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import record_dict_hc_goldens as G     # noqa: E402

pytestmark = pytest.mark.gpu
PAIRS = HC.call_levels()
GUARD = 16


@functools.lru_cache(maxsize=None)
def golden(name):
    return next(c for c in G.load()["calls"] if c["name"] == name)


def call_of(name):
    return next(c for c in HC.calls() if c.name == name)


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


def check_blocks(name, level, out, dst, doff, cap, untouched_behind_minus_one):
    """outLen and bytes against the goldens (and the witness), guards and the slots' tails against the 0xCD they were filled with"""
    call, g = call_of(name), golden(name)["levels"][str(level)]
    assert out.tolist() == g["outLen"], (name, level)
    used = np.zeros(dst.size, bool)
    witness = W.available()
    for i, (m, d) in enumerate(zip(call.msgs, call.idx)):
        o = int(doff[i])
        if out[i] > 0:
            got = dst[o:o + int(out[i])]
            used[o:o + int(out[i])] = True
            assert G.xxh32(got) == g["xxh32"][i], (name, level, i)
            if str(i) in g["bytes"]:
                assert got.tobytes().hex() == g["bytes"][str(i)], (name, level, i)
            if witness:
                r, want = W.encode(m, call.dicts[d], int(cap[i]), level)
                assert r == out[i] and got.tobytes() == want, (name, level, i)
        elif out[i] < 0 and not untouched_behind_minus_one:
            used[o:o + int(cap[i])] = True
    assert (dst[~used] == 0xCD).all(), (name, level)


@pytest.mark.parametrize("name,level", PAIRS)
def test_host_form(name, level):
    call = call_of(name)
    src, soff, slen, cap, doff, asz, idx, dct, dcoff, dclen = HC.pack(call, golden(name)["levels"][str(level)]["size"], GUARD)
    dst = np.full(asz, 0xCD, np.uint8)
    out = LZ4Codec.EncodeDictBatchPacked(src, soff, slen, dst, doff, cap, idx, dct, dcoff, dclen, LZ4Level(level))
    check_blocks(name, level, out, dst, doff, cap, True)


@pytest.mark.parametrize("name,level", PAIRS)
def test_device_form_tables_and_round_trip(name, level, dc):
    call, g = call_of(name), golden(name)
    src, soff, slen, cap, doff, asz, idx, dct, dcoff, dclen = HC.pack(call, g["levels"][str(level)]["size"], GUARD)
    n = len(call.msgs)
    dev = dc.device
    s = DeviceBatch.from_host(src, soff, slen, dev)
    d = DeviceBatch(torch.full((asz,), 0xCD, dtype=torch.uint8, device=dev), torch.from_numpy(doff.view(np.int64)).to(dev),
                    torch.from_numpy(cap).to(dev))
    t_idx = torch.from_numpy(idx).to(dev)
    t_dct = torch.from_numpy(dct if dct.size else np.zeros(1, np.uint8)).to(dev)
    out_t = encode_dict_device(dc, s, d, t_idx, t_dct, dcoff, dclen, level=LZ4Level(level))
    dc.ctx.synchronize(dc._stream())
    out = out_t.cpu().numpy()
    dst = d.data.cpu().numpy()
    check_blocks(name, level, out, dst, doff, cap, False)
    # the tables the load step left: all heads, the written chain slots
    for k in range(len(call.dicts)):
        heads, chain, kept = dc.dict_hc_state(k)
        assert kept == g["keptLen"][k]
        assert list(G.table_hashes(heads, chain, kept)) == [g["heads_xxh32"][k], g["chain_xxh32"][k]], (name, k)
    # and back, on the device, with the same dictionaries
    if n:
        back = DeviceBatch.empty_slots(np.maximum(slen, 1), dev, fill=0xCD)
        per_off = torch.from_numpy(dcoff[idx].view(np.int64)).to(dev)
        per_len = torch.from_numpy(dclen[idx]).to(dev)
        enc = DeviceBatch(d.data, d.off, torch.clamp(out_t, min=0))
        blen = dc.decode_dict(enc, back, t_dct, per_off, per_len)
        dc.ctx.synchronize(dc._stream())
        blen, bdata, boff = blen.cpu().numpy(), back.data.cpu().numpy(), back.off.cpu().numpy()
        for i, m in enumerate(call.msgs):
            if out[i] > 0:
                assert blen[i] == m.size and bdata[int(boff[i]):int(boff[i]) + m.size].tobytes() == m.tobytes(), (name, level, i)


def test_device_form_reports_an_index_outside_the_list(dc):
    call = call_of("tile")
    src, soff, slen, cap, doff, asz, idx, dct, dcoff, dclen = HC.pack(call, None, GUARD)
    idx = np.array([2, 1], np.int32)
    dev = dc.device
    s = DeviceBatch.from_host(src, soff, slen, dev)
    d = DeviceBatch(torch.full((asz,), 0xCD, dtype=torch.uint8, device=dev), torch.from_numpy(doff.view(np.int64)).to(dev),
                    torch.from_numpy(cap).to(dev))
    out_t = dc.encode_dict(s, d, torch.from_numpy(idx).to(dev), torch.from_numpy(dct).to(dev), dcoff, dclen, level=LZ4Level.L04_HC)
    with pytest.raises(ValueError, match="dictIdx"):
        dc.ctx.synchronize(dc._stream())
    out, dst = out_t.cpu().numpy(), d.data.cpu().numpy()
    assert out[0] == -1 and (dst[int(doff[0]):int(doff[1])] == 0xCD).all()
    assert out[1] == golden("tile")["levels"]["4"]["outLen"][1]
    dc.ctx.synchronize(dc._stream())        # the status word was taken


def test_list_interface():
    call = call_of("interleaved")
    got = LZ4Codec.EncodeDictBatch(call.msgs, call.dicts, call.idx, LZ4Level.L09_HC)
    g = golden("interleaved")["levels"]["9"]
    assert [len(b) for b in got] == g["outLen"] and [G.xxh32(b) for b in got] == g["xxh32"]
