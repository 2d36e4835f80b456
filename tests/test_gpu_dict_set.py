"""k4lz4_dict_set on the GPU: for every call of tests/dict_encode_cases.py (level 0) and tests/dict_hc_encode_cases.py
(the levels each call names) one set is built from the call's dictionaries, and encoding against it -- host form and device form --
gives the blocks the committed goldens record (liblz4's; liblz4 itself is asked too where the machine has it), with the 0xCD guards
and the slots' tails untouched; the same arena the per-call calls give; the tables the goldens' hashes pin; blocks that decode again
through the set (device form everywhere, host form on one call, -1 for "no dictionary", K4LZ4_FLAG_PARTIAL against
k4lz4_decode_dict_batch_device).  Then what makes a set a set: it does not depend on the caller's memory after create, any number of
calls on any stream and from a second context reuse it without a load step, and what the per-call calls refuse it refuses."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import dict_encode_cases as DC
import dict_encode_witness as W
import dict_hc_encode_cases as HC
import dict_hc_encode_witness as HW
from k4os.compression.lz4_amd import DICT_FAST, DICT_HC, DictionarySet, LZ4Codec, LZ4Level, _native, encode_dict_device, encode_dictset_device, pack_blocks
from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import record_dict_goldens as G          # noqa: E402
import record_dict_hc_goldens as GH      # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 16
CASES = [("fast", c.name, 0) for c in DC.calls()] + [("hc", name, lv) for name, lv in HC.call_levels()]
IDS = [f"{k}-{n}-L{lv}" for k, n, lv in CASES]


def call_of(kind, name):
    return next(c for c in (DC if kind == "fast" else HC).calls() if c.name == name)


@functools.lru_cache(maxsize=None)
def call_golden(kind, name):
    return next(c for c in (G if kind == "fast" else GH).load()["calls"] if c["name"] == name)


def golden(kind, name, level):
    g = call_golden(kind, name)
    return g if kind == "fast" else g["levels"][str(level)]


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


@pytest.fixture(scope="module")
def sets(dc):
    """one set per call, both families, built on first use and closed with the module"""
    made = {}

    def get(kind, name):
        if (kind, name) not in made:
            made[(kind, name)] = DictionarySet(call_of(kind, name).dicts, owner=dc)
        return made[(kind, name)]

    yield get
    for s in made.values():
        s.close()


def packed(kind, name, level):
    return DC.pack(call_of(kind, name), golden(kind, name, level)["size"], GUARD)


def check_blocks(kind, name, level, out, dst, doff, cap, untouched_behind_minus_one):
    """outLen and bytes against the goldens (and the witness), guards and the slots' tails against the 0xCD they were filled with"""
    call, g = call_of(kind, name), golden(kind, name, level)
    assert out.tolist() == g["outLen"], (name, level)
    used = np.zeros(dst.size, bool)
    witness = (W if kind == "fast" else HW).available()
    for i, (m, d) in enumerate(zip(call.msgs, call.idx)):
        o = int(doff[i])
        if out[i] > 0:
            got = dst[o:o + int(out[i])]
            used[o:o + int(out[i])] = True
            assert G.xxh32(got) == g["xxh32"][i], (name, level, i)
            if str(i) in g["bytes"]:
                assert got.tobytes().hex() == g["bytes"][str(i)], (name, level, i)
            if witness:
                r, want = W.encode(m, call.dicts[d], int(cap[i])) if kind == "fast" else HW.encode(m, call.dicts[d], int(cap[i]), level)
                assert r == out[i] and got.tobytes() == want, (name, level, i)
        elif out[i] < 0 and not untouched_behind_minus_one:
            used[o:o + int(cap[i])] = True
    assert (dst[~used] == 0xCD).all(), (name, level)


def device_arena(dev, asz, doff, cap):
    return DeviceBatch(torch.full((asz,), 0xCD, dtype=torch.uint8, device=dev), torch.from_numpy(doff.view(np.int64)).to(dev),
                       torch.from_numpy(cap).to(dev))


@pytest.mark.parametrize("kind,name,level", CASES, ids=IDS)
def test_host_form(kind, name, level, sets):
    src, soff, slen, cap, doff, asz, idx, *_ = packed(kind, name, level)
    dst = np.full(asz, 0xCD, np.uint8)
    out = LZ4Codec.EncodeDictBatchPacked(src, soff, slen, dst, doff, cap, idx, sets(kind, name), level=LZ4Level(level))
    check_blocks(kind, name, level, out, dst, doff, cap, True)
    if (kind, name) == ("fast", "seam"):
        assert dst[int(doff[0]):].tobytes().startswith(DC.SEAM_BLOCK_START)


@pytest.mark.parametrize("kind,name,level", CASES, ids=IDS)
def test_device_form_per_call_arena_tables_and_round_trip(kind, name, level, dc, sets):
    call, ds = call_of(kind, name), sets(kind, name)
    src, soff, slen, cap, doff, asz, idx, dct, dcoff, dclen = packed(kind, name, level)
    n, dev = len(call.msgs), dc.device
    s = DeviceBatch.from_host(src, soff, slen, dev)
    d = device_arena(dev, asz, doff, cap)
    t_idx = torch.from_numpy(idx).to(dev)
    out_t = encode_dictset_device(dc, s, d, t_idx, ds, level=LZ4Level(level))
    dc.ctx.synchronize(dc._stream())
    out, dst = out_t.cpu().numpy(), d.data.cpu().numpy()
    check_blocks(kind, name, level, out, dst, doff, cap, False)
    # the per-call call on the same messages: the same arena, byte for byte
    d2 = device_arena(dev, asz, doff, cap)
    t_dct = torch.from_numpy(dct if dct.size else np.zeros(1, np.uint8)).to(dev)
    out2 = encode_dict_device(dc, s, d2, t_idx, t_dct, dcoff, dclen, level=LZ4Level(level))
    dc.ctx.synchronize(dc._stream())
    assert out2.cpu().numpy().tolist() == out.tolist() and torch.equal(d2.data, d.data), (name, level)
    # the tables, read from the set
    g = call_golden(kind, name)
    for k in range(len(call.dicts)):
        if kind == "fast":
            st = ds.state(k)
            assert int(st["currentOffset"][0]) == DC.K64 and int(st["dictSize"][0]) == g["dictSize"][k]
            assert G.xxh32(st["hashTable"][0].view(np.uint8)) == g["table_xxh32"][k], (name, k)
        else:
            heads, chain, kept = ds.hc_state(k)
            assert kept == g["keptLen"][k]
            assert list(GH.table_hashes(heads, chain, kept)) == [g["heads_xxh32"][k], g["chain_xxh32"][k]], (name, k)
    # and back through the set
    if n:
        back = DeviceBatch.empty_slots(np.maximum(slen, 1), dev, fill=0xCD)
        enc = DeviceBatch(d.data, d.off, torch.clamp(out_t, min=0))
        blen = dc.decode_dictset(enc, back, t_idx, ds)
        dc.ctx.synchronize(dc._stream())
        blen, bdata, boff = blen.cpu().numpy(), back.data.cpu().numpy(), back.off.cpu().numpy()
        for i, m in enumerate(call.msgs):
            if out[i] > 0:
                assert blen[i] == m.size and bdata[int(boff[i]):int(boff[i]) + m.size].tobytes() == m.tobytes(), (name, level, i)


def encoded(kind, name, level, ds):
    """(blocks, idx, messages) of a call, through the host form"""
    call = call_of(kind, name)
    blocks = LZ4Codec.EncodeDictBatch(call.msgs, ds, call.idx, LZ4Level(level))
    assert [len(b) for b in blocks] == golden(kind, name, level)["outLen"]
    return blocks, np.array(call.idx, np.int32), call.msgs


def test_host_form_decodes_and_minus_one_is_no_dictionary(dc, sets):
    ds = sets("fast", "dictionary_lengths")
    blocks, idx, msgs = encoded("fast", "dictionary_lengths", 0, ds)
    plain = LZ4Codec.EncodeBatch([msgs[1], msgs[2]])                       # encoded without a dictionary
    blocks, msgs = blocks + plain, msgs + [msgs[1], msgs[2]]
    idx = np.concatenate([idx, np.array([-1, -1], np.int32)])
    src, soff, slen = pack_blocks([np.frombuffer(b, np.uint8) for b in blocks])
    cap = np.array([max(m.size, 1) for m in msgs], np.int32)
    doff = np.zeros(len(msgs), np.uint64)
    doff[1:] = np.cumsum(cap[:-1].astype(np.uint64) + GUARD)
    doff += GUARD
    dst = np.full(int(doff[-1]) + int(cap[-1]) + GUARD, 0xCD, np.uint8)
    out = LZ4Codec.DecodeDictSetBatchPacked(src, soff, slen, dst, doff, cap, idx, ds)
    used = np.zeros(dst.size, bool)
    for i, m in enumerate(msgs):
        assert out[i] == m.size and dst[int(doff[i]):int(doff[i]) + m.size].tobytes() == m.tobytes(), i
        used[int(doff[i]):int(doff[i]) + m.size] = True
    assert (dst[~used] == 0xCD).all()
    # the same on the device
    dev = dc.device
    enc = DeviceBatch.from_host(src, soff, slen, dev)
    back = device_arena(dev, dst.size, doff, cap)
    blen = dc.decode_dictset(enc, back, torch.from_numpy(idx).to(dev), ds)
    dc.ctx.synchronize(dc._stream())
    assert blen.cpu().numpy().tolist() == out.tolist() and np.array_equal(back.data.cpu().numpy(), dst)


def test_partial_decode_equals_the_per_call_decoder(dc, sets):
    kind, name = "fast", "message_lengths"
    ds, call = sets(kind, name), call_of(kind, name)
    blocks, idx, msgs = encoded(kind, name, 0, ds)
    keep = [i for i, b in enumerate(blocks) if len(b) > 0]
    src, soff, slen = pack_blocks([np.frombuffer(blocks[i], np.uint8) for i in keep])
    cap = np.array([max(msgs[i].size // 2, 1) for i in keep], np.int32)          # stop half way
    dev = dc.device
    enc = DeviceBatch.from_host(src, soff, slen, dev)
    a, b = (DeviceBatch.empty_slots(cap, dev, fill=0xCD) for _ in range(2))
    t_idx = torch.from_numpy(idx[keep]).to(dev)
    got = dc.decode_dictset(enc, a, t_idx, ds, flags=_native.FLAG_PARTIAL)
    dct, dcoff, dclen = pack_blocks(call.dicts)
    per_off = torch.from_numpy(dcoff[idx[keep]].view(np.int64)).to(dev)
    per_len = torch.from_numpy(dclen[idx[keep]]).to(dev)
    want = dc.decode_dict(enc, b, torch.from_numpy(dct).to(dev), per_off, per_len, flags=_native.FLAG_PARTIAL)
    dc.ctx.synchronize(dc._stream())
    assert got.cpu().numpy().tolist() == want.cpu().numpy().tolist() == cap.tolist()
    assert torch.equal(a.data, b.data)
    adata, aoff = a.data.cpu().numpy(), a.off.cpu().numpy()
    for j, i in enumerate(keep):
        assert adata[int(aoff[j]):int(aoff[j]) + int(cap[j])].tobytes() == msgs[i][:int(cap[j])].tobytes(), i


@pytest.mark.parametrize("form", ["host", "device"])
def test_the_set_does_not_depend_on_the_callers_memory(form, dc):
    kind, name = "hc", "interleaved"
    call = call_of(kind, name)
    src, soff, slen, cap, doff, asz, idx, dct, dcoff, dclen = packed(kind, name, 3)
    if form == "host":
        buf = dct.copy()
        ds = DictionarySet(buf, dcoff, dclen, owner=dc)
        buf[:] = 0xFF
    else:
        buf = torch.from_numpy(dct).to(dc.device)
        ds = DictionarySet(buf, dcoff, dclen, owner=dc)
        buf.fill_(0xFF)
        torch.cuda.synchronize()
    with ds:
        for kind, level in (("fast", 0), ("hc", 3)):
            assert call_of("fast", name).dicts[0].tobytes() == call.dicts[0].tobytes()
            src, soff, slen, cap, doff, asz, idx, *_ = packed(kind, name, level)
            dst = np.full(asz, 0xCD, np.uint8)
            out = LZ4Codec.EncodeDictBatchPacked(src, soff, slen, dst, doff, cap, idx, ds, level=LZ4Level(level))
            check_blocks(kind, name, level, out, dst, doff, cap, True)


def test_reuse_across_calls_streams_and_contexts(dc, sets):
    name = "interleaved"
    ds = sets("fast", name)
    fast, hc = call_of("fast", name), call_of("hc", name)
    assert [m.tobytes() for m in fast.msgs] == [m.tobytes() for m in hc.msgs] and fast.idx == hc.idx      # one set serves both lists
    info = ds.info
    assert info == {"nDict": 4, "fast_tables": 4, "hc_tables": 4, "device_bytes": DictionarySet.layout(*pack_blocks(fast.dicts)[1:])[4],
                    "families": DICT_FAST | DICT_HC, "device": dc.device_index, "fast_loads": 1, "hc_loads": 1}
    dev = dc.device
    other = DeviceCodec(0)                                                   # a second context on the same device
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    runs = []
    for k in range(6):
        kind, level = (("fast", 0), ("hc", 3))[k % 2]
        src, soff, slen, cap, doff, asz, idx, *_ = packed(kind, name, level)
        s = DeviceBatch.from_host(src, soff, slen, dev)
        d = device_arena(dev, asz, doff, cap)
        t_idx = torch.from_numpy(idx).to(dev)
        st = streams[(k // 2) % 2]
        st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(st):
            out_t = (other if k == 5 else dc).encode_dictset(s, d, t_idx, ds, level=LZ4Level(level))
        runs.append((kind, level, out_t, d, doff, cap, s, t_idx))
    for st in streams:
        dc.ctx.synchronize(st.cuda_stream)
        other.ctx.synchronize(st.cuda_stream)
    for kind, level, out_t, d, doff, cap, *_ in runs:
        check_blocks(kind, name, level, out_t.cpu().numpy(), d.data.cpu().numpy(), doff, cap, False)
    assert ds.info == info                                                   # no load step per call
    other.ctx.close()


def test_an_index_outside_the_set_device_forms(dc, sets):
    ds = sets("fast", "seam")
    src, soff, slen, cap, doff, asz, idx, *_ = DC.pack(call_of("fast", "seam"), None, GUARD)
    g = golden("fast", "seam", 0)
    dev = dc.device
    s = DeviceBatch.from_host(src, soff, slen, dev)
    good = device_arena(dev, asz, doff, cap)
    good_len = dc.encode_dictset(s, good, torch.from_numpy(idx).to(dev), ds)
    dc.ctx.synchronize(dc._stream())
    bad = idx.copy()
    bad[1], bad[2] = 3, -1
    for level in (0, 3):
        d = device_arena(dev, asz, doff, cap)
        out_t = dc.encode_dictset(s, d, torch.from_numpy(bad).to(dev), ds, level=LZ4Level(level))
        with pytest.raises(ValueError, match="dictIdx"):
            dc.ctx.synchronize(dc._stream())
        out, dst = out_t.cpu().numpy(), d.data.cpu().numpy()
        assert out[1] == -1 and out[2] == -1 and (dst[int(doff[1]):int(doff[3])] == 0xCD).all()
        if level == 0:
            assert out[0] == g["outLen"][0] and out[3] == g["outLen"][3]
            assert np.array_equal(dst[:int(doff[1])], good.data.cpu().numpy()[:int(doff[1])])
        else:
            assert out[0] > 0 and out[3] > 0
        dc.ctx.synchronize(dc._stream())        # the status word was taken
    # decode: 3 and -2 lie outside, -1 is "no dictionary" (message 0's block does not need one to be refused or not: it is decoded with its own)
    msgs = call_of("fast", "seam").msgs
    enc = DeviceBatch(good.data, good.off, torch.clamp(good_len, min=0))
    bcap = np.array([m.size for m in msgs], np.int32)
    boff = np.zeros(len(msgs), np.uint64)
    boff[1:] = np.cumsum(bcap[:-1].astype(np.uint64) + GUARD)
    boff += GUARD
    back = device_arena(dev, int(boff[-1]) + int(bcap[-1]) + GUARD, boff, bcap)
    bad[1], bad[2] = 3, -2
    blen = dc.decode_dictset(enc, back, torch.from_numpy(bad).to(dev), ds)
    with pytest.raises(ValueError, match="dictIdx"):
        dc.ctx.synchronize(dc._stream())
    blen, bdata = blen.cpu().numpy(), back.data.cpu().numpy()
    assert blen[1] == -1 and blen[2] == -1 and (bdata[int(boff[0]) + msgs[0].size:int(boff[3])] == 0xCD).all()
    for i in (0, 3):
        assert blen[i] == msgs[i].size and bdata[int(boff[i]):int(boff[i]) + msgs[i].size].tobytes() == msgs[i].tobytes()
    dc.ctx.synchronize(dc._stream())


def test_refusals(dc, sets):
    kind, name = "fast", "seam"
    call = call_of(kind, name)
    src, soff, slen, cap, doff, asz, idx, *_ = DC.pack(call, None, GUARD)
    both = sets(kind, name)

    def host(ds, level=0, flags=0, index=idx):
        dst = np.full(asz, 0xCD, np.uint8)
        try:
            return LZ4Codec.EncodeDictBatchPacked(src, soff, slen, dst, doff, cap, index, ds, level=level, flags=flags, ctx=dc.ctx)
        except ValueError:
            assert (dst == 0xCD).all()              # a refused call writes nothing
            raise

    with DictionarySet(call.dicts, families=DICT_FAST, owner=dc) as only_fast, DictionarySet(call.dicts, families=DICT_HC, owner=dc) as only_hc:
        assert only_fast.info["hc_tables"] == 0 and only_fast.info["hc_loads"] == 0 and only_hc.info["fast_loads"] == 0
        with pytest.raises(ValueError, match="family"):
            host(only_fast, 3)
        with pytest.raises(ValueError, match="family"):
            host(only_hc, 0)
        with pytest.raises(ValueError):
            only_fast.hc_state(0)
        with pytest.raises(ValueError):
            only_hc.state(0)
        assert host(only_fast, 0).tolist() == golden(kind, name, 0)["outLen"]
        assert host(only_hc, 3).tolist() == host(both, 3).tolist()
    with pytest.raises(ValueError, match="10 - 12"):
        host(both, 10)
    with pytest.raises(ValueError, match="32-bit"):
        host(both, 0, _native.FLAG_X32)
    try:
        LZ4Codec.Enforce32 = True
        with pytest.raises(ValueError, match="32-bit"):
            host(both, 3)
    finally:
        LZ4Codec.Enforce32 = False
    with pytest.raises(ValueError, match="no flags"):
        host(both, 0, _native.FLAG_NO_REORDER)
    for wrong in (3, -1):
        index = idx.copy()
        index[1] = wrong
        with pytest.raises(ValueError, match="dictIdx"):
            host(both, 0, 0, index)
        with pytest.raises(ValueError, match="dictIdx"):
            host(both, 3, 0, index)
    index = idx.copy()
    index[1] = -2
    dst = np.full(asz, 0xCD, np.uint8)
    with pytest.raises(ValueError, match="dictIdx"):
        LZ4Codec.DecodeDictSetBatchPacked(src, soff, slen, dst, doff, cap, index, both, ctx=dc.ctx)
    assert (dst == 0xCD).all()
    with pytest.raises(ValueError):
        DictionarySet(call.dicts, families=0, owner=dc)
    with pytest.raises(ValueError):
        both.state(3)
    dc.lib.k4lz4_dict_set_destroy(None)
    # no messages; no dictionaries
    e8, e64, e32 = np.zeros(1, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.int32)
    for level in (0, 3):
        assert LZ4Codec.EncodeDictBatchPacked(e8, e64, e32, e8.copy(), e64, e32, e32, both, level=level, ctx=dc.ctx).size == 0
    assert LZ4Codec.DecodeDictSetBatchPacked(e8, e64, e32, e8.copy(), e64, e32, e32, both, ctx=dc.ctx).size == 0
    with DictionarySet([], owner=dc) as nothing:
        assert nothing.info["nDict"] == 0 and nothing.info["fast_tables"] == 1 and nothing.info["hc_tables"] == 1
        assert LZ4Codec.EncodeDictBatchPacked(e8, e64, e32, e8.copy(), e64, e32, e32, nothing, ctx=dc.ctx).size == 0
        with pytest.raises(ValueError, match="dictIdx"):
            host(nothing, 0, 0, np.zeros(len(call.msgs), np.int32))
        plain = LZ4Codec.EncodeBatch([call.msgs[0]])
        b, o, l = pack_blocks([np.frombuffer(plain[0], np.uint8)])
        back = np.zeros(call.msgs[0].size, np.uint8)
        got = LZ4Codec.DecodeDictSetBatchPacked(b, o, l, back, np.zeros(1, np.uint64), np.array([back.size], np.int32), np.array([-1], np.int32),
                                                nothing, ctx=dc.ctx)
        assert got[0] == back.size and back.tobytes() == call.msgs[0].tobytes()
