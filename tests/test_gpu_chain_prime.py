"""Chained encoders and decoders opened from a dictionary set on the GPU (k4lz4_chain_encoder_open_dictset /
k4lz4_chain_decoder_open_dictset), host and device forms, the stores apart with guard bytes between them: every
case's bytes, recLoaded, recOut, the ring and the fast-chain state against the committed goldens and, where liblz4 1.9.3 is
present, the live witness; the round trip through decoders opened from the same set; block 1 through k4lz4_decode_dictset_batch; an
opened decoder beside RESET + Inject of the same bytes; RESET after an open; the object forms."""
import functools
import json
import os

import numpy as np
import pytest

import chain_prime_cases as PC
import chain_prime_witness as PW
from k4os.compression.lz4_amd.encoders import ChainEncoderRecord
from test_chain_encoder_host import plan
from test_gpu_chain_encoder import HostForm, DeviceForm
from test_gpu_chain_decoder import HostForm as DecoderHostForm, DeviceForm as DecoderDeviceForm

pytestmark = pytest.mark.gpu
K1, K64 = 1024, 65536


@functools.lru_cache(maxsize=None)
def goldens():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_prime_cases.json")) as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


@functools.lru_cache(maxsize=None)
def witnessed(name):
    return PW.play(PC.case(name)) if PW.available() else None


def make_set(case, families=3):
    from k4os.compression.lz4_amd import DictionarySet
    return DictionarySet(case.dict_buf, case.dict_off, case.dict_len, families=families)


class EncHost(HostForm):
    def open(self, idx, dset):
        self.b.open(idx, dset)
        self.intact()


class EncDevice(DeviceForm):
    def open(self, idx, dset):
        import torch
        self.d.open(idx, dset)
        torch.cuda.synchronize()
        self.intact()


FORMS = {"host": EncHost, "device": EncDevice}


def state_of(f, i):
    return PW.state_words(f.state(i)[0]) if f.records[i].kind == 2 else None


@functools.lru_cache(maxsize=None)
def opened(name):
    """-> (the case's streams that the library opens, their indices in the case)"""
    keep = PC.opened_streams(PC.case(name))
    return PC.subcase(PC.case(name), keep), keep


def play(form, name):
    """the case's opened streams on the GPU, in play()'s shape"""
    case, _ = opened(name)
    n = len(case.settings)
    f = FORMS[form](case.settings)
    with make_set(case) as dset:
        f.open(case.idx, dset)
        rows = [{"open": (f.ring(i), state_of(f, i)), "calls": []} for i in range(n)]
        for call in case.calls:
            before = [bytes(f.records[i]) for i in range(n)]
            model = [plan(ChainEncoderRecord.from_buffer_copy(f.records[i]), call[i])[1] if call[i] else [] for i in range(n)]
            loaded, out, olen, data = f.run(call)
            for i in range(n):
                if not call[i]:
                    assert olen[i] == 0 and bytes(f.records[i]) == before[i]
                assert loaded[i] == model[i]               # recLoaded is the host model's (pinned to the witness without a GPU)
                assert olen[i] == len(data[i])
                rows[i]["calls"].append((loaded[i], out[i], data[i], f.ring(i), state_of(f, i) if call[i] else None))
    return case, f, rows


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", PC.NAMES)
def test_every_call_equals_the_goldens_and_the_witness(name, form):
    case, f, rows = play(form, name)
    keep = opened(name)[1]
    live = witnessed(name)
    if live is not None:                               # byte for byte first: it says where
        for s, (got, want) in enumerate(zip(rows, [live[k] for k in keep])):
            assert got["open"] == want["open"], (name, s, case.settings[s], case.idx[s], "open")
            for c, (g, w) in enumerate(zip(got["calls"], want["calls"])):
                assert g == w, (name, s, case.settings[s], case.idx[s], "call", c)
    got, want = json.loads(json.dumps(PW.summary(case, rows)))["streams"], [goldens()[name]["streams"][k] for k in keep]
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, s, case.settings[s], case.idx[s])
    for s, e in enumerate(case.idx):                   # the host records are what the device holds
        r = f.records[s]
        assert r.taken == case.contents[s].size and r.pointer - r.index == 0
        if r.kind == 2:
            assert [r.currentOffset, r.dictSize] == got[s]["final"][2][1:]
    if name == "seam":                                 # the prefix arm, literally
        assert all(row["calls"][0][2].startswith(PC.SEAM_PREFIX_START) for row in rows)
    if name == "gain":                                 # the dictionary is used: the primed first 1 KiB block is below half of the unprimed one's
        first = [row["calls"][0][1][0] for row in rows]
        for s in (0, 2):                               # L00 and L03
            assert case.idx[s] == 0 and case.idx[s + 1] == -1 and case.settings[s] == case.settings[s + 1]
            assert 0 < first[s] < first[s + 1] / 2, (case.settings[s], first)


def encode_all(case, dset):
    """every stream's blocks over all calls, through the host form: [(recOut, bytes)] per stream"""
    from k4os.compression.lz4_amd.encoders import LZ4EncoderBatch
    enc = LZ4EncoderBatch(case.settings)
    enc.open(case.idx, dset)
    blocks = [[] for _ in case.settings]
    for call in case.calls:
        _, rec_out, olen, data = enc.Run(call)
        for s, b in enumerate(LZ4EncoderBatch.blocks_of(rec_out, olen, data)):
            blocks[s] += b
    return blocks


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", ["mixed", "lengths_b64k", "first_records"])
def test_round_trip_through_decoders_opened_from_the_set(name, form):
    case = opened(name)[0]
    with make_set(case) as dset:
        blocks = encode_all(case, dset)
        dec = (DecoderHostForm if form == "host" else DecoderDeviceForm)([(s[0], s[2], s[3]) for s in case.settings])
        injected = open_decoders(dec, form, case.idx, dset)
        for s, e in enumerate(case.idx):
            assert injected[s] == (min(int(case.dict_len[e]), K64) if e >= 0 else 0)
        ro, out, got = dec.run([[(o < 0, b, 0) for o, b in bl] for bl in blocks], drain=True, caps=[c.size for c in case.contents])
    for s, c in enumerate(case.contents):
        assert out[s] == c.size and got[s] == c.tobytes(), (name, s, case.settings[s], case.idx[s])


def open_decoders(dec, form, idx, dset):
    """-> outLen per decoder; the stores' guards checked"""
    if form == "host":
        out = dec.b.open(idx, dset)
    else:
        import torch
        t = dec.cd.open(torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dec.dev), dset,
                        torch.full((dec.n,), -999, dtype=torch.int64, device=dec.dev))
        torch.cuda.synchronize()
        out = t.cpu().numpy().tolist()
    dec._stores_intact()
    return out


def test_first_blocks_decode_through_the_set_as_an_external_dictionary():
    """block 1 of every primed stream sees only its dictionary: k4lz4_decode_dictset_batch with the same entry returns its bytes"""
    from k4os.compression.lz4_amd import LZ4Codec
    from k4os.compression.lz4_amd.codec import pack_blocks, make_arena
    case = opened("lengths_short")[0]
    with make_set(case) as dset:
        blocks = encode_all(case, dset)
        which = [s for s, bl in enumerate(blocks) if bl[0][0] > 0]                  # (a block stored raw is not a block to decode)
        assert len(which) > len(blocks) * 3 // 4
        src, soff, slen = pack_blocks([np.frombuffer(blocks[s][0][1], np.uint8) for s in which])
        caps = np.full(len(which), K1, np.int32)
        dst, doff = make_arena(caps, fill=0xCD)
        out = LZ4Codec.DecodeDictSetBatchPacked(src, soff, slen, dst, doff, caps, np.array([case.idx[s] for s in which], np.int32), dset)
    for k, s in enumerate(which):
        n = int(out[k])
        assert n > 0 and dst[int(doff[k]):int(doff[k]) + n].tobytes() == case.contents[s][:n].tobytes(), (s, case.settings[s], case.idx[s])


DEC_SETTINGS = [(True, K1, 0), (True, K64, 2), (False, K1, 0), (False, K64, 0), (True, 5 * K1, 1)]


@pytest.mark.parametrize("form", ["host", "device"])
def test_an_opened_decoder_is_one_given_reset_and_inject(form):
    """query words, a drain of everything held, and the next decoded block, beside RESET + a host Inject of the kept bytes"""
    case = opened("lengths_short")[0]
    entries = list(range(len(case.dict_len))) + [-1]
    settings = [st for _ in entries for st in DEC_SETTINGS]
    idx = [e for e in entries for _ in DEC_SETTINGS]
    make = DecoderHostForm if form == "host" else DecoderDeviceForm
    a, b = make(settings), make(settings)
    # the next block: what a chained L00 encoder primed with the same entry writes first (for -1: an unprimed one)
    first = {}
    with make_set(case) as dset:
        for s, e in enumerate(case.idx):
            if case.settings[s][1] == 0:
                first[e] = s
        blocks = encode_all(case, dset)
        from k4os.compression.lz4_amd.encoders import LZ4EncoderBatch
        plain = LZ4EncoderBatch([(True, 0, K1, 0)])
        _, ro, olen, data = plain.Run([[(case.contents[0][:K1], True, False)]])
        nxt = {e: blocks[s][0] for e, s in first.items()}
        nxt[-1] = (ro[0][0], data[0])
        got = open_decoders(a, form, idx, dset)
    kept = [case.dictionary(e)[-K64:].tobytes() if e >= 0 else None for e in idx]
    _, want, _ = b.run([[(True, k, 0)] if k is not None else [] for k in kept])
    assert got == want and any(g == -2 for g in got) and any(g == K64 for g in got)
    qa, qb = np.asarray(a.query()), np.asarray(b.query())
    assert np.array_equal(qa, qb)
    held = [int(x) for x in qa[:, 0]]
    assert a.drain([-h for h in held], held) == b.drain([-h for h in held], held)
    recs = [[(nxt[e][0] < 0, nxt[e][1], 0)] for e in idx]          # (a block stored raw goes through Inject)
    ra, rb = a.run(recs, drain=True, caps=[K1] * len(idx)), b.run(recs, drain=True, caps=[K1] * len(idx))
    assert ra == rb
    assert np.array_equal(np.asarray(a.query()), np.asarray(b.query()))
    for s, (e, setting) in enumerate(zip(idx, settings)):
        if got[s] >= 0 and (setting[0] or e < 0 or got[s] == 0):        # (an independent decoder has no history: its block may not decode)
            src = case.contents[first[e]] if e >= 0 else case.contents[0]
            assert ra[1][s] == len(ra[2][s]) > 0 and ra[2][s] == src[:ra[1][s]].tobytes(), (setting, e)


@pytest.mark.parametrize("form", ["host", "device"])
def test_reset_after_an_open_gives_a_never_primed_stream(form):
    case = opened("first_records")[0]
    n = len(case.settings)
    f, g, fresh = (FORMS[form](case.settings) for _ in range(3))

    def reset(x):
        x.b.Reset() if form == "host" else x.d.reset()
    with make_set(case) as dset:
        f.open(case.idx, dset)
        reset(f)
        g.open([-1] * n, dset)                       # no dictionary: open is RESET
    reset(fresh)
    for i in range(n):
        assert bytes(f.records[i]) == bytes(fresh.records[i]) == bytes(g.records[i])
    data = [b""] * n
    for call in case.calls:
        rf, rg, rn = f.run(call), g.run(call), fresh.run(call)
        assert rf == rn and rg == rn
        for i in range(n):
            assert f.ring(i) == fresh.ring(i) == g.ring(i)
            data[i] += rf[3][i]
    if PW.available():                               # and those are the witness's unprimed bytes
        for i, setting in enumerate(case.settings):
            w = PW.primed_encoder(*setting)
            want = b"".join(w.run(call[i])[2] for call in case.calls)
            w.close()
            assert data[i] == want, (setting, i)


def test_object_forms_with_a_dictionary():
    """LZ4Encoder.Create / LZ4Decoder.Create with dictionary=(set, index): Topup / Encode beside the witness, then Decode"""
    from k4os.compression.lz4_amd import LZ4Level
    from k4os.compression.lz4_amd.encoders import LZ4Encoder, LZ4Decoder
    case = PC.case("first_records")
    goldens_first = goldens()["first_records"]["streams"]
    with make_set(case) as dset:
        for s in (0, 1, 4, 6):                       # L00 and L03 on the 4 KiB entry, L00 and L09 on the 64 KiB entry
            chaining, level, B, extra = case.settings[s]
            e = case.idx[s]
            enc = LZ4Encoder.Create(chaining, LZ4Level(level), B, extra, dictionary=(dset, e))
            dec = LZ4Decoder.Create(chaining, B, extra, dictionary=(dset, e))
            assert enc.BytesReady == 0 and dec.BytesReady == min(int(case.dict_len[e]), K64)
            data = case.contents[s]
            target = np.zeros(B + B // 255 + 16, np.uint8)
            pos, outs = 0, []
            for piece, allow in ((1, True), (12, True), (B, True), (B, False)):     # the case's first four blocks and their allowCopy
                assert enc.Topup(data, pos, piece) == piece
                pos += piece
                n = enc.Encode(target, allowCopy=allow)
                outs.append(n)
                back = np.zeros(B, np.uint8)
                assert (dec.Inject(target, 0, -n) if n < 0 else dec.Decode(target, 0, n)) == piece
                dec.Drain(back, -piece, piece)
                assert back[:piece].tobytes() == data[pos - piece:pos].tobytes()
            want = [o for c in goldens_first[s]["calls"] for o in c[0] if o][:4]
            assert outs == want, (case.settings[s], e)
        # an independent decoder lives on the device when it is given a dictionary, and refuses one it cannot hold
        d = LZ4Decoder.Create(False, K64, 0, dictionary=(dset, 0))
        assert d.BytesReady == 4096
        from k4os.compression.lz4_amd.encoders import InvalidOperationException
        with pytest.raises(InvalidOperationException):
            LZ4Decoder.Create(False, K1, 0, dictionary=(dset, 0))
        with pytest.raises(ValueError):
            LZ4Encoder.Create(False, LZ4Level.L00_FAST, K1, 0, dictionary=(dset, 0))
        with pytest.raises(ValueError):              # the optimal parser's levels are not opened from a dictionary
            LZ4Encoder.Create(True, LZ4Level.L12_MAX, K1, 0, dictionary=(dset, 0))
