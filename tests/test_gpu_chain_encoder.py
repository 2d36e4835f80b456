"""Many open ILZ4Encoders on the GPU (k4lz4_chain_encode_batch) against the witness, through the host form
(encoders.LZ4EncoderBatch) and the device form (device.ChainEncoderDevice), with the stores apart and guard bytes between them:
every call's bytes, recLoaded and recOut, the ring and the fast-chain state read back from the store after every call, the target
refusal, the blocks decoded back by LZ4ChainDecoderBatch, and a whole content written at once against the whole-stream encoders."""
import functools

import numpy as np
import pytest

import chain_encoder_cases as CC
from chain_encoder_witness import WitnessEncoder

pytestmark = pytest.mark.gpu
K1, K64 = 1024, 65536
GUARD = 256


def spread_stores(store, sizes, n):
    """a store of its own for every stream, guard bytes (0xA5) in front, between and behind -> (tensor, offsets from the aligned base)"""
    import torch
    off = GUARD + np.concatenate(([0], np.cumsum(sizes[:-1] + GUARD))).astype(np.int64) if n else np.zeros(0, np.int64)
    t = torch.full((int(sizes.sum()) + GUARD * (n + 2) + 256,), 0xA5, dtype=torch.uint8, device=store.device)
    return t, off


class HostForm:
    def __init__(self, settings):
        from k4os.compression.lz4_amd.encoders import LZ4EncoderBatch
        self.b = b = LZ4EncoderBatch(settings)
        self.sizes = np.array([r.storeBytes for r in b.records[:b.n]], np.int64)
        b.store, off = spread_stores(b.store, self.sizes, b.n)
        b._base = (b.store.data_ptr() + 255) // 256 * 256
        b.store_off = off.astype(np.uint64)
        self.off = off + (b._base - b.store.data_ptr())

    def intact(self):
        s = self.b.store.cpu().numpy()
        mask = np.ones(s.size, bool)
        for o, c in zip(self.off, self.sizes):
            mask[int(o):int(o) + int(c)] = False
        assert (s[mask] == 0xA5).all(), "a write outside a stream's store"

    def run(self, records, caps=None):
        got = self.b.Run(records, caps)
        self.intact()
        return got

    records = property(lambda self: self.b.records)
    ring = lambda self, i: self.b.Ring(i)      # noqa: E731
    state = lambda self, i: self.b.State(i)    # noqa: E731


class DeviceForm:
    def __init__(self, settings):
        from k4os.compression.lz4_amd.device import ChainEncoderDevice
        self.d = d = ChainEncoderDevice(settings)
        self.sizes = d.store_bytes
        d.store, off = spread_stores(d.store, self.sizes, d.n)
        d._base = (d.store.data_ptr() + 255) // 256 * 256
        d.store_off = off.astype(np.uint64)
        self.off = off + (d._base - d.store.data_ptr())
        self.b = self      # (ring / state below)

    intact = HostForm.intact
    records = property(lambda self: self.d.records)
    store = property(lambda self: self.d.store)

    def run(self, records, caps=None):
        import torch
        from k4os.compression.lz4_amd.encoders import encoder_record_table
        d = self.d
        src, roff, rlen, rflags, first, nrec = encoder_record_table(records)
        if caps is None:
            caps = [d.bound(i, rlen[int(f):int(f) + int(k)], rflags[int(f):int(f) + int(k)]) for i, (f, k) in enumerate(zip(first, nrec))]
        caps = np.asarray(caps, np.uint64)
        doff = (GUARD + np.concatenate(([0], np.cumsum(caps[:-1] + np.uint64(GUARD))))).astype(np.uint64)
        dev = d.dc.device
        dst = torch.full((int(caps.sum()) + GUARD * (d.n + 2),), 0xCD, dtype=torch.uint8, device=dev)
        nr = max(int(rlen.size), 1)
        loaded = torch.full((nr,), -77, dtype=torch.int32, device=dev)
        out = torch.full((nr,), -77, dtype=torch.int32, device=dev)
        olen = torch.full((d.n,), -77, dtype=torch.int64, device=dev)
        d.run(torch.from_numpy(src).to(dev), roff, rlen, rflags, first, nrec, dst, doff, caps, loaded, out, olen)
        torch.cuda.synchronize()
        self.intact()
        h, olen = dst.cpu().numpy(), olen.cpu().numpy()
        mask = np.ones(h.size, bool)
        data = []
        for i in range(d.n):
            mask[int(doff[i]):int(doff[i]) + int(caps[i])] = False
            used = max(int(olen[i]), 0)
            data.append(h[int(doff[i]):int(doff[i]) + used].tobytes())
            assert (h[int(doff[i]) + used:int(doff[i]) + int(caps[i])] == 0xCD).all(), "bytes behind the run's total"
        assert (h[mask] == 0xCD).all(), "a write outside a stream's target"
        cut = lambda a: [a.cpu().numpy()[int(f):int(f) + int(k)].tolist() for f, k in zip(first, nrec)]  # noqa: E731
        return cut(loaded), cut(out), olen.tolist(), data

    def ring(self, i):
        r = self.d.records[i]
        from k4os.compression.lz4_amd.encoders import _ring_at
        at = int(self.off[i]) + _ring_at(r)
        return self.d.store[at:at + int(r.pointer)].cpu().numpy().tobytes()

    def state(self, i):
        from k4os.compression.lz4_amd.encoders import FAST_CHAIN_STATE
        at = int(self.off[i])
        return np.frombuffer(self.d.store[at:at + FAST_CHAIN_STATE.itemsize].cpu().numpy().tobytes(), FAST_CHAIN_STATE).copy()


FORMS = {"host": HostForm, "device": DeviceForm}


@functools.lru_cache(maxsize=None)
def witnessed(name):
    """the case and, computed once, the witness's results per call and stream: (loaded, out, bytes, ring, fast state or None)"""
    settings, calls = CASES[name]()
    ws = [WitnessEncoder(*s) for s in settings]
    want = []
    for call in calls:
        row = []
        for w, recs in zip(ws, call):
            loaded, out, data = w.run(recs)
            st = w.codec.state() if w.kind == 2 and recs else None
            row.append((loaded, out, data, w.ring(), st))
        want.append(row)
    for w in ws:
        w.close()
    return settings, calls, want


CASES = {
    "small": CC.small_case,
    "b64k_x0": lambda: CC.big_case(K64, 0, [0, 3, 9]),
    "b64k_x2": lambda: CC.big_case(K64, 2, [0, 12]),
    "b64k_ind": lambda: CC.big_case(K64, 0, [0, 3], chaining=False),
    "b256k": lambda: CC.big_case(256 * K1, 0, [3, 10]),
    "records": CC.record_cases,
    "mixed": CC.mixed_case,
}


def play(form, name):
    settings, calls, want = witnessed(name)
    f = FORMS[form](settings)
    for c, (call, row) in enumerate(zip(calls, want)):
        before = [bytes(f.records[i]) for i in range(len(settings))]
        loaded, out, olen, data = f.run(call)
        for i, (recs, (wl, wo, wd, wring, wst)) in enumerate(zip(call, row)):
            tag = (name, c, i, settings[i])
            if not recs:
                assert olen[i] == 0 and bytes(f.records[i]) == before[i], tag
            assert loaded[i] == wl, tag
            assert out[i] == wo, tag
            assert olen[i] == len(wd) and data[i] == wd, tag
            assert f.ring(i) == wring, tag
            if wst is not None and any(o for o in wo):
                st = f.state(i)[0]
                assert np.array_equal(st["hashTable"], wst["hashTable"]), tag
                assert int(st["currentOffset"]) == wst["currentOffset"] and int(st["dictSize"]) == wst["dictSize"], tag
                assert (f.records[i].currentOffset, f.records[i].dictSize) == (wst["currentOffset"], wst["dictSize"]), tag


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", ["small", "b64k_x0", "b64k_x2", "b64k_ind", "b256k", "records", "mixed"])
def test_every_call_equals_the_witness(form, name):
    play(form, name)


def test_small_case_saves_take_every_residue():
    assert CC._assert_residues() == set(range(16))


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("chaining", [True, False])
def test_four_mib_blocks(chaining, form):
    """B = 4 MiB at L00, 1.5 blocks"""
    B = 4 << 20
    data = CC.content(B + B // 2, 21)
    recs = [(data[:B // 2], False, True), (data[B // 2:B + 100], False, True), (data[B + 100:], False, True), (data[:0], True, True)]
    w = WitnessEncoder(chaining, 0, B, 0)
    f = FORMS[form]([(chaining, 0, B, 0)])
    for r in recs:
        wl, wo, wd = w.run([r])
        loaded, out, olen, got = f.run([[r]])
        assert (loaded[0], out[0], got[0]) == (wl, wo, wd)
        assert f.ring(0) == w.ring()
    w.close()


@pytest.mark.parametrize("form", ["host", "device"])
def test_target_one_byte_below_the_bound_leaves_the_stream(form):
    settings = [(True, 0, K1, 0), (True, 9, K1, 0), (False, 0, K1, 0)]
    data = CC.content(8 * K1, 31)
    warm = [[(data[:1500], False, True)] for _ in settings]
    run = [[(data[1500:3000], False, True), (data[3000:3100], True, False)] for _ in settings]
    ws = [WitnessEncoder(*s) for s in settings]
    f = FORMS[form](settings)
    for w, r in zip(ws, warm):
        w.run(r)
    f.run(warm)
    bound = [K1 + (100 + 100 // 255 + 16)] * 3       # one full block under allowCopy, one forced block of 100 bytes without it
    before = [bytes(f.records[i]) for i in range(3)]
    rings = [f.ring(i) for i in range(3)]
    store = f.b.store.cpu().numpy().copy() if form == "host" else f.store.cpu().numpy().copy()
    caps = [bound[0] - 1, bound[1], bound[2] - 1]
    loaded, out, olen, got = f.run(run, caps)
    wl, wo, wd = ws[1].run(run[1])
    assert (loaded[1], out[1], got[1]) == (wl, wo, wd)
    for i in (0, 2):
        assert olen[i] == -1 and loaded[i] == [0, 0] and out[i] == [0, 0] and got[i] == b""
        assert bytes(f.records[i]) == before[i] and f.ring(i) == rings[i]
    after = f.b.store.cpu().numpy() if form == "host" else f.store.cpu().numpy()
    for i in (0, 2):
        o, c = int(f.off[i]), int(f.sizes[i])
        assert np.array_equal(after[o:o + c], store[o:o + c])
    # the retried run gives the witness's bytes
    loaded, out, olen, got = f.run([run[0], [], run[2]], [bound[0], 0, bound[2]])
    for i in (0, 2):
        wl, wo, wd = ws[i].run(run[i])
        assert (loaded[i], out[i], got[i]) == (wl, wo, wd) and f.ring(i) == ws[i].ring()
    for w in ws:
        w.close()


def test_round_trip_through_the_chain_decoder():
    """each stream's blocks, fed block by block to LZ4ChainDecoderBatch with matching settings, return the content; raw blocks go
    through Inject"""
    from k4os.compression.lz4_amd.encoders import LZ4EncoderBatch, LZ4ChainDecoderBatch
    settings = [(True, 0, K1, 0), (True, 9, 4 * K1, 1), (False, 3, 2 * K1, 0), (True, 0, K64, 0)]
    rng = np.random.default_rng(41)
    contents = [np.concatenate([CC.content(30 * K1, 50 + i), CC.content(3 * K1, 60 + i, "random"), CC.content(40 * K1 + i, 70 + i)]) for i in range(4)]
    enc = LZ4EncoderBatch(settings)
    runs = [CC.offer_all(c, (max(s[2], K1) + K1 - 1) // K1 * K1, [int(rng.integers(1, 9000)) for _ in range(200)], rng, p_force=0.2) + [(c[:0], True, True)]
            for c, s in zip(contents, settings)]
    _, rec_out, olen, data = enc.Run(runs)
    dec = LZ4ChainDecoderBatch([(s[0], s[2], s[3]) for s in settings])
    blocks = LZ4EncoderBatch.blocks_of(rec_out, olen, data)
    caps = [c.size for c in contents]
    ro, out, got = dec.Run([[(o < 0, b, 0) for o, b in bl] for bl in blocks], drain=True, caps=caps)
    for i, c in enumerate(contents):
        assert out[i] == c.size and got[i] == c.tobytes(), i


def test_one_write_and_a_flush_equal_the_whole_stream_encoders():
    from k4os.compression.lz4_amd import encoders as E
    from k4os.compression.lz4_amd import LZ4Level
    settings = [(True, 9, K64, 0), (True, 0, K64, 1), (False, 0, K64, 0)]
    contents = [CC.content(5 * K64 + 1234 + i, 80 + i) for i in range(3)]
    b = E.LZ4EncoderBatch(settings)
    got = [x + y for x, y in zip(b.Write(contents), b.Flush())]

    def whole(out, arena, boff):
        return [(int(n), arena[int(o):int(o) + abs(int(n))].tobytes()) for n, o in zip(out, boff)]
    out, arena, boff, _ = E.encode_hc_chain_packed([contents[0]], K64, 0, LZ4Level.L09_HC, True)
    assert got[0] == whole(out, arena, boff)
    out, arena, boff, _, _ = E.encode_fast_chain_packed([contents[1]], K64, 1, True)
    assert got[1] == whole(out, arena, boff)
    blocks = [contents[2][k:k + K64] for k in range(0, contents[2].size, K64)]
    out, arena, boff = E.encode_blocks_packed(blocks, LZ4Level.L00_FAST, True)
    assert got[2] == whole(out, arena, boff)
