"""Many open ILZ4Decoders on the GPU (k4lz4_chain_decode_batch) against the witness, through the host form
(encoders.LZ4ChainDecoderBatch) and the device form (device.ChainDecoderDevice): the case list and the mutants with guard bytes
around every store and every slot, mixed decoders over many calls, the chain encoders' bytes decoded back, and a stream cut into
runs at every block boundary against k4lz4_decode_chain_batch on it whole."""
import numpy as np
import pytest

import chain_decoder_cases as K
import chain_decoder_witness as W
from test_chain_decoder_emu import undefined_mutants

pytestmark = pytest.mark.gpu
K1, K64 = 1024, 65536
GUARD = 256


class HostForm:
    """the driver interface of chain_decoder_cases.play over LZ4ChainDecoderBatch, its stores moved apart with guard bytes between
    them, in front of the first and behind the last (the drain slots are the library's own staging)"""

    def __init__(self, settings):
        import torch
        from k4os.compression.lz4_amd.encoders import LZ4ChainDecoderBatch
        self.b = b = LZ4ChainDecoderBatch(settings)
        self.n = b.n
        self.sizes = np.array([r.storeBytes for r in b.records[:b.n]], np.int64)
        off = GUARD + np.concatenate(([0], np.cumsum(self.sizes[:-1] + GUARD))).astype(np.int64)
        b.store = torch.full((int(self.sizes.sum()) + GUARD * (b.n + 2) + 256,), 0xA5, dtype=torch.uint8, device=b.store.device)
        b._base = (b.store.data_ptr() + 255) // 256 * 256
        b.store_off = off.astype(np.uint64)
        self.off = off + (b._base - b.store.data_ptr())
        b.Reset()
        self._stores_intact()

    def _stores_intact(self):
        s = self.b.store.cpu().numpy()
        mask = np.ones(s.size, bool)
        for o, c in zip(self.off, self.sizes):
            mask[int(o):int(o) + int(c)] = False
        assert (s[mask] == 0xA5).all(), "a write outside a stream's store"

    def reset(self, which=None):
        self.b.Reset(which)
        self._stores_intact()

    def run(self, records, drain=False, caps=None):
        got = self.b.Run(records, drain, caps)
        self._stores_intact()
        return got

    def drain(self, offsets, lengths):
        return self.b.Drain(offsets, lengths)

    def query(self):
        return self.b.Query()


def host_form(settings):
    return HostForm(settings)


class DeviceForm:
    """the driver interface of chain_decoder_cases.play over ChainDecoderDevice: every array a device tensor, the stores and the
    slots with guard bytes between them"""

    def __init__(self, settings):
        import torch
        from k4os.compression.lz4_amd.device import ChainDecoderDevice
        self.torch = torch
        self.cd = ChainDecoderDevice(settings)
        self.n, dev = self.cd.n, self.cd.dc.device
        self.dev = dev
        # the same stores, moved apart with guards between them
        sizes = self.cd.store_bytes
        off = GUARD + np.concatenate(([0], np.cumsum(sizes[:-1] + GUARD))).astype(np.int64)
        self.cd.store = torch.full((int(sizes.sum()) + GUARD * (self.n + 2) + 256,), 0xA5, dtype=torch.uint8, device=dev)
        off += (-self.cd.store.data_ptr()) % 256
        self.off, self.sizes = off, sizes
        self.cd.store_off = torch.from_numpy(off).to(dev)
        self.cd.reset()
        self._stores_intact()

    def _t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _stores_intact(self):
        s = self.cd.store.cpu().numpy()
        mask = np.ones(s.size, bool)
        for o, c in zip(self.off, self.sizes):
            mask[int(o):int(o) + int(c)] = False
        assert (s[mask] == 0xA5).all(), "a write outside a stream's store"

    def _slots(self, caps):
        caps = np.asarray(caps, np.int64)
        off = GUARD + np.concatenate(([0], np.cumsum(caps[:-1] + GUARD))).astype(np.int64)
        return self.torch.full((int(caps.sum()) + GUARD * (self.n + 1) + 16,), 0xCD, dtype=self.torch.uint8, device=self.dev), off

    def reset(self, which=None):
        assert which is None or list(which) == list(range(self.n))
        self.cd.reset()

    def run(self, records, drain=False, caps=None):
        torch, n = self.torch, self.n
        src, roff, rlen, rbs, first, nrec = W.record_table(records, 64)
        caps = np.zeros(n, np.int64) if caps is None else np.asarray(caps, np.int64)
        dst, doff = self._slots(caps)
        rec_out = torch.full((max(len(rlen), 1),), -999, dtype=torch.int32, device=self.dev)
        out = torch.full((n,), -999, dtype=torch.int64, device=self.dev)
        self.cd.run(self._t(src), self._t(roff.view(np.int64)), self._t(rlen.view(np.int32)), self._t(rbs), self._t(first.view(np.int64)),
                    self._t(nrec.view(np.int32)), rec_out, out, *((dst, self._t(doff), self._t(caps)) if drain else ()))
        torch.cuda.synchronize()
        self._stores_intact()
        rec_out, d = rec_out.cpu().numpy(), dst.cpu().numpy()
        ro = [rec_out[int(f):int(f) + int(k)].tolist() for f, k in zip(first, nrec)]
        given = [sum(r[:next((j for j, g in enumerate(r) if g < 0), len(r))]) if drain else 0 for r in ro]
        mask = np.ones(d.size, bool)
        for i in range(n):
            mask[int(doff[i]):int(doff[i]) + given[i]] = False
        assert (d[mask] == 0xCD).all(), "a write outside what a stream drained"
        return ro, out.cpu().numpy().tolist(), [d[int(doff[i]):int(doff[i]) + given[i]].tobytes() for i in range(n)]

    def drain(self, offsets, lengths):
        torch, n = self.torch, self.n
        lengths = np.asarray(lengths, np.int64)
        dst, doff = self._slots(np.clip(lengths, 0, 1 << 27))
        out = torch.full((n,), -999, dtype=torch.int64, device=self.dev)
        self.cd.drain(self._t(np.asarray(offsets, np.int64)), self._t(lengths), dst, self._t(doff), out)
        torch.cuda.synchronize()
        out, d = out.cpu().numpy(), dst.cpu().numpy()
        mask = np.ones(d.size, bool)
        for i in range(n):
            mask[int(doff[i]):int(doff[i]) + max(int(out[i]), 0)] = False
        assert (d[mask] == 0xCD).all(), "a write outside a drain's range"
        return [int(out[i]) if out[i] < 0 else d[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() for i in range(n)]

    def query(self):
        return self.cd.query().cpu().numpy()


FORMS = {"host": host_form, "device": DeviceForm}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k", range(len(K.BUILDERS)), ids=K.case_ids())
def test_case_against_the_witness(k, form):
    _, settings, calls = K.case(k)
    K.same(K.play(W.WitnessDecoders(settings), calls), K.play(FORMS[form](settings), calls))


_mutants = {}


@pytest.mark.parametrize("form", list(FORMS))
def test_mutants_against_the_witness(form):
    settings, calls = K.mutants()
    if not _mutants:
        _mutants["w"] = undefined_mutants(settings, calls)
    want, skip = _mutants["w"]
    K.same(want, K.play(FORMS[form](settings), calls), skip_bytes=skip)


@pytest.mark.parametrize("form", list(FORMS))
def test_64_mixed_decoders_in_12_calls(form):
    """chained and independent decoders of different block sizes in one call, some of them sitting a call out"""
    from oracle_lib import Oracle
    o = Oracle()
    rng = np.random.default_rng(77)
    settings, streams = [], []
    for s in range(64):
        B = int(rng.choice([K1, 4 * K1, K64]))
        if s % 3 == 2:
            settings.append((0, B, 0))
            streams.append([(False, o.encode(K.content(int(rng.integers(1, B + 1)), 1000 + 50 * s + j), 0), 0) for j in range(14)])
        else:
            settings.append((1, B, int(rng.integers(0, 3))))
            sizes = [int(x) for x in rng.integers(1, B + 1, 14)]
            blocks = K.chain_blocks(K.content(sum(sizes), 1000 + s), sizes, B, "fast" if s % 2 else "hc")
            streams.append([(bool(rng.random() < 0.2), None, 0) for _ in blocks])
            streams[-1] = [(inj, raw if inj else p, 0) for (inj, _, _), (raw, p) in zip(streams[-1], blocks)]
    calls = []
    for c in range(12):
        take = [int(rng.integers(0, 3)) for _ in range(64)]
        calls.append(("run", [st[:t] for st, t in zip(streams, take)], c % 2 == 0, [3 * K64] * 64))
        streams = [st[t:] for st, t in zip(streams, take)]
    K.same(K.play(W.WitnessDecoders(settings), calls), K.play(FORMS[form](settings), calls))


@pytest.mark.parametrize("form", list(FORMS))
def test_a_call_in_which_no_stream_has_a_record(form):
    """the record table is empty (on the device its arrays are empty tensors, whose pointers are NULL): every decoder is untouched"""
    sizes = [700, 900]
    blocks = K.dec(K.chain_blocks(K.content(sum(sizes), 9), sizes, K1))
    calls = [("run", [blocks[:1], []], True, [K1] * 2), ("run", [[], []], True, [K1] * 2), ("run", [[], []], False, None),
             ("run", [blocks[1:], []], True, [K1] * 2)]
    K.same(K.play(W.WitnessDecoders([(1, K1, 0)] * 2), calls), K.play(FORMS[form]([(1, K1, 0)] * 2), calls))


def test_chain_encoders_bytes_decoded_back_through_the_device_form():
    from k4os.compression.lz4_amd.encoders import LZ4FastChainEncoder, LZ4HighChainEncoder
    data = K.content(5 * K64 + 1234, 5)
    for enc in (LZ4FastChainEncoder(K64, 0), LZ4HighChainEncoder(blockSize=K64, extraBlocks=1)):
        pieces = [data[i:i + K64] for i in range(0, data.size, K64)]
        blocks = enc.EncodeBlocks(pieces, allowCopy=True)
        recs = [(int(a) == 3, payload, 0) for a, payload in blocks]         # EncoderAction.Copied: an uncompressed-yet-chained block
        d = DeviceForm([(1, K64, 0)])
        out = b""
        for k in range(0, len(recs), 2):
            ro, total, got = d.run([recs[k:k + 2]], True, [2 * K64])
            assert total[0] == sum(ro[0]) == len(got[0])
            out += got[0]
        assert out == data.tobytes()


def test_runs_at_every_block_boundary_equal_the_whole_stream_decode():
    """one chained stream: decoded whole by k4lz4_decode_chain_batch, and cut into two runs at every block boundary"""
    from k4os.compression.lz4_amd import _native
    sizes = [int(x) for x in np.random.default_rng(3).integers(1, 4 * K1 + 1, 24)]
    data = K.content(sum(sizes), 3)
    blocks = K.chain_blocks(data, sizes, 4 * K1)
    ctx = _native.default_context()
    src = np.frombuffer(b"".join(p for _, p in blocks), np.uint8)
    blen = np.array([len(p) for _, p in blocks], np.uint32)
    boff = np.concatenate(([0], np.cumsum(blen[:-1].astype(np.uint64)))).astype(np.uint64)
    whole = np.zeros(data.size, np.uint8)
    out = np.zeros(1, np.int64)
    first, count, bsz, chained = np.zeros(1, np.uint64), np.array([len(blocks)], np.uint32), np.array([4 * K1], np.int32), np.ones(1, np.uint8)
    doff, dcap = np.zeros(1, np.uint64), np.array([data.size], np.uint64)       # named: the call holds their addresses only
    ctx.check(ctx.lib.k4lz4_decode_chain_batch(ctx.handle, src.ctypes.data, boff.ctypes.data, blen.ctypes.data, len(blocks), first.ctypes.data,
                                               count.ctypes.data, bsz.ctypes.data, chained.ctypes.data, whole.ctypes.data, doff.ctypes.data,
                                               dcap.ctypes.data, out.ctypes.data, 1))
    assert out[0] == data.size and whole.tobytes() == data.tobytes()
    n = len(blocks) + 1
    d = host_form([(1, 4 * K1, 0)] * n)                                     # decoder c: blocks [0, c), then [c, end)
    recs = K.dec(blocks)
    _, t1, g1 = d.run([recs[:c] for c in range(n)], True, [data.size] * n)
    _, t2, g2 = d.run([recs[c:] for c in range(n)], True, [data.size] * n)
    for c in range(n):
        assert t1[c] + t2[c] == data.size and g1[c] + g2[c] == whole.tobytes(), c
