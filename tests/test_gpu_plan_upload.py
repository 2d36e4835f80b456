"""The plan upload (k4lz4_capi.hip: PlanUpload, plan_begin, plan_send) under two device-form calls of one family enqueued back
to back on one non-default stream, with no synchronisation between them: the second call has another stream count and other lengths,
so its plan differs in size and content, and it may write the context's host copy only once the first call's upload has left it.
After one synchronisation both results are compared byte for byte with the family's witness (liblz4 1.9.3 through the witnesses'
transcriptions; for the frame decoder, the content the frames were made of).  One case per plan and family.

What it shows: that a call's plan, laid out anew in another size and with other content, leaves the results of the call before it
as they were.  What it does not show: that a missing wait would be caught -- the host copies are pageable memory, which the runtime
may have taken a copy of before hipMemcpyAsync returns, and nobody has run these cases with the wait taken out."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

import dict_encode_witness as DW
import dict_hc_encode_witness as DHW
import fast_chain_witness as FW
import hc_chain_witness as HW
from chain_encoder_witness import WitnessEncoder
from frame_writer_witness import WitnessWriter
from legacy_stream_witness import WriterCalls
from legacy_witness import Witness
from oracle_lib import Oracle
from k4os.compression.lz4_amd import LZ4Codec, LZ4Frame, LZ4EncoderSettings, LZ4Level, DictionarySet, corpus, _native
from k4os.compression.lz4_amd import legacy as L
from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec, ChainEncoderDevice
from k4os.compression.lz4_amd.encoders import FAST_CHAIN_STATE, encode_fast_chain_device, encoder_record_table
from k4os.compression.lz4_amd.frames import FrameWriterDevice, decode_frames_device

pytestmark = pytest.mark.gpu
K1, K64 = 1024, 65536
FIRST, SECOND = [1 * K1, 5 * K1, 70 * K1], [3 * K1]       # the two calls' streams: three, then one


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


@pytest.fixture(scope="module")
def text():
    return corpus.class_bytes("dickens", 400000, 21)


def contents(text, sizes, at):
    """one piece of the text per size, from `at` on"""
    out = []
    for n in sizes:
        out.append(text[at:at + n])
        at += n
    return out


def packed(dev, pieces):
    """-> (device bytes, offsets, lengths)"""
    lens = np.array([p.size for p in pieces], np.int64)
    off = np.concatenate(([0], np.cumsum(lens)))[:-1].astype(np.int64)
    return torch.from_numpy(np.concatenate(pieces + [np.zeros(1, np.uint8)])).to(dev), off, lens


def cut(buf, off, length):
    h, n = buf.cpu().numpy(), length.cpu().numpy() if isinstance(length, torch.Tensor) else length
    return [h[int(o):int(o) + int(k)].tobytes() for o, k in zip(off, n)]


def blocks_of(out, arena, boff):
    """the chained stream calls' results -> [(outLen, bytes)] per block"""
    o, a = out.cpu().numpy(), arena.cpu().numpy()
    return [(int(n), a[int(at):int(at) + abs(int(n))].tobytes()) for n, at in zip(o, boff)]


# ---- the cases: prepare(dc, text) stages every input of both calls and returns (first, second, check); first() and second() only
# enqueue, check(a, b) runs after the one synchronisation ---------------------------------------------------------------------------
def frame_writer(dc, text):
    sets = ([LZ4EncoderSettings(ContentChecksum=True), LZ4EncoderSettings(ChainBlocks=True, CompressionLevel=LZ4Level.L03_HC, BlockChecksum=True),
             LZ4EncoderSettings(ChainBlocks=True)], [LZ4EncoderSettings(ChainBlocks=True, BlockChecksum=True)])
    pieces = (contents(text, FIRST, 0), contents(text, SECOND, 100000))
    staged = [packed(dc.device, p) for p in pieces]
    writers = [FrameWriterDevice(dc, len(s), s) for s in sets]
    oracle = Oracle()

    def check(*got):
        for k, (out, ooff, olen) in enumerate(got):
            want = [WitnessWriter(s, oracle=oracle).write_close(p) for s, p in zip(sets[k], pieces[k])]
            assert cut(out, ooff, olen) == want, k
    return (lambda: writers[0].close(*staged[0])), (lambda: writers[1].close(*staged[1])), check


def legacy_writer(dc, text):
    B = 16 * K1
    high = ([False, True, False], [True])
    pieces = (contents(text, FIRST, 0), contents(text, SECOND, 100000))
    staged = [packed(dc.device, p) for p in pieces]
    writers = [L.LegacyWriterDevice(dc, len(h), h, B) for h in high]
    w = Witness()

    def check(*got):
        for k, (out, ooff, olen) in enumerate(got):
            want = [WriterCalls(w, h, B).dispose(p.tobytes()) for h, p in zip(high[k], pieces[k])]
            assert cut(out, ooff, olen) == want, k
    return (lambda: writers[0].close(*staged[0])), (lambda: writers[1].close(*staged[1])), check


class EncoderRun:
    """one k4lz4_chain_encode_batch_device call of a ChainEncoderDevice, every input staged: one forced record per stream"""

    def __init__(self, dc, settings, pieces):
        self.settings, self.pieces = settings, pieces
        self.d = d = ChainEncoderDevice(settings, dc)
        self.records = [[(p.tobytes(), True, True)] for p in pieces]
        src, self.roff, self.rlen, self.rflags, self.first, self.nrec = encoder_record_table(self.records)
        self.caps = np.array([d.bound(i, self.rlen[i:i + 1], self.rflags[i:i + 1]) for i in range(d.n)], np.uint64)
        self.doff = np.concatenate(([0], np.cumsum((self.caps[:-1] + np.uint64(15)) // np.uint64(16) * np.uint64(16)))).astype(np.uint64)
        dev = dc.device
        self.src = torch.from_numpy(src).to(dev)
        self.dst = torch.full((int(self.caps.sum()) + 16 * d.n + 64,), 0xCD, dtype=torch.uint8, device=dev)
        self.loaded = torch.full((d.n,), -77, dtype=torch.int32, device=dev)
        self.out = torch.full((d.n,), -77, dtype=torch.int32, device=dev)
        self.olen = torch.full((d.n,), -77, dtype=torch.int64, device=dev)

    def __call__(self):
        self.d.run(self.src, self.roff, self.rlen, self.rflags, self.first, self.nrec, self.dst, self.doff, self.caps, self.loaded, self.out,
                   self.olen)

    def check(self):
        data = cut(self.dst, self.doff, self.olen)
        loaded, out = self.loaded.cpu().numpy().tolist(), self.out.cpu().numpy().tolist()
        for i, (s, recs) in enumerate(zip(self.settings, self.records)):
            w = WitnessEncoder(*s)
            wl, wo, wd = w.run(recs)
            w.close()
            assert ([loaded[i]], [out[i]], data[i]) == (wl, wo, wd), (i, s)

    def fast_state(self, i):
        at = int(self.d.store_off[i]) + (self.d._base - self.d.store.data_ptr())
        return self.d.store[at:at + FAST_CHAIN_STATE.itemsize].cpu().numpy()


def chain_encoder_encode(dc, text):
    a = EncoderRun(dc, [(True, 0, K64, 0), (True, 3, K64, 0), (False, 0, K64, 0)], contents(text, FIRST, 0))
    b = EncoderRun(dc, [(True, 3, 4 * K1, 1)], contents(text, SECOND, 100000))
    return a, b, lambda *_: (a.check(), b.check())


def chain_encoder_reset(dc, text):
    """RESET of three fast-chain encoders that have encoded (its plan: the three pieces that clear their states), then a run of one"""
    a = EncoderRun(dc, [(True, 0, K64, 0)] * 3, contents(text, FIRST, 0))
    b = EncoderRun(dc, [(True, 0, 4 * K1, 0)], contents(text, SECOND, 100000))
    a()
    dc.ctx.synchronize(dc._stream())
    a.check()
    assert all(a.fast_state(i).any() for i in range(3))

    def check(*_):
        assert not any(a.fast_state(i).any() for i in range(3)), "a state RESET did not clear"
        assert all(r.pointer == 0 and r.currentOffset == 0 for r in a.d.records[:3])
        b.check()
    return a.d.reset, b, check


def hc_chain_streams(dc, text):
    level, bs = 3, 16 * K1
    pieces = (contents(text, FIRST, 0), contents(text, SECOND, 100000))
    calls = []
    for p in pieces:
        data, off, lens = packed(dc.device, p)
        nblk = (lens + bs - 1) // bs
        slot = bs + bs // 255 + 16
        doff = np.concatenate(([0], np.cumsum(nblk * slot)))[:-1].astype(np.uint64)
        nb = int(nblk.sum())
        arena = torch.full((nb * slot + 64,), 0xCD, dtype=torch.uint8, device=dc.device)
        out = torch.zeros(nb, dtype=torch.int32, device=dc.device)
        boff = np.concatenate([doff[s] + np.arange(nblk[s], dtype=np.uint64) * np.uint64(slot) for s in range(len(p))])
        args = (data, off.astype(np.uint64), lens, np.full(len(p), bs, np.int32), np.zeros(len(p), np.int32), doff)
        calls.append((args, arena, out, boff, nb))

    def run(k):
        (data, off, lens, bsz, ext, doff), arena, out, boff, nb = calls[k]
        dc.ctx.check(dc.lib.k4lz4_encode_hc_chain_batch_device(dc.ctx.handle, data.data_ptr(), off.ctypes.data, lens.ctypes.data, bsz.ctypes.data,
                                                               ext.ctypes.data, None, len(lens), arena.data_ptr(), doff.ctypes.data,
                                                               out.data_ptr(), nb, level, _native.FLAG_ALLOW_COPY, C.c_void_p(dc._stream())))

    def check(*_):
        for k, (_, arena, out, boff, _) in enumerate(calls):
            want = [b for c in pieces[k] for b in HW.witness_blocks(c, level, bs, 0)]
            assert blocks_of(out, arena, boff) == want, k
    return (lambda: run(0)), (lambda: run(1)), check


def fast_chain_streams(dc, text):
    bs = 16 * K1
    pieces = (contents(text, FIRST, 0), contents(text, SECOND, 100000))
    staged = [packed(dc.device, p) for p in pieces]

    def check(*got):
        for k, (out, arena, boff, nblk, _) in enumerate(got):
            want = [b for c in pieces[k] for b in FW.witness_stream(c, bs, 0)[0]]
            assert blocks_of(out, arena, boff) == want, k
    return (lambda: encode_fast_chain_device(dc, *staged[0], bs)), (lambda: encode_fast_chain_device(dc, *staged[1], bs)), check


def dict_encode(level, witness):
    def prepare(dc, text):
        dicts = ([text[200000:208000], text[210000:250000]], [text[260000:263000]])
        index = ([0, 1, 0], [0])
        pieces = (contents(text, FIRST, 205000), contents(text, SECOND, 261000))
        calls = []
        for d, ix, p in zip(dicts, index, pieces):
            data, off, lens = packed(dc.device, p)
            src = DeviceBatch(data, torch.from_numpy(off).to(dc.device), torch.from_numpy(lens.astype(np.int32)).to(dc.device))
            dst = DeviceBatch.empty_slots([LZ4Codec.MaximumOutputSize(int(n)) for n in lens], dc.device, fill=0xCD)
            dd, doff, dlen = packed(dc.device, d)
            calls.append((src, dst, torch.from_numpy(np.array(ix, np.int32)).to(dc.device), dd, doff, dlen, dc.new_out_len(len(p))))

        def run(k):
            src, dst, ix, dd, doff, dlen, out = calls[k]
            dc.encode_dict(src, dst, ix, dd, doff, dlen, out_len=out, level=LZ4Level(level))

        def check(*_):
            for k, (src, dst, _, _, _, _, out) in enumerate(calls):
                o = out.cpu().numpy()
                got = cut(dst.data, dst.off.cpu().numpy(), np.maximum(o, 0))
                for i, p in enumerate(pieces[k]):
                    r, want = witness(p, dicts[k][index[k][i]], LZ4Codec.MaximumOutputSize(p.size))
                    assert (int(o[i]), got[i]) == (r, want), (k, i)
        return (lambda: run(0)), (lambda: run(1)), check
    return prepare


def frames_dictset(dc, text):
    """frames that name a DictID, written by LZ4Frame.EncodeBatch against a set of two entries and a set of one; read back against them.
    k4lz4_decode_frames_dictset_device waits for the stream inside the call (it reads the block count back), so the first call's id
    table has gone up before the second call begins: this case covers the change of the table's size and content between calls, not
    the wait of fdict_plan's protocol."""
    dicts = ([text[200000:208000], text[210000:250000]], [text[260000:263000]])
    ids = ([7, 9], [5])
    index = ([0, 1, 0], [0])
    pieces = (contents(text, FIRST, 205000), contents(text, SECOND, 261000))
    sets = [DictionarySet(d, owner=dc) for d in dicts]
    calls = []
    for k, p in enumerate(pieces):
        chained = LZ4EncoderSettings(ChainBlocks=True, ContentChecksum=True)
        frames = LZ4Frame.EncodeBatch(p, chained if k == 0 else LZ4EncoderSettings(), ctx=dc.ctx, dictionary=(sets[k], ids[k]), dict_index=index[k])
        data, off, lens = packed(dc.device, [np.frombuffer(f, np.uint8) for f in frames])
        cap = np.array([c.size for c in p], np.int64)
        o_off = np.concatenate(([0], np.cumsum((cap + 15) // 16 * 16)))[:-1]
        buf = torch.full((int(o_off[-1] + cap[-1]) + 64,), 0xCD, dtype=torch.uint8, device=dc.device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(dc.device)      # noqa: E731
        calls.append((data, t(off), t(lens), (buf, t(o_off), t(cap)), o_off))

    def run(k):
        data, off, lens, out, _ = calls[k]
        return decode_frames_device(dc, data, off, lens, out=out, raise_errors=False, dictionary=(sets[k], ids[k]))[2]

    def check(*got):
        for k, olen in enumerate(got):
            assert olen.cpu().numpy().tolist() == [c.size for c in pieces[k]], k
            assert cut(calls[k][3][0], calls[k][4], olen) == [c.tobytes() for c in pieces[k]], k
        for s in sets:
            s.close()
    return (lambda: run(0)), (lambda: run(1)), check


def dict_witness(message, dictionary, cap):
    r, data = DW.encode(message, dictionary, cap)
    return DW.codec_result(message.size, r), data


def dict_hc_witness(message, dictionary, cap):
    r, data = DHW.encode(message, dictionary, cap, 9)
    return DHW.codec_result(message.size, r), data


CASES = {
    "frame_writer": frame_writer,
    "legacy_writer": legacy_writer,
    "chain_encoder_encode": chain_encoder_encode,
    "chain_encoder_reset": chain_encoder_reset,
    "hc_chain_streams": hc_chain_streams,
    "fast_chain_streams": fast_chain_streams,
    "dict_encode": dict_encode(0, dict_witness),
    "dict_hc_encode": dict_encode(9, dict_hc_witness),
    "frames_dictset": frames_dictset,
}


@pytest.mark.parametrize("case", CASES)
def test_two_calls_back_to_back_on_one_stream(dc, text, case):
    side = torch.cuda.Stream(dc.device)
    with torch.cuda.stream(side):
        first, second, check = CASES[case](dc, text)
        dc.ctx.synchronize(side.cuda_stream)          # the staging is over; from here on nothing waits but the end
        a = first()
        b = second()
        dc.ctx.synchronize(side.cuda_stream)
        check(a, b)
