"""The incremental LZ4Stream reader fed its source in pieces, on the GPU (k4lz4_legacy_feed.hpp through the C ABI, host and device
form): logical reads (frame_feed_cases.FedDriver) against legacy_stream_witness.Reader over the WHOLE source.  Guard bytes lie around
every output slot, every store and every piece and are checked after every call."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

import legacy_feed_cases as LC
from legacy_witness import Witness
from test_legacy_host import valid_streams, damaged_streams
from k4os.compression.lz4_amd import corpus
from k4os.compression.lz4_amd import legacy as L
from k4os.compression.lz4_amd.device import DeviceCodec, _dp

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


@pytest.fixture(scope="module")
def w():
    return Witness()


def _guarded(lens, fill):
    lens = np.asarray(lens, np.int64)
    off = (GUARD + np.concatenate(([0], np.cumsum(lens[:-1] + GUARD)))).astype(np.uint64) if len(lens) else np.zeros(0, np.uint64)
    return np.full(int(lens.sum()) + GUARD * (len(lens) + 1) + 16, fill, np.uint8), off


def _intact(buf, off, caps, fill, what):
    mask = np.ones(buf.size, bool)
    for o, c in zip(off, caps):
        mask[int(o):int(o) + int(c)] = False
    assert (buf[mask] == fill).all(), f"a write outside {what}"


class GpuFedReaders:
    """n fed readers behind FedDriver's raw.call: one k4lz4_legacy_read_fed_batch (form "host") or _device (form "device") per call"""

    def __init__(self, dc, n, max_block, form, direct=True, max_count=None):
        self.dc, self.n, self.form, self.direct, self.max_count = dc, n, form, direct, max_count
        self.lib = dc.lib
        self.record = L.legacy_reader_record(max_block, dc.lib, fed=True)
        sb = int(self.record.storeBytes)
        self.store_off = (256 + np.arange(n, dtype=np.uint64) * np.uint64(sb + 256)).astype(np.uint64)
        self.store = torch.full((n * (sb + 256) + 256,), 0xA5, dtype=torch.uint8, device=dc.device)
        g = (np.arange(n + 1, dtype=np.int64) * (sb + 256))[:, None] + np.arange(256, dtype=np.int64)[None, :]
        self.guard_idx = torch.from_numpy(g.reshape(-1)).to(dc.device)
        self.store_off_d = torch.from_numpy(self.store_off.astype(np.int64)).to(dc.device)
        self.call(LC.RESET, [b""] * n, np.zeros(n, np.int64), np.zeros(n, np.int64), False)

    def call(self, op, pieces, final, counts, interactive):
        n, lib, dev = self.n, self.lib, self.dc.device
        counts = np.ascontiguousarray(counts, np.int64)
        final = np.ascontiguousarray(final, np.int64)
        lens = np.array([len(p) for p in pieces], np.uint64)
        src, soff = _guarded(lens, 0xEE)
        for p, o in zip(pieces, soff):
            src[int(o):int(o) + len(p)] = np.frombuffer(bytes(p), np.uint8)
        caps = np.maximum(counts, 0) if op == LC.READ else np.zeros(n, np.int64)
        dst, doff = _guarded(caps, 0xCD)
        out, consumed, need = (np.full(n, -999, np.int64) for _ in range(3))
        flags = L.LREAD_INTERACTIVE if interactive else 0
        p = lambda a: a.ctypes.data  # noqa: E731
        if self.form == "host":
            rc = lib.k4lz4_legacy_read_fed_batch(self.dc.ctx.handle, C.byref(self.record), _dp(self.store), p(self.store_off), p(src), p(soff),
                                                 p(lens), p(final), p(dst), p(doff), p(counts), p(out), p(consumed), p(need), n, op, flags)
            self.dc.ctx.check(rc)
        else:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else a).to(dev)  # noqa: E731
            src_d, dst_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
            o_d, c_d, n_d = (torch.full((n,), -999, dtype=torch.int64, device=dev) for _ in range(3))
            mc = (self.max_count or int(counts.max())) if self.direct and op == LC.READ else 0
            so_d, sl_d, f_d, do_d, cnt_d = t(soff), t(lens), t(final), t(doff), t(counts)
            rc = lib.k4lz4_legacy_read_fed_batch_device(self.dc.ctx.handle, C.byref(self.record), _dp(self.store), _dp(self.store_off_d),
                                                        _dp(src_d), _dp(so_d), _dp(sl_d), _dp(f_d), _dp(dst_d), _dp(do_d),
                                                        _dp(cnt_d), _dp(o_d), _dp(c_d), _dp(n_d), n, op, flags, mc,
                                                        C.c_void_p(self.dc._stream()))
            self.dc.ctx.check(rc)
            torch.cuda.synchronize()
            dst, out, consumed, need = dst_d.cpu().numpy(), o_d.cpu().numpy(), c_d.cpu().numpy(), n_d.cpu().numpy()
            assert (src_d.cpu().numpy() == src).all(), "a piece was written to"
        _intact(dst, doff, caps, 0xCD, "a stream's slot")
        assert bool((self.store[self.guard_idx] == 0xA5).all()), "a write outside a stream's store"
        return out, [dst[int(doff[i]):int(doff[i]) + max(int(out[i]), 0)].tobytes() if op == LC.READ else b"" for i in range(n)], consumed, need

    def query(self):
        q = np.zeros(self.n * L.LSQ_WORDS, np.int64)
        self.dc.ctx.check(self.lib.k4lz4_legacy_reader_query(self.dc.ctx.handle, _dp(self.store), self.store_off.ctypes.data, self.n,
                                                             q.ctypes.data))
        return q.reshape(self.n, L.LSQ_WORDS)


FORMS = ["host", "device"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("interactive", [False, True], ids=["read", "interactive"])
def test_every_single_cut_in_100_byte_reads(dc, w, form, interactive):
    src, content = LC.small_stream(w, 300)
    ks = list(range(len(src) + 1))
    sources = [src] * len(ks)
    rd = GpuFedReaders(dc, len(ks), 300, form)
    drv = LC.driver(rd, sources, [[k, len(src)] for k in ks])
    reads = sum(-(-c[3] // 100) for c in LC.layout(src)) + 3
    wit = LC.check_reads(drv, w, sources, [[100] * len(ks)] * reads, interactive, 300)
    q = rd.query()
    LC.check_query(q, wit)
    assert all(x.pos == len(src) for x in wit) and (q[:, L.LSQ_BYTES_READ] == len(content)).all()
    at_k = {u for i, u, _ in drv.starved if u == ks[i]}
    assert at_k >= set(range(1, len(src)))


def _chunk_len(s):
    try:
        return max([c[2] for c in LC.layout(s)] + [16])
    except (AssertionError, IndexError):
        return 64


@pytest.mark.parametrize("form", FORMS)
def test_valid_streams_in_random_pieces_against_whole_source_readers(dc, w, form):
    """100-byte reads all the way, then random counts; after every completed logical read Query() words 0-4 equal those of
    LZ4StreamReaderBatch readers over the whole sources that made the same reads"""
    rng = np.random.default_rng(41)
    srcs = valid_streams(w)
    n = len(srcs)
    rd = GpuFedReaders(dc, n, 65536, form)
    drv = LC.driver(rd, srcs, [LC.random_ends(rng, len(s), _chunk_len(s)) for s in srcs])
    whole = L.LZ4StreamReaderBatch(srcs, 65536)
    wit = [LC.TrackedReader(w, s, False, 65536) for s in srcs]
    plan = [[100] * n] * 12 + [[None if rng.random() < 0.07 else int(rng.choice([0, 1, 17, 1000, 4096, 30000, int(rng.integers(1, 30000))]))
                                for _ in range(n)] for _ in range(12)] + [[1 << 20] * n] * 2
    for counts in plan:
        got = drv.read(np.array([-1 if c is None else c for c in counts], np.int64), False)
        ref = whole.Read(counts)
        for i, c in enumerate(counts):
            if c is not None:
                assert got[i] == wit[i].call(c) == ref[i], (i, c)
        LC.check_query(rd.query(), wit, whole.Query())
    LC.check_code_timing(drv, wit)
    assert len(drv.starved) > n and rd.query()[:, L.LSQ_BATCHED].sum() > 0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("interactive", [False, True], ids=["read", "interactive"])
def test_mutants_and_truncations_cut_at_random_places(dc, w, form, interactive):
    rng = np.random.default_rng(42)
    srcs = damaged_streams(w)
    base = w.encode_stream(corpus.class_bytes("dickens", 20000, 6).tobytes(), False, 4096)
    for _ in range(16):
        m = bytearray(base)
        m[int(rng.integers(4, len(m)))] ^= 1 << int(rng.integers(0, 8))
        srcs.append(bytes(m))
    srcs += [base[:int(k)] for k in rng.integers(1, len(base), 8)]
    rd = GpuFedReaders(dc, len(srcs), 4096, form)
    drv = LC.driver(rd, srcs, [LC.random_ends(rng, len(s), 1500) for s in srcs], with_layout=False)
    plan = [[100] * len(srcs)] * 6 + [[int(rng.choice([0, 7, 4095, 4096, 4097, 9000])) for _ in srcs] for _ in range(6)] + [[1 << 20] * len(srcs)] * 2
    wit = LC.check_reads(drv, w, srcs, plan, interactive, 4096)
    LC.check_query(rd.query(), wit)
    LC.check_code_timing(drv, wit)
    ran_out = [i for i, x in enumerate(wit) if x.failed == -1 and x.short_last]
    assert ran_out and all(drv.code_final[i] for i in ran_out) and sum(x.failed is not None for x in wit) > len(wit) // 3


@pytest.mark.parametrize("form", FORMS)
def test_refused_chunk_spanning_several_pieces(dc, w, form):
    text = corpus.class_bytes("xml", 9000, 3).tobytes()
    good = w.encode_stream(text[:1000], False, 1000)
    big = w.encode_stream(text, False, 16384)
    src = good + big
    p0 = len(good) + LC.layout(big)[0][1]
    cuts = [len(good) // 2, p0 - 1, p0 + 10, p0 + 300, len(src) - 1]
    srcs = [src, src, src[:len(src) - 5]]
    ends = [cuts + [len(src)], cuts + [len(src), len(src)], cuts[:-1] + [len(src) - 5]]
    rd = GpuFedReaders(dc, 3, 1000, form)
    drv = LC.driver(rd, srcs, ends, with_layout=False)
    wit = LC.check_reads(drv, w, srcs, [[600] * 3, [5000] * 3, [10] * 3], False, 1000)
    assert [x.failed for x in wit] == [-8, -8, -1]
    assert drv.code_at[:2] == [len(src), len(src)] and drv.code_final == [True, False, True]
    assert (0, p0 + 300, len(src) - p0 - 300) in drv.starved


def _pin(dc, w, form, Bsz, k, high=False, distinct=8, n=64):
    pairs = LC.full_chunk_streams(w, distinct, k, Bsz, seed=11, high=high)
    srcs = [pairs[i % distinct][0] for i in range(n)]
    ends = [LC.ends_inside_chunks(s, 1.5) for s in srcs]
    rd = GpuFedReaders(dc, n, Bsz, form, max_count=k * Bsz + 100)
    drv = LC.driver(rd, srcs, ends)
    got = drv.read(np.full(n, k * Bsz + 100, np.int64), False)
    wit = [LC.TrackedReader(w, pairs[i][0], False, Bsz) for i in range(distinct)]
    want = [x.call(k * Bsz + 100) for x in wit]
    for i in range(n):
        assert got[i] == want[i % distinct] == pairs[i % distinct][1], i
    q = rd.query()
    assert (q[:, L.LSQ_POSITION] == [len(s) for s in srcs]).all() and (q[:, L.LSQ_CHUNKS] == k).all()
    assert (q[:, L.LSQ_BATCHED] == q[:, L.LSQ_CHUNKS]).all() and (q[:, L.LSQ_HANDED_BACK] == 0).all(), q[:4]
    assert drv.read(np.full(n, 10, np.int64), False) == [b""] * n


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("Bsz,k", [(4096, 9), (65536, 6), (1 << 20, 3)], ids=["4K", "64K", "1M"])
def test_direct_path_pin(dc, w, form, Bsz, k):
    """64 streams of k full chunks fed in pieces of about 1.5 chunks that each end inside a chunk, one large count: every chunk goes
    through the batch decoder (the cut ones as row 0 from the stash), none through the general reader"""
    _pin(dc, w, form, Bsz, k)


def test_high_compression_streams(dc, w):
    _pin(dc, w, "device", 65536, 4, high=True, distinct=4, n=16)


def test_payload_flip_in_a_planned_chunk(dc, w):
    (good, content), = LC.full_chunk_streams(w, 1, 6, 4096, seed=9)
    lay = LC.layout(good)
    bad = bytearray(good)
    bad[lay[2][1]:lay[2][1] + 3] = b"\xff\xff\xff"
    srcs = [good, bytes(bad), good, bytes(bad)]
    cut = lay[4][1] + 5
    rd = GpuFedReaders(dc, 4, 4096, "device")
    drv = LC.driver(rd, srcs, [[cut, len(s)] for s in srcs], with_layout=False)
    wit = LC.check_reads(drv, w, srcs, [[5 * 4096] * 4, [4096] * 4], False, 4096)
    assert [x.failed for x in wit] == [None, -4, None, -4] and drv.code_at[1] == cut
    q = rd.query()
    assert list(q[:, L.LSQ_HANDED_BACK]) == [0, 1, 0, 1] and q[0, L.LSQ_BATCHED] == 6 and q[1, L.LSQ_BATCHED] == 0


def test_writer_output_fed_as_it_is_produced(dc, w):
    """LegacyWriterDevice's per-call output is the reader's piece, where the writer left it in device memory: lengths and offsets are
    the writer's device tensors, nothing of the data passes through the host.  One read of the whole content starves call after call."""
    n, Bsz = 16, 4096
    rng = np.random.default_rng(43)
    text = corpus.class_bytes("xml", 400000, 5).tobytes()
    contents = [bytearray() for _ in range(n)]
    wd = L.LegacyWriterDevice(dc, n, False, Bsz)
    rd = L.LegacyFedReaderDevice(dc, n, Bsz)
    total = 60000
    out_buf = torch.full((n * total + 64,), 0xCD, dtype=torch.uint8, device=dc.device)
    delivered = np.zeros(n, np.int64)
    steps = 6
    for k in range(steps):
        sizes = [int(rng.integers(1, 9000)) for _ in range(n)]
        pieces = [text[a:a + s] for a, s in zip(rng.integers(0, 300000, n), sizes)]
        for c, p in zip(contents, pieces):
            c += p
        lens = np.array(sizes, np.int64)
        off = np.concatenate(([0], np.cumsum(lens[:-1])))
        data = torch.from_numpy(np.frombuffer(b"".join(pieces), np.uint8).copy()).to(dc.device)
        last = k == steps - 1
        buf, w_off, w_len = (wd.close if last else wd.write)(data, off, lens)
        fin = np.full(n, int(last), np.int64)
        counts = total - delivered
        _, _, o_len, consumed, need = rd.read(buf, w_off, w_len, fin, counts, out=(out_buf, np.arange(n) * total + delivered),
                                              max_count=total)
        o, c, nd, wl = o_len.cpu().numpy(), consumed.cpu().numpy(), need.cpu().numpy(), w_len.cpu().numpy()
        assert (o >= 0).all() and (c == wl).all() and ((nd > 0) == (not last)).all(), (k, o, c, nd)
        delivered += o
    got = out_buf.cpu().numpy()
    for i in range(n):
        assert delivered[i] == len(contents[i]) and got[i * total:i * total + delivered[i]].tobytes() == bytes(contents[i]), i
    q = rd.query().cpu().numpy()
    assert (q[:, L.LSQ_CODE] == 0).all() and (q[:, L.LSQ_BYTES_READ] == delivered).all() and q[:, L.LSQ_BATCHED].sum() > 0


def test_feed_and_read_of_the_host_class(dc, w):
    srcs = valid_streams(w)[:6]
    fr = L.LZ4StreamFedReaderBatch(len(srcs), 65536)
    wit = [LC.TrackedReader(w, s, False, 65536) for s in srcs]
    at = [0] * len(srcs)
    got = [bytearray() for _ in srcs]
    want = [x.call(1 << 20) for x in wit]
    remaining = [1 << 20] * len(srcs)
    for _ in range(200):
        step = [min(777, len(s) - a) for s, a in zip(srcs, at)]
        fr.Feed([s[a:a + k] for s, a, k in zip(srcs, at, step)], [a + k == len(s) for s, a, k in zip(srcs, at, step)])
        at = [a + k for a, k in zip(at, step)]
        out, consumed, need = fr.Read([r if r > 0 else None for r in remaining])
        for i, o in enumerate(out):
            if o is not None:
                got[i] += o
                remaining[i] = remaining[i] - len(o) if need[i] > 0 else 0
        if not any(r > 0 for r in remaining):
            break
    assert [bytes(g) for g in got] == want
    assert (fr.Query()[:, L.LSQ_POSITION] == [len(s) for s in srcs]).all()


def test_each_family_refuses_the_other_record(dc):
    lib, n = dc.lib, 1
    plain, fed = L.legacy_reader_record(4096, lib), L.legacy_reader_record(4096, lib, fed=True)
    store = torch.zeros(int(fed.storeBytes) + 64, dtype=torch.uint8, device=dc.device)
    z = np.zeros(n, np.uint64)
    cnt, out, cons, need = (np.zeros(n, np.int64) for _ in range(4))
    p = lambda a: a.ctypes.data  # noqa: E731
    assert lib.k4lz4_legacy_read_batch(dc.ctx.handle, C.byref(fed), _dp(store), p(z), p(z), p(z), p(z), p(z), p(z), p(cnt), p(out), n,
                                       L.LREAD_RESET, 0) == -2
    assert lib.k4lz4_legacy_read_fed_batch(dc.ctx.handle, C.byref(plain), _dp(store), p(z), p(z), p(z), p(z), None, p(z), p(z), p(cnt), p(out),
                                           p(cons), p(need), n, L.LREAD_RESET, 0) == -2
    d = lambda: torch.zeros(n, dtype=torch.int64, device=dc.device)  # noqa: E731
    a = [d() for _ in range(8)]
    assert lib.k4lz4_legacy_read_batch_device(dc.ctx.handle, C.byref(fed), _dp(store), _dp(a[0]), _dp(store), _dp(a[1]), _dp(a[2]), _dp(store),
                                              _dp(a[3]), _dp(a[4]), _dp(a[5]), n, L.LREAD_RESET, 0, 0, None) == -2
    assert lib.k4lz4_legacy_read_fed_batch_device(dc.ctx.handle, C.byref(plain), _dp(store), _dp(a[0]), _dp(store), _dp(a[1]), _dp(a[2]), None,
                                                  _dp(store), _dp(a[3]), _dp(a[4]), _dp(a[5]), _dp(a[6]), _dp(a[7]), n, L.LREAD_RESET, 0, 0,
                                                  None) == -2
    assert lib.k4lz4_legacy_read_fed_batch(dc.ctx.handle, C.byref(fed), _dp(store), p(z), p(z), p(z), p(z), None, p(z), p(z), p(cnt), p(out),
                                           p(cons), p(need), n, L.LREAD_RESET, 0) == 0
