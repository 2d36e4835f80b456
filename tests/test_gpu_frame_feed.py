"""The fed frame reader on the GPU (k4lz4_frame_read_fed_batch / _device, LZ4FrameFedReaderBatch / FrameFedReaderDevice; DESIGN.md
4.15), host and device form: logical reads (frame_feed_cases.FedDriver) against the witness over the WHOLE source, with guard bytes
around every output slot, every store and every piece, and every raw call held to the contract (consumed, need, final)."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

import frame_feed_cases as FC
import frame_reader_cases as K
from test_frame_layer import LZ4F
from k4os.compression.lz4_amd import LZ4EncoderSettings, LZ4Level, corpus, pack_blocks
from k4os.compression.lz4_amd import FrameWriterDevice, LZ4FrameReaderBatch, LZ4FrameFedReaderBatch, FrameFedReaderDevice
from k4os.compression.lz4_amd import frames as F
from k4os.compression.lz4_amd.device import DeviceCodec

pytestmark = pytest.mark.gpu
K64 = 65536
GUARD = 64


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


class FedReaders:
    """n fed readers through the C ABI with guarded slots, stores and pieces; host=True: k4lz4_frame_read_fed_batch, else the device
    form.  call() is what frame_feed_cases.FedDriver drives."""

    def __init__(self, dc, n, max_block=4 << 20, host=False, fast=True):
        self.dc, self.host, self.n, self.fast = dc, host, n, fast
        self.rec = F.frame_reader_record(max_block, dc.lib, fed=True)
        self.sb = int(self.rec.storeBytes)
        self.step = self.sb + 256
        self.store = torch.full((n * self.step + 512,), 0xA5, dtype=torch.uint8, device=dc.device)
        self.store_off = 256 + np.arange(n, dtype=np.uint64) * np.uint64(self.step)
        self.d_store_off = torch.from_numpy(self.store_off.astype(np.int64)).to(dc.device)
        self.call(F.FREAD_RESET, [b""] * n, np.zeros(n, np.int64), np.zeros(n, np.int64), False)

    def call(self, op, pieces, final, counts, interactive):
        n, dev = self.n, self.dc.device
        counts = np.ascontiguousarray(counts, np.int64)
        final = np.ascontiguousarray(final, np.int64)
        lens = np.array([len(p) for p in pieces], np.uint64)
        soff = np.full(n, GUARD, np.uint64)
        soff[1:] += np.cumsum(lens[:-1] + np.uint64(GUARD))
        src = np.full(int(lens.sum()) + GUARD * (n + 1), 0xEE, np.uint8)
        for i, p in enumerate(pieces):
            src[int(soff[i]):int(soff[i]) + len(p)] = np.frombuffer(bytes(p), np.uint8)
        caps = np.maximum(counts, 0).astype(np.uint64) if op == F.FREAD_READ else np.zeros(n, np.uint64)
        doff = np.full(n, GUARD, np.uint64)
        doff[1:] += np.cumsum(caps[:-1] + np.uint64(GUARD))
        total = int(caps.sum()) + GUARD * (n + 1)
        flags = F.FREAD_INTERACTIVE if interactive else 0
        lib, ctx = self.dc.lib, self.dc.ctx
        if self.host:
            dst = np.full(total, 0xCD, np.uint8)
            out, consumed, need = (np.full(n, -999, np.int64) for _ in range(3))
            ctx.check(lib.k4lz4_frame_read_fed_batch(
                ctx.handle, C.byref(self.rec), self.store.data_ptr(), self.store_off.ctypes.data, src.ctypes.data, soff.ctypes.data,
                lens.ctypes.data, final.ctypes.data, dst.ctypes.data, doff.ctypes.data, counts.ctypes.data, out.ctypes.data,
                consumed.ctypes.data, need.ctypes.data, n, op, flags))
        else:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else a).to(dev)  # noqa: E731
            d_src, d_soff, d_len, d_fin, d_cnt, d_doff = up(src.view(np.uint8)), up(soff), up(lens), up(final), up(counts), up(doff)
            d_dst = torch.full((total,), 0xCD, dtype=torch.uint8, device=dev)
            d_out, d_cons, d_need = (torch.full((n,), -999, dtype=torch.int64, device=dev) for _ in range(3))
            ctx.check(lib.k4lz4_frame_read_fed_batch_device(
                ctx.handle, C.byref(self.rec), self.store.data_ptr(), self.d_store_off.data_ptr(), d_src.data_ptr(), d_soff.data_ptr(),
                d_len.data_ptr(), d_fin.data_ptr(), d_dst.data_ptr(), d_doff.data_ptr(), d_cnt.data_ptr(), d_out.data_ptr(),
                d_cons.data_ptr(), d_need.data_ptr(), n, op, flags, int(max(counts.max(), 0)) if self.fast else 0,
                C.c_void_p(self.dc._stream())))
            dst, out, consumed, need = d_dst.cpu().numpy(), d_out.cpu().numpy(), d_cons.cpu().numpy(), d_need.cpu().numpy()
        if op == F.FREAD_READ:
            mask = np.ones(dst.size, bool)
            for i in range(n):
                mask[int(doff[i]):int(doff[i] + caps[i])] = False
            assert (dst[mask] == 0xCD).all(), "a write outside a stream's slot"
        return out, [dst[int(doff[i]):int(doff[i]) + max(int(out[i]), 0)].tobytes() if op == F.FREAD_READ else b"" for i in range(n)], consumed, need

    def query(self):
        q = np.zeros(self.n * F.FRQ_WORDS, np.int64)
        self.dc.ctx.check(self.dc.lib.k4lz4_frame_reader_query(self.dc.ctx.handle, self.store.data_ptr(), self.store_off.ctypes.data, self.n,
                                                               q.ctypes.data))
        return q.reshape(self.n, F.FRQ_WORDS)

    def check_store_guards(self):
        s = self.store
        body = s[256:256 + self.n * self.step].view(self.n, self.step)
        assert bool((s[:256] == 0xA5).all()) and bool((body[:, self.sb:] == 0xA5).all()) and bool((s[256 + self.n * self.step:] == 0xA5).all()), \
            "a write outside a stream's store"


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("count,near", [(1 << 20, None), (100, None), (7, 40), (1, 16)], ids=["whole", "100", "7", "1"])
def test_every_single_cut(dc, host, count, near):
    """as test_frame_feed_emu.py::test_every_single_cut, on the device: reads of 100 bytes all the way, reads of 7 and 1 bytes within
    `near` bytes of every block end, EndMark and frame boundary (one large read through the middle of each 64 KiB block)"""
    src, content = FC.small_source()
    ks = list(range(len(src) + 1))
    sources = [src] * len(ks)
    rd = FedReaders(dc, len(ks), max_block=K64, host=host)
    drv = FC.FedDriver(rd, sources, [[k, len(src)] for k in ks], FC.field_end_fn(sources))
    plan = FC.reads_to_the_end(src, count, len(ks), near, FC.small_content_ends())
    wit = K.check_reads(drv, sources, plan, [f"k{k}" for k in ks], max_block=K64)
    q = rd.query()
    for i, w in enumerate(wit):
        assert (int(q[i, 0]), int(q[i, 2])) == (w.bytes_read, w.phase) == (len(content), 0), ks[i]
    at_k = {u for i, u, _ in drv.starved if u == ks[i]}
    assert at_k >= set(range(1, len(src)))
    rd.check_store_guards()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_random_pieces(dc, host):
    rng = np.random.default_rng(31)
    srcs = K.valid_sources(LZ4F()) + [(n, s, None) for n, s in K.quirk_sources()]
    names, sources = [s[0] for s in srcs], [s[1] for s in srcs]
    bs_of = [FC.block_size_of(n) for n in names]
    rd = FedReaders(dc, len(sources), host=host)
    drv = FC.FedDriver(rd, sources, [FC.random_ends(rng, len(s), b) for s, b in zip(sources, bs_of)])
    plan = K.read_plan(np.random.default_rng(17), len(sources), bs_of, calls=7, top=3 << 20, rest=2 << 20)
    wit = K.check_reads(FC.OpenMixer(drv, sources, rng), sources, plan, names)
    q = rd.query()
    for i, w in enumerate(wit):
        assert (int(q[i, 0]), int(q[i, 2]), int(q[i, 3])) == (w.bytes_read, w.phase, w.failed or 0), names[i]
        if srcs[i][2] is not None:
            assert w.failed is None and w.bytes_read == len(srcs[i][2]), names[i]
    FC.check_code_timing(drv, wit, names)
    assert len(drv.starved) > len(sources) and q[:, 6].sum() > 0
    rd.check_store_guards()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_defects_come_when_their_bytes_do(dc, host):
    rng = np.random.default_rng(33)
    c = corpus.class_bytes("xml", 200_000, 2).tobytes()
    bases = [K.indep_frame(c, K64, True, True, True), LZ4F().compress(np.frombuffer(c, np.uint8), 4, True, True, True, False),
             K.indep_frame(c[:70_000], K64, False, False, False, cut=30_000, raw_every=2),
             LZ4F().compress(np.frombuffer(c, np.uint8), 4, True, True, False, False)]
    names, sources, loose = [], [], []
    for b, base in enumerate(bases):
        info = F.parse_frame(base)
        for n, m in K.structural_mutants(base):
            names.append(f"{b}:{n}"); sources.append(m); loose.append(None)
        for n, m, k in K.payload_mutants(base, rng, 16):
            names.append(f"{b}:{n}"); sources.append(m)
            loose.append(None if info.descriptor.BlockChecksum else k * (30_000 if b == 2 else K64))
    rd = FedReaders(dc, len(sources), max_block=K64, host=host)
    drv = FC.FedDriver(rd, sources, [FC.random_ends(rng, len(s), K64) for s in sources])
    plan = [(np.array([int(rng.choice([0, 7, K64 - 1, K64, K64 + 1, 100_000])) for _ in sources], np.int64), k == 1) for k in range(4)]
    plan += [(np.full(len(sources), 1 << 20, np.int64), False)] * 3
    wit = K.check_reads(drv, sources, plan, names, max_block=K64, loose_from=loose)
    assert {w.failed for w in wit} >= {-1, -2, -3, -4, -5, -6, -7, -8, None}
    FC.check_code_timing(drv, wit, names)
    cuts = [i for i, n in enumerate(names) if ":cut@" in n and wit[i].failed == -1]
    assert cuts and all(drv.code_final[i] for i in cuts)
    rd.check_store_guards()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_both_ways_in_one_call(dc, host):
    """streams of full 64 KiB independent blocks fed in pieces of 8 records plus 1000 bytes are served by the fast path in every call
    and never handed back; a stream with a short block inside a piece is handed back; chained and irregular streams are the general
    reader's; all deliver the witness's bytes"""
    c = corpus.class_bytes("dickens", 32 * K64, 6).tobytes()
    regular = K.indep_frame(c, K64, True, True)
    plain = K.indep_frame(c, K64, False, False)
    short_in = K.frame_of([K.compress(c[:K64]), K.compress(c[K64:K64 + 5000])] + [K.compress(c[k * K64:(k + 1) * K64]) for k in range(2, 12)],
                          [False] * 12, c[:K64 + 5000] + c[2 * K64:12 * K64], K64, False, True, True)
    chained = LZ4F().compress(np.frombuffer(c[:10 * K64], np.uint8), 4, True, True, False, False)
    irregular = K.indep_frame(c[:300_000], K64, True, True, cut=10_000)
    kinds = [("regular", regular), ("plain", plain), ("short-inside", short_in), ("chained", chained), ("irregular", irregular)]
    names, sources = [k for k, _ in kinds] * 4, [s for _, s in kinds] * 4

    def ends_of(s):
        info = F.parse_frame(s)
        rec = [o - 4 for o in info.block_off] + [len(s)]
        e = [rec[k] + 1000 for k in range(8, len(rec) - 1, 8)]
        return [x for x in e if x < len(s)] + [len(s)]
    rd = FedReaders(dc, len(sources), max_block=K64, host=host)
    drv = FC.FedDriver(rd, sources, [ends_of(s) for s in sources], FC.field_end_fn(sources))
    wit = K.check_reads(drv, sources, [(np.full(len(sources), 8 * K64, np.int64), False)] * 6, names, max_block=K64)
    q = rd.query()
    for i, n in enumerate(names):
        assert int(q[i, 0]) == wit[i].bytes_read > 0, n
        if n in ("regular", "plain"):
            assert q[i, 6] > 0 and q[i, 7] == 0, (n, q[i])
        if n == "short-inside":
            assert q[i, 7] >= 1, (n, q[i])
        if n == "chained":
            assert q[i, 6] == 0 and q[i, 7] == 0, (n, q[i])
    rd.check_store_guards()


def test_writer_output_fed_as_it_is_produced(dc):
    """FrameWriterDevice's per-call output goes, call by call, into a fed FrameReaderDevice: no host copy in between; the reader
    returns the written bytes"""
    rng = np.random.default_rng(8)
    settings = [LZ4EncoderSettings(ContentChecksum=True), LZ4EncoderSettings(BlockSize=256 << 10, BlockChecksum=True),
                LZ4EncoderSettings(ChainBlocks=True, ContentChecksum=True), LZ4EncoderSettings(ChainBlocks=True, CompressionLevel=LZ4Level.L03_HC)] * 4
    n = len(settings)
    contents = [corpus.class_bytes(("dickens", "xml", "mozilla", "x-ray")[i % 4], 900_000 + 1000 * i, i) for i in range(n)]
    data_h, off, _ = pack_blocks(contents)
    data = torch.from_numpy(data_h).to(dc.device)
    w = FrameWriterDevice(dc, n, settings)
    rd = FrameFedReaderDevice(dc, n)
    at = np.zeros(n, np.int64)
    kept = []
    counts = torch.full((n,), 1 << 20, dtype=torch.int64, device=dc.device)
    for call in range(7):
        last = call == 6
        ln = np.array([contents[i].size - int(at[i]) if last else min(int(rng.choice([0, 1, 70_000, 200_000, 333_333])), contents[i].size - int(at[i]))
                       for i in range(n)], np.int64)
        out, o_off, o_len = (w.close if last else w.write)(data, off.astype(np.int64) + at, ln)
        fin = torch.full((n,), int(last), dtype=torch.int64, device=dc.device)
        # every read asks for more than the frame holds, so it consumes its whole piece and starves until the frame's end arrives
        kept.append((o_len,) + rd.read(out, F._dev_i64(o_off, dc.device), o_len, fin, counts, max_count=1 << 20))
        at += ln
    got = [b""] * n
    for k, (o_len, buf, r_off, r_len, consumed, need) in enumerate(kept):
        h, ln, cons, nd, fed = buf.cpu().numpy(), r_len.cpu().numpy(), consumed.cpu().numpy(), need.cpu().numpy(), o_len.cpu().numpy()
        assert (ln >= 0).all() and (cons == fed).all(), k
        assert ((nd > 0) == (k < 6)).all(), (k, nd)
        got = [g + h[int(r_off[i]):int(r_off[i]) + int(ln[i])].tobytes() for i, g in enumerate(got)]
    for i in range(n):
        assert got[i] == contents[i].tobytes(), i
    q = rd.query().cpu().numpy()
    assert q[:, 0].tolist() == [c.size for c in contents] and (q[:, 2] == 0).all()


def test_fed_and_whole_source_readers_agree(dc):
    rng = np.random.default_rng(41)
    srcs = K.valid_sources(LZ4F(), big=False)
    names, sources = [s[0] for s in srcs], [s[1] for s in srcs]
    bs_of = [FC.block_size_of(n) for n in names]
    whole = LZ4FrameReaderBatch(sources, raise_errors=False)
    fed = FedReaders(dc, len(sources), host=True)
    drv = FC.FedDriver(fed, sources, [FC.random_ends(rng, len(s), b) for s, b in zip(sources, bs_of)])
    for counts, interactive in K.read_plan(np.random.default_rng(5), len(sources), bs_of, calls=6, top=400_000):
        a = whole.Read([None if c < 0 else int(c) for c in counts], interactive)
        b = drv.read(counts, interactive)
        assert a == b, (counts.tolist(), interactive)
        assert (whole.Query()[:, :5] == fed.query()[:, :5]).all()


def test_records_are_not_interchangeable_and_the_mirror_reads(dc):
    lib, ctx = dc.lib, dc.ctx
    plain, fedrec = F.frame_reader_record(K64, lib), F.frame_reader_record(K64, lib, fed=True)
    assert fedrec.storeBytes == plain.storeBytes + 65792 == lib.k4lz4_frame_reader_store_bytes(C.byref(fedrec))
    store = torch.zeros(int(fedrec.storeBytes) + 64, dtype=torch.uint8, device=dc.device)
    z, o = np.zeros(1, np.uint64), np.zeros(1, np.int64)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert lib.k4lz4_frame_read_batch(ctx.handle, C.byref(fedrec), store.data_ptr(), p(z), None, p(z), p(z), None, p(z), p(o), p(o), 1,
                                      F.FREAD_RESET, 0) == lib.k4lz4_frame_read_fed_batch(
        ctx.handle, C.byref(plain), store.data_ptr(), p(z), None, p(z), p(z), None, None, p(z), p(o), p(o), p(o.copy()), p(o.copy()), 1,
        F.FREAD_RESET, 0) != 0
    c = corpus.class_bytes("dickens", 300_000, 1).tobytes()
    good = K.indep_frame(c, K64, True, True, True)
    info = F.parse_frame(good)
    cut = info.block_off[1] + 10                                   # inside the second record's payload
    rest = info.block_off[2] - 4 - cut                             # ... which ends in front of the third length word
    r = LZ4FrameFedReaderBatch(2)
    r.Feed([good[:5], good[:cut]])
    assert r.Open() == [False, True] and r.Need.tolist() == [1, 0]
    assert r.Read([100_000, 100_000]) == [b"", c[:K64]] and r.Need.tolist() == [1, rest] and [len(q) for q in r.queue] == [0, 0]
    r.Feed([good[5:], good[cut:]], final=[True, True])
    assert r.ReadAll([100_000, 100_000 - K64]) == [c[:100_000], c[K64:100_000]] and r.BytesRead == [100_000, 100_000]
    assert r.ReadAll([1 << 20, 1 << 20]) == [c[100_000:], c[100_000:]] and r.ReadAll([5, 5]) == [b"", b""]
    bad = bytearray(good); bad[40] ^= 1
    r = LZ4FrameFedReaderBatch(1)
    r.Feed([bytes(bad)], final=[True])
    with pytest.raises(F.InvalidDataException, match="block checksum"):
        r.Read([10])
