"""The incremental frame reader on the GPU (k4lz4_frame_read_batch / _device, LZ4FrameReaderBatch / FrameReaderDevice; DESIGN.md
4.14): every call's lengths, codes and bytes against the witness (frame_reader_witness.py), in the host form and in the device
form, with guard bytes around every output slot and every store.  Hostile inputs are there to be refused."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

import frame_reader_cases as K
from frame_reader_witness import WitnessReader
from test_frame_layer import LZ4F
from k4os.compression.lz4_amd import LZ4Frame, LZ4EncoderSettings, LZ4Level, corpus, pack_blocks, encode_fast_chain_frames
from k4os.compression.lz4_amd import LZ4FrameWriterBatch, LZ4FrameReaderBatch, FrameWriterDevice, FrameReaderDevice
from k4os.compression.lz4_amd import frames as F
from k4os.compression.lz4_amd.device import DeviceCodec

pytestmark = pytest.mark.gpu
K64 = 65536
GUARD = 64


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


class Readers:
    """n readers through the C ABI with guarded slots and stores; host=True: k4lz4_frame_read_batch, else the device form"""

    def __init__(self, dc, sources, max_block=4 << 20, host=False, fast=True):
        self.dc, self.host, self.n, self.fast = dc, host, len(sources), fast
        self.rec = F.frame_reader_record(max_block, dc.lib)
        self.sb = int(self.rec.storeBytes)
        self.step = self.sb + 256
        self.store = torch.full((self.n * self.step + 512,), 0xA5, dtype=torch.uint8, device=dc.device)
        self.store_off = 256 + np.arange(self.n, dtype=np.uint64) * np.uint64(self.step)
        views = [np.frombuffer(bytes(s), np.uint8) for s in sources]
        self.src, off, _ = pack_blocks(views)
        self.src_off, self.src_len = np.ascontiguousarray(off, np.uint64), np.array([v.size for v in views], np.uint64)
        if not host:
            self.d_src = torch.from_numpy(self.src).to(dc.device)
            self.d = [torch.from_numpy(a.astype(np.int64)).to(dc.device) for a in (self.store_off, self.src_off, self.src_len)]
        else:
            # the host form works on the context's own stream, which does not wait for torch's: the 0xA5 fill of the stores has to
            # be over before RESET writes them, or it overwrites the streams it reaches late
            torch.cuda.synchronize()
        self.call(F.FREAD_RESET, np.zeros(self.n, np.int64), False)

    def call(self, op, counts, interactive):
        counts = np.ascontiguousarray(counts, np.int64)
        caps = np.maximum(counts, 0).astype(np.uint64)
        doff = np.full(self.n, GUARD, np.uint64)
        doff[1:] += np.cumsum(caps[:-1] + np.uint64(GUARD))
        total = int(caps.sum()) + GUARD * (self.n + 1)
        flags = F.FREAD_INTERACTIVE if interactive else 0
        lib, ctx = self.dc.lib, self.dc.ctx
        if self.host:
            dst = np.full(total, 0xCD, np.uint8)
            out = np.full(self.n, -999, np.int64)
            ctx.check(lib.k4lz4_frame_read_batch(ctx.handle, C.byref(self.rec), self.store.data_ptr(), self.store_off.ctypes.data,
                                                 self.src.ctypes.data, self.src_off.ctypes.data, self.src_len.ctypes.data, dst.ctypes.data,
                                                 doff.ctypes.data, counts.ctypes.data, out.ctypes.data, self.n, op, flags))
        else:
            d_dst = torch.full((total,), 0xCD, dtype=torch.uint8, device=self.dc.device)
            d_out = torch.full((self.n,), -999, dtype=torch.int64, device=self.dc.device)
            d_cnt, d_doff = torch.from_numpy(counts).to(self.dc.device), torch.from_numpy(doff.astype(np.int64)).to(self.dc.device)
            ctx.check(lib.k4lz4_frame_read_batch_device(ctx.handle, C.byref(self.rec), self.store.data_ptr(), self.d[0].data_ptr(),
                                                        self.d_src.data_ptr(), self.d[1].data_ptr(), self.d[2].data_ptr(), d_dst.data_ptr(),
                                                        d_doff.data_ptr(), d_cnt.data_ptr(), d_out.data_ptr(), self.n, op, flags,
                                                        int(max(counts.max(), 0)) if self.fast else 0,
                                                        C.c_void_p(self.dc._stream())))
            dst, out = d_dst.cpu().numpy(), d_out.cpu().numpy()
        if op == F.FREAD_READ:
            for i in range(self.n):                         # the guard in front of every slot, and the one behind the last
                assert (dst[int(doff[i]) - GUARD:int(doff[i])] == 0xCD).all(), ("a write outside a stream's slot", i)
            assert (dst[int(doff[-1] + caps[-1]):] == 0xCD).all(), "a write behind the last slot"
        return out, [dst[int(doff[i]):int(doff[i]) + max(int(out[i]), 0)].tobytes() if op == F.FREAD_READ else b"" for i in range(self.n)]

    def read(self, counts, interactive=False):
        out, data = self.call(F.FREAD_READ, counts, interactive)
        return [None if counts[i] < 0 else (int(out[i]) if out[i] < 0 else data[i]) for i in range(self.n)]

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


def gpu_made_sources():
    """frames this library writes: LZ4Frame.EncodeBatch (independent and chained, L00 / L03_HC / L09_HC), encode_fast_chain_frames,
    LZ4FrameWriterBatch with a BlockSize below 64 KiB and short writes"""
    contents = [corpus.class_bytes(c, n, k) for k, (c, n) in enumerate((("dickens", 300_000), ("xml", 65_536), ("x-ray", 200_001), ("mozilla", 1_100_000)))]
    out = []
    for lvl in (LZ4Level.L00_FAST, LZ4Level.L03_HC, LZ4Level.L09_HC):
        for chain in (False, True):
            if chain and lvl == LZ4Level.L00_FAST:
                continue
            for bs, bsum, csum, clen in ((K64, True, True, False), (256 << 10, False, True, True), (1 << 20, False, False, False)):
                s = LZ4EncoderSettings(BlockSize=bs, BlockChecksum=bsum, ContentChecksum=csum, ContentLength=None,
                                       ChainBlocks=chain, CompressionLevel=lvl)
                for f, c in zip(LZ4Frame.EncodeBatch(contents, s), contents):
                    out.append((f"batch-L{int(lvl)}-{int(chain)}-{bs}", f, c.tobytes(), bs))
    for bs, bsum in ((K64, True), (4 << 20, False)):
        s = LZ4EncoderSettings(ChainBlocks=True, BlockSize=bs, BlockChecksum=bsum, ContentChecksum=True)
        for f, c in zip(encode_fast_chain_frames(contents, s), contents):
            out.append((f"fastchain-{bs}", f, c.tobytes(), bs))
    rng = np.random.default_rng(4)
    settings = [LZ4EncoderSettings(BlockSize=10_000, ContentChecksum=True), LZ4EncoderSettings(BlockSize=40_000, BlockChecksum=True),
                LZ4EncoderSettings(BlockSize=K64, ChainBlocks=True, ContentChecksum=True),
                LZ4EncoderSettings(BlockSize=30_000, ChainBlocks=True, CompressionLevel=LZ4Level.L03_HC, BlockChecksum=True)]
    w = LZ4FrameWriterBatch(len(settings), settings)
    frames, at = [b""] * len(settings), [0] * len(settings)
    for _ in range(9):
        chunks = []
        for i in range(len(settings)):
            n = int(rng.choice([0, 1, 500, 9_999, 25_000, 70_000]))
            chunks.append(contents[i].tobytes()[at[i]:at[i] + n]); at[i] += len(chunks[-1])
        frames = [f + b for f, b in zip(frames, w.Write(chunks))]
    frames = [f + b for f, b in zip(frames, w.Close())]
    for i, f in enumerate(frames):
        out.append((f"writer-{i}", f, contents[i].tobytes()[:at[i]], K64))
    return out


def bs_of_name(n):
    return K.BLOCK_SIZES[int(n.split("-b")[1][0])] if n.startswith(("indep-b", "linked-b", "linked-raw-b")) else K64


@pytest.fixture(scope="module")
def mixed(dc):
    made = gpu_made_sources()
    host = K.valid_sources(LZ4F())
    names = [m[0] for m in made] + [h[0] for h in host]
    sources = [m[1] for m in made] + [h[1] for h in host]
    contents = [m[2] for m in made] + [h[2] for h in host]
    bs = [m[3] for m in made] + [bs_of_name(h[0]) for h in host]
    # sources of two and three of this library's frames
    for a, b, c in ((0, 20, 40), (50, 3, 60), (70, 71, 72)):
        names.append(f"cat-{a}-{b}-{c}"); sources.append(sources[a] + sources[b] + sources[c]); contents.append(contents[a] + contents[b] + contents[c])
        bs.append(K64)
    assert len(sources) >= 96
    return names, sources, contents, bs


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_mixed_streams_in_random_reads(dc, mixed, host):
    names, sources, contents, bs = mixed
    rd = Readers(dc, sources, host=host)
    plan = K.read_plan(np.random.default_rng(17), len(sources), bs, calls=7, top=3 << 20, rest=2 << 20)
    wit = K.check_reads(rd, sources, plan, names)
    q = rd.query()
    for i, w in enumerate(wit):
        assert w.failed is None and w.bytes_read == len(contents[i]), names[i]
        assert (int(q[i, 0]), int(q[i, 2])) == (w.bytes_read, w.phase), names[i]
    # the general reader decoded blocks in place and through the buffer, the fast path served blocks and handed streams back
    assert q[:, 5].sum() > 0 and (q[:, 4] - q[:, 5] - q[:, 6]).sum() > 0 and q[:, 6].sum() > 0 and q[:, 7].sum() > 0
    rd.check_store_guards()


def test_fast_path_holds_for_some_streams_and_fails_for_others_in_one_call(dc):
    """one batch, one call: streams of full blocks are served by the fast path (K4LZ4_FRQ_FAST counts their blocks), streams with a
    short middle block, a block that decodes to blockSize + 8 or a failing block checksum are planned, fail the verification and are
    replayed by the general reader (K4LZ4_FRQ_HANDED_BACK), chained streams are never planned -- all against the witness; with
    maxCount = 0 the same calls run on the general reader alone and count no fast block"""
    c = corpus.class_bytes("dickens", 6 * K64 + 100, 6).tobytes()
    rnd = corpus.random_bytes(2 * K64, 1).tobytes()
    regular = K.indep_frame(c, K64, True, True)
    with_raw = K.frame_of([K.compress(c[:K64]), rnd[:K64], rnd[K64:], K.compress(c[K64:2 * K64])], [False, True, True, False],
                          c[:K64] + rnd + c[K64:2 * K64], K64, False, True, True)
    short_mid = K.frame_of([K.compress(c[:K64]), K.compress(c[K64:K64 + 5000]), K.compress(c[2 * K64:3 * K64])], [False] * 3,
                           c[:K64] + c[K64:K64 + 5000] + c[2 * K64:3 * K64], K64, False, True, True)
    chained = LZ4F().compress(np.frombuffer(c, np.uint8), 4, True, True, False, False)
    bad = bytearray(regular); bad[K64 + 3000] ^= 4
    over = K.frame_of([K.rle_block(K64 + 8), K.compress(c[:K64])], [False, False], bytes([0x42]) * (K64 + 8) + c[:K64], K64, False, False, True)
    big = K.indep_frame(corpus.class_bytes("xml", 3 << 20, 2).tobytes(), 1 << 20, False, True)
    kinds = [("regular", regular), ("raw", with_raw), ("short-middle", short_mid), ("chained", chained), ("bad-block-sum", bytes(bad)),
             ("over8", over), ("two", regular + regular), ("big", big)]
    names = [k for k, _ in kinds] * 6
    sources = [s for _, s in kinds] * 6
    plan = [(np.full(len(sources), n, np.int64), False) for n in (2 * K64, K64 + 1000, K64, 3 * K64, 1 << 20, 1 << 20, 1 << 20)]
    for host in (False, True):
        rd = Readers(dc, sources, max_block=1 << 20, host=host)
        first = rd.read(plan[0][0])
        q = rd.query()
        by = {k: q[i] for i, k in enumerate(names[:len(kinds)])}
        assert by["regular"][6] == 2 and by["raw"][6] == 2 and by["two"][6] == 2 and by["big"][6] == 1, q[:8, 6]
        assert by["short-middle"][7] == 1 and by["over8"][7] == 1 and by["bad-block-sum"][7] == 1 and by["chained"][7] == 0, q[:8, 7]
        assert by["short-middle"][6] == 0 and by["chained"][6] == 0 and by["short-middle"][4] > 0 and by["chained"][4] > 0
        wit = [WitnessReader(s, 1 << 20) for s in sources]
        assert first == [w.read(2 * K64) for w in wit]
        rd2 = Readers(dc, sources, max_block=1 << 20, host=host)
        K.check_reads(rd2, sources, plan, names, max_block=1 << 20)
        rd2.check_store_guards()
    slow = Readers(dc, sources, max_block=1 << 20, fast=False)
    K.check_reads(slow, sources, plan, names, max_block=1 << 20)
    assert slow.query()[:, 6].sum() == 0 and slow.query()[:, 7].sum() == 0


def test_a_store_continues_under_the_other_form(dc, mixed):
    """host form for some calls, device form for the others, on the same stores"""
    names, sources, contents, bs = mixed
    pick = list(range(0, len(sources), 3))
    sources, names, bs = [sources[i] for i in pick], [names[i] for i in pick], [bs[i] for i in pick]
    host, dev = Readers(dc, sources, host=True), Readers(dc, sources, host=False)
    dev.store = host.store                                  # one set of stores (the same layout), two forms

    class Switching:
        calls = 0

        def read(self, counts, interactive=False):
            Switching.calls += 1
            return (host if Switching.calls % 3 == 0 else dev).read(counts, interactive)
    K.check_reads(Switching(), sources, K.read_plan(np.random.default_rng(23), len(sources), bs, calls=8, top=1 << 20, rest=2 << 20), names)
    host.check_store_guards()


def test_one_read_equals_decode_frames_device(dc, mixed):
    names, sources, contents, _ = mixed
    pick = [i for i, n in enumerate(names) if not n.startswith(("cat-", "two-", "three-", "empty-first", "linked-then", "no-source"))]
    frames = [sources[i] for i in pick]
    data, off, _ = pack_blocks([np.frombuffer(f, np.uint8) for f in frames])
    d = torch.from_numpy(data).to(dc.device)
    ln = np.array([len(f) for f in frames], np.int64)
    buf, o_off, o_len = F.decode_frames_device(dc, d, off.astype(np.int64), ln)
    rd = FrameReaderDevice(dc, d, off.astype(np.int64), ln)
    out, r_off, r_len = rd.read(np.array([len(contents[i]) + 9 for i in pick], np.int64))
    h1, n1, h2, n2 = buf.cpu().numpy(), o_len.cpu().numpy(), out.cpu().numpy(), r_len.cpu().numpy()
    for k, i in enumerate(pick):
        whole = h1[int(o_off[k]):int(o_off[k]) + int(n1[k])].tobytes()
        assert n1[k] == n2[k] == len(contents[i]) and whole == h2[int(r_off[k]):int(r_off[k]) + int(n2[k])].tobytes() == contents[i], names[i]
    assert LZ4Frame.Decode(frames[0]) == WitnessReader(frames[0]).read(len(contents[pick[0]]) + 1)


def test_writer_to_reader_on_the_device(dc):
    rng = np.random.default_rng(8)
    settings = [LZ4EncoderSettings(ContentChecksum=True), LZ4EncoderSettings(BlockSize=256 << 10, BlockChecksum=True),
                LZ4EncoderSettings(ChainBlocks=True, ContentChecksum=True), LZ4EncoderSettings(ChainBlocks=True, CompressionLevel=LZ4Level.L03_HC)] * 4
    n = len(settings)
    contents = [corpus.class_bytes(("dickens", "xml", "mozilla", "x-ray")[i % 4], 900_000 + 1000 * i, i) for i in range(n)]
    data_h, off, _ = pack_blocks(contents)
    data = torch.from_numpy(data_h).to(dc.device)
    w = FrameWriterDevice(dc, n, settings)
    pieces, at = [[] for _ in range(n)], np.zeros(n, np.int64)
    for call in range(7):
        ln = np.array([min(int(rng.choice([0, 1, 70_000, 200_000, 333_333])), contents[i].size - int(at[i])) for i in range(n)], np.int64)
        last = call == 6
        if last:
            ln = np.array([contents[i].size - int(at[i]) for i in range(n)], np.int64)
        out, o_off, o_len = (w.close if last else w.write)(data, off.astype(np.int64) + at, ln)
        lens = o_len.cpu().numpy()
        for i in range(n):
            assert lens[i] >= 0
            pieces[i].append(out[int(o_off[i]):int(o_off[i]) + int(lens[i])])
        at += ln
    frames = [torch.cat(p) for p in pieces]
    f_len = np.array([f.numel() for f in frames], np.int64)
    f_off = np.concatenate(([0], np.cumsum((f_len + 15) // 16 * 16)))[:-1]
    arena = torch.zeros(int(f_off[-1] + f_len[-1]) + 64, dtype=torch.uint8, device=dc.device)
    for f, o in zip(frames, f_off):
        arena[int(o):int(o) + f.numel()] = f
    rd = FrameReaderDevice(dc, arena, f_off, f_len)
    got = [b""] * n
    for _ in range(40):
        counts = np.array([int(rng.choice([1, 4096, K64 - 1, K64 + 1, 150_000, 400_000])) for _ in range(n)], np.int64)
        out, r_off, r_len = rd.read(counts)
        h, ln = out.cpu().numpy(), r_len.cpu().numpy()
        assert (ln >= 0).all()
        got = [g + h[int(r_off[i]):int(r_off[i]) + int(ln[i])].tobytes() for i, g in enumerate(got)]
        if not ln.any():
            break
    for i in range(n):
        assert got[i] == contents[i].tobytes(), i
    q = rd.query().cpu().numpy()
    assert q[:, 0].tolist() == [c.size for c in contents] and (q[:, 2] == 0).all()


def _defect_plan(rng, n):
    plan = [(np.array([int(rng.choice([0, 7, K64 - 1, K64, K64 + 1, 100_000])) for _ in range(n)], np.int64), k == 1) for k in range(4)]
    return plan + [(np.full(n, 1 << 20, np.int64), False)] * 3


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_structural_defects_and_flips_under_block_checksums(dc, host):
    """the failing call's index, the code and every earlier call's bytes equal the witness's; failed streams stay failed"""
    rng = np.random.default_rng(21)
    c = corpus.class_bytes("xml", 200_000, 2).tobytes()
    lz4f = LZ4F()
    bases = [K.indep_frame(c, K64, True, True, True), lz4f.compress(np.frombuffer(c, np.uint8), 4, True, True, True, False),
             K.indep_frame(c[:70_000], K64, False, False, False, cut=30_000, raw_every=2)]
    muts = [(f"{b}:{n}", m) for b, base in enumerate(bases) for n, m in K.structural_mutants(base)]
    muts += [(f"{b}:{n}", m) for b, base in enumerate(bases[:2]) for n, m, _ in K.payload_mutants(base, rng, 16)]
    muts += K.quirk_sources()
    muts.append(("block-size-above-max", K.indep_frame(c, 256 << 10)))
    names, sources = [n for n, _ in muts], [s for _, s in muts]
    rd = Readers(dc, sources, max_block=K64, host=host)
    wit = K.check_reads(rd, sources, _defect_plan(rng, len(sources)), names, max_block=K64)
    codes = {w.failed for w in wit}
    assert codes >= {-1, -2, -3, -4, -5, -6, -7, -8, -11, None}, codes
    rd.check_store_guards()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_payload_flips_without_block_checksums(dc, host):
    """accept / reject, the failing call's index, every outLen and the guards equal the witness's; bytes are compared up to the
    start of the first mutated block (a hostile match offset of 0 leaves bytes the reference itself does not define)"""
    rng = np.random.default_rng(22)
    c = corpus.class_bytes("dickens", 250_000, 5).tobytes()
    lz4f = LZ4F()
    bases = [K.indep_frame(c, K64, False, True), lz4f.compress(np.frombuffer(c, np.uint8), 4, True, True, False, False),
             K.indep_frame(c, K64, False, False)]
    names, sources, loose = [], [], []
    for b, base in enumerate(bases):
        for n, m, k in K.payload_mutants(base, rng, 40):
            names.append(f"{b}:{n}"); sources.append(m); loose.append(k * K64)
    rd = Readers(dc, sources, max_block=K64, host=host)
    wit = K.check_reads(rd, sources, _defect_plan(rng, len(sources)), names, max_block=K64, loose_from=loose)
    assert {w.failed for w in wit} >= {-6, -8, None}
    rd.check_store_guards()


def test_python_mirror_reads_and_raises(dc):
    c = corpus.class_bytes("dickens", 300_000, 1).tobytes()
    good = K.indep_frame(c, K64, True, True, True)
    r = LZ4FrameReaderBatch([good, good + good, b""])
    assert r.FrameLength == [len(c), len(c), None]
    first = r.Read([100_000, None, 5])
    assert first == [c[:100_000], None, b""] and r.BytesRead == [100_000, 0, 0]
    assert r.Read([1 << 20, 1 << 20, 1], interactive=True) == [c[100_000:2 * K64], c[:K64], b""]
    bad = bytearray(good); bad[40] ^= 1
    with pytest.raises(F.InvalidDataException, match="block checksum"):
        LZ4FrameReaderBatch([good, bytes(bad)]).Read([10, 10])
    r = LZ4FrameReaderBatch([good, bytes(bad)], raise_errors=False)
    assert r.Read([10, 10]) == [c[:10], None] and r.LastCodes.tolist() == [0, -7] and r.Read([10, 10])[1] is None
