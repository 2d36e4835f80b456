"""LZ4Stream written and read piece by piece on the GPU (k4lz4_legacy_stream.hpp through the C ABI, host and device form), call by
call against the witness (legacy_stream_witness.py over the compiled reference engine).  Guard bytes lie around every output
slot, every store and every source."""
import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

from legacy_witness import Witness
from legacy_stream_witness import WriterCalls, read_calls, lazy_flush
from test_legacy_host import valid_streams, damaged_streams
from k4os.compression.lz4_amd import LZ4Legacy, corpus
from k4os.compression.lz4_amd import legacy as L
from k4os.compression.lz4_amd.device import DeviceCodec

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


@pytest.fixture(scope="module")
def w():
    return Witness()


def guarded(pieces, fill):
    """pieces behind each other with GUARD bytes of `fill` around each -> (array, offsets, lengths)"""
    lens = np.array([len(p) for p in pieces], np.int64)
    off = GUARD + np.concatenate(([0], np.cumsum(lens[:-1] + GUARD))).astype(np.int64) if len(pieces) else np.zeros(0, np.int64)
    buf = np.full(int(lens.sum()) + GUARD * (len(pieces) + 1) + 16, fill, np.uint8)
    for p, o in zip(pieces, off):
        buf[int(o):int(o) + len(p)] = np.frombuffer(bytes(p), np.uint8)
    return buf, off, lens


def guards_intact(buf, off, caps, fill, what):
    mask = np.ones(buf.size, bool)
    for o, c in zip(off, caps):
        mask[int(o):int(o) + int(c)] = False
    assert (buf[mask] == fill).all(), f"a write outside {what}"


def guard_stores(obj, dev, n, sizes):
    """replace an object's store by one with guard bytes around every stream's part"""
    sizes = np.broadcast_to(np.asarray(sizes, np.int64), (n,))
    off = (256 + np.concatenate(([0], np.cumsum(sizes[:-1] + 256)))).astype(np.int64)
    obj.store = torch.full((int(sizes.sum()) + 256 * (n + 1),), 0xA5, dtype=torch.uint8, device=dev)
    return off, sizes


# ---- writer -----------------------------------------------------------------------------------------------------------------
BLOCKS = [16, 4096, 65536, 1 << 20]


def writer_plan(n=64, calls=7, seed=1):
    """per stream (B, high); per call and stream a piece of content or None (sits the call out), and per call the op"""
    rng = np.random.default_rng(seed)
    kinds = [(BLOCKS[i % 4], (i // 4) % 2 == 1) for i in range(n)]
    pool = {c: corpus.class_bytes(c, 5 << 20, 7).tobytes() for c in ("dickens", "xml")}
    pool["noise"] = rng.integers(0, 256, 5 << 20, dtype=np.uint8).tobytes()
    steps = []
    for k in range(calls):
        op = "write" if k < 3 else str(rng.choice(["write", "write", "flush"]))
        pieces = []
        for i, (B, high) in enumerate(kinds):
            if rng.random() < 0.12:
                pieces.append(None)
                continue
            if op == "flush":
                pieces.append(b"")
                continue
            several = B * int(rng.integers(2, 4)) + int(rng.integers(0, 9)) if not (high and B == 1 << 20) else B + 9
            size = int(rng.choice([0, int(rng.integers(1, 16)), B - 1, B, B + 1, several]))
            src = pool[str(rng.choice(["dickens", "xml", "noise"], p=[0.45, 0.4, 0.15]))]
            at = int(rng.integers(0, len(src) - size))
            pieces.append(src[at:at + size])
        steps.append((op, pieces))
    return kinds, steps


def witness_steps(w, kinds, steps):
    wcs = [WriterCalls(w, high, B) for B, high in kinds]
    want = []
    for op, pieces in steps:
        want.append([None if p is None else (wc.write(p) if op == "write" else wc.flush() if op == "flush" else wc.dispose(p))
                     for wc, p in zip(wcs, pieces)])
    return want


@pytest.fixture(scope="module")
def plan(w):
    kinds, steps = writer_plan()
    steps.append(("close", [b"tail" * (i % 3) for i in range(len(kinds))]))
    return kinds, steps, witness_steps(w, kinds, steps)


def test_writer_host_form_every_call_equals_the_witness(w, plan):
    kinds, steps, want = plan
    wb = L.LZ4StreamWriterBatch(len(kinds), [h for _, h in kinds], [b for b, _ in kinds])
    whole = [bytearray() for _ in kinds]
    for (op, pieces), exp in zip(steps, want):
        got = wb.Write(pieces) if op == "write" else wb.Flush([i for i, p in enumerate(pieces) if p is not None]) if op == "flush" \
            else wb.Close(pieces)
        assert (wb.LastCodes == 0).all()
        for i in range(len(kinds)):
            assert got[i] == exp[i], (op, i, kinds[i])
            whole[i] += got[i] or b""
    contents = [b"".join(p for _, ps in steps for p in [ps[i]] if p) for i in range(len(kinds))]
    assert LZ4Legacy.DecodeBatch([bytes(x) for x in whole]) == contents
    # a closed stream refuses, and keeps refusing
    assert wb.Write([b"x"] * len(kinds)) == [None] * len(kinds) and (wb.LastCodes == L.LEGACY_CLOSED).all()


def test_writer_device_form_guards_and_decode(dc, w, plan):
    kinds, steps, want = plan
    n = len(kinds)
    wd = L.LegacyWriterDevice(dc, n, [h for _, h in kinds], [b for b, _ in kinds])
    soff, ssize = guard_stores(wd, dc.device, n, [int(dc.lib.k4lz4_legacy_writer_store_bytes(L.C.byref(wd.records[i]))) for i in range(n)])
    wd.store_off = soff.astype(np.uint64)
    whole = [bytearray() for _ in kinds]
    for (op, pieces), exp in zip(steps, want):
        src, off, lens = guarded([p or b"" for p in pieces], 0xEE)
        lens = np.array([-1 if p is None else len(p) for p in pieces], np.int64)
        opc = {"write": L.LWRITE_WRITE, "flush": L.LWRITE_FLUSH, "close": L.LWRITE_CLOSE}[op]
        caps = wd.bound(lens, opc)
        out, ooff, _ = guarded([bytes(int(c)) for c in caps], 0xCD)
        out[:] = 0xCD
        buf = torch.from_numpy(out).to(dc.device)
        _, _, olen = wd._call(torch.from_numpy(src).to(dc.device), off, lens, opc, dst_cap=caps, out=(buf, ooff))
        h, ol = buf.cpu().numpy(), olen.cpu().numpy()
        guards_intact(h, ooff, np.maximum(ol, 0), 0xCD, "a stream's output")
        for i in range(n):
            if exp[i] is None:
                assert ol[i] == 0
                continue
            got = h[int(ooff[i]):int(ooff[i]) + int(ol[i])].tobytes()
            assert ol[i] >= 0 and got == exp[i], (op, i, kinds[i])
            whole[i] += got
    guards_intact(wd.store.cpu().numpy(), soff, ssize, 0xA5, "a stream's store")
    contents = [b"".join(p for _, ps in steps for p in [ps[i]] if p) for i in range(n)]
    sbuf, so, sl = guarded([bytes(x) for x in whole], 0)
    buf, o, olen = L.decode_legacy_streams_device(dc, torch.from_numpy(sbuf).to(dc.device), so, sl)
    h, ol = buf.cpu().numpy(), olen.cpu().numpy()
    for i in range(n):
        assert h[int(o[i]):int(o[i]) + int(ol[i])].tobytes() == contents[i], i


@pytest.mark.parametrize("high", [False, True])
def test_one_write_and_close_equals_encode_batch(high):
    xml = corpus.class_bytes("xml", 70001, 2).tobytes()
    contents = [xml[:n] for n in (0, 1, 15, 16, 17, 4095, 4096, 4097, 70001)] + \
        [np.random.default_rng(2).integers(0, 256, 9000, dtype=np.uint8).tobytes()]
    for B in (16, 4096):
        want = LZ4Legacy.EncodeBatch(contents, high, B)
        wb = L.LZ4StreamWriterBatch(len(contents), high, B)
        a = wb.Write(contents)
        b = wb.Close()
        assert [x + y for x, y in zip(a, b)] == want
        assert L.LZ4StreamWriterBatch(len(contents), high, B).Close(contents) == want


def test_refused_for_a_short_target_then_retried(w):
    n, B = 8, 4096
    pieces = [corpus.class_bytes("dickens", 3 * B + 7 + i, 3).tobytes() for i in range(n)]
    wb = L.LZ4StreamWriterBatch(n, False, B)
    first = wb.Write([p[:100] for p in pieces])
    assert first == [b""] * n
    caps = np.array([wb.Bound(i, len(pieces[i]) - 100) for i in range(n)], np.uint64)
    short = caps.copy()
    short[::2] -= 1
    got = wb.Write([p[100:] for p in pieces], dst_cap=short)
    assert [g is None for g in got] == [i % 2 == 0 for i in range(n)]
    assert (wb.LastCodes[::2] == L.LEGACY_CAPACITY).all() and (wb.LastCodes[1::2] == 0).all()
    again = wb.Write([pieces[i][100:] if i % 2 == 0 else None for i in range(n)], dst_cap=caps)
    tail = wb.Close()
    for i in range(n):
        wc = WriterCalls(w, False, B)
        wc.write(pieces[i][:100])
        assert (again[i] if i % 2 == 0 else got[i]) == wc.write(pieces[i][100:]), i
        assert tail[i] == wc.dispose(), i


def test_x32_and_flush_arguments(w):
    w32 = Witness(x32=True)
    from k4os.compression.lz4_amd import LZ4Codec
    c = corpus.class_bytes("dickens", 70000, 5).tobytes()
    try:
        LZ4Codec.Enforce32 = True
        wb = L.LZ4StreamWriterBatch(1, False, 65536)
        got = wb.Write([c])[0] + wb.Close()[0]
    finally:
        LZ4Codec.Enforce32 = False
    assert got == w32.encode_stream(c, False, 65536)
    wb = L.LZ4StreamWriterBatch(1)
    with pytest.raises(Exception):
        wb._call([b"abc"], L.LWRITE_FLUSH)                       # a flush takes no bytes
    assert wb.records[0].pending == 0


# ---- reader -----------------------------------------------------------------------------------------------------------------
def reader_sources(w):
    rng = np.random.default_rng(9)
    text = corpus.class_bytes("xml", 900000, 4).tobytes()
    noise = rng.integers(0, 256, 200000, dtype=np.uint8).tobytes()
    ours = LZ4Legacy.EncodeBatch([text[:n] for n in (300000, 65536, 65537, 5000)], False, 65536) + \
        LZ4Legacy.EncodeBatch([text[:200000], noise[:70000]], False, 4096) + LZ4Legacy.EncodeBatch([text[:150000]], True, 65536)
    irregular = [w.encode_stream(text[:90000] + noise[:30000] + text[:50000], False, 16384, pieces=[100, 20000, 1, 16384, 50000], flush_after=True),
                 w.encode_stream(noise[:50000], False, 4096, pieces=[5, 4096, 7000], flush_after=True),
                 w.encode_stream(text[:40000], True, 4096, pieces=[4095, 1, 4097], flush_after=True)]
    a, b = w.encode_stream(text[:30000], False, 8192), w.encode_stream(text[30000:70000], False, 8192)
    irregular.append(a + b"\x00\x00" + b"\x01\x00\x00" + b)                          # empty chunks spliced in
    out = ours + irregular + valid_streams(w)
    while len(out) < 64:
        out.append(out[len(out) % 11])
    return out


def mutants(w):
    base = w.encode_stream(corpus.class_bytes("dickens", 40000, 6).tobytes(), False, 4096)
    out = list(damaged_streams(w))
    rng = np.random.default_rng(10)
    for _ in range(24):                                                               # payload flips
        m = bytearray(base)
        m[int(rng.integers(8, len(m)))] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(m))
    out += [base[:k] for k in (len(base) // 3, len(base) // 2, len(base) - 1)]
    return out


def random_count_calls(rng, n, calls, scale):
    return [[None if rng.random() < 0.08 else int(rng.choice([0, 1, 15, 4096, 4097, int(rng.integers(1, scale)), scale]))
             for _ in range(n)] for _ in range(calls)]


def check_call(want, got_bytes, got_len, i, k):
    if want is None:
        assert got_len == 0, (k, i)
    elif isinstance(want, int):
        assert got_len == want, (k, i, got_len, want)
    else:
        assert got_len == len(want) and got_bytes == want, (k, i, got_len, len(want))


@pytest.mark.parametrize("interactive", [False, True])
@pytest.mark.parametrize("which", ["valid", "mutants"])
def test_reader_host_form(w, interactive, which):
    srcs = reader_sources(w) if which == "valid" else mutants(w)
    n = len(srcs)
    rng = np.random.default_rng(12)
    calls = random_count_calls(rng, n, 12, 70000 if which == "valid" else 9000)
    want = [read_calls(w, s, [c[i] for c in calls], interactive, 1 << 20) for i, s in enumerate(srcs)]
    rb = L.LZ4StreamReaderBatch(srcs, raise_errors=False)
    for k, counts in enumerate(calls):
        got = rb.Read(counts, interactive)
        for i in range(n):
            wk = want[i][k]
            if isinstance(wk, int):
                assert got[i] is None and rb.LastCodes[i] == wk, (k, i, rb.LastCodes[i], wk)
            else:
                assert got[i] == wk, (k, i)
    if which == "mutants":
        with pytest.raises(Exception):
            rr = L.LZ4StreamReaderBatch([srcs[-1]])
            rr.Read([1 << 20])


@pytest.mark.parametrize("interactive", [False, True])
@pytest.mark.parametrize("which", ["valid", "mutants"])
def test_reader_device_form_guards(dc, w, interactive, which):
    srcs = reader_sources(w) if which == "valid" else mutants(w)
    n = len(srcs)
    rng = np.random.default_rng(13)
    calls = random_count_calls(rng, n, 12, 70000 if which == "valid" else 9000)
    want = [read_calls(w, s, [c[i] for c in calls], interactive, 65536) for i, s in enumerate(srcs)]
    sbuf, so, sl = guarded(srcs, 0xEE)
    rd = L.LegacyReaderDevice(dc, torch.from_numpy(sbuf).to(dc.device), so, sl, maxBlockSize=65536)
    soff, ssize = guard_stores(rd, dc.device, n, int(rd.record.storeBytes))
    rd.store_off = torch.from_numpy(soff).to(dc.device)
    rd._call(L.LREAD_RESET, rd._zero, None, None, False)
    for k, counts in enumerate(calls):
        c = np.array([-1 if x is None else x for x in counts], np.int64)
        out, ooff, _ = guarded([bytes(max(int(x), 0)) for x in c], 0xCD)
        out[:] = 0xCD
        buf = torch.from_numpy(out).to(dc.device)
        _, _, olen = rd.read(c, out=(buf, ooff), interactive=interactive, max_count=int(c.max()))
        h, ol = buf.cpu().numpy(), olen.cpu().numpy()
        guards_intact(h, ooff, np.maximum(c, 0), 0xCD, "a stream's slot")
        for i in range(n):
            check_call(want[i][k], h[int(ooff[i]):int(ooff[i]) + max(int(ol[i]), 0)].tobytes(), int(ol[i]), i, k)
    guards_intact(rd.store.cpu().numpy(), soff, ssize, 0xA5, "a stream's store")
    q = rd.query().cpu().numpy()
    if which == "valid" and not interactive:
        assert (q[:, L.LSQ_BATCHED] > 0).any() and (q[:, L.LSQ_CODE] == 0).all()


def test_direct_path_serves_some_streams_and_hands_others_back_in_one_call(dc, w):
    """one call, both kinds: streams the direct path served (their chunks went through the batch decoder) and streams it handed
    back because a payload in the planned range does not decode -- the general kernel reports the defect where the reference does"""
    text = corpus.class_bytes("dickens", 60000, 8).tobytes()
    good = w.encode_stream(text, False, 4096)
    bad = bytearray(good)
    chunks, _ = w.read_chunks(good)
    at = chunks[5][3]
    bad[at] = 0xFF; bad[at + 1] = 0xFF; bad[at + 2] = 0xFF                           # the sixth chunk's first token: literals past its end
    srcs = [good, bytes(bad)] * 4 + [good[:len(good) - 3]]                            # ... and a truncated last chunk
    n = len(srcs)
    sbuf, so, sl = guarded(srcs, 0xEE)
    rd = L.LegacyReaderDevice(dc, torch.from_numpy(sbuf).to(dc.device), so, sl, maxBlockSize=4096)
    counts = [[8192] * n, [30000] * n, [30000] * n]
    want = [read_calls(w, s, [c[i] for c in counts], False, 4096) for i, s in enumerate(srcs)]
    for k, c in enumerate(counts):
        buf, ooff, olen = rd.read(np.array(c, np.int64))
        h, ol = buf.cpu().numpy(), olen.cpu().numpy()
        q = rd.query().cpu().numpy()
        for i in range(n):
            check_call(want[i][k], h[int(ooff[i]):int(ooff[i]) + max(int(ol[i]), 0)].tobytes(), int(ol[i]), i, k)
        if k == 0:
            assert (q[:, L.LSQ_BATCHED] > 0).all() and (q[:, L.LSQ_HANDED_BACK] == 0).all()     # two whole chunks: before any defect
        if k == 1:                                                                    # the call with both kinds
            assert (q[0:8:2, L.LSQ_HANDED_BACK] == 0).all() and (q[0:8:2, L.LSQ_BATCHED] > 3).all()
            assert (q[1:8:2, L.LSQ_HANDED_BACK] == 1).all() and (q[1:8:2, L.LSQ_CODE] == L.LEGACY_INVALID_DATA).all()
            assert (ol[1:8:2] == L.LEGACY_INVALID_DATA).all() and (ol[0:8:2] == 30000).all()
    assert isinstance(want[8][2], int) and want[8][2] == L.LEGACY_END_OF_STREAM


def test_writer_output_read_back_without_a_host_copy(dc, w):
    """every call's output is a whole number of chunks: it goes straight from the writer's device buffer into a reader"""
    n, B = 16, 65536
    rng = np.random.default_rng(14)
    content = [corpus.class_bytes("xml", int(rng.integers(1, 5 * B)), i).tobytes() for i in range(n)]
    data, off, lens = guarded(content, 0xEE)
    d = torch.from_numpy(data).to(dc.device)
    wd = L.LegacyWriterDevice(dc, n, [i % 2 == 1 for i in range(n)], B)
    half = lens // 2
    total = torch.zeros(n, dtype=torch.int64, device=dc.device)
    got = [b""] * n
    pending = np.zeros(n, np.int64)
    for length, o, op in ((half, off, "write"), (lens - half, off + half, "close")):
        buf, ooff, olen = wd.write(d, o, length) if op == "write" else wd.close(d, o, length)
        emitted = np.array([pending[i] + length[i] - lazy_flush(B, int(pending[i]), int(length[i]), op)[1] for i in range(n)], np.int64)
        pending = pending + length - emitted
        rd = L.LegacyReaderDevice(dc, buf, ooff, olen, maxBlockSize=B)                # olen stays on the device
        rbuf, roff, rlen = rd.read(emitted + 5)
        h, rl = rbuf.cpu().numpy(), rlen.cpu().numpy()
        assert (rl == emitted).all()
        for i in range(n):
            got[i] += h[int(roff[i]):int(roff[i]) + int(rl[i])].tobytes()
        total += olen
    assert got == content and (pending == 0).all() and (total.cpu().numpy() > 0).all()
