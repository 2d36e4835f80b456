"""The incremental frame writer on the GPU (k4lz4_frame_write_batch*): every call's bytes per stream against the witness
(frame_writer_witness.py: LZ4FrameWriter transcribed over the oracle's engine and liblz4), the host and device forms against each other,
whole frames against LZ4Frame.EncodeBatch / encode_fast_chain_frames and both readers."""
import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

from frame_writer_witness import WitnessWriter
from oracle_lib import Oracle
from k4os.compression.lz4_amd import LZ4Codec, LZ4Level, LZ4Frame, LZ4EncoderSettings, corpus
from k4os.compression.lz4_amd.device import DeviceCodec
from k4os.compression.lz4_amd.frames import (LZ4FrameWriterBatch, FrameWriterDevice, encode_frames_device, decode_frames_device,
                                             encode_fast_chain_frames, FWRITE_TARGET, FWRITE_CLOSED, FWRITE_LENGTH)

pytestmark = pytest.mark.gpu
K64 = 65536


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def pool():
    rng = np.random.default_rng(11)
    text = corpus.silesia_like_blocks(16, K64, seed=4).reshape(-1)
    noise = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    return np.concatenate([text, noise, text[::-1].copy()])


KINDS = [dict(), dict(CompressionLevel=LZ4Level.L03_HC), dict(CompressionLevel=LZ4Level.L09_HC), dict(CompressionLevel=LZ4Level.L12_MAX),
         dict(ChainBlocks=True, CompressionLevel=LZ4Level.L03_HC), dict(ChainBlocks=True, CompressionLevel=LZ4Level.L09_HC, ExtraMemory=1),
         dict(ChainBlocks=True), dict(ChainBlocks=True, ExtraMemory=200000), dict(BlockSize=256 << 10)]


def _sizes(rng, B):
    pick = rng.integers(0, 7)
    return int([0, rng.integers(1, 16), B, 2 * B, rng.integers(1, 200000), B - 1, rng.integers(16, 4000)][pick])


def _plan(n, calls, seed):
    """per stream: settings (mixed kinds, checksums, some with the content size) and its write sizes"""
    rng = np.random.default_rng(seed)
    settings, sizes = [], []
    for i in range(n):
        k = dict(KINDS[i % len(KINDS)])
        bs = k.pop("BlockSize", K64)
        sz = [_sizes(rng, bs) for _ in range(calls)]
        sz = [s if rng.random() > 0.15 else -1 for s in sz]             # -1: the stream sits this call out
        cl = sum(max(s, 0) for s in sz) if i % 5 == 0 else None
        settings.append(LZ4EncoderSettings(BlockSize=bs, BlockChecksum=bool(rng.integers(0, 2)), ContentChecksum=bool(rng.integers(0, 2)),
                                           ContentLength=cl, **k))
        sizes.append(sz)
    return settings, sizes


def _chunk(pool, rng, n):
    at = int(rng.integers(0, pool.size - n)) if n < pool.size else 0
    return pool[at:at + n]


def test_every_call_matches_the_witness_host_and_device_forms(dc, oracle, pool):
    n, calls = 96, 5
    settings, sizes = _plan(n, calls, 1)
    rng = np.random.default_rng(2)
    host = LZ4FrameWriterBatch(n, settings)
    dev = FrameWriterDevice(dc, n, settings)
    wit = [WitnessWriter(s, oracle=oracle) for s in settings]
    frames = [b""] * n
    contents = [b""] * n
    for c in range(calls + 1):
        closing = c == calls
        chunks = [None if (not closing and sizes[i][c] < 0) else (_chunk(pool, rng, sizes[i][c]) if not closing else None) for i in range(n)]
        if closing:
            got_h = host.Close()
            out, ooff, olen = dev.close()
            want = [w.close() for w in wit]
        else:
            got_h = host.Write(chunks)
            lens = np.array([-1 if ch is None else ch.size for ch in chunks], np.int64)
            packed = np.concatenate([ch for ch in chunks if ch is not None] + [np.zeros(1, np.uint8)])
            off = np.concatenate(([0], np.cumsum(np.maximum(lens, 0))))[:-1]
            data = torch.from_numpy(packed).to(dc.device)
            out, ooff, olen = dev.write(data, off, lens)
            want = [b"" if ch is None else w.write(ch) for w, ch in zip(wit, chunks)]
        torch.cuda.synchronize()
        out_h, olen_h = out.cpu().numpy(), olen.cpu().numpy()
        for i in range(n):
            got_d = out_h[int(ooff[i]):int(ooff[i]) + int(olen_h[i])].tobytes()
            if chunks[i] is None and not closing:
                assert got_h[i] is None and olen_h[i] == 0
                continue
            assert got_h[i] == want[i], (c, i, settings[i], len(got_h[i]), len(want[i]))
            assert got_d == want[i], (c, i, settings[i])
            frames[i] += want[i]
            if chunks[i] is not None:
                contents[i] += chunks[i].tobytes()
    for i in range(n):
        assert LZ4Frame.Decode(frames[i]) == contents[i], i
    blob = np.frombuffer(b"".join(frames), np.uint8)
    foff = np.concatenate(([0], np.cumsum([len(f) for f in frames])))[:-1]
    buf, doff, dlen = decode_frames_device(dc, torch.from_numpy(blob.copy()).to(dc.device), foff, [len(f) for f in frames])
    b, dl = buf.cpu().numpy(), dlen.cpu().numpy()
    for i in range(n):
        assert b[int(doff[i]):int(doff[i]) + int(dl[i])].tobytes() == contents[i], i
    # a closed stream refuses more
    assert host.Write([b"x"] * n) == [None] * n and (host.LastCodes == FWRITE_CLOSED).all()


@pytest.mark.parametrize("kind", range(len(KINDS)))
def test_one_write_and_close_is_encode_batch(dc, pool, kind):
    k = dict(KINDS[kind])
    contents = [pool[:0], pool[:1], pool[:K64], pool[3:3 * K64 + 5], pool[K64 * 5:K64 * 5 + 700000]]
    for bc, cc in ((False, False), (True, True)):
        s = LZ4EncoderSettings(BlockChecksum=bc, ContentChecksum=cc, **k)
        if s.ChainBlocks and int(s.CompressionLevel) < 3:
            want = encode_fast_chain_frames(contents, s)
        else:
            want = LZ4Frame.EncodeBatch(contents, s)
        w = LZ4FrameWriterBatch(len(contents), s)
        got = [a + b for a, b in zip(w.Write(contents), w.Close())]
        assert got == want


def test_content_length_mismatch_is_refused(pool):
    s = LZ4EncoderSettings(ContentLength=10)
    w = LZ4FrameWriterBatch(2, s)
    w.Write([pool[:4], pool[:10]])
    got = w.Close()
    assert got[0] is None and w.LastCodes[0] == FWRITE_LENGTH
    assert got[1] is not None and w.LastCodes[1] == 0
    more = w.Write([pool[:6], None])
    assert more[0] == b"" and w.Close([0])[0] is not None


def test_short_target_keeps_the_stream_and_retry_matches(dc, oracle, pool):
    n = 64
    settings = [LZ4EncoderSettings(BlockChecksum=True, ContentChecksum=True, **KINDS[i % len(KINDS)]) for i in range(n)]
    dev = FrameWriterDevice(dc, n, settings)
    wit = [WitnessWriter(s, oracle=oracle) for s in settings]
    data_h = pool[:300000]
    data = torch.from_numpy(data_h.copy()).to(dc.device)
    lens = np.full(n, 300000, np.int64)
    caps = dev.bound(lens)
    caps[0] -= 1
    caps[7] = 0
    out, ooff, olen = dev.write(data, np.zeros(n, np.int64), lens, dst_cap=caps)
    ol = olen.cpu().numpy()
    assert ol[0] == FWRITE_TARGET and ol[7] == FWRITE_TARGET
    o = out.cpu().numpy()
    for i in range(n):
        if i in (0, 7):
            continue
        assert o[int(ooff[i]):int(ooff[i]) + int(ol[i])].tobytes() == wit[i].write(data_h), i
    retry = np.where(np.isin(np.arange(n), (0, 7)), 300000, -1)
    out, ooff, olen = dev.write(data, np.zeros(n, np.int64), retry)
    o, ol = out.cpu().numpy(), olen.cpu().numpy()
    for i in (0, 7):
        assert o[int(ooff[i]):int(ooff[i]) + int(ol[i])].tobytes() == wit[i].write(data_h), i
    out, ooff, olen = dev.close()
    o, ol = out.cpu().numpy(), olen.cpu().numpy()
    for i in range(n):
        assert o[int(ooff[i]):int(ooff[i]) + int(ol[i])].tobytes() == wit[i].close(), i
    # the context still encodes whole frames
    content = pool[:5 * K64 + 3]
    fr, foff, flen = encode_frames_device(dc, torch.from_numpy(content.copy()).to(dc.device), np.zeros(1, np.int64),
                                          np.array([content.size]), LZ4EncoderSettings(BlockChecksum=True))
    got = fr.cpu().numpy()[int(foff[0]):int(foff[0]) + int(flen.cpu()[0])].tobytes()
    assert got == LZ4Frame.Encode(content, LZ4EncoderSettings(BlockChecksum=True))


def test_open_writes_the_header_alone_and_enforce32(oracle, pool):
    s = LZ4EncoderSettings(ContentChecksum=True)
    w = LZ4FrameWriterBatch(3, s)
    wit = WitnessWriter(s, oracle=oracle)
    header = wit.open()
    assert w.Open([0, 1]) == [header, header, None]
    assert w.Open([0])[0] == b""
    assert w.Close([2]) == [None, None, b""]                           # a frame never opened: CloseFrame writes nothing
    try:
        LZ4Codec.Enforce32 = True
        big = pool[:5 * K64 + 9]
        w32 = LZ4FrameWriterBatch(1, LZ4EncoderSettings())
        ww = WitnessWriter(LZ4EncoderSettings(), x32=True, oracle=oracle)
        assert w32.Write([big])[0] + w32.Close()[0] == ww.write(big) + ww.close()
        with pytest.raises(ValueError):
            LZ4FrameWriterBatch(1, LZ4EncoderSettings(ChainBlocks=True)).Write([big])
    finally:
        LZ4Codec.Enforce32 = False


def test_large_blocks_multi_mib_writes_and_closes_that_carry_bytes(dc, oracle, pool):
    """1 MiB and 4 MiB blocks, writes of several MiB, and CLOSE calls with bytes (Write then CloseFrame in one call) on streams that
    are open and on streams never opened: device form against the witness"""
    big = np.resize(pool, 24 << 20)
    kinds = [dict(BlockSize=1 << 20), dict(BlockSize=4 << 20, BlockChecksum=True, ContentChecksum=True),
             dict(BlockSize=1 << 20, ChainBlocks=True, CompressionLevel=LZ4Level.L03_HC, ContentChecksum=True),
             dict(BlockSize=4 << 20, ChainBlocks=True), dict(BlockSize=1 << 20, ChainBlocks=True, ExtraMemory=1, BlockChecksum=True)]
    n = 10
    settings = [LZ4EncoderSettings(**kinds[i % len(kinds)]) for i in range(n)]
    dev = FrameWriterDevice(dc, n, settings)
    wit = [WitnessWriter(s, oracle=oracle) for s in settings]
    data = torch.from_numpy(big).to(dc.device)
    rng = np.random.default_rng(21)

    def check(out, ooff, olen, want):
        o, ol = out.cpu().numpy(), olen.cpu().numpy()
        for i in range(n):
            assert o[int(ooff[i]):int(ooff[i]) + int(ol[i])].tobytes() == want[i], (i, settings[i])

    for call in range(2):
        lens = np.array([-1 if i >= n - 2 else int(rng.choice([3 << 20, (5 << 20) + 7, 4 << 20])) for i in range(n)], np.int64)
        off = rng.integers(0, big.size - (6 << 20), n)
        want = [b"" if lens[i] < 0 else wit[i].write(big[off[i]:off[i] + lens[i]]) for i in range(n)]
        check(*dev.write(data, off, lens), want)
    lens = np.array([(2 << 20) + 5 if i % 2 else 0 for i in range(n)], np.int64)    # odd streams close with bytes; the last two never opened
    off = rng.integers(0, big.size - (3 << 20), n)
    want = [wit[i].write_close(big[off[i]:off[i] + lens[i]]) if lens[i] else wit[i].close() for i in range(n)]
    check(*dev.close(data, off, lens), want)
