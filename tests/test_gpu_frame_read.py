"""The device frame reader (k4lz4_frame_read.hpp; k4lz4_frame_sizes* / k4lz4_decode_frames* through frames.frame_sizes_device /
decode_frames_device) on the GPU: frames written on the device read back without leaving it, liblz4's frames, frames whose blocks
are not all full, a large mixed batch, damaged frames against LZ4Frame.Decode and the stream-order reader, the host-pointer
forms, and the target's edges."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

import frame_stream_reader as R
from oracle_lib import FrameOracle
from test_frame_layer import LZ4F, _contents
from test_frame_read_host import irregular_frames, empty_frames
from k4os.compression.lz4_amd import LZ4Frame, LZ4EncoderSettings, LZ4Level, corpus, pack_blocks, _native
from k4os.compression.lz4_amd import frames as F
from k4os.compression.lz4_amd.device import DeviceCodec

pytestmark = pytest.mark.gpu

# device code vs the stream-order reader's: equal, except where a bounded target makes the device name the length / capacity
# instead of what the unbounded reader meets later (include/k4lz4.h K4LZ4_FRAME_LENGTH)
ALLOWED = {(-10, -8), (-10, -6), (-9, -6)}
SAME_MESSAGE = (-1, -2, -3, -4, -7, -8)


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


@pytest.fixture(scope="module")
def fo(oracle):
    return FrameOracle(oracle)


@pytest.fixture(scope="module")
def lz4f():
    try:
        return LZ4F()
    except OSError:
        pytest.skip("liblz4.so.1 not present")


def dev_decode(dc, frames, caps=None):
    """-> [(outLen, bytes or None)] through decode_frames_device (sized by frame_sizes_device unless caps are given)"""
    views = [np.frombuffer(bytes(f), np.uint8) for f in frames]
    data, off, _ = pack_blocks(views) if views else (np.zeros(16, np.uint8), np.zeros(0, np.uint64), None)
    d = torch.from_numpy(data).to(dc.device)
    length = np.array([v.size for v in views], np.int64)
    out = None
    if caps is not None:
        caps = np.asarray(caps, np.int64)
        o_off = np.zeros(len(caps), np.int64)
        if len(caps) > 1:
            o_off[1:] = np.cumsum((caps + 15) // 16 * 16)[:-1]
        out = (torch.empty(int(((caps + 15) // 16 * 16).sum()) + 64, dtype=torch.uint8, device=dc.device), o_off, caps)
    buf, o_off, o_len = F.decode_frames_device(dc, d, off.astype(np.int64), length, out=out, raise_errors=False)
    h, n = buf.cpu().numpy(), o_len.cpu().numpy()
    return [(int(x), h[int(o):int(o) + int(x)].tobytes() if x >= 0 else None) for o, x in zip(np.asarray(o_off), n)]


def host_decode(fr):
    try:
        return None, LZ4Frame.Decode(fr)
    except Exception as e:      # noqa: BLE001 -- the class is what is compared
        return e, None


def test_round_trip_on_the_device(dc):
    contents = _contents() + [corpus.class_bytes("dickens", 1_500_000, 11)]
    data_h, off, _ = pack_blocks(contents)
    data = torch.from_numpy(data_h).to(dc.device)
    ln = np.array([c.size for c in contents], np.int64)
    cases = [(b, c, bs, cl, None) for b, c in ((False, False), (True, False), (True, True)) for bs in (65536, 262144) for cl in (False, True)]
    cases += [(True, True, 65536, True, LZ4Level.L03_HC), (False, False, 262144, False, LZ4Level.L03_HC)]
    for bsum, csum, bs, clen, lvl in cases:
        s = LZ4EncoderSettings(BlockSize=bs, BlockChecksum=bsum, ContentChecksum=csum, ContentLength=0 if clen else None,
                               ChainBlocks=lvl is not None, CompressionLevel=lvl or LZ4Level.L00_FAST)
        frames, foff, flen = F.encode_frames_device(dc, data, off.astype(np.int64), ln, s)
        out, o_off, o_len = F.decode_frames_device(dc, frames, foff, flen)          # frame_off host, frame_len device: as returned
        h, n = out.cpu().numpy(), o_len.cpu().numpy()
        for f, c in enumerate(contents):
            assert n[f] == c.size and h[int(o_off[f]):int(o_off[f]) + c.size].tobytes() == c.tobytes(), (f, bsum, csum, bs, clen, lvl)


def test_liblz4_frames_all_flags(dc, lz4f):
    contents = _contents() + [corpus.class_bytes("x-ray", 900_000, 2)]
    frames, want = [], []
    for c in contents:
        for bid in (4, 5, 6, 7):
            for linked in (False, True):
                for cs, bsum, size in ((False, False, False), (True, True, True), (True, False, False), (False, True, True)):
                    frames.append(lz4f.compress(c, bid, linked, cs, bsum, size))
                    want.append(c.tobytes())
    got = dev_decode(dc, frames)
    ref = LZ4Frame.DecodeBatch(frames)
    for i, ((n, b), w, r) in enumerate(zip(got, want, ref)):
        assert n == len(w) and b == w == r, i


def test_irregular_frames_fall_back_to_in_order_decoding(dc):
    contents = [corpus.class_bytes("dickens", 95_000, 3), corpus.class_bytes("xml", 300_001, 4), corpus.random_bytes(25_000, 5)]
    frames = LZ4Frame.EncodeBatch(contents, LZ4EncoderSettings(BlockSize=10000, BlockChecksum=True, ContentChecksum=True))
    hand = irregular_frames()
    got = dev_decode(dc, frames + [f for f, _ in hand])
    for (n, b), c in zip(got, [c.tobytes() for c in contents] + [c for _, c in hand]):
        assert n == len(c) and b == c
    # and a frame with ContentLength whose blocks are short
    clf = LZ4Frame.EncodeBatch(contents, LZ4EncoderSettings(BlockSize=10000))
    assert [b for _, b in dev_decode(dc, clf)] == [c.tobytes() for c in contents] == LZ4Frame.DecodeBatch(clf)


def _mutants(fr):
    info = F.parse_frame(fr)
    def flip(pos, x=0x01):
        b = bytearray(fr); b[pos] ^= x
        return bytes(b)
    return [flip(0), flip(6), flip(info.block_off[1] + 10), flip(len(fr) - 1), fr[:-5], flip(4, 0xC0), flip(info.block_off[0] + 5, 0xFF)]


def test_mixed_batch_of_3000_frames(dc, lz4f):
    rng = np.random.default_rng(7)
    base = [corpus.class_bytes("dickens", int(n), int(s)) for s, n in enumerate(rng.integers(1, 40000, 40))] + [np.zeros(0, np.uint8)]
    indep = LZ4Frame.EncodeBatch(base, LZ4EncoderSettings(BlockSize=65536, BlockChecksum=True, ContentChecksum=True))
    hc = LZ4Frame.EncodeBatch(base, LZ4EncoderSettings(ChainBlocks=True, CompressionLevel=LZ4Level.L03_HC, ContentChecksum=True))
    linked = [lz4f.compress(c, 4, True, True, False, True) for c in base[:20]]
    pool = [(f, c.tobytes()) for f, c in zip(indep + hc, base + base)] + [(f, c.tobytes()) for f, c in zip(linked, base)]
    pool += [(f, None) for f in empty_frames()]
    big = LZ4Frame.Encode(corpus.class_bytes("xml", 200_000, 1), LZ4EncoderSettings(BlockChecksum=True, ContentChecksum=True))
    damaged = _mutants(big)
    frames, want = [], []
    for i in range(3200):
        if i % 11 == 5:
            m = damaged[i % len(damaged)]
            frames.append(m)
            want.append(R.read_frame(m))
        else:
            f, c = pool[int(rng.integers(0, len(pool)))]
            frames.append(f)
            want.append((0, c if c is not None else b""))
    got = dev_decode(dc, frames)
    for i, ((n, b), (code, w)) in enumerate(zip(got, want)):
        if code == 0:
            assert n == len(w) and b == w, i
        else:
            assert n == code or (n, code) in ALLOWED, (i, n, code)


def _compare_with_readers(dc, muts, single_defect):
    got = dev_decode(dc, muts)
    for i, (m, (n, b)) in enumerate(zip(muts, got)):
        code, w = R.read_frame(m)
        exc, ref = host_decode(m)
        if code == 0:
            assert n == len(w) and b == w == ref, i
            continue
        assert n == code or (n, code) in ALLOWED, (i, n, code)
        mine = F.frame_exception(n)
        stream = F.frame_exception(code)
        assert type(mine) is type(stream)
        if code in SAME_MESSAGE and n == code:
            assert str(mine) == str(stream)
        assert exc is not None, i                        # LZ4Frame.Decode fails as well
        if single_defect:
            assert type(exc) is type(mine), (i, exc, mine)
            if code in SAME_MESSAGE:
                assert str(exc) == str(mine), (i, exc, mine)


def test_single_defect_mutants_match_lz4frame_decode(dc):
    data = corpus.class_bytes("dickens", 200000, 5)
    fr = LZ4Frame.Encode(data, LZ4EncoderSettings(BlockChecksum=True, ContentChecksum=True))
    fr2 = LZ4Frame.Encode(data, LZ4EncoderSettings(ContentChecksum=True))
    i2 = F.parse_frame(fr2)
    b = bytearray(fr2); b[i2.block_off[0] + 5] ^= 0xFF
    muts = _mutants(fr)[:5] + [bytes(b)]
    got = dev_decode(dc, muts)
    assert [n for n, _ in got][:5] == [-2, -4, -7, -8, -1]
    _compare_with_readers(dc, muts, True)


def test_random_byte_flips(dc, lz4f):
    rng = np.random.default_rng(12)
    c = corpus.class_bytes("xml", 150_000, 6)
    sources = [LZ4Frame.Encode(c, LZ4EncoderSettings(BlockChecksum=True, ContentChecksum=True, ContentLength=c.size)),
               LZ4Frame.Encode(c, LZ4EncoderSettings(ContentChecksum=True)),
               LZ4Frame.Encode(c, LZ4EncoderSettings(ChainBlocks=True, CompressionLevel=LZ4Level.L03_HC, BlockSize=65536)),
               lz4f.compress(c, 4, True, True, True, True), lz4f.compress(c, 4, False, False, False, False)]
    muts = []
    for fr in sources:
        for _ in range(120):
            b = bytearray(fr)
            b[int(rng.integers(0, len(fr)))] ^= int(rng.integers(1, 256))
            muts.append(bytes(b))
    _compare_with_readers(dc, muts, False)


def test_host_pointer_forms_equal_device_forms(dc, lz4f):
    contents = _contents()
    frames = [lz4f.compress(x, 4, True, True, True, True) for x in contents] + \
        LZ4Frame.EncodeBatch(contents, LZ4EncoderSettings(BlockChecksum=True)) + _mutants(LZ4Frame.Encode(contents[0]))[:5]
    views = [np.frombuffer(f, np.uint8) for f in frames]
    src, off, _ = pack_blocks(views)
    ln = np.array([v.size for v in views], np.uint64)
    n = len(frames)
    ctx = _native.default_context()
    size, status = np.zeros(n, np.uint64), np.zeros(n, np.int32)
    ctx.check(ctx.lib.k4lz4_frame_sizes(ctx.handle, src.ctypes.data, off.ctypes.data, ln.ctypes.data, n, size.ctypes.data, status.ctypes.data))
    d_size, d_status = F.frame_sizes_device(dc, torch.from_numpy(src).to(dc.device), off.astype(np.int64), ln.astype(np.int64))
    assert (d_size.cpu().numpy() == size.astype(np.int64)).all() and (d_status.cpu().numpy() == status).all()
    doff = np.zeros(n, np.uint64)
    doff[1:] = np.cumsum(size[:-1] + 7)
    dst = np.full(int(size.sum()) + 7 * n + 64, 0xA5, np.uint8)
    out = np.zeros(n, np.int64)
    ctx.check(ctx.lib.k4lz4_decode_frames(ctx.handle, src.ctypes.data, off.ctypes.data, ln.ctypes.data, n, dst.ctypes.data,
                                          doff.ctypes.data, size.ctypes.data, out.ctypes.data))
    dev = dev_decode(dc, frames)
    for f in range(n):
        assert out[f] == dev[f][0], f
        if out[f] >= 0:
            assert dst[int(doff[f]):int(doff[f]) + int(out[f])].tobytes() == dev[f][1]
            assert (dst[int(doff[f]) + int(out[f]):int(doff[f]) + int(size[f]) + 7] == 0xA5).all()       # nothing past outLen
        else:
            assert (dst[int(doff[f]):int(doff[f]) + int(size[f]) + 7] == 0xA5).all()


def test_guard_bytes_and_a_target_one_byte_short(dc, lz4f):
    contents = [corpus.class_bytes("dickens", 150_000, 2), corpus.class_bytes("xml", 65536, 3), corpus.lorem(7)]
    frames = LZ4Frame.EncodeBatch(contents, LZ4EncoderSettings(BlockChecksum=True)) + \
        [lz4f.compress(x, 4, True, False, False, False) for x in contents] + \
        LZ4Frame.EncodeBatch(contents, LZ4EncoderSettings(BlockSize=10000))
    want = [c.tobytes() for c in contents] * 3
    views = [np.frombuffer(f, np.uint8) for f in frames]
    src, off, _ = pack_blocks(views)
    ln = np.array([v.size for v in views], np.int64)
    d_src = torch.from_numpy(src).to(dc.device)
    G = 4096
    for short in (0, 1):
        caps = np.array([len(w) - short for w in want], np.int64)
        o_off = G + np.concatenate(([0], np.cumsum(caps + G)[:-1]))
        buf = torch.full((int(o_off[-1] + caps[-1] + G),), 0x5A, dtype=torch.uint8, device=dc.device)
        _, _, o_len = F.decode_frames_device(dc, d_src, off.astype(np.int64), ln, out=(buf, o_off, caps), raise_errors=False)
        h, n = buf.cpu().numpy(), o_len.cpu().numpy()
        for f, w in enumerate(want):
            lo, hi = int(o_off[f]), int(o_off[f] + caps[f])
            assert (h[lo - G:lo] == 0x5A).all() and (h[hi:hi + G] == 0x5A).all(), f          # guards untouched
            if short:
                assert n[f] == -9, f
            else:
                assert n[f] == len(w) and h[lo:hi].tobytes() == w, f
    with pytest.raises(F.InvalidDataException):
        bad = LZ4Frame.Encode(contents[0], LZ4EncoderSettings(BlockChecksum=True))
        F.decode_frames_device(dc, torch.from_numpy(np.frombuffer(_mutants(bad)[2], np.uint8).copy()).to(dc.device), [0], [len(bad)])
