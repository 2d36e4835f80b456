"""Chained HC streams on the GPU (k4lz4_encode_hc_chain_batch, LZ4HighChainEncoder, chained frames), block for block
against liblz4 driven through LZ4EncoderBase's ring buffer (tests/hc_chain_witness.py)."""
import numpy as np
import pytest
import torch

import hc_chain_witness as W
from test_frame_layer import LZ4F
from k4os.compression.lz4_amd import (LZ4Frame, LZ4EncoderSettings, LZ4Level, EncoderAction, TopupAndEncode, FlushAndEncode,
                                      corpus, xxh32_many, _native)
from k4os.compression.lz4_amd import frames as F
from k4os.compression.lz4_amd.encoders import LZ4HighChainEncoder, encode_hc_chain_packed

pytestmark = pytest.mark.gpu

KI, MI = 1024, 1 << 20


@pytest.fixture(scope="module")
def lz4():
    try:
        return W.Lz4HcCodec.lib()
    except OSError:
        pytest.skip("liblz4.so.1 not present")


def _reach_back(dist: int, seed: int) -> np.ndarray:
    """random bytes; at 128 KiB the 300 bytes from `dist` before are repeated, so a match of exactly that distance crosses the
    64 KiB block boundary at 131072 (65535: the farthest a match reaches; 65536: out of reach)"""
    d = corpus.random_bytes(200000, seed).copy()
    d[131072 - 100:131072 + 200] = d[131072 - 100 - dist:131072 + 200 - dist]
    return d


def _runs(seed: int) -> np.ndarray:
    """runs of 1 / 2 / 4-byte patterns between random stretches, so that level 9's pattern analysis meets runs that began
    before a save of the ring buffer"""
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(40):
        parts.append(rng.integers(0, 256, int(rng.integers(100, 3000)), dtype=np.uint8))
        pat = rng.integers(0, 256, [1, 2, 4][k % 3], dtype=np.uint8)
        parts.append(np.tile(pat, int(rng.integers(500, 9000)) // pat.size))
    return np.concatenate(parts)


def _streams(level: int):
    """(content, blockSize, extraBlocks): a ragged batch over every block size and extraBlocks in {0, 1, 3}"""
    small = level >= 10                                       # (the optimal parser: shorter inputs, as the witness runs at MB/s)
    text = corpus.class_bytes("dickens", 700000 if small else 1_500_000, 1)
    mix = corpus.class_bytes("mozilla", 600000 if small else 1_200_000, 2)
    out = [(text, 1 * KI, 0), (text, 64 * KI, 0), (mix, 64 * KI, 1), (text, 256 * KI, 3), (mix, 1 * MI, 0), (text, 4 * MI, 1),
           (corpus.random_bytes(300000, 3), 64 * KI, 0), (_reach_back(65535, 4), 64 * KI, 0), (_reach_back(65536, 5), 64 * KI, 3),
           (_runs(6), 1 * KI, 1), (_runs(7), 64 * KI, 0), (corpus.lorem(5), 64 * KI, 0), (np.zeros(0, np.uint8), 64 * KI, 0),
           (corpus.repeated(9, 150000), 3 * KI, 3), (corpus.class_bytes("xml", 65536 * 3, 8), 65536, 0)]
    if not small:
        out.append((corpus.class_bytes("webster", 9 * MI, 10), 4 * MI, 0))
    return out


def _slots(streams):
    Bs = [(max(b, KI) + KI - 1) // KI * KI for _, b, _ in streams]
    nblk = [-(-c.size // B) for (c, _, _), B in zip(streams, Bs)]
    slot = [B + B // 255 + 16 for B in Bs]
    doff = np.concatenate(([0], np.cumsum([n * s for n, s in zip(nblk, slot)])))[:-1].astype(np.uint64)
    return Bs, nblk, slot, doff


@pytest.mark.parametrize("level", [3, 4, 6, 9, 10, 11, 12])
def test_chain_batch_equals_liblz4_witness_block_for_block(lz4, level):
    streams = _streams(level)
    want = [W.witness_blocks(c, level, b, e) for c, b, e in streams]
    out, arena, boff, nblk = encode_hc_chain_packed([c for c, _, _ in streams], [b for _, b, _ in streams],
                                                    [e for _, _, e in streams], LZ4Level(level), True)
    assert nblk.tolist() == [len(w) for w in want]
    k = 0
    for si, w in enumerate(want):
        for j, (n, data) in enumerate(w):
            got = arena[int(boff[k]):int(boff[k]) + abs(int(out[k]))].tobytes()
            assert int(out[k]) == n and got == data, (level, si, j, int(out[k]), n)
            k += 1


def test_host_call_leaves_guard_bytes_and_device_call_gives_the_same_bytes(lz4):
    streams = [(corpus.class_bytes("dickens", 400000, 1), 64 * KI, 0), (corpus.random_bytes(100000, 2), 16 * KI, 1),
               (_runs(3), 1 * KI, 3), (np.zeros(0, np.uint8), 4 * KI, 0), (corpus.lorem(3), 4 * MI, 0)]
    Bs, nblk, slot, doff = _slots(streams)
    src = np.concatenate([c for c, _, _ in streams])
    soff = np.concatenate(([0], np.cumsum([c.size for c, _, _ in streams])))[:-1].astype(np.uint64)
    slen = np.array([c.size for c, _, _ in streams], np.int64)
    bs = np.array([b for _, b, _ in streams], np.int32)
    ex = np.array([e for _, _, e in streams], np.int32)
    nb = sum(nblk)
    total = int(sum(n * s for n, s in zip(nblk, slot)))
    lib = _native.load_library()
    ctx = _native.default_context()
    for level in (3, 9, 10):
        dst = np.full(total + 64, 0xA5, np.uint8)
        out = np.zeros(nb + 1, np.int32)
        ctx.check(lib.k4lz4_encode_hc_chain_batch(ctx.handle, src.ctypes.data, soff.ctypes.data, slen.ctypes.data, bs.ctypes.data,
                                                  ex.ctypes.data, None, len(streams), dst.ctypes.data, doff.ctypes.data, out.ctypes.data,
                                                  nb + 1, level, _native.FLAG_ALLOW_COPY))
        written = np.zeros(dst.size, bool)
        k = 0
        for si, (c, b, e) in enumerate(streams):
            w = W.witness_blocks(c, level, b, e)
            for j, (n, data) in enumerate(w):
                at = int(doff[si]) + j * slot[si]
                assert int(out[k]) == n and dst[at:at + abs(n)].tobytes() == data
                written[at:at + abs(n)] = True
                k += 1
        assert (dst[~written] == 0xA5).all()                  # nothing outside the blocks' bytes, and the guard after every slot
        # the device form: same bytes, and a slot's bytes past its block stay as they were
        dev = torch.device("cuda", ctx.device)
        d_src = torch.from_numpy(src).to(dev)
        d_dst = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device=dev)
        d_out = torch.zeros(nb, dtype=torch.int32, device=dev)
        ctx.check(lib.k4lz4_encode_hc_chain_batch_device(ctx.handle, d_src.data_ptr(), soff.ctypes.data, slen.ctypes.data, bs.ctypes.data,
                                                         ex.ctypes.data, None, len(streams), d_dst.data_ptr(), doff.ctypes.data,
                                                         d_out.data_ptr(), nb, level, _native.FLAG_ALLOW_COPY, None))
        torch.cuda.synchronize()
        h = d_dst.cpu().numpy()
        assert d_out.cpu().numpy().tolist() == out[:nb].tolist()
        assert (h[written] == dst[written]).all() and (h[total:] == 0x5A).all()
        # a block stored raw may leave bytes of its (longer) encoding behind its -outLen bytes inside its slot, as the independent
        # device path with K4LZ4_FLAG_ALLOW_COPY does; every other slot is untouched behind its block
        k = 0
        for si, n_s in enumerate(nblk):
            for j in range(n_s):
                at = int(doff[si]) + j * slot[si]
                if out[k] > 0:
                    assert (h[at + int(out[k]):at + slot[si]] == 0x5A).all(), (si, j)
                k += 1


def test_enforce32_gives_the_same_bytes(lz4):
    lib = _native.load_library()
    contents = [corpus.class_bytes("dickens", 300000, 4), _runs(5)]
    ref = encode_hc_chain_packed(contents, 64 * KI, 1, LZ4Level.L09_HC, True)
    lib.k4lz4_set_enforce32(1)
    try:
        got = encode_hc_chain_packed(contents, 64 * KI, 1, LZ4Level.L09_HC, True)
    finally:
        lib.k4lz4_set_enforce32(0)
    assert got[0].tolist() == ref[0].tolist()
    for k in range(len(ref[0])):
        n = abs(int(ref[0][k]))
        assert got[1][int(got[2][k]):int(got[2][k]) + n].tobytes() == ref[1][int(ref[2][k]):int(ref[2][k]) + n].tobytes()


def test_chain_encoder_topup_encode_and_encode_blocks(lz4):
    data = corpus.class_bytes("dickens", 200000, 7)
    want = W.witness_blocks(data, 6, 16 * KI, 1)
    enc = LZ4HighChainEncoder(LZ4Level.L06_HC, 16 * KI, 1)
    got, pos = [], 0
    target = np.zeros(16 * KI + 16 * KI // 255 + 16, np.uint8)
    while pos < data.size:
        action, loaded, encoded = TopupAndEncode(enc, data[pos:], target, False, True)
        pos += loaded
        if action in (EncoderAction.Encoded, EncoderAction.Copied):
            got.append((encoded if action == EncoderAction.Encoded else -encoded, target[:encoded].tobytes()))
    action, encoded = FlushAndEncode(enc, target, True, True)
    if action != EncoderAction.None_:
        got.append((encoded if action == EncoderAction.Encoded else -encoded, target[:encoded].tobytes()))
    assert got == want
    enc2 = LZ4HighChainEncoder(LZ4Level.L06_HC, 16 * KI, 1)
    B = enc2.BlockSize
    res = enc2.EncodeBlocks([data[p:p + B] for p in range(0, 5 * B, B)]) + \
        enc2.EncodeBlocks([data[p:p + B] for p in range(5 * B, data.size, B)])
    assert [(a, b) for a, b in res] == [(EncoderAction.Copied if n < 0 else EncoderAction.Encoded, d) for n, d in want]


@pytest.fixture(scope="module")
def lz4f():
    try:
        return LZ4F()
    except OSError:
        pytest.skip("liblz4.so.1 not present")


def _xxh(b):
    return int(xxh32_many([np.frombuffer(b, np.uint8) if isinstance(b, bytes) else b])[0])


@pytest.mark.parametrize("bsum,csum", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("block_size,extra_memory", [(65536, 0), (65536, 200000), (262144, 1)])
def test_chained_frames_equal_witness_and_decode_everywhere(lz4, lz4f, bsum, csum, block_size, extra_memory):
    from k4os.compression.lz4_amd.device import DeviceCodec
    contents = [corpus.class_bytes("dickens", 500000, 1), corpus.random_bytes(70000, 3), corpus.lorem(5), np.zeros(0, np.uint8),
                _runs(4), corpus.repeated(7, 300000)]
    s = LZ4EncoderSettings(ChainBlocks=True, CompressionLevel=LZ4Level.L09_HC, BlockSize=block_size, BlockChecksum=bsum,
                           ContentChecksum=csum, ExtraMemory=extra_memory)
    frames = LZ4Frame.EncodeBatch(contents, s)
    extra = F._extra_blocks(block_size, extra_memory)
    for data, fr in zip(contents, frames):
        want = W.frame_from_blocks(W.witness_blocks(data, 9, block_size, extra), block_size, data, bsum, csum, _xxh)
        assert fr == want
        assert F.parse_frame(fr).descriptor.Chaining
        r, out, used = lz4f.decompress(fr, data.size + 16)
        assert r == 0 and used == len(fr) and out == data.tobytes()
    assert LZ4Frame.DecodeBatch(frames) == [c.tobytes() for c in contents]
    # the device-resident writer
    dc = DeviceCodec(0)
    lens = np.array([c.size for c in contents], np.int64)
    offs = np.concatenate(([0], np.cumsum(lens)))[:-1]
    data_d = torch.from_numpy(np.concatenate(contents)).to(dc.device)
    fr_d, fr_off, fr_len = F.encode_frames_device(dc, data_d, offs, lens, s)
    torch.cuda.synchronize()
    h, fl = fr_d.cpu().numpy(), fr_len.cpu().numpy()
    assert [h[int(o):int(o) + int(n)].tobytes() for o, n in zip(fr_off, fl)] == frames


def test_chained_fast_frames_still_refused():
    data = corpus.lorem(3)
    with pytest.raises(F.NotImplementedException, match="parse"):
        LZ4Frame.Encode(data, LZ4EncoderSettings(ChainBlocks=True))
