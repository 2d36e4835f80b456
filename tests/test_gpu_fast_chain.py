"""Chained fast streams on the GPU (k4lz4_encode_fast_chain_batch, LZ4FastChainEncoder, encode_fast_chain_frames), block for block
and state for state against liblz4 driven through LZ4EncoderBase's ring buffer (tests/fast_chain_witness.py)."""
import struct

import numpy as np
import pytest
import torch

import fast_chain_witness as W
from test_frame_layer import LZ4F
from k4os.compression.lz4_amd import (LZ4Frame, LZ4EncoderSettings, EncoderAction, TopupAndEncode, FlushAndEncode, corpus, xxh32_many)
from k4os.compression.lz4_amd import frames as F
from k4os.compression.lz4_amd.encoders import (LZ4FastChainEncoder, encode_fast_chain_packed, encode_fast_chain_device, FAST_CHAIN_STATE,
                                               fast_chain_blocks)

pytestmark = pytest.mark.gpu

KI, MI = 1024, 1 << 20


@pytest.fixture(scope="module")
def lz4():
    try:
        lib = W.Lz4FastChainCodec.lib()
    except OSError:
        pytest.skip("liblz4.so.1 not present")
    W.check_layout()
    return lib


def _reach_back(dist: int, seed: int) -> np.ndarray:
    """random bytes; at 128 KiB the 300 bytes from `dist` before are repeated: a match of exactly that distance across the block
    boundary at 131072 (65535: the farthest a match reaches; 65536: out of reach)"""
    d = corpus.random_bytes(200000, seed).copy()
    d[131072 - 100:131072 + 200] = d[131072 - 100 - dist:131072 + 200 - dist]
    return d


def _into_block(seed: int) -> np.ndarray:
    """text whose blocks start in the middle of a repeat of earlier bytes: matches that start in the history and run into the block,
    and backward extensions that run into the block's start (lowLimit of a fresh stream's first block, anchors elsewhere)"""
    base = corpus.class_bytes("dickens", 60000, seed)
    out = np.concatenate([base, base[1000:40000], corpus.random_bytes(5000, seed), base[:30000], base])
    return out


def _runs(seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(40):
        parts.append(rng.integers(0, 256, int(rng.integers(100, 3000)), dtype=np.uint8))
        pat = rng.integers(0, 256, [1, 2, 4][k % 3], dtype=np.uint8)
        parts.append(np.tile(pat, int(rng.integers(500, 9000)) // pat.size))
    return np.concatenate(parts)


def _streams():
    """(content, blockSize, extraBlocks): a ragged batch over every block size and extraBlocks in {0, 1, 3}"""
    text = corpus.class_bytes("dickens", 1_500_000, 1)
    mix = corpus.class_bytes("mozilla", 1_200_000, 2)
    return [(text, 1 * KI, 0), (text[:400000], 1 * KI, 3), (text, 3 * KI, 1), (text, 64 * KI, 0), (mix, 64 * KI, 1), (text, 256 * KI, 3),
            (mix, 1 * MI, 0), (text, 4 * MI, 1), (corpus.class_bytes("xml", 65536 * 3, 8), 65536, 0),
            (corpus.random_bytes(300000, 3), 64 * KI, 0), (np.zeros(300000, np.uint8), 64 * KI, 3), (corpus.lorem(5), 64 * KI, 0),
            (_reach_back(65535, 4), 64 * KI, 0), (_reach_back(65536, 5), 64 * KI, 3), (_reach_back(65535, 6), 1 * KI, 0),
            (_into_block(7), 3 * KI, 0), (_into_block(8), 64 * KI, 1), (_runs(6), 1 * KI, 1), (_runs(7), 64 * KI, 0),
            (np.zeros(0, np.uint8), 64 * KI, 0), (text[:7], 64 * KI, 0), (text[:65536 + 12], 64 * KI, 0), (text[:70 * KI + 5], 1 * KI, 0),
            (corpus.repeated(9, 150000), 3 * KI, 3), (corpus.class_bytes("webster", 9 * MI, 10), 4 * MI, 0)]


def _packed_by_config(streams, allow_copy, want_state=False):
    """one call per (blockSize, extraBlocks) -- the call takes them per stream, the helper one value: group by them"""
    res = {}
    for key in sorted({(b, e) for _, b, e in streams}):
        idx = [i for i, (_, b, e) in enumerate(streams) if (b, e) == key]
        out, arena, boff, nblk, st = encode_fast_chain_packed([streams[i][0] for i in idx], key[0], key[1], allow_copy, want_state=want_state)
        k = 0
        for j, i in enumerate(idx):
            blocks = []
            for _ in range(int(nblk[j])):
                n, o = int(out[k]), int(boff[k])
                blocks.append((n, arena[o:o + abs(n)].tobytes()))
                k += 1
            res[i] = (blocks, None if st is None else st[j])
    return [res[i] for i in range(len(streams))]


@pytest.mark.parametrize("allow_copy", [True, False])
def test_fast_chain_batch_equals_liblz4_witness_block_for_block_and_state(lz4, allow_copy):
    streams = _streams()
    got = _packed_by_config(streams, allow_copy, want_state=True)
    for i, (data, B, e) in enumerate(streams):
        want, wst = W.witness_stream(data, B, e, allow_copy)
        blocks, st = got[i]
        assert len(blocks) == len(want), i
        bad = [j for j, (a, b) in enumerate(zip(blocks, want)) if a != b]
        assert not bad, (i, B, e, bad[:5])
        assert np.array_equal(st["hashTable"], wst["hashTable"]), i
        assert int(st["currentOffset"]) == wst["currentOffset"] and int(st["dictSize"]) == wst["dictSize"], i


def test_one_call_with_mixed_block_sizes_equals_per_config_calls(lz4):
    from k4os.compression.lz4_amd import _native
    streams = _streams()[:12]
    ctx = _native.default_context()
    views = [s for s, _, _ in streams]
    bs = [b for _, b, _ in streams]
    ex = [e for _, _, e in streams]
    out, arena, boff, nblk, _ = encode_fast_chain_packed(views, bs, ex, True, ctx)
    k = 0
    for i, (data, B, e) in enumerate(streams):
        want, _ = W.witness_stream(data, B, e, True)
        got = []
        for _ in range(int(nblk[i])):
            got.append((int(out[k]), arena[int(boff[k]):int(boff[k]) + abs(int(out[k]))].tobytes()))
            k += 1
        assert got == want, i


def test_device_form_equals_host_form(lz4):
    from k4os.compression.lz4_amd.device import DeviceCodec
    streams = [s for s, b, e in _streams() if (b, e) == (64 * KI, 0)]
    out_h, arena_h, boff_h, nblk_h, st_h = encode_fast_chain_packed(streams, 64 * KI, 0, True, want_state=True)
    dc = DeviceCodec(0)
    lens = np.array([c.size for c in streams], np.int64)
    offs = np.concatenate(([0], np.cumsum(lens)))[:-1].astype(np.uint64)
    data_d = torch.from_numpy(np.concatenate(streams)).to(dc.device)
    out_d, arena_d, boff_d, nblk_d, st_d = encode_fast_chain_device(dc, data_d, offs, lens, 64 * KI, 0, True, want_state=True)
    torch.cuda.synchronize()
    out_d, a = out_d.cpu().numpy(), arena_d.cpu().numpy()
    assert np.array_equal(out_d, out_h) and np.array_equal(nblk_d, nblk_h)
    for n, oh, od in zip(out_h, boff_h, boff_d):
        assert a[int(od):int(od) + abs(int(n))].tobytes() == arena_h[int(oh):int(oh) + abs(int(n))].tobytes()
    assert st_d.cpu().numpy().tobytes() == st_h.tobytes()
    # a device state continues a stream on the device: the second half of every stream from the first half's state
    cut = [min(c.size, 3 * 65536) for c in streams]
    halves = [c[:k] for c, k in zip(streams, cut)]
    _, _, _, _, st_first = encode_fast_chain_packed(halves, 64 * KI, 0, True, want_state=True)
    rest = [c[k - int(s["dictSize"]):] for c, k, s in zip(streams, cut, st_first)]
    rl = np.array([r.size for r in rest], np.int64)
    ro = np.concatenate(([0], np.cumsum(rl)))[:-1].astype(np.uint64)
    rest_d = torch.from_numpy(np.concatenate(rest)).to(dc.device)
    st_in_d = torch.from_numpy(st_first.view(np.uint8).copy()).to(dc.device)
    o2, ar2, bo2, nb2, st2 = encode_fast_chain_device(dc, rest_d, ro, rl, 64 * KI, 0, True, state_in=st_in_d, want_state=True,
                                                      dictLen=st_first["dictSize"].astype(np.int32))
    torch.cuda.synchronize()
    assert st2.cpu().numpy().tobytes() == st_h.tobytes()


def test_more_streams_than_resident_waves(lz4):
    rng = np.random.default_rng(11)
    text = corpus.class_bytes("dickens", 2_000_000, 12)
    starts = rng.integers(0, text.size - 40000, 3200)
    lens = rng.integers(0, 40000, 3200)
    streams = [text[s:s + n] for s, n in zip(starts, lens)]
    out, arena, boff, nblk, st = encode_fast_chain_packed(streams, 4 * KI, 1, True, want_state=True)
    k = 0
    for i in range(0, len(streams), 7):                        # a checked subset (the witness is one stream at a time)
        k = int(nblk[:i].sum())
        want, wst = W.witness_stream(streams[i], 4 * KI, 1, True)
        got = [(int(out[k + j]), arena[int(boff[k + j]):int(boff[k + j]) + abs(int(out[k + j]))].tobytes()) for j in range(int(nblk[i]))]
        assert got == want, i
        assert np.array_equal(st[i]["hashTable"], wst["hashTable"]) and int(st[i]["currentOffset"]) == streams[i].size


def test_encoder_encode_encode_blocks_topup_and_encode(lz4):
    data = _into_block(3)
    B = 4 * KI
    want, wst = W.witness_stream(data, B, 1, True)
    # Encode block by block
    enc = LZ4FastChainEncoder(B, 1)
    got = []
    dst = np.zeros(B + B // 255 + 16, np.uint8)
    for p in range(0, data.size, B):
        enc.Topup(data[p:p + B])
        n = enc.Encode(dst, allowCopy=True)
        got.append((n, dst[:abs(n)].tobytes()))
    assert got == want
    assert np.array_equal(enc.State[0]["hashTable"], wst["hashTable"])
    # EncodeBlocks in a few calls
    enc = LZ4FastChainEncoder(B, 1)
    got = []
    blocks = [data[p:p + B] for p in range(0, data.size, B)]
    for lo, hi in ((0, 5), (5, 40), (40, len(blocks))):
        got += [(-len(p) if a == EncoderAction.Copied else len(p), p) for a, p in enc.EncodeBlocks(blocks[lo:hi])]
    assert got == want
    # TopupAndEncode / FlushAndEncode with ragged Topup sizes
    for sizes in ([1000, 7000, 3], [B], [5 * B + 17]):
        enc = LZ4FastChainEncoder(B, 1)
        want_r, _ = W.witness_stream(data, B, 1, True, topups=sizes)
        got, pos, k = [], 0, 0
        while pos < data.size:
            piece = data[pos:pos + sizes[k % len(sizes)]]
            k += 1
            action, loaded, n = TopupAndEncode(enc, piece, dst, False, True)
            pos += loaded
            if action in (EncoderAction.Encoded, EncoderAction.Copied):
                got.append((n if action == EncoderAction.Encoded else -n, dst[:abs(n)].tobytes()))
        action, n = FlushAndEncode(enc, dst, True, True)
        if action in (EncoderAction.Encoded, EncoderAction.Copied):
            got.append((n if action == EncoderAction.Encoded else -n, dst[:abs(n)].tobytes()))
        assert got == want_r == want


@pytest.fixture(scope="module")
def lz4f():
    try:
        return LZ4F()
    except OSError:
        pytest.skip("liblz4.so.1 not present")


def _xxh(b):
    return int(xxh32_many([np.frombuffer(b, np.uint8) if isinstance(b, bytes) else b])[0])


def _witness_frame(blocks, block_size, content, bsum, csum, content_length):
    bd = {65536: 4, 262144: 5, 1 << 20: 6, 4 << 20: 7}
    code = next(v for k, v in sorted(bd.items()) if block_size <= k)
    hdr = bytes([(1 << 6) | (int(bsum) << 4) | (int(content_length) << 3) | (int(csum) << 2), code << 4])
    if content_length:
        hdr += struct.pack("<Q", content.size)
    parts = [struct.pack("<I", 0x184D2204), hdr, bytes([(_xxh(hdr) >> 8) & 0xFF])]
    for n, data in blocks:
        parts.append(struct.pack("<I", len(data) | (0x80000000 if n < 0 else 0)))
        parts.append(data)
        if bsum:
            parts.append(struct.pack("<I", _xxh(data)))
    parts.append(struct.pack("<I", 0))
    if csum:
        parts.append(struct.pack("<I", _xxh(content)))
    return b"".join(parts)


@pytest.mark.parametrize("bsum,csum", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("block_size,extra_memory,content_length", [(65536, 0, False), (65536, 200000, True), (262144, 1, False)])
def test_fast_chain_frames_equal_witness_and_decode_everywhere(lz4, lz4f, bsum, csum, block_size, extra_memory, content_length):
    contents = [corpus.class_bytes("dickens", 500000, 1), corpus.random_bytes(70000, 3), corpus.lorem(5), _runs(4),
                corpus.repeated(7, 300000)]
    if not content_length:
        contents.append(np.zeros(0, np.uint8))
    extra = F._extra_blocks(block_size, extra_memory)
    for group in ([c] for c in contents) if content_length else [contents]:
        s = LZ4EncoderSettings(ChainBlocks=True, BlockSize=block_size, BlockChecksum=bsum, ContentChecksum=csum, ExtraMemory=extra_memory,
                               ContentLength=group[0].size if content_length else None)
        frames = F.encode_fast_chain_frames(group, s)
        for data, fr in zip(group, frames):
            blocks, _ = W.witness_stream(data, block_size, extra, True)
            assert fr == _witness_frame(blocks, block_size, data, bsum, csum, content_length)
            assert F.parse_frame(fr).descriptor.Chaining
            r, out, used = lz4f.decompress(fr, data.size + 16)
            assert r == 0 and used == len(fr) and out == data.tobytes()
        assert LZ4Frame.DecodeBatch(frames) == [c.tobytes() for c in group]


def test_block_table_of_the_library_is_the_models():
    # blocks per stream as the call reports them = the model's count (ragged lengths, both ends of the grid)
    lens = [0, 1, 12, 13, 1024, 65536, 65537, 300000]
    out, arena, boff, nblk, _ = encode_fast_chain_packed([np.zeros(n, np.uint8) for n in lens], 1024, 2, True)
    assert list(nblk) == [len(fast_chain_blocks(n, 1024, 2)) for n in lens]
