"""Frames with a predefined dictionary on the GPU (k4lz4_frame_dict.hpp; k4lz4_frame_sizes_dictset* / k4lz4_decode_frames_dictset*
through frames.frame_sizes_device / decode_frames_device / LZ4Frame.DecodeBatch with dictionary=): the case list of
tests/frame_dict_cases.py through the device and the host form against tests/golden/frame_dict_cases.json, every batch decoder
variant under dictionary frames, a mixed batch of 256 three-block frames, and the refusals.  DESIGN.md 4.24."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

import frame_dict_cases as FC
from k4os.compression.lz4_amd import LZ4Frame, LZ4EncoderSettings, LZ4Level, DictionarySet, DICT_FAST, DICT_HC, pack_blocks, _native
from k4os.compression.lz4_amd import frames as F
from k4os.compression.lz4_amd.device import DeviceCodec

pytestmark = pytest.mark.gpu
GUARD = 64
PAIR2, PAIR, SINGLE, DENSE = 1, 2, 3, 4          # enum k4lz4_decode_kernel


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


@pytest.fixture(scope="module")
def golden():
    return FC.load()["cases"]


@pytest.fixture(scope="module")
def E():
    return FC.entries()


@pytest.fixture(scope="module")
def dset(dc, E):
    with DictionarySet(E, owner=dc) as s:
        yield s


def cap_of(c):
    return None if c.cap == "size" else len(c.content) - 1


def device_form(dc, frames, caps, dictionary):
    """-> (outLen, outputs, size, status, dict index): frame_sizes_device and decode_frames_device into slots between guard bytes"""
    views = [np.frombuffer(bytes(f), np.uint8) for f in frames]
    data, off, _ = pack_blocks(views)
    d = torch.from_numpy(data).to(dc.device)
    off, length = off.astype(np.int64), np.array([v.size for v in views], np.int64)
    r = F.frame_sizes_device(dc, d, off, length, dictionary=dictionary)
    size, status = r[0].cpu().numpy(), r[1].cpu().numpy()
    idx = r[2].cpu().numpy() if dictionary is not None else np.full(len(frames), -1)
    cap = np.array([int(s) if c is None else int(c) for s, c in zip(size, caps)], np.int64)
    o_off = GUARD + np.concatenate(([0], np.cumsum(cap + GUARD)))[:-1]
    buf = torch.full((int((cap + GUARD).sum()) + GUARD + 64,), 0xCD, dtype=torch.uint8, device=dc.device)
    _, _, o_len = F.decode_frames_device(dc, d, off, length, out=(buf, o_off, cap), raise_errors=False, dictionary=dictionary)
    h, n = buf.cpu().numpy(), o_len.cpu().numpy()
    mask = np.ones(h.size, bool)
    for o, c in zip(o_off, cap):
        mask[int(o):int(o) + int(c)] = False
    assert (h[mask] == 0xCD).all(), "a byte outside the frames' slots was written"
    return n, [h[int(o):int(o) + int(x)].tobytes() if x >= 0 else None for o, x in zip(o_off, n)], size, status, idx


def host_form(ctx, frames, caps, dset, ids):
    """k4lz4_frame_sizes_dictset + k4lz4_decode_frames_dictset on host arrays (dset None: a NULL set)"""
    views = [np.frombuffer(bytes(f), np.uint8) for f in frames]
    n = len(views)
    src, foff, flen = pack_blocks(views)
    flen = flen.astype(np.uint64)
    size, status, idx = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.int32)
    ids = None if ids is None else np.ascontiguousarray(ids, np.uint32)
    h, ip = (dset.handle if dset is not None else None), (ids.ctypes.data if ids is not None else None)
    u8 = lambda a: a.ctypes.data_as(_native._u8p)      # noqa: E731
    ctx.check(ctx.lib.k4lz4_frame_sizes_dictset(ctx.handle, u8(src), foff.ctypes.data, flen.ctypes.data, n, size.ctypes.data, status.ctypes.data,
                                                idx.ctypes.data, h, ip))
    cap = np.array([int(s) if c is None else int(c) for s, c in zip(size, caps)], np.uint64)
    doff = (GUARD + np.concatenate(([0], np.cumsum(cap + np.uint64(GUARD))))[:-1]).astype(np.uint64)
    dst = np.full(int((cap + np.uint64(GUARD)).sum()) + GUARD + 64, 0xCD, np.uint8)
    out = np.zeros(n, np.int64)
    ctx.check(ctx.lib.k4lz4_decode_frames_dictset(ctx.handle, u8(src), foff.ctypes.data, flen.ctypes.data, n, u8(dst), doff.ctypes.data,
                                                  cap.ctypes.data, out.ctypes.data, h, ip))
    for o, c, k in zip(doff, cap, out):                  # exactly outLen bytes of a frame that decodes, none of one that fails
        assert (dst[int(o) + max(int(k), 0):int(o) + int(c)] == 0xCD).all()
        dst[int(o):int(o) + int(c)] = 0xCD
    assert (dst == 0xCD).all(), "a byte outside the frames' slots was written"
    return out, size, status, idx


def check(c, golden, out_len, out, idx):
    want = golden[c.name]["decoded"]
    if c.expect is not None:
        assert out_len == c.expect, (c.name, out_len)
    else:
        assert want != "rejected" and out_len == want[0] and FC.xxh32(out) == want[1], (c.name, out_len)
    assert idx == c.entry, (c.name, idx)


@pytest.mark.parametrize("families", [DICT_FAST | DICT_HC, DICT_HC])
def test_case_list_device_and_host_forms(dc, golden, E, families):
    """every case of the list in one batch: device form against the goldens, host form equal to the device form"""
    cs = [c for c in FC.cases() if not c.null_set]
    with DictionarySet(E, families=families, owner=dc) as s:
        n, outs, size, status, idx = device_form(dc, [c.frame for c in cs], [cap_of(c) for c in cs], (s, FC.IDS))
        for c, k, o, i in zip(cs, n, outs, idx):
            check(c, golden, int(k), o, int(i))
        assert dc.lib.k4lz4_last_decode_kernel(dc.ctx.handle) & 63 == PAIR2       # a few dozen blocks: two waves per block
        hn, hsize, hstatus, hidx = host_form(dc.ctx, [c.frame for c in cs], [cap_of(c) for c in cs], s, FC.IDS)
    assert (hn == n).all() and (hsize.astype(np.int64) == size).all() and (hstatus == status).all() and (hidx == idx).all()


def test_null_set_is_the_plain_reader(dc, golden):
    cs = FC.cases()
    frames, caps = [c.frame for c in cs], [cap_of(c) for c in cs]
    n, outs, size, status, idx = device_form(dc, frames, caps, None)
    hn, hsize, hstatus, hidx = host_form(dc.ctx, frames, caps, None, None)
    assert (hn == n).all() and (hstatus == status).all() and (hidx == -1).all()
    for c, k, o in zip(cs, n, outs):
        if c.expect in (FC.HEADER_SUM, FC.EOF):
            assert k == c.expect, c.name
        elif c.frame[4] & 1:
            assert k == FC.DICTIONARY, (c.name, k)
        else:
            check(c, golden, int(k), o, -1)


def test_every_batch_decoder_variant_takes_dictionary_blocks(dc, golden, dset):
    """the launcher picks the independent blocks' kernel by blocks per CU: small one-block frames, as many as each variant needs"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    small = [c for c in FC.cases() if c.name.startswith("hand-indep") and len(c.frame) < 200 and not c.null_set and "short-first" not in c.name]
    assert len(small) >= 10 and any(c.expect == FC.BLOCK for c in small)
    # blocks per CU inside each band of launch_decode_like (k4lz4_launch.hpp): pair2 up to hop2_max_per_cu = 12, pair up to 16, single up
    # to 24, dense beyond.  A retuned launcher moves these bands: the counts follow it, what is asserted about dictionary blocks stays.
    for per_cu, kernel in ((10, PAIR2), (14, PAIR), (20, SINGLE), (25, DENSE)):
        cs = [small[i % len(small)] for i in range(per_cu * cu)]
        n, outs, _, _, idx = device_form(dc, [c.frame for c in cs], [None] * len(cs), (dset, FC.IDS))
        assert dc.lib.k4lz4_last_decode_kernel(dc.ctx.handle) & 63 == kernel, per_cu
        done = {}
        for c, k, o, i in zip(cs, n, outs, idx):
            if (c.name, int(k), o, int(i)) != done.get(c.name):
                check(c, golden, int(k), o, int(i))
                done[c.name] = (c.name, int(k), o, int(i))


def test_mixed_batch_of_256_three_block_frames(dc, E, dset):
    """independent and chained, fast and HC, with a dictionary and plain, side by side: multi-workgroup launches of every kernel"""
    rng = np.random.default_rng(9)
    entries = (0, 5, 6, 7, 9)
    contents, idx = [], []
    for f in range(256):
        e = entries[f % len(entries)] if f % 4 else -1
        contents.append(np.frombuffer(FC.content_of(E[max(e, 0)], 2 * FC.K64 + int(rng.integers(1, 3000)), 1000 + f), np.uint8))
        idx.append(e)
    frames = [None] * 256
    kinds = [(False, LZ4Level.L00_FAST), (True, LZ4Level.L00_FAST), (False, LZ4Level.L03_HC), (True, LZ4Level.L03_HC)]
    for k, (chain, level) in enumerate(kinds):
        which = [f for f in range(256) if (f // 4) % 4 == k]
        s = LZ4EncoderSettings(ChainBlocks=chain, CompressionLevel=level, ContentChecksum=bool(k & 1), BlockChecksum=bool(k & 2))
        made = LZ4Frame.EncodeBatch([contents[f] for f in which], s, ctx=dc.ctx, dictionary=(dset, FC.IDS), dict_index=[idx[f] for f in which])
        for f, fr in zip(which, made):
            frames[f] = fr
    n, outs, _, status, got_idx = device_form(dc, frames, [None] * 256, (dset, FC.IDS))
    assert (status == 0).all() and list(got_idx) == idx
    for f in range(256):
        assert n[f] == contents[f].size and outs[f] == contents[f].tobytes(), f
    back = LZ4Frame.DecodeBatch(frames[:16], ctx=dc.ctx, dictionary=(dset, FC.IDS))
    assert back == [c.tobytes() for c in contents[:16]]


def test_refusals_and_the_python_surface(dc, E, dset):
    good = next(c for c in FC.cases() if c.name == "hand-indep-match-in-dictionary")
    src = np.frombuffer(good.frame, np.uint8).copy()
    one, ln = np.zeros(1, np.uint64), np.array([src.size], np.uint64)
    size, status, out = np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros(1, np.int64)
    dst, cap = np.zeros(256, np.uint8), np.array([256], np.uint64)
    u8 = lambda a: a.ctypes.data_as(_native._u8p)      # noqa: E731
    lib, h = dc.lib, dc.ctx.handle
    assert lib.k4lz4_frame_sizes_dictset(h, u8(src), one.ctypes.data, ln.ctypes.data, 1, size.ctypes.data, status.ctypes.data, None, dset.handle,
                                         None) == _native.E_ARG
    assert lib.k4lz4_decode_frames_dictset(h, u8(src), one.ctypes.data, ln.ctypes.data, 1, u8(dst), one.ctypes.data, cap.ctypes.data,
                                           out.ctypes.data, dset.handle, None) == _native.E_ARG
    assert "dictIds" in lib.k4lz4_last_error(h).decode()
    # the plain entry points and the bare calls keep refusing
    with pytest.raises(F.NotImplementedException):
        LZ4Frame.Decode(good.frame)
    with pytest.raises(F.NotImplementedException):
        F.frame_header(F.LZ4Descriptor(None, False, False, False, 7, 65536))
    assert LZ4Frame.Decode(good.frame, dictionary=(dset, FC.IDS)) is not None
    with pytest.raises(F.NotImplementedException):                       # a DictID nothing answers to
        LZ4Frame.Decode(good.frame, dictionary=(dset, [1] * len(FC.IDS)))
    with pytest.raises(ValueError):
        LZ4Frame.Decode(good.frame, dictionary=(dset, [1, 2]))
