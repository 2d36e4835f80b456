"""The host-pointer forms of the stream calls (k4lz4_capi.hip, HostStage) on the GPU: k4lz4_xxh32_batch and
k4lz4_decode_chain_batch against their device forms, and the failure contract of a host-pointer call -- one that fails
part-way leaves its context ready for the next call."""
import numpy as np
import pytest
import torch

from oracle_lib import FrameOracle
from k4os.compression.lz4_amd import LZ4EncoderSettings, LZ4Frame, LZ4Legacy, LZ4Level, corpus, pack_blocks, _native
from k4os.compression.lz4_amd import frames as F
from k4os.compression.lz4_amd.device import DeviceCodec

pytestmark = pytest.mark.gpu

GUARD = 0xCD


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


def test_xxh32_host_form_equals_device_form(dc, oracle):
    rng = np.random.default_rng(5)
    lens = [0, 1, 3, 4, 15, 16, 17, 0, 31, 1000, 65539, 0, 262144 + 5]
    bufs = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    # ragged and not adjacent: a gap of 1..40 bytes in front of every buffer, the zero-length ones included
    off, pos = [], 0
    for b in bufs:
        pos += int(rng.integers(1, 41))
        off.append(pos)
        pos += b.size
    data = np.zeros(pos + 8, np.uint8)
    for o, b in zip(off, bufs):
        data[o:o + b.size] = b
    off = np.array(off, np.uint64)
    ln = np.array(lens, np.uint64)
    n = len(lens)
    fo = FrameOracle(oracle)
    ctx = _native.default_context()
    d_data = torch.from_numpy(data).to(dc.device)
    for seed in (0, 0x9E3779B1):
        host = np.zeros(n, np.uint32)
        ctx.check(ctx.lib.k4lz4_xxh32_batch(ctx.handle, data.ctypes.data, off.ctypes.data, ln.ctypes.data, host.ctypes.data, n, seed))
        dev = dc.xxh32(d_data, torch.from_numpy(off.astype(np.int64)).to(dc.device), torch.from_numpy(ln.astype(np.int64)).to(dc.device),
                       seed)
        torch.cuda.synchronize()
        assert (dev.cpu().numpy().view(np.uint32) == host).all(), seed
        assert [int(x) for x in host] == [fo.xxh32(b, seed) for b in bufs], seed


def _chain_streams():
    """(frames, chained flags, contents): block-linked frames (HC), independent-block frames, one with raw blocks"""
    rng = np.random.default_rng(9)
    contents = [corpus.class_bytes("dickens", 150_000, 1), corpus.class_bytes("xml", 70_000, 2), corpus.lorem(3),
                rng.integers(0, 256, 20_000, dtype=np.uint8), np.zeros(0, np.uint8)]
    linked = LZ4Frame.EncodeBatch(contents, LZ4EncoderSettings(ChainBlocks=True, BlockSize=65536, CompressionLevel=LZ4Level.L03_HC))
    indep = LZ4Frame.EncodeBatch(contents, LZ4EncoderSettings(BlockSize=65536))
    return linked + indep, [1] * len(contents) + [0] * len(contents), contents + contents


def test_decode_chain_host_form_equals_device_form(dc):
    frames, chained, contents = _chain_streams()
    # one more stream with no room at all: the first linked frame, capacity 0
    frames, chained, caps = frames + frames[:1], chained + [1], [c.size for c in contents] + [0]
    views = [np.frombuffer(bytes(f), np.uint8) for f in frames]
    src, foff, _ = pack_blocks(views)
    blk_off, blk_len, first, nblk, bsize = [], [], [], [], []
    for f, v in enumerate(views):
        info = F.parse_frame(v)
        first.append(len(blk_off))
        nblk.append(len(info.block_off))
        blk_off += [int(foff[f]) + o for o in info.block_off]
        blk_len += list(info.block_len)
        bsize.append(info.descriptor.BlockSize)
    assert any(x & 0x80000000 for x in blk_len)           # raw blocks are part of the batch
    n, nb = len(frames), len(blk_off)
    bo, bl = np.array(blk_off, np.uint64), np.array(blk_len, np.uint32)
    first, nblk = np.array(first, np.uint64), np.array(nblk, np.uint32)
    bsize, chained, caps = np.array(bsize, np.int32), np.array(chained, np.uint8), np.array(caps, np.uint64)
    # every caller slot between guard bytes: 16 in front of each slot, 16 behind the last one
    doff = np.zeros(n, np.uint64)
    doff[0] = 16
    doff[1:] = 16 + np.cumsum(caps[:-1] + 16)
    dst = np.full(int(doff[-1] + caps[-1]) + 16, GUARD, np.uint8)
    out = np.zeros(n, np.int64)
    ctx = _native.default_context()
    ctx.check(ctx.lib.k4lz4_decode_chain_batch(ctx.handle, src.ctypes.data, bo.ctypes.data, bl.ctypes.data, nb, first.ctypes.data,
                                               nblk.ctypes.data, bsize.ctypes.data, chained.ctypes.data, dst.ctypes.data,
                                               doff.ctypes.data, caps.ctypes.data, out.ctypes.data, n))

    def t(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(dc.device)
    d_dst = torch.zeros(dst.size, dtype=torch.uint8, device=dc.device)
    d_out = dc.decode_chain(t(src, np.uint8), t(bo, np.int64), t(bl, np.int32), t(first, np.int64), t(nblk, np.int32),
                            t(bsize, np.int32), t(chained, np.uint8), d_dst, t(doff, np.int64), t(caps, np.int64))
    torch.cuda.synchronize()
    d_out, d_dst = d_out.cpu().numpy(), d_dst.cpu().numpy()
    assert (out == d_out).all(), (out, d_out)
    assert (out[:-1] == [c.size for c in contents]).all() and out[-1] < 0
    covered = np.zeros(dst.size, bool)
    for i in range(n):
        o, k = int(doff[i]), int(out[i])
        if k > 0:
            assert dst[o:o + k].tobytes() == d_dst[o:o + k].tobytes() == contents[i].tobytes(), i
            covered[o:o + k] = True
    assert (dst[~covered] == GUARD).all()                  # guard bytes and every byte past an outLen untouched


def test_failed_host_call_leaves_the_context_usable():
    ctx = _native.Context(0)
    try:
        content = corpus.class_bytes("dickens", 100_000, 4)
        frame = np.frombuffer(LZ4Frame.Encode(content), np.uint8).copy()
        off, ln = np.zeros(1, np.uint64), np.array([frame.size], np.uint64)
        out = np.zeros(1, np.int64)
        # a capacity no allocator can give: the call fails at allocation, before any kernel runs
        huge = np.array([1 << 62], np.uint64)
        dst, doff = np.zeros(64, np.uint8), np.zeros(1, np.uint64)
        rc = ctx.lib.k4lz4_decode_frames(ctx.handle, frame.ctypes.data, off.ctypes.data, ln.ctypes.data, 1, dst.ctypes.data,
                                         doff.ctypes.data, huge.ctypes.data, out.ctypes.data)
        assert rc == _native.E_NOMEM
        assert "out of device/pinned memory" in ctx.lib.k4lz4_last_error(ctx.handle).decode()
        # the same context: an ordinary frame call and an ordinary legacy-stream call
        cap = np.array([content.size], np.uint64)
        dst = np.zeros(content.size, np.uint8)
        ctx.check(ctx.lib.k4lz4_decode_frames(ctx.handle, frame.ctypes.data, off.ctypes.data, ln.ctypes.data, 1, dst.ctypes.data,
                                              doff.ctypes.data, cap.ctypes.data, out.ctypes.data))
        assert out[0] == content.size and dst.tobytes() == content.tobytes()
        stream = np.frombuffer(LZ4Legacy.Encode(content, blockSize=32768), np.uint8).copy()
        sln = np.array([stream.size], np.uint64)
        dst[:] = 0
        out[:] = 0
        ctx.check(ctx.lib.k4lz4_decode_legacy_streams(ctx.handle, stream.ctypes.data, off.ctypes.data, sln.ctypes.data, 1,
                                                      dst.ctypes.data, doff.ctypes.data, cap.ctypes.data, out.ctypes.data))
        assert out[0] == content.size and dst.tobytes() == content.tobytes()
    finally:
        ctx.close()
