"""The frame writer with a predefined dictionary on device-resident contents (frames.encode_frames_device with
dictionary=(DictionarySet, ids) and dict_index): the header against liblz4's for the same preferences, the block payloads against the
dictionary encoders and the chain encoders opened from the entry called directly, every frame read back on the device by the reader
with the set (its target sized by frame_sizes_device) and by LZ4F_decompress_usingDict, and the frames equal to the host writer's.
DESIGN.md 4.24."""
import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

import frame_dict_cases as FC
from test_gpu_frame_dict_writer import LEVELS, settings, payloads, contents, dc, E, dset   # noqa: F401  (fixtures)
from k4os.compression.lz4_amd import LZ4Codec, LZ4Frame, LZ4EncoderSettings, LZ4Level, pack_blocks
from k4os.compression.lz4_amd import frames as F
from k4os.compression.lz4_amd.encoders import LZ4Encoder

pytestmark = pytest.mark.gpu


def written(dc, dset, items, s):
    """-> (frames as bytes, the device tensors encode_frames_device returned)"""
    data_h, off, _ = pack_blocks([np.frombuffer(c, np.uint8) for _, c in items])
    data = torch.from_numpy(data_h).to(dc.device)
    ln = np.array([len(c) for _, c in items], np.int64)
    frames, foff, flen = F.encode_frames_device(dc, data, off.astype(np.int64), ln, s, dictionary=(dset, FC.IDS), dict_index=[e for e, _ in items])
    h, n = frames.cpu().numpy(), flen.cpu().numpy()
    return [h[int(o):int(o) + int(k)].tobytes() for o, k in zip(foff, n)], (frames, foff, flen)


def of_kind(contents, chain, level):
    """the chained fast writer takes no plain frames (as without a dictionary)"""
    return [(e, c) for e, c in contents if e >= 0 or not (chain and level < LZ4Level.L03_HC)]


@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("level", LEVELS)
def test_device_writer(dc, dset, contents, E, chain, level):
    items = of_kind(contents, chain, level)
    s = settings(chain, level, int(level) + chain)
    frames, (frames_d, foff, flen) = written(dc, dset, items, s)
    for (e, c), fr in zip(items, frames):
        info, got = payloads(fr)
        assert info.descriptor.Dictionary == (FC.IDS[e] if e >= 0 else None) and info.descriptor.Chaining == chain
        if e < 0:
            assert fr == LZ4Frame.Encode(c, s)
            continue
        # the payloads: the encoders called directly
        if chain:
            enc = LZ4Encoder.Create(True, level, FC.K64, 0, dc.ctx, dictionary=(dset, e))
            want, pos, target = [], 0, np.zeros(LZ4Codec.MaximumOutputSize(enc.BlockSize), np.uint8)
            while pos < len(c):
                pos += enc.Topup(c, pos)
                n = enc.Encode(target, allowCopy=True)
                want.append((n < 0, target[:abs(n)].tobytes()))
        else:
            blocks = [c[p:p + FC.K64] for p in range(0, len(c), FC.K64)]
            direct = LZ4Codec.EncodeDictBatch(blocks, dset, [e] * len(blocks), level)
            want = [(True, b) if len(d) >= len(b) else (False, d) for b, d in zip(blocks, direct)]
        assert got == want, (e, len(c))
        # the header: liblz4's for the same preferences; and liblz4 reads the frame
        if FC.liblz4() is not None:
            ref = FC.lz4f_make([c], E[e].tobytes(), FC.IDS[e], chain, s.BlockChecksum, s.ContentChecksum, False)
            assert fr[:11] == ref[:11], (e, level)
            assert FC.lz4f_decode(fr, E[e].tobytes(), len(c) + 64) == c, (e, level)
    assert any(raw for fr in frames for raw, _ in payloads(fr)[1])
    # the host writer writes the same bytes
    assert frames == LZ4Frame.EncodeBatch([c for _, c in items], s, ctx=dc.ctx, dictionary=(dset, FC.IDS), dict_index=[e for e, _ in items])
    # read back on the device, the target sized by frame_sizes_device with the set
    out, o_off, o_len = F.decode_frames_device(dc, frames_d, foff, flen, dictionary=(dset, FC.IDS))
    h, n = out.cpu().numpy(), o_len.cpu().numpy()
    for f, (_, c) in enumerate(items):
        assert n[f] == len(c) and h[int(o_off[f]):int(o_off[f]) + len(c)].tobytes() == c, f
    size, status, idx = F.frame_sizes_device(dc, frames_d, foff, flen, dictionary=(dset, FC.IDS))
    assert (status.cpu().numpy() == 0).all() and list(idx.cpu().numpy()) == [e for e, _ in items]
    assert (size.cpu().numpy() >= np.array([len(c) for _, c in items])).all()
    if any(e >= 0 and c for e, c in items):
        with pytest.raises(F.NotImplementedException):                   # without the set the reader refuses as before
            F.decode_frames_device(dc, frames_d, foff, flen)


def test_content_length_fills_fourteen_header_bytes(dc, dset, E):
    c = FC.content_of(E[0], 30000, 8)
    s = LZ4EncoderSettings(ContentLength=0, ContentChecksum=True)
    frames, _ = written(dc, dset, [(7, c), (-1, c)], s)
    info = F.parse_frame(frames[0])
    assert info.descriptor.ContentLength == len(c) and info.descriptor.Dictionary == FC.IDS[7] and len(info.header) == 14
    assert F.parse_frame(frames[1]).descriptor.Dictionary is None and len(F.parse_frame(frames[1]).header) == 10
    assert LZ4Frame.DecodeBatch(frames, ctx=dc.ctx, dictionary=(dset, FC.IDS)) == [c, c]
    if FC.liblz4() is not None:
        assert frames[0][:19] == FC.lz4f_make([c], E[7].tobytes(), FC.IDS[7], False, False, True, True)[:19]


def test_device_writer_refusals(dc, dset):
    data = torch.zeros(256, dtype=torch.uint8, device=dc.device)
    off, ln = np.zeros(1, np.int64), np.array([100], np.int64)
    d = (dset, FC.IDS)
    for level in (LZ4Level.L10_OPT, LZ4Level.L12_MAX):
        with pytest.raises(F.NotImplementedException):
            F.encode_frames_device(dc, data, off, ln, LZ4EncoderSettings(CompressionLevel=level), dictionary=d, dict_index=[0])
        F.encode_frames_device(dc, data, off, ln, LZ4EncoderSettings(CompressionLevel=level), dictionary=d, dict_index=[-1])    # plain: as ever
        assert LZ4Frame.Encode(b"x" * 100, level=level, dictionary=d, dict_index=-1) == LZ4Frame.Encode(b"x" * 100, level=level)
    with pytest.raises(ValueError):
        F.encode_frames_device(dc, data, off, ln, dictionary=d, dict_index=[len(FC.IDS)])
    with pytest.raises(ValueError):
        F.encode_frames_device(dc, data, off, ln, dictionary=d, dict_index=[0, 0])
    with pytest.raises(F.NotImplementedException):                       # chained fast frames without an entry: refused as before
        F.encode_frames_device(dc, data, off, ln, LZ4EncoderSettings(ChainBlocks=True), dictionary=d, dict_index=[-1])
    with pytest.raises(F.NotImplementedException):
        F.encode_frames_device(dc, data, off, ln, LZ4EncoderSettings(ChainBlocks=True))
    LZ4Codec.Enforce32 = True
    try:
        with pytest.raises(F.NotImplementedException):
            F.encode_frames_device(dc, data, off, ln, dictionary=d, dict_index=[0])
    finally:
        LZ4Codec.Enforce32 = False
