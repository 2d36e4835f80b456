"""The frame writer with a predefined dictionary on the GPU (LZ4Frame.EncodeBatch / Encode with dictionary=(DictionarySet, ids) and
dict_index): the header against liblz4's for the same preferences, the block payloads against the blocks the dictionary encoders
and the chain encoders opened from the entry write when called directly, and every frame read back by LZ4F_decompress_usingDict and
by the reader with the set.  DESIGN.md 4.24."""
import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

import frame_dict_cases as FC
from k4os.compression.lz4_amd import LZ4Codec, LZ4Frame, LZ4EncoderSettings, LZ4Level, DictionarySet
from k4os.compression.lz4_amd import frames as F
from k4os.compression.lz4_amd.device import DeviceCodec
from k4os.compression.lz4_amd.encoders import LZ4Encoder

pytestmark = pytest.mark.gpu
LEVELS = (LZ4Level.L00_FAST, LZ4Level.L03_HC, LZ4Level.L09_HC)


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


@pytest.fixture(scope="module")
def E():
    return FC.entries()


@pytest.fixture(scope="module")
def dset(dc, E):
    with DictionarySet(E, owner=dc) as s:
        yield s


@pytest.fixture(scope="module")
def contents(E):
    """one block, two blocks and a bit, nothing, and bytes that do not shrink (stored raw)"""
    rng = np.random.default_rng(3)
    return [(0, FC.content_of(E[0], 40000, 1)), (6, FC.content_of(E[6], 2 * FC.K64 + 777, 2)), (9, FC.content_of(E[9], 70000, 3)),
            (0, b""), (5, rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()), (-1, FC.content_of(E[0], 50000, 4))]


def settings(chain, level, k):
    return LZ4EncoderSettings(ChainBlocks=chain, CompressionLevel=level, BlockChecksum=bool(k & 1), ContentChecksum=bool(k & 2))


def written(dc, dset, contents, s):
    return LZ4Frame.EncodeBatch([c for _, c in contents], s, ctx=dc.ctx, dictionary=(dset, FC.IDS), dict_index=[e for e, _ in contents])


def payloads(frame):
    info = F.parse_frame(frame)
    b = np.frombuffer(frame, np.uint8)
    return info, [(bool(l & 0x80000000), b[o:o + (l & 0x7FFFFFFF)].tobytes()) for o, l in zip(info.block_off, info.block_len)]


@pytest.mark.parametrize("level", LEVELS)
def test_independent_blocks_are_the_dictionary_encoders(dc, dset, contents, level):
    frames = written(dc, dset, contents, settings(False, level, int(level)))
    for (e, c), fr in zip(contents, frames):
        info, got = payloads(fr)
        assert info.descriptor.Dictionary == (FC.IDS[e] if e >= 0 else None) and not info.descriptor.Chaining
        if e < 0:
            assert fr == LZ4Frame.Encode(c, settings(False, level, int(level)))
            continue
        blocks = [c[p:p + FC.K64] for p in range(0, len(c), FC.K64)]
        direct = LZ4Codec.EncodeDictBatch(blocks, dset, [e] * len(blocks), level)
        want = [(True, b) if len(d) >= len(b) else (False, d) for b, d in zip(blocks, direct)]
        assert got == want, (e, len(c))
    assert any(raw for fr in frames for raw, _ in payloads(fr)[1])


@pytest.mark.parametrize("level", LEVELS)
def test_chained_blocks_are_a_chain_encoder_opened_from_the_entry(dc, dset, contents, level):
    frames = written(dc, dset, contents, settings(True, level, int(level) + 1))
    for (e, c), fr in zip(contents, frames):
        info, got = payloads(fr)
        assert info.descriptor.Dictionary == (FC.IDS[e] if e >= 0 else None) and info.descriptor.Chaining
        if e < 0:
            continue
        enc = LZ4Encoder.Create(True, level, FC.K64, 0, dc.ctx, dictionary=(dset, e))
        want, pos, target = [], 0, np.zeros(LZ4Codec.MaximumOutputSize(enc.BlockSize), np.uint8)
        while pos < len(c):
            pos += enc.Topup(c, pos)
            n = enc.Encode(target, allowCopy=True)
            want.append((n < 0, target[:abs(n)].tobytes()))
        assert got == want, (e, len(c))


@pytest.mark.parametrize("chain", [False, True])
def test_frames_read_back_by_liblz4_and_by_the_reader(dc, dset, contents, E, chain):
    for k, level in enumerate(LEVELS):
        s = settings(chain, level, k + 1)
        frames = written(dc, dset, contents, s)
        assert LZ4Frame.DecodeBatch(frames, ctx=dc.ctx, dictionary=(dset, FC.IDS)) == [c for _, c in contents]
        for (e, c), fr in zip(contents, frames):
            if e >= 0 and c:
                with pytest.raises(F.NotImplementedException):
                    LZ4Frame.Decode(fr)
            if FC.liblz4() is not None:
                assert FC.lz4f_decode(fr, E[e].tobytes() if e >= 0 else b"", len(c) + 64) == c, (e, level)
                if e >= 0:      # the header: liblz4's for the same preferences
                    ref = FC.lz4f_make([c], E[e].tobytes(), FC.IDS[e], chain, s.BlockChecksum, s.ContentChecksum, False)
                    assert fr[:11] == ref[:11], (e, level)                # magic, FLG, BD, DictID, header checksum


def test_content_length_and_single_encode(dc, dset, E):
    c = FC.content_of(E[0], 30000, 8)
    s = LZ4EncoderSettings(ContentLength=len(c), ContentChecksum=True)
    fr = LZ4Frame.Encode(c, s, dictionary=(dset, FC.IDS), dict_index=7)
    info = F.parse_frame(fr)
    assert info.descriptor.ContentLength == len(c) and info.descriptor.Dictionary == FC.IDS[7] and len(info.header) == 14
    assert LZ4Frame.Decode(fr, dictionary=(dset, FC.IDS)) == c
    if FC.liblz4() is not None:
        ref = FC.lz4f_make([c], E[7].tobytes(), FC.IDS[7], False, False, True, True)
        assert fr[:19] == ref[:19]                    # magic, FLG, BD, content size, DictID, header checksum


def test_writer_refusals(dc, dset):
    for level in (LZ4Level.L10_OPT, LZ4Level.L12_MAX):
        with pytest.raises(F.NotImplementedException):
            LZ4Frame.Encode(b"x" * 100, level=level, dictionary=(dset, FC.IDS), dict_index=0)
    with pytest.raises(ValueError):
        LZ4Frame.Encode(b"x" * 100, dictionary=(dset, FC.IDS), dict_index=len(FC.IDS))
    with pytest.raises(ValueError):
        LZ4Frame.EncodeBatch([b"x", b"y"], dictionary=(dset, FC.IDS), dict_index=[0])
    LZ4Codec.Enforce32 = True
    try:
        with pytest.raises(F.NotImplementedException):
            LZ4Frame.Encode(b"x" * 100, dictionary=(dset, FC.IDS), dict_index=0)
    finally:
        LZ4Codec.Enforce32 = False
