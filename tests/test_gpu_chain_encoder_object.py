"""The LZ4Encoder.Create object on the GPU, call by call beside the witness, for all three kinds: Topup and Encode
as separate calls, TopupAndEncode / FlushAndEncode over it, BytesReady and BlockSize after every call."""
import numpy as np
import pytest

import chain_encoder_cases as CC
from chain_encoder_witness import WitnessEncoder

pytestmark = pytest.mark.gpu
K1 = 1024


@pytest.mark.parametrize("chaining,level,bs,extra", [(False, 0, 2000, 0), (True, 0, 2 * K1, 1), (True, 9, 3 * K1, 0)])
def test_object_follows_the_witness(chaining, level, bs, extra):
    from k4os.compression.lz4_amd import LZ4Encoder, TopupAndEncode, FlushAndEncode, EncoderAction
    rng = np.random.default_rng(level + bs)
    enc = LZ4Encoder.Create(chaining, level, bs, extra)
    w = WitnessEncoder(chaining, level, bs, extra)
    B = enc.BlockSize
    assert B == w.enc.block_size
    data = np.concatenate([CC.content(60 * K1, 5), CC.content(4 * K1, 6, "random"), CC.content(60 * K1, 7)])
    target = np.zeros(B + B // 255 + 16, np.uint8)
    pos = 0
    while pos < data.size:
        piece = data[pos:pos + int(rng.integers(1, 2 * B))]
        how = int(rng.integers(0, 3))
        allow = bool(rng.integers(0, 2))
        if how == 0:                                         # Topup, then now and then Encode
            took = enc.Topup(piece)
            assert took == w.enc.topup(piece, 0, piece.size)
            pos += took
            if enc.BytesReady == B or rng.random() < 0.3:
                we, wd = w.enc.encode(allow)
                got = enc.Encode(target, allowCopy=allow)
                assert got == we and target[:abs(got)].tobytes() == wd
        else:
            force = how == 2
            wl, we, wd = w.topup_and_encode(piece, force, allow)
            action, loaded, encoded = TopupAndEncode(enc, piece, target, force, allow)
            assert (loaded, encoded) == (wl, abs(we) if allow else we) and target[:abs(we)].tobytes() == wd
            assert action == (EncoderAction.Copied if we < 0 else EncoderAction.Encoded if we else EncoderAction.Loaded if wl else EncoderAction.None_)
            pos += loaded
        assert enc.BytesReady == w.enc.bytes_ready
    action, encoded = FlushAndEncode(enc, target)
    we, wd = w.enc.encode(True)
    assert encoded == abs(we) and target[:encoded].tobytes() == wd
    assert enc.Encode(target) == 0 and enc.BytesReady == 0
    # a target below the bound: the reference's exception, and the block is still there for a larger target
    piece = data[:100]
    assert enc.Topup(piece) == w.enc.topup(piece, 0, 100)
    from k4os.compression.lz4_amd import InvalidOperationException
    with pytest.raises(InvalidOperationException):
        enc.Encode(target, length=50)
    assert enc.BytesReady == 100
    we, wd = w.enc.encode(False)
    assert enc.Encode(target) == we and target[:we].tobytes() == wd
    w.close()
