"""The single-object ILZ4Decoder (encoders.LZ4ChainDecoder, LZ4Decoder.Create, DecodeAndDrain) with the kernels under
the host wave emulator in place of the device: the class's own logic -- slices, codes to exceptions, Drain's target offset, Peek --
driven call by call beside chain_decoder_witness (chain_decoder_object.py)."""
import pytest

import chain_decoder_emu as E
import chain_decoder_object as O


class EmuBatch:
    """what LZ4ChainDecoder asks of LZ4ChainDecoderBatch, over chain_decoder_emu.EmuDecoders"""

    def __init__(self, settings, ctx=None):
        self.e = E.EmuDecoders(settings)
        self.n, self.records = self.e.n, self.e.recs
        self.Run, self.Drain, self.Query, self.Reset = self.e.run, self.e.drain, self.e.query, self.e.reset


@pytest.fixture(autouse=True)
def emulated(monkeypatch):
    from k4os.compression.lz4_amd import encoders
    monkeypatch.setattr(encoders, "LZ4ChainDecoderBatch", EmuBatch)


@pytest.mark.parametrize("extra", [0, 2])
def test_create_chained_driven_block_by_block(extra):
    O.chained_block_by_block(extra)


def test_the_independent_variant():
    O.independent_variant()
