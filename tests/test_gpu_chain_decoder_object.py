"""The single-object ILZ4Decoder on the GPU (encoders.LZ4ChainDecoder, LZ4Decoder.Create, DecodeAndDrain) driven
call by call beside chain_decoder_witness (chain_decoder_object.py)."""
import pytest

import chain_decoder_object as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("extra", [0, 2])
def test_create_chained_driven_block_by_block(extra):
    O.chained_block_by_block(extra)


def test_the_independent_variant_on_the_device():
    O.independent_variant()
