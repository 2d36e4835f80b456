"""Drivers for the single-object ILZ4Decoder (encoders.LZ4ChainDecoder, LZ4Decoder.Create, DecodeAndDrain) beside
chain_decoder_witness, shared by the emulator test and the GPU test: Decode with offset / length / blockSize, Inject,
DecodeAndDrain, Drain into a target offset, Peek and BytesReady after every call, a Decode that throws and continues, and Peek /
Drain at both ends of the legal range and one past each.  Test infrastructure only."""
import numpy as np
import pytest

import chain_decoder_cases as K
import chain_decoder_witness as W

K1, K64 = 1024, 65536


def both(lib_call, wit_call):
    """the two calls return the same, or the library raises InvalidOperationException where the witness raises its code"""
    from k4os.compression.lz4_amd.encoders import InvalidOperationException
    try:
        want = wit_call()
    except W.Code:
        with pytest.raises(InvalidOperationException):
            lib_call()
        return None
    got = lib_call()
    assert got == want
    return got


def held(d, w):
    """BytesReady, and everything the decoder holds through Peek and through Drain"""
    ready = w.bytes_ready
    assert d.BytesReady == ready
    assert d.Peek(-ready).tobytes() == w.peek(-ready)
    target = np.full(ready + 7, 0xCD, np.uint8)
    d.Drain(target, -ready, ready, 5)
    assert target[5:5 + ready].tobytes() == w.drain(-ready, ready) and (target[:5] == 0xCD).all() and (target[5 + ready:] == 0xCD).all()


def ends_of_the_range(d, w):
    ready = w.bytes_ready
    assert ready > 2
    for off in (0, -1, -ready, 1, -ready - 1):                                # Peek: LZ4ChainDecoder.cs:106-115
        both(lambda: d.Peek(off).tobytes(), lambda: w.peek(off))
    for off, n in ((0, 0), (-ready, ready), (-ready, 0), (-1, 1), (-2, 1),    # legal: both ends
                   (-ready - 1, 1), (-ready - 1, 0), (-1, 2), (0, 1), (1, 0), (-1, -1), (-ready, ready + 1)):   # one past each
        def lib():
            t = np.zeros(max(n, 0) + 3, np.uint8)
            d.Drain(t, off, n, 3)
            return t[3:3 + max(n, 0)].tobytes()
        both(lib, lambda: w.drain(off, n))


def chained_block_by_block(extra):
    from k4os.compression.lz4_amd.encoders import DecodeAndDrain, LZ4ChainDecoder, LZ4Decoder
    rng = np.random.default_rng(40 + extra)
    sizes = [60000] + [int(x) for x in rng.integers(2, K1 + 1, 40)]            # the ring of B = 1 KiB, extraBlocks = 0 wraps
    blocks = K.chain_blocks(K.content(sum(sizes), 40 + extra), sizes, K64, "fast" if extra else "hc")
    d, w = LZ4Decoder.Create(True, K1 - 5, extra), W.create(True, K1 - 5, extra)
    assert isinstance(d, LZ4ChainDecoder) and d.BlockSize == w.block_size == K1 and d.BytesReady == 0
    both(lambda: d.Peek(0).tobytes(), lambda: w.peek(0))
    both(lambda: d.Peek(-1).tobytes(), lambda: w.peek(-1))
    raw, _ = blocks[0]
    junk = b"\x11" * 9 + raw + b"\x22" * 4
    assert both(lambda: d.Inject(junk, 9, len(raw)), lambda: w.inject(raw)) == len(raw)
    held(d, w)
    for k, (raw, payload) in enumerate(blocks[1:]):
        n, kind = len(raw), k % 5
        if kind == 0:
            assert both(lambda: d.Decode(payload), lambda: w.decode(payload)) == n
        elif kind == 1:                                                         # a slice of a larger source, the exact decoded size
            src = np.frombuffer(b"\x33" * 7 + payload + b"\x44" * 5, np.uint8)
            assert both(lambda: d.Decode(src, 7, len(payload), n), lambda: w.decode(payload, n)) == n
        elif kind == 2:                                                         # one byte less throws, and the decoder continues
            assert both(lambda: d.Decode(payload, 0, None, n - 1), lambda: w.decode(payload, n - 1)) is None
            assert d.BytesReady == w.bytes_ready
            assert both(lambda: d.Decode(payload, blockSize=n), lambda: w.decode(payload, n)) == n
        elif kind == 3:                                                         # uncompressed yet chained
            assert both(lambda: d.Inject(raw), lambda: w.inject(raw)) == n
        else:
            short = k % 2 == 0                                                  # a target one byte short: false, the block stays
            target = np.full(n + (3 if not short else -1), 0xEE, np.uint8)
            ok, decoded = DecodeAndDrain(d, payload, target)
            w_ok, w_decoded, w_bytes = W.decode_and_drain(w, payload, target.size)
            assert (ok, decoded) == (w_ok, w_decoded) == (not short, n)
            assert (target[n:] == 0xEE).all() and (target.tobytes()[:n] == w_bytes == raw if ok else (target == 0xEE).all())
        held(d, w)
        assert d.Peek(-n).tobytes() == raw
    assert DecodeAndDrain(d, b"", np.zeros(8, np.uint8)) == (False, 0) and d.BytesReady == w.bytes_ready
    both(lambda: d.Inject(b"\x00" * (K64 + 1)), lambda: w.inject(b"\x00" * (K64 + 1)))      # longer than max(B, 64 KiB)
    both(lambda: d.Decode(blocks[1][1], blockSize=(1 + extra) * K1 + 33), lambda: w.decode(blocks[1][1], (1 + extra) * K1 + 33))
    held(d, w)
    ends_of_the_range(d, w)


def independent_variant():
    """LZ4ChainDecoder(chaining=False) is LZ4BlockDecoder in a device store; LZ4Decoder.Create(False, ...) gives the host class"""
    from oracle_lib import Oracle
    from k4os.compression.lz4_amd.encoders import DecodeAndDrain, LZ4BlockDecoder, LZ4ChainDecoder, LZ4Decoder
    assert isinstance(LZ4Decoder.Create(False, K1), LZ4BlockDecoder)
    o = Oracle()
    d, w = LZ4ChainDecoder(K1 + 1, 3, chaining=False), W.create(False, K1 + 1)
    assert d.BlockSize == w.block_size == 2 * K1 and d.BytesReady == 0
    for k, n in enumerate((700, 2 * K1, 2 * K1 + 8, 2 * K1 + 9, 1)):           # within B, B, the capacity B + 8, one past it
        raw = K.content(n, 60 + k)
        payload = bytes(o.encode(raw, 0))
        if both(lambda: d.Decode(payload), lambda: w.decode(payload)) is not None:
            held(d, w)                                                          # after a throw the held bytes are nobody's
    both(lambda: d.Decode(payload, blockSize=2 * K1 + 1), lambda: w.decode(payload, 2 * K1 + 1))   # above B: the reference's exception
    both(lambda: d.Decode(b""), lambda: w.decode(b""))
    raw = K.content(900, 70).tobytes()
    assert both(lambda: d.Inject(raw), lambda: w.inject(raw)) == 900
    held(d, w)
    ends_of_the_range(d, w)
    target = np.zeros(K1, np.uint8)
    payload = bytes(o.encode(K.content(333, 71), 0))
    assert DecodeAndDrain(d, payload, target)[:2] == W.decode_and_drain(w, payload, K1)[:2] == (True, 333)
    both(lambda: d.Inject(b"\x00" * (2 * K1 + 9)), lambda: w.inject(b"\x00" * (2 * K1 + 9)))
    assert both(lambda: d.Inject(b""), lambda: w.inject(b"")) == 0 and d.BytesReady == w.bytes_ready == 0
