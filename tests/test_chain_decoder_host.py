"""Many open ILZ4Decoders (k4lz4_chain_decode_batch), what can be checked without a GPU: the witness against
whole-stream decoding and the content, the pin the kernel rests on (the prefix is the ring's bytes before the index, the last
64 KiB of them) extended to Inject and extraBlocks > 0, the host arithmetic of init / store_bytes, and the exported symbols."""
import ctypes as C

import numpy as np
import pytest

import chain_decoder_cases as K
import chain_decoder_witness as W
import hc_chain_witness as HW
from k4os.compression.lz4_amd import _native, encoders as E

K1, K64 = 1024, 65536


def test_witness_decodes_chained_streams_to_their_content():
    """block by block through the witness == hc_chain_witness.decode_chain on the stream whole == the content"""
    rng = np.random.default_rng(5)
    for B, extra, kind, n in ((K1, 0, "fast", 150), (K1, 3, "hc", 150), (K64, 0, "fast", 5), (K64, 2, "hc", 5)):
        sizes = [int(x) for x in rng.integers(1, B + 1, n)]
        data = K.content(sum(sizes), B + extra)
        blocks = K.chain_blocks(data, sizes, B, kind)
        d = W.create(True, B, extra)
        out = bytearray()
        for raw, p in blocks:
            ok, got, b = W.decode_and_drain(d, p, B)
            assert ok and got == len(raw)
            out += b
        assert bytes(out) == data.tobytes() == HW.decode_chain([(len(p), p) for _, p in blocks], B)
        assert d.bytes_ready <= d.output_length


def test_small_ring_moves_overlap_at_every_residue():
    """the case list's B = 1 KiB streams: the index passes 64 KiB + 32 at odd positions and Prepare moves the history down over
    itself by distances of every residue the copy widths care about"""
    _, settings, calls = K.case(0)
    moves = []

    class Traced(W.ChainDecoder):
        def _copy_dict(self, index):
            if index > K64:
                moves.append(index - K64)
            return W.ChainDecoder._copy_dict(self, index)
    w = W.WitnessDecoders(settings)
    w.d = [Traced(b, e) for _, b, e in settings]
    K.play(w, calls)
    assert len(moves) > 100 and all(0 < m < K64 for m in moves)          # source and destination overlap
    assert any(m % 2 for m in moves) and any(m % 4 == 2 for m in moves) and any(m % 8 == 4 for m in moves)
    assert any(m % 16 == 8 for m in moves) and any(m % 16 == 0 for m in moves)
    assert any((K64 + m) % 2 for m in moves)                             # ... at odd byte positions


def test_prefix_is_the_rings_last_64k_after_every_operation():
    """test_frame_reader_host's pin for Decode alone, extended to Inject's three paths, extraBlocks > 0, per-record block sizes and
    calls that throw: the context's prefix is the ring's bytes before the index, the last min(total, 64 KiB) bytes of the stream"""
    rng = np.random.default_rng(7)
    for B, extra in ((K1, 0), (K1, 2), (K64, 0), (K64, 1), (256 << 10, 0)):
        d = W.create(True, B, extra)
        sizes = [int(rng.choice([1, 100, B // 2 + 1, B])) for _ in range(400 if B == K1 else 70)]
        data = K.content(sum(sizes), B + extra)
        blocks = K.chain_blocks(data, sizes, max(B, K64))
        seen = bytearray()
        paths = set()
        for raw, p in blocks:
            if rng.random() < 0.15:
                with pytest.raises(W.Code):
                    d.decode(b"\xff\xff\x00")                            # throws behind Prepare: the move stays
            if rng.random() < 0.4:
                paths.add(1 if d.output_index + len(raw) < d.output_length else 2 if len(raw) >= K64 else 3)
                assert d.inject(raw) == len(raw)
                seen += raw
            else:
                assert d.decode(p, len(raw) if rng.random() < 0.5 else 0) == len(raw)
                seen += raw
            n = min(len(seen), K64)
            assert d.output_index >= n and d.prefix_end == d.base + d.output_index and min(d.prefix_size, K64) == n
            assert d.prefix() == d.peek(-n) == bytes(seen[len(seen) - n:])
        assert {1, 3} <= paths or B > K1


def test_decode_and_drain_and_the_state_after_a_throw():
    blocks = K.chain_blocks(K.content(3000, 9), [1000, 1000, 1000], K1)
    d = W.create(True, K1)
    assert W.decode_and_drain(d, b"", 100) == (False, 0, b"") and d.bytes_ready == 0
    assert W.decode_and_drain(d, blocks[0][1], 1000) == (True, 1000, blocks[0][0])
    assert W.decode_and_drain(d, blocks[1][1], 999) == (False, 1000, b"") and d.bytes_ready == 2000      # decoded, not drained
    assert d.drain(-1000, 1000) == blocks[1][0]
    with pytest.raises(W.Code) as e:
        d.decode(blocks[2][1], 999)
    assert e.value.code == W.DECODE and d.bytes_ready == 2000
    assert d.decode(blocks[2][1], 1000) == 1000 and d.drain(-3000, 3000) == b"".join(b[0] for b in blocks)
    for off, n in ((-3001, 1), (0, 1), (-1, 2), (-1, -1), (1, 0)):
        with pytest.raises(W.Code):
            d.drain(off, n)
    with pytest.raises(W.Code):
        d.peek(1)
    assert d.peek(0) == b"" and d.peek(-2) == blocks[2][0][-2:]


def test_case_list_is_what_the_issue_asks_for():
    ids = K.case_ids()
    assert len(ids) == len(set(ids)) == len(K.BUILDERS)
    _, settings, calls = K.case(ids.index("small_ring"))
    assert settings == [(1, K1, 0)] * 3 and min(sum(len(c[1][i]) for c in calls) for i in range(3)) >= 80
    _, settings, calls = K.case(ids.index("b4m"))
    assert settings == [(1, 4 << 20, 0)] and sum(len(c[1][0]) for c in calls) == 3
    name, settings, calls = K.case(ids.index("issue64"))
    w = W.WitnessDecoders(settings)
    t = K.play(w, calls)
    assert t[0][3][0] == K.issue64_records()[1]
    settings, calls = K.mutants()
    assert len(settings) == K.N_MUTANTS == 300


class _Record(C.Structure):
    _fields_ = [("blockSize", C.c_int32), ("extraBlocks", C.c_int32), ("chaining", C.c_int32), ("reserved", C.c_int32),
                ("storeBytes", C.c_int64)]


class _Settings(C.Structure):
    _fields_ = [("blockSize", C.c_int32), ("extraBlocks", C.c_int32), ("chaining", C.c_int32)]


def test_init_and_store_bytes_arithmetic():
    """host arithmetic, no device: the rounding and the ring's length are the reference's (LZ4ChainDecoder.cs:28-32,
    LZ4BlockDecoder.cs:25-27)"""
    lib = _native.load_library()
    for bs, extra, chaining in ((0, 0, 1), (1, 0, 1), (1024, 0, 1), (1025, 0, 1), (65536, 0, 1), (65536, 2, 1), (4 << 20, 0, 1), (100000, -3, 1),
                                (0, 0, 0), (1025, 7, 0), (65536, 0, 0)):
        rec = _Record()
        assert lib.k4lz4_chain_decoder_init(C.byref(rec), C.byref(_Settings(bs, extra, chaining))) == 0
        B = (max(bs, K1) + K1 - 1) // K1 * K1
        ring = K64 + (1 + max(extra, 0)) * B + 32 if chaining else B + 8
        w = W.create(chaining, bs, extra)
        assert (rec.blockSize, rec.chaining) == (B, chaining) == (w.block_size, w.chaining) and ring == w.output_length
        assert rec.extraBlocks == (max(extra, 0) if chaining else 0)
        assert rec.storeBytes == lib.k4lz4_chain_decoder_store_bytes(C.byref(rec)) == 256 + (ring + 64 + 255) // 256 * 256
        assert rec.storeBytes % 256 == 0 and rec.storeBytes >= 256 + ring + 8
    rec = _Record()
    assert lib.k4lz4_chain_decoder_init(C.byref(rec), None) == 0 and (rec.blockSize, rec.chaining) == (K1, 0)
    assert lib.k4lz4_chain_decoder_init(None, None) == _native.E_ARG
    assert lib.k4lz4_chain_decoder_init(C.byref(rec), C.byref(_Settings(0x7E000000, 0, 1))) == _native.E_ARG
    assert lib.k4lz4_chain_decoder_init(C.byref(rec), C.byref(_Settings(1 << 20, 1 << 12, 1))) == _native.E_ARG
    assert lib.k4lz4_chain_decoder_store_bytes(None) == 0


def test_abi_symbols_and_python_surface():
    lib = _native.load_library()
    for sym in ("k4lz4_chain_decoder_init", "k4lz4_chain_decoder_store_bytes", "k4lz4_chain_decode_batch", "k4lz4_chain_decode_batch_device",
                "k4lz4_chain_drain_batch", "k4lz4_chain_drain_batch_device", "k4lz4_chain_decoder_query", "k4lz4_chain_decoder_query_device"):
        assert sym in _native.SYMBOLS and getattr(lib, sym)
    assert (E.CDEC_RUN, E.CDEC_RESET, E.CDEC_DRAIN, E.CDQ_WORDS) == (0, 1, 1, W.CDQ_WORDS)
    assert (E.CDEC_DECODE, E.CDEC_INJECT, E.CDEC_BLOCK_SIZE, E.CDEC_TARGET, E.CDEC_NOT_RUN, E.CDEC_RANGE, E.CDEC_NO_DECODER) == \
        (W.DECODE, W.INJECT, W.BLOCK_SIZE, W.TARGET, W.NOT_RUN, W.RANGE, W.NO_DECODER)
    rec = E.chain_decoder_record(True, 1000, 2, lib)
    assert (rec.blockSize, rec.extraBlocks, rec.chaining) == (1024, 2, 1)
    assert C.sizeof(E.ChainDecoderRecord) == 24
    assert E.LZ4Decoder.Create and E.LZ4ChainDecoder and E.LZ4ChainDecoderBatch
    assert "Chained *decoding* is frames.py's" not in E.__doc__ and "LZ4ChainDecoder" in E.__doc__
