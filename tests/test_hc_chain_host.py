"""Chained HC streams on the host side (no GPU): the block-table model that k4lz4_encode_hc_chain_batch builds
(encoders.hc_chain_blocks) against a literal transcription of LZ4EncoderBase's ring buffer over the stream context's
indices (LL.high.cs), the liblz4 witness round-tripping through LZ4_decompress_safe_usingDict chaining, and the
refusal of streams that reach the encoder's 2 GB renormalisation."""
import ctypes as C

import numpy as np
import pytest

import hc_chain_witness as W
from k4os.compression.lz4_amd import _native, corpus
from k4os.compression.lz4_amd.encoders import hc_chain_blocks, LZ4HighChainEncoder


@pytest.mark.parametrize("extra", [0, 1, 2, 3])
def test_block_table_model_matches_ring_buffer_transcription(extra):
    sizes = [1, 1000, 1024, 1025, 1500, 3000, 4096, 65535, 65536, 65537, 100000, 262144, 1 << 20]
    lengths = [0, 1, 4, 12, 13, 1023, 1024, 1025, 65536, 65537, 131072, 200001, 700000, 1 << 20, (1 << 20) + 13]
    for B in sizes:
        Br = (max(B, 1024) + 1023) // 1024 * 1024
        for N in lengths + [3 * Br, 7 * Br, 70 * Br]:
            got = hc_chain_blocks(N, B, extra)
            assert got == W.witness_table(N, B, extra), (N, B, extra)
            assert sum(n for _, n, _ in got) == N and all(n == Br for _, n, _ in got[:-1])


def test_block_table_model_saves_every_65_blocks_of_1kib():
    t = hc_chain_blocks(300 * 1024, 1024, 0)
    saves = [k for k in range(1, len(t)) if t[k][2] != t[k - 1][2]]
    assert saves == list(range(65, len(t)))              # 65 KiB fill the ring buffer, then every block is followed by a save
    for s, n, dl in t:                                    # the window [max(dl, s - 64 KiB), s + n) never starts before dictLimit
        assert dl <= max(0, s - 65536)


def test_block_table_model_continuation_is_the_ring_buffer():
    # a stream continued with dictLen = what the ring buffer holds gives the blocks the whole stream gives from there on
    N, B, e = 900000, 4096, 1
    whole = hc_chain_blocks(N, B, e)
    for k in (1, 17, 40, 100):
        s, _, dl = whole[k]
        part = hc_chain_blocks(N - dl, B, e, dictLen=s - dl)
        assert [(a + dl, b, c + dl) for a, b, c in part] == whole[k:]


@pytest.fixture(scope="module")
def lz4():
    try:
        return W.Lz4HcCodec.lib()
    except OSError:
        pytest.skip("liblz4.so.1 not present")


@pytest.mark.parametrize("level", [3, 9, 12])
def test_witness_round_trips_through_chained_decoding(lz4, level):
    contents = [corpus.class_bytes("dickens", 300000, 1), corpus.random_bytes(70000, 2), corpus.lorem(5), np.zeros(0, np.uint8),
                corpus.repeated(7, 200000)]
    for data in contents:
        for B, e in ((1024, 0), (65536, 0), (65536, 2), (262144, 1)):
            blocks = W.witness_blocks(data, level, B, e)
            assert W.decode_chain(blocks, (B + 1023) // 1024 * 1024) == data.tobytes()
            assert all(abs(n) == len(p) for n, p in blocks)


def test_witness_blocks_use_their_history(lz4):
    # random bytes with a period of 50 000: the second block is long matches into the first (a chained stream), not a copy
    part = corpus.random_bytes(50000, 9)
    blocks = W.witness_blocks(np.concatenate([part, part, part]), 9, 65536)
    assert 0 < blocks[1][0] < 400 and 0 < blocks[2][0] < 400


def test_streams_reaching_2gb_are_refused():
    # LZ4_compressHC_continue_generic renormalises a block that starts where end - base > 2 GB, base 64 KiB before the stream
    lib = _native.load_library()
    buf = np.zeros(16, np.uint8)
    off = np.zeros(1, np.uint64)
    bs, ex = np.array([1024], np.int32), np.zeros(1, np.int32)
    dst, out = np.zeros(16, np.uint8), np.zeros(1 << 21, np.int32)
    limit = (1 << 31) - 65536
    for n, refused in ((limit + 1, False), (limit + 1025, True), ((1 << 31) + 5, True)):
        ln = np.array([n], np.int64)
        rc = lib.k4lz4_encode_hc_chain_batch(None, buf.ctypes.data, off.ctypes.data, ln.ctypes.data, bs.ctypes.data, ex.ctypes.data, None,
                                             1, dst.ctypes.data, off.ctypes.data, out.ctypes.data, out.size, 9, 0)
        # (the block table is host arithmetic and is checked before the context: a stream that passes it fails on ctx = NULL)
        assert rc == _native.E_ARG
        assert (b"2 GB" in lib.k4lz4_last_error(None)) == refused, n
        assert (hc_chain_blocks(n, 1024)[-1][0] > limit) == refused


def test_chain_encoder_mirror_surface():
    enc = LZ4HighChainEncoder(1, 1500, -2)                  # level clamped to L03_HC, block size to a whole KiB, extra to 0
    assert enc.BlockSize == 2048 and int(enc._level) == 3 and enc.BytesReady == 0
    assert enc.Topup(np.arange(5000, dtype=np.uint8) % 7) == 2048 and enc.BytesReady == 2048
    assert enc.Topup(np.zeros(10, np.uint8)) == 0


def test_library_exports_the_chain_entry_points():
    import ctypes as C
    raw = C.CDLL(_native.LIB_PATH)
    for name in ("k4lz4_encode_hc_chain_batch", "k4lz4_encode_hc_chain_batch_device"):
        assert name in _native.SYMBOLS and getattr(raw, name) is not None
