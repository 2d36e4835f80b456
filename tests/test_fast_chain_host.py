"""Chained fast streams on the host side (no GPU): the block-table model k4lz4_encode_fast_chain_batch builds
(encoders.fast_chain_blocks) against a transcription of LZ4EncoderBase's ring buffer over the stream context's fields
(LL64.fast.cs:582-667, LL.tools.cs:195-213), the liblz4 witness round-tripping through LZ4_decompress_safe_usingDict chaining,
the 2 GB and 32-bit refusals, and the kernel itself (k4lz4_fast_chain.hpp) under the host wave emulator against the witness."""
import numpy as np
import pytest

import fast_chain_witness as W
import hc_chain_witness as HW
from k4os.compression.lz4_amd import _native, corpus, LZ4Codec
from k4os.compression.lz4_amd.encoders import fast_chain_blocks, LZ4FastChainEncoder, FAST_CHAIN_STATE, encode_fast_chain_packed

KI = 1024


@pytest.mark.parametrize("extra", [0, 1, 2, 3])
def test_block_table_model_matches_ring_buffer_transcription(extra):
    sizes = [1, 1000, 1024, 1025, 1500, 3000, 4096, 65535, 65536, 65537, 100000, 262144, 1 << 20]
    lengths = [0, 1, 4, 12, 13, 1023, 1024, 1025, 65536, 65537, 131072, 200001, 700000, 1 << 20, (1 << 20) + 13]
    for B in sizes:
        Br = (max(B, 1024) + 1023) // 1024 * 1024
        for N in lengths + [3 * Br, 7 * Br, 70 * Br]:
            got = fast_chain_blocks(N, B, extra)
            t = W.witness_table(N, B, extra)
            assert got == t.blocks, (N, B, extra)
            # the arms: a fresh stream's first call takes usingExtDict (empty dictionary), every later one withPrefix64k
            assert t.arms == ["usingExtDict"] * min(1, len(t.arms)) + ["withPrefix64k"] * (len(t.arms) - 1)
            # dictSize is always the ring's _inputIndex, and never small within a stream from its start
            assert [d for _, _, d, _ in got] == t.ring_index and not any(sm for *_, sm in got)


def test_block_table_model_saves_every_65_blocks_of_1kib():
    t = fast_chain_blocks(300 * KI, KI, 0)
    saves = [k for k in range(1, len(t)) if t[k][2] != t[k - 1][2] + t[k - 1][1]]
    assert saves == list(range(65, len(t)))
    assert all(d == 65536 for _, _, d, _ in t[65:])


def test_block_table_model_continuation_and_dict_small():
    N, B, e = 900000, 4096, 1
    whole = fast_chain_blocks(N, B, e)
    for k in (1, 17, 40, 100):
        s, _, d, _ = whole[k]
        part = fast_chain_blocks(N - s + d, B, e, dictLen=d, currentOffset=s)
        assert [(a + s - d, b, c, sm) for a, b, c, sm in part] == whole[k:]
    # a continued stream whose dictionary is shorter than what it has consumed (and below 64 KiB): dictSmall
    assert fast_chain_blocks(5000, 4096, 0, dictLen=1000, currentOffset=70000)[0] == (1000, 4000, 1000, True)


@pytest.fixture(scope="module")
def lz4():
    try:
        lib = W.Lz4FastChainCodec.lib()
    except OSError:
        pytest.skip("liblz4.so.1 not present")
    W.check_layout()
    return lib


def test_witness_round_trips_through_chained_decoding(lz4):
    contents = [corpus.class_bytes("dickens", 300000, 1), corpus.random_bytes(70000, 2), corpus.lorem(5), np.zeros(0, np.uint8),
                corpus.repeated(7, 200000)]
    for data in contents:
        for B, e in ((1024, 0), (65536, 0), (65536, 2), (262144, 1)):
            blocks, st = W.witness_stream(data, B, e)
            assert HW.decode_chain(blocks, (B + 1023) // 1024 * 1024) == data.tobytes()
            assert st["currentOffset"] == data.size


def test_first_chained_block_is_not_the_independent_encoders(lz4):
    # byU32 + hash5 from the first block on: a 64 KiB block of text differs from LZ4Codec.Encode's byU16 / hash4 bytes
    data = corpus.class_bytes("dickens", 65536, 3)
    blocks, _ = W.witness_stream(data, 65536)
    ref = HW.Lz4HcCodec.lib()
    import ctypes as C
    ref.LZ4_compress_default.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    dst = np.zeros(70000, np.uint8)
    n = ref.LZ4_compress_default(data.ctypes.data, dst.ctypes.data, data.size, dst.size)
    assert blocks[0][1] != dst[:n].tobytes()


def test_streams_reaching_2gb_are_refused():
    lib = _native.load_library()
    buf = np.zeros(16, np.uint8)
    off = np.zeros(1, np.uint64)
    bs, ex = np.array([1024], np.int32), np.zeros(1, np.int32)
    dst, out = np.zeros(16, np.uint8), np.zeros(1 << 22, np.int32)
    for n, refused in (((1 << 31), False), ((1 << 31) + 1, True)):
        ln = np.array([n], np.int64)
        rc = lib.k4lz4_encode_fast_chain_batch(None, buf.ctypes.data, off.ctypes.data, ln.ctypes.data, bs.ctypes.data, ex.ctypes.data, None, 1,
                                               None, None, dst.ctypes.data, off.ctypes.data, out.ctypes.data, out.size, 0)
        assert rc == _native.E_ARG                        # (the table is checked before the context: one that passes fails on ctx = NULL)
        assert (b"2 GB" in lib.k4lz4_last_error(None)) == refused, n
    # through a state: currentOffset close to the limit
    st = np.zeros(1, FAST_CHAIN_STATE)
    st["currentOffset"] = (1 << 31) - 1000
    ln = np.array([2000], np.int64)
    rc = lib.k4lz4_encode_fast_chain_batch(None, buf.ctypes.data, off.ctypes.data, ln.ctypes.data, bs.ctypes.data, ex.ctypes.data, None, 1,
                                           st.ctypes.data, None, dst.ctypes.data, off.ctypes.data, out.ctypes.data, out.size, 0)
    assert rc == _native.E_ARG and b"2 GB" in lib.k4lz4_last_error(None)
    with pytest.raises(NotImplementedError):
        fast_chain_blocks((1 << 31) + 1, 65536)


def test_x32_and_argument_refusals():
    lib = _native.load_library()
    buf = np.zeros(16, np.uint8)
    off = np.zeros(1, np.uint64)
    bs, ex = np.array([1024], np.int32), np.zeros(1, np.int32)
    dst, out = np.zeros(16, np.uint8), np.zeros(4, np.int32)
    ln = np.array([10], np.int64)
    args = lambda dl, st, flags: (None, buf.ctypes.data, off.ctypes.data, ln.ctypes.data, bs.ctypes.data, ex.ctypes.data, dl, 1, st, None,
                                  dst.ctypes.data, off.ctypes.data, out.ctypes.data, out.size, flags)
    assert lib.k4lz4_encode_fast_chain_batch(*args(None, None, _native.FLAG_X32)) == _native.E_ARG
    assert b"32-bit" in lib.k4lz4_last_error(None)
    assert lib.k4lz4_encode_fast_chain_batch(*args(None, None, _native.FLAG_NO_REORDER)) == _native.E_ARG
    dl = np.array([4], np.int32)
    assert lib.k4lz4_encode_fast_chain_batch(*args(dl.ctypes.data, None, 0)) == _native.E_ARG      # dictLen without a state
    st = np.zeros(1, FAST_CHAIN_STATE)
    st["currentOffset"], st["dictSize"] = 100, 5
    assert lib.k4lz4_encode_fast_chain_batch(*args(dl.ctypes.data, st.ctypes.data, 0)) == _native.E_ARG   # dictLen != dictSize
    assert b"dictSize" in lib.k4lz4_last_error(None)
    old = LZ4Codec.Enforce32
    try:
        LZ4Codec.Enforce32 = True
        with pytest.raises(NotImplementedError):
            encode_fast_chain_packed([np.zeros(100, np.uint8)], 1024)
        enc = LZ4FastChainEncoder(1024)
        enc.Topup(np.zeros(100, np.uint8))
        with pytest.raises(NotImplementedError):
            enc.Encode(np.zeros(2000, np.uint8), allowCopy=True)
    finally:
        LZ4Codec.Enforce32 = old


def test_fast_chain_encoder_mirror_surface():
    enc = LZ4FastChainEncoder(1500, -2)                       # block size to a whole KiB, extra to 0
    assert enc.BlockSize == 2048 and enc.BytesReady == 0 and enc.State["currentOffset"][0] == 0
    assert enc.Topup(np.arange(5000, dtype=np.uint8) % 7) == 2048 and enc.BytesReady == 2048
    assert enc.Topup(np.zeros(10, np.uint8)) == 0


def test_library_exports_the_fast_chain_entry_points():
    import ctypes as C
    raw = C.CDLL(_native.LIB_PATH)
    for name in ("k4lz4_encode_fast_chain_batch", "k4lz4_encode_fast_chain_batch_device"):
        assert name in _native.SYMBOLS and getattr(raw, name) is not None


# ---- the kernel under the host wave emulator ----------------------------------------------------------------------------------------
def _emu_streams():
    rng = np.random.default_rng(5)
    text = corpus.class_bytes("dickens", 400000, 1)
    reach = corpus.random_bytes(140000, 4).copy()
    reach[131072 - 100:131072 + 200] = reach[131072 - 100 - 65535:131072 + 200 - 65535]
    runs = np.concatenate([np.tile(rng.integers(0, 256, [1, 2, 4][k % 3], dtype=np.uint8), 700) for k in range(30)] +
                          [rng.integers(0, 256, 300, dtype=np.uint8)])
    return [text, text[:100000], corpus.class_bytes("mozilla", 150000, 2), corpus.class_bytes("xml", 90000, 3), corpus.random_bytes(30000, 6),
            np.zeros(80000, np.uint8), corpus.lorem(4)[:20000], reach, runs, np.zeros(0, np.uint8), text[:12], text[:13], text[:5000],
            corpus.repeated(9, 70000)]


@pytest.mark.parametrize("block_size,extra", [(1024, 0), (4096, 3), (65536, 0), (65536, 1), (262144, 0)])
def test_emulated_kernel_equals_witness(lz4, block_size, extra):
    import fast_chain_emu as E
    streams = _emu_streams()
    for allow_copy in (True, False):
        got, st = E.encode(streams, block_size, extra, allow_copy)
        for s, data in enumerate(streams):
            want, wst = W.witness_stream(data, block_size, extra, allow_copy)
            assert got[s] == want, (s, block_size, extra)
            assert np.array_equal(st["hashTable"][s], wst["hashTable"]), s
            assert int(st["currentOffset"][s]) == wst["currentOffset"] and int(st["dictSize"][s]) == wst["dictSize"], s


def test_emulated_kernel_continues_from_a_state(lz4):
    # a stream cut in two calls: the second starts from the first's state with the ring's bytes in front = the whole stream's blocks
    import fast_chain_emu as E
    data = corpus.class_bytes("dickens", 300000, 7)
    B = 4096
    want, wst = W.witness_stream(data, B, 0, True)
    t = fast_chain_blocks(data.size, B)
    k = 40
    s, _, d, _ = t[k]
    first, st1 = E.encode([data[:s]], B, 0, True)
    second, st2 = E.encode([data[s - d:]], B, 0, True, state_in=st1)
    assert int(st1["dictSize"][0]) == d
    assert first[0] + second[0] == want
    assert np.array_equal(st2["hashTable"][0], wst["hashTable"]) and int(st2["currentOffset"][0]) == data.size
