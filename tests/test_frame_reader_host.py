"""The incremental frame reader without a GPU: the witness (frame_reader_witness.py: LZ4FrameReader over LZ4BlockDecoder /
LZ4ChainDecoder, the reference's compiled engine) against the whole-frame reader's transcription and the content, the reference's
corner cases pinned one by one, and the C ABI's symbols and sizes."""
import ctypes as C

import numpy as np
import pytest

import frame_reader_cases as K
import frame_stream_reader as R
from frame_reader_witness import WitnessReader, ChainDecoder, BlockDecoder, engine
from test_frame_layer import LZ4F
from k4os.compression.lz4_amd import _native
from k4os.compression.lz4_amd import frames as F

K64 = 65536


@pytest.fixture(scope="module")
def sources():
    return K.valid_sources(LZ4F())


def test_one_read_equals_the_whole_frame_reader(sources):
    for name, src, content in sources:
        w = WitnessReader(src)
        got = b""
        for _ in range(8):                       # one read per frame (a read ends at the EndMark), then the clean end
            r = w.read(len(content) + 100)
            assert not isinstance(r, int), (name, r)
            got += r
        assert got == content and w.read(10) == b"" and w.bytes_read == len(content), name
        if name.startswith(("indep", "irregular", "linked-b", "linked-raw", "empty")) and name != "empty-first":
            code, whole = R.read_frame(src)
            assert code == 0 and whole == content, name


def test_random_partitions_concatenate_to_the_content(sources):
    rng = np.random.default_rng(11)
    for name, src, content in sources:
        for interactive in (False, True):
            w = WitnessReader(src)
            got, idle = b"", 0
            while idle < 4:
                r = w.read(int(rng.choice([1, 7, 4096, K64 - 1, K64, K64 + 1, 300_000])), interactive)
                assert not isinstance(r, int), (name, r)
                idle = idle + 1 if not r else 0
                got += r
            assert got == content, (name, interactive)


def _q(name):
    return dict(K.quirk_sources())[name]


def test_exact_end_read_then_the_defect_at_the_next_read():
    for name, code in (("bad-content-sum", -8), ("no-endmark", -1), ("half-endmark", -1)):
        w = WitnessReader(_q(name))
        assert len(w.read(2 * K64)) == 2 * K64 and w.failed is None, name      # satisfied at the block's end: the next word is not read
        assert w.read(1) == code and w.read(1) == code, name


def test_blocks_of_nothing():
    w = WitnessReader(_q("raw0-indep"))
    assert len(w.read(3 * K64)) == K64 and w.phase == 1           # the 0-length raw block ends the read, the frame stays open
    assert len(w.read(3 * K64)) == K64 and w.read(5) == b"" and w.phase == 0
    w = WitnessReader(_q("raw0-chain"))
    assert [len(w.read(3 * K64)) for _ in range(3)] == [K64, K64, 0] and w.phase == 0
    w = WitnessReader(_q("empty-block-chain"))
    assert [len(w.read(3 * K64)) for _ in range(3)] == [K64, K64, 0] and w.failed is None
    w = WitnessReader(_q("empty-block-indep"))                    # LZ4Codec.Decode maps 0 to -1
    assert w.read(3 * K64) == -6
    w = WitnessReader(_q("empty-block-indep"))
    assert len(w.read(K64)) == K64 and w.read(1) == -6


def test_block_size_plus_8_under_the_two_decoders():
    for extra in (0, 1, 8):
        w = WitnessReader(_q(f"over{extra}-indep"))
        assert w.read(4 * K64) == bytes([0x42]) * (K64 + extra) + w.src[0:0] + w.read(0) + WitnessReader(_q(f"over{extra}-indep")).read(4 * K64)[K64 + extra:], extra
    assert WitnessReader(_q("over9-indep")).read(10) == -6
    assert len(WitnessReader(_q("over0-chain")).read(4 * K64)) == 2 * K64
    for extra in (1, 8, 9):
        assert WitnessReader(_q(f"over{extra}-chain")).read(10) == -6, extra
    for tag in ("indep", "chain"):
        assert WitnessReader(_q(f"oversized-raw-{tag}")).read(10) == -6
        assert WitnessReader(_q(f"oversized-stored-{tag}")).read(10) == -6


def test_prefix_of_a_chained_frame():
    assert WitnessReader(_q("far-match-no-history")).read(100) == -6
    assert WitnessReader(_q("far-match-short-history")).read(100_000) == -6
    r = WitnessReader(_q("far-match-raw-history")).read(100_000)                # 64 KiB injected: the prefix reaches back 65535
    assert len(r) == K64 + 10 and r[K64 + 1:K64 + 5] == r[2:6]
    assert len(WitnessReader(_q("far-match-65534")).read(100_000)) == 65534 + 10   # 65534 bytes + 1 literal: offset 65535 is the first byte
    assert WitnessReader(_q("far-match-65533")).read(100_000) == -6             # ... and with one byte less it is one too far


def test_trailing_bytes_and_concatenated_frames(sources):
    for t, code in ((1, -1), (2, -1), (3, -1), (4, -2), (9, -2)):
        w = WitnessReader(_q(f"trailing-{t}"))
        assert len(w.read(1 << 20)) == 2 * K64 and w.read(1) == code, t
    assert WitnessReader(_q("only-3-bytes")).open() == -1
    by = {n: (s, c) for n, s, c in sources}
    s, c = by["three-with-empty"]
    w = WitnessReader(s)
    lens = [len(w.read(1 << 22)) for _ in range(5)]
    assert lens[1] == 0 and sum(lens) == len(c) and lens[3:] == [0, 0] and w.open() == 0      # the empty frame is a read of 0
    w = WitnessReader(by["no-source"][0])
    assert w.open() == 0 and w.read(5) == b""


def test_interactive_returns_after_the_first_drain():
    src = K.indep_frame(bytes(range(256)) * 1024, K64)
    w = WitnessReader(src)
    assert len(w.read(3 * K64, True)) == K64 and len(w.read(100, True)) == 100 and len(w.read(K64, True)) == K64 - 100
    assert w.frame_length is None and w.bytes_read == 2 * K64
    w = WitnessReader(K.indep_frame(b"abc" * 1000, K64, clen=True))
    assert w.frame_length is None and w.open() == 1 and w.frame_length == 3000


def test_block_size_above_the_readers_maximum():
    src = K.indep_frame(b"x" * 1000, 1 << 20)
    assert WitnessReader(src, max_block_size=256 << 10).read(10) == -11
    assert WitnessReader(src, max_block_size=1 << 20).read(10) == b"x" * 10


def test_chain_decoder_prefix_is_min_of_total_and_64k():
    """what the kernel relies on: however LZ4ChainDecoder's ring wraps, the context's prefix is min(bytes so far, 64 KiB)"""
    rng = np.random.default_rng(2)
    for bs in (K64, 256 << 10):
        d = ChainDecoder(bs)
        total = 0
        for _ in range(60):
            n = int(rng.choice([1, 100, 65535, K64, bs]))
            if rng.random() < 0.5:
                d.inject(bytes(n))
            else:
                d.decode(K.rle_block(max(n, 25)))
                n = max(n, 25)
            total += n
            assert min(d.prefix_size, K64) == min(total, K64) and d.prefix_end == d.base + d.output_index


def test_abi_symbols_and_sizes():
    lib = _native.load_library()
    for sym in ("k4lz4_frame_reader_init", "k4lz4_frame_reader_store_bytes", "k4lz4_frame_read_batch", "k4lz4_frame_read_batch_device",
                "k4lz4_frame_reader_query", "k4lz4_frame_reader_query_device", "k4lz4_frame_read_table_rows"):
        assert sym in _native.SYMBOLS and getattr(lib, sym)
    for asked, mb in ((0, 4 << 20), (1, K64), (K64, K64), (K64 + 1, 256 << 10), (1 << 20, 1 << 20), (4 << 20, 4 << 20)):
        rec = F.frame_reader_record(asked, lib)
        assert rec.maxBlockSize == mb
        assert rec.storeBytes == lib.k4lz4_frame_reader_store_bytes(C.byref(rec)) == 256 + (K64 + mb + 64 + 255) // 256 * 256
    with pytest.raises(ValueError):
        F.frame_reader_record((4 << 20) + 1, lib)
    # the fast path's block table: count / 64 KiB + 2 rows per stream
    assert [lib.k4lz4_frame_read_table_rows(c) for c in (-1, 0, 1, K64 - 1, K64, 512 << 10, 4 << 20)] == [0, 0, 2, 2, 3, 10, 66]
    assert (F.FRQ_FAST, F.FRQ_HANDED_BACK, F.FRQ_WORDS) == (6, 7, 8)
    assert (F.FREAD_READ, F.FREAD_OPEN, F.FREAD_RESET, F.FREAD_INTERACTIVE, F.FRAME_BLOCK_SIZE) == (0, 1, 2, 1, -11)
    assert engine().name in ("k4ref", "oracle") and BlockDecoder(1).output_length == 1032
