"""The fed frame reader without a GPU: the host model of its store and record (the ABI symbols, the store sizes for the four
block-size codes, a record made as before unchanged byte for byte), and the test infrastructure's own field layout."""
import ctypes as C

import pytest

import frame_feed_cases as FC
import frame_feed_emu as E
from k4os.compression.lz4_amd import _native
from k4os.compression.lz4_amd import frames as F

K64 = 65536


def r256(x):
    return (x + 255) // 256 * 256


def test_abi_symbols_and_store_sizes():
    lib = _native.load_library()
    for sym in ("k4lz4_frame_read_fed_batch", "k4lz4_frame_read_fed_batch_device"):
        assert sym in _native.SYMBOLS and getattr(lib, sym)
    for asked, mb in ((0, 4 << 20), (1, K64), (K64, K64), (K64 + 1, 256 << 10), (1 << 20, 1 << 20), (4 << 20, 4 << 20)):
        plain, fed = F.frame_reader_record(asked, lib), F.frame_reader_record(asked, lib, fed=True)
        # a record made as before: the size test_frame_reader_host.py::test_abi_symbols_and_sizes pins, and the same bytes
        assert plain.storeBytes == lib.k4lz4_frame_reader_store_bytes(C.byref(plain)) == 256 + r256(K64 + mb + 64)
        assert bytes(plain) == bytes(C.c_int32(mb)) + bytes(C.c_int32(0)) + bytes(C.c_int64(plain.storeBytes))
        # a fed record: the same store followed by the stash (a length word, the largest payload, its block checksum)
        assert (fed.maxBlockSize, fed.flags) == (mb, F.FREADER_FED)
        assert fed.storeBytes == lib.k4lz4_frame_reader_store_bytes(C.byref(fed)) == plain.storeBytes + r256(4 + mb + 4)
        assert fed.storeBytes == E.lib().k4emu_ff_store_bytes(asked, 1) and plain.storeBytes == E.lib().k4emu_ff_store_bytes(asked, 0)
    assert E.lib().k4emu_ff_state_bytes() <= 256                       # FrState with the stash's fill and awaited length: FR_STATE_BYTES stays
    with pytest.raises(ValueError):
        F.frame_reader_record((4 << 20) + 1, lib, fed=True)
    rec = F.FrameReaderRecord()
    assert lib.k4lz4_frame_reader_init(C.byref(rec), (C.c_int32 * 2)(K64, 2)) != 0     # an unknown flag
    assert (F.FRQ_WORDS, F.FREADER_FED) == (8, 1)


def test_field_layout_of_the_small_source():
    src, content = FC.small_source()
    ends = FC.field_ends(src)
    assert 300 < len(src) < 1200 and len(content) == 2 * K64 + 280
    # first frame: magic, FLG / BD, ContentLength + HC, then three records, the EndMark and the content checksum
    assert ends[:3] == [4, 6, 15] and ends[3] == 19 and ends[-1] == len(src) + 4 and ends[-2] == len(src)
    fe = FC.field_end_fn([src])
    assert [fe(0, k) for k in (0, 3, 4, 5, 6, 14, 15, 18)] == [4, 4, 6, 6, 15, 15, 19, 19]
    assert sorted(set(ends)) == ends
