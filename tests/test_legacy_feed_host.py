"""The fed LZ4Stream reader without a GPU and without the emulator's kernels: the ABI symbols, the two kinds of record and their store
sizes, the refusal of a record of the other kind at the argument check, and the tests' own model of need (legacy_feed_cases.field_ends)
against the witness.  (The refusal of a fed record by the whole-source calls needs a context, so a device: tests/test_gpu_legacy_feed.py
makes those calls; here the condition their check rests on is pinned -- the two kinds never have the same store size.)"""
import ctypes as C

import pytest

import legacy_feed_cases as LC
from legacy_witness import Witness
from legacy_stream_witness import Reader
from test_legacy_host import valid_streams
from k4os.compression.lz4_amd import _native
from k4os.compression.lz4_amd import legacy as L


@pytest.fixture(scope="module")
def w():
    return Witness()


def r256(x):
    return (x + 255) // 256 * 256


def test_abi_symbols_records_and_store_sizes():
    lib = _native.load_library()
    for sym in ("k4lz4_legacy_reader_init_fed", "k4lz4_legacy_read_fed_batch", "k4lz4_legacy_read_fed_batch_device"):
        assert sym in _native.SYMBOLS and getattr(lib, sym)
    for asked, mb in ((0, 1 << 20), (5, 16), (300, 300), (4096, 4096), (65536, 65536), (1 << 20, 1 << 20), (0x7E000000, 0x7E000000)):
        plain, fed = L.legacy_reader_record(asked, lib), L.legacy_reader_record(asked, lib, fed=True)
        # a record made as before: the same bytes
        assert plain.storeBytes == lib.k4lz4_legacy_reader_store_bytes(C.byref(plain)) == 256 + r256(mb + 64)
        assert bytes(plain) == bytes(C.c_int32(mb)) + bytes(C.c_int32(0)) + bytes(C.c_int64(plain.storeBytes))
        # a fed record: the same store followed by the stash (a header of at most 30 bytes, the largest payload)
        assert (fed.maxBlockSize, fed.flags) == (mb, L.LREADER_FED) and plain.flags == 0
        assert fed.storeBytes == lib.k4lz4_legacy_reader_store_bytes(C.byref(fed)) == plain.storeBytes + r256(30 + mb)
        assert fed.storeBytes != plain.storeBytes and fed.storeBytes % 256 == 0
        assert lib.k4lz4_legacy_read_table_rows(C.byref(fed), 10 * mb) == lib.k4lz4_legacy_read_table_rows(C.byref(plain), 10 * mb) == 12
    with pytest.raises(L.ArgumentException):
        L.legacy_reader_record(0x7E000001, lib, fed=True)
    assert (L.LSQ_WORDS, L.LREADER_FED) == (8, 1)


def test_the_fed_calls_refuse_a_whole_source_record_at_the_argument_check():
    lib = _native.load_library()
    plain, fed = L.legacy_reader_record(4096, lib), L.legacy_reader_record(4096, lib, fed=True)
    tampered = L.legacy_reader_record(4096, lib, fed=True)
    tampered.storeBytes = plain.storeBytes
    for rec, refused in ((plain, True), (tampered, True), (fed, False)):
        for call, tail in ((lib.k4lz4_legacy_read_fed_batch, ()), (lib.k4lz4_legacy_read_fed_batch_device, (0, None))):
            # no context: the record's kind is what the call looks at first
            assert call(None, C.byref(rec), *([None] * 12), 1, L.LREAD_READ, 0, *tail) == _native.E_ARG
            msg = lib.k4lz4_last_error(None).decode()
            assert ("k4lz4_legacy_reader_init_fed" in msg) == refused, (msg, refused)


def test_need_model_against_the_witness(w):
    """field_end(i, u) is u + 1 inside or in front of a header and the payload's end inside a payload: a witness over the first u
    bytes that asks for everything has consumed them all, and a witness over the first field_end(u) bytes gets further than one over
    field_end(u) - 1 -- one more header byte read, or the chunk delivered"""
    src, content = LC.small_stream(w, 300)
    streams = [src] + valid_streams(w)[:3]
    fe = LC.field_end_fn(streams)
    for i, s in enumerate(streams):
        lay = LC.layout(s)
        ends = LC.field_ends(s)
        assert sorted(set(ends)) == ends and ends[-1] == len(s) + 1 and (not lay or ends[-2] == len(s))
        for h, p, c, u, flags in lay:
            assert [fe(i, k) for k in range(h, p)] == list(range(h + 1, p + 1))               # a header: byte by byte
            if c:
                assert {fe(i, k) for k in (p, p + c // 2, p + c - 1)} == {p + c}             # a payload: its end
        total = sum(c[3] for c in lay)
        step = max(1, len(s) // 150)
        for u in list(range(0, min(len(s), 40))) + list(range(40, len(s), step)):
            e = fe(i, u)

            def progress(upto):
                r = Reader(w, s[:upto], False, 65536)
                try:
                    got = len(r.read(total + 1))
                except Exception:
                    got = -1
                return r.pos, r.chunks, got
            pos, _, _ = progress(u)
            assert pos == u                                                                  # everything handed over is consumed
            if e <= len(s):
                a, b = progress(e - 1), progress(e)
                assert b[0] == e and (b[1] > a[1] or b[0] > a[0])
    assert fe(0, 0) == 1 and fe(0, len(src)) == len(src) + 1
