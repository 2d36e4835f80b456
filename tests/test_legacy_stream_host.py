"""LZ4Stream piece by piece, without a GPU: the witness (legacy_stream_witness.py) against itself and against the whole-stream
witness, the lazy-flush rule, and the library's host arithmetic (the record, the model behind k4lz4_legacy_write_bound)."""
import ctypes as C

import numpy as np
import pytest

from legacy_witness import Witness, Thrown
from legacy_stream_witness import Reader, WriterCalls, read_calls, chunk_count, lazy_flush
from test_legacy_host import valid_streams, damaged_streams
from k4os.compression.lz4_amd import _native, corpus
from k4os.compression.lz4_amd import legacy as L


@pytest.fixture(scope="module")
def w():
    return Witness()


def random_counts(rng, total, calls=None):
    """counts of every kind: 0, 1, small, around typical chunk sizes, larger than everything"""
    out = []
    while sum(out) < total + 50 and (calls is None or len(out) < calls):
        out.append(int(rng.choice([0, 1, 2, 15, 16, 17, 999, 1000, 1001, 4096, 5000, 70000, int(rng.integers(1, 3000))])))
    return out + [10, 10]


def test_reader_counts_concatenate_to_decode_stream(w):
    rng = np.random.default_rng(5)
    for s in valid_streams(w):
        want = w.decode_stream(s)
        for interactive in (False, True):
            if interactive:                           # an interactive read delivers at most one chunk's rest: read to the end
                r, got = Reader(w, s, True), []
                while not got or got[-1]:
                    got.append(r.read(int(rng.integers(1, 5000))))
            else:
                got = read_calls(w, s, random_counts(rng, len(want)), interactive)
            assert all(isinstance(g, bytes) for g in got)
            assert b"".join(got) == want
            if not interactive:                       # a non-interactive read is short only at the end of the stream
                counts = random_counts(np.random.default_rng(6), len(want))
                pos = 0
                for c, g in zip(counts, read_calls(w, s, counts)):
                    assert len(g) == min(c, len(want) - pos)
                    pos += len(g)


def test_interactive_reads_never_cross_a_chunk(w):
    rng = np.random.default_rng(7)
    for s in valid_streams(w)[::3]:
        chunks, code = w.read_chunks(s)
        assert code == 0
        edges = np.cumsum([0] + [u for _, u, _, _ in chunks])
        r = Reader(w, s, interactive=True)
        pos = 0
        while True:
            c = int(rng.integers(1, 6000))
            g = r.read(c)
            if not g:
                break
            k = int(np.searchsorted(edges, pos, side="right")) - 1
            assert pos + len(g) <= edges[k + 1] and len(g) == min(c, edges[k + 1] - pos)
            pos += len(g)
        assert pos == edges[-1]


def test_read_byte_and_count_zero(w):
    s = w.encode_stream(corpus.lorem(100).tobytes(), False, 16)
    r = Reader(w, s)
    assert r.read(0) == b"" and r.pos == 0                      # count == 0 acquires nothing
    got = bytearray()
    while (b := r.read_byte()) >= 0:
        got.append(b)
    assert bytes(got) == corpus.lorem(100).tobytes()
    assert read_calls(w, s, [1] * 101) == [bytes([b]) for b in got] + [b""]


def test_reader_codes_and_failed_streams_stay_failed(w):
    rng = np.random.default_rng(8)
    for s in damaged_streams(w):
        _, code = w.read_chunks(s)
        for interactive in (False, True):
            got = read_calls(w, s, random_counts(rng, 8000, calls=40 if interactive else None), interactive)
            codes = [g for g in got if isinstance(g, int)]
            if code == 0:
                assert not codes and w.decode_stream(s).startswith(b"".join(got))
                assert interactive or b"".join(got) == w.decode_stream(s)
            else:
                if not interactive:
                    assert codes and codes[0] == code
                k = next((i for i, g in enumerate(got) if isinstance(g, int)), len(got))
                assert all(g == code for g in got[k:])          # stays failed
                # what was delivered before the failing call is the good chunks' prefix
                good = bytearray()
                for flags, U, Cl, at in w.read_chunks(s)[0]:
                    good += w.decode(s[at:at + Cl], U)[1][:U] if flags & 1 else s[at:at + U]
                assert bytes(good).startswith(b"".join(got[:k]))


def test_reader_block_size_limit(w):
    s = w.encode_stream(corpus.lorem(5000).tobytes(), False, 1000)
    assert read_calls(w, s, [10], max_block_size=999) == [-8]
    assert read_calls(w, s, [5000, 1], max_block_size=1000) == [corpus.lorem(5000).tobytes(), b""]


SIZES = lambda B: [0, 1, 15, 16, B - 1, B, B + 1, 2 * B, 3 * B + 7]      # noqa: E731


@pytest.mark.parametrize("B", [16, 4096, 1 << 20])
def test_writer_lazy_flush_formula(w, B):
    """per call: chunks emitted and bytes pending follow max(0, ceil((p + L) / B) - 1) -- a buffer filled exactly waits"""
    data = corpus.class_bytes("xml", 3 * B + 7, 3).tobytes()
    rng = np.random.default_rng(B)
    wc = WriterCalls(w, False, B)
    whole = bytearray()
    content = bytearray()
    seq = SIZES(B) + [int(x) for x in rng.permutation(SIZES(B))]
    for i, n in enumerate(seq):
        p = wc.pending
        out = wc.write(data[:n])
        content += data[:n]
        e, rest = lazy_flush(B, p, n, "write")
        assert (chunk_count(out), wc.pending) == (e, rest), (B, p, n)
        whole += out
        if i % 3 == 2:
            p = wc.pending
            out = wc.flush()
            assert (chunk_count(out), wc.pending) == lazy_flush(B, p, 0, "flush")
            whole += out
    p = wc.pending
    out = wc.dispose(data[:B])
    content += data[:B]
    assert chunk_count(out) == lazy_flush(B, p, B, "close")[0]
    whole += out
    assert w.decode_stream(bytes(whole)) == bytes(content)
    # a Write that fills the buffer exactly emits nothing; the next byte sends it out
    wc = WriterCalls(w, False, B)
    assert wc.write(data[:B]) == b"" and wc.pending == B
    assert chunk_count(wc.write(data[:1])) == 1 and wc.pending == 1


def test_one_write_and_dispose_is_encode_stream(w):
    c = corpus.lorem(9000).tobytes()
    for high in (False, True):
        for B in (16, 1000, 4096):
            wc = WriterCalls(w, high, B)
            assert wc.write(c) + wc.dispose() == w.encode_stream(c, high, B)
            assert WriterCalls(w, high, B).dispose(c) == w.encode_stream(c, high, B)


# ---- the library's host arithmetic ------------------------------------------------------------------------------------------
def _rec(lib, B, high=False):
    r = L.LegacyWriterRecord()
    assert lib.k4lz4_legacy_writer_init(C.byref(r), B, int(high)) == 0
    return r


@pytest.mark.parametrize("B", [1, 16, 4096, 1 << 20])
def test_write_bound_covers_the_witness(w, B):
    lib = _native.load_library()
    r = _rec(lib, B)
    Beff = max(16, B)
    assert r.blockSize == Beff and lib.k4lz4_legacy_writer_store_bytes(C.byref(r)) >= Beff
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, 3 * Beff + 7, dtype=np.uint8).tobytes()      # incompressible: every chunk is stored
    text = corpus.class_bytes("xml", 3 * Beff + 7, 1).tobytes()
    for data in (noise, text):
        wc = WriterCalls(w, False, B)
        for n in SIZES(Beff):
            for op, name in ((L.LWRITE_WRITE, "write"), (L.LWRITE_FLUSH, "flush")):
                r.pending = wc.pending
                bound = lib.k4lz4_legacy_write_bound(C.byref(r), n if op == L.LWRITE_WRITE else 0, op)
                out = wc.write(data[:n]) if op == L.LWRITE_WRITE else wc.flush()
                assert len(out) <= bound, (B, n, name)
                e, _ = lazy_flush(Beff, r.pending, n if op == L.LWRITE_WRITE else 0, name)
                assert (bound == 0) == (e == 0)
        r.pending = wc.pending
        bound = lib.k4lz4_legacy_write_bound(C.byref(r), 5, L.LWRITE_CLOSE)
        assert len(wc.dispose(data[:5])) <= bound
    r.closed = 1
    assert lib.k4lz4_legacy_write_bound(C.byref(r), 100, L.LWRITE_WRITE) == 0
    assert lib.k4lz4_legacy_write_bound(C.byref(_rec(lib, B)), -1, L.LWRITE_WRITE) == 0


def test_records_and_refusals_of_init():
    lib = _native.load_library()
    r = L.LegacyWriterRecord()
    assert lib.k4lz4_legacy_writer_init(C.byref(r), 0x7E000001, 0) != 0
    rd = L.LegacyReaderRecord()
    assert lib.k4lz4_legacy_reader_init(C.byref(rd), 0) == 0 and rd.maxBlockSize == 1 << 20
    assert lib.k4lz4_legacy_reader_init(C.byref(rd), 5) == 0 and rd.maxBlockSize == 16
    assert rd.storeBytes == lib.k4lz4_legacy_reader_store_bytes(C.byref(rd)) and rd.storeBytes % 256 == 0 and rd.storeBytes >= 256 + 16
    assert lib.k4lz4_legacy_reader_init(C.byref(rd), 4096) == 0
    assert lib.k4lz4_legacy_read_table_rows(C.byref(rd), 0) == 0
    assert lib.k4lz4_legacy_read_table_rows(C.byref(rd), 4096 * 10) == 12
    assert lib.k4lz4_legacy_read_table_rows(C.byref(rd), 1 << 30) == 1024
    assert lib.k4lz4_legacy_reader_init(C.byref(rd), 0x7E000001) != 0
    assert isinstance(L.legacy_exception(L.LEGACY_CLOSED), L.ObjectDisposedException)
    assert isinstance(L.legacy_exception(L.LEGACY_BLOCK_SIZE), L.CapacityError)
