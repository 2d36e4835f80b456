"""lz4net's legacy formats without a GPU: the witness (legacy_witness.py, a transcription of LZ4Wrapper / LZ4Stream over the compiled
reference engine) against itself and the C oracle, and the legacy kernels (k4lz4_legacy.hpp) under the host wave emulator against
the witness: the reader's walk / scan / fill on valid and damaged streams, the writer's rows and record sizes, Unwrap's sizes."""
import struct

import numpy as np
import pytest

import legacy_emu as E
from legacy_witness import Witness, Thrown, END_OF_STREAM, OVERFLOW, NOT_SUPPORTED, INVALID_DATA, ARGUMENT
from k4os.compression.lz4_amd import corpus


@pytest.fixture(scope="module")
def w():
    try:
        return Witness()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libk4ref.so not built")


def varint(v: int) -> bytes:
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def contents():
    return [b"", b"x", corpus.lorem(12).tobytes(), corpus.lorem(5000).tobytes(), np.random.default_rng(5).integers(0, 256, 3000, dtype=np.uint8).tobytes(),
            corpus.class_bytes("dickens", 70000, 2).tobytes(), bytes(40000)]


def valid_streams(w):
    out = []
    for c in contents():
        for bs in (16, 1000, 4096, 65536):
            out.append(w.encode_stream(c, bs % 2 == 0 and bs == 4096, bs))
    c = corpus.lorem(9000).tobytes()
    out.append(w.encode_stream(c, False, 4096, pieces=[100, 5000, 1], flush_after=True))     # ragged chunks
    out.append(w.encode_stream(c, True, 1000, pieces=[17, 17, 2000], flush_after=True))
    return out


def damaged_streams(w):
    """truncations, long varints, negative lengths, C > U, passes, empty chunks, claimed sizes, trailing garbage"""
    base = w.encode_stream(corpus.lorem(3000).tobytes(), False, 1000)
    raw = w.encode_stream(np.random.default_rng(1).integers(0, 256, 300, dtype=np.uint8).tobytes(), False, 1000)
    out = [b"", base[:1]]
    for s in (base, raw):
        out += [s[:k] for k in range(1, min(len(s), 40))]                    # every byte of the first records' headers and payloads
        out += [s[:k] for k in range(len(s) - 12, len(s))]
        out.append(s + b"\x00")                                               # a trailing raw chunk header without U
        out.append(s + b"\x00\x00")                                           # an empty raw chunk: skipped
        out.append(s + b"\x01\x00\x00")                                       # an empty compressed chunk: Decode(empty) == 0 == U
        out.append(s + b"\x01\x05\x00")                                       # compressed, C == 0 < U: InvalidData
        out.append(s + b"\x07")                                               # trailing garbage
    lz = w.ref.compress_fast(np.frombuffer(corpus.lorem(200).tobytes(), np.uint8))
    blk = lz[1][:lz[0]].tobytes()
    rec = lambda fl, U, C, p: varint(fl) + varint(U) + (varint(C) if fl & 1 else b"") + p
    out += [
        rec(1, 200, len(blk), blk),                                           # fine
        rec(1 | 4, 200, len(blk), blk),                                       # passes, compressed: NotSupported
        rec(4, 5, 5, b"abcde"),                                               # passes, raw: accepted
        rec(1, 199, len(blk), blk),                                           # decodes to 200 != 199: InvalidData
        rec(1, 255 * len(blk) + 33, len(blk), blk),                           # claims more than C bytes can make
        rec(1, 10, 11, b"x" * 11),                                            # C > U: EndOfStream
        rec(0, 0xFFFFFFFF, 0, b""),                                           # U -> -1 (raw: C = U): Overflow
        rec(1, 0x7FFFFFFF, 0xFFFFFFFF, b""),                                  # C -> -1: Overflow
        rec(1, 0x1_0000_0005, 3, b"abc"),                                     # U truncated to 5: InvalidData (3 bytes do not decode)
        b"\x80" * 9 + b"\x00" + varint(3) + b"abc",                           # a 10-byte flags varint (value 0)
        b"\x81" * 10 + varint(3) + b"abc",                                    # stops after the 10th byte: flags = 1 | ... | 1<<63
        b"\x80" * 10 + b"\x01" + b"abc",                                      # 11 bytes: the 11th is U
        b"\x80\x80",                                                          # truncated varint
        rec(0, 3, 3, b"ab"),                                                  # truncated payload
        rec(0, 0, 0, b"") * 3,                                                # only empty chunks
        rec(0, 5, 5, b"hello") + rec(1 | 8, 4, 2, b"zz"),                     # passes after a good chunk
        rec(0, 5, 5, b"hello") + rec(1, 5, 2, b"\x00\x00") + rec(1 | 4, 4, 2, b"zz"),   # a decode failure before a structural defect
    ]
    return out


def _codes(w, stream):
    chunks, code = w.read_chunks(stream)
    return code


# ---- the witness ---------------------------------------------------------------------------------------------------------------
def test_witness_round_trips(w, oracle):
    for c in contents():
        for high in (False, True):
            for bs in (16, 4096, 1 << 20):
                s = w.encode_stream(c, high, bs)
                assert w.decode_stream(s) == c
            wr = w.wrap(c, high)
            assert w.unwrap(wr) == (c, True)
            if len(c) > 1:
                U, Cl = struct.unpack_from("<II", wr)
                assert U == len(c)
                if not high and Cl < U:
                    assert wr[8:] == oracle.encode(np.frombuffer(c, np.uint8))      # the C oracle's bytes: LZ4_compress_fast


def test_witness_ragged_chunks(w):
    c = corpus.lorem(9000).tobytes()
    s = w.encode_stream(c, False, 4096, pieces=[100, 5000, 1], flush_after=True)
    chunks, code = w.read_chunks(s)
    assert code == 0 and [U for _, U, _, _ in chunks] == [100, 4096, 904, 1, 3899]
    assert w.decode_stream(s) == c


def test_witness_damage_codes(w):
    want = {END_OF_STREAM, OVERFLOW, NOT_SUPPORTED, INVALID_DATA}
    seen = {_codes(w, s) for s in damaged_streams(w)}
    assert want <= seen and 0 in seen


# ---- the kernels under the emulator ---------------------------------------------------------------------------------------------
def _check_walk(w, streams, walked, caps=None):
    for i, (s, got) in enumerate(zip(streams, walked)):
        chunks, code = w.walk(s)
        assert got.status == code, (i, s[:40])
        assert got.size == sum(U for _, U, _, _ in chunks), i
        cap = (1 << 40) if caps is None else caps[i]
        place, rows = 0, []
        for fl, U, Cl, at in chunks:
            room = cap - place >= U
            rows.append((at, U, Cl if (fl & 1 and room) else 0, 2 if not room else (0 if fl & 1 else 1), place))
            place += U
        assert got.rows == rows, i


def test_emulated_walk_on_valid_streams(w):
    streams = valid_streams(w)
    _check_walk(w, streams, E.walk(streams))


def test_emulated_walk_on_damaged_streams(w):
    streams = damaged_streams(w)
    _check_walk(w, streams, E.walk(streams))


def test_emulated_fill_with_short_targets(w):
    streams = valid_streams(w)[:12]
    caps = [max(0, E.walk([s])[0].size - 1) for s in streams]
    _check_walk(w, streams, E.walk(streams, caps), caps)


def test_emulated_walk_many_streams(w):
    base = valid_streams(w) + damaged_streams(w)
    streams = [base[i % len(base)] for i in range(1500)]
    _check_walk(w, streams, E.walk(streams, threads=8))


def test_emulated_writer_rows_and_record_sizes(w):
    rng = np.random.default_rng(3)
    contents_ = [corpus.lorem(int(n)).tobytes() for n in rng.integers(0, 20000, 40)] + [b"", bytes(5000)]
    for bs in (16, 1000, 4096, 100000):
        plan = E.write_plan([len(c) for c in contents_], bs)
        b = max(16, bs)
        assert plan["rows"] == sum((len(c) + b - 1) // b for c in contents_)
        enc = []
        for r in range(plan["rows"]):
            s = int(plan["owner"][r])
            k = r - int(plan["first"][s])
            U = min(b, len(contents_[s]) - k * b)
            assert int(plan["src_len"][r]) == U and int(plan["enc_cap"][r]) == U - 1
            assert int(plan["src_off"][r]) == int(plan["stream_off"][s]) + k * b
            assert int(plan["enc_off"][r]) == int(plan["arena_off"][s]) + k * b
            src = np.frombuffer(contents_[s][k * b:k * b + U], np.uint8)
            enc.append(w.ref.compress_fast(src, U - 1)[0] if U > 1 else 0)
        plan = E.write_plan([len(c) for c in contents_], bs, enc)
        for s, c in enumerate(contents_):
            stream = w.encode_stream(c, False, bs)
            f, nch = int(plan["first"][s]), int(plan["nch"][s])
            got = int(plan["rec_off"][f + nch - 1] + plan["rec_len"][f + nch - 1] - plan["rec_off"][f]) if nch else 0
            assert got == len(stream), (bs, s)
            chunks, _ = w.read_chunks(stream)
            assert [int(x) for x in plan["rec_len"][f:f + nch]] == [len(varint(fl)) + len(varint(U)) + (len(varint(Cl)) if fl & 1 else 0) + Cl
                                                                    for fl, U, Cl, _ in chunks]


def wrapped_cases(w):
    out = []
    for c in (b"", b"a", corpus.lorem(13).tobytes(), corpus.lorem(4000).tobytes(), bytes(3000)):
        out.append(w.wrap(c))
    good = w.wrap(corpus.lorem(4000).tobytes())
    out += [good[:k] for k in range(0, 10)]
    hdr = lambda U, Cl: struct.pack("<II", U & 0xFFFFFFFF, Cl & 0xFFFFFFFF)
    out += [hdr(100, 150) + bytes(150), hdr(100, 151) + bytes(150), hdr(-5, 3) + b"abc", hdr(-5, -7) + b"",
            hdr(10, -1) + b"", hdr(0, 0), hdr(5, 0), hdr(7, 3) + b"\x30abc", hdr(500, 4) + b"zzzz", good + b"trailing",
            hdr(0x7FFFFFFF, 1) + b"\x00"]
    return out


def _witness_unwrap(w, b):
    try:
        r, ok = w.unwrap(b)
        return len(r), ok
    except Thrown as e:
        return e.code, None


def test_emulated_unwrap_sizes(w):
    cases = wrapped_cases(w)
    out, dlen, dcap = E.unwrap_sizes(cases)
    for i, b in enumerate(cases):
        want, _ = _witness_unwrap(w, b)
        assert int(out[i]) == want, (i, b[:12])
        if want >= 0 and dcap[i]:
            assert int(dcap[i]) == want and int(dlen[i]) == struct.unpack_from("<i", b, 4)[0]
    caps = [max(0, int(x) - 1) for x in out]
    out2, _, _ = E.unwrap_sizes(cases, caps)
    assert [int(x) for x in out2] == [-6 if int(x) > 0 else int(x) for x in out]
