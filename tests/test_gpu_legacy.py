"""lz4net's legacy formats on the GPU (k4lz4_legacy.hpp through the C ABI), byte for byte against the witness (legacy_witness.py:
LZ4Wrapper / LZ4Stream transcribed over the compiled reference engine)."""
import struct

import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

from legacy_witness import Witness, Thrown
from test_legacy_host import valid_streams, damaged_streams, wrapped_cases
from k4os.compression.lz4_amd import LZ4Codec, LZ4Legacy, corpus, pack_blocks
from k4os.compression.lz4_amd import legacy as L
from k4os.compression.lz4_amd.device import DeviceCodec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


@pytest.fixture(scope="module")
def w():
    return Witness()


@pytest.fixture(scope="module")
def w32():
    return Witness(x32=True)


def messages():
    rng = np.random.default_rng(11)
    out = [b"", b"a", corpus.lorem(12).tobytes(), corpus.lorem(13).tobytes()]
    for n in (65546, 65547, 65548):
        out.append(corpus.class_bytes("dickens", n, 1).tobytes())
    out.append(rng.integers(0, 256, 70000, dtype=np.uint8).tobytes())                       # incompressible
    out.append(corpus.class_bytes("xml", (4 << 20) + 7, 2).tobytes())                        # big enough for segments
    out.append(rng.integers(0, 256, (1 << 20) + 3, dtype=np.uint8).tobytes())
    return out


def _dev_bufs(dc, bufs):
    views = [np.frombuffer(bytes(b), np.uint8) for b in bufs]
    data, off, lens = pack_blocks(views)
    return torch.from_numpy(data).to(dc.device), off.astype(np.int64), np.array([v.size for v in views], np.int64)


def _outs(buf, off, length):
    h, n = buf.cpu().numpy(), length.cpu().numpy()
    return [h[int(o):int(o) + int(x)].tobytes() if x >= 0 else int(x) for o, x in zip(np.asarray(off), n)]


@pytest.mark.parametrize("x32", [False, True])
@pytest.mark.parametrize("high", [False, True])
def test_wrap_host_and_device(dc, w, w32, x32, high):
    msgs = messages() if not high else messages()[:9]
    wit = w32 if x32 else w
    want = [wit.wrap(m, high) for m in msgs]
    try:
        LZ4Codec.Enforce32 = x32
        got = LZ4Legacy.WrapBatch(msgs, high=high)
        d, off, ln = _dev_bufs(dc, msgs)
        buf, o, olen = L.wrap_device(dc, d, off, ln, high=high)
        dev = _outs(buf, o, olen)
        one = (LZ4Legacy.WrapHC if high else LZ4Legacy.Wrap)(msgs[3])
    finally:
        LZ4Codec.Enforce32 = False
    for i in range(len(msgs)):
        assert got[i] == want[i], i
        assert dev[i] == want[i], i
    assert one == want[3]


def test_wrap_many_small_messages(dc, w):
    rng = np.random.default_rng(4)
    msgs = [corpus.lorem(int(n)).tobytes() for n in rng.integers(0, 3000, 1200)]
    got = LZ4Legacy.WrapBatch(msgs)
    for m, g in zip(msgs, got):
        assert g == w.wrap(m)


def test_wrap_offsets_and_arguments(w):
    buf = corpus.lorem(500).tobytes()
    assert LZ4Legacy.Wrap(buf, 10, 100) == w.wrap(buf, False, 10, 100)
    assert LZ4Legacy.Wrap(buf, 480) == w.wrap(buf, False, 480)
    assert LZ4Legacy.Wrap(buf, 500) == bytes(8)
    with pytest.raises(L.ArgumentException):
        LZ4Legacy.Wrap(buf, 501)


def test_unwrap_round_trip_and_damage(dc, w):
    good = [w.wrap(m, h) for m in messages() for h in (False,)]
    cases = good + wrapped_cases(w)
    for i, b in enumerate(cases):
        try:
            r, ok = w.unwrap(b)
        except Thrown as e:
            with pytest.raises(type(L.legacy_exception(e.code))):
                LZ4Legacy.Unwrap(b)
            continue
        got, gok = LZ4Legacy.UnwrapBatch([b])
        assert len(got[0]) == len(r) and bool(gok[0]) == ok, i
        if ok:
            assert got[0] == r, i
    d, off, ln = _dev_bufs(dc, cases)
    buf, o, olen, dec = L.unwrap_device(dc, d, off, ln.astype(np.int32))
    outs, decs = _outs(buf, o, olen), dec.cpu().numpy()
    for i, b in enumerate(cases):
        try:
            r, ok = w.unwrap(b)
        except Thrown as e:
            assert outs[i] == e.code, i
            continue
        assert len(outs[i]) == len(r) and (int(decs[i]) == len(r)) == ok, i
        if ok:
            assert outs[i] == r, i
    assert LZ4Legacy.Unwrap(b"\x00" * 4 + good[3], 4) == messages()[3]


def test_unwrap_target_one_byte_short(dc, w):
    good = [w.wrap(m) for m in messages()[1:8]]
    d, off, ln = _dev_bufs(dc, good)
    sizes = np.array([LZ4Legacy.UnwrappedSize(g) for g in good], np.int64)
    caps = sizes - 1
    buf = torch.zeros(int(((sizes + 15) // 16 * 16).sum()) + 64, dtype=torch.uint8, device=dc.device)
    o = np.zeros(len(good), np.int64)
    o[1:] = np.cumsum((sizes + 15) // 16 * 16)[:-1]
    _, _, olen, _ = L.unwrap_device(dc, d, off, ln.astype(np.int32), out=(buf, o, caps))
    assert (olen.cpu().numpy() == L.LEGACY_CAPACITY).all()
    assert not buf.cpu().numpy().any()


@pytest.mark.parametrize("high", [False, True])
@pytest.mark.parametrize("bs", [16, 4096, 65536, 100000, 1 << 20, 4 << 20])
def test_encode_batch_block_sizes(dc, w, high, bs):
    rng = np.random.default_rng(bs)
    contents = [b"", b"q", corpus.lorem(5000).tobytes(), corpus.class_bytes("dickens", 300000, 3).tobytes(),
                rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()]
    if bs >= 65536 and not high:
        contents.append(corpus.class_bytes("xml", (9 << 20) + 5, 1).tobytes())
    if bs == 16:
        contents = contents[:4]
    got = LZ4Legacy.EncodeBatch(contents, high, bs)
    for i, c in enumerate(contents):
        want = w.encode_stream(c, high, bs)
        assert got[i] == want, (i, len(c))
        assert LZ4Legacy.Decode(got[i]) == c
    d, off, ln = _dev_bufs(dc, contents)
    buf, o, olen = L.encode_legacy_streams_device(dc, d, off, ln, high=high, block_size=bs)
    assert _outs(buf, o, olen) == got


def test_encode_enforce32(dc, w32):
    c = corpus.class_bytes("dickens", 200000, 1).tobytes()
    try:
        LZ4Codec.Enforce32 = True
        got = LZ4Legacy.Encode(c, False, 65536)
    finally:
        LZ4Codec.Enforce32 = False
    assert got == w32.encode_stream(c, False, 65536)


def _dev_decode(dc, streams, caps=None):
    d, off, ln = _dev_bufs(dc, streams)
    out = None
    if caps is not None:
        caps = np.asarray(caps, np.int64)
        o = np.zeros(len(caps), np.int64)
        o[1:] = np.cumsum((caps + 15) // 16 * 16)[:-1]
        out = (torch.zeros(int(((caps + 15) // 16 * 16).sum()) + 64, dtype=torch.uint8, device=dc.device), o, caps)
    buf, o, olen = L.decode_legacy_streams_device(dc, d, off, ln, out=out, raise_errors=False)
    return _outs(buf, o, olen)


def _witness_decode(w, s):
    try:
        return w.decode_stream(s)
    except Thrown as e:
        return e.code


def test_decode_valid_ragged_and_damaged(dc, w):
    streams = valid_streams(w) + damaged_streams(w)
    want = [_witness_decode(w, s) for s in streams]
    assert _dev_decode(dc, streams) == want
    for s, x in zip(streams, want):
        if isinstance(x, int):
            with pytest.raises(type(L.legacy_exception(x))):
                LZ4Legacy.Decode(s)
        else:
            assert LZ4Legacy.Decode(s) == x


def test_decode_mixed_batch_of_1500_streams(dc, w):
    base = valid_streams(w) + damaged_streams(w)
    rng = np.random.default_rng(8)
    streams = [base[int(i)] for i in rng.integers(0, len(base), 1500)]
    want = [_witness_decode(w, s) for s in streams]
    assert _dev_decode(dc, streams) == want
    good = [s for s, x in zip(streams, want) if not isinstance(x, int)]
    assert LZ4Legacy.DecodeBatch(good) == [x for x in want if not isinstance(x, int)]


def test_decode_big_streams(dc, w):
    contents = [corpus.class_bytes("xml", (6 << 20) + 11, 4).tobytes(), corpus.class_bytes("dickens", 3 << 20, 5).tobytes()]
    streams = LZ4Legacy.EncodeBatch(contents, False, 1 << 20) + LZ4Legacy.EncodeBatch(contents[1:], True, 4 << 20)
    assert _dev_decode(dc, streams) == contents + contents[1:]


def test_decode_target_capacity_edges(dc, w):
    streams = valid_streams(w)[:20]
    want = [_witness_decode(w, s) for s in streams]
    sizes = [len(x) for x in want]
    assert _dev_decode(dc, streams, sizes) == want
    short = _dev_decode(dc, streams, [max(0, n - 1) for n in sizes])
    assert short == [L.LEGACY_CAPACITY if n > 0 else b"" for n in sizes]
    # a decode failure before the chunk that does not fit is what the stream reports
    s = damaged_streams(w)[-1]
    assert _dev_decode(dc, [s], [10]) == [L.LEGACY_INVALID_DATA]
    assert _dev_decode(dc, [s], [5]) == [L.LEGACY_CAPACITY]


def test_host_sizes_match_device_sizes(dc, w):
    streams = valid_streams(w) + damaged_streams(w)
    d, off, ln = _dev_bufs(dc, streams)
    size, status = L.legacy_stream_sizes_device(dc, d, off, ln)
    for s, sz, st in zip(streams, size.cpu().numpy(), status.cpu().numpy()):
        chunks, code = w.walk(s)
        assert int(st) == code and int(sz) == sum(U for _, U, _, _ in chunks)
