"""The device frame reader's walk (k4lz4_frame_read.hpp: k4_frame_walk_kernel, k4_frame_scan_kernel, k4_frame_fill_kernel) under
the host wave emulator, against the host walk (frames.parse_frame) and a transcription of the reference's stream-order reader
(frame_stream_reader.py): header fields, decoded-size bounds, block tables, and the first defect of damaged frames."""
import ctypes as C
import struct

import numpy as np
import pytest
import xxhash

import frame_read_emu as E
import frame_stream_reader as R
from oracle_lib import FrameOracle
from test_frame_layer import LZ4F, _contents
from k4os.compression.lz4_amd import corpus
from k4os.compression.lz4_amd import frames as F

STRUCTURAL = (-1, -2, -3, -4, -5)


@pytest.fixture(scope="module")
def fo(oracle):
    return FrameOracle(oracle)


@pytest.fixture(scope="module")
def lz4f():
    try:
        return LZ4F()
    except OSError:
        pytest.skip("liblz4.so.1 not present")


def _bound(info: F.FrameInfo) -> int:
    bs = info.descriptor.BlockSize
    total = sum((l & 0x7FFFFFFF) if l & 0x80000000 else F.LZ4Frame._block_cap(bs, l) for l in info.block_len)
    cl = info.descriptor.ContentLength
    return total if cl is None else min(total, cl)


def _check_against_parse(frames, walked, caps=None):
    for i, (fr, w) in enumerate(zip(frames, walked)):
        info = F.parse_frame(fr)
        d = info.descriptor
        assert w.status == 0, i
        assert w.flg == fr[4] and w.bd == fr[5], i
        assert w.block_size == d.BlockSize and w.hdr_end == 4 + len(info.header) + 1, i
        assert w.content_length == (d.ContentLength or 0), i
        assert w.block_off == info.block_off and w.block_len == info.block_len, i
        assert w.block_checksum == (info.block_checksum if d.BlockChecksum else [0] * len(info.block_off)), i
        assert w.content_checksum == (info.content_checksum or 0), i
        assert w.size == _bound(info), i
        bs = d.BlockSize
        cap = (1 << 40) if caps is None else caps[i]
        assert w.block_dst_off == [k * bs for k in range(len(info.block_off))], i
        assert w.block_dst_cap == [max(0, min(bs, cap - k * bs)) for k in range(len(info.block_off))], i
        assert w.block_src_len == [0 if (l & 0x80000000 or d.Chaining or min(bs, cap - k * bs) <= 0) else l
                                   for k, l in enumerate(info.block_len)], i


def test_walk_matches_parse_frame_on_oracle_and_liblz4_frames(fo, lz4f):
    frames = []
    for c in _contents():
        for bsum, csum in ((False, False), (True, False), (False, True), (True, True)):
            frames.append(fo.frame_encode(c, 65536, 0, bsum, csum))
        for bid in (4, 5, 6, 7):
            for linked in (False, True):
                frames.append(lz4f.compress(c, bid, linked, content_checksum=bid % 2 == 0, block_checksum=linked, content_size=bid >= 6))
    walked, counters = E.walk(frames)
    _check_against_parse(frames, walked)
    infos = [F.parse_frame(f) for f in frames]
    assert counters[0] == sum(len(i.block_off) for i in infos)
    assert counters[1] == sum(1 for i in infos if i.descriptor.BlockChecksum and i.block_off)
    assert counters[2] == sum(1 for i in infos if not i.descriptor.Chaining for l in i.block_len if not l & 0x80000000)
    assert counters[3] == sum(1 for i in infos if i.descriptor.ContentChecksum)
    # bytes after a frame are ignored; a target shorter than the blocks gives them the room that is left
    walked2, _ = E.walk([f + b"\x01\x02\x03garbage" for f in frames[:8]], dst_cap=[100000] * 8)
    _check_against_parse(frames[:8], walked2, caps=[100000] * 8)


def _lz4_compress(data: bytes) -> bytes:
    lib = C.CDLL("liblz4.so.1")
    cap = len(data) + len(data) // 255 + 16
    dst = C.create_string_buffer(cap)
    n = lib.LZ4_compress_default(data, dst, len(data), cap)
    assert n > 0
    return dst.raw[:n]


def irregular_frames():
    """frames of this project's writer shape with short and raw middle blocks, and with a ContentLength"""
    data = corpus.class_bytes("dickens", 40000, 9).tobytes()
    rnd = corpus.random_bytes(3000, 4).tobytes()
    out = []
    for bsum, csum, clen in ((False, False, False), (True, True, False), (True, False, True)):
        pieces = [data[:10000], rnd, data[10000:30000], rnd[:700], data[30000:]]
        raw = [False, True, False, True, False]
        payloads = [p if r else _lz4_compress(p) for p, r in zip(pieces, raw)]
        content = b"".join(pieces)
        d = F.LZ4Descriptor(len(content) if clen else None, csum, False, bsum, None, 65536)
        h = xxhash.xxh32(F.frame_header(d), seed=0).intdigest()
        out.append((F.assemble_frame(d, h, payloads, raw, [xxhash.xxh32(p, seed=0).intdigest() for p in payloads],
                                     xxhash.xxh32(content, seed=0).intdigest()), content))
    return out


def empty_frames():
    out = []
    for bsum, csum, clen, chain in ((False, False, False, False), (True, True, True, True), (False, True, False, True)):
        d = F.LZ4Descriptor(0 if clen else None, csum, chain, bsum, None, 65536)
        h = xxhash.xxh32(F.frame_header(d), seed=0).intdigest()
        out.append(F.assemble_frame(d, h, [], [], [], xxhash.xxh32(b"", seed=0).intdigest()))
    return out


def test_walk_of_short_raw_middle_blocks_and_empty_frames():
    frames = [f for f, _ in irregular_frames()] + empty_frames()
    walked, _ = E.walk(frames)
    _check_against_parse(frames, walked)
    for fr, (f, content) in zip(walked, irregular_frames()):
        assert R.read_frame(f) == (0, content)
        assert fr.block_src_len[1] == 0 and fr.block_src_len[3] == 0          # raw blocks are copied, not decoded
    for w in walked[-3:]:
        assert w.block_off == [] and w.size == 0 and w.status == 0
    assert all(R.read_frame(f) == (0, b"") for f in empty_frames())


def test_every_truncation_of_a_small_frame(fo):
    c = corpus.class_bytes("xml", 150000, 2)
    for bsum, csum in ((True, True), (False, False)):
        fr = fo.frame_encode(c, 65536, 0, bsum, csum)
        cuts = [fr[:n] for n in range(len(fr) + 1)]
        walked, _ = E.walk(cuts)
        info = F.parse_frame(fr)
        rec_end = [o + (l & 0x7FFFFFFF) + (4 if bsum else 0) for o, l in zip(info.block_off, info.block_len)]
        for n, w in enumerate(walked):
            want, _ = R.read_frame(cuts[n])
            if n == len(fr):
                assert w.status == 0 and want == 0
                continue
            assert w.status == -1 and want == -1, n
            assert len(w.block_off) == sum(1 for e in rec_end if e <= n), n          # the complete records before the cut
            if w.hdr_end:
                assert w.block_len == info.block_len[:len(w.block_off)], n


def test_every_single_bit_flip_in_a_header(fo, lz4f):
    c = corpus.class_bytes("dickens", 100000, 3)
    sources = [fo.frame_encode(c, 65536, 0, True, True), lz4f.compress(c, 5, True, True, True, content_size=True)]
    for fr in sources:
        hdr_end = 4 + len(F.parse_frame(fr).header) + 1
        muts = []
        for pos in range(hdr_end):
            for bit in range(8):
                b = bytearray(fr)
                b[pos] ^= 1 << bit
                muts.append(bytes(b))
        walked, _ = E.walk(muts)
        for m, w in zip(muts, walked):
            want, _ = R.read_frame(m)
            if want in STRUCTURAL:
                assert w.status == want
            else:
                assert w.status in (0, -1)
        assert {w.status for w in walked} >= {-2, -4}


def test_dictionary_flag_and_stream_order_of_two_defects():
    d = F.LZ4Descriptor(None, False, False, False, None, 65536)
    flg_bd = bytearray(F.frame_header(d))
    flg_bd[0] |= 1                                                              # dictionary id follows
    hdr = bytes(flg_bd) + struct.pack("<I", 0x12345678)
    good = struct.pack("<I", F.MAGIC) + hdr + bytes([(xxhash.xxh32(hdr, seed=0).intdigest() >> 8) & 0xFF]) + struct.pack("<I", 0)
    bad_sum = bytearray(good)
    bad_sum[4 + len(hdr)] ^= 0xFF
    # a frame with a good header and a record that runs past the end, and the same with a broken header checksum as well
    d2 = F.LZ4Descriptor(None, False, False, False, None, 65536)
    h2 = xxhash.xxh32(F.frame_header(d2), seed=0).intdigest()
    trunc = F.assemble_frame(d2, h2, [b"\x10abcdefghijklmnop"], [False], None, None)[:-6]
    trunc_bad = bytearray(trunc)
    trunc_bad[6] ^= 0x55
    walked, _ = E.walk([good, bytes(bad_sum), trunc, bytes(trunc_bad)])
    assert [w.status for w in walked] == [-5, -4, -1, -4]                       # header checksum before the dictionary
    assert [R.read_frame(f)[0] for f in (good, bytes(bad_sum), trunc, bytes(trunc_bad))] == [-5, -4, -1, -4]
    # LZ4Frame.DecodeBatch walks the whole frame first, so it names the dictionary (and the truncation) instead
    assert F.parse_frame(good).descriptor.Dictionary == 0x12345678
    with pytest.raises(EOFError):
        F.parse_frame(bytes(trunc_bad))
    assert walked[0].size == 0 and walked[0].hdr_end == 0


def test_bad_magic_version_and_tiny_inputs():
    d = F.LZ4Descriptor(None, False, False, False, None, 65536)
    h = xxhash.xxh32(F.frame_header(d), seed=0).intdigest()
    fr = F.assemble_frame(d, h, [], [], None, None)
    v0 = bytearray(fr)
    v0[4] &= 0x3F
    frames = [b"", b"\x04\x22", fr[:4], fr[:5], b"\x00" * 12, bytes(v0), fr]
    walked, _ = E.walk(frames)
    assert [w.status for w in walked] == [R.read_frame(f)[0] for f in frames] == [-1, -1, -1, -1, -2, -3, 0]
