"""Sources for the incremental frame reader's tests, all made without a GPU: hand-assembled frames (frames.assemble_frame over
liblz4's blocks), liblz4's own frames (independent and linked), the quirk cases of the issue, structural mutations and read plans.
Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import xxhash

from k4os.compression.lz4_amd import corpus
from k4os.compression.lz4_amd import frames as F

K64 = 65536
BLOCK_SIZES = {4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}
_lz4 = None


def lz4():
    global _lz4
    if _lz4 is None:
        _lz4 = C.CDLL("liblz4.so.1")
    return _lz4


def compress(data: bytes) -> bytes:
    cap = len(data) + len(data) // 255 + 16
    dst = C.create_string_buffer(cap)
    n = lz4().LZ4_compress_default(data, dst, len(data), cap)
    assert n > 0
    return dst.raw[:n]


def x32(b: bytes) -> int:
    return xxhash.xxh32(b, seed=0).intdigest()


def frame_of(payloads, raw, content: bytes, bs=K64, chain=False, bsum=False, csum=False, clen=None, content_hash=None):
    """a frame around given block payloads"""
    d = F.LZ4Descriptor(clen, csum, chain, bsum, None, bs)
    return F.assemble_frame(d, x32(F.frame_header(d)), payloads, raw, [x32(p) for p in payloads],
                            x32(content) if content_hash is None else content_hash)


def indep_frame(content: bytes, bs=K64, bsum=False, csum=False, clen=False, cut=None, raw_every=0):
    """independent blocks cut at `cut` (default: the block size) bytes; every raw_every-th block stored raw"""
    cut = cut or bs
    pieces = [content[i:i + cut] for i in range(0, len(content), cut)]
    raw = [bool(raw_every) and k % raw_every == raw_every - 1 for k in range(len(pieces))]
    payloads = [p if r else compress(p) for p, r in zip(pieces, raw)]
    return frame_of(payloads, raw, content, bs, False, bsum, csum, len(content) if clen else None)


def literal_block(n: int, fill: int = 0x41) -> bytes:
    """one sequence of n literals: a compressed block that decodes to exactly n bytes"""
    out = bytearray()
    if n < 15:
        out.append(n << 4)
    else:
        out.append(0xF0)
        r = n - 15
        while r >= 255:
            out.append(255); r -= 255
        out.append(r)
    return bytes(out) + bytes([fill]) * n


def rle_block(n: int, fill: int = 0x42) -> bytes:
    """a short compressed block that decodes to n >= 25 bytes: 1 literal, one long match at offset 1, 5 literals at the end"""
    m = n - 1 - 5 - 4
    assert m >= 15
    out = bytearray([0x1F, fill, 1, 0])
    r = m - 15
    while r >= 255:
        out.append(255); r -= 255
    out.append(r)
    out += bytes([0x50]) + bytes([fill]) * 5
    return bytes(out)


def valid_sources(lz4f=None, big=True):
    """[(name, source, content)]: one to three frames per source, every flag, all four block-size codes, short and raw middle
    blocks, liblz4's linked frames when lz4f (test_frame_layer.LZ4F) is given"""
    text = corpus.class_bytes("dickens", 700_000, 3).tobytes()
    xml = corpus.class_bytes("xml", 400_000, 4).tobytes()
    rnd = corpus.random_bytes(200_000, 5).tobytes()
    out = []
    k = 0
    for bid, bs in BLOCK_SIZES.items():
        for bsum, csum, clen in ((False, False, False), (True, True, True), (False, True, False), (True, False, False)):
            k += 1
            n = min(len(text), [3 * bs + 1234, 2 * bs, bs - 1, bs + 1][k % 4]) if (big or bs <= (256 << 10)) else 100_000
            c = text[k * 100:k * 100 + n]
            out.append((f"indep-b{bid}-{int(bsum)}{int(csum)}{int(clen)}", indep_frame(c, bs, bsum, csum, clen), c))
    # this project's writer with a BlockSize below 64 KiB and short writes: short middle blocks, raw blocks
    for j, (cut, raw_every) in enumerate(((10000, 0), (4096, 3), (65535, 2), (1, 0))):
        c = (xml[:150_000] if cut > 1 else xml[:300]) + rnd[:5000 * j]
        out.append((f"irregular-{cut}", indep_frame(c, K64, j % 2 == 0, True, j == 1, cut=cut, raw_every=raw_every), c))
    if lz4f is not None:
        for bid in (4, 5, 6, 7):
            for j, (cs, bsum, size) in enumerate(((False, False, False), (True, True, True), (True, False, False))):
                n = [300_000, 70_000, 65_536][j] if bid < 6 or not big else [700_000, 400_000, 70_000][j]
                c = (text + xml)[j * 77:j * 77 + n]
                out.append((f"linked-b{bid}-{j}", lz4f.compress(np.frombuffer(c, np.uint8), bid, True, cs, bsum, size), c))
            c = rnd[:100_000] + text[:100_000]
            out.append((f"linked-raw-b{bid}", lz4f.compress(np.frombuffer(c, np.uint8), bid, True, True, True, False), c))
    # chained frames by hand: raw blocks in between (Inject feeds the prefix)
    empty = frame_of([], [], b"", K64, True, True, True, 0)
    out.append(("empty", empty, b""))
    a, b, c3 = out[0], out[5], out[9]
    out.append(("two-frames", a[1] + b[1], a[2] + b[2]))
    out.append(("three-with-empty", b[1] + empty + c3[1], b[2] + c3[2]))
    out.append(("empty-first", empty + a[1], a[2]))
    if lz4f is not None:
        l1 = [s for s in out if s[0] == "linked-b4-1"][0]
        out.append(("linked-then-indep", l1[1] + a[1] + l1[1], l1[2] + a[2] + l1[2]))
    out.append(("no-source", b"", b""))
    return out


def quirk_sources():
    """[(name, source)] -- the reference's corner cases; the witness says what each read returns"""
    out = []
    c = corpus.class_bytes("dickens", 2 * K64, 8).tobytes()
    good = indep_frame(c, K64, True, True)
    # a bad EndMark (truncated away) and a bad content checksum: an exact-end read does not see them, the next read does
    bad_sum = bytearray(good); bad_sum[-1] ^= 0x10
    out.append(("bad-content-sum", bytes(bad_sum)))
    out.append(("no-endmark", good[:-8]))
    out.append(("half-endmark", good[:-6]))
    for chain in (False, True):
        tag = "chain" if chain else "indep"
        p1 = compress(c[:K64])
        # a raw block of stored length 0 between two blocks; a compressed block of nothing (one token 0x00)
        out.append((f"raw0-{tag}", frame_of([p1, b"", p1], [False, True, False], c[:K64] * 2, K64, chain, True, True)))
        out.append((f"empty-block-{tag}", frame_of([p1, b"\x00", p1], [False, False, False], c[:K64] * 2, K64, chain, False, True)))
        # blocks that decode to blockSize + 1 .. + 8: LZ4BlockDecoder's capacity takes them, LZ4ChainDecoder's does not
        for extra in (0, 1, 8, 9):
            blk = rle_block(K64 + extra)
            body = bytes([0x42]) * (K64 + extra)
            out.append((f"over{extra}-{tag}", frame_of([blk, p1], [False, False], body + c[:K64], K64, chain, False, True)))
        # a stored length above the block size (raw and compressed)
        out.append((f"oversized-raw-{tag}", frame_of([c[:K64 + 1]], [True], c[:K64 + 1], K64, chain)))
        out.append((f"oversized-stored-{tag}", frame_of([literal_block(K64)], [False], b"", K64, chain)))
        # chained: a match that reaches behind the 64 KiB window / behind the start of the frame
        if chain:
            far = bytes([0x10, 0x43, 0xFF, 0xFF, 0x50]) + b"12345"            # offset 65535 after 1 literal
            out.append(("far-match-no-history", frame_of([far], [False], b"", K64, True)))
            out.append(("far-match-short-history", frame_of([p1[:0] + compress(c[:60000]), far], [False, False], b"", K64, True)))
            out.append(("far-match-raw-history", frame_of([c[:K64], far], [True, False], b"", K64, True)))
            out.append(("far-match-65534", frame_of([c[:65534], far], [True, False], b"", K64, True)))
            out.append(("far-match-65533", frame_of([c[:65533], far], [True, False], b"", K64, True)))
    # trailing bytes after the last frame: 1 - 3 are EndOfStream, 4 and more a bad magic
    for t in (1, 2, 3, 4, 9):
        out.append((f"trailing-{t}", good + bytes([0x55]) * t))
    out.append(("only-3-bytes", good[:3]))
    return out


def structural_mutants(source: bytes, max_block=None):
    """[(name, mutant)]: every header byte, length words, checksum words, EndMark, truncation at every record boundary +- 1,
    trailing bytes, the dictionary bit (with a header checksum that holds)"""
    info = F.parse_frame(source)
    out = []

    def flip(pos, x=0x01):
        b = bytearray(source); b[pos] ^= x
        return bytes(b)
    hdr_end = info.block_off[0] - 4 if len(info.block_off) else None
    if hdr_end is None:
        hdr_end = source.index(struct.pack("<I", 0), 6)
    for pos in range(hdr_end):
        out.append((f"hdr{pos}", flip(pos)))
        out.append((f"hdr{pos}x80", flip(pos, 0x80)))
    out.append(("version", flip(4, 0x40)))                          # the one bit the reader's version test looks at
    bounds = [0, 4, 6, hdr_end]
    bsum = 4 if info.descriptor.BlockChecksum else 0
    for off, ln in zip(info.block_off, info.block_len):
        n = ln & 0x7FFFFFFF
        bounds += [off - 4, off, off + n, off + n + bsum]
        for k in range(4):
            out.append((f"len@{off - 4 + k}", flip(off - 4 + k)))
        out.append((f"len-raw-bit@{off - 4}", flip(off - 1, 0x80)))
        out.append((f"len-huge@{off - 4}", source[:off - 4] + struct.pack("<I", 0x7FFFFFF0) + source[off:]))
        if bsum:
            out.append((f"bsum@{off + n}", flip(off + n + 2)))
    end = len(source)
    tail = 4 + (4 if info.descriptor.ContentChecksum else 0)
    bounds += [end - tail, end - tail + 4, end]
    out.append(("endmark", flip(end - tail)))
    if info.descriptor.ContentChecksum:
        out.append(("csum", flip(end - 1, 0x40)))
    for b in sorted(set(bounds)):
        for d in (-1, 0, 1):
            if 0 <= b + d < end:
                out.append((f"cut@{b + d}", source[:b + d]))
    for t in (1, 3, 4, 7):
        out.append((f"trail{t}", source + bytes([0x04, 0x22, 0x4D, 0x18][:t] if t < 4 else b"\x01\x02\x03\x04\x05\x06\x07"[:t])))
    # the dictionary bit with a valid header checksum, with and without room for the id
    flg = source[4] | 0x01
    body = bytes([flg]) + source[5:hdr_end - 1] + b"\x01\x02\x03\x04"
    out.append(("dict", source[:4] + body + bytes([(x32(body) >> 8) & 0xFF]) + source[hdr_end:]))
    out.append(("dict-cut", source[:4] + body[:-2]))
    return out


def payload_mutants(source: bytes, rng, count=12):
    """[(name, mutant, first mutated block's index)]: one flipped payload byte each"""
    info = F.parse_frame(source)
    out = []
    for _ in range(count):
        k = int(rng.integers(0, len(info.block_off)))
        n = info.block_len[k] & 0x7FFFFFFF
        if n == 0:
            continue
        pos = info.block_off[k] + int(rng.integers(0, n))
        b = bytearray(source); b[pos] ^= 1 << int(rng.integers(0, 8))
        out.append((f"flip@{pos}", bytes(b), k))
    return out


def read_plan(rng, n, bs_of, calls=7, top=3 << 20, rest=None):
    """calls x n counts: 0, 1 - 15, B - 1, B, B + 1, 2B, up to `top`; -1 where a stream sits the call out; and which calls are
    interactive"""
    plan = []
    for k in range(calls):
        row = []
        for i in range(n):
            B = bs_of[i]
            pick = int(rng.integers(0, 10))
            row.append([0, int(rng.integers(1, 16)), B - 1, B, B + 1, 2 * B, int(rng.integers(1, top)), int(rng.integers(1, 200_000)),
                        -1, B + 8][pick])
        plan.append((np.array(row, np.int64), k % 3 == 2))
    for _ in range(4):                                             # the rest of the first frame, the next frames, the clean end
        plan.append((np.full(n, rest or top * 4, np.int64), False))
    plan.append((np.full(n, 17, np.int64), False))
    return plan


def check_reads(reader, sources, plan, names=None, max_block=4 << 20, loose_from=None):
    """drives `reader` (read(counts, interactive) -> [bytes | code | None]) and one WitnessReader per source through the plan and
    compares every call.  loose_from[i] = a byte count: stream i's bytes are compared only below that many content bytes (payload
    flips without block checksums), lengths and codes always.  Returns the witnesses."""
    from frame_reader_witness import WitnessReader
    wit = [WitnessReader(s, max_block) for s in sources]
    done = [0] * len(sources)
    for call, (counts, interactive) in enumerate(plan):
        got = reader.read(counts, interactive)
        for i, w in enumerate(wit):
            tag = (call, i, names[i] if names else None, int(counts[i]), interactive)
            if counts[i] < 0:
                assert got[i] is None, tag
                continue
            want = w.read(int(counts[i]), interactive)
            if isinstance(want, int):
                assert got[i] == want, (tag, want, got[i] if isinstance(got[i], int) else len(got[i]))
                continue
            assert not isinstance(got[i], int), (tag, got[i], len(want))
            assert len(got[i]) == len(want), (tag, len(got[i]), len(want))
            if loose_from is None or loose_from[i] is None:
                assert got[i] == want, tag
            else:
                keep = max(0, min(len(want), loose_from[i] - done[i]))
                assert got[i][:keep] == want[:keep], tag
            done[i] += len(want)
    return wit
