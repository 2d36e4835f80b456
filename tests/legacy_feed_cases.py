"""What the fed LZ4Stream reader's tests share, without a GPU and with one: the layout of a stream's fields, the driver that turns
raw fed calls into logical reads (frame_feed_cases.FedDriver through its raw.call / field_end interface), the comparison with
legacy_stream_witness.Reader over the WHOLE source, and the streams and cuts of the tests.  Test infrastructure only."""
from __future__ import annotations

import bisect

import numpy as np

from frame_feed_cases import FedDriver, random_ends          # noqa: F401  (random_ends: pieces of 0, 1-15, bs +- 8, up to 3 bs)
from legacy_stream_witness import Reader
from legacy_witness import Thrown
from k4os.compression.lz4_amd import corpus

READ, RESET = 0, 1
LSQ_POSITION, LSQ_BYTES_READ, LSQ_PENDING, LSQ_CODE, LSQ_CHUNKS, LSQ_DIRECT, LSQ_BATCHED, LSQ_HANDED_BACK = range(8)


def varint(v: int) -> bytes:
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def layout(stream: bytes):
    """the chunks of a well-formed stream: [(header start, payload start, C, U, flags)]"""
    out, pos = [], 0

    def vi():
        nonlocal pos
        v, s = 0, 0
        while True:
            b = stream[pos]
            pos += 1
            v |= (b & 0x7F) << s
            s += 7
            if not b & 0x80:
                return v
    while pos < len(stream):
        h = pos
        flags = vi()
        u = vi()
        c = vi() if flags & 1 else u
        out.append((h, pos, c, u, flags))
        pos += c
    assert pos == len(stream)
    return out


def field_ends(stream: bytes):
    """the ends of the fields of a well-formed stream, in order: every byte of a chunk header is a field of its own (the reference
    reads varints one byte at a time), then the payload; behind the last chunk the first byte of a header that might follow"""
    out = []
    for h, p, c, _, _ in layout(stream):
        out += list(range(h + 1, p + 1))
        if c:
            out.append(p + c)
    out.append(len(stream) + 1)
    return out


def field_end_fn(sources):
    """field_end(i, u): u + 1 inside or in front of a header, the payload's end inside a payload"""
    tables = [field_ends(s) for s in sources]
    return lambda i, u: tables[i][bisect.bisect_right(tables[i], u)]


class TrackedReader(Reader):
    """the witness's reader, remembering whether its last read of the inner stream came up short (END_OF_STREAM from running out)"""
    short_last = False

    def _inner_read(self, n):
        got = super()._inner_read(n)
        self.short_last = len(got) < n
        return got

    def call(self, count):
        try:
            return self.read(int(count))
        except Thrown as e:
            return e.code


def driver(raw, sources, ends, with_layout=True):
    return FedDriver(raw, sources, ends, field_end_fn(sources) if with_layout else None)


def check_reads(drv, w, sources, plan, interactive=False, max_block=None, names=None):
    """plan: [counts per stream] (negative / None: the stream sits the read out) -> every logical read equals ONE Read(count) of the
    witness over the whole source; returns the witnesses"""
    wit = [TrackedReader(w, s, interactive, max_block) for s in sources]
    for k, counts in enumerate(plan):
        counts = [-1 if c is None else int(c) for c in counts]
        got = drv.read(np.array(counts, np.int64), interactive)
        for i, c in enumerate(counts):
            if c < 0:
                assert got[i] is None, (k, i)
                continue
            want = wit[i].call(c)
            tag = (k, i, names[i] if names else None, c, got[i] if isinstance(got[i], int) else len(got[i]),
                   want if isinstance(want, int) else len(want))
            assert got[i] == want, tag
    return wit


def check_code_timing(drv, wit, names=None):
    """defects come when their bytes do: a stream's code was reported no later than the call that handed over the piece holding the
    last byte the witness's reader had consumed when it threw; END_OF_STREAM from running out only in the call with final"""
    for i, w in enumerate(wit):
        tag = (i, names[i] if names else None, w.failed, drv.code_at[i], w.pos)
        if w.failed is None:
            assert drv.code_at[i] is None, tag
            continue
        assert drv.code_at[i] is not None, tag
        if w.failed == -1 and w.short_last:
            assert drv.code_final[i], tag
        else:
            e = drv.ends[i]
            assert drv.code_at[i] <= e[bisect.bisect_left(e, w.pos)], tag


def check_query(q, wit, whole=None):
    """Query() against the witnesses after completed logical reads: the position, the bytes delivered, the pending bytes, the code,
    the chunks (whole: the words of whole-source readers that made the same reads)"""
    for i, w in enumerate(wit):
        if w.failed is None:
            got = tuple(int(x) for x in q[i, :5])
            assert got[LSQ_POSITION] == w.pos and got[LSQ_PENDING] == w.buffer_length - w.buffer_offset and got[LSQ_CODE] == 0, (i, got)
            assert got[LSQ_CHUNKS] == w.chunks, (i, got, w.chunks)
            if whole is not None:
                assert got == tuple(int(x) for x in whole[i, :5]), (i, got, whole[i, :5])
        else:
            assert int(q[i, LSQ_CODE]) == w.failed, (i, q[i])


def small_stream(w, B=300):
    """(stream, content): a compressed chunk, a stored chunk, a short chunk after a flush and an empty chunk, U of a full chunk a
    two-byte varint"""
    rng = np.random.default_rng(17)
    text = corpus.class_bytes("dickens", B, 9).tobytes()
    noise = rng.integers(0, 256, B, dtype=np.uint8).tobytes()
    short = corpus.lorem(40).tobytes()
    s = w.encode_stream(text + noise, False, B) + w.encode_stream(short, False, B) + varint(0) + varint(0) + \
        w.encode_stream(text[:120], False, B)
    lay = layout(s)
    assert [c[3] for c in lay] == [B, B, 40, 0, 120] and [c[4] & 1 for c in lay[:2]] == [1, 0] and lay[0][1] - lay[0][0] >= 4
    return s, text + noise + short + text[:120]


def reads_to_the_end(content_len, count):
    """counts of `count` bytes until the content is delivered, and two more"""
    return [count] * (-(-content_len // count) + 2)


def full_chunk_streams(w, n, k, B, seed=0, high=False):
    """n streams of k full chunks of B bytes each (compressible text, every chunk compressed)"""
    out = []
    for i in range(n):
        c = corpus.class_bytes(("dickens", "xml", "mozilla")[i % 3], k * B, seed + i).tobytes()
        s = w.encode_stream(c, high, B)
        assert len(layout(s)) == k
        out.append((s, c))
    return out


def ends_inside_chunks(stream, frac=1.5):
    """piece ends that each lie inside a chunk's payload, about `frac` chunks' compressed length apart; the last piece is final"""
    lay = layout(stream)
    step = max(1, int(frac * len(stream) / len(lay)))
    ends, at = [], step
    while at < len(stream):
        k = max(j for j, c in enumerate(lay) if c[0] <= at)
        h, p, c = lay[k][:3]
        if not p < at < p + c:                            # move the cut into this chunk's payload
            at = p + max(1, c // 2)
        if ends and at <= ends[-1]:
            at = ends[-1] + step
            continue
        ends.append(at)
        at += step
    return [e for e in ends if e < len(stream)] + [len(stream)]
