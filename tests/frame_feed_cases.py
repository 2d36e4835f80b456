"""What the fed frame reader's tests share, without a GPU and with one: the driver that turns raw fed calls into logical reads (a
READ that, while it comes back starved, is issued again with the count reduced by what it delivered and with the next piece), the
layout of a source's fields, and the ways of cutting a source into pieces.  Test infrastructure only."""
from __future__ import annotations

import bisect

import numpy as np

import frame_reader_cases as K
from k4os.compression.lz4_amd import frames as F

K64 = 65536
READ, OPEN = 0, 1


class FedDriver:
    """n fed readers behind `raw.call(op, pieces, final, counts, interactive) -> (outLen, [bytes], consumed, need)`, each over
    sources[i] cut at ends[i] (non-decreasing piece ends, the last one len(sources[i]); the last piece is the final one).  read() and
    open() are logical reads, so frame_reader_cases.check_reads compares them with a WitnessReader over the whole source.  Every raw
    call is held to the contract: a starved call consumed its whole piece and was not final, a call that is not starved consumed no
    more than it was given, an interactive read that starves has delivered nothing, a piece shorter than the reported need delivers
    nothing and leaves the rest of the need, and with field_end(i, u) -- the end of the field that holds source byte u -- need is
    field_end(i, upto) - upto."""

    def __init__(self, raw, sources, ends, field_end=None):
        self.raw, self.src, self.ends, self.field_end = raw, [bytes(s) for s in sources], [list(e) for e in ends], field_end
        self.n = len(self.src)
        for s, e in zip(self.src, self.ends):
            assert e and e[-1] == len(s) and all(a <= b for a, b in zip(e, e[1:])) and e[0] >= 0
        self.j = [0] * self.n               # the piece in hand
        self.pos = [0] * self.n             # source bytes consumed
        self.short = [None] * self.n        # what must be left of the need after a piece that was shorter than it
        self.calls = 0
        self.starved = []                   # (stream, upto, need) of every starved call
        self.code_at = [None] * self.n      # the source bytes handed over (upto) when a stream failed, and whether that piece was final
        self.code_final = [None] * self.n

    def _logical(self, op, counts, interactive):
        n = self.n
        remaining = [int(c) for c in counts]
        active = [c >= 0 for c in remaining]
        acc = [bytearray() for _ in range(n)]
        res = [None] * n
        while any(active):
            upto = [self.ends[i][self.j[i]] for i in range(n)]
            fin = [int(active[i] and self.j[i] == len(self.ends[i]) - 1) for i in range(n)]
            pieces = [self.src[i][self.pos[i]:upto[i]] if active[i] else b"" for i in range(n)]
            cnts = np.array([remaining[i] if active[i] else -1 for i in range(n)], np.int64)
            out, data, consumed, need = self.raw.call(op, pieces, np.array(fin, np.int64), cnts, interactive)
            self.calls += 1
            for i in range(n):
                tag = (self.calls, i, op, int(cnts[i]), upto[i], int(out[i]), int(consumed[i]), int(need[i]))
                if not active[i]:
                    assert (out[i], consumed[i], need[i]) == (0, 0, 0), tag
                    continue
                if out[i] < 0:
                    res[i] = int(out[i])
                    if self.code_at[i] is None:
                        self.code_at[i], self.code_final[i] = upto[i], bool(fin[i])
                    active[i] = False
                    continue
                assert 0 <= consumed[i] <= len(pieces[i]) and need[i] >= 0, tag
                if op == READ:
                    assert out[i] <= remaining[i] and len(data[i]) == out[i], tag
                    acc[i] += data[i]
                    remaining[i] -= int(out[i])
                self.pos[i] += int(consumed[i])
                if self.short[i] is not None:
                    assert out[i] == 0 and need[i] == self.short[i], (tag, self.short[i])
                    self.short[i] = None
                if need[i] > 0:
                    assert not fin[i] and consumed[i] == len(pieces[i]), tag
                    assert not (interactive and out[i]), tag
                    if op == OPEN:
                        assert out[i] == 0, tag
                    if self.field_end is not None:
                        assert need[i] == self.field_end(i, upto[i]) - upto[i], (tag, self.field_end(i, upto[i]))
                    self.starved.append((i, upto[i], int(need[i])))
                    self.j[i] += 1
                    more = self.ends[i][self.j[i]] - upto[i]
                    if more < need[i] and self.j[i] < len(self.ends[i]) - 1:
                        self.short[i] = int(need[i]) - more
                else:
                    active[i] = False
                    res[i] = bytes(acc[i]) if op == READ else int(out[i])
        return res

    def read(self, counts, interactive=False):
        return self._logical(READ, counts, interactive)

    def open(self, which=None):
        return self._logical(OPEN, [0 if which is None or i in which else -1 for i in range(self.n)], False)


def field_ends(source: bytes):
    """the ends of the fields of a valid source, in order: per frame the magic, FLG / BD, the rest of the header, then per block the
    length word and the payload plus its block checksum, the EndMark and the content checksum; behind the last frame the magic of a
    frame that might follow"""
    out, at = [], 0
    while at < len(source):
        info = F.parse_frame(source, at)
        d = info.descriptor
        out += [at + 4, at + 6, at + 6 + (8 if d.ContentLength is not None else 0) + 1]
        for off, lc in zip(info.block_off, info.block_len):
            out += [off, off + (lc & 0x7FFFFFFF) + (4 if d.BlockChecksum else 0)]
        out.append(out[-1] + 4)
        if d.ContentChecksum:
            out.append(out[-1] + 4)
        at += info.consumed
        assert out[-1] == at
    out.append(at + 4)
    return out


def field_end_fn(sources):
    tables = [field_ends(s) for s in sources]
    return lambda i, u: tables[i][bisect.bisect_right(tables[i], u)]


def small_source():
    """(source, content): two frames in a few hundred bytes with 64 KiB blocks -- block and content checksums and ContentLength in the
    first (a full block, a short block, a raw block), none in the second (a short block, a full block)"""
    text = K.corpus.class_bytes("dickens", 400, 9).tobytes()
    a_blocks = [(K.rle_block(K64, 0x61), False, bytes([0x61]) * K64), (K.compress(text[:150]), False, text[:150]), (text[150:190], True, text[150:190])]
    b_blocks = [(K.compress(text[200:290]), False, text[200:290]), (K.rle_block(K64, 0x62), False, bytes([0x62]) * K64)]
    ca, cb = b"".join(b[2] for b in a_blocks), b"".join(b[2] for b in b_blocks)
    a = K.frame_of([b[0] for b in a_blocks], [b[1] for b in a_blocks], ca, K64, False, True, True, len(ca))
    b = K.frame_of([b[0] for b in b_blocks], [b[1] for b in b_blocks], cb, K64, False, False, False)
    return a + b, ca + cb


def small_content_ends():
    """where the blocks of small_source() end in its content"""
    out, at = [], 0
    for n in (K64, 150, 40, 90, K64):
        at += n
        out.append(at)
    return out


def reads_to_the_end(source, count, n, near=None, block_ends=(), max_block=K64):
    """a plan for frame_reader_cases.check_reads over n streams of the same source: reads of `count` bytes until the source is at
    its end (a read ends at each EndMark) and two more.  near: content that lies more than `near` bytes from both ends of its block
    (block_ends: where the blocks end in the content) is crossed by one large read instead, so that the small reads cover every
    record boundary, EndMark and frame boundary without tens of thousands of calls through the middle of a 64 KiB block."""
    from frame_reader_witness import WitnessReader
    w = WitnessReader(source, max_block)
    plan, p = [], 0
    while True:
        c = count
        if near is not None:
            nxt = min((b for b in block_ends if b > p), default=p)
            prv = max((b for b in block_ends if b <= p), default=0)
            if p - prv >= near and nxt - p > near:
                c = nxt - near - p
        r = w.read(c)
        assert not isinstance(r, int)
        plan.append(c)
        p += len(r)
        if not r and w.pos == len(source) and w.phase == 0:
            break
    return [(np.full(n, c, np.int64), False) for c in plan + [count, count]]


class OpenMixer:
    """a reader for check_reads that puts an OpenFrame on a random subset of the streams in front of every third read and compares
    it with witnesses of its own, kept in step"""

    def __init__(self, drv, sources, rng, max_block=4 << 20):
        from frame_reader_witness import WitnessReader
        self.drv, self.rng, self.k = drv, rng, 0
        self.wit = [WitnessReader(s, max_block) for s in sources]

    def read(self, counts, interactive=False):
        self.k += 1
        if self.k % 3 == 1:
            which = set(int(i) for i in np.flatnonzero(self.rng.random(len(self.wit)) < 0.4))
            got = self.drv.open(which)
            assert got == [w.open() if i in which else None for i, w in enumerate(self.wit)], self.k
        for w, c in zip(self.wit, counts):
            if c >= 0:
                w.read(int(c), interactive)
        return self.drv.read(counts, interactive)


def check_code_timing(drv, wit, names=None):
    """defects come when their bytes do: a stream's code was reported no later than the call that handed over the piece holding the
    last byte the witness's reader had read when it failed; K4LZ4_FRAME_EOF only in the call with final"""
    for i, w in enumerate(wit):
        tag = (i, names[i] if names else None, w.failed, drv.code_at[i], w.pos)
        if w.failed is None:
            assert drv.code_at[i] is None, tag
            continue
        assert drv.code_at[i] is not None, tag
        if w.failed == -1:
            assert drv.code_final[i], tag
        else:
            e = drv.ends[i]
            assert drv.code_at[i] <= e[bisect.bisect_left(e, w.pos)], tag


def random_ends(rng, length, bs):
    """piece ends over a source of `length` bytes: pieces of 0, 1 - 15, around bs +- 8 and up to 3 bs bytes"""
    ends, at = [], 0
    while at < length:
        pick = int(rng.integers(0, 6))
        step = [0, int(rng.integers(1, 16)), int(rng.integers(1, 16)), bs + int(rng.integers(-8, 9)), int(rng.integers(1, 3 * bs + 1)),
                int(rng.integers(1, 3 * bs + 1))][pick]
        at = min(length, at + step)
        ends.append(at)
    if not ends or rng.random() < 0.3:
        ends.append(length)                               # an empty final piece
    return ends


def block_size_of(name):
    return K64 if not name.startswith(("indep-b", "linked-b")) else K.BLOCK_SIZES[int(name.split("-b")[1][0])]
