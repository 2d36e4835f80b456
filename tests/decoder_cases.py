"""The hostile-input case set of the batch decoders, shared by the emulator run, the host pins and the GPU tests
(tests/test_decoder_cases_host.py, tests/test_gpu_decoder_variants.py); test infrastructure, like stream_cases.py.

A *mode* is one way of calling the decoder kernels:
  plain     LZ4_decompress_safe                  (FLAG_RAW_RETURN)
  partial   LZ4_decompress_safe_partial          (FLAG_PARTIAL | FLAG_RAW_RETURN, capacity = bytes wanted)
  dict      LZ4_decompress_safe_usingDict        (FLAG_RAW_RETURN; external dictionaries and prefix placement)
  unpickle  LZ4Pickler.Unpickle                  (capacity = what the envelope's header claims, as a caller sizes it)
`build(mode, oracle, syslz4)` makes, from fixed seeds, the mode's list of (stream, capacity, extra) -- extra is None or
(dictionary, "ext" | "prefix") -- with a tag per case; `layout` puts them into ONE arena filled with 0xCD with GUARD bytes in
front of and behind every slot (a prefix dictionary lies directly in front of its slot, behind the guard; the external
dictionaries lie behind the last slot, each between guards) and `expect` runs an engine (the oracle, or the compiled reference:
the same entry points under another prefix) slot by slot on a copy of that arena.  Streams whose output the reference leaves
undefined (a match at offset 0, a prefix match that reaches in front of a 65 535-byte dictionary) are therefore defined here: by
the fill."""
from __future__ import annotations

import ctypes as C
import os
import struct
from dataclasses import dataclass, field

import numpy as np

from k4os.compression.lz4_amd import corpus
from stream_cases import long_field_streams

GUARD = 32
FILL = 0xCD
MODES = ("plain", "partial", "dict", "unpickle")
FLAG_RAW, FLAG_PARTIAL = 1, 32
FLAGS = {"plain": FLAG_RAW, "partial": FLAG_RAW | FLAG_PARTIAL, "dict": FLAG_RAW, "unpickle": 0}
LONG_SEQUENCES = 4 * 64            # four pipe slots of 64 sequences: a stream beyond this wraps the pair kernels' queue
MUTATIONS = ("truncated", "overwritten", "appended", "small-capacity")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_u8p = C.POINTER(C.c_uint8)


@dataclass
class CaseSet:
    mode: str
    cases: list = field(default_factory=list)      # (stream, capacity, extra)
    tags: list = field(default_factory=list)       # "valid", one of MUTATIONS, "soup", "long-field", "golden", ...

    def add(self, stream, cap, tag, extra=None):
        self.cases.append((np.ascontiguousarray(stream, dtype=np.uint8), int(cap), extra))
        self.tags.append(tag)

    @property
    def mutant(self):
        return np.array([t in MUTATIONS for t in self.tags], bool)

    def subset(self, idx):
        idx = [int(i) for i in idx]
        return CaseSet(self.mode, [self.cases[i] for i in idx], [self.tags[i] for i in idx])

    def tiled(self, times):
        return CaseSet(self.mode, self.cases * times, self.tags * times)


def sequences_parsed(stream: np.ndarray) -> int:
    """sequences a decoder walks before the stream ends or stops making sense (token chain of LL64.dec.cs:175-336, no copying)"""
    s = stream.tobytes()
    i, end, n = 0, len(s), 0
    while i < end:
        t = s[i]; i += 1; n += 1
        ll = t >> 4
        if ll == 15:
            while True:
                if i >= end: return n
                x = s[i]; i += 1; ll += x
                if x != 255: break
        i += ll
        if i + 2 > end: return n
        i += 2
        if (t & 15) == 15:
            while True:
                if i >= end: return n
                x = s[i]; i += 1
                if x != 255: break
    return n


def mutate(good: np.ndarray, true_size: int, count: int, rng):
    """the suite's mutation recipe (test_batch_malformed_streams_raw_returns): the four classes in turn; capacities vary by
    -20 .. +20 around the true size except in the last class, which keeps the stream and shrinks the capacity"""
    out = []
    for t in range(count):
        bad = good.copy()
        k = t % 4
        if k == 0:
            bad = bad[:rng.integers(1, good.size)]
        elif k == 1:
            for _ in range(int(rng.integers(1, 4))):
                bad[rng.integers(0, good.size)] = rng.integers(0, 256)
        elif k == 2:
            bad = np.concatenate([bad, rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8)])
        cap = true_size + int(rng.integers(-20, 21)) if k != 3 else int(rng.integers(0, true_size))
        out.append((bad, max(cap, 0), MUTATIONS[k]))
    return out


EDGE_SIZES = (0, 1, 5, 12, 13, 14, 65535, 65536, 65546, 65547)     # test_batch_ragged_and_empty
SMALL_SOURCES = (("dickens", 1900), ("xml", 6000), ("mr", 600))
LONG_SOURCES = (("mr", 66000), ("dickens", 24000))


def _plain_streams(oracle):
    """(stream, capacity, tag, true size) of the plain mode; the true size is what the partial mode's targets are placed around"""
    rng = np.random.default_rng(31)
    out = []
    for i, s in enumerate(EDGE_SIZES):
        b = corpus.class_bytes(corpus.SILESIA_NAMES[i % 12], s, i) if s else np.zeros(0, np.uint8)
        c = np.frombuffer(oracle.encode(b), np.uint8) if s else np.zeros(0, np.uint8)
        out.append((c, s, "valid", s))
        out.append((c, s + 9, "valid", s))
    for c, cap, _defined in long_field_streams(oracle, np.random.default_rng(77)):
        out.append((c, cap, "long-field", cap))
    soup = np.random.default_rng(43)                                  # test_decode_hostile_streams_random
    good = np.frombuffer(oracle.encode(corpus.class_bytes("xml", 20000, 1)), np.uint8)
    for t in range(300):
        if t % 3 == 0:
            c = soup.integers(0, 256, int(soup.integers(1, 400)), dtype=np.uint8)
        else:
            c = good[:int(soup.integers(20, good.size))].copy()
            for _ in range(int(soup.integers(1, 30))):
                c[soup.integers(0, c.size)] = soup.integers(0, 256)
        cap = int(soup.integers(0, 25000))
        out.append((c, cap, "soup", cap))
    out.append((np.load(os.path.join(GOLDEN, "mutated_stream_offset0_in_shortcut.npy")), 5813, "golden", 5813))
    for name, n in SMALL_SOURCES:
        data = corpus.class_bytes(name, n, 4)
        good = np.frombuffer(oracle.encode(data), np.uint8)
        out.append((good, n, "valid", n))
        out += [(c, cap, tag, n) for c, cap, tag in mutate(good, n, 400, rng)]
    for name, n in LONG_SOURCES:                                      # long enough to wrap the pipe's slots before the damage
        data = corpus.class_bytes(name, n, 4)
        good = np.frombuffer(oracle.encode(data), np.uint8)
        out.append((good, n, "valid", n))
        out += [(c, cap, tag, n) for c, cap, tag in mutate(good, n, 40, rng)]
    return out


def _build_plain(oracle, cs):
    for c, cap, tag, _ in _plain_streams(oracle):
        cs.add(c, cap, tag)


def _build_partial(oracle, cs):
    rng = np.random.default_rng(53)
    for c, _cap, tag, n in _plain_streams(oracle):
        targets = (0, 1, 7, 64, 65, max(n - 1, 0), n, n + 1)
        if tag == "valid":
            for t in targets:
                cs.add(c, t, tag)
        else:                                                          # two per hostile stream: one of the list, one in the back half
            cs.add(c, targets[int(rng.integers(0, 8))], tag)           # (a small target ends before most of the damage)
            cs.add(c, int(rng.integers(n // 2, n + 20)), tag)


def issue64_records():
    raw = open(os.path.join(GOLDEN, "issue64_input.bin"), "rb").read()
    want = np.frombuffer(open(os.path.join(GOLDEN, "issue64_output.bin"), "rb").read(), np.uint8)
    pos, recs = 20, []
    while raw[pos:pos + 4] == b"bv41":
        u, c = struct.unpack_from("<II", raw, pos + 4)
        recs.append((u, np.frombuffer(raw[pos + 12:pos + 12 + c], np.uint8)))
        pos += 12 + c
    return recs, want


DICT_LENGTHS = (0, 1, 100, 65535, 65536, 70000)


def repoint_into_dictionary(stream: np.ndarray, size: int) -> np.ndarray:
    """a valid block of `size` bytes made to need a dictionary, without an encoder: if the dictionary is the block's own content,
    the bytes a match at offset o copies also lie o + size back, wholly inside the dictionary (the match ends before the block
    does).  Every second match whose offset allows it is given that offset; lengths, and so the stream's layout, stay."""
    e = bytearray(stream.tobytes())
    i, k = 0, 0
    while i < len(e):
        t = e[i]; i += 1
        ll = t >> 4
        if ll == 15:
            while True:
                x = e[i]; i += 1; ll += x
                if x != 255: break
        i += ll
        if i >= len(e): break
        o = e[i] | (e[i + 1] << 8)
        if o + size <= 65535 and k % 2 == 0:
            e[i], e[i + 1] = (o + size) & 255, (o + size) >> 8
        k += 1
        i += 2
        if (t & 15) == 15:
            while e[i] == 255: i += 1
            i += 1
    return np.frombuffer(bytes(e), np.uint8)


def _build_dict(oracle, cs, syslz4):
    """streams that need their dictionary: issue64's chained record in any case, liblz4-made ones (LZ4_loadDict +
    LZ4_compress_fast_continue) where liblz4 is present; every dictionary length of DICT_LENGTHS, the dictionary with its first
    byte dropped, both placements, and the four mutation classes over those streams"""
    rng = np.random.default_rng(9)
    recs, want = issue64_records()
    u0 = recs[0][0]
    u1, c1 = recs[1]
    d0 = want[:u0].copy()
    both = ("ext", "prefix")
    dicts = [d0[d0.size - n:] if n <= d0.size else np.concatenate([corpus.random_bytes(n - d0.size, 5), d0]) for n in DICT_LENGTHS]
    dicts += [d0[1:], d0[:-1]]
    for d in dicts:
        for place in both:
            cs.add(c1, u1, "valid", (d, place))
    for delta in (-2, -1, 1, 2, 40):
        for place in both:
            cs.add(c1, u1 + delta, "valid", (d0, place))
    # the bulk of issue64's mutants against ONE external dictionary (an arena holds it once), a few against prefixes of their own
    for c, cap, tag in mutate(c1, u1, 640, rng):
        cs.add(c, cap, tag, (d0, "ext"))
    for c, cap, tag in mutate(c1, u1, 64, rng):
        cs.add(c, cap, tag, (d0, "prefix"))
    # many sequences, half of them reaching into the dictionary (which is the block's own content, see repoint_into_dictionary)
    for cls, n, count in (("xml", 6000, 160), ("dickens", 24000, 40)):
        data = corpus.class_bytes(cls, n, 4)
        c = repoint_into_dictionary(np.frombuffer(oracle.encode(data), np.uint8), n)
        for place in both:
            cs.add(c, n, "valid", (data, place))
            cs.add(c, n, "valid", (data[1:], place))
            for m, cap, tag in mutate(c, n, count, rng):
                cs.add(m, cap, tag, (data, place))
    if syslz4 is None or not getattr(syslz4, "available", True):
        return
    for k, n_dict in enumerate(DICT_LENGTHS):
        cls = corpus.SILESIA_NAMES[k % 12]
        n = 6000 if k % 2 else 3000
        text = corpus.class_bytes(cls, n_dict + n, 4)
        dd, data = text[:n_dict].copy(), text[n_dict:].copy()
        c = syslz4.compress_with_dict(data, dd)
        for place in both:
            cs.add(c, n, "valid", (dd, place))
            cs.add(c, n - 1, "valid", (dd, place))
            cs.add(c, n + 7, "valid", (dd, place))
            cs.add(c, n, "valid", (dd[1:], place))
        ext_mutants, prefix_mutants = (80, 40) if n_dict <= 100 else (40, 8)
        for m, cap, tag in mutate(c, n, ext_mutants, rng):
            cs.add(m, cap, tag, (dd, "ext"))
        for m, cap, tag in mutate(c, n, prefix_mutants, rng):
            cs.add(m, cap, tag, (dd, "prefix"))
    # text that repeats its dictionary: most matches reach into it
    for cls, n_dict, n in (("xml", 3000, 6000), ("nci", 20000, 6000)):
        dd = corpus.class_bytes(cls, n_dict, 6)
        data = np.concatenate([dd[n_dict - n // 2:], corpus.class_bytes(cls, n // 2, 7)])
        c = syslz4.compress_with_dict(data, dd)
        for place in both:
            cs.add(c, n, "valid", (dd, place))
            for m, cap, tag in mutate(c, n, 60, rng):
                cs.add(m, cap, tag, (dd, place))


def claimed_size(p: np.ndarray) -> int:
    """what a caller sizes an envelope's target by (LZ4Pickler.unpickle.cs:131-148, as k4lz4_unpickle_size): the header's
    result length; a header that cannot be read or claims a negative or enormous length gets no room"""
    if p.size == 0 or (int(p[0]) & 7):
        return 0
    code = (int(p[0]) >> 6) & 3
    sod = 4 if code == 3 else code
    if p.size - 1 - sod < 0:
        return 0
    diff = int.from_bytes(p[1:1 + sod].tobytes(), "little")
    rl = (p.size - 1 - sod + diff) & 0xFFFFFFFF
    return rl if rl <= (1 << 20) else 0


def _build_unpickle(oracle, cs):
    msgs = [corpus.lorem(n) for n in (1, 10, 32, 200, 1337, 5000, 0x10000)] + [corpus.random_bytes(n, n) for n in (1, 200, 1337)]
    msgs += [corpus.class_bytes("xml", 6000, 2), corpus.class_bytes("dickens", 24000, 3), corpus.repeated(7, 70000)]
    for m in msgs:                                                     # valid pickles of both header rules; a target one byte off
        for writer in (0, 1):
            p = np.frombuffer(oracle.pickle(m, 0, writer), np.uint8)
            cs.add(p, m.size, "valid")
        cs.add(p, m.size + 1, "valid")
        cs.add(p, max(m.size - 1, 0), "valid")
    cs.add(np.zeros(0, np.uint8), 0, "valid")
    rng = np.random.default_rng(23)                                    # test_unpickle_corruption (emulator)
    base = np.frombuffer(oracle.pickle(corpus.lorem(5000)), np.uint8)
    for t in range(200):
        p = base.copy()
        k = t % 4
        if k == 0:
            p[0] = rng.integers(0, 256)
        elif k == 1:
            p = p[:rng.integers(0, p.size)]
        elif k == 2:
            p[rng.integers(0, p.size)] ^= 1 << rng.integers(0, 8)
        else:
            p = np.concatenate([p, rng.integers(0, 256, 3, dtype=np.uint8)])
        cs.add(p, claimed_size(p), ("overwritten", "truncated", "overwritten", "appended")[k])
    rng = np.random.default_rng(24)                                    # tests/tools/gpu_stress_all.py, envelopes_round
    for i in range(300):
        m = corpus.class_bytes(corpus.SILESIA_NAMES[i % 12], int(rng.integers(1, 9000)), i)
        e = np.frombuffer(oracle.pickle(m, 0, int(rng.integers(0, 2))), np.uint8).copy()
        hits = int(rng.integers(0, 3))
        for _ in range(hits):
            e[int(rng.integers(0, e.size))] = int(rng.integers(0, 256))
        cut = rng.random() < 0.1
        if cut:
            e = e[:int(rng.integers(1, e.size + 1))]
        cs.add(e, claimed_size(e), "truncated" if cut else ("overwritten" if hits else "valid"))
    rng = np.random.default_rng(25)                                    # the four mutation classes over envelopes' payloads
    for cls, n in SMALL_SOURCES + (("dickens", 24000),):
        m = corpus.class_bytes(cls, n, 4)
        good = np.frombuffer(oracle.pickle(m, 0, 0), np.uint8)
        for c, cap, tag in mutate(good, n, 240 if n <= 6000 else 40, rng):
            cs.add(c, cap if tag == "small-capacity" else claimed_size(c), tag)


def build(mode: str, oracle, syslz4=None) -> CaseSet:
    cs = CaseSet(mode)
    if mode == "plain":
        _build_plain(oracle, cs)
    elif mode == "partial":
        _build_partial(oracle, cs)
    elif mode == "dict":
        _build_dict(oracle, cs, syslz4)
    elif mode == "unpickle":
        _build_unpickle(oracle, cs)
    else:
        raise ValueError(mode)
    return cs


@dataclass
class Layout:
    mode: str
    src: np.ndarray
    src_off: np.ndarray          # uint64
    src_len: np.ndarray          # int32
    arena: np.ndarray            # the fill, with the dictionaries in place
    dst_off: np.ndarray          # uint64
    dst_cap: np.ndarray          # int32
    dict_off: np.ndarray         # uint64 (into the arena; dict mode only)
    dict_len: np.ndarray         # int32
    inside: np.ndarray           # bool over the arena: True inside some [slot, slot + capacity)

    @property
    def n(self):
        return int(self.src_len.size)

    def slot(self, i):
        a = int(self.dst_off[i])
        return a, a + int(self.dst_cap[i])


def layout(cs: CaseSet, fill: int = FILL) -> Layout:
    comps = [c for c, _, _ in cs.cases]
    lens = np.array([c.size for c in comps], np.int32)
    soff = np.zeros(len(comps), np.uint64)
    soff[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    src = np.concatenate(comps + [np.zeros(8, np.uint8)])
    n = len(comps)
    doff = np.zeros(n, np.uint64)
    dict_off, dict_len = np.zeros(n, np.uint64), np.zeros(n, np.int32)
    pos, placed = 0, []
    for i, (_, cap, extra) in enumerate(cs.cases):
        pos += GUARD
        if extra is not None and extra[1] == "prefix":
            placed.append((pos, extra[0]))
            dict_off[i], dict_len[i] = pos, extra[0].size
            pos += extra[0].size
        doff[i] = pos
        pos += cap
    pos += GUARD
    shared = {}
    for i, (_, _, extra) in enumerate(cs.cases):
        if extra is not None and extra[1] == "ext":
            d = extra[0]
            key = (d.__array_interface__["data"][0], d.size)
            if key not in shared:
                shared[key] = pos
                placed.append((pos, d))
                pos += d.size + GUARD
            dict_off[i], dict_len[i] = shared[key], d.size
    arena = np.full(pos + GUARD, fill, np.uint8)
    for at, d in placed:
        arena[at:at + d.size] = d
    caps = np.array([cap for _, cap, _ in cs.cases], np.int32)
    edges = np.zeros(arena.size + 1, np.int32)
    np.add.at(edges, doff.astype(np.int64), 1)
    np.add.at(edges, doff.astype(np.int64) + caps, -1)
    inside = np.cumsum(edges[:-1]) > 0
    return Layout(cs.mode, src, soff, lens, arena, doff, caps, dict_off, dict_len, inside)


def expect(lay: Layout, lib, prefix: str = "k4o_"):
    """(out_len, arena) an engine leaves when it decodes every case into its slot of a copy of the arena: lib is the oracle's
    library (prefix "k4o_") or the compiled reference's ("k4ref_"), whose raw entry points have the same shapes.  The envelope of
    the unpickle mode is the oracle's own (k4o_unpickle; the reference has no compiled LZ4Pickler.Unpickle)."""
    arena = lay.arena.copy()
    out = np.zeros(lay.n, np.int32)
    base_s, base_d = lay.src.ctypes.data, arena.ctypes.data
    p = lambda addr: C.cast(addr, _u8p)
    if lay.mode == "unpickle":
        fn = lib.k4o_unpickle
    else:
        fn = getattr(lib, prefix + {"plain": "decompress_safe", "partial": "decompress_safe_partial", "dict": "decompress_safe_using_dict"}[lay.mode])
    for i in range(lay.n):
        s, d = p(base_s + int(lay.src_off[i])), p(base_d + int(lay.dst_off[i]))
        n, cap = int(lay.src_len[i]), int(lay.dst_cap[i])
        if lay.mode == "plain":
            r = fn(s, d, n, cap)
        elif lay.mode == "partial":
            r = fn(s, d, n, cap, cap)
        elif lay.mode == "dict":
            r = fn(s, d, n, cap, p(base_d + int(lay.dict_off[i])), int(lay.dict_len[i]))
        else:
            r = fn(s, n, d, cap)
            r = r if r >= 0 else -1                                    # k4lz4_unpickle_batch: -1 where the reference throws
        out[i] = r
    return out, arena


def check(lay: Layout, want, want_arena, got, got_arena, what=""):
    """the assertions of every run of a mode, emulated or on the device: the engine's result for every stream (the error position
    of a rejected one included), its bytes for every accepted stream, the rest of an accepted stream's slot untouched
    (include/k4lz4.h: bytes beyond outLen are never modified on success), and -- one mask over the whole arena -- every byte outside
    all slots as it was uploaded: the fill in both guards of every slot, rejected streams included, and the dictionaries"""
    got, got_arena = np.asarray(got), np.asarray(got_arena)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} results differ, first stream {bad[0]}: kernel {got[bad[0]]} oracle {want[bad[0]]}"
    outside = ~lay.inside
    touched = np.flatnonzero(got_arena[outside] != lay.arena[outside])
    if touched.size:
        at = int(np.flatnonzero(outside)[touched[0]])
        i = int(np.searchsorted(lay.dst_off.astype(np.int64), at, side="right")) - 1
        raise AssertionError(f"{what}: {touched.size} bytes outside every slot changed, first at {at} (slot {i} is [{lay.slot(max(i, 0))}), result {want[max(i, 0)]})")
    for i in np.flatnonzero(want >= 0):
        a, b = lay.slot(i)
        n = int(want[i])
        assert np.array_equal(got_arena[a:a + n], want_arena[a:a + n]), f"{what}: stream {i}: bytes differ"
        assert (got_arena[a + n:b] == FILL).all(), f"{what}: stream {i}: bytes behind the {n} decoded ones changed"


def comparable(lay: Layout, want) -> np.ndarray:
    """mask over the arena of what two runs of the same cases must agree on: everything but the inside of rejected slots"""
    edges = np.zeros(lay.arena.size + 1, np.int32)
    rej = np.flatnonzero(want < 0)
    np.add.at(edges, lay.dst_off[rej].astype(np.int64), 1)
    np.add.at(edges, lay.dst_off[rej].astype(np.int64) + lay.dst_cap[rej], -1)
    return ~(np.cumsum(edges[:-1]) > 0)


_prepared = {}


def prepared(mode: str, oracle):
    """(cases, layout, the oracle's results, the oracle's arena) of a mode, made once per process and never changed"""
    if mode not in _prepared:
        from oracle_lib import SystemLZ4
        sysl = SystemLZ4()
        cs = build(mode, oracle, sysl if sysl.available else None)
        lay = layout(cs)
        want, want_arena = expect(lay, oracle.lib)
        for a in (lay.src, lay.arena, lay.inside, want, want_arena):
            a.setflags(write=False)
        _prepared[mode] = (cs, lay, want, want_arena)
    return _prepared[mode]
