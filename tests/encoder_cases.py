"""The tight-output case set of the batch encoders, shared by the emulator run, the reference pins and the GPU tests
(tests/test_encoder_cases_host.py, tests/test_gpu_encoder_routes.py); test infrastructure, the encoders' twin of decoder_cases.py.

A *mode* is one way of calling the encoders, a *round* one set of flags of a mode (ROUNDS):
  fast        LZ4Codec.Encode below L03_HC    FLAG_RAW_RETURN (the LLxx-level returns: 0 = did not fit)
  fast-x32    the same                        FLAG_X32 (LZ4Codec's mapping: -1 = did not fit)
  fast-copy   the same                        FLAG_ALLOW_COPY (-srcLen and the raw bytes, or 0 where the reference throws)
  fast-seg    the same                        FLAG_SEGMENTS, and FLAG_SEGMENTS | FLAG_ALLOW_COPY
  hc3 hc9 opt10  LZ4Codec.Encode at L03_HC / L09_HC / L10_OPT     no flag, and FLAG_ALLOW_COPY
  pickle pickle-hc3  LZ4Pickler.Pickle (k4lz4_pickle_batch_device) at L00_FAST / L03_HC
  wrap        LZ4Wrapper.Wrap / WrapHC (k4lz4_wrap_batch_device): the round's "flags" is `high`
`build(mode, oracle)` makes, from fixed seeds, the mode's list of (block, capacity) with a tag per case: blocks at the sizes
where the kernels change behaviour, each under a ladder of capacities around r, the oracle's unlimited result -- so most slots
are REJECTED ones (the output did not fit).  `layout` puts the slots into ONE arena filled with 0xCD with GUARD bytes of its own
in front of and behind every slot (a capacity-0 slot is two adjoining guards; every block lies in the source buffer once);
`expect` runs the oracle slot by slot on a copy of that arena.  `check` holds any engine's (out_len, arena) to that: every
result, and ONE mask over the whole arena -- the accepted slots' bytes, the slack behind them, both guards of every slot, those
of rejected and of zero-capacity slots included.

What the mask leaves out is what include/k4lz4.h leaves undefined, never what an engine happened to do:
  * [off, off + cap) of a slot the oracle rejected (its bytes are undefined on failure);
  * where the engine cuts big blocks into segments (`cuts`: a context with segments on, on a round that uses them -- never
    the HC levels, K4LZ4_NO_SEGMENTS, ALLOW_COPY or the emulated one-kernel pickle) the slack behind the bytes of an accepted
    block that the plan may cut (srcLen >= SEG_MIN and cap >= srcLen - 1: "may write anywhere inside a block's slot before
    outLen is final"; in an envelope: up to the end of the encoder's slot);
  * of an envelope, what the encoder that works in place inside it leaves behind the envelope's end.  This is the one place
    where this set found the product short of "bytes beyond outLen are never modified on success": the pickle and wrap
    calls have no scratch buffer, they encode at +5 (wrap: +8) with capacity srcLen - 1 and close the envelope around the
    bytes afterwards.  The design stays (include/k4lz4.h now says so at both calls) and the mask is exactly what it costs: a
    block that shrank was written as C bytes at +5 and moved down to its header, so the bytes up to 5 + C are open (a wrap's
    header is always 8 bytes: none); one that did not shrink leaves its encoder's whole slot open, up to 4 + srcLen
    (7 + srcLen).  Beyond that the envelope's slot stays untouched, and that is compared."""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass, field

import numpy as np

import adversarial_blocks
from decoder_cases import FILL, GUARD
from k4os.compression.lz4_amd import corpus

FLAG_RAW, FLAG_NO_REORDER, FLAG_NO_SPLIT, FLAG_ALLOW_COPY, FLAG_X32, FLAG_SEGMENTS = 1, 4, 16, 64, 128, 256
MODES = ("fast", "fast-x32", "fast-copy", "fast-seg", "hc3", "hc9", "opt10", "pickle", "pickle-hc3", "wrap")
ROUNDS = {"fast": (FLAG_RAW,), "fast-x32": (FLAG_X32,), "fast-copy": (FLAG_ALLOW_COPY,), "fast-seg": (FLAG_SEGMENTS, FLAG_SEGMENTS | FLAG_ALLOW_COPY),
          "hc3": (0, FLAG_ALLOW_COPY), "hc9": (0, FLAG_ALLOW_COPY), "opt10": (0, FLAG_ALLOW_COPY), "pickle": (0,), "pickle-hc3": (0,), "wrap": (0, 1)}
LEVEL = {"hc3": 3, "hc9": 9, "opt10": 10, "pickle-hc3": 3}
CALL = {"pickle": "pickle", "pickle-hc3": "pickle", "wrap": "wrap"}        # every other mode: "encode"
ENVELOPE_HEAD = {"pickle": 5, "wrap": 8}
# the segment switches the contexts of fast-seg, pickle and wrap are made under (tests/test_gpu_configs_full.py uses the same)
SEG_ENV = {"K4LZ4_SEG_MIN": "70000", "K4LZ4_SEG_TARGET": "49152", "K4LZ4_SEG_WARM": "24576", "K4LZ4_SEG_DIV": "0"}
SEG_MIN = 70000
PARSE_MIN_LEN, LIMIT_64K = 128, 65547
UNWRITTEN = -12345
_u8p = C.POINTER(C.c_uint8)


def call_of(mode):
    return CALL.get(mode, "encode")


@dataclass
class CaseSet:
    mode: str
    blocks: list = field(default_factory=list)     # distinct blocks
    block_tag: list = field(default_factory=list)  # "edge", "text", "binary", "noise", "64k", "repeat", "ll-code", "ml-code", "search-limit", "dense", "big", "cut"
    cases: list = field(default_factory=list)      # (index into blocks, capacity)

    def add_block(self, block, tag):
        self.blocks.append(np.ascontiguousarray(block, dtype=np.uint8))
        self.block_tag.append(tag)
        return len(self.blocks) - 1

    @property
    def tags(self):
        return [self.block_tag[b] for b, _ in self.cases]

    def subset(self, idx):
        """the cases idx, over the blocks they use"""
        idx = [int(i) for i in idx]
        used = sorted({self.cases[i][0] for i in idx})
        new = {b: k for k, b in enumerate(used)}
        return CaseSet(self.mode, [self.blocks[b] for b in used], [self.block_tag[b] for b in used], [(new[self.cases[i][0]], self.cases[i][1]) for i in idx])


TEXT, BINARY, NOISE = "dickens", "ooffice", None


def _class(name, n, seed):
    return corpus.random_bytes(n, 7000 + seed) if name is None else corpus.class_bytes(name, n, seed)


def _blocks(mode):
    """(block, tag) of a mode, before its capacities"""
    envelope = call_of(mode) != "encode"
    out = []
    for k, n in enumerate((0, 1, 5, 12, 13, 14, 64, 127, 128, 129)):                     # 128: PARSE_MIN_LEN
        out.append((corpus.class_bytes(corpus.SILESIA_NAMES[k % 12], n, k) if n else np.zeros(0, np.uint8), "edge"))
    for name, tag in ((TEXT, "text"), (BINARY, "binary"), (NOISE, "noise")):
        for n in (300, 1000, 4096, 8192):
            out.append((_class(name, n, n), tag))
    for k, n in enumerate((65535, 65536, 65546)):                                         # two of each: the last sizes of the byU16 table
        out.append((_class(TEXT, n, 20 + k), "64k"))
        out.append((_class(("xml", "mr", NOISE)[k], n, 30 + k), "64k"))
    for n in (15, 33, 300, 5000, 65536):                                                  # long match-length codes
        out.append((corpus.repeated(0x41 + n % 7, n), "repeat"))
    rng = np.random.default_rng(61)
    for n in (14, 15, 16, 269, 270, 271, 524, 525, 526):                                  # literal-length codes 14 | 15 0 | 15 1, 15 254 | 15 255 0 | ...
        run = rng.integers(0, 256, n, dtype=np.uint8)
        out.append((np.concatenate([run, corpus.repeated(0x5A, 40)]), "ml-code"))          # ... in front of a match
        out.append((run, "ll-code"))                                                       # ... as the last literals
    out += [(b, "search-limit") for b in adversarial_blocks.search_limit_at_block_end()]
    out.append((adversarial_blocks.dense_four_byte_matches(128, 65546, 128), "dense"))
    if mode == "fast-seg":                                                                 # cut under SEG_ENV: text, text + noise + text, noise
        out.append((_class("samba", LIMIT_64K, 3), "big"))                                # the first block of k4_parse_seg_kernel's side, too short to cut
        text = _class(TEXT, 200000, 40)
        out.append((text[:70000], "cut"))
        out.append((text[:123457], "cut"))
        out.append((np.concatenate([text[:60000], corpus.random_bytes(50000, 41), text[60000:150000]]), "cut"))
        out.append((corpus.random_bytes(150001, 42), "cut"))
    elif envelope:
        out.append((_class("samba", LIMIT_64K, 3), "big"))                                # byU32 tables, not cut: 65547 and 68000
        out.append((_class("xml", 68000, 4), "big"))
        out.append((_class("samba", 70000, 5), "cut"))                                    # SEG_MIN itself
        out.append((_class(TEXT, 150000, 43), "cut"))                                     # one message that is cut under SEG_ENV
    else:
        for k, n in enumerate((LIMIT_64K, 70000, 150000)):                                # byU32 tables
            out.append((_class("samba", n, 3 + k), "big"))
    return out


def unlimited(mode, oracle, block):
    """r: what the mode's block encoder returns for the block with room for anything"""
    if block.size == 0 and mode != "fast":
        return 0
    if mode == "fast-x32":
        return oracle.compress_fast_x32(block)[0]
    if mode in LEVEL:
        return oracle.compress_hc(block, LEVEL[mode])[0]
    return oracle.compress_fast(block)[0]


def capacities(mode, oracle, block, rng):
    u = int(block.size)
    if call_of(mode) != "encode":
        h = ENVELOPE_HEAD[call_of(mode)]
        caps = [oracle.lib.k4o_pickle_bound(u) if h == 5 else 8 + u, h + u, h + u - 1, 0]     # the bound, the least accepted, one below, nothing
    else:
        r = unlimited(mode, oracle, block)
        caps = [oracle.compress_bound(u), r + 1, r, r - 1, r - 2, r - 3, r - 5, r - 8, r - 9, r - 13, r // 2, r // 3, 5, 2, 1, 0]
        caps += [int(rng.integers(0, r)) for _ in range(3)] if r > 0 else []
        if mode == "fast-seg":
            caps += [u, u - 1, u - 2]                                                      # the plan cuts a block only when cap >= U - 1
        if r >= u:                                                                         # did not shrink: U <= cap < r is "target too small" (0), never a raw copy
            caps += [u, u - 1]
    return sorted({int(c) for c in caps if c >= 0}, reverse=True)


def build(mode: str, oracle) -> CaseSet:
    if mode not in MODES:
        raise ValueError(mode)
    cs = CaseSet(mode)
    rng = np.random.default_rng(1000 + MODES.index(mode))
    for block, tag in _blocks(mode):
        b = cs.add_block(block, tag)
        for cap in capacities(mode, oracle, cs.blocks[b], rng):
            cs.cases.append((b, cap))
    return cs


@dataclass
class Layout:
    mode: str
    src: np.ndarray
    src_off: np.ndarray          # uint64
    src_len: np.ndarray          # int32
    arena: np.ndarray            # the fill
    dst_off: np.ndarray          # uint64
    dst_cap: np.ndarray          # int32
    block: np.ndarray            # per case: its block (an index into `blocks`)
    tags: list

    @property
    def n(self):
        return int(self.src_len.size)


def layout(cs: CaseSet, fill: int = FILL) -> Layout:
    lens = np.array([b.size for b in cs.blocks], np.int64)
    boff = np.concatenate(([0], np.cumsum(lens[:-1]))) if len(lens) else np.zeros(0, np.int64)
    src = np.concatenate(cs.blocks + [np.zeros(64, np.uint8)])
    which = np.array([b for b, _ in cs.cases], np.int64)
    caps = np.array([c for _, c in cs.cases], np.int64)
    doff = GUARD + np.concatenate(([0], np.cumsum(caps[:-1] + 2 * GUARD))) if len(caps) else np.zeros(0, np.int64)
    arena = np.full(int((caps + 2 * GUARD).sum()) + 16, fill, np.uint8)
    return Layout(cs.mode, src, boff[which].astype(np.uint64), lens[which].astype(np.int32), arena, doff.astype(np.uint64), caps.astype(np.int32), which, cs.tags)


@dataclass
class Expectation:
    want: np.ndarray             # out_len per case
    arena: np.ndarray
    rejected: np.ndarray         # bool per case: the output did not fit
    keep: np.ndarray             # bool over the arena: `comparable`


def _mask(size, starts, ends):
    edges = np.zeros(size + 1, np.int32)
    np.add.at(edges, np.asarray(starts, np.int64), 1)
    np.add.at(edges, np.asarray(ends, np.int64), -1)
    return np.cumsum(edges[:-1]) > 0


def cuts_by_default(mode, flags) -> bool:
    """does a default context (under SEG_ENV) cut this round's big blocks into segments?"""
    if call_of(mode) == "encode":
        return mode == "fast-seg" and bool(flags & FLAG_SEGMENTS) and not flags & FLAG_ALLOW_COPY
    return mode == "pickle" or (mode == "wrap" and not flags)


def comparable(lay: Layout, want, rejected, flags, loose_end=None, cuts=False) -> np.ndarray:
    """mask over the arena of what every engine must agree on with the oracle (the module's docstring says what is left out, and why)"""
    off, cap, u = lay.dst_off.astype(np.int64), lay.dst_cap.astype(np.int64), lay.src_len.astype(np.int64)
    starts, ends = [off[rejected]], [(off + cap)[rejected]]
    ok = ~rejected
    if call_of(lay.mode) != "encode":
        loose = ok & (u > 0)             # loose_end: per case, where the in-place encoder's bytes may end (relative to the slot)
        starts.append((off + want)[loose]); ends.append(np.maximum(off + want, off + np.minimum(cap, loose_end))[loose])
    elif cuts:
        loose = ok & (u >= SEG_MIN) & (cap >= u - 1)
        starts.append((off + np.abs(want))[loose]); ends.append((off + cap)[loose])
    return ~_mask(lay.arena.size, np.concatenate(starts), np.concatenate(ends))


def wrap_expected(oracle, block, high):
    """LZ4Wrapper.Wrap / WrapHC (LZ4Wrapper.cs): [u32 U][u32 C][LZ4Codec.Encode into U bytes], stored raw with C = U where that
    did not shrink; pinned to the transcription over the compiled reference (legacy_witness.Witness.wrap) by the host test"""
    u = int(block.size)
    if u == 0:
        return bytes(8)
    r, d = oracle.compress_hc(block, 9, u) if high else oracle.compress_fast(block, u)
    if r <= 0 or r >= u:
        return struct.pack("<II", u, u) + block.tobytes()
    return struct.pack("<II", u, r) + d[:r].tobytes()


def expect(lay: Layout, oracle, flags: int, lib=None, prefix: str = "k4o_", cuts=None) -> Expectation:
    """what an engine leaves when it encodes every case into its slot of a copy of the arena, by the returns of include/k4lz4.h.
    lib / prefix: another library with the oracle's raw entry points (the compiled reference: "k4ref_"), block modes only.
    cuts: whether the engine cuts big blocks into segments (None: as a default context does for the round)."""
    cuts = cuts_by_default(lay.mode, flags) if cuts is None else cuts
    arena = lay.arena.copy()
    want = np.zeros(lay.n, np.int32)
    rejected = np.zeros(lay.n, bool)
    lib = lib or oracle.lib
    mode, call = lay.mode, call_of(lay.mode)
    p = lambda addr: C.cast(addr, _u8p)
    base_s, base_d = lay.src.ctypes.data, arena.ctypes.data
    if call == "encode":
        fn = getattr(lib, prefix + ("compress_hc" if mode in LEVEL else "compress_fast_x32" if mode == "fast-x32" else "compress_fast"))
        fn.argtypes = [_u8p, _u8p, C.c_int, C.c_int, C.c_int]
        arg = LEVEL.get(mode, 1)
    envelopes = {}
    loose_end = np.zeros(lay.n, np.int64)
    for i in range(lay.n):
        so, n, do, cap = int(lay.src_off[i]), int(lay.src_len[i]), int(lay.dst_off[i]), int(lay.dst_cap[i])
        if call == "encode":
            raw = bool(flags & FLAG_RAW)
            ret = fn(p(base_s + so), p(base_d + do), n, cap, arg) if n > 0 or raw else 0
            rejected[i] = ret <= 0 and (n > 0 or raw)
            r = ret if raw else (0 if n <= 0 else (-1 if ret <= 0 else ret))            # LZ4Codec.cs:40-52
            if flags & FLAG_ALLOW_COPY:                                                  # LZ4EncoderBase.cs:66-88, as k4_allow_copy_kernel states it
                if n <= 0 or r <= 0:
                    r = 0
                elif r >= n:
                    if cap >= n:
                        arena[do:do + n] = lay.src[so:so + n]
                        r = -n
                    else:
                        r, rejected[i] = 0, True
            want[i] = r
            continue
        key = (int(lay.block[i]), flags)
        head = ENVELOPE_HEAD[call]
        if call == "pickle":
            if n <= 0:
                continue                                                                 # Pickle returns an empty array
            if key not in envelopes:
                envelopes[key] = np.frombuffer(oracle.pickle(lay.src[so:so + n], LEVEL.get(mode, 0), 0), np.uint8)
        elif key not in envelopes:
            envelopes[key] = np.frombuffer(wrap_expected(oracle, lay.src[so:so + n], bool(flags)), np.uint8)
        if cap < head + n:
            want[i], rejected[i] = -1, True
            continue
        e = envelopes[key]
        arena[do:do + e.size] = e
        want[i] = e.size
        stored_raw = int(e[0]) == 0 if call == "pickle" else bytes(e[0:4]) == bytes(e[4:8])
        if stored_raw or (cuts and n >= SEG_MIN):
            loose_end[i] = head - 1 + n
        elif call == "pickle":
            loose_end[i] = 5 + (e.size - 1 - (4 if int(e[0]) >> 6 == 3 else int(e[0]) >> 6))
        else:
            loose_end[i] = e.size
    return Expectation(want, arena, rejected, comparable(lay, want, rejected, flags, loose_end, cuts))


def describe(lay: Layout, i: int) -> str:
    return f"slot {i} ({lay.tags[i]}, block of {int(lay.src_len[i])} bytes, capacity {int(lay.dst_cap[i])})"


def check(lay: Layout, exp: Expectation, got, got_arena, what="", src_after=None):
    """the assertions of every run of a round, emulated or on the device: every out_len entry was written and is the oracle's;
    under `comparable` the arena is the oracle's -- the accepted bytes, the slack behind them inside the slot, both guards of every
    slot, rejected and zero-capacity ones included; the sources are what was uploaded.  A difference names the slot, its tag,
    block length and capacity, and the first differing offset relative to the slot: negative is the front guard, >= capacity the
    back guard."""
    got, got_arena = np.asarray(got), np.asarray(got_arena)
    assert got.shape == exp.want.shape and got_arena.shape == exp.arena.shape, (what, got.shape, got_arena.shape)
    unwritten = np.flatnonzero(got == UNWRITTEN)
    assert unwritten.size == 0, f"{what}: {unwritten.size} results were never written, first {describe(lay, int(unwritten[0]))}"
    bad = np.flatnonzero(got != exp.want)
    assert bad.size == 0, f"{what}: {bad.size} results differ, first {describe(lay, int(bad[0]))}: engine {got[bad[0]]} oracle {exp.want[bad[0]]}"
    diff = np.flatnonzero((got_arena != exp.arena) & exp.keep)
    if diff.size:
        at = int(diff[0])
        i = max(int(np.searchsorted(lay.dst_off.astype(np.int64) - GUARD, at, side="right")) - 1, 0)
        raise AssertionError(f"{what}: {diff.size} bytes differ from the oracle's arena, first in {describe(lay, i)}, result {exp.want[i]}, at offset "
                             f"{at - int(lay.dst_off[i])} of the slot: engine {got_arena[at]:#04x} oracle {exp.arena[at]:#04x}")
    if src_after is not None:
        assert np.array_equal(np.asarray(src_after), lay.src), f"{what}: the source buffer changed"


_prepared = {}


def prepared(mode: str, flags: int, oracle, cuts=None):
    """(cases, layout, expectation) of a round, made once per process and never changed"""
    cuts = cuts_by_default(mode, flags) if cuts is None else cuts
    if (mode, flags, cuts) not in _prepared:
        if (mode, None) not in _prepared:
            cs = build(mode, oracle)
            lay = layout(cs)
            for a in (lay.src, lay.arena):
                a.setflags(write=False)
            _prepared[(mode, None)] = (cs, lay)
        cs, lay = _prepared[(mode, None)]
        exp = expect(lay, oracle, flags, cuts=cuts)
        for a in (exp.want, exp.arena, exp.rejected, exp.keep):
            a.setflags(write=False)
        _prepared[(mode, flags, cuts)] = (cs, lay, exp)
    return _prepared[(mode, flags, cuts)]
