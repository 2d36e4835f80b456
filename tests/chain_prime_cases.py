"""The shared list of cases of chained streams opened from a dictionary set (k4lz4_chain_encoder_open_dictset /
k4lz4_chain_decoder_open_dictset): per case the dictionary list a set is made of, the encoders' settings, each
stream's entry (-1: none) and, call by call, every stream's run of TopupAndEncode records.  Built from `corpus` and fixed seeds, the
smallest shapes at which each rule can go wrong.  tests/tools/record_chain_prime_goldens.py records what the witness makes of them
(tests/golden/chain_prime_cases.json); the emulator and GPU tests run them.  Test infrastructure only."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

import numpy as np

import chain_encoder_cases as CC
from dict_encode_cases import SEAM_DICTIONARY, SEAM_MESSAGE, mix, synthetic, u8

K1, K64 = 1024, 65536
# 8 = HASH_UNIT: below it the fast family is empty; 4 = the HC insert limit; 65535 / 65536 flip dictSmall; at 70000 only the last 64 KiB count
DICT_LENGTHS = (0, 1, 3, 4, 7, 8, 9, 100, 4096, 65535, 65536, 70000)
LEVELS = (0, 3, 9, 12)
CONTENT = 140000
SHORT_CONTENT = 8000
# the seam message behind its dictionary as a contiguous prefix: the match at the message's 13th byte extends backwards into the
# dictionary's last byte ('z'), so the token carries 12 literals, not 13 (dict_encode_cases.SEAM_BLOCK_START is the external arm)
SEAM_PREFIX_START = bytes([0xc9]) + b"ABCDEFGHIJKL" + bytes([0x0d, 0x00, 0xff, 0x01])


@dataclass
class Case:
    name: str
    dict_buf: np.ndarray                       # the buffer a set is made of
    dict_off: np.ndarray                       # uint64 per entry
    dict_len: np.ndarray                       # int32 per entry
    settings: List[tuple] = field(default_factory=list)     # (chaining, level, blockSize, extraBlocks) per stream
    idx: List[int] = field(default_factory=list)            # per stream: its entry, -1: none
    contents: List[np.ndarray] = field(default_factory=list)
    calls: List[list] = field(default_factory=list)         # calls[c][s]: records (bytes, force, allowCopy)

    def dictionary(self, e: int) -> np.ndarray:
        return self.dict_buf[int(self.dict_off[e]):int(self.dict_off[e]) + int(self.dict_len[e])]

    def dictionary_of(self, s: int):
        return None if self.idx[s] < 0 else self.dictionary(self.idx[s])

    def add(self, setting, e: int, content: np.ndarray, per_call: list):
        if not self.calls:
            self.calls = [[] for _ in per_call]
        assert len(per_call) == len(self.calls)
        self.settings.append(setting); self.idx.append(e); self.contents.append(content)
        for c, recs in zip(self.calls, per_call):
            c.append(recs)
        return self


def opened_streams(case: Case) -> List[int]:
    """the streams the library opens: a chained stream at a level from 10 on (the optimal parser) is refused with a dictionary
     -- the witness and the goldens keep those streams, the GPU tests assert the refusal"""
    return [s for s, (st, e) in enumerate(zip(case.settings, case.idx)) if not (e >= 0 and st[0] and st[1] >= 10)]


def subcase(case: Case, keep: List[int]) -> Case:
    c = Case(case.name, case.dict_buf, case.dict_off, case.dict_len)
    for s in keep:
        c.add(case.settings[s], case.idx[s], case.contents[s], [call[s] for call in case.calls])
    return c


def packed(name: str, dicts) -> Case:
    lens = np.array([d.size for d in dicts], np.int32)
    off = np.zeros(len(dicts), np.uint64)
    if len(dicts) > 1:
        off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    buf = np.concatenate(list(dicts) + [np.zeros(16, np.uint8)])
    return Case(name, np.ascontiguousarray(buf), off, lens)


def stream_records(data: np.ndarray, B: int, seed: int, n_calls: int = 3, p_force: float = 0.1):
    """the content offered in records of random length (some longer than the free room, some forced short), then a flush, cut over
    n_calls calls"""
    rng = np.random.default_rng(seed)
    pieces, left = [], data.size
    while left > 0:
        pieces.append(min(int(rng.integers(1, 3 * B)), left)); left -= pieces[-1]
    recs = CC.offer_all(data, B, pieces, rng, p_force=p_force)
    recs.append((data[:0], True, True))
    return CC.split_calls(recs, n_calls, rng)


def whole_blocks(data: np.ndarray, B: int, n_calls: int = 3):
    """one record per block, unforced, and a flush: for B = 64 KiB and 140 000 bytes three blocks, a call each"""
    recs = [(data[k:k + B], False, True) for k in range(0, data.size, B)] + [(data[:0], True, True)]
    cut = [[] for _ in range(n_calls)]
    for k, r in enumerate(recs):
        cut[min(k, n_calls - 1)].append(r)
    return cut


def lengths_case(name: str, B: int, extra: int, lengths, how, content: int = CONTENT, levels=LEVELS) -> Case:
    xml = synthetic("xml", 400000, 3)
    c = packed(name, [xml[1000:1000 + n].copy() for n in lengths])
    for e, n in enumerate(lengths):
        k = DICT_LENGTHS.index(n)                       # (the seeds follow the length, whichever lengths a case takes)
        data = mix(c.dictionary(e), xml[120000:], content, 500 + k)
        for level in levels:
            c.add((True, level, B, extra), e, data, how(data, B, 40 + k))
    return c


def first_records_case() -> Case:
    """right behind the dictionary: a FlushAndEncode with nothing loaded (no block), a forced block of 1 byte, one of 12 bytes (below 13
    bytes the fast and hash-chain parsers write literals only), a record longer than the free room; then the rest and a flush"""
    text = synthetic("dickens", 200000, 5)
    c = packed("first_records", [text[:4096].copy(), text[:K64].copy()])
    B = K1
    for e in range(2):
        d = c.dictionary(e)
        data = np.concatenate([d[100:101], d[200:212], mix(d, text[100000:], 6 * B, 600 + e)])
        e0 = data[:0]
        recs = [(e0, True, True), (data[0:1], True, True), (data[1:13], True, True), (data[13:13 + 3 * B], False, True)]
        pos = 13 + B                                                 # Topup took B of the 3 B offered
        while pos < data.size:
            recs.append((data[pos:pos + B], False, False)); pos += B
        recs.append((e0, True, True))
        for level in LEVELS:
            c.add((True, level, B, 0), e, data, [recs[:2], recs[2:5], recs[5:]])
    return c


def seam_case() -> Case:
    c = packed("seam", [u8(SEAM_DICTIONARY)])
    m = u8(SEAM_MESSAGE)
    for level in LEVELS:
        c.add((True, level, K1, 0), 0, m, [[(m, True, False)]])
    return c


def gain_dictionary() -> np.ndarray:
    return synthetic("dickens", 300000, 9)[100000:100000 + K64].copy()


def gain_case() -> Case:
    """a stream that begins with a 4 000-byte slice of its own 64 KiB dictionary, primed and not, at L00 and L03"""
    d = gain_dictionary()
    fresh = synthetic("dickens", 300000, 9)[200000:]
    data = np.concatenate([d[30000:34000], fresh[:96]])
    c = packed("gain", [d])
    recs = [[(data[k:k + K1], False, False) for k in range(0, 4 * K1, K1)]]
    for level in (0, 3):
        for e in (0, -1):
            c.add((True, level, K1, 0), e, data, recs)
    return c


def mixed_case(n_streams: int = 64, seed: int = 91) -> Case:
    """64 streams of mixed kinds opened and run together in three calls: independent encoders and some chained ones without a
    dictionary; a 70 000-byte entry and the 64 KiB it keeps as an entry of their own (same bytes: one table); one dictionary used by
    many streams"""
    rng = np.random.default_rng(seed)
    text = synthetic("dickens", 400000, 7)
    xml = synthetic("xml", 200000, 7)
    buf = np.concatenate([text[:70000], xml[:20000], text[300000:300005], np.zeros(16, np.uint8)])
    off = np.array([0, 70000 - K64, 70000, 90000, 90000], np.uint64)
    ln = np.array([70000, K64, 20000, 5, 0], np.int32)
    c = Case("mixed", np.ascontiguousarray(buf), off, ln)
    kinds = [(True, 0), (True, 3), (False, 0), (True, 9), (True, 1), (True, 12), (False, 3), (True, 10)]
    sizes = [(K1, 0), (4 * K1, 1), (K64, 0), (3 * K1, 2)]
    for s in range(n_streams):
        ch, lv = kinds[s % len(kinds)]
        B, ex = sizes[int(rng.integers(0, len(sizes)))]
        e = -1 if (not ch or s % 5 == 0) else (0 if s % 3 == 0 else int(rng.integers(0, 5)))
        total = (70 * K1 if B == K1 and s % 4 == 0 else int(rng.integers(2, 9)) * min(B, 8 * K1) // 2) + int(rng.integers(0, 17))
        src = xml[100000:] if e == 2 else text[150000:]
        data = mix(c.dictionary(e), src, total, seed + s) if e >= 0 else src[s * 100:s * 100 + total].copy()
        c.add((ch, lv, B, ex), e, data, stream_records(data, B, seed + s, p_force=0.15))
    return c


BUILDERS = {
    # every length and kind over a short content; the long geometries (the ring saves twice, first with the dictionary still in the
    # window) over the lengths where the window is full or nearly so
    "lengths_short": lambda: lengths_case("lengths_short", K1, 0, DICT_LENGTHS, stream_records, content=SHORT_CONTENT),
    "lengths_b1k": lambda: lengths_case("lengths_b1k", K1, 0, (4096, 70000), stream_records),
    "lengths_b1k_x2": lambda: lengths_case("lengths_b1k_x2", K1, 2, (9, 65536), stream_records, levels=(0, 9)),
    "lengths_b64k": lambda: lengths_case("lengths_b64k", K64, 0, (7, 4096, 65536, 70000), lambda data, B, seed: whole_blocks(data, B)),
    "first_records": first_records_case,
    "seam": seam_case,
    "gain": gain_case,
    "mixed": mixed_case,
}
NAMES = tuple(BUILDERS)
_built = {}


def case(name: str) -> Case:
    """the case, built once; nobody changes it"""
    if name not in _built:
        _built[name] = BUILDERS[name]()
    return _built[name]
