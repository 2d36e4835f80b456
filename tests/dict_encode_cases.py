"""The shared list of cases of the dictionary encoder (k4lz4_encode_dict_batch): calls, each a list of dictionaries and a list of
messages with their entry of that list and how their dstCap is chosen.  Built from `corpus` and fixed seeds, the smallest shapes
at which each rule of the usingExtDict arm can go wrong.  tests/tools/record_dict_goldens.py records what liblz4 makes of them
(tests/golden/dict_encode_cases.json); the emulator tests and the GPU tests run them.  Test infrastructure only.

A message's cap: "bound" = k4lz4_compress_bound(len), "exact" = the size of the block the witness writes with room to spare (the
bytes must still be the same), "minus1" = one less (the result must be -1).  The sizes come from the witness or from the goldens."""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import List

import numpy as np

from k4os.compression.lz4_amd import corpus

K64 = 65536
MESSAGE_LENGTHS = (0, 1, 12, 13, 64, 1024, 4096, 65536, 65547, 200000)     # 13 = MFLIMIT + 1; 65 547 = LZ4_64Klimit: byU32 on both sides
DICT_LENGTHS = (0, 7, 8, 9, 100, 4096, 65535, 65536, 70000)                # 8 = HASH_UNIT; at 70 000 only the last 64 KiB count

SEAM_DICTIONARY = b"q" * 100 + b"the quick brown fox jumps z"
SEAM_MESSAGE = b"ABCDEFGHIJKL" + b"zABCDEFGHIJKL" + b"0123456789abcdef" * 3
# encoded against an external dictionary the block starts like this; as a contiguous prefix it would start c9 41 42 .. 4c 0d 00 ff 01:
# there the backward extension of the match at the message's 13th byte runs into the dictionary's last byte ('z')
SEAM_BLOCK_START = bytes([0xd8]) + b"ABCDEFGHIJKL" + bytes([0x7a, 0x0d, 0x00, 0xff, 0x01])


@dataclass
class Call:
    name: str
    dicts: List[np.ndarray]
    msgs: List[np.ndarray] = field(default_factory=list)
    idx: List[int] = field(default_factory=list)
    caps: List[str] = field(default_factory=list)
    big: bool = False          # too many messages for the emulator; the GPU runs it

    def add(self, msg, d: int, cap: str = "bound"):
        self.msgs.append(np.ascontiguousarray(msg, np.uint8))
        self.idx.append(d)
        self.caps.append(cap)
        return self


def bound(n: int) -> int:
    return n + n // 255 + 16


def synthetic(name: str, n: int, seed: int) -> np.ndarray:
    """corpus.class_bytes' synthetic stand-in even where K4LZ4_CORPUS_DIR names real files: the goldens pin these bytes"""
    saved = os.environ.pop("K4LZ4_CORPUS_DIR", None)
    try:
        return corpus.class_bytes(name, n, seed)
    finally:
        if saved is not None:
            os.environ["K4LZ4_CORPUS_DIR"] = saved


def u8(b: bytes) -> np.ndarray:
    return np.frombuffer(b, np.uint8).copy()


def mix(dictionary: np.ndarray, fresh: np.ndarray, n: int, seed: int) -> np.ndarray:
    """n bytes: pieces of the dictionary (so that matches reach into it) between pieces the dictionary does not hold"""
    rng = np.random.default_rng(seed)
    out, have, at = [], 0, 0
    while have < n:
        k = int(rng.integers(5, 120))
        if dictionary.size >= 16 and rng.random() < 0.5:
            s = int(rng.integers(0, dictionary.size - 8))
            piece = dictionary[s:s + k]
        else:
            piece = fresh[at:at + k]
            at = (at + k) % max(fresh.size - 200, 1)
        out.append(piece)
        have += piece.size
    return np.concatenate(out)[:n].copy() if n else np.zeros(0, np.uint8)


def hash5(b: np.ndarray, p: int) -> int:
    """LZ4_hash5 of the eight bytes at b[p:] (little endian, 12 bits)"""
    v = int.from_bytes(bytes(b[p:p + 8]), "little")
    return (((v << 24) * 889523592379) & 0xFFFFFFFFFFFFFFFF) >> 52


def reference_table(dictionary: np.ndarray) -> np.ndarray:
    """LZ4_loadDict's table, written down from its definition: the last 64 KiB, every third position up to dictEnd - 8 in order, the
    index 65536 - (dictEnd - p); fewer than 8 bytes leave it empty"""
    tab = np.zeros(4096, np.uint32)
    if dictionary.size >= 8:
        kept = dictionary[-K64:]
        for p in range(0, kept.size - 8 + 1, 3):
            tab[hash5(kept, p)] = K64 - (kept.size - p)
    return tab


def build() -> List[Call]:
    calls: List[Call] = []
    text = synthetic("dickens", 400000, 3)
    xml = synthetic("xml", 200000, 3)
    noise = corpus.random_bytes(K64 + 70000, 11)

    # every message length against one 4 KiB dictionary of the same class
    c = Call("message_lengths", [text[:4096].copy()])
    for i, n in enumerate(MESSAGE_LENGTHS):
        c.add(mix(c.dicts[0], text[100000:], n, 100 + i), 0)
    calls.append(c)

    # every dictionary length, two messages each, interleaved among the dictionaries in one call; at 70 000 the kept part starts
    # at 4464: one message begins with the dictionary's bytes from just behind that start (candidates with the smallest indices:
    # only a position q < k of the message is within 65 535 of kept offset k, so its backward extension ends at the message's
    # first byte before it could reach the kept start), one with the 30 bytes in front of the kept start, which nothing may match
    c = Call("dictionary_lengths", [xml[1000:1000 + n].copy() for n in DICT_LENGTHS])
    for rnd in range(2):
        for d, n in enumerate(DICT_LENGTHS):
            c.add(mix(c.dicts[d], xml[120000:], 13 if rnd else 1024, 200 + d), d)
    long_d = c.dicts[DICT_LENGTHS.index(70000)]
    ks = 70000 - K64
    c.add(np.concatenate([long_d[ks + 3:ks + 400], xml[150000:150100]]), DICT_LENGTHS.index(70000))
    c.add(np.concatenate([long_d[ks - 30:ks + 300], xml[150000:150100]]), DICT_LENGTHS.index(70000))
    c.add(np.concatenate([xml[150000:150040], long_d[ks - 30:ks + 300]]), DICT_LENGTHS.index(70000))
    full = c.dicts[DICT_LENGTHS.index(65536)]
    c.add(np.concatenate([full[3:300], xml[150000:150100]]), DICT_LENGTHS.index(65536))
    calls.append(c)

    # the seam, pinned literally; and a match that starts in the dictionary, runs through dictEnd and goes on against the message's start
    c = Call("seam", [u8(SEAM_DICTIONARY), text[:4096].copy(), text[:100].copy()])
    c.add(u8(SEAM_MESSAGE), 0)
    c.add(np.tile(c.dicts[1][-40:], 5), 1)
    c.add(np.tile(c.dicts[2][-40:], 5), 2)
    c.add(np.concatenate([c.dicts[1][-40:], c.dicts[1][-40:-8], text[200000:200050]]), 1)
    calls.append(c)

    # a full dictionary and a message of noise that repeats dictionary bytes: a candidate at distance 65 535 (kept offset k = q + 1:
    # usable) and at 65 536 (k = q: refused).  A full dictionary puts five positions on every slot and the last one stays, so the
    # dictionary's tail is one short pattern: the noise in front of it keeps its slots (checked here with reference_table)
    d = np.concatenate([noise[:8000], np.tile(u8(b"0123456789ab"), K64 // 12 + 1)])[:K64].copy()
    tab = reference_table(d)
    alive = [k for k in range(21, 4000, 3) if tab[hash5(d, k)] == k]
    k1 = alive[0]
    k2 = next(k for k in alive if k > k1 + 64)
    k3 = next(k for k in alive if k > k2 + 64)
    m = noise[K64:K64 + 4096].copy()
    m[k1 - 1:k1 + 15] = d[k1:k1 + 16]          # distance 65 535
    m[k2:k2 + 16] = d[k2:k2 + 16]              # distance 65 536
    m[k3 - 3:k3 + 37] = d[k3:k3 + 40]          # distance 65 533
    m[3900:3940] = d[7000:7040]                # a kept offset far beyond its position
    calls.append(Call("distance_limits", [d]).add(m, 0))

    # a short dictionary: dictSmall.  The message repeats itself, so "test next position" runs on slots the dictionary left empty or stale
    d = u8(bytes(corpus.lorem(100)))
    m = np.concatenate([corpus.lorem(700), d[10:90], corpus.lorem(700)[200:], d[:60], np.tile(u8(b"abcdefgh01234567"), 20)])
    c = Call("dict_small", [d, text[:9].copy(), np.zeros(0, np.uint8)])
    c.add(m, 0).add(m[:500], 1).add(m[:500], 2).add(np.concatenate([text[:9], text[:9], m[:100]]), 1)
    calls.append(c)

    # incompressible, all-zero and lorem messages; the dictionary ends in zeros, so the zero run starts in it and crosses the seam
    d = np.concatenate([corpus.lorem(4000), np.zeros(96, np.uint8)])
    c = Call("content_kinds", [d])
    c.add(corpus.random_bytes(1024, 5), 0).add(np.zeros(4096, np.uint8), 0).add(corpus.lorem(3000), 0).add(np.zeros(13, np.uint8), 0)
    c.add(corpus.random_bytes(300, 6), 0)
    calls.append(c)

    # dstCap exactly the witness's size (same bytes) and one less (-1)
    d = text[:4096].copy()
    c = Call("caps", [d, u8(SEAM_DICTIONARY)])
    for cap in ("exact", "minus1"):
        c.add(mix(d, text[100000:], 1024, 300), 0, cap)
        c.add(u8(SEAM_MESSAGE), 1, cap)
        c.add(mix(d, text[100000:], 13, 301), 0, cap)
        c.add(corpus.random_bytes(1024, 7), 0, cap)
        c.add(mix(d, text[100000:], 12, 302), 0, cap)
        c.add(np.tile(d[-40:], 40), 0, cap)
    calls.append(c)

    # several dictionaries, the messages interleaved among them (two entries of the list are the same bytes: one table)
    dicts = [text[:K64].copy(), xml[:20000].copy(), text[:K64].copy(), synthetic("osdb", 3000, 3)]
    c = Call("interleaved", dicts)
    fresh = [text[150000:], xml[100000:], text[250000:], synthetic("osdb", 60000, 4)]
    for i in range(24):
        k = i % 4
        c.add(mix(dicts[k], fresh[k], (1024, 4096, 700, 33)[(i // 4) % 4], 400 + i), k)
    calls.append(c)

    calls.append(Call("no_messages", [text[:500].copy()]))
    calls.append(Call("nothing", []))

    # more messages than the chip has wave slots (256 CUs x 8): the ticket hands out a second round
    d = text[:K64].copy()
    c = Call("ticket_rounds", [d], big=True)
    rng = np.random.default_rng(12)
    for i in range(4096):
        s = int(rng.integers(0, 300000))
        m = text[s:s + 1024].copy()
        k = int(rng.integers(0, K64 - 200))
        m[400:560] = d[k:k + 160]
        c.add(m, 0)
    calls.append(c)
    return calls


_calls = None


def calls() -> List[Call]:
    """the list, built once; nobody changes it"""
    global _calls
    if _calls is None:
        _calls = build()
    return _calls


def pack(call: Call, sizes=None, guard: int = 16):
    """(src, srcOff, srcLen, dstCap, dstOff, arena size, dictIdx, dict, dictOff, dictLen) for one call.  sizes: the witness's block
    sizes per message, needed where a cap is "exact" or "minus1".  The arena's slots lie `guard` bytes apart."""
    n = len(call.msgs)
    src_len = np.array([m.size for m in call.msgs], np.int32)
    src_off = np.zeros(n, np.uint64)
    if n > 1:
        src_off[1:] = np.cumsum(src_len[:-1].astype(np.uint64))
    src = np.concatenate(call.msgs + [np.zeros(16, np.uint8)]) if n else np.zeros(16, np.uint8)
    cap = np.zeros(n, np.int32)
    for i, how in enumerate(call.caps):
        cap[i] = bound(int(src_len[i])) if how == "bound" else int(sizes[i]) - (how == "minus1")
    dst_off = np.zeros(n, np.uint64)
    at = guard
    for i in range(n):
        dst_off[i] = at
        at += int(cap[i]) + guard
    dict_len = np.array([d.size for d in call.dicts], np.int32)
    dict_off = np.zeros(len(call.dicts), np.uint64)
    if len(call.dicts) > 1:
        dict_off[1:] = np.cumsum(dict_len[:-1].astype(np.uint64))
    dct = np.concatenate(call.dicts + [np.zeros(0, np.uint8)]) if call.dicts else np.zeros(0, np.uint8)
    return src, src_off, src_len, cap, dst_off, at + 16, np.array(call.idx, np.int32), np.ascontiguousarray(dct), dict_off, dict_len
