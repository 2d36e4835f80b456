"""The shared list of cases of the HC dictionary encoder (k4lz4_encode_dict_hc_batch): calls as in tests/dict_encode_cases.py (whose
Call, pack, mix, synthetic and seam constants are used here), each with the levels it runs at.  The smallest shapes at which each rule
of the external-dictionary arm of the hash-chain search can go wrong (DESIGN.md 4.21 numbers the rules).
tests/tools/record_dict_hc_goldens.py records what liblz4 makes of them (tests/golden/dict_hc_encode_cases.json); the emulator tests
and the GPU tests run them.  Test infrastructure only."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

import dict_encode_cases as DC
from dict_encode_cases import Call, K64, SEAM_DICTIONARY, SEAM_MESSAGE, mix, pack, synthetic, u8      # noqa: F401
from k4os.compression.lz4_amd import corpus

LEVELS = (3, 4, 6, 9)            # one record; a walk into a second record; a longer walk; pattern analysis
MESSAGE_LENGTHS = (0, 1, 12, 13, 64, 1024, 4096)
DICT_LENGTHS = (0, 3, 4, 5, 100, 4096, 65535, 65536, 70000)     # 4: the first length at which a position enters the chain
PERIODS = (1, 2, 3, 4)


@dataclass
class HcCall(Call):
    levels: Tuple[int, ...] = LEVELS


def pattern(period: int, n: int) -> np.ndarray:
    return np.tile(u8(b"abcd"[:period]), n // period + 1)[:n].copy()


def build() -> List[HcCall]:
    calls: List[HcCall] = []
    text = synthetic("dickens", 400000, 3)
    xml = synthetic("xml", 200000, 3)
    noise = corpus.random_bytes(K64 + 70000, 11)

    c = HcCall("message_lengths", [text[:4096].copy()])
    for i, n in enumerate(MESSAGE_LENGTHS):
        c.add(mix(c.dicts[0], text[100000:], n, 100 + i), 0)
    calls.append(c)

    # rule 4 and positions beyond 16 bits: the message outgrows the dictionary, whose pieces it keeps repeating
    c = HcCall("long_message", [text[:4096].copy()], levels=(3, 9))
    c.add(mix(c.dicts[0], text[100000:], 70000, 110), 0)
    calls.append(c)

    c = HcCall("dictionary_lengths", [xml[1000:1000 + n].copy() for n in DICT_LENGTHS])
    for rnd in range(2):
        for d, n in enumerate(DICT_LENGTHS):
            c.add(mix(c.dicts[d], xml[120000:], 13 if rnd else 1024, 200 + d), d)
    calls.append(c)

    # rule 2: a match at the message's 13th byte whose backward extension would run into the dictionary's last byte
    calls.append(HcCall("seam", [u8(SEAM_DICTIONARY)]).add(u8(SEAM_MESSAGE), 0))

    # rule 1: the dictionary's last three positions never enter the chain ("XYZW" straddles the seam)
    d = np.concatenate([text[:600], u8(b"XYZ")])
    m = np.concatenate([u8(b"W0123"), text[5000:5040], u8(b"XYZW0123"), text[6000:6050]])
    calls.append(HcCall("tail3", [d]).add(m, 0))

    # rule 3: a match that starts in the dictionary, runs through dictEnd and goes on against the message's start
    d = text[:4096].copy()
    calls.append(HcCall("tile", [d, text[:100].copy()]).add(np.tile(d[-40:], 5), 0).add(np.tile(text[60:100], 5), 1))

    # rule 5: runs of a 1-, 2-, 3- and 4-byte pattern across the seam, both ways round
    lorem = corpus.lorem(2000)
    c = HcCall("periods", [])
    for p in PERIODS:
        c.dicts.append(np.concatenate([lorem[:500], pattern(p, 700)]))
        c.add(np.concatenate([pattern(p, 900), lorem[500:800], pattern(p, 333), lorem[800:900]]), len(c.dicts) - 1)
        c.dicts.append(pattern(p, 2000))
        c.add(np.concatenate([lorem[:50], pattern(p, 5000)]), len(c.dicts) - 1)
    calls.append(c)

    c = HcCall("zeros", [np.zeros(4096, np.uint8), np.zeros(8192, np.uint8)])
    c.add(np.zeros(8192, np.uint8), 0).add(np.zeros(4096, np.uint8), 1).add(np.zeros(13, np.uint8), 0)
    calls.append(c)

    # rule 4: a full dictionary of noise; kept offset k is usable from message position q iff 65536 - k + q <= 65535
    d = noise[:K64].copy()
    m = noise[K64:K64 + 4096].copy()
    m[500:516] = d[501:517]            # distance 65 535: usable
    m[1500:1516] = d[1500:1516]        # distance 65 536: refused
    m[2500:2540] = d[2503:2543]        # distance 65 533: usable
    calls.append(HcCall("distance_limits", [d]).add(m, 0))

    d = text[:4096].copy()
    c = HcCall("caps", [d, u8(SEAM_DICTIONARY), calls[4].dicts[0]])
    for cap in ("exact", "minus1"):
        c.add(u8(SEAM_MESSAGE), 1, cap)
        c.add(calls[4].msgs[0], 2, cap)
        c.add(mix(d, text[100000:], 1024, 300), 0, cap)
        c.add(mix(d, text[100000:], 13, 301), 0, cap)
        c.add(mix(d, text[100000:], 12, 302), 0, cap)
        c.add(corpus.random_bytes(1024, 7), 0, cap)
    calls.append(c)

    dicts = [text[:K64].copy(), xml[:20000].copy(), text[:K64].copy(), synthetic("osdb", 3000, 3)]
    c = HcCall("interleaved", dicts)
    fresh = [text[150000:], xml[100000:], text[250000:], synthetic("osdb", 60000, 4)]
    for i in range(24):
        k = i % 4
        c.add(mix(dicts[k], fresh[k], (1024, 4096, 700, 33)[(i // 4) % 4], 400 + i), k)
    calls.append(c)

    calls.append(HcCall("no_messages", [text[:500].copy()]))
    calls.append(HcCall("nothing", []))

    c = HcCall("noise", [text[:4096].copy()])
    c.add(corpus.random_bytes(1024, 5), 0).add(corpus.random_bytes(300, 6), 0)
    calls.append(c)

    # more messages than the chip has wave slots: the ticket hands out further rounds
    d = text[:K64].copy()
    c = HcCall("ticket_rounds", [d], big=True, levels=(3,))
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


def calls() -> List[HcCall]:
    """the list, built once; nobody changes it"""
    global _calls
    if _calls is None:
        _calls = build()
    return _calls


def call_levels():
    """(call name, level) for every pair the tests run"""
    return [(c.name, lv) for c in calls() for lv in c.levels]
