"""The case list the chain encoder's emulator and GPU tests share: per case the encoders' settings and, call by
call, every encoder's run of TopupAndEncode records.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

from k4os.compression.lz4_amd import corpus
from chain_encoder_witness import WitnessEncoder

K1, K64 = 1024, 65536


def content(n: int, seed: int, kind: str = "text") -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    blocks = corpus.silesia_like_blocks((n + K64 - 1) // K64, K64, seed=seed)
    return np.ascontiguousarray(blocks.reshape(-1)[:n])


def offer_all(data: np.ndarray, block_size: int, pieces, rng, p_force=0.0, allow=True):
    """records that offer `data` in pieces of the given lengths, each piece until it is in (the rest goes into a later record, as
    the contract asks), forcing a short block now and then.  Returns a flat record list; the model is a counting witness."""
    w = WitnessEncoder(True, 0, block_size, 0, counting=True)      # (only Topup's arithmetic is used: the same for every kind)
    recs, pos = [], 0
    for n in pieces:
        end = min(pos + n, data.size)
        while pos < end:
            force = bool(rng.random() < p_force)
            e = w.enc
            take = min(max(e.index + e.block_size - e.pointer, 0), end - pos)
            # offer more than fits now and then: Topup takes only `take`
            over = int(rng.integers(0, 3)) == 0
            piece = data[pos:end] if over else data[pos:pos + take]
            recs.append((piece, force, allow))
            e.topup(data, pos, piece.size)
            if e.bytes_ready >= (1 if force else e.block_size):
                e.commit()                               # (kind-independent: only the room matters, and a save keeps index == pointer)
            pos += take
    return recs


def split_calls(recs, n_calls, rng):
    cuts = sorted(int(x) for x in rng.integers(0, len(recs) + 1, n_calls - 1))
    cuts = [0] + cuts + [len(recs)]
    return [recs[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def small_stream(seed: int, total=200 * K1, B=K1):
    """about 200 KiB in records of random length with forced short blocks of 1 .. B - 1 bytes, then a flush"""
    rng = np.random.default_rng(seed)
    data = content(total, seed)
    pieces = []
    left = total
    while left > 0:
        n = int(rng.integers(1, 3 * B))
        pieces.append(min(n, left)); left -= pieces[-1]
    recs = offer_all(data, B, pieces, rng, p_force=0.25)
    recs.append((data[:0], True, True))
    return data, recs


def save_distances(settings, recs):
    w = WitnessEncoder(*settings, counting=True)
    w.run(recs)
    return w.codec.saves


# B = 1 KiB, extraBlocks 0: (chaining, level, blockSize, extraBlocks)
SMALL_SETTINGS = [(True, 0, K1, 0), (True, 3, K1, 0), (True, 9, K1, 0), (True, 12, K1, 0), (False, 0, K1, 0), (False, 3, K1, 0)]
SMALL_SEEDS = [11, 12, 13]


def small_case():
    """-> (settings per stream, calls[c][s] = records): every SMALL_SETTINGS kind over every seed's stream, in 6 calls"""
    settings, per_stream = [], []
    for st in SMALL_SETTINGS:
        for seed in SMALL_SEEDS:
            _, recs = small_stream(seed)
            settings.append(st)
            per_stream.append(split_calls(recs, 6, np.random.default_rng(seed + 100)))
    calls = [[ps[c] for ps in per_stream] for c in range(6)]
    return settings, calls


def _assert_residues():
    got = set()
    for seed in SMALL_SEEDS:
        _, recs = small_stream(seed)
        d = save_distances((True, 3, K1, 0), recs)
        assert len(d) >= 2, "each stream sees at least two saves"
        got |= {x % 16 for x in d}
    return got


def big_case(B: int, extra: int, levels, chaining=True, seed=5):
    """5 blocks per stream with a forced block of 1 byte and one of 12 bytes in the middle and a record that fills the block exactly"""
    rng = np.random.default_rng(seed)
    settings, per_stream = [], []
    for k, level in enumerate(levels):
        data = content(5 * B + 13, seed + k)
        recs, pos = [], 0
        def put(n, force=False, allow=True):
            nonlocal pos
            recs.append((data[pos:pos + n], force, allow)); pos += n
        put(B)                      # fills the block exactly
        put(B // 2); put(B - B // 2)
        put(1, True)                # a forced block of 1 byte
        put(B - 7); put(7)
        put(12, True)               # and one of 12 bytes
        put(B // 3); put(B - B // 3)
        put(B)
        recs.append((data[:0], False, True)); recs.append((data[:0], True, True))
        settings.append((chaining, level, B, extra))
        per_stream.append(split_calls(recs, 3, rng))
    return settings, [[ps[c] for ps in per_stream] for c in range(3)]


def record_cases():
    """runs of 0, 1 and 9 records, recLen 0 with and without FORCE, incompressible bytes with and without ALLOW_COPY, a stream that
    sits a call out: three streams (L00 chained, L09 chained, L00 independent) in 4 calls"""
    settings = [(True, 0, 2 * K1, 0), (True, 9, 2 * K1, 1), (False, 0, 2 * K1, 0)]
    noise = content(40 * K1, 3, "random")
    text = content(40 * K1, 4)
    e = noise[:0]
    calls = []
    for s in range(3):
        r1 = [(e, False, True)]                                                      # nothing, no force: None
        r9 = [(noise[0:2048], False, True), (noise[2048:4096], False, False), (text[0:100], False, True), (e, True, True),
              (noise[4096:4196], True, False), (noise[4196:4296], True, True), (e, True, True), (e, False, False), (text[100:2148], False, True)]
        r3 = [(text[2148:3000], False, True), (e, True, False), (noise[5000:5013], True, True)]
        calls.append([r1, r9, [], r3])
    calls = [[calls[s][c] for s in range(3)] for c in range(4)]
    calls[2][1] = [(text[3000:3500], False, True)]       # stream 1 runs in the call the others sit out
    return settings, calls


def mixed_case(n_streams=64, n_calls=12, seed=77):
    """64 encoders of mixed kinds, levels and sizes in 12 calls"""
    rng = np.random.default_rng(seed)
    kinds = [(True, 0), (True, 1), (True, 3), (True, 9), (True, 12), (False, 0), (False, 3), (False, 10)]
    sizes = [(K1, 0), (4 * K1, 1), (16 * K1, 0), (K64, 0), (3 * K1, 3)]
    settings, per_stream = [], []
    for s in range(n_streams):
        ch, lv = kinds[s % len(kinds)]
        B, ex = sizes[int(rng.integers(0, len(sizes)))]
        total = int(rng.integers(1, 40)) * B // 4 + int(rng.integers(0, 17)) + (80 * K1 if B == K1 else 0)
        data = content(total, seed + s, "random" if s % 7 == 3 else "text")
        pieces, left = [], total
        while left > 0:
            pieces.append(min(int(rng.integers(1, 2 * B)), left)); left -= pieces[-1]
        recs = offer_all(data, B, pieces, rng, p_force=0.15, allow=bool(s % 3))
        recs.append((data[:0], True, True))
        settings.append((ch, lv, B, ex))
        per_stream.append(split_calls(recs, n_calls, rng))
    return settings, [[ps[c] for ps in per_stream] for c in range(n_calls)]
