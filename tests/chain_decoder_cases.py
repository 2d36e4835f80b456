"""The case list of the chained-decoder tests (k4lz4_chain_decode_batch), shared by the emulator and the GPU tests.

A case is (name, settings, calls): settings one (chaining, blockSize, extraBlocks) per stream, calls a list of
  ("run", records per stream [(inject, bytes, blockSize)], drain flag, caps or None)
  ("drain", offsets, lengths)
  ("reset", streams)
play() applies them to a driver (the witness's WitnessDecoders, the emulator's EmuDecoders, the GPU's) and returns the transcript:
per run the record results, the totals and the drained bytes, and behind every run the whole of what each decoder holds
(Drain(-BytesReady, BytesReady): how far back a drain reaches is part of the contract) and the query words.  Chained blocks come
from the CPU witnesses of the two chain encoders (liblz4 driven through LZ4EncoderBase's ring).  Test infrastructure only."""
from __future__ import annotations

import os
import struct

import numpy as np

import fast_chain_witness as FW
import hc_chain_witness as HW
from chain_decoder_witness import BLOCK_SIZE, DECODE, INJECT, NOT_RUN, RANGE, TARGET  # noqa: F401

K1, K64 = 1024, 65536
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EMPTY_BLOCK = b"\x00"          # the single token 0x00: a chained block that decodes to nothing


def content(n: int, seed: int) -> np.ndarray:
    """compressible, with repeats from up to 60 KiB back: matches that reach over many blocks"""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(64)]
    out = bytearray()
    while len(out) < n:
        if len(out) > 200 and rng.random() < 0.3:
            back = int(rng.integers(1, min(len(out), 60000)))
            ln = int(rng.integers(4, 400))
            at = len(out) - back
            out += bytes(out[at:at + ln]) if ln <= back else (bytes(out[at:]) * (ln // back + 1))[:ln]
        else:
            out += b" ".join(words[int(i)] for i in rng.integers(0, 64, 12))
    return np.frombuffer(bytes(out[:n]), np.uint8).copy()


def chain_blocks(data: np.ndarray, sizes, enc_block: int, kind: str = "fast", extra: int = 0):
    """the chained blocks an encoder cuts when it is topped up by sizes[k] bytes and flushed: [(raw bytes, payload)]"""
    codec = FW.Lz4FastChainCodec() if kind == "fast" else HW.Lz4HcCodec(9)
    enc = HW.RingEncoder(codec, enc_block, extra)
    out, pos = [], 0
    for n in sizes:
        assert enc.topup(data, pos, n) == n
        got, payload = enc.encode(False)
        assert got == len(payload) > 0
        out.append((data[pos:pos + n].tobytes(), payload))
        pos += n
    codec.close()
    return out


def dec(blocks, bs=0):
    return [(False, p, bs) for _, p in blocks]


def cut(records, counts):
    """the records in runs of counts[0], counts[1], ... (cyclic)"""
    out, at, k = [], 0, 0
    while at < len(records):
        c = counts[k % len(counts)]
        out.append(records[at:at + c])
        at += c
        k += 1
    return out


def _small_ring():
    """B = 1 KiB, extraBlocks = 0: the index passes 64 KiB + 32 at odd byte positions and nearly every block moves the history down
    over itself, by distances of every residue (test_chain_decoder_host checks the residues that occurred)"""
    streams = []
    for seed in (11, 12, 13):
        rng = np.random.default_rng(seed)
        sizes = [60000 - seed] + [int(x) for x in rng.integers(1, K1 + 1, 90)]     # the first, stored raw, fills most of the ring
        blocks = chain_blocks(content(sum(sizes), seed), sizes, K64, "fast" if seed != 12 else "hc")
        streams.append([(True, blocks[0][0], 0)] + dec(blocks[1:]))
    calls = []
    runs = [cut(s, c) for s, c in zip(streams, ((9, 1, 0, 9), (1, 9, 9), (9, 9, 1, 0)))]
    for k in range(max(len(r) for r in runs)):
        calls.append(("run", [r[k] if k < len(r) else [] for r in runs], k % 3 != 0, [K64 + 9 * K1] * 3))
    return "small-ring-wraps", [(1, K1, 0)] * 3, calls


def _b64k():
    rng = np.random.default_rng(21)
    settings, streams = [], []
    for extra, kind in ((0, "hc"), (2, "fast"), (0, "fast")):
        sizes = [K64, K64] + [int(x) for x in rng.integers(1, K64 + 1, 5)] + [K64]
        streams.append(dec(chain_blocks(content(sum(sizes), 20 + extra + len(kind)), sizes, K64, kind, extra)))
        settings.append((1, K64, extra))
    calls = [("run", [s[k:k + 2] for s in streams], k == 2, [2 * K64] * 3) for k in range(0, 8, 2)]
    return "b64k-extra-0-and-2", settings, calls


def _b4m():
    B = 4 << 20
    sizes = [B, 3 * (1 << 20) + 17, B]
    data = np.resize(content(50021, 31), sum(sizes))
    blocks = chain_blocks(data, sizes, B)
    return "b4m-three-blocks", [(1, B, 0)], [("run", [dec(blocks[:1])], True, [B]), ("run", [dec(blocks[1:])], False, None)]


def _empty_block():
    sizes = [700, 1, 1024, 333]
    b = dec(chain_blocks(content(sum(sizes), 41), sizes, K1))
    e = (False, EMPTY_BLOCK, 0)
    recs = [e, b[0], b[1], e, e, b[2], e, b[3]]
    return "block-of-nothing", [(1, K1, 0), (1, K1, 0)], [("run", [recs, recs], False, None), ("reset", [0, 1]),
                                                        ("run", [recs[:4], recs[:1]], True, [4096, 0]), ("run", [recs[4:], recs[1:]], True, [4096, 4096])]


def _inject_paths():
    """chained, B = 1 KiB, ring 66 592: Inject behind (path 1), 64 KiB and longer to the front (path 2), the tail of the history
    moved down first (path 3), and one byte too long; small blocks in between are decoded, so every Inject is seen as prefix"""
    sizes = [1000, K64, 700, K64, K64 - 1, 1000, 500, 1024, 900, 65000, 300]
    blocks = chain_blocks(content(sum(sizes), 51), sizes, K64)
    recs = [(n > K1, raw if n > K1 else p, 0) for (raw, p), n in zip(blocks, sizes)]
    recs[0] = (True, blocks[0][0], 0)                           # path 1 into a fresh decoder
    recs[6] = (True, blocks[6][0], 0)                           # path 3 with a long tail: index 66 536 + 500
    too_long = (True, bytes(K64 + 1), 0)
    calls = [("run", [recs[:3]], False, None), ("run", [[too_long, recs[3]]], False, None), ("run", [recs[3:5]], True, [2 * K64]),
             ("run", [[recs[5]]], False, None), ("run", [[recs[6]]], False, None), ("run", [recs[7:9] + [too_long]], True, [4096]),
             ("run", [recs[9:]], True, [K64 + 300])]
    return "inject-three-paths", [(1, K1, 0)], calls


def _inject_dictionary():
    """Inject as a pre-made dictionary, then blocks whose matches reach into it; B = 64 KiB with a dictionary of 64 KiB and more"""
    out_s, out_r = [], []
    for B, extra, dsize, seed in ((K1, 0, 5000, 61), (K64, 0, K64, 62), (2 * K64, 1, K64 + 4321, 63)):
        sizes = [dsize] + [min(B, 3000)] * 4
        blocks = chain_blocks(content(sum(sizes), seed), sizes, max(B, dsize))
        out_s.append((1, B, extra))
        out_r.append([(True, blocks[0][0], 0)] + dec(blocks[1:]))
    return "inject-as-dictionary", out_s, [("run", [r[:2] for r in out_r], False, None), ("run", [r[2:] for r in out_r], True, [12000] * 3)]


def _record_block_size():
    sizes = [2000, 1500, 2080, 1024, 10]
    blocks = chain_blocks(content(sum(sizes), 71), sizes, K64)
    p = [b[1] for b in blocks]
    chained = [[(False, p[0], 2000)], [(False, p[1], 1499), (False, p[2], 2080)], [(False, p[1], 1500), (False, p[2], 2081), (False, p[3], 0)],
               [(False, p[2], 2080), (False, p[3], 1024), (False, p[4], 0x7fffffff)], [(False, p[4], 10)]]
    from oracle_lib import Oracle
    o = Oracle()
    ind = [o.encode(content(n, 72 + n), 0) for n in (1024, 600)]
    independent = [[(False, ind[0], 1024)], [(False, ind[1], 1025), (False, ind[1], 0)], [(False, ind[1], 600)], [(False, ind[0], -5)], []]
    return "per-record-block-size", [(1, K1, 1), (0, K1, 0)], [("run", [c, i], False, None) for c, i in zip(chained, independent)]


def _run_lengths():
    sizes = [int(x) for x in np.random.default_rng(81).integers(1, K1 + 1, 30)]
    s = [dec(chain_blocks(content(sum(sizes), 81 + k), sizes, K1)) for k in range(3)]
    calls = []
    for k, drain in enumerate((True, False, True)):
        lens = [(0, 1, 9), (9, 0, 1), (1, 9, 0)][k]
        take = [s[i][:lens[i]] for i in range(3)]
        s = [s[i][lens[i]:] for i in range(3)]
        calls.append(("run", take, drain, [9 * K1] * 3))
    return "runs-of-0-1-9", [(1, K1, 0)] * 3, calls


def _target_short():
    sizes = [400, 500, 600, 700, 800]
    chained = dec(chain_blocks(content(sum(sizes), 91), sizes, K1))
    from oracle_lib import Oracle
    o = Oracle()
    ind = [(False, o.encode(content(n, 92 + n), 0), 0) for n in sizes]
    cap = [sizes[0] + sizes[1] + sizes[2] - 1] * 2
    calls = [("run", [chained, ind], True, cap), ("drain", [-600, -600], [600, 600]), ("run", [chained[3:], ind[3:]], True, [1500, 1500])]
    return "target-one-byte-short", [(1, K1, 0), (0, K1, 0)], calls


def _drain_ranges():
    sizes = [1000, 24]
    chained = dec(chain_blocks(content(sum(sizes), 101), sizes, K1))
    from oracle_lib import Oracle
    ind = [(False, Oracle().encode(content(777, 102), 0), 0)]
    calls = [("drain", [0, 0], [0, 0]), ("drain", [-1, -1], [1, 0]), ("run", [chained, ind], False, None)]
    for off, ln in (((-1024, -777), (1024, 777)), ((-1025, -778), (1, 1)), ((0, 0), (0, 0)), ((0, 0), (1, 1)), ((-1, -1), (1, 1)), ((-1, -1), (2, 2)),
                    ((-1024, -777), (1025, 778)), ((-10, -10), (-1, -1)), ((1, 1), (0, 0)), ((-500, -500), (100, 500))):
        calls.append(("drain", list(off), list(ln)))
    return "drain-ranges", [(1, K1, 0), (0, K1, 0)], calls


def _independent():
    from oracle_lib import Oracle
    o = Oracle()
    B = K1
    blk = lambda n, seed: (False, o.encode(content(n, seed), 0), 0)  # noqa: E731
    raw = lambda n, seed: (True, content(n, seed).tobytes(), 0)  # noqa: E731
    recs = [blk(B + k, 110 + k) for k in range(1, 9)] + [blk(B + 9, 119), blk(10, 120), (False, b"", 0), blk(B, 121), (True, b"", 0),
                                                         raw(B + 8, 122), raw(B + 9, 123), raw(5, 124), blk(B + 8, 125)]
    runs = [recs[0:4], recs[4:9], recs[8:10], recs[9:11], recs[10:12], recs[11:13], recs[13:15], recs[14:16], recs[15:17]]
    calls = [("run", [r, r], k % 2 == 0, [8 * K1] * 2) for k, r in enumerate(runs)]
    calls.insert(5, ("run", [[(False, b"", 0), recs[0]], [recs[0], (False, b"", 0)]], False, None))
    return "independent-decoders", [(0, B, 0), (0, B - 5, 3)], calls


def _fail_after_move():
    """a block that does not decode, met when Prepare has just moved the history: the move stays, the block is not counted"""
    sizes = [K64, 100, 500, 500]
    blocks = chain_blocks(content(sum(sizes), 131), sizes, K64)
    recs = [(True, blocks[0][0], 0), (True, blocks[1][0], 0), (False, b"\xff\xff\x00", 0), (False, blocks[2][1], 0), (False, blocks[3][1], 0)]
    return "code-after-prepare", [(1, K1, 0)], [("run", [recs[:4]], False, None), ("run", [recs[2:4]], True, [K1]), ("run", [recs[3:]], True, [K1])]


def issue64_records():
    raw = open(os.path.join(GOLDEN, "issue64_input.bin"), "rb").read()
    pos, recs = 20, []
    while raw[pos:pos + 4] == b"bv41":
        u, c = struct.unpack_from("<II", raw, pos + 4)
        recs.append((u, raw[pos + 12:pos + 12 + c]))
        pos += 12 + c
    return recs, open(os.path.join(GOLDEN, "issue64_output.bin"), "rb").read()


def _issue64():
    recs, want = issue64_records()
    assert len(recs) == 2
    return "issue64-bv41", [(1, K64, 0)], [("run", [[(False, p, u) for u, p in recs]], True, [len(want)])]


BUILDERS = [_small_ring, _b64k, _b4m, _empty_block, _inject_paths, _inject_dictionary, _record_block_size, _run_lengths, _target_short,
            _drain_ranges, _independent, _fail_after_move, _issue64]
_cache = {}


def case(k: int):
    if k not in _cache:
        _cache[k] = BUILDERS[k]()
    return _cache[k]


def case_ids():
    return [b.__name__.lstrip("_") for b in BUILDERS]


# ---- mutants ---------------------------------------------------------------------------------------------------------------
N_MUTANTS = 300


def mutants():
    """300 seeded payload mutations of chained streams, one decoder each: ("run" the blocks before, "run" the mutant, "run" the
    unmutated next block).  -> (settings, calls)"""
    if "m" in _cache:
        return _cache["m"]
    rng = np.random.default_rng(2024)
    pools = []
    for seed, kind, B in ((201, "fast", K1), (202, "hc", K1), (203, "fast", 4 * K1)):
        sizes = [int(x) for x in np.random.default_rng(seed).integers(B // 2, B + 1, 8)]
        pools.append((B, dec(chain_blocks(content(sum(sizes), seed), sizes, B, kind))))
    settings, before, mutant, after = [], [], [], []
    for m in range(N_MUTANTS):
        B, blocks = pools[m % len(pools)]
        j = int(rng.integers(0, len(blocks) - 1))
        p = bytearray(blocks[j][1])
        how = m % 4
        if how == 3:
            p = p[:int(rng.integers(0, len(p)))]                                # truncation
        else:
            for _ in range(1 if how == 0 else int(rng.integers(2, 5))):         # flips: a bit, or a few bytes
                at = int(rng.integers(0, len(p)))
                p[at] = p[at] ^ (1 << int(rng.integers(0, 8))) if how == 0 else int(rng.integers(0, 256))
        settings.append((1, B, int(m % 5 == 0)))
        before.append(blocks[:j])
        mutant.append([(False, bytes(p), 0)])
        after.append([blocks[j + 1]])
    calls = [("run", before, False, None), ("run", mutant, True, [8 * K1] * N_MUTANTS), ("run", after, True, [8 * K1] * N_MUTANTS)]
    _cache["m"] = (settings, calls)
    return _cache["m"]


# ---- playing a case --------------------------------------------------------------------------------------------------------
def play(d, calls, fill=None):
    """fill: (witness only) the byte that lies behind every decoder's index before each run"""
    t = []
    for c in calls:
        if c[0] == "run":
            if fill is not None:
                for w in d.d:
                    w.fill(fill)
            rec_out, out_len, drained = d.run(c[1], c[2], c[3])
            q = d.query()
            ready = [int(x) for x in q[:, 0]]
            held = d.drain([-r for r in ready], ready)
            # an independent decoder whose Decode threw keeps its BytesReady, but the failed decode has written over the block it held
            # (in the reference too, as far as its own copy loops got): those bytes are nobody's until the next record replaces them
            held = [len(h) if q[i, 5] == 0 and q[i, 4] == DECODE else h for i, h in enumerate(held)]
            t.append(("run", rec_out, [int(x) for x in out_len], drained, held, q[:, :7].tolist()))
        elif c[0] == "drain":
            t.append(("drain", d.drain(c[1], c[2])))
        else:
            d.reset(c[1])
            t.append(("reset", d.query()[:, :7].tolist()))
    return t


def same(want, got, skip_bytes=()):
    """the two transcripts agree; skip_bytes: streams whose bytes the reference leaves undefined (results and codes still compared)"""
    assert len(want) == len(got)
    for k, (w, g) in enumerate(zip(want, got)):
        assert w[0] == g[0]
        if w[0] == "run":
            assert w[1] == g[1], f"call {k}: record results"
            assert w[2] == g[2], f"call {k}: totals"
            assert w[5] == g[5], f"call {k}: query words"
            for i in range(len(w[3])):
                if i in skip_bytes:
                    assert len(w[3][i]) == len(g[3][i]) and len(w[4][i]) == len(g[4][i])
                    continue
                assert w[3][i] == g[3][i], f"call {k}, stream {i}: drained bytes"
                assert w[4][i] == g[4][i], f"call {k}, stream {i}: what the decoder holds"
        else:
            assert w[1] == g[1], f"call {k}: {w[0]}"
