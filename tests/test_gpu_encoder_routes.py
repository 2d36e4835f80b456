"""Every route the batch launcher can send an encode, pickle or wrap call down, on device arenas, under tight output limits
(tests/encoder_cases.py; proven on the CPU by tests/test_encoder_cases_host.py).  Everything goes through the device forms on
torch tensors, so the arena a kernel wrote into is the arena that is read back: a write outside a slot -- behind it or in front of
it, for an accepted or a REJECTED block -- shows.

The launcher chooses by switches, flags and blocks per CU (k4lz4_launch.hpp: fast_route, fast_chunk, hc_chunk).
A context reads its switches when it is created, so every variant is a context made under its environment; every batch count is
derived from the CU count the device reports; `k4lz4_last_encode_route` says after every call which kernel families it launched
and how (queue, persistent, priorities, cost order, device split, migration, more than one chunk), and a variant whose call did
not take exactly its route fails -- a threshold that moves shows here, where the bytes would have stayed right.

Shapes: "full" is a round's whole case set in calls of at most 8 blocks per CU; ("small", n) its cases of at most 2 KiB repeated
to exactly n, in ONE call; the others are cuts of the full set named where they are made.  Device forms do not know the blocks'
lengths on the host, so k4_parse_big_kernel and k4_encode_fast_rest_kernel are launched whatever the chunk holds."""
import os

import numpy as np
import pytest

import encoder_cases as ec
from k4os.compression.lz4_amd import _native as K

pytestmark = pytest.mark.gpu

R = lambda *names: sum(getattr(K, "ENCODE_ROUTE_" + n) for n in names)
# the two-step encoder on a batch of whole blocks, and on a ragged batch (FLAG_SEGMENTS, pickles, wraps) whose big blocks are cut
TWO_STEP = R("PARSE", "PARSE_BIG", "REST", "PCOST_ORDER", "MIGRATE")
TWO_STEP_SEG = R("PARSE", "PARSE_SEG", "REST", "SEGMENTS", "MIGRATE")
DEVICE_SPLIT = R("LDS", "GTAB", "TWO_KERNELS")
# HC: (calls whose blocks are all at most 64 KiB, calls with a longer one); launch_hc decides by the longest block of a call
HC3 = (R("HC_CHAIN_PART", "HC_CAND_LDS", "HC_PARSE_SEG4"), R("HC_CHAIN_MEM", "HC_CAND_MEM", "HC_PARSE"))
HC9 = (R("HC_CHAIN_PART", "HC_CAND_LDS", "HC_PARSE"), R("HC_CHAIN_MEM", "HC_CAND_MEM", "HC_PARSE"))
OPT = (R("HC_CHAIN_PART", "HC_PARSE_OPT"), R("HC_CHAIN_MEM", "HC_PARSE_OPT"))
COPY, ENV = R("ALLOW_COPY"), R("ENVELOPE")
both = lambda pair, extra: tuple(r | extra for r in pair)
RAW, X32, ACOPY, SEG, NO_REORDER, NO_SPLIT = ec.FLAG_RAW, ec.FLAG_X32, ec.FLAG_ALLOW_COPY, ec.FLAG_SEGMENTS, ec.FLAG_NO_REORDER, ec.FLAG_NO_SPLIT


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def codec_under(env):
    """a DeviceCodec whose context was created under env (the switches are read then), the environment restored"""
    from k4os.compression.lz4_amd.device import DeviceCodec
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return DeviceCodec(0)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


# ---- shapes: (layout, expectation, calls) with calls a list of index arrays, one device call each ----

_shapes = {}


def even_spans(idx, most):
    """idx in contiguous calls of equal size, at most `most` each"""
    k = max(1, -(-len(idx) // most))
    return [np.asarray(c) for c in np.array_split(np.asarray(idx), k)]


def strided(idx, most):
    """idx in calls of at most `most` that each hold every k-th case: every call gets every kind of block"""
    k = max(1, -(-len(idx) // most))
    return [np.asarray(idx[j::k]) for j in range(k)]


def shape(mode, flags, oracle, what, cuts):
    """cuts: whether the variant's context cuts big blocks into segments (what `comparable` may then leave open)"""
    key = (mode, flags, what, cuts)
    if key in _shapes:
        return _shapes[key]
    cu = cu_count()
    cs, lay, exp = ec.prepared(mode, flags, oracle, cuts)

    def cut_of(mode, flags, oracle, idx):
        l = ec.layout(cs.subset(idx))
        return l, ec.expect(l, oracle, flags, cuts=cuts)
    size = np.array([cs.blocks[b].size for b, _ in cs.cases])
    tag = np.array(cs.tags)
    every = np.arange(len(cs.cases))
    small = every[size <= 2048]
    spread = lambda idx, n: idx[np.unique(np.linspace(0, len(idx) - 1, min(n, len(idx))).astype(int))]
    one_call = lambda l: [np.arange(l.n)]
    if what == "full":
        out = (lay, exp, even_spans(every, 8 * cu))
    elif what == "full, one call":
        out = (lay, exp, one_call(lay))
    elif what == "full by longest block":            # HC: calls of blocks of at most 64 KiB, then calls with the longer ones
        out = (lay, exp, strided(every[size <= 65536], 8 * cu) + strided(every[size > 65536], 8 * cu))
    elif what[0] == "small":                          # the cases of at most 2 KiB repeated to exactly n
        l, e = cut_of(mode, flags, oracle, small[np.arange(what[1]) % len(small)])
        out = (l, e, one_call(l))
    elif what[0] == "small + cut":                    # ... in front of every case of the blocks that segments cut
        l, e = cut_of(mode, flags, oracle, np.concatenate([small[np.arange(what[1]) % len(small)], every[tag == "cut"]]))
        out = (l, e, one_call(l))
    elif what == "512 of all":                        # every seventh or so of the full set, the big blocks among them
        l, e = cut_of(mode, flags, oracle, spread(every, 512))
        out = (l, e, one_call(l))
    elif what == "512 with the cut":                  # every case of the cut blocks and a spread of the others, 512 together
        cut = every[tag == "cut"]
        l, e = cut_of(mode, flags, oracle, np.concatenate([spread(every[tag != "cut"], 512 - len(cut)), cut]))
        out = (l, e, one_call(l))
    elif what == "big + 37":                          # the blocks of 65 547 bytes and more behind 37 small cases
        l, e = cut_of(mode, flags, oracle, np.concatenate([spread(small, 37), every[size >= ec.LIMIT_64K]]))
        out = (l, e, one_call(l))
    elif what == "64k + 100":                         # where the 32-bit engine hashes differently, behind 100 small cases
        l, e = cut_of(mode, flags, oracle, np.concatenate([spread(small, 100), every[size >= 65535]]))
        out = (l, e, one_call(l))
    elif what == "20 per tag":                        # (the instrumented twin takes blocks below 65 547 bytes)
        idx = np.concatenate([spread(every[(tag == t) & (size < ec.LIMIT_64K)], 20) for t in sorted(set(tag))])
        l, e = cut_of(mode, flags, oracle, np.sort(idx))
        out = (l, e, one_call(l))
    else:
        raise ValueError(what)
    _shapes[key] = out
    return out


def run_on_device(codec, lay, calls, flags, profile=None):
    """the layout's cases through the device form of its mode, one call per entry of `calls`, all into one arena on the device;
    after the calls k4lz4_synchronize must report K4LZ4_OK.  Returns (out_len, the arena and the source buffer as they are
    afterwards, what k4lz4_last_encode_route reported after every call)."""
    import torch
    from k4os.compression.lz4_amd import wrap_device
    from k4os.compression.lz4_amd.device import DeviceBatch
    dev = codec.device
    up = lambda a, t=None: torch.from_numpy(np.array(a if t is None else a.view(t))).to(dev)      # (a copy: the prepared arrays are read-only)
    src, arena = up(lay.src), up(lay.arena)
    soff, slen, doff, dcap = up(lay.src_off, np.int64), up(lay.src_len), up(lay.dst_off, np.int64), up(lay.dst_cap)
    out = torch.full((lay.n,), ec.UNWRITTEN, dtype=torch.int32, device=dev)
    routes = []
    call = ec.call_of(lay.mode)
    for idx in calls:
        sel = torch.from_numpy(np.asarray(idx, np.int64)).to(dev)
        s, d = DeviceBatch(src, soff[sel], slen[sel]), DeviceBatch(arena, doff[sel], dcap[sel])
        part = torch.full((len(idx),), ec.UNWRITTEN, dtype=torch.int32, device=dev)
        if profile is not None:
            codec.profile(profile, s, d, part)
        elif call == "pickle":
            codec.pickle(s, d, part, level=ec.LEVEL.get(lay.mode, 0))
        elif call == "wrap":           # (wrap_device makes its own out_len, filled with 0: no wrap returns 0, so an entry never written still shows)
            part = wrap_device(codec, s.data, s.off, s.length, high=bool(flags), out=(d.data, d.off, d.length))[2]
        else:
            codec.encode(s, d, part, level=ec.LEVEL.get(lay.mode, 0), flags=flags)
        routes.append(codec.ctx.last_encode_route())
        out[sel] = part
    rc = codec.lib.k4lz4_synchronize(codec.ctx.handle, codec._stream())
    assert rc == K.K4LZ4_OK, (rc, codec.lib.k4lz4_last_error(codec.ctx.handle))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), arena.cpu().numpy(), src.cpu().numpy(), routes


_baseline = {}
_trouble = []       # a variant whose device calls failed as calls (a HIP error, a context in trouble): no later variant touches the device


def run_variant(oracle, mode, flags, env, what, route, profile=None, expect_flags=None):
    """one context made under env, the shape's calls, the route of every call, `check` against the oracle, and -- on the full
    set -- the same results and, under `comparable`, the same arena as a default context's run of the same calls"""
    cu = cu_count()
    eflags = flags if expect_flags is None else expect_flags
    cuts = ec.cuts_by_default(mode, eflags) and "K4LZ4_NO_SEGMENTS" not in env
    lay, exp, calls = shape(mode, eflags, oracle, what, cuts)
    if ec.call_of(mode) != "encode" or mode == "fast-seg":
        env = dict(ec.SEG_ENV, **env)
    name = f"{mode} flags {flags} {env or 'default context'} {what}"
    if _trouble:
        pytest.fail(f"not run: the device calls of '{_trouble[0]}' failed, and nothing more is started on a device in that state")
    codec = codec_under(env)
    try:
        got, got_arena, src_after, routes = run_on_device(codec, lay, calls, flags, profile)
    except BaseException:
        _trouble.append(name)
        raise
    finally:
        codec.ctx.close()
    if callable(route):
        route = route(cu, [len(c) for c in calls])
    if isinstance(route, tuple):                      # HC: by the longest block of the call
        route = [route[int(lay.src_len[c].max() > 65536)] for c in calls]
    elif not isinstance(route, list):
        route = [route] * len(calls)
    print(f"{name}: {lay.n} cases in {len(calls)} calls of {sorted({len(c) for c in calls})} on {cu} CUs: " +
          ", ".join(sorted({K.encode_route_names(r) for r in routes})))
    for k, (r, w) in enumerate(zip(routes, route)):
        assert r == w, f"{name}: call {k} of {len(calls[k])} blocks on {cu} CUs took {K.encode_route_names(r)}, the variant's route is {K.encode_route_names(w)}"
    ec.check(lay, exp, got, got_arena, name, src_after=src_after)
    if isinstance(what, str) and what.startswith("full"):
        key = (mode, eflags, what)
        if key not in _baseline:
            if env in ({}, ec.SEG_ENV) and flags == eflags and profile is None:
                _baseline[key] = (got, got_arena)
            else:
                base = codec_under(ec.SEG_ENV if env.keys() >= ec.SEG_ENV.keys() else {})
                try:
                    _baseline[key] = run_on_device(base, lay, calls, eflags)[:2]
                except BaseException:
                    _trouble.append(name + " (the default context's run)")
                    raise
                finally:
                    base.ctx.close()
        base_len, base_arena = _baseline[key]
        assert np.array_equal(got, base_len), name
        diff = np.flatnonzero((got_arena != base_arena) & exp.keep & ec.prepared(mode, eflags, oracle)[2].keep)
        assert diff.size == 0, f"{name}: {diff.size} bytes differ from the default context's arena, first at {int(diff[0])}"


def queue_if_more_than(per_cu, base):
    return lambda cu, counts: [base | (R("QUEUE") if n > per_cu * cu else 0) for n in counts]


FAST = [   # name: (environment, flags, shape, route)
    ("default", {}, RAW, "full", TWO_STEP),
    ("pace", {}, RAW, ("small", lambda cu: 12 * cu), TWO_STEP | R("PARSE_PACE")),
    ("persistent", {}, RAW, ("small", lambda cu: 16 * cu + 1), TWO_STEP | R("QUEUE", "PERSISTENT")),
    ("persistent, twice", {}, RAW, ("small", lambda cu: 32 * cu + 2), TWO_STEP | R("QUEUE", "PERSISTENT")),
    # without the persistent launch: equal parts of at most one residency, here two of 8 * cu + 1 and 8 * cu (the first with priorities)
    ("no-persist", {"K4LZ4_NO_PERSIST": "1"}, RAW, ("small", lambda cu: 16 * cu + 1), TWO_STEP | R("PARSE_PACE", "CHUNKS")),
    ("no-persist, twice", {"K4LZ4_NO_PERSIST": "1"}, RAW, ("small", lambda cu: 32 * cu + 2), TWO_STEP | R("PARSE_PACE", "CHUNKS")),
    ("index order", {}, RAW | NO_REORDER, "full", TWO_STEP & ~R("PCOST_ORDER")),
    ("index order, beyond one residency", {}, RAW | NO_REORDER, ("small", lambda cu: 16 * cu + 1), (TWO_STEP & ~R("PCOST_ORDER")) | R("PARSE_PACE", "CHUNKS")),
    ("no-split", {}, RAW | NO_SPLIT, "full", R("MORE")),
    ("no-split, more than 8 per CU", {}, RAW | NO_SPLIT, ("small", lambda cu: 8 * cu + 52), R("LDS")),
    ("emit kernel", {"K4LZ4_NO_INLINE_EMIT": "1"}, RAW, "full", R("PARSE", "EMIT", "REST", "PCOST_ORDER", "MIGRATE")),
    ("queue, 3 waves", {"K4LZ4_PARSE_QUEUE": "1", "K4LZ4_PARSE_WAVES": "3"}, RAW, "full", queue_if_more_than(3, TWO_STEP)),
    ("no-migrate", {"K4LZ4_NO_MIGRATE": "1"}, RAW, ("small", lambda cu: 10 * cu), (TWO_STEP | R("PARSE_PACE")) & ~R("MIGRATE")),
    ("no-pcost", {"K4LZ4_NO_PCOST": "1"}, RAW, ("small", lambda cu: 10 * cu), (TWO_STEP | R("PARSE_PACE")) & ~R("PCOST_ORDER")),
    ("no-pace", {"K4LZ4_NO_PACE": "1"}, RAW, ("small", lambda cu: 10 * cu), TWO_STEP),
    ("no-parse-big", {"K4LZ4_NO_PARSE_BIG": "1"}, RAW, "big + 37", TWO_STEP & ~R("PARSE_BIG")),
    ("one-kernel more", {"K4LZ4_NO_PARSE": "1"}, RAW, "512 of all", R("MORE")),
    # up to 8 blocks per CU the LDS-table kernel's share is the whole batch: the pair is the 28-known-bytes kernel alone
    ("one-kernel pair, up to 8 per CU", {"K4LZ4_NO_PARSE": "1"}, RAW, ("small", lambda cu: 8 * cu), R("MORE")),
    ("one-kernel device split", {"K4LZ4_NO_PARSE": "1"}, RAW, ("small", lambda cu: 8 * cu + 52), DEVICE_SPLIT),
    ("fixed share", {"K4LZ4_NO_PARSE": "1", "K4LZ4_SPLIT_PCT": "30"}, RAW, ("small", lambda cu: 8 * cu + 1), R("LDS", "GTAB")),
]


def sized(what):
    """("small", lambda cu: 16 * cu + 1) -> ("small", n) on this device"""
    return (what[0], int(what[1](cu_count()))) if isinstance(what, tuple) else what


@pytest.mark.parametrize("name,env,flags,what,route", FAST, ids=[v[0] for v in FAST])
def test_fast_route_on_device_arena(oracle, name, env, flags, what, route):
    """one route of LZ4Codec.Encode below L03_HC: every call took exactly the variant's route; out_len is the oracle's for every
    block, 0 where the output did not fit; every accepted block's bytes are the oracle's and the rest of its slot untouched; every
    byte outside all slots -- both guards of every slot, REJECTED and zero-capacity ones included -- is what was uploaded; the
    sources are unchanged; the context reports no trouble"""
    run_variant(oracle, "fast", flags, env, sized(what), route, expect_flags=flags & ~(NO_REORDER | NO_SPLIT))


@pytest.mark.parametrize("profile,route", [(4, TWO_STEP), (0, R("PROF"))], ids=["stamped", "prof twin"])
def test_fast_profiled_on_device_arena(oracle, profile, route):
    """k4lz4_profile_batch_device: the ordinary kernels stamping every block, and the instrumented one-kernel twin, on 20 cases
    per kind of block (below 65 547 bytes) -- the same limits, LZ4Codec's returns (the call takes no flags)"""
    run_variant(oracle, "fast", 0, {}, "20 per tag", route, profile=profile)


OTHER = [  # mode, name, environment, flags, shape, route
    ("fast-x32", "default", {}, X32, "64k + 100", TWO_STEP),
    ("fast-x32", "one-kernel", {"K4LZ4_NO_PARSE": "1"}, X32, "64k + 100", R("MORE")),
    ("fast-copy", "default", {}, ACOPY, "full", TWO_STEP | COPY),
    ("fast-copy", "persistent", {}, ACOPY, ("small", lambda cu: 16 * cu + 1), TWO_STEP | R("QUEUE", "PERSISTENT") | COPY),
    ("fast-copy", "one-kernel device split", {"K4LZ4_NO_PARSE": "1"}, ACOPY, ("small", lambda cu: 8 * cu + 52), DEVICE_SPLIT | COPY),
    # FLAG_SEGMENTS: a ragged batch is ONE launch; beyond 16 per CU k4_parse_kernel's waves take their blocks from the queue
    ("fast-seg", "default", {}, SEG, "full", TWO_STEP_SEG),
    ("fast-seg", "default, one call", {}, SEG, "full, one call", queue_if_more_than(16, TWO_STEP_SEG)),
    ("fast-seg", "no-parse-seg, up to 512", {"K4LZ4_NO_PARSE_SEG": "1"}, SEG, "512 with the cut", R("LDS", "SEGMENTS")),
    ("fast-seg", "no-parse-seg, device split", {"K4LZ4_NO_PARSE_SEG": "1"}, SEG, ("small + cut", lambda cu: 8 * cu + 52), DEVICE_SPLIT | R("SEGMENTS")),
    ("fast-seg", "no-segments", {"K4LZ4_NO_SEGMENTS": "1"}, SEG, "full", R("PARSE", "PARSE_BIG", "REST", "MIGRATE")),
    ("fast-seg", "join encodes again", {"K4LZ4_SEG_SPIN_MAX": "1"}, SEG, "full", TWO_STEP_SEG),
    # ... with ALLOW_COPY segments and the two-step encoder go off: the one-kernel encoders take the 150 000-byte blocks whole
    ("fast-seg", "allow-copy", {}, SEG | ACOPY, "full", R("MORE") | COPY),
    ("fast-seg", "allow-copy, one call", {}, SEG | ACOPY, "full, one call", lambda cu, counts: [(DEVICE_SPLIT if n > 8 * cu and n > 512 else R("MORE")) | COPY for n in counts]),
    ("fast-seg", "allow-copy, no-parse-seg", {"K4LZ4_NO_PARSE_SEG": "1"}, SEG | ACOPY, "full", R("MORE") | COPY),
    ("fast-seg", "allow-copy, no-segments", {"K4LZ4_NO_SEGMENTS": "1"}, SEG | ACOPY, "full", R("MORE") | COPY),
    ("fast-seg", "allow-copy, join encodes again", {"K4LZ4_SEG_SPIN_MAX": "1"}, SEG | ACOPY, "full", R("MORE") | COPY),
    ("hc3", "default", {}, 0, "full by longest block", HC3),
    ("hc3", "allow-copy", {}, ACOPY, "full by longest block", both(HC3, COPY)),
    ("hc3", "one wave", {"K4LZ4_HC_SEGS": "1"}, 0, "full by longest block", (HC3[0] ^ R("HC_PARSE_SEG4", "HC_PARSE_REC"), HC3[1])),
    ("hc3", "two waves", {"K4LZ4_HC_SEGS": "2"}, 0, "full by longest block", (HC3[0] ^ R("HC_PARSE_SEG4", "HC_PARSE_SEG2"), HC3[1])),
    ("hc3", "no records", {"K4LZ4_NO_HC_RECORDS": "1"}, 0, "full by longest block", (HC3[0] ^ R("HC_PARSE_SEG4", "HC_PARSE"), HC3[1])),
    ("hc3", "chain-lds", {"K4LZ4_HC_CHAIN_OLD": "1"}, 0, "full by longest block", (HC3[0] ^ R("HC_CHAIN_PART", "HC_CHAIN_LDS"), HC3[1])),
    ("hc3", "cand-mem", {"K4LZ4_HC_CAND_MEM": "1"}, 0, "full by longest block", (HC3[0] ^ R("HC_CAND_LDS", "HC_CAND_MEM"), HC3[1])),
    # no block of 8 KiB (HC_SEG_MIN_LEN) in the call: one wave per block whatever their number.  (launch_hc's other way down to
    # one wave, `cnt * 2 <= slots` failing, is NOT watched here: its chunk is 4096 blocks and slots = 32 per CU, so on a part of
    # 256 CUs the condition always holds; only a smaller part, or another chunk size, can reach it.)
    ("hc3", "short blocks", {}, 0, ("small", lambda cu: 16 * cu + 1), HC3[0] ^ R("HC_PARSE_SEG4", "HC_PARSE_REC")),
    ("hc9", "default", {}, 0, "full by longest block", HC9),
    ("hc9", "allow-copy", {}, ACOPY, "full by longest block", both(HC9, COPY)),
    ("hc9", "cand-mem", {"K4LZ4_HC_CAND_MEM": "1"}, 0, "full by longest block", (HC9[0] ^ R("HC_CAND_LDS", "HC_CAND_MEM"), HC9[1])),
    ("opt10", "default", {}, 0, "full by longest block", OPT),
    ("opt10", "allow-copy", {}, ACOPY, "full by longest block", both(OPT, COPY)),
    ("opt10", "cand-mem", {"K4LZ4_HC_CAND_MEM": "1"}, 0, "full by longest block", OPT),          # (levels 10 and up take no candidate records)
    ("pickle", "default", {}, 0, "full, one call", TWO_STEP_SEG | ENV),
    ("pickle", "no-segments", {"K4LZ4_NO_SEGMENTS": "1"}, 0, "full, one call", R("PICKLE")),
    ("pickle-hc3", "default", {}, 0, "full by longest block", both(HC3, ENV)),
    ("wrap", "default", {}, 0, "full, one call", TWO_STEP_SEG | ENV),
    ("wrap", "high", {}, 1, "full by longest block", both(HC9, ENV)),
]


@pytest.mark.parametrize("mode,name,env,flags,what,route", OTHER, ids=[f"{v[0]}: {v[1]}" for v in OTHER])
def test_route_on_device_arena(oracle, mode, name, env, flags, what, route):
    """the same for the other ways of calling the encoders: the 32-bit engine's bytes, ALLOW_COPY (-srcLen and the raw bytes, 0
    where the reference throws -- also for U <= capacity < r), FLAG_SEGMENTS with capacities around U - 1, the HC levels by the
    longest block of a call, and the envelopes (-1 below 5 + U or 8 + U, with both guards in place)"""
    run_variant(oracle, mode, flags, env, sized(what), route)


def test_route_witness_is_cleared_by_encodes_and_left_alone_by_decodes(oracle):
    """k4lz4_last_encode_route: nothing before the first encode; an encode's route; a decode leaves it; the next encode replaces it"""
    import torch
    from k4os.compression.lz4_amd import corpus
    from k4os.compression.lz4_amd.device import DeviceBatch
    if _trouble:
        pytest.fail(f"not run: the device calls of '{_trouble[0]}' failed")
    codec = codec_under({})
    try:
        assert codec.ctx.last_encode_route() == K.ENCODE_ROUTE_NONE
        blocks = np.stack([corpus.class_bytes("xml", 4096, k) for k in range(4)])
        src = DeviceBatch.from_host(blocks.reshape(-1), np.arange(4, dtype=np.uint64) * 4096, np.full(4, 4096, np.int32), codec.device)
        comp = DeviceBatch.empty_slots(np.full(4, 4400), codec.device)
        clen = codec.encode(src, comp)
        assert codec.ctx.last_encode_route() == TWO_STEP
        back = DeviceBatch.empty_slots(np.full(4, 4096), codec.device)
        dlen = codec.decode(DeviceBatch(comp.data, comp.off, clen), back)
        assert codec.ctx.last_encode_route() == TWO_STEP
        codec.encode(src, comp, level=9)
        assert codec.ctx.last_encode_route() == HC9[0]
        torch.cuda.synchronize(codec.device)
        assert (dlen.cpu().numpy() == 4096).all() and np.array_equal(back.data.cpu().numpy()[:4 * 4096].reshape(4, 4096), blocks)
    finally:
        codec.ctx.close()
