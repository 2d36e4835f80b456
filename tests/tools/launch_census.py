#!/usr/bin/env python3
"""Launch census: one call per routing case of the batch launcher (csrc/k4lz4_launch.hpp), to be run under a kernel trace, so that
two builds can be compared by the launches they make -- bytes cannot show that a batch quietly took a slower route.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tests/tools/launch_census.py     (on each build)
    python tests/tools/launch_census.py --trim OUT/.../*_kernel_trace.csv profiles/launch_census.csv
    python tests/tools/launch_census.py --compare profiles/launch_census_parent.csv profiles/launch_census.csv
    python tests/tools/launch_census.py --time        (small-call host cost: medians of 2000 one-block calls, one JSON line)

A driver, not a test: no assertions on results.  --compare exits non-zero when the two traces differ as multisets of
(kernel name, grid, workgroup size, LDS bytes); order and queues may differ (kernels on the side queues run beside the main one).
Block counts are relative to the chip's CU count, read from the device.  Switches are read when a context is made, so every
switch gets a context of its own."""
from __future__ import annotations

import collections
import contextlib
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

COLUMNS = {"name": ("Kernel_Name",), "grid": ("Grid_Size", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"),
           "workgroup": ("Workgroup_Size", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z"),
           "lds": ("LDS_Block_Size", "Group_Segment_Size")}


def read_trace(path):
    """a kernel trace (raw, or trimmed by --trim) as a Counter of (name, grid, workgroup, lds) tuples"""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = collections.Counter()
    for r in rows:
        key = []
        for what, names in COLUMNS.items():
            vals = [r[c] for c in names if c in r]
            if not vals:
                raise SystemExit(f"{path}: no column for {what} (one of {names}); has {list(r)}")
            key.append("x".join(vals))
        out[tuple(key)] += int(r.get("Launches", 1))
    return out


def trim(raw, out):
    """the four columns the comparison reads, equal launches counted on one row"""
    rows = read_trace(raw)
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Kernel_Name", "Grid_Size", "Workgroup_Size", "LDS_Block_Size", "Launches"])
        w.writerows(k + (n,) for k, n in sorted(rows.items()))
    print(f"{out}: {sum(rows.values())} launches, {len(rows)} kinds")


def compare(a, b):
    ca, cb = read_trace(a), read_trace(b)
    bad = 0
    for k in sorted(set(ca) | set(cb)):
        if ca[k] != cb[k]:
            bad += 1
            print(f"{ca[k]:5d} x in {a}, {cb[k]:5d} x in {b}: {k[0]} grid {k[1]} workgroup {k[2]} LDS {k[3]}")
    print(f"{sum(ca.values())} launches in {a}, {sum(cb.values())} in {b}: {bad} kinds of launch differ")
    return 1 if bad else 0


@contextlib.contextmanager
def switches(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def drive(timing):
    import numpy as np
    import torch
    from k4os.compression.lz4_amd import LZ4Codec, LZ4Legacy, LZ4Level, LZ4Pickler, _native, corpus, make_arena, pack_blocks
    from k4os.compression.lz4_amd._native import (FLAG_ALLOW_COPY, FLAG_NO_REORDER, FLAG_NO_SPLIT, FLAG_REORDER, FLAG_SEGMENTS, FLAG_X32)
    from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec

    torch.cuda.set_device(0)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    dev = torch.device("cuda", 0)
    pool = corpus.silesia_like_blocks(24 * cu + 1, 256, seed=41)

    def small(n, size=256):
        return [pool[i % len(pool)][:size] for i in range(n)]

    def codec(**env):
        with switches({k: str(v) for k, v in env.items()}):
            return DeviceCodec(0)

    def host_ctx(**env):
        with switches({k: str(v) for k, v in env.items()}):
            return _native.Context(-1)

    def to_device(blocks):
        return DeviceBatch.from_host(*pack_blocks(blocks), dev)

    def encode(dc, blocks, flags=0, level=LZ4Level.L00_FAST, call="encode", bound=LZ4Codec.MaximumOutputSize):
        src = to_device(blocks)
        dst = DeviceBatch.empty_slots(np.array([bound(b.size) for b in blocks]), dev)
        out = getattr(dc, call)(src, dst, level=level, flags=flags)
        torch.cuda.synchronize()
        return src, dst, out

    dc0 = codec()

    def decode(dc, blocks, flags=0, call="decode", packed_by="encode", bound=LZ4Codec.MaximumOutputSize, dicts=False):
        _, comp, clen = encode(dc0, blocks, call=packed_by, bound=bound)
        back = DeviceBatch.empty_slots(np.array([b.size for b in blocks]), dev)
        src = DeviceBatch(comp.data, comp.off, clen)
        if dicts:
            d = to_device(small(len(blocks), 64))
            dc.decode_dict(src, back, d.data, d.off, d.length)
        elif call == "decode":
            dc.decode(src, back, flags=flags)
        else:
            dc.unpickle(src, back)
        torch.cuda.synchronize()

    def host_encode(ctx, blocks, flags=0):
        src, soff, slen = pack_blocks(blocks)
        caps = np.array([LZ4Codec.MaximumOutputSize(b.size) for b in blocks], np.int32)
        dst, doff = make_arena(caps)
        LZ4Codec.EncodeBatchPacked(src, soff, slen, dst, doff, caps, flags=flags, ctx=ctx)

    if timing:
        one = small(1)
        src = to_device(one)
        dst = DeviceBatch.empty_slots(np.array([LZ4Codec.MaximumOutputSize(256)]), dev)
        out = dc0.new_out_len(1)
        back = DeviceBatch.empty_slots(np.array([256]), dev)
        dc0.encode(src, dst, out)
        torch.cuda.synchronize()
        comp = DeviceBatch(dst.data, dst.off, out.clone())
        res = {}
        for name, fn in (("encode_1_block_us", lambda: dc0.encode(src, dst, out)), ("decode_1_block_us", lambda: dc0.decode(comp, back, out))):
            t = []
            for i in range(2200):
                t0 = time.perf_counter()
                fn()
                dc0.ctx.synchronize(dc0._stream())
                t.append(time.perf_counter() - t0)
            res[name] = round(float(np.median(t[200:])) * 1e6, 2)
        print(json.dumps(res))
        return

    big3 = [corpus.class_bytes("samba", n, 3) for n in (65547, 70000, 150000)]
    two_mib = corpus.class_bytes("dickens", 2 << 20, 1)
    ragged = small(600) + [two_mib]
    hc20 = [b for b in corpus.silesia_like_blocks(20, 8192, seed=42)]
    lib = _native.load_library()

    # fast encode, device buffers, default context
    for n in (1, 300, 2049, 16 * cu, 16 * cu + 1):
        encode(dc0, small(n))
    encode(dc0, small(16 * cu + 1), FLAG_NO_REORDER)
    encode(dc0, small(600), FLAG_NO_SPLIT)
    encode(dc0, small(8 * cu + 52), FLAG_NO_SPLIT)
    encode(dc0, small(600), FLAG_ALLOW_COPY)
    encode(dc0, small(600), FLAG_X32)
    encode(dc0, small(37) + big3)
    text = corpus.lorem(4096)
    target = np.zeros(LZ4Codec.MaximumOutputSize(text.size), np.uint8)
    lib.k4lz4_compress_fast(text.ctypes.data, target.ctypes.data, text.size, target.size, 2)
    # segments
    encode(dc0, ragged, FLAG_SEGMENTS)
    encode(dc0, ragged, FLAG_SEGMENTS | FLAG_ALLOW_COPY)
    encode(dc0, small(10) + [two_mib], FLAG_SEGMENTS | FLAG_ALLOW_COPY)
    # host-pointer form: the lengths are known on the host
    hc = host_ctx()
    host_encode(hc, small(300, 100))
    host_encode(hc, small(300))
    host_encode(hc, [b[:100] if i % 2 else b for i, b in enumerate(small(300))])
    # pickle / wrap (host-pointer form: a small batch without a big message keeps k4_pickle_kernel; and on device buffers)
    LZ4Pickler.PickleBatch(small(100), ctx=hc)
    LZ4Pickler.PickleBatch(small(600), ctx=hc)
    LZ4Pickler.PickleBatch(small(19) + [two_mib], ctx=hc)
    LZ4Legacy.WrapBatch(small(3), ctx=hc)
    LZ4Pickler.PickleBatch(small(20), level=LZ4Level.L03_HC, ctx=hc)
    LZ4Legacy.WrapBatch(small(20), high=True, ctx=hc)
    encode(dc0, small(600), call="pickle", bound=lib.k4lz4_pickle_bound)
    # HC
    for level in (LZ4Level.L03_HC, LZ4Level.L09_HC, LZ4Level.L10_OPT):
        encode(dc0, hc20, level=level)
    encode(dc0, [corpus.class_bytes("samba", 100000, s) for s in (5, 6)], level=LZ4Level.L03_HC)
    # decode, unpickle
    for n in (5, 12 * cu + 1, 16 * cu + 1, 24 * cu + 1):
        decode(dc0, small(n))
    decode(dc0, small(600), FLAG_REORDER)
    decode(dc0, small(20), dicts=True)
    for blocks in (small(5), small(100), small(12 * cu + 1, 20), small(64 * cu + 1, 20)):
        decode(dc0, blocks, call="unpickle", packed_by="pickle", bound=lib.k4lz4_pickle_bound)
    hc.close()
    # the profiling twins (0 encode, 1 decode, 2 pair decode) and the ordinary kernels stamping (4 encode, 5 decode)
    src, comp, clen = encode(dc0, small(20))
    for mode in (0, 4):
        dc0.profile(mode, src, comp)
    back = DeviceBatch.empty_slots(np.full(20, 256), dev)
    for mode in (1, 2, 5):
        dc0.profile(mode, DeviceBatch(comp.data, comp.off, clen), back)
    torch.cuda.synchronize()
    # one fresh context per switch
    for env in ({"K4LZ4_NO_PARSE": 1}, {"K4LZ4_NO_INLINE_EMIT": 1}, {"K4LZ4_NO_PERSIST": 1}, {"K4LZ4_PARSE_QUEUE": 1, "K4LZ4_PARSE_WAVES": 3},
                {"K4LZ4_NO_PCOST": 1}, {"K4LZ4_NO_MIGRATE": 1}, {"K4LZ4_NO_PACE": 1}, {"K4LZ4_SPLIT_PCT": 30}):
        dc = codec(**env)
        encode(dc, small(2049))
        encode(dc, small(16 * cu + 1))
    encode(codec(K4LZ4_NO_PARSE_BIG=1), small(37) + big3)
    for env in ({"K4LZ4_NO_PARSE_SEG": 1}, {"K4LZ4_NO_SEGMENTS": 1}):
        dc = codec(**env)
        encode(dc, small(2049))
        encode(dc, ragged, FLAG_SEGMENTS)
        # (without the two-step way for ragged batches: the one-kernel pair with its *_seg twins, the single *_seg launch)
        encode(dc, small(8 * cu + 52) + [two_mib], FLAG_SEGMENTS)
        encode(dc, small(10) + [two_mib], FLAG_SEGMENTS)
    dc = codec(K4LZ4_NO_PAIR=1)
    encode(dc, small(2049))
    decode(dc, small(5))
    decode(dc, small(5), call="unpickle", packed_by="pickle", bound=lib.k4lz4_pickle_bound)
    for env in ({"K4LZ4_NO_HC_RECORDS": 1}, {"K4LZ4_HC_CHAIN_OLD": 1}, {"K4LZ4_HC_CAND_MEM": 1}, {"K4LZ4_HC_SEGS": 2}):
        dc = codec(**env)
        encode(dc, small(2049))
        encode(dc, hc20, level=LZ4Level.L03_HC)
    torch.cuda.synchronize()
    print(f"launch census done on {cu} CUs")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 4 and sys.argv[1] == "--trim":
        trim(sys.argv[2], sys.argv[3])
    elif sys.argv[1:] in ([], ["--time"]):
        drive(timing=bool(sys.argv[1:]))
    else:
        sys.exit(__doc__)
