#!/usr/bin/env python
"""Chained against independent L00_FAST blocks on one batch (device-resident: k4lz4_encode_fast_chain_batch_device against
k4lz4_encode_batch_device on the same blocks), and the liblz4 witness (tests/fast_chain_witness.py) on the host's threads; the
GPU's chained bytes are checked against the witness on a subset of the streams.  One JSON line per shape.

    python tests/tools/fast_chain_timing.py --shapes 256x4 4096x1 --reps 5
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import fast_chain_witness as W  # noqa: E402
from k4os.compression.lz4_amd import _native, corpus  # noqa: E402


def run(ns, mib, B, reps, threads, check):
    N = mib << 20
    classes = ["dickens", "mozilla", "xml", "webster", "nci", "samba", "x-ray", "ooffice"]
    distinct = [corpus.class_bytes(classes[s % len(classes)], N, 100 + s) for s in range(min(ns, 16))]
    contents = [distinct[s % len(distinct)] for s in range(ns)]          # (16 distinct contents, repeated: the kernel does not care)
    src = np.concatenate(contents)
    soff = (np.arange(ns, dtype=np.uint64) * np.uint64(N))
    slen = np.full(ns, N, np.int64)
    bsz = np.full(ns, B, np.int32)
    ext = np.zeros(ns, np.int32)
    nblk = N // B
    nb = ns * nblk
    slot = B + B // 255 + 16
    doff = (np.arange(ns, dtype=np.uint64) * np.uint64(nblk * slot))
    ctx = _native.default_context()
    lib = ctx.lib
    dev = torch.device("cuda", ctx.device)
    d_src = torch.from_numpy(src).to(dev)
    d_dst = torch.empty(nb * slot + 64, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(nb, dtype=torch.int32, device=dev)
    d_boff = torch.from_numpy((np.arange(nb, dtype=np.uint64) * np.uint64(B)).view(np.int64)).to(dev)
    d_blen = torch.full((nb,), B, dtype=torch.int32, device=dev)
    d_sloff = torch.from_numpy((np.arange(nb, dtype=np.uint64) * np.uint64(slot)).view(np.int64)).to(dev)
    d_cap = torch.full((nb,), slot, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def chained():
        ctx.check(lib.k4lz4_encode_fast_chain_batch_device(ctx.handle, d_src.data_ptr(), soff.ctypes.data, slen.ctypes.data, bsz.ctypes.data,
                                                           ext.ctypes.data, None, ns, None, None, d_dst.data_ptr(), doff.ctypes.data,
                                                           d_out.data_ptr(), nb, _native.FLAG_ALLOW_COPY, stream))

    def independent():
        ctx.check(lib.k4lz4_encode_batch_device(ctx.handle, d_src.data_ptr(), d_boff.data_ptr(), d_blen.data_ptr(), d_dst.data_ptr(),
                                                d_sloff.data_ptr(), d_cap.data_ptr(), d_out.data_ptr(), nb, 0, _native.FLAG_ALLOW_COPY, stream))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    ind_ms = timed(independent)
    ch_ms = timed(chained)
    out = d_out.cpu().numpy()
    dst = d_dst.cpu().numpy()
    ok = True
    for s in range(min(check, ns)):
        want, _ = W.witness_stream(contents[s], B, 0, True)
        for j, (n, data) in enumerate(want):
            k = s * nblk + j
            at = int(doff[s]) + j * slot
            ok = ok and int(out[k]) == n and dst[at:at + abs(n)].tobytes() == data
    n_host = min(ns, 4 * threads)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda c: W.witness_stream(c, B, 0, True), contents[:n_host]))
    host_s = time.perf_counter() - t0
    gib = ns * N / (1 << 30)
    return {"streams": ns, "stream_mib": mib, "block": B, "blocks": nb, "independent_ms": round(ind_ms, 2), "chained_ms": round(ch_ms, 2),
            "chained_over_independent": round(ch_ms / ind_ms, 3), "independent_gibs": round(gib / (ind_ms / 1e3), 2),
            "chained_gibs": round(gib / (ch_ms / 1e3), 2), "witness_host_gibs": round(n_host * N / (1 << 30) / host_s, 3),
            "witness_threads": threads, "checked_streams": min(check, ns), "bit_exact": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["256x4", "4096x1"], help="streams x MiB per stream")
    ap.add_argument("--block", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--check", type=int, default=16, help="streams whose bytes are compared with the witness")
    a = ap.parse_args()
    for shape in a.shapes:
        ns, mib = (int(x) for x in shape.split("x"))
        print(json.dumps(run(ns, mib, a.block, a.reps, a.threads, a.check)), flush=True)


if __name__ == "__main__":
    main()
