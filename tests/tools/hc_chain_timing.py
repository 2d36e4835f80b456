#!/usr/bin/env python
"""Chained against independent HC blocks on one batch (device-resident, k4lz4_encode_hc_chain_batch_device against
k4lz4_encode_batch_device on the same 64 KiB blocks), and the liblz4 witness (tests/hc_chain_witness.py) on the host's
threads; the GPU's chained bytes are checked against the witness.  One JSON line per level.

    python tests/tools/hc_chain_timing.py --streams 256 --mib 4 --levels 3 9 --reps 5
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
import hc_chain_witness as W  # noqa: E402
from k4os.compression.lz4_amd import _native, corpus  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--mib", type=int, default=4)
    ap.add_argument("--block", type=int, default=65536)
    ap.add_argument("--levels", type=int, nargs="+", default=[3, 9])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--check", type=int, default=16, help="streams whose bytes are compared with the witness")
    a = ap.parse_args()
    ns, N, B = a.streams, a.mib << 20, a.block
    classes = ["dickens", "mozilla", "xml", "webster", "nci", "samba", "x-ray", "ooffice"]
    contents = [corpus.class_bytes(classes[s % len(classes)], N, 100 + s) for s in range(ns)]
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
    # independent blocks: the same 64 KiB blocks, one slot each
    d_boff = torch.from_numpy((np.arange(nb, dtype=np.uint64) * np.uint64(B)).view(np.int64)).to(dev)
    d_blen = torch.full((nb,), B, dtype=torch.int32, device=dev)
    d_sloff = torch.from_numpy((np.arange(nb, dtype=np.uint64) * np.uint64(slot)).view(np.int64)).to(dev)
    d_cap = torch.full((nb,), slot, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def chained(level):
        ctx.check(lib.k4lz4_encode_hc_chain_batch_device(ctx.handle, d_src.data_ptr(), soff.ctypes.data, slen.ctypes.data, bsz.ctypes.data,
                                                         ext.ctypes.data, None, ns, d_dst.data_ptr(), doff.ctypes.data, d_out.data_ptr(),
                                                         nb, level, _native.FLAG_ALLOW_COPY, stream))

    def independent(level):
        ctx.check(lib.k4lz4_encode_batch_device(ctx.handle, d_src.data_ptr(), d_boff.data_ptr(), d_blen.data_ptr(), d_dst.data_ptr(),
                                                d_sloff.data_ptr(), d_cap.data_ptr(), d_out.data_ptr(), nb, level, _native.FLAG_ALLOW_COPY,
                                                stream))

    def timed(fn, level):
        fn(level)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(level)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), float(min(ts))

    for level in a.levels:
        ind_ms, ind_min = timed(independent, level)
        ch_ms, ch_min = timed(chained, level)
        out = d_out.cpu().numpy()
        dst = d_dst.cpu().numpy()
        ok = True
        for s in range(min(a.check, ns)):
            want = W.witness_blocks(contents[s], level, B, 0)
            for j, (n, data) in enumerate(want):
                k = s * nblk + j
                at = int(doff[s]) + j * slot
                ok = ok and int(out[k]) == n and dst[at:at + abs(n)].tobytes() == data
        n_host = min(ns, 4 * a.threads)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(a.threads) as ex:
            list(ex.map(lambda c: W.witness_blocks(c, level, B, 0), contents[:n_host]))
        host_s = time.perf_counter() - t0
        gib = ns * N / (1 << 30)
        print(json.dumps({"level": level, "streams": ns, "stream_mib": a.mib, "block": B, "blocks": nb,
                          "independent_ms": round(ind_ms, 2), "chained_ms": round(ch_ms, 2), "chained_over_independent": round(ch_ms / ind_ms, 3),
                          "independent_gibs": round(gib / (ind_ms / 1e3), 2), "chained_gibs": round(gib / (ch_ms / 1e3), 2),
                          "witness_host_gibs": round(n_host * N / (1 << 30) / host_s, 3), "witness_threads": a.threads,
                          "checked_streams": min(a.check, ns), "bit_exact": bool(ok)}), flush=True)


if __name__ == "__main__":
    main()
