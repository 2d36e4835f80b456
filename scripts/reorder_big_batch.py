#!/usr/bin/env python
"""decode of K4_BLOCKS oracle-encoded 4 KiB blocks with and without K4LZ4_FLAG_REORDER (cost by length, k4_order_kernel's plain
form over the whole batch): median ms per call of each, and their difference = what cost + order kernels take"""
import json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle_lib import Oracle
from k4os.compression.lz4_amd import LZ4Codec, corpus, make_arena
from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec
from k4os.compression.lz4_amd import _native
oracle = Oracle()
n = int(os.environ.get("K4_BLOCKS", str(1 << 19)))
bs = 4096
dc = DeviceCodec(0)
base = corpus.silesia_like_blocks(1 << 14, bs, seed=3)
blocks = np.tile(base, (-(-n // base.shape[0]), 1))[:n].copy()
# ragged lengths so that the by-length buckets are several
rng = np.random.default_rng(5)
lens = np.full(n, bs, np.int32) if os.environ.get('K4_UNIFORM') else rng.integers(64, bs + 1, n).astype(np.int32)
off = np.arange(n, dtype=np.uint64) * bs
caps = np.full(n, LZ4Codec.MaximumOutputSize(bs), np.int32)
ref, ref_off = make_arena(caps)
clen_h = oracle.encode_batch(blocks.reshape(-1), off, lens, ref, ref_off, caps, threads=16)
comp = DeviceBatch.from_host(ref, ref_off, clen_h, dc.device)
back = DeviceBatch.empty_slots(np.full(n, bs, np.int32), dc.device)
dlen = dc.new_out_len(n)
res = {"blocks": n, "uniform": bool(os.environ.get("K4_UNIFORM"))}
for name, flags in (("plain", 0), ("reorder", _native.FLAG_REORDER)):
    for _ in range(2):
        dc.decode(comp, back, dlen, flags=flags)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(11)]
    for i in range(10):
        ev[i].record(); dc.decode(comp, back, dlen, flags=flags)
    ev[10].record(); torch.cuda.synchronize()
    res[name + "_ms"] = round(sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(10))[5], 4)
    res[name + "_ok"] = bool(np.array_equal(dlen.cpu().numpy(), lens))
res["order_cost_ms"] = round(res["reorder_ms"] - res["plain_ms"], 4)
print(json.dumps(res), flush=True)
