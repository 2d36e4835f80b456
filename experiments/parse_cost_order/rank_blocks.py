#!/usr/bin/env python
"""Per-block cost buckets for the throw-away oracle order from the parent's per-block stamps (stamp_dump.py).
The bench batch tiles 32 unique blocks per class: unique block u = (b % 12, (b // 12) % 32).  Per u: mean duration of its instances
that had an LDS table all the time, mean duration of the others.  ratio = median over the u that have both of (other / LDS).
P: bucket by the LDS duration (a u without an LDS instance: other / ratio).
Q: bucket by the duration with a start in memory (a u without one: LDS x ratio).
Usage: rank_blocks.py parent.npy OUT_P.bin OUT_Q.bin"""
import sys
import numpy as np
res = np.load(sys.argv[1])
reps, n, _ = res.shape
b = np.arange(n)
u = (b % 12) * 32 + (b // 12) % 32
dur = (res[:, :, 1] - res[:, :, 0]) / 1e5
k = res[:, :, 2].astype(int)
lds_s = np.zeros(384); lds_n = np.zeros(384); mem_s = np.zeros(384); mem_n = np.zeros(384)
for r in range(reps):
    np.add.at(lds_s, u[k[r] == 4], dur[r][k[r] == 4]); np.add.at(lds_n, u[k[r] == 4], 1)
    np.add.at(mem_s, u[k[r] != 4], dur[r][k[r] != 4]); np.add.at(mem_n, u[k[r] != 4], 1)
lds = np.where(lds_n > 0, lds_s / np.maximum(lds_n, 1), np.nan)
mem = np.where(mem_n > 0, mem_s / np.maximum(mem_n, 1), np.nan)
both = (lds_n >= 2) & (mem_n >= 2)
ratio = float(np.median(mem[both] / lds[both])) if both.any() else 1.17
P = np.where(np.isnan(lds), mem / ratio, lds)
Q = np.where(np.isnan(mem), lds * ratio, mem)
print("unique blocks with LDS stamps %d, with others %d, with both %d; ratio other / LDS %.3f" % ((lds_n > 0).sum(), (mem_n > 0).sum(), both.sum(), ratio))
for tag, est, path in (("P", P, sys.argv[2]), ("Q", Q, sys.argv[3])):
    bkt = np.clip(np.round(est / (est.max() * 1.0001) * 63.0), 0, 63).astype(np.uint8)
    bkt[u].tofile(path)
    cut = np.sort(est[u])[::-1][2304 - 1]
    print("%s: estimate ms min %.3f max %.3f; the 2304th most expensive block has %.3f; LDS share per class:" % (tag, est.min(), est.max(), cut),
          " ".join("%d:%.2f" % (c, float((est[u][c::12] >= cut).mean())) for c in range(12)))
