#!/usr/bin/env python
"""Per-block encode stamps of the bench batch (profile mode 4): REPS launches, saved as [REPS, n, 4] float64 = start, end, placement
(4 LDS, 5 memory, 6 memory then LDS), parse-through; run from the root of the tree whose library is to be stamped.
Usage: stamp_dump.py OUT.npy [REPS]"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.getcwd())
from k4os.compression.lz4_amd import LZ4Codec, corpus
from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec

out, reps = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 4
n, bs = 4096, 65536
blocks = corpus.silesia_like_blocks(n, bs, seed=2)
dc = DeviceCodec(0)
lens = np.full(n, bs, np.int32)
off = np.arange(n, dtype=np.uint64) * bs
src = DeviceBatch.from_host(blocks.reshape(-1), off, lens, dc.device)
comp = DeviceBatch.empty_slots(np.full(n, LZ4Codec.MaximumOutputSize(bs)), dc.device)
dc.encode(src, comp)
torch.cuda.synchronize()
res = []
for rep in range(reps + 1):
    _, c = dc.profile(4, src, comp)
    torch.cuda.synchronize()
    c = c.cpu().numpy().astype(np.float64)
    if rep: res.append(np.stack([c[:, 8], c[:, 9], c[:, 11], c[:, 12]], axis=1))
res = np.stack(res)
np.save(out, res)
for r in res:
    st, en, k = r[:, 0], r[:, 1], r[:, 2].astype(int)
    t0 = st.min()
    print("span ms %.3f | LDS n %d last end %.3f | memory n %d last end %.3f | moved n %d last end %.3f" % (
        (en.max() - t0) / 1e5, (k == 4).sum(), (en[k == 4].max() - t0) / 1e5, (k == 5).sum(), (en[k == 5].max() - t0) / 1e5 if (k == 5).any() else 0,
        (k == 6).sum(), (en[k == 6].max() - t0) / 1e5 if (k == 6).any() else 0))
names = corpus.SILESIA_NAMES
r = res[-1]
k = r[:, 2].astype(int)
for ci, name in enumerate(names):
    idx = np.arange(ci, n, 12)
    d = (r[idx, 1] - r[idx, 0]) / 1e5
    kk = k[idx]
    print("  %-8s LDS %3d mem %3d moved %3d | dur LDS mean %.3f max %.3f | not-LDS mean %.3f max %.3f | end max %.3f" % (
        name, (kk == 4).sum(), (kk == 5).sum(), (kk == 6).sum(),
        d[kk == 4].mean() if (kk == 4).any() else 0, d[kk == 4].max() if (kk == 4).any() else 0,
        d[kk != 4].mean() if (kk != 4).any() else 0, d[kk != 4].max() if (kk != 4).any() else 0, (r[idx, 1].max() - r[:, 0].min()) / 1e5))
