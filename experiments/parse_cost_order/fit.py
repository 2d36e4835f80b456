"""Fit of the dry parse's counts to the stamped LDS durations of the bench batch's 384 different blocks, per sample (see README.md).
Usage: fit.py WORKDIR"""
import ctypes as C, os, sys, subprocess, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
WORK = sys.argv[1]          # a working directory: libstudy.so (fit_stats.cpp built like tests/emu/Makefile builds the emulator) and the *_blocks.npy of stamp_dump.py
from k4os.compression.lz4_amd import corpus
so = os.path.join(WORK, "libstudy.so")
lib = C.CDLL(so)
n, bs = 4096, 65536
cache = os.path.join(WORK, "blocks.npy")
if os.path.exists(cache): blocks = np.load(cache)
else:
    blocks = corpus.silesia_like_blocks(n, bs, seed=2); np.save(cache, blocks)
uidx = np.array([ci + 12 * t for ci in range(12) for t in range(32)])
ub = np.ascontiguousarray(blocks[uidx])
off = (np.arange(384, dtype=np.uint64) * bs); lens = np.full(384, bs, np.int32)
def stats(o, l):
    out = np.zeros((384, 8), np.uint32)
    lib.study_stats(ub.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_void_p(off.ctypes.data), C.c_void_p(lens.ctypes.data), C.c_longlong(384), C.c_uint32(o), C.c_uint32(l), C.c_void_p(out.ctypes.data), C.c_int(8), C.c_uint32(0), C.c_int(0))     # (form 0: the block's own table; the sample's: fit_sample_table.py)
    return out[:, :6].astype(np.float64), out[:, 6].astype(np.float64)
# truth
b = np.arange(n); u = (b % 12) * 32 + (b // 12) % 32
ls = np.zeros(384); ln = np.zeros(384); ms = np.zeros(384); mn = np.zeros(384)
for f in ("parent_blocks", "oracleP_blocks", "oracleQ_blocks"):
    res = np.load(os.path.join(WORK, "%s.npy" % f))
    for r in res:
        d = (r[:, 1] - r[:, 0]) / 1e5; k = r[:, 2].astype(int)
        np.add.at(ls, u[k == 4], d[k == 4]); np.add.at(ln, u[k == 4], 1)
        np.add.at(ms, u[k != 4], d[k != 4]); np.add.at(mn, u[k != 4], 1)
lds = np.where(ln > 0, ls / np.maximum(ln, 1), np.nan); mem = np.where(mn > 0, ms / np.maximum(mn, 1), np.nan)
both = (ln >= 2) & (mn >= 2)
ratio = np.median(mem[both] / lds[both]); print("ratio", ratio, "both", both.sum(), "lds known", (ln > 0).sum())
truth = np.where(np.isnan(lds), mem / ratio, lds)
np.save(os.path.join(WORK, "truth.npy"), truth)
names = corpus.SILESIA_NAMES
def evaluate(tag, est):
    # batch-level: top 2304 by est get LDS
    e = est[u] + 1e-9 * np.random.default_rng(0).random(n)
    t = truth[u]
    cut = np.sort(e)[::-1][2303]
    inl = e >= cut
    tail_mem = (t[~inl] * ratio).max(); tail_lds = t[inl].max()
    tcut = np.sort(t)[::-1][2303]
    mis = ((t >= tcut) & ~inl).sum()
    from scipy.stats import spearmanr
    rho = spearmanr(est, truth).correlation
    # heavy memory blocks: how many memory-start blocks have predicted mem time above 2.75
    print("%-28s rho %.3f misplaced %4d  tail mem %.3f lds %.3f  mem>2.7: %4d  mem>2.85: %4d" % (tag, rho, mis, tail_mem, tail_lds, (t[~inl] * ratio > 2.7).sum(), (t[~inl] * ratio > 2.85).sum()))
evaluate("truth", truth)
full, _ = stats(0, 65536)
np.save(os.path.join(WORK, "full.npy"), full)
for ci, nm in enumerate(names):
    s = full[ci * 32:(ci + 1) * 32]
    print("%-8s truth %.3f | rounds %6.0f slow %6.0f nseq %6.0f groups %6.0f lazies %6.0f longs %6.0f" % ((nm, truth[ci * 32:(ci + 1) * 32].mean()) + tuple(s.mean(0))))
# fit on full stats: truth ~ w . stats + c
A = np.c_[full, np.ones(384)]
w, *_ = np.linalg.lstsq(A, truth, rcond=None)
print("fit full (ms per unit):", w, "resid rms", np.sqrt(((A @ w - truth) ** 2).mean()))
from scipy.optimize import nnls
w2, _ = nnls(A, truth); print("nnls:", w2, "rms", np.sqrt(((A @ w2 - truth) ** 2).mean()))
evaluate("full stats, lstsq", A @ w)
evaluate("full stats, nnls", A @ w2)
evaluate("full stats, old pcost w", full @ np.array([6500, 3000, 120, 150, 480, 1500.]))
evaluate("full rounds only", full[:, 0])
for (o, l) in ((0, 256), (0, 512), (0, 1024), (0, 2048), (0, 3072), (32768, 512), (32768, 1024), (16384, 1024), (4096, 1024), (1024, 1024)):
    s, sl = stats(o, l)
    sc = s * (bs / sl)[:, None]
    evaluate("sample %d+%d nnls-w" % (o, l), np.c_[sc, np.ones(384)] @ w2)
    evaluate("sample %d+%d lstsq-w" % (o, l), np.c_[sc, np.ones(384)] @ w)
    evaluate("sample %d+%d oldw" % (o, l), sc @ np.array([6500, 3000, 120, 150, 480, 1500.]))
    # refit on the sample itself
    As = np.c_[sc, np.ones(384)]; ws, _ = nnls(As, truth)
    evaluate("sample %d+%d refit" % (o, l), As @ ws); print("    refit w", np.round(ws, 6))
    np.save(os.path.join(WORK, "s_%d_%d.npy" % (o, l)), sc)
