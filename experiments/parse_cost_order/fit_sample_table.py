"""The fit of fit.py for the sample's own table (FastTable<3>): per hash width, sample and round limit, the dry parse's counts over the
384 different blocks of the bench batch, refitted without negative weights, printed as the nine fields of K4LZ4_PCOST_FIT.
Usage: fit_sample_table.py WORKDIR      (WORKDIR: libstudy13.so = any build (form 0 is the block's own table), libstudy11.so and
libstudy12.so = fit_stats.cpp built with -DK4_SAMPLE_HASH_BITS=11 / 12; truth.npy of fit.py if there is one)
Without truth.npy (the per-block stamps are not kept in the repository) the truth is section 2's fit of the WHOLE block's counts to the
stamps -- 1.28 us a round, 0.84 a strided round, 0.094 a sequence, 0.036 a group, 0.70 a long count, 0.23 ms a block; correlation
0.97 with the stamps --, which is the best estimate of a block's duration there is short of stamping it."""
import ctypes as C, os, sys, numpy as np
from scipy.optimize import nnls
from scipy.stats import spearmanr
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from k4os.compression.lz4_amd import corpus
WORK = sys.argv[1]
n, bs = 4096, 65536
cache = os.path.join(WORK, "blocks.npy")
if os.path.exists(cache): blocks = np.load(cache)
else:
    blocks = corpus.silesia_like_blocks(n, bs, seed=2); np.save(cache, blocks)
uidx = np.array([ci + 12 * t for ci in range(12) for t in range(32)])
ub = np.ascontiguousarray(blocks[uidx])
off = (np.arange(384, dtype=np.uint64) * bs); lens = np.full(384, bs, np.int32)
names = corpus.SILESIA_NAMES
b = np.arange(n); u = (b % 12) * 32 + (b // 12) % 32


def stats(lib, o, l, cap, form):
    out = np.zeros((384, 8), np.uint32)
    lib.study_stats(ub.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_void_p(off.ctypes.data), C.c_void_p(lens.ctypes.data), C.c_longlong(384), C.c_uint32(o), C.c_uint32(l),
                    C.c_void_p(out.ctypes.data), C.c_int(8), C.c_uint32(cap), C.c_int(form))
    return out[:, :6].astype(np.float64), out[:, 6].astype(np.float64)


libs = {bits: C.CDLL(os.path.join(WORK, "libstudy%d.so" % bits)) for bits in (13, 12, 11)}
tp = os.path.join(WORK, "truth.npy")
if os.path.exists(tp):
    truth = np.load(tp); print("truth: stamped LDS durations (truth.npy)")
else:
    full, _ = stats(libs[13], 0, bs, 0, 0)
    truth = full @ np.array([1.28e-3, 0.84e-3, 0.094e-3, 0.036e-3, 0.0, 0.70e-3]) + 0.23
    print("truth: the whole block's counts by section 2's weights (no stamps here)")
for ci, nm in enumerate(names):
    print("  %-8s truth ms mean %.3f min %.3f max %.3f" % (nm, truth[ci * 32:(ci + 1) * 32].mean(), truth[ci * 32:(ci + 1) * 32].min(), truth[ci * 32:(ci + 1) * 32].max()))
t_all = truth[u]
tcut = np.sort(t_all)[::-1][2303]
for bits in (13, 12, 11):
    for (l, cap) in ((2048, 10), (2048, 12), (1024, 12), (2048, 14), (1024, 14), (1024, 16), (1536, 12), (768, 12)):
        s, cov = stats(libs[bits], 0, l, cap, 0 if bits == 13 else 1)
        sc = s * (bs / np.maximum(cov, 1))[:, None]
        A = np.c_[sc, np.ones(384)]
        w, _ = nnls(A, truth)
        est = A @ w
        e = est[u] + 1e-9 * np.random.default_rng(0).random(n)
        inl = e >= np.sort(e)[::-1][2303]
        mis = int(((t_all >= tcut) & ~inl).sum())
        share = {nm: float(inl[np.arange(ci, n, 12)].mean()) for ci, nm in enumerate(names) if nm in ("nci", "xml", "samba", "mozilla", "mr", "ooffice", "osdb", "sao")}
        fit = ",".join(str(int(round(x * 1e6))) for x in w)
        print("bits %2d sample %4d limit %2d: rho %.3f misplaced %4d heaviest without LDS %.3f ms | K4LZ4_PCOST_FIT=%d,%d,%s | LDS share %s" % (
            bits, l, cap, spearmanr(est, truth).correlation, mis, t_all[~inl].max(), l, cap, fit, " ".join("%s %.2f" % kv for kv in share.items())))
