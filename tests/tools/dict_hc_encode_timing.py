#!/usr/bin/env python
"""k4lz4_encode_dict_hc_batch_device against k4lz4_encode_batch_device (the same HC level, no dictionary) on the same device-resident
messages, and liblz4 (LZ4_loadDictHC once, the stream state copied for every message, LZ4_compress_HC_continue; and LZ4_compress_HC
without a dictionary) on 16 host threads: the median of 5 calls after a warm-up, for 262 144 x 1 KiB and 65 536 x 4 KiB messages with
one shared 64 KiB dictionary, at levels 3 and 9.  Writes profiles/dict_hc_encode_timing.txt.  The load step is timed by a call with
no messages (upload of the list, table kernel); what the rest of a call takes beyond that is the order kernels and the encode kernel.

    python tests/tools/dict_hc_encode_timing.py [--shapes 262144x1024 65536x4096] [--levels 3 9] [--reps 5] [--out profiles/dict_hc_encode_timing.txt]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import dict_encode_cases as DC  # noqa: E402
from k4os.compression.lz4_amd import _native  # noqa: E402

HOST_C = r"""
#include <pthread.h>
#include <stdint.h>
#include <string.h>
#include <time.h>
#define STATE 262200                                   /* LZ4_STREAMHCSIZE of liblz4 1.9.3 */
void *LZ4_createStreamHC(void);
int LZ4_freeStreamHC(void *s);
void LZ4_resetStreamHC_fast(void *s, int level);
int LZ4_loadDictHC(void *s, const char *d, int n);
int LZ4_compress_HC_continue(void *s, const char *src, char *dst, int n, int cap);
int LZ4_compress_HC(const char *src, char *dst, int n, int cap, int level);
typedef struct { const char *src; char *dst; const void *loaded; long long first, count; int len, cap, use_dict, level; long long bytes; } job_t;
static void *work(void *p)
{
    job_t *j = (job_t *)p;
    void *st = LZ4_createStreamHC();
    for (long long i = j->first; i < j->first + j->count; i++) {
        int r;
        if (j->use_dict) { memcpy(st, j->loaded, STATE); r = LZ4_compress_HC_continue(st, j->src + i * j->len, j->dst + i * j->cap, j->len, j->cap); }
        else r = LZ4_compress_HC(j->src + i * j->len, j->dst + i * j->cap, j->len, j->cap, j->level);
        j->bytes += r;
    }
    LZ4_freeStreamHC(st);
    return 0;
}
double run(const char *src, char *dst, long long n, int len, int cap, const char *dict, int dict_len, int threads, int use_dict, int level, long long *bytes)
{
    void *loaded = LZ4_createStreamHC();
    pthread_t t[64];
    job_t j[64];
    struct timespec a, b;
    if (threads > 64) threads = 64;
    clock_gettime(CLOCK_MONOTONIC, &a);
    LZ4_resetStreamHC_fast(loaded, level);
    LZ4_loadDictHC(loaded, dict, dict_len);
    for (int k = 0; k < threads; k++) {
        j[k] = (job_t){src, dst, loaded, n * k / threads, n * (k + 1) / threads - n * k / threads, len, cap, use_dict, level, 0};
        pthread_create(&t[k], 0, work, &j[k]);
    }
    *bytes = 0;
    for (int k = 0; k < threads; k++) { pthread_join(t[k], 0); *bytes += j[k].bytes; }
    clock_gettime(CLOCK_MONOTONIC, &b);
    LZ4_freeStreamHC(loaded);
    return (b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) * 1e-6;
}
"""


def host_lib():
    """the host figure's few lines of C against the system liblz4, or None where there is no compiler or no liblz4"""
    d = tempfile.mkdtemp(prefix="k4lz4_dict_hc_timing_")
    src, so = os.path.join(d, "host.c"), os.path.join(d, "host.so")
    with open(src, "w") as f:
        f.write(HOST_C)
    try:
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-pthread", src, "-o", so, "-l:liblz4.so.1"], stderr=subprocess.DEVNULL)
        lib = C.CDLL(so)
    except (OSError, subprocess.CalledProcessError):
        return None
    lib.run.restype = C.c_double
    lib.run.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    return lib


def messages(n, size, cls="dickens"):
    """n messages of `size` bytes and a 64 KiB dictionary cut from the same class: the messages' text is not the dictionary's"""
    base = DC.synthetic(cls, (8 << 20) + size + DC.K64, 3)
    dictionary = base[:DC.K64].copy()
    pool = base[DC.K64:]
    starts = np.random.default_rng(5).integers(0, pool.size - size, n)
    idx = starts[:, None] + np.arange(size)[None, :]
    return np.ascontiguousarray(pool[idx].reshape(-1)), dictionary


def run(n, size, level, reps, threads, host):
    src, dictionary = messages(n, size)
    cap = DC.bound(size)
    ctx = _native.default_context()
    lib = ctx.lib
    dev = torch.device("cuda", ctx.device)
    d_src = torch.from_numpy(src).to(dev)
    d_dst = torch.empty(n * cap + 64, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    d_off = torch.from_numpy((np.arange(n, dtype=np.int64) * size)).to(dev)
    d_len = torch.full((n,), size, dtype=torch.int32, device=dev)
    d_doff = torch.from_numpy((np.arange(n, dtype=np.int64) * cap)).to(dev)
    d_cap = torch.full((n,), cap, dtype=torch.int32, device=dev)
    d_idx = torch.zeros(n, dtype=torch.int32, device=dev)
    d_dict = torch.from_numpy(dictionary).to(dev)
    doff, dlen = np.zeros(1, np.uint64), np.array([dictionary.size], np.int32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    batch = (d_src.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_dst.data_ptr(), d_doff.data_ptr(), d_cap.data_ptr(), d_out.data_ptr())

    def with_dict(count=n):
        ctx.check(lib.k4lz4_encode_dict_hc_batch_device(ctx.handle, *batch, count, level, 0, d_idx.data_ptr(), d_dict.data_ptr(), doff.ctypes.data,
                                                        dlen.ctypes.data, 1, stream))

    def plain():
        ctx.check(lib.k4lz4_encode_batch_device(ctx.handle, *batch, n, level, 0, stream))

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

    plain_ms = timed(plain)
    plain_c = int(d_out.clamp(min=0).sum().item())
    dict_ms = timed(with_dict)
    dict_c = int(d_out.clamp(min=0).sum().item())
    assert int((d_out <= 0).sum().item()) == 0
    load_ms = timed(lambda: with_dict(0))
    total = n * size
    gib = lambda ms: total / (ms * 1e-3) / (1 << 30)
    lines = [f"level {level}: {n} x {size} B messages, one shared 64 KiB dictionary (synthetic dickens), device-resident, median of {reps} after a warm-up",
             f"  k4lz4_encode_dict_hc_batch_device    {dict_ms:9.3f} ms  {gib(dict_ms):7.2f} GiB/s   sum(C)/sum(U) {dict_c / total:.3f}",
             f"    load step alone (a call of 0 messages: list upload + k4_dict_hc_load_kernel)  {load_ms:.3f} ms",
             f"    the rest (k4_dict_cost_kernel, k4_order_kernel, k4_dict_hc_encode_kernel)    {dict_ms - load_ms:.3f} ms",
             f"  k4lz4_encode_batch_device, level {level}   {plain_ms:9.3f} ms  {gib(plain_ms):7.2f} GiB/s   sum(C)/sum(U) {plain_c / total:.3f}"]
    if host is not None:
        dst = np.empty(n * cap, np.uint8)
        got = C.c_longlong()
        for use_dict, what in ((1, "LZ4_loadDictHC + LZ4_compress_HC_continue"), (0, "LZ4_compress_HC")):
            ts = []
            for _ in range(reps + 1):
                ts.append(host.run(src.ctypes.data, dst.ctypes.data, n, size, cap, dictionary.ctypes.data, dictionary.size, threads, use_dict, level, C.byref(got)))
            ms = float(np.median(ts[1:]))
            lines.append(f"  liblz4, {threads} host threads, {what:42s} {ms:9.3f} ms  {gib(ms):7.2f} GiB/s   sum(C)/sum(U) {got.value / total:.3f}")
            if use_dict:
                assert got.value == dict_c, "the GPU's blocks and liblz4's differ in total size"
    else:
        lines.append("  liblz4 on host threads: not measured (no compiler or no liblz4.so.1 here)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["262144x1024", "65536x4096"])
    ap.add_argument("--levels", nargs="*", type=int, default=[3, 9])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_hc_encode_timing.txt"))
    a = ap.parse_args()
    host = host_lib()
    lines = []
    for s in a.shapes:
        n, size = (int(x) for x in s.split("x"))
        for level in a.levels:
            lines += run(n, size, level, a.reps, a.threads, host) + [""]
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
