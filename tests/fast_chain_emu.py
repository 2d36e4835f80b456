"""The chained fast encoder's kernel (k4lz4_fast_chain.hpp) under the host wave emulator: tests/emu/emu_fast_chain.cpp +
tests/emu/emu_runtime.cpp, built by g++ into a library of its own.  The block table is encoders.fast_chain_blocks' (the
library builds the same on the host).  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

from k4os.compression.lz4_amd.encoders import FAST_CHAIN_STATE, fast_chain_blocks, _round_block_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
SO = os.path.join(EMU_DIR, "libk4lz4_emu_fast_chain.so")


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_fast_chain.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
        glob.glob(os.path.join(CSRC, "*.hpp"))

    def stale():
        return not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs)
    if stale():
        import fcntl
        with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if stale():
                tmp = f"{SO}.{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                                       "-Wno-attributes", "-pthread", "-I", EMU_DIR, "-I", CSRC, "-shared", "-o", tmp,
                                       os.path.join(EMU_DIR, "emu_fast_chain.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.k4emu_fast_chain.argtypes = [C.c_void_p] * 17 + [C.c_longlong, C.c_int, C.c_int, C.c_int]
    return _lib


def encode(contents, block_size: int, extra_blocks: int = 0, allow_copy: bool = True, state_in=None, workgroups: int = 2, threads: int = 4):
    """-> ([(outLen, payload)] per stream, states after the streams)"""
    ns = len(contents)
    contents = [np.ascontiguousarray(c, np.uint8) for c in contents]
    B = _round_block_size(block_size)
    slot = B + B // 255 + 16
    st_in = None if state_in is None else np.ascontiguousarray(state_in, FAST_CHAIN_STATE)
    soff = np.zeros(ns, np.uint64)
    slen = np.array([c.size for c in contents], np.uint64)
    if ns > 1:
        soff[1:] = np.cumsum(((slen + 15) // 16 * 16)[:-1])
    src = np.zeros(int(((slen + 15) // 16 * 16).sum()) + 64, np.uint8)
    for s, c in enumerate(contents):
        src[int(soff[s]):int(soff[s]) + c.size] = c
    tables = []
    for s, c in enumerate(contents):
        d0 = 0 if st_in is None else int(st_in["dictSize"][s])
        cur0 = 0 if st_in is None else int(st_in["currentOffset"][s])
        tables.append((fast_chain_blocks(c.size, B, extra_blocks, d0, cur0), cur0 - d0))
    nblk = np.array([len(t) for t, _ in tables], np.uint32)
    first = np.concatenate(([0], np.cumsum(nblk.astype(np.int64))))[:-1].astype(np.int64)
    idx0 = np.array([i for _, i in tables], np.uint32)
    nb = int(nblk.sum())
    rows = [r for t, _ in tables for r in t]
    bpos = np.array([r[0] for r in rows], np.uint32)
    blen = np.array([r[1] for r in rows], np.int32)
    bdict = np.array([r[2] for r in rows], np.uint32)
    dict_end = []
    L = 65536 + (1 + max(int(extra_blocks), 0)) * B + 32
    for s_, c in enumerate(contents):                    # the dictSize the ring leaves behind the stream's last block (and its save)
        d = ptr = pos = 0 if st_in is None else int(st_in["dictSize"][s_])
        while pos < c.size:
            n = min(B, c.size - pos)
            pos += n; ptr += n; d += n
            if ptr + B > L:
                d = ptr = min(65536, d)
        dict_end.append(d)
    dict_end = np.array(dict_end, np.uint32)
    doff = np.array([s * 0 for s in range(nb)], np.uint64)
    k = 0
    for s in range(ns):
        for j in range(int(nblk[s])):
            doff[k] = (int(first[s]) + j) * slot
            k += 1
    cap = np.full(max(nb, 1), slot, np.int32)
    dst = np.zeros(max(nb, 1) * slot + 64, np.uint8)
    out = np.full(max(nb, 1), -12345, np.int32)
    order = np.argsort(-(slen.astype(np.int64)), kind="stable").astype(np.uint32)
    st_out = np.zeros(ns, FAST_CHAIN_STATE)
    p = lambda a: None if a is None else a.ctypes.data
    lib().k4emu_fast_chain(p(src), p(soff), p(slen), p(first), p(nblk), p(idx0), p(dict_end), p(order), p(bpos), p(blen), p(bdict), p(doff),
                           p(cap), p(dst), p(out), p(st_in), p(st_out), ns, int(allow_copy), workgroups, threads)
    res = []
    for s in range(ns):
        blocks = []
        for j in range(int(nblk[s])):
            b = int(first[s]) + j
            n = int(out[b])
            blocks.append((n, dst[int(doff[b]):int(doff[b]) + abs(n)].tobytes()))
        res.append(blocks)
    return res, st_out
