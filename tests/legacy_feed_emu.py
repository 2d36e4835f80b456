"""The fed LZ4Stream reader's kernels (k4lz4_legacy_feed.hpp) under the host wave emulator: tests/emu/emu_legacy_feed.cpp +
tests/emu/emu_runtime.cpp, built by g++ into a library of its own.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
SO = os.path.join(EMU_DIR, "libk4lz4_emu_legacy_feed.so")
LSQ_WORDS = 8


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_legacy_feed.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
        glob.glob(os.path.join(CSRC, "*.hpp")) + [os.path.join(ROOT, "include", "k4lz4.h")]

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
                                       os.path.join(EMU_DIR, "emu_legacy_feed.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.k4emu_lf_store_bytes.restype = C.c_longlong
        _lib.k4emu_lf_store_bytes.argtypes = [C.c_longlong, C.c_int]
        _lib.k4emu_lf_state_bytes.restype = C.c_longlong
        _lib.k4emu_lf_call.restype = None
        _lib.k4emu_lf_call.argtypes = [C.c_longlong] + [C.c_void_p] * 12 + [C.c_longlong, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p,
                                                                           C.c_void_p, C.c_int]
        _lib.k4emu_lf_whole_call.restype = None
        _lib.k4emu_lf_whole_call.argtypes = [C.c_longlong] + [C.c_void_p] * 9 + [C.c_longlong, C.c_int, C.c_int, C.c_int]
        _lib.k4emu_lf_query.restype = None
        _lib.k4emu_lf_query.argtypes = [C.c_void_p] * 3 + [C.c_longlong, C.c_int]
    return _lib


class EmuFedReaders:
    """n fed LZ4Stream readers over host arrays: call() is one k4lz4_legacy_read_fed_batch_device, with guard bytes around every
    store, every output slot and every piece (legacy_feed_cases.driver drives it).  direct: READs that are not interactive go the
    device form's way with maxCount = max_count, or the largest count; topup=False leaves the direct path's top-up step out."""
    GUARD = 64

    def __init__(self, n, max_block=1 << 16, threads=4, direct=False, topup=True, max_count=None):
        self.n, self.max_block, self.threads = n, max_block, threads
        self.direct, self.topup, self.max_count = direct, topup, max_count
        self.plans, self.heads = [], []     # per direct call: each stream's plan state (0 not planned, 1 handed back, 2 served), top-up bytes
        self.sb = int(lib().k4emu_lf_store_bytes(max_block, 1))
        step = self.sb + 256
        self.store = np.full(self.n * step + 256, 0xA5, np.uint8)
        self.store_off = (256 + np.arange(self.n, dtype=np.uint64) * step).astype(np.uint64)
        assert self.store.ctypes.data % 8 == 0
        self.call(1, [b""] * n, np.zeros(n, np.int64), np.zeros(n, np.int64), False)

    def call(self, op, pieces, final, counts, interactive):
        """-> (outLen, [bytes delivered], consumed, need)"""
        n = self.n
        counts = np.ascontiguousarray(counts, np.int64)
        final = np.ascontiguousarray(final, np.int64)
        lens = np.array([len(p) for p in pieces], np.uint64)
        src_off = np.full(n, self.GUARD, np.uint64)
        if n > 1:
            src_off[1:] += np.cumsum(lens[:-1] + np.uint64(self.GUARD))
        src = np.full(int(lens.sum()) + self.GUARD * (n + 1), 0xEE, np.uint8)
        for i, p in enumerate(pieces):
            src[int(src_off[i]):int(src_off[i]) + len(p)] = np.frombuffer(bytes(p), np.uint8)
        caps = np.maximum(counts, 0).astype(np.uint64) if op == 0 else np.zeros(n, np.uint64)
        doff = np.full(n, self.GUARD, np.uint64)
        if n > 1:
            doff[1:] += np.cumsum(caps[:-1] + np.uint64(self.GUARD))
        dst = np.full(int(caps.sum()) + self.GUARD * (n + 1), 0xCD, np.uint8)
        out, consumed, need = (np.full(n, -999, np.int64) for _ in range(3))
        plan, head = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        max_count = (self.max_count or int(counts.max())) if self.direct and op == 0 and not interactive else 0
        p = lambda a: a.ctypes.data  # noqa: E731
        lib().k4emu_lf_call(self.max_block, p(self.store), p(self.store_off), p(src), p(src_off), p(lens), p(final), p(dst), p(doff), p(counts),
                            p(out), p(consumed), p(need), n, op, int(interactive), max_count, int(self.topup), p(plan), p(head), self.threads)
        if max_count > 0:
            self.plans.append(plan)
            self.heads.append(head)
        mask = np.ones(dst.size, bool)
        for i in range(n):
            mask[int(doff[i]):int(doff[i] + caps[i])] = False
        assert (dst[mask] == 0xCD).all(), "a write outside a stream's slot"
        smask = np.ones(self.store.size, bool)
        for i in range(n):
            smask[int(self.store_off[i]):int(self.store_off[i]) + self.sb] = False
        assert (self.store[smask] == 0xA5).all(), "a write outside a stream's store"
        return out, [dst[int(doff[i]):int(doff[i]) + max(int(out[i]), 0)].tobytes() if op == 0 else b"" for i in range(n)], consumed, need

    def query(self):
        q = np.zeros(self.n * LSQ_WORDS, np.int64)
        lib().k4emu_lf_query(self.store.ctypes.data, self.store_off.ctypes.data, q.ctypes.data, self.n, 1)
        return q.reshape(self.n, LSQ_WORDS)
