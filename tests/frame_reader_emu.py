"""The incremental frame reader's kernels (k4lz4_frame_reader.hpp) under the host wave emulator: tests/emu/emu_frame_reader.cpp +
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
SO = os.path.join(EMU_DIR, "libk4lz4_emu_frame_reader.so")
FRQ_WORDS = 8


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_frame_reader.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
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
                                       os.path.join(EMU_DIR, "emu_frame_reader.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.k4emu_fr_store_bytes.restype = C.c_longlong
        _lib.k4emu_fr_store_bytes.argtypes = [C.c_longlong]
        _lib.k4emu_fr_call.restype = None
        _lib.k4emu_fr_call.argtypes = [C.c_longlong] + [C.c_void_p] * 9 + [C.c_longlong, C.c_int, C.c_int, C.c_int]
        _lib.k4emu_fr_table_rows.restype = C.c_longlong
        _lib.k4emu_fr_table_rows.argtypes = [C.c_longlong]
        _lib.k4emu_fr_call_fast.restype = None
        _lib.k4emu_fr_call_fast.argtypes = [C.c_longlong] + [C.c_void_p] * 9 + [C.c_longlong, C.c_longlong, C.c_void_p, C.c_int]
        _lib.k4emu_fr_query.restype = None
        _lib.k4emu_fr_query.argtypes = [C.c_void_p] * 3 + [C.c_longlong, C.c_int]
        _lib.k4emu_fr_xxh.restype = C.c_uint32
        _lib.k4emu_fr_xxh.argtypes = [C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_int]
    return _lib


class EmuReaders:
    """n readers over host arrays, with guard bytes around every store and every output slot"""
    GUARD = 64

    def __init__(self, sources, max_block=4 << 20, threads=4, fast=False):
        self.n = len(sources)
        self.fast = fast                    # READs that are not interactive go the device form's way with maxCount = the largest count
        self.plans = []                     # per fast call: each stream's plan state (0 not planned, 1 handed back, 2 served)
        self.max_block, self.threads = max_block, threads
        self.sb = int(lib().k4emu_fr_store_bytes(max_block))
        step = self.sb + 256
        self.store = np.full(self.n * step + 256, 0xA5, np.uint8)
        self.store_off = (256 + np.arange(self.n, dtype=np.uint64) * step).astype(np.uint64)
        assert self.store.ctypes.data % 8 == 0
        lens = np.array([len(s) for s in sources], np.uint64)
        self.src_off = np.zeros(self.n, np.uint64)
        if self.n > 1:
            self.src_off[1:] = np.cumsum(lens[:-1] + np.uint64(self.GUARD))
        self.src_len = lens
        self.src = np.full(int(lens.sum()) + self.GUARD * (self.n + 1), 0xEE, np.uint8)
        for i, s in enumerate(sources):
            self.src[int(self.src_off[i]):int(self.src_off[i]) + len(s)] = np.frombuffer(bytes(s), np.uint8)
        self._call(2, np.zeros(self.n, np.int64), False)

    def _call(self, op, counts, interactive):
        counts = np.ascontiguousarray(counts, np.int64)
        caps = np.maximum(counts, 0).astype(np.uint64)
        doff = np.full(self.n, self.GUARD, np.uint64)
        if self.n > 1:
            doff[1:] += np.cumsum(caps[:-1] + np.uint64(self.GUARD))
        dst = np.full(int(caps.sum()) + self.GUARD * (self.n + 1), 0xCD, np.uint8)
        out = np.full(self.n, -999, np.int64)
        p = lambda a: a.ctypes.data  # noqa: E731
        if self.fast and op == 0 and not interactive and counts.max() > 0:
            plan = np.zeros(self.n, np.uint32)
            lib().k4emu_fr_call_fast(self.max_block, p(self.store), p(self.store_off), p(self.src), p(self.src_off), p(self.src_len), p(dst),
                                     p(doff), p(counts), p(out), self.n, int(counts.max()), p(plan), self.threads)
            self.plans.append(plan)
        else:
            lib().k4emu_fr_call(self.max_block, p(self.store), p(self.store_off), p(self.src), p(self.src_off), p(self.src_len), p(dst), p(doff),
                                p(counts), p(out), self.n, op, int(interactive), self.threads)
        # guards: between the slots, and between the stores
        mask = np.ones(dst.size, bool)
        for i in range(self.n):
            mask[int(doff[i]):int(doff[i] + caps[i])] = False
        assert (dst[mask] == 0xCD).all(), "a write outside a stream's slot"
        smask = np.ones(self.store.size, bool)
        for i in range(self.n):
            smask[int(self.store_off[i]):int(self.store_off[i]) + self.sb] = False
        assert (self.store[smask] == 0xA5).all(), "a write outside a stream's store"
        return out, [dst[int(doff[i]):int(doff[i]) + max(int(out[i]), 0)].tobytes() for i in range(self.n)]

    def read(self, counts, interactive=False):
        """-> list of bytes | code | None (the stream sat the call out)"""
        out, data = self._call(0, counts, interactive)
        return [None if counts[i] < 0 else (int(out[i]) if out[i] < 0 else data[i]) for i in range(self.n)]

    def open(self, which=None):
        counts = np.array([0 if which is None or i in which else -1 for i in range(self.n)], np.int64)
        out, _ = self._call(1, counts, False)
        return [None if counts[i] < 0 else int(out[i]) for i in range(self.n)]

    def query(self):
        q = np.zeros(self.n * FRQ_WORDS, np.int64)
        lib().k4emu_fr_query(self.store.ctypes.data, self.store_off.ctypes.data, q.ctypes.data, self.n, 1)
        return q.reshape(self.n, FRQ_WORDS)
