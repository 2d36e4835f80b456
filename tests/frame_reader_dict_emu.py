"""The incremental frame readers against a dictionary set (k4lz4_frame_reader_dict.hpp) under the host wave emulator:
tests/emu/emu_frame_reader_dict.cpp + tests/emu/emu_runtime.cpp, built by g++ into a library of its own.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
SO = os.path.join(EMU_DIR, "libk4lz4_emu_frame_reader_dict.so")
FRQ_WORDS = 8
GUARD = 64


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_frame_reader_dict.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
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
                                       os.path.join(EMU_DIR, "emu_frame_reader_dict.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.k4emu_frd_store_bytes.restype = C.c_longlong
        _lib.k4emu_frd_store_bytes.argtypes = [C.c_longlong, C.c_int]
        _lib.k4emu_frd_call.restype = None
        _lib.k4emu_frd_call.argtypes = [C.c_int, C.c_longlong] + [C.c_void_p] * 12 + [C.c_longlong, C.c_int, C.c_int, C.c_longlong] + \
            [C.c_void_p] * 5 + [C.c_int, C.c_int]
        _lib.k4emu_frd_query.restype = None
        _lib.k4emu_frd_query.argtypes = [C.c_void_p] * 3 + [C.c_longlong, C.c_int]
        _lib.k4emu_frd_entries.restype = None
        _lib.k4emu_frd_entries.argtypes = [C.c_void_p] * 3 + [C.c_longlong]
    return _lib


def _p(a):
    return a.ctypes.data


class EmuSet:
    """what a k4lz4_dict_set holds for the decoders -- every entry's last 64 KiB -- between guard bytes, and the call's id table;
    entries None: no set (the plain calls' kernels)"""

    def __init__(self, entries, ids):
        self.none = entries is None
        kept = [] if self.none else [np.frombuffer(bytes(e)[-65536:], np.uint8) for e in entries]
        self.nd = -1 if self.none else len(kept)
        self.off = np.zeros(max(len(kept), 1), np.uint64)
        self.len = np.zeros(max(len(kept), 1), np.int32)
        at = GUARD
        for e, k in enumerate(kept):
            self.off[e], self.len[e] = at, k.size
            at += k.size + GUARD
        self.buf = np.full(at + GUARD, 0x5A, np.uint8)
        for e, k in enumerate(kept):
            self.buf[int(self.off[e]):int(self.off[e]) + k.size] = k
        self.image = self.buf.copy()
        self.ids = np.array(list(ids) if not self.none and len(kept) else [0], np.uint32)

    def args(self):
        return [_p(self.buf), _p(self.off), _p(self.len), _p(self.ids), self.nd]

    def check(self):
        assert (self.buf == self.image).all(), "a write into the set or its guards"


class _Stores:
    def __init__(self, n, max_block, fed, threads, fast):
        self.n, self.max_block, self.fed, self.threads, self.fast = n, max_block, int(fed), threads, fast
        self.plans = []                     # per fast call: each stream's plan state (0 not planned, 1 handed back, 2 served)
        self.sb = int(lib().k4emu_frd_store_bytes(max_block, self.fed))
        step = self.sb + 256
        self.store = np.full(n * step + 256, 0xA5, np.uint8)
        self.store_off = (256 + np.arange(n, dtype=np.uint64) * step).astype(np.uint64)
        assert self.store.ctypes.data % 8 == 0

    def _run(self, dset, op, src, src_off, src_len, final, counts, interactive):
        n = self.n
        caps = np.maximum(counts, 0).astype(np.uint64) if op == 0 else np.zeros(n, np.uint64)
        doff = np.full(n, GUARD, np.uint64)
        if n > 1:
            doff[1:] += np.cumsum(caps[:-1] + np.uint64(GUARD))
        dst = np.full(int(caps.sum()) + GUARD * (n + 1), 0xCD, np.uint8)
        out, consumed, need = (np.full(n, -999, np.int64) for _ in range(3))
        plan = np.zeros(n, np.uint32)
        max_count = int(counts.max()) if self.fast and op == 0 and not interactive else 0
        src_image = src.copy()
        lib().k4emu_frd_call(self.fed, self.max_block, _p(self.store), _p(self.store_off), _p(src), _p(src_off), _p(src_len), _p(final), _p(dst),
                             _p(doff), _p(counts), _p(out), _p(consumed), _p(need), n, op, int(interactive), max_count, _p(plan), *dset.args(),
                             self.threads)
        if max_count > 0:
            self.plans.append(plan)
        mask = np.ones(dst.size, bool)
        for i in range(n):
            mask[int(doff[i]):int(doff[i] + caps[i])] = False
        assert (dst[mask] == 0xCD).all(), "a write outside a stream's slot"
        smask = np.ones(self.store.size, bool)
        for i in range(n):
            smask[int(self.store_off[i]):int(self.store_off[i]) + self.sb] = False
        assert (self.store[smask] == 0xA5).all(), "a write outside a stream's store"
        assert (src == src_image).all(), "a write into the sources or their guards"
        dset.check()
        data = [dst[int(doff[i]):int(doff[i]) + max(int(out[i]), 0)].tobytes() if op == 0 else b"" for i in range(n)]
        return out, data, consumed, need

    def query(self):
        q = np.zeros(self.n * FRQ_WORDS, np.int64)
        lib().k4emu_frd_query(_p(self.store), _p(self.store_off), _p(q), self.n, 1)
        return q.reshape(self.n, FRQ_WORDS)

    def entries(self):
        """FrState::dictEntry per stream: the open frame's entry, -1 for none"""
        e = np.zeros(self.n, np.uint32)
        lib().k4emu_frd_entries(_p(self.store), _p(self.store_off), _p(e), self.n)
        return e.astype(np.int64) - 1


class EmuDictReaders(_Stores):
    """n readers over whole sources (k4lz4_frame_read_dictset_batch_device), guard bytes around every store, slot, source and the set;
    `dset` may be replaced between calls"""

    def __init__(self, sources, entries, ids, max_block=65536, threads=4, fast=False):
        super().__init__(len(sources), max_block, False, threads, fast)
        self.dset = EmuSet(entries, ids)
        lens = np.array([len(s) for s in sources], np.uint64)
        self.src_off = np.full(self.n, GUARD, np.uint64)
        if self.n > 1:
            self.src_off[1:] += np.cumsum(lens[:-1] + np.uint64(GUARD))
        self.src_len = lens
        self.src = np.full(int(lens.sum()) + GUARD * (self.n + 1), 0xEE, np.uint8)
        for i, s in enumerate(sources):
            self.src[int(self.src_off[i]):int(self.src_off[i]) + len(s)] = np.frombuffer(bytes(s), np.uint8)
        self._call(2, np.zeros(self.n, np.int64), False)

    def _call(self, op, counts, interactive):
        counts = np.ascontiguousarray(counts, np.int64)
        out, data, _, _ = self._run(self.dset, op, self.src, self.src_off, self.src_len, np.zeros(self.n, np.int64), counts, interactive)
        return out, data

    def read(self, counts, interactive=False):
        """-> list of bytes | code | None (the stream sat the call out)"""
        out, data = self._call(0, counts, interactive)
        return [None if counts[i] < 0 else (int(out[i]) if out[i] < 0 else data[i]) for i in range(self.n)]

    def open(self, which=None):
        counts = np.array([0 if which is None or i in which else -1 for i in range(self.n)], np.int64)
        out, _ = self._call(1, counts, False)
        return [None if counts[i] < 0 else int(out[i]) for i in range(self.n)]


class EmuDictFedReaders(_Stores):
    """n fed readers (k4lz4_frame_read_fed_dictset_batch_device): call() is one raw call, guard bytes around every store, slot,
    piece and the set (frame_feed_cases.FedDriver drives it)"""

    def __init__(self, n, entries, ids, max_block=65536, threads=4, fast=False):
        super().__init__(n, max_block, True, threads, fast)
        self.dset = EmuSet(entries, ids)
        self.call(2, [b""] * n, np.zeros(n, np.int64), np.zeros(n, np.int64), False)

    def call(self, op, pieces, final, counts, interactive):
        """-> (outLen, [bytes delivered], consumed, need)"""
        n = self.n
        counts = np.ascontiguousarray(counts, np.int64)
        final = np.ascontiguousarray(final, np.int64)
        lens = np.array([len(p) for p in pieces], np.uint64)
        src_off = np.full(n, GUARD, np.uint64)
        if n > 1:
            src_off[1:] += np.cumsum(lens[:-1] + np.uint64(GUARD))
        src = np.full(int(lens.sum()) + GUARD * (n + 1), 0xEE, np.uint8)
        for i, p in enumerate(pieces):
            src[int(src_off[i]):int(src_off[i]) + len(p)] = np.frombuffer(bytes(p), np.uint8)
        return self._run(self.dset, op, src, src_off, lens, final, counts, interactive)
