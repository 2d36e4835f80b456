"""LZ4Stream piece by piece (k4lz4_legacy_stream.hpp) under the host wave emulator: tests/emu/emu_legacy_stream.cpp +
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
SO = os.path.join(EMU_DIR, "libk4lz4_emu_legacy_stream.so")
LSQ_WORDS = 8
GUARD = 64


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_legacy_stream.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
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
                                       os.path.join(EMU_DIR, "emu_legacy_stream.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.k4emu_ls_writer_store_bytes.restype = C.c_longlong
        _lib.k4emu_ls_write_bound.restype = C.c_longlong
        _lib.k4emu_ls_write_bound.argtypes = [C.c_void_p, C.c_longlong, C.c_int]
        _lib.k4emu_ls_write.restype = None
        _lib.k4emu_ls_write.argtypes = [C.c_void_p] * 10 + [C.c_longlong, C.c_int, C.c_int]
        _lib.k4emu_ls_reader_store_bytes.restype = C.c_longlong
        _lib.k4emu_ls_reader_store_bytes.argtypes = [C.c_longlong]
        _lib.k4emu_ls_read.restype = None
        _lib.k4emu_ls_read.argtypes = [C.c_longlong] + [C.c_void_p] * 9 + [C.c_longlong, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int]
        _lib.k4emu_ls_query.restype = None
        _lib.k4emu_ls_query.argtypes = [C.c_void_p] * 3 + [C.c_longlong, C.c_int]
    return _lib


class WriterRecord(C.Structure):
    _fields_ = [("blockSize", C.c_int32), ("high", C.c_int32), ("pending", C.c_int32), ("closed", C.c_int32)]


def _guarded(pieces, fill):
    lens = np.array([len(p) for p in pieces], np.uint64)
    off = np.full(len(pieces), GUARD, np.uint64)
    if len(pieces) > 1:
        off[1:] += np.cumsum(lens[:-1] + np.uint64(GUARD))
    buf = np.full(int(lens.sum()) + GUARD * (len(pieces) + 1) + 16, fill, np.uint8)
    for p, o in zip(pieces, off):
        buf[int(o):int(o) + len(p)] = np.frombuffer(bytes(p), np.uint8)
    return buf, off, lens


def _intact(buf, off, caps, fill, what):
    mask = np.ones(buf.size, bool)
    for o, c in zip(off, caps):
        mask[int(o):int(o) + int(c)] = False
    assert (buf[mask] == fill).all(), f"a write outside {what}"


class EmuWriters:
    """n fast LZ4Streams in Compress mode over host arrays: call() is one k4lz4_legacy_write_batch_device, with guard bytes around
    every store, every output slot and every piece"""

    def __init__(self, block_sizes, threads=4):
        self.n, self.threads = len(block_sizes), threads
        self.recs = (WriterRecord * self.n)()
        sizes = []
        for i, b in enumerate(block_sizes):
            lib().k4emu_ls_writer_init(C.byref(self.recs[i]), int(b), 0)
            sizes.append(int(lib().k4emu_ls_writer_store_bytes(C.byref(self.recs[i]))))
        self.sizes = np.array(sizes, np.int64)
        self.store_off = (256 + np.concatenate(([0], np.cumsum(self.sizes[:-1] + 256)))).astype(np.uint64)
        self.store = np.full(int(self.sizes.sum()) + 256 * (self.n + 1), 0xA5, np.uint8)

    def call(self, op, pieces, short=()):
        """pieces[i]: bytes or None (untouched); short: streams whose target is one byte below the bound -> (outLen, [bytes or None])"""
        n = self.n
        lens = np.array([-1 if p is None else len(p) for p in pieces], np.int64)
        src, soff, _ = _guarded([p or b"" for p in pieces], 0xEE)
        caps = np.array([lib().k4emu_ls_write_bound(C.byref(self.recs[i]), int(lens[i]), op) for i in range(n)], np.uint64)
        asked = caps.copy()
        for i in short:
            asked[i] = max(int(asked[i]) - 1, 0)
        dst, doff, _ = _guarded([bytes(int(c)) for c in caps], 0xCD)
        dst[:] = 0xCD
        out = np.full(n, -999, np.int64)
        before = [(r.blockSize, r.high, r.pending, r.closed) for r in self.recs]
        p = lambda a: a.ctypes.data  # noqa: E731
        lib().k4emu_ls_write(self.recs, p(self.store), p(self.store_off), p(src), p(soff), p(lens), p(dst), p(doff), p(asked), p(out), n, op,
                             self.threads)
        _intact(dst, doff, np.maximum(out, 0), 0xCD, "a stream's output")
        _intact(self.store, self.store_off, self.sizes, 0xA5, "a stream's store")
        for i in range(n):
            if out[i] < 0 or lens[i] < 0:
                assert (self.recs[i].blockSize, self.recs[i].high, self.recs[i].pending, self.recs[i].closed) == before[i]
        return out, [dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() if lens[i] >= 0 and out[i] >= 0 else None for i in range(n)]


class EmuReaders:
    """n LZ4Streams in Decompress mode over host arrays: read() is one k4lz4_legacy_read_batch_device"""

    def __init__(self, sources, max_block=1 << 16, threads=4, direct=True):
        self.n, self.threads, self.max_block, self.direct = len(sources), threads, max_block, direct
        self.src, self.src_off, self.src_len = _guarded(sources, 0xEE)
        self.sb = int(lib().k4emu_ls_reader_store_bytes(max_block))
        self.store_off = (256 + np.arange(self.n, dtype=np.uint64) * np.uint64(self.sb + 256)).astype(np.uint64)
        self.store = np.full(self.n * (self.sb + 256) + 256, 0xA5, np.uint8)
        self.plans = []
        self._call(1, np.zeros(self.n, np.int64), False)

    def _call(self, op, counts, interactive):
        n = self.n
        counts = np.ascontiguousarray(counts, np.int64)
        caps = np.maximum(counts, 0) if op == 0 else np.zeros(n, np.int64)
        dst, doff, _ = _guarded([bytes(int(c)) for c in caps], 0xCD)
        dst[:] = 0xCD
        out = np.full(n, -999, np.int64)
        plan = np.zeros(n, np.uint32)
        max_count = int(counts.max()) if self.direct and op == 0 else 0
        p = lambda a: a.ctypes.data  # noqa: E731
        lib().k4emu_ls_read(self.max_block, p(self.store), p(self.store_off), p(self.src), p(self.src_off), p(self.src_len), p(dst), p(doff),
                            p(counts), p(out), n, op, int(interactive), max_count, p(plan), self.threads)
        if op == 0:
            self.plans.append(plan)
        _intact(dst, doff, caps, 0xCD, "a stream's slot")
        _intact(self.store, self.store_off, np.full(n, self.sb), 0xA5, "a stream's store")
        return out, [dst[int(doff[i]):int(doff[i]) + max(int(out[i]), 0)].tobytes() for i in range(n)]

    def read(self, counts, interactive=False):
        """-> per stream: bytes, the code (int), or None where the count is None"""
        c = np.array([-1 if x is None else x for x in counts], np.int64)
        out, got = self._call(0, c, interactive)
        return [None if c[i] < 0 else (int(out[i]) if out[i] < 0 else got[i]) for i in range(self.n)]

    def query(self):
        q = np.zeros(self.n * LSQ_WORDS, np.int64)
        lib().k4emu_ls_query(self.store.ctypes.data, self.store_off.ctypes.data, q.ctypes.data, self.n, 1)
        return q.reshape(self.n, LSQ_WORDS)
