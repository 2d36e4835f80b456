"""Many open ILZ4Decoders (k4lz4_chain_decoder.hpp) under the host wave emulator: tests/emu/emu_chain_decoder.cpp +
tests/emu/emu_runtime.cpp, built by g++ into a library of its own.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

from chain_decoder_witness import CDQ_WORDS, record_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
SO = os.path.join(EMU_DIR, "libk4lz4_emu_chain_decoder.so")
GUARD = 64
STORE_GUARD = 256


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_chain_decoder.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
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
                                       os.path.join(EMU_DIR, "emu_chain_decoder.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        for f in (_lib.k4emu_cd_block_size, _lib.k4emu_cd_ring_length, _lib.k4emu_cd_store_bytes):
            f.restype = C.c_longlong
        _lib.k4emu_cd_block_size.argtypes = [C.c_longlong]
        _lib.k4emu_cd_ring_length.argtypes = [C.c_longlong, C.c_longlong, C.c_int]
        _lib.k4emu_cd_store_bytes.argtypes = [C.c_longlong, C.c_longlong, C.c_int]
        _lib.k4emu_cd_reset.restype = None
        _lib.k4emu_cd_reset.argtypes = [C.c_void_p] * 4 + [C.c_longlong, C.c_int]
        _lib.k4emu_cd_run.restype = None
        _lib.k4emu_cd_run.argtypes = [C.c_void_p] * 13 + [C.c_longlong, C.c_int, C.c_int]
        _lib.k4emu_cd_drain.restype = None
        _lib.k4emu_cd_drain.argtypes = [C.c_void_p] * 7 + [C.c_longlong, C.c_int]
        _lib.k4emu_cd_query.restype = None
        _lib.k4emu_cd_query.argtypes = [C.c_void_p] * 3 + [C.c_longlong, C.c_int]
    return _lib


class Record(C.Structure):
    """k4lz4_chain_decoder"""
    _fields_ = [("blockSize", C.c_int32), ("extraBlocks", C.c_int32), ("chaining", C.c_int32), ("reserved", C.c_int32),
                ("storeBytes", C.c_int64)]


def slots(caps, guard, fill):
    """-> (buffer filled with `fill`, offsets): slots of caps[i] bytes with `guard` bytes before, between and behind them"""
    caps = np.asarray(caps, np.uint64)
    off = np.full(len(caps), guard, np.uint64)
    if len(caps) > 1:
        off[1:] += np.cumsum(caps[:-1] + np.uint64(guard))
    return np.full(int(caps.sum()) + guard * (len(caps) + 1) + 16, fill, np.uint8), off


def intact(buf, off, caps, fill, what):
    mask = np.ones(buf.size, bool)
    for o, c in zip(off, caps):
        mask[int(o):int(o) + int(c)] = False
    assert (buf[mask] == fill).all(), f"a write outside {what}"


class EmuDecoders:
    """n decoders over host arrays: every call is one launch of the device form's kernel, with guard bytes around every store, every
    drain slot and every source"""

    def __init__(self, settings, threads=4):
        self.settings = list(settings)
        self.n, self.threads = len(self.settings), threads
        self.recs = (Record * self.n)()
        for r, (c, b, e) in zip(self.recs, self.settings):
            B = int(lib().k4emu_cd_block_size(int(b)))
            r.blockSize, r.extraBlocks, r.chaining = B, (max(int(e), 0) if c else 0), (1 if c else 0)
            r.storeBytes = lib().k4emu_cd_store_bytes(B, r.extraBlocks, r.chaining)
        self.sizes = np.array([r.storeBytes for r in self.recs], np.uint64)
        assert not (self.sizes % 256).any()
        self.store = np.full(int(self.sizes.sum()) + STORE_GUARD * (self.n + 1) + 512, 0xA5, np.uint8)
        pad = (-self.store.ctypes.data) % 256        # the stores are 256-byte aligned in memory
        self.store_off = (pad + STORE_GUARD + np.concatenate(([0], np.cumsum(self.sizes[:-1] + np.uint64(STORE_GUARD))))).astype(np.uint64)
        assert not ((self.store.ctypes.data + self.store_off.astype(np.int64)) % 256).any()
        self.reset()

    def _check_stores(self):
        intact(self.store, self.store_off, self.sizes, 0xA5, "a stream's store")

    def reset(self, which=None):
        idx = np.arange(self.n) if which is None else np.asarray(list(which), np.int64)
        if idx.size == 0:
            return
        recs = (Record * idx.size)(*[self.recs[int(i)] for i in idx])
        off = np.ascontiguousarray(self.store_off[idx])
        out = np.full(idx.size, -999, np.int64)
        lib().k4emu_cd_reset(recs, self.store.ctypes.data, off.ctypes.data, out.ctypes.data, idx.size, 1)
        assert (out == 0).all()
        self._check_stores()

    def run(self, records, drain=False, caps=None):
        n = self.n
        src, roff, rlen, rbs, first, nrec = record_table(records, GUARD)
        caps = np.zeros(n, np.uint64) if caps is None else np.asarray(caps, np.uint64)
        dst, doff = slots(caps, GUARD, 0xCD)
        rec_out = np.full(max(len(rlen), 1), -999, np.int32)
        out = np.full(n, -999, np.int64)
        p = lambda a: a.ctypes.data  # noqa: E731
        lib().k4emu_cd_run(p(self.store), p(self.store_off), p(src), p(roff), p(rlen), p(rbs), p(first), p(nrec), p(dst) if drain else None,
                           p(doff) if drain else None, p(caps) if drain else None, p(rec_out), p(out), n, 1 if drain else 0, self.threads)
        self._check_stores()
        intact(dst, doff, caps, 0xCD, "a stream's drain slot")
        ro = [rec_out[int(f):int(f) + int(k)].tolist() for f, k in zip(first, nrec)]
        given = [sum(g for g in r[:next((j for j, g in enumerate(r) if g < 0), len(r))]) if drain else 0 for r in ro]
        for i in range(n):                           # what lies behind the drained bytes stays as it was
            assert (dst[int(doff[i]) + given[i]:int(doff[i]) + int(caps[i])] == 0xCD).all()
        return ro, out.tolist(), [dst[int(doff[i]):int(doff[i]) + given[i]].tobytes() for i in range(n)]

    def drain(self, offsets, lengths):
        n = self.n
        offsets, lengths = np.asarray(offsets, np.int64), np.asarray(lengths, np.int64)
        caps = np.clip(lengths, 0, 1 << 27).astype(np.uint64)
        dst, doff = slots(caps, GUARD, 0xCD)
        out = np.full(n, -999, np.int64)
        before = self.store.copy()
        lib().k4emu_cd_drain(self.store.ctypes.data, self.store_off.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, dst.ctypes.data,
                             doff.ctypes.data, out.ctypes.data, n, self.threads)
        assert (self.store == before).all(), "a drain changed a store"
        intact(dst, doff, np.maximum(out, 0), 0xCD, "a drain's range")
        return [int(out[i]) if out[i] < 0 else dst[int(doff[i]):int(doff[i]) + int(out[i])].tobytes() for i in range(n)]

    def query(self):
        q = np.zeros(self.n * CDQ_WORDS, np.int64)
        lib().k4emu_cd_query(self.store.ctypes.data, self.store_off.ctypes.data, q.ctypes.data, self.n, 1)
        return q.reshape(self.n, CDQ_WORDS)
