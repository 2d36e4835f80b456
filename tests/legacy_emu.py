"""The legacy stream kernels (k4lz4_legacy.hpp: reader walk / scan / fill, writer count / scan / fill / record sizes, Unwrap sizes)
under the host wave emulator: tests/emu/emu_legacy.cpp +
tests/emu/emu_runtime.cpp, built by g++ into a library of its own.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess
from dataclasses import dataclass
from typing import List

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
SO = os.path.join(EMU_DIR, "libk4lz4_emu_legacy.so")


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_legacy.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
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
                                       os.path.join(EMU_DIR, "emu_legacy.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.k4emu_legacy_read.restype = C.c_longlong
        _lib.k4emu_legacy_read.argtypes = [C.c_void_p] * 3 + [C.c_longlong] + [C.c_void_p] * 16 + [C.c_longlong, C.c_int]
        _lib.k4emu_legacy_write.restype = C.c_longlong
        _lib.k4emu_legacy_write.argtypes = [C.c_void_p] * 2 + [C.c_longlong, C.c_int] + [C.c_void_p] * 11 + [C.c_longlong, C.c_void_p, C.c_int]
        _lib.k4emu_unwrap_sizes.restype = None
        _lib.k4emu_unwrap_sizes.argtypes = [C.c_void_p] * 4 + [C.c_longlong] + [C.c_void_p] * 4 + [C.c_int]
    return _lib


def _pack(bufs):
    n = len(bufs)
    bufs = [np.frombuffer(bytes(b), np.uint8) for b in bufs]
    off = np.zeros(n, np.uint64)
    ln = np.array([b.size for b in bufs], np.uint64)
    if n > 1:
        off[1:] = np.cumsum(((ln + 15) // 16 * 16)[:-1])
    src = np.zeros(int(((ln + 15) // 16 * 16).sum()) + 64, np.uint8)
    for i, b in enumerate(bufs):
        src[int(off[i]):int(off[i]) + b.size] = b
    return src, off, ln


@dataclass
class Walked:
    status: int
    size: int
    rows: List[tuple]         # (payload offset in the stream, U, C or 0 for raw, kind, dst offset)


def walk(streams, dst_cap=None, threads: int = 4):
    n = len(streams)
    src, off, ln = _pack(streams)
    cap = np.array(dst_cap if dst_cap is not None else [1 << 40] * n, np.uint64)
    doff = np.arange(n, dtype=np.uint64) * np.uint64(1 << 41)
    m = max(n, 1)
    nch, bound, first, size = (np.zeros(m, np.uint64) for _ in range(4))
    status, st2 = np.zeros(m, np.int32), np.zeros(m, np.int32)
    mr = int(ln.sum()) // 3 + 1
    roff, rdst = np.zeros(mr, np.uint64), np.zeros(mr, np.uint64)
    rown, ridx = np.zeros(mr, np.uint32), np.zeros(mr, np.uint32)
    rsrc, rcap, rlen = (np.zeros(mr, np.int32) for _ in range(3))
    rkind = np.zeros(mr, np.uint8)
    p = lambda a: a.ctypes.data
    rows = lib().k4emu_legacy_read(p(src), p(off), p(ln), n, p(doff), p(cap), p(nch), p(bound), p(status), p(first), p(size), p(st2),
                                   p(roff), p(rdst), p(rown), p(ridx), p(rsrc), p(rcap), p(rlen), p(rkind), mr, threads)
    assert rows >= 0 and rows == int(nch[:n].sum())
    assert (size[:n] == bound[:n]).all() and (st2[:n] == status[:n]).all()
    out = []
    for s in range(n):
        rs = range(int(first[s]), int(first[s]) + int(nch[s]))
        assert all(int(rown[r]) == s and int(ridx[r]) == r - int(first[s]) for r in rs)
        out.append(Walked(int(status[s]), int(bound[s]),
                          [(int(roff[r] - off[s]), int(rlen[r]), int(rsrc[r]), int(rkind[r]), int(rdst[r] - doff[s])) for r in rs]))
    return out


def write_plan(lengths, block_size, enc_len=None, threads: int = 4):
    """-> dict of the writer's per-stream and per-row arrays (enc_len: per row, the encoder's result; None: stop after the fill)"""
    n = len(lengths)
    ln = np.array(lengths, np.uint64)
    off = np.zeros(n, np.uint64)
    if n > 1:
        off[1:] = np.cumsum(ln[:-1])
    m = max(n, 1)
    nch, first, aoff = (np.zeros(m, np.uint64) for _ in range(3))
    bs = max(16, block_size)
    mr = int(sum((int(x) + bs - 1) // bs for x in lengths)) + 1
    csrc, cenc, rlen, roff = (np.zeros(mr, np.uint64) for _ in range(4))
    clen, ccap = np.zeros(mr, np.int32), np.zeros(mr, np.int32)
    own = np.zeros(mr, np.uint32)
    el = None if enc_len is None else np.ascontiguousarray(np.concatenate([np.asarray(enc_len, np.int32), np.zeros(1, np.int32)]))
    ab = np.zeros(1, np.uint64)
    p = lambda a: a.ctypes.data
    rows = lib().k4emu_legacy_write(p(off), p(ln), n, block_size, p(nch), p(first), p(aoff), p(csrc), p(clen), p(cenc), p(ccap), p(own),
                                    None if el is None else p(el), p(rlen), p(roff), mr, p(ab), threads)
    assert rows >= 0
    return dict(rows=rows, nch=nch[:n], first=first[:n], arena_off=aoff[:n], arena_bytes=int(ab[0]), src_off=csrc[:rows] - 0,
                src_len=clen[:rows], enc_off=cenc[:rows], enc_cap=ccap[:rows], owner=own[:rows], rec_len=rlen[:rows], rec_off=roff[:rows],
                stream_off=off)


def unwrap_sizes(bufs, caps=None, threads: int = 2):
    n = len(bufs)
    src, off, ln = _pack(bufs)
    ln32 = ln.astype(np.int32)
    cap = np.array(caps if caps is not None else [0x7FFFFFFF] * n, np.int32)
    m = max(n, 1)
    out, dlen, dcap = (np.zeros(m, np.int32) for _ in range(3))
    doff = np.zeros(m, np.uint64)
    p = lambda a: a.ctypes.data
    lib().k4emu_unwrap_sizes(p(src), p(off), p(ln32), p(cap), n, p(out), p(doff), p(dlen), p(dcap), threads)
    return out[:n], dlen[:n], dcap[:n]
