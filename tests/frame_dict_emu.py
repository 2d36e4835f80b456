"""k4lz4_decode_frames_dictset_device's launch sequence over the kernels of k4lz4_frame_dict.hpp / k4lz4_frame_read.hpp under the host
wave emulator: tests/emu/emu_frame_dict.cpp + tests/emu/emu_runtime.cpp, built by g++ into a library of its own.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
SO = os.path.join(EMU_DIR, "libk4lz4_emu_frame_dict.so")
GUARD = 64


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_frame_dict.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
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
                                       os.path.join(EMU_DIR, "emu_frame_dict.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.k4emu_frame_dict_decode.restype = C.c_int
        _lib.k4emu_frame_dict_decode.argtypes = [C.c_void_p] * 3 + [C.c_longlong] + [C.c_void_p] * 11 + [C.c_int] * 3
    return _lib


def pack(items, align=16, guard=0):
    """byte strings / arrays -> (buffer, offsets u64, lengths u64), `guard` bytes in front of and between them"""
    arrs = [np.frombuffer(bytes(x), np.uint8) if not isinstance(x, np.ndarray) else x for x in items]
    lens = np.array([a.size for a in arrs], np.uint64)
    off = np.zeros(len(arrs), np.uint64)
    at = guard
    for i, a in enumerate(arrs):
        off[i] = at
        at += (a.size + align - 1) // align * align + guard
    buf = np.zeros(at + 64, np.uint8)
    for a, o in zip(arrs, off):
        buf[int(o):int(o) + a.size] = a
    return buf, off, lens


def decode(frames, caps, entries=None, ids=None, chain_waves=1024, threads=4):
    """-> (outLen i64, outputs, size u64, status i32, dict index i32).  entries None: no set (the plain kernels).  caps[f] None: the
    size the walk reports.  Every slot lies between GUARD bytes of 0xCD, which are checked."""
    n = len(frames)
    src, foff, flen = pack(frames)
    if entries is not None:
        kept = [np.ascontiguousarray(e[-65536:], np.uint8) for e in entries]
        dbuf, eoff, elen = pack(kept, align=64)
        elen32 = elen.astype(np.int32)
        idarr = np.array(ids, np.uint32)
        nd = len(entries)
    else:
        dbuf, eoff, elen32, idarr, nd = np.zeros(64, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros(1, np.uint32), -1
    size, status, idx = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.int32)
    out = np.zeros(n, np.int64)
    p = lambda a: a.ctypes.data
    # a first pass sizes the targets (the walk alone would do; the whole sequence runs against targets of no bytes)
    zero = np.zeros(n, np.uint64)
    scratch = np.zeros(64, np.uint8)
    lib().k4emu_frame_dict_decode(p(src), p(foff), p(flen), n, p(scratch), p(zero), p(zero), p(out), p(size), p(status), p(idx), p(dbuf), p(eoff),
                                  p(elen32), p(idarr), nd, chain_waves, threads)
    cap = np.array([int(s) if c is None else int(c) for s, c in zip(size, caps)], np.uint64)
    doff = np.zeros(n, np.uint64)
    at = GUARD
    for f in range(n):
        doff[f] = at
        at += int(cap[f]) + GUARD
    dst = np.full(at + 64, 0xCD, np.uint8)
    for f in range(n):
        dst[int(doff[f]):int(doff[f]) + int(cap[f])] = 0
    size2, status2, idx2 = size.copy(), status.copy(), idx.copy()
    lib().k4emu_frame_dict_decode(p(src), p(foff), p(flen), n, p(dst), p(doff), p(cap), p(out), p(size2), p(status2), p(idx2), p(dbuf), p(eoff),
                                  p(elen32), p(idarr), nd, chain_waves, threads)
    assert (size2 == size).all() and (status2 == status).all() and (idx2 == idx).all()
    mask = np.ones(dst.size, bool)
    for f in range(n):
        mask[int(doff[f]):int(doff[f]) + int(cap[f])] = False
    assert (dst[mask] == 0xCD).all(), "a byte outside the frames' slots was written"
    outs = [dst[int(doff[f]):int(doff[f]) + int(out[f])].tobytes() if out[f] >= 0 else None for f in range(n)]
    return out, outs, size, status, idx
