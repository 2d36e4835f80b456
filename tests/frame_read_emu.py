"""The frame reader's walk, scan and fill kernels (k4lz4_frame_read.hpp) under the host wave emulator: tests/emu/emu_frame_read.cpp +
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
SO = os.path.join(EMU_DIR, "libk4lz4_emu_frame_read.so")


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_frame_read.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
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
                                       os.path.join(EMU_DIR, "emu_frame_read.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.k4emu_frame_read.restype = C.c_longlong
        _lib.k4emu_frame_read.argtypes = [C.c_void_p] * 3 + [C.c_longlong] + [C.c_void_p] * 20 + [C.c_longlong] + [C.c_void_p] * 3 + [C.c_int]
    return _lib


@dataclass
class Walked:
    """one frame as the kernels saw it"""
    status: int
    size: int                 # the decoded-size bound (k4lz4_frame_sizes)
    flg: int
    bd: int
    block_size: int
    content_length: int
    content_checksum: int
    hdr_end: int
    block_off: List[int]      # inside the frame
    block_len: List[int]      # bit 31 = raw
    block_checksum: List[int]
    block_dst_off: List[int]  # the parallel decoder's place (relative to the frame's dstOff)
    block_dst_cap: List[int]
    block_src_len: List[int]


def walk(frames, dst_cap=None, threads: int = 4):
    """-> ([Walked] per frame, counters)"""
    n = len(frames)
    frames = [np.frombuffer(bytes(f), np.uint8) for f in frames]
    foff = np.zeros(n, np.uint64)
    flen = np.array([f.size for f in frames], np.uint64)
    if n > 1:
        foff[1:] = np.cumsum(((flen + 15) // 16 * 16)[:-1])
    src = np.zeros(int(((flen + 15) // 16 * 16).sum()) + 64, np.uint8)
    for i, f in enumerate(frames):
        src[int(foff[i]):int(foff[i]) + f.size] = f
    cap = np.array(dst_cap if dst_cap is not None else [1 << 40] * n, np.uint64)
    doff = np.arange(n, dtype=np.uint64) * np.uint64(1 << 41)
    u64 = lambda: np.zeros(max(n, 1), np.uint64)
    u32 = lambda: np.zeros(max(n, 1), np.uint32)
    i32 = lambda: np.zeros(max(n, 1), np.int32)
    bound, clen, first, nblk, status, desc, bsize, csum, hdr_end = u64(), u64(), u64(), u32(), i32(), u32(), i32(), u32(), u32()
    size, st2 = u64(), i32()
    mb = int(flen.sum()) // 4 + 1
    boff, bhlen, bdoff = (np.zeros(mb, np.uint64) for _ in range(3))
    blen, bown, bidx, bsum = (np.zeros(mb, np.uint32) for _ in range(4))
    bsrc, bdcap = np.zeros(mb, np.int32), np.zeros(mb, np.int32)
    counters = np.zeros(4, np.uint64)
    p = lambda a: a.ctypes.data
    nb = lib().k4emu_frame_read(p(src), p(foff), p(flen), n, p(doff), p(cap), p(bound), p(clen), p(first), p(nblk), p(status), p(desc),
                                p(bsize), p(csum), p(hdr_end), p(boff), p(bhlen), p(bdoff), p(blen), p(bown), p(bidx), p(bsum), p(bsrc),
                                p(bdcap), mb, p(counters), p(size), p(st2), threads)
    assert nb >= 0
    assert (size[:n] == bound[:n]).all() and (st2[:n] == status[:n]).all()
    assert int(counters[0]) == nb == int(nblk[:n].sum())
    out = []
    for f in range(n):
        rows = range(int(first[f]), int(first[f]) + int(nblk[f]))
        assert all(int(bown[r]) == f and int(bidx[r]) == r - int(first[f]) for r in rows)
        out.append(Walked(int(status[f]), int(bound[f]), int(desc[f]) & 0xFF, int(desc[f]) >> 8, int(bsize[f]), int(clen[f]), int(csum[f]),
                          int(hdr_end[f]), [int(boff[r] - foff[f]) for r in rows], [int(blen[r]) for r in rows],
                          [int(bsum[r]) for r in rows], [int(bdoff[r] - doff[f]) for r in rows], [int(bdcap[r]) for r in rows],
                          [int(bsrc[r]) for r in rows]))
    return out, [int(c) for c in counters]
