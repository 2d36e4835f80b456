"""The HC dictionary encoder's kernels (k4lz4_dict_encode_hc.hpp) under the host wave emulator: tests/emu/emu_dict_encode_hc.cpp +
tests/emu/emu_runtime.cpp, built by g++ into a library of its own.  The list of distinct dictionaries is planned here the way
k4lz4_capi.hip's dict_list plans it for the HC family.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
SO = os.path.join(EMU_DIR, "libk4lz4_emu_dict_encode_hc.so")


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_dict_encode_hc.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
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
                                       os.path.join(EMU_DIR, "emu_dict_encode_hc.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.k4emu_dict_hc_encode.argtypes = [C.c_void_p] * 7 + [C.c_longlong, C.c_int] + [C.c_void_p] * 5 + \
            [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return _lib


def plan(dict_off, dict_len):
    """per entry (kept offset, kept length, table) and per distinct table (kept offset, kept length): the HC family's dict_list of k4lz4_capi.hip.
    Every byte of a dictionary counts, down to one (LZ4_loadDictHC keeps what LZ4_loadDict drops)"""
    nd = len(dict_len)
    kept_off, kept_len, table = np.zeros(nd, np.uint64), np.zeros(nd, np.uint32), np.zeros(nd, np.uint32)
    seen, t_off, t_len = {}, [], []
    for d in range(nd):
        n = int(dict_len[d])
        if n > 0:
            kept_len[d] = min(n, 65536)
            kept_off[d] = int(dict_off[d]) + n - int(kept_len[d])
        key = (int(kept_off[d]), int(kept_len[d]))
        if key not in seen:
            seen[key] = len(t_off)
            t_off.append(key[0]); t_len.append(key[1])
        table[d] = seen[key]
    return kept_off, kept_len, table, np.array(t_off or [0], np.uint64), np.array(t_len or [0], np.uint32)


def encode(src, src_off, src_len, dst, dst_off, dst_cap, level, dict_idx, dct, dict_off, dict_len, workgroups: int = 2, threads: int = 4):
    """-> (outLen, heads[nDict, 32768], chain[nDict, 65536] as the load kernel left them, kept length per entry, status word);
    dst is written in place"""
    n = len(src_len)
    kept_off, kept_len, table, t_off, t_len = plan(dict_off, dict_len)
    tb = lib().k4emu_dict_hc_table_bytes()
    tables = np.full((len(t_off), tb), 0xEE, np.uint8)
    out = np.full(max(n, 1), -12345, np.int32)
    status = np.zeros(1, np.uint32)
    idx = np.ascontiguousarray(dict_idx, np.int32)
    p = lambda a: a.ctypes.data if a.size else None
    rc = lib().k4emu_dict_hc_encode(p(src), p(src_off), p(src_len), p(dst), p(dst_off), p(dst_cap), p(out), n, int(level), p(idx), p(dct),
                                    p(kept_off), p(kept_len), p(table), len(dict_len), p(t_off), p(t_len), len(t_off), p(tables), p(status),
                                    workgroups, threads)
    assert rc != 1, "the dispatch order is not a permutation of the messages"
    assert rc != 2, "a wave slot's head table is not zero after the launch"
    heads = np.ascontiguousarray(tables[:, :131072]).view("<u4")
    chain = np.ascontiguousarray(tables[:, 131072:]).view("<u2")
    sel = table if len(dict_len) else table[:0]
    return out[:n], heads[sel], chain[sel], kept_len, int(status[0])
