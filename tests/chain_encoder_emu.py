"""Many open ILZ4Encoders (k4lz4_chain_encoder.hpp) under the host wave emulator: tests/emu/emu_chain_encoder.cpp +
tests/emu/emu_runtime.cpp, built by g++ into a library of its own.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
SO = os.path.join(EMU_DIR, "libk4lz4_emu_chain_encoder.so")


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_chain_encoder.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
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
                                       os.path.join(EMU_DIR, "emu_chain_encoder.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.k4emu_ce_call.restype = C.c_longlong
        _lib.k4emu_ce_call.argtypes = [C.c_void_p] * 7 + [C.c_longlong] + [C.c_void_p] * 2 + [C.c_longlong] + [C.c_void_p] * 3 + [C.c_longlong] + \
            [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int]
    return _lib
