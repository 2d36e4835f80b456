"""The open kernels (k4lz4_chain_open.hpp) under the host wave emulator: tests/emu/emu_chain_prime.cpp + tests/emu/emu_runtime.cpp,
built by g++ into a library of its own.  The set's memory is laid out here the way k4lz4_dict_set_create carves it (kept bytes and
tables at 64-byte steps), the encoders' rows the way k4lz4_chain_encoder_open_dictset_device fills them, with the library's own
k4lz4_chain_encoder_open_plan for the records.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

from k4os.compression.lz4_amd import _native, encoders as E
from dict_encode_cases import reference_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
SO = os.path.join(EMU_DIR, "libk4lz4_emu_chain_prime.so")
K64 = 65536
GUARD = 256
ROW = np.dtype([("ring", "<u8"), ("state", "<u8"), ("kept", "<u8"), ("table", "<u8"), ("keptLen", "<u4"), ("fast", "<u4"),
                ("currentOffset", "<u4"), ("dictSize", "<u4")])


def build() -> str:
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_chain_prime.cpp", "emu_runtime.cpp")] + glob.glob(os.path.join(EMU_DIR, "hip", "*.h")) + \
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
                                       os.path.join(EMU_DIR, "emu_chain_prime.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
                os.replace(tmp, SO)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.k4emu_ce_open.restype = None
        _lib.k4emu_ce_open.argtypes = [C.c_void_p] * 3 + [C.c_longlong, C.c_int]
        _lib.k4emu_cd_open.restype = None
        _lib.k4emu_cd_open.argtypes = [C.c_void_p] * 9 + [C.c_longlong, C.c_int, C.c_int]
        assert _lib.k4emu_open_row_bytes() == ROW.itemsize
    return _lib


def aligned(nbytes: int, fill: int, align: int = 256):
    """-> (buffer filled with `fill`, the offset of its first `align`-aligned byte)"""
    buf = np.full(nbytes + align, fill, np.uint8)
    return buf, (-buf.ctypes.data) % align


class EmuSet:
    """a k4lz4_dict_set's memory for a list of dictionaries: every entry's last 64 KiB and its LZ4_loadDict table (entries that keep
    fewer than 8 bytes share the zeroed one), with guard bytes (0x5A) around the allocation"""

    def __init__(self, dictionaries):
        self.kept = [np.ascontiguousarray(d, np.uint8)[max(len(d) - K64, 0):] for d in dictionaries]
        self.n = len(self.kept)
        at, self.entry_off = 0, np.zeros(max(self.n, 1), np.uint64)
        for e, k in enumerate(self.kept):
            self.entry_off[e] = at
            at += (k.size + 63) // 64 * 64
        at += 64
        self.entry_len = np.array([k.size for k in self.kept] + [0] * (self.n == 0), np.int32)
        self.table_off = np.zeros(max(self.n, 1), np.uint64)
        self.tables = [reference_table(k) for k in self.kept]
        empty = at
        at += 16384
        for e, k in enumerate(self.kept):
            self.table_off[e] = at if k.size >= 8 else empty
            at += 16384 if k.size >= 8 else 0
        self.bytes = at
        self.buf, pad = aligned(at + 2 * GUARD, 0x5A)
        self.base = pad + GUARD
        mem = self.buf[self.base:self.base + at]
        mem[:] = 0x33                                       # what lies between the regions is nobody's
        mem[empty:empty + 16384] = 0
        for e, k in enumerate(self.kept):
            mem[int(self.entry_off[e]):int(self.entry_off[e]) + k.size] = k
            if k.size >= 8:
                mem[int(self.table_off[e]):int(self.table_off[e]) + 16384] = self.tables[e].view(np.uint8)
        self.before = self.buf.copy()

    @property
    def ptr(self) -> int:
        return self.buf.ctypes.data + self.base

    def unchanged(self):
        assert np.array_equal(self.buf, self.before), "the set's memory was written"


class EmuEncoders:
    """n encoder stores (guard bytes 0xA5 around each) and their host records"""

    def __init__(self, settings):
        self.records = [E.chain_encoder_record(*s) for s in settings]
        self.n = len(self.records)
        self.sizes = np.array([r.storeBytes for r in self.records], np.int64)
        self.store, pad = aligned(int(self.sizes.sum()) + GUARD * (self.n + 1), 0xA5)
        self.store_off = (pad + GUARD + np.concatenate(([0], np.cumsum(self.sizes[:-1] + GUARD)))).astype(np.uint64)
        assert not ((self.store.ctypes.data + self.store_off.astype(np.int64)) % 256).any()

    def intact(self):
        mask = np.ones(self.store.size, bool)
        for o, c in zip(self.store_off, self.sizes):
            mask[int(o):int(o) + int(c)] = False
        assert (self.store[mask] == 0xA5).all(), "a write outside a stream's store"

    def open(self, idx, st: EmuSet, threads: int = 4):
        """what k4lz4_chain_encoder_open_dictset_device does: the records through k4lz4_chain_encoder_open_plan, the rows, one launch"""
        nat = _native.load_library()
        rows = np.zeros(self.n, ROW)
        for s, (rec, e) in enumerate(zip(self.records, idx)):
            assert nat.k4lz4_chain_encoder_open_plan(C.byref(rec), int(st.entry_len[e]) if e >= 0 else -1) == 0
            r = rows[s]
            r["ring"] = int(self.store_off[s]) + E._ring_at(rec)
            r["keptLen"] = rec.pointer
            if rec.pointer:
                r["kept"] = st.entry_off[e]
            if rec.kind == 2:
                r["state"] = self.store_off[s]
                r["fast"] = 1 if rec.dictSize else 2
                if rec.dictSize:
                    r["table"] = st.table_off[e]
                r["currentOffset"], r["dictSize"] = rec.currentOffset, rec.dictSize
        lib().k4emu_ce_open(rows.ctypes.data, self.store.ctypes.data, st.ptr, self.n, threads)
        self.intact()
        st.unchanged()
        return rows

    def ring(self, s: int) -> bytes:
        at = int(self.store_off[s]) + E._ring_at(self.records[s])
        return self.store[at:at + int(self.records[s].pointer)].tobytes()

    def state(self, s: int):
        at = int(self.store_off[s])
        return np.frombuffer(self.store[at:at + E.FAST_CHAIN_STATE.itemsize].tobytes(), E.FAST_CHAIN_STATE)[0]

    def untouched_behind(self, s: int, rows):
        """nothing of the store but the state and the ring's first keptLen bytes is written"""
        o, c = int(self.store_off[s]), int(self.sizes[s])
        mask = np.ones(c, bool)
        if rows[s]["fast"]:
            mask[:E.FAST_CHAIN_STATE.itemsize] = False
        at = E._ring_at(self.records[s])
        mask[at:at + int(rows[s]["keptLen"])] = False
        assert (self.store[o:o + c][mask] == 0xA5).all(), "a write beyond the kept bytes"


def cd_open(decoders, idx, st: EmuSet, threads: int = 4):
    """k4_cdec_open_kernel on a chain_decoder_emu.EmuDecoders' stores -> (outLen, the status word)"""
    idx = np.ascontiguousarray(idx, np.int32)
    out = np.full(decoders.n, -999, np.int64)
    status = np.zeros(1, np.uint32)
    lib().k4emu_cd_open(decoders.recs, decoders.store.ctypes.data, decoders.store_off.ctypes.data, idx.ctypes.data, st.ptr,
                        st.entry_off.ctypes.data, st.entry_len.ctypes.data, out.ctypes.data, status.ctypes.data, decoders.n, st.n, threads)
    decoders._check_stores()
    st.unchanged()
    return out.tolist(), int(status[0])
