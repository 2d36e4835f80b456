"""The witness of the HC dictionary encoder: the system liblz4 (1.9.3) -- LZ4_createStreamHC, LZ4_resetStreamHC_fast(level),
LZ4_loadDictHC, LZ4_compress_HC_continue -- and its LZ4_streamHC_t read back after the load (hashTable at byte 0, chainTable at byte
131072).  The dictionary and the message lie in one buffer with a gap between them, so that liblz4 never sees the dictionary
directly in front of the source (that would be the prefix arm).  A sound witness for levels 3 .. 9 only.  Test
infrastructure only."""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle_lib import SystemLZ4

K64 = 65536
OFF_HASH, OFF_CHAIN = 0, 131072
_sys = None
_lib = None


def system():
    global _sys
    if _sys is None:
        _sys = SystemLZ4()
    return _sys


def available() -> bool:
    s = system()
    return bool(s.available and s.version == 10903)


def lib():
    global _lib
    if _lib is None:
        L = system().lib
        L.LZ4_createStreamHC.restype = C.c_void_p
        L.LZ4_freeStreamHC.argtypes = [C.c_void_p]
        L.LZ4_resetStreamHC_fast.argtypes = [C.c_void_p, C.c_int]
        L.LZ4_loadDictHC.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.LZ4_compress_HC_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        _lib = L
    return _lib


def load_state(dictionary: np.ndarray, level: int = 9) -> dict:
    """hashTable (32768 words) and chainTable (65536 halfwords) of a stream after LZ4_loadDictHC(dictionary)"""
    L = lib()
    d = np.ascontiguousarray(dictionary, np.uint8)
    buf = np.concatenate([d, np.zeros(8, np.uint8)])
    st = L.LZ4_createStreamHC()
    try:
        L.LZ4_resetStreamHC_fast(st, level)
        L.LZ4_loadDictHC(st, buf.ctypes.data, d.size)
        raw = np.frombuffer(bytes((C.c_uint8 * (OFF_CHAIN + 131072)).from_address(st)), np.uint8)
    finally:
        L.LZ4_freeStreamHC(st)
    return {"hashTable": raw[OFF_HASH:OFF_HASH + 131072].view("<u4").copy(), "chainTable": raw[OFF_CHAIN:OFF_CHAIN + 131072].view("<u2").copy()}


def encode(message: np.ndarray, dictionary: np.ndarray, cap: int, level: int, prefix: bool = False):
    """(LZ4_compress_HC_continue's return, the bytes it wrote) for a fresh stream with the dictionary loaded.  prefix: the message
    directly behind the dictionary -- the other arm, for the tests that show the two differ"""
    L = lib()
    m = np.ascontiguousarray(message, np.uint8)
    d = np.ascontiguousarray(dictionary, np.uint8)
    gap = 0 if prefix else 64
    buf = np.concatenate([d, np.full(gap, 0x5A, np.uint8), m, np.zeros(8, np.uint8)])
    dst = np.full(max(cap, 0) + 8, 0xCD, np.uint8)
    st = L.LZ4_createStreamHC()
    try:
        L.LZ4_resetStreamHC_fast(st, level)
        L.LZ4_loadDictHC(st, buf.ctypes.data, d.size)
        r = L.LZ4_compress_HC_continue(st, buf.ctypes.data + d.size + gap, dst.ctypes.data, m.size, cap)
    finally:
        L.LZ4_freeStreamHC(st)
    assert (dst[max(cap, 0):] == 0xCD).all()
    return int(r), dst[:max(r, 0)].tobytes()


def codec_result(n: int, r: int) -> int:
    """what k4lz4_encode_dict_hc_batch reports for liblz4's return r on a message of n bytes"""
    return 0 if n == 0 else (-1 if r <= 0 else r)


def reference_tables(dictionary: np.ndarray):
    """LZ4_loadDictHC's tables written down from their definition: heads (index 65536 + k, 0 empty) and, for k < D - 3, the chain
    delta of slot k; the mask of written chain slots"""
    kept = np.ascontiguousarray(dictionary[-K64:] if dictionary.size else dictionary, np.uint8)
    D = kept.size
    heads = np.zeros(32768, np.uint32)
    chain = np.full(65536, 0xFFFF, np.uint16)
    written = np.zeros(65536, bool)
    if D >= 4:
        v = kept[:D - 3].astype(np.uint32) | kept[1:D - 2].astype(np.uint32) << 8 | kept[2:D - 1].astype(np.uint32) << 16 | kept[3:D].astype(np.uint32) << 24
        h = ((v.astype(np.uint64) * 2654435761) & 0xFFFFFFFF) >> 17
        for k in range(D - 3):
            delta = K64 + k - int(heads[h[k]])
            chain[k] = min(delta, 65535)
            heads[h[k]] = K64 + k
        written[:D - 3] = True
    return heads, chain, written
