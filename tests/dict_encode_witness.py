"""The witness of the dictionary encoder: the system liblz4 (1.9.3) -- LZ4_loadDict, then LZ4_compress_fast_continue(..., 1) on that
stream -- and its LZ4_stream_t read back after the load (fast_chain_witness has the layout).  The dictionary and the message lie in
one buffer with a gap between them, so that liblz4 never sees the dictionary directly in front of the source (that would be the
prefix arm).  Test infrastructure only."""
from __future__ import annotations

import ctypes as C

import numpy as np

import fast_chain_witness as FW
from oracle_lib import SystemLZ4

_sys = None


def system():
    global _sys
    if _sys is None:
        _sys = SystemLZ4()
    return _sys


def available() -> bool:
    s = system()
    return bool(s.available and s.version == 10903)


def load_state(dictionary: np.ndarray) -> dict:
    """hashTable / currentOffset / dictSize of a stream after LZ4_loadDict(dictionary)"""
    L = system().lib
    d = np.ascontiguousarray(dictionary, np.uint8)
    buf = np.concatenate([d, np.zeros(8, np.uint8)])
    st = L.LZ4_createStream()
    try:
        L.LZ4_loadDict(C.c_void_p(st), buf.ctypes.data_as(C.POINTER(C.c_uint8)), d.size)
        raw = np.frombuffer(bytes((C.c_uint8 * FW.STATE_BYTES).from_address(st)), np.uint8)
    finally:
        L.LZ4_freeStream(C.c_void_p(st))
    return {"hashTable": raw[:16384].view("<u4").copy(), "currentOffset": int(raw[FW.OFF_CURRENT:FW.OFF_CURRENT + 4].view("<u4")[0]),
            "dictSize": int(raw[FW.OFF_DICTSIZE:FW.OFF_DICTSIZE + 4].view("<u4")[0])}


def encode(message: np.ndarray, dictionary: np.ndarray, cap: int):
    """(LZ4_compress_fast_continue's return, the bytes it wrote) for a fresh stream with the dictionary loaded"""
    L = system().lib
    m = np.ascontiguousarray(message, np.uint8)
    d = np.ascontiguousarray(dictionary, np.uint8)
    buf = np.concatenate([d, np.full(64, 0x5A, np.uint8), m, np.zeros(8, np.uint8)])
    dst = np.full(max(cap, 0) + 8, 0xCD, np.uint8)
    u8p = C.POINTER(C.c_uint8)
    base = buf.ctypes.data
    st = L.LZ4_createStream()
    try:
        L.LZ4_loadDict(C.c_void_p(st), C.cast(base, u8p), d.size)
        r = L.LZ4_compress_fast_continue(C.c_void_p(st), C.cast(base + d.size + 64, u8p), dst.ctypes.data_as(u8p), m.size, cap, 1)
    finally:
        L.LZ4_freeStream(C.c_void_p(st))
    assert (dst[max(cap, 0):] == 0xCD).all()
    return int(r), dst[:max(r, 0)].tobytes()


def codec_result(n: int, r: int) -> int:
    """what k4lz4_encode_dict_batch reports for liblz4's return r on a message of n bytes"""
    return 0 if n == 0 else (-1 if r <= 0 else r)
