"""ctypes binding of libk4lz4.so (include/k4lz4.h).  This is the ONLY compute path of the package:
if the shared object is missing, or no gfx950 device is usable, every operation raises -- there is
no CPU fallback (the CPU oracle under oracle/ is test infrastructure and is never imported here)."""
from __future__ import annotations

import ctypes as C
import os
import threading

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libk4lz4.so")

K4LZ4_OK = 0
E_HIP, E_ARG, E_NOMEM, E_NO_DEVICE, E_UNSUPPORTED = -1, -2, -3, -4, -5
FLAG_RAW_RETURN = 1
FLAG_PICKLE_WRITER = 2
FLAG_NO_REORDER = 4
FLAG_REORDER = 8
FLAG_NO_SPLIT = 16
FLAG_PARTIAL = 32
FLAG_X32 = 128
FLAG_ALLOW_COPY = 64
FLAG_SEGMENTS = 256
# enum k4lz4_decode_kernel (k4lz4_last_decode_kernel, a diagnostic)
DECODE_KERNEL_NONE, DECODE_KERNEL_PAIR2, DECODE_KERNEL_PAIR, DECODE_KERNEL_SINGLE, DECODE_KERNEL_DENSE, DECODE_KERNEL_PROF = 0, 1, 2, 3, 4, 5
DECODE_KERNEL_UNPICKLE_PAIR2, DECODE_KERNEL_UNPICKLE_PAIR, DECODE_KERNEL_UNPICKLE_SINGLE = 9, 10, 11
DECODE_KERNEL_PACE = 64
# enum k4lz4_encode_route (k4lz4_last_encode_route, a diagnostic): one bit per kernel family and launch fact
ENCODE_ROUTE_NONE = 0
ENCODE_ROUTE_PARSE = 1 << 0
ENCODE_ROUTE_PARSE_BIG = 1 << 1
ENCODE_ROUTE_PARSE_SEG = 1 << 2
ENCODE_ROUTE_EMIT = 1 << 3
ENCODE_ROUTE_REST = 1 << 4
ENCODE_ROUTE_LDS = 1 << 5
ENCODE_ROUTE_MORE = 1 << 6
ENCODE_ROUTE_GTAB = 1 << 7
ENCODE_ROUTE_SEGMENTS = 1 << 8
ENCODE_ROUTE_PROF = 1 << 9
ENCODE_ROUTE_ALLOW_COPY = 1 << 10
ENCODE_ROUTE_PICKLE = 1 << 11
ENCODE_ROUTE_ENVELOPE = 1 << 12
ENCODE_ROUTE_HC_CHAIN_PART = 1 << 13
ENCODE_ROUTE_HC_CHAIN_LDS = 1 << 14
ENCODE_ROUTE_HC_CHAIN_MEM = 1 << 15
ENCODE_ROUTE_HC_CAND_LDS = 1 << 16
ENCODE_ROUTE_HC_CAND_MEM = 1 << 17
ENCODE_ROUTE_HC_PARSE = 1 << 18
ENCODE_ROUTE_HC_PARSE_REC = 1 << 19
ENCODE_ROUTE_HC_PARSE_SEG2 = 1 << 20
ENCODE_ROUTE_HC_PARSE_SEG4 = 1 << 21
ENCODE_ROUTE_HC_PARSE_OPT = 1 << 22
ENCODE_ROUTE_QUEUE = 1 << 23
ENCODE_ROUTE_PERSISTENT = 1 << 24
ENCODE_ROUTE_PARSE_PACE = 1 << 25
ENCODE_ROUTE_PCOST_ORDER = 1 << 26
ENCODE_ROUTE_TWO_KERNELS = 1 << 27
ENCODE_ROUTE_MIGRATE = 1 << 28
ENCODE_ROUTE_CHUNKS = 1 << 29
ENCODE_ROUTE_NAMES = ("PARSE", "PARSE_BIG", "PARSE_SEG", "EMIT", "REST", "LDS", "MORE", "GTAB", "SEGMENTS", "PROF", "ALLOW_COPY", "PICKLE", "ENVELOPE", "HC_CHAIN_PART", "HC_CHAIN_LDS", "HC_CHAIN_MEM", "HC_CAND_LDS", "HC_CAND_MEM", "HC_PARSE", "HC_PARSE_REC", "HC_PARSE_SEG2", "HC_PARSE_SEG4", "HC_PARSE_OPT", "QUEUE", "PERSISTENT", "PARSE_PACE", "PCOST_ORDER", "TWO_KERNELS", "MIGRATE", "CHUNKS")      # bit i is ENCODE_ROUTE_<ENCODE_ROUTE_NAMES[i]>


def encode_route_names(route: int) -> str:
    """the bits of a k4lz4_last_encode_route value by name, for messages"""
    return "+".join(n.lower() for i, n in enumerate(ENCODE_ROUTE_NAMES) if route >> i & 1) or "none"

_u8p = C.c_void_p
_BATCH = [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
# k4lz4_frame_write_batch*: ctx, w, store, storeOff, src, srcOff, srcLen, dst, dstOff, dstCap, outLen
_FWRITE = [C.c_void_p, C.c_void_p, _u8p, C.c_void_p, _u8p, C.c_void_p, C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p]
_FREAD = [C.c_void_p] * 11
_LEGACY_ENC = [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, _u8p, C.c_void_p, C.c_void_p, C.c_void_p]

# every symbol include/k4lz4.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "k4lz4_version": (C.c_int, []),
    "k4lz4_device_count": (C.c_int, []),
    "k4lz4_recommended_min_batch": (C.c_int64, [C.c_int, C.c_int32, C.c_double]),
    "k4lz4_ctx_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "k4lz4_ctx_destroy": (None, [C.c_void_p]),
    "k4lz4_last_error": (C.c_char_p, [C.c_void_p]),
    "k4lz4_ctx_device": (C.c_int, [C.c_void_p]),
    "k4lz4_synchronize": (C.c_int, [C.c_void_p, C.c_void_p]),
    "k4lz4_ctx_reserve_hc": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    "k4lz4_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "k4lz4_host_unregister": (C.c_int, [C.c_void_p]),
    "k4lz4_selftest_chains": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_uint32)]),
    "k4lz4_last_decode_kernel": (C.c_int, [C.c_void_p]),
    "k4lz4_last_encode_route": (C.c_int, [C.c_void_p]),
    "k4lz4_set_enforce32": (None, [C.c_int]),
    "k4lz4_get_enforce32": (C.c_int, []),
    "k4lz4_compress_bound": (C.c_int, [C.c_int]),
    "k4lz4_last_status": (C.c_int, []),
    "k4lz4_compress_fast": (C.c_int, [_u8p, _u8p, C.c_int, C.c_int, C.c_int]),
    "k4lz4_compress_hc": (C.c_int, [_u8p, _u8p, C.c_int, C.c_int, C.c_int]),
    "k4lz4_decompress_safe": (C.c_int, [_u8p, _u8p, C.c_int, C.c_int]),
    "k4lz4_decompress_safe_partial": (C.c_int, [_u8p, _u8p, C.c_int, C.c_int]),
    "k4lz4_encode_batch": (C.c_int, _BATCH + [C.c_int, C.c_int]),
    "k4lz4_decompress_safe_using_dict": (C.c_int, [_u8p, _u8p, C.c_int, C.c_int, _u8p, C.c_int]),
    "k4lz4_decode_batch": (C.c_int, _BATCH + [C.c_int]),
    "k4lz4_decode_dict_batch": (C.c_int, _BATCH + [C.c_int, _u8p, C.c_void_p, C.c_void_p]),
    "k4lz4_decode_dict_batch_device": (C.c_int, _BATCH + [C.c_int, _u8p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "k4lz4_encode_batch_device": (C.c_int, _BATCH + [C.c_int, C.c_int, C.c_void_p]),
    "k4lz4_decode_batch_device": (C.c_int, _BATCH + [C.c_int, C.c_void_p]),
    "k4lz4_pickle_bound": (C.c_int, [C.c_int]),
    "k4lz4_unpickle_size": (C.c_int, [_u8p, C.c_int]),
    "k4lz4_pickle_batch": (C.c_int, _BATCH + [C.c_int, C.c_int]),
    "k4lz4_unpickle_batch": (C.c_int, _BATCH + [C.c_int]),
    "k4lz4_pickle_batch_device": (C.c_int, _BATCH + [C.c_int, C.c_int, C.c_void_p]),
    "k4lz4_unpickle_batch_device": (C.c_int, _BATCH + [C.c_int, C.c_void_p]),
    "k4lz4_profile_batch_device": (C.c_int, [C.c_void_p, C.c_int] + _BATCH[1:] + [C.c_void_p, C.c_void_p]),
    "k4lz4_xxh32_batch": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32]),
    "k4lz4_xxh32_batch_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p]),
    "k4lz4_decode_chain_batch": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "k4lz4_decode_chain_batch_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "k4lz4_frame_assemble_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, _u8p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _u8p, C.c_void_p, C.c_int64, C.c_void_p]),
    "k4lz4_unpickle_sizes_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "k4lz4_frame_sizes_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "k4lz4_decode_frames_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, _u8p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "k4lz4_frame_sizes": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "k4lz4_decode_frames": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, _u8p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "k4lz4_allow_copy_batch_device": (C.c_int, _BATCH + [C.c_void_p]),
    "k4lz4_frame_sizes_dictset_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "k4lz4_decode_frames_dictset_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, _u8p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "k4lz4_frame_sizes_dictset": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "k4lz4_decode_frames_dictset": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, _u8p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "k4lz4_encode_hc_chain_batch": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, _u8p,
                                              C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int]),
    "k4lz4_encode_hc_chain_batch_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, _u8p,
                                                     C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "k4lz4_encode_fast_chain_batch": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                C.c_void_p, C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    "k4lz4_encode_fast_chain_batch_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                       C.c_void_p, C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    # ... level, flags, dictIdx, dict, dictOff, dictLen, nDict [, stream]
    "k4lz4_encode_dict_batch": (C.c_int, _BATCH + [C.c_int, C.c_int, C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int32]),
    "k4lz4_encode_dict_batch_device": (C.c_int, _BATCH + [C.c_int, C.c_int, C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "k4lz4_encode_dict_state": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "k4lz4_encode_dict_hc_batch": (C.c_int, _BATCH + [C.c_int, C.c_int, C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int32]),
    "k4lz4_encode_dict_hc_batch_device": (C.c_int, _BATCH + [C.c_int, C.c_int, C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "k4lz4_encode_dict_hc_state": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # k4lz4_dict_set: ctx, dict, dictOff, dictLen, nDict, families, &set [, stream]
    "k4lz4_dict_set_create": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.POINTER(C.c_void_p)]),
    "k4lz4_dict_set_create_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    "k4lz4_dict_set_destroy": (None, [C.c_void_p]),
    "k4lz4_dict_set_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "k4lz4_dict_set_layout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "k4lz4_dict_set_state": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "k4lz4_dict_set_hc_state": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ... level, flags, dictIdx, set [, stream]
    "k4lz4_encode_dictset_batch": (C.c_int, _BATCH + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "k4lz4_encode_dictset_batch_device": (C.c_int, _BATCH + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ... flags, dictIdx, set [, stream]
    "k4lz4_decode_dictset_batch": (C.c_int, _BATCH + [C.c_int, C.c_void_p, C.c_void_p]),
    "k4lz4_decode_dictset_batch_device": (C.c_int, _BATCH + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "k4lz4_wrap_bound": (C.c_int, [C.c_int]),
    "k4lz4_wrap_batch": (C.c_int, _BATCH + [C.c_int, C.c_int]),
    "k4lz4_wrap_batch_device": (C.c_int, _BATCH + [C.c_int, C.c_int, C.c_void_p]),
    "k4lz4_unwrap_size": (C.c_int, [_u8p, C.c_int64]),
    "k4lz4_unwrap_sizes_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "k4lz4_unwrap_batch": (C.c_int, _BATCH[:8] + [C.c_void_p, C.c_int64]),
    "k4lz4_unwrap_batch_device": (C.c_int, _BATCH[:8] + [C.c_void_p, C.c_int64, C.c_void_p]),
    "k4lz4_legacy_stream_bound": (C.c_int64, [C.c_int64, C.c_int]),
    "k4lz4_encode_legacy_streams": (C.c_int, _LEGACY_ENC),
    "k4lz4_encode_legacy_streams_device": (C.c_int, _LEGACY_ENC + [C.c_void_p]),
    "k4lz4_legacy_stream_sizes": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "k4lz4_legacy_stream_sizes_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "k4lz4_decode_legacy_streams": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, _u8p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "k4lz4_decode_legacy_streams_device": (C.c_int, [C.c_void_p, _u8p, C.c_void_p, C.c_void_p, C.c_int64, _u8p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]),
    "k4lz4_frame_writer_init": (C.c_int, [C.c_void_p, C.c_void_p]),
    "k4lz4_frame_writer_store_bytes": (C.c_int64, [C.c_void_p]),
    "k4lz4_frame_write_bound": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int]),
    "k4lz4_frame_write_batch": (C.c_int, _FWRITE + [C.c_int64, C.c_int, C.c_int]),
    "k4lz4_frame_write_batch_device": (C.c_int, _FWRITE + [C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "k4lz4_frame_reader_init": (C.c_int, [C.c_void_p, C.c_void_p]),
    "k4lz4_frame_reader_store_bytes": (C.c_int64, [C.c_void_p]),
    "k4lz4_frame_read_batch": (C.c_int, _FREAD + [C.c_int64, C.c_int, C.c_int]),
    "k4lz4_frame_read_batch_device": (C.c_int, _FREAD + [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "k4lz4_frame_read_table_rows": (C.c_int64, [C.c_int64]),
    "k4lz4_frame_read_fed_batch": (C.c_int, [C.c_void_p] * 14 + [C.c_int64, C.c_int, C.c_int]),
    "k4lz4_frame_read_fed_batch_device": (C.c_int, [C.c_void_p] * 14 + [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    # ... set, dictIds [, stream]
    "k4lz4_frame_read_dictset_batch": (C.c_int, _FREAD + [C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "k4lz4_frame_read_dictset_batch_device": (C.c_int, _FREAD + [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "k4lz4_frame_read_fed_dictset_batch": (C.c_int, [C.c_void_p] * 14 + [C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "k4lz4_frame_read_fed_dictset_batch_device": (C.c_int, [C.c_void_p] * 14 + [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                                            C.c_void_p]),
    "k4lz4_frame_reader_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "k4lz4_frame_reader_query_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "k4lz4_legacy_writer_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "k4lz4_legacy_writer_store_bytes": (C.c_int64, [C.c_void_p]),
    "k4lz4_legacy_write_bound": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int]),
    "k4lz4_legacy_write_batch": (C.c_int, _FWRITE + [C.c_int64, C.c_int, C.c_int]),
    "k4lz4_legacy_write_batch_device": (C.c_int, _FWRITE + [C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "k4lz4_legacy_reader_init": (C.c_int, [C.c_void_p, C.c_int]),
    "k4lz4_legacy_reader_store_bytes": (C.c_int64, [C.c_void_p]),
    "k4lz4_legacy_read_table_rows": (C.c_int64, [C.c_void_p, C.c_int64]),
    "k4lz4_legacy_read_batch": (C.c_int, _FREAD + [C.c_int64, C.c_int, C.c_int]),
    "k4lz4_legacy_read_batch_device": (C.c_int, _FREAD + [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "k4lz4_legacy_reader_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "k4lz4_legacy_reader_query_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "k4lz4_legacy_reader_init_fed": (C.c_int, [C.c_void_p, C.c_int]),
    "k4lz4_legacy_read_fed_batch": (C.c_int, [C.c_void_p] * 14 + [C.c_int64, C.c_int, C.c_int]),
    "k4lz4_legacy_read_fed_batch_device": (C.c_int, [C.c_void_p] * 14 + [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "k4lz4_chain_decoder_init": (C.c_int, [C.c_void_p, C.c_void_p]),
    "k4lz4_chain_decoder_store_bytes": (C.c_int64, [C.c_void_p]),
    # ctx, dec, store, storeOff, src, recOff, recLen, recBlockSize, [nRecords,] firstRec, nRec, dst, dstOff, dstCap, recOut, outLen
    "k4lz4_chain_decode_batch": (C.c_int, [C.c_void_p] * 8 + [C.c_int64] + [C.c_void_p] * 7 + [C.c_int64, C.c_int, C.c_int]),
    "k4lz4_chain_decode_batch_device": (C.c_int, [C.c_void_p] * 15 + [C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "k4lz4_chain_drain_batch": (C.c_int, [C.c_void_p] * 8 + [C.c_int64]),
    "k4lz4_chain_drain_batch_device": (C.c_int, [C.c_void_p] * 8 + [C.c_int64, C.c_void_p]),
    "k4lz4_chain_decoder_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "k4lz4_chain_decoder_query_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "k4lz4_chain_encoder_init": (C.c_int, [C.c_void_p, C.c_void_p]),
    "k4lz4_chain_encoder_store_bytes": (C.c_int64, [C.c_void_p]),
    "k4lz4_chain_encode_bound": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "k4lz4_chain_encode_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "k4lz4_chain_encode_blocks": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "k4lz4_chain_table_rows": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "k4lz4_chain_encode_batch": (C.c_int, [C.c_void_p] * 8 + [C.c_int64] + [C.c_void_p] * 8 + [C.c_int64, C.c_int, C.c_int]),
    "k4lz4_chain_encode_batch_device": (C.c_int, [C.c_void_p] * 8 + [C.c_int64] + [C.c_void_p] * 8 + [C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    # open from a k4lz4_dict_set: ctx, enc | dec, store, storeOff, dictIdx, set, [outLen,] n [, stream]
    "k4lz4_chain_encoder_open_plan": (C.c_int, [C.c_void_p, C.c_int32]),
    "k4lz4_chain_encoder_open_dictset": (C.c_int, [C.c_void_p] * 6 + [C.c_int64]),
    "k4lz4_chain_encoder_open_dictset_device": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_void_p]),
    "k4lz4_chain_decoder_open_dictset": (C.c_int, [C.c_void_p] * 7 + [C.c_int64]),
    "k4lz4_chain_decoder_open_dictset_device": (C.c_int, [C.c_void_p] * 7 + [C.c_int64, C.c_void_p]),
}


class NativeLibraryError(RuntimeError):
    """libk4lz4.so is missing / unusable, or a HIP call failed."""


_lib = None
_lib_lock = threading.Lock()


def _share_hip_runtime():
    """PyTorch-ROCm wheels carry their own libamdhip64.so.  Two HIP runtimes in one process do not both
    see the GPU, and which one a process gets would depend on whether torch or libk4lz4 was imported
    first.  Map torch's copy (if there is one) before libk4lz4.so so that its NEEDED libamdhip64.so.7
    binds to it, and a later `import torch` finds the same runtime.  No torch import, no GPU touch."""
    import importlib.util
    if any("libamdhip64" in line for line in _mapped_objects()):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass        # fall back to the system runtime named by libk4lz4.so's RUNPATH


def _mapped_objects():
    try:
        with open("/proc/self/maps") as f:
            return f.readlines()
    except OSError:
        return []


def load_library(path: str | None = None):
    """dlopen libk4lz4.so and type every declared symbol.  Does not touch the GPU."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise NativeLibraryError(
                f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        _share_hip_runtime()
        lib = C.CDLL(p)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)   # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        if path is None:
            _lib = lib
        return lib


class Context:
    """k4lz4_ctx: one per GPU per host thread."""

    def __init__(self, device: int = -1):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.k4lz4_ctx_create(C.byref(h), device)
        if rc != K4LZ4_OK:
            msg = (self.lib.k4lz4_last_error(None) or b"").decode()
            raise NativeLibraryError(f"k4lz4_ctx_create failed ({rc}): {msg}")
        self.handle = h

    @property
    def device(self) -> int:
        return self.lib.k4lz4_ctx_device(self.handle)

    def check(self, rc: int):
        if rc == K4LZ4_OK:
            return
        msg = (self.lib.k4lz4_last_error(self.handle) or b"").decode()
        if rc == E_ARG:
            raise ValueError(msg)
        if rc == E_UNSUPPORTED:
            raise NotImplementedError(msg)
        if rc == E_NOMEM:
            raise MemoryError(msg)
        raise NativeLibraryError(f"libk4lz4 error {rc}: {msg}")

    def synchronize(self, stream: int = 0):
        self.check(self.lib.k4lz4_synchronize(self.handle, C.c_void_p(stream)))

    def last_decode_kernel(self) -> int:
        """DECODE_KERNEL_* of this context's most recent decode / unpickle launch, DECODE_KERNEL_PACE or-ed in (a diagnostic)"""
        return int(self.lib.k4lz4_last_decode_kernel(self.handle))

    def last_encode_route(self) -> int:
        """ENCODE_ROUTE_* bits of this context's most recent encode / pickle / wrap call: the kernel families it launched and a few
        facts about the launches, or-ed over its launch chunks (a diagnostic)"""
        return int(self.lib.k4lz4_last_encode_route(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.k4lz4_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_tls = threading.local()


def default_context() -> Context:
    """Per-thread context on the current device (LOCAL_RANK when launched by torch.distributed.run)."""
    ctx = getattr(_tls, "ctx", None)
    if ctx is None:
        dev = -1
        if "LOCAL_RANK" in os.environ:
            lib = load_library()
            n = lib.k4lz4_device_count()
            if n > 0:
                dev = int(os.environ["LOCAL_RANK"]) % n
        ctx = Context(dev)
        _tls.ctx = ctx
    return ctx


def _check_plain(lib, rc: int):
    if rc == K4LZ4_OK:
        return
    msg = (lib.k4lz4_last_error(None) or b"").decode()
    if rc == E_ARG:
        raise ValueError(msg)
    if rc == E_NOMEM:
        raise MemoryError(msg)
    raise NativeLibraryError(f"libk4lz4 error {rc}: {msg}")


def host_register(arr) -> None:
    """k4lz4_host_register: page-lock a (C-contiguous) numpy buffer that is reused across host-pointer batch calls, so that
    its bytes move between the caller's pages and the GPU without the stop in a staging buffer."""
    lib = load_library()
    _check_plain(lib, lib.k4lz4_host_register(C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes)))


def host_unregister(arr) -> None:
    lib = load_library()
    _check_plain(lib, lib.k4lz4_host_unregister(C.c_void_p(arr.ctypes.data)))


def check_last_status(lib):
    """raise if the thread's last LLxx-shaped call failed for an infrastructure reason"""
    rc = lib.k4lz4_last_status()
    if rc == K4LZ4_OK:
        return
    msg = (lib.k4lz4_last_error(None) or b"").decode()
    if rc == E_ARG:
        raise ValueError(msg)
    if rc == E_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == E_NOMEM:
        raise MemoryError(msg)
    raise NativeLibraryError(f"libk4lz4 error {rc}: {msg}")
