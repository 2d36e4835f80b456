/*
 * k4lz4.h -- C ABI of libk4lz4.so: the MI355X (gfx950) LZ4 block codec that sits behind the
 * K4os.Compression.LZ4 block API.  Plain pointers and sizes only; no HIP or torch types.
 *
 * Every entry point names the reference interface (paths relative to the reference repository,
 * src/K4os.Compression.LZ4/...) it replaces.  INTEGRATION.md shows the C# P/Invoke stubs and
 * the `Algorithm.Native` arm a maintainer would add to Engine/LLxx.cs.
 *
 * Conventions
 *   - All block lengths are `int32_t` like the reference (`int`), offsets into batch buffers are
 *     `uint64_t`.  Input size limit: 0x7E000000 (Engine/LL.types.cs:19).
 *   - Per-block results in `outLen[i]` follow LZ4Codec (LZ4Codec.cs:40-52, :104-115):
 *       > 0 bytes written, 0 for an empty input, -1 on failure (output too small / corrupt input).
 *     With K4LZ4_FLAG_RAW_RETURN they are the LLxx-level returns instead (Engine/LLxx.cs:17-26,
 *     :65-75): bytes written, 0 = did not fit, decode error = -(input position) - 1.
 *   - Bytes of dst[i] beyond outLen[i] are never modified on success
 *     (src/K4os.Compression.LZ4.Tests/SpanTests.cs:36-44) -- by the block encoders and the decoders.  Two deliberate exceptions,
 *     both stated where they apply and both confined to the slot: the pickle and wrap calls encode in place inside the
 *     envelope's slot (see k4lz4_pickle_batch, k4lz4_wrap_batch), and K4LZ4_FLAG_SEGMENTS.  On failure (an encode, pickle or wrap whose output did not fit
 *     dstCap[i]) nothing outside dst + dstOff[i] .. + dstCap[i] is written, and the slot's own bytes are then undefined;
 *     K4LZ4_FLAG_SEGMENTS may write anywhere inside the slot before outLen is final.
 *   - Call-level return: K4LZ4_OK or a negative k4lz4_status; text via k4lz4_last_error().
 *     The library never throws, aborts or calls back.  No pointer is retained after return
 *     (the *_device calls return after enqueueing on the given stream; the buffers must stay
 *     valid until that stream work completes).  A host-pointer call that fails part-way drains the work
 *     it queued and clears the context's status word before it returns, so the next call starts clean.
 *   - There is NO CPU fallback: without a usable gfx950 device every compute entry point fails
 *     with K4LZ4_E_NO_DEVICE.
 *   - A k4lz4_ctx is bound to one GPU and may be used by one host thread at a time; different
 *     contexts are independent (reentrant like the reference's static API).  The context owns device
 *     scratch (dispatch order, hash tables, HC work areas) that every call reuses: calls on ONE context
 *     are therefore serialised on the device even when they are given different streams (the second
 *     call's stream waits for the first call's work); use one context per stream for concurrency.
 *   - Trouble that is not a property of a block's data (a decoder wave pair timing out on its partner,
 *     an HC scratch reservation that was too small) is never reported through outLen alone: the blocks
 *     concerned say "failed" AND the next synchronising call on the context (every host-pointer call,
 *     k4lz4_synchronize) returns K4LZ4_E_HIP / K4LZ4_E_NOMEM with the reason(s) in k4lz4_last_error().
 *     The report is kept per CONTEXT (a word of device memory the context owns and hands to its kernels):
 *     contexts that share a device -- one per managed thread in the .NET shim -- never see or clear each
 *     other's.  This holds for pickles too: an HC pickle that was not encoded for want of reserved scratch
 *     has outLen = -1, never a valid raw envelope.
 */
#ifndef K4LZ4_H
#define K4LZ4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define K4LZ4_API __attribute__((visibility("default")))
#define K4LZ4_VERSION 100 /* 0.1.0 */

typedef struct k4lz4_ctx k4lz4_ctx;

enum k4lz4_status {
    K4LZ4_OK = 0,
    K4LZ4_E_HIP = -1,         /* HIP runtime error, see k4lz4_last_error */
    K4LZ4_E_ARG = -2,         /* NULL pointer / negative count (the C# shim raises ArgumentException) */
    K4LZ4_E_NOMEM = -3,
    K4LZ4_E_NO_DEVICE = -4,   /* no gfx950 device visible */
    K4LZ4_E_UNSUPPORTED = -5  /* reserved: every LZ4Level is implemented (levels above L12_MAX behave as L12_MAX, LL64.high.cs:1160) */
};

/* LZ4Level.cs:6-39 -- the numeric value is part of the ABI */
enum k4lz4_level {
    K4LZ4_L00_FAST = 0,
    K4LZ4_L03_HC = 3, K4LZ4_L04_HC = 4, K4LZ4_L05_HC = 5, K4LZ4_L06_HC = 6, K4LZ4_L07_HC = 7,
    K4LZ4_L08_HC = 8, K4LZ4_L09_HC = 9, K4LZ4_L10_OPT = 10, K4LZ4_L11_OPT = 11, K4LZ4_L12_MAX = 12
};

enum k4lz4_flags {
    K4LZ4_FLAG_RAW_RETURN = 1,    /* outLen = LLxx-level return values */
    K4LZ4_FLAG_PICKLE_WRITER = 2, /* LZ4Pickler IBufferWriter path header rule (LZ4Pickler.pickle.cs:113-158) */
    K4LZ4_FLAG_NO_REORDER = 4,    /* encode/pickle/unpickle: dispatch blocks in index order instead of most-expensive-first */
    K4LZ4_FLAG_REORDER = 8,       /* decode: dispatch longest inputs first (useful for ragged batches; unpickle does it by default) */
    K4LZ4_FLAG_NO_SPLIT = 16,     /* encode: do not run part of the batch on the global-memory-table kernel */
    K4LZ4_FLAG_ALLOW_COPY = 64,   /* encode: LZ4EncoderBase.Encode(allowCopy) -- a block that does not shrink is stored raw, outLen = -srcLen;
                                     outLen = 0 where the reference throws "target buffer too small" (Encoders/LZ4EncoderBase.cs:66-88) */
    K4LZ4_FLAG_X32 = 128,         /* fast encode / pickle: the 32-bit engine's bytes (LZ4Codec.Enforce32, LZ4Codec.cs:14-25): inputs of
                                     64 KiB and more are hashed with LZ4_hash4 instead of LZ4_hash5 (x32/LL32.tools.cs:141-148) */
    K4LZ4_FLAG_PARTIAL = 32,      /* decode: LZ4Codec.PartialDecode -- stop once dstCap[i] bytes are produced (LZ4Codec.cs:123-173) */
    K4LZ4_FLAG_SEGMENTS = 256     /* fast encode: blocks of 1.5 MiB and more that are also a large share of the batch may be encoded by several
                                     wavefronts (segments whose joints are verified; a block that does not verify is encoded again by one), see
                                     DESIGN.md 4.6 -- same bytes, a 4 MiB block in 50 ms instead of 165; needs dstCap[i] >= srcLen[i] - 1 and
                                     may write anywhere inside a block's slot before outLen is final.  The pickle calls do this by themselves. */
};

K4LZ4_API int k4lz4_version(void);
K4LZ4_API int k4lz4_device_count(void);

/* Below which batch size a caller should stay on the managed engine (LZ4Codec.cs:40-52 -> LLxx -> LL64 on the host).
 * One wavefront encodes a 64 KiB block in about 2 ms and decodes it in 0.6 ms however small the batch is (the chip is fast
 * because it runs thousands of blocks side by side, not because a block is fast), so a device call has a floor; a host that
 * sustains `hostGiBs` on this work beats it below
 *     floor(kind, blockBytes) * hostGiBs / blockBytes   blocks.
 * kind: 0 fast-level encode, 1 decode, 2 HC encode (level 3); blockBytes: uncompressed bytes per block;
 * hostGiBs: what the caller's host threads sustain together on such blocks (the reference's engine, measured on the 256-thread
 * host of the MI355X box: 0.8 GiB/s encode / 4 GiB/s decode per thread, 32 / 35 GiB/s with all threads); <= 0: those box figures.
 * For data that starts and ends in host memory use the host-pointer rate (about 22 GiB/s encode, 28-37 decode) as the device's
 * ceiling as well: a host faster than that never gains.  Returns the number of blocks (>= 1), or a negative error. */
K4LZ4_API int64_t k4lz4_recommended_min_batch(int kind, int32_t blockBytes, double hostGiBs);

/* device < 0: the calling thread's current HIP device */
K4LZ4_API int k4lz4_ctx_create(k4lz4_ctx **out, int device);
K4LZ4_API void k4lz4_ctx_destroy(k4lz4_ctx *ctx);
/* ctx may be NULL: last error of the calling thread's implicit context / of ctx creation */
K4LZ4_API const char *k4lz4_last_error(const k4lz4_ctx *ctx);
K4LZ4_API int k4lz4_ctx_device(const k4lz4_ctx *ctx);
/* blocks until everything this ctx enqueued on `stream` (NULL = default stream) has finished; returns the call-level
 * status of that work (see "Trouble that is not a property of a block's data" above) */
K4LZ4_API int k4lz4_synchronize(k4lz4_ctx *ctx, void *stream);
/* HC levels (L03_HC and up) need work areas proportional to the batch: 20 bytes per input byte (36 before round 6).  A device-resident call
 * does not know its batch's size on the host, so by default it reads it back -- ONE synchronisation per 4096 blocks.
 * After this call, device-resident HC encodes / pickles on ctx whose blocks total at most totalSrcBytes (per call) and are
 * at most longestBlock bytes each only enqueue, like every other *_device call; a batch that exceeds the reservation is
 * not encoded (outLen = failure, K4LZ4_E_NOMEM at the next synchronising call).  (0, 0) removes the reservation. */
K4LZ4_API int k4lz4_ctx_reserve_hc(k4lz4_ctx *ctx, int64_t totalSrcBytes, int32_t longestBlock);
/* Page-locks [ptr, ptr + bytes) of the caller's memory (hipHostRegister) and remembers the range: host-pointer batch calls
 * whose source span, or whose destination slots, lie inside a registered range move those bytes straight between the
 * caller's pages and the GPU instead of through the context's pinned staging buffers (no counterpart in the reference; a
 * .NET caller registers a pinned array / NativeMemory block it reuses across calls).  Results are the same byte for byte:
 * exactly outLen[i] bytes are written to slot i either way.  Registering costs about as much as the copy it saves, so it
 * pays for buffers that are used more than once.  The range must stay registered until every call that uses it has
 * returned; unregister with the same ptr.  Process-wide, any thread. */
K4LZ4_API int k4lz4_host_register(void *ptr, size_t bytes);
K4LZ4_API int k4lz4_host_unregister(void *ptr);
/* Diagnostic, no counterpart in the reference: the three serial chains of the kernels exist as hand-written scalar ISA and
 * as C (the form the CPU wave emulator of the test suite runs).  Runs both forms on the device over `waves` x `rounds`
 * pseudo-random well-formed inputs; mismatches[0..2] = rounds in which they disagreed (token chain of the decoder, hop
 * chain of the fast encoder, its variant with pair fall-backs).  All zero on a healthy build. */
K4LZ4_API int k4lz4_selftest_chains(k4lz4_ctx *ctx, int waves, int rounds, uint32_t seed, uint32_t mismatches[3]);
/* Diagnostic, no counterpart in the reference: which decoder kernel the most recent decode or unpickle launch of ctx used (the
 * launcher chooses by blocks per CU; a call of more blocks than one launch takes reports its last launch), with
 * K4LZ4_DECODE_KERNEL_PACE or-ed in when that launch ran with the late-blocks-first priorities.  K4LZ4_DECODE_KERNEL_NONE before
 * the first such launch (also for a NULL ctx).  Recorded on the host when the launch is enqueued: it does not wait. */
enum k4lz4_decode_kernel {
    K4LZ4_DECODE_KERNEL_NONE = 0,
    K4LZ4_DECODE_KERNEL_PAIR2 = 1,          /* k4_decode_pair2_kernel: two waves per block, the token chain two links per hop */
    K4LZ4_DECODE_KERNEL_PAIR = 2,           /* k4_decode_pair_kernel: two waves per block, one link per hop */
    K4LZ4_DECODE_KERNEL_SINGLE = 3,         /* k4_decode_kernel: one wave per block */
    K4LZ4_DECODE_KERNEL_DENSE = 4,          /* k4_decode_dense_kernel: one wave per block, seven waves per SIMD */
    K4LZ4_DECODE_KERNEL_PROF = 5,           /* an instrumented twin (k4lz4_profile_batch_device) */
    K4LZ4_DECODE_KERNEL_UNPICKLE_PAIR2 = 9, /* k4_unpickle_pair2_kernel */
    K4LZ4_DECODE_KERNEL_UNPICKLE_PAIR = 10, /* k4_unpickle_pair_kernel */
    K4LZ4_DECODE_KERNEL_UNPICKLE_SINGLE = 11, /* k4_unpickle_kernel */
    K4LZ4_DECODE_KERNEL_PACE = 64           /* flag: a.pace was armed for the launch */
};
K4LZ4_API int k4lz4_last_decode_kernel(const k4lz4_ctx *ctx);
/* Diagnostic, no counterpart in the reference: the route ctx's most recent encode, pickle or wrap call took through the batch
 * launcher, as a set of bits -- one per kernel family the call launched, and a few facts about the launches that bytes cannot
 * show.  Every bit is stored on the host at the line that issues the launch, or-ed over the call's launch chunks, and cleared
 * when the next encode, pickle or wrap call enters the launcher (a decode leaves it alone; a chained HC encode, which shares
 * the HC launcher, clears it too and reports its own HC bits).  K4LZ4_ENCODE_ROUTE_NONE before the first such call (also for a
 * NULL ctx).  It does not wait, and no kernel, grid or scratch depends on it. */
enum k4lz4_encode_route {
    K4LZ4_ENCODE_ROUTE_NONE = 0,
    /* fast levels, the two-step encoder (k4lz4_parse.hpp) */
    K4LZ4_ENCODE_ROUTE_PARSE = 1 << 0,         /* k4_parse_kernel */
    K4LZ4_ENCODE_ROUTE_PARSE_BIG = 1 << 1,     /* k4_parse_big_kernel: blocks of 65 547 bytes and more */
    K4LZ4_ENCODE_ROUTE_PARSE_SEG = 1 << 2,     /* k4_parse_seg_kernel: ragged batches, the big blocks and the later segments */
    K4LZ4_ENCODE_ROUTE_EMIT = 1 << 3,          /* k4_emit_kernel (K4LZ4_NO_INLINE_EMIT) */
    K4LZ4_ENCODE_ROUTE_REST = 1 << 4,          /* k4_encode_fast_rest_kernel: the blocks the parse left alone */
    /* fast levels, the one-kernel encoders (k4lz4_encode_fast.hpp) */
    K4LZ4_ENCODE_ROUTE_LDS = 1 << 5,           /* k4_encode_fast_kernel, or its twin k4_encode_fast_seg_kernel (then with _SEGMENTS) */
    K4LZ4_ENCODE_ROUTE_MORE = 1 << 6,          /* k4_encode_fast_more_kernel: at most 8 blocks per CU */
    K4LZ4_ENCODE_ROUTE_GTAB = 1 << 7,          /* k4_encode_fast_gtab_kernel beside the LDS-table kernel, or its *_seg twin */
    K4LZ4_ENCODE_ROUTE_SEGMENTS = 1 << 8,      /* blocks cut into segments: k4_encode_seg_kernel and the *_seg twins, and the join */
    K4LZ4_ENCODE_ROUTE_PROF = 1 << 9,          /* k4_encode_fast_prof_kernel (k4lz4_profile_batch_device, decode = 0) */
    K4LZ4_ENCODE_ROUTE_ALLOW_COPY = 1 << 10,   /* k4_allow_copy_kernel behind the encoders (K4LZ4_FLAG_ALLOW_COPY) */
    K4LZ4_ENCODE_ROUTE_PICKLE = 1 << 11,       /* k4_pickle_kernel: a small batch of pickles by one kernel */
    K4LZ4_ENCODE_ROUTE_ENVELOPE = 1 << 12,     /* pickles and wraps through the encoders: the prep and finish kernels around them */
    /* HC levels (k4lz4_encode_hc.hpp) */
    K4LZ4_ENCODE_ROUTE_HC_CHAIN_PART = 1 << 13, /* k4_hc_chain_part_kernel */
    K4LZ4_ENCODE_ROUTE_HC_CHAIN_LDS = 1 << 14,  /* k4_hc_chain_lds_kernel (K4LZ4_HC_CHAIN_OLD) */
    K4LZ4_ENCODE_ROUTE_HC_CHAIN_MEM = 1 << 15,  /* k4_hc_chain_kernel: tables in memory */
    K4LZ4_ENCODE_ROUTE_HC_CAND_LDS = 1 << 16,   /* k4_hc_walk_lds_kernel + k4_hc_cand_lds_kernel */
    K4LZ4_ENCODE_ROUTE_HC_CAND_MEM = 1 << 17,   /* k4_hc_cand_kernel (K4LZ4_HC_CAND_MEM, blocks over 64 KiB) */
    K4LZ4_ENCODE_ROUTE_HC_PARSE = 1 << 18,      /* k4_hc_parse_kernel */
    K4LZ4_ENCODE_ROUTE_HC_PARSE_REC = 1 << 19,  /* k4_hc_parse_rec_kernel: level 3, one wave per block */
    K4LZ4_ENCODE_ROUTE_HC_PARSE_SEG2 = 1 << 20, /* k4_hc_parse_seg2_kernel: two waves per block */
    K4LZ4_ENCODE_ROUTE_HC_PARSE_SEG4 = 1 << 21, /* k4_hc_parse_seg4_kernel: four waves per block */
    K4LZ4_ENCODE_ROUTE_HC_PARSE_OPT = 1 << 22,  /* k4_hc_parse_opt_kernel: levels 10 and up */
    /* facts about the fast-level launches */
    K4LZ4_ENCODE_ROUTE_QUEUE = 1 << 23,        /* k4_parse_kernel's waves took their blocks from the queue */
    K4LZ4_ENCODE_ROUTE_PERSISTENT = 1 << 24,   /* ... in one persistent launch for a batch beyond one residency */
    K4LZ4_ENCODE_ROUTE_PARSE_PACE = 1 << 25,   /* k4_parse_kernel ran with the late-blocks-first priorities */
    K4LZ4_ENCODE_ROUTE_PCOST_ORDER = 1 << 26,  /* the dispatch order came from the parse's own cost estimate */
    K4LZ4_ENCODE_ROUTE_TWO_KERNELS = 1 << 27,  /* the order was split between the two one-kernel encoders on the device */
    K4LZ4_ENCODE_ROUTE_MIGRATE = 1 << 28,      /* k4_parse_kernel's blocks may move into an LDS table that became free */
    K4LZ4_ENCODE_ROUTE_CHUNKS = 1 << 29        /* the call took more than one launch chunk */
};
K4LZ4_API int k4lz4_last_encode_route(const k4lz4_ctx *ctx);

/* LZ4Codec.MaximumOutputSize (LZ4Codec.cs:30-31) == LL.LZ4_compressBound (Engine/LL.tools.cs:38-40).
 * Pure host arithmetic. */
/* LZ4Codec.Enforce32 (process-wide, like LL.Enforce32): every fast-level encode and pickle behaves as with K4LZ4_FLAG_X32 */
K4LZ4_API void k4lz4_set_enforce32(int on);
K4LZ4_API int k4lz4_get_enforce32(void);
K4LZ4_API int k4lz4_compress_bound(int n);

/* ---- per-block entry points: the Engine/LLxx.cs seam, same argument order and returns ------
 * (host pointers; each call is a batch of one on the calling thread's implicit context) */
/* These mirror the reference's `int` returns, which cannot carry an infrastructure failure (no
 * GPU, HIP error, unsupported level): such a failure returns 0 (encode) / -1 (decode) and sets the
 * thread's status, which the host shim must check: K4LZ4_OK or a negative k4lz4_status. */
K4LZ4_API int k4lz4_last_status(void);
/* LLxx.LZ4_compress_fast (Engine/LLxx.cs:65-75) */
K4LZ4_API int k4lz4_compress_fast(const uint8_t *src, uint8_t *dst, int srcLen, int dstCap, int acceleration);
/* LLxx.LZ4_compress_HC (Engine/LLxx.cs:94-103); level >= K4LZ4_L03_HC (LZ4Level has nothing between FAST and L03_HC, and
 * LZ4Codec routes lower values to the fast encoder, LZ4Codec.cs:48-50): lower values fail with K4LZ4_E_ARG */
K4LZ4_API int k4lz4_compress_hc(const uint8_t *src, uint8_t *dst, int srcLen, int dstCap, int level);
/* LLxx.LZ4_decompress_safe (Engine/LLxx.cs:17-26) */
K4LZ4_API int k4lz4_decompress_safe(const uint8_t *src, uint8_t *dst, int srcLen, int dstCap);
/* LLxx.LZ4_decompress_safe_partial (Engine/LLxx.cs:29-39): decoding stops at targetLen bytes */
K4LZ4_API int k4lz4_decompress_safe_partial(const uint8_t *src, uint8_t *dst, int srcLen, int targetLen);
/* LLxx.LZ4_decompress_safe_usingDict (Engine/LLxx.cs:41-55; LL64.dec.cs:523-546) behind
 * LZ4Codec.Decode(source, target, dictionary) (LZ4Codec.cs:144-160).  A dictionary that ends exactly at dst is
 * decoded with the reference's prefix semantics, any other one with its external-dictionary semantics. */
K4LZ4_API int k4lz4_decompress_safe_using_dict(const uint8_t *src, uint8_t *dst, int srcLen, int dstCap,
                                               const uint8_t *dict, int dictLen);

/* ---- batches of independent blocks (what LZ4Codec.Encode / Decode callers loop over) --------
 * block i: input  src + srcOff[i], srcLen[i] bytes;  output dst + dstOff[i], dstCap[i] bytes.
 * Host variants take host pointers and stage through the GPU; they return when done.      */
K4LZ4_API int k4lz4_encode_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                 uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen,
                                 int64_t n, int level, int flags);
K4LZ4_API int k4lz4_decode_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                 uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen,
                                 int64_t n, int flags);

/* Device-resident variants: every pointer (including srcOff/srcLen/dstOff/dstCap/outLen) is a
 * device pointer on ctx's GPU; `stream` is a hipStream_t (NULL = default stream).  Asynchronous. */
K4LZ4_API int k4lz4_encode_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff,
                                        const int32_t *srcLen, uint8_t *dst, const uint64_t *dstOff,
                                        const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags,
                                        void *stream);
K4LZ4_API int k4lz4_decode_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff,
                                        const int32_t *srcLen, uint8_t *dst, const uint64_t *dstOff,
                                        const int32_t *dstCap, int32_t *outLen, int64_t n, int flags, void *stream);

/* Batched LZ4Codec.Decode(source, target, dictionary): block i is decoded against
 * dict[dictOff[i] .. dictOff[i]+dictLen[i]) (dictLen[i] <= 0: no dictionary).  Chained blocks of one
 * stream (LZ4ChainDecoder's layout: each block's dictionary is the previous 64 KiB of output) are NOT a
 * batch -- they depend on each other; independent streams each holding a dictionary are. */
K4LZ4_API int k4lz4_decode_dict_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                      uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen,
                                      int64_t n, int flags, const uint8_t *dict, const uint64_t *dictOff,
                                      const int32_t *dictLen);
K4LZ4_API int k4lz4_decode_dict_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff,
                                             const int32_t *srcLen, uint8_t *dst, const uint64_t *dstOff,
                                             const int32_t *dstCap, int32_t *outLen, int64_t n, int flags,
                                             const uint8_t *dict, const uint64_t *dictOff, const int32_t *dictLen,
                                             void *stream);

/* ---- LZ4Pickler envelope, version 0 (LZ4Pickler.pickle.cs:51-228, LZ4Pickler.unpickle.cs:18-158)
 * pickle:   outLen[i] = envelope bytes written to dst + dstOff[i]; dstCap[i] must be at least
 *           k4lz4_pickle_bound(srcLen[i]); 0 for an empty message (Pickle returns an empty array).
 * unpickle: dstCap[i] must equal the size k4lz4_unpickle_size reports (the reference allocates
 *           exactly that); outLen[i] = that size, or -1 where the reference throws
 *           InvalidDataException (bad version, short header, size mismatch, corrupt block).
 * A deliberate deviation from "bytes beyond outLen are never modified on success": there is no scratch buffer, the block
 * encoder works in place inside the envelope's slot (at +5, capacity srcLen - 1) and the envelope is closed around its bytes
 * afterwards (the reference encodes into a rented buffer and copies).  So behind a pickle's outLen[i] bytes the slot may hold
 * what the encoder wrote: the last 4 - sizeOfDiff bytes of a block that was moved down to its header; up to 4 + srcLen[i] where
 * the block did not shrink (a raw envelope of 1 + srcLen[i] bytes) or the message was cut into segments.  Nothing beyond
 * 4 + srcLen[i], and nothing outside the slot where dstCap[i] is too small (outLen[i] = -1).  A caller that needs the slack
 * untouched sizes the slot by outLen after the call, as LZ4Pickler.Pickle's callers receive an array of exactly that size.  */
K4LZ4_API int k4lz4_pickle_bound(int srcLen);
/* host arithmetic on one envelope: unpickled size, or -1 when the header is corrupt */
K4LZ4_API int k4lz4_unpickle_size(const uint8_t *pickle, int pickleLen);
K4LZ4_API int k4lz4_pickle_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                 uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen,
                                 int64_t n, int level, int flags);
K4LZ4_API int k4lz4_unpickle_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                   uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen,
                                   int64_t n, int flags);
K4LZ4_API int k4lz4_pickle_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff,
                                        const int32_t *srcLen, uint8_t *dst, const uint64_t *dstOff,
                                        const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags,
                                        void *stream);
K4LZ4_API int k4lz4_unpickle_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff,
                                          const int32_t *srcLen, uint8_t *dst, const uint64_t *dstOff,
                                          const int32_t *dstCap, int32_t *outLen, int64_t n, int flags,
                                          void *stream);
/* device-side k4lz4_unpickle_size for a whole batch: outLen[i] = unpickled size or -1 */
K4LZ4_API int k4lz4_unpickle_sizes_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff,
                                          const int32_t *srcLen, int32_t *outLen, int64_t n, void *stream);

/* ---- diagnostics -----------------------------------------------------------------------------
 * Runs the encode (decode = 0, L00_FAST, blocks < 65547 B) or decode (decode = 1) kernel's
 * instrumented twin on a device-resident batch and fills `counters` (device pointer, 16 x uint64
 * per block): [0] total shader cycles, [1..3] cycles per phase (encode: probe / extend / emit;
 * decode: parse / literals / matches), [4..7] event counts, [8]/[9] start/end on the 100 MHz
 * real-time counter, [10] HW_ID of the executing wave.  Results in dst/outLen
 * are identical to the normal kernels; timing is perturbed (each phase drains its memory traffic).
 * decode = 4 (encode) / 5 (decode): the ORDINARY kernels run and only record, per block, [8] start and [9] end on the
 * real-time counter, [10] HW_ID and -- encode -- [11] which kernel took the block (1 LDS table, 2 global table, 3 the
 * 28-known-bytes variant; 4 / 5 / 6 the two-step encoder of k4lz4_parse.hpp: table in LDS, in memory, moved into LDS on the way):
 * when each block of a batch really starts and ends (scripts/stamp_probe.py).
 * NOTE: in a default build, decode = 0 (encode phases) instruments the ONE-KERNEL encoder of rounds 1-4, not the two-step encoder
 * that LZ4Codec.Encode batches ship through; its phase probe is a build with -DK4_PARSE_PROF (scripts/parse_probe.py). */
K4LZ4_API int k4lz4_profile_batch_device(k4lz4_ctx *ctx, int decode, const uint8_t *src, const uint64_t *srcOff,
                                         const int32_t *srcLen, uint8_t *dst, const uint64_t *dstOff,
                                         const int32_t *dstCap, int32_t *outLen, int64_t n, uint64_t *counters,
                                         void *stream);

/* ---- frame layer (K4os.Compression.LZ4.Streams: Frames/LZ4FrameWriter.cs, LZ4FrameReader.async.cs) ----------- */

/* XXH32.DigestOf for n buffers (K4os.Hash.xxHash 1.0.8, NuGet; call sites Frames/LZ4FrameWriter.cs:100,:162-182,
 * Internal/Stash.cs:149-150): out[i] = xxHash32(data[off[i] .. off[i]+len[i]), seed). */
K4LZ4_API int k4lz4_xxh32_batch(k4lz4_ctx *ctx, const uint8_t *data, const uint64_t *off, const uint64_t *len,
                                uint32_t *out, int64_t n, uint32_t seed);
K4LZ4_API int k4lz4_xxh32_batch_device(k4lz4_ctx *ctx, const uint8_t *data, const uint64_t *off, const uint64_t *len,
                                       uint32_t *out, int64_t n, uint32_t seed, void *stream);

/* Block streams decoded in order, one stream per wavefront: ILZ4Decoder.Decode / Inject over the blocks of a frame
 * (Frames/LZ4FrameReader.async.cs:108-136; Encoders/LZ4BlockDecoder.cs:39-71 for independent blocks,
 * Encoders/LZ4ChainDecoder.cs -> LL64.LZ4_decompress_safe_continue for chained ones).  Stream s owns blocks
 * firstBlk[s] .. firstBlk[s]+nBlk[s]-1; blkLen has bit 31 set for blocks stored raw (LZ4FrameWriter.cs:159-160).
 * outLen[s] = bytes produced, -6 when a block does not decode, -9 when dstCap[s] is too small. */
K4LZ4_API int k4lz4_decode_chain_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *blkOff, const uint32_t *blkLen,
                                       int64_t nBlocks, const uint64_t *firstBlk, const uint32_t *nBlk,
                                       const int32_t *blockSize, const uint8_t *chained, uint8_t *dst,
                                       const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen, int64_t nStreams);
K4LZ4_API int k4lz4_decode_chain_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *blkOff,
                                              const uint32_t *blkLen, const uint64_t *firstBlk, const uint32_t *nBlk,
                                              const int32_t *blockSize, const uint8_t *chained, uint8_t *dst,
                                              const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen,
                                              int64_t nStreams, void *stream);

/* Chained HC block streams: LZ4HighChainEncoder(level, blockSize, extraBlocks) (Encoders/LZ4HighChainEncoder.cs, LZ4EncoderBase.cs)
 * fed a whole content and flushed block by block -- LZ4_compress_HC_continue over the encoder's ring buffer, LZ4_saveDictHC when it
 * is full -- which is what LZ4Stream.Encode / LZ4Frame.Encode write at L03_HC .. L12_MAX with ChainBlocks = true (their default).
 * Many streams per call; the blocks of all of them are encoded side by side (a block needs the bytes before it, not
 * the parse of the block before it).  Stream s: content src + srcOff[s], srcLen[s] bytes; blockSize[s] is rounded up to a whole
 * KiB, at least 1 KiB (call it B); extraBlocks[s] as the encoder's constructor takes it (NULL: 0 for every stream; the frame
 * writer passes max(extraMemory > 0 ? blockSize : 0, extraMemory) / blockSize, Streams/Extensions.cs:18-19).  dictLen[s] (NULL:
 * 0): the stream continues an encoder whose ring buffer holds the content's first dictLen[s] bytes in front of the next block
 * (LZ4EncoderBase's buffer before _inputIndex, at most 65536 + (1 + extraBlocks) * B + 32 bytes): no block is written for them.
 * Stream s has ceil((srcLen[s] - dictLen[s]) / B) blocks; block j of it is written to dst + dstOff[s] + j * k4lz4_compress_bound(B), its result is
 * outLen[first(s) + j], where first(s) is the number of blocks of the streams before s (nBlocks: entries of outLen, at least
 * the total).  outLen: bytes written, or with K4LZ4_FLAG_ALLOW_COPY (LZ4EncoderBase.Encode(allowCopy)) -length for a block
 * stored raw.  level is clamped to 3..12 like the constructor does.  The only flag is K4LZ4_FLAG_ALLOW_COPY.  A stream whose
 * blocks reach 2 GB (LZ4_compressHC_continue_generic renormalises there) is refused with K4LZ4_E_ARG (counted from the content's
 * start: a caller that continues a longer stream through dictLen checks its own position).
 * _device: src, dst and outLen are device pointers; srcOff, srcLen, blockSize, extraBlocks and dstOff stay HOST arrays (the
 * block table is host index work, built inside the call).  Asynchronous on `stream` like the other *_device calls. */
K4LZ4_API int k4lz4_encode_hc_chain_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen,
                                          const int32_t *blockSize, const int32_t *extraBlocks, const int32_t *dictLen,
                                          int64_t nStreams, uint8_t *dst, const uint64_t *dstOff, int32_t *outLen, int64_t nBlocks,
                                          int level, int flags);
K4LZ4_API int k4lz4_encode_hc_chain_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen,
                                                 const int32_t *blockSize, const int32_t *extraBlocks, const int32_t *dictLen,
                                                 int64_t nStreams, uint8_t *dst, const uint64_t *dstOff, int32_t *outLen,
                                                 int64_t nBlocks, int level, int flags, void *stream);

/* Chained fast block streams: LZ4FastChainEncoder(blockSize, extraBlocks) (Encoders/LZ4FastChainEncoder.cs, LZ4EncoderBase.cs) fed
 * a whole content and flushed block by block -- LZ4_compress_fast_continue(acceleration 1) over the encoder's ring buffer,
 * LZ4_saveDict when it is full -- which is what LZ4Stream.Encode / LZ4Frame.Encode write below L03_HC with ChainBlocks = true.
 * The arguments are the HC pair's (above) without level.  A stream's table holds the positions its parse visited, so its blocks are
 * encoded in order by one wavefront; the streams run side by side.  The table is byU32 with hash5 for every block, so a
 * fresh stream's first block is not the independent L00_FAST encoder's bytes.
 * stateIn (NULL: every stream is fresh) / stateOut (NULL: not wanted): one k4lz4_fast_chain_state per stream, the stream context's
 * hash table and indices word for word (LZ4_stream_t's hashTable, currentOffset, dictSize) as they stand before the first / after
 * the last block of the call.  They are what lets an encoder continue a stream across calls: pass stateOut back as stateIn with the
 * ring buffer's bytes in front of the next content (dictLen[s] == stateIn[s].dictSize, else K4LZ4_E_ARG; without stateIn dictLen
 * must be 0).  The only flag is K4LZ4_FLAG_ALLOW_COPY; K4LZ4_FLAG_X32 and a process under k4lz4_set_enforce32(1) are refused with
 * K4LZ4_E_ARG (the 32-bit engine's chained encoder is not offered).  A block that would take currentOffset past 2 GB
 * (LZ4_renormDictT rescales the table there) is refused with K4LZ4_E_ARG.
 * _device: src, dst, outLen, stateIn and stateOut are device pointers; the per-stream arrays stay HOST arrays.  With stateIn the call
 * reads the states' two indices back to the host first (it waits for `stream` there), then runs asynchronously on it. */
typedef struct k4lz4_fast_chain_state {
    uint32_t hashTable[4096];
    uint32_t currentOffset;
    uint32_t dictSize;
    uint32_t reserved[2];
} k4lz4_fast_chain_state;
K4LZ4_API int k4lz4_encode_fast_chain_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen,
                                            const int32_t *blockSize, const int32_t *extraBlocks, const int32_t *dictLen,
                                            int64_t nStreams, const k4lz4_fast_chain_state *stateIn, k4lz4_fast_chain_state *stateOut,
                                            uint8_t *dst, const uint64_t *dstOff, int32_t *outLen, int64_t nBlocks, int flags);
K4LZ4_API int k4lz4_encode_fast_chain_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen,
                                                   const int32_t *blockSize, const int32_t *extraBlocks, const int32_t *dictLen,
                                                   int64_t nStreams, const k4lz4_fast_chain_state *stateIn,
                                                   k4lz4_fast_chain_state *stateOut, uint8_t *dst, const uint64_t *dstOff,
                                                   int32_t *outLen, int64_t nBlocks, int flags, void *stream);

/* Messages encoded against shared dictionaries, fast levels: the counterpart of k4lz4_decode_dict_batch.  Message i (srcLen[i]
 * bytes at src + srcOff[i]) is encoded against entry dictIdx[i] of a list of nDict dictionaries (dictLen[d] bytes at
 * dict + dictOff[d]) -- a list, not one dictionary per message, because the point is few dictionaries and many messages.  Block i is
 * byte for byte what LZ4_loadDict(stream, dictionary, dictLen) followed by LZ4_compress_fast_continue(stream, src, dst, srcLen,
 * dstCap, 1) writes (LL64.tools.cs:175-206, LL64.fast.cs:582-667: the usingExtDict arm, the dictionary does not lie in front of the
 * message), and decodes with k4lz4_decode_dict_batch given the same dictionary.  Only a dictionary's last 64 KiB count; one of fewer
 * than 8 bytes (dictLen 0 included) is valid and empty, as LZ4_loadDict has it.  The table of every distinct dictionary of the list
 * is built once per call (16 KiB each, in the context's scratch), then one wavefront encodes each message.
 * outLen[i] follows k4lz4_encode_batch: the bytes written, 0 for an empty message, -1 when the block does not fit dstCap[i]
 * (limitedOutput returns 0 there); bytes of dst behind outLen[i] are not touched (behind a -1 the slot's content is unspecified in
 * the _device form).
 * Refused with K4LZ4_E_ARG: level >= K4LZ4_L03_HC (the hash-chain levels are k4lz4_encode_dict_hc_batch's, below);
 * K4LZ4_FLAG_X32 or a process under k4lz4_set_enforce32(1) (LL32's LZ4_loadDict has a 4-byte HASH_UNIT and hash4: no
 * witness for it), and every other flag; a negative dictLen; a dictIdx outside [0, nDict).
 * _device: src, dst, outLen, dict and the per-message arrays (srcOff, srcLen, dstOff, dstCap, dictIdx) are device pointers; the
 * list's arrays (dictOff, dictLen) stay HOST arrays.  It runs asynchronously on `stream`.  It cannot look at dictIdx before it runs:
 * a message whose dictIdx lies outside the list gets outLen -1, nothing of it is written, and the next synchronising call on the
 * context (k4lz4_synchronize, any host-pointer call) returns K4LZ4_E_ARG.
 * k4lz4_encode_dict_state, for tests: the stream context LZ4_loadDict left for entry d of the list of the context's most recent
 * k4lz4_encode_dict_batch[_device] call -- hashTable word for word, currentOffset (65536), dictSize (the kept length) -- into a HOST
 * struct; it waits for that call. */
K4LZ4_API int k4lz4_encode_dict_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                      uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n,
                                      int level, int flags, const int32_t *dictIdx, const uint8_t *dict, const uint64_t *dictOff,
                                      const int32_t *dictLen, int32_t nDict);
K4LZ4_API int k4lz4_encode_dict_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                             uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen,
                                             int64_t n, int level, int flags, const int32_t *dictIdx, const uint8_t *dict,
                                             const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict, void *stream);
K4LZ4_API int k4lz4_encode_dict_state(k4lz4_ctx *ctx, int32_t d, k4lz4_fast_chain_state *out);

/* The same at the hash-chain levels K4LZ4_L03_HC .. K4LZ4_L09_HC: block i is byte for byte what LZ4_resetStreamHC_fast(stream, level),
 * LZ4_loadDictHC(stream, dictionary, dictLen), LZ4_compress_HC_continue(stream, src, dst, srcLen, dstCap) write in that order
 * (LL.high.cs:74-88, :124-140, :187-207; LL64.high.cs:1259-1311 and the matchIndex < dictLimit arm of LZ4HC_InsertAndGetWiderMatch),
 * and decodes with k4lz4_decode_dict_batch given the same dictionary.  Arguments, the host and _device forms, outLen and the
 * treatment of a dictIdx outside the list are k4lz4_encode_dict_batch's.  Only a dictionary's last 64 KiB count; every length is
 * valid, 0 .. 3 bytes included (nothing of such a dictionary enters the chain, as LZ4_loadDictHC has it).
 * Scratch, in the context, grow-only: 256 KiB per DISTINCT dictionary of the list (hash heads 32768 x 4 bytes, chain deltas
 * 65536 x 2 bytes, built once per call and shared by all messages of that dictionary), 8 bytes per message (dispatch order), and
 * 256 KiB per wavefront of the encode launch (its table of message positions) -- one wavefront per message up to eight per
 * compute unit, so at most 512 MiB on a 256-CU device however many messages the call has; nothing per message grows with the
 * dictionary's length or the message's.
 * Refused with K4LZ4_E_ARG: level < K4LZ4_L03_HC (k4lz4_encode_dict_batch); level >= K4LZ4_L10_OPT (the optimal parser with a
 * dictionary: the only witness a test can reach, liblz4 1.9.3, and the reference differ there on about 0.3 % of inputs, so there is
 * nothing to pin the bytes against); K4LZ4_FLAG_X32 or a process under k4lz4_set_enforce32(1), and every other flag; a negative
 * dictLen, n or nDict; in the host form a dictIdx outside [0, nDict).
 * k4lz4_encode_dict_hc_state, for tests: what LZ4_loadDictHC left for entry d of the list of the context's most recent
 * k4lz4_encode_dict_hc_batch[_device] call, into HOST arrays: hashTable (32768 words: the index 65536 + k of the latest kept position
 * with the hash, 0 for none), chainTable (65536 halfwords: slot k is the delta of kept position k for k < keptLen - 3, 0xFFFF
 * elsewhere) and the kept length; it waits for that call. */
K4LZ4_API int k4lz4_encode_dict_hc_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                         uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n,
                                         int level, int flags, const int32_t *dictIdx, const uint8_t *dict, const uint64_t *dictOff,
                                         const int32_t *dictLen, int32_t nDict);
K4LZ4_API int k4lz4_encode_dict_hc_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                                uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen,
                                                int64_t n, int level, int flags, const int32_t *dictIdx, const uint8_t *dict,
                                                const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict, void *stream);
K4LZ4_API int k4lz4_encode_dict_hc_state(k4lz4_ctx *ctx, int32_t d, uint32_t *hashTable, uint16_t *chainTable, int32_t *keptLen);

/* Dictionaries that stay prepared on the device: k4lz4_dict_set.  The two calls above load their list anew on every
 * call; a set is the same list loaded once -- created, then only read, by any number of later encode and decode calls of any context
 * on its device, on any stream -- and freed with k4lz4_dict_set_destroy.  It cannot be appended to or changed.
 * For every entry it keeps, in one device allocation of its own: the last 64 KiB of the dictionary's bytes (every length down to one
 * byte), and per family of `families` the per-entry words and the tables the encode kernels take: K4LZ4_DICT_FAST is LZ4_loadDict's
 * table (16 KiB per distinct dictionary; below 8 bytes a dictionary is the empty one), K4LZ4_DICT_HC is LZ4_loadDictHC's heads and
 * chain (256 KiB per distinct dictionary; every length counts).  Entries that keep the same range of `dict` share a region and, within
 * a family, a table -- the rules of k4lz4_encode_dict_batch and k4lz4_encode_dict_hc_batch.
 * k4lz4_dict_set_create: dict, dictOff and dictLen are host pointers.  It returns after the bytes are copied and the tables are
 * built; the caller may free or overwrite `dict` at once.  Refused with K4LZ4_E_ARG: families 0 or with unknown bits, a negative
 * nDict or dictLen, a NULL array that is needed.  _device: dict is a device pointer, valid once `stream` reaches this point; dictOff
 * and dictLen stay host arrays; it too returns only after the set is complete (it synchronises `stream`).
 * k4lz4_dict_set_destroy waits for every call on the set's device that may still read it; NULL is a no-op.
 * k4lz4_dict_set_info: out[0] nDict, [1] distinct tables of the fast family, [2] of the HC family (0: family absent), [3] device bytes
 * held, [4] families, [5] device ordinal, [6] load-kernel launches so far for the fast family, [7] for the HC family: the last two
 * are what create launched and stay there -- no later call loads anything.
 * k4lz4_dict_set_layout, host arithmetic without a GPU and what create itself uses: per entry the kept length (min(dictLen, 65536)),
 * where its kept bytes lie in the set's allocation (every distinct kept range at the next 64-byte step, in list order; an empty one
 * takes no room), its table in either family (-1: family absent), and the allocation's size.  Any output pointer may be NULL.
 * k4lz4_dict_set_state / _hc_state: k4lz4_encode_dict_state / k4lz4_encode_dict_hc_state for entry d of the set -- read from the set,
 * so they do not depend on any context's most recent call. */
enum { K4LZ4_DICT_FAST = 1, K4LZ4_DICT_HC = 2 };
typedef struct k4lz4_dict_set k4lz4_dict_set;
K4LZ4_API int k4lz4_dict_set_create(k4lz4_ctx *ctx, const uint8_t *dict, const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict,
                                    int families, k4lz4_dict_set **set);
K4LZ4_API int k4lz4_dict_set_create_device(k4lz4_ctx *ctx, const uint8_t *dict, const uint64_t *dictOff, const int32_t *dictLen,
                                           int32_t nDict, int families, k4lz4_dict_set **set, void *stream);
K4LZ4_API void k4lz4_dict_set_destroy(k4lz4_dict_set *set);
K4LZ4_API int k4lz4_dict_set_info(const k4lz4_dict_set *set, int64_t out[8]);
K4LZ4_API int k4lz4_dict_set_layout(const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict, int families, int32_t *keptLen,
                                    uint64_t *keptAt, int32_t *tableFast, int32_t *tableHc, uint64_t *bytes);
K4LZ4_API int k4lz4_dict_set_state(const k4lz4_dict_set *set, int32_t d, k4lz4_fast_chain_state *out);
K4LZ4_API int k4lz4_dict_set_hc_state(const k4lz4_dict_set *set, int32_t d, uint32_t *hashTable, uint16_t *chainTable, int32_t *keptLen);

/* k4lz4_encode_dict_batch (level 0 .. 2) and k4lz4_encode_dict_hc_batch (level 3 .. 9) with the list being a set: block i is byte for
 * byte what those calls write for the same list, outLen and the untouched bytes behind it are theirs, and so is a dictIdx outside
 * [0, nDict): K4LZ4_E_ARG up front in the host form; in the _device form outLen -1, nothing written, and K4LZ4_E_ARG at the next
 * synchronising call on the context.  The call loads nothing: it launches the cost, order and encode kernels on the set's memory; the
 * context's scratch carries the ticket and histogram words, cost and order and the HC wave slots (it is the scratch of the per-call
 * calls, so their state queries refuse after a set call).  The host form stages the messages only.
 * Refused with K4LZ4_E_ARG: a level whose family the set was created without; level >= K4LZ4_L10_OPT; K4LZ4_FLAG_X32 or a process
 * under k4lz4_set_enforce32(1), and every other flag; a set on another device than the context's. */
K4LZ4_API int k4lz4_encode_dictset_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                         uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n,
                                         int level, int flags, const int32_t *dictIdx, const k4lz4_dict_set *set);
K4LZ4_API int k4lz4_encode_dictset_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                                uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen,
                                                int64_t n, int level, int flags, const int32_t *dictIdx, const k4lz4_dict_set *set,
                                                void *stream);

/* k4lz4_decode_dict_batch with message i's dictionary being entry dictIdx[i] of the set; dictIdx[i] == -1: no dictionary.  The flags
 * are that call's (K4LZ4_FLAG_PARTIAL included) and so are the decoder kernels.  The kept bytes are all a decoder can ask for: a
 * match offset is at most 65535, so nothing in front of a dictionary's last 64 KiB is reachable, and with 64 KiB present the
 * before-start check cannot fire where it would not have fired with the whole dictionary.  The dictionary is always external to the
 * target (never its prefix).  Any other index outside [0, nDict) is treated as by the encode call: K4LZ4_E_ARG up front in the host
 * form; in the _device form (dictIdx a device pointer) that message is not decoded -- outLen -1, its slot untouched -- and the next
 * synchronising call on the context returns K4LZ4_E_ARG.  A set of either family serves. */
K4LZ4_API int k4lz4_decode_dictset_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                         uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n,
                                         int flags, const int32_t *dictIdx, const k4lz4_dict_set *set);
K4LZ4_API int k4lz4_decode_dictset_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                                uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen,
                                                int64_t n, int flags, const int32_t *dictIdx, const k4lz4_dict_set *set, void *stream);

/* Frame writer on device-resident data: after k4lz4_encode_batch_device(..., K4LZ4_FLAG_ALLOW_COPY) and
 * k4lz4_xxh32_batch_device, lays the frames out (Frames/LZ4FrameWriter.cs:57-108 header, LZ4FrameWriter.async.cs:15-27
 * block records, :75-90 EndMark + content checksum).  The caller computes the positions (recOff, frameOff, tailOff) from
 * the block split and the encoded lengths; hdr holds 16 bytes per frame of which hdrLen[f] (FLG, BD [, content size]) are
 * used, hdrSum[f] their XXH32.  frameLen[f] receives each frame's length. */
K4LZ4_API int k4lz4_frame_assemble_device(k4lz4_ctx *ctx, const uint8_t *arena, const uint64_t *slotOff, const int32_t *outLen,
                                          const uint32_t *blkSum, const uint64_t *recOff, int64_t nBlocks, const uint8_t *hdr,
                                          const uint32_t *hdrLen, const uint32_t *hdrSum, const uint64_t *frameOff,
                                          const uint64_t *tailOff, const uint32_t *contentSum, uint8_t *frames,
                                          uint64_t *frameLen, int64_t nFrames, void *stream);

/* ---- frame reader on device-resident frames: LZ4FrameReader (Frames/LZ4FrameReader.blocking.cs ReadHeader / ReadBlock) over
 * many whole frames at once.  Frame f is src[frameOff[f] .. frameOff[f] + frameLen[f]); nothing outside that
 * range is read, and bytes after the frame's end (EndMark, content checksum) are ignored.  Header fields, the header checksum
 * and the block records are walked on the device, one thread per frame; block checksums, decoding and the content checksum
 * are the batch kernels' (independent-block frames: every block decoded in parallel straight into its place; chained frames,
 * and independent frames whose blocks are not all full but the last: in order, one stream per frame).
 *
 * Per-frame results (outLen, outStatus).  A frame reports the first defect the reference's reader meets in stream order: header
 * fields, header checksum, dictionary, then per block truncation, block checksum, decoding; then EndMark and content checksum;
 * then ContentLength.  -6 and -9 are the chain API's (k4lz4_decode_chain_batch). */
#define K4LZ4_FRAME_EOF            (-1)   /* the frame ends early (header, block record or trailer): EndOfStream */
#define K4LZ4_FRAME_MAGIC          (-2)   /* "LZ4 frame magic number expected" */
#define K4LZ4_FRAME_VERSION        (-3)   /* "LZ4 frame version unknown" ((FLG >> 6) & 0x11 != 1, as the reader tests it) */
#define K4LZ4_FRAME_HEADER_SUM     (-4)   /* "Invalid LZ4 frame header checksum" */
#define K4LZ4_FRAME_DICTIONARY     (-5)   /* predefined dictionary: NotImplementedException */
#define K4LZ4_FRAME_BLOCK          (-6)   /* a block does not decode */
#define K4LZ4_FRAME_BLOCK_SUM      (-7)   /* "Invalid block checksum" */
#define K4LZ4_FRAME_CONTENT_SUM    (-8)   /* "Invalid content checksum" */
#define K4LZ4_FRAME_CAPACITY       (-9)   /* dstCap[f] is too small for what the frame produces */
#define K4LZ4_FRAME_LENGTH         (-10)  /* the output does not match the declared ContentLength (also: it would pass a ContentLength
                                             that is <= dstCap[f], which is this code and not -9) */

/* outSize[f] = what frame f may decode to at most, without trusting its header: per block min(blockSize, 255 * stored + 32), the
 * stored length for a raw block, the total capped by ContentLength when the frame declares one (what LZ4Frame.DecodeBatch allows);
 * outStatus[f] = 0, or the header / structure defect the walk found (-1 .. -5; with -1 after the header, outSize covers the
 * complete blocks before the end).  Every pointer is a device pointer.  Asynchronous on `stream`.  Mirrors
 * k4lz4_unpickle_sizes_device. */
K4LZ4_API int k4lz4_frame_sizes_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen,
                                       int64_t n, uint64_t *outSize, int32_t *outStatus, void *stream);
/* Decodes frame f into dst + dstOff[f] (at most dstCap[f] bytes; outSize of k4lz4_frame_sizes_device always suffices);
 * outLen[f] = bytes produced, or a K4LZ4_FRAME_* code.  Bytes of a slot past outLen[f] may be written (with blocks that later
 * turn out not to fit, or with blocks of a failing frame) but nothing outside [dstOff[f], dstOff[f] + dstCap[f]) is.  Every
 * pointer is a device pointer.  The number of blocks is known only on the device: the call reads it back once to size its
 * grow-only block table (56 bytes per block, plus 105 bytes per frame), so it WAITS FOR `stream` there, after the walk; everything
 * else is enqueued on `stream`. */
K4LZ4_API int k4lz4_decode_frames_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen,
                                         int64_t n, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen,
                                         void *stream);
/* The same on host memory (staged through the GPU like k4lz4_decode_chain_batch; the staging is sized by the sum of dstCap):
 * exactly outLen[f] bytes are written to dst + dstOff[f] for a frame that decodes, none for one that fails.  Synchronous. */
K4LZ4_API int k4lz4_frame_sizes(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                                uint64_t *outSize, int32_t *outStatus);
K4LZ4_API int k4lz4_decode_frames(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                                  uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen);

/* ---- legacy formats: K4os.Compression.LZ4.Legacy (LZ4Wrapper.cs, LZ4Stream.cs) ------------------------------
 * Per-item codes: the exception the reference throws, in the order it meets them. */
#define K4LZ4_LEGACY_END_OF_STREAM (-1)   /* EndOfStreamException: truncated varint or payload, a varint where the stream ends, C > U */
#define K4LZ4_LEGACY_OVERFLOW      (-2)   /* OverflowException: a negative length (after truncation to 32 bits) reaches new byte[] */
#define K4LZ4_LEGACY_NOT_SUPPORTED (-3)   /* NotSupportedException: a compressed chunk with passes ((int)flags >> 2 != 0) */
#define K4LZ4_LEGACY_INVALID_DATA  (-4)   /* InvalidDataException: a compressed chunk does not decode to exactly U bytes (also: U > 255 * C + 32) */
#define K4LZ4_LEGACY_ARGUMENT      (-5)   /* ArgumentException (Unwrap): fewer than 8 bytes, a payload past the end, a negative source length */
#define K4LZ4_LEGACY_CAPACITY      (-6)   /* not the reference's: the caller's target is too small */
#define K4LZ4_LEGACY_NOT_ENCODED   (-7)   /* not the reference's: an HC chunk was not encoded for want of reserved scratch
                                             (k4lz4_ctx_reserve_hc; the call's status says so too) */

/* LZ4Wrapper.Wrap / WrapHC: outLen[i] = 8 + payload bytes written to dst + dstOff[i] ([u32 U][u32 C][block], or [u32 U][u32 U][the
 * bytes] when the block is not shorter than U; 8 zero bytes for an empty message), -1 when dstCap[i] < k4lz4_wrap_bound(srcLen[i]).
 * high = 0: L00_FAST, else L09_HC.  flags: K4LZ4_FLAG_X32, K4LZ4_FLAG_NO_REORDER.  The encoder writes straight into the slot
 * (cap U - 1); fast batches take the pickles' two-step encoder and segments, HC the pickles' envelope path.  Scratch: the
 * encoders' (d_pk_meta, 16 bytes per message; HC as k4lz4_pickle_batch).  As with pickles (the same deliberate deviation), behind
 * outLen[i] the slot may hold what the encoder wrote in place at +8 where the block did not shrink or the message was cut into
 * segments, up to 7 + srcLen[i]; a block that shrank leaves nothing behind outLen[i] (the header is always 8 bytes).  Where the
 * slot is too small nothing outside it is written. */
K4LZ4_API int k4lz4_wrap_bound(int srcLen);
K4LZ4_API int k4lz4_wrap_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                               const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int high, int flags);
K4LZ4_API int k4lz4_wrap_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                                      const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int high, int flags,
                                      void *stream);
/* LZ4Wrapper.Unwrap on one buffer of len bytes (host arithmetic): the result's length, or K4LZ4_LEGACY_ARGUMENT / _OVERFLOW */
K4LZ4_API int k4lz4_unwrap_size(const uint8_t *buf, int64_t len);
/* the same for a batch on the device: outLen[i] = length or code */
K4LZ4_API int k4lz4_unwrap_sizes_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                        int32_t *outLen, int64_t n, void *stream);
/* Unwrap a batch: outLen[i] = the length Unwrap returns (bytes at dst + dstOff[i]), a K4LZ4_LEGACY_* code, or K4LZ4_LEGACY_CAPACITY
 * when dstCap[i] is smaller.  decoded[i] = what LZ4Codec.Decode returned: the decoded length, -1 for a payload that does not decode,
 * 0 for an empty payload; for a stored (raw) result its length.  Unwrap ignores that value and returns outLen bytes all the same:
 * decoded[i] == outLen[i] says the bytes are the payload's.  Compressed payloads go through the batch decoder with cap = outLen.
 * Scratch (device form): 20 bytes per buffer. */
K4LZ4_API int k4lz4_unwrap_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                                 const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int32_t *decoded, int64_t n);
K4LZ4_API int k4lz4_unwrap_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                        uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int32_t *decoded,
                                        int64_t n, void *stream);

/* LZ4Stream (LZ4Legacy.Encode) with the whole content written and the stream disposed: chunks of max(16, blockSize) bytes, each
 * `varint(flags) varint(U) [varint(C)] payload`, compressed iff C < U, HighCompression (2) on every chunk of a high stream.
 * The most a stream of srcLen bytes takes: */
K4LZ4_API int64_t k4lz4_legacy_stream_bound(int64_t srcLen, int blockSize);
/* Content i = src[srcOff[i] .. + srcLen[i]) -> stream i at dst + dstOff[i]; outLen[i] = its bytes, K4LZ4_LEGACY_CAPACITY when it
 * does not fit dstCap[i] (nothing is written then), or K4LZ4_LEGACY_NOT_ENCODED.  high = 0: L00_FAST, else L09_HC; flags:
 * K4LZ4_FLAG_X32.  Every chunk of every stream is encoded in one batch into an arena; record sizes, their scan and the assembly
 * run on the device.  The device form reads the chunk count back once (it WAITS FOR `stream` after the first scan).  Grow-only
 * scratch: 36 bytes per stream, 48 bytes per chunk, and an arena of the contents' bytes (each rounded up to 16). */
K4LZ4_API int k4lz4_encode_legacy_streams(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, int64_t n,
                                          int blockSize, int high, int flags, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                                          int64_t *outLen);
K4LZ4_API int k4lz4_encode_legacy_streams_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen,
                                                 int64_t n, int blockSize, int high, int flags, uint8_t *dst, const uint64_t *dstOff,
                                                 const uint64_t *dstCap, int64_t *outLen, void *stream);
/* Stream i = src[streamOff[i] .. + streamLen[i]), read as LZ4Stream (LZ4Legacy.Decode) reads it to its end; nothing outside that
 * range is read.  outSize[i] = the bytes of the chunks before the first structural defect, each compressed chunk's U trusted only
 * up to 255 * C + 32 (a chunk that claims more is an InvalidData defect there); outStatus[i] = 0 or that defect's code. */
K4LZ4_API int k4lz4_legacy_stream_sizes(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *streamOff, const uint64_t *streamLen,
                                        int64_t n, uint64_t *outSize, int32_t *outStatus);
K4LZ4_API int k4lz4_legacy_stream_sizes_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *streamOff, const uint64_t *streamLen,
                                               int64_t n, uint64_t *outSize, int32_t *outStatus, void *stream);
/* Decodes stream i into dst + dstOff[i]; outLen[i] = the content's bytes, or the code of the first defect in stream order: a chunk
 * that does not decode (compressed chunks before the walk's defect are decoded by the batch decoder, straight into place, cap U),
 * a chunk that does not fit dstCap[i] (K4LZ4_LEGACY_CAPACITY at that chunk), or the walk's structural defect.  Bytes of a failing
 * stream's slot may be written, nothing outside [dstOff[i], dstOff[i] + dstCap[i]).  The device form reads the chunk count back
 * once (it WAITS FOR `stream` after the walk).  Grow-only scratch: 36 bytes per stream and 48 bytes per chunk. */
K4LZ4_API int k4lz4_decode_legacy_streams(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *streamOff, const uint64_t *streamLen,
                                          int64_t n, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen);
K4LZ4_API int k4lz4_decode_legacy_streams_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *streamOff, const uint64_t *streamLen,
                                                 int64_t n, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen,
                                                 void *stream);

/* ---- incremental frame writer: many LZ4FrameWriters (Frames/LZ4FrameWriter*.cs, Streams/LZ4EncoderStream.cs:44-66) advanced by one
 * Write, OpenFrame or CloseFrame each per call.  For every stream a call returns exactly the bytes the reference's
 * writer pushes to its inner stream during that call: the header at the first Write (even an empty one) or at an explicit open,
 * a block record for every block that fills up (TopupAndEncode(forceEncode: false, allowCopy: true)), and at close the last partial
 * block, the EndMark and the content checksum.  Block and content checksums and ContentLength follow LZ4Frame.EncodeBatch (the
 * content size is written when asked for; a close whose byte count differs is refused).  Levels: every LZ4Level for independent
 * and chained-HC frames; chained frames below L03_HC take LZ4FastChainEncoder's blocks (not under K4LZ4_FLAG_X32 / Enforce32:
 * K4LZ4_E_ARG).  Chained streams longer than 2 GB - 64 KiB are refused with K4LZ4_E_ARG.
 *
 * k4lz4_frame_writer is the per-stream record, in HOST memory, owned by the caller: the settings and the counters.  The counters depend
 * on lengths only, so a call updates them without waiting for the device.  The bytes a stream holds between calls (the encoder's
 * ring buffer: the saved dictionary and the pending bytes), its XXH32 state and, for chained fast streams, its
 * k4lz4_fast_chain_state live in a DEVICE store of k4lz4_frame_writer_store_bytes(w) bytes at store + storeOff[s], also the caller's;
 * it needs no initialisation. */
typedef struct k4lz4_frame_writer_settings {
    int64_t contentLength;       /* < 0: no content size in the header */
    int32_t blockSize;           /* the descriptor's BlockSize, 1 .. 4 MiB (LZ4FrameWriter.cs:184-189) */
    int32_t level;               /* k4lz4_level */
    int32_t chainBlocks, blockChecksum, contentChecksum;
    int32_t extraMemory;         /* LZ4EncoderSettings.ExtraMemory (Streams/Extensions.cs:18-19) */
} k4lz4_frame_writer_settings;

typedef struct k4lz4_frame_writer {
    k4lz4_frame_writer_settings settings;
    int32_t kind;                /* 0 independent blocks, 1 chained HC, 2 chained fast */
    int32_t encBlock;            /* the encoder's block: BlockSize, or for chained frames the ring's whole-KiB block */
    int32_t extraBlocks;
    int32_t ringBytes;           /* the ring buffer: 64 KiB + (1 + extraBlocks) * encBlock + 32, or encBlock for independent blocks */
    int64_t written;             /* content bytes taken so far */
    int32_t index, pointer;      /* the ring: its encoded prefix (the dictionary) and the bytes it holds */
    uint32_t currentOffset, dictSize; /* chained fast: LZ4_stream_t's two indices */
    int32_t phase;               /* 0 not opened, 1 open, 2 closed */
    int32_t reserved;
} k4lz4_frame_writer;

enum k4lz4_frame_write_op { K4LZ4_FWRITE_WRITE = 0, K4LZ4_FWRITE_OPEN = 1, K4LZ4_FWRITE_CLOSE = 2 };

/* per-stream codes in outLen (decided on the host before anything is enqueued; such a stream keeps its record and store unchanged) */
#define K4LZ4_FWRITE_TARGET        (-1)   /* dstCap[s] is below k4lz4_frame_write_bound */
#define K4LZ4_FWRITE_CLOSED        (-2)   /* the stream was closed by an earlier call */
#define K4LZ4_FWRITE_LENGTH        (-3)   /* close: the bytes written differ from the settings' contentLength */

/* K4LZ4_OK or K4LZ4_E_ARG (a block size outside 1 .. 4 MiB) */
K4LZ4_API int k4lz4_frame_writer_init(k4lz4_frame_writer *w, const k4lz4_frame_writer_settings *settings);
K4LZ4_API int64_t k4lz4_frame_writer_store_bytes(const k4lz4_frame_writer *w);
/* the most a call can emit for the stream: srcLen new bytes, closing (CLOSE) or not */
K4LZ4_API int64_t k4lz4_frame_write_bound(const k4lz4_frame_writer *w, int64_t srcLen, int closing);
/* op: k4lz4_frame_write_op for every stream; srcLen[s] < 0 leaves stream s untouched (outLen 0).  WRITE: srcLen[s] bytes at
 * src + srcOff[s]; OPEN: srcLen[s] must be 0; CLOSE: srcLen[s] bytes are written first, then the frame is closed.  flags:
 * K4LZ4_FLAG_X32 (LZ4Codec.Enforce32 is read as well).  outLen[s]: the bytes written at dst + dstOff[s], or a K4LZ4_FWRITE_* code.
 * A call-level failure (K4LZ4_E_ARG is decided before anything is enqueued) leaves every record as it was; after K4LZ4_E_HIP or
 * K4LZ4_E_NOMEM the stores of the streams the call ran are undefined and those streams cannot be continued.
 * _device: src, store, dst and outLen (int64_t) are device pointers, the other arrays host arrays.  It enqueues this call's work on `stream`
 * and returns without waiting for it.  Before it rewrites its host-side plan it waits until the previous writer call's plan has been
 * copied up (the context's own event), and each chained group waits the same way for the previous chained block table, as
 * k4lz4_encode_hc_chain_batch_device does: a call whose batch holds two or more chained groups (two HC levels, HC and fast, with and
 * without block checksums) therefore waits, part-way, until the device has reached the previous group's table upload. */
K4LZ4_API int k4lz4_frame_write_batch(k4lz4_ctx *ctx, k4lz4_frame_writer *w, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                                      const uint64_t *srcOff, const int64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                                      int64_t *outLen, int64_t n, int op, int flags);
K4LZ4_API int k4lz4_frame_write_batch_device(k4lz4_ctx *ctx, k4lz4_frame_writer *w, uint8_t *store, const uint64_t *storeOff,
                                             const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen, uint8_t *dst,
                                             const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen, int64_t n, int op, int flags,
                                             void *stream);

/* ---- incremental frame reader: many LZ4FrameReaders (Frames/LZ4FrameReader*.cs, Streams/LZ4DecoderStream.cs) advanced by one
 * ReadManyBytes(count[s]) or one OpenFrame each per call.  Stream s is src[srcOff[s] .. srcOff[s] + srcLen[s]): zero
 * or more frames one after another, all of it present at every call (the same bytes at every call: the reader keeps its position,
 * not the data); nothing outside that range is read.  A READ delivers what the reference's reader delivers for the same sequence of
 * reads: it opens a frame if none is open (no bytes left: 0; one to three bytes left: K4LZ4_FRAME_EOF), then reads blocks and drains
 * them until count[s] bytes are delivered, the EndMark is read (the frame is closed and the read ends with what it has, possibly 0;
 * the next read opens the next frame), or a block yields nothing (a raw block of stored length 0; under chained frames a compressed
 * block that decodes to nothing).  A read satisfied exactly at a block's end does not look at the next length word.  Independent
 * frames are decoded as LZ4BlockDecoder does (capacity blockSize + 8, a block of nothing is a defect), chained ones as
 * LZ4ChainDecoder does (capacity blockSize, the last 64 KiB of the frame's output as prefix).  The output is not compared with a
 * declared ContentLength (the reference's reader does not; k4lz4_decode_frames does).  interactive != 0: return after the first
 * drain.  OPEN is OpenFrame().
 *
 * outLen[s]: READ: the bytes written at dst + dstOff[s] (0 .. count[s]); OPEN: 1 a frame is open, 0 the source is at its end; or the
 * code of the exception the reference throws during that call, in the order it meets them: K4LZ4_FRAME_EOF .. _CONTENT_SUM with
 * their meanings above (-9 and -10 do not occur), or K4LZ4_FRAME_BLOCK_SIZE.  A stored block length above the frame's block size is
 * K4LZ4_FRAME_BLOCK (in the reference it overruns a pooled buffer whose length depends on the pool).  A stream that has reported a
 * code is failed: every later call reports the same code and touches nothing.  The bytes of a failing call's slot are unspecified;
 * nothing outside [dstOff[s], dstOff[s] + count[s]) is ever written.  count[s] < 0 leaves stream s untouched (outLen 0).
 *
 * Everything a reader keeps between calls lives in a caller-owned DEVICE store of k4lz4_frame_reader_store_bytes(r) bytes at
 * store + storeOff[s] (256-byte aligned): position, phase, descriptor, the content checksum's state, the undrained rest of one block
 * and, for chained frames, the 64 KiB of history.  It must be reset once (K4LZ4_FREAD_RESET) before its first use.  The host record
 * holds the settings and the store size and is never changed by a call. */
#define K4LZ4_FRAME_BLOCK_SIZE     (-11)  /* the frame's block size is above the reader's maxBlockSize (not the reference's) */

typedef struct k4lz4_frame_reader_settings {
    int32_t maxBlockSize;        /* the largest block size the store holds: rounded up to 64 KiB, 256 KiB, 1 MiB or 4 MiB; <= 0: 4 MiB */
    int32_t flags;               /* 0, or K4LZ4_FREADER_FED: a record for k4lz4_frame_read_fed_batch (below) */
} k4lz4_frame_reader_settings;

typedef struct k4lz4_frame_reader {
    k4lz4_frame_reader_settings settings;      /* maxBlockSize as rounded */
    int64_t storeBytes;                        /* per stream */
} k4lz4_frame_reader;

enum k4lz4_frame_read_op { K4LZ4_FREAD_READ = 0, K4LZ4_FREAD_OPEN = 1, K4LZ4_FREAD_RESET = 2 };
#define K4LZ4_FREAD_INTERACTIVE 1          /* flags: ReadManyBytes(buffer, interactive: true) */

/* k4lz4_frame_reader_query: int64 words per stream */
enum { K4LZ4_FRQ_BYTES_READ = 0,       /* GetBytesRead: over all the frames read so far */
       K4LZ4_FRQ_FRAME_LENGTH = 1,     /* the open frame's ContentLength; -1: no frame is open or it declares none */
       K4LZ4_FRQ_PHASE = 2,            /* 0 no frame open, 1 a frame is open, 2 failed */
       K4LZ4_FRQ_CODE = 3,             /* the failed stream's code */
       K4LZ4_FRQ_BLOCKS = 4,           /* blocks read so far */
       K4LZ4_FRQ_DIRECT = 5,           /* of those, decoded straight into dst */
       K4LZ4_FRQ_FAST = 6,             /* of those, decoded by the batch decoder on the fast path */
       K4LZ4_FRQ_HANDED_BACK = 7,      /* calls in which the fast path's hypothesis failed for the stream and the general reader replayed it */
       K4LZ4_FRQ_WORDS = 8 };

/* K4LZ4_OK or K4LZ4_E_ARG (a maxBlockSize above 4 MiB, unknown flags) */
K4LZ4_API int k4lz4_frame_reader_init(k4lz4_frame_reader *r, const k4lz4_frame_reader_settings *settings);
K4LZ4_API int64_t k4lz4_frame_reader_store_bytes(const k4lz4_frame_reader *r);
/* op: k4lz4_frame_read_op for every stream of the call (RESET: count[s] >= 0 resets stream s's store; src, dst may be NULL for RESET
 * and OPEN where nothing is written).  flags: K4LZ4_FREAD_INTERACTIVE.
 * k4lz4_frame_read_batch: store is a device pointer, every other pointer a host pointer; the sources and the per-stream arrays are
 * staged through the context's staging buffers, the bytes come back into dst + dstOff[s].  Synchronous.
 * _device: every pointer is a device pointer (the per-stream arrays too).  maxCount: no count[s] of the call is above it (the host
 * form takes the largest count).  It bounds the fast path's block table -- maxCount / 64 KiB + 2 rows per stream in the context's
 * grow-only scratch (about 48 bytes a row) -- so the call enqueues on `stream` and returns without waiting for its own work (a scratch
 * that has to grow waits for the context's earlier work).  maxCount <= 0: the general reader alone, one kernel.
 * Two ways through a READ: streams that read with nothing pending from an independent-block frame are planned under
 * the hypothesis that the blocks the read covers are full: those blocks go through the batch decoder straight into dst, the one that
 * straddles the read's end into the store, and a kernel verifies the hypothesis and commits the state.  Every other stream, and every
 * stream whose hypothesis fails, is read by the general reader (one wavefront per stream) from its unchanged state, in the same call. */
K4LZ4_API int k4lz4_frame_read_batch(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff,
                                     const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst,
                                     const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t n, int op, int flags);
K4LZ4_API int k4lz4_frame_read_batch_device(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff,
                                            const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst,
                                            const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t n, int op, int flags,
                                            int64_t maxCount, void *stream);
/* rows of the fast path's block table per stream for a call whose counts do not pass maxCount */
K4LZ4_API int64_t k4lz4_frame_read_table_rows(int64_t maxCount);
/* out[s * K4LZ4_FRQ_WORDS + k]: host form (storeOff, out host arrays; synchronous) and device form (device arrays; asynchronous) */
K4LZ4_API int k4lz4_frame_reader_query(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out);
K4LZ4_API int k4lz4_frame_reader_query_device(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out,
                                              void *stream);

/* ---- The incremental frame reader fed its source in pieces ------------------------------------------------
 * What LZ4DecoderStream does over a socket, a pipe or a file that hands bytes over as they arrive: the reference loops over short
 * reads of its inner stream until the field it wants is complete (Streams/Internal/ReaderExtensions.cs:10-28), so how a source is
 * cut into pieces is invisible in what is delivered.  Here stream s's source is the concatenation of the pieces given so far.  For
 * a call, src[srcOff[s] .. + srcLen[s]) is the part of it the reader has not consumed yet (any length, 0 included) and
 * final[s] != 0 says that no byte will follow it (final == NULL: none is final).  One READ or OPEN per stream and call.
 *
 * A record made with K4LZ4_FREADER_FED has a larger store -- today's, followed by a stash of 4 + maxBlockSize + 4 bytes (rounded to
 * 256) that holds at most one incomplete field -- and is taken by the _fed calls only; they refuse any other record, and the calls
 * above refuse a fed record (K4LZ4_E_ARG).  k4lz4_frame_reader_query[_device] read either kind of store.
 *
 * starved      the field the reader needs next (the 4 bytes of the magic; FLG / BD; the rest of the header once FLG is known; a
 *              length word; a payload plus its block checksum; the content checksum behind an EndMark) is not wholly there and
 *              final[s] == 0: the call ends for that stream with outLen[s] what was delivered so far (0 .. count[s]; OPEN: 0),
 *              consumed[s] == srcLen[s] (the incomplete field's bytes are kept in the store) and need[s] > 0, the number of further
 *              bytes with which that field is complete.  Issue the read again with the count reduced by outLen[s] and with further
 *              source; with fewer than need[s] bytes it delivers nothing and reports what is still missing.  The bytes, the total
 *              and the code of such a sequence are those of ONE ReadManyBytes(count) over the concatenated source, however it was
 *              cut.  With final[s] != 0 running out is what it is above: nothing left before a frame is a clean end (0), anything
 *              else K4LZ4_FRAME_EOF.
 * not starved  need[s] == 0 and consumed[s] <= srcLen[s]: present the unconsumed rest first in the next call.  Nothing is kept in
 *              the store then.  A read satisfied exactly at a block's end does not consume the next length word.
 * defects      are reported in the call in which their bytes are present: a wrong magic after 4 bytes, a bad version after 6, a
 *              stored length above the block size after the length word.  consumed[s] of a failing call is unspecified.
 * count[s] < 0 leaves the stream untouched (outLen, consumed, need 0).
 *
 * k4lz4_frame_read_fed_batch: store is a device pointer, every other pointer a host pointer; only the pieces go up, through the
 * context's staging buffers; dst, outLen, consumed and need come back.  Synchronous.  _device: every pointer a device pointer,
 * maxCount as above; enqueues on `stream` and returns, nothing is read back.  The fast path takes streams with nothing kept and
 * nothing pending in an independent-block frame, over the records that are wholly in the piece. */
#define K4LZ4_FREADER_FED 1                /* k4lz4_frame_reader_settings.flags */
K4LZ4_API int k4lz4_frame_read_fed_batch(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff,
                                         const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, const int64_t *final,
                                         uint8_t *dst, const uint64_t *dstOff, const int64_t *count, int64_t *outLen,
                                         int64_t *consumed, int64_t *need, int64_t n, int op, int flags);
K4LZ4_API int k4lz4_frame_read_fed_batch_device(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff,
                                                const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen,
                                                const int64_t *final, uint8_t *dst, const uint64_t *dstOff, const int64_t *count,
                                                int64_t *outLen, int64_t *consumed, int64_t *need, int64_t n, int op, int flags,
                                                int64_t maxCount, void *stream);

/* ---- LZ4Stream written and read piece by piece: many open K4os.Compression.LZ4.Legacy.LZ4Streams advanced by one Write, Flush,
 * Dispose or Read each per call ---------------------------------------------------------------------------------
 * Writer.  For every stream a call returns exactly the bytes the reference's stream pushes to its inner stream during that call.
 * The reference flushes lazily (LZ4Stream.cs:425-439): a buffer that a Write fills exactly is not emitted by that call -- it goes
 * out when the next byte arrives, or at Flush / Dispose.  With p pending bytes and L > 0 new ones a WRITE emits
 * max(0, ceil((p + L) / B) - 1) chunks of B = max(16, blockSize) bytes and leaves p + L - B * emitted pending; L == 0 emits
 * nothing.  FLUSH emits the pending bytes as one chunk if there are any.  CLOSE writes its bytes first, then flushes, and the
 * stream is closed.
 *
 * k4lz4_legacy_writer is the per-stream record, in HOST memory, owned by the caller.  Everything in it follows from lengths, so a
 * call advances it without waiting for the device.  The pending bytes (the stream's _buffer) live in a DEVICE store of
 * k4lz4_legacy_writer_store_bytes(w) bytes at store + storeOff[s], also the caller's; it needs no initialisation. */
#define K4LZ4_LEGACY_BLOCK_SIZE    (-8)   /* not the reference's: a chunk's U is above the reader's maxBlockSize */
#define K4LZ4_LEGACY_CLOSED        (-9)   /* not the reference's: the stream was closed by an earlier call */

typedef struct k4lz4_legacy_writer {
    int32_t blockSize;           /* as applied: max(16, blockSize) */
    int32_t high;                /* 0: L00_FAST; else L09_HC, HighCompression on every chunk */
    int32_t pending;             /* _bufferOffset: bytes in the store */
    int32_t closed;
} k4lz4_legacy_writer;

enum k4lz4_legacy_write_op { K4LZ4_LWRITE_WRITE = 0, K4LZ4_LWRITE_FLUSH = 1, K4LZ4_LWRITE_CLOSE = 2 };

/* K4LZ4_OK or K4LZ4_E_ARG (a block size above 0x7E000000, the block encoder's longest input) */
K4LZ4_API int k4lz4_legacy_writer_init(k4lz4_legacy_writer *w, int blockSize, int high);
K4LZ4_API int64_t k4lz4_legacy_writer_store_bytes(const k4lz4_legacy_writer *w);
/* the most a call with op can emit for the stream given srcLen new bytes (FLUSH takes none) */
K4LZ4_API int64_t k4lz4_legacy_write_bound(const k4lz4_legacy_writer *w, int64_t srcLen, int op);
/* op: k4lz4_legacy_write_op for every stream of the call; srcLen[s] < 0 leaves stream s untouched (outLen 0).  WRITE and CLOSE take
 * srcLen[s] bytes at src + srcOff[s]; for FLUSH srcLen[s] must be 0.  flags: K4LZ4_FLAG_X32 (LZ4Codec.Enforce32 is read as well).
 * outLen[s]: the bytes written at dst + dstOff[s]; K4LZ4_LEGACY_CAPACITY (dstCap[s] is below k4lz4_legacy_write_bound) or
 * K4LZ4_LEGACY_CLOSED, both decided on the host before anything is enqueued -- such a stream keeps its record and store as they
 * were and the call may be issued again; or K4LZ4_LEGACY_NOT_ENCODED.  A call-level K4LZ4_E_ARG leaves every record as it was.
 * Only the first chunk of a call can straddle the store and the call's bytes: it is staged into a window; every other chunk is
 * encoded from src in place.  All chunks of all streams go through the batch encoder in one batch per level (cap U - 1); record
 * sizes, their scan and the assembly run on the device, then the tail is appended to the store.
 * _device: src, store, dst and outLen (int64_t) are device pointers, the other arrays host arrays.  It enqueues on `stream` and
 * returns: nothing is read back.  Before it rewrites its host-side plan it waits until the previous writer call's plan (this
 * writer's or the frame writer's) has been copied up. */
K4LZ4_API int k4lz4_legacy_write_batch(k4lz4_ctx *ctx, k4lz4_legacy_writer *w, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                                       const uint64_t *srcOff, const int64_t *srcLen, uint8_t *dst, const uint64_t *dstOff,
                                       const uint64_t *dstCap, int64_t *outLen, int64_t n, int op, int flags);
K4LZ4_API int k4lz4_legacy_write_batch_device(k4lz4_ctx *ctx, k4lz4_legacy_writer *w, uint8_t *store, const uint64_t *storeOff,
                                              const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen, uint8_t *dst,
                                              const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen, int64_t n, int op, int flags,
                                              void *stream);

/* Reader.  Stream s is src[srcOff[s] .. + srcLen[s]), all of it present at every call (the reader keeps its position, not the
 * data); nothing outside that range is read.  A READ delivers, byte for byte and exception for exception, what LZ4Stream.Read
 * (LZ4Stream.cs:349-377) returns for the same sequence of counts: it drains the buffered chunk and acquires chunks
 * (AcquireNextChunk, :248-294; chunks that produce no bytes are skipped) until count[s] bytes are delivered or the source ends
 * cleanly; with K4LZ4_LREAD_INTERACTIVE it returns after the first copy.  count 0 acquires nothing; ReadByte is a read of 1.
 * outLen[s]: the bytes written at dst + dstOff[s] (0 .. count[s]), or the code of the exception the reference throws during that
 * call -- K4LZ4_LEGACY_END_OF_STREAM, _OVERFLOW, _NOT_SUPPORTED, _INVALID_DATA in AcquireNextChunk's order, as
 * k4lz4_decode_legacy_streams reports them -- or K4LZ4_LEGACY_BLOCK_SIZE.  A stream that has reported a code is failed: every
 * later call reports the same code and touches nothing.  The bytes of a failing call's slot are unspecified; nothing outside
 * [dstOff[s], dstOff[s] + count[s]) is ever written.  count[s] < 0 leaves stream s untouched (outLen 0).
 *
 * The state (source position, _bufferOffset, _bufferLength, the code) and one decoded chunk live in a caller-owned DEVICE store of
 * k4lz4_legacy_reader_store_bytes(r) bytes at store + storeOff[s] (256-byte aligned), reset once (K4LZ4_LREAD_RESET) before its
 * first use.  The host record holds settings only.  Sources that arrive in pieces (4.15's contract) are read by
 * k4lz4_legacy_read_fed_batch, below, through a record of its own kind. */
typedef struct k4lz4_legacy_reader {
    int32_t maxBlockSize;        /* the largest chunk (U) the store holds; as applied: max(16, asked), asked <= 0: 1 MiB */
    int32_t flags;               /* 0, or K4LZ4_LREADER_FED: a record for k4lz4_legacy_read_fed_batch (below) */
    int64_t storeBytes;          /* per stream */
} k4lz4_legacy_reader;

enum k4lz4_legacy_read_op { K4LZ4_LREAD_READ = 0, K4LZ4_LREAD_RESET = 1 };
#define K4LZ4_LREAD_INTERACTIVE 1          /* flags: LZ4StreamFlags.InteractiveRead */

/* k4lz4_legacy_reader_query: int64 words per stream */
enum { K4LZ4_LSQ_POSITION = 0,         /* bytes of the source consumed */
       K4LZ4_LSQ_BYTES_READ = 1,       /* bytes delivered */
       K4LZ4_LSQ_PENDING = 2,          /* _bufferLength - _bufferOffset */
       K4LZ4_LSQ_CODE = 3,             /* the failed stream's code, else 0 */
       K4LZ4_LSQ_CHUNKS = 4,           /* chunks acquired (those that produce bytes) */
       K4LZ4_LSQ_DIRECT = 5,           /* of those, made straight in dst by the general kernel */
       K4LZ4_LSQ_BATCHED = 6,          /* of those, decoded by the batch decoder on the direct path */
       K4LZ4_LSQ_HANDED_BACK = 7,      /* calls in which the direct path handed the stream back to the general kernel */
       K4LZ4_LSQ_WORDS = 8 };

/* K4LZ4_OK or K4LZ4_E_ARG (a maxBlockSize above 0x7E000000) */
K4LZ4_API int k4lz4_legacy_reader_init(k4lz4_legacy_reader *r, int maxBlockSize);
K4LZ4_API int64_t k4lz4_legacy_reader_store_bytes(const k4lz4_legacy_reader *r);
/* rows of the direct path's chunk table per stream: min(maxCount / maxBlockSize + 2, 1024) */
K4LZ4_API int64_t k4lz4_legacy_read_table_rows(const k4lz4_legacy_reader *r, int64_t maxCount);
/* k4lz4_legacy_read_batch: store is a device pointer, every other pointer a host pointer; synchronous.
 * _device: every pointer is a device pointer (the per-stream arrays too); enqueues on `stream` and returns.  maxCount: no count[s]
 * is above it; it bounds the direct path's chunk table (<= 0: the general kernel alone).
 * Two ways through a READ, decided on the device: streams that read (not interactive) with nothing pending are planned by a walk
 * over their chunk headers; whole chunks go through the batch decoder straight into dst (stored ones are copied), the chunk that
 * straddles the read's end into the store.  Interactive streams, streams with bytes pending, streams with more whole chunks than
 * table rows and streams with a defect in the planned range are read by the general kernel (one wavefront per stream) from their
 * unchanged state, in the same call. */
K4LZ4_API int k4lz4_legacy_read_batch(k4lz4_ctx *ctx, const k4lz4_legacy_reader *r, uint8_t *store, const uint64_t *storeOff,
                                      const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst,
                                      const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t n, int op, int flags);
K4LZ4_API int k4lz4_legacy_read_batch_device(k4lz4_ctx *ctx, const k4lz4_legacy_reader *r, uint8_t *store, const uint64_t *storeOff,
                                             const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst,
                                             const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t n, int op, int flags,
                                             int64_t maxCount, void *stream);
/* out[s * K4LZ4_LSQ_WORDS + k]: host form (storeOff, out host arrays; synchronous) and device form (device arrays; asynchronous) */
K4LZ4_API int k4lz4_legacy_reader_query(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out);
K4LZ4_API int k4lz4_legacy_reader_query_device(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out,
                                               void *stream);

/* ---- The incremental LZ4Stream reader fed its source in pieces ---------------------------------------------
 * What LZ4Stream does in Decompress mode over a socket, a pipe or a file that hands bytes over as they arrive: the reference reads
 * a chunk's varints one byte at a time (TryReadVarInt, LZ4Stream.cs:133-155) and loops until a payload is complete (ReadBlock,
 * :176-191), so how a source is cut into pieces is invisible in what Read returns.  Here stream s's source is the concatenation of
 * the pieces given so far.  For a call, src[srcOff[s] .. + srcLen[s]) is the part of it the reader has not consumed yet (any
 * length, 0 included) and final[s] != 0 says that no byte will follow it (final == NULL: none is final).  op and flags are
 * k4lz4_legacy_read_op and K4LZ4_LREAD_INTERACTIVE.
 *
 * A record made by k4lz4_legacy_reader_init_fed (flags == K4LZ4_LREADER_FED) has a larger store -- today's, followed by a stash of
 * 30 + maxBlockSize bytes (rounded to 256: one chunk header, one payload) that holds at most one incomplete field -- and is taken
 * by the _fed calls only; they refuse any other record, and the calls above refuse a fed record (K4LZ4_E_ARG).
 * k4lz4_legacy_reader_query[_device] read either kind of store; for a fed stream K4LZ4_LSQ_POSITION is the sum of consumed.
 *
 * starved      the field the reader needs next -- the next byte of a chunk header (the flags varint, the U varint, the C varint of a
 *              compressed chunk: need 1), or a chunk's payload of C bytes (need: the bytes still missing) -- is not wholly there and
 *              final[s] == 0: the call ends for that stream with outLen[s] what was delivered so far (0 .. count[s]),
 *              consumed[s] == srcLen[s] (the incomplete field's bytes are kept in the store) and need[s] > 0.  Issue the read again
 *              with the count reduced by outLen[s] and with further source; with fewer than need[s] bytes it delivers nothing and
 *              reports what is still missing.  The bytes, the total and the code of such a sequence are those of ONE
 *              LZ4Stream.Read(count) over the concatenated source, however it was cut.  An interactive read that starves has
 *              delivered nothing.  With final[s] != 0, no byte left at a chunk boundary is the clean end (the read ends with what it
 *              has) and running out inside a header or a payload is K4LZ4_LEGACY_END_OF_STREAM -- which, from running out, occurs
 *              only with final.
 * not starved  need[s] == 0 and consumed[s] <= srcLen[s]: present the unconsumed rest first in the next call.  Nothing of an
 *              incomplete field is kept then.  A read satisfied exactly at a chunk's end does not consume the next header byte;
 *              count 0 consumes nothing.
 * defects      come when their bytes do, with the codes of the calls above in their order: C > U (END_OF_STREAM) and C < 0
 *              (OVERFLOW) in the call that completes the header; everything else (passes != 0, U > 255 C + 32, U > maxBlockSize, a
 *              payload that does not decode to U) in the call that hands over the payload's last byte.  The payload of a chunk that
 *              is refused whatever its bytes are (U > maxBlockSize, passes != 0) is counted, not kept.  consumed[s] of a failing
 *              call is unspecified; a failed stream stays failed and touches nothing.
 * count[s] < 0 leaves the stream untouched (outLen, consumed, need 0).
 *
 * k4lz4_legacy_read_fed_batch: store is a device pointer, every other pointer a host pointer; only the pieces go up, through the
 * context's staging buffers; dst, outLen, consumed and need come back.  Synchronous.  _device: every pointer a device pointer,
 * maxCount as above (<= 0: the general reader alone); enqueues on `stream` and returns, nothing is read back.  The direct path
 * takes streams that read (not interactive) with nothing pending and a stash that is empty or that the piece completes: the kept
 * chunk is completed from the head of the piece and goes through the batch decoder as the first row, the chunks wholly in the piece
 * follow; where those do not satisfy the count the piece's tail is kept and the read is left starved. */
#define K4LZ4_LREADER_FED 1                /* k4lz4_legacy_reader.flags */
K4LZ4_API int k4lz4_legacy_reader_init_fed(k4lz4_legacy_reader *r, int maxBlockSize);
K4LZ4_API int k4lz4_legacy_read_fed_batch(k4lz4_ctx *ctx, const k4lz4_legacy_reader *r, uint8_t *store, const uint64_t *storeOff,
                                          const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, const int64_t *final,
                                          uint8_t *dst, const uint64_t *dstOff, const int64_t *count, int64_t *outLen,
                                          int64_t *consumed, int64_t *need, int64_t n, int op, int flags);
K4LZ4_API int k4lz4_legacy_read_fed_batch_device(k4lz4_ctx *ctx, const k4lz4_legacy_reader *r, uint8_t *store, const uint64_t *storeOff,
                                                 const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen,
                                                 const int64_t *final, uint8_t *dst, const uint64_t *dstOff, const int64_t *count,
                                                 int64_t *outLen, int64_t *consumed, int64_t *need, int64_t n, int op, int flags,
                                                 int64_t maxCount, void *stream);

/* ---- Many open ILZ4Decoders advanced per call -------------------------------------------------------------
 * Stream s is one decoder as LZ4Decoder.Create(chaining, blockSize, extraBlocks) makes it (Encoders/LZ4Decoder.cs): an
 * LZ4ChainDecoder (Encoders/LZ4ChainDecoder.cs), or without chaining an LZ4BlockDecoder (Encoders/LZ4BlockDecoder.cs).  Its state
 * and its ring buffer live in a caller-owned DEVICE store of k4lz4_chain_decoder_store_bytes(d) bytes at store + storeOff[s]
 * (256-byte aligned), made a fresh decoder by K4LZ4_CDEC_RESET before its first use.  Results are byte for byte and defect for
 * defect the reference's decoder's for the same sequence of calls.
 *
 * The ring is the reference's: 65536 + (1 + extraBlocks) * B + 32 bytes for a chained decoder, B + 8 for an independent one, with
 * B = blockSize rounded up to a whole KiB, at least 1 KiB.  Prepare(blockSize) moves the last min(index, 64 KiB) bytes to the
 * front when index + blockSize would pass the end; Inject appends, or (64 KiB and longer) goes to the front, or moves the tail of
 * the history down first.  The block that follows sees as prefix the ring's bytes before the index, the last 64 KiB of them.  An
 * independent decoder holds one block: every Decode or Inject replaces what was there, Inject of nothing empties it.
 *
 * RUN.  Stream s owns records firstRec[s] .. firstRec[s] + nRec[s] - 1 of the record table, applied in order; nRec[s] == 0 leaves
 * the stream untouched (outLen 0).  Record r is src[recOff[r] .. + (recLen[r] & 0x7fffffff)): Decode(source, length,
 * recBlockSize[r]), or with bit 31 of recLen[r] set Inject(source, length).  recBlockSize may be NULL (every record 0).  Chained:
 * a blockSize <= 0 means B; otherwise it is what Prepare makes room for and the decode's capacity, and a value above
 * (1 + extraBlocks) * B + 32 is refused with K4LZ4_CDEC_BLOCK_SIZE (this library's own: the reference would write past its buffer
 * after CopyDict).  Independent: the capacity is B + 8 whatever the value, and a value above B is K4LZ4_CDEC_BLOCK_SIZE (the
 * reference's InvalidOperationException).  With K4LZ4_CDEC_DRAIN every record's bytes -- Inject's too -- are appended to
 * dst + dstOff[s] the way DecodeAndDrain calls Drain(target, -decoded, decoded) (Encoders/LZ4EncoderExtensions.cs:305-323; a
 * Decode record of length 0 then decodes nothing and leaves the decoder as it is, as there); without it nothing is copied and
 * BytesReady grows.
 *   recOut[r]   the bytes the record produced (0 is legal for a chained Decode), or its code; K4LZ4_CDEC_NOT_RUN for the records
 *               behind a failing one
 *   outLen[s]   the run's total, or the failing record's code
 * Codes, in the order the reference meets them: K4LZ4_CDEC_BLOCK_SIZE; K4LZ4_CDEC_DECODE (Decode threw: the block does not decode
 * within its capacity); K4LZ4_CDEC_INJECT (longer than max(B, 64 KiB), than B + 8 for an independent decoder);
 * K4LZ4_CDEC_TARGET (dstCap[s] has less room left than the record produced -- DecodeAndDrain returning false: the block IS decoded
 * and stays in the decoder, where a later drain fetches it; the records behind it are not run).  A decoder that reported a code is
 * not failed: it holds what the reference's object holds after the exception -- Prepare's move applied, the failing block not
 * counted, the earlier records of the run applied -- and the next call continues from there.  A store that was never reset
 * answers K4LZ4_CDEC_NO_DECODER.  Nothing outside [dstOff[s], dstOff[s] + dstCap[s]) and the stream's own store is written.
 *
 * RESET takes the records (dec[s]) and writes nothing but the stores (outLen 0); a RUN takes no records, the store remembers.
 * DRAIN is Drain(target, offset, length): offset[s] is relative to BytesReady (<= 0); outLen[s] is length[s], or K4LZ4_CDEC_RANGE
 * where the reference's range check throws.  It does not change the store.  Peek(offset) is a drain of -offset bytes.
 *
 * k4lz4_chain_decode_batch / k4lz4_chain_drain_batch / k4lz4_chain_decoder_query: store is a device pointer, every other pointer
 * a host pointer; sources and per-stream arrays go through the context's staging buffers; synchronous.  _device: every pointer
 * is a device pointer (dec and the per-stream arrays too); enqueues on `stream` -- one launch for a RUN, one for a RESET -- and
 * returns; nothing is read back.  K4LZ4_E_ARG (a store that is not 256-byte aligned, an unknown op or flag, a negative count, in
 * the host forms a record that k4lz4_chain_decoder_init did not make or a stream whose records lie outside the table) is decided
 * before anything is enqueued. */
typedef struct k4lz4_chain_decoder_settings {
    int32_t blockSize;
    int32_t extraBlocks;
    int32_t chaining;            /* 0: LZ4BlockDecoder (extraBlocks is ignored) */
} k4lz4_chain_decoder_settings;

typedef struct k4lz4_chain_decoder {
    int32_t blockSize;           /* as rounded: Mem.RoundUp(Math.Max(blockSize, 1 KiB), 1 KiB) */
    int32_t extraBlocks;         /* as applied: max(extraBlocks, 0); 0 without chaining */
    int32_t chaining;            /* 0 or 1 */
    int32_t reserved;
    int64_t storeBytes;          /* per stream */
} k4lz4_chain_decoder;

enum k4lz4_chain_decode_op { K4LZ4_CDEC_RUN = 0, K4LZ4_CDEC_RESET = 1 };
#define K4LZ4_CDEC_DRAIN 1                 /* flags */

#define K4LZ4_CDEC_DECODE       (-1)   /* Decode threw: the block does not decode within its capacity */
#define K4LZ4_CDEC_INJECT       (-2)   /* Inject threw: longer than the decoder takes */
#define K4LZ4_CDEC_BLOCK_SIZE   (-3)   /* the per-record blockSize was refused */
#define K4LZ4_CDEC_TARGET       (-4)   /* DecodeAndDrain returned false: the drain target is too small, the block stays */
#define K4LZ4_CDEC_NOT_RUN      (-5)   /* a record behind a failing one */
#define K4LZ4_CDEC_RANGE        (-6)   /* Drain threw: the range is not inside what is ready */
#define K4LZ4_CDEC_NO_DECODER   (-7)   /* the store was never reset */
#define K4LZ4_CDEC_DICT_INDEX   (-8)   /* k4lz4_chain_decoder_open_dictset_device: dictIdx[s] is outside the set; the store is untouched */

/* k4lz4_chain_decoder_query: int64 words per stream */
enum { K4LZ4_CDQ_BYTES_READY = 0,      /* BytesReady */
       K4LZ4_CDQ_BLOCK_SIZE = 1,       /* BlockSize */
       K4LZ4_CDQ_RECORDS = 2,          /* records applied */
       K4LZ4_CDQ_BYTES = 3,            /* the bytes they produced */
       K4LZ4_CDQ_CODE = 4,             /* the last run's code, 0 when it reported none */
       K4LZ4_CDQ_CHAINING = 5,
       K4LZ4_CDQ_EXTRA_BLOCKS = 6,
       K4LZ4_CDQ_MOVES = 7,            /* moves inside the ring (a statistic) */
       K4LZ4_CDQ_WORDS = 8 };

/* host arithmetic, no device needed.  K4LZ4_OK, or K4LZ4_E_ARG (NULL, or a ring above 0x7E000000 bytes) */
K4LZ4_API int k4lz4_chain_decoder_init(k4lz4_chain_decoder *d, const k4lz4_chain_decoder_settings *settings);
K4LZ4_API int64_t k4lz4_chain_decoder_store_bytes(const k4lz4_chain_decoder *d);
/* dec: n records (RESET; ignored by RUN, may be NULL).  nRecords: the record table's rows.  dst, dstOff, dstCap: with
 * K4LZ4_CDEC_DRAIN.  recOut: nRecords words, of which the rows owned by a stream with nRec[s] > 0 are written and no others;
 * outLen: n.  k4lz4_chain_drain_batch's host form stages per stream what the decoder holds at most, so a length out of range costs
 * no room.  src, recOff and recLen may be NULL when the record table is empty (every
 * nRec[s] is 0): the host form checks that against nRecords, the device form reads them only for a stream that has records. */
K4LZ4_API int k4lz4_chain_decode_batch(k4lz4_ctx *ctx, const k4lz4_chain_decoder *dec, uint8_t *store, const uint64_t *storeOff,
                                       const uint8_t *src, const uint64_t *recOff, const uint32_t *recLen, const int32_t *recBlockSize,
                                       int64_t nRecords, const uint64_t *firstRec, const uint32_t *nRec, uint8_t *dst,
                                       const uint64_t *dstOff, const uint64_t *dstCap, int32_t *recOut, int64_t *outLen, int64_t n,
                                       int op, int flags);
K4LZ4_API int k4lz4_chain_decode_batch_device(k4lz4_ctx *ctx, const k4lz4_chain_decoder *dec, uint8_t *store, const uint64_t *storeOff,
                                              const uint8_t *src, const uint64_t *recOff, const uint32_t *recLen,
                                              const int32_t *recBlockSize, const uint64_t *firstRec, const uint32_t *nRec, uint8_t *dst,
                                              const uint64_t *dstOff, const uint64_t *dstCap, int32_t *recOut, int64_t *outLen, int64_t n,
                                              int op, int flags, void *stream);
K4LZ4_API int k4lz4_chain_drain_batch(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, const int64_t *offset,
                                      const int64_t *length, uint8_t *dst, const uint64_t *dstOff, int64_t *outLen, int64_t n);
K4LZ4_API int k4lz4_chain_drain_batch_device(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, const int64_t *offset,
                                             const int64_t *length, uint8_t *dst, const uint64_t *dstOff, int64_t *outLen, int64_t n,
                                             void *stream);
/* out[s * K4LZ4_CDQ_WORDS + k] */
K4LZ4_API int k4lz4_chain_decoder_query(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out);
K4LZ4_API int k4lz4_chain_decoder_query_device(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out,
                                               void *stream);

/* ---- Many open ILZ4Encoders advanced per call -------------------------------------------------------------
 * Stream s is one encoder as LZ4Encoder.Create(chaining, level, blockSize, extraBlocks) makes it (Encoders/LZ4Encoder.cs): without
 * chaining an LZ4BlockEncoder(level, blockSize), with chaining below L03_HC an LZ4FastChainEncoder(blockSize, extraBlocks), from
 * L03_HC on an LZ4HighChainEncoder(level, blockSize, extraBlocks).  B is blockSize rounded up to a whole KiB, at least 1 KiB, and
 * extraBlocks at least 0 (LZ4EncoderBase's constructor); the HC level is clamped to L03_HC .. L12_MAX (LZ4HighChainEncoder.cs).
 * Every block is byte for byte what the reference's encoder object writes for the same sequence of calls.
 *
 * k4lz4_chain_encoder is the per-stream record, in HOST memory, owned by the caller: the settings as rounded and the counters
 * that follow from lengths alone (_inputIndex, _inputPointer, the bytes taken, the fast chain's currentOffset / dictSize, the
 * blocks emitted).  A call advances them without waiting for the device.  The bytes live in a caller-owned DEVICE store of
 * k4lz4_chain_encoder_store_bytes(e) bytes at store + storeOff[s] (256-byte aligned): for a chained fast stream its
 * k4lz4_fast_chain_state, then the ring -- 65536 + (1 + extraBlocks) * B + 32 bytes chained, B + 32 independent, and 8 more as the
 * reference allocates.  It needs no initialisation.  After a run the ring holds what the reference's InputBuffer holds, from 0 to
 * _inputPointer.
 *
 * RUN.  Stream s owns records firstRec[s] .. firstRec[s] + nRec[s] - 1 of the record table, applied in order; nRec[s] == 0 leaves
 * the stream untouched (outLen 0).  Record r is one TopupAndEncode(src[recOff[r] .. + recLen[r]), forceEncode, allowCopy)
 * (Encoders/LZ4EncoderExtensions.cs:117-210), its two switches the bits K4LZ4_CENC_FORCE and K4LZ4_CENC_ALLOW_COPY of recFlags[r];
 * recLen[r] == 0 with K4LZ4_CENC_FORCE is FlushAndEncode.  Without FORCE the record encodes only when BytesReady == B, with it
 * from 1 byte: a block shorter than B may stand in the middle of a chained stream.
 *   recLoaded[r]  what Topup took; less than recLen[r] when the block fills -- the caller offers the rest in a later record
 *   recOut[r]     the reference's `encoded` before the sign is dropped: > 0 an encoded block, < 0 the block stored raw under
 *                 allowCopy (its length negated), 0 nothing encoded.  The action: 0 -> None (recLoaded 0) or Loaded; > 0 -> Encoded;
 *                 < 0 -> Copied
 *   outLen[s]     the run's total, or a code
 * The run's blocks are appended to dst + dstOff[s] in record order, each right behind the one before it (the reference's caller
 * advancing its target by |encoded|).  Nothing outside [dstOff[s], dstOff[s] + dstCap[s]) and the stream's own store is written.
 *
 * K4LZ4_CENC_TARGET: dstCap[s] is below k4lz4_chain_encode_bound(e, the run) -- the sum, over the blocks the run will encode (which
 * follow from lengths alone), of k4lz4_compress_bound(len), or of len where the record allows copying.  The stream keeps its
 * record and store and none of the run's Topups is applied (recLoaded and recOut 0).  This rule is this library's own and stricter
 * than the reference, which throws only when a block really does not fit its target.  It is decided on the host before anything is
 * enqueued, and so is K4LZ4_E_ARG at call level: a chained fast stream under K4LZ4_FLAG_X32 / Enforce32 (independent encoders
 * honour it, as k4lz4_encode_batch does), a chained stream past 2 GB (the encoders' renormalisation), a store that is not 256-byte
 * aligned, unknown flags or record flags, a record longer than INT32_MAX, records outside the table.  A call-level failure leaves
 * every record as it was.
 *
 * RESET makes fresh encoders: it zeroes the records' counters (and a chained fast stream's state in the store).  What an
 * ILZ4Encoder answers -- BytesReady = pointer - index, BlockSize -- is host arithmetic on the record and needs no call.
 *
 * k4lz4_chain_encode_batch: store is a device pointer, every other pointer a host pointer; sources and the target go through the
 * context's staging buffers; synchronous.  _device: src, store, dst, recLoaded, recOut and outLen are device pointers, the plan
 * arrays (enc, storeOff, recOff, recLen, recFlags, firstRec, nRec, dstOff, dstCap) host arrays; it enqueues on `stream` and returns
 * without waiting for its own work.  It waits for the upload of the previous call's plan (the context's own event) before it
 * rewrites it, and each chained group for the previous chained block table, as k4lz4_frame_write_batch_device does.  The launch
 * count depends on the (kind, level) groups in the call, not on the number of streams. */
typedef struct k4lz4_chain_encoder_settings {
    int32_t chaining;
    int32_t level;               /* k4lz4_level */
    int32_t blockSize;
    int32_t extraBlocks;
} k4lz4_chain_encoder_settings;

typedef struct k4lz4_chain_encoder {
    int32_t kind;                /* 0 LZ4BlockEncoder, 1 LZ4HighChainEncoder, 2 LZ4FastChainEncoder */
    int32_t level;               /* as clamped (HC); 0 for the fast chain */
    int32_t blockSize;           /* as rounded */
    int32_t extraBlocks;         /* as applied; 0 without chaining */
    int32_t ringBytes;           /* _inputLength */
    int32_t index, pointer;      /* _inputIndex, _inputPointer */
    uint32_t currentOffset, dictSize; /* chained fast: LZ4_stream_t's two indices */
    int32_t reserved;
    int64_t taken;               /* bytes Topup took so far */
    int64_t blocks;              /* blocks emitted so far */
    int64_t storeBytes;          /* per stream */
} k4lz4_chain_encoder;

enum k4lz4_chain_encode_op { K4LZ4_CENC_RUN = 0, K4LZ4_CENC_RESET = 1 };
#define K4LZ4_CENC_FORCE       1          /* recFlags */
#define K4LZ4_CENC_ALLOW_COPY  2
#define K4LZ4_CENC_TARGET      (-1)       /* dstCap[s] is below k4lz4_chain_encode_bound */

/* host arithmetic, no device needed.  K4LZ4_OK, or K4LZ4_E_ARG (NULL, a block size above the input size limit) */
K4LZ4_API int k4lz4_chain_encoder_init(k4lz4_chain_encoder *e, const k4lz4_chain_encoder_settings *settings);
K4LZ4_API int64_t k4lz4_chain_encoder_store_bytes(const k4lz4_chain_encoder *e);
/* the most a run of nRec records can emit for the stream */
K4LZ4_API int64_t k4lz4_chain_encode_bound(const k4lz4_chain_encoder *e, const uint32_t *recLen, const uint32_t *recFlags, int64_t nRec);
/* the record as the run would leave it, and what each record loads and whether it encodes (blockLen[r]: the block's length, 0 none):
 * the host's model alone, nothing runs.  `after`, recLoaded and blockLen may be NULL */
K4LZ4_API int k4lz4_chain_encode_plan(const k4lz4_chain_encoder *e, const uint32_t *recLen, const uint32_t *recFlags, int64_t nRec,
                                      k4lz4_chain_encoder *after, int32_t *recLoaded, int32_t *blockLen);
/* the two pieces of host arithmetic the call is laid out with, for checking them against each other (no device needed); a row
 * is four int64 words: start, length, the HC context's dictLimit or the fast chain's dictSize in front of the block, dictSmall.
 * k4lz4_chain_encode_blocks: the blocks the run would encode, as the record model yields them, in the coordinates of the window [the
 * ring | the bytes the run loads] (dictLimit: the window position of the ring's first byte) -> the number of blocks (at most maxRows
 * rows are written), or -1.  k4lz4_chain_table_rows: the chained encoders' block table for explicit block lengths -- kind 1 HC,
 * 2 fast; the content's first dictLen bytes are what the ring holds. */
K4LZ4_API int64_t k4lz4_chain_encode_blocks(const k4lz4_chain_encoder *e, const uint32_t *recLen, const uint32_t *recFlags, int64_t nRec,
                                            int64_t *rows, int64_t maxRows);
K4LZ4_API int k4lz4_chain_table_rows(int kind, int64_t dictLen, int64_t currentOffset, const int32_t *len, int64_t n, int32_t blockSize,
                                     int32_t extraBlocks, int64_t *rows);
/* flags: K4LZ4_FLAG_X32.  nRecords: the record table's rows.  recLoaded, recOut: nRecords words, of which the rows owned by a
 * stream with nRec[s] > 0 are written and no others */
K4LZ4_API int k4lz4_chain_encode_batch(k4lz4_ctx *ctx, k4lz4_chain_encoder *enc, uint8_t *store, const uint64_t *storeOff,
                                       const uint8_t *src, const uint64_t *recOff, const uint32_t *recLen, const uint32_t *recFlags,
                                       int64_t nRecords, const uint64_t *firstRec, const uint32_t *nRec, uint8_t *dst,
                                       const uint64_t *dstOff, const uint64_t *dstCap, int32_t *recLoaded, int32_t *recOut,
                                       int64_t *outLen, int64_t n, int op, int flags);
K4LZ4_API int k4lz4_chain_encode_batch_device(k4lz4_ctx *ctx, k4lz4_chain_encoder *enc, uint8_t *store, const uint64_t *storeOff,
                                              const uint8_t *src, const uint64_t *recOff, const uint32_t *recLen,
                                              const uint32_t *recFlags, int64_t nRecords, const uint64_t *firstRec, const uint32_t *nRec,
                                              uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int32_t *recLoaded,
                                              int32_t *recOut, int64_t *outLen, int64_t n, int op, int flags, void *stream);

/* ---- Chained encoders and decoders opened from a prepared dictionary set -----------------------------------
 * "Open" makes fresh streams, as RESET does, and primes those that name an entry of a k4lz4_dict_set -- dictIdx[s] = e >= 0; -1: a
 * fresh stream without a dictionary -- in one call and one launch per side.  d = min(dictLen, 65536) is what the entry keeps.
 *
 * Encoder.  Stream s is LZ4Encoder.Create(...)'s object with this done before its first TopupAndEncode: the kept bytes copied to
 * ring positions [0, d), _inputIndex = _inputPointer = d, and LZ4_loadDict(stream, ring, d) (fast chain) or
 * LZ4_loadDictHC(stream, ring, d) (HC chain, the level kept).  The dictionary is the stream's PREFIX, not an external dictionary:
 * the first block follows it in the ring, may extend a match backwards into it, and it stays in the window until 64 KiB of content
 * have pushed it out.  Fast chain: an entry that keeps fewer than 8 bytes is the empty dictionary -- the ring stays empty, the state
 * is the zeroed table with currentOffset 65536 and dictSize 0; otherwise index = pointer = dictSize = d and currentOffset = 65536,
 * and the store's k4lz4_fast_chain_state is the set's table for the entry with those two words.  HC chain: every length counts,
 * down to one byte (the tables are a function of the ring's bytes), at K4LZ4_L03_HC .. K4LZ4_L09_HC; a stream at K4LZ4_L10_OPT or
 * above is refused with an entry (the optimal parser has no witness behind a dictionary yet) and opens without
 * one.  A later plain RESET gives a fresh stream without a dictionary.  A set of either family serves HC encoders and decoders; a
 * chained fast encoder needs K4LZ4_DICT_FAST in the set.
 *   k4lz4_chain_encoder_open_plan   host arithmetic, no device: the record as open leaves it for an entry of dictLen bytes
 *                                   (dictLen < 0: no dictionary).  K4LZ4_E_ARG, the record as it was: NULL, not a record of
 *                                   k4lz4_chain_encoder_init, dictLen >= 0 on an independent encoder or at K4LZ4_L10_OPT or above
 *   k4lz4_chain_encoder_open_dictset[_device]   enc, storeOff and dictIdx are host arrays in both forms, store a device pointer.  The
 *                                   host form is synchronous, _device enqueues on `stream` and returns; the records are advanced at
 *                                   once.  K4LZ4_E_ARG before anything is enqueued, every record as it was: an index outside
 *                                   [-1, nDict); an index >= 0 on an independent encoder (LZ4BlockEncoder has no dictionary), on
 *                                   a stream at K4LZ4_L10_OPT or above, or on a chained fast stream when the set lacks the
 *                                   fast family or the process is under Enforce32 (k4lz4_set_enforce32; the call takes no flags); a
 *                                   set on another device than the context; a misaligned store; a record that
 *                                   k4lz4_chain_encoder_init did not make.
 *
 * Decoder.  Stream s is LZ4Decoder.Create(...)'s object after one Inject(kept bytes): geometry, BytesReady, the counters and the
 * code (K4LZ4_CDEC_INJECT for an independent decoder whose B + 8 is shorter than the entry) are that record's.  outLen[s] is the
 * bytes injected (0 for -1 or an empty entry) or the code.
 *   k4lz4_chain_decoder_open_dictset          dec and dictIdx are host arrays; an index outside [-1, nDict) is K4LZ4_E_ARG up front
 *   k4lz4_chain_decoder_open_dictset_device   dec, storeOff, dictIdx and outLen are device pointers; such an index leaves that store
 *                                   untouched, sets outLen[s] = K4LZ4_CDEC_DICT_INDEX and makes the next synchronising call return
 *                                   K4LZ4_E_ARG (as k4lz4_decode_dictset_batch_device) */
K4LZ4_API int k4lz4_chain_encoder_open_plan(k4lz4_chain_encoder *e, int32_t dictLen);
K4LZ4_API int k4lz4_chain_encoder_open_dictset(k4lz4_ctx *ctx, k4lz4_chain_encoder *enc, uint8_t *store, const uint64_t *storeOff,
                                               const int32_t *dictIdx, const k4lz4_dict_set *set, int64_t n);
K4LZ4_API int k4lz4_chain_encoder_open_dictset_device(k4lz4_ctx *ctx, k4lz4_chain_encoder *enc, uint8_t *store, const uint64_t *storeOff,
                                                      const int32_t *dictIdx, const k4lz4_dict_set *set, int64_t n, void *stream);
K4LZ4_API int k4lz4_chain_decoder_open_dictset(k4lz4_ctx *ctx, const k4lz4_chain_decoder *dec, uint8_t *store, const uint64_t *storeOff,
                                               const int32_t *dictIdx, const k4lz4_dict_set *set, int64_t *outLen, int64_t n);
K4LZ4_API int k4lz4_chain_decoder_open_dictset_device(k4lz4_ctx *ctx, const k4lz4_chain_decoder *dec, uint8_t *store,
                                                      const uint64_t *storeOff, const int32_t *dictIdx, const k4lz4_dict_set *set,
                                                      int64_t *outLen, int64_t n, void *stream);

/* ---- frames with a predefined dictionary read against a set ---------------------------------------------------
 * The frame reader above (k4lz4_frame_sizes*, k4lz4_decode_frames*) with a k4lz4_dict_set beside it: frames whose FLG has the
 * dictionary bit (what `lz4 -D` and LZ4F_compressFrame_usingCDict write) are decoded against an entry of the set instead of being
 * reported as K4LZ4_FRAME_DICTIONARY.  The set stays as it is; the ids are the call's: dictIds is a HOST array of set->nDict
 * uint32_t in both forms, entry e answers to DictID dictIds[e], and it is copied to the context's scratch per call.
 *   - a frame's DictID resolves to the FIRST entry whose id equals it (duplicate ids: the later entries are never chosen);
 *   - a frame without the bit decodes without a dictionary, as in the plain calls;
 *   - a DictID that resolves to nothing is K4LZ4_FRAME_DICTIONARY at its place in the defect order: after the header checksum
 *     (which covers the DictID: a flipped DictID byte is K4LZ4_FRAME_HEADER_SUM, a header cut inside it K4LZ4_FRAME_EOF), before
 *     the first block.  No code is new.
 * Independent-block frames: every compressed block is decoded against the entry's kept bytes (the last 64 KiB of the dictionary)
 * as an external dictionary, in parallel and straight into place; blocks never see each other.  Chained frames: in order, one
 * wave per frame, the history being the kept bytes followed by the output so far.  An offset that reaches before the first kept
 * byte is K4LZ4_FRAME_BLOCK.  Content checksum and ContentLength cover the content only.  Result codes, defect order and what
 * may be written are those of k4lz4_decode_frames_device.
 * outDictIdx (optional, NULL: not wanted): per frame the entry it resolved to, -1 for none (no bit, a header defect, unknown id).
 * K4LZ4_E_ARG before anything is enqueued: a set on another device than the context; NULL dictIds with a non-NULL set.  A NULL
 * set (dictIds is then ignored) behaves exactly like the plain call: DictID frames report K4LZ4_FRAME_DICTIONARY.
 * The _device forms take device pointers for everything but dictIds; k4lz4_decode_frames_dictset_device waits for `stream` once
 * like k4lz4_decode_frames_device.  In-order work is dealt to two decoders: frames without an entry (no DictID, or an entry of no bytes)
 * keep k4lz4_decode_chain_batch_device's kernels, frames with one go to a one-wave kernel bounded at sixteen waves per compute unit
 * (measured on 4096 chained single-block frames: 1.18 ms against the plain kernels' 1.05 ms).  Only when a chained frame resolved to
 * an entry does that kernel get windows in the context's scratch, grow-only: 64 KiB per frame of the call up to sixteen per compute
 * unit (256 MiB on a 256-CU device).
 * Writing such frames needs no call of its own: the header is FLG bit 0 and the DictID (LE32) after the content size -- at most 14
 * descriptor bytes, which fit the 16-byte hdr rows of k4lz4_frame_assemble_device -- and the blocks are those of
 * k4lz4_encode_dictset_batch with the allowCopy rule (independent frames) or of a chain encoder opened from the entry with
 * k4lz4_chain_encoder_open_dictset (chained frames); frames.py composes them.
 * Refused, exactly: by every call that takes no set, and by these with a NULL set, every DictID (K4LZ4_FRAME_DICTIONARY) -- the
 * incremental frame readers have calls of their own that take one (k4lz4_frame_read_dictset_batch, k4lz4_frame_read_fed_dictset_batch
 * below); by the incremental frame writer (k4lz4_frame_write_batch and its _device form) the
 * dictionary bit, with or without a set anywhere; by the encoders the writer is made of, K4LZ4_L10_OPT .. K4LZ4_L12_MAX with a
 * dictionary and the 32-bit engine (K4LZ4_FLAG_X32, k4lz4_set_enforce32). */
/* The allowCopy rule (LZ4EncoderBase.Encode(allowCopy: true)) behind an encoder that takes no flags, on device pointers: block i
 * with outLen[i] >= srcLen[i] is stored raw (its srcLen[i] bytes copied to dst + dstOff[i], outLen[i] = -srcLen[i]; 0 when
 * dstCap[i] is too small for that), outLen[i] <= 0 becomes 0 -- what K4LZ4_FLAG_ALLOW_COPY does behind k4lz4_encode_batch_device.
 * The writer of dictionary frames on device-resident contents runs it behind k4lz4_encode_dictset_batch_device.  Asynchronous. */
K4LZ4_API int k4lz4_allow_copy_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                            uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n,
                                            void *stream);
K4LZ4_API int k4lz4_frame_sizes_dictset_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen,
                                               int64_t n, uint64_t *outSize, int32_t *outStatus, int32_t *outDictIdx,
                                               const k4lz4_dict_set *set, const uint32_t *dictIds, void *stream);
K4LZ4_API int k4lz4_decode_frames_dictset_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen,
                                                 int64_t n, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen,
                                                 const k4lz4_dict_set *set, const uint32_t *dictIds, void *stream);
K4LZ4_API int k4lz4_frame_sizes_dictset(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                                        uint64_t *outSize, int32_t *outStatus, int32_t *outDictIdx, const k4lz4_dict_set *set,
                                        const uint32_t *dictIds);
K4LZ4_API int k4lz4_decode_frames_dictset(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                                          uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen,
                                          const k4lz4_dict_set *set, const uint32_t *dictIds);

/* ---- the incremental frame readers against a set --------------------------------------------------------------
 * k4lz4_frame_read_batch[_device] and k4lz4_frame_read_fed_batch[_device] with a k4lz4_dict_set beside them:
 * each call is its counterpart's argument list with `set, dictIds` added (in front of `stream` in the _device forms), and everything
 * said of the counterpart holds -- ops, flags, codes, what is written, maxCount, the two ways through a READ, starving and need.
 * Records and stores are the counterparts': k4lz4_frame_reader_store_bytes does not change, a store made for one works with the other.
 * dictIds is a HOST array of set->nDict uint32_t in both forms and goes up per call through the context (the caller may free it when
 * the call returns; the _device forms stay asynchronous).  The rules are 4.24's:
 *   - a frame's DictID resolves to the FIRST entry whose id equals it; a frame without the dictionary bit is read as in the plain calls;
 *   - a DictID nothing answers to is K4LZ4_FRAME_DICTIONARY where the plain calls report every DictID: behind the header checksum (a
 *     flipped DictID byte is K4LZ4_FRAME_HEADER_SUM), before the first block; an OPEN reports it too.  A source that ends inside the
 *     DictID is K4LZ4_FRAME_EOF; a fed stream that is not final starves there with need the bytes that complete the header;
 *   - independent-block frames: every compressed block is decoded against the entry's kept bytes (the last 64 KiB) as an external
 *     dictionary, on both ways through a READ; chained frames: the kept bytes are the history in front of the first block, as
 *     LZ4ChainDecoder's after Inject.  The kept bytes are never delivered, never counted in K4LZ4_FRQ_BYTES_READ and never enter the
 *     content checksum.  An offset that reaches before the first kept byte is K4LZ4_FRAME_BLOCK; an entry of no bytes reads as a
 *     plain frame (whose id still has to resolve).
 * The store remembers which entry the open frame resolved to, from the header to the frame's end; a source of several frames may
 * name another entry, or none, per frame.  THE CALLER PASSES THE SAME SET AND THE SAME IDS FOR AS LONG AS A FRAME IS OPEN.  A call that
 * brings a set which does not have the remembered entry fails the stream with K4LZ4_FRAME_DICTIONARY and reads nothing of the set;
 * a set that has it but holds other bytes there is not noticed.
 * A NULL set (dictIds is then ignored) makes each call exactly its counterpart.  K4LZ4_E_ARG before anything is enqueued: a set on
 * another device than the context, NULL dictIds with a set, and what the counterpart refuses (a record of the other kind).
 * No status code and no query word is new.  Not here: the incremental frame writer with a dictionary. */
K4LZ4_API int k4lz4_frame_read_dictset_batch(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff,
                                             const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst,
                                             const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t n, int op, int flags,
                                             const k4lz4_dict_set *set, const uint32_t *dictIds);
K4LZ4_API int k4lz4_frame_read_dictset_batch_device(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff,
                                                    const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst,
                                                    const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t n, int op,
                                                    int flags, int64_t maxCount, const k4lz4_dict_set *set, const uint32_t *dictIds,
                                                    void *stream);
K4LZ4_API int k4lz4_frame_read_fed_dictset_batch(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff,
                                                 const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, const int64_t *final,
                                                 uint8_t *dst, const uint64_t *dstOff, const int64_t *count, int64_t *outLen,
                                                 int64_t *consumed, int64_t *need, int64_t n, int op, int flags,
                                                 const k4lz4_dict_set *set, const uint32_t *dictIds);
K4LZ4_API int k4lz4_frame_read_fed_dictset_batch_device(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store,
                                                        const uint64_t *storeOff, const uint8_t *src, const uint64_t *srcOff,
                                                        const uint64_t *srcLen, const int64_t *final, uint8_t *dst, const uint64_t *dstOff,
                                                        const int64_t *count, int64_t *outLen, int64_t *consumed, int64_t *need, int64_t n,
                                                        int op, int flags, int64_t maxCount, const k4lz4_dict_set *set,
                                                        const uint32_t *dictIds, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* K4LZ4_H */
