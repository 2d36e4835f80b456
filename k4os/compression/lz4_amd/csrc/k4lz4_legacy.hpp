/*
 * k4lz4_legacy.hpp -- lz4net's legacy formats (K4os.Compression.LZ4.Legacy) on top of the block kernels.
 *
 * Wrapped buffer (LZ4Wrapper.cs): [u32 U][u32 C][block], or [u32 U][u32 U][raw bytes] when the block is not shorter than U;
 * U = 0 is eight zero bytes.  As for pickles (k4lz4_pickle.hpp), "encode with cap U, raw when the result is <= 0 or >= U"
 * reduces to "compressed iff the unlimited size C < U": the encoder writes straight into dst + 8 with cap U - 1.
 *   k4_wrap_prep_kernel        encoder slot = dstOff + 8, cap U - 1 (0: empty message or a slot too small)
 *   k4_wrap_finish_kernel      one wave per message: both words, or the raw copy
 *   k4_unwrap_sizes_kernel     one thread per buffer: LZ4Wrapper.Unwrap's checks -> the result length or a code, and the route
 *                              (raw copy, or the batch decoder with cap = outLen)
 *   k4_unwrap_finish_kernel    one wave per buffer: the raw copies; what LZ4Codec.Decode returned for the others
 *
 * Legacy stream (LZ4Stream.cs): chunks `varint(flags) varint(U) [varint(C) if compressed] payload`, flags Compressed = 1,
 * HighCompression = 2, every chunk compressed on its own.
 *   writer  k4_lw_count_kernel (chunks and arena bytes per stream) -> k4_legacy_scan_kernel (x2) -> one wait -> k4_lw_fill_kernel
 *           (a row per chunk) -> the block encoder into the arena (cap U - 1) -> k4_lw_header_kernel (record bytes per chunk)
 *           -> k4_legacy_scan_kernel (record offsets) -> k4_lw_assemble_kernel (wave per chunk) -> k4_lw_finish_kernel
 *   reader  k4_lr_walk_kernel (thread per stream: every check of AcquireNextChunk in stream order, never outside the stream)
 *           -> k4_legacy_scan_kernel -> one wait -> k4_lr_fill_kernel (a row per chunk that produces bytes) -> the batch
 *           decoder straight into place -> k4_lr_copy_kernel (raw chunks, wave per chunk; a chunk that did not decode or fit
 *           -> atomicMin of the stream's first defect in stream order) -> k4_lr_finish_kernel
 */
#pragma once
#include "k4lz4_decode.hpp"

namespace k4 {

/* per-item codes (include/k4lz4.h K4LZ4_LEGACY_*) */
constexpr int LG_END_OF_STREAM = -1, LG_OVERFLOW = -2, LG_NOT_SUPPORTED = -3, LG_INVALID_DATA = -4, LG_ARGUMENT = -5,
              LG_CAPACITY = -6, LG_NOT_ENCODED = -7;

__device__ __forceinline__ void poke32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

/* ---- Wrap ------------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void k4_wrap_prep_kernel(BatchArgs a, uint64_t *encOff, int32_t *encCap)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.n) return;
    const int U = a.srcLen[b];
    encOff[b] = a.dstOff[b] + 8u;
    encCap[b] = (U > 0 && (long long)a.dstCap[b] >= 8ll + U) ? U - 1 : 0;
}

constexpr int WRAP_FINISH_WAVES_PER_WG = 4;
/* outLen = 8 + payload, or -1 (slot too small; an HC block not encoded for want of reserved scratch) */
__global__ __launch_bounds__(64 * WRAP_FINISH_WAVES_PER_WG) void k4_wrap_finish_kernel(BatchArgs a, const int32_t *encLen)
{
    const int lane = lane_id();
    const long long b = (long long)blockIdx.x * WRAP_FINISH_WAVES_PER_WG + (long long)uni(threadIdx.x >> 6);
    if (b >= a.n) return;
    const int U = a.srcLen[b] > 0 ? a.srcLen[b] : 0;
    uint8_t *dst = a.dst + a.dstOff[b];
    int r;
    if ((long long)a.dstCap[b] < 8ll + U) r = -1;
    else if (U > 1 && encLen[b] == HC_NO_SCRATCH) r = -1;
    else {
        const int C = U > 1 ? encLen[b] : 0;
        const bool raw = C <= 0 || C >= U;                       /* LZ4Wrapper.cs:71 */
        if (raw) wave_copy(dst + 8, a.src + a.srcOff[b], (uint32_t)U, lane);
        if (lane == 0) {
            poke32(dst, (uint32_t)U);
            poke32(dst + 4, (uint32_t)(raw ? U : C));
        }
        r = 8 + (raw ? U : C);
    }
    if (lane == 0) a.outLen[b] = r;
}

/* ---- Unwrap ----------------------------------------------------------------------------------------------------------- */
/* LZ4Wrapper.Unwrap on one buffer of `len` bytes: the result length (>= 0) or a code; *decode: the payload goes through
 * LZ4Codec.Decode (inLen < outLen), *inLen: the payload length */
__host__ __device__ __forceinline__ long long unwrap_plan(const uint8_t *p, long long len, bool *decode, int *inLenOut)
{
    *decode = false; *inLenOut = 0;
    if (len < 8) return LG_ARGUMENT;                                      /* :111-112 */
    const int outLen = (int)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    const int inLen = (int)((uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24);
    if ((long long)inLen > len - 8) return LG_ARGUMENT;                  /* :116-117 */
    *inLenOut = inLen;
    if (inLen >= outLen) return inLen < 0 ? LG_OVERFLOW : inLen;          /* :121-126, new byte[inLen] */
    if (outLen < 0) return LG_OVERFLOW;                                   /* new byte[outLen] */
    if (inLen < 0) return LG_ARGUMENT;                                    /* LZ4Codec.Decode -> Validate */
    *decode = true;
    return outLen;
}

struct UnwrapArgs {
    const uint8_t *src;
    const uint64_t *srcOff;
    const int32_t *srcLen;
    const int32_t *dstCap;
    long long n;
    int32_t *outLen;          /* result length or K4LZ4_LEGACY_* */
    uint64_t *decOff;         /* batch decoder: payload */
    int32_t *decLen;          /* ... its length, 0: not decoded here */
    int32_t *decCap;          /* ... cap = outLen */
};

__global__ __launch_bounds__(256) void k4_unwrap_sizes_kernel(UnwrapArgs a)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.n) return;
    bool dec;
    int in;
    const int len = a.srcLen[b];
    long long r = unwrap_plan(a.src + a.srcOff[b], len, &dec, &in);
    if (a.dstCap && r > (long long)a.dstCap[b]) { r = LG_CAPACITY; dec = false; }
    a.outLen[b] = (int32_t)r;
    if (a.decOff) {
        a.decOff[b] = a.srcOff[b] + 8u;
        a.decLen[b] = (dec && r >= 0) ? in : 0;                  /* inLen 0: LZ4Codec.Decode returns 0 without decoding */
        a.decCap[b] = (dec && r >= 0) ? (int32_t)r : 0;
    }
}

/* raw results are copied; `decoded` = what LZ4Codec.Decode returned (the copied length for raw results, 0 for failed items) */
__global__ __launch_bounds__(256) void k4_unwrap_finish_kernel(const uint8_t *src, const uint64_t *srcOff, uint8_t *dst,
                                                               const uint64_t *dstOff, UnwrapArgs a, const int32_t *decOut,
                                                               int32_t *decoded)
{
    const int lane = lane_id();
    const long long b = (long long)blockIdx.x * 4 + (long long)uni(threadIdx.x >> 6);
    if (b >= a.n) return;
    const int r = a.outLen[b];
    int d = 0;
    if (r >= 0) {
        if (a.decCap[b] == 0 || r == 0) {                        /* raw (inLen >= outLen) */
            wave_copy(dst + dstOff[b], src + srcOff[b] + 8, (uint32_t)r, lane);
            d = r;
        } else if (a.decLen[b] == 0) {
            uint8_t *o = dst + dstOff[b];                        /* LZ4Codec.cs:108-109: nothing decoded into new byte[outLen] */
            for (uint32_t k = (uint32_t)lane; k < (uint32_t)r; k += 64) o[k] = 0;
            d = 0;
        } else {
            d = decOut[b] <= 0 ? -1 : decOut[b];                 /* LZ4Codec.cs:114 */
        }
    }
    if (lane == 0) decoded[b] = d;
}

/* ---- legacy stream: shared pieces ------------------------------------------------------------------------------------ */
constexpr int LEGACY_SCAN_THREADS = 256;

/* one workgroup: first[i] = sum of v before i, *total = the sum; 1024 values per step */
__global__ __launch_bounds__(LEGACY_SCAN_THREADS) void k4_legacy_scan_kernel(const uint64_t *v, uint64_t *first, long long n,
                                                                            unsigned long long *total)
{
    __shared__ unsigned long long wsum[LEGACY_SCAN_THREADS / 64];
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    unsigned long long carry = 0;
    for (long long base = 0; base < n; base += LEGACY_SCAN_THREADS * 4) {
        const long long i0 = base + (long long)threadIdx.x * 4;
        unsigned long long x4[4], s = 0;
        for (int k = 0; k < 4; k++) {
            x4[k] = i0 + k < n ? v[i0 + k] : 0u;
            s += x4[k];
        }
        unsigned long long x = s;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = __shfl_up(x, (unsigned)d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        unsigned long long before = 0, tot = 0;
        for (int w = 0; w < LEGACY_SCAN_THREADS / 64; w++) {
            if (w < wave) before += wsum[w];
            tot += wsum[w];
        }
        unsigned long long e = carry + before + x - s;
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) first[i0 + k] = e;
            e += x4[k];
        }
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__host__ __device__ __forceinline__ int varint_size(uint64_t v)
{
    int k = 1;
    while (v >= 0x80u) { v >>= 7; k++; }
    return k;
}
__device__ __forceinline__ uint8_t *put_varint(uint8_t *p, uint64_t v)   /* LZ4Stream.cs WriteVarInt */
{
    for (;;) {
        const uint8_t b = (uint8_t)(v & 0x7fu);
        v >>= 7;
        *p++ = (uint8_t)(b | (v == 0 ? 0 : 0x80));
        if (v == 0) return p;
    }
}

/* ---- legacy stream writer -------------------------------------------------------------------------------------------- */
struct LegacyWriteArgs {
    const uint8_t *src;
    const uint64_t *srcOff;         /* per stream */
    const uint64_t *srcLen;
    long long n;
    uint64_t bs;                    /* chunk size, >= 16 */
    int high;
    uint64_t *nch;                  /* per stream: chunks */
    uint64_t *pad;                  /* ... arena bytes */
    uint64_t *first;                /* ... first row */
    uint64_t *arenaOff;             /* ... first arena byte */
    long long rows;
    uint32_t *owner;                /* per row */
    uint64_t *cSrcOff;
    int32_t *cSrcLen;
    uint64_t *cEncOff;
    int32_t *cEncCap;
    int32_t *cEncLen;
    uint64_t *recLen;               /* record bytes */
    uint64_t *recOff;               /* exclusive scan of recLen over all rows */
};

__global__ __launch_bounds__(256) void k4_lw_count_kernel(LegacyWriteArgs a)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n) return;
    const uint64_t len = a.srcLen[s];
    a.nch[s] = (len + a.bs - 1) / a.bs;
    a.pad[s] = (len + 15u) & ~(uint64_t)15u;
}

/* the stream that owns row r: the last s with first[s] <= r (streams without chunks share their successor's first row) */
__device__ __forceinline__ long long owner_of(const uint64_t *first, long long n, uint64_t r)
{
    long long lo = 0, hi = n;                       /* first index with first[i] > r */
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (first[mid] <= r) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

/* a row per chunk: its source, its arena slot (the chunk's place in the stream's padded copy of the content), cap U - 1 */
__global__ __launch_bounds__(256) void k4_lw_fill_kernel(LegacyWriteArgs a)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.rows) return;
    const long long s = owner_of(a.first, a.n, (uint64_t)r);
    const uint64_t k = (uint64_t)r - a.first[s], at = k * a.bs, len = a.srcLen[s];
    const uint64_t U = len - at < a.bs ? len - at : a.bs;
    a.owner[r] = (uint32_t)s;
    a.cSrcOff[r] = a.srcOff[s] + at;
    a.cSrcLen[r] = (int32_t)U;
    a.cEncOff[r] = a.arenaOff[s] + at;
    a.cEncCap[r] = (int32_t)U - 1;
}

/* LZ4Stream.cs FlushCurrentChunk: a compressed chunk is C > 0 && C < U; the record's bytes follow from that */
__device__ __forceinline__ bool lw_compressed(int U, int encLen) { return U > 1 && encLen > 0 && encLen < U; }

__global__ __launch_bounds__(256) void k4_lw_header_kernel(LegacyWriteArgs a)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.rows) return;
    const int U = a.cSrcLen[r], C = a.cEncLen[r];
    const bool comp = lw_compressed(U, C);
    a.recLen[r] = 1u + (uint64_t)varint_size((uint64_t)U) + (comp ? (uint64_t)varint_size((uint64_t)C) + (uint64_t)C : (uint64_t)U);
}

/* stream s: records [first[s], first[s] + nch[s]) -- bytes from recOff[first] up to the end of its last record */
__device__ __forceinline__ uint64_t lw_stream_bytes(const LegacyWriteArgs &a, long long s)
{
    const uint64_t n = a.nch[s];
    if (!n) return 0;
    const uint64_t f = a.first[s], l = f + n - 1;
    return a.recOff[l] + a.recLen[l] - a.recOff[f];
}

__device__ __forceinline__ bool lw_not_encoded(const LegacyWriteArgs &a, long long r)
{
    return a.cSrcLen[r] > 1 && a.cEncLen[r] == HC_NO_SCRATCH;
}

/* one wave per chunk: its varints and its payload (the block from the arena, or the source bytes), packed into the stream's
 * slot when the whole stream fits */
__global__ __launch_bounds__(256) void k4_lw_assemble_kernel(LegacyWriteArgs a, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                                                             const uint8_t *arena)
{
    const int lane = lane_id();
    const long long r = (long long)blockIdx.x * 4 + (long long)uni(threadIdx.x >> 6);
    if (r >= a.rows) return;
    const long long s = a.owner[r];
    if (lw_stream_bytes(a, s) > dstCap[s]) return;
    uint8_t *p = dst + dstOff[s] + (a.recOff[r] - a.recOff[a.first[s]]);
    const int U = a.cSrcLen[r], C = a.cEncLen[r];
    const bool comp = lw_compressed(U, C);
    const int hdr = 1 + varint_size((uint64_t)U) + (comp ? varint_size((uint64_t)C) : 0);
    if (lane == 0) {
        uint8_t *q = put_varint(p, (uint64_t)((comp ? 1 : 0) | (a.high ? 2 : 0)));
        q = put_varint(q, (uint64_t)U);
        if (comp) put_varint(q, (uint64_t)C);
    }
    if (comp) wave_copy(p + hdr, arena + a.cEncOff[r], (uint32_t)C, lane);
    else wave_copy(p + hdr, a.src + a.cSrcOff[r], (uint32_t)U, lane);
}

__global__ __launch_bounds__(256) void k4_lw_finish_kernel(LegacyWriteArgs a, const uint64_t *dstCap, int64_t *outLen)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n) return;
    const uint64_t bytes = lw_stream_bytes(a, s);
    long long r = bytes > dstCap[s] ? (long long)LG_CAPACITY : (long long)bytes;
    for (uint64_t k = 0; k < a.nch[s] && r >= 0; k++)
        if (lw_not_encoded(a, (long long)(a.first[s] + k))) r = LG_NOT_ENCODED;
    outLen[s] = r;
}

/* ---- legacy stream reader -------------------------------------------------------------------------------------------- */
struct LegacyChunk { uint64_t off; int32_t U, C; bool comp; };

/* LZ4Stream.cs TryReadVarInt: 7 bits per byte, at most ten bytes; 0 = clean end (nothing read), -1 = truncated, 1 = read */
__host__ __device__ __forceinline__ int read_varint(const uint8_t *p, uint64_t end, uint64_t *pos, uint64_t *out)
{
    uint64_t v = 0;
    int count = 0;
    for (;;) {
        if (*pos >= end) return count == 0 ? 0 : -1;
        const uint32_t b = p[(*pos)++];
        v += (uint64_t)(b & 0x7fu) << count;
        count += 7;
        if ((b & 0x80u) == 0 || count >= 64) break;
    }
    *out = v;
    return 1;
}

/* AcquireNextChunk (LZ4Stream.cs:248-297) without the decode: 1 = a chunk (payload checked to lie inside), 0 = clean end of
 * the stream, < 0 = the code of the first defect.  Chunks that produce no bytes are returned too (U == 0). */
__host__ __device__ __forceinline__ int legacy_next_chunk(const uint8_t *p, uint64_t end, uint64_t *pos, LegacyChunk *c)
{
    uint64_t flags, u, cl = 0;
    int k = read_varint(p, end, pos, &flags);
    if (k == 0) return 0;
    if (k < 0) return LG_END_OF_STREAM;
    const bool comp = (flags & 1u) != 0;
    if (read_varint(p, end, pos, &u) <= 0) return LG_END_OF_STREAM;       /* ReadVarInt: a clean end is an end of stream too */
    if (comp && read_varint(p, end, pos, &cl) <= 0) return LG_END_OF_STREAM;
    const int U = (int)(uint32_t)u;
    const int C = comp ? (int)(uint32_t)cl : U;
    if (C > U) return LG_END_OF_STREAM;
    if (C < 0) return LG_OVERFLOW;                                        /* new byte[compressedLength] */
    if (end - *pos < (uint64_t)C) return LG_END_OF_STREAM;                /* ReadBlock came up short */
    c->off = *pos; c->U = U; c->C = C; c->comp = comp;
    *pos += (uint64_t)C;
    if (comp) {
        if (((int)(uint32_t)flags >> 2) != 0) return LG_NOT_SUPPORTED;    /* passes */
        /* LZ4Codec.Decode: an empty source decodes to 0 bytes; C bytes never decode to more than 255 * C + 32 */
        if (C == 0 ? U != 0 : (uint64_t)U > 255ull * (uint64_t)C + 32u) return LG_INVALID_DATA;
    }
    return 1;
}

struct LegacyReadArgs {
    const uint8_t *src;
    const uint64_t *streamOff;
    const uint64_t *streamLen;
    long long n;
    uint64_t *nch;                  /* per stream: chunks that produce bytes, before the walk's defect */
    uint64_t *bound;                /* ... their bytes (sum of U) */
    int32_t *status;                /* ... 0, or the walk's defect (after nch chunks) */
    uint64_t *first;                /* ... first row */
    unsigned long long *key;        /* ... first defect in stream order: chunk << 8 | -code, ~0: none */
    uint64_t *outSize;              /* k4lz4_legacy_stream_sizes_device, or nullptr */
    int32_t *outStatus;
};

struct LegacyRows {
    uint64_t *off;                  /* payload, absolute in src */
    uint64_t *dstOff;               /* place in the output */
    uint32_t *owner;
    uint32_t *idx;                  /* chunk among the stream's rows */
    int32_t *srcLen;                /* batch decoder: C; 0 for raw chunks and chunks without room */
    int32_t *dstCap;                /* ... U; 0 where srcLen is 0 */
    int32_t *len;                   /* U */
    int32_t *outLen;                /* batch decoder's result */
    uint8_t *kind;                  /* 0 compressed, 1 raw, 2 no room */
};

__global__ __launch_bounds__(256) void k4_lr_walk_kernel(LegacyReadArgs a)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n) return;
    const uint8_t *p = a.src + a.streamOff[s];
    const uint64_t end = a.streamLen[s];
    uint64_t pos = 0, nch = 0, bound = 0;
    int st = 0;
    for (;;) {
        LegacyChunk c;
        const int k = legacy_next_chunk(p, end, &pos, &c);
        if (k <= 0) { st = k; break; }
        if (c.U > 0) {
            if (nch == 0xffffffffull) { st = LG_CAPACITY; break; }          /* (row indices are 32-bit) */
            nch++;
            bound += (uint64_t)c.U;
        }
    }
    a.nch[s] = nch;
    a.bound[s] = bound;
    a.status[s] = st;
    if (a.outSize) a.outSize[s] = bound;
    if (a.outStatus) a.outStatus[s] = st;
}

/* one thread per stream walks its records again (the walk checked them) and writes its rows; a chunk whose place does not fit
 * the stream's target is not decoded and reports LG_CAPACITY at its position */
__global__ __launch_bounds__(256) void k4_lr_fill_kernel(LegacyReadArgs a, LegacyRows rw, const uint64_t *dstOff, const uint64_t *dstCap)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n) return;
    const uint64_t nch = a.nch[s];
    a.key[s] = a.status[s] ? (nch << 8 | (unsigned long long)(-a.status[s])) : ~0ull;
    const uint8_t *p = a.src + a.streamOff[s];
    const uint64_t end = a.streamLen[s], cap = dstCap[s];
    uint64_t pos = 0, row = a.first[s], place = 0;
    for (uint64_t j = 0; j < nch;) {
        LegacyChunk c;
        if (legacy_next_chunk(p, end, &pos, &c) != 1) break;              /* (cannot happen before nch rows) */
        if (c.U == 0) continue;
        const bool room = cap >= place && cap - place >= (uint64_t)c.U;
        rw.off[row] = a.streamOff[s] + c.off;
        rw.dstOff[row] = dstOff[s] + place;
        rw.owner[row] = (uint32_t)s;
        rw.idx[row] = (uint32_t)j;
        rw.srcLen[row] = room && c.comp ? c.C : 0;
        rw.dstCap[row] = room && c.comp ? c.U : 0;
        rw.len[row] = c.U;
        rw.kind[row] = !room ? 2 : c.comp ? 0 : 1;
        place += (uint64_t)c.U;
        row++; j++;
    }
}

/* one wave per row: raw chunks are copied into place; a chunk that did not decode to U bytes, or had no room, is a defect at its
 * position (LZ4Stream.cs:288-289: InvalidData) */
__global__ __launch_bounds__(256) void k4_lr_copy_kernel(const uint8_t *src, uint8_t *dst, LegacyReadArgs a, LegacyRows rw, long long rows)
{
    const int lane = lane_id();
    const long long r = (long long)blockIdx.x * 4 + (long long)uni(threadIdx.x >> 6);
    if (r >= rows) return;
    const uint32_t kind = rw.kind[r];
    if (kind == 1) wave_copy(dst + rw.dstOff[r], src + rw.off[r], (uint32_t)rw.len[r], lane);
    if (lane == 0) {
        int code = 0;
        if (kind == 2) code = LG_CAPACITY;
        else if (kind == 0 && rw.outLen[r] != rw.len[r]) code = LG_INVALID_DATA;
        if (code) atomicMin(a.key + rw.owner[r], (unsigned long long)rw.idx[r] << 8 | (unsigned long long)(-code));
    }
}

__global__ __launch_bounds__(256) void k4_lr_finish_kernel(LegacyReadArgs a, int64_t *outLen)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n) return;
    const unsigned long long k = a.key[s];
    outLen[s] = k == ~0ull ? (int64_t)a.bound[s] : -(int64_t)(k & 0xffu);
}

}  // namespace k4
