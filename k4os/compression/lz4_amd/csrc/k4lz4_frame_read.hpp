/*
 * k4lz4_frame_read.hpp -- frame reader on device-resident frames:
 * the walk of Frames/LZ4FrameReader.blocking.cs ReadHeader / ReadBlock over frames that sit in device memory.
 *
 *   k4_frame_walk_kernel      one thread per frame: magic, FLG/BD, content size, header checksum (XXH32 of at most 14
 *                             bytes, in the thread), dictionary, then the block records up to the EndMark and the
 *                             content checksum.  Per frame: status, block count, descriptor, the decoded-size bound.
 *   k4_frame_scan_kernel      one workgroup: exclusive scan of the block counts -> each frame's first table row
 *   k4_frame_fill_kernel      one thread per frame walks its records again and writes its rows of the block table
 *   k4_frame_bsum_kernel      per block: stored against computed block checksum -> first failing block of the frame
 *   k4_frame_place_kernel     one wave per block of an independent-block frame: copies raw blocks into place and checks
 *                             that the blocks decoded in parallel fill their slots (all full but the last)
 *   k4_frame_route_kernel     per frame: which frames the in-order stream decoder (k4_decode_chain*_kernel) takes
 *   k4_frame_settle_kernel    per frame: the result in stream order, and what the content checksum covers
 *   k4_frame_finish_kernel    per frame: content checksum and ContentLength -> outLen
 *
 * The heavy work is the existing kernels': k4_xxh32_kernel (block and content checksums), the batch decoder (compressed
 * blocks of independent-block frames, each straight into its place dst + dstOff[f] + k * blockSize) and the chained
 * stream decoders (chained frames, and independent frames whose blocks do not sit at k * blockSize).
 * A frame is read only inside [frameOff[f], frameOff[f] + frameLen[f]); every length word is checked against what is
 * left before the bytes it names are touched.
 */
#pragma once
#include "k4lz4_frame.hpp"
#include "k4lz4_xxh32.hpp"

namespace k4 {

/* per-frame codes (include/k4lz4.h K4LZ4_FRAME_*) */
constexpr int FR_EOF = -1, FR_MAGIC = -2, FR_VERSION = -3, FR_HEADER = -4, FR_DICT = -5, FR_BLOCK = -6, FR_BLOCK_SUM = -7,
              FR_CONTENT_SUM = -8, FR_CAP = -9, FR_LENGTH = -10;
constexpr uint32_t FRAME_MAGIC = 0x184D2204u;
constexpr uint32_t FR_NONE = 0xffffffffu;        /* kbad: no block fails its checksum */

/* FLG bits (LZ4FrameReader.blocking.cs ReadHeader) */
constexpr uint32_t FLG_INDEPENDENT = 0x20u, FLG_BLOCK_SUM = 0x10u, FLG_SIZE = 0x08u, FLG_CONTENT_SUM = 0x04u, FLG_DICT = 0x01u;

/* per frame, structure of arrays (device scratch of the context) */
struct FrameTab {
    uint64_t *bound;        /* decoded-size bound: per block min(blockSize, 255 * stored + 32), stored if raw; capped by ContentLength */
    uint64_t *demand;       /* the same without the cap: more than the blocks can produce */
    uint64_t *clen;         /* declared ContentLength */
    uint64_t *first;        /* first row of the block table */
    uint64_t *produced;     /* bytes the parallel path placed */
    uint64_t *hashLen;      /* bytes the content checksum covers (0: not checked) */
    int64_t *res;           /* result before the content checksum / ContentLength checks */
    int64_t *serialOut;     /* in-order stream decoder's outLen */
    uint32_t *nblk;         /* complete block records walked */
    int32_t *status;        /* walk: 0, or the first structural defect (FR_EOF after nblk records when hdrEnd != 0) */
    uint32_t *desc;         /* FLG | BD << 8 */
    int32_t *bsize;         /* block size from BD */
    uint32_t *csum;         /* stored content checksum */
    uint32_t *hdrEnd;       /* offset of the first block record; 0: the header failed */
    uint32_t *kbad;         /* first block whose checksum fails, FR_NONE: none */
    uint32_t *irregular;    /* the parallel placement did not hold */
    uint32_t *nSerial;      /* blocks the in-order decoder takes (0: none) */
    uint32_t *sum;          /* computed content checksum */
    uint8_t *chained;
};

/* per block, structure of arrays */
struct BlockTab {
    uint64_t *off;          /* payload, absolute offset in src */
    uint64_t *hlen;         /* bytes the block checksum covers (0 when the frame has none) */
    uint64_t *dstOff;       /* parallel decoder: dstOff[f] + k * blockSize */
    uint32_t *len;          /* stored length, bit 31 = raw */
    uint32_t *owner;
    uint32_t *idx;          /* index inside the frame */
    uint32_t *sum;          /* stored block checksum */
    uint32_t *got;          /* computed block checksum */
    int32_t *srcLen;        /* parallel decoder: stored length; 0 for raw blocks, chained frames and blocks without room */
    int32_t *dstCap;        /* parallel decoder: min(blockSize, room) */
    int32_t *outLen;        /* parallel decoder's result */
};

/* counters the host reads back (the one wait of k4lz4_decode_frames_device) */
enum { FRC_BLOCKS = 0, FRC_BSUM_FRAMES = 1, FRC_INDEP_BLOCKS = 2, FRC_CSUM_FRAMES = 3, FRC_COUNT = 4 };

/* XXH32 (seed 0) of a header: at most 14 bytes, so no stripes */
__device__ __forceinline__ uint32_t xxh32_short(const uint8_t *p, uint32_t len)
{
    uint32_t h = XXH_P5 + len, i = 0;
    for (; i + 4 <= len; i += 4) h = xxh_rotl(h + ld32u(p + i) * XXH_P3, 17) * XXH_P4;
    for (; i < len; i++) h = xxh_rotl(h + (uint32_t)p[i] * XXH_P5, 11) * XXH_P1;
    h ^= h >> 15; h *= XXH_P2; h ^= h >> 13; h *= XXH_P3; h ^= h >> 16;
    return h;
}

__device__ __forceinline__ int frame_block_size(uint32_t bd)       /* LZ4FrameReader.cs MaxBlockSize */
{
    const uint32_t c = (bd >> 4) & 7u;
    return c == 7 ? 4 << 20 : c == 6 ? 1 << 20 : c == 5 ? 256 << 10 : 64 << 10;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

struct FrameWalkArgs {
    const uint8_t *src;
    const uint64_t *frameOff;
    const uint64_t *frameLen;
    long long n;
    FrameTab t;
    unsigned long long *counters;    /* FRC_* (zeroed by the host), or nullptr */
    uint64_t *outSize;               /* k4lz4_frame_sizes_device, or nullptr */
    int32_t *outStatus;
};

/* the id table of a call with a dictionary set (k4lz4_frame_dict.hpp): entry e answers to DictID ids[e] */
struct FrameWalkIds {
    const uint32_t *ids;
    int nDict;
    int32_t *dictIdx;                /* per frame, out: the entry, -1: none */
    int32_t *outDictIdx;             /* the caller's copy, or nullptr */
    unsigned long long *chained;     /* counter: chained frames that resolved to an entry, or nullptr */
};

/* the walk of one frame per thread.  WITH_IDS: a DictID is looked up in the call's id table once the header checksum has passed
 * (it covers those bytes) -- the first entry whose id equals it, FR_DICT when there is none; without, every DictID is FR_DICT */
template <bool WITH_IDS>
__device__ __forceinline__ void frame_walk_body(const FrameWalkArgs &a, const FrameWalkIds &d)
{
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = f < a.n;
    int st = 0;
    int32_t entry = -1;
    uint64_t id_at = 0;
    uint32_t flg = 0, bd = 0, hdr_end = 0, nb = 0, csum = 0, indep = 0;
    uint64_t clen = 0, bound = 0;
    int bs = 64 << 10;
    if (live) {
        const uint8_t *p = a.src + a.frameOff[f];
        const uint64_t end = a.frameLen[f];
        uint64_t pos = 0;
        do {
            if (end < 4) { st = FR_EOF; break; }
            if (ld32u(p) != FRAME_MAGIC) { st = FR_MAGIC; break; }
            if (end < 6) { st = FR_EOF; break; }
            flg = p[4]; bd = p[5]; pos = 6;
            if (((flg >> 6) & 0x11u) != 1u) { st = FR_VERSION; break; }          /* as the reader writes it */
            if (flg & FLG_SIZE) {
                if (end - pos < 8) { st = FR_EOF; break; }
                clen = ld64u(p + pos); pos += 8;
            }
            if (flg & FLG_DICT) {
                if (end - pos < 4) { st = FR_EOF; break; }
                id_at = pos; pos += 4;
            }
            if (end - pos < 1) { st = FR_EOF; break; }
            if (((xxh32_short(p + 4, (uint32_t)(pos - 4)) >> 8) & 0xffu) != p[pos]) { st = FR_HEADER; break; }
            pos += 1;
            if (flg & FLG_DICT) {
                if (WITH_IDS) {
                    const uint32_t id = ld32u(p + id_at);
                    for (int e = 0; e < d.nDict; e++)
                        if (d.ids[e] == id) { entry = e; break; }
                }
                if (entry < 0) { st = FR_DICT; break; }
            }
            hdr_end = (uint32_t)pos;
            bs = frame_block_size(bd);
            const uint64_t trailer = (flg & FLG_BLOCK_SUM) ? 4 : 0;
            for (;;) {
                if (end - pos < 4) { st = FR_EOF; break; }
                const uint32_t lc = ld32u(p + pos);
                pos += 4;
                if (lc == 0) {                                                      /* EndMark */
                    if (flg & FLG_CONTENT_SUM) {
                        if (end - pos < 4) { st = FR_EOF; break; }
                        csum = ld32u(p + pos);
                    }
                    break;
                }
                const uint64_t sn = lc & 0x7fffffffu;
                if (end - pos < sn + trailer) { st = FR_EOF; break; }
                pos += sn + trailer;
                const bool raw = (lc & 0x80000000u) != 0;
                bound += raw ? sn : (255 * sn + 32 < (uint64_t)bs ? 255 * sn + 32 : (uint64_t)bs);
                nb++;
                if (!raw && (flg & FLG_INDEPENDENT)) indep++;
            }
        } while (0);
        if (!hdr_end) bound = 0;
        a.t.demand[f] = bound;
        if ((flg & FLG_SIZE) && hdr_end && bound > clen) bound = clen;
        a.t.bound[f] = bound;
        a.t.clen[f] = clen;
        a.t.nblk[f] = nb;
        a.t.status[f] = st;
        a.t.desc[f] = flg | bd << 8;
        a.t.bsize[f] = bs;
        a.t.csum[f] = csum;
        a.t.hdrEnd[f] = hdr_end;
        if (WITH_IDS) {
            if (!hdr_end) entry = -1;
            d.dictIdx[f] = entry;
            if (d.outDictIdx) d.outDictIdx[f] = entry;
        }
        if (a.outSize) a.outSize[f] = bound;
        if (a.outStatus) a.outStatus[f] = st;
    }
    if (a.counters) {
        const unsigned long long bsum = wave_sum64(hdr_end && nb && (flg & FLG_BLOCK_SUM) ? 1ull : 0ull);
        const unsigned long long ind = wave_sum64(indep);
        const unsigned long long cs = wave_sum64(hdr_end && (flg & FLG_CONTENT_SUM) ? 1ull : 0ull);
        if (lane_id() == 0) {
            if (bsum) atomicAdd(a.counters + FRC_BSUM_FRAMES, bsum);
            if (ind) atomicAdd(a.counters + FRC_INDEP_BLOCKS, ind);
            if (cs) atomicAdd(a.counters + FRC_CSUM_FRAMES, cs);
        }
    }
    if (WITH_IDS && d.chained) {
        const unsigned long long dc = wave_sum64(hdr_end && entry >= 0 && !(flg & FLG_INDEPENDENT) ? 1ull : 0ull);
        if (dc && lane_id() == 0) atomicAdd(d.chained, dc);
    }
}

__global__ __launch_bounds__(256) void k4_frame_walk_kernel(FrameWalkArgs a)
{
    frame_walk_body<false>(a, FrameWalkIds{});
}

constexpr int FRAME_SCAN_THREADS = 256;

/* one workgroup: first[f] = sum of nblk before f, counters[FRC_BLOCKS] = the total; 1024 frames per step */
__global__ __launch_bounds__(FRAME_SCAN_THREADS) void k4_frame_scan_kernel(const uint32_t *nblk, uint64_t *first, long long n,
                                                                          unsigned long long *counters)
{
    __shared__ unsigned long long wsum[FRAME_SCAN_THREADS / 64];
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    unsigned long long carry = 0;
    for (long long base = 0; base < n; base += FRAME_SCAN_THREADS * 4) {
        const long long i0 = base + (long long)threadIdx.x * 4;
        uint32_t v[4];
        unsigned long long s = 0;
        for (int k = 0; k < 4; k++) {
            v[k] = i0 + k < n ? nblk[i0 + k] : 0u;
            s += v[k];
        }
        unsigned long long x = s;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = __shfl_up(x, (unsigned)d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        unsigned long long before = 0, tot = 0;
        for (int w = 0; w < FRAME_SCAN_THREADS / 64; w++) {
            if (w < wave) before += wsum[w];
            tot += wsum[w];
        }
        unsigned long long e = carry + before + x - s;
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) first[i0 + k] = e;
            e += v[k];
        }
        carry += tot;
        __syncthreads();                         /* wsum is rewritten by the next step */
    }
    if (threadIdx.x == 0) counters[FRC_BLOCKS] = carry;
}

struct FrameFillArgs {
    const uint8_t *src;
    const uint64_t *frameOff;
    const uint64_t *dstOff;          /* per frame */
    const uint64_t *dstCap;
    long long n;
    FrameTab t;
    BlockTab b;
};

/* one thread per frame: its rows of the block table, and the per-frame words the block kernels accumulate into */
__global__ __launch_bounds__(256) void k4_frame_fill_kernel(FrameFillArgs a)
{
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= a.n) return;
    a.t.kbad[f] = FR_NONE;
    a.t.irregular[f] = 0;
    a.t.produced[f] = 0;
    const uint32_t hdr_end = a.t.hdrEnd[f], nb = a.t.nblk[f];
    if (!hdr_end || !nb) return;
    const uint32_t flg = a.t.desc[f] & 0xffu;
    const bool chained = !(flg & FLG_INDEPENDENT), bsum = (flg & FLG_BLOCK_SUM) != 0;
    const uint64_t bs = (uint64_t)a.t.bsize[f], cap = a.dstCap[f], d0 = a.dstOff[f], base = a.frameOff[f];
    const uint8_t *p = a.src + base;
    uint64_t pos = hdr_end, row = a.t.first[f];
    for (uint32_t k = 0; k < nb; k++, row++) {                  /* the walk checked every record read here */
        const uint32_t lc = ld32u(p + pos);
        pos += 4;
        const uint32_t sn = lc & 0x7fffffffu;
        const bool raw = (lc & 0x80000000u) != 0;
        const uint64_t at = (uint64_t)k * bs;
        const uint64_t room = cap > at ? cap - at : 0;
        const int32_t bcap = (int32_t)(room < bs ? room : bs);
        a.b.off[row] = base + pos;
        a.b.len[row] = lc;
        a.b.owner[row] = (uint32_t)f;
        a.b.idx[row] = k;
        a.b.hlen[row] = bsum ? sn : 0;
        a.b.sum[row] = bsum ? ld32u(p + pos + sn) : 0u;
        a.b.srcLen[row] = (raw || chained || bcap == 0) ? 0 : (int32_t)sn;
        a.b.dstOff[row] = d0 + at;
        a.b.dstCap[row] = bcap;
        pos += sn + (bsum ? 4 : 0);
    }
}

/* per block: a block checksum that does not match -> the frame's first failing block */
__global__ __launch_bounds__(256) void k4_frame_bsum_kernel(FrameTab t, BlockTab b, long long nb)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= nb) return;
    const uint32_t f = b.owner[r];
    if ((t.desc[f] & FLG_BLOCK_SUM) && b.got[r] != b.sum[r]) atomicMin(t.kbad + f, b.idx[r]);
}

__device__ __forceinline__ uint32_t frame_decode_count(const FrameTab &t, uint32_t f)
{
    const uint32_t nb = t.nblk[f], kb = t.kbad[f];
    return kb < nb ? kb : nb;                   /* blocks before the first failing checksum are decoded (stream order) */
}

/* one wave per block of an independent-block frame: raw blocks are copied into place; a frame whose blocks do not all fill
 * their slots (short or failed block before the last, a raw block longer than its slot) is irregular */
__global__ __launch_bounds__(256) void k4_frame_place_kernel(const uint8_t *src, uint8_t *dst, FrameTab t, BlockTab b, long long nb)
{
    const int lane = lane_id();
    const long long r = (long long)blockIdx.x * 4 + (long long)uni(threadIdx.x >> 6);
    if (r >= nb) return;
    const uint32_t f = b.owner[r];
    if (!(t.desc[f] & FLG_INDEPENDENT)) return;
    const uint32_t k = b.idx[r], nd = frame_decode_count(t, f);
    if (k >= nd) return;
    const uint32_t lc = b.len[r], sn = lc & 0x7fffffffu;
    const int32_t cap = b.dstCap[r];
    long long got;
    if (lc & 0x80000000u) {
        got = (long long)sn <= (long long)cap ? (long long)sn : -1;
        if (got > 0) wave_copy(dst + b.dstOff[r], src + b.off[r], sn, lane);
    } else {
        got = cap > 0 ? (long long)b.outLen[r] : -1;
    }
    if (lane == 0) {
        if (got < 0 || (k + 1 < nd && got != (long long)t.bsize[f])) atomicOr(t.irregular + f, 1u);
        else if (got > 0) atomicAdd((unsigned long long *)t.produced + f, (unsigned long long)got);
    }
}

/* per frame: chained frames and irregular independent ones go to the in-order decoder with their blocks up to the first
 * failing checksum; the others with none */
__global__ __launch_bounds__(256) void k4_frame_route_kernel(FrameTab t, long long n)
{
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    const bool chained = !(t.desc[f] & FLG_INDEPENDENT);
    t.chained[f] = chained ? 1 : 0;
    t.nSerial[f] = t.hdrEnd[f] && (chained || t.irregular[f]) ? frame_decode_count(t, (uint32_t)f) : 0u;
}

/* per frame, in the order ReadBlock meets things: a block that does not decode (or a target that is too small), a block
 * checksum, the end of the input; then what the content checksum covers */
__global__ __launch_bounds__(256) void k4_frame_settle_kernel(FrameTab t, const uint64_t *dstCap, long long n)
{
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    const uint32_t flg = t.desc[f] & 0xffu;
    const int st = t.status[f];
    long long r;
    if (!t.hdrEnd[f]) {
        r = st;
    } else {
        const bool serial = !(flg & FLG_INDEPENDENT) || t.irregular[f];
        r = serial ? (long long)t.serialOut[f] : (long long)t.produced[f];
        const bool bad_sum = t.kbad[f] != FR_NONE;
        if (r == FR_CAP) {
            /* a target that holds all the blocks can produce was not too small: the block failed.  Else, the output would pass
             * a declared ContentLength that fits the target: a length defect, which the reader meets only after every later
             * block (their checksums, the end of the input) */
            if (dstCap[f] >= t.demand[f]) r = FR_BLOCK;
            else if ((flg & FLG_SIZE) && t.clen[f] <= dstCap[f]) r = bad_sum ? FR_BLOCK_SUM : st == FR_EOF ? FR_EOF : FR_LENGTH;
        } else if (r >= 0) {
            if (bad_sum) r = FR_BLOCK_SUM;
            else if (st) r = st;
        }
    }
    t.res[f] = r;
    t.hashLen[f] = (r >= 0 && (flg & FLG_CONTENT_SUM)) ? (uint64_t)r : 0u;
}

__global__ __launch_bounds__(256) void k4_frame_finish_kernel(FrameTab t, int64_t *outLen, long long n, int have_sum)
{
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    const uint32_t flg = t.desc[f] & 0xffu;
    long long r = t.res[f];
    if (r >= 0) {
        if ((flg & FLG_CONTENT_SUM) && have_sum && t.sum[f] != t.csum[f]) r = FR_CONTENT_SUM;
        else if ((flg & FLG_SIZE) && (uint64_t)r != t.clen[f]) r = FR_LENGTH;
    }
    outLen[f] = r;
}

}  // namespace k4
