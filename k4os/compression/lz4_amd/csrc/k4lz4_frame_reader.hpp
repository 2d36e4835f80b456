/*
 * k4lz4_frame_reader.hpp -- the incremental frame reader on the device (k4lz4_frame_read_batch).
 *
 * Each call advances many LZ4FrameReaders by one ReadManyBytes (Frames/LZ4FrameReader.async.cs:150-172) or one OpenFrame
 * (LZ4FrameReader.cs:138-139 -> EnsureHeader, .async.cs:46-47).  Stream s is src[srcOff[s] .. + srcLen[s]): zero or more frames
 * one after another, all of it present at every call.  How many blocks a read consumes depends on the data, so everything a
 * reader keeps between calls lives in the stream's DEVICE store and the host keeps nothing but the settings:
 *
 *   FrState (FR_STATE_BYTES)   source position, phase (no frame / open / failed + code), FLG / BD, block size, ContentLength,
 *                              _decoded (the undrained count), bytes read, the content checksum's XXH32 streaming state
 *   buffer  (fr_buffer_bytes)  the decoder's output: for chained frames the bytes decoded so far, kept contiguous -- the last
 *                              64 KiB of them are the next block's prefix -- and moved down to the front when the next block
 *                              would not fit (LZ4ChainDecoder.Prepare / CopyDict, LZ4ChainDecoder.cs:117-132; where the bytes
 *                              sit is not observable, which bytes are the prefix is); for independent frames one block
 *
 *   k4_fr_read_kernel          one wavefront per stream runs the reference's loop as written: EnsureHeader -> ReadHeader
 *                              (.async.cs:50-108), then while bytes are wanted ReadBlock (.async.cs:110-137: length word, EndMark
 *                              and content checksum, payload, block checksum over the stored bytes, Inject or Decode, content
 *                              checksum over the whole block) and Drain (LZ4FrameReader.cs:98-112).  A block of an independent
 *                              frame that fits into what the read still wants (blockSize + 8 bytes, LZ4BlockDecoder's capacity,
 *                              LZ4BlockDecoder.cs:27,49) is decoded straight into dst, every other block into the buffer.
 *
 * The block decoder is decode_block (k4lz4_decode.hpp), with the buffer's tail as prefix for chained frames: LZ4ChainDecoder
 * decodes with capacity blockSize at the end of its output (LZ4ChainDecoder.cs:45-61) through LZ4_decompress_safe_continue
 * (LL64.dec.cs:558-608), whose prefix is min(bytes of the frame so far, 64 KiB) however its ring wraps.
 *
 * What differs from the reference, on purpose: a stored length above blockSize does not fit the reference's block buffer
 * (AllocBuffer(blockSize), a pooled array whose real length depends on the pool): it is refused here as a block defect
 * (FR_BLOCK) before its bytes are looked at.  A frame whose block size is above the reader's maxBlockSize is FR_BLOCK_SIZE.
 * A stream that has reported a code stays failed.  Nothing outside [srcOff[s], srcOff[s] + srcLen[s]) is read (whole aligned
 * dwords around it, as the batch decoder does) and nothing outside [dstOff[s], dstOff[s] + count[s]) or the store is written.
 */
#pragma once
#include "k4lz4_decode.hpp"
#include "k4lz4_frame_read.hpp"
#include "k4lz4_frame_write.hpp"

namespace k4 {

constexpr int FR_BLOCK_SIZE = -11;               /* include/k4lz4.h K4LZ4_FRAME_BLOCK_SIZE */
constexpr int FR_OP_READ = 0, FR_OP_OPEN = 1, FR_OP_RESET = 2;
constexpr int FR_PHASE_NONE = 0, FR_PHASE_OPEN = 1, FR_PHASE_FAILED = 2;
constexpr int64_t FR_STATE_BYTES = 256;
constexpr uint32_t FR_HISTORY = 65536;
constexpr uint32_t FR_PLAN_NONE = 0, FR_PLAN_FAST = 1, FR_PLAN_DONE = 2;

struct FrState {
    unsigned long long pos;          /* next unread byte of the source, relative to srcOff[s] */
    unsigned long long bytesRead;    /* GetBytesRead: over all frames of the source */
    unsigned long long clen;         /* the open frame's ContentLength */
    int32_t phase, code;
    uint32_t flg, bd;
    int32_t bsize;
    uint32_t pending;                /* _decoded: bytes of the last block not drained yet, the buffer's [tail - pending, tail) */
    uint32_t tail;                   /* decoded bytes in the buffer */
    uint32_t direct;                 /* blocks decoded straight into dst (a statistic) */
    unsigned long long blocks;       /* blocks read (a statistic) */
    unsigned long long fastBlocks;   /* of those, decoded by the batch decoder on the fast path */
    unsigned long long handedBack;   /* calls in which the fast path's hypothesis failed and the general reader replayed the stream */
    FwXxhState content;              /* XXH32.State of the content checksum */
    FwXxhState scratch;              /* a block checksum in the making */
    uint32_t stashFill;              /* fed records (k4lz4_frame_feed.hpp): bytes of an incomplete field kept behind the buffer */
    uint32_t stashWant;              /* ... and the length with which that field is complete (0: nothing is awaited) */
    uint32_t dictEntry;              /* calls with a dictionary set (k4lz4_frame_reader_dict.hpp): the entry the open frame's DictID resolved
                                      * to, + 1 (0: none) -- set where the header is accepted, cleared where the frame closes */
};
static_assert(sizeof(FrState) <= (size_t)FR_STATE_BYTES, "FrState outgrew its slot");

/* the decoder's buffer behind the state: 64 KiB of history and one block of the largest size (+ 8: LZ4BlockDecoder's capacity) */
__host__ __device__ inline int64_t fr_buffer_bytes(int64_t maxBlock) { return (int64_t)FR_HISTORY + maxBlock + 64; }
__host__ __device__ inline int64_t fr_store_bytes(int64_t maxBlock) { return FR_STATE_BYTES + ((fr_buffer_bytes(maxBlock) + 255) & ~(int64_t)255); }
/* the reader's maxBlockSize: whole block-size codes, 64 KiB .. 4 MiB (0: 4 MiB) */
inline int32_t fr_max_block(int64_t asked)
{
    if (asked <= 0) return 4 << 20;
    return asked <= (64 << 10) ? 64 << 10 : asked <= (256 << 10) ? 256 << 10 : asked <= (1 << 20) ? 1 << 20 : 4 << 20;
}

/* XXH32.Update of a streaming state by one wave: lanes 0-3 own the four accumulators (k4_fw_xxh32_kernel's scheme), the other
 * lanes run along with nothing to do.  Every lane returns after the state is rewritten and visible to the wave. */
__device__ __forceinline__ void fr_xxh_update(FwXxhState *st, const uint8_t *p, uint64_t n, bool fresh, int lane)
{
    const int c = lane & 3;
    const bool live = lane < 4;
    const uint64_t len = live ? n : 0u;
    uint32_t m[4] = {0u, 0u, 0u, 0u}, carried = 0u, v;
    unsigned long long total = 0ull;
    if (fresh || !live) {                                /* XXH32.Reset(seed 0) */
        v = c == 0 ? XXH_P1 + XXH_P2 : c == 1 ? XXH_P2 : c == 2 ? 0u : 0u - XXH_P1;
    } else {
        const uint32_t *w = (const uint32_t *)st->mem;
        m[0] = w[0]; m[1] = w[1]; m[2] = w[2]; m[3] = w[3];
        carried = st->memsize; total = st->total; v = st->acc[c];
    }
    uint64_t at = 0;
    if ((uint64_t)carried + len >= 16u) {
        if (carried) {
            uint32_t x = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t i = 4u * (uint32_t)c + k;
                const uint32_t word = (i >> 2) == 0 ? m[0] : (i >> 2) == 1 ? m[1] : (i >> 2) == 2 ? m[2] : m[3];
                const uint32_t byte = i < carried ? (word >> (8u * (i & 3u))) & 0xffu : (uint32_t)p[i - carried];
                x |= byte << (8u * k);
            }
            v = xxh_round(v, x);
            at = 16u - carried;
        }
        const uint64_t stripes = (len - at) >> 4;
        const uint8_t *q = p + at + 4 * c;
        uint64_t s = 0;
        if (stripes >= 16) {
            uint32_t x[8], y[8];
#pragma unroll
            for (int k = 0; k < 8; k++) x[k] = ld32u(q + 16 * k);
            q += 128;
            for (s = 8; s + 8 <= stripes; s += 8) {
#pragma unroll
                for (int k = 0; k < 8; k++) y[k] = ld32u(q + 16 * k);
                q += 128;
#pragma unroll
                for (int k = 0; k < 8; k++) v = xxh_round(v, x[k]);
#pragma unroll
                for (int k = 0; k < 8; k++) x[k] = y[k];
            }
#pragma unroll
            for (int k = 0; k < 8; k++) v = xxh_round(v, x[k]);
        }
        for (; s < stripes; s++) { v = xxh_round(v, ld32u(q)); q += 16; }
        at += stripes << 4;
        carried = 0u;
    }
    wave_sync();                                         /* every lane has read the state before any lane rewrites it */
    if (live) {
        st->acc[c] = v;
        if (c == 0) {
            const uint32_t rest = (uint32_t)(len - at);
            st->reserved = 0u;
            for (uint32_t i = 0; i < rest; i++) st->mem[carried + i] = p[at + i];
            st->memsize = carried + rest;
            st->total = total + len;
        }
    }
    wave_sync();
}

/* the dictionary set of a call that has one (k4lz4_frame_reader_dict.hpp): entry e answers to DictID ids[e], its kept
 * bytes are dict[entryOff[e] .. + entryLen[e]) */
struct FrDict {
    const uint8_t *dict;
    const uint64_t *entryOff;
    const int32_t *entryLen;
    const uint32_t *ids;
    int nDict;
};

/* ReadHeader (.async.cs:50-108) over h[0 .. left), left >= 1: 0 and the fields, or the code of the first defect.  WITH_IDS: a DictID is
 * looked up in the call's id table where it is refused otherwise -- entry1 is the first entry whose id equals it, + 1 (0: the frame
 * names none), FR_DICT when there is none */
struct FrHeader { uint32_t flg, bd, len; int bs; uint64_t clen; };
template <bool WITH_IDS>
__device__ __forceinline__ int fr_parse_header_ids(const uint8_t *h, uint64_t left, int32_t maxBlock, FrHeader &o, const FrDict &d, uint32_t &entry1)
{
    uint64_t at;
    if (left < 4) return FR_EOF;
    if (ld32u(h) != FRAME_MAGIC) return FR_MAGIC;
    if (left < 6) return FR_EOF;
    o.flg = h[4]; o.bd = h[5]; at = 6;
    if (((o.flg >> 6) & 0x11u) != 1u) return FR_VERSION;                    /* as the reader writes it */
    o.clen = 0;
    if (o.flg & FLG_SIZE) {
        if (left - at < 8) return FR_EOF;
        o.clen = ld64u(h + at); at += 8;
    }
    if (o.flg & FLG_DICT) {
        if (left - at < 4) return FR_EOF;
        at += 4;
    }
    if (left - at < 1) return FR_EOF;
    if (((xxh32_short(h + 4, (uint32_t)(at - 4)) >> 8) & 0xffu) != h[at]) return FR_HEADER;
    at += 1;
    if (WITH_IDS) {
        entry1 = 0u;
        if (o.flg & FLG_DICT) {
            const uint32_t id = ld32u(h + at - 5);
            for (int e = 0; e < d.nDict; e++)
                if (d.ids[e] == id) { entry1 = (uint32_t)e + 1u; break; }
            if (!entry1) return FR_DICT;
        }
    } else if (o.flg & FLG_DICT) return FR_DICT;
    o.bs = frame_block_size(o.bd);
    if (o.bs > maxBlock) return FR_BLOCK_SIZE;                              /* where the reference creates its decoder */
    o.len = (uint32_t)at;
    return 0;
}
__device__ __forceinline__ int fr_parse_header(const uint8_t *h, uint64_t left, int32_t maxBlock, FrHeader &o)
{
    uint32_t none;
    return fr_parse_header_ids<false>(h, left, maxBlock, o, FrDict{}, none);
}

/* the kept bytes of entry1 - 1 (their end and how many), nothing for entry1 == 0; entry1 <= d.nDict.  The same in every lane. */
__device__ __forceinline__ uint32_t fr_dict_kept(const FrDict &d, uint32_t entry1, const uint8_t *&end)
{
    end = nullptr;
    if (!entry1) return 0u;
    const uint32_t len = uni((uint32_t)d.entryLen[entry1 - 1u]);
    end = d.dict + d.entryOff[entry1 - 1u] + len;
    return len;
}

struct FrReadArgs {
    const uint8_t *src;
    const uint64_t *srcOff, *srcLen;
    uint8_t *store;
    const uint64_t *storeOff;
    uint8_t *dst;
    const uint64_t *dstOff;
    const int64_t *count;            /* READ: bytes wanted; < 0: the stream sits this call out */
    int64_t *outLen;
    long long n;
    int op;                          /* FR_OP_* */
    int interactive;
    int32_t maxBlock;
    const uint32_t *done;            /* per stream: FR_PLAN_DONE where the fast path has served the call, or nullptr */
};

constexpr int FR_WAVES_PER_WG = DECODE_WAVES_PER_WG;

/* the loop described at the top: its text is k4lz4_frame_reader_loop.hpp, which k4_fr_dict_read_kernel (k4lz4_frame_reader_dict.hpp)
 * includes as well, with the dictionary's lines switched on */
__global__ __launch_bounds__(64 * FR_WAVES_PER_WG) void k4_fr_read_kernel(FrReadArgs a)
{
    __shared__ uint32_t lds[FR_WAVES_PER_WG][DECODE_LDS_DWORDS];
#define FR_LOOP_DICT 0
#include "k4lz4_frame_reader_loop.hpp"
#undef FR_LOOP_DICT
}

/* ---- the fast path for what real writers produce: independent-block frames whose blocks are full -------------
 * k4_fr_plan_kernel    one thread per stream walks ahead from the stored position under the hypothesis that the next
 *                      ceil(count / blockSize) records are blocks of exactly blockSize bytes: every record is checked against the
 *                      source range, the state is not touched.  Blocks that fall wholly inside the read get a row that sends them
 *                      through the batch decoder straight into dst, the one that straddles the read's end a row into the store.
 *                      A stream takes part when it reads (not interactive), has nothing pending, and its frame (open, or opened by
 *                      this walk) has independent blocks; everything else is the general reader's.
 *   -> k4_xxh32_kernel (block checksums), the batch decoder twice (rows into dst, rows into the stores) ->
 *   k4_fr_commit_kernel  one wave per stream verifies the hypothesis -- every block produced exactly blockSize, checksums hold --,
 *                      copies raw blocks and the straddling block's first bytes, updates the content checksum once over the call's
 *                      bytes in order and commits the state; a stream whose hypothesis failed keeps its state and is replayed by
 *                      k4_fr_read_kernel (FrReadArgs::done), decided on the device. */
struct FrPlan {
    unsigned long long posAfter;     /* source position behind the last record walked */
    unsigned long long clen;
    uint32_t state;                  /* FR_PLAN_* */
    uint32_t nblk;                   /* records walked: nfull into dst, then the straddling one */
    uint32_t nfull, part;            /* part: bytes of the straddling block the read takes (0: none) */
    uint32_t opened;                 /* the walk read a header */
    uint32_t flg, bd;
    int32_t bs;
};

struct FrFastArgs {
    FrReadArgs r;
    FrPlan *plan;
    uint32_t *done;
    long long rows;                  /* table rows per stream: fr_table_rows(maxCount) */
    /* per row (stream s: rows [s * rows, s * rows + nfull)): the batch decoder's arguments for blocks into dst */
    uint64_t *srcOff, *dstOff, *hlen;
    int32_t *srcLen, *dstCap, *outLen;
    uint32_t *sum, *got, *lc;
    /* per stream: the straddling block, decoded into the store's buffer (offsets from r.store) */
    uint64_t *sSrcOff, *sDstOff;
    int32_t *sSrcLen, *sDstCap, *sOutLen;
};

__host__ __device__ inline long long fr_table_rows(long long maxCount) { return maxCount > 0 ? maxCount / 65536 + 2 : 0; }

/* the fast path's words of a call with a dictionary set: the batch decoder's dictionary arguments for the rows into dst and for the
 * straddling blocks, and what the plan resolved for the commit to store */
struct FrDictRows {
    FrDict d;
    uint64_t *dictOff;               /* per row */
    int32_t *dictLen;
    signed char *dictMode;
    uint64_t *sDictOff;              /* per stream: the straddling block */
    int32_t *sDictLen;
    signed char *sDictMode;
    uint32_t *entry;                 /* per stream: the frame's entry + 1 (0: none) */
};

/* every row of stream s and its straddling block decode against entry1 - 1's kept bytes -- the set's memory is never the bytes in
 * front of a target (mode 2) */
__device__ __forceinline__ void fr_plan_dict_rows(const FrDictRows &w, long long s, long long row0, long long rows, uint32_t entry1)
{
    const uint64_t off = entry1 ? w.d.entryOff[entry1 - 1u] : 0ull;
    const int32_t len = entry1 ? w.d.entryLen[entry1 - 1u] : 0;
    for (long long j = 0; j < rows; j++) { w.dictOff[row0 + j] = off; w.dictLen[row0 + j] = len; w.dictMode[row0 + j] = 2; }
    w.sDictOff[s] = off; w.sDictLen[s] = len; w.sDictMode[s] = 2;
    w.entry[s] = entry1;
}

/* k4_fr_plan_kernel's body.  DICT (k4_fr_dict_plan_kernel): the walk resolves a DictID when it reads a header, or takes the entry the
 * open frame has; a stored entry the set does not have is the general reader's to report */
template <bool DICT>
__device__ __forceinline__ void fr_plan_body(const FrFastArgs &a, const FrDictRows &w)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.r.n) return;
    FrPlan pl{};
    a.sSrcLen[s] = 0; a.sDstCap[s] = 0; a.sSrcOff[s] = 0; a.sDstOff[s] = 0; a.sOutLen[s] = 0;
    const long long row0 = s * a.rows;
    const int64_t want = a.r.count[s];
    const FrState *st = (const FrState *)(a.r.store + a.r.storeOff[s]);
    uint32_t used = 0, entry1 = 0;
    do {
        if (want <= 0 || a.r.interactive || st->phase == FR_PHASE_FAILED || st->pending != 0) break;
        const uint8_t *p = a.r.src + a.r.srcOff[s];
        const uint64_t end = a.r.srcLen[s];
        uint64_t pos = st->pos;
        FrHeader hd{st->flg, st->bd, 0u, st->bsize, st->clen};
        if (st->phase != FR_PHASE_OPEN) {
            if (pos >= end || fr_parse_header_ids<DICT>(p + pos, end - pos, a.r.maxBlock, hd, w.d, entry1) != 0) break;
            pos += hd.len;
            pl.opened = 1;
        } else if (DICT) {
            entry1 = st->dictEntry;
            if (entry1 > (uint32_t)w.d.nDict) break;
        }
        if (!(hd.flg & FLG_INDEPENDENT)) break;
        const uint64_t bs = (uint64_t)hd.bs, need = (uint64_t)want;
        const uint64_t k = (need + bs - 1) / bs;
        if ((long long)k > a.rows) break;
        const uint64_t nfull = need / bs;
        const bool bsum = (hd.flg & FLG_BLOCK_SUM) != 0;
        bool ok = true;
        for (uint64_t j = 0; j < k; j++) {
            if (end - pos < 4) { ok = false; break; }
            const uint32_t lc = ld32u(p + pos);
            const uint32_t sn = lc & 0x7fffffffu;
            const bool raw = (lc & 0x80000000u) != 0;
            pos += 4;
            if (lc == 0 || sn > bs || (raw && sn != bs) || end - pos < (uint64_t)sn + (bsum ? 4u : 0u)) { ok = false; break; }
            const uint64_t at = a.r.srcOff[s] + pos;
            const long long r = row0 + (long long)j;
            a.lc[r] = lc;
            a.srcOff[r] = at;
            a.hlen[r] = bsum ? sn : 0u;
            a.sum[r] = bsum ? ld32u(p + pos + sn) : 0u;
            a.srcLen[r] = 0; a.dstCap[r] = 0; a.outLen[r] = 0;
            a.dstOff[r] = a.r.dstOff[s] + j * bs;
            if (j < nfull) {
                if (!raw) { a.srcLen[r] = (int32_t)sn; a.dstCap[r] = (int32_t)bs; }
            } else if (!raw) {                               /* the straddling block: LZ4BlockDecoder's capacity, into the buffer */
                a.sSrcOff[s] = at; a.sSrcLen[s] = (int32_t)sn;
                a.sDstOff[s] = a.r.storeOff[s] + (uint64_t)FR_STATE_BYTES; a.sDstCap[s] = (int32_t)bs + 8;
            }
            used = (uint32_t)j + 1u;
            pos += sn + (bsum ? 4u : 0u);
        }
        if (!ok) break;
        pl.state = FR_PLAN_FAST;
        pl.posAfter = pos; pl.clen = hd.clen; pl.nblk = (uint32_t)k; pl.nfull = (uint32_t)nfull; pl.part = (uint32_t)(need - nfull * bs);
        pl.flg = hd.flg; pl.bd = hd.bd; pl.bs = hd.bs;
    } while (0);
    if (pl.state != FR_PLAN_FAST) {                          /* nothing of a stream that is not taken goes to the decoders */
        for (uint32_t j = 0; j < used; j++) { a.srcLen[row0 + j] = 0; a.hlen[row0 + j] = 0; }
        a.sSrcLen[s] = 0;
        used = 0;
    }
    for (long long j = used; j < a.rows; j++) { a.srcLen[row0 + j] = 0; a.dstCap[row0 + j] = 0; a.hlen[row0 + j] = 0; a.srcOff[row0 + j] = 0; a.dstOff[row0 + j] = 0; }
    a.plan[s] = pl;
    a.done[s] = FR_PLAN_NONE;
    if (DICT) fr_plan_dict_rows(w, s, row0, a.rows, pl.state == FR_PLAN_FAST ? entry1 : 0u);
}

__global__ __launch_bounds__(256) void k4_fr_plan_kernel(FrFastArgs a)
{
    fr_plan_body<false>(a, FrDictRows{});
}

/* k4_fr_commit_kernel's body.  entry (k4_fr_dict_commit_kernel): per stream the word the plan resolved, committed with the state */
template <bool DICT>
__device__ __forceinline__ void fr_commit_body(const FrFastArgs &a, const uint32_t *entry)
{
    const int lane = lane_id();
    const long long s = (long long)blockIdx.x * FR_WAVES_PER_WG + (long long)uni(threadIdx.x >> 6);
    if (s >= a.r.n) return;
    const FrPlan pl = a.plan[s];
    if (pl.state != FR_PLAN_FAST) return;
    FrState *st = (FrState *)(a.r.store + a.r.storeOff[s]);
    uint8_t *buf = (uint8_t *)st + FR_STATE_BYTES;
    uint8_t *out = a.r.dst + a.r.dstOff[s];
    const long long row0 = s * a.rows;
    const uint32_t bs = (uint32_t)pl.bs;
    /* the hypothesis: every block produced exactly blockSize, every block checksum holds */
    bool ok = true;
    for (uint32_t j0 = 0; j0 < pl.nblk; j0 += 64u) {
        const uint32_t j = j0 + (uint32_t)lane;
        bool good = true;
        if (j < pl.nblk) {
            const long long r = row0 + j;
            const uint32_t lc = a.lc[r];
            if (!(lc & 0x80000000u)) good = (j < pl.nfull ? a.outLen[r] : a.sOutLen[s]) == (int32_t)bs;
            if ((pl.flg & FLG_BLOCK_SUM) && a.got[r] != a.sum[r]) good = false;
        }
        if (ballot(!good)) ok = false;
    }
    if (!ok) {                                               /* handed back: the state is as it was */
        if (lane == 0) st->handedBack += 1;
        return;
    }
    for (uint32_t j = 0; j < pl.nblk; j++) {                 /* raw blocks: Inject */
        const long long r = row0 + j;
        if (uni(a.lc[r]) & 0x80000000u) wave_copy(j < pl.nfull ? out + (uint64_t)j * bs : buf, a.r.src + a.srcOff[r], bs, lane);
    }
    wave_sync();
    if (pl.part) wave_copy(out + (uint64_t)pl.nfull * bs, buf, pl.part, lane);
    if (pl.flg & FLG_CONTENT_SUM) {                          /* one update over the call's bytes in order (the straddling block whole) */
        fr_xxh_update(&st->content, out, (uint64_t)pl.nfull * bs, pl.opened != 0, lane);
        if (pl.part) fr_xxh_update(&st->content, buf, bs, false, lane);
    }
    wave_sync();
    if (lane == 0) {
        st->pos = pl.posAfter; st->clen = pl.clen; st->phase = FR_PHASE_OPEN; st->code = 0;
        st->flg = pl.flg; st->bd = pl.bd; st->bsize = pl.bs;
        st->pending = pl.part ? bs - pl.part : 0u;
        st->tail = pl.part ? bs : 0u;
        st->bytesRead += (uint64_t)pl.nfull * bs + pl.part;
        st->blocks += pl.nblk; st->fastBlocks += pl.nblk;
        if (DICT) st->dictEntry = entry[s];
        a.r.outLen[s] = (int64_t)((uint64_t)pl.nfull * bs + pl.part);
        a.done[s] = FR_PLAN_DONE;
    }
}

__global__ __launch_bounds__(64 * FR_WAVES_PER_WG) void k4_fr_commit_kernel(FrFastArgs a)
{
    fr_commit_body<false>(a, nullptr);
}

/* per stream: bytes read, the open frame's ContentLength (-1: no frame open, or it declares none), phase, code, blocks read, blocks
 * decoded straight into dst -- K4LZ4_FRQ_* words of out + s * K4LZ4_FRQ_WORDS */
constexpr int FRQ_WORDS = 8;
__global__ __launch_bounds__(256) void k4_fr_query_kernel(const uint8_t *store, const uint64_t *storeOff, int64_t *out, long long n)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const FrState *st = (const FrState *)(store + storeOff[s]);
    int64_t *o = out + s * FRQ_WORDS;
    o[0] = (int64_t)st->bytesRead;
    o[1] = st->phase == FR_PHASE_OPEN && (st->flg & FLG_SIZE) ? (int64_t)st->clen : -1;
    o[2] = st->phase;
    o[3] = st->phase == FR_PHASE_FAILED ? st->code : 0;
    o[4] = (int64_t)st->blocks;
    o[5] = (int64_t)st->direct;
    o[6] = (int64_t)st->fastBlocks;
    o[7] = (int64_t)st->handedBack;
}

}  // namespace k4
