/*
 * k4lz4_frame_feed.hpp -- the incremental frame reader fed its source in pieces (k4lz4_frame_read_fed_batch).
 *
 * k4lz4_frame_reader.hpp reads a source that is all there at every call.  Here stream s's source is the concatenation of the pieces
 * given so far, and src[srcOff[s] .. + srcLen[s]) is the part of it the reader has not consumed yet; final[s] != 0 says that no byte
 * follows it.  The reference hides short reads of its inner stream in TryReadBlock (Streams/Internal/ReaderExtensions.cs:10-28),
 * which loops until the field it wants is complete, so how a source is cut is invisible in what is delivered.  The same here:
 *
 *   fields       the magic (4), FLG / BD (2), the rest of the header once FLG is known, a length word (4), a payload plus its block
 *                checksum, the content checksum behind an EndMark.  A field wholly inside the piece is read and decoded FROM THE
 *                PIECE.  A field that the piece cuts goes to the stream's STASH (behind the reader's buffer in its store,
 *                4 + maxBlockSize + 4 bytes: a length word stays in front of its payload, a header's fields stay together) and the
 *                call ends starved: outLen is what was delivered so far, consumed == srcLen, need > 0 the bytes with which the
 *                field is complete.  While the stash is not empty the reader first tops it up from the piece to the awaited length
 *                and then decodes from the stash.  So a record is copied at most once and only where a piece ends inside it.
 *   starved      only with final[s] == 0; with final running out is what it is in 4.14 (nothing left before a frame: a clean end,
 *                anything else FR_EOF).  A defect the reference meets with the bytes present is reported when those bytes are
 *                present: a wrong magic after 4 bytes, a bad version after 6, a stored length above the block size after the
 *                length word.  The state is at a field boundary, so the loop of .async.cs:150-172 resumes where it stood.
 *   not starved  need == 0, consumed <= srcLen, the stash is empty: the caller presents the unconsumed rest first in the next call.
 *
 *   k4_fr_feed_kernel         one wavefront per stream: k4_fr_read_kernel's loop with its source reads behind fr_feed_field
 *   k4_fr_feed_plan_kernel /  the fast path of 4.14 for pieces: streams with an empty stash, nothing pending and an independent-
 *   k4_fr_feed_commit_kernel  block frame are planned over the records that are WHOLLY IN THE PIECE (full blocks), bounded by the
 *                             count; where those do not satisfy the count the commit stashes the piece's tail (less than one
 *                             record), sets need and leaves the read starved.  A failed hypothesis is replayed by k4_fr_feed_kernel.
 *
 * The existing kernels are compiled from the same text as before; FrState gained two words at its end that they never touch
 * (a reset zeroes them with the rest of the slot).
 */
#pragma once
#include "k4lz4_frame_reader.hpp"

namespace k4 {

constexpr int32_t FR_SETTING_FED = 1;            /* include/k4lz4.h K4LZ4_FREADER_FED */

/* the stash behind the buffer: a length word, the largest payload, its block checksum */
__host__ __device__ inline int64_t fr_stash_bytes(int64_t maxBlock) { return (4 + maxBlock + 4 + 255) & ~(int64_t)255; }
__host__ __device__ inline int64_t fr_fed_store_bytes(int64_t maxBlock) { return fr_store_bytes(maxBlock) + fr_stash_bytes(maxBlock); }

/* ReadHeader's order over the first `have` bytes of a header: the length with which its next field is complete (4 the magic, 6
 * FLG / BD, then the whole header), 0 when h holds the whole header, or the code of a defect that is visible already */
__device__ __forceinline__ int fr_header_want(const uint8_t *h, uint32_t have)
{
    if (have < 4u) return 4;
    if (ld32u(h) != FRAME_MAGIC) return FR_MAGIC;
    if (have < 6u) return 6;
    const uint32_t flg = h[4];
    if (((flg >> 6) & 0x11u) != 1u) return FR_VERSION;
    const uint32_t len = 6u + ((flg & FLG_SIZE) ? 8u : 0u) + ((flg & FLG_DICT) ? 4u : 0u) + 1u;
    return have < len ? (int)len : 0;
}

/* where a fed reader's bytes come from: the piece from `at` on, behind `fill` bytes of the stash.  The same in every lane. */
struct FrFeedSrc {
    const uint8_t *p;
    uint64_t at, end;
    uint8_t *stash;
    uint32_t fill;
};

/* the first `want` bytes of the field the reader stands at, contiguous: in the piece when the stash is empty, else in the stash
 * after a top-up from the piece.  nullptr: they are not all there yet. */
__device__ __forceinline__ const uint8_t *fr_feed_field(FrFeedSrc &f, uint32_t want, int lane)
{
    if (f.fill == 0u) return f.end - f.at >= (uint64_t)want ? f.p + f.at : nullptr;
    if (f.fill < want) {
        const uint64_t left = f.end - f.at;
        const uint32_t top = left < (uint64_t)(want - f.fill) ? (uint32_t)left : want - f.fill;
        if (top) {
            wave_sync();
            wave_copy(f.stash + f.fill, f.p + f.at, top, lane);
            wave_sync();
        }
        f.fill += top; f.at += top;
    }
    return f.fill >= want ? f.stash : nullptr;
}
/* the field of `len` bytes that fr_feed_field returned is consumed (its bytes stay where they are) */
__device__ __forceinline__ void fr_feed_take(FrFeedSrc &f, uint32_t len)
{
    if (f.fill) f.fill = 0u; else f.at += len;
}
/* starved: what the piece has of the field goes to the stash; returns the bytes still missing of `want` */
__device__ __forceinline__ uint32_t fr_feed_keep(FrFeedSrc &f, uint32_t want, int lane)
{
    if (f.fill == 0u) {
        const uint32_t n = (uint32_t)(f.end - f.at);
        if (n) {
            wave_sync();
            wave_copy(f.stash, f.p + f.at, n, lane);
            wave_sync();
        }
        f.fill = n; f.at = f.end;
    }
    return want - f.fill;
}

struct FrFeedArgs {
    FrReadArgs r;                    /* r.src .. r.srcLen: the pieces */
    const int64_t *final;            /* per stream: != 0 no byte follows the piece; nullptr: none is final */
    int64_t *consumed, *need;
};

/* the loop's text is k4lz4_frame_feed_loop.hpp, which k4_fr_dict_feed_kernel (k4lz4_frame_reader_dict.hpp) includes as well */
__global__ __launch_bounds__(64 * FR_WAVES_PER_WG) void k4_fr_feed_kernel(FrFeedArgs fa)
{
    __shared__ uint32_t lds[FR_WAVES_PER_WG][DECODE_LDS_DWORDS];
#define FR_LOOP_DICT 0
#include "k4lz4_frame_feed_loop.hpp"
#undef FR_LOOP_DICT
}

/* ---- the fast path for pieces -------------------------------------------------------------------------------------------------
 * FrFastArgs and its table as in k4lz4_frame_reader.hpp; per stream two more words: the piece's tail that the commit stashes and the
 * length the cut field is waiting for (0: the read is not starved). */
struct FrFeedFastArgs {
    FrFastArgs f;
    const int64_t *final;
    int64_t *consumed, *need;
    uint32_t *tail, *want;
};

/* k4_fr_feed_plan_kernel's body; DICT (k4_fr_dict_feed_plan_kernel) as in fr_plan_body */
template <bool DICT>
__device__ __forceinline__ void fr_feed_plan_body(const FrFeedFastArgs &fa, const FrDictRows &w)
{
    const FrFastArgs &a = fa.f;
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.r.n) return;
    FrPlan pl{};
    a.sSrcLen[s] = 0; a.sDstCap[s] = 0; a.sSrcOff[s] = 0; a.sDstOff[s] = 0; a.sOutLen[s] = 0;
    const long long row0 = s * a.rows;
    const int64_t want = a.r.count[s];
    const FrState *st = (const FrState *)(a.r.store + a.r.storeOff[s]);
    uint32_t used = 0, tl = 0, tw = 0, entry1 = 0;
    do {
        if (want <= 0 || a.r.interactive || st->phase == FR_PHASE_FAILED || st->pending != 0 || st->stashFill != 0) break;
        const uint8_t *p = a.r.src + a.r.srcOff[s];
        const uint64_t end = a.r.srcLen[s];
        uint64_t pos = 0;
        FrHeader hd{st->flg, st->bd, 0u, st->bsize, st->clen};
        if (st->phase != FR_PHASE_OPEN) {
            if (end == 0 || fr_parse_header_ids<DICT>(p, end, a.r.maxBlock, hd, w.d, entry1) != 0) break;
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
        uint64_t m = 0;
        for (uint64_t j = 0; j < k; j++) {
            const uint64_t left = end - pos;
            if (left < 4) { tw = 4u; break; }                /* the piece ends in front of, or inside, a length word */
            const uint32_t lc = ld32u(p + pos);
            const uint32_t sn = lc & 0x7fffffffu;
            const bool raw = (lc & 0x80000000u) != 0;
            if (lc == 0 || sn > bs || (raw && sn != bs)) { ok = false; break; }
            const uint32_t rl = 4u + sn + (bsum ? 4u : 0u);
            if (left < rl) { tw = rl; break; }               /* ... inside a record */
            const uint64_t at = a.r.srcOff[s] + pos + 4;
            const long long r = row0 + (long long)j;
            a.lc[r] = lc;
            a.srcOff[r] = at;
            a.hlen[r] = bsum ? sn : 0u;
            a.sum[r] = bsum ? ld32u(p + pos + 4 + sn) : 0u;
            a.srcLen[r] = 0; a.dstCap[r] = 0; a.outLen[r] = 0;
            a.dstOff[r] = a.r.dstOff[s] + j * bs;
            if (j < nfull) {
                if (!raw) { a.srcLen[r] = (int32_t)sn; a.dstCap[r] = (int32_t)bs; }
            } else if (!raw) {                               /* the straddling block: LZ4BlockDecoder's capacity, into the buffer */
                a.sSrcOff[s] = at; a.sSrcLen[s] = (int32_t)sn;
                a.sDstOff[s] = a.r.storeOff[s] + (uint64_t)FR_STATE_BYTES; a.sDstCap[s] = (int32_t)bs + 8;
            }
            used = (uint32_t)j + 1u;
            m = j + 1;
            pos += rl;
        }
        if (!ok) break;
        if (m < k) {                                         /* the piece's whole records do not satisfy the count */
            if (m == 0 || (fa.final && fa.final[s] != 0)) break;
            tl = (uint32_t)(end - pos);
        }
        pl.state = FR_PLAN_FAST;
        pl.posAfter = pos; pl.clen = hd.clen; pl.nblk = (uint32_t)m;
        pl.nfull = (uint32_t)(m < nfull ? m : nfull);
        pl.part = m == k ? (uint32_t)(need - nfull * bs) : 0u;
        pl.flg = hd.flg; pl.bd = hd.bd; pl.bs = hd.bs;
    } while (0);
    if (pl.state != FR_PLAN_FAST) {                          /* nothing of a stream that is not taken goes to the decoders */
        for (uint32_t j = 0; j < used; j++) { a.srcLen[row0 + j] = 0; a.hlen[row0 + j] = 0; }
        a.sSrcLen[s] = 0;
        used = 0; tl = 0; tw = 0;
    }
    for (long long j = used; j < a.rows; j++) { a.srcLen[row0 + j] = 0; a.dstCap[row0 + j] = 0; a.hlen[row0 + j] = 0; a.srcOff[row0 + j] = 0; a.dstOff[row0 + j] = 0; }
    a.plan[s] = pl;
    a.done[s] = FR_PLAN_NONE;
    fa.tail[s] = tl; fa.want[s] = tw;
    if (DICT) fr_plan_dict_rows(w, s, row0, a.rows, pl.state == FR_PLAN_FAST ? entry1 : 0u);
}

__global__ __launch_bounds__(256) void k4_fr_feed_plan_kernel(FrFeedFastArgs fa)
{
    fr_feed_plan_body<false>(fa, FrDictRows{});
}

/* k4_fr_feed_commit_kernel's body; entry (k4_fr_dict_feed_commit_kernel) as in fr_commit_body */
template <bool DICT>
__device__ __forceinline__ void fr_feed_commit_body(const FrFeedFastArgs &fa, const uint32_t *entry)
{
    const FrFastArgs &a = fa.f;
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
    const uint32_t tl = uni(fa.tail[s]), tw = uni(fa.want[s]);
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
    /* the piece's tail, less than one record, waits in the stash for the rest of its field */
    if (tl) wave_copy((uint8_t *)st + fr_store_bytes(a.r.maxBlock), a.r.src + a.r.srcOff[s] + pl.posAfter, tl, lane);
    wave_sync();
    if (lane == 0) {
        st->pos += pl.posAfter + tl; st->clen = pl.clen; st->phase = FR_PHASE_OPEN; st->code = 0;
        st->flg = pl.flg; st->bd = pl.bd; st->bsize = pl.bs;
        st->pending = pl.part ? bs - pl.part : 0u;
        st->tail = pl.part ? bs : 0u;
        st->bytesRead += (uint64_t)pl.nfull * bs + pl.part;
        st->blocks += pl.nblk; st->fastBlocks += pl.nblk;
        st->stashFill = tl; st->stashWant = tw;
        if (DICT) st->dictEntry = entry[s];
        a.r.outLen[s] = (int64_t)((uint64_t)pl.nfull * bs + pl.part);
        fa.consumed[s] = (int64_t)(pl.posAfter + tl);
        fa.need[s] = tw ? (int64_t)(tw - tl) : 0;
        a.done[s] = FR_PLAN_DONE;
    }
}

__global__ __launch_bounds__(64 * FR_WAVES_PER_WG) void k4_fr_feed_commit_kernel(FrFeedFastArgs fa)
{
    fr_feed_commit_body<false>(fa, nullptr);
}

}  // namespace k4
