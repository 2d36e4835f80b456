/*
 * k4lz4_legacy_feed.hpp -- the incremental LZ4Stream reader fed its source in pieces (k4lz4_legacy_read_fed_batch).
 *
 * k4lz4_legacy_stream.hpp reads a source that is all there at every call.  Here stream s's source is the concatenation of the pieces
 * given so far, and src[srcOff[s] .. + srcLen[s]) is the part of it the reader has not consumed yet; final[s] != 0 says that no byte
 * follows it.  The reference hides short reads of its inner stream in TryReadVarInt (LZ4Stream.cs:133-155: one byte at a time) and
 * in ReadBlock (:176-191: a loop until the payload is complete), so how a source is cut is invisible in what Read returns.  The
 * same here:
 *
 *   fields       a chunk's header (the flags varint, the U varint, the C varint of a compressed chunk: at most LS_HDR_MAX bytes,
 *                awaited one byte at a time, need 1) and its payload of C bytes (need: the bytes still missing).  A field wholly
 *                inside the piece is parsed and decoded FROM THE PIECE.  A field that the piece cuts goes to the stream's STASH
 *                (behind the reader's buffer in its store: LS_HDR_MAX header bytes, then a payload of at most maxBlockSize bytes)
 *                and the call ends starved: outLen is what was delivered so far, consumed == srcLen, need > 0.  While the stash is
 *                not empty the reader first tops it up from the piece and then decodes from the stash.  So a payload byte is copied
 *                at most once and only where a piece ends inside its chunk.
 *   refused      a chunk that is refused whatever its bytes are (U above maxBlockSize, passes != 0) has its payload counted, not
 *                kept (LsFeedExt::pass), and reports its code in the call that hands over the payload's last byte -- where the
 *                reference's ReadBlock returns.  C > U and C < 0 are reported in the call that completes the header.
 *   starved      only with final[s] == 0; with final, no byte left at a chunk boundary is the clean end and running out inside a
 *                header or a payload is LG_END_OF_STREAM.
 *
 *   k4_ls_feed_kernel          one wavefront per stream: k4_ls_read_kernel's loop with its source reads behind the stash
 *   k4_ls_feed_topup_kernel    the direct path's first step, one wave per stream: a kept header and / or payload that the head of the
 *                              piece completes is completed in the stash; a committed transition of its own (head[s]: the bytes of
 *                              the piece it consumed, from which every later step of the call starts)
 *   k4_ls_feed_plan_kernel /   4.16's direct path for pieces: streams that read with nothing pending and a stash that is empty or
 *   k4_ls_feed_commit_kernel   holds a whole chunk are planned -- the stash's chunk is row 0, the chunks WHOLLY IN THE PIECE follow,
 *                              bounded by the count; the chunk that straddles the read's end goes into the store's buffer.  Where
 *                              those do not satisfy the count the commit stashes the piece's tail (less than one chunk), sets need
 *                              and leaves the read starved.  A failed hypothesis is replayed by k4_ls_feed_kernel from the
 *                              topped-up state.  Rows hold addresses (the stash is not part of src): the decoder's bases are null.
 *
 * The kernels of k4lz4_legacy_stream.hpp are compiled from the same text as before; LsFeedExt lives in the spare bytes of the state's
 * slot behind LsState, which they never touch (a reset zeroes the whole slot).
 */
#pragma once
#include "k4lz4_legacy_stream.hpp"

namespace k4 {

constexpr int32_t LS_READER_FED = 1;             /* include/k4lz4.h K4LZ4_LREADER_FED */
constexpr uint32_t LS_HDR_MAX = 30;              /* three varints of at most ten bytes (TryReadVarInt stops at 64 bits) */

__host__ __device__ inline int64_t ls_stash_bytes(int64_t maxBlock) { return ((int64_t)LS_HDR_MAX + maxBlock + 255) & ~(int64_t)255; }
__host__ __device__ inline int64_t ls_fed_store_bytes(int64_t maxBlock) { return ls_rd_store_bytes(maxBlock) + ls_stash_bytes(maxBlock); }

/* behind LsState in the state's slot */
struct LsFeedExt {
    unsigned long long pass;         /* payload bytes of a refused chunk that have not gone by yet */
    uint32_t fill;                   /* bytes kept: phase 0 of a header, at the stash's start; phase 1 of the payload, behind LS_HDR_MAX */
    uint32_t want;                   /* the length the kept field waits for (0: nothing is awaited) */
    uint32_t phase;                  /* 0: at or inside a header; 1: the header is parsed (hFlags, hU, hC), inside its payload */
    uint32_t hFlags;
    int32_t hU, hC;
};
static_assert(sizeof(LsState) % 8 == 0 && sizeof(LsState) + sizeof(LsFeedExt) <= (size_t)LS_STATE_BYTES, "LsState and LsFeedExt outgrew the slot");

__host__ __device__ __forceinline__ LsFeedExt *ls_feed_ext(const LsState *st) { return (LsFeedExt *)((uint8_t *)st + sizeof(LsState)); }
__host__ __device__ __forceinline__ uint8_t *ls_feed_stash(const LsState *st, int32_t maxBlock) { return (uint8_t *)st + ls_rd_store_bytes(maxBlock); }

struct LsHeader { uint32_t flags; int32_t U, C; uint32_t len; };

/* the chunk header in the first `have` bytes of h: 1 = it is all there (h.len bytes), 0 = it is not.  TryReadVarInt's rule per
 * field (7 bits per byte, at most ten bytes), the two or three fields in ONE loop over the bytes: with a loop per varint hipcc lost
 * the flags word of a compressed chunk on gfx950 -- the register that held it across the C varint's loop was given to that loop,
 * in scalar and in vector registers alike (seen in the ISA, and on the GPU as compressed chunks copied like stored ones, where the
 * host emulator decoded them) -- so no value is carried across a later loop here. */
__host__ __device__ __forceinline__ int ls_header_scan(const uint8_t *h, uint32_t have, LsHeader *o)
{
    uint64_t v = 0;
    uint32_t flags = 0, U = 0, C = 0, field = 0, shift = 0;
    for (uint32_t pos = 0; pos < have;) {
        const uint32_t b = h[pos++];
        v += (uint64_t)(b & 0x7fu) << shift;
        shift += 7;
        if ((b & 0x80u) != 0 && shift < 64) continue;
        const uint32_t w = (uint32_t)v;
        flags = field == 0 ? w : flags;
        U = field == 1 ? w : U;
        C = field == 2 ? w : C;
        v = 0; shift = 0;
        if (++field == ((flags & 1u) ? 3u : 2u)) {
            o->flags = flags;
            o->U = (int32_t)U;
            o->C = (flags & 1u) ? (int32_t)C : (int32_t)U;
            o->len = pos;
            return 1;
        }
    }
    return 0;
}
/* what the header alone decides (LZ4Stream.cs:262-266) */
__host__ __device__ __forceinline__ int ls_header_code(const LsHeader &h) { return h.C > h.U ? LG_END_OF_STREAM : h.C < 0 ? LG_OVERFLOW : 0; }
/* refused whatever the payload's bytes are: it is counted, not kept */
__host__ __device__ __forceinline__ bool ls_refused(uint32_t flags, int32_t U, int32_t maxBlock)
{
    return ((flags & 1u) && ((int)flags >> 2) != 0) || U > maxBlock;
}
/* what is decided once the payload is there, in legacy_next_chunk's order, then the reader's limit */
__host__ __device__ __forceinline__ int ls_chunk_code(uint32_t flags, int32_t U, int32_t C, int32_t maxBlock)
{
    if (flags & 1u) {
        if (((int)flags >> 2) != 0) return LG_NOT_SUPPORTED;
        if (C == 0 ? U != 0 : (uint64_t)U > 255ull * (uint64_t)C + 32u) return LG_INVALID_DATA;
    }
    return U > maxBlock ? LG_BLOCK_SIZE : 0;
}

struct LsFeedArgs {
    LsReadArgs r;                    /* r.src .. r.srcLen: the pieces */
    const int64_t *final;            /* per stream: != 0 no byte follows the piece; nullptr: none is final */
    int64_t *consumed, *need;
    const uint32_t *head;            /* per stream: the bytes of the piece the top-up step has consumed already, or nullptr */
};

__global__ __launch_bounds__(64 * LS_WAVES_PER_WG) void k4_ls_feed_kernel(LsFeedArgs fa)
{
    __shared__ uint32_t lds[LS_WAVES_PER_WG][DECODE_LDS_DWORDS];
    const LsReadArgs &a = fa.r;
    const int lane = lane_id();
    const uint32_t wave = uni(threadIdx.x >> 6);
    const long long s = (long long)blockIdx.x * LS_WAVES_PER_WG + (long long)wave;
    if (s >= a.n) return;
    if (a.done && a.done[s] == LS_PLAN_DONE) return;
    const int64_t want = a.count[s];
    if (want < 0) {                                          /* untouched */
        if (lane == 0) { a.outLen[s] = 0; fa.consumed[s] = 0; fa.need[s] = 0; }
        return;
    }
    LsState *st = (LsState *)(a.store + a.storeOff[s]);
    LsFeedExt *ex = ls_feed_ext(st);
    uint8_t *buf = (uint8_t *)st + LS_STATE_BYTES;
    uint8_t *stash = ls_feed_stash(st, a.maxBlock);
    if (a.op == LS_OP_RESET) {
        uint32_t *w = (uint32_t *)st;
        if (lane < (int)(LS_STATE_BYTES / 4)) w[lane] = 0u;
        if (lane == 0) { a.outLen[s] = 0; fa.consumed[s] = 0; fa.need[s] = 0; }
        return;
    }
    /* the state, the same in every lane */
    uint64_t bytes_read = st->bytesRead, chunks = st->chunks, direct = st->direct, pass = ex->pass;
    uint32_t buf_off = st->bufOff, buf_len = st->bufLen, fill = ex->fill, phase = ex->phase, hflags = ex->hFlags;
    int32_t hU = ex->hU, hC = ex->hC;
    const int code = st->code;
    const uint32_t failed = st->failed;
    wave_sync();
    if (failed) {                                            /* failed streams stay failed and touch nothing */
        if (lane == 0) { a.outLen[s] = code; fa.consumed[s] = 0; fa.need[s] = 0; }
        return;
    }
    const uint8_t *p = a.src + a.srcOff[s];
    const uint64_t end = a.srcLen[s], at0 = fa.head ? (uint64_t)fa.head[s] : 0u;
    const bool fin = fa.final && fa.final[s] != 0;
    uint8_t *out = a.dst + a.dstOff[s];
    uint64_t at = at0, offset = 0, count = (uint64_t)want, need = 0;
    int fail = 0;
    while (count > 0) {                                      /* Read (LZ4Stream.cs:355-374) */
        const uint32_t have = buf_len - buf_off;
        if (have == 0) {
            /* ---- AcquireNextChunk (:248-294) over the fed source; an empty chunk goes round again (:291) */
            if (phase == 0u) {                               /* the header: in the piece, or in the stash after a top-up */
                LsHeader h;
                const uint64_t left = end - at;
                if (fill == 0u) {
                    if (ls_header_scan(p + at, left > LS_HDR_MAX ? LS_HDR_MAX : (uint32_t)left, &h)) {
                        at += h.len;
                    } else {                                 /* (fewer than LS_HDR_MAX bytes are left) */
                        if (fin) { if (left) fail = LG_END_OF_STREAM; break; }      /* nothing left: the legitimate end */
                        if (left) {
                            wave_sync();
                            wave_copy(stash, p + at, (uint32_t)left, lane);
                            wave_sync();
                        }
                        fill = (uint32_t)left; at = end; need = 1;
                        break;
                    }
                } else {
                    const uint32_t top = left < (uint64_t)(LS_HDR_MAX - fill) ? (uint32_t)left : LS_HDR_MAX - fill;
                    if (top) {
                        wave_sync();
                        wave_copy(stash + fill, p + at, top, lane);
                        wave_sync();
                    }
                    if (ls_header_scan(stash, fill + top, &h)) {
                        at += h.len - fill; fill = 0u;
                    } else {
                        fill += top; at += top;
                        if (fin) fail = LG_END_OF_STREAM; else need = 1;
                        break;
                    }
                }
                fail = ls_header_code(h);
                if (fail) break;
                hflags = h.flags; hU = h.U; hC = h.C;
                phase = 1u;
                pass = ls_refused(hflags, hU, a.maxBlock) ? (uint64_t)hC : 0u;
            }
            /* ---- ReadBlock (:176-191): C bytes */
            const uint64_t left = end - at;
            const uint32_t C = (uint32_t)hC, U = (uint32_t)hU;
            const uint8_t *payload;
            if (ls_refused(hflags, hU, a.maxBlock)) {
                const uint64_t take = left < pass ? left : pass;
                at += take; pass -= take;
                if (pass) { if (fin) fail = LG_END_OF_STREAM; else need = pass; }
                else fail = ls_chunk_code(hflags, hU, hC, a.maxBlock);
                break;
            }
            if (fill == 0u && left >= (uint64_t)C) {
                payload = p + at;
                at += C;
            } else {
                const uint32_t top = left < (uint64_t)(C - fill) ? (uint32_t)left : C - fill;
                if (top) {
                    wave_sync();
                    wave_copy(stash + LS_HDR_MAX + fill, p + at, top, lane);
                    wave_sync();
                }
                fill += top; at += top;
                if (fill < C) { if (fin) fail = LG_END_OF_STREAM; else need = C - fill; break; }
                payload = stash + LS_HDR_MAX;
                fill = 0u;
            }
            phase = 0u;
            fail = ls_chunk_code(hflags, hU, hC, a.maxBlock);
            if (fail) break;
            if (U == 0u) continue;
            const bool to_dst = count >= U;                  /* the whole chunk is wanted: made where it is delivered */
            uint8_t *made = to_dst ? out + offset : buf;
            wave_sync();
            if (hflags & 1u) {
                const int ret = decode_block(payload, hC, made, hU, lane, lds[wave]);
                wave_sync();
                if (ret != hU) { fail = LG_INVALID_DATA; break; }       /* :283-284 */
            } else {
                wave_copy(made, payload, U, lane);
                wave_sync();
            }
            chunks++;
            if (to_dst) {
                direct++;
                buf_off = buf_len = 0;
                bytes_read += U; offset += U; count -= U;
                if (a.interactive) break;
                continue;
            }
            buf_off = 0; buf_len = U;
            continue;
        }
        const uint32_t n = count < have ? (uint32_t)count : have;
        wave_sync();
        wave_copy(out + offset, buf + buf_off, n, lane);
        buf_off += n; bytes_read += n; offset += n; count -= n;
        if (a.interactive) break;                            /* :369 */
    }
    if (fail) need = 0;
    wave_sync();
    if (lane == 0) {
        st->pos += at - at0; st->bytesRead = bytes_read; st->chunks = chunks; st->direct = direct;
        st->bufOff = buf_off; st->bufLen = buf_len;
        if (fail) { st->failed = 1u; st->code = fail; }
        ex->pass = pass; ex->fill = fill; ex->phase = phase; ex->hFlags = hflags; ex->hU = hU; ex->hC = hC;
        ex->want = need ? (pass ? 0u : fill + (uint32_t)need) : 0u;
        a.outLen[s] = fail ? (int64_t)fail : (int64_t)offset;
        fa.consumed[s] = (int64_t)at;
        fa.need[s] = (int64_t)need;
    }
}

/* ---- the direct path for pieces ----------------------------------------------------------------------------------------------- */
struct LsFeedPlan {
    unsigned long long posAfter;     /* offset in the piece behind the last whole chunk walked */
    unsigned long long delivered;    /* bytes of the whole chunks */
    unsigned long long sRawAddr;     /* the straddling chunk's payload when it is stored (an address) */
    unsigned long long need;         /* != 0: the read is left starved */
    uint32_t state;                  /* LS_PLAN_* */
    uint32_t nrows;                  /* whole chunks: rows [s * rows, s * rows + nrows) */
    uint32_t part;                   /* bytes of the straddling chunk the read takes (0: none) */
    uint32_t sU;                     /* its U */
    uint32_t sRaw;
    uint32_t tail;                   /* bytes of the piece behind posAfter that the commit keeps: an incomplete header, or ... */
    uint32_t tailHdr;                /* ... a complete header of tailHdr bytes (tFlags, tU, tC) and what is there of its payload */
    uint32_t tFlags;
    int32_t tU, tC;
};

struct LsFeedDirectArgs {
    LsFeedArgs f;
    LsFeedPlan *plan;
    uint32_t *done;
    uint32_t *head;
    long long rows;                  /* table rows per stream */
    /* per row: the batch decoder's arguments, ADDRESSES for null bases (srcLen 0: a stored chunk of rawLen bytes, or an unused row) */
    uint64_t *srcAddr, *dstAddr;
    int32_t *srcLen, *dstCap, *outLen;
    uint32_t *rawLen;
    /* per stream: the straddling chunk, decoded into the store's buffer */
    uint64_t *sSrcAddr, *sDstAddr;
    int32_t *sSrcLen, *sDstCap, *sOutLen;
};

/* streams the direct path may take: they read, not interactively, with nothing pending in the buffer */
__device__ __forceinline__ bool ls_feed_direct_ok(const LsReadArgs &r, long long s, const LsState *st)
{
    return r.count[s] > 0 && !r.interactive && !st->failed && st->bufOff >= st->bufLen;
}

/* one wave per stream: the kept field is completed from the head of the piece when the piece has all of it */
__global__ __launch_bounds__(64 * LS_WAVES_PER_WG) void k4_ls_feed_topup_kernel(LsFeedDirectArgs a)
{
    const LsReadArgs &r = a.f.r;
    const int lane = lane_id();
    const long long s = (long long)blockIdx.x * LS_WAVES_PER_WG + (long long)uni(threadIdx.x >> 6);
    if (s >= r.n) return;
    if (lane == 0) a.head[s] = 0u;
    LsState *st = (LsState *)(r.store + r.storeOff[s]);
    LsFeedExt *ex = ls_feed_ext(st);
    if (!ls_feed_direct_ok(r, s, st)) return;
    const uint32_t phase = ex->phase, fill = ex->fill;
    LsHeader h{ex->hFlags, ex->hU, ex->hC, 0u};
    const bool passing = ex->pass != 0;
    wave_sync();
    if ((phase == 0u && fill == 0u) || passing) return;      /* nothing kept; a refused chunk goes by in the general reader */
    uint8_t *stash = ls_feed_stash(st, r.maxBlock);
    const uint8_t *p = r.src + r.srcOff[s];
    const uint64_t end = r.srcLen[s];
    uint64_t at = 0;
    uint32_t kept = fill;                                    /* of the payload */
    if (phase == 0u) {
        const uint32_t top = end < (uint64_t)(LS_HDR_MAX - fill) ? (uint32_t)end : LS_HDR_MAX - fill;
        if (top) {                                           /* (bytes behind fill are not part of the state until it is raised) */
            wave_copy(stash + fill, p, top, lane);
            wave_sync();
        }
        if (!ls_header_scan(stash, fill + top, &h)) return;
        if (ls_header_code(h) != 0) return;                  /* the general reader reports it */
        at = h.len - fill;
        kept = 0u;
    }
    if (ls_refused(h.flags, h.U, r.maxBlock)) return;
    const uint32_t C = (uint32_t)h.C;
    if (end - at < (uint64_t)(C - kept)) return;             /* still cut: the general reader keeps what there is and starves */
    wave_copy(stash + LS_HDR_MAX + kept, p + at, C - kept, lane);
    at += C - kept;
    wave_sync();
    if (lane == 0) {                                         /* the transition: a whole chunk waits in the stash */
        ex->phase = 1u; ex->hFlags = h.flags; ex->hU = h.U; ex->hC = h.C;
        ex->fill = C; ex->want = C;
        st->pos += at;
        a.head[s] = (uint32_t)at;
    }
}

__global__ __launch_bounds__(256) void k4_ls_feed_plan_kernel(LsFeedDirectArgs a)
{
    const LsReadArgs &r = a.f.r;
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= r.n) return;
    LsFeedPlan pl{};
    a.sSrcLen[s] = 0; a.sDstCap[s] = 0; a.sSrcAddr[s] = 0; a.sDstAddr[s] = 0; a.sOutLen[s] = 0;
    const long long row0 = s * a.rows;
    const LsState *st = (const LsState *)(r.store + r.storeOff[s]);
    const LsFeedExt *ex = ls_feed_ext(st);
    uint32_t used = 0;
    do {
        if (!ls_feed_direct_ok(r, s, st) || ex->pass != 0) break;
        const bool whole = ex->phase == 1u && ex->fill == (uint32_t)ex->hC && !ls_refused(ex->hFlags, ex->hU, r.maxBlock);
        if (!whole && (ex->phase != 0u || ex->fill != 0u)) break;      /* an incomplete field is kept: the general reader's */
        const uint8_t *p = r.src + r.srcOff[s];
        const uint64_t end = r.srcLen[s];
        const bool fin = a.f.final && a.f.final[s] != 0;
        uint64_t pos = a.head[s], left = (uint64_t)r.count[s], given = 0;
        bool ok = true;
        /* a chunk whose payload is at `from`: a row while the read wants all of it, else the straddling chunk */
        auto place = [&](const uint8_t *from, const LsHeader &h) {
            const uint64_t U = (uint64_t)h.U;
            const bool comp = (h.flags & 1u) != 0;
            if (left >= U) {
                if ((long long)used >= a.rows) { ok = false; return; }         /* more chunks than rows */
                const long long row = row0 + used;
                a.srcAddr[row] = (uint64_t)(uintptr_t)from; a.dstAddr[row] = (uint64_t)(uintptr_t)(r.dst + r.dstOff[s] + given);
                a.srcLen[row] = comp ? h.C : 0; a.dstCap[row] = comp ? h.U : 0; a.outLen[row] = 0;
                a.rawLen[row] = comp ? 0u : (uint32_t)U;
                used++;
                given += U; left -= U;
            } else {                                                          /* into the buffer */
                pl.part = (uint32_t)left; pl.sU = (uint32_t)U; pl.sRaw = comp ? 0u : 1u; pl.sRawAddr = (unsigned long long)(uintptr_t)from;
                if (comp) {
                    a.sSrcAddr[s] = (uint64_t)(uintptr_t)from; a.sSrcLen[s] = h.C;
                    a.sDstAddr[s] = (uint64_t)(uintptr_t)((const uint8_t *)st + LS_STATE_BYTES); a.sDstCap[s] = h.U;
                }
                left = 0;
            }
        };
        if (whole) {                                                          /* row 0: the chunk the top-up completed */
            const LsHeader h{ex->hFlags, ex->hU, ex->hC, 0u};
            if (ls_chunk_code(h.flags, h.U, h.C, r.maxBlock) != 0) break;
            if (h.U != 0) place(ls_feed_stash(st, r.maxBlock) + LS_HDR_MAX, h);
        }
        while (ok && left > 0) {                                              /* the chunks wholly in the piece */
            const uint64_t avail = end - pos;
            LsHeader h;
            if (!ls_header_scan(p + pos, avail > LS_HDR_MAX ? LS_HDR_MAX : (uint32_t)avail, &h)) { pl.tail = (uint32_t)avail; break; }
            if (ls_header_code(h) != 0 || ls_refused(h.flags, h.U, r.maxBlock)) { ok = false; break; }   /* reported where it is met */
            if (avail - h.len < (uint64_t)h.C) {
                if (avail > 0xffffffffull) { ok = false; break; }
                pl.tail = (uint32_t)avail; pl.tailHdr = h.len; pl.tFlags = h.flags; pl.tU = h.U; pl.tC = h.C;
                break;
            }
            if (ls_chunk_code(h.flags, h.U, h.C, r.maxBlock) != 0) { ok = false; break; }
            pos += h.len + (uint64_t)h.C;
            if (h.U != 0) place(p + pos - (uint64_t)h.C, h);
        }
        if (!ok) break;
        if (left > 0) {                                                       /* the piece's whole chunks do not satisfy the count */
            if (!fin) pl.need = pl.tailHdr ? (uint64_t)pl.tC - (pl.tail - pl.tailHdr) : 1u;
            else if (pl.tail) break;                                          /* it runs out inside a chunk: the general reader's code */
        }
        if (used == 0 && !pl.part) break;                                     /* nothing for the decoder */
        pl.state = LS_PLAN_DIRECT;
        pl.posAfter = pos; pl.delivered = given; pl.nrows = used;
    } while (0);
    if (pl.state != LS_PLAN_DIRECT) {                        /* nothing of a stream that is not taken goes to the decoder */
        pl = LsFeedPlan{};
        a.sSrcLen[s] = 0; a.sDstCap[s] = 0;
        used = 0;
    }
    for (long long j = used; j < a.rows; j++) {
        a.srcLen[row0 + j] = 0; a.dstCap[row0 + j] = 0; a.srcAddr[row0 + j] = 0; a.dstAddr[row0 + j] = 0; a.rawLen[row0 + j] = 0u;
    }
    a.plan[s] = pl;
    a.done[s] = LS_PLAN_NONE;
}

__global__ __launch_bounds__(64 * LS_WAVES_PER_WG) void k4_ls_feed_commit_kernel(LsFeedDirectArgs a)
{
    const LsReadArgs &r = a.f.r;
    const int lane = lane_id();
    const long long s = (long long)blockIdx.x * LS_WAVES_PER_WG + (long long)uni(threadIdx.x >> 6);
    if (s >= r.n) return;
    const LsFeedPlan pl = a.plan[s];
    if (pl.state != LS_PLAN_DIRECT) return;
    LsState *st = (LsState *)(r.store + r.storeOff[s]);
    LsFeedExt *ex = ls_feed_ext(st);
    uint8_t *buf = (uint8_t *)st + LS_STATE_BYTES;
    uint8_t *stash = ls_feed_stash(st, r.maxBlock);
    uint8_t *out = r.dst + r.dstOff[s];
    const uint8_t *p = r.src + r.srcOff[s];
    const long long row0 = s * a.rows;
    const uint32_t head = uni(a.head[s]);
    /* every compressed chunk decoded to exactly its U (LZ4Stream.cs:283-284) */
    bool ok = true;
    for (uint32_t j0 = 0; j0 < pl.nrows; j0 += 64u) {
        const uint32_t j = j0 + (uint32_t)lane;
        bool good = true;
        if (j < pl.nrows && a.srcLen[row0 + j] > 0) good = a.outLen[row0 + j] == a.dstCap[row0 + j];
        if (ballot(!good)) ok = false;
    }
    if (pl.part && !pl.sRaw && a.sOutLen[s] != (int32_t)pl.sU) ok = false;
    if (!ok) {                                               /* handed back: the state is as the top-up left it */
        if (lane == 0) st->handedBack += 1;
        return;
    }
    for (uint32_t j = 0; j < pl.nrows; j++) {                /* stored chunks */
        const uint32_t raw = uni(a.rawLen[row0 + j]);
        if (raw) wave_copy((uint8_t *)(uintptr_t)a.dstAddr[row0 + j], (const uint8_t *)(uintptr_t)a.srcAddr[row0 + j], raw, lane);
    }
    if (pl.part) {
        if (pl.sRaw) wave_copy(buf, (const uint8_t *)(uintptr_t)pl.sRawAddr, pl.sU, lane);
        wave_sync();
        wave_copy(out + pl.delivered, buf, pl.part, lane);
    }
    wave_sync();                                             /* the stash's chunk has been read: the piece's tail takes its place */
    const uint32_t kept = pl.tailHdr ? pl.tail - pl.tailHdr : pl.tail;
    if (pl.need && kept) wave_copy(pl.tailHdr ? stash + LS_HDR_MAX : stash, p + pl.posAfter + pl.tailHdr, kept, lane);
    wave_sync();
    if (lane == 0) {
        const uint64_t taken = pl.posAfter + (pl.need ? pl.tail : 0u);
        st->pos += taken - head;
        st->bufOff = pl.part; st->bufLen = pl.part ? pl.sU : 0u;
        st->bytesRead += pl.delivered + pl.part;
        st->chunks += pl.nrows + (pl.part ? 1u : 0u);
        st->batched += pl.nrows + (pl.part ? 1u : 0u);
        ex->pass = 0u;
        ex->phase = pl.need && pl.tailHdr ? 1u : 0u;
        ex->fill = pl.need ? kept : 0u;
        ex->want = pl.need ? kept + (uint32_t)pl.need : 0u;
        ex->hFlags = pl.tFlags; ex->hU = pl.tU; ex->hC = pl.tC;
        r.outLen[s] = (int64_t)(pl.delivered + pl.part);
        a.f.consumed[s] = (int64_t)taken;
        a.f.need[s] = (int64_t)pl.need;
        a.done[s] = LS_PLAN_DONE;
    }
}

}  // namespace k4
