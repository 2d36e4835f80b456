/*
 * k4lz4_legacy_stream.hpp -- lz4net's LZ4Stream written to and read from piece by piece (k4lz4_legacy_write_batch,
 * k4lz4_legacy_read_batch), on top of the block kernels and k4lz4_legacy.hpp's chunk parser.
 *
 * Writer.  Each call advances many LZ4Streams in Compress mode by one Write, Flush or Dispose (LZ4Stream.cs:209-243, :313-316,
 * :414-450).  The reference flushes lazily: a buffer that a Write fills exactly goes out when the next byte arrives, or at Flush /
 * Dispose (:425-439).  How many chunks a call emits and how many bytes stay pending follow from lengths alone (ls_w_model), so
 * the host builds the chunk table and advances the record without waiting for the device:
 *   k4_fw_copy_kernel      (k4lz4_frame_write.hpp, unchanged) stages the one chunk that straddles the store and the call's bytes
 *                          into a window: [store | head of src]
 *   -> the batch encoder   every chunk of every stream, one batch per level, cap U - 1 (compressed iff C < U)
 *   k4_ls_reclen_kernel    record bytes per chunk -> k4_legacy_scan_kernel (record offsets)
 *   k4_ls_assemble_kernel  one wave per chunk: the varints, then the block, or the raw bytes of a stored chunk
 *   k4_fw_copy_kernel      the tail of the call's bytes is appended to the store (after everything that reads the store)
 *   k4_ls_finish_kernel    outLen per stream
 *
 * Reader.  Each call advances many LZ4Streams in Decompress mode by one Read(count) (LZ4Stream.cs:349-377 over AcquireNextChunk,
 * :248-294).  How many chunks a read consumes depends on the data, so the state lives in the stream's DEVICE store: LsState
 * (source position, _bufferOffset, _bufferLength, the code) followed by one decoded chunk of at most maxBlockSize bytes.
 *   k4_ls_read_kernel      one wavefront per stream runs the loop as written: drain what is pending, parse the varints
 *                          (legacy_next_chunk: every check in the reference's order), decode the chunk with decode_block or copy
 *                          a stored one, copy out.  A chunk that fits wholly into what the read still wants is made in dst.
 *   k4_ls_plan_kernel      the direct path: one thread per stream walks ahead from the stored position over the chunk headers;
 *                          chunks wholly inside the read get rows for the batch decoder (cap U, straight into dst), the chunk
 *                          that straddles the read's end is decoded into the store
 *   k4_ls_commit_kernel    one wave per stream checks that every row decoded to its U, copies stored chunks and the straddler's
 *                          head, commits the state.  A stream with a defect in the planned range keeps its state and is replayed
 *                          by k4_ls_read_kernel in the same call, so the defect is reported where the reference meets it.
 * What differs from the reference, on purpose: a chunk whose U is above the reader's maxBlockSize is LG_BLOCK_SIZE (the reference
 * allocates a buffer of that size); a stream that has reported a code stays failed.
 */
#pragma once
#include <vector>
#include "k4lz4_legacy.hpp"
#include "k4lz4_frame_write.hpp"

namespace k4 {

constexpr int LG_BLOCK_SIZE = -8, LG_CLOSED = -9;     /* include/k4lz4.h K4LZ4_LEGACY_BLOCK_SIZE, _CLOSED */
constexpr int LS_OP_WRITE = 0, LS_OP_FLUSH = 1, LS_OP_CLOSE = 2;
constexpr int LS_OP_READ = 0, LS_OP_RESET = 1;

/* ---- writer: the model ------------------------------------------------------------------------------------------------- */
/* p pending bytes, L new ones, chunks of B: how many chunks the call emits, the last one's length, what stays pending.
 * WRITE: L > 0 emits max(0, ceil((p + L) / B) - 1) chunks of B -- the last buffer, even a full one, waits for the next byte;
 * FLUSH: the pending bytes as one chunk; CLOSE: the write, then the flush. */
struct LsWAfter { int64_t nch, last, pending; };
__host__ __device__ inline LsWAfter ls_w_model(int64_t B, int64_t p, int64_t L, int op)
{
    LsWAfter a{0, 0, p};
    if (op == LS_OP_FLUSH) { if (p > 0) a = LsWAfter{1, p, 0}; return a; }
    const int64_t total = p + L;
    const int64_t e = L > 0 ? (total + B - 1) / B - 1 : 0;
    a.nch = e; a.last = B; a.pending = total - B * e;
    if (op == LS_OP_CLOSE) {
        if (a.pending > 0) { a.nch++; a.last = a.pending; }
        a.pending = 0;
    }
    return a;
}
/* the most a call can emit: a record is 1 + at most 5 + 5 bytes of varints and at most U - 1 bytes, or 1 + 5 and U bytes */
inline int64_t ls_w_bound(const k4lz4_legacy_writer &w, int64_t L, int op)
{
    if (L < 0 || w.closed) return 0;
    const LsWAfter a = ls_w_model(w.blockSize, w.pending, op == LS_OP_FLUSH ? 0 : L, op);
    return a.nch ? (a.nch - 1) * ((int64_t)w.blockSize + 10) + a.last + 10 : 0;
}
inline int64_t ls_w_store_bytes(const k4lz4_legacy_writer &w) { return ((int64_t)w.blockSize + 63) / 64 * 64; }

/* ---- writer: the kernels ----------------------------------------------------------------------------------------------- */
struct LsWStream {
    unsigned long long out;      /* dstOff: the stream's output slot */
    unsigned long long first;    /* its first chunk among the call's */
    uint32_t nch;
    int32_t code;                /* < 0: refused, written to outLen; 0: runs; 1: left untouched */
    uint32_t high;
    uint32_t reserved;
};

struct LsWriteArgs {
    const LsWStream *streams;
    long long n, rows;
    const uint64_t *cSrc;        /* per chunk: where its bytes are (an address: the window, the store or the caller's source) */
    const uint64_t *cEnc;        /* ... its arena slot (an address) */
    const int32_t *cLen;         /* ... U */
    const uint32_t *owner;
    int32_t *cEncLen;            /* the encoder's result */
    uint64_t *recLen, *recOff;
};

__global__ __launch_bounds__(256) void k4_ls_reclen_kernel(LsWriteArgs a)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.rows) return;
    const int U = a.cLen[r], C = a.cEncLen[r];
    const bool comp = lw_compressed(U, C);
    a.recLen[r] = 1u + (uint64_t)varint_size((uint64_t)U) + (comp ? (uint64_t)varint_size((uint64_t)C) + (uint64_t)C : (uint64_t)U);
}

/* one wave per chunk: flags, U, [C], then the block from the arena or the chunk's own bytes (LZ4Stream.cs:229-240) */
__global__ __launch_bounds__(256) void k4_ls_assemble_kernel(LsWriteArgs a, uint8_t *dst)
{
    const int lane = lane_id();
    const long long r = (long long)blockIdx.x * 4 + (long long)uni(threadIdx.x >> 6);
    if (r >= a.rows) return;
    const LsWStream &s = a.streams[a.owner[r]];
    uint8_t *p = dst + s.out + (a.recOff[r] - a.recOff[s.first]);
    const int U = a.cLen[r], C = a.cEncLen[r];
    const bool comp = lw_compressed(U, C);
    const int hdr = 1 + varint_size((uint64_t)U) + (comp ? varint_size((uint64_t)C) : 0);
    if (lane == 0) {
        uint8_t *q = put_varint(p, (uint64_t)((comp ? 1 : 0) | (s.high ? 2 : 0)));
        q = put_varint(q, (uint64_t)U);
        if (comp) put_varint(q, (uint64_t)C);
    }
    if (comp) wave_copy(p + hdr, (const uint8_t *)(uintptr_t)a.cEnc[r], (uint32_t)C, lane);
    else wave_copy(p + hdr, (const uint8_t *)(uintptr_t)a.cSrc[r], (uint32_t)U, lane);
}

__global__ __launch_bounds__(256) void k4_ls_finish_kernel(LsWriteArgs a, int64_t *outLen)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const LsWStream &s = a.streams[i];
    if (s.code != 0) { outLen[i] = s.code < 0 ? (int64_t)s.code : 0; return; }
    long long r = 0;
    if (s.nch) {
        const unsigned long long l = s.first + s.nch - 1u;
        r = (long long)(a.recOff[l] + a.recLen[l] - a.recOff[s.first]);
        for (unsigned long long k = s.first; k <= l; k++)
            if (a.cLen[k] > 1 && a.cEncLen[k] == HC_NO_SCRATCH) { r = LG_NOT_ENCODED; break; }
    }
    outLen[i] = r;
}

/* ---- writer: the host's plan (k4lz4_capi.hip; tests/emu/emu_legacy_stream.cpp runs the same) ------------------------------
 * ls_w_layout decides the per-stream codes and sizes the call's scratch: the uploaded plan first (streams, pieces, the chunk
 * table), then what the kernels fill, then the windows and the arena.  ls_w_fill writes the plan for a scratch at `d`. */
struct LsWLayout {
    int64_t rows = 0, nfast = 0, nstage = 0, ntail = 0;
    size_t o_streams = 0, o_stage = 0, o_tail = 0, o_src = 0, o_enc = 0, o_len = 0, o_cap = 0, o_owner = 0, plan_bytes = 0;
    size_t o_elen = 0, o_rlen = 0, o_roff = 0, o_cnt = 0, o_win = 0, o_arena = 0, total = 0;
    unsigned long long stage_chunks = 0, tail_chunks = 0;
};
inline size_t ls_take(size_t &at, size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; }
inline bool ls_w_staged(const k4lz4_legacy_writer &w, const LsWAfter &a) { return a.nch > 0 && w.pending > 0 && w.pending < (a.nch > 1 ? (int64_t)w.blockSize : a.last); }

/* code[i]: 1 untouched, 0 runs, < 0 refused */
inline void ls_w_layout(const k4lz4_legacy_writer *w, const int64_t *srcLen, const uint64_t *dstCap, int64_t n, int op,
                        std::vector<int32_t> &code, LsWLayout &L)
{
    code.assign((size_t)n, 1);
    size_t win = 0, arena = 0;
    for (int64_t i = 0; i < n; i++) {
        if (srcLen[i] < 0) continue;
        if (w[i].closed) { code[(size_t)i] = LG_CLOSED; continue; }
        if ((int64_t)std::min<uint64_t>(dstCap[i], (uint64_t)INT64_MAX) < ls_w_bound(w[i], srcLen[i], op)) { code[(size_t)i] = LG_CAPACITY; continue; }
        code[(size_t)i] = 0;
        const int64_t len = op == LS_OP_FLUSH ? 0 : srcLen[i];
        const LsWAfter a = ls_w_model(w[i].blockSize, w[i].pending, len, op);
        L.rows += a.nch;
        if (!w[i].high) L.nfast += a.nch;
        if (ls_w_staged(w[i], a)) { L.nstage += 2; win += (size_t)((a.nch > 1 ? w[i].blockSize : a.last) + 31) & ~(size_t)15; }
        if (a.pending > 0 && len > 0) L.ntail += 1;
        arena += (size_t)((a.nch > 1 ? (a.nch - 1) * (((int64_t)w[i].blockSize + 15) & ~(int64_t)15) : 0) + (a.nch ? (a.last + 15) & ~(int64_t)15 : 0));
    }
    size_t at = 0;
    const size_t rows = (size_t)L.rows;
    L.o_streams = ls_take(at, (size_t)n * sizeof(LsWStream));
    L.o_stage = ls_take(at, (size_t)L.nstage * sizeof(FwPiece)); L.o_tail = ls_take(at, (size_t)L.ntail * sizeof(FwPiece));
    L.o_src = ls_take(at, rows * 8); L.o_enc = ls_take(at, rows * 8); L.o_len = ls_take(at, rows * 4); L.o_cap = ls_take(at, rows * 4);
    L.o_owner = ls_take(at, rows * 4);
    L.plan_bytes = at;
    L.o_elen = ls_take(at, rows * 4); L.o_rlen = ls_take(at, rows * 8); L.o_roff = ls_take(at, rows * 8); L.o_cnt = ls_take(at, 64);
    L.o_win = ls_take(at, win); L.o_arena = ls_take(at, arena);
    L.total = at + 64;
}

/* h: plan_bytes of host memory; d: the device scratch the plan is uploaded to (the addresses in the plan point into it) */
inline void ls_w_fill(const k4lz4_legacy_writer *w, uint8_t *store, const uint64_t *storeOff, const uint8_t *src, const uint64_t *srcOff,
                      const int64_t *srcLen, const uint64_t *dstOff, int64_t n, int op, const std::vector<int32_t> &code, LsWLayout &L,
                      uint8_t *h, uint8_t *d)
{
    LsWStream *hs = (LsWStream *)(h + L.o_streams);
    FwPiece *hstage = (FwPiece *)(h + L.o_stage), *htail = (FwPiece *)(h + L.o_tail);
    uint64_t *hsrc = (uint64_t *)(h + L.o_src), *henc = (uint64_t *)(h + L.o_enc);
    int32_t *hlen = (int32_t *)(h + L.o_len), *hcap = (int32_t *)(h + L.o_cap);
    uint32_t *howner = (uint32_t *)(h + L.o_owner);
    int64_t rf = 0, rh = L.nfast, ks = 0, kt = 0;
    size_t win = L.o_win, arena = L.o_arena;
    for (int64_t i = 0; i < n; i++) {
        LsWStream &row = hs[i];
        row = LsWStream{dstOff[i], 0ull, 0u, code[(size_t)i], w[i].high ? 1u : 0u, 0u};
        if (row.code != 0) continue;
        const int64_t B = w[i].blockSize, p = w[i].pending, len = op == LS_OP_FLUSH ? 0 : srcLen[i];
        const LsWAfter a = ls_w_model(B, p, len, op);
        uint8_t *sto = store + storeOff[i];
        const uint8_t *in = len > 0 ? src + srcOff[i] : nullptr;
        int64_t &r = w[i].high ? rh : rf;
        row.first = (unsigned long long)r; row.nch = (uint32_t)a.nch;
        for (int64_t k = 0; k < a.nch; k++, r++) {
            const int64_t U = k + 1 < a.nch ? B : a.last;
            const int64_t at = k * B;                                /* in [store | src] */
            const uint8_t *from;
            if (k == 0 && ls_w_staged(w[i], a)) {
                uint8_t *wp = d + win;
                win += (size_t)(U + 31) & ~(size_t)15;
                hstage[ks++] = FwPiece{wp, sto, (unsigned long long)p, 0};
                hstage[ks++] = FwPiece{wp + p, in, (unsigned long long)(U - p), 0};
                from = wp;
            } else {
                from = at < p ? sto : in + (at - p);                 /* a chunk that lies wholly in the store is encoded where it is */
            }
            hsrc[r] = (uint64_t)(uintptr_t)from; hlen[r] = (int32_t)U; hcap[r] = (int32_t)U - 1;
            henc[r] = (uint64_t)(uintptr_t)(d + arena); arena += (size_t)(U + 15) & ~(size_t)15;
            howner[r] = (uint32_t)i;
        }
        if (a.pending > 0 && len > 0)                                /* the tail: behind the pending bytes, or a fresh buffer's first bytes */
            htail[kt++] = a.nch ? FwPiece{sto, in + (len - a.pending), (unsigned long long)a.pending, 0}
                                : FwPiece{sto + p, in, (unsigned long long)len, 0};
    }
    auto chunks = [](FwPiece *pc, int64_t cnt) {
        unsigned long long c = 0;
        for (int64_t k = 0; k < cnt; k++) { pc[k].chunk0 = c; c += std::max<unsigned long long>(1, (pc[k].len + FW_CHUNK - 1) / FW_CHUNK); }
        return c;
    };
    L.stage_chunks = chunks(hstage, ks); L.tail_chunks = chunks(htail, kt);
}

inline void ls_w_advance(k4lz4_legacy_writer &w, int64_t srcLen, int op)
{
    w.pending = (int32_t)ls_w_model(w.blockSize, w.pending, op == LS_OP_FLUSH ? 0 : srcLen, op).pending;
    if (op == LS_OP_CLOSE) w.closed = 1;
}

/* ---- reader ------------------------------------------------------------------------------------------------------------ */
constexpr int64_t LS_STATE_BYTES = 256;
constexpr uint32_t LS_PLAN_NONE = 0, LS_PLAN_DIRECT = 1, LS_PLAN_DONE = 2;
constexpr long long LS_MAX_ROWS = 1024;

struct LsState {
    unsigned long long pos;          /* next unread byte of the source, relative to srcOff[s] */
    unsigned long long bytesRead;    /* bytes delivered so far */
    unsigned long long chunks;       /* chunks acquired (those that produce bytes) */
    unsigned long long direct;       /* of those, made in dst by the general kernel */
    unsigned long long batched;      /* of those, decoded by the batch decoder on the direct path */
    unsigned long long handedBack;   /* calls in which the direct path handed the stream back to the general kernel */
    uint32_t bufOff, bufLen;         /* _bufferOffset, _bufferLength */
    int32_t code;
    uint32_t failed;
};
static_assert(sizeof(LsState) <= (size_t)LS_STATE_BYTES, "LsState outgrew its slot");

__host__ __device__ inline int64_t ls_rd_store_bytes(int64_t maxBlock) { return LS_STATE_BYTES + ((maxBlock + 64 + 255) & ~(int64_t)255); }
__host__ __device__ inline long long ls_table_rows(long long maxCount, long long maxBlock)
{
    if (maxCount <= 0 || maxBlock <= 0) return 0;
    const long long r = maxCount / maxBlock + 2;
    return r < LS_MAX_ROWS ? r : LS_MAX_ROWS;
}

struct LsReadArgs {
    const uint8_t *src;
    const uint64_t *srcOff, *srcLen;
    uint8_t *store;
    const uint64_t *storeOff;
    uint8_t *dst;
    const uint64_t *dstOff;
    const int64_t *count;            /* bytes wanted; < 0: the stream sits this call out */
    int64_t *outLen;
    long long n;
    int op;                          /* LS_OP_READ / LS_OP_RESET */
    int interactive;
    int32_t maxBlock;
    const uint32_t *done;            /* per stream: LS_PLAN_DONE where the direct path has served the call, or nullptr */
};

constexpr int LS_WAVES_PER_WG = DECODE_WAVES_PER_WG;

__global__ __launch_bounds__(64 * LS_WAVES_PER_WG) void k4_ls_read_kernel(LsReadArgs a)
{
    __shared__ uint32_t lds[LS_WAVES_PER_WG][DECODE_LDS_DWORDS];
    const int lane = lane_id();
    const uint32_t wave = uni(threadIdx.x >> 6);
    const long long s = (long long)blockIdx.x * LS_WAVES_PER_WG + (long long)wave;
    if (s >= a.n) return;
    if (a.done && a.done[s] == LS_PLAN_DONE) return;
    const int64_t want = a.count[s];
    if (want < 0) {
        if (lane == 0) a.outLen[s] = 0;
        return;
    }
    LsState *st = (LsState *)(a.store + a.storeOff[s]);
    uint8_t *buf = (uint8_t *)st + LS_STATE_BYTES;
    if (a.op == LS_OP_RESET) {
        uint32_t *w = (uint32_t *)st;
        if (lane < (int)(LS_STATE_BYTES / 4)) w[lane] = 0u;
        if (lane == 0) a.outLen[s] = 0;
        return;
    }
    /* the state, the same in every lane */
    uint64_t pos = st->pos, bytes_read = st->bytesRead, chunks = st->chunks, direct = st->direct;
    uint32_t buf_off = st->bufOff, buf_len = st->bufLen;
    int code = st->code;
    const uint32_t failed = st->failed;
    wave_sync();
    if (failed) {                                            /* failed streams stay failed and touch nothing */
        if (lane == 0) a.outLen[s] = code;
        return;
    }
    const uint8_t *p = a.src + a.srcOff[s];
    const uint64_t end = a.srcLen[s];
    uint8_t *out = a.dst + a.dstOff[s];
    uint64_t offset = 0, count = (uint64_t)want;
    int fail = 0;
    while (count > 0) {                                      /* Read (LZ4Stream.cs:355-374) */
        const uint32_t have = buf_len - buf_off;
        if (have == 0) {
            /* ---- AcquireNextChunk (:248-294); an empty chunk goes round again (:291) */
            LegacyChunk c;
            const int k = legacy_next_chunk(p, end, &pos, &c);
            if (k == 0) break;                               /* the legitimate end: the read ends with what it has */
            if (k < 0) { fail = k; break; }
            if (c.U > a.maxBlock) { fail = LG_BLOCK_SIZE; break; }
            if (c.U == 0) continue;
            const uint32_t U = (uint32_t)c.U;
            const bool to_dst = count >= U;                  /* the whole chunk is wanted: made where it is delivered */
            uint8_t *made = to_dst ? out + offset : buf;
            wave_sync();
            if (c.comp) {
                const int ret = decode_block(p + c.off, c.C, made, c.U, lane, lds[wave]);
                wave_sync();
                if (ret != c.U) { fail = LG_INVALID_DATA; break; }      /* :283-284 */
            } else {
                wave_copy(made, p + c.off, U, lane);
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
    wave_sync();
    if (lane == 0) {
        st->pos = pos; st->bytesRead = bytes_read; st->chunks = chunks; st->direct = direct;
        st->bufOff = buf_off; st->bufLen = buf_len;
        if (fail) { st->failed = 1u; st->code = fail; }
        a.outLen[s] = fail ? (int64_t)fail : (int64_t)offset;
    }
}

/* ---- the direct path ------------------------------------------------------------------------------------------------------ */
struct LsPlan {
    unsigned long long posAfter;     /* source position behind the last chunk walked */
    unsigned long long delivered;    /* bytes of the whole chunks */
    unsigned long long sRawOff;      /* the straddling chunk's payload when it is stored, relative to src */
    uint32_t state;                  /* LS_PLAN_* */
    uint32_t nrows;                  /* whole chunks: rows [s * rows, s * rows + nrows) */
    uint32_t part;                   /* bytes of the straddling chunk the read takes (0: none) */
    uint32_t sU;                     /* its U */
    uint32_t sRaw;
    uint32_t reserved;
};

struct LsDirectArgs {
    LsReadArgs r;
    LsPlan *plan;
    uint32_t *done;
    long long rows;                  /* table rows per stream */
    /* per row: the batch decoder's arguments (srcLen 0: a stored chunk of rawLen bytes, or an unused row) */
    uint64_t *srcOff, *dstOff;
    int32_t *srcLen, *dstCap, *outLen;
    uint32_t *rawLen;
    /* per stream: the straddling chunk, decoded into the store's buffer (offsets from r.store) */
    uint64_t *sSrcOff, *sDstOff;
    int32_t *sSrcLen, *sDstCap, *sOutLen;
};

__global__ __launch_bounds__(256) void k4_ls_plan_kernel(LsDirectArgs a)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.r.n) return;
    LsPlan pl{};
    a.sSrcLen[s] = 0; a.sDstCap[s] = 0; a.sSrcOff[s] = 0; a.sDstOff[s] = 0; a.sOutLen[s] = 0;
    const long long row0 = s * a.rows;
    const int64_t want = a.r.count[s];
    const LsState *st = (const LsState *)(a.r.store + a.r.storeOff[s]);
    uint32_t used = 0;
    do {
        if (want <= 0 || a.r.interactive || st->failed || st->bufOff < st->bufLen) break;
        const uint8_t *p = a.r.src + a.r.srcOff[s];
        const uint64_t end = a.r.srcLen[s];
        uint64_t pos = st->pos, left = (uint64_t)want, given = 0;
        bool ok = true;
        while (left > 0) {
            LegacyChunk c;
            const int k = legacy_next_chunk(p, end, &pos, &c);
            if (k == 0) break;                                        /* the source ends inside the read */
            if (k < 0 || c.U > a.r.maxBlock) { ok = false; break; }   /* a defect: the general kernel reports it where it is met */
            if (c.U == 0) continue;
            const uint64_t U = (uint64_t)c.U;
            if (left >= U) {
                if ((long long)used >= a.rows) { ok = false; break; } /* more chunks than rows */
                const long long r = row0 + used;
                a.srcOff[r] = a.r.srcOff[s] + c.off; a.dstOff[r] = a.r.dstOff[s] + given;
                a.srcLen[r] = c.comp ? c.C : 0; a.dstCap[r] = c.comp ? c.U : 0; a.outLen[r] = 0;
                a.rawLen[r] = c.comp ? 0u : (uint32_t)U;
                used++;
                given += U; left -= U;
            } else {                                                  /* the straddling chunk: into the buffer */
                pl.part = (uint32_t)left; pl.sU = (uint32_t)U; pl.sRaw = c.comp ? 0u : 1u; pl.sRawOff = a.r.srcOff[s] + c.off;
                if (c.comp) {
                    a.sSrcOff[s] = a.r.srcOff[s] + c.off; a.sSrcLen[s] = c.C;
                    a.sDstOff[s] = a.r.storeOff[s] + (uint64_t)LS_STATE_BYTES; a.sDstCap[s] = c.U;
                }
                left = 0;
            }
        }
        if (!ok) break;
        pl.state = LS_PLAN_DIRECT;
        pl.posAfter = pos; pl.delivered = given; pl.nrows = used;
    } while (0);
    if (pl.state != LS_PLAN_DIRECT) {                        /* nothing of a stream that is not taken goes to the decoder */
        a.sSrcLen[s] = 0; a.sDstCap[s] = 0;
        used = 0;
    }
    for (long long j = used; j < a.rows; j++) {
        a.srcLen[row0 + j] = 0; a.dstCap[row0 + j] = 0; a.srcOff[row0 + j] = 0; a.dstOff[row0 + j] = 0; a.rawLen[row0 + j] = 0u;
    }
    a.plan[s] = pl;
    a.done[s] = LS_PLAN_NONE;
}

__global__ __launch_bounds__(64 * LS_WAVES_PER_WG) void k4_ls_commit_kernel(LsDirectArgs a)
{
    const int lane = lane_id();
    const long long s = (long long)blockIdx.x * LS_WAVES_PER_WG + (long long)uni(threadIdx.x >> 6);
    if (s >= a.r.n) return;
    const LsPlan pl = a.plan[s];
    if (pl.state != LS_PLAN_DIRECT) return;
    LsState *st = (LsState *)(a.r.store + a.r.storeOff[s]);
    uint8_t *buf = (uint8_t *)st + LS_STATE_BYTES;
    uint8_t *out = a.r.dst + a.r.dstOff[s];
    const long long row0 = s * a.rows;
    /* every compressed chunk decoded to exactly its U (LZ4Stream.cs:283-284) */
    bool ok = true;
    for (uint32_t j0 = 0; j0 < pl.nrows; j0 += 64u) {
        const uint32_t j = j0 + (uint32_t)lane;
        bool good = true;
        if (j < pl.nrows && a.srcLen[row0 + j] > 0) good = a.outLen[row0 + j] == a.dstCap[row0 + j];
        if (ballot(!good)) ok = false;
    }
    if (pl.part && !pl.sRaw && a.sOutLen[s] != (int32_t)pl.sU) ok = false;
    if (!ok) {                                               /* handed back: the state is as it was */
        if (lane == 0) st->handedBack += 1;
        return;
    }
    for (uint32_t j = 0; j < pl.nrows; j++) {                /* stored chunks */
        const uint32_t raw = uni(a.rawLen[row0 + j]);
        if (raw) wave_copy(a.r.dst + a.dstOff[row0 + j], a.r.src + a.srcOff[row0 + j], raw, lane);
    }
    if (pl.part) {
        if (pl.sRaw) wave_copy(buf, a.r.src + pl.sRawOff, pl.sU, lane);
        wave_sync();
        wave_copy(out + pl.delivered, buf, pl.part, lane);
    }
    wave_sync();
    if (lane == 0) {
        st->pos = pl.posAfter;
        st->bufOff = pl.part; st->bufLen = pl.part ? pl.sU : 0u;
        st->bytesRead += pl.delivered + pl.part;
        st->chunks += pl.nrows + (pl.part ? 1u : 0u);
        st->batched += pl.nrows + (pl.part ? 1u : 0u);
        a.r.outLen[s] = (int64_t)(pl.delivered + pl.part);
        a.done[s] = LS_PLAN_DONE;
    }
}

/* K4LZ4_LSQ_* words of out + s * LSQ_WORDS */
constexpr int LSQ_WORDS = 8;
__global__ __launch_bounds__(256) void k4_ls_query_kernel(const uint8_t *store, const uint64_t *storeOff, int64_t *out, long long n)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const LsState *st = (const LsState *)(store + storeOff[s]);
    int64_t *o = out + s * LSQ_WORDS;
    o[0] = (int64_t)st->pos;
    o[1] = (int64_t)st->bytesRead;
    o[2] = (int64_t)(st->bufLen - st->bufOff);
    o[3] = st->failed ? st->code : 0;
    o[4] = (int64_t)st->chunks;
    o[5] = (int64_t)st->direct;
    o[6] = (int64_t)st->batched;
    o[7] = (int64_t)st->handedBack;
}

}  // namespace k4
