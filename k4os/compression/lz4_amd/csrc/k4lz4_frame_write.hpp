/*
 * k4lz4_frame_write.hpp -- the incremental frame writer on the device (k4lz4_frame_write_batch).
 *
 * Each call advances many LZ4FrameWriters by one Write (Frames/LZ4FrameWriter.async.cs:29-47), an OpenFrame
 * (LZ4FrameWriter.cs:217) or a CloseFrame (LZ4FrameWriter.async.cs:59-90).  The host knows every length, so it lays out
 * where things go; these kernels move the bytes:
 *   k4_fw_xxh32_kernel   XXH32.Update over this call's bytes, four lanes per stream, the state (the published XXH32
 *                        streaming state: four accumulators, total length, up to 15 carried bytes) kept in the stream's store
 *   k4_fw_copy_kernel    a list of pieces (dst, src, len; src == nullptr: zeros): stages [ring | this call's bytes] into a
 *                        window the existing encoders read, and writes the ring (and a fast-chain state) back afterwards
 *   k4_fw_reclen_kernel  per block: record bytes (length word, payload, block checksum) and the stored payload length
 *   -> k4_legacy_scan_kernel (record offsets over the call's blocks) ->
 *   k4_fw_place_kernel   per block: where its record goes inside its stream's output slot
 *   -> k4_frame_blocks_kernel (the records) ->
 *   k4_fw_edges_kernel   per stream: the header (magic, FLG/BD, content size, header checksum byte) if the call opens the
 *                        frame, EndMark and content checksum if it closes it, and outLen
 * and, on the host, the record's model (fw_model: LZ4EncoderBase's ring over the call's window), the bound and the refusals.
 */
#pragma once
#include <algorithm>
#include "../../../../include/k4lz4.h"
#include "k4lz4_xxh32.hpp"
#include "k4lz4_frame.hpp"

namespace k4 {

/* XXH32's streaming state (XXH32_state_t: total_len_32 widened to 64 bits, v1..v4, mem32[4], memsize) */
struct FwXxhState {
    uint32_t acc[4];
    unsigned long long total;
    uint8_t mem[16];
    uint32_t memsize;
    uint32_t reserved;
};

struct FwHashItem {
    const uint8_t *data;         /* this call's bytes */
    unsigned long long len;
    FwXxhState *state;
    uint32_t fresh;              /* XXH32.Reset first (TryStashFrame -> InitializeContentChecksum) */
    uint32_t reserved;
};

constexpr int FW_THREADS = 256;

/* four lanes per stream, lane c owns accumulator c.  Every lane reads the state into registers first; a stripe that straddles the
 * carried bytes and this call's is put together bytewise. */
__global__ __launch_bounds__(FW_THREADS) void k4_fw_xxh32_kernel(const FwHashItem *items, long long n)
{
    const long long t = (long long)blockIdx.x * FW_THREADS + threadIdx.x;
    const long long g = t >> 2;
    const int c = (int)(t & 3);
    const bool live = g < n;
    const FwHashItem it = live ? items[g] : FwHashItem{nullptr, 0ull, nullptr, 1u, 0u};
    FwXxhState *st = it.state;
    uint32_t m[4] = {0u, 0u, 0u, 0u}, carried = 0u, v;
    unsigned long long total = 0ull;
    if (it.fresh) {                                      /* XXH32.Reset(seed 0) */
        v = c == 0 ? XXH_P1 + XXH_P2 : c == 1 ? XXH_P2 : c == 2 ? 0u : 0u - XXH_P1;
    } else {
        const uint32_t *w = (const uint32_t *)st->mem;
        m[0] = w[0]; m[1] = w[1]; m[2] = w[2]; m[3] = w[3];
        carried = st->memsize; total = st->total; v = st->acc[c];
    }
    const uint64_t len = it.len;
    const uint8_t *p = it.data;
    uint64_t at = 0;                                     /* where in this call's bytes the next whole stripe starts */
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
            /* as k4_xxh32_kernel: eight loads per chain in flight while the previous eight are folded in */
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
        carried = 0u;                                    /* the carried bytes went into the first stripe */
    }
    wave_sync();                                         /* every lane has read the state before any lane rewrites it */
    if (!live) return;
    st->acc[c] = v;
    if (c == 0) {
        const uint32_t rest = (uint32_t)(len - at);      /* < 16 - carried */
        if (it.fresh) { st->reserved = 0u; }
        for (uint32_t i = 0; i < rest; i++) st->mem[carried + i] = p[at + i];
        st->memsize = carried + rest;
        st->total = total + len;
    }
}

/* XXH32.Digest of a streaming state */
__device__ __forceinline__ uint32_t fw_xxh32_digest(const FwXxhState &st)
{
    uint32_t h = st.total >= 16u ? xxh_rotl(st.acc[0], 1) + xxh_rotl(st.acc[1], 7) + xxh_rotl(st.acc[2], 12) + xxh_rotl(st.acc[3], 18)
                                 : XXH_P5;        /* (seed 0: acc[2] is the seed) */
    h += (uint32_t)st.total;
    uint32_t i = 0;
    for (; i + 4 <= st.memsize; i += 4) {
        const uint32_t x = (uint32_t)st.mem[i] | ((uint32_t)st.mem[i + 1] << 8) | ((uint32_t)st.mem[i + 2] << 16) | ((uint32_t)st.mem[i + 3] << 24);
        h = xxh_rotl(h + x * XXH_P3, 17) * XXH_P4;
    }
    for (; i < st.memsize; i++) h = xxh_rotl(h + (uint32_t)st.mem[i] * XXH_P5, 11) * XXH_P1;
    h ^= h >> 15; h *= XXH_P2; h ^= h >> 13; h *= XXH_P3; h ^= h >> 16;
    return h;
}

/* XXH32.DigestOf of at most 15 bytes (the header's) */
__device__ __forceinline__ uint32_t fw_xxh32_small(const uint8_t *p, uint32_t len)
{
    uint32_t h = XXH_P5 + len, i = 0;
    for (; i + 4 <= len; i += 4) {
        const uint32_t x = (uint32_t)p[i] | ((uint32_t)p[i + 1] << 8) | ((uint32_t)p[i + 2] << 16) | ((uint32_t)p[i + 3] << 24);
        h = xxh_rotl(h + x * XXH_P3, 17) * XXH_P4;
    }
    for (; i < len; i++) h = xxh_rotl(h + (uint32_t)p[i] * XXH_P5, 11) * XXH_P1;
    h ^= h >> 15; h *= XXH_P2; h ^= h >> 13; h *= XXH_P3; h ^= h >> 16;
    return h;
}

/* ---- copies: pieces cut into FW_CHUNK-byte chunks, one workgroup per chunk ---------------------------------------------- */
constexpr uint32_t FW_CHUNK = 64u << 10;

struct FwPiece {
    uint8_t *dst;
    const uint8_t *src;          /* nullptr: zeros */
    unsigned long long len;
    unsigned long long chunk0;   /* the piece's first chunk among all the pieces' */
};

__global__ __launch_bounds__(FW_THREADS) void k4_fw_copy_kernel(const FwPiece *pieces, long long n)
{
    const unsigned long long chunk = blockIdx.x;
    long long lo = 0, hi = n - 1;                        /* the last piece whose chunk0 <= chunk */
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (pieces[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
    }
    const FwPiece pc = pieces[lo];
    const unsigned long long begin = (chunk - pc.chunk0) * FW_CHUNK;
    if (begin >= pc.len) return;
    const uint32_t len = (uint32_t)(pc.len - begin < FW_CHUNK ? pc.len - begin : FW_CHUNK);
    uint8_t *d = pc.dst + begin;
    if (!pc.src) {
        for (uint32_t k = threadIdx.x; k < len; k += FW_THREADS) d[k] = 0;
        return;
    }
    const uint8_t *s = pc.src + begin;
    const uint32_t nv = len >> 4;                        /* 16 bytes per lane and step (unaligned dwordx4), the rest bytewise */
    for (uint32_t v = threadIdx.x; v < nv; v += FW_THREADS) st128u(d + 16ull * v, ld128u(s + 16ull * v));
    for (uint32_t k = (nv << 4) + threadIdx.x; k < len; k += FW_THREADS) d[k] = s[k];
}

/* ---- records ---------------------------------------------------------------------------------------------------------------- */
/* per block: the stored payload length (for the block checksums) and the record's bytes; blocks from firstSum on carry a checksum */
__global__ __launch_bounds__(FW_THREADS) void k4_fw_reclen_kernel(const int32_t *outLen, unsigned long long *stored,
                                                                 unsigned long long *recLen, long long nb, long long firstSum)
{
    const long long b = (long long)blockIdx.x * FW_THREADS + threadIdx.x;
    if (b >= nb) return;
    const int32_t got = outLen[b];
    const unsigned long long n = (unsigned long long)(got < 0 ? -(long long)got : (long long)got);
    stored[b] = n;
    recLen[b] = n + 4u + (b >= firstSum ? 4u : 0u);
}

struct FwStream {
    unsigned long long out;      /* dstOff: the stream's output slot */
    unsigned long long first;    /* its first block among the call's */
    uint32_t nblk;
    int32_t code;                /* < 0: refused (K4LZ4_FWRITE_*), written to outLen; 0: runs; 1: left untouched */
    uint32_t hdrLen;             /* FLG..: 2 or 10 bytes, 0: the call does not open the frame */
    uint32_t close;              /* 1: EndMark; 2: EndMark and content checksum */
    uint8_t hdr[16];
    const FwXxhState *xxh;
};

/* per block: its record's offset in dst -- its stream's slot, behind the header, at the exclusive scan of the records before it */
__global__ __launch_bounds__(FW_THREADS) void k4_fw_place_kernel(const FwStream *streams, const uint32_t *owner,
                                                                const unsigned long long *excl, unsigned long long *recOff, long long nb)
{
    const long long b = (long long)blockIdx.x * FW_THREADS + threadIdx.x;
    if (b >= nb) return;
    const FwStream &s = streams[owner[b]];
    const uint32_t head = s.hdrLen ? 4u + s.hdrLen + 1u : 0u;
    recOff[b] = s.out + head + excl[b] - excl[s.first];
}

/* per stream: header, tail, outLen (LZ4FrameWriter.cs:57-108; LZ4FrameWriter.async.cs:75-90) */
__global__ __launch_bounds__(FW_THREADS) void k4_fw_edges_kernel(const FwStream *streams, const unsigned long long *excl,
                                                                const unsigned long long *recLen, uint8_t *dst, long long *outLen, long long n)
{
    const long long i = (long long)blockIdx.x * FW_THREADS + threadIdx.x;
    if (i >= n) return;
    const FwStream &s = streams[i];
    if (s.code != 0) { outLen[i] = s.code < 0 ? (long long)s.code : 0ll; return; }
    uint8_t *p = dst + s.out;
    unsigned long long at = 0;
    if (s.hdrLen) {
        ((U32u *)p)->v = 0x184D2204u;
        for (uint32_t k = 0; k < s.hdrLen; k++) p[4 + k] = s.hdr[k];
        p[4 + s.hdrLen] = (uint8_t)(fw_xxh32_small(s.hdr, s.hdrLen) >> 8);
        at = 4u + s.hdrLen + 1u;
    }
    if (s.nblk) {
        const unsigned long long last = s.first + s.nblk - 1u;
        at += excl[last] + recLen[last] - excl[s.first];
    }
    if (s.close) {
        ((U32u *)(p + at))->v = 0u;
        at += 4u;
        if (s.close == 2) { ((U32u *)(p + at))->v = fw_xxh32_digest(*s.xxh); at += 4u; }
    }
    outLen[i] = (long long)at;
}

/* ---- host side: the record, the model, the bound (k4lz4_capi.hip; tests/emu/emu_frame_write.cpp runs the same).  A stream's store: its XXH32 state (64 bytes), for chained
 * fast streams its k4lz4_fast_chain_state, then the encoder's ring buffer. */
constexpr int64_t FW_XXH_BYTES = 64;
constexpr int64_t FW_STATE_BYTES = ((int64_t)sizeof(k4lz4_fast_chain_state) + 63) / 64 * 64;
constexpr int64_t FW_CHAIN_LIMIT = ((int64_t)1 << 31) - 65536;     /* encoders.HC_CHAIN_LIMIT; the fast chain's is checked per block */

inline int64_t fw_ring_at(const k4lz4_frame_writer &w) { return FW_XXH_BYTES + (w.kind == 2 ? FW_STATE_BYTES : 0); }
inline int64_t fw_slot(const k4lz4_frame_writer &w) { return (int64_t)w.encBlock + w.encBlock / 255 + 16; }

/* FLG, BD [, content size]: the bytes the header checksum covers (LZ4FrameWriter.cs:65-100) */
inline uint32_t fw_header(const k4lz4_frame_writer &w, uint8_t *h)
{
    const k4lz4_frame_writer_settings &s = w.settings;
    const int bs = s.blockSize;
    const int code = bs <= (64 << 10) ? 4 : bs <= (256 << 10) ? 5 : bs <= (1 << 20) ? 6 : 7;
    h[0] = (uint8_t)((1 << 6) | ((s.chainBlocks ? 0 : 1) << 5) | ((s.blockChecksum ? 1 : 0) << 4) | ((s.contentLength >= 0 ? 1 : 0) << 3) |
                     ((s.contentChecksum ? 1 : 0) << 2));
    h[1] = (uint8_t)(code << 4);
    if (s.contentLength < 0) return 2;
    for (int i = 0; i < 8; i++) h[2 + i] = (uint8_t)((uint64_t)s.contentLength >> (8 * i));
    return 10;
}

/* does this call open the frame: a Write (even an empty one, TryStashFrame in WriteManyBytes), an OpenFrame, or a CloseFrame that
 * writes bytes first; a CloseFrame of a stream never opened writes nothing (_encoder == null) */
inline bool fw_opens(const k4lz4_frame_writer &w, int64_t srcLen, bool closing) { return w.phase == 0 && !(closing && srcLen == 0); }

/* where the ring stands after a call: LZ4EncoderBase's Topup / Encode / Commit in window coordinates (the window is the ring's
 * bytes followed by this call's), as encoders.py's hc_chain_blocks / fast_chain_blocks model it -- every block that fills up is
 * encoded (TopupAndEncode(forceEncode: false)), at close the rest too (FlushAndEncode).  block(start, len) per block. */
struct FwAfter {
    int64_t index = 0, pointer = 0, ws = 0, nblk = 0;   /* ws: the window position the ring's first byte comes from */
    uint32_t cur = 0, dict = 0;
    bool too_long = false;
};

template <class Block>
inline FwAfter fw_model(const k4lz4_frame_writer &w, int64_t srcLen, bool closing, Block block)
{
    FwAfter a;
    const int64_t B = w.encBlock, L = w.ringBytes, total = (int64_t)w.pointer + srcLen;
    int64_t s = w.index, ws = 0, dl = 0, d = w.dictSize, cur = w.currentOffset;
    while (s < total) {
        const int64_t n = std::min(B, total - s);
        if (n < B && !closing) break;
        if (w.kind == 2 && cur + n > ((int64_t)1 << 31)) a.too_long = true;      /* LZ4_renormDictT (LL64.tools.cs:157-173) */
        block(s, n);
        a.nblk++;
        s += n; d += n; cur += n;
        const int64_t ptr = s - ws;
        if (w.kind == 0) {                                   /* LZ4BlockEncoder: CopyDict keeps nothing */
            ws = s;
        } else if (ptr + B > L) {                            /* Commit -> LZ4_saveDictHC / LZ4_saveDict (Engine/LL.tools.cs:195-213) */
            int64_t keep;
            if (w.kind == 1) { keep = std::min<int64_t>(65536, std::min(ptr, s - dl)); if (keep < 4) keep = 0; dl = s - keep; }
            else { keep = std::min<int64_t>(65536, d); d = keep; }
            ws = s - keep;
        }
    }
    a.index = s - ws; a.pointer = total - ws; a.ws = ws; a.cur = (uint32_t)cur; a.dict = (uint32_t)d;
    return a;
}

inline int64_t fw_bound(const k4lz4_frame_writer &w, int64_t srcLen, bool closing)
{
    if (srcLen < 0 || w.phase == 2) return 0;
    int64_t b = 0;
    if (fw_opens(w, srcLen, closing)) b += 4 + (w.settings.contentLength >= 0 ? 10 : 2) + 1;
    else if (w.phase == 0) return 0;
    const int64_t pend = (int64_t)w.pointer - w.index + srcLen, B = w.encBlock;
    const int64_t rec = 4 + (w.settings.blockChecksum ? 4 : 0);           /* allowCopy: a payload is never longer than its block */
    b += pend / B * (rec + B);
    if (closing) b += (pend % B ? rec + pend % B : 0) + 4 + (w.settings.contentChecksum ? 4 : 0);
    return b;
}

/* the per-stream refusal, decided before anything is enqueued (K4LZ4_FWRITE_*), or 0 */
inline int32_t fw_code(const k4lz4_frame_writer &w, int64_t srcLen, bool closing, uint64_t dstCap)
{
    if (w.phase == 2) return K4LZ4_FWRITE_CLOSED;
    const int64_t cl = w.settings.contentLength;
    if (closing && cl >= 0 && ((w.phase == 1 && w.written + srcLen != cl) || (w.phase == 0 && srcLen > 0 && srcLen != cl)))
        return K4LZ4_FWRITE_LENGTH;
    if ((int64_t)dstCap < fw_bound(w, srcLen, closing)) return K4LZ4_FWRITE_TARGET;
    return 0;
}

/* the record after a call that ran the stream */
inline void fw_advance(k4lz4_frame_writer &w, int64_t srcLen, bool closing, const FwAfter &a)
{
    const bool opens = fw_opens(w, srcLen, closing);
    if (closing) w.phase = 2;
    else if (opens) w.phase = 1;
    w.written += srcLen;
    w.index = (int32_t)a.index; w.pointer = (int32_t)a.pointer;
    if (w.kind == 2) { w.currentOffset = a.cur; w.dictSize = a.dict; }
}

}  // namespace k4
