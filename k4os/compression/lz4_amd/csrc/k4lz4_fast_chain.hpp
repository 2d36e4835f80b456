/*
 * k4lz4_fast_chain.hpp -- chained L00_FAST streams (LZ4FastChainEncoder), one wavefront per stream.
 *
 * Replaces, for many streams at once, the reference's
 *   LZ4FastChainEncoder over LZ4EncoderBase     Encoders/LZ4FastChainEncoder.cs, Encoders/LZ4EncoderBase.cs:28-97
 *   LL64.LZ4_compress_fast_continue             Engine/x64/LL64.fast.cs:582-667
 *   LL64.LZ4_compress_generic                   Engine/x64/LL64.fast.cs:34-513   (byU32 + hash5, acceleration 1,
 *                                               usingExtDict with an empty dictionary for a fresh stream's first block,
 *                                               withPrefix64k for every later one; noDictIssue | dictSmall; limitedOutput)
 *   LZ4_saveDict                                Engine/LL.tools.cs:195-213
 * with byte-identical blocks.  The table holds only the positions the parse visited, so block k + 1 needs the table block k's parse
 * left behind: a stream is serial.  Streams are not, and a wave carries its stream's 16 KiB table in LDS from block to block.
 *
 * Content coordinates.  The ring buffer always puts the next block right behind the bytes it keeps (LZ4_saveDict moves the last
 * <= 64 KiB to its start and the stream context's indices stay as they are), so every block can be encoded in place in the caller's
 * contiguous content: stream index = content position + idx0, idx0 = currentOffset - dictLen at the stream's start.  The host's block
 * table (k4lz4_capi.hip, fast_chain_table) gives each block its start, length and dictSize (what the ring holds in front of it).
 * Per block: lowLimit = start - dictSize (the backward extension stops there), and with dictSmall (dictSize < 64 KiB and below
 * currentOffset) no candidate below prefixIdxLimit = startIndex - dictSize (in the search and in "test next position").  A fresh
 * stream's first block takes the extDict arm with an empty dictionary, which is the same parse as the prefix arm with dictSize 0.
 *
 * The search.  The reference probes one position at a time and puts each one before the next look-up.  A wave probes 64 of the
 * search's positions (LL64.fast.cs:156-172, probe_offset) at once: a probe's candidate is the nearest earlier probe of the window with
 * the same hash, else the table entry as it stood when the window began; the first probe that finds a match ends the search, and the
 * puts of it and the probes before it are applied (atomicMax: a stream's indices only grow, so the last put of a hash wins, as in the
 * reference).  Everything behind a match -- backward extension, the token, the match length, "fill table" and "test next position"
 * (:237-463) -- is the reference's scalar sequence, with the lanes comparing and copying bytes.
 */
#pragma once
#include "k4lz4_encode_fast.hpp"

namespace k4 {

constexpr int FAST_CHAIN_WAVES_PER_WG = 8;            /* 8 x (16 KiB table + 512 B of hash bits) of LDS per workgroup, one workgroup per CU */
constexpr int FAST_CHAIN_SEEN_DWORDS = 128;           /* one bit per hash value: does a window hold a hash twice */
constexpr int FAST_CHAIN_LDS_DWORDS = 4096 + FAST_CHAIN_SEEN_DWORDS;

/* k4lz4_fast_chain_state (include/k4lz4.h): LZ4_stream_t's hashTable and the two indices, in the reference's own terms */
struct FastChainState {
    uint32_t hashTable[4096];
    uint32_t currentOffset;
    uint32_t dictSize;
    uint32_t reserved[2];
};

struct FastChainArgs {
    const uint8_t *src;
    /* per stream (index s) */
    const uint64_t *soff;       /* content start in src */
    const uint64_t *slen;       /* content length */
    const int64_t *first;       /* its first block in the per-block arrays */
    const uint32_t *nblk;       /* its number of blocks */
    const uint32_t *idx0;       /* stream index of content byte 0 */
    const uint32_t *dict_end;   /* dictSize after its last block (and the ring's save behind it) */
    const uint32_t *order;      /* streams, longest first */
    /* per block */
    const uint32_t *bpos;       /* start, content coordinates */
    const int32_t *blen;
    const uint32_t *bdict;      /* dictSize when the block is encoded (= the ring's _inputIndex) */
    const uint64_t *doff;       /* its slot in dst */
    const int32_t *cap;         /* the slot's size */
    uint8_t *dst;
    int32_t *outLen;
    const FastChainState *state_in;   /* per stream, or nullptr: a fresh stream */
    FastChainState *state_out;        /* per stream, or nullptr */
    uint32_t *ticket;                 /* one zeroed word: streams handed out */
    long long n;                      /* streams */
    int allow_copy;
};

typedef FastTable<0> ChainTable;

/* LL64.LZ4_compress_generic for one block of a chained stream.  c: the content, tab: the stream's table (LDS), seen: the wave's hash
 * bits (zero on entry and on return).  Returns the block's length, 0 when it does not fit `cap` (the reference returns 0 there). */
__device__ __forceinline__ int fast_chain_block(const uint8_t *c, const uint32_t pos, const uint32_t n, const uint32_t dict, const uint32_t idx0,
                                                uint32_t *tab, uint32_t *seen, uint8_t *dst, const int cap, const int lane)
{
    const uint32_t start = idx0 + pos;                                   /* startIndex = currentOffset */
    const bool small = dict < 65536u && dict < start;                    /* dictIssue == dictSmall (LL64.fast.cs:617, :650) */
    const uint32_t pfx = start - dict;                                   /* prefixIdxLimit */
    const uint32_t low = pos - dict;                                     /* lowLimit */
    const uint32_t iend = pos + n;
    const uint32_t ucap = (uint32_t)cap;
    uint32_t op = 0u, anchor = pos;

    /* a candidate (stream index mi) for the position p (stream index cur): the reference's refusals, and its first four bytes */
    auto usable = [&](uint32_t mi, uint32_t p) -> bool {
        const uint32_t cur = idx0 + p;
        if (small && mi < pfx) return false;                             /* :219-220, :450 */
        if (mi + (uint32_t)DISTANCE_MAX < cur) return false;             /* :221-224 */
        if (mi < idx0 || mi >= cur) return false;                        /* (never with a state this encoder or liblz4 wrote) */
        return ld32u(c + (mi - idx0)) == ld32u(c + p);
    };

    if (n >= (uint32_t)MFLIMIT + 1u) {                                 /* LZ4_minLength (:130) */
        const uint32_t mfl1 = iend - (uint32_t)MFLIMIT + 1u;             /* mflimitPlusOne */
        const uint32_t mlimit = iend - (uint32_t)LASTLITERALS;           /* matchlimit */
        uint32_t ip = pos;
        {   /* first byte (:134) */
            const uint32_t h = ChainTable::hash(c + ip);
            wave_sync();
            tab[h] = idx0 + ip;
            wave_sync();
        }
        ip++;
        bool done = false;
        while (!done) {
            /* ---- search (:156-231): windows of 64 probes ---- */
            uint32_t match = 0u;
            bool found = false;
            const uint32_t s0 = ip;
            for (uint32_t t = 0u;; t += 64u) {
                const uint32_t q = s0 + probe_offset(t + (uint32_t)lane, 1u);
                const uint32_t qn = s0 + probe_offset(t + (uint32_t)lane + 1u, 1u);
                const bool val = qn <= mfl1;                             /* :172: probe t is made only if probe t + 1 is still inside */
                const uint32_t qq = val ? q : pos;
                const uint32_t h = ChainTable::hash(c + qq);
                uint32_t mi = tab[h];
                const uint32_t bit = h;
                const bool twice = val && ((atomicOr(&seen[bit >> 5], 1u << (bit & 31u)) >> (bit & 31u)) & 1u) != 0u;
                const unsigned long long valm = ballot(val);
                if (ballot(twice)) {
                    /* the nearest earlier probe of the window with the same hash was put by then */
                    bool got = false;
                    for (int d = 1; d < 64; d++) {
                        const uint32_t hd = (uint32_t)__shfl_up((int)h, (unsigned)d);
                        const uint32_t qd = (uint32_t)__shfl_up((int)q, (unsigned)d);
                        if (!got && lane >= d && hd == h) { mi = idx0 + qd; got = true; }
                    }
                }
                wave_sync();
                if (val) seen[bit >> 5] = 0u;
                const bool ok = val && usable(mi, q);
                const unsigned long long hitm = ballot(ok);
                const int f = hitm ? ctz64(hitm) : 64;
                wave_sync();
                if (val && lane <= f) atomicMax(&tab[h], idx0 + q);    /* :176 put of every probe made, the hit's included */
                wave_sync();
                if (hitm) {
                    ip = readlane_u32(q, f);
                    match = readlane_u32(mi, f) - idx0;
                    found = true;
                    break;
                }
                if (valm != ~0ull) break;                                /* :172 -> _last_literals */
            }
            if (!found) break;

            /* ---- catch up (:237-242) ---- */
            {
                const uint32_t bmax = min(ip - anchor, match > low ? match - low : 0u);
                uint32_t back = 0u;
                for (uint32_t k0 = 0u; k0 < bmax; k0 += 64u) {
                    const uint32_t i = k0 + (uint32_t)lane;
                    const bool eq = i < bmax && c[ip - 1u - i] == c[match - 1u - i];
                    const unsigned long long ne = ballot(!eq);
                    if (ne) { back = k0 + (uint32_t)ctz64(ne); break; }
                    back = k0 + 64u;
                }
                back = min(back, bmax);
                ip -= back;
                match -= back;
            }

            /* ---- literals (:244-282) ---- */
            uint32_t tokp, tok;
            {
                const uint32_t lit = ip - anchor;
                if ((unsigned long long)op + 1u + lit + 2u + 1u + (uint32_t)LASTLITERALS + lit / 255u > ucap) return 0;
                tokp = op++;
                if (lit >= (uint32_t)RUN_MASK) {
                    tok = (uint32_t)RUN_MASK << ML_BITS;
                    const uint32_t rem = lit - (uint32_t)RUN_MASK;
                    emit_length_run(dst, op, rem, lane);
                    op += rem / 255u + 1u;
                } else {
                    tok = lit << ML_BITS;
                }
                wave_copy(dst + op, c + anchor, lit, lane);
                op += lit;
            }

            /* ---- match, then "test next position" as long as it finds one (:284-463) ---- */
            for (;;) {
                if (lane == 0) { dst[op] = (uint8_t)(ip - match); dst[op + 1u] = (uint8_t)((ip - match) >> 8); }
                op += 2u;
                const uint32_t mc = wave_count(c + ip + (uint32_t)MINMATCH, c + match + (uint32_t)MINMATCH, mlimit - (ip + (uint32_t)MINMATCH), lane);
                if ((unsigned long long)op + 1u + (uint32_t)LASTLITERALS + (mc + 240u) / 255u > ucap) return 0;
                ip += (uint32_t)MINMATCH + mc;
                if (mc >= (uint32_t)ML_MASK) {
                    tok += (uint32_t)ML_MASK;
                    const uint32_t rem = mc - (uint32_t)ML_MASK;
                    emit_length_run(dst, op, rem, lane);
                    op += rem / 255u + 1u;
                } else {
                    tok += mc;
                }
                if (lane == 0) dst[tokp] = (uint8_t)tok;
                anchor = ip;
                if (ip >= mfl1) { done = true; break; }                    /* :391 */
                const uint32_t h2 = ChainTable::hash(c + ip - 2u);
                const uint32_t h = ChainTable::hash(c + ip);
                wave_sync();
                tab[h2] = idx0 + ip - 2u;                                    /* :394 fill table */
                wave_sync();
                const uint32_t mi = tab[h];
                wave_sync();
                tab[h] = idx0 + ip;                                          /* :445 */
                wave_sync();
                if (!usable(mi, ip)) break;
                match = mi - idx0;
                tokp = op++;
                tok = 0u;
            }
            if (!done) ip++;                                                 /* :466 */
        }
    }

    /* ---- last literals (:468-509) ---- */
    {
        const uint32_t last = iend - anchor;
        if ((unsigned long long)op + last + 1u + (last + 255u - (uint32_t)RUN_MASK) / 255u > ucap) return 0;
        if (last >= (uint32_t)RUN_MASK) {
            if (lane == 0) dst[op] = (uint8_t)(RUN_MASK << ML_BITS);
            op++;
            const uint32_t rem = last - (uint32_t)RUN_MASK;
            emit_length_run(dst, op, rem, lane);
            op += rem / 255u + 1u;
        } else {
            if (lane == 0) dst[op] = (uint8_t)(last << ML_BITS);
            op++;
        }
        wave_copy(dst + op, c + anchor, last, lane);
        op += last;
    }
    return (int)op;
}

/* a wave takes the next stream (longest first) when it is done with one: batches larger than residency work */
__global__ __launch_bounds__(64 * FAST_CHAIN_WAVES_PER_WG) void k4_fast_chain_kernel(FastChainArgs a)
{
    __shared__ uint32_t lds[FAST_CHAIN_WAVES_PER_WG][FAST_CHAIN_LDS_DWORDS];
    const int lane = lane_id();
    const uint32_t wave = uni(threadIdx.x >> 6);
    uint32_t *tab = lds[wave];
    uint32_t *seen = tab + 4096;
    for (int k = lane; k < FAST_CHAIN_SEEN_DWORDS; k += 64) seen[k] = 0u;
    for (;;) {
        uint32_t t = 0u;
        if (lane == 0) t = atomicAdd(a.ticket, 1u);
        t = uni(t);
        if ((long long)t >= a.n) break;
        const uint32_t s = a.order[t];
        const FastChainState *in = a.state_in ? a.state_in + s : nullptr;
        if (in) {
            for (int k = lane; k < 1024; k += 64) ((uint4 *)tab)[k] = ((const uint4 *)in->hashTable)[k];
        } else {
            for (int k = lane; k < 1024; k += 64) ((uint4 *)tab)[k] = make_uint4(0u, 0u, 0u, 0u);     /* LZ4_initStream */
        }
        wave_sync();
        const uint8_t *c = a.src + a.soff[s];
        const uint32_t idx0 = a.idx0[s];
        const long long b0 = (long long)a.first[s];
        const uint32_t nb = a.nblk[s];
        for (uint32_t j = 0u; j < nb; j++) {
            const long long b = b0 + (long long)j;
            const uint32_t pos = a.bpos[b], n = (uint32_t)a.blen[b];
            uint8_t *d = a.dst + a.doff[b];
            int r = fast_chain_block(c, pos, n, a.bdict[b], idx0, tab, seen, d, a.cap[b], lane);
            if (a.allow_copy && r >= (int)n) {                     /* LZ4EncoderBase.Encode(allowCopy): stored raw, the context advances all the same */
                wave_sync();
                wave_copy(d, c + pos, n, lane);
                r = -(int)n;
            }
            if (lane == 0) a.outLen[b] = r;
        }
        if (a.state_out) {
            FastChainState *out = a.state_out + s;
            wave_sync();
            for (int k = lane; k < 1024; k += 64) ((uint4 *)out->hashTable)[k] = ((const uint4 *)tab)[k];
            if (lane == 0) {
                out->currentOffset = idx0 + (uint32_t)a.slen[s];
                out->dictSize = a.dict_end[s];
                out->reserved[0] = out->reserved[1] = 0u;
            }
        }
        wave_sync();
    }
}

}  // namespace k4
