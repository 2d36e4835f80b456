/*
 * k4lz4_dict_encode_hc.hpp -- batches of messages encoded against shared dictionaries at the hash-chain levels 3 .. 9
 * (k4lz4_encode_dict_hc_batch).  DESIGN.md 4.21.
 *
 * Replaces, for many messages at once, "reset the HC stream, load the dictionary, compress the message":
 *   LL.LZ4_resetStreamHC_fast / LZ4_loadDictHC        Engine/LL.high.cs:74-88, :187-207
 *   LL.LZ4HC_setExternalDict                          Engine/LL.high.cs:124-140
 *   LL64.LZ4_compress_HC_continue                     Engine/x64/LL64.high.cs:1259-1311
 *   LL64.LZ4HC_InsertAndGetWiderMatch                 Engine/x64/LL64.high.cs:70-383   (the matchIndex < dictLimit arm, no dictCtx)
 *   LL64.LZ4HC_compress_hashChain                     Engine/x64/LL64.high.cs:512-800
 * with byte-identical blocks.
 *
 * Indices are the reference's: kept[k] (the last <= 64 KiB of the dictionary, D bytes) is 65536 + k, message byte q is
 * 65536 + D + q; lowLimit = 65536, dictLimit = 65536 + D.
 *
 * Load (k4_dict_hc_load_kernel), one workgroup per distinct dictionary: the hash heads (32768 x u32, an index or 0) and the chain
 * deltas (65536 x u16, slot k for kept[k]) over kept[0 .. D - 4]: the last three positions never enter the chain, and nothing does
 * with D < 4.  The tables are written once per call and read by every message of that dictionary; nothing of them is copied.
 *
 * Encode (k4_dict_hc_encode_kernel), one wavefront per message, handed out longest first by a ticket.  Every wave SLOT of the launch
 * (not every message) owns a head table and a chain table for message positions.  The wave inserts positions as the reference does --
 * up to the position it searches, 64 per step -- into its own head table; a hash the message has not seen links to the dictionary's
 * head; which hashes occur twice within a step comes from a bit per hash in LDS (4 KiB per wave).  A search walks candidates one at a time, reads a candidate's bytes from the buffer it lies in and its chain delta from the
 * dictionary's table or its own.  The reference keeps one chainTable for both, indexed by the index's low 16 bits; a message position
 * overwrites the slot of the index 65536 before it, which is further back than any search that comes after that insert may look, so
 * two tables give the same walks.  After a message the wave zeroes the heads it wrote (by hashing the inserted positions again).
 * The two buffers are never read as if they were adjacent: counts compare single bytes through the buffer each lies in, and a
 * four-byte load that would straddle the seam is assembled.
 */
#pragma once
#include "k4lz4_dict_encode.hpp"

namespace k4 {

constexpr uint32_t DHC_LOW = 65536u;                    /* lowLimit: the index of kept[0] */
constexpr int DHC_HASH_LOG = 15;
constexpr uint32_t DHC_HEADS = 1u << DHC_HASH_LOG;      /* words of a head table */
constexpr uint32_t DHC_CHAIN = 65536u;                  /* u16 deltas of a chain table */
constexpr uint32_t DHC_TABLE_BYTES = DHC_HEADS * 4u + DHC_CHAIN * 2u;      /* heads, then chain: per distinct dictionary and per wave slot */
constexpr int DHC_LOAD_THREADS = 256;
constexpr int DHC_WAVES_PER_WG = 4;
constexpr int DHC_OPTIMAL_ML = (ML_MASK - 1) + MINMATCH;

__device__ __forceinline__ uint32_t dhc_hash(uint32_t v) { return (v * 2654435761u) >> (MINMATCH * 8 - DHC_HASH_LOG); }

struct DictHcLoadArgs {
    const uint8_t *dict;
    const uint64_t *keptOff;    /* per table: where the kept bytes start in dict */
    const uint32_t *keptLen;    /* per table: D */
    uint8_t *tables;            /* DHC_TABLE_BYTES per table */
};

struct DictHcEncArgs {
    const uint8_t *src;
    const uint64_t *srcOff;
    const int32_t *srcLen;
    uint8_t *dst;
    const uint64_t *dstOff;
    const int32_t *dstCap;
    int32_t *outLen;
    const int32_t *dictIdx;
    const uint8_t *dict;
    const uint64_t *keptOff;    /* per entry of the list */
    const uint32_t *keptLen;
    const uint32_t *table;
    const uint8_t *tables;      /* the dictionaries' tables */
    uint8_t *slots;             /* DHC_TABLE_BYTES per wave of the launch; heads zero on entry and on return */
    const uint32_t *order;      /* messages, longest first */
    uint32_t *ticket;
    uint32_t *status;
    long long n;
    int nDict;
    int level;
};

/* for every active lane the nearest lower active lane whose h is the same, or -1; later: a higher lane has it too.  dup: at least
 * one lane of every hash that occurs twice; one turn of the loop per such hash */
__device__ __forceinline__ int dhc_same_before(uint32_t h, bool act, unsigned long long dup, int lane, bool &later)
{
    int from = -1;
    later = false;
    while (dup) {
        const uint32_t hj = readlane_u32(h, ctz64(dup));
        const bool mine = act && h == hj;
        const unsigned long long m = ballot(mine);
        if (mine) {
            const unsigned long long below = m & ((1ull << lane) - 1ull);
            from = below ? 63 - (int)__clzll((long long)below) : -1;
            later = ((m >> lane) >> 1) != 0ull;
        }
        dup &= ~m;
    }
    return from;
}

/* LZ4_loadDictHC's LZ4HC_Insert(end - 3) over the kept bytes: one wave enters 64 positions per step through a head table in LDS.
 * Memory is touched once per 16 steps (1024 bytes in, 1024 deltas out): a step that waits for memory costs ten steps that do not. */
constexpr uint32_t DHC_LOAD_CHUNK = 1024u;
__global__ __launch_bounds__(DHC_LOAD_THREADS) void k4_dict_hc_load_kernel(DictHcLoadArgs a)
{
    __shared__ uint32_t tab[DHC_HEADS];                                /* the index of the latest position with the hash; 0: none */
    __shared__ __attribute__((aligned(16))) uint8_t bytes[DHC_LOAD_CHUNK + 16];
    __shared__ __attribute__((aligned(16))) uint16_t stage[DHC_LOAD_CHUNK];
    const uint32_t t = blockIdx.x;
    uint32_t *heads = (uint32_t *)(a.tables + (size_t)DHC_TABLE_BYTES * t);
    uint16_t *chain = (uint16_t *)(heads + DHC_HEADS);
    const uint32_t D = a.keptLen[t];
    const uint8_t *d = a.dict + a.keptOff[t];
    for (uint32_t k = threadIdx.x; k < DHC_HEADS; k += (uint32_t)DHC_LOAD_THREADS) tab[k] = 0u;
    for (uint32_t k = threadIdx.x; k < DHC_CHAIN; k += (uint32_t)DHC_LOAD_THREADS) chain[k] = 0xFFFFu;      /* LZ4HC_clearTables */
    __syncthreads();
    if (threadIdx.x < 64u && D >= 4u) {
        const int lane = (int)threadIdx.x;
        const uint32_t np = D - 3u;                                    /* positions 0 .. D - 4 */
        for (uint32_t k1 = 0; k1 < np; k1 += DHC_LOAD_CHUNK) {
            {   /* the chunk's bytes and the three behind them, as far as the dictionary goes */
                const uint32_t nb = D - k1 < DHC_LOAD_CHUNK + 3u ? D - k1 : DHC_LOAD_CHUNK + 3u;
                const uint32_t at = 16u * (uint32_t)lane;
                if (at + 16u <= nb) *(U128u *)(bytes + at) = ld128u(d + k1 + at);
                else for (uint32_t i = at; i < nb && i < at + 16u; i++) bytes[i] = d[k1 + i];
                if (DHC_LOAD_CHUNK + (uint32_t)lane < nb) bytes[DHC_LOAD_CHUNK + (uint32_t)lane] = d[k1 + DHC_LOAD_CHUNK + (uint32_t)lane];
            }
            wave_sync();
            for (uint32_t s0 = 0; s0 < DHC_LOAD_CHUNK && k1 + s0 < np; s0 += 64u) {
                const uint32_t k0 = k1 + s0;
                const uint32_t cnt = np - k0 < 64u ? np - k0 : 64u;
                const uint32_t k = k0 + (uint32_t)lane;
                const bool act = (uint32_t)lane < cnt;
                const uint8_t *bp = bytes + s0 + (uint32_t)lane;
                const uint32_t v = (uint32_t)bp[0] | (uint32_t)bp[1] << 8 | (uint32_t)bp[2] << 16 | (uint32_t)bp[3] << 24;
                const uint32_t h = act ? dhc_hash(v) : 0xffffff00u + (uint32_t)lane;
                uint32_t before = act ? tab[h] : 0u;
                wave_sync();
                if (act) tab[h] = DHC_LOW + k;                          /* one lane per hash gets through */
                wave_sync();
                const unsigned long long dup = ballot(act && tab[h] != DHC_LOW + k);
                if (dup) {                                             /* a hash twice in the step: in lane order, the last one stays */
                    bool later;
                    const int from = dhc_same_before(h, act, dup, lane, later);
                    if (from >= 0) before = DHC_LOW + k0 + (uint32_t)from;
                    wave_sync();
                    if (act && !later) tab[h] = DHC_LOW + k;
                }
                const uint32_t delta = DHC_LOW + k - before;           /* an empty slot is 0: the delta is capped */
                stage[s0 + (uint32_t)lane] = (uint16_t)(!act || delta > (uint32_t)DISTANCE_MAX ? (uint32_t)DISTANCE_MAX : delta);
                wave_sync();
            }
            {   /* the chunk's deltas: 16 per lane; positions from np on keep 0xFFFF */
                const uint32_t at = 16u * (uint32_t)lane;
                if (k1 + at < np) {
                    uint16_t *out = chain + k1 + at;
                    const uint32_t left = np - (k1 + at);
                    if (left >= 16u) { ((uint4 *)out)[0] = ((const uint4 *)(stage + at))[0]; ((uint4 *)out)[1] = ((const uint4 *)(stage + at))[1]; }
                    else for (uint32_t i = 0; i < left; i++) out[i] = stage[at + i];
                }
            }
            wave_sync();
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < DHC_HEADS; k += (uint32_t)DHC_LOAD_THREADS) heads[k] = tab[k];
}

/* one message behind one dictionary, as one wave sees it */
struct DhcState {
    const uint8_t *dk;          /* kept bytes */
    const uint8_t *c;           /* the message */
    const uint32_t *dhead;      /* the dictionary's tables */
    const uint16_t *dchain;
    uint32_t *mhead;            /* this wave slot's */
    uint16_t *mchain;
    uint32_t *seen;             /* this wave's bit per hash (LDS), zero between steps: which hashes occur twice in a step */
    uint32_t dl;                /* dictLimit = 65536 + D: the index of the message's first byte */
    uint32_t next;              /* nextToUpdate */
};

__device__ __forceinline__ uint32_t dhc_ld_u32(const uint32_t *p)
{
#ifndef K4_HOST_EMU
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);       /* a vector load: the wave's own stores are behind it */
#else
    return *(const volatile uint32_t *)p;
#endif
}
__device__ __forceinline__ uint32_t dhc_ld_u16(const uint16_t *p)
{
#ifndef K4_HOST_EMU
    return (uint32_t)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#else
    return (uint32_t)*(const volatile uint16_t *)p;
#endif
}

/* the byte at an index (any lane its own) */
__device__ __forceinline__ uint32_t dhc_byte(const DhcState &s, uint32_t idx) { return idx < s.dl ? s.dk[idx - DHC_LOW] : s.c[idx - s.dl]; }

/* Mem.Peek4 at a wave-uniform index; the caller has made sure that the four bytes exist */
__device__ __forceinline__ uint32_t dhc_peek4(const DhcState &s, uint32_t idx)
{
    if (idx >= s.dl) return uni(ld32u(s.c + (idx - s.dl)));
    if (idx + 4u <= s.dl) return uni(ld32u(s.dk + (idx - DHC_LOW)));
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4u; k++) v |= dhc_byte(s, idx + k) << (8u * k);
    return uni(v);
}

/* DELTANEXTU16(chainTable, idx) */
__device__ __forceinline__ uint32_t dhc_delta(const DhcState &s, uint32_t idx)
{
    return uni(idx < s.dl ? dhc_ld_u16(s.dchain + (idx - DHC_LOW)) : dhc_ld_u16(s.mchain + ((idx - s.dl) & 0xFFFFu)));
}

/* equal bytes at a[] / b[] going forward, at most maxn; a and b are indices that do not cross the seam within maxn */
__device__ __forceinline__ uint32_t dhc_count(const DhcState &s, uint32_t a, uint32_t b, uint32_t maxn, int lane)
{
    uint32_t done = 0;
    for (;;) {
        const uint32_t i = done + (uint32_t)lane;
        const bool eq = i < maxn && dhc_byte(s, a + i) == dhc_byte(s, b + i);
        const unsigned long long ne = ~ballot(eq);
        const int run = ne ? ctz64(ne) : 64;
        done += (uint32_t)run;
        if (run < 64) return done;
    }
}

/* equal bytes before a / b going backward, at most maxn */
__device__ __forceinline__ uint32_t dhc_count_back(const DhcState &s, uint32_t a, uint32_t b, uint32_t maxn, int lane)
{
    uint32_t done = 0;
    for (;;) {
        const uint32_t i = done + (uint32_t)lane;
        const bool eq = i < maxn && dhc_byte(s, a - 1u - i) == dhc_byte(s, b - 1u - i);
        const unsigned long long ne = ~ballot(eq);
        const int run = ne ? ctz64(ne) : 64;
        done += (uint32_t)run;
        if (run < 64) return done;
    }
}

/* LZ4HC_countPattern over [from, limit), the pattern's byte `phase` first; LZ4HC_reverseCountPattern over [low, at), the byte before
 * `phase` first.  Only a pattern of four equal bytes is ever confirmed (:214-215), so the phase only keeps the reference's shape. */
__device__ __forceinline__ uint32_t dhc_count_pattern(const DhcState &s, uint32_t from, uint32_t limit, uint32_t pattern, uint32_t phase, int lane)
{
    uint32_t done = 0;
    for (;;) {
        const uint32_t i = done + (uint32_t)lane;
        const bool eq = from + i < limit && dhc_byte(s, from + i) == ((pattern >> (8u * ((phase + i) & 3u))) & 0xFFu);
        const unsigned long long ne = ~ballot(eq);
        const int run = ne ? ctz64(ne) : 64;
        done += (uint32_t)run;
        if (run < 64) return done;
    }
}
__device__ __forceinline__ uint32_t dhc_reverse_count_pattern(const DhcState &s, uint32_t at, uint32_t low, uint32_t pattern, uint32_t phase, int lane)
{
    uint32_t done = 0;
    for (;;) {
        const uint32_t i = done + (uint32_t)lane;
        const bool eq = i < at - low && dhc_byte(s, at - 1u - i) == ((pattern >> (8u * ((phase + 3u - (i & 3u)) & 3u))) & 0xFFu);
        const unsigned long long ne = ~ballot(eq);
        const int run = ne ? ctz64(ne) : 64;
        done += (uint32_t)run;
        if (run < 64) return done;
    }
}

__device__ __forceinline__ bool dhc_protect(uint32_t dl, uint32_t idx) { return (uint32_t)((dl - 1u) - idx) >= 3u; }       /* LZ4HC_protectDictEnd */

/* LZ4HC_Insert up to the index `target` (LL.high.cs:102-122), 64 positions per step */
__device__ __forceinline__ void dhc_insert(DhcState &s, uint32_t target, int lane)
{
    while (s.next < target) {
        const uint32_t cnt = target - s.next < 64u ? target - s.next : 64u;
        const uint32_t idx = s.next + (uint32_t)lane;
        const bool act = (uint32_t)lane < cnt;
        const uint32_t h = act ? dhc_hash(ld32u(s.c + (idx - s.dl))) : 0xffffff00u + (uint32_t)lane;
        uint32_t before = 0u;
        if (act) {
            before = dhc_ld_u32(s.mhead + h);
            if (!before) before = s.dhead[h];
        }
        bool later = false;
        if (cnt > 1u) {
            const bool twice = act && ((atomicOr(&s.seen[h >> 5], 1u << (h & 31u)) >> (h & 31u)) & 1u) != 0u;
            const unsigned long long dup = ballot(twice);
            wave_sync();
            if (act) s.seen[h >> 5] = 0u;
            if (dup) {
                const int from = dhc_same_before(h, act, dup, lane, later);
                if (from >= 0) before = s.next + (uint32_t)from;
            }
        }
        wave_sync();
        if (act) {
            const uint32_t delta = idx - before;
            s.mchain[(idx - s.dl) & 0xFFFFu] = (uint16_t)(delta > (uint32_t)DISTANCE_MAX ? (uint32_t)DISTANCE_MAX : delta);
            if (!later) s.mhead[h] = idx;                            /* the step's last position with the hash stays */
        }
        wave_sync();
        s.next += cnt;
    }
}

struct DhcMatch { int len; uint32_t mpos, spos; };          /* longest, *matchpos, *startpos as indices */

/* LZ4HC_InsertAndGetWiderMatch (LL64.high.cs:70-383), chainSwap off, no dictCtx; all positions are indices.  The two-byte test of
 * :124-125 only skips candidates that cannot beat `longest` (both bytes lie inside any longer match) and is left out. */
__device__ __forceinline__ DhcMatch dhc_search(DhcState &s, uint32_t ip, uint32_t ilow, uint32_t ihigh, int longest, uint32_t mpos, uint32_t spos,
                                               int attempts, bool pattern_analysis, int lane)
{
    DhcMatch r;
    r.len = longest; r.mpos = mpos; r.spos = spos;
    const uint32_t lowest = DHC_LOW + (uint32_t)DISTANCE_MAX + 1u > ip ? DHC_LOW : ip - (uint32_t)DISTANCE_MAX;
    const uint32_t look_back = ip - ilow;
    const uint32_t pattern = dhc_peek4(s, ip);
    int repeat = 0;                                          /* 0 untested, 1 not a repeating pattern, 2 confirmed */
    uint32_t src_pattern_length = 0;
    dhc_insert(s, ip, lane);
    uint32_t mi;
    {
        const uint32_t h = dhc_hash(pattern);
        mi = uni(dhc_ld_u32(s.mhead + h));
        if (!mi) mi = uni(s.dhead[h]);
    }
    while (mi >= lowest && attempts != 0) {
        attempts--;
        if (mi >= s.dl) {                                    /* within the message (:117-142) */
            if (dhc_peek4(s, mi) == pattern) {
                const uint32_t maxb = look_back < mi - s.dl ? look_back : mi - s.dl;
                const uint32_t back = maxb ? dhc_count_back(s, ip, mi, maxb, lane) : 0u;
                const uint32_t fwd = dhc_count(s, ip + MINMATCH, mi + MINMATCH, ihigh - (ip + MINMATCH), lane);
                const int ml = (int)(MINMATCH + fwd + back);
                if (ml > r.len) { r.len = ml; r.mpos = mi - back; r.spos = ip - back; }
            }
        } else {                                             /* in the dictionary (:143-170) */
            if (dhc_peek4(s, mi) == pattern) {
                uint32_t vlimit = ip + (s.dl - mi);
                if (vlimit > ihigh) vlimit = ihigh;
                uint32_t mlen = MINMATCH + (vlimit > ip + MINMATCH ? dhc_count(s, ip + MINMATCH, mi + MINMATCH, vlimit - (ip + MINMATCH), lane) : 0u);
                if (ip + mlen == vlimit && vlimit < ihigh) mlen += dhc_count(s, ip + mlen, s.dl, ihigh - (ip + mlen), lane);
                const uint32_t maxb = look_back < mi - DHC_LOW ? look_back : mi - DHC_LOW;
                const uint32_t back = maxb ? dhc_count_back(s, ip, mi, maxb, lane) : 0u;
                const int ml = (int)(mlen + back);
                if (ml > r.len) { r.len = ml; r.mpos = mi - back; r.spos = ip - back; }
            }
        }
        const uint32_t dist = dhc_delta(s, mi);
        if (pattern_analysis && dist == 1u) {                /* :208-337 */
            const uint32_t cidx = mi - 1u;
            if (repeat == 0) {
                if (((pattern & 0xFFFFu) == (pattern >> 16)) && ((pattern & 0xFFu) == (pattern >> 24))) {
                    repeat = 2;
                    src_pattern_length = dhc_count_pattern(s, ip + MINMATCH, ihigh, pattern, 0u, lane) + MINMATCH;
                } else {
                    repeat = 1;
                }
            }
            if (repeat == 2 && cidx >= lowest && dhc_protect(s.dl, cidx)) {
                const bool ext = cidx < s.dl;
                if (dhc_peek4(s, cidx) == pattern) {
                    uint32_t fwd = dhc_count_pattern(s, cidx + MINMATCH, ext ? s.dl : ihigh, pattern, 0u, lane) + MINMATCH;
                    if (ext && cidx + fwd == s.dl) fwd += dhc_count_pattern(s, s.dl, ihigh, pattern, fwd & 3u, lane);       /* rotated (:240-246) */
                    uint32_t back_len = dhc_reverse_count_pattern(s, cidx, ext ? DHC_LOW : s.dl, pattern, 0u, lane);
                    if (!ext && cidx - back_len == s.dl && DHC_LOW < s.dl)                                                  /* :253-260 */
                        back_len += dhc_reverse_count_pattern(s, s.dl, DHC_LOW, pattern, (0u - back_len) & 3u, lane);
                    {
                        const uint32_t far = cidx - back_len;
                        back_len = cidx - (far > lowest ? far : lowest);
                    }
                    const uint32_t cur_seg = back_len + fwd;
                    if (cur_seg >= src_pattern_length && fwd <= src_pattern_length) {
                        const uint32_t nmi = cidx + fwd - src_pattern_length;
                        mi = dhc_protect(s.dl, nmi) ? nmi : s.dl;
                    } else {
                        const uint32_t nmi = cidx - back_len;
                        if (!dhc_protect(s.dl, nmi)) {
                            mi = s.dl;
                        } else {
                            mi = nmi;
                            if (look_back == 0u) {
                                const uint32_t max_ml = cur_seg < src_pattern_length ? cur_seg : src_pattern_length;
                                if ((uint32_t)r.len < max_ml) {
                                    if (ip - mi > (uint32_t)DISTANCE_MAX) break;
                                    r.len = (int)max_ml; r.mpos = mi; r.spos = ip;
                                }
                                const uint32_t d2 = dhc_delta(s, mi);
                                if (d2 > mi) break;
                                mi -= d2;
                            }
                        }
                    }
                    continue;
                }
            }
        }
        mi -= dist;                                          /* follow the chain */
    }
    return r;
}

/* LZ4HC_encodeSequence (LL64.high.cs:435-510); ip, anchor: positions of the message; off = ip - match.  false on output overflow */
__device__ __forceinline__ bool dhc_encode_sequence(const uint8_t *c, uint8_t *dst, uint32_t &ip, int64_t &op, uint32_t &anchor, int match_length,
                                                    uint32_t match, bool limited, int64_t oend, int lane)
{
    const int64_t token_pos = op;
    op++;
    uint32_t length = ip - anchor;
    if (limited && op + (int64_t)(length / 255u) + length + (2 + 1 + LASTLITERALS) > oend) return false;
    uint32_t token;
    if (length >= (uint32_t)RUN_MASK) {
        const uint32_t len = length - RUN_MASK;
        token = (uint32_t)RUN_MASK << ML_BITS;
        const uint32_t nb = len / 255u;
        wave_fill(dst + op, 255, nb, lane);
        if (lane == 0) dst[op + nb] = (uint8_t)(len - nb * 255u);
        op += nb + 1u;
    } else {
        token = length << ML_BITS;
    }
    wave_copy(dst + op, c + anchor, length, lane);
    op += length;
    if (lane == 0) {
        const uint32_t off = ip - match;
        dst[op] = (uint8_t)off;
        dst[op + 1] = (uint8_t)(off >> 8);
    }
    op += 2;
    length = (uint32_t)match_length - MINMATCH;
    if (limited && op + (int64_t)(length / 255u) + (1 + LASTLITERALS) > oend) return false;
    if (length >= (uint32_t)ML_MASK) {
        token += ML_MASK;
        length -= ML_MASK;
        const uint32_t nb = length / 255u;
        wave_fill(dst + op, 255, nb, lane);
        if (lane == 0) dst[op + nb] = (uint8_t)(length - nb * 255u);
        op += nb + 1u;
    } else {
        token += length;
    }
    if (lane == 0) dst[token_pos] = (uint8_t)token;
    ip += (uint32_t)match_length;
    anchor = ip;
    return true;
}

__device__ __forceinline__ int dhc_nb_searches(int level)       /* clTable (LL64.high.cs:1124-1138), levels 3 .. 9 */
{
    return level <= 3 ? 4 : level == 4 ? 8 : level == 5 ? 16 : level == 6 ? 32 : level == 7 ? 64 : level == 8 ? 128 : 256;
}

/* LZ4HC_compress_hashChain (LL64.high.cs:512-800) for one message of n > 0 bytes behind its dictionary; positions ip, anchor, start*,
 * ref* count from the message's first byte (a ref in the dictionary wraps below 0: only differences are used).  Returns the block's
 * length, 0 when it does not fit. */
__device__ __forceinline__ int dhc_block(DhcState &s, const uint32_t n, uint8_t *dst, const int dst_cap, const int level, const int lane)
{
    const bool limited = dst_cap < (int)(n + n / 255u + 16u);      /* LZ4_compressBound of n <= LZ4_MAX_INPUT_SIZE (:1303) */
    const int64_t oend = dst_cap;
    const int max_attempts = dhc_nb_searches(level);
    const bool pa = max_attempts > 128;
    const uint8_t *c = s.c;
    uint32_t ip = 0u, anchor = 0u;
    int64_t op = 0;
#define K4_DHC_EMIT(ML, REF) do { if (!dhc_encode_sequence(c, dst, ip, op, anchor, (ML), (REF), limited, oend, lane)) return 0; } while (0)
    if (n >= (uint32_t)MFLIMIT + 1u) {
        const uint32_t mflimit = n - MFLIMIT;
        const uint32_t ihigh = s.dl + n - LASTLITERALS;
        auto search = [&](uint32_t p, uint32_t low, int longest, uint32_t mpos, uint32_t spos) -> DhcMatch {
            DhcMatch m = dhc_search(s, s.dl + p, s.dl + low, ihigh, longest, s.dl + mpos, s.dl + spos, max_attempts, pa, lane);
            m.mpos -= s.dl; m.spos -= s.dl;
            return m;
        };
        while (ip <= mflimit) {
            const DhcMatch m = search(ip, ip, MINMATCH - 1, 0u, ip);
            int ml = m.len;
            uint32_t ref = m.mpos;
            if (ml < MINMATCH) { ip++; continue; }
            uint32_t start0 = ip, ref0 = ref;
            int ml0 = ml;
            int ml2 = 0, ml3 = 0;
            uint32_t start2 = 0, ref2 = 0, start3 = 0, ref3 = 0;
            bool go_search2 = true;
            for (;;) {   /* one pass = _Search2 (if requested) followed by _Search3 rounds */
                if (go_search2) {
                    if (ip + (uint32_t)ml <= mflimit) {
                        const DhcMatch m2 = search(ip + (uint32_t)ml - 2u, ip, ml, ref2, start2);
                        ml2 = m2.len; ref2 = m2.mpos; start2 = m2.spos;
                    } else {
                        ml2 = ml;
                    }
                    if (ml2 == ml) {                           /* no better match: encode ML1 */
                        K4_DHC_EMIT(ml, ref);
                        break;
                    }
                    if (start0 < ip) {
                        if (start2 < ip + (uint32_t)ml0) { ip = start0; ref = ref0; ml = ml0; }
                    }
                    if (start2 - ip < 3u) {                    /* first match too small: removed */
                        ml = ml2; ip = start2; ref = ref2;
                        continue;                              /* goto _Search2 */
                    }
                }
                go_search2 = false;
                /* _Search3 */
                if (start2 - ip < (uint32_t)DHC_OPTIMAL_ML) {
                    int new_ml = ml;
                    if (new_ml > DHC_OPTIMAL_ML) new_ml = DHC_OPTIMAL_ML;
                    if (ip + (uint32_t)new_ml > start2 + (uint32_t)ml2 - MINMATCH) new_ml = (int)(start2 - ip) + ml2 - MINMATCH;
                    const int correction = new_ml - (int)(start2 - ip);
                    if (correction > 0) { start2 += (uint32_t)correction; ref2 += (uint32_t)correction; ml2 -= correction; }
                }
                if (start2 + (uint32_t)ml2 <= mflimit) {
                    const DhcMatch m3 = search(start2 + (uint32_t)ml2 - 3u, start2, ml2, ref3, start3);
                    ml3 = m3.len; ref3 = m3.mpos; start3 = m3.spos;
                } else {
                    ml3 = ml2;
                }
                if (ml3 == ml2) {                              /* no better match: encode ML1 and ML2 */
                    if (start2 < ip + (uint32_t)ml) ml = (int)(start2 - ip);
                    K4_DHC_EMIT(ml, ref);
                    ip = start2;
                    K4_DHC_EMIT(ml2, ref2);
                    break;
                }
                if (start3 < ip + (uint32_t)ml + 3u) {         /* not enough space for match 2: remove it */
                    if (start3 >= ip + (uint32_t)ml) {         /* write Seq1 now; Seq3 becomes Seq1 */
                        if (start2 < ip + (uint32_t)ml) {
                            const int correction = (int)(ip + (uint32_t)ml - start2);
                            start2 += (uint32_t)correction; ref2 += (uint32_t)correction; ml2 -= correction;
                            if (ml2 < MINMATCH) { start2 = start3; ref2 = ref3; ml2 = ml3; }
                        }
                        K4_DHC_EMIT(ml, ref);
                        ip = start3; ref = ref3; ml = ml3;
                        start0 = start2; ref0 = ref2; ml0 = ml2;
                        go_search2 = true;
                        continue;                              /* goto _Search2 */
                    }
                    start2 = start3; ref2 = ref3; ml2 = ml3;
                    continue;                                  /* goto _Search3 */
                }
                /* three ascending matches: write the first one */
                if (start2 < ip + (uint32_t)ml) {
                    if (start2 - ip < (uint32_t)DHC_OPTIMAL_ML) {
                        if (ml > DHC_OPTIMAL_ML) ml = DHC_OPTIMAL_ML;
                        if (ip + (uint32_t)ml > start2 + (uint32_t)ml2 - MINMATCH) ml = (int)(start2 - ip) + ml2 - MINMATCH;
                        const int correction = ml - (int)(start2 - ip);
                        if (correction > 0) { start2 += (uint32_t)correction; ref2 += (uint32_t)correction; ml2 -= correction; }
                    } else {
                        ml = (int)(start2 - ip);
                    }
                }
                K4_DHC_EMIT(ml, ref);
                ip = start2; ref = ref2; ml = ml2;             /* ML2 becomes ML1, ML3 becomes ML2 */
                start2 = start3; ref2 = ref3; ml2 = ml3;
                /* goto _Search3 */
            }
        }
    }
#undef K4_DHC_EMIT
    /* _last_literals (:751-787) */
    {
        const uint32_t last_run = n - anchor;
        const uint32_t lit_length = (last_run + 255u - RUN_MASK) / 255u;
        if (limited && op + 1 + (int64_t)lit_length + last_run > oend) return 0;
        if (last_run >= (uint32_t)RUN_MASK) {
            const uint32_t acc = last_run - RUN_MASK;
            const uint32_t nb = acc / 255u;
            if (lane == 0) dst[op] = (uint8_t)(RUN_MASK << ML_BITS);
            wave_fill(dst + op + 1, 255, nb, lane);
            if (lane == 0) dst[op + 1 + nb] = (uint8_t)(acc - nb * 255u);
            op += 2 + nb;
        } else {
            if (lane == 0) dst[op] = (uint8_t)(last_run << ML_BITS);
            op++;
        }
        wave_copy(dst + op, c + anchor, last_run, lane);
        op += last_run;
    }
    return (int)op;
}

/* a wave takes the next message (longest first) when it is done with one: a batch of any size is one launch.  One way round the
 * loop and no `continue` ("A loop the compiler took apart"). */
__global__ __launch_bounds__(64 * DHC_WAVES_PER_WG) void k4_dict_hc_encode_kernel(DictHcEncArgs a)
{
    __shared__ uint32_t seen[DHC_WAVES_PER_WG][DHC_HEADS / 32u];
    const int lane = lane_id();
    const uint32_t wave = uni(threadIdx.x >> 6);
    const uint32_t slot = uni(blockIdx.x * (uint32_t)DHC_WAVES_PER_WG + wave);
    DhcState s;
    s.seen = seen[wave];
    for (uint32_t k = (uint32_t)lane; k < DHC_HEADS / 32u; k += 64u) s.seen[k] = 0u;
    wave_sync();
    s.mhead = (uint32_t *)(a.slots + (size_t)DHC_TABLE_BYTES * slot);
    s.mchain = (uint16_t *)(s.mhead + DHC_HEADS);
    for (;;) {
        uint32_t t = 0u;
        if (lane == 0) t = atomicAdd(a.ticket, 1u);
        t = uni(t);
        if ((long long)t >= a.n) break;
        const long long b = (long long)uni(a.order[t]);
        const int len = (int)uni((uint32_t)a.srcLen[b]);
        const int cap = (int)uni((uint32_t)a.dstCap[b]);
        const int di = (int)uni((uint32_t)a.dictIdx[b]);
        const bool listed = di >= 0 && di < a.nDict;
        int ret = 0;
        if (!listed) {
            dev_status_raise(lane == 0 ? a.status : nullptr, DEV_STATUS_DICT_INDEX);
        } else if (len > 0 && len <= MAX_INPUT_SIZE) {
            const uint32_t D = uni(a.keptLen[di]);
            const uint8_t *tb = a.tables + (size_t)DHC_TABLE_BYTES * uni(a.table[di]);
            s.dk = a.dict + a.keptOff[di];
            s.c = a.src + a.srcOff[b];
            s.dhead = (const uint32_t *)tb;
            s.dchain = (const uint16_t *)(s.dhead + DHC_HEADS);
            s.dl = DHC_LOW + D;
            s.next = s.dl;
            ret = dhc_block(s, (uint32_t)len, a.dst + a.dstOff[b], cap < 0 ? 0 : cap, a.level, lane);
            /* the heads this message wrote go back to zero: the positions [dl, next) were inserted */
            wave_sync();
            for (uint32_t i0 = s.dl; i0 < s.next; i0 += 64u) {
                const uint32_t idx = i0 + (uint32_t)lane;
                if (idx < s.next) s.mhead[dhc_hash(ld32u(s.c + (idx - s.dl)))] = 0u;
            }
        }
        if (lane == 0) a.outLen[b] = !listed ? -1 : len <= 0 ? 0 : ret <= 0 ? -1 : ret;      /* the LZ4Codec convention of k4lz4_encode_batch */
        wave_sync();
    }
}

}  // namespace k4
