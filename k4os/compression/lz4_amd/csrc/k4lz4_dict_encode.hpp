/*
 * k4lz4_dict_encode.hpp -- batches of messages encoded against shared dictionaries (k4lz4_encode_dict_batch), fast levels.
 *
 * Replaces, for many messages at once, the idiom "load the dictionary once, copy the stream state for every message":
 *   LL64.LZ4_loadDict                           Engine/x64/LL64.tools.cs:175-206
 *   LL64.LZ4_compress_fast_continue             Engine/x64/LL64.fast.cs:582-667   (the dictionary does not lie in front of the source)
 *   LL64.LZ4_compress_generic                   Engine/x64/LL64.fast.cs:34-513    (byU32 + hash5, acceleration 1, usingExtDict,
 *                                               dictSmall iff the kept dictionary is shorter than 64 KiB; limitedOutput)
 * with byte-identical blocks.
 *
 * Load (k4_dict_load_kernel), one workgroup per distinct dictionary.  Only the last 64 KiB count; the positions p = kept start,
 * + 3, + 6, ... while p <= dictEnd - 8 are put with the index 65536 - (dictEnd - p): currentOffset is 64 KiB after the load whatever
 * the dictionary's length, so the dictionary ends at index 65536 and the message begins there.  The reference puts in order and the
 * last put of a hash wins; the indices grow with p, so threads over the positions with atomicMax build the same table (as the
 * chained encoder's probes do, k4lz4_fast_chain.hpp).  A dictionary of fewer than 8 bytes leaves the table empty and dictSize 0.
 *
 * An empty slot is 0, and index 0 is never a usable candidate, so the two cannot be told apart and need not be: with a full
 * dictionary (64 KiB kept, the only case in which a put has index 0) every position of the message has an index of 65536 or more
 * and the distance check matchIndex + 65535 < current refuses index 0; with a smaller one the parse runs under dictSmall and
 * prefixIdxLimit = 65536 - dictSize > 0 refuses it.  The refusals come before the candidate's bytes are looked at.
 *
 * Encode (k4_dict_encode_kernel), one wavefront per message, handed out longest first by a ticket.  A wave copies its dictionary's
 * table (16 KiB, L2-resident) into its LDS table and parses the one block the way fast_chain_block does (64 probes per window,
 * the same-hash rule, atomicMax puts), in the usingExtDict arm: startIndex = 65536; a candidate below it lives in the dictionary's
 * memory (at kept start + index - prefixIdxLimit), one at or above it in the message's.  The backward extension stops at the start
 * of the buffer the match lies in (the kept start or the message's first byte: both are position 0 of their buffer here); a
 * dictionary match that reaches dictEnd goes on against the message's first bytes (:314-324).  The two buffers are never read as if
 * they were contiguous: the dictionary's loads are the four bytes of a candidate, which the load step only puts at dictEnd - 8 or
 * before, and count_exact, which assembles a tail of fewer than four bytes from single bytes.
 */
#pragma once
#include "k4lz4_fast_chain.hpp"

namespace k4 {

constexpr uint32_t DICT_START = 65536u;               /* currentOffset after LZ4_loadDict: the message's first byte has this index */
constexpr int DICT_LOAD_THREADS = 256;

struct DictLoadArgs {
    const uint8_t *dict;
    const uint64_t *keptOff;    /* per table: where the kept bytes (the last <= 64 KiB) start in dict */
    const uint32_t *keptLen;    /* per table: dictSize -- 0 for a dictionary of fewer than 8 bytes */
    uint32_t *tables;           /* 4096 words per table */
};

struct DictEncArgs {
    const uint8_t *src;
    const uint64_t *srcOff;
    const int32_t *srcLen;
    uint8_t *dst;
    const uint64_t *dstOff;
    const int32_t *dstCap;
    int32_t *outLen;
    const int32_t *dictIdx;     /* per message: its entry of the dictionary list */
    const uint8_t *dict;
    /* per entry of the list */
    const uint64_t *keptOff;
    const uint32_t *keptLen;
    const uint32_t *table;      /* which of the prepared tables is its */
    const uint32_t *tables;
    const uint32_t *order;      /* messages, longest first */
    uint32_t *ticket;           /* one zeroed word: messages handed out */
    uint32_t *status;           /* the context's status word, or nullptr */
    long long n;
    int nDict;
};

__global__ __launch_bounds__(DICT_LOAD_THREADS) void k4_dict_load_kernel(DictLoadArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t tab[4096];
    const uint32_t t = blockIdx.x;
    for (uint32_t k = threadIdx.x; k < 4096u; k += (uint32_t)DICT_LOAD_THREADS) tab[k] = 0u;     /* LZ4_resetStream */
    __syncthreads();
    const uint32_t len = a.keptLen[t];
    if (len >= 8u) {                                                   /* HASH_UNIT */
        const uint8_t *d = a.dict + a.keptOff[t];
        const uint32_t np = (len - 8u) / 3u + 1u;                      /* p = 0, 3, ... while p <= len - 8 */
        for (uint32_t k = threadIdx.x; k < np; k += (uint32_t)DICT_LOAD_THREADS) {
            const uint32_t p = 3u * k;
            atomicMax(&tab[ChainTable::hash(d + p)], DICT_START - (len - p));
        }
    }
    __syncthreads();
    uint4 *out = (uint4 *)(a.tables + 4096ull * t);
    for (uint32_t k = threadIdx.x; k < 1024u; k += (uint32_t)DICT_LOAD_THREADS) out[k] = ((const uint4 *)tab)[k];
}

/* two buckets per octave of the length, below COST_BUCKETS (the lengths are below 2^31): what k4_order_kernel sorts by */
__device__ __forceinline__ uint32_t len_bucket(uint32_t len)
{
    if (len < 4u) return len;
    const uint32_t l = 31u - (uint32_t)__clz((int)len);
    return 2u * l + ((len >> (l - 1u)) & 1u);
}

/* cost bucket per message by its length and the buckets' counts, for k4_order_kernel (k4lz4_encode_fast.hpp): BatchArgs'
 * srcLen, n, cost and hist (zeroed) are what it reads and writes */
__global__ __launch_bounds__(256) void k4_dict_cost_kernel(BatchArgs a)
{
    __shared__ uint32_t h[COST_BUCKETS];
    if (threadIdx.x < (unsigned)COST_BUCKETS) h[threadIdx.x] = 0u;
    __syncthreads();
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b < a.n) {
        const int len = a.srcLen[b];
        const uint32_t bkt = len_bucket(len > 0 ? (uint32_t)len : 0u);
        a.cost[b] = bkt;
        atomicAdd(&h[bkt], 1u);
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)COST_BUCKETS && h[threadIdx.x]) atomicAdd(&a.hist[threadIdx.x], h[threadIdx.x]);
}

/* number of equal bytes at a[] / b[], at most maxn, reading no byte at or behind a + maxn or b + maxn */
__device__ __forceinline__ uint32_t count_exact(const uint8_t *a, const uint8_t *b, uint32_t maxn, int lane)
{
    uint32_t done = 0;
    for (;;) {
        const uint32_t i = done + 4u * (uint32_t)lane;
        uint32_t neq = 0;
        if (i < maxn) {
            const uint32_t avail = maxn - i < 4u ? maxn - i : 4u;
            uint32_t x = 0;
            if (avail == 4u) x = ld32u(a + i) ^ ld32u(b + i);
            else for (uint32_t k = 0; k < avail; k++) x |= (uint32_t)(a[i + k] ^ b[i + k]) << (8u * k);
            const uint32_t e = x ? (uint32_t)(__ffs(x) - 1) >> 3 : 4u;
            neq = e < avail ? e : avail;
        }
        const unsigned long long notfull = ballot(neq != 4u);
        if (!notfull) { done += 256u; continue; }
        const int fl = ctz64(notfull);
        return done + 4u * (uint32_t)fl + readlane_u32(neq, fl);
    }
}

/* LL64.LZ4_compress_generic, usingExtDict, for one message behind a loaded dictionary.  c: the message (n > 0 bytes), dk: the kept
 * dictionary (dsize bytes, 0 or 8 .. 65536), tab: the wave's copy of the dictionary's table (LDS), seen: the wave's hash bits (zero
 * on entry and on return).  Returns the block's length, 0 when it does not fit `cap` (the reference returns 0 there). */
__device__ __forceinline__ int dict_block(const uint8_t *c, const uint32_t n, const uint8_t *dk, const uint32_t dsize, uint32_t *tab, uint32_t *seen,
                                          uint8_t *dst, const int cap, const int lane)
{
    const bool small = dsize < 65536u;                                   /* dictSmall: dictSize < 64 KiB (and < currentOffset = 64 KiB) (:650) */
    const uint32_t pfx = DICT_START - dsize;                             /* prefixIdxLimit: the kept start's index */
    const uint32_t iend = n;
    const uint32_t ucap = (uint32_t)cap;
    uint32_t op = 0u, anchor = 0u;

    /* a candidate (index mi) for the position p: the reference's refusals, then its first four bytes from the buffer it lies in */
    auto usable = [&](uint32_t mi, uint32_t p) -> bool {
        const uint32_t cur = DICT_START + p;
        if (small && mi < pfx) return false;                             /* :219-220, :450 */
        if (mi + (uint32_t)DISTANCE_MAX < cur) return false;             /* :221-224 */
        if (mi >= cur) return false;                                     /* (never) */
        if (mi < DICT_START) {
            if (mi < pfx || mi + (uint32_t)MINMATCH > DICT_START) return false;     /* (never with a table the load step wrote) */
            return ld32u(dk + (mi - pfx)) == ld32u(c + p);
        }
        return ld32u(c + (mi - DICT_START)) == ld32u(c + p);
    };

    if (n >= (uint32_t)MFLIMIT + 1u) {                                 /* LZ4_minLength (:130) */
        const uint32_t mfl1 = iend - (uint32_t)MFLIMIT + 1u;             /* mflimitPlusOne */
        const uint32_t mlimit = iend - (uint32_t)LASTLITERALS;           /* matchlimit */
        uint32_t ip = 0u;
        {   /* first byte (:134) */
            const uint32_t h = ChainTable::hash(c);
            wave_sync();
            tab[h] = DICT_START;
            wave_sync();
        }
        ip++;
        bool done = false;
        while (!done) {
            /* ---- search (:156-231): windows of 64 probes ---- */
            uint32_t mi_found = 0u;
            bool found = false;
            const uint32_t s0 = ip;
            for (uint32_t t = 0u;; t += 64u) {
                const uint32_t q = s0 + probe_offset(t + (uint32_t)lane, 1u);
                const uint32_t qn = s0 + probe_offset(t + (uint32_t)lane + 1u, 1u);
                const bool val = qn <= mfl1;                             /* :172: probe t is made only if probe t + 1 is still inside */
                const uint32_t qq = val ? q : 0u;
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
                        if (!got && lane >= d && hd == h) { mi = DICT_START + qd; got = true; }
                    }
                }
                wave_sync();
                if (val) seen[bit >> 5] = 0u;
                const bool ok = val && usable(mi, q);
                const unsigned long long hitm = ballot(ok);
                const int f = hitm ? ctz64(hitm) : 64;
                wave_sync();
                if (val && lane <= f) atomicMax(&tab[h], DICT_START + q);     /* :176 put of every probe made, the hit's included */
                wave_sync();
                if (hitm) {
                    ip = readlane_u32(q, f);
                    mi_found = readlane_u32(mi, f);
                    found = true;
                    break;
                }
                if (valm != ~0ull) break;                                /* :172 -> _last_literals */
            }
            if (!found) break;

            /* where the match lies (:193-206): the dictionary's memory or the message's; `match` counts from that buffer's start */
            uint32_t off = DICT_START + ip - mi_found;                   /* :228: offset = current - matchIndex */
            bool ind = mi_found < DICT_START;
            const uint8_t *mb = ind ? dk : c;
            uint32_t match = ind ? mi_found - pfx : mi_found - DICT_START;

            /* ---- catch up (:237-242): lowLimit is the start of the match's buffer ---- */
            {
                const uint32_t bmax = min(ip - anchor, match);
                uint32_t back = 0u;
                for (uint32_t k0 = 0u; k0 < bmax; k0 += 64u) {
                    const uint32_t i = k0 + (uint32_t)lane;
                    const bool eq = i < bmax && c[ip - 1u - i] == mb[match - 1u - i];
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
                if (lane == 0) { dst[op] = (uint8_t)off; dst[op + 1u] = (uint8_t)(off >> 8); }
                op += 2u;
                uint32_t mc;
                if (ind) {                                               /* :314-324: up to dictEnd, then on against the message's start */
                    const uint32_t lim = min(ip + (dsize - match), mlimit);
                    mc = count_exact(c + ip + (uint32_t)MINMATCH, mb + match + (uint32_t)MINMATCH, lim - (ip + (uint32_t)MINMATCH), lane);
                    if (ip + (uint32_t)MINMATCH + mc == lim) mc += count_exact(c + lim, c, mlimit - lim, lane);
                } else {
                    mc = count_exact(c + ip + (uint32_t)MINMATCH, mb + match + (uint32_t)MINMATCH, mlimit - (ip + (uint32_t)MINMATCH), lane);
                }
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
                tab[h2] = DICT_START + ip - 2u;                              /* :394 fill table */
                wave_sync();
                const uint32_t mi = tab[h];
                wave_sync();
                tab[h] = DICT_START + ip;                                    /* :445 */
                wave_sync();
                if (!usable(mi, ip)) break;
                off = DICT_START + ip - mi;
                ind = mi < DICT_START;
                mb = ind ? dk : c;
                match = ind ? mi - pfx : mi - DICT_START;
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

/* a wave takes the next message (longest first) when it is done with one: a batch of any size is one launch */
__global__ __launch_bounds__(64 * FAST_CHAIN_WAVES_PER_WG) void k4_dict_encode_kernel(DictEncArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[FAST_CHAIN_WAVES_PER_WG][FAST_CHAIN_LDS_DWORDS];
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
        const long long b = (long long)uni(a.order[t]);
        const int len = (int)uni((uint32_t)a.srcLen[b]);
        const int cap = (int)uni((uint32_t)a.dstCap[b]);
        const int di = (int)uni((uint32_t)a.dictIdx[b]);
        /* (one way round the loop, no `continue`: with a second back edge the compiler sent the lanes other than 0 round again without
         * lane 0 and its ticket -- they never finish) */
        const bool listed = di >= 0 && di < a.nDict;
        int ret = 0;
        if (!listed) {
            dev_status_raise(lane == 0 ? a.status : nullptr, DEV_STATUS_DICT_INDEX);
        } else if (len > 0 && len <= MAX_INPUT_SIZE) {
            const uint32_t dsize = uni(a.keptLen[di]);
            if (len >= MFLIMIT + 1) {                                /* shorter messages are literals alone and never look at the table */
                const uint4 *seed = (const uint4 *)(a.tables + 4096ull * uni(a.table[di]));
                wave_sync();
                for (int k = lane; k < 1024; k += 64) ((uint4 *)tab)[k] = seed[k];
                wave_sync();
            }
            ret = dict_block(a.src + a.srcOff[b], (uint32_t)len, a.dict + a.keptOff[di], dsize, tab, seen, a.dst + a.dstOff[b], cap < 0 ? 0 : cap, lane);
        }
        if (lane == 0) a.outLen[b] = !listed ? -1 : len <= 0 ? 0 : ret <= 0 ? -1 : ret;      /* the LZ4Codec convention of k4lz4_encode_batch */
        wave_sync();
    }
}

}  // namespace k4
