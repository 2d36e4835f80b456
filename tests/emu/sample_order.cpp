/* tests/emu/sample_order.cpp -- the cost sample's own table (k4lz4_encode_fast.hpp, FastTable<3>; k4lz4_parse.hpp, parse_block's TT = 3
 * and parse_cost_body) and the stable order (k4_order_kernel) in the host wave emulator.  Built two ways by
 * tests/test_sample_table_order.py: as a shared library for k4emu_porder_threads below (the order launch run by a number of host
 * threads of the caller's choosing), and as a program of its own with -fsanitize=address:
 *   every block lies in an arena with poisoned bytes in front of it and behind it, and is sampled by a wave whose table and `seen`
 * set are heap blocks of exactly a wave's allotment (2 << K4_SAMPLE_HASH_BITS bytes and PARSE_SEEN_DWORDS words) -- a read outside
 * the block or an access outside the allotment stops the program; then the whole estimate and order over the same lengths: a
 * permutation, dearer buckets first, ascending indices inside a bucket, the same with one host thread and with four.  Before that
 * the order alone from given buckets (k4emu_order_only), cost[] and order[] heap blocks of exactly n words: launches whose stretches
 * are several steps of 256 blocks, and launches whose last workgroups have no stretch (70 000 blocks in 256 workgroups: stretches
 * of 512, nothing for workgroups 137 to 255), in both forms of the kernel.
 * Test infrastructure only. */
#include "hip/hip_runtime.h"
#include "k4lz4_decode.hpp"
#include "k4lz4_encode_fast.hpp"
#include "k4lz4_parse.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

extern "C" int k4emu_porder_threads(const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, long long n, uint32_t *cost, uint32_t *order,
                                    int cost_threads, int order_threads)
{
    k4::BatchArgs a{};
    a.src = src; a.srcOff = srcOff; a.srcLen = srcLen; a.n = n; a.accel = 1;
    std::vector<uint32_t> hist(2 * (size_t)k4::PCOST_BUCKETS, 0u);
    a.cost = cost; a.hist = hist.data(); a.order_out = order;
    if (n <= 0) return 0;
    k4emu::launch_fn(dim3((unsigned)((n + k4::PCOST_WAVES_PER_WG - 1) / k4::PCOST_WAVES_PER_WG)), dim3(64 * k4::PCOST_WAVES_PER_WG), [=] { k4::k4_pcost_kernel(a); }, cost_threads);
    k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_porder_kernel(a); }, order_threads);
    return 0;
}

/* the order alone, from given buckets (below 512 with fine, below 64 without), launched with `grid` workgroups (0: what the host
 * launches, order_workgroups); cost[] and order[] are the caller's, n words each */
extern "C" int k4emu_order_only(const uint32_t *cost, long long n, unsigned grid, int fine, int threads, uint32_t *order)
{
    const uint32_t nb = fine ? (uint32_t)k4::PCOST_BUCKETS : (uint32_t)k4::COST_BUCKETS;
    std::vector<uint32_t> hist(2 * (size_t)nb + 16, 0u);
    for (long long i = 0; i < n; i++) { if (cost[i] >= nb) return 1; hist[cost[i]]++; }
    k4::BatchArgs a{};
    a.n = n; a.cost = const_cast<uint32_t *>(cost); a.hist = hist.data(); a.order_out = order;
    if (n <= 0) return 0;
    k4emu::launch_fn(dim3(grid ? grid : k4::order_workgroups(n)), dim3(256), [=] { k4::k4_order_kernel(a, 0xffffffffu, fine); }, threads);
    return 0;
}

namespace {
/* order[] against cost[]: every index once, dearer buckets first, ascending indices inside a bucket */
bool stable_permutation(const uint32_t *cost, const uint32_t *order, long long n, const char *what)
{
    std::vector<int> met((size_t)n, 0);
    for (long long i = 0; i < n; i++) {
        const uint32_t o = order[i];
        if (o >= (uint32_t)n || met[o]++) { printf("%s: order[%lld] = %u\n", what, i, o); return false; }
        if (i && (cost[o] > cost[order[i - 1]] || (cost[o] == cost[order[i - 1]] && o < order[i - 1]))) { printf("%s: order[%lld] = %u is out of place\n", what, i, o); return false; }
    }
    return true;
}

/* k4_order_kernel where a workgroup's stretch is several steps of 256 blocks (the count of a bucket carried from step to step) and
 * where the last workgroups of the launch have no stretch at all; cost[] and order[] are heap blocks of exactly n words */
bool order_stretches()
{
    struct Case { long long n; unsigned grid; int fine; uint32_t buckets; } const cases[] = {
        {2000, 3, 1, 40}, {2000, 3, 0, 7}, {1793, 2, 1, 1}, {70000, 256, 1, 300}, {70000, 256, 0, 64}, {70000, 0, 1, 2}, {300000, 0, 1, 512}, {513, 256, 1, 9}};
    uint64_t x = 0x2545F4914F6CDD1Dull;
    for (const Case &c : cases) {
        uint32_t *cost = (uint32_t *)malloc((size_t)c.n * 4), *o1 = (uint32_t *)malloc((size_t)c.n * 4), *o4 = (uint32_t *)malloc((size_t)c.n * 4);
        if (!cost || !o1 || !o4) return false;
        for (long long i = 0; i < c.n; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; cost[i] = (uint32_t)((x >> 33) % c.buckets); o1[i] = o4[i] = 0xffffffffu; }
        char what[96];
        snprintf(what, sizeof what, "order of %lld blocks, grid %u, fine %d", c.n, c.grid, c.fine);
        if (k4emu_order_only(cost, c.n, c.grid, c.fine, 1, o1) || k4emu_order_only(cost, c.n, c.grid, c.fine, 4, o4)) return false;
        if (!stable_permutation(cost, o1, c.n, what)) return false;
        for (long long i = 0; i < c.n; i++) if (o1[i] != o4[i]) { printf("%s: order[%lld] differs with four threads\n", what, i); return false; }
        free(cost); free(o1); free(o4);
    }
    return true;
}

const uint32_t SAMPLE = k4::PCOST_FIT.sample;
const long long COUNTS[] = {1, 15, 16, 17, 255, 256, 257, 1025};
const size_t GAP = 64;

/* one block's sample by one wave, table and `seen` given */
void sample_one(const uint8_t *src, uint32_t len, uint16_t *tab, uint32_t *seen, uint32_t *out)
{
    k4emu::launch_fn(dim3(1), dim3(64), [=] {
        k4::ParseStats st;
        st.max_rounds = k4::PCOST_FIT.max_rounds;
        const uint32_t nseq = k4::parse_block<1, false, true, 3>(src, len, nullptr, tab, seen, k4::lane_id(), nullptr, &st);
        if (k4::lane_id() == 0) { out[0] = nseq; out[1] = st.rounds; out[2] = st.covered; }
    }, 1);
}
}

int main()
{
    const int LENGTHS[] = {0, 1, 12, 13, 127, 128, (int)SAMPLE - 1, (int)SAMPLE, (int)SAMPLE + 1, 4096, 65535, 65546, 65547};
    const int NL = (int)(sizeof(LENGTHS) / sizeof(LENGTHS[0]));
    uint64_t x = 0x9E3779B97F4A7C15ull;
    if (!order_stretches()) return 1;
    for (long long n : COUNTS) {
        std::vector<int32_t> len((size_t)n);
        std::vector<uint64_t> off((size_t)n);
        size_t total = GAP;
        for (long long i = 0; i < n; i++) {
            len[(size_t)i] = LENGTHS[(size_t)(i * 5 + n) % (size_t)NL];
            off[(size_t)i] = total;
            total += (((size_t)len[(size_t)i] + 7) & ~(size_t)7) + GAP;
        }
        uint8_t *arena = (uint8_t *)aligned_alloc(64, (total + 63) & ~(size_t)63);
        if (!arena) return 2;
        /* text-like and binary-like stretches in turn: short repeats, so that the sample meets matches, groups and stops */
        for (size_t k = 0; k < total; k++) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            arena[k] = (k / 4096) % 2 ? (uint8_t)(x >> 56) : (uint8_t)("the quick brown fox "[(k + (x >> 60)) % 20]);
        }
        POISON(arena, total);
        for (long long i = 0; i < n; i++) UNPOISON(arena + off[(size_t)i], (size_t)len[(size_t)i]);

        /* the sample form alone, in a wave's exact allotment (the blocks parse_cost_body gives it: PARSE_MIN_LEN .. LIMIT_64K - 1) */
        if (n <= 257) {
            for (long long i = 0; i < n; i++) {
                const int l = len[(size_t)i];
                if (l < (int)k4::PARSE_MIN_LEN || l >= k4::LIMIT_64K) continue;
                uint16_t *tab = (uint16_t *)aligned_alloc(16, (size_t)k4::PCOST_TABLE_DWORDS * 4);
                uint32_t *seen = (uint32_t *)aligned_alloc(16, (size_t)k4::PARSE_SEEN_DWORDS * 4);
                if (!tab || !seen) return 2;
                uint32_t out[3] = {0u, 0u, 0u};
                const uint32_t s = (uint32_t)l < SAMPLE ? (uint32_t)l : SAMPLE;
                sample_one(arena + off[(size_t)i], s, tab, seen, out);
                if (out[1] == 0u || out[1] > k4::PCOST_FIT.max_rounds || out[2] == 0u || out[2] > s) { printf("n %lld block %lld (%d bytes): rounds %u covered %u\n", n, i, l, out[1], out[2]); return 1; }
                free(tab); free(seen);
            }
        }

        std::vector<uint32_t> cost((size_t)n, 0xffffffffu), order1((size_t)n, 0xffffffffu), order4((size_t)n, 0xffffffffu), cost4((size_t)n, 0xffffffffu);
        k4emu_porder_threads(arena, off.data(), len.data(), n, cost.data(), order1.data(), 1, 1);
        k4emu_porder_threads(arena, off.data(), len.data(), n, cost4.data(), order4.data(), 4, 4);
        std::vector<int> met((size_t)n, 0);
        for (long long i = 0; i < n; i++) {
            const uint32_t o = order1[(size_t)i];
            if (cost[(size_t)i] >= (uint32_t)k4::PCOST_BUCKETS || cost4[(size_t)i] != cost[(size_t)i]) { printf("n %lld: block %lld: bucket %u / %u\n", n, i, cost[(size_t)i], cost4[(size_t)i]); return 1; }
            if (o >= (uint32_t)n || met[o]++) { printf("n %lld: order[%lld] = %u\n", n, i, o); return 1; }
            if (o != order4[(size_t)i]) { printf("n %lld: order[%lld] = %u with one thread, %u with four\n", n, i, o, order4[(size_t)i]); return 1; }
            if (i) {
                const uint32_t p = order1[(size_t)i - 1];
                if (cost[o] > cost[p]) { printf("n %lld: order[%lld] is dearer than the one before\n", n, i); return 1; }
                if (cost[o] == cost[p] && o < p) { printf("n %lld: order[%lld] = %u stands behind %u of its bucket\n", n, i, o, p); return 1; }
            }
        }
        UNPOISON(arena, total);
        free(arena);
    }
    printf("ok\n");
    return 0;
}
