/* tests/emu/parse_cost_main.cpp -- a program of its own around the two-step encoder's cost estimate and order (k4lz4_parse.hpp:
 * parse_cost_body; k4lz4_encode_fast.hpp: k4_order_kernel's fine form) in the host wave emulator, meant to be built with
 * -fsanitize=address (tests/test_parse_cost_order.py does).  Every block of a batch lies in an arena with poisoned bytes in front
 * of it and behind it, so a sample that reads outside its block stops the program; the order that comes out must hold every index
 * once.  Test infrastructure only. */
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

static const int LENGTHS[] = {0, 1, 127, 128, 129, 65535, 65546, 65547};
static const long long COUNTS[] = {1, 2, 15, 16, 17, 255, 256, 257};
static const size_t GAP = 64;

int main()
{
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (long long n : COUNTS) {
        std::vector<int32_t> len((size_t)n);
        std::vector<uint64_t> off((size_t)n);
        size_t total = GAP;
        for (long long i = 0; i < n; i++) {
            len[(size_t)i] = LENGTHS[(size_t)(i * 5 + n) % 8];
            off[(size_t)i] = total;
            total += (((size_t)len[(size_t)i] + 7) & ~(size_t)7) + GAP;
        }
        uint8_t *arena = (uint8_t *)aligned_alloc(64, (total + 63) & ~(size_t)63);
        if (!arena) return 2;
        /* text-like and binary-like blocks in turn: short repeats, so that the sample meets matches, groups and stops */
        for (size_t k = 0; k < total; k++) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            arena[k] = (k / 4096) % 2 ? (uint8_t)(x >> 56) : (uint8_t)("the quick brown fox "[(k + (x >> 60)) % 20]);
        }
        POISON(arena, total);
        for (long long i = 0; i < n; i++) UNPOISON(arena + off[(size_t)i], (size_t)len[(size_t)i]);
        std::vector<uint32_t> cost((size_t)n, 0xffffffffu), order((size_t)n, 0xffffffffu), hist(2 * (size_t)k4::PCOST_BUCKETS, 0u);
        k4::BatchArgs a{};
        a.src = arena; a.srcOff = off.data(); a.srcLen = len.data(); a.n = n; a.accel = 1;
        a.cost = cost.data(); a.hist = hist.data(); a.order_out = order.data();
        k4emu::launch_fn(dim3((unsigned)((n + k4::PCOST_WAVES_PER_WG - 1) / k4::PCOST_WAVES_PER_WG)), dim3(64 * k4::PCOST_WAVES_PER_WG), [=] { k4::k4_pcost_kernel(a); }, 1);
        k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_porder_kernel(a); }, 1);
        std::vector<int> seen((size_t)n, 0);
        for (long long i = 0; i < n; i++) {
            if (cost[(size_t)i] >= (uint32_t)k4::PCOST_BUCKETS) { printf("n %lld: block %lld has no bucket\n", n, i); return 1; }
            if (order[(size_t)i] >= (uint32_t)n || seen[order[(size_t)i]]++) { printf("n %lld: order[%lld] = %u\n", n, i, order[(size_t)i]); return 1; }
            if (i && cost[order[(size_t)i]] > cost[order[(size_t)i - 1]]) { printf("n %lld: order[%lld] is dearer than the one before\n", n, i); return 1; }
        }
        UNPOISON(arena, total);
        free(arena);
    }
    printf("ok\n");
    return 0;
}
