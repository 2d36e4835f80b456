/* tests/emu/emu_legacy_feed.cpp -- the fed LZ4Stream reader's kernels (k4lz4_legacy_feed.hpp) compiled against the host wave emulator,
 * in a library of its own (tests/legacy_feed_emu.py builds it).  One call of k4emu_lf_call is what k4lz4_legacy_read_fed_batch_device
 * does for n streams: the same kernels on the caller's arrays.  Test infrastructure only. */
#include "hip/hip_runtime.h"

/* (the emulator has the 32-bit form only; k4_lr_copy_kernel is compiled here but not run) */
static inline unsigned long long atomicMin(unsigned long long *p, unsigned long long v)
{
    unsigned long long cur = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return cur;
}

#include "k4lz4_legacy_feed.hpp"

#include <vector>

extern "C" {

long long k4emu_lf_store_bytes(long long maxBlock, int fed) { return fed ? k4::ls_fed_store_bytes(maxBlock) : k4::ls_rd_store_bytes(maxBlock); }
long long k4emu_lf_state_bytes() { return (long long)(sizeof(k4::LsState) + sizeof(k4::LsFeedExt)); }

/* maxCount > 0 and a READ that is not interactive: the direct path's launches first, as the device form; topup != 0: with its top-up
 * step (0 leaves it out: what a build without it would do).  plan_out (n words, may be NULL): each stream's plan state after the
 * commit (0 not planned, 1 planned and handed back, 2 served by the direct path); head_out (n words, may be NULL): the bytes the
 * top-up step took from each piece */
void k4emu_lf_call(long long maxBlock, uint8_t *store, const uint64_t *storeOff, const uint8_t *src, const uint64_t *srcOff,
                   const uint64_t *srcLen, const int64_t *final, uint8_t *dst, const uint64_t *dstOff, const int64_t *count,
                   int64_t *outLen, int64_t *consumed, int64_t *need, long long n, int op, int interactive, long long maxCount,
                   int topup, uint32_t *plan_out, uint32_t *head_out, int threads)
{
    if (n <= 0) return;
    k4::LsFeedArgs a{{src, srcOff, srcLen, store, storeOff, dst, dstOff, count, outLen, n, op, interactive, (int32_t)maxBlock, nullptr},
                     final, consumed, need, nullptr};
    const dim3 waves((unsigned)((n + k4::LS_WAVES_PER_WG - 1) / k4::LS_WAVES_PER_WG)), wg(64 * k4::LS_WAVES_PER_WG);
    const long long rows = k4::ls_table_rows(maxCount, maxBlock);
    std::vector<uint32_t> done((size_t)n, 0), head((size_t)n, 0);
    for (long long i = 0; i < n; i++) {
        if (plan_out) plan_out[i] = 0u;
        if (head_out) head_out[i] = 0u;
    }
    if (op == k4::LS_OP_READ && !interactive && rows > 0) {
        const size_t nr = (size_t)(n * rows) + 1;
        std::vector<k4::LsFeedPlan> plan((size_t)n);
        std::vector<uint64_t> so(nr), dof(nr), sso((size_t)n), sdo((size_t)n);
        std::vector<int32_t> sl(nr), dc(nr), ol(nr), ssl((size_t)n), sdc((size_t)n), sol((size_t)n);
        std::vector<uint32_t> raw(nr);
        k4::LsFeedDirectArgs f{};
        f.f = a; f.rows = rows; f.plan = plan.data(); f.done = done.data(); f.head = head.data();
        f.srcAddr = so.data(); f.dstAddr = dof.data(); f.srcLen = sl.data(); f.dstCap = dc.data(); f.outLen = ol.data(); f.rawLen = raw.data();
        f.sSrcAddr = sso.data(); f.sDstAddr = sdo.data(); f.sSrcLen = ssl.data(); f.sDstCap = sdc.data(); f.sOutLen = sol.data();
        if (topup) k4emu::launch_fn(waves, wg, [=] { k4::k4_ls_feed_topup_kernel(f); }, threads);
        k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_ls_feed_plan_kernel(f); }, threads);
        const long long nb = n * rows;
        k4::BatchArgs b1{};
        b1.src = nullptr; b1.srcOff = f.srcAddr; b1.srcLen = f.srcLen; b1.dst = nullptr; b1.dstOff = f.dstAddr; b1.dstCap = f.dstCap; b1.outLen = f.outLen; b1.n = nb;
        k4emu::launch_fn(dim3((unsigned)((nb + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG)), dim3(64 * k4::DECODE_WAVES_PER_WG),
                         [=] { k4::k4_decode_kernel(b1); }, threads);
        k4::BatchArgs b2{};
        b2.src = nullptr; b2.srcOff = f.sSrcAddr; b2.srcLen = f.sSrcLen; b2.dst = nullptr; b2.dstOff = f.sDstAddr; b2.dstCap = f.sDstCap; b2.outLen = f.sOutLen; b2.n = n;
        k4emu::launch_fn(dim3((unsigned)((n + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG)), dim3(64 * k4::DECODE_WAVES_PER_WG),
                         [=] { k4::k4_decode_kernel(b2); }, threads);
        k4emu::launch_fn(waves, wg, [=] { k4::k4_ls_feed_commit_kernel(f); }, threads);
        for (long long i = 0; i < n; i++) {
            if (plan_out) plan_out[i] = done[(size_t)i] == k4::LS_PLAN_DONE ? 2u : plan[(size_t)i].state;
            if (head_out) head_out[i] = head[(size_t)i];
        }
        a.r.done = done.data(); a.head = head.data();
    }
    k4emu::launch_fn(waves, wg, [=] { k4::k4_ls_feed_kernel(a); }, threads);
}

/* the whole-source reader of 4.16 on the same arrays (one launch of k4_ls_read_kernel), for comparisons of the two */
void k4emu_lf_whole_call(long long maxBlock, uint8_t *store, const uint64_t *storeOff, const uint8_t *src, const uint64_t *srcOff,
                         const uint64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const int64_t *count, int64_t *outLen, long long n, int op,
                         int interactive, int threads)
{
    if (n <= 0) return;
    const k4::LsReadArgs a{src, srcOff, srcLen, store, storeOff, dst, dstOff, count, outLen, n, op, interactive, (int32_t)maxBlock, nullptr};
    k4emu::launch_fn(dim3((unsigned)((n + k4::LS_WAVES_PER_WG - 1) / k4::LS_WAVES_PER_WG)), dim3(64 * k4::LS_WAVES_PER_WG),
                     [=] { k4::k4_ls_read_kernel(a); }, threads);
}

void k4emu_lf_query(const uint8_t *store, const uint64_t *storeOff, int64_t *out, long long n, int threads)
{
    if (n <= 0) return;
    k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_ls_query_kernel(store, storeOff, out, n); }, threads);
}

}  // extern "C"
