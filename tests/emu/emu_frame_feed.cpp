/* tests/emu/emu_frame_feed.cpp -- the fed frame reader's kernels (k4lz4_frame_feed.hpp) compiled against the host wave emulator, in
 * a library of its own (tests/frame_feed_emu.py builds it).  One call of k4emu_ff_call is what k4lz4_frame_read_fed_batch_device
 * does for n streams: the same kernels on the caller's arrays.  Test infrastructure only. */
#include "hip/hip_runtime.h"

#include "k4lz4_frame_feed.hpp"

#include <vector>

extern "C" {

long long k4emu_ff_store_bytes(long long maxBlock, int fed)
{
    const long long mb = k4::fr_max_block(maxBlock);
    return fed ? k4::fr_fed_store_bytes(mb) : k4::fr_store_bytes(mb);
}
long long k4emu_ff_state_bytes() { return (long long)sizeof(k4::FrState); }

/* maxCount > 0 and a READ that is not interactive: the fast path's launches first, as the device form; plan_out (n words, may be
 * NULL): each stream's plan state after the commit (0 not planned, 1 planned and handed back, 2 served by the fast path) */
void k4emu_ff_call(long long maxBlock, uint8_t *store, const uint64_t *storeOff, const uint8_t *src, const uint64_t *srcOff,
                   const uint64_t *srcLen, const int64_t *final, uint8_t *dst, const uint64_t *dstOff, const int64_t *count,
                   int64_t *outLen, int64_t *consumed, int64_t *need, long long n, int op, int interactive, long long maxCount,
                   uint32_t *plan_out, int threads)
{
    if (n <= 0) return;
    k4::FrFeedArgs a{{src, srcOff, srcLen, store, storeOff, dst, dstOff, count, outLen, n, op, interactive, k4::fr_max_block(maxBlock), nullptr},
                     final, consumed, need};
    const dim3 waves((unsigned)((n + k4::FR_WAVES_PER_WG - 1) / k4::FR_WAVES_PER_WG)), wg(64 * k4::FR_WAVES_PER_WG);
    const long long rows = k4::fr_table_rows(maxCount);
    std::vector<uint32_t> done((size_t)n);
    if (op == k4::FR_OP_READ && !interactive && rows > 0) {
        const size_t nr = (size_t)(n * rows) + 1;
        std::vector<k4::FrPlan> plan((size_t)n);
        std::vector<uint32_t> sum(nr), got(nr), lc(nr), tl((size_t)n), tw((size_t)n);
        std::vector<uint64_t> so(nr), dof(nr), hl(nr), sso((size_t)n), sdo((size_t)n);
        std::vector<int32_t> sl(nr), dc(nr), ol(nr), ssl((size_t)n), sdc((size_t)n), sol((size_t)n);
        k4::FrFeedFastArgs ff{};
        k4::FrFastArgs &f = ff.f;
        f.r = a.r; f.rows = rows; f.plan = plan.data(); f.done = done.data();
        f.srcOff = so.data(); f.dstOff = dof.data(); f.hlen = hl.data(); f.srcLen = sl.data(); f.dstCap = dc.data(); f.outLen = ol.data();
        f.sum = sum.data(); f.got = got.data(); f.lc = lc.data();
        f.sSrcOff = sso.data(); f.sDstOff = sdo.data(); f.sSrcLen = ssl.data(); f.sDstCap = sdc.data(); f.sOutLen = sol.data();
        ff.final = final; ff.consumed = consumed; ff.need = need; ff.tail = tl.data(); ff.want = tw.data();
        k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_fr_feed_plan_kernel(ff); }, threads);
        const long long nb = n * rows;
        k4::HashArgs ha{src, f.srcOff, f.hlen, f.got, nb, 0u};
        k4emu::launch_fn(dim3((unsigned)((nb * 4 + k4::XXH_THREADS - 1) / k4::XXH_THREADS)), dim3(k4::XXH_THREADS), [=] { k4::k4_xxh32_kernel(ha); }, threads);
        k4::BatchArgs b1{};
        b1.src = src; b1.srcOff = f.srcOff; b1.srcLen = f.srcLen; b1.dst = dst; b1.dstOff = f.dstOff; b1.dstCap = f.dstCap; b1.outLen = f.outLen; b1.n = nb;
        k4emu::launch_fn(dim3((unsigned)((nb + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG)), dim3(64 * k4::DECODE_WAVES_PER_WG),
                         [=] { k4::k4_decode_kernel(b1); }, threads);
        k4::BatchArgs b2{};
        b2.src = src; b2.srcOff = f.sSrcOff; b2.srcLen = f.sSrcLen; b2.dst = store; b2.dstOff = f.sDstOff; b2.dstCap = f.sDstCap; b2.outLen = f.sOutLen; b2.n = n;
        k4emu::launch_fn(dim3((unsigned)((n + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG)), dim3(64 * k4::DECODE_WAVES_PER_WG),
                         [=] { k4::k4_decode_kernel(b2); }, threads);
        k4emu::launch_fn(waves, wg, [=] { k4::k4_fr_feed_commit_kernel(ff); }, threads);
        for (long long i = 0; plan_out && i < n; i++) plan_out[i] = done[(size_t)i] == k4::FR_PLAN_DONE ? 2u : plan[(size_t)i].state;
        a.r.done = done.data();
    } else {
        for (long long i = 0; plan_out && i < n; i++) plan_out[i] = 0u;
    }
    k4emu::launch_fn(waves, wg, [=] { k4::k4_fr_feed_kernel(a); }, threads);
}

/* the whole-source reader of 4.14 on the same arrays (one launch of k4_fr_read_kernel), for comparisons of the two */
void k4emu_ff_whole_call(long long maxBlock, uint8_t *store, const uint64_t *storeOff, const uint8_t *src, const uint64_t *srcOff,
                         const uint64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const int64_t *count, int64_t *outLen, long long n, int op,
                         int interactive, int threads)
{
    if (n <= 0) return;
    const k4::FrReadArgs a{src, srcOff, srcLen, store, storeOff, dst, dstOff, count, outLen, n, op, interactive, k4::fr_max_block(maxBlock), nullptr};
    k4emu::launch_fn(dim3((unsigned)((n + k4::FR_WAVES_PER_WG - 1) / k4::FR_WAVES_PER_WG)), dim3(64 * k4::FR_WAVES_PER_WG),
                     [=] { k4::k4_fr_read_kernel(a); }, threads);
}

void k4emu_ff_query(const uint8_t *store, const uint64_t *storeOff, int64_t *out, long long n, int threads)
{
    if (n <= 0) return;
    k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_fr_query_kernel(store, storeOff, out, n); }, threads);
}

}  // extern "C"
