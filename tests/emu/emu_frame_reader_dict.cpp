/* tests/emu/emu_frame_reader_dict.cpp -- the incremental frame readers against a dictionary set (k4lz4_frame_reader_dict.hpp) compiled
 * against the host wave emulator, in a library of its own (tests/frame_reader_dict_emu.py builds it).  One call of k4emu_frd_call is
 * what k4lz4_frame_read_dictset_batch_device (fed == 0) or k4lz4_frame_read_fed_dictset_batch_device (fed != 0) does for n streams:
 * read_device's launch sequence (k4lz4_capi.hip) over the same kernels on the caller's arrays.  nDict < 0: no set, the kernels of
 * the plain calls.  Test infrastructure only. */
#include "hip/hip_runtime.h"

#include "k4lz4_frame_reader_dict.hpp"

#include <vector>

namespace {

/* the fast path's tables, on the host */
struct Tables {
    std::vector<k4::FrPlan> plan;
    std::vector<uint32_t> done, sum, got, lc, tl, tw, entry;
    std::vector<uint64_t> so, dof, hl, sso, sdo, dictOff, sDictOff;
    std::vector<int32_t> sl, dc, ol, ssl, sdc, sol, dictLen, sDictLen;
    std::vector<signed char> dictMode, sDictMode;
    Tables(size_t n, size_t nr)
        : plan(n), done(n), sum(nr), got(nr), lc(nr), tl(n), tw(n), entry(n), so(nr), dof(nr), hl(nr), sso(n), sdo(n), dictOff(nr), sDictOff(n),
          sl(nr), dc(nr), ol(nr), ssl(n), sdc(n), sol(n), dictLen(nr), sDictLen(n), dictMode(nr), sDictMode(n) {}
    void place(k4::FrFastArgs &f, long long rows)
    {
        f.rows = rows; f.plan = plan.data(); f.done = done.data();
        f.srcOff = so.data(); f.dstOff = dof.data(); f.hlen = hl.data(); f.srcLen = sl.data(); f.dstCap = dc.data(); f.outLen = ol.data();
        f.sum = sum.data(); f.got = got.data(); f.lc = lc.data();
        f.sSrcOff = sso.data(); f.sDstOff = sdo.data(); f.sSrcLen = ssl.data(); f.sDstCap = sdc.data(); f.sOutLen = sol.data();
    }
    void place(k4::FrDictRows &w, const k4::FrDict &d)
    {
        w.d = d;
        w.dictOff = dictOff.data(); w.dictLen = dictLen.data(); w.dictMode = dictMode.data();
        w.sDictOff = sDictOff.data(); w.sDictLen = sDictLen.data(); w.sDictMode = sDictMode.data(); w.entry = entry.data();
    }
};

}  // namespace

extern "C" {

long long k4emu_frd_store_bytes(long long maxBlock, int fed)
{
    const long long mb = k4::fr_max_block(maxBlock);
    return fed ? k4::fr_fed_store_bytes(mb) : k4::fr_store_bytes(mb);
}

/* maxCount > 0 and a READ that is not interactive: the fast path's launches first, as the device form; plan_out (n words, may be
 * NULL): each stream's plan state after the commit (0 not planned, 1 planned and handed back, 2 served by the fast path).
 * final, consumed, need: the fed form's (ignored with fed == 0) */
void k4emu_frd_call(int fed, long long maxBlock, uint8_t *store, const uint64_t *storeOff, const uint8_t *src, const uint64_t *srcOff,
                    const uint64_t *srcLen, const int64_t *final, uint8_t *dst, const uint64_t *dstOff, const int64_t *count, int64_t *outLen,
                    int64_t *consumed, int64_t *need, long long n, int op, int interactive, long long maxCount, uint32_t *plan_out,
                    const uint8_t *dict, const uint64_t *entryOff, const int32_t *entryLen, const uint32_t *ids, int nDict, int threads)
{
    if (n <= 0) return;
    const bool set = nDict >= 0;
    const k4::FrDict d{dict, entryOff, entryLen, ids, set ? nDict : 0};
    k4::FrReadArgs r{src, srcOff, srcLen, store, storeOff, dst, dstOff, count, outLen, n, op, interactive, k4::fr_max_block(maxBlock), nullptr};
    const dim3 waves((unsigned)((n + k4::FR_WAVES_PER_WG - 1) / k4::FR_WAVES_PER_WG)), wg(64 * k4::FR_WAVES_PER_WG);
    const long long rows = op == k4::FR_OP_READ && !interactive ? k4::fr_table_rows(maxCount) : 0;
    Tables t((size_t)n, (size_t)(n * rows) + 1);
    for (long long i = 0; plan_out && i < n; i++) plan_out[i] = 0u;
    if (rows > 0) {
        k4::FrDictFastArgs df{};
        k4::FrDictFeedFastArgs dff{};
        k4::FrFastArgs &f = fed ? dff.f.f : df.f;
        f.r = r;
        t.place(f, rows);
        t.place(fed ? dff.w : df.w, d);
        if (fed) {
            dff.f.final = final; dff.f.consumed = consumed; dff.f.need = need; dff.f.tail = t.tl.data(); dff.f.want = t.tw.data();
        }
        const dim3 pgrid((unsigned)((n + 255) / 256));
        if (fed && set) k4emu::launch_fn(pgrid, dim3(256), [=] { k4::k4_fr_dict_feed_plan_kernel(dff); }, threads);
        else if (fed) k4emu::launch_fn(pgrid, dim3(256), [=] { k4::k4_fr_feed_plan_kernel(dff.f); }, threads);
        else if (set) k4emu::launch_fn(pgrid, dim3(256), [=] { k4::k4_fr_dict_plan_kernel(df); }, threads);
        else k4emu::launch_fn(pgrid, dim3(256), [=] { k4::k4_fr_plan_kernel(df.f); }, threads);
        const long long nb = n * rows;
        k4::HashArgs ha{src, f.srcOff, f.hlen, f.got, nb, 0u};
        k4emu::launch_fn(dim3((unsigned)((nb * 4 + k4::XXH_THREADS - 1) / k4::XXH_THREADS)), dim3(k4::XXH_THREADS), [=] { k4::k4_xxh32_kernel(ha); }, threads);
        k4::BatchArgs b1{};
        b1.src = src; b1.srcOff = f.srcOff; b1.srcLen = f.srcLen; b1.dst = dst; b1.dstOff = f.dstOff; b1.dstCap = f.dstCap; b1.outLen = f.outLen; b1.n = nb;
        k4::BatchArgs b2{};
        b2.src = src; b2.srcOff = f.sSrcOff; b2.srcLen = f.sSrcLen; b2.dst = store; b2.dstOff = f.sDstOff; b2.dstCap = f.sDstCap; b2.outLen = f.sOutLen; b2.n = n;
        if (set) {
            b1.dict = dict; b1.dictOff = t.dictOff.data(); b1.dictLen = t.dictLen.data(); b1.dictMode = t.dictMode.data();
            b2.dict = dict; b2.dictOff = t.sDictOff.data(); b2.dictLen = t.sDictLen.data(); b2.dictMode = t.sDictMode.data();
        }
        k4emu::launch_fn(dim3((unsigned)((nb + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG)), dim3(64 * k4::DECODE_WAVES_PER_WG),
                         [=] { k4::k4_decode_kernel(b1); }, threads);
        k4emu::launch_fn(dim3((unsigned)((n + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG)), dim3(64 * k4::DECODE_WAVES_PER_WG),
                         [=] { k4::k4_decode_kernel(b2); }, threads);
        if (fed && set) k4emu::launch_fn(waves, wg, [=] { k4::k4_fr_dict_feed_commit_kernel(dff); }, threads);
        else if (fed) k4emu::launch_fn(waves, wg, [=] { k4::k4_fr_feed_commit_kernel(dff.f); }, threads);
        else if (set) k4emu::launch_fn(waves, wg, [=] { k4::k4_fr_dict_commit_kernel(df); }, threads);
        else k4emu::launch_fn(waves, wg, [=] { k4::k4_fr_commit_kernel(df.f); }, threads);
        for (long long i = 0; plan_out && i < n; i++) plan_out[i] = t.done[(size_t)i] == k4::FR_PLAN_DONE ? 2u : t.plan[(size_t)i].state;
        r.done = t.done.data();
    }
    const k4::FrFeedArgs fa{r, final, consumed, need};
    if (fed && set) k4emu::launch_fn(waves, wg, [=] { k4::k4_fr_dict_feed_kernel(k4::FrDictFeedArgs{fa, d}); }, threads);
    else if (fed) k4emu::launch_fn(waves, wg, [=] { k4::k4_fr_feed_kernel(fa); }, threads);
    else if (set) k4emu::launch_fn(waves, wg, [=] { k4::k4_fr_dict_read_kernel(k4::FrDictReadArgs{r, d}); }, threads);
    else k4emu::launch_fn(waves, wg, [=] { k4::k4_fr_read_kernel(r); }, threads);
}

void k4emu_frd_query(const uint8_t *store, const uint64_t *storeOff, int64_t *out, long long n, int threads)
{
    if (n <= 0) return;
    k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_fr_query_kernel(store, storeOff, out, n); }, threads);
}

/* FrState::dictEntry of every stream: the open frame's entry + 1 */
void k4emu_frd_entries(const uint8_t *store, const uint64_t *storeOff, uint32_t *out, long long n)
{
    for (long long i = 0; i < n; i++) out[i] = ((const k4::FrState *)(store + storeOff[i]))->dictEntry;
}

}  // extern "C"
