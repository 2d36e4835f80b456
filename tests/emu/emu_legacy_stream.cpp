/* tests/emu/emu_legacy_stream.cpp -- LZ4Stream piece by piece (k4lz4_legacy_stream.hpp) compiled against the host wave emulator, in
 * a library of its own (tests/legacy_stream_emu.py builds it).  One call of k4emu_ls_write / k4emu_ls_read is what the device
 * forms do for n streams: the same host plan and the same kernels on the caller's arrays.  Test infrastructure only. */
#include "hip/hip_runtime.h"

/* (the emulator has the 32-bit form only; k4_lr_copy_kernel is compiled here but not run) */
static inline unsigned long long atomicMin(unsigned long long *p, unsigned long long v)
{
    unsigned long long cur = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return cur;
}

#include "k4lz4_encode_fast.hpp"
#include "k4lz4_legacy_stream.hpp"

#include <string.h>
#include <vector>

extern "C" {

int k4emu_ls_writer_init(k4lz4_legacy_writer *w, int blockSize, int high)
{
    w->blockSize = blockSize < 16 ? 16 : blockSize; w->high = high ? 1 : 0; w->pending = 0; w->closed = 0;
    return 0;
}
long long k4emu_ls_writer_store_bytes(const k4lz4_legacy_writer *w) { return k4::ls_w_store_bytes(*w); }
long long k4emu_ls_write_bound(const k4lz4_legacy_writer *w, long long srcLen, int op) { return k4::ls_w_bound(*w, srcLen, op); }

/* k4lz4_legacy_write_batch_device for fast streams (the HC rows' encoder is not part of this library) */
void k4emu_ls_write(k4lz4_legacy_writer *w, uint8_t *store, const uint64_t *storeOff, const uint8_t *src, const uint64_t *srcOff,
                    const int64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen, long long n, int op,
                    int threads)
{
    if (n <= 0) return;
    std::vector<int32_t> code;
    k4::LsWLayout L;
    k4::ls_w_layout(w, srcLen, dstCap, n, op, code, L);
    std::vector<uint8_t> hv(L.plan_bytes + 64, 0), dv(L.total + 64, 0);
    uint8_t *h = hv.data(), *d = dv.data();
    k4::ls_w_fill(w, store, storeOff, src, srcOff, srcLen, dstOff, n, op, code, L, h, d);
    memcpy(d, h, L.plan_bytes);
    k4::LsWriteArgs a{};
    a.streams = (const k4::LsWStream *)(d + L.o_streams); a.n = n; a.rows = L.rows;
    a.cSrc = (const uint64_t *)(d + L.o_src); a.cEnc = (const uint64_t *)(d + L.o_enc); a.cLen = (const int32_t *)(d + L.o_len);
    a.owner = (const uint32_t *)(d + L.o_owner);
    a.cEncLen = (int32_t *)(d + L.o_elen); a.recLen = (uint64_t *)(d + L.o_rlen); a.recOff = (uint64_t *)(d + L.o_roff);
    const k4::FwPiece *stage = (const k4::FwPiece *)(d + L.o_stage), *tail = (const k4::FwPiece *)(d + L.o_tail);
    const long long nstage = L.nstage, ntail = L.ntail, rows = L.rows;
    if (nstage) k4emu::launch_fn(dim3((unsigned)L.stage_chunks), dim3(k4::FW_THREADS), [=] { k4::k4_fw_copy_kernel(stage, nstage); }, threads);
    if (rows) {
        k4::BatchArgs b{};
        b.src = nullptr; b.srcOff = a.cSrc; b.srcLen = a.cLen; b.dst = nullptr; b.dstOff = a.cEnc; b.dstCap = (const int32_t *)(d + L.o_cap);
        b.outLen = a.cEncLen; b.n = rows; b.level = 0; b.accel = 1; b.flags = k4::FLAG_RAW_RETURN;
        k4emu::launch_fn(dim3((unsigned)((rows + k4::ENCODE_WAVES_PER_WG - 1) / k4::ENCODE_WAVES_PER_WG)), dim3(64 * k4::ENCODE_WAVES_PER_WG),
                         [=] { k4::k4_encode_fast_kernel(b); }, threads);
        unsigned long long *cnt = (unsigned long long *)(d + L.o_cnt);
        k4emu::launch_fn(dim3((unsigned)((rows + 255) / 256)), dim3(256), [=] { k4::k4_ls_reclen_kernel(a); }, threads);
        k4emu::launch_fn(dim3(1), dim3(k4::LEGACY_SCAN_THREADS), [=] { k4::k4_legacy_scan_kernel(a.recLen, a.recOff, rows, cnt); }, threads);
        k4emu::launch_fn(dim3((unsigned)((rows + 3) / 4)), dim3(256), [=] { k4::k4_ls_assemble_kernel(a, dst); }, threads);
    }
    if (ntail) k4emu::launch_fn(dim3((unsigned)L.tail_chunks), dim3(k4::FW_THREADS), [=] { k4::k4_fw_copy_kernel(tail, ntail); }, threads);
    k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_ls_finish_kernel(a, outLen); }, threads);
    for (long long i = 0; i < n; i++)
        if (code[(size_t)i] == 0) k4::ls_w_advance(w[i], srcLen[i], op);
}

long long k4emu_ls_reader_store_bytes(long long maxBlock) { return k4::ls_rd_store_bytes(maxBlock); }

/* k4lz4_legacy_read_batch_device; plan_out (n words, may be NULL): 0 not planned, 1 planned and handed back, 2 served directly */
void k4emu_ls_read(long long maxBlock, uint8_t *store, const uint64_t *storeOff, const uint8_t *src, const uint64_t *srcOff,
                   const uint64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const int64_t *count, int64_t *outLen, long long n, int op,
                   int interactive, long long maxCount, uint32_t *plan_out, int threads)
{
    if (n <= 0) return;
    k4::LsReadArgs a{src, srcOff, srcLen, store, storeOff, dst, dstOff, count, outLen, n, op, interactive, (int32_t)maxBlock, nullptr};
    const dim3 waves((unsigned)((n + k4::LS_WAVES_PER_WG - 1) / k4::LS_WAVES_PER_WG)), wg(64 * k4::LS_WAVES_PER_WG);
    const long long rows = k4::ls_table_rows(maxCount, maxBlock);
    std::vector<uint32_t> done((size_t)n, 0);
    for (long long i = 0; plan_out && i < n; i++) plan_out[i] = 0u;
    if (op == k4::LS_OP_READ && !interactive && rows > 0) {
        const size_t nr = (size_t)(n * rows) + 1;
        std::vector<k4::LsPlan> plan((size_t)n);
        std::vector<uint64_t> so(nr), dof(nr), sso((size_t)n), sdo((size_t)n);
        std::vector<int32_t> sl(nr), dc(nr), ol(nr), ssl((size_t)n), sdc((size_t)n), sol((size_t)n);
        std::vector<uint32_t> raw(nr);
        k4::LsDirectArgs f{};
        f.r = a; f.rows = rows; f.plan = plan.data(); f.done = done.data();
        f.srcOff = so.data(); f.dstOff = dof.data(); f.srcLen = sl.data(); f.dstCap = dc.data(); f.outLen = ol.data(); f.rawLen = raw.data();
        f.sSrcOff = sso.data(); f.sDstOff = sdo.data(); f.sSrcLen = ssl.data(); f.sDstCap = sdc.data(); f.sOutLen = sol.data();
        k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_ls_plan_kernel(f); }, threads);
        const long long nb = n * rows;
        k4::BatchArgs b1{};
        b1.src = src; b1.srcOff = f.srcOff; b1.srcLen = f.srcLen; b1.dst = dst; b1.dstOff = f.dstOff; b1.dstCap = f.dstCap; b1.outLen = f.outLen; b1.n = nb;
        k4emu::launch_fn(dim3((unsigned)((nb + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG)), dim3(64 * k4::DECODE_WAVES_PER_WG),
                         [=] { k4::k4_decode_kernel(b1); }, threads);
        k4::BatchArgs b2{};
        b2.src = src; b2.srcOff = f.sSrcOff; b2.srcLen = f.sSrcLen; b2.dst = store; b2.dstOff = f.sDstOff; b2.dstCap = f.sDstCap; b2.outLen = f.sOutLen; b2.n = n;
        k4emu::launch_fn(dim3((unsigned)((n + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG)), dim3(64 * k4::DECODE_WAVES_PER_WG),
                         [=] { k4::k4_decode_kernel(b2); }, threads);
        k4emu::launch_fn(waves, wg, [=] { k4::k4_ls_commit_kernel(f); }, threads);
        for (long long i = 0; plan_out && i < n; i++) plan_out[i] = done[(size_t)i] == k4::LS_PLAN_DONE ? 2u : plan[(size_t)i].state;
        a.done = done.data();
    }
    k4emu::launch_fn(waves, wg, [=] { k4::k4_ls_read_kernel(a); }, threads);
}

void k4emu_ls_query(const uint8_t *store, const uint64_t *storeOff, int64_t *out, long long n, int threads)
{
    if (n <= 0) return;
    k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_ls_query_kernel(store, storeOff, out, n); }, threads);
}

}  // extern "C"
