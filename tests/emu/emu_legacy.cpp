/* tests/emu/emu_legacy.cpp -- the legacy stream kernels (k4lz4_legacy.hpp) compiled against the host wave emulator, in a library
 * of its own (tests/legacy_emu.py builds it): the reader's walk, scan and fill, the writer's count, scan, fill and record sizes,
 * and Unwrap's sizes.  The caller owns every array.  Test infrastructure only. */
#include "hip/hip_runtime.h"

/* (the emulator has the 32-bit form only; k4_lr_copy_kernel is compiled here but not run) */
static inline unsigned long long atomicMin(unsigned long long *p, unsigned long long v)
{
    unsigned long long cur = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return cur;
}

#include "k4lz4_legacy.hpp"

#include <vector>

extern "C" {

/* reader: per stream nch, bound, status, first (rows are sized by maxRows); per row off, dstOff, owner, idx, srcLen, dstCap, len,
 * kind.  Returns the number of rows, or -1 when they do not fit maxRows. */
long long k4emu_legacy_read(const uint8_t *src, const uint64_t *off, const uint64_t *len, long long n, const uint64_t *dstOff,
                            const uint64_t *dstCap, uint64_t *nch, uint64_t *bound, int32_t *status, uint64_t *first, uint64_t *outSize,
                            int32_t *outStatus, uint64_t *roff, uint64_t *rdst, uint32_t *rowner, uint32_t *ridx, int32_t *rsrcLen,
                            int32_t *rdstCap, int32_t *rlen, uint8_t *rkind, long long maxRows, int threads)
{
    if (n <= 0) return 0;
    std::vector<unsigned long long> key(n), cnt(8, 0);
    k4::LegacyReadArgs a{src, off, len, n, nch, bound, status, first, key.data(), outSize, outStatus};
    const unsigned grid = (unsigned)((n + 255) / 256);
    unsigned long long *c = cnt.data();
    k4emu::launch_fn(dim3(grid), dim3(256), [=] { k4::k4_lr_walk_kernel(a); }, threads);
    k4emu::launch_fn(dim3(1), dim3(k4::LEGACY_SCAN_THREADS), [=] { k4::k4_legacy_scan_kernel(nch, first, n, c); }, threads);
    const long long rows = (long long)cnt[0];
    if (rows > maxRows) return -1;
    std::vector<int32_t> outLen(rows > 0 ? rows : 1);
    k4::LegacyRows rw{roff, rdst, rowner, ridx, rsrcLen, rdstCap, rlen, outLen.data(), rkind};
    k4emu::launch_fn(dim3(grid), dim3(256), [=] { k4::k4_lr_fill_kernel(a, rw, dstOff, dstCap); }, threads);
    return rows;
}

/* writer, up to the record sizes: per stream nch, first, arenaOff; per row srcOff, srcLen, encOff, encCap, owner; then, with the
 * caller's encoder results encLen (nullptr: stop after the fill), recLen and recOff.  Returns the number of rows, -1 when they do
 * not fit maxRows. */
long long k4emu_legacy_write(const uint64_t *srcOff, const uint64_t *srcLen, long long n, int blockSize, uint64_t *nch, uint64_t *first,
                             uint64_t *arenaOff, uint64_t *cSrcOff, int32_t *cSrcLen, uint64_t *cEncOff, int32_t *cEncCap, uint32_t *owner,
                             int32_t *cEncLen, uint64_t *recLen, uint64_t *recOff, long long maxRows, unsigned long long *arenaBytes,
                             int threads)
{
    if (n <= 0) return 0;
    std::vector<uint64_t> pad(n);
    std::vector<unsigned long long> cnt(8, 0);
    k4::LegacyWriteArgs a{};
    a.srcOff = srcOff; a.srcLen = srcLen; a.n = n; a.bs = (uint64_t)(blockSize < 16 ? 16 : blockSize);
    a.nch = nch; a.pad = pad.data(); a.first = first; a.arenaOff = arenaOff;
    const unsigned grid = (unsigned)((n + 255) / 256);
    unsigned long long *c = cnt.data();
    const uint64_t *pp = pad.data();
    k4emu::launch_fn(dim3(grid), dim3(256), [=] { k4::k4_lw_count_kernel(a); }, threads);
    k4emu::launch_fn(dim3(1), dim3(k4::LEGACY_SCAN_THREADS), [=] { k4::k4_legacy_scan_kernel(nch, first, n, c); }, threads);
    k4emu::launch_fn(dim3(1), dim3(k4::LEGACY_SCAN_THREADS), [=] { k4::k4_legacy_scan_kernel(pp, arenaOff, n, c + 1); }, threads);
    const long long rows = (long long)cnt[0];
    *arenaBytes = cnt[1];
    if (rows > maxRows) return -1;
    a.rows = rows;
    a.owner = owner; a.cSrcOff = cSrcOff; a.cSrcLen = cSrcLen; a.cEncOff = cEncOff; a.cEncCap = cEncCap;
    a.cEncLen = cEncLen; a.recLen = recLen; a.recOff = recOff;
    if (rows <= 0) return 0;
    const unsigned rgrid = (unsigned)((rows + 255) / 256);
    k4emu::launch_fn(dim3(rgrid), dim3(256), [=] { k4::k4_lw_fill_kernel(a); }, threads);
    if (!cEncLen) return rows;
    k4emu::launch_fn(dim3(rgrid), dim3(256), [=] { k4::k4_lw_header_kernel(a); }, threads);
    k4emu::launch_fn(dim3(1), dim3(k4::LEGACY_SCAN_THREADS), [=] { k4::k4_legacy_scan_kernel(recLen, recOff, rows, c + 2); }, threads);
    return rows;
}

/* Unwrap's sizes: outLen per buffer, and the route (decOff, decLen, decCap) */
void k4emu_unwrap_sizes(const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, const int32_t *dstCap, long long n,
                        int32_t *outLen, uint64_t *decOff, int32_t *decLen, int32_t *decCap, int threads)
{
    if (n <= 0) return;
    k4::UnwrapArgs u{src, srcOff, srcLen, dstCap, n, outLen, decOff, decLen, decCap};
    k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_unwrap_sizes_kernel(u); }, threads);
}

}
