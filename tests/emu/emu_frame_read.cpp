/* tests/emu/emu_frame_read.cpp -- the frame reader's walk, scan and fill kernels (k4lz4_frame_read.hpp) compiled against the host
 * wave emulator, in a library of its own (tests/frame_read_emu.py builds it).  The caller owns every array; the block table is
 * sized by the caller (maxBlocks rows).  Test infrastructure only. */
#include "hip/hip_runtime.h"
#include "k4lz4_frame_read.hpp"

#include <vector>

extern "C" {

/* frame arrays: bound, clen, first (u64); nblk, status, desc, bsize, csum, hdrEnd (32-bit); block arrays: off, hlen, dstOff (u64),
 * len, owner, idx, sum (u32), srcLen, dstCap (i32); counters: FRC_COUNT words.  Returns the number of blocks, or -1 when they do
 * not fit maxBlocks. */
long long k4emu_frame_read(const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, long long n, const uint64_t *dstOff,
                           const uint64_t *dstCap, uint64_t *bound, uint64_t *clen, uint64_t *first, uint32_t *nblk, int32_t *status,
                           uint32_t *desc, int32_t *bsize, uint32_t *csum, uint32_t *hdrEnd, uint64_t *boff, uint64_t *bhlen,
                           uint64_t *bdstOff, uint32_t *blen, uint32_t *bowner, uint32_t *bidx, uint32_t *bsum, int32_t *bsrcLen,
                           int32_t *bdstCap, long long maxBlocks, unsigned long long *counters, uint64_t *outSize, int32_t *outStatus,
                           int threads)
{
    if (n <= 0) return 0;
    std::vector<uint64_t> demand(n), produced(n), hashLen(n);
    std::vector<int64_t> res(n), serialOut(n);
    std::vector<uint32_t> kbad(n), irregular(n), nSerial(n), sum(n);
    std::vector<uint8_t> chained(n);
    k4::FrameTab t{bound, demand.data(), clen, first, produced.data(), hashLen.data(), res.data(), serialOut.data(), nblk, status, desc, bsize, csum,
                   hdrEnd, kbad.data(), irregular.data(), nSerial.data(), sum.data(), chained.data()};
    for (int i = 0; i < k4::FRC_COUNT; i++) counters[i] = 0;
    const unsigned grid = (unsigned)((n + 255) / 256);
    k4::FrameWalkArgs w{src, frameOff, frameLen, n, t, counters, outSize, outStatus};
    k4emu::launch_fn(dim3(grid), dim3(256), [=] { k4::k4_frame_walk_kernel(w); }, threads);
    k4emu::launch_fn(dim3(1), dim3(k4::FRAME_SCAN_THREADS), [=] { k4::k4_frame_scan_kernel(nblk, first, n, counters); }, threads);
    const long long nb = (long long)counters[k4::FRC_BLOCKS];
    if (nb > maxBlocks) return -1;
    std::vector<uint32_t> got(nb > 0 ? nb : 1);
    std::vector<int32_t> outLen(nb > 0 ? nb : 1);
    k4::BlockTab b{boff, bhlen, bdstOff, blen, bowner, bidx, bsum, got.data(), bsrcLen, bdstCap, outLen.data()};
    k4::FrameFillArgs fa{src, frameOff, dstOff, dstCap, n, t, b};
    k4emu::launch_fn(dim3(grid), dim3(256), [=] { k4::k4_frame_fill_kernel(fa); }, threads);
    return nb;
}

}
