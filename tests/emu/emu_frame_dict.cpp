/* tests/emu/emu_frame_dict.cpp -- k4lz4_decode_frames_dictset_device's launch sequence (k4lz4_capi.hip decode_frames_run) over the
 * kernels of k4lz4_frame_dict.hpp and k4lz4_frame_read.hpp, compiled against the host wave emulator, in a library of its own
 * (tests/frame_dict_emu.py builds it).  nDict < 0: no set, the plain kernels.  The caller owns every array.  Test infrastructure only. */
#include "hip/hip_runtime.h"
#include "k4lz4_frame_dict.hpp"

#include <algorithm>
#include <vector>

extern "C" {

/* chainWaves: waves of the in-order decoder's grid (a window each); streams beyond them are taken in turns */
int k4emu_frame_dict_decode(const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, long long n, uint8_t *dst,
                            const uint64_t *dstOff, const uint64_t *dstCap, long long *outLen, uint64_t *outSize, int32_t *outStatus,
                            int32_t *outDictIdx, const uint8_t *dict, const uint64_t *entryOff, const int32_t *entryLen, const uint32_t *ids,
                            int nDict, int chainWaves, int threads)
{
    if (n <= 0) return 0;
    const bool set = nDict >= 0;
    const size_t N = (size_t)n;
    std::vector<uint64_t> bound(N), demand(N), clen(N), first(N), produced(N), hashLen(N);
    std::vector<int64_t> res(N), serialOut(N);
    std::vector<uint32_t> nblk(N), desc(N), csum(N), hdrEnd(N), kbad(N), irregular(N), nSerial(N), sum(N);
    std::vector<int32_t> status(N), bsize(N), idx(N, -1);
    std::vector<uint8_t> chained(N);
    k4::FrameTab t{bound.data(), demand.data(), clen.data(), first.data(), produced.data(), hashLen.data(), res.data(), serialOut.data(),
                   nblk.data(), status.data(), desc.data(), bsize.data(), csum.data(), hdrEnd.data(), kbad.data(), irregular.data(),
                   nSerial.data(), sum.data(), chained.data()};
    unsigned long long counters[k4::FRC_DICT_COUNT] = {};
    const unsigned fgrid = (unsigned)((n + 255) / 256);
    k4::FrameWalkArgs w{src, frameOff, frameLen, n, t, counters, outSize, outStatus};
    if (set) {
        k4::FrameWalkIds wd{ids, nDict, idx.data(), outDictIdx, counters + k4::FRC_DICT_CHAINED};
        k4emu::launch_fn(dim3(fgrid), dim3(256), [=] { k4::k4_frame_walk_dict_kernel(w, wd); }, threads);
    } else {
        k4emu::launch_fn(dim3(fgrid), dim3(256), [=] { k4::k4_frame_walk_kernel(w); }, threads);
        if (outDictIdx) std::fill(outDictIdx, outDictIdx + n, -1);
    }
    uint32_t *nblk_p = nblk.data();
    uint64_t *first_p = first.data();
    unsigned long long *cnt = counters;
    k4emu::launch_fn(dim3(1), dim3(k4::FRAME_SCAN_THREADS), [=] { k4::k4_frame_scan_kernel(nblk_p, first_p, n, cnt); }, threads);
    const long long nb = (long long)counters[k4::FRC_BLOCKS];
    const size_t R = (size_t)std::max<long long>(nb, 1);
    std::vector<uint64_t> boff(R), bhlen(R), bdstOff(R), dictOff(R);
    std::vector<uint32_t> blen(R), bowner(R), bidx(R), bsum(R), got(R);
    std::vector<int32_t> bsrcLen(R), bdstCap(R), boutLen(R), dictLen(R);
    std::vector<signed char> dictMode(R);
    k4::BlockTab b{boff.data(), bhlen.data(), bdstOff.data(), blen.data(), bowner.data(), bidx.data(), bsum.data(), got.data(), bsrcLen.data(),
                   bdstCap.data(), boutLen.data()};
    k4::FrameFillArgs fa{src, frameOff, dstOff, dstCap, n, t, b};
    k4emu::launch_fn(dim3(fgrid), dim3(256), [=] { k4::k4_frame_fill_kernel(fa); }, threads);
    if (nb && counters[k4::FRC_BSUM_FRAMES]) {
        k4::HashArgs ha{src, b.off, b.hlen, b.got, nb, 0u};
        k4emu::launch_fn(dim3((unsigned)((nb * 4 + k4::XXH_THREADS - 1) / k4::XXH_THREADS)), dim3(k4::XXH_THREADS), [=] { k4::k4_xxh32_kernel(ha); },
                         threads);
        k4emu::launch_fn(dim3((unsigned)((nb + 255) / 256)), dim3(256), [=] { k4::k4_frame_bsum_kernel(t, b, nb); }, threads);
    }
    if (nb && counters[k4::FRC_INDEP_BLOCKS]) {
        k4::BatchArgs a{};
        a.src = src; a.srcOff = b.off; a.srcLen = b.srcLen; a.dst = dst; a.dstOff = b.dstOff; a.dstCap = b.dstCap; a.outLen = b.outLen; a.n = nb;
        a.accel = 1;
        if (set) {
            k4::FrameDictRowsArgs ra{b.owner, idx.data(), entryOff, entryLen, dictOff.data(), dictLen.data(), dictMode.data(), nb};
            k4emu::launch_fn(dim3((unsigned)((nb + 255) / 256)), dim3(256), [=] { k4::k4_frame_dict_rows_kernel(ra); }, threads);
            a.dict = dict; a.dictOff = dictOff.data(); a.dictLen = dictLen.data(); a.dictMode = dictMode.data();
        }
        k4emu::launch_fn(dim3((unsigned)((nb + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG)), dim3(64 * k4::DECODE_WAVES_PER_WG),
                         [=] { k4::k4_decode_kernel(a); }, threads);
    }
    if (nb) k4emu::launch_fn(dim3((unsigned)((nb + 3) / 4)), dim3(256), [=] { k4::k4_frame_place_kernel(src, dst, t, b, nb); }, threads);
    k4emu::launch_fn(dim3(fgrid), dim3(256), [=] { k4::k4_frame_route_kernel(t, n); }, threads);
    k4::ChainArgs ca{src, b.off, b.len, t.first, t.nSerial, t.bsize, t.chained, dst, dstOff, dstCap, (long long *)t.serialOut, n, nullptr};
    if (set) {
        const long long per = k4::DECODE_WAVES_PER_WG;
        const long long cw = (std::min<long long>(n, std::max(chainWaves, 1)) + per - 1) / per * per;
        /* as decode_frames_run: the frames without an entry to the plain decoder, windows only when a chained frame has an entry */
        std::vector<uint32_t> nPlain(N), nDictSerial(N);
        uint32_t *np = nPlain.data(), *nd = nDictSerial.data();
        const int32_t *ip = idx.data();
        k4emu::launch_fn(dim3(fgrid), dim3(256), [=] { k4::k4_frame_dict_split_kernel(t.nSerial, ip, entryLen, np, nd, n); }, threads);
        k4::ChainArgs cp = ca;
        cp.nBlk = np;
        k4emu::launch_fn(dim3((unsigned)((n + per - 1) / per)), dim3(64 * (unsigned)per), [=] { k4::k4_decode_chain_kernel(cp); }, threads);
        ca.nBlk = nd;
        std::vector<uint8_t> windows(counters[k4::FRC_DICT_CHAINED] ? (size_t)cw * k4::FRAME_DICT_WINDOW : 0, 0xEE);
        k4::ChainDictArgs cd{ca, idx.data(), dict, entryOff, entryLen, windows.data()};
        k4emu::launch_fn(dim3((unsigned)(cw / per)), dim3(64 * (unsigned)per), [=] { k4::k4_decode_chain_dict_kernel(cd); }, threads);
    } else {
        k4emu::launch_fn(dim3((unsigned)((n + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG)), dim3(64 * k4::DECODE_WAVES_PER_WG),
                         [=] { k4::k4_decode_chain_kernel(ca); }, threads);
    }
    k4emu::launch_fn(dim3(fgrid), dim3(256), [=] { k4::k4_frame_settle_kernel(t, dstCap, n); }, threads);
    if (counters[k4::FRC_CSUM_FRAMES]) {
        k4::HashArgs ha{dst, dstOff, t.hashLen, t.sum, n, 0u};
        k4emu::launch_fn(dim3((unsigned)((n * 4 + k4::XXH_THREADS - 1) / k4::XXH_THREADS)), dim3(k4::XXH_THREADS), [=] { k4::k4_xxh32_kernel(ha); },
                         threads);
    }
    const int have = counters[k4::FRC_CSUM_FRAMES] ? 1 : 0;
    int64_t *out = (int64_t *)outLen;
    k4emu::launch_fn(dim3(fgrid), dim3(256), [=] { k4::k4_frame_finish_kernel(t, out, n, have); }, threads);
    return 0;
}

}
