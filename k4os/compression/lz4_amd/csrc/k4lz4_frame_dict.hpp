/*
 * k4lz4_frame_dict.hpp -- frames with a predefined dictionary (FLG bit 0, DictID) read on the device against a
 * k4lz4_dict_set.  The reader of k4lz4_frame_read.hpp with four kernels of its own; scan, fill, block
 * checksums, placement, routing, settle and finish are that reader's, as they are.
 *
 *   k4_frame_walk_dict_kernel    k4_frame_walk_kernel's walk (one body, frame_walk_body<WITH_IDS> in k4lz4_frame_read.hpp), and
 *                                after the header checksum has passed the DictID is looked up in the call's id table (first
 *                                entry whose id equals it).  Per frame: the entry, or -1.  A
 *                                DictID that resolves to nothing is K4LZ4_FRAME_DICTIONARY where the plain walk reports it.
 *   k4_frame_dict_rows_kernel    one thread per block: the owner's entry as the block's external dictionary (BatchArgs::dictOff /
 *                                dictLen / dictMode 2) for the batch decoder -- independent blocks see the dictionary and
 *                                never each other.
 *   k4_frame_dict_split_kernel   one thread per frame: in-order work of frames without an entry (or with an empty one) stays with
 *                                k4_decode_chain*_kernel, that of frames with one goes to k4_decode_chain_dict_kernel.
 *   k4_decode_chain_dict_kernel  k4_decode_chain_kernel with a dictionary per stream: one wave per stream, blocks in order.
 *                                Independent streams (the irregular ones) give every block the dictionary.  A chained stream's
 *                                history is the dictionary's kept bytes followed by the output so far; while that output is
 *                                shorter than 65535 bytes the two are not contiguous, so for a block that starts at
 *                                0 < op < 65535 the wave builds them next to each other in its 64 KiB window (the last
 *                                65536 - op dictionary bytes, then dst[0, op)) and decodes against that as an external
 *                                dictionary; at op == 0 the dictionary itself serves, from op >= 65535 on the output alone
 *                                (the prefix path of k4_decode_chain_kernel).  decode_block is used as it is.
 *                                The grid is bounded (a window per wave): a wave takes streams s, s + waves, ...
 *
 * A window is rebuilt only for blocks that start below 65535 bytes of output: with full 64 KiB blocks, never.
 * Included last by k4lz4_capi.hip: device code that comes in front of other kernels renumbers their registers.
 */
#pragma once
#include "k4lz4_frame_read.hpp"

namespace k4 {

/* one more word behind the reader's counters (FRC_*, zeroed with them): chained frames that resolved to an entry -- only they use
 * the in-order decoder's windows */
constexpr int FRC_DICT_CHAINED = FRC_COUNT, FRC_DICT_COUNT = FRC_COUNT + 1;

__global__ __launch_bounds__(256) void k4_frame_walk_dict_kernel(FrameWalkArgs a, FrameWalkIds d)
{
    frame_walk_body<true>(a, d);
}

struct FrameDictRowsArgs {
    const uint32_t *owner;           /* per block: its frame */
    const int32_t *dictIdx;          /* per frame */
    const uint64_t *entryOff;        /* per entry: where its kept bytes start in the set's memory */
    const int32_t *entryLen;         /* per entry: how many are kept (at most 65536) */
    uint64_t *dictOff;               /* out, per block */
    int32_t *dictLen;
    signed char *dictMode;
    long long nb;
};

__global__ __launch_bounds__(256) void k4_frame_dict_rows_kernel(FrameDictRowsArgs a)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.nb) return;
    const int32_t e = a.dictIdx[a.owner[r]];
    a.dictOff[r] = e >= 0 ? a.entryOff[e] : 0ull;
    a.dictLen[r] = e >= 0 ? a.entryLen[e] : 0;
    a.dictMode[r] = 2;               /* the set's memory is never the bytes in front of a target */
}

/* per frame: the in-order work of a call with a set, dealt to two kernels -- frames that resolved to an entry with bytes go to
 * k4_decode_chain_dict_kernel (nDictSerial), the others stay with k4lz4_decode_chain_batch_device's kernels (nPlainSerial) */
__global__ __launch_bounds__(256) void k4_frame_dict_split_kernel(const uint32_t *nSerial, const int32_t *dictIdx, const int32_t *entryLen,
                                                                  uint32_t *nPlainSerial, uint32_t *nDictSerial, long long n)
{
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    const int32_t e = dictIdx[f];
    const bool with = e >= 0 && entryLen[e] > 0;
    nPlainSerial[f] = with ? 0u : nSerial[f];
    nDictSerial[f] = with ? nSerial[f] : 0u;
}

constexpr uint32_t FRAME_DICT_WINDOW = 65536u;

struct ChainDictArgs {
    ChainArgs c;
    const int32_t *dictIdx;          /* per stream: its entry, -1: none */
    const uint8_t *dict;             /* the set's memory */
    const uint64_t *entryOff;
    const int32_t *entryLen;
    uint8_t *windows;                /* FRAME_DICT_WINDOW bytes per wave of the grid */
};

/* 108 VGPRs, four waves per SIMD: an occupancy hint of six costs 18 spilled VGPRs, and the grid below is one residency at four */
__global__ __launch_bounds__(64 * DECODE_WAVES_PER_WG) void k4_decode_chain_dict_kernel(ChainDictArgs d)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[DECODE_WAVES_PER_WG][DECODE_LDS_DWORDS];
    const ChainArgs &a = d.c;
    const int lane = lane_id();
    const int wave = (int)uni(threadIdx.x >> 6);
    const long long slot = (long long)blockIdx.x * DECODE_WAVES_PER_WG + wave;
    const long long waves = (long long)gridDim.x * DECODE_WAVES_PER_WG;
    uint8_t *const win = d.windows + (uint64_t)slot * FRAME_DICT_WINDOW;
    for (long long s = slot; s < a.n; s += waves) {
        uint8_t *out = a.dst + a.dstOff[s];
        const uint64_t cap = a.dstCap[s];
        const uint64_t first = a.firstBlk[s];
        const uint32_t count = a.nBlk[s];
        if (!count) continue;                                        /* not this kernel's frame: its outLen is not touched */
        const int block_size = a.blockSize[s];
        const bool chained = a.chained[s] != 0;
        const int32_t e = d.dictIdx[s];
        const uint32_t dlen = e >= 0 ? (uint32_t)d.entryLen[e] : 0u;
        const uint8_t *dend = e >= 0 ? d.dict + d.entryOff[e] + dlen : nullptr;
        uint64_t op = 0;
        long long result = 0;
        for (uint32_t k = 0; k < count; k++) {
            const uint32_t lc = a.blkLen[first + k];
            const uint32_t n = lc & 0x7fffffffu;
            const uint8_t *in = a.src + a.blkOff[first + k];
            const uint64_t room = cap - op;
            if (lc & 0x80000000u) {                                  /* LZ4BlockDecoder.Inject */
                if (n > room) { result = -9; break; }
                wave_sync();
                wave_copy(out + op, in, n, lane);
                op += n;
            } else {
                const int want = (int)(room < (uint64_t)block_size ? room : (uint64_t)block_size);
                DecodeDict dict{nullptr, 0u, 0};
                wave_sync();                                         /* the previous block's stores -> this block's loads */
                if (dlen != 0u && (!chained || op == 0)) {
                    dict.end = dend; dict.size = dlen; dict.mode = 2;
                } else if (chained && op > 0) {
                    if (dlen == 0u || op >= 65535u) {
                        dict.end = out + op;
                        dict.size = op >= 65535u ? 65536u : (uint32_t)op;
                        dict.mode = 1;
                    } else {                                         /* both at once: side by side in the window */
                        const uint32_t have = (uint32_t)op;
                        const uint32_t keep = dlen < FRAME_DICT_WINDOW - have ? dlen : FRAME_DICT_WINDOW - have;
                        wave_copy(win, dend - keep, keep, lane);
                        wave_copy(win + keep, out, have, lane);
                        wave_sync();
                        dict.end = win + keep + have; dict.size = keep + have; dict.mode = 2;
                    }
                }
                const int got = decode_block(in, (int)n, out + op, want, lane, lds[wave], nullptr, false, dict);
                if (got < 0) { result = room < (uint64_t)block_size ? -9 : -6; break; }
                op += (uint64_t)got;
            }
        }
        if (lane == 0) a.outLen[s] = result < 0 ? result : (long long)op;
        wave_sync();                                                 /* the window's readers are done before the next stream's */
    }
}

}  // namespace k4
