/* study: DRY parse stats of a sample of every block (host emulator).  form 0: the block's own table (byU16, 13-bit hash), form 1: the
 * sample's table (FastTable<3>, K4_SAMPLE_HASH_BITS: build once per width, -DK4_SAMPLE_HASH_BITS=11 / 12) */
#include "hip/hip_runtime.h"
#include "k4lz4_decode.hpp"
#include "k4lz4_encode_fast.hpp"
#include "k4lz4_parse.hpp"
#include <vector>

namespace k4 {
__global__ void stats_kernel(BatchArgs a, uint32_t off, uint32_t len, uint32_t *out, uint32_t cap = 0, int form = 0)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[PCOST_WAVES_PER_WG][4096 + PARSE_SEEN_DWORDS];
    const int lane = lane_id();
    const uint32_t wave = uni(threadIdx.x >> 6);
    const long long b = (long long)blockIdx.x * PCOST_WAVES_PER_WG + (long long)wave;
    if (b >= a.n) return;
    const uint32_t src_len = (uint32_t)a.srcLen[b];
    uint32_t o = off, s = len;
    if (o + s > src_len) { o = 0; s = s < src_len ? s : src_len; }
    ParseStats st; st.max_rounds = cap;
    uint32_t nseq;
    if (form == 0) nseq = parse_block<1, false, true>(a.src + a.srcOff[b] + o, s, nullptr, (uint16_t *)lds[wave], lds[wave] + 4096, lane, nullptr, &st);
    else nseq = parse_block<1, false, true, 3>(a.src + a.srcOff[b] + o, s, nullptr, (uint16_t *)lds[wave], lds[wave] + 4096, lane, nullptr, &st);
    if (lane == 0) { uint32_t *w = out + 8 * b; w[0] = st.rounds; w[1] = st.slow; w[2] = nseq; w[3] = st.groups; w[4] = st.lazies; w[5] = st.longs; w[6] = st.covered; }
}
}

extern "C" int study_stats(const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, long long n, uint32_t off, uint32_t len, uint32_t *out, int threads, uint32_t cap, int form)
{
    k4::BatchArgs a{};
    a.src = src; a.srcOff = srcOff; a.srcLen = srcLen; a.n = n; a.accel = 1;
    k4emu::launch_fn(dim3((unsigned)((n + k4::PCOST_WAVES_PER_WG - 1) / k4::PCOST_WAVES_PER_WG)), dim3(64 * k4::PCOST_WAVES_PER_WG), [=] { k4::stats_kernel(a, off, len, out, cap, form); }, threads);
    return 0;
}
