/* tests/emu/emu_dict_encode.cpp -- the dictionary encoder's kernels (k4lz4_dict_encode.hpp: load, cost + order, encode) compiled
 * against the host wave emulator, in a library of its own (tests/dict_encode_emu.py builds it).  The list of distinct dictionaries
 * comes from the caller, laid out as k4::DictLoadArgs / k4::DictEncArgs want it.  Test infrastructure only. */
#include "hip/hip_runtime.h"
#include "k4lz4_dict_encode.hpp"
#include <vector>

extern "C" {

int k4emu_dict_encode(const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst, const uint64_t *dstOff,
                      const int32_t *dstCap, int32_t *outLen, long long n, const int32_t *dictIdx, const uint8_t *dict,
                      const uint64_t *keptOff, const uint32_t *keptLen, const uint32_t *table, int nDict, const uint64_t *tOff,
                      const uint32_t *tLen, int nTables, uint32_t *tables, uint32_t *status, int workgroups, int threads)
{
    k4emu::launch_fn(dim3((unsigned)nTables), dim3(k4::DICT_LOAD_THREADS), [=] { k4::k4_dict_load_kernel(k4::DictLoadArgs{dict, tOff, tLen, tables}); }, threads);
    if (n <= 0) return 0;
    std::vector<uint32_t> cost((size_t)n), order((size_t)n, 0xffffffffu), hist(2 * k4::COST_BUCKETS + 1, 0u);
    k4::BatchArgs o{};
    o.srcLen = srcLen; o.n = n; o.cost = cost.data(); o.hist = hist.data(); o.order_out = order.data();
    const unsigned g256 = (unsigned)((n + 255) / 256);
    k4emu::launch_fn(dim3(g256), dim3(256), [=] { k4::k4_dict_cost_kernel(o); }, threads);
    k4emu::launch_fn(dim3(g256), dim3(256), [=] { k4::k4_order_kernel(o, 0xffffffffu); }, threads);
    for (long long i = 0; i < n; i++) if (order[(size_t)i] >= (uint32_t)n) return 1;
    uint32_t ticket = 0;
    k4::DictEncArgs a{src, srcOff, srcLen, dst, dstOff, dstCap, outLen, dictIdx, dict, keptOff, keptLen, table, tables, order.data(), &ticket, status, n, nDict};
    k4emu::launch_fn(dim3((unsigned)workgroups), dim3(64 * k4::FAST_CHAIN_WAVES_PER_WG), [=] { k4::k4_dict_encode_kernel(a); }, threads);
    return 0;
}

}
