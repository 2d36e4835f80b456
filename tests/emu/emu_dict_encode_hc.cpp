/* tests/emu/emu_dict_encode_hc.cpp -- the HC dictionary encoder's kernels (k4lz4_dict_encode_hc.hpp: load, cost + order, encode)
 * compiled against the host wave emulator, in a library of its own (tests/dict_hc_encode_emu.py builds it).  The list of distinct
 * dictionaries comes from the caller, laid out as k4::DictHcLoadArgs / k4::DictHcEncArgs want it.  Test infrastructure only. */
#include "hip/hip_runtime.h"
#include "k4lz4_dict_encode_hc.hpp"
#include <vector>

extern "C" {

int k4emu_dict_hc_table_bytes(void) { return (int)k4::DHC_TABLE_BYTES; }

/* returns 0, 1: the dispatch order is no permutation, 2: a wave slot's heads are not zero after the launch */
int k4emu_dict_hc_encode(const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst, const uint64_t *dstOff,
                         const int32_t *dstCap, int32_t *outLen, long long n, int level, const int32_t *dictIdx, const uint8_t *dict,
                         const uint64_t *keptOff, const uint32_t *keptLen, const uint32_t *table, int nDict, const uint64_t *tOff,
                         const uint32_t *tLen, int nTables, uint8_t *tables, uint32_t *status, int workgroups, int threads)
{
    k4emu::launch_fn(dim3((unsigned)nTables), dim3(k4::DHC_LOAD_THREADS), [=] { k4::k4_dict_hc_load_kernel(k4::DictHcLoadArgs{dict, tOff, tLen, tables}); }, threads);
    if (n <= 0) return 0;
    std::vector<uint32_t> cost((size_t)n), order((size_t)n, 0xffffffffu), hist(2 * k4::COST_BUCKETS + 1, 0u);
    k4::BatchArgs o{};
    o.srcLen = srcLen; o.n = n; o.cost = cost.data(); o.hist = hist.data(); o.order_out = order.data();
    const unsigned g256 = (unsigned)((n + 255) / 256);
    k4emu::launch_fn(dim3(g256), dim3(256), [=] { k4::k4_dict_cost_kernel(o); }, threads);
    k4emu::launch_fn(dim3(g256), dim3(256), [=] { k4::k4_order_kernel(o, 0xffffffffu); }, threads);
    for (long long i = 0; i < n; i++) if (order[(size_t)i] >= (uint32_t)n) return 1;
    uint32_t ticket = 0;
    std::vector<uint8_t> slots((size_t)k4::DHC_TABLE_BYTES * (size_t)workgroups * k4::DHC_WAVES_PER_WG, 0);
    for (size_t s = 0; s < (size_t)workgroups * k4::DHC_WAVES_PER_WG; s++)      /* the chain slots hold anything: they are written before they are read */
        for (size_t k = (size_t)k4::DHC_HEADS * 4; k < k4::DHC_TABLE_BYTES; k++) slots[s * k4::DHC_TABLE_BYTES + k] = 0xA5;
    k4::DictHcEncArgs a{src, srcOff, srcLen, dst, dstOff, dstCap, outLen, dictIdx, dict, keptOff, keptLen, table, tables, slots.data(),
                        order.data(), &ticket, status, n, nDict, level};
    k4emu::launch_fn(dim3((unsigned)workgroups), dim3(64 * k4::DHC_WAVES_PER_WG), [=] { k4::k4_dict_hc_encode_kernel(a); }, threads);
    for (size_t s = 0; s < (size_t)workgroups * k4::DHC_WAVES_PER_WG; s++)
        for (size_t k = 0; k < (size_t)k4::DHC_HEADS * 4; k++) if (slots[s * k4::DHC_TABLE_BYTES + k]) return 2;
    return 0;
}

}
