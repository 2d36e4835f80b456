/*
 * k4lz4_dict_set.hpp -- the device side of k4lz4_dict_set: dictionaries that stay prepared on the device across calls.
 *
 * The set's memory holds what k4_dict_load_kernel / k4_dict_hc_load_kernel and k4_dict_encode_kernel / k4_dict_hc_encode_kernel take
 * as arguments (kept bytes, per-table and per-entry words, tables); those four kernels run on it as they are.  The one kernel that
 * is new serves k4lz4_decode_dictset_batch_device: the decoders take a dictionary per MESSAGE (BatchArgs::dictOff / dictLen /
 * dictMode), the caller has an index per message into the set, and only the device can look at it.
 *
 * k4_dict_pick_kernel, one thread per message, no loop, no ticket.
 *   phase 0 (before the decode launch): dictOff[i], dictLen[i] from the set's entry dictIdx[i]; dictIdx -1 is "no dictionary"
 *           (dictLen 0).  The mode is always 2 (external): the set's memory is never the bytes in front of a target, whatever the
 *           addresses happen to be.  Any other index outside [0, nDict) raises DEV_STATUS_DICT_INDEX and gives the message a
 *           capacity of 0 in the call's private copy of dstCap, so no decoder writes a byte of its slot.
 *   phase 1 (behind the decode launch): outLen[i] = -1 for those messages, whatever the decoder made of a target of no bytes.
 *
 * Included last by k4lz4_capi.hip: device code that comes in front of other kernels renumbers their registers.
 */
#pragma once
#include "k4lz4_common.hpp"

namespace k4 {

struct DictPickArgs {
    const int32_t *dictIdx;     /* per message: its entry of the set, or -1 */
    const uint64_t *entryOff;   /* per entry: where its kept bytes start in the set's memory */
    const int32_t *entryLen;    /* per entry: how many are kept (at most 65536) */
    const int32_t *dstCap;      /* the caller's */
    uint64_t *dictOff;          /* out, per message */
    int32_t *dictLen;
    signed char *dictMode;
    int32_t *cap;               /* the call's copy of dstCap: 0 where the index is bad */
    int32_t *outLen;            /* phase 1 */
    uint32_t *status;           /* the context's status word, or nullptr */
    long long n;
    int nDict;
    int phase;
};

__global__ __launch_bounds__(256) void k4_dict_pick_kernel(DictPickArgs a)
{
    const long long i = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (i >= a.n) return;
    const int32_t di = a.dictIdx[i];
    const bool bad = di < -1 || di >= a.nDict;
    if (a.phase == 0) {
        const bool has = di >= 0 && !bad;
        a.dictOff[i] = has ? a.entryOff[di] : 0ull;
        a.dictLen[i] = has ? a.entryLen[di] : 0;
        a.dictMode[i] = 2;
        a.cap[i] = bad ? 0 : a.dstCap[i];
        if (bad) dev_status_raise(a.status, DEV_STATUS_DICT_INDEX);
    } else if (bad) {
        a.outLen[i] = -1;
    }
}

} // namespace k4
