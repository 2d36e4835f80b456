/* tests/emu/emu_fast_chain.cpp -- the chained fast encoder's kernel (k4lz4_fast_chain.hpp) compiled against the host wave
 * emulator, in a library of its own (tests/fast_chain_emu.py builds it).  The block table comes from the caller, laid out as
 * k4::FastChainArgs wants it.  Test infrastructure only. */
#include "hip/hip_runtime.h"
#include "k4lz4_fast_chain.hpp"

extern "C" {

int k4emu_fast_chain(const uint8_t *src, const uint64_t *soff, const uint64_t *slen, const int64_t *first, const uint32_t *nblk,
                     const uint32_t *idx0, const uint32_t *dict_end, const uint32_t *order, const uint32_t *bpos, const int32_t *blen,
                     const uint32_t *bdict, const uint64_t *doff, const int32_t *cap, uint8_t *dst, int32_t *outLen,
                     const void *state_in, void *state_out, long long n, int allow_copy, int workgroups, int threads)
{
    if (n <= 0) return 0;
    uint32_t ticket = 0;
    k4::FastChainArgs a{};
    a.src = src; a.soff = soff; a.slen = slen; a.first = first; a.nblk = nblk; a.idx0 = idx0; a.dict_end = dict_end; a.order = order;
    a.bpos = bpos; a.blen = blen; a.bdict = bdict; a.doff = doff; a.cap = cap; a.dst = dst; a.outLen = outLen;
    a.state_in = (const k4::FastChainState *)state_in; a.state_out = (k4::FastChainState *)state_out;
    a.ticket = &ticket; a.n = n; a.allow_copy = allow_copy;
    k4emu::launch_fn(dim3((unsigned)workgroups), dim3(64 * k4::FAST_CHAIN_WAVES_PER_WG), [=] { k4::k4_fast_chain_kernel(a); }, threads);
    return 0;
}

}
