/* tests/emu/emu_chain_prime.cpp -- the two open kernels (k4lz4_chain_open.hpp) compiled against the host wave emulator, in a
 * library of its own (tests/chain_prime_emu.py builds it).  One call is what the device forms launch for n streams: the same
 * kernels on the caller's arrays, the set's memory laid out by the caller.  Test infrastructure only. */
#include "hip/hip_runtime.h"
#include "k4lz4_chain_open.hpp"

extern "C" {

int k4emu_open_row_bytes() { return (int)sizeof(k4::CeOpenStream); }

void k4emu_ce_open(const k4::CeOpenStream *rows, uint8_t *store, const uint8_t *set, long long n, int threads)
{
    if (n <= 0) return;
    k4emu::launch_fn(dim3((unsigned)n), dim3(k4::OPEN_WAVE), [=] { k4::k4_ce_open_kernel(rows, store, set, n); }, threads);
}

void k4emu_cd_open(const k4::CdRecord *dec, uint8_t *store, const uint64_t *storeOff, const int32_t *dictIdx, const uint8_t *set,
                   const uint64_t *entryOff, const int32_t *entryLen, int64_t *outLen, uint32_t *status, long long n, int nDict, int threads)
{
    if (n <= 0) return;
    const k4::CdOpenArgs a{dec, store, storeOff, dictIdx, set, entryOff, entryLen, outLen, status, n, nDict};
    k4emu::launch_fn(dim3((unsigned)n), dim3(k4::OPEN_WAVE), [=] { k4::k4_cdec_open_kernel(a); }, threads);
}

}  // extern "C"
