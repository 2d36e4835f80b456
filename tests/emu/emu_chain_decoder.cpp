/* tests/emu/emu_chain_decoder.cpp -- many open ILZ4Decoders (k4lz4_chain_decoder.hpp) compiled against the host wave emulator, in a
 * library of its own (tests/chain_decoder_emu.py builds it).  One call of k4emu_cd_run / k4emu_cd_reset / k4emu_cd_drain is what
 * the device forms do for n streams: the same kernels on the caller's arrays.  Test infrastructure only. */
#include "hip/hip_runtime.h"
#include "k4lz4_chain_decoder.hpp"

extern "C" {

long long k4emu_cd_block_size(long long asked) { return k4::cd_block_size(asked); }
long long k4emu_cd_ring_length(long long B, long long extra, int chaining) { return k4::cd_ring_length(B, extra, chaining != 0); }
long long k4emu_cd_store_bytes(long long B, long long extra, int chaining) { return k4::cd_store_bytes(B, extra, chaining != 0); }

void k4emu_cd_reset(const k4::CdRecord *dec, uint8_t *store, const uint64_t *storeOff, int64_t *outLen, long long n, int threads)
{
    if (n <= 0) return;
    k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_cdec_reset_kernel(dec, store, storeOff, outLen, n); }, threads);
}

void k4emu_cd_run(uint8_t *store, const uint64_t *storeOff, const uint8_t *src, const uint64_t *recOff, const uint32_t *recLen,
                  const int32_t *recBlockSize, const uint64_t *firstRec, const uint32_t *nRec, uint8_t *dst, const uint64_t *dstOff,
                  const uint64_t *dstCap, int32_t *recOut, int64_t *outLen, long long n, int flags, int threads)
{
    if (n <= 0) return;
    k4::CdRunArgs a{src, recOff, recLen, recBlockSize, firstRec, nRec, store, storeOff, dst, dstOff, dstCap, recOut, outLen, n, flags, nullptr};
    k4emu::launch_fn(dim3((unsigned)((n + k4::DECODE_PAIRS_PER_WG - 1) / k4::DECODE_PAIRS_PER_WG)), dim3(128 * k4::DECODE_PAIRS_PER_WG),
                     [=] { k4::k4_cdec_run_kernel(a); }, threads);
}

void k4emu_cd_drain(const uint8_t *store, const uint64_t *storeOff, const int64_t *offset, const int64_t *length, uint8_t *dst,
                    const uint64_t *dstOff, int64_t *outLen, long long n, int threads)
{
    if (n <= 0) return;
    k4::CdDrainArgs a{store, storeOff, dst, dstOff, offset, length, outLen, n};
    k4emu::launch_fn(dim3((unsigned)((n + 3) / 4)), dim3(256), [=] { k4::k4_cdec_drain_kernel(a); }, threads);
}

void k4emu_cd_query(const uint8_t *store, const uint64_t *storeOff, int64_t *out, long long n, int threads)
{
    if (n <= 0) return;
    k4emu::launch_fn(dim3((unsigned)((n + 255) / 256)), dim3(256), [=] { k4::k4_cdec_query_kernel(store, storeOff, out, n); }, threads);
}

}  // extern "C"
