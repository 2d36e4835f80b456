/*
 * k4lz4_chain_open.hpp -- open chained encoders and decoders from a prepared dictionary set (k4lz4_chain_encoder_open_dictset,
 * k4lz4_chain_decoder_open_dictset).
 *
 * "Open" makes fresh streams, as RESET does, and primes those that name an entry of a k4lz4_dict_set: one launch per side.
 *
 *   k4_ce_open_kernel     one wavefront per stream, laid out by the host (every length is known there).  The entry's kept bytes go to
 *                         ring positions [0, d): the dictionary is the stream's PREFIX -- the first block follows it in the ring, as
 *                         after LZ4_loadDict / LZ4_loadDictHC on the ring.  A chained fast stream's k4lz4_fast_chain_state in the store
 *                         becomes the set's table for the entry (LZ4_loadDict's, 4096 words) with currentOffset 65536 and dictSize d;
 *                         without an entry, or with one that keeps fewer than 8 bytes, the zeroed table.  The HC tables are a
 *                         function of the ring's bytes (4.9) and need nothing.
 *   k4_cdec_open_kernel   one wavefront per stream; the records and indices are on the device, as k4lz4_chain_decode_batch_device has
 *                         them.  What k4_cdec_reset_kernel writes, then the effect of one Inject(kept bytes) on that fresh decoder
 *                         (LZ4ChainDecoder.cs:64-93 path 1: the bytes at the ring's start; LZ4BlockDecoder.cs:58-71, which refuses
 *                         more than B + 8 bytes with K4LZ4_CDEC_INJECT).  An index outside [-1, nDict) leaves the store untouched,
 *                         reports K4LZ4_CDEC_DICT_INDEX and raises DEV_STATUS_DICT_INDEX.
 *
 * Neither kernel has a ticket, and every loop has one back edge; the grid is the stream count.  The set's regions and the stores
 * are 64- and 256-byte aligned, the copies write exact lengths.
 *
 * Included last by k4lz4_capi.hip: device code that comes in front of other kernels renumbers their registers.
 */
#pragma once
#include "../../../../include/k4lz4.h"
#include "k4lz4_common.hpp"
#include "k4lz4_chain_decoder.hpp"

namespace k4 {

constexpr int CD_DICT_INDEX = -8;                /* include/k4lz4.h K4LZ4_CDEC_DICT_INDEX */
constexpr uint32_t OPEN_CURRENT_OFFSET = 65536u; /* LZ4_loadDict: LZ4_resetStream, then currentOffset += 64 KB, whatever the length */
constexpr uint32_t OPEN_FAST_WORDS = 4096u;      /* k4lz4_fast_chain_state::hashTable */
constexpr int OPEN_WAVE = 64;

/* one stream of k4lz4_chain_encoder_open_dictset, as the host lays it out */
struct CeOpenStream {
    unsigned long long ring;         /* where ring position 0 is in the store */
    unsigned long long state;        /* where the k4lz4_fast_chain_state is in the store (fast != 0) */
    unsigned long long kept;         /* the entry's kept bytes in the set's memory */
    unsigned long long table;        /* the entry's table of the fast family in the set's memory (fast == 1) */
    uint32_t keptLen;                /* bytes that go to the ring, 0: none */
    uint32_t fast;                   /* 0: no state in the store; 1: the set's table; 2: the zeroed table */
    uint32_t currentOffset, dictSize;
};

__global__ __launch_bounds__(OPEN_WAVE) void k4_ce_open_kernel(const CeOpenStream *streams, uint8_t *store, const uint8_t *set, long long n)
{
    const long long s = blockIdx.x;
    if (s >= n) return;
    const int lane = (int)threadIdx.x;
    const CeOpenStream r = streams[s];
    if (r.keptLen) wave_copy(store + r.ring, set + r.kept, r.keptLen, lane);
    if (r.fast == 0) return;
    uint8_t *st = store + r.state;
    const U128u zero = {{0u, 0u, 0u, 0u}};
    const bool load = r.fast == 1;
    const uint8_t *tab = load ? set + r.table : st;      /* (never read without `load`) */
    for (uint32_t k = (uint32_t)lane; k < OPEN_FAST_WORDS / 4u; k += (uint32_t)OPEN_WAVE)
        st128u(st + 16ull * k, load ? ld128u(tab + 16ull * k) : zero);
    if (lane == 0) {                                     /* currentOffset, dictSize, reserved[2] */
        const U128u tail = {{r.currentOffset, r.dictSize, 0u, 0u}};
        st128u(st + 4ull * OPEN_FAST_WORDS, tail);
    }
}

struct CdOpenArgs {
    const CdRecord *dec;             /* per stream, as RESET takes them */
    uint8_t *store;
    const uint64_t *storeOff;
    const int32_t *dictIdx;          /* per stream: its entry of the set, or -1 */
    const uint8_t *set;              /* the set's memory */
    const uint64_t *entryOff;        /* per entry: where its kept bytes start in it */
    const int32_t *entryLen;         /* per entry: how many are kept (at most 65536) */
    int64_t *outLen;                 /* per stream: the bytes injected, or a code */
    uint32_t *status;                /* the context's status word, or nullptr */
    long long n;
    int nDict;
};

__global__ __launch_bounds__(OPEN_WAVE) void k4_cdec_open_kernel(CdOpenArgs a)
{
    const long long s = blockIdx.x;
    if (s >= a.n) return;
    const int lane = (int)threadIdx.x;
    const int32_t di = a.dictIdx[s];
    if (di < -1 || di >= a.nDict) {                      /* nothing of the store is touched */
        if (lane == 0) {
            a.outLen[s] = CD_DICT_INDEX;
            dev_status_raise(a.status, DEV_STATUS_DICT_INDEX);
        }
        return;
    }
    const CdRecord r = a.dec[s];
    const int32_t B = (int32_t)cd_block_size(r.blockSize);
    const int32_t chaining = r.chaining ? 1 : 0;
    const int32_t extra = chaining ? (r.extraBlocks < 0 ? 0 : r.extraBlocks) : 0;
    const uint32_t ring_len = (uint32_t)cd_ring_length(B, extra, chaining != 0);
    /* Inject on the fresh decoder: a chained one takes up to max(B, 64 KiB) and the kept bytes are at most 64 KiB, below the ring's
       length, so they land at its start; an independent one takes up to its ring's length */
    const uint32_t len = di >= 0 ? (uint32_t)a.entryLen[di] : 0u;
    const bool refused = di >= 0 && !chaining && len > ring_len;
    const uint32_t index = refused ? 0u : len;
    const uint32_t records = di >= 0 && !refused ? 1u : 0u;
    uint8_t *base = a.store + a.storeOff[s];
    /* CdState, one word per lane: magic, blockSize, extraBlocks, chaining, index, lastCode, records, bytes, moves (64-bit each) */
    static_assert(CD_STATE_BYTES == 4 * OPEN_WAVE, "one word of CdState per lane");
    const uint32_t w = lane == 0 ? CD_MAGIC : lane == 1 ? (uint32_t)B : lane == 2 ? (uint32_t)extra : lane == 3 ? (uint32_t)chaining :
                       lane == 4 ? index : lane == 5 ? (refused ? (uint32_t)CD_INJECT : 0u) : lane == 6 ? records : lane == 8 ? index : 0u;
    ((uint32_t *)base)[lane] = w;
    if (index) wave_copy(base + CD_STATE_BYTES, a.set + a.entryOff[di], index, lane);
    if (lane == 0) a.outLen[s] = refused ? (int64_t)CD_INJECT : (int64_t)index;
}

static_assert(sizeof(k4lz4_fast_chain_state) == 4 * OPEN_FAST_WORDS + 16, "the state is the table and four words");

}  // namespace k4
