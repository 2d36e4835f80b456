/*
 * k4lz4_chain_decoder.hpp -- many open ILZ4Decoders advanced per call (k4lz4_chain_decode_batch).
 *
 * A stream is one decoder as LZ4Decoder.Create(chaining, blockSize, extraBlocks) makes it (Encoders/LZ4Decoder.cs): an
 * LZ4ChainDecoder (Encoders/LZ4ChainDecoder.cs) or, without chaining, an LZ4BlockDecoder (Encoders/LZ4BlockDecoder.cs).  A call
 * applies a run of Decode(source, length, blockSize) / Inject(source, length) records to each of them in order, optionally drained
 * the way DecodeAndDrain drains (Encoders/LZ4EncoderExtensions.cs:305-323).  Everything a decoder keeps lives in its DEVICE store:
 *
 *   CdState (CD_STATE_BYTES)   the settings as rounded (written by RESET), _outputIndex, counters, the last run's code
 *   ring                       _outputBuffer, with the reference's length: 65536 + (1 + extraBlocks) * B + 32 for a chained
 *                              decoder (LZ4ChainDecoder.cs:32), B + 8 for an independent one (LZ4BlockDecoder.cs:27).  BytesReady
 *                              and how far back Drain reaches are observable, so the geometry is the reference's exactly:
 *                              Prepare / CopyDict (:117-132) move the last min(index, 64 KiB) bytes to the front when
 *                              index + blockSize passes the end, Inject (:64-93) takes its three paths.
 *
 * LZ4_streamDecode_t needs no words of its own: after every operation prefixEnd is the ring's index and prefixSize is
 * min(index, 64 KiB) or more (LL.LZ4_setStreamDecode in CopyDict / ApplyDict, += result in LZ4_decompress_safe_continue,
 * LL64.dec.cs:558-608), so the next block's prefix is the ring's bytes before the index, the last 64 KiB of them: DecodeDict
 * mode 1 at the index.  The external-dictionary and double-dictionary arms are never reached.
 *
 *   k4_cdec_run_kernel     two wavefronts per stream (as k4_decode_chain_pair_kernel): one parses the records' blocks
 *                          (decode_block<false, 1>), and may run blocks ahead -- it reads the sources only, and the decoded size it
 *                          needs it computes itself; the other (decode_block<false, 2>) moves the ring, copies literals and matches,
 *                          copies Inject's bytes, drains, and writes the results and the state.  Both make the same decisions --
 *                          Prepare, Inject's path, every code -- from the same numbers.
 *   k4_cdec_reset_kernel   a store becomes a fresh decoder with the settings of its record
 *   k4_cdec_drain_kernel   Drain(target, offset, length) (LZ4ChainDecoder.cs:96-103): one wave per stream, the store is not changed
 *   k4_cdec_query_kernel   one thread per stream
 *
 * The moves inside the ring overlap whenever the index is between 64 KiB and 128 KiB: wave_shift_down moves downwards in ascending
 * 1 KiB steps, each loaded by every lane before any lane stores, which is safe for any distance; a wave_sync stands between a
 * move and whatever reads or writes the ring next.
 *
 * A decoder that reported a code is not failed (the reference's is not): the state is what the reference's object holds after
 * the exception -- Prepare's move applied, the failing block not counted -- and the next call continues from there.  Nothing
 * outside [dstOff[s], dstOff[s] + dstCap[s]) and the stream's own store is written.
 */
#pragma once
#include "k4lz4_decode.hpp"

namespace k4 {

/* include/k4lz4.h K4LZ4_CDEC_* */
constexpr int CD_DECODE = -1, CD_INJECT = -2, CD_BLOCK_SIZE = -3, CD_TARGET = -4, CD_NOT_RUN = -5, CD_RANGE = -6, CD_NO_DECODER = -7;
constexpr int CD_OP_RUN = 0, CD_OP_RESET = 1;
constexpr int CD_FLAG_DRAIN = 1;
constexpr int64_t CD_STATE_BYTES = 256;
constexpr uint32_t CD_HISTORY = 65536;
constexpr uint32_t CD_MAGIC = 0x4443344bu;       /* "K4CD" */
constexpr int32_t CD_MAX_RING = 0x7E000000;

/* the host record's words (k4lz4_chain_decoder), as the kernels read them */
struct CdRecord {
    int32_t blockSize, extraBlocks, chaining, reserved;
    int64_t storeBytes;
};

struct CdState {
    uint32_t magic;
    int32_t blockSize, extraBlocks, chaining;    /* as rounded */
    uint32_t index;                              /* _outputIndex: BytesReady */
    int32_t lastCode;                            /* the last run's code, 0 when it reported none */
    unsigned long long records;                  /* records applied */
    unsigned long long bytes;                    /* bytes they produced */
    unsigned long long moves;                    /* moves inside the ring (a statistic) */
};
static_assert(sizeof(CdState) <= (size_t)CD_STATE_BYTES, "CdState outgrew its slot");

/* Mem.RoundUp(Math.Max(blockSize, Mem.K1), Mem.K1) */
__host__ __device__ inline int64_t cd_block_size(int64_t asked) { return ((asked < 1024 ? 1024 : asked) + 1023) / 1024 * 1024; }
/* _outputLength */
__host__ __device__ inline int64_t cd_ring_length(int64_t B, int64_t extra, bool chaining)
{
    return chaining ? (int64_t)CD_HISTORY + (1 + (extra < 0 ? 0 : extra)) * B + 32 : B + 8;
}
/* the largest per-record blockSize of a chained decoder: with it index + blockSize <= _outputLength holds after CopyDict */
__host__ __device__ inline int64_t cd_max_record_block(int64_t B, int64_t extra) { return (1 + (extra < 0 ? 0 : extra)) * B + 32; }
/* state, then the ring (the reference allocates _outputLength + 8) with room for the copies' whole 16-byte stores */
__host__ __device__ inline int64_t cd_store_bytes(int64_t B, int64_t extra, bool chaining)
{
    return CD_STATE_BYTES + ((cd_ring_length(B, extra, chaining) + 64 + 255) & ~(int64_t)255);
}

struct CdRunArgs {
    const uint8_t *src;
    const uint64_t *recOff;          /* per record: where its bytes are in src */
    const uint32_t *recLen;          /* per record: their length, bit 31 = Inject */
    const int32_t *recBlockSize;     /* per record: Decode's blockSize (<= 0: the decoder's), or nullptr */
    const uint64_t *firstRec;        /* per stream */
    const uint32_t *nRec;            /* per stream; 0: the stream is left untouched */
    uint8_t *store;
    const uint64_t *storeOff;
    uint8_t *dst;                    /* with CD_FLAG_DRAIN */
    const uint64_t *dstOff, *dstCap;
    int32_t *recOut;                 /* per record: bytes produced or a code */
    int64_t *outLen;                 /* per stream: the run's total or the failing record's code */
    long long n;
    int flags;
    uint32_t *status;
};

__global__ __launch_bounds__(256) void k4_cdec_reset_kernel(const CdRecord *dec, uint8_t *store, const uint64_t *storeOff, int64_t *outLen, long long n)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    CdState *st = (CdState *)(store + storeOff[s]);
    const CdRecord r = dec[s];
    uint32_t *w = (uint32_t *)st;
    for (int i = 0; i < (int)(CD_STATE_BYTES / 4); i++) w[i] = 0u;
    st->blockSize = (int32_t)cd_block_size(r.blockSize);
    st->extraBlocks = r.chaining ? (r.extraBlocks < 0 ? 0 : r.extraBlocks) : 0;
    st->chaining = r.chaining ? 1 : 0;
    st->magic = CD_MAGIC;
    if (outLen) outLen[s] = 0;
}

__global__ __launch_bounds__(128 * DECODE_PAIRS_PER_WG) __attribute__((amdgpu_waves_per_eu(4, 8))) void k4_cdec_run_kernel(CdRunArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[DECODE_PAIRS_PER_WG][DECODE_PAIR_LDS_DWORDS];
    const int lane = lane_id();
    const uint32_t wave = uni(threadIdx.x >> 6);
    const uint32_t pair = wave >> 1, role = (wave ^ blockIdx.x) & 1u;   /* as in k4_decode_pair_kernel: 0 parses, 1 copies */
    const long long s = (long long)blockIdx.x * DECODE_PAIRS_PER_WG + (long long)pair;
    uint32_t *ring_lds = lds[pair], *pipe = lds[pair] + RING_DWORDS;
    if (role == 0) pipe_init(pipe, a.status, lane);
    /* the state, the same in every lane of both waves; the copying wave rewrites it only when the run is over */
    CdState *st = nullptr;
    uint32_t magic = 0, index = 0;
    int32_t B = 0, extra = 0, chaining = 0;
    unsigned long long records = 0, bytes = 0, moves = 0;
    if (s < a.n) {
        st = (CdState *)(a.store + a.storeOff[s]);
        magic = st->magic; B = st->blockSize; extra = st->extraBlocks; chaining = st->chaining; index = st->index;
        records = st->records; bytes = st->bytes; moves = st->moves;
    }
    __syncthreads();
    if (s >= a.n) return;
    const uint32_t count = a.nRec[s];
    const bool writes = role == 1;
    if (count == 0) {                                            /* untouched */
        if (writes && lane == 0) a.outLen[s] = 0;
        return;
    }
    const uint64_t first = a.firstRec[s];
    if (magic != CD_MAGIC) {                                     /* never reset: nothing of the store is believed */
        if (writes) {
            for (uint32_t k = (uint32_t)lane; k < count; k += 64u) a.recOut[first + k] = k == 0 ? CD_NO_DECODER : CD_NOT_RUN;
            if (lane == 0) a.outLen[s] = CD_NO_DECODER;
        }
        return;
    }
    uint8_t *buf = (uint8_t *)st + CD_STATE_BYTES;
    const uint32_t ring_len = (uint32_t)cd_ring_length(B, extra, chaining != 0);
    const bool drain = (a.flags & CD_FLAG_DRAIN) != 0;
    uint8_t *out = drain ? a.dst + a.dstOff[s] : nullptr;
    const uint64_t cap = drain ? a.dstCap[s] : 0u;
    uint64_t given = 0, total = 0;
    int fail = 0;
    uint32_t seq = 0, k = 0;
    for (; k < count; k++) {
        const uint32_t lc = a.recLen[first + k];
        const uint32_t n = lc & 0x7fffffffu;
        const bool inject = (lc & 0x80000000u) != 0;
        const uint8_t *in = a.src + a.recOff[first + k];
        uint32_t got = 0;
        const uint8_t *made = buf;                               /* where the record's bytes are */
        if (drain && !inject && n == 0) {                        /* DecodeAndDrain: sourceLength <= 0 decodes nothing (:313-314) */
            if (writes && lane == 0) a.recOut[first + k] = 0;
            continue;
        }
        if (inject) {
            if (n == 0) {                                        /* LZ4ChainDecoder.cs:66-67; LZ4BlockDecoder.cs:62-63 empties */
                if (!chaining) index = 0;
            } else if (!chaining) {                              /* LZ4BlockDecoder.Inject :58-71 */
                if (n > ring_len) { fail = CD_INJECT; break; }
                if (writes) {
                    wave_sync();
                    wave_copy(buf, in, n, lane);
                }
                index = n;
            } else {                                             /* LZ4ChainDecoder.Inject :64-93 */
                if (n > ((uint32_t)B > CD_HISTORY ? (uint32_t)B : CD_HISTORY)) { fail = CD_INJECT; break; }
                if (index + n < ring_len) {
                    made = buf + index;
                    index += n;
                } else if (n >= CD_HISTORY) {
                    index = n;
                } else {
                    const uint32_t tail = CD_HISTORY - n < index ? CD_HISTORY - n : index;
                    if (writes) {
                        wave_sync();
                        wave_shift_down(buf, buf + index - tail, tail, lane);
                    }
                    moves++;
                    made = buf + tail;
                    index = tail + n;
                }
                if (writes) {
                    wave_sync();
                    wave_copy((uint8_t *)made, in, n, lane);
                }
            }
            got = n;
        } else if (!chaining) {                                  /* LZ4BlockDecoder.Decode :39-55 */
            const int32_t bs = a.recBlockSize ? a.recBlockSize[first + k] : 0;
            if (bs > B) { fail = CD_BLOCK_SIZE; break; }
            int d = 0;                                           /* LZ4Codec.Decode: an empty source is 0, <= 0 from the engine is -1 */
            if (n > 0) {
                if (role == 0) {
                    d = decode_block<false, 1>(in, (int)n, buf, (int)ring_len, lane, ring_lds, nullptr, false, DecodeDict{nullptr, 0u, 0}, pipe, &seq);
                } else {
                    wave_sync();
                    d = decode_block<false, 2>(in, (int)n, buf, (int)ring_len, lane, ring_lds, nullptr, false, DecodeDict{nullptr, 0u, 0}, pipe, &seq);
                }
                if (d <= 0) { fail = CD_DECODE; break; }
            }
            index = (uint32_t)d;
            got = (uint32_t)d;
        } else {                                                 /* LZ4ChainDecoder.Decode :45-61 */
            int32_t bs = a.recBlockSize ? a.recBlockSize[first + k] : 0;
            if (bs <= 0) bs = B;
            if ((int64_t)bs > cd_max_record_block(B, extra)) { fail = CD_BLOCK_SIZE; break; }    /* the reference would pass its buffer's end */
            if (index + (uint32_t)bs > ring_len) {               /* Prepare -> CopyDict :117-132 */
                const uint32_t keep = index < CD_HISTORY ? index : CD_HISTORY;
                if (writes && keep != index) {
                    wave_sync();
                    wave_shift_down(buf, buf + index - keep, keep, lane);
                }
                if (keep != index) moves++;
                index = keep;
            }
            made = buf + index;
            DecodeDict dict{nullptr, 0u, 0};
            if (index) {
                const uint32_t hist = index < CD_HISTORY ? index : CD_HISTORY;
                dict = DecodeDict{made, hist >= 65535u ? 65536u : hist, 1};
            }
            int d;
            if (role == 0) {
                d = decode_block<false, 1>(in, (int)n, (uint8_t *)made, bs, lane, ring_lds, nullptr, false, dict, pipe, &seq);
            } else {
                wave_sync();                                     /* the move's and the previous record's stores -> this block's loads */
                d = decode_block<false, 2>(in, (int)n, (uint8_t *)made, bs, lane, ring_lds, nullptr, false, dict, pipe, &seq);
            }
            if (d < 0) { fail = CD_DECODE; break; }              /* 0 is a block of nothing */
            index += (uint32_t)d;
            got = (uint32_t)d;
        }
        records++; bytes += got; total += got;
        if (drain && got) {                                      /* Drain(target, -decoded, decoded), or DecodeAndDrain's false */
            if (cap - given < got) { fail = CD_TARGET; break; }
            if (writes) {
                wave_sync();
                wave_copy(out + given, made, got, lane);
            }
            given += got;
        }
        if (writes && lane == 0) a.recOut[first + k] = (int32_t)got;
    }
    if (!writes) return;
    if (fail) {
        for (uint32_t j = k + (uint32_t)lane; j < count; j += 64u) a.recOut[first + j] = j == k ? fail : CD_NOT_RUN;
    }
    wave_sync();
    if (lane == 0) {
        st->index = index; st->records = records; st->bytes = bytes; st->moves = moves; st->lastCode = fail;
        a.outLen[s] = fail ? (int64_t)fail : (int64_t)total;
    }
}

struct CdDrainArgs {
    const uint8_t *store;
    const uint64_t *storeOff;
    uint8_t *dst;
    const uint64_t *dstOff;
    const int64_t *offset;           /* relative to BytesReady: <= 0 */
    const int64_t *length;
    int64_t *outLen;                 /* length[s], or CD_RANGE */
    long long n;
};

__global__ __launch_bounds__(256) void k4_cdec_drain_kernel(CdDrainArgs a)
{
    const int lane = lane_id();
    const long long s = (long long)blockIdx.x * 4 + (long long)uni(threadIdx.x >> 6);
    if (s >= a.n) return;
    const CdState *st = (const CdState *)(a.store + a.storeOff[s]);
    int64_t result;
    if (st->magic != CD_MAGIC) {
        result = CD_NO_DECODER;
    } else {
        const int64_t index = (int64_t)st->index, at = index + a.offset[s], len = a.length[s];
        if (at < 0 || len < 0 || at > index || len > index - at) {        /* LZ4ChainDecoder.cs:99-100 */
            result = CD_RANGE;
        } else {
            wave_copy(a.dst + a.dstOff[s], (const uint8_t *)st + CD_STATE_BYTES + at, (uint32_t)len, lane);
            result = len;
        }
    }
    if (lane == 0) a.outLen[s] = result;
}

/* K4LZ4_CDQ_* words of out + s * CDQ_WORDS */
constexpr int CDQ_WORDS = 8;
__global__ __launch_bounds__(256) void k4_cdec_query_kernel(const uint8_t *store, const uint64_t *storeOff, int64_t *out, long long n)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const CdState *st = (const CdState *)(store + storeOff[s]);
    int64_t *o = out + s * CDQ_WORDS;
    const bool live = st->magic == CD_MAGIC;
    o[0] = live ? (int64_t)st->index : 0;
    o[1] = live ? st->blockSize : 0;
    o[2] = live ? (int64_t)st->records : 0;
    o[3] = live ? (int64_t)st->bytes : 0;
    o[4] = live ? st->lastCode : CD_NO_DECODER;
    o[5] = live ? st->chaining : 0;
    o[6] = live ? st->extraBlocks : 0;
    o[7] = live ? (int64_t)st->moves : 0;
}

}  // namespace k4
