/*
 * k4lz4_chain_encoder.hpp -- many open ILZ4Encoders advanced per call (k4lz4_chain_encode_batch).
 *
 * Each call applies to every stream a run of TopupAndEncode records (Encoders/LZ4EncoderExtensions.cs:117-210 over
 * Encoders/LZ4EncoderBase.cs).  Every length is known on the host, so the host lays the call out (ce_model: LZ4EncoderBase's ring over
 * the window [what the ring keeps | the bytes the run loads], with explicit block lengths -- a forced block may be shorter than
 * BlockSize in mid-stream); the existing encoders encode the window's blocks into k4lz4_compress_bound-sized slots; the frame
 * writer's copy kernel (k4_fw_copy_kernel) stages the window and writes the ring back (the window is scratch of the context, so no
 * move overlaps); and
 *   k4_ce_place_kernel   one wave per stream: applies the allowCopy rule per record, packs the run's blocks into dst + dstOff[s] in
 *                        record order and writes recLoaded, recOut and outLen
 * A stream's store: for chained fast streams its k4lz4_fast_chain_state, then the encoder's ring buffer.
 *
 * Two pieces of host arithmetic describe the same ring and must agree: ce_model, which walks the records, and ce_hc_rows /
 * ce_fast_rows, which walk block lengths and fill every chained encoder's plan (k4lz4_capi.hip: hc_chain_table / fast_chain_table,
 * whose whole streams have every length BlockSize but the last, and their _lens twins).  k4lz4_chain_encode_blocks and
 * k4lz4_chain_table_rows expose both; tests/test_chain_encoder_host.py compares them with each other and with the witness.
 */
#pragma once
#include <algorithm>
#include "../../../../include/k4lz4.h"
#include "k4lz4_common.hpp"

namespace k4 {

struct CeStream {
    unsigned long long out, cap;         /* dstOff, dstCap */
    unsigned long long firstRec, firstBlk;
    uint32_t nRec;
    int32_t code;                        /* < 0: refused (K4LZ4_CENC_*); 0: runs; 1: left untouched (no records) */
};

struct CeRec {
    int32_t loaded;                      /* what Topup took */
    int32_t blk;                         /* the record's block among its stream's in this call, -1: it encodes nothing */
    uint32_t allow, reserved;
};

struct CeBlock {
    unsigned long long slot, raw;        /* the encoder's slot and the block's own bytes in the window, both offsets into the scratch */
    int32_t len, reserved;
};

constexpr int CE_WAVE = 64;

__global__ __launch_bounds__(CE_WAVE) void k4_ce_place_kernel(const CeStream *streams, const CeRec *recs, const CeBlock *blocks, const int32_t *enc,
                                                            const uint8_t *scratch, uint8_t *dst, int32_t *recLoaded, int32_t *recOut,
                                                            long long *outLen, long long n)
{
    const long long s = blockIdx.x;
    if (s >= n) return;
    const int lane = (int)threadIdx.x;
    const CeStream st = streams[s];
    if (st.code != 0) {
        if (st.code < 0)
            for (uint32_t r = (uint32_t)lane; r < st.nRec; r += CE_WAVE) { recLoaded[st.firstRec + r] = 0; recOut[st.firstRec + r] = 0; }
        if (lane == 0) outLen[s] = st.code < 0 ? (long long)st.code : 0ll;
        return;
    }
    uint8_t *out = dst + st.out;
    unsigned long long at = 0;
    bool fits = true;
    for (uint32_t r = 0; r < st.nRec; r++) {
        const CeRec rec = recs[st.firstRec + r];
        int32_t res = 0;
        if (rec.blk >= 0 && fits) {
            const CeBlock b = blocks[st.firstBlk + (uint32_t)rec.blk];
            const int32_t got = enc[st.firstBlk + (uint32_t)rec.blk];
            /* LZ4EncoderBase.Encode: a block that did not shrink is stored raw under allowCopy */
            const bool raw = rec.allow && got >= b.len;
            const uint32_t bytes = raw ? (uint32_t)b.len : (uint32_t)(got > 0 ? got : 0);
            if (got <= 0 || at + bytes > st.cap) {
                fits = false;                            /* (the host's bound rules this out: nothing is written past the target) */
            } else {
                wave_copy(out + at, scratch + (raw ? b.raw : b.slot), bytes, lane);
                res = raw ? -b.len : got;
                at += bytes;
            }
        }
        if (lane == 0) { recLoaded[st.firstRec + r] = rec.loaded; recOut[st.firstRec + r] = res; }
    }
    if (lane == 0) outLen[s] = fits ? (long long)at : (long long)K4LZ4_CENC_TARGET;
}

/* ---- host side: the record, the model, the bound (k4lz4_capi.hip; tests/emu/emu_chain_encoder.cpp lays a call out the same way) */
constexpr int64_t CE_STATE_BYTES = ((int64_t)sizeof(k4lz4_fast_chain_state) + 255) / 256 * 256;
constexpr int64_t CE_CHAIN_LIMIT = (int64_t)1 << 31;

inline int64_t ce_ring_at(const k4lz4_chain_encoder &e) { return e.kind == 2 ? CE_STATE_BYTES : 0; }
inline int64_t ce_bound_of(int64_t n) { return n + n / 255 + 16; }                     /* k4lz4_compress_bound */
inline int64_t ce_slot(const k4lz4_chain_encoder &e) { return ce_bound_of(e.blockSize); }

/* Encoders/LZ4Encoder.cs: Create; LZ4EncoderBase's and LZ4HighChainEncoder's constructors */
inline void ce_init(k4lz4_chain_encoder &e, const k4lz4_chain_encoder_settings &s)
{
    e = k4lz4_chain_encoder{};
    e.kind = !s.chaining ? 0 : s.level < K4LZ4_L03_HC ? 2 : 1;
    e.level = e.kind == 1 ? std::max<int32_t>(K4LZ4_L03_HC, std::min<int32_t>(K4LZ4_L12_MAX, s.level)) : e.kind == 2 ? 0 : s.level;
    const int64_t b = (std::max<int64_t>(s.blockSize, 1024) + 1023) / 1024 * 1024;    /* Mem.RoundUp(Math.Max(blockSize, Mem.K1), Mem.K1) */
    e.blockSize = (int32_t)b;
    e.extraBlocks = e.kind == 0 ? 0 : std::max<int32_t>(s.extraBlocks, 0);
    const int64_t ring = (e.kind == 0 ? 0 : 65536) + (1 + (int64_t)e.extraBlocks) * b + 32;   /* LZ4EncoderBase.cs:34 */
    e.ringBytes = (int32_t)ring;
    e.storeBytes = (ce_ring_at(e) + ring + 8 + 255) / 256 * 256;
}

/* LZ4EncoderBase under TopupAndEncode, in window coordinates: ring position p is window position ws + p, and the bytes a record
 * loads go to the window's end.  rec(r, loaded, at): record r took `loaded` bytes, which go to window position `at`;
 * block(r, start, len, dict, ws, small): record r encodes [start, start + len) with the ring's first byte at window position ws
 * (the HC context's dictLimit) and, for the fast chain, dictSize bytes in front of it; small is LZ4_compress_fast_continue's choice
 * of dictSmall (dictSize < 64 KiB and < currentOffset). */
struct CeAfter {
    int64_t index = 0, pointer = 0, ws = 0, nblk = 0, loaded = 0, bound = 0;
    uint32_t cur = 0, dict = 0;
    bool too_long = false;
};

template <class Rec, class Block>
inline CeAfter ce_model(const k4lz4_chain_encoder &e, const uint32_t *recLen, const uint32_t *recFlags, int64_t nrec, Rec rec, Block block)
{
    CeAfter a;
    const int64_t B = e.blockSize, L = e.ringBytes;
    int64_t idx = e.index, ptr = e.pointer, ws = 0, d = e.dictSize, cur = e.currentOffset;
    int64_t encoded = e.taken - (e.pointer - e.index);       /* stream bytes encoded so far */
    for (int64_t r = 0; r < nrec; r++) {
        const int64_t len = recLen[r];
        const bool force = (recFlags[r] & K4LZ4_CENC_FORCE) != 0, allow = (recFlags[r] & K4LZ4_CENC_ALLOW_COPY) != 0;
        int64_t loaded = 0;
        if (len > 0) {                                       /* Topup */
            const int64_t space = idx + B - ptr;
            if (space > 0) loaded = std::min(space, len);
        }
        rec(r, loaded, ws + ptr);
        ptr += loaded; a.loaded += loaded;
        const int64_t n = ptr - idx;                         /* FlushAndEncode: BytesReady */
        if (n < (force ? 1 : B)) continue;
        if (e.kind == 1 && encoded + 65536 > CE_CHAIN_LIMIT) a.too_long = true;      /* LZ4_compressHC_continue_generic's renormalisation */
        if (e.kind == 2 && cur + n > CE_CHAIN_LIMIT) a.too_long = true;              /* LZ4_renormDictT */
        block(r, ws + idx, n, d, ws, e.kind == 2 && d < 65536 && d < cur);
        a.nblk++;
        a.bound += allow ? n : ce_bound_of(n);
        d += n; cur += n; encoded += n;
        idx = ptr;                                           /* Commit */
        if (idx + B > L) {
            int64_t keep = 0;                                /* LZ4BlockEncoder.CopyDict */
            if (e.kind == 1) { keep = std::min<int64_t>(65536, ptr); if (keep < 4) keep = 0; }      /* LZ4_saveDictHC */
            else if (e.kind == 2) { keep = std::min<int64_t>(65536, std::min(ptr, d)); d = keep; }  /* LZ4_saveDict */
            ws += ptr - keep;
            idx = ptr = keep;
        }
    }
    a.index = idx; a.pointer = ptr; a.ws = ws; a.cur = (uint32_t)cur; a.dict = (uint32_t)d;
    return a;
}

inline CeAfter ce_after(const k4lz4_chain_encoder &e, const uint32_t *recLen, const uint32_t *recFlags, int64_t nrec)
{
    return ce_model(e, recLen, recFlags, nrec, [](int64_t, int64_t, int64_t) {}, [](int64_t, int64_t, int64_t, int64_t, int64_t, bool) {});
}

/* the record after a run */
inline void ce_advance(k4lz4_chain_encoder &e, const CeAfter &a)
{
    e.index = (int32_t)a.index; e.pointer = (int32_t)a.pointer;
    e.taken += a.loaded; e.blocks += a.nblk;
    if (e.kind == 2) { e.currentOffset = a.cur; e.dictSize = a.dict; }
}

/* ---- the chained encoders' block tables, the one walk over LZ4EncoderBase's ring that hc_chain_table / fast_chain_table and their
 * _lens twins (k4lz4_capi.hip) fill their plans through: the content's first D bytes are what the ring buffer holds, block j
 * is the next len[j] bytes (len: an array, or anything else with []).  A whole stream has every length B but the last. */
template <class Len, class Row>   /* row(j, ws, pos, len, dictLimit): the block sees [ws, pos) in front of it, ws = max(dictLimit, pos - 64 KiB) */
inline void ce_hc_rows(int64_t D, Len len, int64_t n, int64_t B, int64_t extra, Row row)
{
    const int64_t L = 65536 + (1 + extra) * B + 32;
    int64_t ptr = D, dl = 0, pos = D;
    for (int64_t j = 0; j < n; j++) {
        row(j, std::max(dl, pos - 65536), pos, (int64_t)len[j], dl);
        pos += len[j]; ptr += len[j];
        if (ptr + B > L) {                                   /* Commit -> LZ4_saveDictHC(ctx, buf, ptr) */
            int64_t d = std::min<int64_t>(65536, std::min(ptr, pos - dl));
            if (d < 4) d = 0;
            dl = pos - d; ptr = d;
        }
    }
}

template <class Len, class Row>   /* row(j, pos, len, dictSize, dictSmall) -> the dictSize after the last block's Commit; cur0: currentOffset */
inline int64_t ce_fast_rows(int64_t D, int64_t cur0, Len len, int64_t n, int64_t B, int64_t extra, Row row)
{
    const int64_t L = 65536 + (1 + extra) * B + 32;
    int64_t ptr = D, dict = D, pos = D, cur = cur0;
    for (int64_t j = 0; j < n; j++) {
        row(j, pos, (int64_t)len[j], dict, dict < 65536 && dict < cur);
        pos += len[j]; ptr += len[j]; dict += len[j]; cur += len[j];
        if (ptr + B > L) { dict = std::min<int64_t>(65536, dict); ptr = dict; }      /* Commit -> LZ4_saveDict(ctx, buf, ptr) */
    }
    return dict;
}

}  // namespace k4
