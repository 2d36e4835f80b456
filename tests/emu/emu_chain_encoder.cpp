/* tests/emu/emu_chain_encoder.cpp -- many open ILZ4Encoders (k4lz4_chain_encoder.hpp) compiled against the host wave emulator, in a
 * library of its own (tests/chain_encoder_emu.py builds it).  One call of k4emu_ce_call is what k4lz4_chain_encode_batch_device
 * does for n streams, laid out by the same model, with the block encoders replaced by the caller's encoded blocks: staging into
 * the windows, ring and state write-back (k4_fw_copy_kernel) and placement (k4_ce_place_kernel).  Every window and every slot lies
 * between guard bytes in a scratch of this file's own, checked after the kernels.  Test infrastructure only. */
#include "hip/hip_runtime.h"
#include "k4lz4_frame_write.hpp"
#include "k4lz4_chain_encoder.hpp"

#include <cstring>
#include <vector>

namespace {
constexpr size_t GUARD = 64;
constexpr uint8_t FILL = 0xEE;
}

extern "C" {

/* encLen / encArena + encOff: the caller's encoder results (before the allowCopy rule) for the call's blocks, streams in order,
 * each stream's blocks in record order.  honourBound 0 skips the host's refusal, so that a target below the bound reaches the
 * placement kernel.  Returns the number of blocks, -1 when the caller's block count differs, -2 when a guard byte of the scratch
 * was written. */
long long k4emu_ce_call(k4lz4_chain_encoder *enc, uint8_t *store, const uint64_t *storeOff, const uint8_t *src, const uint64_t *recOff,
                        const uint32_t *recLen, const uint32_t *recFlags, long long nRecords, const uint64_t *firstRec, const uint32_t *nRec,
                        long long n, const int32_t *encLen, const uint8_t *encArena, const uint64_t *encOff, long long nEnc, uint8_t *dst,
                        const uint64_t *dstOff, const uint64_t *dstCap, int honourBound, int32_t *recLoaded, int32_t *recOut, int64_t *outLen,
                        int threads)
{
    std::vector<k4::CeAfter> after((size_t)n);
    std::vector<k4::CeStream> rows((size_t)n);
    std::vector<k4::CeRec> recs((size_t)std::max<long long>(nRecords, 1));
    std::vector<k4::CeBlock> blocks;
    std::vector<uint64_t> win((size_t)n, 0), first((size_t)n, 0);
    std::vector<std::pair<size_t, size_t>> guards;          /* (offset, bytes) of every guard range */
    size_t at = 0;
    auto take = [&](size_t bytes) {
        guards.push_back({at, GUARD}); at += GUARD;
        const size_t o = at; at += bytes;
        guards.push_back({at, GUARD}); at += GUARD;
        return o;
    };
    long long nb = 0, nfast = 0;
    for (long long i = 0; i < n; i++) {
        k4::CeStream &row = rows[(size_t)i];
        row = k4::CeStream{};
        row.nRec = nRec[i]; row.firstRec = nRec[i] ? firstRec[i] : 0; row.code = 1;
        if (!nRec[i]) continue;
        after[(size_t)i] = k4::ce_after(enc[i], recLen + firstRec[i], recFlags + firstRec[i], nRec[i]);
        row.code = honourBound && (int64_t)dstCap[i] < after[(size_t)i].bound ? K4LZ4_CENC_TARGET : 0;
        if (row.code != 0) continue;
        row.out = dstOff[i]; row.cap = dstCap[i]; row.firstBlk = (unsigned long long)nb;
        first[(size_t)i] = (uint64_t)nb;
        nb += after[(size_t)i].nblk;
        if (after[(size_t)i].nblk && enc[i].kind == 2) nfast++;
    }
    if (nb != nEnc) return -1;
    blocks.resize((size_t)std::max<long long>(nb, 1));
    for (long long i = 0; i < n; i++)
        if (rows[(size_t)i].code == 0 && after[(size_t)i].nblk) win[(size_t)i] = take((size_t)(enc[i].pointer + after[(size_t)i].loaded));
    std::vector<uint64_t> slot0((size_t)n, 0);
    for (long long i = 0; i < n; i++)
        if (rows[(size_t)i].code == 0)
            for (int64_t j = 0; j < after[(size_t)i].nblk; j++) {
                const size_t o = take((size_t)k4::ce_slot(enc[i]));
                blocks[(size_t)(first[(size_t)i] + (uint64_t)j)].slot = o;
            }
    const size_t o_stin = take((size_t)std::max<long long>(nfast, 1) * sizeof(k4lz4_fast_chain_state)),
                 o_stout = take((size_t)std::max<long long>(nfast, 1) * sizeof(k4lz4_fast_chain_state));
    std::vector<uint8_t> scratch(at + 64, FILL);
    uint8_t *d = scratch.data();
    k4lz4_fast_chain_state *stin = (k4lz4_fast_chain_state *)(d + o_stin), *stout = (k4lz4_fast_chain_state *)(d + o_stout);

    std::vector<k4::FwPiece> stage, back;
    long long kfast = 0;
    for (long long i = 0; i < n; i++) {
        if (rows[(size_t)i].code != 0) continue;
        const k4lz4_chain_encoder &e = enc[i];
        const k4::CeAfter &a = after[(size_t)i];
        uint8_t *sto = store + storeOff[i], *ring = sto + k4::ce_ring_at(e);
        const bool runs = a.nblk > 0;
        uint8_t *wp = d + win[(size_t)i];
        k4::CeRec *rr = recs.data() + firstRec[i];
        const uint64_t *ro = recOff + firstRec[i];
        int64_t j = 0;
        if (runs) stage.push_back(k4::FwPiece{wp, ring, (unsigned long long)e.pointer, 0});
        k4::ce_model(e, recLen + firstRec[i], recFlags + firstRec[i], nRec[i],
            [&](int64_t r, int64_t loaded, int64_t where) {
                rr[r].loaded = (int32_t)loaded; rr[r].blk = -1; rr[r].allow = (recFlags[firstRec[i] + r] & K4LZ4_CENC_ALLOW_COPY) ? 1u : 0u;
                if (loaded) stage.push_back(k4::FwPiece{(runs ? wp : ring) + where, src + ro[r], (unsigned long long)loaded, 0});
            },
            [&](int64_t r, int64_t start, int64_t len, int64_t, int64_t, bool) {
                k4::CeBlock &b = blocks[(size_t)(first[(size_t)i] + (uint64_t)j)];
                rr[r].blk = (int32_t)j; b.raw = win[(size_t)i] + (uint64_t)start; b.len = (int32_t)len;
                j++;
            });
        if (!runs) continue;
        const int64_t r0 = a.ws == 0 ? e.pointer : 0;
        back.push_back(k4::FwPiece{ring + r0, wp + a.ws + r0, (unsigned long long)(a.pointer - r0), 0});
        if (e.kind == 2) {
            const long long f = kfast++;
            stage.push_back(k4::FwPiece{(uint8_t *)(stin + f), e.currentOffset ? (const uint8_t *)sto : nullptr, sizeof(k4lz4_fast_chain_state), 0});
            back.push_back(k4::FwPiece{sto, (const uint8_t *)(stout + f), sizeof(k4lz4_fast_chain_state), 0});
        }
    }
    auto copy = [&](std::vector<k4::FwPiece> &p) {
        if (p.empty()) return;
        unsigned long long c = 0;
        for (auto &x : p) { x.chunk0 = c; c += std::max<unsigned long long>(1, (x.len + k4::FW_CHUNK - 1) / k4::FW_CHUNK); }
        const k4::FwPiece *pp = p.data();
        const long long cnt = (long long)p.size();
        k4emu::launch_fn(dim3((unsigned)c), dim3(k4::FW_THREADS), [=] { k4::k4_fw_copy_kernel(pp, cnt); }, threads);
    };
    copy(stage);
    /* the encoders' stand-in: the caller's blocks go into the slots; a fast chain's state goes through unchanged */
    for (long long b = 0; b < nb; b++)
        if (encLen[b] > 0) memcpy(d + blocks[(size_t)b].slot, encArena + encOff[b], (size_t)encLen[b]);
    if (kfast) memcpy(stout, stin, (size_t)kfast * sizeof(k4lz4_fast_chain_state));
    copy(back);
    const k4::CeStream *rp = rows.data();
    const k4::CeRec *cp = recs.data();
    const k4::CeBlock *bp = blocks.data();
    const uint8_t *dc = d;
    long long *ol = (long long *)outLen;
    k4emu::launch_fn(dim3((unsigned)n), dim3(k4::CE_WAVE), [=] { k4::k4_ce_place_kernel(rp, cp, bp, encLen, dc, dst, recLoaded, recOut, ol, n); }, threads);
    for (const auto &g : guards)
        for (size_t k = 0; k < g.second; k++)
            if (d[g.first + k] != FILL) return -2;
    for (long long i = 0; i < n; i++)
        if (rows[(size_t)i].code == 0) k4::ce_advance(enc[i], after[(size_t)i]);
    return nb;
}

}  // extern "C"
