/* tests/emu/emu_frame_write.cpp -- the incremental frame writer's kernels (k4lz4_frame_write.hpp) and its host half (the record's
 * model, refusals and advance) compiled against the host wave emulator, in a library of its own (tests/frame_write_emu.py builds it).
 * One call of k4emu_fw_call is what k4lz4_frame_write_batch_device does for n streams, with the block encoder replaced by the caller's
 * encoded blocks: XXH32.Update, staging into the window, ring write-back, record sizes, block checksums, the scan, the records'
 * places, the records and the edges.  The caller owns every array.  Test infrastructure only. */
#include "hip/hip_runtime.h"

/* (the emulator has the 32-bit form only; k4lz4_legacy.hpp, whose scan the writer uses, needs the 64-bit one to compile) */
static inline unsigned long long atomicMin(unsigned long long *p, unsigned long long v)
{
    unsigned long long cur = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return cur;
}

#include "k4lz4_legacy.hpp"
#include "k4lz4_frame_write.hpp"

#include <vector>

extern "C" {

/* XXH32.Update of state[i] over data + off[i] (len[i] bytes), reset first where fresh[i]; then the digests */
void k4emu_fw_xxh32(const uint8_t *data, const uint64_t *off, const uint64_t *len, const uint32_t *fresh, k4::FwXxhState *state,
                    uint32_t *digest, long long n, int threads)
{
    if (n <= 0) return;
    std::vector<k4::FwHashItem> items((size_t)n);
    for (long long i = 0; i < n; i++) items[(size_t)i] = k4::FwHashItem{data + off[i], len[i], state + i, fresh[i], 0u};
    const k4::FwHashItem *p = items.data();
    k4emu::launch_fn(dim3((unsigned)((n * 4 + k4::FW_THREADS - 1) / k4::FW_THREADS)), dim3(k4::FW_THREADS), [=] { k4::k4_fw_xxh32_kernel(p, n); },
                     threads);
    for (long long i = 0; i < n; i++) digest[i] = k4::fw_xxh32_digest(state[i]);
}

/* the model alone: per stream its code and the call's blocks (start in window coordinates, length), the records advanced for the streams
 * that run.  Returns the number of blocks, or -1 when they do not fit maxBlocks. */
long long k4emu_fw_plan(k4lz4_frame_writer *w, const int64_t *srcLen, const uint64_t *dstCap, long long n, int op, int32_t *code,
                        uint32_t *nblk, int64_t *blkStart, int64_t *blkLen, long long maxBlocks)
{
    const bool closing = op == K4LZ4_FWRITE_CLOSE;
    long long k = 0;
    for (long long i = 0; i < n; i++) {
        nblk[i] = 0;
        code[i] = srcLen[i] < 0 ? 1 : k4::fw_code(w[i], srcLen[i], closing, dstCap[i]);
        if (code[i] != 0) continue;
        const k4::FwAfter a = k4::fw_model(w[i], srcLen[i], closing, [&](int64_t s, int64_t l) {
            if (k < maxBlocks) { blkStart[k] = s; blkLen[k] = l; }
            k++;
        });
        nblk[i] = (uint32_t)a.nblk;
        k4::fw_advance(w[i], srcLen[i], closing, a);
    }
    return k > maxBlocks ? -1 : k;
}

/* one call, as the device form runs it, for streams that are all run (no refusals): encLen / encArena + encOff are the caller's encoder
 * results for the call's blocks in stream order.  Returns the number of blocks, -1 when the caller's block count differs. */
long long k4emu_fw_call(k4lz4_frame_writer *w, uint8_t *store, const uint64_t *storeOff, const uint8_t *src, const uint64_t *srcOff,
                        const int64_t *srcLen, long long n, int op, const int32_t *encLen, const uint8_t *encArena, const uint64_t *encOff,
                        long long nEnc, uint8_t *dst, const uint64_t *dstOff, int64_t *outLen, int threads)
{
    const bool closing = op == K4LZ4_FWRITE_CLOSE;
    std::vector<k4::FwAfter> after((size_t)n);
    std::vector<k4::FwStream> rows((size_t)n);
    std::vector<k4::FwHashItem> hash;
    std::vector<k4::FwPiece> stage, back;
    std::vector<std::vector<uint8_t>> win((size_t)n);
    std::vector<uint32_t> owner;
    std::vector<int64_t> bsum_first;
    long long nb = 0;
    for (long long i = 0; i < n; i++) {
        k4::FwStream &row = rows[(size_t)i];
        row = k4::FwStream{};
        const k4lz4_frame_writer &r = w[i];
        const int64_t len = srcLen[i];
        if (len < 0) { row.code = 1; continue; }
        const k4::FwAfter a = k4::fw_model(r, len, closing, [&](int64_t, int64_t) { owner.push_back((uint32_t)i); });
        after[(size_t)i] = a;
        uint8_t *sto = store + storeOff[i];
        const bool opens = k4::fw_opens(r, len, closing);
        row.out = dstOff[i]; row.first = (unsigned long long)nb; row.nblk = (uint32_t)a.nblk;
        row.hdrLen = opens ? k4::fw_header(r, row.hdr) : 0;
        row.close = closing && !(r.phase == 0 && len == 0) ? (r.settings.contentChecksum ? 2u : 1u) : 0u;
        row.xxh = (const k4::FwXxhState *)sto;
        nb += a.nblk;
        if (r.settings.contentChecksum && (len > 0 || opens))
            hash.push_back(k4::FwHashItem{src + srcOff[i], (unsigned long long)len, (k4::FwXxhState *)sto, opens ? 1u : 0u, 0u});
        uint8_t *ring = sto + k4::fw_ring_at(r);
        if (a.nblk) {
            win[(size_t)i].assign((size_t)(r.pointer + len) + 16, 0);
            uint8_t *wp = win[(size_t)i].data();
            stage.push_back(k4::FwPiece{wp, ring, (unsigned long long)r.pointer, 0});
            stage.push_back(k4::FwPiece{wp + r.pointer, src + srcOff[i], (unsigned long long)len, 0});
            const int64_t r0 = a.ws == 0 ? r.pointer : 0;
            back.push_back(k4::FwPiece{ring + r0, wp + a.ws + r0, (unsigned long long)(a.pointer - r0), 0});
        } else if (len > 0) {
            stage.push_back(k4::FwPiece{ring + r.pointer, src + srcOff[i], (unsigned long long)len, 0});
        }
    }
    if (nb != nEnc) return -1;
    auto copy = [&](std::vector<k4::FwPiece> &p) {
        if (p.empty()) return;
        unsigned long long c = 0;
        for (auto &x : p) { x.chunk0 = c; c += std::max<unsigned long long>(1, (x.len + k4::FW_CHUNK - 1) / k4::FW_CHUNK); }
        const k4::FwPiece *pp = p.data();
        const long long cnt = (long long)p.size();
        k4emu::launch_fn(dim3((unsigned)c), dim3(k4::FW_THREADS), [=] { k4::k4_fw_copy_kernel(pp, cnt); }, threads);
    };
    if (!hash.empty()) {
        const k4::FwHashItem *hp = hash.data();
        const long long nh = (long long)hash.size();
        k4emu::launch_fn(dim3((unsigned)((nh * 4 + k4::FW_THREADS - 1) / k4::FW_THREADS)), dim3(k4::FW_THREADS), [=] { k4::k4_fw_xxh32_kernel(hp, nh); },
                         threads);
    }
    copy(stage);
    copy(back);                                   /* (the encoder would run between the two: the caller's blocks stand in for it) */
    const long long nbb = std::max<long long>(nb, 1);
    std::vector<unsigned long long> stored((size_t)nbb), rec((size_t)nbb), excl((size_t)nbb), roff((size_t)nbb), cnt(8, 0);
    std::vector<uint32_t> sums((size_t)nbb);
    std::vector<int32_t> outl(encLen, encLen + nb);
    const k4::FwStream *rp = rows.data();
    if (nb) {
        const int32_t *ol = outl.data();
        unsigned long long *sp = stored.data(), *rl = rec.data(), *ex = excl.data(), *ro = roff.data(), *cp = cnt.data();
        const uint32_t *op_ = owner.data();
        uint32_t *sm = sums.data();
        const unsigned bgrid = (unsigned)((nb + k4::FW_THREADS - 1) / k4::FW_THREADS);
        /* record sizes: every block with a checksum here, the stream's own setting below (the library orders its blocks so that those
         * with checksums come last and passes their first index) */
        k4emu::launch_fn(dim3(bgrid), dim3(k4::FW_THREADS), [=] { k4::k4_fw_reclen_kernel(ol, sp, rl, nb, 0); }, threads);
        for (long long b = 0; b < nb; b++) if (!w[owner[(size_t)b]].settings.blockChecksum) rec[(size_t)b] -= 4;
        k4::HashArgs ha{encArena, encOff, (const uint64_t *)sp, sm, nb, 0u};
        k4emu::launch_fn(dim3((unsigned)((nb * 4 + k4::XXH_THREADS - 1) / k4::XXH_THREADS)), dim3(k4::XXH_THREADS), [=] { k4::k4_xxh32_kernel(ha); },
                         threads);
        k4emu::launch_fn(dim3(1), dim3(k4::LEGACY_SCAN_THREADS), [=] { k4::k4_legacy_scan_kernel((const uint64_t *)rl, (uint64_t *)ex, nb, cp); },
                         threads);
        k4emu::launch_fn(dim3(bgrid), dim3(k4::FW_THREADS), [=] { k4::k4_fw_place_kernel(rp, op_, ex, ro, nb); }, threads);
        for (long long b = 0; b < nb; b++) {
            const bool bs = w[owner[(size_t)b]].settings.blockChecksum != 0;
            k4::FrameBlocksArgs fa{encArena, encOff + b, ol + b, bs ? sm + b : nullptr, (const uint64_t *)ro + b, dst, 1};
            k4emu::launch_fn(dim3(1), dim3(256), [=] { k4::k4_frame_blocks_kernel(fa); }, threads);
        }
    }
    const unsigned long long *ex = excl.data(), *rl = rec.data();
    long long *ol64 = (long long *)outLen;
    k4emu::launch_fn(dim3((unsigned)((n + k4::FW_THREADS - 1) / k4::FW_THREADS)), dim3(k4::FW_THREADS),
                     [=] { k4::k4_fw_edges_kernel(rp, ex, rl, dst, ol64, n); }, threads);
    for (long long i = 0; i < n; i++)
        if (srcLen[i] >= 0) k4::fw_advance(w[i], srcLen[i], closing, after[(size_t)i]);
    return nb;
}

}  // extern "C"
