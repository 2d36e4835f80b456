/*
 * k4lz4_capi.hip -- host side of libk4lz4.so (see include/k4lz4.h for the contract).
 *
 * The only compute path is the gfx950 kernels in this directory; there is no CPU fallback.
 * Host-pointer batch calls stage through device buffers owned by the context:
 *   H2D  the source span + the four metadata vectors
 *   run  one kernel launch per batch (one wavefront per block)
 *   D2H  outLen, then the produced bytes (compact device layout -> pinned staging -> the
 *        caller's slots, copying exactly outLen[i] bytes so dst[ret..cap) stays untouched,
 *        SpanTests.cs:36-44).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <memory>
#include <new>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <chrono>
#include <vector>

#include "../../../../include/k4lz4.h"
#include "k4lz4_decode.hpp"
#include "k4lz4_encode_fast.hpp"
#include "k4lz4_parse.hpp"
#include "k4lz4_pickle.hpp"
#include "k4lz4_segments.hpp"
#include "k4lz4_encode_hc.hpp"
#include "k4lz4_fast_chain.hpp"
#include "k4lz4_frame.hpp"
#include "k4lz4_frame_read.hpp"
#include "k4lz4_legacy.hpp"
#include "k4lz4_frame_write.hpp"
#include "k4lz4_frame_reader.hpp"
#include "k4lz4_frame_feed.hpp"
#include "k4lz4_legacy_stream.hpp"
#include "k4lz4_legacy_feed.hpp"
#include "k4lz4_chain_decoder.hpp"
#include "k4lz4_chain_encoder.hpp"
#include "k4lz4_xxh32.hpp"
#include "k4lz4_selftest.hpp"
#include "k4lz4_dict_encode.hpp"
#include "k4lz4_dict_encode_hc.hpp"
#include "k4lz4_dict_set.hpp"
#include "k4lz4_chain_open.hpp"
#include "k4lz4_frame_dict.hpp"
#include "k4lz4_frame_reader_dict.hpp"

constexpr int MAX_PARTS = 8;      /* a big host-pointer call is staged, run and brought back in up to this many parts */

/* What a device form builds on the host and sends up with its launches (a block table, a writer's plan, a list's words): the host
 * copy is rewritten only after ev says the previous upload of it is over (plan_begin, plan_send).  dev: the grow-only device
 * scratch the plan is laid out in, grown by grow_scratch. */
struct PlanUpload {
    std::vector<uint8_t> host;
    uint8_t *dev = nullptr; size_t cap = 0;
    hipEvent_t ev = nullptr;
};

struct k4lz4_ctx {
    int device = -1;
    std::string error;
    hipStream_t stream = nullptr;   /* used by the host-pointer calls */
    int accel = 1;                  /* fast-encoder acceleration of the next launch (LLxx-level calls only) */
    unsigned long long *prof = nullptr;   /* diagnostic counters of the next launch (k4lz4_profile_batch_device) */
    bool prof_pair = false;               /* ... of the two-waves-per-block decoder (32 counters per block) */
    bool prof_stamp = false;              /* ... or only start / end / placement of every block, written by the ordinary kernels */
    /* grow-only device / pinned scratch for the host-pointer calls */
    uint8_t *d_src = nullptr; size_t d_src_cap = 0;
    uint8_t *d_dst = nullptr; size_t d_dst_cap = 0;
    uint8_t *d_meta = nullptr; size_t d_meta_cap = 0;
    uint8_t *h_stage = nullptr; size_t h_stage_cap = 0;
    uint8_t *d_sched = nullptr; size_t d_sched_cap = 0;   /* dispatch-order scratch: cost[n], order[n], counters */
    int cu_count = 256;
    uint8_t *d_dict = nullptr; size_t d_dict_cap = 0;         /* host-pointer decode with dictionaries: staged dictionaries + their metadata */
    uint8_t *d_gtab = nullptr; size_t d_gtab_cap = 0;         /* fast encoder: hash tables of the blocks encoded without an LDS table */
    hipStream_t aux = nullptr;                                /* second queue: those blocks run beside the LDS-table kernel */
    hipStream_t aux2 = nullptr;                               /* third queue: the later segments of blocks cut into segments (k4lz4_segments.hpp) */
    hipEvent_t ev_join2 = nullptr;
    uint8_t *d_seg = nullptr; size_t d_seg_cap = 0;           /* segment records, work list, snapshots, tables */
    uint8_t *d_seg_first = nullptr; size_t d_seg_first_cap = 0;   /* per block: its first segment's record or -1 */
    bool use_segments = true;                                 /* K4LZ4_NO_SEGMENTS */
    uint32_t seg_min = 1024u << 10, seg_target = 640u << 10, seg_warm = 384u << 10;   /* K4LZ4_SEG_MIN / _TARGET / _WARM (bytes) */
    uint32_t seg_target_max = 1408u << 10;                    /* K4LZ4_SEG_TARGET_MAX; K4LZ4_SEG_TARGET alone fixes the size (1152 KiB until round 6: the two-step encoder's runs are faster, gpurun_out/r6o) */
    uint32_t seg_spin_max = 0;                                /* K4LZ4_SEG_SPIN_MAX: polls a run waits for its successor's cut (0: SEG_SPIN_MAX); tests force the exit with 1 */
    uint32_t seg_div = 3500;                                  /* K4LZ4_SEG_DIV: blocks shorter than the batch's bytes / this stay whole */
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    uint8_t *d_hc_hash = nullptr; size_t d_hc_hash_cap = 0;   /* HC: per-block hash tables of one launch chunk */
    uint8_t *d_hc_work = nullptr; size_t d_hc_work_cap = 0;   /* HC: prev[] / cand[] of one launch chunk */
    uint8_t *d_hc_meta = nullptr; size_t d_hc_meta_cap = 0;   /* HC: work offsets, pickle slots */
    uint8_t *d_pk_meta = nullptr; size_t d_pk_meta_cap = 0;   /* fast-level pickles through the encoder kernels: encoder slots and results */
    int pickle_split_min = 512;           /* K4LZ4_PICKLE_SPLIT_MIN: batches of more messages than this go that way */
    /* The scratch above is shared by all calls on this context but ordered only by the stream a call runs on: the end of
     * every launch is recorded here and the next launch on a DIFFERENT stream waits for it before it touches the scratch
     * (calls on one context are serialised across streams). */
    hipEvent_t ev_busy = nullptr;
    hipStream_t last_stream = nullptr;
    bool busy = false;
    /* k4lz4_ctx_reserve_hc: HC levels sized without asking the device (0 = not reserved) */
    uint64_t hc_res_total = 0; uint32_t hc_res_longest = 0;
    /* host-pointer calls of some size stage through two pinned buffers per direction, filled / emptied by a few threads while
     * the DMA engine moves the previous chunk; d_pack takes the produced bytes packed next to each other */
    uint8_t *h_in[2] = {nullptr, nullptr}; size_t h_in_cap[2] = {0, 0};
    uint8_t *h_out[2] = {nullptr, nullptr}; size_t h_out_cap[2] = {0, 0};
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    uint8_t *d_pack = nullptr; size_t d_pack_cap = 0;
    /* big host-pointer calls run as two halves: the second half's bytes go up (copy queue) while the first half's kernels
     * run, the first half's results come down while the second half's kernels run; results' sizes via a pinned array */
    hipStream_t copyq = nullptr;
    hipStream_t dlq = nullptr;          /* ... and the way back has a queue (and a thread, and helper threads) of its own: up and down at once */
    hipEvent_t ev_up[MAX_PARTS] = {}, ev_len[MAX_PARTS] = {};
    uint8_t *h_len = nullptr; size_t h_len_cap = 0;
    struct Pool *pool = nullptr, *pool_dl = nullptr;   /* helper threads of the upload side, of the download side */
    bool pool_failed = false, pool_dl_failed = false;
    int stage_threads = 7;      /* helper threads of the staging copies (K4LZ4_STAGE_THREADS - 1, read once at creation) */
    /* diagnostic switches, read once at creation: K4LZ4_SPLIT_PCT (1..100, share of an encode batch on the LDS-table kernel),
     * K4LZ4_NO_PAIR (decode with one wave per block) */
    uint32_t *d_pace = nullptr;     /* the per-SIMD slots of the late-blocks-first priorities (k4lz4_common.hpp, Pace) */
    uint32_t *d_status = nullptr;   /* this context's status word: DEV_STATUS_* bits raised by its kernels (k4lz4_common.hpp) */
    int split_pct = -1;
    bool no_pair = false;
    int direct_span_pct = 200;            /* K4LZ4_DIRECT_SPAN_PCT: a registered source goes up as it lies while its span is at most this share of its blocks' bytes */
    bool no_direct = false;               /* K4LZ4_NO_DIRECT: registered host memory is staged like any other */
    int lds_floor_per_cu = 8;             /* K4LZ4_LDS_FLOOR: blocks per CU the LDS-table kernel gets at least */
    int cost_pct = 48;                    /* K4LZ4_COST_PCT: the LDS-table kernel's share of a batch's estimated cost (k4_order_kernel) */
    int dec_parts = 4, dec_parts_direct = 8;   /* K4LZ4_DEC_PARTS, K4LZ4_DEC_PARTS_DIRECT: parts of a big decode-like host-pointer call (2..MAX_PARTS); with a registered destination */
    int last_decode_kernel = 0;           /* k4lz4_last_decode_kernel: enum k4lz4_decode_kernel of the latest KIND_DECODE / KIND_UNPICKLE launch (launch_decode_like) */
    int last_encode_route = 0;            /* k4lz4_last_encode_route: enum k4lz4_encode_route bits of the latest encode / pickle / wrap call, or-ed over its launch chunks */
    int hop2_max_per_cu = 12;             /* K4LZ4_HOP2_MAX: pair decoders follow the token chain two links per hop in launches of up to this many blocks per CU */
    bool hc_cand_lds = true;              /* K4LZ4_HC_CAND_MEM unsets it: blocks of at most 64 KiB get their candidate records by k4_hc_cand_kernel (from memory) */
    int hc_cand_dynlds = 0;               /* K4LZ4_HC_CAND_DYNLDS (a measurement switch): bytes of unused LDS per workgroup of k4_hc_cand_kernel, i.e. fewer of them per CU */
    int hc_segs = 0;                      /* K4LZ4_HC_SEGS = 1 / 2 / 4: waves per block of the level-3 parse (0: by the batch's size) */
    bool hc_chain_parts = true;           /* K4LZ4_HC_CHAIN_OLD unsets it: blocks of at most 64 KiB build their chains with sixteen waves per block (k4_hc_chain_part_kernel) */
    int hc_mem_pct = 33;                  /* K4LZ4_HC_MEM_PCT: share of an HC chunk whose chains are built with the table in memory, beside the LDS-table kernel */
    int pace_min_per_cu = 6;              /* K4LZ4_PACE_MIN: batches of more blocks per CU than this use the priorities (measured: 8 per CU +3 % encode, +7 % decode; 4 per CU -1 %, -4 %) */
    int parse_pace_min_per_cu = 8;        /* ... and the same for k4_parse_kernel's priorities (k4lz4_parse.hpp, ParsePace; measured on 64 KiB blocks, encode launch:
                                           * 2 and 4 per CU -1.2 %, 8 per CU level, 16 per CU +4.6 %) */
    bool parse_pace_queue = false;        /* K4LZ4_PACE_QUEUE: ... also where every wave takes block after block from the queue (measured: 64 blocks of 64 KiB
                                           * per CU -1.3 %, 256 of 4 KiB -3 %, so not by default) */
    bool use_pace = true;                 /* K4LZ4_NO_PACE: without the late-blocks-first priorities */
    bool prof_gtab = false;               /* K4LZ4_PROF_GTAB: the instrumented encoder keeps its table in global memory */
    uint8_t *d_parse = nullptr; size_t d_parse_cap = 0;       /* two-kernel fast encoder (k4lz4_parse.hpp): records, per-block counts, tables of the waves without an LDS table */
    bool use_parse = true;                /* K4LZ4_NO_PARSE: fast-level batches go to the one-kernel encoders as before */
    bool parse_queue = false;             /* K4LZ4_PARSE_QUEUE */
    bool hc_records = true;               /* K4LZ4_NO_HC_RECORDS: level 3 writes its sequences out inside the parse loop (rounds 1-5) */
    bool parse_seg = true;                /* K4LZ4_NO_PARSE_SEG: ragged batches (pickles, K4LZ4_FLAG_SEGMENTS) through the one-kernel encoders and their *_seg twins (rounds 3-5) */
    bool parse_big = true;                /* K4LZ4_NO_PARSE_BIG: blocks of 65 547 bytes and more stay with the one-kernel encoder (round 5) */
    bool parse_persist = true;            /* K4LZ4_NO_PERSIST: batches beyond one residency in launches of one residency each (round 5) instead of one persistent launch */
    bool parse_inline_emit = true;        /* K4LZ4_NO_INLINE_EMIT: the blocks' bytes by k4_emit_kernel behind the parse instead of by the parsing waves themselves */
    bool parse_migrate = true;            /* K4LZ4_NO_MIGRATE: blocks whose table lives in memory stay there (k4lz4_parse.hpp, ParseCtl) */
    bool parse_pcost = true;              /* K4LZ4_NO_PCOST: the one-kernel encoder's sequence count over 256 bytes orders the two-step encoder's blocks, as before
                                           * the parse's own estimate (k4lz4_parse.hpp, ParseCost) did; K4LZ4_PCOST, which used to switch that on, still may be set */
    k4::ParseCost pcost_fit = k4::PCOST_FIT;      /* K4LZ4_PCOST_FIT: sample,max_rounds,round,slow,seq,group,lazy,long,base (the fields of ParseCost) for trying another fit */
    int parse_waves = 16;                 /* K4LZ4_PARSE_WAVES: blocks per workgroup (= per CU) of the parse kernel, at most PARSE_MAX_WAVES */
    bool trace = false;         /* K4LZ4_TRACE: host-pointer calls print where their time went (stderr) */
    /* chained HC and fast streams (k4lz4_encode_hc_chain_batch*, k4lz4_encode_fast_chain_batch*): the block table */
    PlanUpload chain_plan;
    /* frame reader (k4lz4_frame_read.hpp): per-frame words and the block table, both grow-only */
    uint8_t *d_fr = nullptr; size_t d_fr_cap = 0;
    uint8_t *d_fb = nullptr; size_t d_fb_cap = 0;
    /* legacy streams (k4lz4_legacy.hpp): per-stream words, the chunk table and the writer's arena, all grow-only */
    uint8_t *d_lg = nullptr; size_t d_lg_cap = 0;
    uint8_t *d_frd = nullptr; size_t d_frd_cap = 0;      /* the incremental reader's fast path: plans and block table */
    uint8_t *d_lgr = nullptr; size_t d_lgr_cap = 0;
    uint8_t *d_lga = nullptr; size_t d_lga_cap = 0;
    /* incremental frame writer (k4lz4_frame_write.hpp): the call's plan, and the device scratch it is laid out in with the windows,
     * the arena and the fast-chain states.  The LZ4Stream writer, the chain encoder and its open from a set share it. */
    PlanUpload fw_plan;
    /* messages against shared dictionaries, per family of levels (fast: k4lz4_dict_encode.hpp, 16 KiB of tables per distinct
     * dictionary; HC: k4lz4_dict_encode_hc.hpp, 256 KiB each and as much per wave of the encode launch).  plan.dev: the tables,
     * the list's words, the dispatch order and the wave slots (dict_layout); plan.host: the copy of the words that goes up;
     * table, kept: which table and what kept length the most recent call gave every entry of its list (the state queries) --
     * empty after a call against a k4lz4_dict_set.  The families share nothing: neither disturbs what the other left for its
     * query. */
    struct DictScratch {
        PlanUpload plan;
        std::vector<uint32_t> table, kept;
    } dict_fast, dict_hc;
    /* k4lz4_decode_dictset_batch_device: the per-message dictionary words k4_dict_pick_kernel writes, and its copy of dstCap; grow-only */
    uint8_t *d_dpick = nullptr; size_t d_dpick_cap = 0;
    /* frames with a DictID (k4lz4_frame_dict.hpp): the call's id table and the entry of every frame; the blocks' dictionary words
     * and the in-order decoder's windows; both grow-only.  fdict_plan: the ids on their way up into d_fdx (it has no scratch of its own) */
    uint8_t *d_fdx = nullptr; size_t d_fdx_cap = 0;
    uint8_t *d_fdb = nullptr; size_t d_fdb_cap = 0;
    PlanUpload fdict_plan;
};

/* the switches above, read from the environment once, when a context is created */
static void read_switches(k4lz4_ctx &c)
{
    if (const char *pct = getenv("K4LZ4_SPLIT_PCT")) { const int v = atoi(pct); c.split_pct = v < 1 ? 1 : (v > 100 ? 100 : v); }
    c.no_pair = getenv("K4LZ4_NO_PAIR") != nullptr;
    c.prof_gtab = getenv("K4LZ4_PROF_GTAB") != nullptr;
    c.use_pace = getenv("K4LZ4_NO_PACE") == nullptr;
    if (const char *e = getenv("K4LZ4_PACE_MIN")) c.pace_min_per_cu = c.parse_pace_min_per_cu = std::max(0, atoi(e));
    c.parse_pace_queue = getenv("K4LZ4_PACE_QUEUE") != nullptr;
    if (const char *e = getenv("K4LZ4_DIRECT_SPAN_PCT")) c.direct_span_pct = std::max(100, atoi(e));
    if (const char *e = getenv("K4LZ4_NO_DIRECT")) c.no_direct = atoi(e) != 0;
    if (const char *e = getenv("K4LZ4_LDS_FLOOR")) c.lds_floor_per_cu = std::max(0, std::min(8, atoi(e)));
    if (const char *e = getenv("K4LZ4_COST_PCT")) c.cost_pct = std::max(1, std::min(99, atoi(e)));
    if (const char *e = getenv("K4LZ4_DEC_PARTS")) c.dec_parts = std::max(2, std::min(MAX_PARTS, atoi(e)));
    if (const char *e = getenv("K4LZ4_DEC_PARTS_DIRECT")) c.dec_parts_direct = std::max(2, std::min(MAX_PARTS, atoi(e)));
    if (const char *e = getenv("K4LZ4_HOP2_MAX")) c.hop2_max_per_cu = std::max(0, atoi(e));
    c.hc_chain_parts = getenv("K4LZ4_HC_CHAIN_OLD") == nullptr;
    c.hc_cand_lds = getenv("K4LZ4_HC_CAND_MEM") == nullptr;
    if (const char *e = getenv("K4LZ4_HC_CAND_DYNLDS")) c.hc_cand_dynlds = std::max(0, std::min(65536, atoi(e)));
    if (const char *e = getenv("K4LZ4_HC_SEGS")) { const int v = atoi(e); c.hc_segs = v >= 4 ? 4 : (v >= 2 ? 2 : (v == 1 ? 1 : 0)); }
    if (const char *e = getenv("K4LZ4_HC_MEM_PCT")) c.hc_mem_pct = std::max(0, std::min(100, atoi(e)));
    c.use_segments = getenv("K4LZ4_NO_SEGMENTS") == nullptr;
    if (const char *e = getenv("K4LZ4_SEG_MIN")) c.seg_min = (uint32_t)std::max(65536 + 4096, atoi(e));
    if (const char *e = getenv("K4LZ4_SEG_TARGET")) c.seg_target = c.seg_target_max = (uint32_t)std::max(8192, atoi(e));
    if (const char *e = getenv("K4LZ4_SEG_TARGET_MAX")) c.seg_target_max = (uint32_t)std::max(8192, atoi(e));
    if (const char *e = getenv("K4LZ4_SEG_WARM")) c.seg_warm = (uint32_t)std::max(0, atoi(e));
    if (const char *e = getenv("K4LZ4_SEG_SPIN_MAX")) c.seg_spin_max = (uint32_t)std::max(0, atoi(e));
    if (const char *e = getenv("K4LZ4_SEG_DIV")) c.seg_div = (uint32_t)std::max(0, atoi(e));
    if (const char *e = getenv("K4LZ4_PICKLE_SPLIT_MIN")) c.pickle_split_min = std::max(0, atoi(e));
    if (const char *e = getenv("K4LZ4_STAGE_THREADS")) c.stage_threads = std::max(0, std::min(63, atoi(e) - 1));
    c.use_parse = getenv("K4LZ4_NO_PARSE") == nullptr;
    c.parse_queue = getenv("K4LZ4_PARSE_QUEUE") != nullptr;
    c.parse_persist = getenv("K4LZ4_NO_PERSIST") == nullptr;
    c.parse_big = getenv("K4LZ4_NO_PARSE_BIG") == nullptr;
    c.parse_seg = getenv("K4LZ4_NO_PARSE_SEG") == nullptr;
    c.hc_records = getenv("K4LZ4_NO_HC_RECORDS") == nullptr;
    c.parse_pcost = getenv("K4LZ4_NO_PCOST") == nullptr || getenv("K4LZ4_PCOST") != nullptr;
    if (const char *e = getenv("K4LZ4_PCOST_FIT")) {
        unsigned v[9];
        if (sscanf(e, "%u,%u,%u,%u,%u,%u,%u,%u,%u", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8]) == 9 && v[0] >= k4::PARSE_MIN_LEN && v[0] < 65536u)
            c.pcost_fit = k4::ParseCost{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]};
    }
    c.parse_migrate = getenv("K4LZ4_NO_MIGRATE") == nullptr;
    c.parse_inline_emit = getenv("K4LZ4_NO_INLINE_EMIT") == nullptr;
    if (const char *e = getenv("K4LZ4_PARSE_WAVES")) c.parse_waves = std::max(1, std::min(k4::PARSE_MAX_WAVES, atoi(e)));
    c.trace = getenv("K4LZ4_TRACE") != nullptr;
}

/* k4lz4_dict_set: one device allocation that nothing writes after create.  Carved at 64-byte steps in this order:
 * the kept bytes of every distinct dictionary; the entries' words for the decoders; per family the words and tables its load and
 * encode kernels take.  The host keeps what the queries and the argument checks need. */
struct k4lz4_dict_set {
    struct Family {
        bool on = false;
        uint64_t *toff = nullptr, *eoff = nullptr;          /* device: per table / per entry, where the kept bytes start in buf */
        uint32_t *tlen = nullptr, *elen = nullptr, *etab = nullptr;
        uint8_t *tables = nullptr;
        std::vector<uint32_t> table, kept;                  /* host, per entry */
        int64_t ntables = 0, loads = 0;
    };
    int device = -1;
    int32_t nDict = 0;
    int families = 0;
    uint8_t *buf = nullptr;
    uint64_t bytes = 0;
    uint64_t *dec_off = nullptr;                            /* device, per entry: the kept bytes for the decoders */
    int32_t *dec_len = nullptr;
    std::vector<uint64_t> keptAt;                           /* host, per entry */
    std::vector<int32_t> keptLen;
    Family fast, hc;
};

/* a few helper threads for the staging copies of big host-pointer calls (memcpy between the caller's pageable memory and
 * the pinned buffers is what limits such calls, not PCIe) */
struct Pool {
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable cv_work, cv_done;
    std::function<void(int)> job;
    int parts = 0, next = 0, pending = 0;
    unsigned long long gen = 0;
    bool stop = false;
    explicit Pool(int nthreads)
    {
        for (int t = 0; t < nthreads; t++) workers.emplace_back([this] { run(); });
    }
    ~Pool()
    {
        { std::lock_guard<std::mutex> g(m); stop = true; }
        cv_work.notify_all();
        for (auto &w : workers) w.join();
    }
    void run()
    {
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv_work.wait(lk, [this] { return stop || next < parts; });
            if (stop) return;
            const int i = next++;
            lk.unlock();
            job(i);
            lk.lock();
            if (--pending == 0) cv_done.notify_all();
        }
    }
    /* f(0) .. f(parts - 1), the caller takes part as well */
    void parallel(int nparts, const std::function<void(int)> &f)
    {
        if (nparts <= 1 || workers.empty()) { for (int i = 0; i < nparts; i++) f(i); return; }
        std::unique_lock<std::mutex> lk(m);
        job = f; parts = nparts; next = 0; pending = nparts; gen++;
        cv_work.notify_all();
        while (next < parts) {
            const int i = next++;
            lk.unlock();
            f(i);
            lk.lock();
            if (--pending == 0) cv_done.notify_all();
        }
        cv_done.wait(lk, [this] { return pending == 0; });
        parts = 0;
    }
};

namespace {

thread_local std::string tl_error;
thread_local int tl_status = K4LZ4_OK;

std::mutex g_err_mu;   /* a host-pointer call's download thread and its staging thread may both fail at the same moment */
int fail(k4lz4_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) { std::lock_guard<std::mutex> g(g_err_mu); ctx->error = msg; }
    tl_error = msg;
    return code;
}

int hip_fail(k4lz4_ctx *ctx, hipError_t e, const char *what)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    (void)hipGetLastError();
    return fail(ctx, K4LZ4_E_HIP, buf);
}

#define K4_HIP(ctx, call)                                                   \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #call);              \
    } while (0)

enum Kind { KIND_ENCODE, KIND_DECODE, KIND_PICKLE, KIND_UNPICKLE, KIND_WRAP };
/* the envelope an encode is wrapped in (launch_hc): none, LZ4Pickler's, LZ4Wrapper's */
enum Envelope { ENV_NONE, ENV_PICKLE, ENV_WRAP };
constexpr int FLAG_SEGMENTS_OK = 1 << 20;   /* launch_fast_encode: big blocks may be cut into segments (k4lz4_segments.hpp); not part of the API */

/* LL.Enforce32 (Engine/LL.tools.cs:19-27): a process-wide switch in the reference, so here too */
std::atomic<int> g_enforce32{0};

int grow(k4lz4_ctx *ctx, uint8_t **p, size_t *cap, size_t need, bool pinned);

/* After a synchronisation of the call's stream: did a kernel launched through THIS context report call-level trouble?
 * Reads and clears the context's own word -- only this context's kernels write it and they have finished, so nothing can
 * land between the read and the clear -- and reports every bit that is set. */
int take_device_status(k4lz4_ctx *ctx)
{
    uint32_t v = 0;
    if (!ctx->d_status) return K4LZ4_OK;
    if (hipMemcpy(&v, ctx->d_status, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return K4LZ4_OK; }
    if (v == 0) return K4LZ4_OK;
    (void)hipMemset(ctx->d_status, 0, sizeof v);
    const bool nomem = (v & k4::DEV_STATUS_HC_SCRATCH) != 0, timeout = (v & k4::DEV_STATUS_PIPE_TIMEOUT) != 0;
    std::string msg;
    if (!nomem && !timeout && (v & k4::DEV_STATUS_DICT_INDEX))
        return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_dict_batch_device: a dictIdx outside the dictionary list: those messages report -1");
    if (nomem) msg += "HC scratch reserved with k4lz4_ctx_reserve_hc was too small for the batch: its blocks were not encoded";
    if (timeout) msg += std::string(nomem ? "; " : "") + "a wave gave up waiting for its partner wave (a decoder pair, or the waves that parse one block at HC level 3: scheduling time-out, not corrupt data): the affected blocks report failure";
    return fail(ctx, nomem ? K4LZ4_E_NOMEM : K4LZ4_E_HIP, msg.c_str());
}

/* one wave per item, W waves per workgroup */
#define K4_LAUNCH_WAVES(kernel, items, W, stream, ...) \
    hipLaunchKernelGGL(kernel, dim3((unsigned)(((items) + (W) - 1) / (W))), dim3(64 * (W)), 0, stream, __VA_ARGS__)

/* scratch that has to grow is freed first: what still runs on it must be finished (same-stream reuse needs no wait).  For scratch
 * that one call's own launches order on `stream`; the device forms' scratch, ordered by ev_busy, grows through grow_scratch */
int grow_after(k4lz4_ctx *ctx, hipStream_t stream, uint8_t **p, size_t *cap, size_t need)
{
    if (need > *cap) K4_HIP(ctx, hipStreamSynchronize(stream));
    return grow(ctx, p, cap, need, false);
}

/* the envelope around an encode: the encoders' slots prepared in front of them (LZ4Pickler: block = envelope + 5, cap U - 1;
 * LZ4Wrapper: + 8, cap U - 1), the envelopes closed behind them */
void envelope_prep(Envelope env, k4::BatchArgs a, uint64_t *encOff, int32_t *encCap, hipStream_t stream)
{
    if (env == ENV_PICKLE) hipLaunchKernelGGL(k4::k4_pickle_prep_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a, encOff, encCap);
    if (env == ENV_WRAP) hipLaunchKernelGGL(k4::k4_wrap_prep_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a, encOff, encCap);
}

void envelope_finish(Envelope env, k4::BatchArgs a, int32_t *encLen, hipStream_t stream)
{
    if (env == ENV_PICKLE) K4_LAUNCH_WAVES(k4::k4_pickle_finish_kernel, a.n, k4::PICKLE_FINISH_WAVES_PER_WG, stream, a, encLen);
    if (env == ENV_WRAP) K4_LAUNCH_WAVES(k4::k4_wrap_finish_kernel, a.n, k4::WRAP_FINISH_WAVES_PER_WG, stream, a, encLen);
}

/* per-block dictionaries for decode (device pointers) */
struct DictArgs {
    const uint8_t *dict;
    const uint64_t *off;
    const int32_t *len;
    const signed char *mode;
};

/* the batch launcher (launch_inner and what it dispatches to): enqueues the kernels for n blocks; all pointers are device pointers */
#include "k4lz4_launch.hpp"

/* A device form's prologue: the context's scratch (dispatch order, hash tables, HC work areas, the stream formats' tables)
 * may still be in use by a call that was enqueued on another stream -- st waits for it. */
hipError_t order_after_ctx(k4lz4_ctx *ctx, hipStream_t st)
{
    return ctx->busy && ctx->last_stream != st ? hipStreamWaitEvent(st, ctx->ev_busy, 0) : hipSuccess;
}

/* ... and its epilogue: the end of its work on st is what the next call on another stream waits for */
void mark_busy(k4lz4_ctx *ctx, hipStream_t st)
{
    if (hipEventRecord(ctx->ev_busy, st) == hipSuccess) { ctx->busy = true; ctx->last_stream = st; }
    else (void)hipGetLastError();
}

/* grow-only scratch of the device forms: grow frees the old buffer, so one that has to grow waits for the context's earlier work */
int grow_scratch(k4lz4_ctx *ctx, uint8_t **p, size_t *cap, size_t need)
{
    if (need > *cap && ctx->busy) K4_HIP(ctx, hipEventSynchronize(ctx->ev_busy));
    return grow(ctx, p, cap, need, false);
}

/* The plan upload, first half: the previous upload of p's host copy is over (the event is made on first use), and the copy has
 * `bytes` bytes -- zeroed: all of them 0; otherwise what was there stays and the caller writes every byte it sends. */
int plan_begin(k4lz4_ctx *ctx, PlanUpload &p, size_t bytes, bool zeroed)
{
    if (!p.ev) K4_HIP(ctx, hipEventCreateWithFlags(&p.ev, hipEventDisableTiming));
    else K4_HIP(ctx, hipEventSynchronize(p.ev));
    try { if (zeroed) p.host.assign(bytes, 0); else p.host.resize(bytes); } catch (...) { return fail(ctx, K4LZ4_E_NOMEM, "out of host memory"); }
    return K4LZ4_OK;
}

/* ... second half: the first `bytes` of the host copy go to dev on `stream`, behind the context's earlier work, and the event
 * says when they have left. */
int plan_send(k4lz4_ctx *ctx, PlanUpload &p, void *dev, size_t bytes, hipStream_t stream)
{
    K4_HIP(ctx, order_after_ctx(ctx, stream));
    K4_HIP(ctx, hipMemcpyAsync(dev, p.host.data(), bytes, hipMemcpyHostToDevice, stream));
    K4_HIP(ctx, hipEventRecord(p.ev, stream));
    return K4LZ4_OK;
}

int launch(k4lz4_ctx *ctx, Kind kind, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
           const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags,
           hipStream_t stream, const DictArgs *dd = nullptr, const int32_t *hostLen = nullptr)
{
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, order_after_ctx(ctx, stream));
    const int rc = launch_inner(ctx, kind, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, level, flags, stream, dd, hostLen);
    mark_busy(ctx, stream);
    return rc;
}

int grow(k4lz4_ctx *ctx, uint8_t **p, size_t *cap, size_t need, bool pinned)
{
    if (need <= *cap) return K4LZ4_OK;
    const size_t want = std::max(need, *cap + *cap / 2);
    if (*p) {
        if (pinned) (void)hipHostFree(*p); else (void)hipFree(*p);
        *p = nullptr; *cap = 0;
    }
    hipError_t e = pinned ? hipHostMalloc((void **)p, want, hipHostMallocDefault) : hipMalloc((void **)p, want);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, K4LZ4_E_NOMEM, "out of device/pinned memory"); }
    *cap = want;
    return K4LZ4_OK;
}

int check_batch_args(k4lz4_ctx *ctx, const void *src, const void *srcOff, const void *srcLen, const void *dst,
                     const void *dstOff, const void *dstCap, const void *outLen, int64_t n)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0) return fail(ctx, K4LZ4_E_ARG, "negative block count");
    if (n > 0 && (!src || !srcOff || !srcLen || !dst || !dstOff || !dstCap || !outLen))
        return fail(ctx, K4LZ4_E_ARG, "NULL batch pointer");
    return K4LZ4_OK;
}

constexpr size_t STAGE_CHUNK = (size_t)16 << 20;

Pool *pool_of(k4lz4_ctx *ctx)
{
    if (!ctx->pool && !ctx->pool_failed) {
        const unsigned hw = std::thread::hardware_concurrency();
        const int nthreads = (int)std::min<unsigned>((unsigned)ctx->stage_threads, hw > 2 ? hw / 2 - 1 : 0u);
        /* std::thread's constructor throws when the system has no thread to give: nothing may leave a C entry point that way,
         * and the copies work without helpers (pool == nullptr: the calling thread does them alone) */
        try { ctx->pool = new Pool(nthreads); } catch (...) { ctx->pool = nullptr; ctx->pool_failed = true; }
    }
    return ctx->pool;
}

Pool *pool_dl_of(k4lz4_ctx *ctx)
{
    if (!ctx->pool_dl && !ctx->pool_dl_failed) {
        const unsigned hw = std::thread::hardware_concurrency();
        const int nthreads = (int)std::min<unsigned>((unsigned)ctx->stage_threads, hw > 2 ? hw / 2 - 1 : 0u);
        try { ctx->pool_dl = new Pool(nthreads); } catch (...) { ctx->pool_dl = nullptr; ctx->pool_dl_failed = true; }
    }
    return ctx->pool_dl;
}

/* memcpy split over the helper threads */
void parallel_copy(k4lz4_ctx *ctx, uint8_t *d, const uint8_t *s, size_t nbytes)
{
    Pool *p = pool_of(ctx);
    const int parts = p ? (int)std::min<size_t>(p->workers.size() + 1, std::max<size_t>(1, nbytes >> 20)) : 1;
    if (parts <= 1) { memcpy(d, s, nbytes); return; }
    /* (the parts' size rounded UP before it is rounded to 64: with nbytes / parts a multiple of 64 and a remainder left, `parts`
     * pieces of the rounded-down size stop up to parts - 1 bytes short of the end -- the last bytes of an upload's last chunk
     * stayed what the pinned buffer held before; found by tests/tools/gpu_stress_encode.py in round 5) */
    const size_t per = (((nbytes + (size_t)parts - 1) / (size_t)parts) + 63) & ~(size_t)63;
    p->parallel(parts, [=](int i) {
        const size_t lo = per * (size_t)i;
        if (lo < nbytes) memcpy(d + lo, s + lo, std::min(per, nbytes - lo));
    });
}

/* caller's (pageable) memory -> device: small transfers directly, big ones through two pinned buffers so that the copy into
 * the buffer for chunk k+1 runs while the DMA engine moves chunk k */
int staged_upload(k4lz4_ctx *ctx, uint8_t *d_dst, const uint8_t *h_src, size_t nbytes, hipStream_t st)
{
    if (nbytes < 2 * STAGE_CHUNK) {
        K4_HIP(ctx, hipMemcpyAsync(d_dst, h_src, nbytes, hipMemcpyHostToDevice, st));
        return K4LZ4_OK;
    }
    int rc;
    for (int b = 0; b < 2; b++)
        if ((rc = grow(ctx, &ctx->h_in[b], &ctx->h_in_cap[b], STAGE_CHUNK, true)) != K4LZ4_OK) return rc;
    bool used[2] = {true, true};            /* an earlier upload of this call may still be reading the buffers */
    int b = 0;
    for (size_t pos = 0; pos < nbytes; pos += STAGE_CHUNK, b ^= 1) {
        const size_t len = std::min(STAGE_CHUNK, nbytes - pos);
        if (used[b]) K4_HIP(ctx, hipEventSynchronize(ctx->ev_in[b]));   /* the DMA out of this buffer two chunks ago */
        parallel_copy(ctx, ctx->h_in[b], h_src + pos, len);
        K4_HIP(ctx, hipMemcpyAsync(d_dst + pos, ctx->h_in[b], len, hipMemcpyHostToDevice, st));
        K4_HIP(ctx, hipEventRecord(ctx->ev_in[b], st));
        used[b] = true;
    }
    return K4LZ4_OK;
}

/* The same for blocks that lie far apart in the caller's memory (compressed blocks in slots of worst-case size: the
 * span is 1.7 times the bytes): only the blocks travel, packed next to each other at 16-byte steps -- the copy into the
 * pinned buffer is being made anyway.  packed[i] = where block i goes on the device (ascending, 16-byte steps, given);
 * blocks first .. last-1. */
int staged_upload_packed(k4lz4_ctx *ctx, uint8_t *d_dst, const uint8_t *h_base, const uint64_t *srcOff, const int32_t *srcLen,
                         int64_t first_block, int64_t last_block, const uint64_t *packed, hipStream_t st)
{
    int rc;
    for (int b = 0; b < 2; b++)
        if ((rc = grow(ctx, &ctx->h_in[b], &ctx->h_in_cap[b], STAGE_CHUNK, true)) != K4LZ4_OK) return rc;
    bool used[2] = {true, true};            /* an earlier upload of this call may still be reading the buffers */
    int b = 0;
    for (int64_t first = first_block; first < last_block; b ^= 1) {
        const uint64_t base = packed[first];             /* device offset of the chunk being filled */
        uint64_t fill = 0;
        int64_t last = first;
        for (; last < last_block; last++) {
            const uint64_t len = srcLen[last] > 0 ? (((uint64_t)srcLen[last] + 15u) & ~(uint64_t)15u) : 0u;
            if (fill + len > STAGE_CHUNK) break;
            fill += len;
        }
        if (used[b]) K4_HIP(ctx, hipEventSynchronize(ctx->ev_in[b]));   /* the DMA out of this buffer two chunks ago */
        uint8_t *buf = ctx->h_in[b];
        const int64_t cnt = last - first;
        Pool *p = pool_of(ctx);
        const int parts = p && fill >= ((uint64_t)2 << 20) ? (int)std::min<int64_t>((int64_t)p->workers.size() + 1, cnt) : 1;
        auto body = [&, parts](int part) {
            const int64_t a = first + cnt * part / parts, e = first + cnt * (part + 1) / parts;
            for (int64_t i = a; i < e; i++)
                if (srcLen[i] > 0) memcpy(buf + (packed[i] - base), h_base + srcOff[i], (size_t)srcLen[i]);
        };
        if (parts <= 1) body(0); else p->parallel(parts, body);
        if (fill) K4_HIP(ctx, hipMemcpyAsync(d_dst + base, buf, (size_t)fill, hipMemcpyHostToDevice, st));
        K4_HIP(ctx, hipEventRecord(ctx->ev_in[b], st));
        used[b] = true;
        first = last;
    }
    return K4LZ4_OK;
}

/* device -> the caller's slots: block i's stored[i] bytes sit at d_from + from_off[i]; chunks of whole blocks come over
 * into a pinned buffer while the previous chunk is scattered into the slots by the helper threads */
int staged_download(k4lz4_ctx *ctx, uint8_t *dst, const uint64_t *dstOff, const uint8_t *d_from, const uint64_t *from_off,
                    const int32_t *stored, int64_t n, hipStream_t st, Pool *p)
{
    struct Chunk { int64_t first, last; uint64_t lo, hi; };
    std::vector<Chunk> chunks;
    size_t biggest = 0;
    for (int64_t i = 0; i < n;) {
        while (i < n && stored[i] <= 0) i++;
        if (i >= n) break;
        Chunk c{i, i, from_off[i], from_off[i] + (uint64_t)stored[i]};
        for (int64_t j = i + 1; j < n; j++) {
            if (stored[j] <= 0) { c.last = j; continue; }
            const uint64_t hi = from_off[j] + (uint64_t)stored[j];
            if (hi - c.lo > STAGE_CHUNK) break;
            c.last = j; c.hi = hi;
        }
        biggest = std::max(biggest, (size_t)(c.hi - c.lo));
        chunks.push_back(c);
        i = c.last + 1;
    }
    if (chunks.empty()) return K4LZ4_OK;
    int rc;
    for (int b = 0; b < 2; b++)
        if ((rc = grow(ctx, &ctx->h_out[b], &ctx->h_out_cap[b], biggest + 64, true)) != K4LZ4_OK) return rc;
    auto scatter = [&](const Chunk &c, const uint8_t *buf) {
        const int64_t cnt = c.last - c.first + 1;
        const int parts = p && (c.hi - c.lo) >= ((uint64_t)2 << 20) ? (int)std::min<int64_t>((int64_t)p->workers.size() + 1, cnt) : 1;
        auto body = [&, parts](int part) {
            const int64_t a = c.first + cnt * part / parts, e = c.first + cnt * (part + 1) / parts;
            for (int64_t i = a; i < e; i++)
                if (stored[i] > 0) memcpy(dst + dstOff[i], buf + (from_off[i] - c.lo), (size_t)stored[i]);
        };
        if (parts <= 1) body(0); else p->parallel(parts, body);
    };
    for (size_t k = 0; k < chunks.size(); k++) {
        const int b = (int)(k & 1);
        K4_HIP(ctx, hipMemcpyAsync(ctx->h_out[b], d_from + chunks[k].lo, (size_t)(chunks[k].hi - chunks[k].lo), hipMemcpyDeviceToHost, st));
        K4_HIP(ctx, hipEventRecord(ctx->ev_out[b], st));
        if (k > 0) {                                      /* the previous chunk has arrived by now, or soon: scatter it while this one flies */
            K4_HIP(ctx, hipEventSynchronize(ctx->ev_out[b ^ 1]));
            scatter(chunks[k - 1], ctx->h_out[b ^ 1]);
        }
    }
    const int lastb = (int)((chunks.size() - 1) & 1);
    K4_HIP(ctx, hipEventSynchronize(ctx->ev_out[lastb]));
    scatter(chunks.back(), ctx->h_out[lastb]);
    return K4LZ4_OK;
}

/* Host memory the caller has page-locked through k4lz4_host_register: the DMA engine reads and writes it directly, so a
 * host-pointer call whose source or destination lies inside such a range skips the pinned staging buffers on that side. */
std::mutex g_reg_mu;
struct RegRange { uintptr_t first; size_t second; bool pinned; };      /* pinned: hipHostRegister has succeeded -- until then the range only blocks overlapping registrations */
std::vector<RegRange> g_reg;   /* [start, bytes), guarded by g_reg_mu */

bool registered(const void *p, size_t bytes)
{
    if (!p || !bytes) return false;
    const uintptr_t a = (uintptr_t)p;
    std::lock_guard<std::mutex> g(g_reg_mu);
    for (const auto &r : g_reg)
        if (r.pinned && a >= r.first && a - r.first <= r.second && bytes <= r.second - (a - r.first)) return true;
    return false;
}

constexpr size_t DIRECT_RUNS_MAX = 64;

/* device -> registered caller memory without the stop in a pinned buffer: blocks whose stored bytes follow one another both on
 * the device and in the caller's memory travel as one copy (a decoded batch in adjacent slots: one copy per part).  More than
 * DIRECT_RUNS_MAX such runs (compressed blocks in worst-case slots: every block its own) are cheaper through the buffers:
 * returns false and has enqueued nothing.  Exactly stored[i] bytes land in slot i, as on the staged way. */
bool direct_download(k4lz4_ctx *ctx, uint8_t *dst, const uint64_t *dstOff, const uint8_t *d_from, const uint64_t *from_off,
                     const int32_t *stored, int64_t n, hipStream_t st, int *rc)
{
    struct Run { uint64_t host, dev, len; };
    std::vector<Run> runs;
    for (int64_t i = 0; i < n; i++) {
        if (stored[i] <= 0) continue;
        if (!runs.empty() && runs.back().host + runs.back().len == dstOff[i] && runs.back().dev + runs.back().len == from_off[i])
            runs.back().len += (uint64_t)stored[i];
        else {
            if (runs.size() == DIRECT_RUNS_MAX) return false;
            runs.push_back(Run{dstOff[i], from_off[i], (uint64_t)stored[i]});
        }
    }
    *rc = K4LZ4_OK;
    for (const Run &r : runs) {
        const hipError_t e = hipMemcpyAsync(dst + r.host, d_from + r.dev, (size_t)r.len, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) { *rc = hip_fail(ctx, e, "hipMemcpyAsync"); break; }
    }
    return true;
}

int run_host_inner(k4lz4_ctx *ctx, Kind kind, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                   uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level,
                   int flags, const DictArgs *hd);

/* A host-pointer call that fails part-way has copies and kernels in flight on the context's queues that use its staging
 * buffers and scratch: they are drained -- and a status bit they may have raised is taken with them -- before the error is
 * returned, so that the next call on the context starts from nothing.  The call's own error message stays. */
void drain_after_failure(k4lz4_ctx *ctx)
{
    const std::string why = ctx->error;
    for (hipStream_t q : {ctx->stream, ctx->copyq, ctx->dlq, ctx->aux, ctx->aux2})
        if (q) (void)hipStreamSynchronize(q);
    (void)hipGetLastError();
    (void)take_device_status(ctx);
    ctx->error = why;
    tl_error = why;
}

/* host-pointer batch: stage, run, scatter */
int run_host(k4lz4_ctx *ctx, Kind kind, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
             uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level,
             int flags, const DictArgs *hd = nullptr)
{
    const int rc = run_host_inner(ctx, kind, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, level, flags, hd);
    if (rc != K4LZ4_OK && ctx) drain_after_failure(ctx);
    return rc;
}

int run_host_inner(k4lz4_ctx *ctx, Kind kind, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                   uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level,
                   int flags, const DictArgs *hd)
{
    int rc = check_batch_args(ctx, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n);
    if (rc != K4LZ4_OK) return rc;
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    const auto tr0 = std::chrono::steady_clock::now();
    auto lap = [&, last = tr0](const char *what) mutable {
        if (!ctx->trace) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[k4lz4 trace] %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - last).count());
        last = now;
    };

    /* source span and compact destination layout */
    uint64_t lo = UINT64_MAX, hi = 0;
    std::vector<uint64_t> h_soff((size_t)n), h_doff((size_t)n);
    std::vector<int32_t> h_cap((size_t)n);
    uint64_t dtotal = 0;
    uint64_t packed_bytes = 0, longest = 0;
    bool ascending = true;                  /* the blocks lie one after the other in the caller's memory, in index order */
    for (int64_t i = 0; i < n; i++) {
        const int32_t len = srcLen[i];
        if (len > 0) {
            if (hi != 0 && srcOff[i] < hi) ascending = false;
            lo = std::min(lo, srcOff[i]);
            hi = std::max(hi, srcOff[i] + (uint64_t)len);
            packed_bytes += ((uint64_t)len + 15u) & ~(uint64_t)15u;
            longest = std::max<uint64_t>(longest, (uint64_t)len);
        }
        h_cap[(size_t)i] = dstCap[i] < 0 ? 0 : dstCap[i];
        h_doff[(size_t)i] = dtotal;
        dtotal += ((uint64_t)h_cap[(size_t)i] + 15u) & ~(uint64_t)15u;
    }
    if (lo == UINT64_MAX) { lo = 0; hi = 0; }
    const size_t span = (size_t)(hi - lo);
    /* blocks that fill less than 7/8 of their span (and each fit a staging chunk) travel packed */
    /* a registered source goes up as it lies (its span, straight from the caller's pages) unless that is over twice the bytes */
    const bool src_reg = span > 0 && !ctx->no_direct && registered(src + lo, span) && (uint64_t)span * 100u <= (uint64_t)ctx->direct_span_pct * packed_bytes;
    const bool packed = !src_reg && span >= 2 * STAGE_CHUNK && packed_bytes + (packed_bytes >> 3) < span && longest <= STAGE_CHUNK;
    {
        uint64_t at = 0;
        for (int64_t i = 0; i < n; i++) {
            const uint64_t len = srcLen[i] > 0 ? (uint64_t)srcLen[i] : 0u;
            h_soff[(size_t)i] = packed ? at : (len ? srcOff[i] - lo : 0);
            at += (len + 15u) & ~(uint64_t)15u;
        }
    }
    /* Two halves (of about equal source bytes) when the call is big: see k4lz4_ctx::copyq.  HC levels and dictionaries keep
     * to one part (their launches size scratch and synchronise on their own). */
    const uint64_t up_bytes = packed ? packed_bytes : (uint64_t)span;
    const bool hc = (kind == KIND_ENCODE || kind == KIND_PICKLE || kind == KIND_WRAP) && level >= K4LZ4_L03_HC;
    /* Encoders: two parts (a part's kernels last as long as their slowest block whatever their number, and the parts' kernels
     * run one after the other).  Decoders, whose kernels are short: four, so that more of the way up and of the way down
     * overlap. */
    bool dst_reg = false;                   /* the caller's slots lie in registered memory: whole runs of them come back in one copy each */
    if (!ctx->no_direct) {
        uint64_t dlo = UINT64_MAX, dhi = 0;
        for (int64_t i = 0; i < n; i++)
            if (h_cap[(size_t)i] > 0) { dlo = std::min(dlo, dstOff[i]); dhi = std::max(dhi, dstOff[i] + (uint64_t)h_cap[(size_t)i]); }
        dst_reg = dlo != UINT64_MAX && registered(dst + dlo, (size_t)(dhi - dlo));
    }
    int nparts = 1;
    int64_t part_lo[MAX_PARTS], part_hi[MAX_PARTS];
    for (int q = 0; q < MAX_PARTS; q++) { part_lo[q] = q ? n : 0; part_hi[q] = n; }
    if (n >= 1024 && up_bytes >= 4 * STAGE_CHUNK && (packed || ascending) && !hc && !(hd && hd->dict)) {
        const bool decode_like = kind == KIND_DECODE || kind == KIND_UNPICKLE;
        /* (a registered destination: no scatter thread to keep fed, so the shorter the first and the last part the better -- eight
         * parts 36.9 GiB/s, six 35.9, four 34.4 on the bench batch; through the buffers eight parts are slower than four, 27 against 29) */
        const int want = decode_like && n >= 2048 && up_bytes >= 8 * STAGE_CHUNK ? (dst_reg && n >= 4096 ? ctx->dec_parts_direct : ctx->dec_parts) : 2;
        int64_t cuts[MAX_PARTS + 1];
        for (int q = 0; q <= MAX_PARTS; q++) cuts[q] = q ? n : 0;
        uint64_t acc = 0;
        int k = 1;
        for (int64_t i = 0; i < n && k < want; i++) {
            acc += srcLen[i] > 0 ? (((uint64_t)srcLen[i] + 15u) & ~(uint64_t)15u) : 0u;
            if (acc >= packed_bytes * (uint64_t)k / (uint64_t)want) cuts[k++] = i + 1;   /* (the blocks' own bytes: a span has its gaps) */
        }
        bool ok = k == want;
        cuts[want] = n;
        for (int q = 0; q < want && ok; q++) ok = cuts[q + 1] - cuts[q] >= 256;
        if (ok) {
            nparts = want;
            for (int q = 0; q < want; q++) { part_lo[q] = cuts[q]; part_hi[q] = cuts[q + 1]; }
        }
    }
    const size_t meta_bytes = (size_t)n * (8 + 4 + 8 + 4 + 4 + 8);
    if ((rc = grow(ctx, &ctx->d_src, &ctx->d_src_cap, span + 64, false)) != K4LZ4_OK) return rc;
    if ((rc = grow(ctx, &ctx->d_dst, &ctx->d_dst_cap, (size_t)dtotal + 64, false)) != K4LZ4_OK) return rc;
    if ((rc = grow(ctx, &ctx->d_meta, &ctx->d_meta_cap, meta_bytes + 64, false)) != K4LZ4_OK) return rc;
    if ((rc = grow(ctx, &ctx->h_len, &ctx->h_len_cap, (size_t)n * 4 + 64, true)) != K4LZ4_OK) return rc;

    uint64_t *d_soff = (uint64_t *)ctx->d_meta;
    uint64_t *d_doff = d_soff + n;
    uint64_t *d_poff = d_doff + n;
    int32_t *d_slen = (int32_t *)(d_poff + n);
    int32_t *d_cap = d_slen + n;
    int32_t *d_out = d_cap + n;
    int32_t *h_len = (int32_t *)ctx->h_len;
    hipStream_t st = ctx->stream;
    hipStream_t cq = nparts > 1 ? ctx->copyq : st;          /* one part: everything in order on the one queue, as ever */
    K4_HIP(ctx, hipMemcpyAsync(d_soff, h_soff.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    K4_HIP(ctx, hipMemcpyAsync(d_doff, h_doff.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    K4_HIP(ctx, hipMemcpyAsync(d_slen, srcLen, (size_t)n * 4, hipMemcpyHostToDevice, st));
    K4_HIP(ctx, hipMemcpyAsync(d_cap, h_cap.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    DictArgs ddev{nullptr, nullptr, nullptr, nullptr};
    std::vector<uint64_t> h_dictoff;
    std::vector<signed char> h_mode;
    if (hd && hd->dict) {
        /* dictionaries: stage their span; prefix-vs-external is decided on the HOST addresses
         * (LL64.dec.cs:531-541: dictStart + dictSize == dest) because staging breaks adjacency */
        uint64_t dlo = UINT64_MAX, dhi = 0;
        h_dictoff.assign((size_t)n, 0);
        h_mode.assign((size_t)n, 0);
        for (int64_t i = 0; i < n; i++) {
            const int32_t len = hd->len[i];
            if (len <= 0) continue;
            dlo = std::min(dlo, hd->off[i]);
            dhi = std::max(dhi, hd->off[i] + (uint64_t)len);
            h_mode[(size_t)i] = hd->dict + hd->off[i] + len == dst + dstOff[i] ? 1 : 2;
        }
        if (dlo != UINT64_MAX) {
            for (int64_t i = 0; i < n; i++) h_dictoff[(size_t)i] = hd->len[i] > 0 ? hd->off[i] - dlo : 0;
            const size_t dspan = (size_t)(dhi - dlo);
            const size_t need = dspan + 64 + (size_t)n * (8 + 4 + 1) + 64;
            if ((rc = grow(ctx, &ctx->d_dict, &ctx->d_dict_cap, need, false)) != K4LZ4_OK) return rc;
            uint8_t *base = ctx->d_dict;
            uint64_t *d_dictoff = (uint64_t *)(base + ((dspan + 63) & ~(size_t)63));
            int32_t *d_dictlen = (int32_t *)(d_dictoff + n);
            signed char *d_mode = (signed char *)(d_dictlen + n);
            K4_HIP(ctx, hipMemcpyAsync(base, hd->dict + dlo, dspan, hipMemcpyHostToDevice, st));
            K4_HIP(ctx, hipMemcpyAsync(d_dictoff, h_dictoff.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
            K4_HIP(ctx, hipMemcpyAsync(d_dictlen, hd->len, (size_t)n * 4, hipMemcpyHostToDevice, st));
            K4_HIP(ctx, hipMemcpyAsync(d_mode, h_mode.data(), (size_t)n, hipMemcpyHostToDevice, st));
            ddev = DictArgs{base, d_dictoff, d_dictlen, d_mode};
        }
    }
    lap("prepare");

    /* ---- The way back, part by part.  What each block produced is packed next to each other on the device (when that saves a
     * tenth or more of the transfer) and comes back through the pinned buffers in chunks cut at block boundaries; exactly
     * outLen[i] bytes land in each caller slot.  With more than one part this runs on a thread of its own (own queue, own
     * pinned buffers, own helper threads) while this thread stages and launches the later parts: PCIe carries both ways at
     * once, and so do the host's copies.  `launched` says how many parts have had their kernels and their ev_len enqueued. ---- */
    const bool raw_negative = (flags & K4LZ4_FLAG_ALLOW_COPY) && kind == KIND_ENCODE;
    std::vector<uint64_t> h_poff((size_t)n);
    std::vector<int32_t> stored((size_t)n);
    if (nparts > 1 && (rc = grow(ctx, &ctx->d_pack, &ctx->d_pack_cap, (size_t)dtotal + 64, false)) != K4LZ4_OK) return rc;
    hipStream_t dq = nparts > 1 ? ctx->dlq : st;
    std::mutex dm;
    std::condition_variable dcv;
    int launched = 0;                       /* guarded by dm */
    bool abandon = false;                   /* the staging side failed: the way back stops waiting */
    std::string dl_error;
    auto download_part = [&](int p, uint64_t &pack_base) -> int {
        const int64_t b0 = part_lo[p], b1 = part_hi[p], cnt = b1 - b0;
        K4_HIP(ctx, hipEventSynchronize(ctx->ev_len[p]));
        memcpy(outLen + b0, h_len + b0, (size_t)cnt * 4);
        uint64_t used = 0, cap_total = 0;
        for (int64_t i = b0; i < b1; i++) {
            const int32_t got = outLen[i];
            int32_t sv = (got < 0 && raw_negative) ? -got : got;   /* raw blocks come back as -length */
            if (sv < 0 || sv > h_cap[(size_t)i]) sv = 0;
            stored[(size_t)i] = sv;
            h_poff[(size_t)i] = pack_base + used;
            used += ((uint64_t)sv + 15u) & ~(uint64_t)15u;
            cap_total += ((uint64_t)h_cap[(size_t)i] + 15u) & ~(uint64_t)15u;
        }
        const uint8_t *d_from = ctx->d_dst;
        const uint64_t *from_off = h_doff.data() + b0;
        if (dq != st) K4_HIP(ctx, hipStreamWaitEvent(dq, ctx->ev_len[p], 0));    /* this part's kernels are through */
        if (cnt > 1 && used + (used >> 3) < cap_total) {
            int rc2;
            if (nparts == 1 && (rc2 = grow(ctx, &ctx->d_pack, &ctx->d_pack_cap, (size_t)dtotal + 64, false)) != K4LZ4_OK) return rc2;
            K4_HIP(ctx, hipMemcpyAsync(d_poff + b0, h_poff.data() + b0, (size_t)cnt * 8, hipMemcpyHostToDevice, dq));
            hipLaunchKernelGGL(k4::k4_compact_kernel, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, dq, ctx->d_dst, d_doff + b0, d_out + b0,
                               ctx->d_pack, d_poff + b0, (long long)cnt, raw_negative ? 1 : 0);
            K4_HIP(ctx, hipGetLastError());
            d_from = ctx->d_pack;
            from_off = h_poff.data() + b0;
        }
        pack_base += used;
        if (dst_reg) {
            int rc3 = K4LZ4_OK;
            if (direct_download(ctx, dst, dstOff + b0, d_from, from_off, stored.data() + b0, cnt, dq, &rc3)) return rc3;
        }
        return staged_download(ctx, dst, dstOff + b0, d_from, from_off, stored.data() + b0, cnt, dq, nparts > 1 ? pool_dl_of(ctx) : pool_of(ctx));
    };
    int dl_rc = K4LZ4_OK;
    auto download_all = [&]() {
        try {      /* it may run as a thread: nothing may escape (std::terminate), and its message is its own (tl_error) */
            (void)hipSetDevice(ctx->device);
            uint64_t pack_base = 0;
            for (int p = 0; p < nparts; p++) {
                {
                    std::unique_lock<std::mutex> lk(dm);
                    dcv.wait(lk, [&] { return launched > p || abandon; });
                    if (launched <= p) return;
                }
                const int r = download_part(p, pack_base);
                if (r != K4LZ4_OK) { dl_rc = r; dl_error = tl_error; return; }
            }
            if (hipStreamSynchronize(dq) != hipSuccess) { (void)hipGetLastError(); dl_rc = K4LZ4_E_HIP; dl_error = "download queue failed"; }
        } catch (const std::bad_alloc &) { dl_rc = K4LZ4_E_NOMEM; dl_error = "download: out of host memory";
        } catch (...) { dl_rc = K4LZ4_E_HIP; dl_error = "download: unexpected exception"; }
    };
    std::thread dl_thread;
    bool threaded = false;
    if (nparts > 1) {
        try { dl_thread = std::thread(download_all); threaded = true; } catch (...) { threaded = false; }   /* no thread to be had: in line, below */
    }
    auto finish = [&](int up_rc) -> int {   /* every way out of the staging loop comes through here */
        if (threaded) {
            { std::lock_guard<std::mutex> g(dm); if (up_rc != K4LZ4_OK) abandon = true; }
            dcv.notify_all();
            dl_thread.join();
        } else if (up_rc == K4LZ4_OK) {
            { std::lock_guard<std::mutex> g(dm); launched = nparts; }
            download_all();
        }
        if (up_rc != K4LZ4_OK) return up_rc;
        if (dl_rc != K4LZ4_OK) return fail(ctx, dl_rc, dl_error);
        return K4LZ4_OK;
    };

    /* ---- up and launch, part by part: the host stages part k + 1 while part k's kernels run ---- */
    for (int p = 0; p < nparts; p++) {
        const int64_t b0 = part_lo[p], b1 = part_hi[p], cnt = b1 - b0;
        if (packed) {
            if ((rc = staged_upload_packed(ctx, ctx->d_src, src, srcOff, srcLen, b0, b1, h_soff.data(), cq)) != K4LZ4_OK) return finish(rc);
        } else {
            /* ascending blocks (or one part): this part's stretch of the span */
            uint64_t a = UINT64_MAX, e = 0;
            for (int64_t i = b0; i < b1; i++)
                if (srcLen[i] > 0) { a = std::min(a, h_soff[(size_t)i]); e = std::max(e, h_soff[(size_t)i] + (uint64_t)srcLen[i]); }
            if (nparts == 1) { a = 0; e = span; }
            if (a != UINT64_MAX && e > a) {
                if (src_reg) {
                    const hipError_t ue = hipMemcpyAsync(ctx->d_src + a, src + lo + a, (size_t)(e - a), hipMemcpyHostToDevice, cq);
                    if (ue != hipSuccess) return finish(hip_fail(ctx, ue, "hipMemcpyAsync"));
                } else if ((rc = staged_upload(ctx, ctx->d_src + a, src + lo + a, (size_t)(e - a), cq)) != K4LZ4_OK) return finish(rc);
            }
        }
        hipError_t he = hipSuccess;
        if (cq != st) {
            he = hipEventRecord(ctx->ev_up[p], cq);
            if (he == hipSuccess) he = hipStreamWaitEvent(st, ctx->ev_up[p], 0);
            if (he != hipSuccess) return finish(hip_fail(ctx, he, "hipEventRecord"));
        }
        DictArgs dpart = ddev;
        /* The kernels' target is the context's staging buffer, and a hostile stream with a match offset of 0 "copies output bytes onto
         * themselves" (LL64.dec.cs:408-418): those bytes stay what the target held.  Decode-like calls therefore start from a zeroed
         * target (this part's range of it; a memset on the device, ~0.1 ms per 256 MB beside the milliseconds of PCIe), so that such
         * bytes are zeros and never what an earlier call of this context left there.  Not in the kernels: carrying the
         * case through decode_block cost the pair kernel five spilled VGPRs and the single-wave kernels a wave per SIMD. */
        if (kind != KIND_ENCODE && kind != KIND_PICKLE && kind != KIND_WRAP) {
            const uint64_t lo_d = h_doff[(size_t)b0];
            const uint64_t hi_d = b1 < n ? h_doff[(size_t)b1] : dtotal;
            if (hi_d > lo_d) { const hipError_t me = hipMemsetAsync(ctx->d_dst + lo_d, 0, (size_t)(hi_d - lo_d), st); if (me != hipSuccess) return finish(hip_fail(ctx, me, "hipMemsetAsync")); }
        }
        rc = launch(ctx, kind, ctx->d_src, d_soff + b0, d_slen + b0, ctx->d_dst, d_doff + b0, d_cap + b0, d_out + b0, cnt, level, flags, st,
                    &dpart, srcLen + b0);
        if (rc != K4LZ4_OK) return finish(rc);
        he = hipMemcpyAsync(h_len + b0, d_out + b0, (size_t)cnt * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipEventRecord(ctx->ev_len[p], st);
        if (he != hipSuccess) return finish(hip_fail(ctx, he, "hipMemcpyAsync"));
        { std::lock_guard<std::mutex> g(dm); launched = p + 1; }
        dcv.notify_all();
        lap(p == 0 ? "up+launch" : "up+launch+");
    }
    rc = finish(K4LZ4_OK);
    lap("down");
    if (rc != K4LZ4_OK) return rc;
    K4_HIP(ctx, hipStreamSynchronize(st));
    if (cq != st) K4_HIP(ctx, hipStreamSynchronize(cq));
    return take_device_status(ctx);
}

int run_device(k4lz4_ctx *ctx, Kind kind, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
               uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level,
               int flags, void *stream, const DictArgs *dd = nullptr)
{
    int rc = check_batch_args(ctx, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n);
    if (rc != K4LZ4_OK) return rc;
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    return launch(ctx, kind, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, level, flags, (hipStream_t)stream, dd);
}

struct CtxDeleter { void operator()(k4lz4_ctx *c) const { k4lz4_ctx_destroy(c); } };
thread_local std::unique_ptr<k4lz4_ctx, CtxDeleter> tl_ctx;

k4lz4_ctx *implicit_ctx()
{
    if (!tl_ctx) {
        k4lz4_ctx *c = nullptr;
        if (k4lz4_ctx_create(&c, -1) != K4LZ4_OK) return nullptr;
        tl_ctx.reset(c);
    }
    return tl_ctx.get();
}

/* batch of one with LLxx-level returns */
int single(Kind kind, const uint8_t *src, uint8_t *dst, int srcLen, int dstCap, int level, int accel = 1, int extra_flags = 0,
           const uint8_t *dict = nullptr, int dictLen = 0)
{
    tl_status = K4LZ4_OK;
    k4lz4_ctx *ctx = implicit_ctx();
    if (!ctx) { tl_status = K4LZ4_E_NO_DEVICE; return kind == KIND_DECODE ? -1 : 0; }
    if (!src || !dst) { tl_status = fail(ctx, K4LZ4_E_ARG, "NULL buffer"); return kind == KIND_DECODE ? -1 : 0; }
    const uint64_t off = 0;
    int32_t slen = srcLen, cap = dstCap, out = 0;
    ctx->accel = accel < 1 ? 1 : accel;
    int32_t dlen = dictLen;
    const DictArgs hd{dict, &off, &dlen, nullptr};
    const int rc = run_host(ctx, kind, src, &off, &slen, dst, &off, &cap, &out, 1, level, K4LZ4_FLAG_RAW_RETURN | extra_flags,
                            dict && dictLen > 0 ? &hd : nullptr);
    ctx->accel = 1;
    tl_status = rc;
    if (rc != K4LZ4_OK) return kind == KIND_DECODE ? -1 : 0;
    return out;
}

/* ---- chained HC streams (LZ4HighChainEncoder, k4lz4_encode_hc_chain_batch) ------------------------------------------------
 * LZ4EncoderBase's ring buffer (Encoders/LZ4EncoderBase.cs: Topup / Encode / Commit -> LZ4_saveDictHC, Engine/LL.high.cs:168) in
 * stream coordinates.  Block k of a stream is LZ4_compress_HC_continue over [s, s + len) with everything since dictLimit in front of
 * it.  The HC tables are a function of the data alone (k4lz4_encode_hc.hpp), so what the block needs of the blocks before it is
 * their bytes: a window from max(dictLimit, s - 65536) on -- no search reaches further back (lowestMatchIndex, LL64.high.cs:93-94)
 * and lowLimit == dictLimit throughout, so the extDict arm is never taken.  Every block of every stream is therefore independent
 * of the others' parses and the whole batch is one launch sequence. */
struct HcChainPlan {
    int64_t nb = 0;
    uint64_t *woff = nullptr, *boff = nullptr, *doff = nullptr;   /* window / block start in src, slot in dst */
    int32_t *wlen = nullptr, *hist = nullptr, *blen = nullptr, *cap = nullptr;
    static constexpr size_t PER_BLOCK = 3 * 8 + 4 * 4;
    void place(uint8_t *base, int64_t n)
    {
        nb = n;
        woff = (uint64_t *)base; boff = woff + n; doff = boff + n;
        wlen = (int32_t *)(doff + n); hist = wlen + n; blen = hist + n; cap = blen + n;
    }
};

/* LZ4EncoderBase's block size: rounded up to a whole KiB, at least 1 KiB (LZ4EncoderBase.cs:23) */
int64_t hc_chain_block_size(int32_t blockSize) { const int64_t b = std::max<int64_t>(blockSize, 1024); return (b + 1023) / 1024 * 1024; }

/* A whole stream as block lengths for the one ring model (k4lz4_chain_encoder.hpp: ce_hc_rows, ce_fast_rows): its `fresh` bytes
 * behind the dictionary are B repeated, then the remainder; none when there are none */
struct WholeLens {
    int64_t fresh, B;
    int64_t count() const { return fresh / B + (fresh % B != 0); }
    int64_t operator[](int64_t j) const { return std::min(B, fresh - j * B); }
};

/* one stream's rows of the table, from row k on, out of its block lengths; block j goes to dstOff + j * k4lz4_compress_bound(B) */
template <class Len>
void hc_chain_rows(HcChainPlan *fill, int64_t k, uint64_t srcOff, uint64_t dstOff, int64_t D, Len len, int64_t count, int64_t B, int64_t extra)
{
    const int64_t slot = B + B / 255 + 16;                            /* k4lz4_compress_bound(B) */
    k4::ce_hc_rows(D, len, count, B, extra, [&](int64_t j, int64_t ws, int64_t pos, int64_t n, int64_t) {
        const int64_t r = k + j;
        fill->woff[r] = srcOff + (uint64_t)ws; fill->boff[r] = srcOff + (uint64_t)pos;
        fill->doff[r] = dstOff + (uint64_t)(j * slot);
        fill->wlen[r] = (int32_t)(pos - ws + n); fill->hist[r] = (int32_t)(pos - ws);
        fill->blen[r] = (int32_t)n; fill->cap[r] = (int32_t)slot;
    });
}

/* counts the blocks (fill == nullptr) or lays the table out in `fill`; the streams' contents start at srcOff[s], their first dictLen[s]
 * bytes are what the encoder's ring buffer already holds (ptr = dictLen, dictLimit at the content's start), block j of stream s goes to
 * dstOff[s] + j * k4lz4_compress_bound(B) */
int hc_chain_table(k4lz4_ctx *ctx, const uint64_t *srcOff, const int64_t *srcLen, const int32_t *blockSize, const int32_t *extraBlocks,
                   const int32_t *dictLen, int64_t nStreams, const uint64_t *dstOff, int64_t &nb, HcChainPlan *fill)
{
    int64_t k = 0;
    for (int64_t si = 0; si < nStreams; si++) {
        const int64_t N = srcLen[si];
        const int64_t B = hc_chain_block_size(blockSize[si]);
        const int64_t extra = extraBlocks ? std::max<int32_t>(extraBlocks[si], 0) : 0;
        const int64_t D = dictLen ? dictLen[si] : 0;
        if (N < 0) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_hc_chain_batch: negative content length");
        if (D < 0 || D > N) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_hc_chain_batch: dictLen outside the content");
        if (B > k4::MAX_INPUT_SIZE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_hc_chain_batch: block size above the input size limit");
        const WholeLens lens{N - D, B};
        /* LZ4_compressHC_continue_generic renormalises once end - base > 2 GB (LL64.high.cs:1271-1276): not offered (the last block starts furthest in) */
        if (lens.count() > 0 && 65536 + D + (lens.count() - 1) * B > ((int64_t)1 << 31))
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_hc_chain_batch: a chained stream longer than 2 GB (the encoder's renormalisation) is not supported");
        if (fill) hc_chain_rows(fill, k, srcOff[si], dstOff[si], D, lens, lens.count(), B, extra);
        k += lens.count();
    }
    nb = k;
    return K4LZ4_OK;
}

/* the same table with explicit block lengths: stream s has blocks lens.len[lens.first[s] .. + lens.count[s]), which may be shorter
 * than B in mid-stream; its content is dictLen[s] bytes and the blocks behind them */
struct ChainLens { const int64_t *first; const int32_t *count; const int32_t *len; };

int hc_chain_table_lens(k4lz4_ctx *ctx, const uint64_t *srcOff, const ChainLens &lens, const int32_t *blockSize, const int32_t *extraBlocks,
                        const int32_t *dictLen, int64_t nStreams, const uint64_t *dstOff, int64_t &nb, HcChainPlan *fill)
{
    int64_t k = 0;
    for (int64_t si = 0; si < nStreams; si++) {
        const int64_t B = hc_chain_block_size(blockSize[si]);
        const int64_t extra = extraBlocks ? std::max<int32_t>(extraBlocks[si], 0) : 0;
        const int64_t D = dictLen ? dictLen[si] : 0;
        const int32_t *len = lens.len + lens.first[si];
        if (D < 0 || lens.count[si] < 0) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: bad block table");
        if (B > k4::MAX_INPUT_SIZE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: block size above the input size limit");
        for (int64_t j = 0; j < lens.count[si]; j++)
            if (len[j] <= 0 || len[j] > B) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: a block length outside 1 .. BlockSize");
        if (fill) hc_chain_rows(fill, k, srcOff[si], dstOff[si], D, len, lens.count[si], B, extra);
        k += lens.count[si];
    }
    nb = k;
    return K4LZ4_OK;
}

/* k4lz4_encode_hc_chain_batch_device: src / dst / outLen device pointers, the per-stream arrays host pointers */
int hc_chain_run(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen, const int32_t *blockSize,
                 const int32_t *extraBlocks, const int32_t *dictLen, int64_t nStreams, uint8_t *dst, const uint64_t *dstOff, int32_t *outLen, int64_t nBlocks,
                 int level, int flags, hipStream_t stream, const ChainLens *lens = nullptr)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (nStreams < 0 || nBlocks < 0 || (nStreams > 0 && (!src || !srcOff || !srcLen || !blockSize || !dst || !dstOff || !outLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (flags & ~(int)K4LZ4_FLAG_ALLOW_COPY) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_hc_chain_batch: the only flag it takes is K4LZ4_FLAG_ALLOW_COPY");
    level = std::max<int>(K4LZ4_L03_HC, std::min<int>(K4LZ4_L12_MAX, level));       /* LZ4HighChainEncoder's constructor */
    int64_t nb = 0;
    auto table = [&](HcChainPlan *fill) {
        return lens ? hc_chain_table_lens(ctx, srcOff, *lens, blockSize, extraBlocks, dictLen, nStreams, dstOff, nb, fill)
                    : hc_chain_table(ctx, srcOff, srcLen, blockSize, extraBlocks, dictLen, nStreams, dstOff, nb, fill);
    };
    int rc = table(nullptr);
    if (rc != K4LZ4_OK) return rc;
    if (nb > nBlocks) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_hc_chain_batch: outLen has fewer entries than the streams have blocks");
    if (nb == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    PlanUpload &plan = ctx->chain_plan;
    const size_t bytes = (size_t)nb * HcChainPlan::PER_BLOCK;
    if ((rc = plan_begin(ctx, plan, bytes, false)) != K4LZ4_OK) return rc;
    HcChainPlan h;
    h.place(plan.host.data(), nb);
    rc = table(&h);
    if (rc != K4LZ4_OK) return rc;
    if ((rc = grow_scratch(ctx, &plan.dev, &plan.cap, bytes)) != K4LZ4_OK) return rc;
    HcChainPlan d;
    d.place(plan.dev, nb);
    if ((rc = plan_send(ctx, plan, plan.dev, bytes, stream)) != K4LZ4_OK) return rc;
    ctx->last_encode_route = K4LZ4_ENCODE_ROUTE_NONE;    /* (this call reaches launch_hc without passing launch_inner) */
    rc = launch_hc(ctx, ENV_NONE, src, d.woff, d.wlen, dst, d.doff, d.cap, outLen, nb, level, 0, stream, h.wlen, d.hist);
    if (rc == K4LZ4_OK && (flags & K4LZ4_FLAG_ALLOW_COPY)) {
        /* LZ4EncoderBase.Encode(allowCopy): a block that did not shrink is stored raw -- its bytes stay in the history all the same */
        for (int64_t first = 0; first < nb; first += (int64_t)1 << 24) {
            const int64_t cnt = std::min<int64_t>((int64_t)1 << 24, nb - first);
            k4::BatchArgs a{};
            a.src = src; a.srcOff = d.boff + first; a.srcLen = d.blen + first;
            a.dst = dst; a.dstOff = d.doff + first; a.dstCap = d.cap + first; a.outLen = outLen + first; a.n = cnt;
            hipLaunchKernelGGL(k4::k4_allow_copy_kernel, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, stream, a);
        }
        if (hipGetLastError() != hipSuccess) rc = fail(ctx, K4LZ4_E_HIP, "k4_allow_copy_kernel launch failed");
    }
    mark_busy(ctx, stream);
    return rc;
}

/* ---- chained fast streams (LZ4FastChainEncoder, k4lz4_encode_fast_chain_batch) ----------------------------------------------
 * LZ4EncoderBase's ring buffer (Topup / Encode / Commit -> LZ4_saveDict, Engine/LL.tools.cs:195-213) in content coordinates, as for
 * HC above.  What differs: the table holds the positions the parse visited, so a stream's blocks are encoded in order by one wave
 * that keeps the table (k4lz4_fast_chain.hpp); per block the kernel needs its start, length and dictSize -- the ring's _inputIndex,
 * which LZ4_compress_generic adds every block to (withPrefix64k; the first call's extDict arm sets it to the block's length, the
 * same number) and LZ4_saveDict cuts to 64 KiB. */
struct FastChainPlan {
    int64_t ns = 0, nb = 0;
    uint32_t *ticket = nullptr;
    uint64_t *soff = nullptr, *slen = nullptr, *doff = nullptr;
    int64_t *first = nullptr;
    uint32_t *nblk = nullptr, *idx0 = nullptr, *dict_end = nullptr, *order = nullptr, *bpos = nullptr, *bdict = nullptr;
    int32_t *blen = nullptr, *cap = nullptr;
    static size_t bytes(int64_t ns, int64_t nb) { return 16 + (size_t)ns * (3 * 8 + 4 * 4) + (size_t)nb * (8 + 4 * 4); }
    void place(uint8_t *base, int64_t s, int64_t b)
    {
        ns = s; nb = b;
        ticket = (uint32_t *)base;
        soff = (uint64_t *)(base + 16); slen = soff + s; first = (int64_t *)(slen + s); doff = (uint64_t *)(first + s);
        nblk = (uint32_t *)(doff + b); idx0 = nblk + s; dict_end = idx0 + s; order = dict_end + s;
        bpos = order + s; blen = (int32_t *)(bpos + b); bdict = (uint32_t *)(blen + b); cap = (int32_t *)(bdict + b);
    }
};

/* stream si's words and its rows of the table, from row k on, out of its block lengths (`total` bytes in all); cur: its currentOffset */
template <class Len>
void fast_chain_rows(FastChainPlan *fill, int64_t si, int64_t k, uint64_t srcOff, uint64_t dstOff, int64_t D, int64_t cur, Len len, int64_t count,
                     int64_t total, int64_t B, int64_t extra)
{
    const int64_t slot = B + B / 255 + 16;                            /* k4lz4_compress_bound(B) */
    const int64_t dict = k4::ce_fast_rows(D, cur, len, count, B, extra, [&](int64_t j, int64_t pos, int64_t n, int64_t d, bool) {
        const int64_t r = k + j;
        fill->bpos[r] = (uint32_t)pos; fill->blen[r] = (int32_t)n; fill->bdict[r] = (uint32_t)d;
        fill->doff[r] = dstOff + (uint64_t)(j * slot); fill->cap[r] = (int32_t)slot;
    });
    fill->soff[si] = srcOff; fill->slen[si] = (uint64_t)(D + total); fill->first[si] = k; fill->nblk[si] = (uint32_t)count;
    fill->idx0[si] = (uint32_t)(cur - D); fill->dict_end[si] = (uint32_t)dict;
}

/* counts the blocks (fill == nullptr) or lays the table out in `fill`.  cur0 / sdict: the streams' state (currentOffset, dictSize), or
 * nullptr for fresh streams; the content's first dictLen[s] bytes are what the ring buffer holds (dictLen == dictSize) */
int fast_chain_table(k4lz4_ctx *ctx, const uint64_t *srcOff, const int64_t *srcLen, const int32_t *blockSize, const int32_t *extraBlocks,
                     const int32_t *dictLen, const uint32_t *cur0, const uint32_t *sdict, int64_t nStreams, const uint64_t *dstOff, int64_t &nb,
                     FastChainPlan *fill)
{
    int64_t k = 0;
    for (int64_t si = 0; si < nStreams; si++) {
        const int64_t N = srcLen[si];
        const int64_t B = hc_chain_block_size(blockSize[si]);
        const int64_t extra = extraBlocks ? std::max<int32_t>(extraBlocks[si], 0) : 0;
        const int64_t D = dictLen ? dictLen[si] : 0;
        if (N < 0) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_fast_chain_batch: negative content length");
        if (D < 0 || D > N) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_fast_chain_batch: dictLen outside the content");
        if (B > k4::MAX_INPUT_SIZE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_fast_chain_batch: block size above the input size limit");
        int64_t cur = 0;
        if (cur0) {
            if ((int64_t)sdict[si] != D) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_fast_chain_batch: dictLen differs from the state's dictSize");
            if (sdict[si] > cur0[si]) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_fast_chain_batch: a state whose dictSize exceeds its currentOffset");
            cur = cur0[si];
        } else if (D != 0) {
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_fast_chain_batch: dictLen without a state (the table is what continues a stream)");
        }
        const WholeLens lens{N - D, B};
        /* LZ4_renormDictT (LL64.tools.cs:157-173) rescales the table once currentOffset + inputSize > 2 GB: not offered (the last block ends furthest in) */
        if (lens.count() > 0 && N - D > ((int64_t)1 << 31) - cur)
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_fast_chain_batch: a chained stream longer than 2 GB (the encoder's renormalisation) is not supported");
        if (fill) fast_chain_rows(fill, si, k, srcOff[si], dstOff[si], D, cur, lens, lens.count(), N - D, B, extra);
        k += lens.count();
    }
    nb = k;
    return K4LZ4_OK;
}

/* the same table with explicit block lengths (ce_fast_rows), as hc_chain_table_lens */
int fast_chain_table_lens(k4lz4_ctx *ctx, const uint64_t *srcOff, const ChainLens &lens, const int32_t *blockSize, const int32_t *extraBlocks,
                          const int32_t *dictLen, const uint32_t *cur0, const uint32_t *sdict, int64_t nStreams, const uint64_t *dstOff,
                          int64_t &nb, FastChainPlan *fill)
{
    int64_t k = 0;
    for (int64_t si = 0; si < nStreams; si++) {
        const int64_t B = hc_chain_block_size(blockSize[si]);
        const int64_t extra = extraBlocks ? std::max<int32_t>(extraBlocks[si], 0) : 0;
        const int64_t D = dictLen ? dictLen[si] : 0;
        const int32_t *len = lens.len + lens.first[si];
        if (D < 0 || lens.count[si] < 0 || !cur0 || !sdict) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: bad block table");
        if ((int64_t)sdict[si] != D || sdict[si] > cur0[si]) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: a state that does not fit its ring");
        if (B > k4::MAX_INPUT_SIZE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: block size above the input size limit");
        int64_t total = 0;
        for (int64_t j = 0; j < lens.count[si]; j++) {
            if (len[j] <= 0 || len[j] > B) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: a block length outside 1 .. BlockSize");
            total += len[j];
        }
        if ((int64_t)cur0[si] + total > ((int64_t)1 << 31))
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: a chained stream longer than 2 GB (the encoder's renormalisation) is not supported");
        if (fill) fast_chain_rows(fill, si, k, srcOff[si], dstOff[si], D, (int64_t)cur0[si], len, lens.count[si], total, B, extra);
        k += lens.count[si];
    }
    nb = k;
    return K4LZ4_OK;
}

int fast_chain_flags(k4lz4_ctx *ctx, int flags)
{
    if ((flags & K4LZ4_FLAG_X32) || g_enforce32.load(std::memory_order_relaxed))
        return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_fast_chain_batch: the 32-bit engine's chained encoder (LZ4Codec.Enforce32) is not supported");
    if (flags & ~(int)K4LZ4_FLAG_ALLOW_COPY) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_fast_chain_batch: the only flag it takes is K4LZ4_FLAG_ALLOW_COPY");
    return K4LZ4_OK;
}

/* src / dst / outLen / states: device pointers; the per-stream arrays and cur0 / sdict (the input states' two indices): host */
int fast_chain_run(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen, const int32_t *blockSize,
                   const int32_t *extraBlocks, const int32_t *dictLen, const uint32_t *cur0, const uint32_t *sdict, int64_t nStreams,
                   const k4lz4_fast_chain_state *stateIn, k4lz4_fast_chain_state *stateOut, uint8_t *dst, const uint64_t *dstOff,
                   int32_t *outLen, int64_t nBlocks, int flags, hipStream_t stream, const ChainLens *lens = nullptr)
{
    int64_t nb = 0;
    auto table = [&](FastChainPlan *fill) {
        return lens ? fast_chain_table_lens(ctx, srcOff, *lens, blockSize, extraBlocks, dictLen, cur0, sdict, nStreams, dstOff, nb, fill)
                    : fast_chain_table(ctx, srcOff, srcLen, blockSize, extraBlocks, dictLen, cur0, sdict, nStreams, dstOff, nb, fill);
    };
    int rc = table(nullptr);
    if (rc != K4LZ4_OK) return rc;
    if (nb > nBlocks) return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_fast_chain_batch: outLen has fewer entries than the streams have blocks");
    if (nStreams == 0 || (nb == 0 && !stateOut)) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    PlanUpload &plan = ctx->chain_plan;
    const size_t bytes = FastChainPlan::bytes(nStreams, nb);
    if ((rc = plan_begin(ctx, plan, bytes, true)) != K4LZ4_OK) return rc;
    FastChainPlan h;
    h.place(plan.host.data(), nStreams, nb);
    rc = table(&h);
    if (rc != K4LZ4_OK) return rc;
    {   /* longest first: a wave that is done takes the next stream (the ticket) */
        std::vector<uint32_t> ord((size_t)nStreams);
        for (int64_t si = 0; si < nStreams; si++) ord[(size_t)si] = (uint32_t)si;
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return srcLen[x] - (dictLen ? dictLen[x] : 0) > srcLen[y] - (dictLen ? dictLen[y] : 0); });
        memcpy(h.order, ord.data(), ord.size() * 4);
    }
    if ((rc = grow_scratch(ctx, &plan.dev, &plan.cap, bytes)) != K4LZ4_OK) return rc;
    FastChainPlan d;
    d.place(plan.dev, nStreams, nb);
    if ((rc = plan_send(ctx, plan, plan.dev, bytes, stream)) != K4LZ4_OK) return rc;
    k4::FastChainArgs a{};
    a.src = src; a.soff = d.soff; a.slen = d.slen; a.first = d.first; a.nblk = d.nblk; a.idx0 = d.idx0; a.dict_end = d.dict_end; a.order = d.order;
    a.bpos = d.bpos; a.blen = d.blen; a.bdict = d.bdict; a.doff = d.doff; a.cap = d.cap; a.dst = dst; a.outLen = outLen;
    a.state_in = (const k4::FastChainState *)stateIn; a.state_out = (k4::FastChainState *)stateOut;
    a.ticket = d.ticket; a.n = nStreams; a.allow_copy = (flags & K4LZ4_FLAG_ALLOW_COPY) ? 1 : 0;
    const int64_t wgs = std::min<int64_t>((nStreams + k4::FAST_CHAIN_WAVES_PER_WG - 1) / k4::FAST_CHAIN_WAVES_PER_WG, ctx->cu_count);
    hipLaunchKernelGGL(k4::k4_fast_chain_kernel, dim3((unsigned)wgs), dim3(64 * k4::FAST_CHAIN_WAVES_PER_WG), 0, stream, a);
    if (hipGetLastError() != hipSuccess) rc = fail(ctx, K4LZ4_E_HIP, "k4_fast_chain_kernel launch failed");
    mark_busy(ctx, stream);
    return rc;
}

/* the two indices of every input state, from the host's copy (or nullptr) */
void fast_chain_indices(const k4lz4_fast_chain_state *st, int64_t n, std::vector<uint32_t> &cur0, std::vector<uint32_t> &sdict)
{
    cur0.resize((size_t)n); sdict.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) { cur0[(size_t)i] = st[i].currentOffset; sdict[(size_t)i] = st[i].dictSize; }
}

/* ---- frame reader scratch (k4lz4_frame_read.hpp): per-frame words behind 64 bytes of counters, and the block table.
 * Grow-only; a table that has to grow waits for the context's earlier work first (grow frees the old one). */
constexpr size_t FRAME_BYTES = 8 * 8 + 10 * 4 + 1, BLOCK_BYTES = 3 * 8 + 8 * 4;

int frame_scratch(k4lz4_ctx *ctx, int64_t n, k4::FrameTab *t, unsigned long long **counters)
{
    int rc;
    if ((rc = grow_scratch(ctx, &ctx->d_fr, &ctx->d_fr_cap, 64 + (size_t)n * FRAME_BYTES + 64)) != K4LZ4_OK) return rc;
    uint8_t *m = ctx->d_fr;
    const size_t w8 = (size_t)n * 8, w4 = (size_t)n * 4;
    *counters = (unsigned long long *)m;         m += 64;
    t->bound = (uint64_t *)m;                    m += w8;
    t->demand = (uint64_t *)m;                   m += w8;
    t->clen = (uint64_t *)m;                     m += w8;
    t->first = (uint64_t *)m;                    m += w8;
    t->produced = (uint64_t *)m;                 m += w8;
    t->hashLen = (uint64_t *)m;                  m += w8;
    t->res = (int64_t *)m;                       m += w8;
    t->serialOut = (int64_t *)m;                 m += w8;
    t->nblk = (uint32_t *)m;                     m += w4;
    t->status = (int32_t *)m;                    m += w4;
    t->desc = (uint32_t *)m;                     m += w4;
    t->bsize = (int32_t *)m;                     m += w4;
    t->csum = (uint32_t *)m;                     m += w4;
    t->hdrEnd = (uint32_t *)m;                   m += w4;
    t->kbad = (uint32_t *)m;                     m += w4;
    t->irregular = (uint32_t *)m;                m += w4;
    t->nSerial = (uint32_t *)m;                  m += w4;
    t->sum = (uint32_t *)m;                      m += w4;
    t->chained = m;
    return K4LZ4_OK;
}

int block_scratch(k4lz4_ctx *ctx, int64_t nb, k4::BlockTab *b)
{
    int rc;
    if ((rc = grow_scratch(ctx, &ctx->d_fb, &ctx->d_fb_cap, (size_t)std::max<int64_t>(nb, 1) * BLOCK_BYTES + 64)) != K4LZ4_OK) return rc;
    uint8_t *m = ctx->d_fb;
    const size_t w8 = (size_t)std::max<int64_t>(nb, 1) * 8, w4 = w8 / 2;
    b->off = (uint64_t *)m;                      m += w8;
    b->hlen = (uint64_t *)m;                     m += w8;
    b->dstOff = (uint64_t *)m;                   m += w8;
    b->len = (uint32_t *)m;                      m += w4;
    b->owner = (uint32_t *)m;                    m += w4;
    b->idx = (uint32_t *)m;                      m += w4;
    b->sum = (uint32_t *)m;                      m += w4;
    b->got = (uint32_t *)m;                      m += w4;
    b->srcLen = (int32_t *)m;                    m += w4;
    b->dstCap = (int32_t *)m;                    m += w4;
    b->outLen = (int32_t *)m;
    return K4LZ4_OK;
}

/* ---- legacy formats (k4lz4_legacy.hpp): grow-only scratch, grown by grow_scratch */
constexpr size_t LG_STREAM_BYTES = 4 * 8 + 4, LG_ROW_BYTES = 48;

/* per-stream words behind 64 bytes of counters: four u64 arrays and one 32-bit array */
int lg_streams(k4lz4_ctx *ctx, int64_t n, unsigned long long **cnt, uint64_t *w[4], int32_t **w32)
{
    int rc;
    if ((rc = grow_scratch(ctx, &ctx->d_lg, &ctx->d_lg_cap, 64 + (size_t)n * LG_STREAM_BYTES + 64)) != K4LZ4_OK) return rc;
    uint8_t *m = ctx->d_lg;
    *cnt = (unsigned long long *)m;
    m += 64;
    for (int i = 0; i < 4; i++, m += (size_t)n * 8) w[i] = (uint64_t *)m;
    *w32 = (int32_t *)m;
    return K4LZ4_OK;
}

/* ---- the host-pointer forms of the stream calls: one staging path.  A call lays out its inputs in ctx->d_src (span(): one
 * span of the caller's buffer, offsets rebased; pack(): every stream's content at a 16-byte step), its output slots at 16-byte
 * steps at the same offsets of ctx->d_dst and ctx->h_stage (slots()) and its per-item arrays at 16-byte steps of ctx->d_meta
 * (meta(): uploaded from a host array, or left for the kernels).  upload() grows the buffers, then queues the copies; the call
 * runs its device form on st; finish() queues the downloads, synchronises once, takes the status word and copies each item's
 * bytes into the caller's slot.  A stage that has queued work and is left without a finished synchronisation -- any failure
 * after the first enqueue -- drains the context on the way out. */
struct HostStage {
    struct Down { void *host; const void *dev; size_t bytes; };
    struct Up { uint8_t **base; uint64_t at; const void *host; size_t bytes; };       /* base: &ctx->d_src or &ctx->d_meta */
    k4lz4_ctx *const ctx;
    const hipStream_t st;
    std::vector<uint64_t> in_off, slot;     /* per item: its input's offset in d_src, its output slot's in d_dst / h_stage */
    std::vector<Up> ups;
    std::vector<std::function<void()>> places;
    uint64_t in_bytes = 0, out_bytes = 0, meta_bytes = 0;
    bool zero = false, queued = false, done = false;

    explicit HostStage(k4lz4_ctx *c) : ctx(c), st(c->stream) {}
    ~HostStage() { if (queued && !done) drain_after_failure(ctx); }
    template <class Len> void span(const uint8_t *s, const uint64_t *off, int64_t n, Len len)
    {
        uint64_t lo = UINT64_MAX, hi = 0;
        for (int64_t i = 0; i < n; i++)
            if (len(i)) { lo = std::min(lo, off[i]); hi = std::max(hi, off[i] + len(i)); }
        if (lo == UINT64_MAX) lo = hi = 0;
        in_off.assign((size_t)n, 0);
        for (int64_t i = 0; i < n; i++) if (len(i)) in_off[(size_t)i] = off[i] - lo;
        in_bytes = hi - lo;
        ups.push_back(Up{&ctx->d_src, 0, s + lo, (size_t)in_bytes});
    }
    void pack(const uint8_t *s, const uint64_t *off, const int64_t *len, int64_t n)
    {
        in_off.resize((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            in_off[(size_t)i] = in_bytes;
            ups.push_back(Up{&ctx->d_src, in_bytes, s + off[i], (size_t)std::max<int64_t>(len[i], 0)});
            in_bytes += ((uint64_t)len[i] + 15u) & ~(uint64_t)15u;
        }
    }
    /* clear: the slots start as zeros (a hostile stream's offset-0 matches leave zeros, not an earlier call's bytes: see run_host_inner) */
    template <class Cap> void slots(int64_t n, Cap cap, bool clear)
    {
        slot.resize((size_t)n);
        for (int64_t i = 0; i < n; i++) { slot[(size_t)i] = out_bytes; out_bytes += ((uint64_t)cap(i) + 15u) & ~(uint64_t)15u; }
        zero = clear;
    }
    template <class T> void meta(T **p, int64_t count, const void *host = nullptr)
    {
        const uint64_t at = meta_bytes;
        places.push_back([this, p, at] { *p = (T *)(ctx->d_meta + at); });
        ups.push_back(Up{&ctx->d_meta, at, host, host ? (size_t)count * sizeof(T) : 0});
        meta_bytes += ((uint64_t)count * sizeof(T) + 15u) & ~(uint64_t)15u;
    }
    int upload()
    {
        int rc;
        if ((rc = grow(ctx, &ctx->d_src, &ctx->d_src_cap, (size_t)in_bytes + 64, false)) != K4LZ4_OK ||
            (rc = grow(ctx, &ctx->d_meta, &ctx->d_meta_cap, (size_t)meta_bytes + 64, false)) != K4LZ4_OK ||
            (!slot.empty() && ((rc = grow(ctx, &ctx->d_dst, &ctx->d_dst_cap, (size_t)out_bytes + 64, false)) != K4LZ4_OK ||
                               (rc = grow(ctx, &ctx->h_stage, &ctx->h_stage_cap, (size_t)out_bytes + 64, true)) != K4LZ4_OK)))
            return rc;
        for (const auto &place : places) place();
        queued = true;
        for (const Up &u : ups)
            if (u.bytes) K4_HIP(ctx, hipMemcpyAsync(*u.base + u.at, u.host, u.bytes, hipMemcpyHostToDevice, st));
        if (zero && out_bytes) K4_HIP(ctx, hipMemsetAsync(ctx->d_dst, 0, (size_t)out_bytes, st));
        return K4LZ4_OK;
    }
    /* bytes(i): how many bytes of item i's slot go to dst + dstOff[i] */
    int finish(std::initializer_list<Down> results, uint8_t *dst = nullptr, const uint64_t *dstOff = nullptr,
               const std::function<size_t(int64_t)> &bytes = nullptr)
    {
        for (const Down &d : results)
            if (d.bytes) K4_HIP(ctx, hipMemcpyAsync(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost, st));
        if (out_bytes) K4_HIP(ctx, hipMemcpyAsync(ctx->h_stage, ctx->d_dst, (size_t)out_bytes, hipMemcpyDeviceToHost, st));
        K4_HIP(ctx, hipStreamSynchronize(st));
        done = true;
        const int rc = take_device_status(ctx);
        for (size_t i = 0; rc == K4LZ4_OK && bytes && i < slot.size(); i++)
            if (const size_t b = bytes((int64_t)i)) memcpy(dst + dstOff[i], ctx->h_stage + slot[i], b);
        return rc;
    }
};

/* the chained encoders' host forms after their argument checks.  table(nb) counts the blocks (host arithmetic: before the
 * context); the contents go up packed, every stream's block slots lie behind each other, the states in the tail of the
 * metadata; run(s, nb, d_out, d_in, d_outst) is the device form; exactly |outLen| bytes of every block's slot go to the caller's */
template <class Table, class Run>
int chain_host(k4lz4_ctx *ctx, const char *what, Table table, Run run, const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen,
               const int32_t *blockSize, const int32_t *dictLen, int64_t nStreams, const k4lz4_fast_chain_state *stateIn,
               k4lz4_fast_chain_state *stateOut, uint8_t *dst, const uint64_t *dstOff, int32_t *outLen, int64_t nBlocks)
{
    int64_t nb = 0;
    int rc = table(nb);
    if (rc != K4LZ4_OK) return rc;
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (nb > nBlocks) return fail(ctx, K4LZ4_E_ARG, std::string(what) + ": outLen has fewer entries than the streams have blocks");
    if (nStreams == 0 || (nb == 0 && !stateOut)) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    HostStage s(ctx);
    s.pack(src, srcOff, srcLen, nStreams);
    auto fresh = [&](int64_t si) { return srcLen[si] - (dictLen ? dictLen[si] : 0); };     /* (validated by the block table) */
    s.slots(nStreams, [&](int64_t si) {
        const uint64_t B = (uint64_t)hc_chain_block_size(blockSize[si]);
        return ((uint64_t)fresh(si) + B - 1u) / B * (B + B / 255 + 16);
    }, false);
    int32_t *d_out;
    k4lz4_fast_chain_state *d_in = nullptr, *d_outst = nullptr;
    s.meta(&d_out, nb);
    if (stateIn) s.meta(&d_in, nStreams, stateIn);
    if (stateOut) s.meta(&d_outst, nStreams);
    if ((rc = s.upload()) != K4LZ4_OK || (rc = run(s, nb, d_out, d_in, d_outst)) != K4LZ4_OK ||
        (rc = s.finish({{outLen, d_out, (size_t)nb * 4}, {stateOut, d_outst, stateOut ? (size_t)nStreams * sizeof(*stateOut) : 0}})) != K4LZ4_OK)
        return rc;
    int64_t k = 0;
    for (int64_t si = 0; si < nStreams; si++) {
        const int64_t B = hc_chain_block_size(blockSize[si]), slot = B + B / 255 + 16;
        for (int64_t j = 0; j * B < fresh(si); j++, k++)
            if (outLen[k]) memcpy(dst + dstOff[si] + (uint64_t)(j * slot), ctx->h_stage + s.slot[(size_t)si] + (uint64_t)(j * slot),
                                  (size_t)std::abs((int64_t)outLen[k]));
    }
    return K4LZ4_OK;
}

/* the size calls (k4lz4_frame_sizes, k4lz4_legacy_stream_sizes): the streams' span up, their sizes and statuses down */
template <class Device>
int host_sizes(Device device, k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *off, const uint64_t *len, int64_t n,
               uint64_t *outSize, int32_t *outStatus)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!src || !off || !len || !outSize || !outStatus))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    HostStage s(ctx);
    s.span(src, off, n, [&](int64_t i) { return len[i]; });
    uint64_t *d_off, *d_len, *d_size;
    int32_t *d_status;
    s.meta(&d_off, n, s.in_off.data()); s.meta(&d_len, n, len); s.meta(&d_size, n); s.meta(&d_status, n);
    int rc;
    if ((rc = s.upload()) != K4LZ4_OK || (rc = device(ctx, ctx->d_src, d_off, d_len, n, d_size, d_status, s.st)) != K4LZ4_OK)
        return rc;
    return s.finish({{outSize, d_size, (size_t)n * 8}, {outStatus, d_status, (size_t)n * 4}});
}

/* the slot-filling stream calls with u64 offsets, lengths and capacities (k4lz4_decode_frames, the legacy streams' encoder and
 * decoder); device(ctx, src, off, len, n, dst, dstOff, dstCap, outLen, stream) is the device form.  zero: the slots start as
 * zeros (the decoders); capped: an outLen beyond the slot's capacity copies nothing */
template <class Device>
int host_streams(Device device, k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *off, const uint64_t *len, int64_t n,
                 uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen, bool zero, bool capped)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!src || !off || !len || !dst || !dstOff || !dstCap || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    HostStage s(ctx);
    s.span(src, off, n, [&](int64_t i) { return len[i]; });
    s.slots(n, [&](int64_t i) { return dstCap[i]; }, zero);
    uint64_t *d_off, *d_len, *d_doff, *d_dcap;
    int64_t *d_out;
    s.meta(&d_off, n, s.in_off.data()); s.meta(&d_len, n, len); s.meta(&d_doff, n, s.slot.data()); s.meta(&d_dcap, n, dstCap);
    s.meta(&d_out, n);
    int rc;
    if ((rc = s.upload()) != K4LZ4_OK || (rc = device(ctx, ctx->d_src, d_off, d_len, n, ctx->d_dst, d_doff, d_dcap, d_out, s.st)) != K4LZ4_OK)
        return rc;
    return s.finish({{outLen, d_out, (size_t)n * 8}}, dst, dstOff, [&](int64_t i) {
        return outLen[i] > 0 && (!capped || (uint64_t)outLen[i] <= dstCap[i]) ? (size_t)outLen[i] : 0;
    });
}

/* ---- the incremental readers and the per-stream queries: one device form, one host form, one query pair.
 * The direct path's tables come out of ctx->d_frd at 64-byte steps.  A layout runs twice over the same Carve calls: without a base
 * it measures what grow_scratch is asked for, with one it places the pointers -- the size cannot fall behind the arrays. */
struct Carve {
    uint8_t *const base;
    size_t at = 0;
    template <class T> void take(T *&p, size_t count)
    {
        p = base ? (T *)(base + at) : nullptr;
        at += (count * sizeof(T) + 63) & ~(size_t)63;
    }
};

/* the end of a host form whose items are blocks in slots of dstCap bytes: outLen comes down, and of every slot the outLen bytes
 * if they fit */
int finish_blocks(HostStage &s, int32_t *outLen, const int32_t *d_out, int64_t n, uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap)
{
    return s.finish({{outLen, d_out, (size_t)n * 4}}, dst, dstOff,
                    [&](int64_t i) { return outLen[i] > 0 && outLen[i] <= dstCap[i] ? (size_t)outLen[i] : 0; });
}

/* ---- messages against shared dictionaries: k4lz4_encode_dict_batch below level 3 (k4lz4_dict_encode.hpp),
 * k4lz4_encode_dict_hc_batch at levels 3 - 9 (k4lz4_dict_encode_hc.hpp), k4lz4_encode_dictset_batch at both against a
 * k4lz4_dict_set (k4lz4_dict_set.hpp); each in a host form and a device form.  They are one path: what differs between the two
 * families of levels stands in DictFamily, and a call's own list differs from a set in where dict_encode_run takes the tables
 * and the entries' words from. */
struct DictList {
    std::vector<uint64_t> keptOff;            /* per entry */
    std::vector<uint32_t> keptLen, table;
    std::vector<uint32_t> rep;                /* per table: an entry that has it */
};

/* a call's messages, output slots and indices: the caller's pointers, or in the run device pointers */
struct DictBatch {
    const uint8_t *src; const uint64_t *srcOff; const int32_t *srcLen;
    uint8_t *dst; const uint64_t *dstOff; const int32_t *dstCap;
    int32_t *outLen; int64_t n; const int32_t *dictIdx;
};

/* where a call's dictionaries come from: a set, or its own list (dict: the buffer the list's offsets refer to) */
struct DictSource {
    bool of_set;
    const k4lz4_dict_set *set;
    const uint8_t *dict; const uint64_t *dictOff; const int32_t *dictLen; int32_t nDict;
};

/* a family's scratch (k4lz4_ctx::DictScratch::plan.dev), at 64-byte steps in this order: [ticket, hist] [tables] [per table: keptOff,
 * keptLen] [per entry: keptOff, keptLen, table] [cost[n], order[n]] [wave slots].  What goes up from the host lies between the
 * tables and cost[].  A call against a set finds tables and words in the set: nt = nd = 0, and those parts take no room. */
constexpr size_t DICT_HEAD_WORDS = 64 + 2 * k4::COST_BUCKETS + 16;
struct DictLayout {
    uint32_t *head;
    uint8_t *tables;
    uint64_t *toff; uint32_t *tlen; uint64_t *eoff; uint32_t *elen, *etab;
    uint32_t *cost, *order;
    uint8_t *slots;
};

/* what the encode kernels read of the dictionaries: the kept bytes' buffer, the entries' words, the tables */
struct DictTables { const uint8_t *dict; const uint64_t *eoff; const uint32_t *elen, *etab; const uint8_t *tables; int nd; };

constexpr int DHC_WGS_PER_CU = 2;      /* eight waves per CU: the wave slots' tables are 256 KiB each */

void dict_fast_load(hipStream_t st, unsigned nt, const uint8_t *dict, const uint64_t *toff, const uint32_t *tlen, uint8_t *tables)
{
    hipLaunchKernelGGL(k4::k4_dict_load_kernel, dim3(nt), dim3(k4::DICT_LOAD_THREADS), 0, st, k4::DictLoadArgs{dict, toff, tlen, (uint32_t *)tables});
}
void dict_hc_load(hipStream_t st, unsigned nt, const uint8_t *dict, const uint64_t *toff, const uint32_t *tlen, uint8_t *tables)
{
    hipLaunchKernelGGL(k4::k4_dict_hc_load_kernel, dim3(nt), dim3(k4::DHC_LOAD_THREADS), 0, st, k4::DictHcLoadArgs{dict, toff, tlen, tables});
}
void dict_fast_encode(hipStream_t st, unsigned wgs, const DictBatch &b, const DictTables &t, const DictLayout &w, uint32_t *status, int)
{
    k4::DictEncArgs a{b.src, b.srcOff, b.srcLen, b.dst, b.dstOff, b.dstCap, b.outLen, b.dictIdx, t.dict, t.eoff, t.elen, t.etab,
                      (const uint32_t *)t.tables, w.order, w.head, status, b.n, t.nd};
    hipLaunchKernelGGL(k4::k4_dict_encode_kernel, dim3(wgs), dim3(64 * k4::FAST_CHAIN_WAVES_PER_WG), 0, st, a);
}
void dict_hc_encode(hipStream_t st, unsigned wgs, const DictBatch &b, const DictTables &t, const DictLayout &w, uint32_t *status, int level)
{
    k4::DictHcEncArgs a{b.src, b.srcOff, b.srcLen, b.dst, b.dstOff, b.dstCap, b.outLen, b.dictIdx, t.dict, t.eoff, t.elen, t.etab,
                        t.tables, w.slots, w.order, w.head, status, b.n, t.nd, level};
    hipLaunchKernelGGL(k4::k4_dict_hc_encode_kernel, dim3(wgs), dim3(64 * k4::DHC_WAVES_PER_WG), 0, st, a);
}

/* what differs between the fast levels (LZ4_loadDict + LZ4_compress_fast_continue) and the HC levels (LZ4_loadDictHC +
 * LZ4_compress_HC_continue) */
struct DictFamily {
    const char *who;               /* the entry point that takes a list, for messages */
    const char *other_levels;       /* how it refuses the other family's levels */
    uint32_t min_kept;              /* the shortest dictionary of which anything is kept (LZ4_loadDict: HASH_UNIT; LZ4_loadDictHC: a byte) */
    size_t table_bytes;             /* per distinct dictionary */
    int waves_per_wg, wgs_per_cu;   /* the encode launch: a workgroup per so many messages, at most so many per CU */
    bool slots;                     /* every wave of the encode launch works in a table of its own, zeroed before the launch */
    void (*load)(hipStream_t st, unsigned nt, const uint8_t *dict, const uint64_t *toff, const uint32_t *tlen, uint8_t *tables);
    void (*encode)(hipStream_t st, unsigned wgs, const DictBatch &b, const DictTables &t, const DictLayout &w, uint32_t *status, int level);
    k4lz4_ctx::DictScratch k4lz4_ctx::*scratch;
    k4lz4_dict_set::Family k4lz4_dict_set::*in_set;
};
const DictFamily FAMILY_FAST{"k4lz4_encode_dict_batch", ": HC levels with a dictionary are not supported", 8u, 4096u * 4u,
                             k4::FAST_CHAIN_WAVES_PER_WG, 1, false, dict_fast_load, dict_fast_encode, &k4lz4_ctx::dict_fast, &k4lz4_dict_set::fast};
const DictFamily FAMILY_HC{"k4lz4_encode_dict_hc_batch",
                           ": levels below 3 are k4lz4_encode_dict_batch's (LZ4_loadDict + LZ4_compress_fast_continue)", 1u,
                           (size_t)k4::DHC_TABLE_BYTES, k4::DHC_WAVES_PER_WG, DHC_WGS_PER_CU, true, dict_hc_load, dict_hc_encode,
                           &k4lz4_ctx::dict_hc, &k4lz4_dict_set::hc};

const DictFamily &dict_family(int level) { return level >= K4LZ4_L03_HC ? FAMILY_HC : FAMILY_FAST; }
const char *dict_caller(const DictFamily &fam, bool of_set) { return of_set ? "k4lz4_encode_dictset_batch" : fam.who; }

/* which bytes of every dictionary are kept -- the last 64 KiB, of one shorter than min_kept nothing -- and which entries share a
 * table: those that keep the same bytes (same kept start, same kept length; the empty ones are one).  used: which entries the
 * messages refer to (the host form knows), or nullptr: all of them. */
int dict_list(k4lz4_ctx *ctx, uint32_t min_kept, const char *who, const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict,
              const uint8_t *used, DictList &l)
{
    l.keptOff.assign((size_t)nDict, 0); l.keptLen.assign((size_t)nDict, 0); l.table.assign((size_t)nDict, 0xffffffffu); l.rep.clear();
    std::map<std::pair<uint64_t, uint32_t>, uint32_t> seen;
    for (int32_t d = 0; d < nDict; d++) {
        if (dictLen[d] < 0) return fail(ctx, K4LZ4_E_ARG, std::string(who) + ": negative dictLen");
        if (used && !used[d]) continue;
        const uint32_t len = (uint32_t)dictLen[d];
        if (len >= min_kept) {
            l.keptLen[(size_t)d] = std::min<uint32_t>(len, 65536u);
            l.keptOff[(size_t)d] = dictOff[d] + (len - l.keptLen[(size_t)d]);
        }
        const auto key = std::make_pair(l.keptOff[(size_t)d], l.keptLen[(size_t)d]);
        auto it = seen.find(key);
        if (it == seen.end()) { it = seen.emplace(key, (uint32_t)l.rep.size()).first; l.rep.push_back((uint32_t)d); }
        l.table[(size_t)d] = it->second;
    }
    return K4LZ4_OK;
}

/* a list's words for a family's load and encode kernels: per table where its kept bytes start and how many they are, per entry
 * the same and its table.  The arrays come zeroed: an empty list still has one (empty) table */
void dict_words(const DictList &l, uint64_t *toff, uint32_t *tlen, uint64_t *eoff, uint32_t *elen, uint32_t *etab)
{
    for (size_t t = 0; t < l.rep.size(); t++) { toff[t] = l.keptOff[l.rep[t]]; tlen[t] = l.keptLen[l.rep[t]]; }
    for (size_t d = 0; d < l.table.size(); d++) { eoff[d] = l.keptOff[d]; elen[d] = l.keptLen[d]; etab[d] = l.table[d]; }
}

/* returns the bytes that go up from the host: from toff to cost[] */
size_t dict_layout(Carve &c, DictLayout &w, const DictFamily &fam, size_t nt, size_t nd, size_t n, size_t nslots)
{
    c.take(w.head, DICT_HEAD_WORDS); c.take(w.tables, nt * fam.table_bytes);
    const size_t up = c.at;
    c.take(w.toff, nt); c.take(w.tlen, nt); c.take(w.eoff, nd); c.take(w.elen, nd); c.take(w.etab, nd);
    const size_t up_bytes = c.at - up;
    c.take(w.cost, n); c.take(w.order, n); c.take(w.slots, nslots * fam.table_bytes);
    return up_bytes;
}

/* every refusal of the six encode calls that needs no device; b's and s's pointers are the caller's */
int dict_encode_args(k4lz4_ctx *ctx, const DictFamily &fam, int level, int flags, const DictBatch &b, const DictSource &s)
{
    auto refuse = [&](const char *why) { return fail(ctx, K4LZ4_E_ARG, std::string(dict_caller(fam, s.of_set)) + why); };
    const int rc = check_batch_args(ctx, b.src, b.srcOff, b.srcLen, b.dst, b.dstOff, b.dstCap, b.outLen, b.n);
    if (rc != K4LZ4_OK) return rc;
    if (s.of_set && !s.set) return refuse(": set is NULL");
    if (!s.of_set && &dict_family(level) != &fam) return refuse(fam.other_levels);
    if (level >= K4LZ4_L10_OPT)
        return refuse(": levels 10 - 12 with a dictionary are not supported (no sound witness for the optimal parser in this mode)");
    if ((flags & K4LZ4_FLAG_X32) || g_enforce32.load(std::memory_order_relaxed))
        return refuse(": the 32-bit engine (LZ4Codec.Enforce32) is not supported");
    if (flags) return refuse(": it takes no flags");
    if (s.of_set) {
        if (!(s.set->*fam.in_set).on)
            return refuse(": the set was created without this level's family (K4LZ4_DICT_FAST below level 3, K4LZ4_DICT_HC from there)");
        if (s.set->device != ctx->device) return refuse(": the set lives on another device than the context");
        if (b.n > 0 && !b.dictIdx) return refuse(": NULL dictIdx");
        if (b.n > 0xffffffffll) return refuse(": more than 2^32 - 1 messages");
        return K4LZ4_OK;
    }
    if (s.nDict < 0 || (s.nDict > 0 && (!s.dictOff || !s.dictLen)) || (b.n > 0 && !b.dictIdx)) return refuse(": bad dictionary list");
    for (int32_t d = 0; d < s.nDict; d++) {
        if (s.dictLen[d] < 0) return refuse(": negative dictLen");
        if (s.dictLen[d] > 0 && !s.dict) return refuse(": NULL dictionary buffer");
    }
    return K4LZ4_OK;
}

/* all of b's pointers are device pointers; load, order, encode on `stream`.  With a list -- the call's own, its offsets into the
 * device buffer dict -- the list's words go up once the previous upload is over, the load kernel builds the tables (also for
 * no messages), and the family's scratch remembers them for the state query.  With a set the tables and words are the set's:
 * nothing goes up, nothing is waited for, no messages are nothing to do, and the scratch, laid out anew, remembers nothing. */
int dict_encode_run(k4lz4_ctx *ctx, const DictFamily &fam, int level, const DictBatch &b, const uint8_t *dict, const DictList *list,
                    const k4lz4_dict_set *set, hipStream_t stream)
{
    const char *const who = dict_caller(fam, !list);
    const int64_t n = b.n;
    if (!list && n == 0) return K4LZ4_OK;
    if (n > 0xffffffffll) return fail(ctx, K4LZ4_E_ARG, std::string(who) + ": more than 2^32 - 1 messages");      /* (of a set the argument check said so) */
    k4lz4_ctx::DictScratch &sc = ctx->*fam.scratch;
    const size_t nd = list ? list->table.size() : 0, nt = list ? std::max<size_t>(list->rep.size(), 1) : 0;
    const int64_t wgs = std::min<int64_t>((n + fam.waves_per_wg - 1) / fam.waves_per_wg, (int64_t)ctx->cu_count * fam.wgs_per_cu);
    const size_t nslots = fam.slots ? (size_t)wgs * (size_t)fam.waves_per_wg : 0;
    DictLayout w;
    Carve m{nullptr};
    const size_t up_bytes = dict_layout(m, w, fam, nt, nd, (size_t)n, nslots);
    int rc;
    if (list && (rc = plan_begin(ctx, sc.plan, up_bytes, true)) != K4LZ4_OK) return rc;
    if ((rc = grow_scratch(ctx, &sc.plan.dev, &sc.plan.cap, m.at + 64)) != K4LZ4_OK) return rc;
    Carve dv{sc.plan.dev};
    dict_layout(dv, w, fam, nt, nd, (size_t)n, nslots);
    if (list) {
        auto host = [&](auto *p) { return (decltype(p))(sc.plan.host.data() + ((uint8_t *)p - (uint8_t *)w.toff)); };      /* host image of the same layout */
        dict_words(*list, host(w.toff), host(w.tlen), host(w.eoff), host(w.elen), host(w.etab));
        sc.table = list->table; sc.kept = list->keptLen;
        if ((rc = plan_send(ctx, sc.plan, w.toff, up_bytes, stream)) != K4LZ4_OK) return rc;
    } else {
        sc.table.clear(); sc.kept.clear();
        K4_HIP(ctx, order_after_ctx(ctx, stream));
    }
    K4_HIP(ctx, hipMemsetAsync(w.head, 0, DICT_HEAD_WORDS * 4, stream));
    if (list) fam.load(stream, (unsigned)nt, dict, w.toff, w.tlen, w.tables);
    if (n > 0) {
        /* the wave slots' heads start at zero (a wave leaves them so behind every message); the chain halves are written before they are read */
        if (fam.slots) K4_HIP(ctx, hipMemsetAsync(w.slots, 0, nslots * fam.table_bytes, stream));
        k4::BatchArgs o{};
        o.srcLen = b.srcLen; o.n = n; o.cost = w.cost; o.hist = w.head + 64; o.order_out = w.order;
        const unsigned g256 = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(k4::k4_dict_cost_kernel, dim3(g256), dim3(256), 0, stream, o);
        hipLaunchKernelGGL(k4::k4_order_kernel, dim3(k4::order_workgroups(n)), dim3(256), 0, stream, o, 0xffffffffu);
        const k4lz4_dict_set::Family *f = list ? nullptr : &(set->*fam.in_set);
        const DictTables t = list ? DictTables{dict, w.eoff, w.elen, w.etab, w.tables, (int)nd}
                                  : DictTables{set->buf, f->eoff, f->elen, f->etab, f->tables, (int)set->nDict};
        fam.encode(stream, (unsigned)wgs, b, t, w, ctx->d_status, level);
    }
    rc = hipGetLastError() != hipSuccess ? fail(ctx, K4LZ4_E_HIP, std::string(who) + ": kernel launch failed") : K4LZ4_OK;
    mark_busy(ctx, stream);
    return rc;
}

/* the device forms: the caller's pointers are device pointers, but for the list's two arrays */
int dict_encode_device(k4lz4_ctx *ctx, const DictFamily &fam, int level, int flags, const DictBatch &b, const DictSource &s, void *stream)
{
    int rc = dict_encode_args(ctx, fam, level, flags, b, s);
    if (rc != K4LZ4_OK) return rc;
    DictList l;
    if (!s.of_set && (rc = dict_list(ctx, fam.min_kept, fam.who, s.dictOff, s.dictLen, s.nDict, nullptr, l)) != K4LZ4_OK) return rc;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    return dict_encode_run(ctx, fam, level, b, s.dict, s.of_set ? nullptr : &l, s.set, (hipStream_t)stream);
}

/* the host forms: the messages' span goes up and, with a list, behind it the kept bytes of every dictionary in use; the run
 * works on the staged buffers */
int dict_encode_host(k4lz4_ctx *ctx, const DictFamily &fam, int level, int flags, const DictBatch &b, const DictSource &s)
{
    int rc = dict_encode_args(ctx, fam, level, flags, b, s);
    if (rc != K4LZ4_OK) return rc;
    const int32_t nDict = s.of_set ? s.set->nDict : s.nDict;
    std::vector<uint8_t> used(s.of_set ? 0 : (size_t)nDict, 0);
    for (int64_t i = 0; i < b.n; i++) {
        if (b.dictIdx[i] < 0 || b.dictIdx[i] >= nDict)
            return fail(ctx, K4LZ4_E_ARG, std::string(dict_caller(fam, s.of_set)) + ": a dictIdx outside the dictionary list");
        if (!s.of_set) used[(size_t)b.dictIdx[i]] = 1;
    }
    if (s.of_set && b.n == 0) return K4LZ4_OK;
    DictList l;
    if (!s.of_set && (rc = dict_list(ctx, fam.min_kept, fam.who, s.dictOff, s.dictLen, nDict, used.data(), l)) != K4LZ4_OK) return rc;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    HostStage st(ctx);
    st.span(b.src, b.srcOff, b.n, [&](int64_t i) { return (uint64_t)std::max<int32_t>(b.srcLen[i], 0); });
    if (!s.of_set) {
        /* the kept bytes of every dictionary in use go up behind the messages, at 16-byte steps of the same buffer: there the
         * list's offsets point from here on */
        std::vector<uint64_t> at_of(l.rep.size(), 0);
        for (size_t t = 0; t < l.rep.size(); t++) {
            const uint32_t d = l.rep[t];
            if (!l.keptLen[d]) continue;
            at_of[t] = (st.in_bytes + 15u) & ~(uint64_t)15u;
            st.ups.push_back(HostStage::Up{&ctx->d_src, at_of[t], s.dict + l.keptOff[d], (size_t)l.keptLen[d]});
            st.in_bytes = at_of[t] + l.keptLen[d];
        }
        for (size_t e = 0; e < l.table.size(); e++)
            if (used[e]) l.keptOff[e] = at_of[l.table[e]];
    }
    st.slots(b.n, [&](int64_t i) { return (uint64_t)std::max<int32_t>(b.dstCap[i], 0); }, false);
    uint64_t *d_off, *d_doff;
    int32_t *d_len, *d_cap, *d_out, *d_idx;
    st.meta(&d_off, b.n, st.in_off.data()); st.meta(&d_len, b.n, b.srcLen); st.meta(&d_doff, b.n, st.slot.data()); st.meta(&d_cap, b.n, b.dstCap);
    st.meta(&d_idx, b.n, b.dictIdx); st.meta(&d_out, b.n);
    if ((rc = st.upload()) != K4LZ4_OK) return rc;
    const DictBatch staged{ctx->d_src, d_off, d_len, ctx->d_dst, d_doff, d_cap, d_out, b.n, d_idx};
    if ((rc = dict_encode_run(ctx, fam, level, staged, ctx->d_src, s.of_set ? nullptr : &l, s.set, st.st)) != K4LZ4_OK) return rc;
    return finish_blocks(st, b.outLen, d_out, b.n, b.dst, b.dstOff, b.dstCap);
}

/* the table the family's most recent call with a list of its own gave entry d of that list, or nullptr */
const uint8_t *dict_loaded_table(k4lz4_ctx *ctx, const DictFamily &fam, int32_t d)
{
    const k4lz4_ctx::DictScratch &sc = ctx->*fam.scratch;
    if (d < 0 || (size_t)d >= sc.table.size() || sc.table[(size_t)d] == 0xffffffffu || !sc.plan.dev) return nullptr;
    Carve c{sc.plan.dev};
    DictLayout w;
    dict_layout(c, w, fam, 1, 0, 0, 0);
    return w.tables + fam.table_bytes * sc.table[(size_t)d];
}

/* what the state queries answer from a table on the device: of a call's own list, or of a set (then without a context) */
int dict_fast_state(k4lz4_ctx *ctx, const uint8_t *table, uint32_t kept, k4lz4_fast_chain_state *out)
{
    K4_HIP(ctx, hipMemcpy(out->hashTable, table, sizeof out->hashTable, hipMemcpyDeviceToHost));
    out->currentOffset = k4::DICT_START;
    out->dictSize = kept;
    out->reserved[0] = out->reserved[1] = 0;
    return K4LZ4_OK;
}
int dict_hc_state(k4lz4_ctx *ctx, const uint8_t *table, uint32_t kept, uint32_t *hashTable, uint16_t *chainTable, int32_t *keptLen)
{
    K4_HIP(ctx, hipMemcpy(hashTable, table, (size_t)k4::DHC_HEADS * 4, hipMemcpyDeviceToHost));
    K4_HIP(ctx, hipMemcpy(chainTable, table + (size_t)k4::DHC_HEADS * 4, (size_t)k4::DHC_CHAIN * 2, hipMemcpyDeviceToHost));
    *keptLen = (int32_t)kept;
    return K4LZ4_OK;
}

void direct_layout(Carve &c, k4::FrFastArgs &f, size_t n, size_t nr)
{
    c.take(f.plan, n); c.take(f.done, n);
    c.take(f.sSrcOff, n); c.take(f.sDstOff, n); c.take(f.sSrcLen, n); c.take(f.sDstCap, n); c.take(f.sOutLen, n);
    c.take(f.srcOff, nr); c.take(f.dstOff, nr); c.take(f.hlen, nr); c.take(f.srcLen, nr); c.take(f.dstCap, nr); c.take(f.outLen, nr);
    c.take(f.sum, nr); c.take(f.got, nr); c.take(f.lc, nr);
}
void direct_layout(Carve &c, k4::FrFeedFastArgs &ff, size_t n, size_t nr)
{
    direct_layout(c, ff.f, n, nr);
    c.take(ff.tail, n); c.take(ff.want, n);
}
void direct_layout(Carve &c, k4::FrDictRows &w, size_t n, size_t nr)
{
    c.take(w.dictOff, nr); c.take(w.dictLen, nr); c.take(w.dictMode, nr);
    c.take(w.sDictOff, n); c.take(w.sDictLen, n); c.take(w.sDictMode, n); c.take(w.entry, n);
}
void direct_layout(Carve &c, k4::FrDictFastArgs &d, size_t n, size_t nr)
{
    direct_layout(c, d.f, n, nr);
    direct_layout(c, d.w, n, nr);
}
void direct_layout(Carve &c, k4::FrDictFeedFastArgs &d, size_t n, size_t nr)
{
    direct_layout(c, d.f, n, nr);
    direct_layout(c, d.w, n, nr);
}
void direct_layout(Carve &c, k4::LsDirectArgs &f, size_t n, size_t nr)
{
    c.take(f.plan, n); c.take(f.done, n);
    c.take(f.sSrcOff, n); c.take(f.sDstOff, n); c.take(f.sSrcLen, n); c.take(f.sDstCap, n); c.take(f.sOutLen, n);
    c.take(f.srcOff, nr); c.take(f.dstOff, nr); c.take(f.srcLen, nr); c.take(f.dstCap, nr); c.take(f.outLen, nr); c.take(f.rawLen, nr);
}
void direct_layout(Carve &c, k4::LsFeedDirectArgs &f, size_t n, size_t nr)
{
    c.take(f.plan, n); c.take(f.done, n); c.take(f.head, n);
    c.take(f.sSrcAddr, n); c.take(f.sDstAddr, n); c.take(f.sSrcLen, n); c.take(f.sDstCap, n); c.take(f.sOutLen, n);
    c.take(f.srcAddr, nr); c.take(f.dstAddr, nr); c.take(f.srcLen, nr); c.take(f.dstCap, nr); c.take(f.outLen, nr); c.take(f.rawLen, nr);
}

/* What tells the readers apart on the host.  Args: what the per-stream reader kernel (READ) takes; Direct: what the direct
 * path's PLAN and COMMIT kernels take, table(d) the part of it that holds the tables; begin() hands the call's arrays to the direct
 * path and served() hands the reader kernel what the commit left for it.  SUMS: block checksums between plan and decode.
 * ADDRESSES: the rows hold addresses -- a row's source may be the stash, which TOPUP completes first --, the decoder's bases are null.
 * DICT: the call has a dictionary set -- words(d) are the plan's dictionary words for the batch decoder. */
struct FrameReader {
    using Args = k4::FrReadArgs; using Direct = k4::FrFastArgs;
    static constexpr int WAVES = k4::FR_WAVES_PER_WG;
    static constexpr bool SUMS = true, ADDRESSES = false, DICT = false;
    static constexpr const char *ROWS_PASS = "k4lz4_frame_read_batch: maxCount / 64 KiB + 2 rows per stream pass 2^31 rows";
    static constexpr auto PLAN = k4::k4_fr_plan_kernel, COMMIT = k4::k4_fr_commit_kernel;
    static constexpr auto READ = k4::k4_fr_read_kernel;
    static Args &reader(Args &a) { return a; }
    static Direct &table(Direct &d) { return d; }
    static void begin(Direct &d, const Args &a) { d.r = a; }
    static void served(Args &a, const Direct &d) { a.done = d.done; }
};
struct FedFrameReader {
    using Args = k4::FrFeedArgs; using Direct = k4::FrFeedFastArgs;
    static constexpr int WAVES = k4::FR_WAVES_PER_WG;
    static constexpr bool SUMS = true, ADDRESSES = false, DICT = false;
    static constexpr const char *ROWS_PASS = "k4lz4_frame_read_fed_batch: maxCount / 64 KiB + 2 rows per stream pass 2^31 rows";
    static constexpr auto PLAN = k4::k4_fr_feed_plan_kernel, COMMIT = k4::k4_fr_feed_commit_kernel;
    static constexpr auto READ = k4::k4_fr_feed_kernel;
    static k4::FrReadArgs &reader(Args &a) { return a.r; }
    static k4::FrFastArgs &table(Direct &d) { return d.f; }
    static void begin(Direct &d, const Args &a) { d.f.r = a.r; d.final = a.final; d.consumed = a.consumed; d.need = a.need; }
    static void served(Args &a, const Direct &d) { a.r.done = d.f.done; }
};
struct DictFrameReader {
    using Args = k4::FrDictReadArgs; using Direct = k4::FrDictFastArgs;
    static constexpr int WAVES = k4::FR_WAVES_PER_WG;
    static constexpr bool SUMS = true, ADDRESSES = false, DICT = true;
    static constexpr const char *ROWS_PASS = "k4lz4_frame_read_dictset_batch: maxCount / 64 KiB + 2 rows per stream pass 2^31 rows";
    static constexpr auto PLAN = k4::k4_fr_dict_plan_kernel, COMMIT = k4::k4_fr_dict_commit_kernel;
    static constexpr auto READ = k4::k4_fr_dict_read_kernel;
    static k4::FrReadArgs &reader(Args &a) { return a.r; }
    static k4::FrFastArgs &table(Direct &d) { return d.f; }
    static const k4::FrDictRows &words(const Direct &d) { return d.w; }
    static void begin(Direct &d, const Args &a) { d.f.r = a.r; d.w.d = a.d; }
    static void served(Args &a, const Direct &d) { a.r.done = d.f.done; }
};
struct DictFedFrameReader {
    using Args = k4::FrDictFeedArgs; using Direct = k4::FrDictFeedFastArgs;
    static constexpr int WAVES = k4::FR_WAVES_PER_WG;
    static constexpr bool SUMS = true, ADDRESSES = false, DICT = true;
    static constexpr const char *ROWS_PASS = "k4lz4_frame_read_fed_dictset_batch: maxCount / 64 KiB + 2 rows per stream pass 2^31 rows";
    static constexpr auto PLAN = k4::k4_fr_dict_feed_plan_kernel, COMMIT = k4::k4_fr_dict_feed_commit_kernel;
    static constexpr auto READ = k4::k4_fr_dict_feed_kernel;
    static k4::FrReadArgs &reader(Args &a) { return a.f.r; }
    static k4::FrFastArgs &table(Direct &d) { return d.f.f; }
    static const k4::FrDictRows &words(const Direct &d) { return d.w; }
    static void begin(Direct &d, const Args &a) { FedFrameReader::begin(d.f, a.f); d.w.d = a.d; }
    static void served(Args &a, const Direct &d) { a.f.r.done = d.f.f.done; }
};
struct LegacyReader {
    using Args = k4::LsReadArgs; using Direct = k4::LsDirectArgs;
    static constexpr int WAVES = k4::LS_WAVES_PER_WG;
    static constexpr bool SUMS = false, ADDRESSES = false, DICT = false;
    static constexpr const char *ROWS_PASS = "k4lz4_legacy_read_batch: the chunk table passes 2^31 rows";
    static constexpr auto PLAN = k4::k4_ls_plan_kernel, COMMIT = k4::k4_ls_commit_kernel;
    static constexpr auto READ = k4::k4_ls_read_kernel;
    static Args &reader(Args &a) { return a; }
    static Direct &table(Direct &d) { return d; }
    static void begin(Direct &d, const Args &a) { d.r = a; }
    static void served(Args &a, const Direct &d) { a.done = d.done; }
};
struct FedLegacyReader {
    using Args = k4::LsFeedArgs; using Direct = k4::LsFeedDirectArgs;
    static constexpr int WAVES = k4::LS_WAVES_PER_WG;
    static constexpr bool SUMS = false, ADDRESSES = true, DICT = false;
    static constexpr const char *ROWS_PASS = "k4lz4_legacy_read_fed_batch: the chunk table passes 2^31 rows";
    static constexpr auto TOPUP = k4::k4_ls_feed_topup_kernel, PLAN = k4::k4_ls_feed_plan_kernel, COMMIT = k4::k4_ls_feed_commit_kernel;
    static constexpr auto READ = k4::k4_ls_feed_kernel;
    static k4::LsReadArgs &reader(Args &a) { return a.r; }
    static Direct &table(Direct &d) { return d; }
    static void begin(Direct &d, const Args &a) { d.f = a; }
    static void served(Args &a, const Direct &d) { a.r.done = d.done; a.head = d.head; }
};

/* a reader's device form after its argument checks.  rows: the table rows per stream when the call takes the direct path (a READ
 * that is not interactive), else 0.  The direct path: plan, block checksums, the batch decoder into dst and into the stores, check
 * and commit; the table is bounded by maxCount, so nothing is read back.  Then the per-stream reader for what is left. */
template <class F>
int read_device(k4lz4_ctx *ctx, typename F::Args a, long long rows, void *stream)
{
    auto &r = F::reader(a);
    const long long n = r.n;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    K4_HIP(ctx, order_after_ctx(ctx, st));
    const dim3 waves((unsigned)((n + F::WAVES - 1) / F::WAVES)), wg(64 * F::WAVES);
    if (rows > 0) {
        if (n * rows > 0x7fffffffll) return fail(ctx, K4LZ4_E_ARG, F::ROWS_PASS);
        const size_t nr = (size_t)n * (size_t)rows;
        typename F::Direct d{};
        F::begin(d, a);
        auto &t = F::table(d);
        t.rows = rows;
        Carve measure{nullptr};
        direct_layout(measure, d, (size_t)n, nr);
        int rc;
        if ((rc = grow_scratch(ctx, &ctx->d_frd, &ctx->d_frd_cap, measure.at)) != K4LZ4_OK) return rc;
        Carve place{ctx->d_frd};
        direct_layout(place, d, (size_t)n, nr);
        if constexpr (F::ADDRESSES) hipLaunchKernelGGL(F::TOPUP, waves, wg, 0, st, d);
        hipLaunchKernelGGL(F::PLAN, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d);
        K4_HIP(ctx, hipGetLastError());
        if constexpr (F::SUMS)
            if ((rc = k4lz4_xxh32_batch_device(ctx, r.src, t.srcOff, t.hlen, t.got, (int64_t)nr, 0, st)) != K4LZ4_OK) return rc;
        DictArgs rows_dict{}, stores_dict{};               /* DICT: every row against its stream's entry, the set's bytes as dict */
        if constexpr (F::DICT) {
            const k4::FrDictRows &w = F::words(d);
            rows_dict = DictArgs{w.d.dict, w.dictOff, w.dictLen, w.dictMode};
            stores_dict = DictArgs{w.d.dict, w.sDictOff, w.sDictLen, w.sDictMode};
        }
        if constexpr (F::ADDRESSES) {
            if ((rc = launch(ctx, KIND_DECODE, nullptr, t.srcAddr, t.srcLen, nullptr, t.dstAddr, t.dstCap, t.outLen, (int64_t)nr, 0, 0, st)) != K4LZ4_OK ||
                (rc = launch(ctx, KIND_DECODE, nullptr, t.sSrcAddr, t.sSrcLen, nullptr, t.sDstAddr, t.sDstCap, t.sOutLen, n, 0, 0, st)) != K4LZ4_OK)
                return rc;
        } else {
            if ((rc = launch(ctx, KIND_DECODE, r.src, t.srcOff, t.srcLen, r.dst, t.dstOff, t.dstCap, t.outLen, (int64_t)nr, 0, 0, st,
                             F::DICT ? &rows_dict : nullptr)) != K4LZ4_OK ||
                (rc = launch(ctx, KIND_DECODE, r.src, t.sSrcOff, t.sSrcLen, r.store, t.sDstOff, t.sDstCap, t.sOutLen, n, 0, 0, st,
                             F::DICT ? &stores_dict : nullptr)) != K4LZ4_OK)
                return rc;
        }
        hipLaunchKernelGGL(F::COMMIT, waves, wg, 0, st, d);
        F::served(a, d);
    }
    hipLaunchKernelGGL(F::READ, waves, wg, 0, st, a);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    return K4LZ4_OK;
}

/* the arrays of a reader's call: the caller's in the host form, their staged copies in what it hands its device form */
struct ReadArrays {
    const uint64_t *storeOff;
    const uint8_t *src;
    const uint64_t *srcOff, *srcLen;
    const int64_t *final;                  /* final, consumed, need: the fed forms' (consumed == nullptr: not a fed form) */
    uint8_t *dst;
    const uint64_t *dstOff;
    const int64_t *count;
    int64_t *outLen, *consumed, *need;
};

/* a reader's host form after its argument checks.  sends: the op takes pieces -- they go up packed, and a stream that sits the call
 * out (count < 0) sends nothing; fills: the op is READ -- slots of count bytes, outLen[i] of them for the caller;
 * device(staged, maxCount, stream) is the device form */
template <class Device>
int host_read(k4lz4_ctx *ctx, const ReadArrays &h, int64_t n, bool sends, bool fills, Device device)
{
    const bool fed = h.consumed != nullptr;
    int64_t maxCount = 0;
    for (int64_t i = 0; fills && i < n; i++) maxCount = std::max(maxCount, h.count[i]);
    for (int64_t i = 0; sends && i < n; i++)
        if (h.count[i] >= 0 && h.srcLen[i] > 0 && !h.src) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    K4_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int64_t> len0((size_t)n, 0), fin0((size_t)n, 0);
    std::vector<uint64_t> off0((size_t)n, 0);
    for (int64_t i = 0; sends && i < n; i++)
        if (h.count[i] >= 0) { len0[(size_t)i] = (int64_t)h.srcLen[i]; off0[(size_t)i] = h.srcOff[i]; fin0[(size_t)i] = h.final ? h.final[i] : 0; }
    HostStage s(ctx);
    s.pack(h.src, off0.data(), len0.data(), n);
    s.slots(n, [&](int64_t i) { return fills && h.count[i] > 0 ? (uint64_t)h.count[i] : 0u; }, false);
    uint64_t *d_soff, *d_slen, *d_store, *d_doff;
    int64_t *d_count, *d_out, *d_fin = nullptr, *d_cons = nullptr, *d_need = nullptr;
    s.meta(&d_soff, n, s.in_off.data()); s.meta(&d_slen, n, len0.data()); s.meta(&d_store, n, h.storeOff); s.meta(&d_doff, n, s.slot.data());
    s.meta(&d_count, n, h.count); s.meta(&d_out, n);
    if (fed) { s.meta(&d_fin, n, fin0.data()); s.meta(&d_cons, n); s.meta(&d_need, n); }
    int rc;
    if ((rc = s.upload()) != K4LZ4_OK ||
        (rc = device(ReadArrays{d_store, ctx->d_src, d_soff, d_slen, d_fin, ctx->d_dst, d_doff, d_count, d_out, d_cons, d_need}, maxCount,
                     s.st)) != K4LZ4_OK)
        return rc;
    const size_t fed_bytes = fed ? (size_t)n * 8 : 0;
    return s.finish({{h.outLen, d_out, (size_t)n * 8}, {h.consumed, d_cons, fed_bytes}, {h.need, d_need, fed_bytes}}, h.dst, h.dstOff,
                    [&](int64_t i) { return fills && h.outLen[i] > 0 ? (size_t)h.outLen[i] : 0; });
}

/* the per-stream queries (k4lz4_frame_reader_query, k4lz4_legacy_reader_query, k4lz4_chain_decoder_query): words int64 per stream */
using QueryKernel = void (*)(const uint8_t *, const uint64_t *, int64_t *, long long);
int query_device(k4lz4_ctx *ctx, QueryKernel kernel, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!store || !storeOff || !out))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    K4_HIP(ctx, order_after_ctx(ctx, st));
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, store, storeOff, out, (long long)n);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    return K4LZ4_OK;
}

using QueryDevice = int (*)(k4lz4_ctx *, const uint8_t *, const uint64_t *, int64_t, int64_t *, void *);
int query_host(k4lz4_ctx *ctx, int64_t words, QueryDevice device, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!store || !storeOff || !out))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    HostStage s(ctx);
    uint64_t *d_store;
    int64_t *d_out;
    s.meta(&d_store, n, storeOff); s.meta(&d_out, n * words);
    int rc;
    if ((rc = s.upload()) != K4LZ4_OK || (rc = device(ctx, store, d_store, n, d_out, s.st)) != K4LZ4_OK) return rc;
    return s.finish({{out, d_out, (size_t)(n * words) * 8}});
}

/* ---- incremental frame writer: the host half of k4lz4_frame_write.hpp (the store's layout, the header, the ring model, the bound) */
using k4::FW_XXH_BYTES; using k4::FW_CHAIN_LIMIT; using k4::FwAfter;
using k4::fw_ring_at; using k4::fw_slot; using k4::fw_header; using k4::fw_opens; using k4::fw_model; using k4::fw_bound; using k4::fw_code;
using k4::fw_advance;

size_t fw_take(size_t &at, size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; }

/* numbers the chunks of the pieces k4_fw_copy_kernel takes (a workgroup per chunk, an empty piece has one); returns their count */
unsigned long long fw_chunks(k4::FwPiece *p, size_t cnt)
{
    unsigned long long c = 0;
    for (size_t k = 0; k < cnt; k++) { p[k].chunk0 = c; c += std::max<unsigned long long>(1, (p[k].len + k4::FW_CHUNK - 1) / k4::FW_CHUNK); }
    return c;
}

}  // namespace

extern "C" {

int k4lz4_version(void) { return K4LZ4_VERSION; }

void k4lz4_set_enforce32(int on) { g_enforce32.store(on ? 1 : 0, std::memory_order_relaxed); }
int k4lz4_get_enforce32(void) { return g_enforce32.load(std::memory_order_relaxed); }

int k4lz4_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int k4lz4_ctx_create(k4lz4_ctx **out, int device)
{
    if (!out) return fail(nullptr, K4LZ4_E_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, K4LZ4_E_NO_DEVICE, "no HIP device visible (libk4lz4 has no CPU fallback)");
    }
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); device = 0; }
    }
    if (device >= n) return fail(nullptr, K4LZ4_E_ARG, "device index out of range");
    hipDeviceProp_t prop;
    K4_HIP(nullptr, hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, K4LZ4_E_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", libk4lz4 is built for gfx950 only");
    k4lz4_ctx *ctx = new (std::nothrow) k4lz4_ctx();
    if (!ctx) return fail(nullptr, K4LZ4_E_NOMEM, "out of host memory");
    ctx->device = device;
    ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_status, 64);
    if (e == hipSuccess) e = hipMemset(ctx->d_status, 0, 64);
    if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_pace, k4::PACE_BYTES);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->copyq, hipStreamNonBlocking);
    if (e == hipSuccess) {
        /* the later segments of cut blocks are the longest jobs of their launch and others wait for their cuts: the queue they
         * are dispatched from comes first when the chip is full (K4LZ4_SEG_PRIO=0: an ordinary queue) */
        int least = 0, greatest = 0;
        const char *pe = getenv("K4LZ4_SEG_PRIO");
        if ((!pe || atoi(pe) != 0) && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
            e = hipStreamCreateWithPriority(&ctx->aux2, hipStreamNonBlocking, greatest);
        else { (void)hipGetLastError(); e = hipStreamCreateWithFlags(&ctx->aux2, hipStreamNonBlocking); }
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_join2, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_busy, hipEventDisableTiming);
    for (int b = 0; b < 2 && e == hipSuccess; b++) {
        e = hipEventCreateWithFlags(&ctx->ev_in[b], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_out[b], hipEventDisableTiming);
    }
    for (int b = 0; b < MAX_PARTS && e == hipSuccess; b++) {
        e = hipEventCreateWithFlags(&ctx->ev_up[b], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_len[b], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->dlq, hipStreamNonBlocking);
    read_switches(*ctx);
    if (e != hipSuccess) { delete ctx; return hip_fail(nullptr, e, "hipStreamCreate"); }
    *out = ctx;
    return K4LZ4_OK;
}

void k4lz4_ctx_destroy(k4lz4_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
    if (ctx->aux) { (void)hipStreamSynchronize(ctx->aux); (void)hipStreamDestroy(ctx->aux); }
    if (ctx->aux2) { (void)hipStreamSynchronize(ctx->aux2); (void)hipStreamDestroy(ctx->aux2); }
    if (ctx->ev_join2) (void)hipEventDestroy(ctx->ev_join2);
    if (ctx->d_seg) (void)hipFree(ctx->d_seg);
    if (ctx->d_seg_first) (void)hipFree(ctx->d_seg_first);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->ev_busy) (void)hipEventDestroy(ctx->ev_busy);
    for (int b = 0; b < 2; b++) {
        if (ctx->ev_in[b]) (void)hipEventDestroy(ctx->ev_in[b]);
        if (ctx->ev_out[b]) (void)hipEventDestroy(ctx->ev_out[b]);
        if (ctx->h_in[b]) (void)hipHostFree(ctx->h_in[b]);
        if (ctx->h_out[b]) (void)hipHostFree(ctx->h_out[b]);
    }
    if (ctx->d_pack) (void)hipFree(ctx->d_pack);
    if (ctx->h_len) (void)hipHostFree(ctx->h_len);
    for (int b = 0; b < MAX_PARTS; b++) {
        if (ctx->ev_up[b]) (void)hipEventDestroy(ctx->ev_up[b]);
        if (ctx->ev_len[b]) (void)hipEventDestroy(ctx->ev_len[b]);
    }
    if (ctx->copyq) (void)hipStreamDestroy(ctx->copyq);
    if (ctx->dlq) (void)hipStreamDestroy(ctx->dlq);
    delete ctx->pool;
    delete ctx->pool_dl;
    if (ctx->d_status) (void)hipFree(ctx->d_status);
    if (ctx->d_pace) (void)hipFree(ctx->d_pace);
    if (ctx->d_gtab) (void)hipFree(ctx->d_gtab);
    if (ctx->d_parse) (void)hipFree(ctx->d_parse);
    if (ctx->d_dict) (void)hipFree(ctx->d_dict);
    if (ctx->d_src) (void)hipFree(ctx->d_src);
    if (ctx->d_dst) (void)hipFree(ctx->d_dst);
    if (ctx->d_meta) (void)hipFree(ctx->d_meta);
    if (ctx->d_fr) (void)hipFree(ctx->d_fr);
    if (ctx->d_fb) (void)hipFree(ctx->d_fb);
    if (ctx->d_lg) (void)hipFree(ctx->d_lg);
    if (ctx->d_frd) (void)hipFree(ctx->d_frd);
    if (ctx->d_lgr) (void)hipFree(ctx->d_lgr);
    if (ctx->d_lga) (void)hipFree(ctx->d_lga);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    if (ctx->d_sched) (void)hipFree(ctx->d_sched);
    if (ctx->d_hc_hash) (void)hipFree(ctx->d_hc_hash);
    if (ctx->d_hc_work) (void)hipFree(ctx->d_hc_work);
    if (ctx->d_hc_meta) (void)hipFree(ctx->d_hc_meta);
    for (PlanUpload *p : {&ctx->chain_plan, &ctx->fw_plan, &ctx->fdict_plan, &ctx->dict_fast.plan, &ctx->dict_hc.plan}) {
        if (p->dev) (void)hipFree(p->dev);
        if (p->ev) (void)hipEventDestroy(p->ev);
    }
    if (ctx->d_pk_meta) (void)hipFree(ctx->d_pk_meta);
    if (ctx->d_dpick) (void)hipFree(ctx->d_dpick);
    if (ctx->d_fdx) (void)hipFree(ctx->d_fdx);
    if (ctx->d_fdb) (void)hipFree(ctx->d_fdb);
    delete ctx;
}

const char *k4lz4_last_error(const k4lz4_ctx *ctx) { return ctx ? ctx->error.c_str() : tl_error.c_str(); }

/* measured floors of a device call (profiles/r5_block_count_scaling.txt: a 64 KiB text block alone 2.0 ms to encode -- 2.9 ms with the
 * one-kernel encoder of rounds 1-4 --, 0.55 ms to decode; r18_stamp.txt: 8.7 ms at HC level 3): the time of ONE block on its wavefront, scaled with the block length (a wavefront's
 * time per block is linear in its length), never below the launch + synchronisation cost of a call */
int64_t k4lz4_recommended_min_batch(int kind, int32_t blockBytes, double hostGiBs)
{
    if (kind < 0 || kind > 2 || blockBytes <= 0) return K4LZ4_E_ARG;
    static const double floor_ms_64k[3] = {2.0, 0.55, 2.9};      /* (HC level 3: 8.7 until round 6; profiles/r6_hc_small_batches.txt) */
    static const double box_host_GiBs[3] = {32.0, 35.0, 2.2};
    const double host = hostGiBs > 0.0 ? hostGiBs : box_host_GiBs[kind];
    double floor_ms = floor_ms_64k[kind] * (double)blockBytes / 65536.0;
    /* (fast encode of blocks of 65 547 bytes and more -- byU32 tables -- is the one-kernel encoder's: its floor is the older, higher one) */
    if (kind == 0 && blockBytes >= k4::LIMIT_64K) floor_ms = 2.9 * (double)blockBytes / 65536.0;
    if (floor_ms < 0.05) floor_ms = 0.05;
    const double blocks = floor_ms * 1e-3 * host * 1073741824.0 / (double)blockBytes;
    return blocks < 1.0 ? 1 : (int64_t)(blocks + 0.999);
}

int k4lz4_ctx_device(const k4lz4_ctx *ctx) { return ctx ? ctx->device : -1; }

int k4lz4_synchronize(k4lz4_ctx *ctx, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    K4_HIP(ctx, hipSetDevice(ctx->device));
    K4_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
    return take_device_status(ctx);
}

int k4lz4_host_register(void *ptr, size_t bytes)
{
    if (!ptr || !bytes) { tl_error = "k4lz4_host_register: empty range"; return K4LZ4_E_ARG; }
    /* one lock scope for check + insert: the range is entered before the (slow) pinning so that a second thread registering an
     * overlapping range is refused; if pinning fails the entry is taken out again */
    const uintptr_t a = (uintptr_t)ptr;
    try {
        std::lock_guard<std::mutex> g(g_reg_mu);
        for (const auto &r : g_reg)
            if (a < r.first + r.second && r.first < a + bytes) { tl_error = "k4lz4_host_register: overlaps a registered range"; return K4LZ4_E_ARG; }
        g_reg.push_back(RegRange{a, bytes, false});
    } catch (const std::bad_alloc &) { tl_error = "k4lz4_host_register: out of host memory"; return K4LZ4_E_NOMEM; }
    const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        {
            std::lock_guard<std::mutex> g(g_reg_mu);
            auto it = std::find_if(g_reg.begin(), g_reg.end(), [&](const RegRange &r) { return r.first == a && r.second == bytes && !r.pinned; });
            if (it != g_reg.end()) g_reg.erase(it);
        }
        tl_error = std::string("hipHostRegister: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? K4LZ4_E_NOMEM : K4LZ4_E_HIP;
    }
    {   /* only now do host-pointer calls treat the range as page-locked, and only now can it be unregistered */
        std::lock_guard<std::mutex> g(g_reg_mu);
        auto it = std::find_if(g_reg.begin(), g_reg.end(), [&](const RegRange &r) { return r.first == a && r.second == bytes && !r.pinned; });
        if (it != g_reg.end()) it->pinned = true;
    }
    return K4LZ4_OK;
}

int k4lz4_host_unregister(void *ptr)
{
    {
        std::lock_guard<std::mutex> g(g_reg_mu);
        auto it = std::find_if(g_reg.begin(), g_reg.end(), [&](const RegRange &r) { return r.first == (uintptr_t)ptr && r.pinned; });      /* (a range still being pinned is not there yet) */
        if (it == g_reg.end()) { tl_error = "k4lz4_host_unregister: not a registered range"; return K4LZ4_E_ARG; }
        g_reg.erase(it);
    }
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) { (void)hipGetLastError(); tl_error = std::string("hipHostUnregister: ") + hipGetErrorString(e); return K4LZ4_E_HIP; }
    return K4LZ4_OK;
}

int k4lz4_ctx_reserve_hc(k4lz4_ctx *ctx, int64_t totalSrcBytes, int32_t longestBlock)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (totalSrcBytes < 0 || longestBlock < 0) return fail(ctx, K4LZ4_E_ARG, "negative reservation");
    ctx->hc_res_total = (uint64_t)totalSrcBytes;
    ctx->hc_res_longest = (uint32_t)longestBlock;
    return K4LZ4_OK;
}

int k4lz4_selftest_chains(k4lz4_ctx *ctx, int waves, int rounds, uint32_t seed, uint32_t mismatches[3])
{
    if (!ctx || !mismatches || waves <= 0 || rounds <= 0) return fail(ctx, K4LZ4_E_ARG, "selftest: bad arguments");
    K4_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t *d_res = nullptr;
    K4_HIP(ctx, hipMalloc((void **)&d_res, 3 * sizeof(uint32_t)));
    hipError_t e = hipMemsetAsync(d_res, 0, 3 * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k4::k4_chain_selftest_kernel, dim3((unsigned)waves), dim3(64), 0, ctx->stream, seed, rounds, d_res);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(mismatches, d_res, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_res);
    K4_HIP(ctx, e);
    return K4LZ4_OK;
}

int k4lz4_last_decode_kernel(const k4lz4_ctx *ctx) { return ctx ? ctx->last_decode_kernel : K4LZ4_DECODE_KERNEL_NONE; }
int k4lz4_last_encode_route(const k4lz4_ctx *ctx) { return ctx ? ctx->last_encode_route : K4LZ4_ENCODE_ROUTE_NONE; }

int k4lz4_last_status(void) { return tl_status; }

int k4lz4_compress_bound(int n) { return n > 0x7E000000 ? 0 : n + n / 255 + 16; }

int k4lz4_compress_fast(const uint8_t *src, uint8_t *dst, int srcLen, int dstCap, int acceleration)
{
    return single(KIND_ENCODE, src, dst, srcLen, dstCap, K4LZ4_L00_FAST, acceleration);
}

int k4lz4_compress_hc(const uint8_t *src, uint8_t *dst, int srcLen, int dstCap, int level)
{
    /* LZ4Level has no value between L00_FAST and L03_HC and LZ4Codec never passes one (LZ4Codec.cs:48-50); the upstream
     * meaning of levels below 3 (default 9 / two attempts, LL64.high.cs:1155-1160) is not implemented: refuse, do not guess */
    if (level < K4LZ4_L03_HC) {
        tl_status = fail(nullptr, K4LZ4_E_ARG, "k4lz4_compress_hc: level must be L03_HC (3) or higher");
        return 0;
    }
    return single(KIND_ENCODE, src, dst, srcLen, dstCap, level);
}

int k4lz4_decompress_safe(const uint8_t *src, uint8_t *dst, int srcLen, int dstCap)
{
    return single(KIND_DECODE, src, dst, srcLen, dstCap, 0);
}

int k4lz4_decompress_safe_partial(const uint8_t *src, uint8_t *dst, int srcLen, int targetLen)
{
    return single(KIND_DECODE, src, dst, srcLen, targetLen, 0, 1, K4LZ4_FLAG_PARTIAL);
}

int k4lz4_encode_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                       const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags)
{
    return run_host(ctx, KIND_ENCODE, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, level, flags);
}

int k4lz4_decompress_safe_using_dict(const uint8_t *src, uint8_t *dst, int srcLen, int dstCap, const uint8_t *dict, int dictLen)
{
    return single(KIND_DECODE, src, dst, srcLen, dstCap, 0, 1, 0, dict, dictLen);
}

int k4lz4_decode_dict_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                            const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int flags,
                            const uint8_t *dict, const uint64_t *dictOff, const int32_t *dictLen)
{
    if (dict && n > 0 && (!dictOff || !dictLen)) return fail(ctx, K4LZ4_E_ARG, "NULL dictionary offsets/lengths");
    const DictArgs hd{dict, dictOff, dictLen, nullptr};
    return run_host(ctx, KIND_DECODE, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, 0, flags, dict ? &hd : nullptr);
}

int k4lz4_decode_dict_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                   uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n,
                                   int flags, const uint8_t *dict, const uint64_t *dictOff, const int32_t *dictLen,
                                   void *stream)
{
    if (dict && n > 0 && (!dictOff || !dictLen)) return fail(ctx, K4LZ4_E_ARG, "NULL dictionary offsets/lengths");
    const DictArgs dd{dict, dictOff, dictLen, nullptr};
    return run_device(ctx, KIND_DECODE, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, 0, flags, stream, dict ? &dd : nullptr);
}

int k4lz4_decode_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                       const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int flags)
{
    return run_host(ctx, KIND_DECODE, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, 0, flags);
}

int k4lz4_encode_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                              uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n,
                              int level, int flags, void *stream)
{
    return run_device(ctx, KIND_ENCODE, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, level, flags, stream);
}

int k4lz4_decode_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                              uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n,
                              int flags, void *stream)
{
    return run_device(ctx, KIND_DECODE, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, 0, flags, stream);
}

int k4lz4_pickle_bound(int srcLen) { return srcLen <= 0 ? 0 : 1 + 4 + srcLen; }

int k4lz4_unpickle_size(const uint8_t *p, int len)
{
    /* LZ4Pickler.unpickle.cs:131-148 */
    if (len == 0) return 0;
    if (!p || len < 0) return -1;
    if ((p[0] & 7) != 0) return -1;
    const int code = (p[0] >> 6) & 3;
    const int sod = code == 3 ? 4 : code;
    const int data_len = len - 1 - sod;
    if (data_len < 0) return -1;
    uint32_t diff = 0;
    for (int i = 0; i < sod; i++) diff |= (uint32_t)p[1 + i] << (8 * i);
    const int r = (int)((uint32_t)data_len + diff);
    return r < 0 ? -1 : r;
}

int k4lz4_pickle_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                       const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags)
{
    return run_host(ctx, KIND_PICKLE, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, level, flags);
}

int k4lz4_unpickle_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                         const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int flags)
{
    return run_host(ctx, KIND_UNPICKLE, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, 0, flags);
}

int k4lz4_pickle_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                              uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n,
                              int level, int flags, void *stream)
{
    return run_device(ctx, KIND_PICKLE, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, level, flags, stream);
}

int k4lz4_unpickle_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n,
                                int flags, void *stream)
{
    return run_device(ctx, KIND_UNPICKLE, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, 0, flags, stream);
}

int k4lz4_profile_batch_device(k4lz4_ctx *ctx, int decode, const uint8_t *src, const uint64_t *srcOff,
                               const int32_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const int32_t *dstCap,
                               int32_t *outLen, int64_t n, uint64_t *counters, void *stream)
{
    if (!ctx || !counters) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    ctx->prof = (unsigned long long *)counters;
    ctx->prof_pair = decode == 2;        /* 2: the two-waves-per-block decoder, 32 counters per block (parsing wave, copying wave) */
    ctx->prof_stamp = decode >= 4;       /* 4 / 5: the ordinary encode / decode kernels, which only record [8] start, [9] end, [10] HW_ID, [11] kernel */
    const int rc = run_device(ctx, (decode && decode != 4) ? KIND_DECODE : KIND_ENCODE, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n,
                              K4LZ4_L00_FAST, 0, stream);
    ctx->prof = nullptr;
    ctx->prof_stamp = false;
    return rc;
}

/* ---- frame layer -------------------------------------------------------------------------------- */
int k4lz4_xxh32_batch_device(k4lz4_ctx *ctx, const uint8_t *data, const uint64_t *off, const uint64_t *len,
                             uint32_t *out, int64_t n, uint32_t seed, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!data || !off || !len || !out))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t per_launch = (int64_t)1 << 24;
    for (int64_t first = 0; first < n; first += per_launch) {
        const int64_t cnt = std::min<int64_t>(per_launch, n - first);
        k4::HashArgs a{data, off + first, len + first, out + first, cnt, seed};
        hipLaunchKernelGGL(k4::k4_xxh32_kernel, dim3((unsigned)((cnt * 4 + k4::XXH_THREADS - 1) / k4::XXH_THREADS)),
                           dim3(k4::XXH_THREADS), 0, (hipStream_t)stream, a);
    }
    K4_HIP(ctx, hipGetLastError());
    return K4LZ4_OK;
}

int k4lz4_xxh32_batch(k4lz4_ctx *ctx, const uint8_t *data, const uint64_t *off, const uint64_t *len, uint32_t *out,
                      int64_t n, uint32_t seed)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!data || !off || !len || !out))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    HostStage s(ctx);
    s.span(data, off, n, [&](int64_t i) { return len[i]; });
    uint64_t *d_off, *d_len;
    uint32_t *d_out;
    s.meta(&d_off, n, s.in_off.data()); s.meta(&d_len, n, len); s.meta(&d_out, n);
    int rc;
    if ((rc = s.upload()) != K4LZ4_OK || (rc = k4lz4_xxh32_batch_device(ctx, ctx->d_src, d_off, d_len, d_out, n, seed, s.st)) != K4LZ4_OK)
        return rc;
    return s.finish({{out, d_out, (size_t)n * 4}});
}

int k4lz4_decode_chain_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *blkOff, const uint32_t *blkLen,
                                    const uint64_t *firstBlk, const uint32_t *nBlk, const int32_t *blockSize,
                                    const uint8_t *chained, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                                    int64_t *outLen, int64_t nStreams, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (nStreams < 0 || (nStreams > 0 && (!src || !blkOff || !blkLen || !firstBlk || !nBlk || !blockSize || !chained || !dst ||
                                          !dstOff || !dstCap || !outLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (nStreams == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    k4::ChainArgs a{src, blkOff, blkLen, firstBlk, nBlk, blockSize, chained, dst, dstOff, dstCap, (long long *)outLen, nStreams, ctx->d_status};
    const unsigned grid = (unsigned)((nStreams + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG);
    if (nStreams <= 16 * (int64_t)ctx->cu_count && !ctx->no_pair) {  /* room for two waves per stream */
        hipLaunchKernelGGL(k4::k4_decode_chain_pair_kernel, dim3((unsigned)((nStreams + k4::DECODE_PAIRS_PER_WG - 1) / k4::DECODE_PAIRS_PER_WG)),
                           dim3(128 * k4::DECODE_PAIRS_PER_WG), 0, (hipStream_t)stream, a);
    } else
        hipLaunchKernelGGL(k4::k4_decode_chain_kernel, dim3(grid), dim3(64 * k4::DECODE_WAVES_PER_WG), 0, (hipStream_t)stream, a);
    K4_HIP(ctx, hipGetLastError());
    return K4LZ4_OK;
}

int k4lz4_decode_chain_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *blkOff, const uint32_t *blkLen,
                             int64_t nBlocks, const uint64_t *firstBlk, const uint32_t *nBlk, const int32_t *blockSize,
                             const uint8_t *chained, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                             int64_t *outLen, int64_t nStreams)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (nStreams < 0 || nBlocks < 0 ||
        (nStreams > 0 && (!src || !firstBlk || !nBlk || !blockSize || !chained || !dst || !dstOff || !dstCap || !outLen)) ||
        (nBlocks > 0 && (!blkOff || !blkLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (nStreams == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    for (int64_t i = 0; i < nStreams; i++)
        if (firstBlk[i] + nBlk[i] > (uint64_t)nBlocks) return fail(ctx, K4LZ4_E_ARG, "stream refers to blocks outside the block table");
    HostStage s(ctx);
    s.span(src, blkOff, nBlocks, [&](int64_t i) { return (uint64_t)(blkLen[i] & 0x7fffffffu); });
    s.slots(nStreams, [&](int64_t i) { return dstCap[i]; }, true);
    uint64_t *d_boff, *d_first, *d_doff, *d_dcap;
    int64_t *d_out;
    uint32_t *d_blen, *d_nblk;
    int32_t *d_bsize;
    uint8_t *d_chained;
    s.meta(&d_boff, nBlocks, s.in_off.data()); s.meta(&d_blen, nBlocks, blkLen);
    s.meta(&d_first, nStreams, firstBlk); s.meta(&d_doff, nStreams, s.slot.data()); s.meta(&d_dcap, nStreams, dstCap);
    s.meta(&d_nblk, nStreams, nBlk); s.meta(&d_bsize, nStreams, blockSize); s.meta(&d_chained, nStreams, chained); s.meta(&d_out, nStreams);
    int rc;
    if ((rc = s.upload()) != K4LZ4_OK ||
        (rc = k4lz4_decode_chain_batch_device(ctx, ctx->d_src, d_boff, d_blen, d_first, d_nblk, d_bsize, d_chained, ctx->d_dst, d_doff,
                                              d_dcap, d_out, nStreams, s.st)) != K4LZ4_OK)
        return rc;
    return s.finish({{outLen, d_out, (size_t)nStreams * 8}}, dst, dstOff,
                    [&](int64_t i) { return outLen[i] > 0 && (uint64_t)outLen[i] <= dstCap[i] ? (size_t)outLen[i] : 0; });
}

int k4lz4_frame_assemble_device(k4lz4_ctx *ctx, const uint8_t *arena, const uint64_t *slotOff, const int32_t *outLen,
                                const uint32_t *blkSum, const uint64_t *recOff, int64_t nBlocks, const uint8_t *hdr,
                                const uint32_t *hdrLen, const uint32_t *hdrSum, const uint64_t *frameOff,
                                const uint64_t *tailOff, const uint32_t *contentSum, uint8_t *frames, uint64_t *frameLen,
                                int64_t nFrames, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (nBlocks < 0 || nFrames < 0 || (nBlocks > 0 && (!arena || !slotOff || !outLen || !recOff)) ||
        (nFrames > 0 && (!hdr || !hdrLen || !hdrSum || !frameOff || !tailOff || !frames || !frameLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    K4_HIP(ctx, hipSetDevice(ctx->device));
    if (nBlocks > 0) {
        k4::FrameBlocksArgs a{arena, slotOff, outLen, blkSum, recOff, frames, nBlocks};
        hipLaunchKernelGGL(k4::k4_frame_blocks_kernel, dim3((unsigned)((nBlocks + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    }
    if (nFrames > 0) {
        k4::FrameEdgesArgs e{hdr, hdrLen, hdrSum, frameOff, tailOff, contentSum, frames, frameLen, nFrames};
        hipLaunchKernelGGL(k4::k4_frame_edges_kernel, dim3((unsigned)((nFrames + 255) / 256)), dim3(256), 0, (hipStream_t)stream, e);
    }
    K4_HIP(ctx, hipGetLastError());
    return K4LZ4_OK;
}

int k4lz4_unpickle_sizes_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                int32_t *outLen, int64_t n, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!src || !srcOff || !srcLen || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    k4::BatchArgs a{};
    a.src = src; a.srcOff = srcOff; a.srcLen = srcLen; a.outLen = outLen; a.n = n;
    hipLaunchKernelGGL(k4::k4_unpickle_sizes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    K4_HIP(ctx, hipGetLastError());
    return K4LZ4_OK;
}

int k4lz4_encode_hc_chain_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen,
                                       const int32_t *blockSize, const int32_t *extraBlocks, const int32_t *dictLen, int64_t nStreams,
                                       uint8_t *dst, const uint64_t *dstOff, int32_t *outLen, int64_t nBlocks, int level, int flags,
                                       void *stream)
{
    return hc_chain_run(ctx, src, srcOff, srcLen, blockSize, extraBlocks, dictLen, nStreams, dst, dstOff, outLen, nBlocks, level, flags,
                        (hipStream_t)stream);
}

int k4lz4_encode_hc_chain_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen,
                                const int32_t *blockSize, const int32_t *extraBlocks, const int32_t *dictLen, int64_t nStreams,
                                uint8_t *dst, const uint64_t *dstOff, int32_t *outLen, int64_t nBlocks, int level, int flags)
{
    if (nStreams < 0 || nBlocks < 0 || (nStreams > 0 && (!src || !srcOff || !srcLen || !blockSize || !dst || !dstOff || !outLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    return chain_host(ctx, "k4lz4_encode_hc_chain_batch",
        [&](int64_t &nb) { return hc_chain_table(ctx, srcOff, srcLen, blockSize, extraBlocks, dictLen, nStreams, dstOff, nb, nullptr); },
        [&](HostStage &s, int64_t nb, int32_t *d_out, k4lz4_fast_chain_state *, k4lz4_fast_chain_state *) {
            return hc_chain_run(ctx, ctx->d_src, s.in_off.data(), srcLen, blockSize, extraBlocks, dictLen, nStreams, ctx->d_dst, s.slot.data(),
                                d_out, nb, level, flags, s.st);
        },
        src, srcOff, srcLen, blockSize, dictLen, nStreams, nullptr, nullptr, dst, dstOff, outLen, nBlocks);
}


int k4lz4_encode_fast_chain_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen,
                                         const int32_t *blockSize, const int32_t *extraBlocks, const int32_t *dictLen, int64_t nStreams,
                                         const k4lz4_fast_chain_state *stateIn, k4lz4_fast_chain_state *stateOut, uint8_t *dst,
                                         const uint64_t *dstOff, int32_t *outLen, int64_t nBlocks, int flags, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (nStreams < 0 || nBlocks < 0 || (nStreams > 0 && (!src || !srcOff || !srcLen || !blockSize || !dst || !dstOff || !outLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    int rc = fast_chain_flags(ctx, flags);
    if (rc != K4LZ4_OK) return rc;
    std::vector<uint32_t> cur0, sdict;
    if (stateIn && nStreams > 0) {
        /* the block table needs the two indices of every input state on the host (a strided copy: 8 bytes per state) */
        K4_HIP(ctx, hipSetDevice(ctx->device));
        std::vector<uint32_t> idx((size_t)nStreams * 2);
        K4_HIP(ctx, hipMemcpy2DAsync(idx.data(), 8, &stateIn[0].currentOffset, sizeof(k4lz4_fast_chain_state), 8, (size_t)nStreams,
                                     hipMemcpyDeviceToHost, (hipStream_t)stream));
        K4_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
        cur0.resize((size_t)nStreams); sdict.resize((size_t)nStreams);
        for (int64_t i = 0; i < nStreams; i++) { cur0[(size_t)i] = idx[(size_t)(2 * i)]; sdict[(size_t)i] = idx[(size_t)(2 * i + 1)]; }
    }
    return fast_chain_run(ctx, src, srcOff, srcLen, blockSize, extraBlocks, dictLen, stateIn ? cur0.data() : nullptr, stateIn ? sdict.data() : nullptr,
                          nStreams, stateIn, stateOut, dst, dstOff, outLen, nBlocks, flags, (hipStream_t)stream);
}

int k4lz4_encode_fast_chain_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int64_t *srcLen,
                                  const int32_t *blockSize, const int32_t *extraBlocks, const int32_t *dictLen, int64_t nStreams,
                                  const k4lz4_fast_chain_state *stateIn, k4lz4_fast_chain_state *stateOut, uint8_t *dst,
                                  const uint64_t *dstOff, int32_t *outLen, int64_t nBlocks, int flags)
{
    if (nStreams < 0 || nBlocks < 0 || (nStreams > 0 && (!src || !srcOff || !srcLen || !blockSize || !dst || !dstOff || !outLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    int rc = fast_chain_flags(ctx, flags);
    if (rc != K4LZ4_OK) return rc;
    std::vector<uint32_t> cur0, sdict;
    if (stateIn) fast_chain_indices(stateIn, nStreams, cur0, sdict);
    const uint32_t *c0 = stateIn ? cur0.data() : nullptr, *sd = stateIn ? sdict.data() : nullptr;
    return chain_host(ctx, "k4lz4_encode_fast_chain_batch",
        [&](int64_t &nb) { return fast_chain_table(ctx, srcOff, srcLen, blockSize, extraBlocks, dictLen, c0, sd, nStreams, dstOff, nb, nullptr); },
        [&](HostStage &s, int64_t nb, int32_t *d_out, k4lz4_fast_chain_state *d_in, k4lz4_fast_chain_state *d_outst) {
            return fast_chain_run(ctx, ctx->d_src, s.in_off.data(), srcLen, blockSize, extraBlocks, dictLen, c0, sd, nStreams, d_in, d_outst,
                                  ctx->d_dst, s.slot.data(), d_out, nb, flags, s.st);
        },
        src, srcOff, srcLen, blockSize, dictLen, nStreams, stateIn, stateOut, dst, dstOff, outLen, nBlocks);
}


/* ---- messages against shared dictionaries: the entry points of the path above the C ABI ------------- */
int k4lz4_encode_dict_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                                   const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags,
                                   const int32_t *dictIdx, const uint8_t *dict, const uint64_t *dictOff, const int32_t *dictLen,
                                   int32_t nDict, void *stream)
{
    return dict_encode_device(ctx, FAMILY_FAST, level, flags, DictBatch{src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, dictIdx},
                              DictSource{false, nullptr, dict, dictOff, dictLen, nDict}, stream);
}

int k4lz4_encode_dict_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                            const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags,
                            const int32_t *dictIdx, const uint8_t *dict, const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict)
{
    return dict_encode_host(ctx, FAMILY_FAST, level, flags, DictBatch{src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, dictIdx},
                            DictSource{false, nullptr, dict, dictOff, dictLen, nDict});
}

int k4lz4_encode_dict_hc_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                                      const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags,
                                      const int32_t *dictIdx, const uint8_t *dict, const uint64_t *dictOff, const int32_t *dictLen,
                                      int32_t nDict, void *stream)
{
    return dict_encode_device(ctx, FAMILY_HC, level, flags, DictBatch{src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, dictIdx},
                              DictSource{false, nullptr, dict, dictOff, dictLen, nDict}, stream);
}

int k4lz4_encode_dict_hc_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                               const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags,
                               const int32_t *dictIdx, const uint8_t *dict, const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict)
{
    return dict_encode_host(ctx, FAMILY_HC, level, flags, DictBatch{src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, dictIdx},
                            DictSource{false, nullptr, dict, dictOff, dictLen, nDict});
}

int k4lz4_encode_dictset_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                                      const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags,
                                      const int32_t *dictIdx, const k4lz4_dict_set *set, void *stream)
{
    return dict_encode_device(ctx, dict_family(level), level, flags, DictBatch{src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, dictIdx},
                              DictSource{true, set, nullptr, nullptr, nullptr, 0}, stream);
}

int k4lz4_encode_dictset_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                               const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags,
                               const int32_t *dictIdx, const k4lz4_dict_set *set)
{
    return dict_encode_host(ctx, dict_family(level), level, flags, DictBatch{src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, dictIdx},
                            DictSource{true, set, nullptr, nullptr, nullptr, 0});
}

int k4lz4_encode_dict_state(k4lz4_ctx *ctx, int32_t d, k4lz4_fast_chain_state *out)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    const uint8_t *table = out ? dict_loaded_table(ctx, FAMILY_FAST, d) : nullptr;
    if (!table)
        return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_dict_state: no such dictionary in the context's most recent k4lz4_encode_dict_batch call");
    K4_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->busy) K4_HIP(ctx, hipEventSynchronize(ctx->ev_busy));
    return dict_fast_state(ctx, table, ctx->dict_fast.kept[(size_t)d], out);
}

int k4lz4_encode_dict_hc_state(k4lz4_ctx *ctx, int32_t d, uint32_t *hashTable, uint16_t *chainTable, int32_t *keptLen)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    const uint8_t *table = hashTable && chainTable && keptLen ? dict_loaded_table(ctx, FAMILY_HC, d) : nullptr;
    if (!table)
        return fail(ctx, K4LZ4_E_ARG, "k4lz4_encode_dict_hc_state: no such dictionary in the context's most recent k4lz4_encode_dict_hc_batch call");
    K4_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->busy) K4_HIP(ctx, hipEventSynchronize(ctx->ev_busy));
    return dict_hc_state(ctx, table, ctx->dict_hc.kept[(size_t)d], hashTable, chainTable, keptLen);
}

/* ---- k4lz4_dict_set (k4lz4_dict_set.hpp) ---------------------------------------------------------------------
 * Which bytes are kept is the HC family's rule (the last 64 KiB of every length down to one byte: the decoders need them whatever
 * the families), and that dict_list is the HC family's; the fast family has its own (below 8 bytes: the empty table, dictSize 0).
 * Every distinct kept range gets a region of the set's memory at the next 64-byte step. */
struct DictSetPlan {
    DictList bytes, fast;
    std::vector<uint64_t> regionAt;        /* per distinct kept range (= per HC table) */
    uint64_t total = 0;
};

static void dict_set_carve(Carve &c, const DictSetPlan &p, size_t nd, int families, k4lz4_dict_set &s, std::vector<uint64_t> &regionAt)
{
    uint8_t *b;
    regionAt.assign(p.bytes.rep.size(), 0);
    for (size_t t = 0; t < p.bytes.rep.size(); t++) { regionAt[t] = c.at; c.take(b, (size_t)p.bytes.keptLen[p.bytes.rep[t]]); }
    c.take(b, 64);                                                        /* nothing lies right behind the last dictionary byte */
    c.take(s.dec_off, nd); c.take(s.dec_len, nd);
    auto family = [&](const DictFamily &fam, const DictList &l) {
        k4lz4_dict_set::Family &f = s.*fam.in_set;
        const size_t nt = std::max<size_t>(l.rep.size(), 1);
        c.take(f.toff, nt); c.take(f.tlen, nt); c.take(f.eoff, nd); c.take(f.elen, nd); c.take(f.etab, nd);
        c.take(f.tables, nt * fam.table_bytes);
    };
    if (families & K4LZ4_DICT_FAST) family(FAMILY_FAST, p.fast);
    if (families & K4LZ4_DICT_HC) family(FAMILY_HC, p.bytes);
}

static int dict_set_plan(k4lz4_ctx *ctx, const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict, int families, DictSetPlan &p)
{
    if (families == 0 || (families & ~(K4LZ4_DICT_FAST | K4LZ4_DICT_HC)))
        return fail(ctx, K4LZ4_E_ARG, "k4lz4_dict_set: families is a mask of K4LZ4_DICT_FAST and K4LZ4_DICT_HC, at least one of them");
    if (nDict < 0 || (nDict > 0 && (!dictOff || !dictLen))) return fail(ctx, K4LZ4_E_ARG, "k4lz4_dict_set: bad dictionary list");
    for (int32_t d = 0; d < nDict; d++)
        if (dictLen[d] < 0) return fail(ctx, K4LZ4_E_ARG, "k4lz4_dict_set: negative dictLen");
    int rc;
    try {
        if ((rc = dict_list(ctx, FAMILY_HC.min_kept, "k4lz4_dict_set", dictOff, dictLen, nDict, nullptr, p.bytes)) != K4LZ4_OK) return rc;
        if ((families & K4LZ4_DICT_FAST) &&
            (rc = dict_list(ctx, FAMILY_FAST.min_kept, "k4lz4_dict_set", dictOff, dictLen, nDict, nullptr, p.fast)) != K4LZ4_OK)
            return rc;
        Carve m{nullptr};
        k4lz4_dict_set measure;
        dict_set_carve(m, p, (size_t)nDict, families, measure, p.regionAt);
        p.total = m.at;
    } catch (...) { return fail(ctx, K4LZ4_E_NOMEM, "out of host memory"); }
    return K4LZ4_OK;
}

int k4lz4_dict_set_layout(const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict, int families, int32_t *keptLen, uint64_t *keptAt,
                          int32_t *tableFast, int32_t *tableHc, uint64_t *bytes)
{
    DictSetPlan p;
    const int rc = dict_set_plan(nullptr, dictOff, dictLen, nDict, families, p);
    if (rc != K4LZ4_OK) return rc;
    for (int32_t d = 0; d < nDict; d++) {
        if (keptLen) keptLen[d] = (int32_t)p.bytes.keptLen[(size_t)d];
        if (keptAt) keptAt[d] = p.regionAt[p.bytes.table[(size_t)d]];
        if (tableFast) tableFast[d] = (families & K4LZ4_DICT_FAST) ? (int32_t)p.fast.table[(size_t)d] : -1;
        if (tableHc) tableHc[d] = (families & K4LZ4_DICT_HC) ? (int32_t)p.bytes.table[(size_t)d] : -1;
    }
    if (bytes) *bytes = p.total;
    return K4LZ4_OK;
}

void k4lz4_dict_set_destroy(k4lz4_dict_set *set)
{
    if (!set) return;
    /* calls that read the set may still run on any stream of its device: they are waited for */
    if (set->buf && hipSetDevice(set->device) == hipSuccess) { (void)hipDeviceSynchronize(); (void)hipFree(set->buf); }
    (void)hipGetLastError();
    delete set;
}

/* dict: a host pointer, or a device pointer that is valid once st reaches this point */
static int dict_set_create(k4lz4_ctx *ctx, const uint8_t *dict, bool on_device, const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict,
                           int families, k4lz4_dict_set **out, hipStream_t st)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (!out) return fail(ctx, K4LZ4_E_ARG, "k4lz4_dict_set_create: NULL result pointer");
    *out = nullptr;
    DictSetPlan p;
    int rc = dict_set_plan(ctx, dictOff, dictLen, nDict, families, p);
    if (rc != K4LZ4_OK) return rc;
    for (int32_t d = 0; d < nDict; d++)
        if (dictLen[d] > 0 && !dict) return fail(ctx, K4LZ4_E_ARG, "k4lz4_dict_set_create: NULL dictionary buffer");
    K4_HIP(ctx, hipSetDevice(ctx->device));
    struct Deleter { void operator()(k4lz4_dict_set *s) const { k4lz4_dict_set_destroy(s); } };
    std::unique_ptr<k4lz4_dict_set, Deleter> s(new (std::nothrow) k4lz4_dict_set);
    if (!s) return fail(ctx, K4LZ4_E_NOMEM, "out of host memory");
    const size_t nd = (size_t)nDict;
    std::vector<uint64_t> dec_off, w_toff[2], w_eoff[2];
    std::vector<int32_t> dec_len;
    std::vector<uint32_t> w_tlen[2], w_elen[2], w_etab[2];
    try {
        s->device = ctx->device; s->nDict = nDict; s->families = families; s->bytes = p.total;
        s->keptAt.resize(nd); s->keptLen.resize(nd);
        for (size_t d = 0; d < nd; d++) { s->keptAt[d] = p.regionAt[p.bytes.table[d]]; s->keptLen[d] = (int32_t)p.bytes.keptLen[d]; }
        dec_off = s->keptAt; dec_len = s->keptLen;
        for (int k = 0; k < 2; k++) {
            if (!(families & (k ? K4LZ4_DICT_HC : K4LZ4_DICT_FAST))) continue;
            DictList l = k ? p.bytes : p.fast;
            k4lz4_dict_set::Family &f = k ? s->hc : s->fast;
            f.on = true; f.table = l.table; f.kept = l.keptLen; f.ntables = (int64_t)std::max<size_t>(l.rep.size(), 1);
            for (size_t d = 0; d < nd; d++) l.keptOff[d] = l.keptLen[d] ? s->keptAt[d] : 0;     /* the kept bytes lie in the set's memory */
            w_toff[k].assign((size_t)f.ntables, 0); w_tlen[k].assign((size_t)f.ntables, 0);     /* an empty list: one empty table */
            w_eoff[k].assign(nd, 0); w_elen[k].assign(nd, 0); w_etab[k].assign(nd, 0);
            dict_words(l, w_toff[k].data(), w_tlen[k].data(), w_eoff[k].data(), w_elen[k].data(), w_etab[k].data());
        }
    } catch (...) { return fail(ctx, K4LZ4_E_NOMEM, "out of host memory"); }
    if (hipMalloc((void **)&s->buf, (size_t)p.total) != hipSuccess) { (void)hipGetLastError(); s->buf = nullptr; return fail(ctx, K4LZ4_E_NOMEM, "out of device memory"); }
    Carve cv{s->buf};
    std::vector<uint64_t> at;
    dict_set_carve(cv, p, nd, families, *s, at);
    for (size_t t = 0; t < p.bytes.rep.size(); t++) {
        const uint32_t d = p.bytes.rep[t];
        if (p.bytes.keptLen[d])
            K4_HIP(ctx, hipMemcpyAsync(s->buf + at[t], dict + p.bytes.keptOff[d], (size_t)p.bytes.keptLen[d],
                                       on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    auto up = [&](void *dev, const void *host, size_t bytes) {
        return bytes ? hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    K4_HIP(ctx, up(s->dec_off, dec_off.data(), nd * 8));
    K4_HIP(ctx, up(s->dec_len, dec_len.data(), nd * 4));
    for (int k = 0; k < 2; k++) {
        k4lz4_dict_set::Family &f = k ? s->hc : s->fast;
        if (!f.on) continue;
        const size_t nt = (size_t)f.ntables;
        K4_HIP(ctx, up(f.toff, w_toff[k].data(), nt * 8));
        K4_HIP(ctx, up(f.tlen, w_tlen[k].data(), nt * 4));
        K4_HIP(ctx, up(f.eoff, w_eoff[k].data(), nd * 8));
        K4_HIP(ctx, up(f.elen, w_elen[k].data(), nd * 4));
        K4_HIP(ctx, up(f.etab, w_etab[k].data(), nd * 4));
        (k ? FAMILY_HC : FAMILY_FAST).load(st, (unsigned)nt, s->buf, f.toff, f.tlen, f.tables);
        if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(st); return fail(ctx, K4LZ4_E_HIP, "k4lz4_dict_set_create: kernel launch failed"); }
        f.loads++;
    }
    K4_HIP(ctx, hipStreamSynchronize(st));                               /* the host words above and the caller's bytes are free again */
    *out = s.release();
    return K4LZ4_OK;
}

int k4lz4_dict_set_create(k4lz4_ctx *ctx, const uint8_t *dict, const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict, int families,
                          k4lz4_dict_set **set)
{
    return dict_set_create(ctx, dict, false, dictOff, dictLen, nDict, families, set, ctx ? ctx->stream : nullptr);
}

int k4lz4_dict_set_create_device(k4lz4_ctx *ctx, const uint8_t *dict, const uint64_t *dictOff, const int32_t *dictLen, int32_t nDict,
                                 int families, k4lz4_dict_set **set, void *stream)
{
    return dict_set_create(ctx, dict, true, dictOff, dictLen, nDict, families, set, (hipStream_t)stream);
}

int k4lz4_dict_set_info(const k4lz4_dict_set *set, int64_t out[8])
{
    if (!set || !out) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_dict_set_info: NULL argument");
    out[0] = set->nDict; out[1] = set->fast.ntables; out[2] = set->hc.ntables; out[3] = (int64_t)set->bytes;
    out[4] = set->families; out[5] = set->device; out[6] = set->fast.loads; out[7] = set->hc.loads;
    return K4LZ4_OK;
}

int k4lz4_dict_set_state(const k4lz4_dict_set *set, int32_t d, k4lz4_fast_chain_state *out)
{
    if (!set || !out || d < 0 || d >= set->nDict || !set->fast.on)
        return fail(nullptr, K4LZ4_E_ARG, "k4lz4_dict_set_state: no such dictionary, or a set without K4LZ4_DICT_FAST");
    K4_HIP(nullptr, hipSetDevice(set->device));
    return dict_fast_state(nullptr, set->fast.tables + FAMILY_FAST.table_bytes * set->fast.table[(size_t)d], set->fast.kept[(size_t)d], out);
}

int k4lz4_dict_set_hc_state(const k4lz4_dict_set *set, int32_t d, uint32_t *hashTable, uint16_t *chainTable, int32_t *keptLen)
{
    if (!set || !hashTable || !chainTable || !keptLen || d < 0 || d >= set->nDict || !set->hc.on)
        return fail(nullptr, K4LZ4_E_ARG, "k4lz4_dict_set_hc_state: no such dictionary, or a set without K4LZ4_DICT_HC");
    K4_HIP(nullptr, hipSetDevice(set->device));
    return dict_hc_state(nullptr, set->hc.tables + FAMILY_HC.table_bytes * set->hc.table[(size_t)d], set->hc.kept[(size_t)d], hashTable, chainTable,
                         keptLen);
}

static int dictset_decode_args(k4lz4_ctx *ctx, const void *src, const void *srcOff, const void *srcLen, const void *dst, const void *dstOff,
                               const void *dstCap, const void *outLen, int64_t n, const void *dictIdx, const k4lz4_dict_set *set)
{
    const int rc = check_batch_args(ctx, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n);
    if (rc != K4LZ4_OK) return rc;
    if (!set) return fail(ctx, K4LZ4_E_ARG, "k4lz4_decode_dictset_batch: set is NULL");
    if (set->device != ctx->device) return fail(ctx, K4LZ4_E_ARG, "k4lz4_decode_dictset_batch: the set lives on another device than the context");
    if (n > 0 && !dictIdx) return fail(ctx, K4LZ4_E_ARG, "k4lz4_decode_dictset_batch: NULL dictIdx");
    return K4LZ4_OK;
}

int k4lz4_decode_dictset_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                                      const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int flags,
                                      const int32_t *dictIdx, const k4lz4_dict_set *set, void *stream)
{
    int rc = dictset_decode_args(ctx, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, dictIdx, set);
    if (rc != K4LZ4_OK || n == 0) return rc;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    k4::DictPickArgs a{};
    auto layout = [&](Carve &cv) { cv.take(a.dictOff, (size_t)n); cv.take(a.dictLen, (size_t)n); cv.take(a.cap, (size_t)n); cv.take(a.dictMode, (size_t)n); };
    Carve m{nullptr};
    layout(m);
    if ((rc = grow_scratch(ctx, &ctx->d_dpick, &ctx->d_dpick_cap, m.at + 64)) != K4LZ4_OK) return rc;
    Carve dv{ctx->d_dpick};
    layout(dv);
    a.dictIdx = dictIdx; a.entryOff = set->dec_off; a.entryLen = set->dec_len; a.dstCap = dstCap; a.outLen = outLen; a.status = ctx->d_status;
    a.n = n; a.nDict = set->nDict; a.phase = 0;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (grid.x == 0 || n > 0x7fffffffll * 256) return fail(ctx, K4LZ4_E_ARG, "k4lz4_decode_dictset_batch: too many messages");
    K4_HIP(ctx, order_after_ctx(ctx, st));
    hipLaunchKernelGGL(k4::k4_dict_pick_kernel, grid, dim3(256), 0, st, a);
    mark_busy(ctx, st);
    const DictArgs dd{set->buf, a.dictOff, a.dictLen, a.dictMode};
    rc = launch(ctx, KIND_DECODE, src, srcOff, srcLen, dst, dstOff, a.cap, outLen, n, 0, flags, st, &dd);
    a.phase = 1;
    hipLaunchKernelGGL(k4::k4_dict_pick_kernel, grid, dim3(256), 0, st, a);
    if (hipGetLastError() != hipSuccess && rc == K4LZ4_OK) rc = fail(ctx, K4LZ4_E_HIP, "k4lz4_decode_dictset_batch: kernel launch failed");
    mark_busy(ctx, st);
    return rc;
}

int k4lz4_decode_dictset_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                               const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int flags, const int32_t *dictIdx,
                               const k4lz4_dict_set *set)
{
    int rc = dictset_decode_args(ctx, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, dictIdx, set);
    if (rc != K4LZ4_OK) return rc;
    for (int64_t i = 0; i < n; i++)
        if (dictIdx[i] < -1 || dictIdx[i] >= set->nDict) return fail(ctx, K4LZ4_E_ARG, "k4lz4_decode_dictset_batch: a dictIdx outside the dictionary list");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    /* the pick kernel's arithmetic, on the host; the dictionaries are where they have been since create */
    std::vector<uint64_t> h_off((size_t)n, 0);
    std::vector<int32_t> h_len((size_t)n, 0);
    std::vector<signed char> h_mode((size_t)n, 2);
    for (int64_t i = 0; i < n; i++)
        if (dictIdx[i] >= 0) { h_off[(size_t)i] = set->keptAt[(size_t)dictIdx[i]]; h_len[(size_t)i] = set->keptLen[(size_t)dictIdx[i]]; }
    HostStage s(ctx);
    s.span(src, srcOff, n, [&](int64_t i) { return (uint64_t)std::max<int32_t>(srcLen[i], 0); });
    s.slots(n, [&](int64_t i) { return (uint64_t)std::max<int32_t>(dstCap[i], 0); }, true);
    uint64_t *d_off, *d_doff, *d_dictoff;
    int32_t *d_len, *d_cap, *d_out, *d_dictlen;
    signed char *d_mode;
    s.meta(&d_off, n, s.in_off.data()); s.meta(&d_len, n, srcLen); s.meta(&d_doff, n, s.slot.data()); s.meta(&d_cap, n, dstCap);
    s.meta(&d_dictoff, n, h_off.data()); s.meta(&d_dictlen, n, h_len.data()); s.meta(&d_mode, n, h_mode.data()); s.meta(&d_out, n);
    if ((rc = s.upload()) != K4LZ4_OK) return rc;
    const DictArgs dd{set->buf, d_dictoff, d_dictlen, d_mode};
    if ((rc = launch(ctx, KIND_DECODE, ctx->d_src, d_off, d_len, ctx->d_dst, d_doff, d_cap, d_out, n, 0, flags, s.st, &dd)) != K4LZ4_OK) return rc;
    return finish_blocks(s, outLen, d_out, n, dst, dstOff, dstCap);
}

/* ---- frame reader (k4lz4_frame_read.hpp) ---------------------------------------------------------------- */

/* frames with a DictID against a set (k4lz4_frame_dict.hpp): the refusals, and the call's scratch -- the id table
 * (a host array in both forms, through ctx->fdict_plan) and the entry every frame resolves to */
constexpr int64_t FRAME_DICT_WAVES_PER_CU = 16;      /* of the in-order decoder, a 64 KiB window each: one residency at four waves per SIMD */

static int frame_dict_args(k4lz4_ctx *ctx, const k4lz4_dict_set *set, const uint32_t *dictIds, const char *what)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (!set) return K4LZ4_OK;
    if (set->device != ctx->device) return fail(ctx, K4LZ4_E_ARG, std::string(what) + ": the set lives on another device than the context");
    if (!dictIds) return fail(ctx, K4LZ4_E_ARG, std::string(what) + ": NULL dictIds with a set");
    return K4LZ4_OK;
}

static int frame_dict_ids(k4lz4_ctx *ctx, const k4lz4_dict_set *set, const uint32_t *dictIds, int64_t n, hipStream_t st, uint32_t **ids,
                          int32_t **idx)
{
    const size_t nd = (size_t)set->nDict;
    auto layout = [&](Carve &cv) { cv.take(*ids, nd); cv.take(*idx, (size_t)n); };
    Carve m{nullptr};
    layout(m);
    int rc;
    if ((rc = grow_scratch(ctx, &ctx->d_fdx, &ctx->d_fdx_cap, m.at + 64)) != K4LZ4_OK) return rc;
    Carve dv{ctx->d_fdx};
    layout(dv);
    if (!nd) return K4LZ4_OK;
    if ((rc = plan_begin(ctx, ctx->fdict_plan, nd * 4, false)) != K4LZ4_OK) return rc;
    memcpy(ctx->fdict_plan.host.data(), dictIds, nd * 4);
    /* (not plan_send: the callers have put st behind the context's work already, in front of their own scratch) */
    K4_HIP(ctx, hipMemcpyAsync(*ids, ctx->fdict_plan.host.data(), nd * 4, hipMemcpyHostToDevice, st));
    K4_HIP(ctx, hipEventRecord(ctx->fdict_plan.ev, st));
    return K4LZ4_OK;
}

/* the walk of a call: the plain one, or with a set the one that resolves DictIDs (w.counters, w.outSize, w.outStatus as the call wants) */
static int frame_walk(k4lz4_ctx *ctx, k4::FrameWalkArgs w, const k4lz4_dict_set *set, const uint32_t *dictIds, int32_t *outDictIdx,
                      hipStream_t st, int32_t **idx)
{
    const dim3 grid((unsigned)((w.n + 255) / 256));
    *idx = nullptr;
    if (!set) {
        hipLaunchKernelGGL(k4::k4_frame_walk_kernel, grid, dim3(256), 0, st, w);
        if (outDictIdx) K4_HIP(ctx, hipMemsetAsync(outDictIdx, 0xff, (size_t)w.n * 4, st));      /* -1: none */
        return K4LZ4_OK;
    }
    uint32_t *ids = nullptr;
    int rc;
    if ((rc = frame_dict_ids(ctx, set, dictIds, w.n, st, &ids, idx)) != K4LZ4_OK) return rc;
    const k4::FrameWalkIds wd{ids, set->nDict, *idx, outDictIdx, w.counters ? w.counters + k4::FRC_DICT_CHAINED : nullptr};
    hipLaunchKernelGGL(k4::k4_frame_walk_dict_kernel, grid, dim3(256), 0, st, w, wd);
    return K4LZ4_OK;
}

static int frame_sizes_run(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                           uint64_t *outSize, int32_t *outStatus, int32_t *outDictIdx, const k4lz4_dict_set *set, const uint32_t *dictIds,
                           void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!src || !frameOff || !frameLen || !outSize || !outStatus))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    K4_HIP(ctx, order_after_ctx(ctx, st));
    k4::FrameTab t;
    unsigned long long *cnt;
    int rc;
    int32_t *idx;
    if ((rc = frame_scratch(ctx, n, &t, &cnt)) != K4LZ4_OK) return rc;
    k4::FrameWalkArgs w{src, frameOff, frameLen, n, t, nullptr, outSize, outStatus};
    if ((rc = frame_walk(ctx, w, set, dictIds, outDictIdx, st, &idx)) != K4LZ4_OK) return rc;
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    return K4LZ4_OK;
}

int k4lz4_frame_sizes_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                             uint64_t *outSize, int32_t *outStatus, void *stream)
{
    return frame_sizes_run(ctx, src, frameOff, frameLen, n, outSize, outStatus, nullptr, nullptr, nullptr, stream);
}

int k4lz4_frame_sizes_dictset_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                                     uint64_t *outSize, int32_t *outStatus, int32_t *outDictIdx, const k4lz4_dict_set *set,
                                     const uint32_t *dictIds, void *stream)
{
    const int rc = frame_dict_args(ctx, set, dictIds, "k4lz4_frame_sizes_dictset");
    if (rc != K4LZ4_OK) return rc;
    return frame_sizes_run(ctx, src, frameOff, frameLen, n, outSize, outStatus, outDictIdx, set, dictIds, stream);
}

/* set == nullptr: k4lz4_decode_frames_device as it always was; with a set, k4lz4_decode_frames_dictset_device */
static int decode_frames_run(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                             uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen, const k4lz4_dict_set *set,
                             const uint32_t *dictIds, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!src || !frameOff || !frameLen || !dst || !dstOff || !dstCap || !outLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    K4_HIP(ctx, order_after_ctx(ctx, st));
    k4::FrameTab t;
    k4::BlockTab b;
    unsigned long long *cnt;
    int rc;
    int32_t *idx;
    if ((rc = frame_scratch(ctx, n, &t, &cnt)) != K4LZ4_OK) return rc;
    const unsigned fgrid = (unsigned)((n + 255) / 256);
    K4_HIP(ctx, hipMemsetAsync(cnt, 0, 64, st));
    k4::FrameWalkArgs w{src, frameOff, frameLen, n, t, cnt, nullptr, nullptr};
    if ((rc = frame_walk(ctx, w, set, dictIds, nullptr, st, &idx)) != K4LZ4_OK) return rc;
    hipLaunchKernelGGL(k4::k4_frame_scan_kernel, dim3(1), dim3(k4::FRAME_SCAN_THREADS), 0, st, t.nblk, t.first, (long long)n, cnt);
    K4_HIP(ctx, hipGetLastError());
    /* the one wait: the block count sizes the table (and says which passes have work) */
    unsigned long long h[k4::FRC_DICT_COUNT];       /* (the last word stays 0 without a set) */
    K4_HIP(ctx, hipMemcpyAsync(h, cnt, sizeof h, hipMemcpyDeviceToHost, st));
    K4_HIP(ctx, hipStreamSynchronize(st));
    const int64_t nb = (int64_t)h[k4::FRC_BLOCKS];
    if ((rc = block_scratch(ctx, nb, &b)) != K4LZ4_OK) return rc;
    /* with a set: every block's dictionary words, the in-order work dealt to the two decoders, and the windows of the dictionary
     * decoder's waves -- none when no chained frame resolved to an entry: only such frames use them */
    k4::FrameDictRowsArgs ra{};
    uint8_t *windows = nullptr;
    uint32_t *n_plain = nullptr, *n_dict = nullptr;
    const int64_t cwaves = (std::min<int64_t>(n, FRAME_DICT_WAVES_PER_CU * (int64_t)ctx->cu_count) + k4::DECODE_WAVES_PER_WG - 1) / k4::DECODE_WAVES_PER_WG *
                           k4::DECODE_WAVES_PER_WG;                 /* whole workgroups: every wave of the grid has a window */
    if (set) {
        const size_t rows = (size_t)std::max<int64_t>(nb, 1);
        auto layout = [&](Carve &cv) {
            cv.take(ra.dictOff, rows); cv.take(ra.dictLen, rows); cv.take(ra.dictMode, rows);
            cv.take(n_plain, (size_t)n); cv.take(n_dict, (size_t)n);
            cv.take(windows, h[k4::FRC_DICT_CHAINED] ? (size_t)cwaves * k4::FRAME_DICT_WINDOW : 0);
        };
        Carve m{nullptr};
        layout(m);
        if ((rc = grow_scratch(ctx, &ctx->d_fdb, &ctx->d_fdb_cap, m.at + 64)) != K4LZ4_OK) return rc;
        Carve dv{ctx->d_fdb};
        layout(dv);
        ra.owner = b.owner; ra.dictIdx = idx; ra.entryOff = set->dec_off; ra.entryLen = set->dec_len; ra.nb = nb;
    }
    k4::FrameFillArgs fa{src, frameOff, dstOff, dstCap, n, t, b};
    hipLaunchKernelGGL(k4::k4_frame_fill_kernel, dim3(fgrid), dim3(256), 0, st, fa);
    K4_HIP(ctx, hipGetLastError());
    if (nb && h[k4::FRC_BSUM_FRAMES]) {
        if ((rc = k4lz4_xxh32_batch_device(ctx, src, b.off, b.hlen, b.got, nb, 0, st)) != K4LZ4_OK) return rc;
        hipLaunchKernelGGL(k4::k4_frame_bsum_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, t, b, (long long)nb);
    }
    if (nb && h[k4::FRC_INDEP_BLOCKS]) {
        if (set) hipLaunchKernelGGL(k4::k4_frame_dict_rows_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, ra);
        const DictArgs dd{set ? set->buf : nullptr, ra.dictOff, ra.dictLen, ra.dictMode};
        if ((rc = launch(ctx, KIND_DECODE, src, b.off, b.srcLen, dst, b.dstOff, b.dstCap, b.outLen, nb, 0, 0, st, set ? &dd : nullptr)) != K4LZ4_OK)
            return rc;
    }
    if (nb) hipLaunchKernelGGL(k4::k4_frame_place_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st, src, dst, t, b, (long long)nb);
    hipLaunchKernelGGL(k4::k4_frame_route_kernel, dim3(fgrid), dim3(256), 0, st, t, (long long)n);
    K4_HIP(ctx, hipGetLastError());
    /* chained frames, and independent ones whose blocks did not fill their places: in order, one stream per frame (frames
     * without such work have no blocks there) */
    if (set) {
        /* frames without an entry (or with an empty one) keep the plain call's decoders; those with one follow, and write only their own results */
        hipLaunchKernelGGL(k4::k4_frame_dict_split_kernel, dim3(fgrid), dim3(256), 0, st, t.nSerial, idx, set->dec_len, n_plain, n_dict, (long long)n);
        if ((rc = k4lz4_decode_chain_batch_device(ctx, src, b.off, b.len, t.first, n_plain, t.bsize, t.chained, dst, dstOff, dstCap, t.serialOut, n,
                                                  st)) != K4LZ4_OK)
            return rc;
        k4::ChainDictArgs ca{{src, b.off, b.len, t.first, n_dict, t.bsize, t.chained, dst, dstOff, dstCap, (long long *)t.serialOut, n, ctx->d_status},
                             idx, set->buf, set->dec_off, set->dec_len, windows};
        K4_LAUNCH_WAVES(k4::k4_decode_chain_dict_kernel, cwaves, k4::DECODE_WAVES_PER_WG, st, ca);
        K4_HIP(ctx, hipGetLastError());
    } else if ((rc = k4lz4_decode_chain_batch_device(ctx, src, b.off, b.len, t.first, t.nSerial, t.bsize, t.chained, dst, dstOff, dstCap,
                                                     t.serialOut, n, st)) != K4LZ4_OK)
        return rc;
    hipLaunchKernelGGL(k4::k4_frame_settle_kernel, dim3(fgrid), dim3(256), 0, st, t, dstCap, (long long)n);
    if (h[k4::FRC_CSUM_FRAMES]) {
        if ((rc = k4lz4_xxh32_batch_device(ctx, dst, dstOff, t.hashLen, t.sum, n, 0, st)) != K4LZ4_OK) return rc;
    }
    hipLaunchKernelGGL(k4::k4_frame_finish_kernel, dim3(fgrid), dim3(256), 0, st, t, outLen, (long long)n,
                       h[k4::FRC_CSUM_FRAMES] ? 1 : 0);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    return K4LZ4_OK;
}

int k4lz4_decode_frames_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                               uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen, void *stream)
{
    return decode_frames_run(ctx, src, frameOff, frameLen, n, dst, dstOff, dstCap, outLen, nullptr, nullptr, stream);
}

int k4lz4_decode_frames_dictset_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                                       uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen,
                                       const k4lz4_dict_set *set, const uint32_t *dictIds, void *stream)
{
    const int rc = frame_dict_args(ctx, set, dictIds, "k4lz4_decode_frames_dictset");
    if (rc != K4LZ4_OK) return rc;
    return decode_frames_run(ctx, src, frameOff, frameLen, n, dst, dstOff, dstCap, outLen, set, dictIds, stream);
}

int k4lz4_frame_sizes(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                      uint64_t *outSize, int32_t *outStatus)
{
    return host_sizes(k4lz4_frame_sizes_device, ctx, src, frameOff, frameLen, n, outSize, outStatus);
}

int k4lz4_decode_frames(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                        uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen)
{
    return host_streams(k4lz4_decode_frames_device, ctx, src, frameOff, frameLen, n, dst, dstOff, dstCap, outLen, /* zero */ true,
                        /* capped */ true);
}

/* the allowCopy rule behind an encoder that takes no flags (the dictionary encoders): k4_allow_copy_kernel over the call's blocks */
int k4lz4_allow_copy_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                                  const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, void *stream)
{
    const int rc = check_batch_args(ctx, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n);
    if (rc != K4LZ4_OK || n == 0) return rc;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    for (int64_t first = 0; first < n; first += (int64_t)1 << 24) {
        const int64_t cnt = std::min<int64_t>((int64_t)1 << 24, n - first);
        k4::BatchArgs a{};
        a.src = src; a.srcOff = srcOff + first; a.srcLen = srcLen + first;
        a.dst = dst; a.dstOff = dstOff + first; a.dstCap = dstCap + first; a.outLen = outLen + first; a.n = cnt;
        hipLaunchKernelGGL(k4::k4_allow_copy_kernel, dim3((unsigned)((cnt + 3) / 4)), dim3(256), 0, st, a);
    }
    K4_HIP(ctx, hipGetLastError());
    return K4LZ4_OK;
}

int k4lz4_frame_sizes_dictset(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                              uint64_t *outSize, int32_t *outStatus, int32_t *outDictIdx, const k4lz4_dict_set *set, const uint32_t *dictIds)
{
    int rc = frame_dict_args(ctx, set, dictIds, "k4lz4_frame_sizes_dictset");
    if (rc != K4LZ4_OK) return rc;
    if (n < 0 || (n > 0 && (!src || !frameOff || !frameLen || !outSize || !outStatus))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    HostStage s(ctx);
    s.span(src, frameOff, n, [&](int64_t i) { return frameLen[i]; });
    uint64_t *d_off, *d_len, *d_size;
    int32_t *d_status, *d_idx;
    s.meta(&d_off, n, s.in_off.data()); s.meta(&d_len, n, frameLen); s.meta(&d_size, n); s.meta(&d_status, n); s.meta(&d_idx, n);
    if ((rc = s.upload()) != K4LZ4_OK ||
        (rc = frame_sizes_run(ctx, ctx->d_src, d_off, d_len, n, d_size, d_status, d_idx, set, dictIds, s.st)) != K4LZ4_OK)
        return rc;
    return s.finish({{outSize, d_size, (size_t)n * 8}, {outStatus, d_status, (size_t)n * 4}, {outDictIdx, d_idx, outDictIdx ? (size_t)n * 4 : 0}});
}

int k4lz4_decode_frames_dictset(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *frameOff, const uint64_t *frameLen, int64_t n,
                                uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen, const k4lz4_dict_set *set,
                                const uint32_t *dictIds)
{
    const int rc = frame_dict_args(ctx, set, dictIds, "k4lz4_decode_frames_dictset");
    if (rc != K4LZ4_OK) return rc;
    auto device = [&](k4lz4_ctx *c, const uint8_t *s, const uint64_t *off, const uint64_t *len, int64_t count, uint8_t *d, const uint64_t *dOff,
                      const uint64_t *dCap, int64_t *out, void *st) {
        return decode_frames_run(c, s, off, len, count, d, dOff, dCap, out, set, dictIds, st);
    };
    return host_streams(device, ctx, src, frameOff, frameLen, n, dst, dstOff, dstCap, outLen, /* zero */ true, /* capped */ true);
}

/* ---- legacy formats: LZ4Wrapper, LZ4Stream (k4lz4_legacy.hpp) ------------------------------------------ */
int k4lz4_wrap_bound(int srcLen) { return srcLen < 0 || srcLen > 0x7fffffff - 8 ? 0 : 8 + srcLen; }

int k4lz4_wrap_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                     const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int high, int flags)
{
    return run_host(ctx, KIND_WRAP, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, high ? K4LZ4_L09_HC : K4LZ4_L00_FAST,
                    flags & (K4LZ4_FLAG_X32 | K4LZ4_FLAG_NO_REORDER));
}

int k4lz4_wrap_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                            const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int high, int flags, void *stream)
{
    return run_device(ctx, KIND_WRAP, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, high ? K4LZ4_L09_HC : K4LZ4_L00_FAST,
                      flags & (K4LZ4_FLAG_X32 | K4LZ4_FLAG_NO_REORDER), stream);
}

int k4lz4_unwrap_size(const uint8_t *buf, int64_t len)
{
    if (len < 0 || (len > 0 && !buf)) return K4LZ4_LEGACY_ARGUMENT;
    if (len > 0x7fffffff) len = 0x7fffffff;           /* (a .NET array) */
    bool dec;
    int in;
    return (int)k4::unwrap_plan(buf, len, &dec, &in);
}

int k4lz4_unwrap_sizes_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, int32_t *outLen,
                              int64_t n, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!src || !srcOff || !srcLen || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    k4::UnwrapArgs u{src, srcOff, srcLen, nullptr, n, outLen, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(k4::k4_unwrap_sizes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u);
    K4_HIP(ctx, hipGetLastError());
    return K4LZ4_OK;
}

int k4lz4_unwrap_batch_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                              const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int32_t *decoded, int64_t n, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!src || !srcOff || !srcLen || !dst || !dstOff || !dstCap || !outLen || !decoded)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    K4_HIP(ctx, order_after_ctx(ctx, st));
    int rc;
    if ((rc = grow_scratch(ctx, &ctx->d_lg, &ctx->d_lg_cap, (size_t)n * 20 + 64)) != K4LZ4_OK) return rc;
    uint64_t *d_off = (uint64_t *)ctx->d_lg;
    int32_t *d_len = (int32_t *)(d_off + n), *d_cap = d_len + n, *d_out = d_cap + n;
    k4::UnwrapArgs u{src, srcOff, srcLen, dstCap, n, outLen, d_off, d_len, d_cap};
    hipLaunchKernelGGL(k4::k4_unwrap_sizes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, u);
    K4_HIP(ctx, hipGetLastError());
    /* the payloads that LZ4Codec.Decode takes, by the ordinary batch decoder with cap = outLen (the others have length 0) */
    if ((rc = launch(ctx, KIND_DECODE, src, d_off, d_len, dst, dstOff, d_cap, d_out, n, 0, 0, st)) != K4LZ4_OK) return rc;
    hipLaunchKernelGGL(k4::k4_unwrap_finish_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, src, srcOff, dst, dstOff, u, d_out, decoded);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    return K4LZ4_OK;
}

int k4lz4_unwrap_batch(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                       const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int32_t *decoded, int64_t n)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!src || !srcOff || !srcLen || !dst || !dstOff || !dstCap || !outLen || !decoded)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> slen((size_t)n);
    for (int64_t i = 0; i < n; i++) slen[(size_t)i] = std::max(srcLen[i], 0);
    HostStage s(ctx);
    s.span(src, srcOff, n, [&](int64_t i) { return (uint64_t)slen[(size_t)i]; });
    s.slots(n, [&](int64_t i) { return (uint64_t)std::max(dstCap[i], 0); }, true);
    uint64_t *d_off, *d_doff;
    int32_t *d_slen, *d_cap, *d_out, *d_dec;
    s.meta(&d_off, n, s.in_off.data()); s.meta(&d_doff, n, s.slot.data()); s.meta(&d_slen, n, slen.data()); s.meta(&d_cap, n, dstCap);
    s.meta(&d_out, n); s.meta(&d_dec, n);
    int rc;
    if ((rc = s.upload()) != K4LZ4_OK ||
        (rc = k4lz4_unwrap_batch_device(ctx, ctx->d_src, d_off, d_slen, ctx->d_dst, d_doff, d_cap, d_out, d_dec, n, s.st)) != K4LZ4_OK)
        return rc;
    return s.finish({{outLen, d_out, (size_t)n * 4}, {decoded, d_dec, (size_t)n * 4}}, dst, dstOff,
                    [&](int64_t i) { return outLen[i] > 0 ? (size_t)outLen[i] : 0; });
}

int64_t k4lz4_legacy_stream_bound(int64_t srcLen, int blockSize)
{
    if (srcLen < 0) return 0;
    const int64_t bs = std::max(16, blockSize);
    return srcLen + 10 * ((srcLen + bs - 1) / bs);       /* a compressed record: 1 + 5 + 5 bytes of varints and at most U - 1 */
}

int k4lz4_encode_legacy_streams_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, int64_t n,
                                       int blockSize, int high, int flags, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                                       int64_t *outLen, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!src || !srcOff || !srcLen || !dst || !dstOff || !dstCap || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    K4_HIP(ctx, order_after_ctx(ctx, st));
    unsigned long long *cnt;
    uint64_t *w[4];
    int32_t *w32;
    int rc;
    if ((rc = lg_streams(ctx, n, &cnt, w, &w32)) != K4LZ4_OK) return rc;
    k4::LegacyWriteArgs a{};
    a.src = src; a.srcOff = srcOff; a.srcLen = srcLen; a.n = n; a.bs = (uint64_t)std::max(16, blockSize); a.high = high ? 1 : 0;
    a.nch = w[0]; a.pad = w[1]; a.first = w[2]; a.arenaOff = w[3];
    const unsigned sgrid = (unsigned)((n + 255) / 256);
    K4_HIP(ctx, hipMemsetAsync(cnt, 0, 64, st));
    hipLaunchKernelGGL(k4::k4_lw_count_kernel, dim3(sgrid), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k4::k4_legacy_scan_kernel, dim3(1), dim3(k4::LEGACY_SCAN_THREADS), 0, st, (const uint64_t *)a.nch, a.first, (long long)n, cnt);
    hipLaunchKernelGGL(k4::k4_legacy_scan_kernel, dim3(1), dim3(k4::LEGACY_SCAN_THREADS), 0, st, (const uint64_t *)a.pad, a.arenaOff, (long long)n, cnt + 1);
    K4_HIP(ctx, hipGetLastError());
    /* the one wait: chunks and arena bytes size the chunk table and the arena */
    unsigned long long h[2];
    K4_HIP(ctx, hipMemcpyAsync(h, cnt, sizeof h, hipMemcpyDeviceToHost, st));
    K4_HIP(ctx, hipStreamSynchronize(st));
    const int64_t rows = (int64_t)h[0];
    if (h[0] > 0xffffffffull) return fail(ctx, K4LZ4_E_ARG, "more than 2^32 chunks in one call");
    if ((rc = grow_scratch(ctx, &ctx->d_lgr, &ctx->d_lgr_cap, (size_t)std::max<int64_t>(rows, 1) * LG_ROW_BYTES + 64)) != K4LZ4_OK) return rc;
    if ((rc = grow_scratch(ctx, &ctx->d_lga, &ctx->d_lga_cap, (size_t)h[1] + 64)) != K4LZ4_OK) return rc;
    {
        uint8_t *m = ctx->d_lgr;
        const size_t w8 = (size_t)std::max<int64_t>(rows, 1) * 8, w4 = w8 / 2;
        a.cSrcOff = (uint64_t *)m;  m += w8;
        a.cEncOff = (uint64_t *)m;  m += w8;
        a.recLen = (uint64_t *)m;   m += w8;
        a.recOff = (uint64_t *)m;   m += w8;
        a.owner = (uint32_t *)m;    m += w4;
        a.cSrcLen = (int32_t *)m;   m += w4;
        a.cEncCap = (int32_t *)m;   m += w4;
        a.cEncLen = (int32_t *)m;
    }
    a.rows = rows;
    if (rows) {
        const unsigned rgrid = (unsigned)((rows + 255) / 256);
        hipLaunchKernelGGL(k4::k4_lw_fill_kernel, dim3(rgrid), dim3(256), 0, st, a);
        K4_HIP(ctx, hipGetLastError());
        /* every chunk of every stream in one batch, cap U - 1: compressed iff C < U (LZ4Stream.cs FlushCurrentChunk); few big chunks
         * may be cut into segments */
        const int seg_ok = (!high && a.bs >= ctx->seg_min && rows <= 2 * (int64_t)ctx->cu_count) ? FLAG_SEGMENTS_OK : 0;
        if ((rc = launch(ctx, KIND_ENCODE, src, a.cSrcOff, a.cSrcLen, ctx->d_lga, a.cEncOff, a.cEncCap, a.cEncLen, rows,
                         high ? K4LZ4_L09_HC : K4LZ4_L00_FAST, (flags & K4LZ4_FLAG_X32) | K4LZ4_FLAG_RAW_RETURN | seg_ok, st)) != K4LZ4_OK)
            return rc;
        hipLaunchKernelGGL(k4::k4_lw_header_kernel, dim3(rgrid), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k4::k4_legacy_scan_kernel, dim3(1), dim3(k4::LEGACY_SCAN_THREADS), 0, st, (const uint64_t *)a.recLen, a.recOff, (long long)rows, cnt + 2);
        hipLaunchKernelGGL(k4::k4_lw_assemble_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a, dst, dstOff, dstCap, (const uint8_t *)ctx->d_lga);
    }
    hipLaunchKernelGGL(k4::k4_lw_finish_kernel, dim3(sgrid), dim3(256), 0, st, a, dstCap, outLen);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    return K4LZ4_OK;
}

int k4lz4_encode_legacy_streams(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, int64_t n,
                                int blockSize, int high, int flags, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                                int64_t *outLen)
{
    auto device = [=](k4lz4_ctx *c, const uint8_t *s, const uint64_t *off, const uint64_t *len, int64_t m, uint8_t *d,
                      const uint64_t *dOff, const uint64_t *dCap, int64_t *out, void *st) {
        return k4lz4_encode_legacy_streams_device(c, s, off, len, m, blockSize, high, flags, d, dOff, dCap, out, st);
    };
    return host_streams(device, ctx, src, srcOff, srcLen, n, dst, dstOff, dstCap, outLen, /* zero */ false, /* capped */ false);
}

int k4lz4_legacy_stream_sizes_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *streamOff, const uint64_t *streamLen, int64_t n,
                                     uint64_t *outSize, int32_t *outStatus, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!src || !streamOff || !streamLen || !outSize || !outStatus))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    K4_HIP(ctx, order_after_ctx(ctx, st));
    unsigned long long *cnt;
    uint64_t *w[4];
    int32_t *w32;
    int rc;
    if ((rc = lg_streams(ctx, n, &cnt, w, &w32)) != K4LZ4_OK) return rc;
    k4::LegacyReadArgs a{src, streamOff, streamLen, n, w[0], w[1], w32, w[2], (unsigned long long *)w[3], outSize, outStatus};
    hipLaunchKernelGGL(k4::k4_lr_walk_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    return K4LZ4_OK;
}

int k4lz4_decode_legacy_streams_device(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *streamOff, const uint64_t *streamLen, int64_t n,
                                       uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!src || !streamOff || !streamLen || !dst || !dstOff || !dstCap || !outLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    K4_HIP(ctx, order_after_ctx(ctx, st));
    unsigned long long *cnt;
    uint64_t *w[4];
    int32_t *w32;
    int rc;
    if ((rc = lg_streams(ctx, n, &cnt, w, &w32)) != K4LZ4_OK) return rc;
    k4::LegacyReadArgs a{src, streamOff, streamLen, n, w[0], w[1], w32, w[2], (unsigned long long *)w[3], nullptr, nullptr};
    const unsigned sgrid = (unsigned)((n + 255) / 256);
    K4_HIP(ctx, hipMemsetAsync(cnt, 0, 64, st));
    hipLaunchKernelGGL(k4::k4_lr_walk_kernel, dim3(sgrid), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k4::k4_legacy_scan_kernel, dim3(1), dim3(k4::LEGACY_SCAN_THREADS), 0, st, (const uint64_t *)a.nch, a.first, (long long)n, cnt);
    K4_HIP(ctx, hipGetLastError());
    /* the one wait: the chunk count sizes the table */
    unsigned long long h = 0;
    K4_HIP(ctx, hipMemcpyAsync(&h, cnt, sizeof h, hipMemcpyDeviceToHost, st));
    K4_HIP(ctx, hipStreamSynchronize(st));
    const int64_t rows = (int64_t)h;
    if (h > 0xffffffffull) return fail(ctx, K4LZ4_E_ARG, "more than 2^32 chunks in one call");
    if ((rc = grow_scratch(ctx, &ctx->d_lgr, &ctx->d_lgr_cap, (size_t)std::max<int64_t>(rows, 1) * LG_ROW_BYTES + 64)) != K4LZ4_OK) return rc;
    k4::LegacyRows rw;
    {
        uint8_t *m = ctx->d_lgr;
        const size_t w8 = (size_t)std::max<int64_t>(rows, 1) * 8, w4 = w8 / 2;
        rw.off = (uint64_t *)m;     m += w8;
        rw.dstOff = (uint64_t *)m;  m += w8;
        rw.owner = (uint32_t *)m;   m += w4;
        rw.idx = (uint32_t *)m;     m += w4;
        rw.srcLen = (int32_t *)m;   m += w4;
        rw.dstCap = (int32_t *)m;   m += w4;
        rw.len = (int32_t *)m;      m += w4;
        rw.outLen = (int32_t *)m;   m += w4;
        rw.kind = m;
    }
    hipLaunchKernelGGL(k4::k4_lr_fill_kernel, dim3(sgrid), dim3(256), 0, st, a, rw, dstOff, dstCap);
    K4_HIP(ctx, hipGetLastError());
    if (rows) {
        /* compressed chunks straight into place, cap U; raw chunks (srcLen 0 there) copied behind them */
        if ((rc = launch(ctx, KIND_DECODE, src, rw.off, rw.srcLen, dst, rw.dstOff, rw.dstCap, rw.outLen, rows, 0, 0, st)) != K4LZ4_OK) return rc;
        hipLaunchKernelGGL(k4::k4_lr_copy_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, src, dst, a, rw, (long long)rows);
    }
    hipLaunchKernelGGL(k4::k4_lr_finish_kernel, dim3(sgrid), dim3(256), 0, st, a, outLen);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    return K4LZ4_OK;
}

int k4lz4_legacy_stream_sizes(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *streamOff, const uint64_t *streamLen, int64_t n,
                              uint64_t *outSize, int32_t *outStatus)
{
    return host_sizes(k4lz4_legacy_stream_sizes_device, ctx, src, streamOff, streamLen, n, outSize, outStatus);
}

int k4lz4_decode_legacy_streams(k4lz4_ctx *ctx, const uint8_t *src, const uint64_t *streamOff, const uint64_t *streamLen, int64_t n,
                                uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap, int64_t *outLen)
{
    return host_streams(k4lz4_decode_legacy_streams_device, ctx, src, streamOff, streamLen, n, dst, dstOff, dstCap, outLen,
                        /* zero */ true, /* capped */ false);
}

/* ---- incremental frame writer (k4lz4_frame_write.hpp) ------------------------------------------------------- */
int k4lz4_frame_writer_init(k4lz4_frame_writer *w, const k4lz4_frame_writer_settings *settings)
{
    if (!w || !settings) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_frame_writer_init: NULL argument");
    const k4lz4_frame_writer_settings &s = *settings;
    if (s.blockSize <= 0 || s.blockSize > (4 << 20)) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_frame_writer_init: block size outside 1 .. 4 MiB");
    memset(w, 0, sizeof *w);
    w->settings = s;
    w->settings.chainBlocks = s.chainBlocks ? 1 : 0; w->settings.blockChecksum = s.blockChecksum ? 1 : 0;
    w->settings.contentChecksum = s.contentChecksum ? 1 : 0;
    if (w->settings.contentLength < 0) w->settings.contentLength = -1;
    const int64_t bs = s.blockSize;
    w->kind = !s.chainBlocks ? 0 : s.level >= K4LZ4_L03_HC ? 1 : 2;
    w->extraBlocks = (int32_t)(std::max<int64_t>(s.extraMemory > 0 ? bs : 0, s.extraMemory) / bs);     /* Streams/Extensions.cs:18-19 */
    w->encBlock = w->kind == 0 ? (int32_t)bs : (int32_t)hc_chain_block_size(s.blockSize);
    w->ringBytes = w->kind == 0 ? w->encBlock : (int32_t)(65536 + (1 + (int64_t)w->extraBlocks) * w->encBlock + 32);   /* LZ4EncoderBase.cs:25 */
    return K4LZ4_OK;
}

int64_t k4lz4_frame_writer_store_bytes(const k4lz4_frame_writer *w)
{
    return w ? (fw_ring_at(*w) + w->ringBytes + 8 + 63) / 64 * 64 : 0;
}

int64_t k4lz4_frame_write_bound(const k4lz4_frame_writer *w, int64_t srcLen, int closing)
{
    return w ? fw_bound(*w, srcLen, closing != 0) : 0;
}

int k4lz4_frame_write_batch_device(k4lz4_ctx *ctx, k4lz4_frame_writer *w, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                                   const uint64_t *srcOff, const int64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                                   int64_t *outLen, int64_t n, int op, int flags, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!w || !store || !storeOff || !srcOff || !srcLen || !dst || !dstOff || !dstCap || !outLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (op < K4LZ4_FWRITE_WRITE || op > K4LZ4_FWRITE_CLOSE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_write_batch: unknown op");
    if (flags & ~(int)K4LZ4_FLAG_X32) return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_write_batch: the only flag it takes is K4LZ4_FLAG_X32");
    if (n == 0) return K4LZ4_OK;
    const bool x32 = (flags & K4LZ4_FLAG_X32) || g_enforce32.load(std::memory_order_relaxed);
    const bool closing = op == K4LZ4_FWRITE_CLOSE;
    hipStream_t st = (hipStream_t)stream;

    /* ---- the plan: per-stream codes, the model's blocks, the groups -- host index arithmetic, nothing enqueued yet */
    std::vector<int32_t> code((size_t)n, 1);
    std::vector<FwAfter> after((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const k4lz4_frame_writer &r = w[i];
        const int64_t len = srcLen[i];
        if (len < 0) continue;
        if (op == K4LZ4_FWRITE_OPEN && len != 0) return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_write_batch: an open takes no bytes");
        if (r.kind == 2 && x32)
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_write_batch: the 32-bit engine's chained encoder (LZ4Codec.Enforce32) is not supported");
        if ((code[(size_t)i] = fw_code(r, len, closing, dstCap[i])) != 0) continue;
        if (r.kind == 1 && r.written + len > FW_CHAIN_LIMIT)
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_write_batch: a chained stream longer than 2 GB (the encoder's renormalisation) is not supported");
        after[(size_t)i] = fw_model(r, len, closing, [](int64_t, int64_t) {});
        if (after[(size_t)i].too_long)
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_write_batch: a chained stream longer than 2 GB (the encoder's renormalisation) is not supported");
        code[(size_t)i] = 0;
    }
    /* groups of streams whose blocks go to one encoder call: (block checksum, kind, level), those without checksums first */
    auto key = [&](int64_t i) { const k4lz4_frame_writer &r = w[i]; return r.settings.blockChecksum * 1000 + r.kind * 100 + (r.kind == 2 ? 0 : r.settings.level); };
    std::vector<int> keys;
    for (int64_t i = 0; i < n; i++) if (code[(size_t)i] == 0 && after[(size_t)i].nblk) keys.push_back(key(i));
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    struct Group { int key; std::vector<int64_t> streams; int64_t first = 0, nb = 0; };
    std::vector<Group> groups(keys.size());
    for (size_t g = 0; g < keys.size(); g++) groups[g].key = keys[g];
    for (int64_t i = 0; i < n; i++)
        if (code[(size_t)i] == 0 && after[(size_t)i].nblk)
            groups[(size_t)(std::lower_bound(keys.begin(), keys.end(), key(i)) - keys.begin())].streams.push_back(i);
    int64_t nb = 0, firstSum = -1, nind = 0, nfast = 0, nhash = 0, nstage = 0, nback = 0;
    for (Group &g : groups) {
        g.first = nb;
        for (int64_t i : g.streams) g.nb += after[(size_t)i].nblk;
        nb += g.nb;
        if (g.key >= 1000 && firstSum < 0) firstSum = g.first;
        if (g.key % 1000 < 100) nind += g.nb;
        if (g.key % 1000 / 100 == 2) nfast += (int64_t)g.streams.size();
    }
    if (firstSum < 0) firstSum = nb;
    if (nb > 0xffffffffll) return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_write_batch: more than 2^32 blocks in one call");
    for (int64_t i = 0; i < n; i++) {
        if (code[(size_t)i] != 0) continue;
        const k4lz4_frame_writer &r = w[i];
        if (r.settings.contentChecksum && (srcLen[i] > 0 || fw_opens(r, srcLen[i], closing))) nhash++;
        if (after[(size_t)i].nblk) { nstage += 2; nback += 1; }
        else if (srcLen[i] > 0) nstage += 1;
    }
    nstage += nfast; nback += nfast;

    /* ---- scratch layout: the uploaded plan first, then what the kernels fill, then windows, arena and states */
    size_t at = 0;
    const size_t o_streams = fw_take(at, (size_t)n * sizeof(k4::FwStream)), o_hash = fw_take(at, (size_t)nhash * sizeof(k4::FwHashItem)),
                 o_stage = fw_take(at, (size_t)nstage * sizeof(k4::FwPiece)), o_back = fw_take(at, (size_t)nback * sizeof(k4::FwPiece)),
                 o_owner = fw_take(at, (size_t)nb * 4), o_slot = fw_take(at, (size_t)nb * 8),
                 o_isrc = fw_take(at, (size_t)nind * 8), o_ilen = fw_take(at, (size_t)nind * 4), o_icap = fw_take(at, (size_t)nind * 4);
    const size_t plan_bytes = at;
    const size_t o_out = fw_take(at, (size_t)nb * 4), o_stored = fw_take(at, (size_t)nb * 8), o_rec = fw_take(at, (size_t)nb * 8),
                 o_excl = fw_take(at, (size_t)nb * 8), o_roff = fw_take(at, (size_t)nb * 8), o_sum = fw_take(at, (size_t)nb * 4),
                 o_cnt = fw_take(at, 64);
    std::vector<uint64_t> win((size_t)n, 0), aoff((size_t)n, 0);
    for (const Group &g : groups)
        for (int64_t i : g.streams) { win[(size_t)i] = at; fw_take(at, (size_t)(w[i].pointer + srcLen[i]) + 16); }
    for (const Group &g : groups)
        for (int64_t i : g.streams) { aoff[(size_t)i] = at; fw_take(at, (size_t)(after[(size_t)i].nblk * fw_slot(w[i]))); }
    const size_t o_stin = fw_take(at, (size_t)nfast * sizeof(k4lz4_fast_chain_state)),
                 o_stout = fw_take(at, (size_t)nfast * sizeof(k4lz4_fast_chain_state));
    const size_t total_bytes = at + 64;

    K4_HIP(ctx, hipSetDevice(ctx->device));
    PlanUpload &plan = ctx->fw_plan;
    int rc;
    if ((rc = plan_begin(ctx, plan, plan_bytes + 64, true)) != K4LZ4_OK) return rc;
    if ((rc = grow_scratch(ctx, &plan.dev, &plan.cap, total_bytes)) != K4LZ4_OK) return rc;
    uint8_t *h = plan.host.data(), *d = plan.dev;
    k4::FwStream *hs = (k4::FwStream *)(h + o_streams);
    k4::FwHashItem *hh = (k4::FwHashItem *)(h + o_hash);
    k4::FwPiece *hstage = (k4::FwPiece *)(h + o_stage), *hback = (k4::FwPiece *)(h + o_back);
    uint32_t *howner = (uint32_t *)(h + o_owner);
    uint64_t *hslot = (uint64_t *)(h + o_slot), *hisrc = (uint64_t *)(h + o_isrc);
    int32_t *hilen = (int32_t *)(h + o_ilen), *hicap = (int32_t *)(h + o_icap);
    k4lz4_fast_chain_state *d_stin = (k4lz4_fast_chain_state *)(d + o_stin), *d_stout = (k4lz4_fast_chain_state *)(d + o_stout);

    /* per stream: the table row, the hash item, the pieces; per block: owner, arena slot, the independent blocks' arrays */
    int64_t kh = 0, ks = 0, kb = 0, kfast = 0;
    std::vector<int64_t> first((size_t)n, 0), fast_index((size_t)n, -1);
    for (const Group &g : groups) {
        int64_t b = g.first, ind = 0;
        for (const Group &g2 : groups) if (&g2 == &g) break; else if (g2.key % 1000 < 100) ind += g2.nb;
        for (int64_t i : g.streams) {
            first[(size_t)i] = b;
            const int64_t slot = fw_slot(w[i]);
            int64_t j = 0;
            fw_model(w[i], srcLen[i], closing, [&](int64_t start, int64_t len) {
                howner[b] = (uint32_t)i;
                hslot[b] = aoff[(size_t)i] + (uint64_t)(j * slot);
                if (g.key % 1000 < 100) {
                    hisrc[ind] = win[(size_t)i] + (uint64_t)start; hilen[ind] = (int32_t)len; hicap[ind] = (int32_t)slot; ind++;
                }
                b++; j++;
            });
            if (w[i].kind == 2) fast_index[(size_t)i] = kfast++;
        }
    }
    for (int64_t i = 0; i < n; i++) {
        k4::FwStream &row = hs[i];
        row.code = code[(size_t)i];
        if (row.code != 0) continue;
        const k4lz4_frame_writer &r = w[i];
        const FwAfter &a = after[(size_t)i];
        uint8_t *sto = store + storeOff[i];
        const int64_t len = srcLen[i];
        row.out = dstOff[i]; row.first = (unsigned long long)first[(size_t)i]; row.nblk = (uint32_t)a.nblk;
        const bool opens = fw_opens(r, len, closing);
        row.hdrLen = opens ? fw_header(r, row.hdr) : 0;
        row.close = closing && !(r.phase == 0 && len == 0) ? (r.settings.contentChecksum ? 2u : 1u) : 0u;
        row.xxh = (const k4::FwXxhState *)sto;
        if (r.settings.contentChecksum && (len > 0 || opens)) {
            hh[kh].data = src + srcOff[i]; hh[kh].len = (unsigned long long)len; hh[kh].state = (k4::FwXxhState *)sto;
            hh[kh].fresh = opens ? 1u : 0u; kh++;
        }
        uint8_t *ring = sto + fw_ring_at(r);
        if (a.nblk) {
            uint8_t *wp = d + win[(size_t)i];
            hstage[ks++] = k4::FwPiece{wp, ring, (unsigned long long)r.pointer, 0};
            hstage[ks++] = k4::FwPiece{wp + r.pointer, src + srcOff[i], (unsigned long long)len, 0};
            const int64_t r0 = a.ws == 0 ? r.pointer : 0;                 /* bytes of the ring that stay where they are */
            hback[kb++] = k4::FwPiece{ring + r0, wp + a.ws + r0, (unsigned long long)(a.pointer - r0), 0};
            if (r.kind == 2) {
                const int64_t f = fast_index[(size_t)i];
                k4lz4_fast_chain_state *sst = (k4lz4_fast_chain_state *)(sto + FW_XXH_BYTES);
                /* a stream that has encoded nothing yet starts from a zeroed LZ4_stream_t (LZ4FastChainEncoder.cs) */
                hstage[ks++] = k4::FwPiece{(uint8_t *)(d_stin + f), r.currentOffset ? (const uint8_t *)sst : nullptr, sizeof(k4lz4_fast_chain_state), 0};
                hback[kb++] = k4::FwPiece{(uint8_t *)sst, (const uint8_t *)(d_stout + f), sizeof(k4lz4_fast_chain_state), 0};
            }
        } else if (len > 0) {
            hstage[ks++] = k4::FwPiece{ring + r.pointer, src + srcOff[i], (unsigned long long)len, 0};
        }
    }
    const unsigned long long stage_chunks = fw_chunks(hstage, (size_t)ks), back_chunks = fw_chunks(hback, (size_t)kb);

    /* ---- enqueue: plan up, hash, stage, encode, write back, records, edges */
    if ((rc = plan_send(ctx, plan, d, plan_bytes, st)) != K4LZ4_OK) return rc;
    const k4::FwStream *d_streams = (const k4::FwStream *)(d + o_streams);
    int32_t *d_out = (int32_t *)(d + o_out);
    unsigned long long *d_stored = (unsigned long long *)(d + o_stored), *d_rec = (unsigned long long *)(d + o_rec),
                       *d_excl = (unsigned long long *)(d + o_excl), *d_roff = (unsigned long long *)(d + o_roff);
    uint32_t *d_sum = (uint32_t *)(d + o_sum);
    if (kh) hipLaunchKernelGGL(k4::k4_fw_xxh32_kernel, dim3((unsigned)((kh * 4 + k4::FW_THREADS - 1) / k4::FW_THREADS)), dim3(k4::FW_THREADS), 0, st,
                               (const k4::FwHashItem *)(d + o_hash), (long long)kh);
    if (ks) hipLaunchKernelGGL(k4::k4_fw_copy_kernel, dim3((unsigned)stage_chunks), dim3(k4::FW_THREADS), 0, st, (const k4::FwPiece *)(d + o_stage), (long long)ks);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    int64_t ind = 0;
    for (const Group &g : groups) {
        const int kind = g.key % 1000 / 100, level = g.key % 100;
        const int64_t ns = (int64_t)g.streams.size();
        if (kind == 0) {
            rc = launch(ctx, KIND_ENCODE, d, (const uint64_t *)(d + o_isrc) + ind, (const int32_t *)(d + o_ilen) + ind, d,
                        (const uint64_t *)(d + o_slot) + g.first, (const int32_t *)(d + o_icap) + ind, d_out + g.first, g.nb, level,
                        K4LZ4_FLAG_ALLOW_COPY | (x32 ? K4LZ4_FLAG_X32 : 0), st, nullptr, hilen + ind);
            ind += g.nb;
        } else {
            std::vector<uint64_t> soff((size_t)ns), doff((size_t)ns);
            std::vector<int64_t> slen((size_t)ns);
            std::vector<int32_t> bsz((size_t)ns), ext((size_t)ns), dlen((size_t)ns);
            std::vector<uint32_t> cur0((size_t)ns), sdict((size_t)ns);
            int64_t f0 = -1;
            for (int64_t k = 0; k < ns; k++) {
                const int64_t i = g.streams[(size_t)k];
                soff[(size_t)k] = win[(size_t)i]; doff[(size_t)k] = aoff[(size_t)i];
                /* the window up to the end of the last block this call encodes */
                int64_t end = w[i].index;
                fw_model(w[i], srcLen[i], closing, [&](int64_t s0, int64_t l0) { end = s0 + l0; });
                slen[(size_t)k] = end;
                bsz[(size_t)k] = w[i].settings.blockSize; ext[(size_t)k] = w[i].extraBlocks; dlen[(size_t)k] = w[i].index;
                cur0[(size_t)k] = w[i].currentOffset; sdict[(size_t)k] = w[i].dictSize;
                if (f0 < 0) f0 = fast_index[(size_t)i];
            }
            if (kind == 1)
                rc = hc_chain_run(ctx, d, soff.data(), slen.data(), bsz.data(), ext.data(), dlen.data(), ns, d, doff.data(), d_out + g.first, g.nb,
                                  level, K4LZ4_FLAG_ALLOW_COPY, st);
            else      /* the states' two indices from the records (k4lz4_encode_fast_chain_batch_device reads them back instead) */
                rc = fast_chain_run(ctx, d, soff.data(), slen.data(), bsz.data(), ext.data(), dlen.data(), cur0.data(), sdict.data(), ns,
                                    d_stin + f0, d_stout + f0, d, doff.data(), d_out + g.first, g.nb, K4LZ4_FLAG_ALLOW_COPY, st);
        }
        if (rc != K4LZ4_OK) return rc;
    }
    if (kb) hipLaunchKernelGGL(k4::k4_fw_copy_kernel, dim3((unsigned)back_chunks), dim3(k4::FW_THREADS), 0, st, (const k4::FwPiece *)(d + o_back), (long long)kb);
    if (nb) {
        const unsigned bgrid = (unsigned)((nb + k4::FW_THREADS - 1) / k4::FW_THREADS);
        hipLaunchKernelGGL(k4::k4_fw_reclen_kernel, dim3(bgrid), dim3(k4::FW_THREADS), 0, st, (const int32_t *)d_out, d_stored, d_rec, (long long)nb, (long long)firstSum);
        if (firstSum < nb) {
            k4::HashArgs ha{d, (const uint64_t *)(d + o_slot) + firstSum, (const uint64_t *)d_stored + firstSum, d_sum + firstSum, nb - firstSum, 0u};
            hipLaunchKernelGGL(k4::k4_xxh32_kernel, dim3((unsigned)(((nb - firstSum) * 4 + k4::XXH_THREADS - 1) / k4::XXH_THREADS)), dim3(k4::XXH_THREADS), 0, st, ha);
        }
        hipLaunchKernelGGL(k4::k4_legacy_scan_kernel, dim3(1), dim3(k4::LEGACY_SCAN_THREADS), 0, st, (const uint64_t *)d_rec, (uint64_t *)d_excl,
                           (long long)nb, (unsigned long long *)(d + o_cnt));
        hipLaunchKernelGGL(k4::k4_fw_place_kernel, dim3(bgrid), dim3(k4::FW_THREADS), 0, st, d_streams, (const uint32_t *)(d + o_owner),
                           (const unsigned long long *)d_excl, d_roff, (long long)nb);
        if (firstSum > 0) {
            k4::FrameBlocksArgs fa{d, (const uint64_t *)(d + o_slot), d_out, nullptr, (const uint64_t *)d_roff, dst, firstSum};
            hipLaunchKernelGGL(k4::k4_frame_blocks_kernel, dim3((unsigned)((firstSum + 3) / 4)), dim3(256), 0, st, fa);
        }
        if (firstSum < nb) {
            k4::FrameBlocksArgs fa{d, (const uint64_t *)(d + o_slot) + firstSum, d_out + firstSum, d_sum + firstSum, (const uint64_t *)d_roff + firstSum,
                                   dst, nb - firstSum};
            hipLaunchKernelGGL(k4::k4_frame_blocks_kernel, dim3((unsigned)((nb - firstSum + 3) / 4)), dim3(256), 0, st, fa);
        }
    }
    hipLaunchKernelGGL(k4::k4_fw_edges_kernel, dim3((unsigned)((n + k4::FW_THREADS - 1) / k4::FW_THREADS)), dim3(k4::FW_THREADS), 0, st, d_streams,
                       (const unsigned long long *)d_excl, (const unsigned long long *)d_rec, dst, (long long *)outLen, (long long)n);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);

    /* ---- the records: what the calls enqueued leaves them in */
    for (int64_t i = 0; i < n; i++) {
        if (code[(size_t)i] != 0) continue;
        fw_advance(w[i], srcLen[i], closing, after[(size_t)i]);
    }
    return K4LZ4_OK;
}

int k4lz4_frame_write_batch(k4lz4_ctx *ctx, k4lz4_frame_writer *w, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                            const uint64_t *srcOff, const int64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                            int64_t *outLen, int64_t n, int op, int flags)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!w || !store || !storeOff || !srcOff || !srcLen || !dst || !dstOff || !dstCap || !outLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    for (int64_t i = 0; i < n; i++)
        if (srcLen[i] > 0 && !src) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    K4_HIP(ctx, hipSetDevice(ctx->device));
    /* the output slots: what the call can emit, not the caller's capacities (the codes are decided on dstCap all the same) */
    std::vector<uint64_t> cap((size_t)n);
    for (int64_t i = 0; i < n; i++) cap[(size_t)i] = std::min<uint64_t>(dstCap[i], (uint64_t)fw_bound(w[i], srcLen[i], op == K4LZ4_FWRITE_CLOSE));
    std::vector<int64_t> len0((size_t)n);
    for (int64_t i = 0; i < n; i++) len0[(size_t)i] = std::max<int64_t>(srcLen[i], 0);
    HostStage s(ctx);
    s.pack(src, srcOff, len0.data(), n);
    s.slots(n, [&](int64_t i) { return cap[(size_t)i]; }, false);
    int64_t *d_out;
    s.meta(&d_out, n);
    int rc;
    if ((rc = s.upload()) != K4LZ4_OK ||
        (rc = k4lz4_frame_write_batch_device(ctx, w, store, storeOff, ctx->d_src, s.in_off.data(), srcLen, ctx->d_dst, s.slot.data(), cap.data(),
                                             d_out, n, op, flags, s.st)) != K4LZ4_OK)
        return rc;
    /* codes from dstCap: the device form saw the clipped capacities, which pass the same bound */
    return s.finish({{outLen, d_out, (size_t)n * 8}}, dst, dstOff, [&](int64_t i) { return outLen[i] > 0 ? (size_t)outLen[i] : 0; });
}

/* ---- incremental frame reader (k4lz4_frame_reader.hpp) --------------------------------------------------- */
int k4lz4_frame_reader_init(k4lz4_frame_reader *r, const k4lz4_frame_reader_settings *settings)
{
    if (!r) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_frame_reader_init: NULL argument");
    const int32_t asked = settings ? settings->maxBlockSize : 0;
    if (asked > (4 << 20)) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_frame_reader_init: maxBlockSize above 4 MiB");
    const int32_t flags = settings ? settings->flags : 0;
    if (flags & ~(int32_t)K4LZ4_FREADER_FED) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_frame_reader_init: the only flag it takes is K4LZ4_FREADER_FED");
    r->settings.maxBlockSize = k4::fr_max_block(asked);
    r->settings.flags = flags;
    r->storeBytes = flags ? k4::fr_fed_store_bytes(r->settings.maxBlockSize) : k4::fr_store_bytes(r->settings.maxBlockSize);
    return K4LZ4_OK;
}

int64_t k4lz4_frame_reader_store_bytes(const k4lz4_frame_reader *r) { return r ? r->storeBytes : 0; }
int64_t k4lz4_frame_read_table_rows(int64_t maxCount) { return k4::fr_table_rows(maxCount); }

/* the readers against a dictionary set (k4lz4_frame_reader_dict.hpp): the set's words and the call's id table -- a
 * host array in both forms, staged like k4lz4_decode_frames_dictset's -- for the kernels */
static int reader_dict(k4lz4_ctx *ctx, const k4lz4_dict_set *set, const uint32_t *dictIds, hipStream_t st, k4::FrDict *d)
{
    K4_HIP(ctx, hipSetDevice(ctx->device));
    K4_HIP(ctx, order_after_ctx(ctx, st));
    uint32_t *ids = nullptr;
    int32_t *idx = nullptr;
    const int rc = frame_dict_ids(ctx, set, dictIds, 0, st, &ids, &idx);
    if (rc != K4LZ4_OK) return rc;
    *d = k4::FrDict{set->buf, set->dec_off, set->dec_len, ids, set->nDict};
    return K4LZ4_OK;
}

/* set == nullptr: k4lz4_frame_read_batch_device as it always was; with a set, k4lz4_frame_read_dictset_batch_device */
static int frame_read_run(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                          const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const int64_t *count,
                          int64_t *outLen, int64_t n, int op, int flags, int64_t maxCount, const k4lz4_dict_set *set, const uint32_t *dictIds,
                          void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (op < K4LZ4_FREAD_READ || op > K4LZ4_FREAD_RESET) return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_read_batch: unknown op");
    if (flags & ~(int)K4LZ4_FREAD_INTERACTIVE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_read_batch: the only flag it takes is K4LZ4_FREAD_INTERACTIVE");
    if (n < 0 || (n > 0 && (!r || !store || !storeOff || !count || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && op != K4LZ4_FREAD_RESET && (!src || !srcOff || !srcLen)) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && op == K4LZ4_FREAD_READ && (!dst || !dstOff)) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && (r->storeBytes != k4::fr_store_bytes(r->settings.maxBlockSize) || r->settings.maxBlockSize != k4::fr_max_block(r->settings.maxBlockSize)))
        return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_read_batch: the record was not made by k4lz4_frame_reader_init");
    if (n == 0) return K4LZ4_OK;
    const int interactive = (flags & K4LZ4_FREAD_INTERACTIVE) ? 1 : 0;
    const k4::FrReadArgs a{src, srcOff, srcLen, store, storeOff, dst, dstOff, count, outLen, (long long)n, op, interactive, r->settings.maxBlockSize,
                           nullptr};
    const long long rows = op == K4LZ4_FREAD_READ && !interactive ? k4::fr_table_rows(maxCount) : 0;
    if (!set) return read_device<FrameReader>(ctx, a, rows, stream);
    k4::FrDict d;
    const int rc = reader_dict(ctx, set, dictIds, (hipStream_t)stream, &d);
    if (rc != K4LZ4_OK) return rc;
    return read_device<DictFrameReader>(ctx, {a, d}, rows, stream);
}

int k4lz4_frame_read_batch_device(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff,
                                  const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst,
                                  const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t n, int op, int flags,
                                  int64_t maxCount, void *stream)
{
    return frame_read_run(ctx, r, store, storeOff, src, srcOff, srcLen, dst, dstOff, count, outLen, n, op, flags, maxCount, nullptr, nullptr, stream);
}

int k4lz4_frame_read_dictset_batch_device(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff,
                                          const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst,
                                          const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t n, int op, int flags,
                                          int64_t maxCount, const k4lz4_dict_set *set, const uint32_t *dictIds, void *stream)
{
    const int rc = frame_dict_args(ctx, set, dictIds, "k4lz4_frame_read_dictset_batch");
    if (rc != K4LZ4_OK) return rc;
    return frame_read_run(ctx, r, store, storeOff, src, srcOff, srcLen, dst, dstOff, count, outLen, n, op, flags, maxCount, set, dictIds, stream);
}

static int frame_read_host(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                           const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const int64_t *count,
                           int64_t *outLen, int64_t n, int op, int flags, const k4lz4_dict_set *set, const uint32_t *dictIds)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (op < K4LZ4_FREAD_READ || op > K4LZ4_FREAD_RESET) return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_read_batch: unknown op");
    if (n < 0 || (n > 0 && (!r || !store || !storeOff || !count || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && op != K4LZ4_FREAD_RESET && (!srcOff || !srcLen)) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && op == K4LZ4_FREAD_READ && (!dst || !dstOff)) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (flags & ~(int)K4LZ4_FREAD_INTERACTIVE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_read_batch: the only flag it takes is K4LZ4_FREAD_INTERACTIVE");
    if (n > 0 && (r->storeBytes != k4::fr_store_bytes(r->settings.maxBlockSize) || r->settings.maxBlockSize != k4::fr_max_block(r->settings.maxBlockSize)))
        return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_read_batch: the record was not made by k4lz4_frame_reader_init");
    if (n == 0) return K4LZ4_OK;
    return host_read(ctx, {storeOff, src, srcOff, srcLen, nullptr, dst, dstOff, count, outLen, nullptr, nullptr}, n,
                     /* sends */ op != K4LZ4_FREAD_RESET, /* fills */ op == K4LZ4_FREAD_READ,
                     [&](const ReadArrays &d, int64_t maxCount, hipStream_t st) {
                         return frame_read_run(ctx, r, store, d.storeOff, d.src, d.srcOff, d.srcLen, d.dst, d.dstOff, d.count, d.outLen, n, op,
                                               flags, maxCount, set, dictIds, st);
                     });
}

int k4lz4_frame_read_batch(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                           const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const int64_t *count,
                           int64_t *outLen, int64_t n, int op, int flags)
{
    return frame_read_host(ctx, r, store, storeOff, src, srcOff, srcLen, dst, dstOff, count, outLen, n, op, flags, nullptr, nullptr);
}

int k4lz4_frame_read_dictset_batch(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                                   const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const int64_t *count,
                                   int64_t *outLen, int64_t n, int op, int flags, const k4lz4_dict_set *set, const uint32_t *dictIds)
{
    const int rc = frame_dict_args(ctx, set, dictIds, "k4lz4_frame_read_dictset_batch");
    if (rc != K4LZ4_OK) return rc;
    return frame_read_host(ctx, r, store, storeOff, src, srcOff, srcLen, dst, dstOff, count, outLen, n, op, flags, set, dictIds);
}

int k4lz4_frame_reader_query_device(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out, void *stream)
{
    return query_device(ctx, k4::k4_fr_query_kernel, store, storeOff, n, out, stream);
}

int k4lz4_frame_reader_query(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out)
{
    return query_host(ctx, K4LZ4_FRQ_WORDS, k4lz4_frame_reader_query_device, store, storeOff, n, out);
}

/* ---- the incremental frame reader fed its source in pieces (k4lz4_frame_feed.hpp) ------------------------- */
static int fed_args(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, const void *store, const void *storeOff, const void *srcOff, const void *srcLen,
                    const void *dst, const void *dstOff, const void *count, const void *outLen, const void *consumed, const void *need,
                    int64_t n, int op, int flags)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (op < K4LZ4_FREAD_READ || op > K4LZ4_FREAD_RESET) return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_read_fed_batch: unknown op");
    if (flags & ~(int)K4LZ4_FREAD_INTERACTIVE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_read_fed_batch: the only flag it takes is K4LZ4_FREAD_INTERACTIVE");
    if (n < 0 || (n > 0 && (!r || !store || !storeOff || !count || !outLen || !consumed || !need))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && op != K4LZ4_FREAD_RESET && (!srcOff || !srcLen)) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && op == K4LZ4_FREAD_READ && (!dst || !dstOff)) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && (r->settings.flags != K4LZ4_FREADER_FED || r->settings.maxBlockSize != k4::fr_max_block(r->settings.maxBlockSize) ||
                  r->storeBytes != k4::fr_fed_store_bytes(r->settings.maxBlockSize)))
        return fail(ctx, K4LZ4_E_ARG, "k4lz4_frame_read_fed_batch: the record was not made by k4lz4_frame_reader_init with K4LZ4_FREADER_FED");
    return K4LZ4_OK;
}

/* set == nullptr: k4lz4_frame_read_fed_batch_device as it always was; with a set, k4lz4_frame_read_fed_dictset_batch_device */
static int frame_read_fed_run(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                              const uint64_t *srcOff, const uint64_t *srcLen, const int64_t *final, uint8_t *dst, const uint64_t *dstOff,
                              const int64_t *count, int64_t *outLen, int64_t *consumed, int64_t *need, int64_t n, int op, int flags,
                              int64_t maxCount, const k4lz4_dict_set *set, const uint32_t *dictIds, void *stream)
{
    int rc;
    if ((rc = fed_args(ctx, r, store, storeOff, srcOff, srcLen, dst, dstOff, count, outLen, consumed, need, n, op, flags)) != K4LZ4_OK) return rc;
    if (n > 0 && op != K4LZ4_FREAD_RESET && !src) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    const int interactive = (flags & K4LZ4_FREAD_INTERACTIVE) ? 1 : 0;
    const k4::FrFeedArgs a{{src, srcOff, srcLen, store, storeOff, dst, dstOff, count, outLen, (long long)n, op, interactive, r->settings.maxBlockSize,
                            nullptr}, final, consumed, need};
    const long long rows = op == K4LZ4_FREAD_READ && !interactive ? k4::fr_table_rows(maxCount) : 0;
    if (!set) return read_device<FedFrameReader>(ctx, a, rows, stream);
    k4::FrDict d;
    if ((rc = reader_dict(ctx, set, dictIds, (hipStream_t)stream, &d)) != K4LZ4_OK) return rc;
    return read_device<DictFedFrameReader>(ctx, {a, d}, rows, stream);
}

int k4lz4_frame_read_fed_batch_device(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff,
                                      const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, const int64_t *final,
                                      uint8_t *dst, const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t *consumed,
                                      int64_t *need, int64_t n, int op, int flags, int64_t maxCount, void *stream)
{
    return frame_read_fed_run(ctx, r, store, storeOff, src, srcOff, srcLen, final, dst, dstOff, count, outLen, consumed, need, n, op, flags, maxCount,
                              nullptr, nullptr, stream);
}

int k4lz4_frame_read_fed_dictset_batch_device(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff,
                                              const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, const int64_t *final,
                                              uint8_t *dst, const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t *consumed,
                                              int64_t *need, int64_t n, int op, int flags, int64_t maxCount, const k4lz4_dict_set *set,
                                              const uint32_t *dictIds, void *stream)
{
    const int rc = frame_dict_args(ctx, set, dictIds, "k4lz4_frame_read_fed_dictset_batch");
    if (rc != K4LZ4_OK) return rc;
    return frame_read_fed_run(ctx, r, store, storeOff, src, srcOff, srcLen, final, dst, dstOff, count, outLen, consumed, need, n, op, flags, maxCount,
                              set, dictIds, stream);
}

static int frame_read_fed_host(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                               const uint64_t *srcOff, const uint64_t *srcLen, const int64_t *final, uint8_t *dst, const uint64_t *dstOff,
                               const int64_t *count, int64_t *outLen, int64_t *consumed, int64_t *need, int64_t n, int op, int flags,
                               const k4lz4_dict_set *set, const uint32_t *dictIds)
{
    int rc;
    if ((rc = fed_args(ctx, r, store, storeOff, srcOff, srcLen, dst, dstOff, count, outLen, consumed, need, n, op, flags)) != K4LZ4_OK) return rc;
    if (n == 0) return K4LZ4_OK;
    return host_read(ctx, {storeOff, src, srcOff, srcLen, final, dst, dstOff, count, outLen, consumed, need}, n,
                     /* sends */ op != K4LZ4_FREAD_RESET, /* fills */ op == K4LZ4_FREAD_READ,
                     [&](const ReadArrays &d, int64_t maxCount, hipStream_t st) {
                         return frame_read_fed_run(ctx, r, store, d.storeOff, d.src, d.srcOff, d.srcLen, d.final, d.dst, d.dstOff, d.count,
                                                   d.outLen, d.consumed, d.need, n, op, flags, maxCount, set, dictIds, st);
                     });
}

int k4lz4_frame_read_fed_batch(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                               const uint64_t *srcOff, const uint64_t *srcLen, const int64_t *final, uint8_t *dst, const uint64_t *dstOff,
                               const int64_t *count, int64_t *outLen, int64_t *consumed, int64_t *need, int64_t n, int op, int flags)
{
    return frame_read_fed_host(ctx, r, store, storeOff, src, srcOff, srcLen, final, dst, dstOff, count, outLen, consumed, need, n, op, flags,
                               nullptr, nullptr);
}

int k4lz4_frame_read_fed_dictset_batch(k4lz4_ctx *ctx, const k4lz4_frame_reader *r, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                                       const uint64_t *srcOff, const uint64_t *srcLen, const int64_t *final, uint8_t *dst, const uint64_t *dstOff,
                                       const int64_t *count, int64_t *outLen, int64_t *consumed, int64_t *need, int64_t n, int op, int flags,
                                       const k4lz4_dict_set *set, const uint32_t *dictIds)
{
    const int rc = frame_dict_args(ctx, set, dictIds, "k4lz4_frame_read_fed_dictset_batch");
    if (rc != K4LZ4_OK) return rc;
    return frame_read_fed_host(ctx, r, store, storeOff, src, srcOff, srcLen, final, dst, dstOff, count, outLen, consumed, need, n, op, flags, set,
                               dictIds);
}

/* ---- LZ4Stream written and read piece by piece (k4lz4_legacy_stream.hpp) ---------------------------------- */
int k4lz4_legacy_writer_init(k4lz4_legacy_writer *w, int blockSize, int high)
{
    if (!w) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_legacy_writer_init: NULL argument");
    if (blockSize > 0x7E000000) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_legacy_writer_init: block size above 0x7E000000");
    w->blockSize = std::max(16, blockSize);              /* LZ4Stream.cs:89 */
    w->high = high ? 1 : 0;
    w->pending = 0; w->closed = 0;
    return K4LZ4_OK;
}

int64_t k4lz4_legacy_writer_store_bytes(const k4lz4_legacy_writer *w) { return w ? k4::ls_w_store_bytes(*w) : 0; }

int64_t k4lz4_legacy_write_bound(const k4lz4_legacy_writer *w, int64_t srcLen, int op)
{
    return w && op >= K4LZ4_LWRITE_WRITE && op <= K4LZ4_LWRITE_CLOSE ? k4::ls_w_bound(*w, srcLen, op) : 0;
}

int k4lz4_legacy_write_batch_device(k4lz4_ctx *ctx, k4lz4_legacy_writer *w, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                                    const uint64_t *srcOff, const int64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                                    int64_t *outLen, int64_t n, int op, int flags, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!w || !store || !storeOff || !srcOff || !srcLen || !dst || !dstOff || !dstCap || !outLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (op < K4LZ4_LWRITE_WRITE || op > K4LZ4_LWRITE_CLOSE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_write_batch: unknown op");
    if (flags & ~(int)K4LZ4_FLAG_X32) return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_write_batch: the only flag it takes is K4LZ4_FLAG_X32");
    if (n == 0) return K4LZ4_OK;
    for (int64_t i = 0; i < n; i++) {
        if (op == K4LZ4_LWRITE_FLUSH && srcLen[i] > 0) return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_write_batch: a flush takes no bytes");
        if (srcLen[i] > 0 && !src) return fail(ctx, K4LZ4_E_ARG, "bad argument");
        if (srcLen[i] >= 0 && (w[i].blockSize < 16 || w[i].pending < 0 || w[i].pending > w[i].blockSize))
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_write_batch: the record was not made by k4lz4_legacy_writer_init");
    }
    hipStream_t st = (hipStream_t)stream;

    /* ---- the plan: per-stream codes and the chunk table -- host arithmetic over lengths, nothing enqueued yet */
    std::vector<int32_t> code;
    k4::LsWLayout L;
    try { k4::ls_w_layout(w, srcLen, dstCap, n, op, code, L); } catch (...) { return fail(ctx, K4LZ4_E_NOMEM, "out of host memory"); }
    if (L.rows > 0xffffffffll) return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_write_batch: more than 2^32 chunks in one call");
    K4_HIP(ctx, hipSetDevice(ctx->device));
    PlanUpload &plan = ctx->fw_plan;      /* the writers share the plan buffers */
    int rc;
    if ((rc = plan_begin(ctx, plan, L.plan_bytes + 64, true)) != K4LZ4_OK) return rc;
    if ((rc = grow_scratch(ctx, &plan.dev, &plan.cap, L.total)) != K4LZ4_OK) return rc;
    uint8_t *h = plan.host.data(), *d = plan.dev;
    k4::ls_w_fill(w, store, storeOff, src, srcOff, srcLen, dstOff, n, op, code, L, h, d);

    /* ---- enqueue: plan up, stage, encode (a batch per level), records, assembly, tails, lengths */
    if ((rc = plan_send(ctx, plan, d, L.plan_bytes, st)) != K4LZ4_OK) return rc;
    k4::LsWriteArgs a{};
    a.streams = (const k4::LsWStream *)(d + L.o_streams); a.n = n; a.rows = L.rows;
    a.cSrc = (const uint64_t *)(d + L.o_src); a.cEnc = (const uint64_t *)(d + L.o_enc); a.cLen = (const int32_t *)(d + L.o_len);
    a.owner = (const uint32_t *)(d + L.o_owner);
    a.cEncLen = (int32_t *)(d + L.o_elen); a.recLen = (uint64_t *)(d + L.o_rlen); a.recOff = (uint64_t *)(d + L.o_roff);
    if (L.nstage) hipLaunchKernelGGL(k4::k4_fw_copy_kernel, dim3((unsigned)L.stage_chunks), dim3(k4::FW_THREADS), 0, st,
                                     (const k4::FwPiece *)(d + L.o_stage), (long long)L.nstage);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    /* sources and arena slots are addresses (window, store, the caller's bytes): the encoder's bases are null.  The lengths are
     * on the host, so HC sizes its work area without asking the device. */
    const int32_t *hlen = (const int32_t *)(h + L.o_len), *dcap = (const int32_t *)(d + L.o_cap);
    const int xf = flags & K4LZ4_FLAG_X32;
    if (L.nfast && (rc = launch(ctx, KIND_ENCODE, nullptr, a.cSrc, a.cLen, nullptr, a.cEnc, dcap, a.cEncLen, L.nfast, K4LZ4_L00_FAST,
                                xf | K4LZ4_FLAG_RAW_RETURN, st, nullptr, hlen)) != K4LZ4_OK)
        return rc;
    if (L.rows > L.nfast && (rc = launch(ctx, KIND_ENCODE, nullptr, a.cSrc + L.nfast, a.cLen + L.nfast, nullptr, a.cEnc + L.nfast, dcap + L.nfast,
                                         a.cEncLen + L.nfast, L.rows - L.nfast, K4LZ4_L09_HC, xf | K4LZ4_FLAG_RAW_RETURN, st, nullptr,
                                         hlen + L.nfast)) != K4LZ4_OK)
        return rc;
    if (L.rows) {
        hipLaunchKernelGGL(k4::k4_ls_reclen_kernel, dim3((unsigned)((L.rows + 255) / 256)), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k4::k4_legacy_scan_kernel, dim3(1), dim3(k4::LEGACY_SCAN_THREADS), 0, st, (const uint64_t *)a.recLen, a.recOff,
                           (long long)L.rows, (unsigned long long *)(d + L.o_cnt));
        hipLaunchKernelGGL(k4::k4_ls_assemble_kernel, dim3((unsigned)((L.rows + 3) / 4)), dim3(256), 0, st, a, dst);
    }
    if (L.ntail) hipLaunchKernelGGL(k4::k4_fw_copy_kernel, dim3((unsigned)L.tail_chunks), dim3(k4::FW_THREADS), 0, st,
                                    (const k4::FwPiece *)(d + L.o_tail), (long long)L.ntail);
    hipLaunchKernelGGL(k4::k4_ls_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, outLen);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);

    /* ---- the records: what the calls enqueued leaves them in */
    for (int64_t i = 0; i < n; i++)
        if (code[(size_t)i] == 0) k4::ls_w_advance(w[i], srcLen[i], op);
    return K4LZ4_OK;
}

int k4lz4_legacy_write_batch(k4lz4_ctx *ctx, k4lz4_legacy_writer *w, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                             const uint64_t *srcOff, const int64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                             int64_t *outLen, int64_t n, int op, int flags)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!w || !store || !storeOff || !srcOff || !srcLen || !dst || !dstOff || !dstCap || !outLen)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (op < K4LZ4_LWRITE_WRITE || op > K4LZ4_LWRITE_CLOSE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_write_batch: unknown op");
    if (n == 0) return K4LZ4_OK;
    for (int64_t i = 0; i < n; i++)
        if (srcLen[i] > 0 && !src) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    K4_HIP(ctx, hipSetDevice(ctx->device));
    /* the output slots: what the call can emit, not the caller's capacities (the codes are decided on dstCap all the same) */
    std::vector<uint64_t> cap((size_t)n);
    std::vector<int64_t> len0((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        cap[(size_t)i] = std::min<uint64_t>(dstCap[i], (uint64_t)k4::ls_w_bound(w[i], srcLen[i], op));
        len0[(size_t)i] = op == K4LZ4_LWRITE_FLUSH ? 0 : std::max<int64_t>(srcLen[i], 0);
    }
    HostStage s(ctx);
    s.pack(src, srcOff, len0.data(), n);
    s.slots(n, [&](int64_t i) { return cap[(size_t)i]; }, false);
    int64_t *d_out;
    s.meta(&d_out, n);
    int rc;
    if ((rc = s.upload()) != K4LZ4_OK ||
        (rc = k4lz4_legacy_write_batch_device(ctx, w, store, storeOff, ctx->d_src, s.in_off.data(), srcLen, ctx->d_dst, s.slot.data(), dstCap,
                                              d_out, n, op, flags, s.st)) != K4LZ4_OK)
        return rc;
    return s.finish({{outLen, d_out, (size_t)n * 8}}, dst, dstOff, [&](int64_t i) { return outLen[i] > 0 ? (size_t)outLen[i] : 0; });
}

int k4lz4_legacy_reader_init(k4lz4_legacy_reader *r, int maxBlockSize)
{
    if (!r) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_legacy_reader_init: NULL argument");
    if (maxBlockSize > 0x7E000000) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_legacy_reader_init: maxBlockSize above 0x7E000000");
    r->maxBlockSize = maxBlockSize <= 0 ? 1 << 20 : std::max(16, maxBlockSize);
    r->flags = 0;
    r->storeBytes = k4::ls_rd_store_bytes(r->maxBlockSize);
    return K4LZ4_OK;
}

int64_t k4lz4_legacy_reader_store_bytes(const k4lz4_legacy_reader *r) { return r ? r->storeBytes : 0; }
int64_t k4lz4_legacy_read_table_rows(const k4lz4_legacy_reader *r, int64_t maxCount) { return r ? k4::ls_table_rows(maxCount, r->maxBlockSize) : 0; }

int k4lz4_legacy_read_batch_device(k4lz4_ctx *ctx, const k4lz4_legacy_reader *r, uint8_t *store, const uint64_t *storeOff,
                                   const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst,
                                   const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t n, int op, int flags,
                                   int64_t maxCount, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (op < K4LZ4_LREAD_READ || op > K4LZ4_LREAD_RESET) return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_read_batch: unknown op");
    if (flags & ~(int)K4LZ4_LREAD_INTERACTIVE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_read_batch: the only flag it takes is K4LZ4_LREAD_INTERACTIVE");
    if (n < 0 || (n > 0 && (!r || !store || !storeOff || !count || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && op == K4LZ4_LREAD_READ && (!src || !srcOff || !srcLen || !dst || !dstOff)) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && (r->maxBlockSize < 16 || r->storeBytes != k4::ls_rd_store_bytes(r->maxBlockSize)))
        return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_read_batch: the record was not made by k4lz4_legacy_reader_init");
    if (n == 0) return K4LZ4_OK;
    const int interactive = (flags & K4LZ4_LREAD_INTERACTIVE) ? 1 : 0;
    return read_device<LegacyReader>(ctx, {src, srcOff, srcLen, store, storeOff, dst, dstOff, count, outLen, (long long)n, op, interactive,
                                           r->maxBlockSize, nullptr},
                                     op == K4LZ4_LREAD_READ && !interactive ? k4::ls_table_rows(maxCount, r->maxBlockSize) : 0, stream);
}

int k4lz4_legacy_read_batch(k4lz4_ctx *ctx, const k4lz4_legacy_reader *r, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                            const uint64_t *srcOff, const uint64_t *srcLen, uint8_t *dst, const uint64_t *dstOff, const int64_t *count,
                            int64_t *outLen, int64_t n, int op, int flags)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (op < K4LZ4_LREAD_READ || op > K4LZ4_LREAD_RESET) return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_read_batch: unknown op");
    if (n < 0 || (n > 0 && (!r || !store || !storeOff || !count || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && op == K4LZ4_LREAD_READ && (!srcOff || !srcLen || !dst || !dstOff)) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    return host_read(ctx, {storeOff, src, srcOff, srcLen, nullptr, dst, dstOff, count, outLen, nullptr, nullptr}, n,
                     /* sends */ op == K4LZ4_LREAD_READ, /* fills */ op == K4LZ4_LREAD_READ,
                     [&](const ReadArrays &d, int64_t maxCount, hipStream_t st) {
                         return k4lz4_legacy_read_batch_device(ctx, r, store, d.storeOff, d.src, d.srcOff, d.srcLen, d.dst, d.dstOff, d.count,
                                                               d.outLen, n, op, flags, maxCount, st);
                     });
}

int k4lz4_legacy_reader_query_device(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out, void *stream)
{
    return query_device(ctx, k4::k4_ls_query_kernel, store, storeOff, n, out, stream);
}

int k4lz4_legacy_reader_query(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out)
{
    return query_host(ctx, K4LZ4_LSQ_WORDS, k4lz4_legacy_reader_query_device, store, storeOff, n, out);
}

/* ---- the incremental LZ4Stream reader fed its source in pieces (k4lz4_legacy_feed.hpp) --------------------- */
int k4lz4_legacy_reader_init_fed(k4lz4_legacy_reader *r, int maxBlockSize)
{
    const int rc = k4lz4_legacy_reader_init(r, maxBlockSize);
    if (rc != K4LZ4_OK) return rc;
    r->flags = K4LZ4_LREADER_FED;
    r->storeBytes = k4::ls_fed_store_bytes(r->maxBlockSize);
    return K4LZ4_OK;
}

/* the record's kind is checked first: a record of the other family is refused whatever else the call holds */
static int lfed_args(k4lz4_ctx *ctx, const k4lz4_legacy_reader *r, const void *store, const void *storeOff, const void *srcOff, const void *srcLen,
                     const void *dst, const void *dstOff, const void *count, const void *outLen, const void *consumed, const void *need,
                     int64_t n, int op, int flags)
{
    if (n > 0 && r && (r->flags != K4LZ4_LREADER_FED || r->maxBlockSize < 16 || r->storeBytes != k4::ls_fed_store_bytes(r->maxBlockSize)))
        return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_read_fed_batch: the record was not made by k4lz4_legacy_reader_init_fed");
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (op < K4LZ4_LREAD_READ || op > K4LZ4_LREAD_RESET) return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_read_fed_batch: unknown op");
    if (flags & ~(int)K4LZ4_LREAD_INTERACTIVE) return fail(ctx, K4LZ4_E_ARG, "k4lz4_legacy_read_fed_batch: the only flag it takes is K4LZ4_LREAD_INTERACTIVE");
    if (n < 0 || (n > 0 && (!r || !store || !storeOff || !count || !outLen || !consumed || !need))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && op == K4LZ4_LREAD_READ && (!srcOff || !srcLen || !dst || !dstOff)) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    return K4LZ4_OK;
}

int k4lz4_legacy_read_fed_batch_device(k4lz4_ctx *ctx, const k4lz4_legacy_reader *r, uint8_t *store, const uint64_t *storeOff,
                                       const uint8_t *src, const uint64_t *srcOff, const uint64_t *srcLen, const int64_t *final,
                                       uint8_t *dst, const uint64_t *dstOff, const int64_t *count, int64_t *outLen, int64_t *consumed,
                                       int64_t *need, int64_t n, int op, int flags, int64_t maxCount, void *stream)
{
    int rc;
    if ((rc = lfed_args(ctx, r, store, storeOff, srcOff, srcLen, dst, dstOff, count, outLen, consumed, need, n, op, flags)) != K4LZ4_OK) return rc;
    if (n > 0 && op == K4LZ4_LREAD_READ && !src) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    const int interactive = (flags & K4LZ4_LREAD_INTERACTIVE) ? 1 : 0;
    return read_device<FedLegacyReader>(ctx, {{src, srcOff, srcLen, store, storeOff, dst, dstOff, count, outLen, (long long)n, op, interactive,
                                               r->maxBlockSize, nullptr}, final, consumed, need, nullptr},
                                        op == K4LZ4_LREAD_READ && !interactive ? k4::ls_table_rows(maxCount, r->maxBlockSize) : 0, stream);
}

int k4lz4_legacy_read_fed_batch(k4lz4_ctx *ctx, const k4lz4_legacy_reader *r, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                                const uint64_t *srcOff, const uint64_t *srcLen, const int64_t *final, uint8_t *dst, const uint64_t *dstOff,
                                const int64_t *count, int64_t *outLen, int64_t *consumed, int64_t *need, int64_t n, int op, int flags)
{
    int rc;
    if ((rc = lfed_args(ctx, r, store, storeOff, srcOff, srcLen, dst, dstOff, count, outLen, consumed, need, n, op, flags)) != K4LZ4_OK) return rc;
    if (n == 0) return K4LZ4_OK;
    return host_read(ctx, {storeOff, src, srcOff, srcLen, final, dst, dstOff, count, outLen, consumed, need}, n,
                     /* sends */ op == K4LZ4_LREAD_READ, /* fills */ op == K4LZ4_LREAD_READ,
                     [&](const ReadArrays &d, int64_t maxCount, hipStream_t st) {
                         return k4lz4_legacy_read_fed_batch_device(ctx, r, store, d.storeOff, d.src, d.srcOff, d.srcLen, d.final, d.dst, d.dstOff,
                                                                   d.count, d.outLen, d.consumed, d.need, n, op, flags, maxCount, st);
                     });
}

/* ---- many open ILZ4Decoders advanced per call (k4lz4_chain_decoder.hpp) ------------------------------------ */
static_assert(sizeof(k4lz4_chain_decoder) == sizeof(k4::CdRecord), "k4lz4_chain_decoder and the kernels' CdRecord are one layout");

int k4lz4_chain_decoder_init(k4lz4_chain_decoder *d, const k4lz4_chain_decoder_settings *settings)
{
    if (!d) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_chain_decoder_init: NULL argument");
    const int64_t B = k4::cd_block_size(settings ? settings->blockSize : 0);
    const bool chaining = settings && settings->chaining != 0;
    const int64_t extra = chaining ? std::max<int64_t>(settings->extraBlocks, 0) : 0;
    if (B > k4::CD_MAX_RING || extra > k4::CD_MAX_RING || k4::cd_ring_length(B, extra, chaining) > k4::CD_MAX_RING)
        return fail(nullptr, K4LZ4_E_ARG, "k4lz4_chain_decoder_init: the ring buffer passes 0x7E000000 bytes");
    d->blockSize = (int32_t)B; d->extraBlocks = (int32_t)extra; d->chaining = chaining ? 1 : 0; d->reserved = 0;
    d->storeBytes = k4::cd_store_bytes(B, extra, chaining);
    return K4LZ4_OK;
}

int64_t k4lz4_chain_decoder_store_bytes(const k4lz4_chain_decoder *d) { return d ? d->storeBytes : 0; }

static int cdec_args(k4lz4_ctx *ctx, const void *dec, const void *store, const void *storeOff, const void *src, const void *recOff,
                     const void *recLen, const void *firstRec, const void *nRec, const void *dst, const void *dstOff, const void *dstCap,
                     const void *recOut, const void *outLen, int64_t n, int op, int flags)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (op < K4LZ4_CDEC_RUN || op > K4LZ4_CDEC_RESET) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decode_batch: unknown op");
    if (flags & ~(int)K4LZ4_CDEC_DRAIN) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decode_batch: the only flag it takes is K4LZ4_CDEC_DRAIN");
    if (n < 0 || (n > 0 && (!store || !storeOff || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && ((uintptr_t)store & 255u)) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decode_batch: the store is not 256-byte aligned");
    if (n > 0 && op == K4LZ4_CDEC_RESET && !dec) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decode_batch: RESET takes the decoders' records");
    /* src, recOff and recLen belong to the record table, which is empty when every nRec is 0: only the host form, which is told
       nRecords, can refuse them; the kernel reads none of them for a stream without records */
    if (n > 0 && op == K4LZ4_CDEC_RUN && (!firstRec || !nRec || !recOut)) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && op == K4LZ4_CDEC_RUN && (flags & K4LZ4_CDEC_DRAIN) && (!dst || !dstOff || !dstCap)) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    return K4LZ4_OK;
}

int k4lz4_chain_decode_batch_device(k4lz4_ctx *ctx, const k4lz4_chain_decoder *dec, uint8_t *store, const uint64_t *storeOff,
                                    const uint8_t *src, const uint64_t *recOff, const uint32_t *recLen, const int32_t *recBlockSize,
                                    const uint64_t *firstRec, const uint32_t *nRec, uint8_t *dst, const uint64_t *dstOff,
                                    const uint64_t *dstCap, int32_t *recOut, int64_t *outLen, int64_t n, int op, int flags, void *stream)
{
    int rc;
    if ((rc = cdec_args(ctx, dec, store, storeOff, src, recOff, recLen, firstRec, nRec, dst, dstOff, dstCap, recOut, outLen, n, op, flags)) !=
        K4LZ4_OK)
        return rc;
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    K4_HIP(ctx, order_after_ctx(ctx, st));
    if (op == K4LZ4_CDEC_RESET) {
        hipLaunchKernelGGL(k4::k4_cdec_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const k4::CdRecord *)dec, store,
                           storeOff, outLen, (long long)n);
    } else {
        k4::CdRunArgs a{src, recOff, recLen, recBlockSize, firstRec, nRec, store, storeOff, dst, dstOff, dstCap, recOut, outLen, (long long)n,
                        flags, ctx->d_status};
        hipLaunchKernelGGL(k4::k4_cdec_run_kernel, dim3((unsigned)((n + k4::DECODE_PAIRS_PER_WG - 1) / k4::DECODE_PAIRS_PER_WG)),
                           dim3(128 * k4::DECODE_PAIRS_PER_WG), 0, st, a);
    }
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    return K4LZ4_OK;
}

int k4lz4_chain_decode_batch(k4lz4_ctx *ctx, const k4lz4_chain_decoder *dec, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                             const uint64_t *recOff, const uint32_t *recLen, const int32_t *recBlockSize, int64_t nRecords,
                             const uint64_t *firstRec, const uint32_t *nRec, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                             int32_t *recOut, int64_t *outLen, int64_t n, int op, int flags)
{
    int rc;
    if ((rc = cdec_args(ctx, dec, store, storeOff, src, recOff, recLen, firstRec, nRec, dst, dstOff, dstCap, recOut, outLen, n, op, flags)) !=
        K4LZ4_OK)
        return rc;
    if (n == 0) return K4LZ4_OK;
    const bool runs = op == K4LZ4_CDEC_RUN, drains = runs && (flags & K4LZ4_CDEC_DRAIN);
    if (nRecords < 0 || (runs && nRecords > 0 && (!recOff || !recLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    for (int64_t i = 0; i < n; i++) {
        if (storeOff[i] & 255u) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decode_batch: a stream's store is not 256-byte aligned");
        if (runs && firstRec[i] + nRec[i] > (uint64_t)nRecords && nRec[i])
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decode_batch: a stream refers to records outside the record table");
        if (!runs && (dec[i].blockSize != k4::cd_block_size(dec[i].blockSize) || dec[i].extraBlocks < 0 || (dec[i].chaining & ~1) ||
                      dec[i].storeBytes != k4::cd_store_bytes(dec[i].blockSize, dec[i].extraBlocks, dec[i].chaining != 0)))
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decode_batch: a record was not made by k4lz4_chain_decoder_init");
    }
    /* only the records of streams that run send their bytes up */
    std::vector<uint8_t> used((size_t)(runs ? nRecords : 0), 0);
    for (int64_t i = 0; runs && i < n; i++)
        for (uint32_t k = 0; k < nRec[i]; k++) used[(size_t)(firstRec[i] + k)] = 1;
    for (int64_t r = 0; runs && r < nRecords; r++)
        if (used[(size_t)r] && (recLen[r] & 0x7fffffffu) && !src) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    K4_HIP(ctx, hipSetDevice(ctx->device));
    HostStage s(ctx);
    const int64_t nr = runs ? nRecords : 0;
    s.span(src, recOff, nr, [&](int64_t r) { return used[(size_t)r] ? (uint64_t)(recLen[r] & 0x7fffffffu) : (uint64_t)0; });
    if (drains) s.slots(n, [&](int64_t i) { return nRec[i] ? dstCap[i] : (uint64_t)0; }, false);
    uint64_t *d_store, *d_roff = nullptr, *d_first = nullptr, *d_doff = nullptr, *d_dcap = nullptr;
    uint32_t *d_rlen = nullptr, *d_nrec = nullptr;
    int32_t *d_rbs = nullptr, *d_rout = nullptr;
    int64_t *d_out;
    k4lz4_chain_decoder *d_dec = nullptr;
    s.meta(&d_store, n, storeOff); s.meta(&d_out, n);
    if (runs) {
        s.meta(&d_roff, nr, s.in_off.data()); s.meta(&d_rlen, nr, recLen);
        if (recBlockSize) s.meta(&d_rbs, nr, recBlockSize);
        s.meta(&d_first, n, firstRec); s.meta(&d_nrec, n, nRec); s.meta(&d_rout, nr);
        if (drains) { s.meta(&d_doff, n, s.slot.data()); s.meta(&d_dcap, n, dstCap); }
    } else {
        s.meta(&d_dec, n, dec);
    }
    if ((rc = s.upload()) != K4LZ4_OK ||
        (rc = k4lz4_chain_decode_batch_device(ctx, d_dec, store, d_store, ctx->d_src, d_roff, d_rlen, d_rbs, d_first, d_nrec, ctx->d_dst, d_doff,
                                              d_dcap, d_rout, d_out, n, op, flags, s.st)) != K4LZ4_OK)
        return rc;
    /* the kernel writes the rows of streams that run and no others: only those reach the caller's recOut */
    std::vector<int32_t> rout((size_t)nr, 0);
    /* a stream's slot holds what its records produced before the one that failed, if one did */
    auto drained = [&](int64_t i) {
        size_t b = 0;
        for (uint32_t k = 0; drains && k < nRec[i]; k++) {
            const int32_t got = rout[(size_t)(firstRec[i] + k)];
            if (got < 0) break;
            b += (size_t)got;
        }
        return b;
    };
    if ((rc = s.finish({{outLen, d_out, (size_t)n * 8}, {rout.data(), d_rout, (size_t)nr * 4}}, dst, dstOff, drained)) != K4LZ4_OK) return rc;
    for (int64_t r = 0; r < nr; r++)
        if (used[(size_t)r]) recOut[r] = rout[(size_t)r];
    return K4LZ4_OK;
}

int k4lz4_chain_drain_batch_device(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, const int64_t *offset, const int64_t *length,
                                   uint8_t *dst, const uint64_t *dstOff, int64_t *outLen, int64_t n, void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!store || !storeOff || !offset || !length || !dst || !dstOff || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && ((uintptr_t)store & 255u)) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_drain_batch: the store is not 256-byte aligned");
    if (n == 0) return K4LZ4_OK;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    K4_HIP(ctx, order_after_ctx(ctx, st));
    k4::CdDrainArgs a{store, storeOff, dst, dstOff, offset, length, outLen, (long long)n};
    hipLaunchKernelGGL(k4::k4_cdec_drain_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, a);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    return K4LZ4_OK;
}

int k4lz4_chain_drain_batch(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, const int64_t *offset, const int64_t *length,
                            uint8_t *dst, const uint64_t *dstOff, int64_t *outLen, int64_t n)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!store || !storeOff || !offset || !length || !dstOff || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    if ((uintptr_t)store & 255u) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_drain_batch: the store is not 256-byte aligned");
    for (int64_t i = 0; i < n; i++) {
        if (storeOff[i] & 255u) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_drain_batch: a stream's store is not 256-byte aligned");
        if (length[i] > 0 && !dst) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    }
    /* a range the device will refuse takes no room: the slots are sized by what each decoder holds now */
    std::vector<int64_t> q((size_t)n * K4LZ4_CDQ_WORDS);
    int rc;
    if ((rc = k4lz4_chain_decoder_query(ctx, store, storeOff, n, q.data())) != K4LZ4_OK) return rc;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    HostStage s(ctx);
    s.slots(n, [&](int64_t i) {
        return length[i] > 0 && length[i] <= q[(size_t)i * K4LZ4_CDQ_WORDS + K4LZ4_CDQ_BYTES_READY] ? (uint64_t)length[i] : (uint64_t)0;
    }, false);
    uint64_t *d_store, *d_doff;
    int64_t *d_offset, *d_length, *d_out;
    s.meta(&d_store, n, storeOff); s.meta(&d_doff, n, s.slot.data()); s.meta(&d_offset, n, offset); s.meta(&d_length, n, length); s.meta(&d_out, n);
    if ((rc = s.upload()) != K4LZ4_OK ||
        (rc = k4lz4_chain_drain_batch_device(ctx, store, d_store, d_offset, d_length, ctx->d_dst, d_doff, d_out, n, s.st)) != K4LZ4_OK)
        return rc;
    return s.finish({{outLen, d_out, (size_t)n * 8}}, dst, dstOff, [&](int64_t i) { return outLen[i] > 0 ? (size_t)outLen[i] : 0; });
}

int k4lz4_chain_decoder_query_device(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out, void *stream)
{
    return query_device(ctx, k4::k4_cdec_query_kernel, store, storeOff, n, out, stream);
}

int k4lz4_chain_decoder_query(k4lz4_ctx *ctx, const uint8_t *store, const uint64_t *storeOff, int64_t n, int64_t *out)
{
    return query_host(ctx, K4LZ4_CDQ_WORDS, k4lz4_chain_decoder_query_device, store, storeOff, n, out);
}

/* ---- many open ILZ4Encoders advanced per call (k4lz4_chain_encoder.hpp) ------------------------------------ */
int k4lz4_chain_encoder_init(k4lz4_chain_encoder *e, const k4lz4_chain_encoder_settings *settings)
{
    if (!e || !settings) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_chain_encoder_init: NULL argument");
    if (settings->blockSize > k4::MAX_INPUT_SIZE - 1023)
        return fail(nullptr, K4LZ4_E_ARG, "k4lz4_chain_encoder_init: block size above the input size limit");
    k4::ce_init(*e, *settings);
    if ((int64_t)65536 + (1 + (int64_t)e->extraBlocks) * e->blockSize + 32 > 0x7E000000ll)
        return fail(nullptr, K4LZ4_E_ARG, "k4lz4_chain_encoder_init: the ring buffer passes 0x7E000000 bytes");
    return K4LZ4_OK;
}

int64_t k4lz4_chain_encoder_store_bytes(const k4lz4_chain_encoder *e) { return e ? e->storeBytes : 0; }

int64_t k4lz4_chain_encode_bound(const k4lz4_chain_encoder *e, const uint32_t *recLen, const uint32_t *recFlags, int64_t nRec)
{
    if (!e || nRec <= 0 || !recLen || !recFlags) return 0;
    return k4::ce_after(*e, recLen, recFlags, nRec).bound;
}

int k4lz4_chain_encode_plan(const k4lz4_chain_encoder *e, const uint32_t *recLen, const uint32_t *recFlags, int64_t nRec,
                            k4lz4_chain_encoder *after, int32_t *recLoaded, int32_t *blockLen)
{
    if (!e || nRec < 0 || (nRec > 0 && (!recLen || !recFlags))) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_chain_encode_plan: bad argument");
    for (int64_t r = 0; r < nRec; r++) if (blockLen) blockLen[r] = 0;
    const k4::CeAfter a = k4::ce_model(*e, recLen, recFlags, nRec,
                                       [&](int64_t r, int64_t loaded, int64_t) { if (recLoaded) recLoaded[r] = (int32_t)loaded; },
                                       [&](int64_t r, int64_t, int64_t len, int64_t, int64_t, bool) { if (blockLen) blockLen[r] = (int32_t)len; });
    if (after) { *after = *e; k4::ce_advance(*after, a); }
    return K4LZ4_OK;
}

int64_t k4lz4_chain_encode_blocks(const k4lz4_chain_encoder *e, const uint32_t *recLen, const uint32_t *recFlags, int64_t nRec, int64_t *rows,
                                  int64_t maxRows)
{
    if (!e || nRec < 0 || (nRec > 0 && (!recLen || !recFlags)) || maxRows < 0 || (maxRows > 0 && !rows)) return -1;
    int64_t k = 0;
    k4::ce_model(*e, recLen, recFlags, nRec, [](int64_t, int64_t, int64_t) {},
                 [&](int64_t, int64_t start, int64_t len, int64_t dict, int64_t ws, bool small) {
                     if (k < maxRows) { int64_t *r = rows + 4 * k; r[0] = start; r[1] = len; r[2] = e->kind == 2 ? dict : ws; r[3] = small ? 1 : 0; }
                     k++;
                 });
    return k;
}

int k4lz4_chain_table_rows(int kind, int64_t dictLen, int64_t currentOffset, const int32_t *len, int64_t n, int32_t blockSize,
                           int32_t extraBlocks, int64_t *rows)
{
    if ((kind != 1 && kind != 2) || dictLen < 0 || n < 0 || (n > 0 && (!len || !rows))) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_chain_table_rows: bad argument");
    const int64_t B = hc_chain_block_size(blockSize), extra = std::max<int32_t>(extraBlocks, 0);
    if (kind == 1)
        k4::ce_hc_rows(dictLen, len, n, B, extra, [&](int64_t j, int64_t, int64_t pos, int64_t l, int64_t dl) {
            int64_t *r = rows + 4 * j; r[0] = pos; r[1] = l; r[2] = dl; r[3] = 0;
        });
    else
        k4::ce_fast_rows(dictLen, currentOffset, len, n, B, extra, [&](int64_t j, int64_t pos, int64_t l, int64_t d, bool small) {
            int64_t *r = rows + 4 * j; r[0] = pos; r[1] = l; r[2] = d; r[3] = small ? 1 : 0;
        });
    return K4LZ4_OK;
}

/* is the record one that k4lz4_chain_encoder_init made and the calls advanced? */
static bool ce_record_ok(const k4lz4_chain_encoder &e)
{
    k4lz4_chain_encoder probe;
    const k4lz4_chain_encoder_settings back{e.kind != 0, e.kind == 2 ? 0 : e.kind == 1 ? std::max<int32_t>(e.level, K4LZ4_L03_HC) : e.level,
                                            e.blockSize, e.extraBlocks};
    k4::ce_init(probe, back);
    return !(e.kind < 0 || e.kind > 2 || probe.kind != e.kind || probe.blockSize != e.blockSize || probe.ringBytes != e.ringBytes ||
             probe.storeBytes != e.storeBytes || e.index < 0 || e.index > e.pointer || e.pointer > e.ringBytes);
}

int k4lz4_chain_encode_batch_device(k4lz4_ctx *ctx, k4lz4_chain_encoder *enc, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                                    const uint64_t *recOff, const uint32_t *recLen, const uint32_t *recFlags, int64_t nRecords,
                                    const uint64_t *firstRec, const uint32_t *nRec, uint8_t *dst, const uint64_t *dstOff,
                                    const uint64_t *dstCap, int32_t *recLoaded, int32_t *recOut, int64_t *outLen, int64_t n, int op, int flags,
                                    void *stream)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (op < K4LZ4_CENC_RUN || op > K4LZ4_CENC_RESET) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: unknown op");
    if (flags & ~(int)K4LZ4_FLAG_X32) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: the only flag it takes is K4LZ4_FLAG_X32");
    if (n < 0 || nRecords < 0 || (n > 0 && (!enc || !store || !storeOff))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    if ((uintptr_t)store & 255u) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: the store is not 256-byte aligned");
    for (int64_t i = 0; i < n; i++) {
        if (storeOff[i] & 255u) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: a stream's store is not 256-byte aligned");
        if (!ce_record_ok(enc[i])) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: a record was not made by k4lz4_chain_encoder_init");
    }
    const bool x32 = (flags & K4LZ4_FLAG_X32) || g_enforce32.load(std::memory_order_relaxed);
    hipStream_t st = (hipStream_t)stream;
    std::vector<k4::FwPiece> stage, back;
    PlanUpload &plan = ctx->fw_plan;      /* the writers' */
    int rc;

    if (op == K4LZ4_CENC_RESET) {
        for (int64_t i = 0; i < n; i++)
            if (enc[i].kind == 2)
                stage.push_back(k4::FwPiece{store + storeOff[i], nullptr, sizeof(k4lz4_fast_chain_state), 0});
        if (!stage.empty()) {
            const unsigned long long c = fw_chunks(stage.data(), stage.size());
            const size_t bytes = stage.size() * sizeof(k4::FwPiece);
            K4_HIP(ctx, hipSetDevice(ctx->device));
            if ((rc = plan_begin(ctx, plan, bytes + 64, true)) != K4LZ4_OK) return rc;
            if ((rc = grow_scratch(ctx, &plan.dev, &plan.cap, bytes + 64)) != K4LZ4_OK) return rc;
            memcpy(plan.host.data(), stage.data(), bytes);
            if ((rc = plan_send(ctx, plan, plan.dev, bytes, st)) != K4LZ4_OK) return rc;
            hipLaunchKernelGGL(k4::k4_fw_copy_kernel, dim3((unsigned)c), dim3(k4::FW_THREADS), 0, st, (const k4::FwPiece *)plan.dev, (long long)stage.size());
            K4_HIP(ctx, hipGetLastError());
            mark_busy(ctx, st);
        }
        for (int64_t i = 0; i < n; i++) {
            k4lz4_chain_encoder &e = enc[i];
            e.index = e.pointer = 0; e.currentOffset = e.dictSize = 0; e.taken = e.blocks = 0;
        }
        return K4LZ4_OK;
    }

    if (!firstRec || !nRec || !dstOff || !dstCap || !outLen || !dst) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    /* ---- the plan: per-stream codes and the model's blocks -- host index arithmetic, nothing enqueued yet */
    std::vector<int32_t> code((size_t)n, 1);
    std::vector<k4::CeAfter> after((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (nRec[i] == 0) continue;
        if (firstRec[i] > (uint64_t)nRecords || (uint64_t)nRec[i] > (uint64_t)nRecords - firstRec[i])
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: a stream refers to records outside the record table");
        if (!recOff || !recLen || !recFlags || !recLoaded || !recOut) return fail(ctx, K4LZ4_E_ARG, "bad argument");
        const uint32_t *rl = recLen + firstRec[i], *rf = recFlags + firstRec[i];
        for (uint32_t r = 0; r < nRec[i]; r++) {
            if (rf[r] & ~(uint32_t)(K4LZ4_CENC_FORCE | K4LZ4_CENC_ALLOW_COPY)) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: unknown record flags");
            if (rl[r] > 0x7fffffffu) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: a record longer than INT32_MAX");
            if (rl[r] && !src) return fail(ctx, K4LZ4_E_ARG, "bad argument");
        }
        if (enc[i].kind == 2 && x32)
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: the 32-bit engine's chained encoder (LZ4Codec.Enforce32) is not supported");
        after[(size_t)i] = k4::ce_after(enc[i], rl, rf, nRec[i]);
        if (after[(size_t)i].too_long)
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: a chained stream longer than 2 GB (the encoder's renormalisation) is not supported");
        code[(size_t)i] = (int64_t)std::min<uint64_t>(dstCap[i], (uint64_t)INT64_MAX) < after[(size_t)i].bound ? K4LZ4_CENC_TARGET : 0;
    }
    /* groups of streams whose blocks go to one encoder call: (kind, level) */
    auto key = [&](int64_t i) { return enc[i].kind * 100 + (enc[i].kind == 2 ? 0 : enc[i].level); };
    std::vector<int> keys;
    for (int64_t i = 0; i < n; i++) if (code[(size_t)i] == 0 && after[(size_t)i].nblk) keys.push_back(key(i));
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    struct Group { int key; std::vector<int64_t> streams; int64_t first = 0, nb = 0; };
    std::vector<Group> groups(keys.size());
    for (size_t g = 0; g < keys.size(); g++) groups[g].key = keys[g];
    for (int64_t i = 0; i < n; i++)
        if (code[(size_t)i] == 0 && after[(size_t)i].nblk)
            groups[(size_t)(std::lower_bound(keys.begin(), keys.end(), key(i)) - keys.begin())].streams.push_back(i);
    int64_t nb = 0, nfast = 0;
    for (Group &g : groups) {
        g.first = nb;
        for (int64_t i : g.streams) g.nb += after[(size_t)i].nblk;
        nb += g.nb;
        if (g.key / 100 == 2) nfast += (int64_t)g.streams.size();
    }
    if (nb > 0x7fffffffll) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: more than 2^31 blocks in one call");

    /* ---- scratch layout: the uploaded plan first, then what the kernels fill, then windows, arena and states */
    size_t at = 0;
    const size_t o_streams = fw_take(at, (size_t)n * sizeof(k4::CeStream)), o_recs = fw_take(at, (size_t)nRecords * sizeof(k4::CeRec)),
                 o_blocks = fw_take(at, (size_t)nb * sizeof(k4::CeBlock)), o_slot = fw_take(at, (size_t)nb * 8),
                 o_isrc = fw_take(at, (size_t)nb * 8), o_ilen = fw_take(at, (size_t)nb * 4), o_icap = fw_take(at, (size_t)nb * 4);
    std::vector<uint64_t> win((size_t)n, 0), aoff((size_t)n, 0);
    /* (the pieces' tables follow the fixed part: their count is known once the streams are walked, their room is bounded now) */
    size_t npiece_max = 0;
    for (int64_t i = 0; i < n; i++) if (code[(size_t)i] == 0) npiece_max += (size_t)nRec[i] + 4;
    const size_t o_stage = fw_take(at, npiece_max * sizeof(k4::FwPiece)), o_back = fw_take(at, (2 * (size_t)n + 1) * sizeof(k4::FwPiece));
    const size_t plan_bytes = at;
    const size_t o_out = fw_take(at, (size_t)nb * 4);
    for (const Group &g : groups)
        for (int64_t i : g.streams) { win[(size_t)i] = at; fw_take(at, (size_t)(enc[i].pointer + after[(size_t)i].loaded) + 16); }
    for (const Group &g : groups)
        for (int64_t i : g.streams) { aoff[(size_t)i] = at; fw_take(at, (size_t)(after[(size_t)i].nblk * k4::ce_slot(enc[i]))); }
    const size_t o_stin = fw_take(at, (size_t)nfast * sizeof(k4lz4_fast_chain_state)),
                 o_stout = fw_take(at, (size_t)nfast * sizeof(k4lz4_fast_chain_state));
    const size_t total_bytes = at + 64;

    K4_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = plan_begin(ctx, plan, plan_bytes + 64, true)) != K4LZ4_OK) return rc;
    if ((rc = grow_scratch(ctx, &plan.dev, &plan.cap, total_bytes)) != K4LZ4_OK) return rc;
    uint8_t *h = plan.host.data(), *d = plan.dev;
    k4::CeStream *hs = (k4::CeStream *)(h + o_streams);
    k4::CeRec *hr = (k4::CeRec *)(h + o_recs);
    k4::CeBlock *hb = (k4::CeBlock *)(h + o_blocks);
    uint64_t *hslot = (uint64_t *)(h + o_slot), *hisrc = (uint64_t *)(h + o_isrc);
    int32_t *hilen = (int32_t *)(h + o_ilen), *hicap = (int32_t *)(h + o_icap);
    k4lz4_fast_chain_state *d_stin = (k4lz4_fast_chain_state *)(d + o_stin), *d_stout = (k4lz4_fast_chain_state *)(d + o_stout);

    std::vector<int64_t> first((size_t)n, 0), fast_index((size_t)n, -1);
    int64_t kfast = 0;
    for (const Group &g : groups) {
        int64_t b = g.first;
        for (int64_t i : g.streams) { first[(size_t)i] = b; b += after[(size_t)i].nblk; if (enc[i].kind == 2) fast_index[(size_t)i] = kfast++; }
    }
    for (int64_t i = 0; i < n; i++) {
        k4::CeStream &row = hs[i];
        row.code = code[(size_t)i]; row.nRec = nRec[i]; row.firstRec = nRec[i] ? firstRec[i] : 0;
        if (row.code != 0) continue;
        const k4lz4_chain_encoder &e = enc[i];
        const k4::CeAfter &a = after[(size_t)i];
        row.out = dstOff[i]; row.cap = dstCap[i]; row.firstBlk = (unsigned long long)first[(size_t)i];
        uint8_t *sto = store + storeOff[i], *ring = sto + k4::ce_ring_at(e);
        const bool runs = a.nblk > 0;
        uint8_t *wp = d + win[(size_t)i];
        const int64_t slot = k4::ce_slot(e);
        const uint64_t *ro = recOff + firstRec[i];
        k4::CeRec *rr = hr + firstRec[i];
        int64_t j = 0;
        if (runs) stage.push_back(k4::FwPiece{wp, ring, (unsigned long long)e.pointer, 0});
        k4::ce_model(e, recLen + firstRec[i], recFlags + firstRec[i], nRec[i],
            [&](int64_t r, int64_t loaded, int64_t where) {
                rr[r].loaded = (int32_t)loaded; rr[r].blk = -1; rr[r].allow = (recFlags[firstRec[i] + r] & K4LZ4_CENC_ALLOW_COPY) ? 1u : 0u;
                /* a stream that encodes nothing this run appends straight to its ring (ws stays 0: `where` is the ring's position) */
                if (loaded) stage.push_back(k4::FwPiece{(runs ? wp : ring) + where, src + ro[r], (unsigned long long)loaded, 0});
            },
            [&](int64_t r, int64_t start, int64_t len, int64_t, int64_t, bool) {
                const int64_t b = first[(size_t)i] + j;
                rr[r].blk = (int32_t)j;
                hb[b].slot = aoff[(size_t)i] + (uint64_t)(j * slot); hb[b].raw = win[(size_t)i] + (uint64_t)start; hb[b].len = (int32_t)len;
                hslot[b] = hb[b].slot; hisrc[b] = hb[b].raw; hilen[b] = (int32_t)len; hicap[b] = (int32_t)slot;
                j++;
            });
        if (!runs) continue;
        const int64_t r0 = a.ws == 0 ? e.pointer : 0;                    /* bytes of the ring that stay where they are */
        back.push_back(k4::FwPiece{ring + r0, wp + a.ws + r0, (unsigned long long)(a.pointer - r0), 0});
        if (e.kind == 2) {
            const int64_t f = fast_index[(size_t)i];
            /* a stream that has encoded nothing yet starts from a zeroed LZ4_stream_t (LZ4FastChainEncoder.cs) */
            stage.push_back(k4::FwPiece{(uint8_t *)(d_stin + f), e.currentOffset ? (const uint8_t *)sto : nullptr, sizeof(k4lz4_fast_chain_state), 0});
            back.push_back(k4::FwPiece{sto, (const uint8_t *)(d_stout + f), sizeof(k4lz4_fast_chain_state), 0});
        }
    }
    if (stage.size() > npiece_max || back.size() > 2 * (size_t)n) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: internal: piece table overflow");
    const unsigned long long stage_chunks = fw_chunks(stage.data(), stage.size()), back_chunks = fw_chunks(back.data(), back.size());
    if (!stage.empty()) memcpy(h + o_stage, stage.data(), stage.size() * sizeof(k4::FwPiece));
    if (!back.empty()) memcpy(h + o_back, back.data(), back.size() * sizeof(k4::FwPiece));

    /* ---- enqueue: plan up, stage, encode, write back, place */
    if ((rc = plan_send(ctx, plan, d, plan_bytes, st)) != K4LZ4_OK) return rc;
    int32_t *d_out = (int32_t *)(d + o_out);
    if (!stage.empty())
        hipLaunchKernelGGL(k4::k4_fw_copy_kernel, dim3((unsigned)stage_chunks), dim3(k4::FW_THREADS), 0, st, (const k4::FwPiece *)(d + o_stage), (long long)stage.size());
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    for (const Group &g : groups) {
        const int kind = g.key / 100, level = g.key % 100;
        const int64_t ns = (int64_t)g.streams.size();
        if (kind == 0) {
            rc = launch(ctx, KIND_ENCODE, d, (const uint64_t *)(d + o_isrc) + g.first, (const int32_t *)(d + o_ilen) + g.first, d,
                        (const uint64_t *)(d + o_slot) + g.first, (const int32_t *)(d + o_icap) + g.first, d_out + g.first, g.nb, level,
                        x32 ? K4LZ4_FLAG_X32 : 0, st, nullptr, hilen + g.first);
        } else {
            std::vector<uint64_t> soff((size_t)ns), doff((size_t)ns);
            std::vector<int64_t> slen((size_t)ns), lfirst((size_t)ns);
            std::vector<int32_t> bsz((size_t)ns), ext((size_t)ns), dlen((size_t)ns), lcount((size_t)ns);
            std::vector<uint32_t> cur0((size_t)ns), sdict((size_t)ns);
            int64_t f0 = -1;
            for (int64_t k = 0; k < ns; k++) {
                const int64_t i = g.streams[(size_t)k];
                soff[(size_t)k] = win[(size_t)i]; doff[(size_t)k] = aoff[(size_t)i];
                lfirst[(size_t)k] = first[(size_t)i] - g.first; lcount[(size_t)k] = (int32_t)after[(size_t)i].nblk;
                int64_t total = enc[i].index;
                for (int64_t j = 0; j < after[(size_t)i].nblk; j++) total += hilen[first[(size_t)i] + j];
                slen[(size_t)k] = total;
                bsz[(size_t)k] = enc[i].blockSize; ext[(size_t)k] = enc[i].extraBlocks; dlen[(size_t)k] = enc[i].index;
                cur0[(size_t)k] = enc[i].currentOffset; sdict[(size_t)k] = enc[i].dictSize;
                if (f0 < 0) f0 = fast_index[(size_t)i];
            }
            const ChainLens lens{lfirst.data(), lcount.data(), hilen + g.first};
            /* allowCopy is a record's switch here: the encoders keep every block encoded and k4_ce_place_kernel applies the rule */
            if (kind == 1)
                rc = hc_chain_run(ctx, d, soff.data(), slen.data(), bsz.data(), ext.data(), dlen.data(), ns, d, doff.data(), d_out + g.first, g.nb,
                                  level, 0, st, &lens);
            else
                rc = fast_chain_run(ctx, d, soff.data(), slen.data(), bsz.data(), ext.data(), dlen.data(), cur0.data(), sdict.data(), ns,
                                    d_stin + f0, d_stout + f0, d, doff.data(), d_out + g.first, g.nb, 0, st, &lens);
        }
        if (rc != K4LZ4_OK) return rc;
    }
    if (!back.empty())
        hipLaunchKernelGGL(k4::k4_fw_copy_kernel, dim3((unsigned)back_chunks), dim3(k4::FW_THREADS), 0, st, (const k4::FwPiece *)(d + o_back), (long long)back.size());
    hipLaunchKernelGGL(k4::k4_ce_place_kernel, dim3((unsigned)n), dim3(k4::CE_WAVE), 0, st, (const k4::CeStream *)(d + o_streams),
                       (const k4::CeRec *)(d + o_recs), (const k4::CeBlock *)(d + o_blocks), (const int32_t *)d_out, (const uint8_t *)d, dst,
                       recLoaded, recOut, (long long *)outLen, (long long)n);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);

    /* ---- the records: what the calls enqueued leaves them in */
    for (int64_t i = 0; i < n; i++)
        if (code[(size_t)i] == 0) k4::ce_advance(enc[i], after[(size_t)i]);
    return K4LZ4_OK;
}

int k4lz4_chain_encode_batch(k4lz4_ctx *ctx, k4lz4_chain_encoder *enc, uint8_t *store, const uint64_t *storeOff, const uint8_t *src,
                             const uint64_t *recOff, const uint32_t *recLen, const uint32_t *recFlags, int64_t nRecords,
                             const uint64_t *firstRec, const uint32_t *nRec, uint8_t *dst, const uint64_t *dstOff, const uint64_t *dstCap,
                             int32_t *recLoaded, int32_t *recOut, int64_t *outLen, int64_t n, int op, int flags)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (op == K4LZ4_CENC_RESET || n <= 0) {
        const int rc0 = k4lz4_chain_encode_batch_device(ctx, enc, store, storeOff, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                                        nullptr, nullptr, nullptr, nullptr, nullptr, n, op, flags, ctx->stream);
        if (rc0 == K4LZ4_OK && n > 0) K4_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return rc0;
    }
    if (nRecords < 0 || !enc || !firstRec || !nRec || !dstOff || !dstCap || !outLen || !dst ||
        (nRecords > 0 && (!recOff || !recLen || !recFlags || !recLoaded || !recOut)))
        return fail(ctx, K4LZ4_E_ARG, "bad argument");
    std::vector<int64_t> len64((size_t)nRecords);
    for (int64_t r = 0; r < nRecords; r++) {
        if (recLen[r] > 0x7fffffffu) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: a record longer than INT32_MAX");
        if (recLen[r] && !src) return fail(ctx, K4LZ4_E_ARG, "bad argument");
        len64[(size_t)r] = recLen[r];
    }
    /* the output slots: what the run can emit, not the caller's capacities (the codes are decided on dstCap all the same) */
    std::vector<uint64_t> cap((size_t)n, 0);
    for (int64_t i = 0; i < n; i++) {
        if (nRec[i] == 0) continue;
        if (firstRec[i] > (uint64_t)nRecords || (uint64_t)nRec[i] > (uint64_t)nRecords - firstRec[i])
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_encode_batch: a stream refers to records outside the record table");
        cap[(size_t)i] = std::min<uint64_t>(dstCap[i], (uint64_t)k4lz4_chain_encode_bound(enc + i, recLen + firstRec[i], recFlags + firstRec[i], nRec[i]));
    }
    K4_HIP(ctx, hipSetDevice(ctx->device));
    HostStage s(ctx);
    s.pack(src, recOff, len64.data(), nRecords);
    s.slots(n, [&](int64_t i) { return cap[(size_t)i]; }, false);
    int64_t *d_out;
    int32_t *d_loaded, *d_rout;
    s.meta(&d_out, n); s.meta(&d_loaded, std::max<int64_t>(nRecords, 1)); s.meta(&d_rout, std::max<int64_t>(nRecords, 1));
    std::vector<int32_t> h_loaded((size_t)std::max<int64_t>(nRecords, 1)), h_rout((size_t)std::max<int64_t>(nRecords, 1));
    int rc;
    if ((rc = s.upload()) != K4LZ4_OK ||
        (rc = k4lz4_chain_encode_batch_device(ctx, enc, store, storeOff, ctx->d_src, s.in_off.data(), recLen, recFlags, nRecords, firstRec, nRec,
                                              ctx->d_dst, s.slot.data(), cap.data(), d_loaded, d_rout, d_out, n, op, flags, s.st)) != K4LZ4_OK)
        return rc;
    rc = s.finish({{outLen, d_out, (size_t)n * 8}, {h_loaded.data(), d_loaded, (size_t)nRecords * 4}, {h_rout.data(), d_rout, (size_t)nRecords * 4}},
                  dst, dstOff, [&](int64_t i) { return outLen[i] > 0 ? (size_t)outLen[i] : 0; });
    if (rc != K4LZ4_OK) return rc;
    for (int64_t i = 0; i < n; i++)
        for (uint32_t r = 0; r < nRec[i]; r++) { recLoaded[firstRec[i] + r] = h_loaded[(size_t)(firstRec[i] + r)]; recOut[firstRec[i] + r] = h_rout[(size_t)(firstRec[i] + r)]; }
    return K4LZ4_OK;
}

/* ---- chained encoders and decoders opened from a dictionary set (k4lz4_chain_open.hpp) --------------------- */
/* the record of a fresh stream (what RESET leaves), then LZ4_loadDict's / LZ4_loadDictHC's effect on it for dictLen bytes (< 0: none) */
static void ce_open_record(k4lz4_chain_encoder &e, int32_t dictLen)
{
    e.index = e.pointer = 0; e.currentOffset = e.dictSize = 0; e.taken = e.blocks = 0;
    if (dictLen < 0 || e.kind == 0) return;
    const int32_t d = std::min<int32_t>(dictLen, 65536);
    if (e.kind == 2) {
        e.currentOffset = k4::OPEN_CURRENT_OFFSET;           /* whatever the length: LZ4_resetStream, currentOffset += 64 KB */
        if (d < (int32_t)FAMILY_FAST.min_kept) return;       /* below HASH_UNIT nothing is loaded: the ring stays empty too */
        e.dictSize = (uint32_t)d;
    }
    e.index = e.pointer = d;
}

/* the optimal parser's levels are not opened from a dictionary: the case list's forced 12-byte block left the witness there (the
 * parser searches a block of exactly MFLIMIT bytes once, LL64.high.cs:823-837; the kernels search none below MFLIMIT + 1), and a
 * level without a witness is not shipped */
static bool ce_open_no_witness(const k4lz4_chain_encoder &e) { return e.kind == 1 && e.level >= K4LZ4_L10_OPT; }
static const char *const CE_OPEN_NO_OPT = ": levels from K4LZ4_L10_OPT on are not opened from a dictionary (L03_HC .. L09_HC and the fast chain are)";

int k4lz4_chain_encoder_open_plan(k4lz4_chain_encoder *e, int32_t dictLen)
{
    if (!e || !ce_record_ok(*e)) return fail(nullptr, K4LZ4_E_ARG, "k4lz4_chain_encoder_open_plan: not a record of k4lz4_chain_encoder_init");
    if (e->kind == 0 && dictLen >= 0)
        return fail(nullptr, K4LZ4_E_ARG, "k4lz4_chain_encoder_open_plan: an independent encoder (LZ4BlockEncoder) has no dictionary");
    if (ce_open_no_witness(*e) && dictLen >= 0) return fail(nullptr, K4LZ4_E_ARG, std::string("k4lz4_chain_encoder_open_plan") + CE_OPEN_NO_OPT);
    ce_open_record(*e, dictLen);
    return K4LZ4_OK;
}

int k4lz4_chain_encoder_open_dictset_device(k4lz4_ctx *ctx, k4lz4_chain_encoder *enc, uint8_t *store, const uint64_t *storeOff,
                                            const int32_t *dictIdx, const k4lz4_dict_set *set, int64_t n, void *stream)
{
    const char *who = "k4lz4_chain_encoder_open_dictset";
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || n > 0x7fffffffll || (n > 0 && (!enc || !store || !storeOff || !dictIdx || !set))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n == 0) return K4LZ4_OK;
    if (set->device != ctx->device) return fail(ctx, K4LZ4_E_ARG, std::string(who) + ": the set lives on another device than the context");
    if ((uintptr_t)store & 255u) return fail(ctx, K4LZ4_E_ARG, std::string(who) + ": the store is not 256-byte aligned");
    const bool x32 = g_enforce32.load(std::memory_order_relaxed) != 0;
    for (int64_t i = 0; i < n; i++) {
        if (storeOff[i] & 255u) return fail(ctx, K4LZ4_E_ARG, std::string(who) + ": a stream's store is not 256-byte aligned");
        if (!ce_record_ok(enc[i])) return fail(ctx, K4LZ4_E_ARG, std::string(who) + ": a record was not made by k4lz4_chain_encoder_init");
        const int32_t di = dictIdx[i];
        if (di < -1 || di >= set->nDict) return fail(ctx, K4LZ4_E_ARG, std::string(who) + ": a dictIdx outside the set");
        if (di < 0) continue;
        if (enc[i].kind == 0) return fail(ctx, K4LZ4_E_ARG, std::string(who) + ": an independent encoder (LZ4BlockEncoder) has no dictionary");
        if (ce_open_no_witness(enc[i])) return fail(ctx, K4LZ4_E_ARG, std::string(who) + CE_OPEN_NO_OPT);
        if (enc[i].kind == 2 && !set->fast.on)
            return fail(ctx, K4LZ4_E_ARG, std::string(who) + ": a chained fast encoder needs a set created with K4LZ4_DICT_FAST");
        if (enc[i].kind == 2 && x32)
            return fail(ctx, K4LZ4_E_ARG, std::string(who) + ": the 32-bit engine's chained encoder (LZ4Codec.Enforce32) is not supported");
    }
    /* ---- the plan: host arithmetic, nothing enqueued yet */
    std::vector<k4::CeOpenStream> rows((size_t)n);
    std::vector<k4lz4_chain_encoder> after(enc, enc + n);
    for (int64_t i = 0; i < n; i++) {
        const int32_t di = dictIdx[i];
        k4lz4_chain_encoder &e = after[(size_t)i];
        ce_open_record(e, di >= 0 ? set->keptLen[(size_t)di] : -1);
        k4::CeOpenStream &r = rows[(size_t)i];
        r = k4::CeOpenStream{};
        r.ring = storeOff[i] + (uint64_t)k4::ce_ring_at(e);
        r.keptLen = (uint32_t)e.pointer;                     /* what the ring holds in front of the first block */
        if (r.keptLen) r.kept = set->keptAt[(size_t)di];
        if (e.kind != 2) continue;
        r.state = storeOff[i];
        r.fast = e.dictSize ? 1u : 2u;
        if (e.dictSize) r.table = (uint64_t)(set->fast.tables - set->buf) + (uint64_t)FAMILY_FAST.table_bytes * set->fast.table[(size_t)di];
        r.currentOffset = e.currentOffset; r.dictSize = e.dictSize;
    }
    const size_t bytes = rows.size() * sizeof(k4::CeOpenStream);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    PlanUpload &plan = ctx->fw_plan;      /* the writers' */
    if ((rc = plan_begin(ctx, plan, bytes + 64, true)) != K4LZ4_OK) return rc;
    if ((rc = grow_scratch(ctx, &plan.dev, &plan.cap, bytes + 64)) != K4LZ4_OK) return rc;
    memcpy(plan.host.data(), rows.data(), bytes);
    if ((rc = plan_send(ctx, plan, plan.dev, bytes, st)) != K4LZ4_OK) return rc;
    hipLaunchKernelGGL(k4::k4_ce_open_kernel, dim3((unsigned)n), dim3(k4::OPEN_WAVE), 0, st, (const k4::CeOpenStream *)plan.dev, store,
                       (const uint8_t *)set->buf, (long long)n);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    std::copy(after.begin(), after.end(), enc);
    return K4LZ4_OK;
}

int k4lz4_chain_encoder_open_dictset(k4lz4_ctx *ctx, k4lz4_chain_encoder *enc, uint8_t *store, const uint64_t *storeOff, const int32_t *dictIdx,
                                     const k4lz4_dict_set *set, int64_t n)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    const int rc = k4lz4_chain_encoder_open_dictset_device(ctx, enc, store, storeOff, dictIdx, set, n, ctx->stream);
    if (rc == K4LZ4_OK && n > 0) K4_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return rc;
}

static int cdec_open_args(k4lz4_ctx *ctx, const void *dec, const void *store, const void *storeOff, const void *dictIdx, const k4lz4_dict_set *set,
                          const void *outLen, int64_t n)
{
    if (!ctx) return fail(nullptr, K4LZ4_E_ARG, "ctx is NULL");
    if (n < 0 || n > 0x7fffffffll || (n > 0 && (!dec || !store || !storeOff || !dictIdx || !set || !outLen))) return fail(ctx, K4LZ4_E_ARG, "bad argument");
    if (n > 0 && set->device != ctx->device)
        return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decoder_open_dictset: the set lives on another device than the context");
    if (n > 0 && ((uintptr_t)store & 255u)) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decoder_open_dictset: the store is not 256-byte aligned");
    return K4LZ4_OK;
}

int k4lz4_chain_decoder_open_dictset_device(k4lz4_ctx *ctx, const k4lz4_chain_decoder *dec, uint8_t *store, const uint64_t *storeOff,
                                            const int32_t *dictIdx, const k4lz4_dict_set *set, int64_t *outLen, int64_t n, void *stream)
{
    const int rc = cdec_open_args(ctx, dec, store, storeOff, dictIdx, set, outLen, n);
    if (rc != K4LZ4_OK || n == 0) return rc;
    K4_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    K4_HIP(ctx, order_after_ctx(ctx, st));
    const k4::CdOpenArgs a{(const k4::CdRecord *)dec, store, storeOff, dictIdx, set->buf, set->dec_off, set->dec_len, outLen, ctx->d_status,
                           (long long)n, set->nDict};
    hipLaunchKernelGGL(k4::k4_cdec_open_kernel, dim3((unsigned)n), dim3(k4::OPEN_WAVE), 0, st, a);
    K4_HIP(ctx, hipGetLastError());
    mark_busy(ctx, st);
    return K4LZ4_OK;
}

int k4lz4_chain_decoder_open_dictset(k4lz4_ctx *ctx, const k4lz4_chain_decoder *dec, uint8_t *store, const uint64_t *storeOff,
                                     const int32_t *dictIdx, const k4lz4_dict_set *set, int64_t *outLen, int64_t n)
{
    int rc = cdec_open_args(ctx, dec, store, storeOff, dictIdx, set, outLen, n);
    if (rc != K4LZ4_OK || n == 0) return rc;
    for (int64_t i = 0; i < n; i++) {
        if (storeOff[i] & 255u) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decoder_open_dictset: a stream's store is not 256-byte aligned");
        if (dec[i].blockSize != k4::cd_block_size(dec[i].blockSize) || dec[i].extraBlocks < 0 || (dec[i].chaining & ~1) ||
            dec[i].storeBytes != k4::cd_store_bytes(dec[i].blockSize, dec[i].extraBlocks, dec[i].chaining != 0))
            return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decoder_open_dictset: a record was not made by k4lz4_chain_decoder_init");
        if (dictIdx[i] < -1 || dictIdx[i] >= set->nDict) return fail(ctx, K4LZ4_E_ARG, "k4lz4_chain_decoder_open_dictset: a dictIdx outside the set");
    }
    K4_HIP(ctx, hipSetDevice(ctx->device));
    HostStage s(ctx);
    k4lz4_chain_decoder *d_dec;
    uint64_t *d_store;
    int32_t *d_idx;
    int64_t *d_out;
    s.meta(&d_dec, n, dec); s.meta(&d_store, n, storeOff); s.meta(&d_idx, n, dictIdx); s.meta(&d_out, n);
    if ((rc = s.upload()) != K4LZ4_OK ||
        (rc = k4lz4_chain_decoder_open_dictset_device(ctx, d_dec, store, d_store, d_idx, set, d_out, n, s.st)) != K4LZ4_OK)
        return rc;
    return s.finish({{outLen, d_out, (size_t)n * 8}});
}

}  // extern "C"
