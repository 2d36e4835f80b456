/* The batch launcher: which kernels a batch of blocks gets, and their launches.  A part of k4lz4_capi.hip -- included there, inside
 * its unnamed namespace, behind the helpers the launchers share (grow_after, envelope_prep / envelope_finish, DictArgs) -- and of
 * no other file.
 *
 *   launch_inner          the dispatcher
 *   launch_hc             the HC levels: hc_chunk() decides once per launch chunk which kernels run, launch_hc sizes the scratch and launches them
 *   launch_envelope       fast-level pickles and wraps the encoders' way: prep, launch_fast_encode on the slots, finish
 *   launch_fast_encode    LZ4Codec.Encode below level 3: fast_route() decides once per call and fast_chunk() once per launch chunk
 *                         which kernels run; order_prelude, segment_plan, two_step_chunk and one_kernel_chunk launch what they say
 *   launch_decode_like    decode, unpickle and the small-batch pickle kernel */
#pragma once

constexpr int64_t LAUNCH_CHUNK_MAX = 1 << 24;   /* blocks per launch (grid.x * blockDim.x must stay < 2^32) */

/* blocks first .. first + cnt of a call's batch */
k4::BatchArgs slice(k4::BatchArgs b, int64_t first, int64_t cnt)
{
    b.srcOff += first; b.srcLen += first; b.dstOff += first; b.dstCap += first; b.outLen += first; b.n = cnt;
    return b;
}

/* K4LZ4_FLAG_ALLOW_COPY: blocks that did not shrink are stored raw, behind whatever encoded them */
void allow_copy(k4lz4_ctx *ctx, k4::BatchArgs a, hipStream_t stream)
{
    ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_ALLOW_COPY;
    K4_LAUNCH_WAVES(k4::k4_allow_copy_kernel, a.n, 4, stream, a);
}

/* cost-ordered dispatch (most expensive blocks first): its grow-only scratch, laid out for launch chunks of up to cnt_max blocks */
struct Sched {
    uint32_t *hist, *cost, *order;
};

int sched_scratch(k4lz4_ctx *ctx, hipStream_t stream, size_t cnt_max, Sched *s)
{
    const size_t hist_words = std::max<size_t>(2 * (size_t)k4::PCOST_BUCKETS, 2 * (size_t)k4::COST_BUCKETS + 16);
    const int rc = grow_after(ctx, stream, &ctx->d_sched, &ctx->d_sched_cap, cnt_max * 8 + hist_words * 4 + 64);
    if (rc != K4LZ4_OK) return rc;
    s->hist = (uint32_t *)ctx->d_sched;
    s->cost = s->hist + hist_words;     /* [2 * COST_BUCKETS]: where the second encoder kernel's part of the order begins */
    s->order = s->cost + cnt_max;
    return K4LZ4_OK;
}

/* how many slots the LDS-table encoder kernel is launched with for a batch of cnt blocks: a fixed share of the number
 * (K4LZ4_SPLIT_PCT), or the most the device-side split by cost (k4_order_kernel, cost_pct hundredths of the cost, at least one
 * residency) can ask for -- that kernel clamps its count to this value, so a block is never left to neither kernel */
int64_t lds_share(const k4lz4_ctx *ctx, int64_t cnt)
{
    const int64_t lds_slots = 8 * (int64_t)ctx->cu_count;
    if (ctx->split_pct > 0) return std::min<int64_t>(cnt, std::max<int64_t>(1, cnt * ctx->split_pct / 100));
    const int64_t pct = std::max<int64_t>(48, std::min<int64_t>(ctx->cost_pct, 100));
    return std::min<int64_t>(cnt, std::max<int64_t>(lds_slots, (cnt * pct + 99) / 100));
}

/* The blocks' costs and their dispatch order, into a.cost / a.hist / a.order (and a.split).  Two forms:
 * pcost -- the two-kernel encoder's own estimate and order (k4lz4_parse.hpp, ParseCost): one workgroup of sixteen waves per CU at
 *   most, every wave's table in LDS; the order's workgroups each place a stretch of the batch (k4_order_kernel);
 * else -- by the one-kernel encoder's sequence count over `sample` bytes, or by length (decoders); two_kernels: k4_order_kernel
 *   also splits the order between the two encoder kernels by cost: 48 % of it, at least one residency of the LDS-table kernel
 *   (K4LZ4_SPLIT_PCT fixes a share of the NUMBER of blocks instead) */
int order_prelude(k4lz4_ctx *ctx, hipStream_t stream, k4::BatchArgs &a, const Sched &s, bool pcost, int by_length, int sample, bool two_kernels)
{
    const int64_t cnt = a.n;
    a.cost = s.cost; a.hist = s.hist; a.order_out = s.order;
    if (pcost) {
        const int64_t wgs = std::min<int64_t>((cnt + k4::PARSE_MAX_WAVES - 1) / k4::PARSE_MAX_WAVES, ctx->cu_count);
        K4_HIP(ctx, hipMemsetAsync(s.hist, 0, k4::PCOST_BUCKETS * 4, stream));
        hipLaunchKernelGGL(static_cast<void (*)(k4::BatchArgs, k4::ParseCost)>(k4::k4_cost_kernel), dim3((unsigned)wgs), dim3(64 * k4::PARSE_MAX_WAVES), 0, stream, a, ctx->pcost_fit);
        hipLaunchKernelGGL(k4::k4_order_kernel, dim3(k4::order_workgroups(cnt)), dim3(256), 0, stream, a, 0xffffffffu, 1);
    } else {
        K4_HIP(ctx, hipMemsetAsync(s.hist, 0, (2 * k4::COST_BUCKETS + 16) * 4, stream));
        K4_LAUNCH_WAVES(k4::k4_cost_kernel, cnt, 1, stream, a, by_length, sample);
        k4::BatchArgs ao = a;
        ao.first = two_kernels ? (uint32_t)ctx->cost_pct : 0u;
        ao.total = (uint32_t)((int64_t)ctx->lds_floor_per_cu * (int64_t)ctx->cu_count);
        hipLaunchKernelGGL(k4::k4_order_kernel, dim3(k4::order_workgroups(cnt)), dim3(256), 0, stream, ao, (uint32_t)lds_share(ctx, cnt));
        if (two_kernels) a.split = s.hist + 2 * k4::COST_BUCKETS;
    }
    a.order = s.order;
    return K4LZ4_OK;
}

/* ---- fast encode: the route ---- */

/* what is decided once per call */
struct FastRoute {
    bool prof;            /* k4lz4_profile_batch_device: counters or stamps per block */
    bool prof_twin;       /* ... by the instrumented one-kernel encoder */
    bool split_ok;        /* the batch may be split between two kernels (no K4LZ4_FLAG_NO_SPLIT) */
    bool allow_copy;      /* K4LZ4_FLAG_ALLOW_COPY */
    bool two_step;        /* the two-kernel encoder (k4lz4_parse.hpp) on a batch of whole blocks */
    bool two_step_seg;    /* ... on a batch that may be ragged */
    bool persistent;      /* ... in one launch for a batch beyond one residency */
    int64_t chunk_max;    /* blocks per launch chunk */
    bool reorder;         /* cost-ordered dispatch */
    bool pcost_order;     /* ... by the parse's own estimate (order_prelude) */
    int cost_sample;      /* ... else over this many bytes */
    bool segments;        /* big blocks are cut into segments (k4lz4_segments.hpp) */
};

FastRoute fast_route(const k4lz4_ctx *ctx, int flags, int64_t n)
{
#ifdef K4_PARSE_PROF
    const bool parse_prof_ok = true;
#else
    const bool parse_prof_ok = false;
#endif
    /* what is resident at once: 16 blocks per CU (the parse kernel's one workgroup per CU, nine waves with their table in LDS and
     * seven that move into a table as one becomes free) */
    const int64_t residency = (int64_t)k4::PARSE_MAX_WAVES * (int64_t)ctx->cu_count;
    const bool ragged = (flags & (FLAG_SEGMENTS_OK | K4LZ4_FLAG_SEGMENTS)) != 0;      /* pickles, K4LZ4_FLAG_SEGMENTS */
    FastRoute r{};
    r.prof = ctx->prof != nullptr;
    r.prof_twin = r.prof && !ctx->prof_stamp;
    r.split_ok = !(flags & K4LZ4_FLAG_NO_SPLIT);
    r.allow_copy = (flags & K4LZ4_FLAG_ALLOW_COPY) != 0;
    /* LZ4Codec.Encode's case -- acceleration 1, no segments -- goes through the two-kernel encoder (k4lz4_parse.hpp): which
     * sequences (one wavefront per block, 64 x K positions per round, 16 blocks per workgroup = per CU dealt from the cost
     * order, the nine most expensive of a workgroup with their table in LDS), then their bytes (a throughput kernel), then
     * whatever block the parse left alone (65 547 bytes and more, very short ones) by the one-kernel encoder. */
    r.two_step = ctx->use_parse && ctx->accel == 1 && (!r.prof || parse_prof_ok || ctx->prof_stamp) && !ragged && r.split_ok;
    /* round 6: ragged batches -- pickles, K4LZ4_FLAG_SEGMENTS -- through the two-step encoder as well: the blocks below 65 547 bytes by
     * k4_parse_kernel, the others (and the later segments of the cut ones) by k4_parse_seg_kernel, the join as before */
    r.two_step_seg = ctx->use_parse && ctx->parse_big && ctx->parse_seg && ctx->parse_inline_emit && ctx->accel == 1 && !r.prof && ragged &&
                     r.split_ok && !(flags & (K4LZ4_FLAG_NO_REORDER | K4LZ4_FLAG_ALLOW_COPY));
    /* round 6: the two-step encoder takes a batch beyond one residency in ONE persistent launch -- one workgroup of sixteen waves per
     * CU, every wave takes the next block of the cost order when it is done with one (the waves with LDS tables from the expensive
     * end, the others from the cheap end), records in per-wave slots -- instead of launches of one residency each with their own tail */
    r.persistent = r.two_step && ctx->parse_persist && ctx->parse_inline_emit && !r.prof && n > residency && !(flags & K4LZ4_FLAG_NO_REORDER);
    /* Batches beyond one residency otherwise -- with K4LZ4_NO_PERSIST, or through the one-kernel encoders of rounds 1-4 --: equal
     * parts of at most one residency each; a block takes its ~2-3 ms whatever the batch, so those launches are best full.  Not for
     * batches that may be ragged: those need their one cost-ordered launch. */
    r.chunk_max = LAUNCH_CHUNK_MAX;
    if (!ragged && r.split_ok && ctx->split_pct <= 0 && !r.prof && n > residency && !r.persistent) {
        const int64_t parts = (n + residency - 1) / residency;
        r.chunk_max = (n + parts - 1) / parts;
    }
    if (r.two_step && !r.persistent) r.chunk_max = std::min(r.chunk_max, residency);
    /* cost-ordered dispatch (most expensive blocks first): encoders by default */
    r.reorder = n > 1 && !(flags & K4LZ4_FLAG_NO_REORDER);
    r.pcost_order = r.reorder && r.two_step && ctx->parse_pcost;
    r.cost_sample = r.two_step ? k4::COST_SAMPLE_PARSE : k4::COST_SAMPLE;
    /* big blocks in several segments (k4lz4_segments.hpp): the plan is made on the device, the later segments run on a queue of
     * their own beside the ordinary kernels (which take a cut block's first segment), the pieces are joined afterwards */
    r.segments = ragged && ctx->use_segments && !r.prof && !r.allow_copy;
    return r;
}

/* what is decided per launch chunk of cnt blocks; hostLen: the chunk's lengths where the host knows them, else nullptr */
struct FastChunk {
    bool pace;                      /* the one-kernel encoders' late-blocks-first priorities (k4lz4_common.hpp, Pace) */
    size_t seg_items;               /* segments: how many the plan can come to */
    bool two_kernels;               /* the order is split between the two one-kernel encoders by cost, on the device (a.split) */
    /* the two-step encoder */
    bool parse_here;                /* this chunk goes through it */
    bool any_small, any_big;        /* blocks for k4_parse_kernel, for k4_parse_big_kernel */
    bool seg_two_step;              /* k4_parse_seg_kernel behind the first launch */
    bool queue, slot_recs, parse_pace;
    bool rest;                      /* blocks the parse leaves alone: k4_encode_fast_rest_kernel */
    int64_t waves, nwg, nwg_seg;
    /* the one-kernel encoders */
    bool pair;                      /* LDS-table kernel and global-table kernel side by side */
    bool more;                      /* k4_encode_fast_more_kernel */
    int64_t n_lds, n_g;             /* the pair's launch sizes */
};

FastChunk fast_chunk(const k4lz4_ctx *ctx, const FastRoute &r, int64_t cnt, const int32_t *hostLen)
{
    const int64_t cu = ctx->cu_count;
    FastChunk c{};
    c.pace = !r.two_step && ctx->use_pace && ctx->d_pace && cnt > (int64_t)ctx->pace_min_per_cu * cu;   /* more than two blocks per SIMD */
    if (r.segments) {
        /* every item costs a 16 KiB snapshot and a 16 KiB table slot, so where the host knows the lengths the arrays are sized by
         * them (an upper bound: the plan's segments are never shorter than seg_target, its threshold never below seg_min) instead
         * of by the most a launch may have */
        c.seg_items = (size_t)k4::SEG_MAX_ITEMS;
        if (hostLen) {
            size_t bound = 0;
            for (int64_t i = 0; i < cnt && bound < c.seg_items; i++) {
                const int32_t u = hostLen[i];
                if (u > 0 && (uint32_t)u >= ctx->seg_min) bound += ((size_t)u + ctx->seg_target - 1) / ctx->seg_target;
            }
            c.seg_items = std::min(c.seg_items, std::max<size_t>(bound, 2));
        }
    }
    c.two_kernels = r.reorder && !r.pcost_order && !r.prof && r.split_ok && cnt > 512 && cnt > 8 * cu && ctx->split_pct <= 0;

    c.parse_here = r.two_step || (r.two_step_seg && (r.reorder || cnt == 1));
    /* blocks of 65 547 bytes and more (byU32 tables) go through k4_parse_big_kernel behind the first launch -- where the parsing
     * waves write their blocks out themselves (a big block has more sequences than a record slot holds) */
    const bool big_ok = ctx->parse_big && ctx->parse_inline_emit;
    c.any_small = true; c.any_big = big_ok;
    if (c.parse_here && hostLen) {             /* nothing for the parse kernels in this part (all blocks too short): no scratch, no launch */
        c.any_small = false; c.any_big = false;
        for (int64_t i = 0; i < cnt && !(c.any_small && (c.any_big || !big_ok)); i++) {
            if (hostLen[i] >= (int32_t)k4::PARSE_MIN_LEN && hostLen[i] < k4::LIMIT_64K) c.any_small = true;
            else if (hostLen[i] >= k4::LIMIT_64K && big_ok) c.any_big = true;
        }
        c.parse_here = c.any_small || c.any_big;
    }
    if (c.parse_here) {
        c.waves = std::max<int64_t>(1, std::min<int64_t>(ctx->parse_waves, (cnt + cu - 1) / cu));
        c.seg_two_step = r.segments && r.two_step_seg;
        /* K4LZ4_PARSE_QUEUE, and every batch beyond one residency: one workgroup per CU at most, every wave takes the next block of
         * the cost order when it is done with one */
        c.queue = (ctx->parse_queue || r.persistent || r.two_step_seg) && r.reorder && cnt > c.waves * cu;
        c.nwg = c.queue ? cu : (cnt + c.waves - 1) / c.waves;
        /* the segments' launch: always sixteen waves per workgroup, one workgroup per CU at most, everything from its queue */
        if (c.seg_two_step) c.nwg_seg = std::min<int64_t>(cu, (cnt + (int64_t)c.seg_items + k4::PARSE_MAX_WAVES - 1) / k4::PARSE_MAX_WAVES);
        /* records: a slot per wave of the launch where the parsing waves write their blocks out themselves, else one per block */
        c.slot_recs = ctx->parse_inline_emit;
        /* late blocks first among the waves of a SIMD (k4lz4_parse.hpp, ParsePace): its words are LDS of the workgroup, so
         * nothing is filled or launched for it; k4_parse_kernel alone reads the switch */
        c.parse_pace = r.two_step && ctx->use_pace && (!c.queue || ctx->parse_pace_queue) && cnt > (int64_t)ctx->parse_pace_min_per_cu * cu;
        c.rest = true;          /* (where the host knows the lengths it knows whether there is anything left) */
        if (hostLen) {
            c.rest = false;
            for (int64_t i = 0; i < cnt && !c.rest; i++) c.rest = hostLen[i] < (int32_t)k4::PARSE_MIN_LEN || (hostLen[i] >= k4::LIMIT_64K && !c.any_big);
        }
    }

    /* Only 8 blocks per CU fit with their hash table in LDS.  The most expensive blocks (front of the dispatch order) take those
     * slots; the others are encoded at the same time on a second queue by the global-memory-table variant of the kernel. */
    /* measured on MI355X (profiles/r02_split_sweep.txt): best when the LDS-table kernel gets one full residency of the chip
     * (8 blocks per CU) or about 48 % of a larger batch; one block more than a residency starts a second pass and costs 20 % */
    c.pair = r.reorder && cnt > 512 && r.split_ok;
    c.n_lds = lds_share(ctx, cnt);
    /* (with the split decided on the device: n_lds is the most the LDS-table kernel can get -- the share of the cost is never a
     * larger share of the number -- and the other kernel is sized for the least) */
    c.n_g = cnt - (c.two_kernels ? std::min<int64_t>(cnt, (int64_t)ctx->lds_floor_per_cu * cu) : c.n_lds);
    /* a half-empty chip: the variant that buys latency with instructions */
    c.more = cnt <= 8 * cu && (!c.pair || c.n_g == 0);
    return c;
}

/* ---- fast encode: the launches ---- */

/* big blocks in several segments: scratch for up to max_items of them, the plan (made on the device), a's pointers to it */
int segment_plan(k4lz4_ctx *ctx, hipStream_t stream, k4::BatchArgs &a, size_t max_items, k4::SegArgs *sg)
{
    static_assert(k4::SEG_HDR_DWORDS * 4 == 256, "seg_first_of finds the header in front of the items");
    const size_t o_items = 256, o_work = o_items + max_items * sizeof(k4::SegItem);
    const size_t o_blocks = o_work + max_items * 4, o_snaps = (o_blocks + (size_t)k4::SEG_MAX_BLOCKS * 4 + 255) & ~(size_t)255;
    const size_t o_tables = o_snaps + max_items * k4::SEG_SNAP_DWORDS * 4, total = o_tables + max_items * 16384;
    if (total > ctx->d_seg_cap || (size_t)a.n * 4 > ctx->d_seg_first_cap) {
        K4_HIP(ctx, hipStreamSynchronize(stream));
        K4_HIP(ctx, hipStreamSynchronize(ctx->aux2));
    }
    int rc = grow(ctx, &ctx->d_seg, &ctx->d_seg_cap, total, false);
    if (rc == K4LZ4_OK) rc = grow(ctx, &ctx->d_seg_first, &ctx->d_seg_first_cap, (size_t)a.n * 4, false);
    if (rc != K4LZ4_OK) return rc;
    sg->hdr = (k4::SegHdr *)ctx->d_seg; sg->items = (k4::SegItem *)(ctx->d_seg + o_items); sg->work = (uint32_t *)(ctx->d_seg + o_work);
    sg->blocks = (uint32_t *)(ctx->d_seg + o_blocks); sg->snaps = (uint32_t *)(ctx->d_seg + o_snaps); sg->tables = (uint32_t *)(ctx->d_seg + o_tables);
    sg->first = (int32_t *)ctx->d_seg_first;
    sg->seg_min = ctx->seg_min; sg->seg_target = ctx->seg_target; sg->seg_warm = ctx->seg_warm; sg->seg_div = ctx->seg_div; sg->seg_target_max = ctx->seg_target_max; sg->spin_max = ctx->seg_spin_max; sg->max_items = (uint32_t)max_items;
    hipLaunchKernelGGL(k4::k4_seg_plan_kernel, dim3(1), dim3(256), 0, stream, a, *sg);
    a.seg_first = sg->first; a.seg_items = sg->items; a.seg_snaps = sg->snaps;
    return K4LZ4_OK;
}

/* the later segments: on their queue, before the ordinary kernels are launched (their waves are the ones others wait for) */
int segments_start(k4lz4_ctx *ctx, hipStream_t stream, k4::BatchArgs a, k4::SegArgs sg)
{
    K4_HIP(ctx, hipEventRecord(ctx->ev_fork, stream));
    K4_HIP(ctx, hipStreamWaitEvent(ctx->aux2, ctx->ev_fork, 0));
    ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_SEGMENTS;
    K4_LAUNCH_WAVES(k4::k4_encode_seg_kernel, sg.max_items, k4::ENCODE_WAVES_PER_WG, ctx->aux2, a, sg);
    K4_HIP(ctx, hipEventRecord(ctx->ev_join2, ctx->aux2));
    return K4LZ4_OK;
}

/* the cut blocks' pieces: joined, or encoded again (k4lz4_segments.hpp) */
void segments_join_launch(hipStream_t stream, k4::BatchArgs a, k4::SegArgs sg)
{
    hipLaunchKernelGGL(k4::k4_seg_join_kernel, dim3((unsigned)std::min<int64_t>(k4::SEG_MAX_BLOCKS, a.n)), dim3(64), 0, stream, a, sg);
}

int segments_join(k4lz4_ctx *ctx, hipStream_t stream, k4::BatchArgs a, k4::SegArgs sg)
{
    K4_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_join2, 0));
    segments_join_launch(stream, a, sg);
    return K4LZ4_OK;
}

/* a chunk through the one-kernel encoders of rounds 1-4 */
int one_kernel_chunk(k4lz4_ctx *ctx, const FastRoute &r, const FastChunk &c, k4::BatchArgs a, k4::SegArgs sg, hipStream_t stream)
{
    const int64_t cnt = a.n;
    int rc;
    if (r.prof_twin) {
        if (ctx->prof_gtab) {    /* diagnostics: the instrumented encoder with its table in global memory, like the global-table kernel */
            if ((rc = grow_after(ctx, ctx->aux, &ctx->d_gtab, &ctx->d_gtab_cap, (size_t)cnt * 16384)) != K4LZ4_OK) return rc;
            a.gtab = (uint32_t *)ctx->d_gtab;
        }
        ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_PROF;
        K4_LAUNCH_WAVES(k4::k4_encode_fast_prof_kernel, cnt, 1, stream, a);
        return K4LZ4_OK;
    }
    const int64_t gchunk = 8192;
    if (c.pair && (rc = grow_after(ctx, ctx->aux, &ctx->d_gtab, &ctx->d_gtab_cap, (size_t)std::min(c.n_g, gchunk) * 16384)) != K4LZ4_OK) return rc;
    if (r.segments && (rc = segments_start(ctx, stream, a, sg)) != K4LZ4_OK) return rc;
    k4::BatchArgs al = a;
    if (c.pair) {
        if (c.n_g > 0) ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_GTAB | (r.segments ? K4LZ4_ENCODE_ROUTE_SEGMENTS : 0) | (c.two_kernels ? K4LZ4_ENCODE_ROUTE_TWO_KERNELS : 0);
        K4_HIP(ctx, hipEventRecord(ctx->ev_fork, stream));
        K4_HIP(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
        for (int64_t g0 = 0; g0 < c.n_g; g0 += gchunk) {
            k4::BatchArgs ag = a;
            ag.first = (uint32_t)((c.two_kernels ? 0 : c.n_lds) + g0);
            ag.total = (uint32_t)cnt;
            ag.gtab = (uint32_t *)ctx->d_gtab;
            ag.n = std::min(gchunk, c.n_g - g0);
            if (r.segments) K4_LAUNCH_WAVES(k4::k4_encode_fast_gtab_seg_kernel, ag.n, k4::ENCODE_WAVES_PER_WG, ctx->aux, ag);
            else K4_LAUNCH_WAVES(k4::k4_encode_fast_gtab_kernel, ag.n, k4::ENCODE_WAVES_PER_WG, ctx->aux, ag);
        }
        K4_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->aux));
        al.n = c.n_lds;
    }
    ctx->last_encode_route |= r.segments ? K4LZ4_ENCODE_ROUTE_LDS | K4LZ4_ENCODE_ROUTE_SEGMENTS : c.more ? K4LZ4_ENCODE_ROUTE_MORE : K4LZ4_ENCODE_ROUTE_LDS;
    if (r.segments) K4_LAUNCH_WAVES(k4::k4_encode_fast_seg_kernel, al.n, k4::ENCODE_WAVES_PER_WG, stream, al);
    else if (c.more) K4_LAUNCH_WAVES(k4::k4_encode_fast_more_kernel, al.n, k4::ENCODE_WAVES_PER_WG, stream, al);
    else K4_LAUNCH_WAVES(k4::k4_encode_fast_kernel, al.n, k4::ENCODE_WAVES_PER_WG, stream, al);
    if (c.pair) K4_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_join, 0));
    if (r.segments && (rc = segments_join(ctx, stream, a, sg)) != K4LZ4_OK) return rc;
    return K4LZ4_OK;
}

/* a chunk through the two-kernel encoder: which sequences (k4_parse_kernel, then k4_parse_seg_kernel or k4_parse_big_kernel for
 * what the first launch leaves them), their bytes, the blocks the parse left alone */
int two_step_chunk(k4lz4_ctx *ctx, const FastRoute &r, const FastChunk &c, k4::BatchArgs a, k4::SegArgs sg, hipStream_t stream)
{
    const int64_t cnt = a.n;
    const size_t rec_slots = c.slot_recs ? std::max((size_t)c.nwg * (size_t)c.waves, (size_t)c.nwg_seg * k4::PARSE_MAX_WAVES) : (size_t)cnt;
    const size_t o_meta = rec_slots * k4::PARSE_REC_STRIDE * sizeof(uint2), o_gtab = (o_meta + (size_t)cnt * 8 + 64 + 255) & ~(size_t)255;
    const size_t need = o_gtab + std::max(c.waves > k4::PARSE_LDS_TABLES ? (size_t)c.nwg * k4::PARSE_MAX_WAVES * 16384 : 0, (size_t)c.nwg_seg * k4::PARSE_MAX_WAVES * 16384);
    if (grow_after(ctx, stream, &ctx->d_parse, &ctx->d_parse_cap, need) != K4LZ4_OK) {
        /* (no room for the records: the one-kernel encoders need next to none -- the same bytes, a third slower) */
        { std::lock_guard<std::mutex> g(g_err_mu); ctx->error.clear(); }
        return one_kernel_chunk(ctx, r, c, a, sg, stream);
    }
    k4::ParseArgs pa{};
    pa.recs = (uint2 *)ctx->d_parse; pa.meta = (uint32_t *)(ctx->d_parse + o_meta); pa.gtab = (uint32_t *)(ctx->d_parse + o_gtab);
    pa.nwg = (uint32_t)c.nwg;
    pa.inline_emit = ctx->parse_inline_emit ? 1u : 0u;
    pa.slot_recs = c.slot_recs ? 1u : 0u;
    pa.migrate = ctx->parse_migrate ? 1u : 0u;
    pa.big = c.any_big ? 1u : 0u;
    pa.pace = c.parse_pace ? 1u : 0u;
    /* eight words behind the counts: the two launches' queues (three words each) and, word 3, the number of blocks the first
     * launch leaves to the second */
    K4_HIP(ctx, hipMemsetAsync(pa.meta + 2 * cnt, 0, 32, stream));
    if (c.queue) pa.queue = pa.meta + 2 * cnt;
    pa.nbig = pa.meta + 2 * cnt + 3;
    /* (the first launch also says whose every block is -- PARSE_BIG / PARSE_REST --, so it runs even without a block of its own) */
    ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_PARSE | (c.queue ? K4LZ4_ENCODE_ROUTE_QUEUE : 0) | (r.persistent ? K4LZ4_ENCODE_ROUTE_PERSISTENT : 0) |
                              (c.parse_pace ? K4LZ4_ENCODE_ROUTE_PARSE_PACE : 0) | (pa.migrate ? K4LZ4_ENCODE_ROUTE_MIGRATE : 0);
    hipLaunchKernelGGL(k4::k4_parse_kernel, dim3((unsigned)c.nwg), dim3((unsigned)(64 * c.waves)), 0, stream, a, pa);
    if (c.seg_two_step) {
        k4::ParseArgs pb = pa;
        pb.queue = pa.meta + 2 * cnt + 4;
        pb.nwg = (uint32_t)c.nwg_seg;
        ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_PARSE_SEG;
        hipLaunchKernelGGL(k4::k4_parse_seg_kernel, dim3((unsigned)c.nwg_seg), dim3(64 * k4::PARSE_MAX_WAVES), 0, stream, a, pb, sg);
    } else if (c.any_big) {
        k4::ParseArgs pb = pa;
        if (c.queue) pb.queue = pa.queue + 4;
        ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_PARSE_BIG;
        hipLaunchKernelGGL(k4::k4_parse_big_kernel, dim3((unsigned)c.nwg), dim3((unsigned)(64 * c.waves)), 0, stream, a, pb);
    }
    ctx->last_encode_route |= (pa.inline_emit ? 0 : K4LZ4_ENCODE_ROUTE_EMIT) | (c.rest ? K4LZ4_ENCODE_ROUTE_REST : 0) | (c.seg_two_step ? K4LZ4_ENCODE_ROUTE_SEGMENTS : 0);
    if (!pa.inline_emit) K4_LAUNCH_WAVES(k4::k4_emit_kernel, cnt, k4::EMIT_WAVES_PER_WG, stream, a, pa);
    if (c.rest) K4_LAUNCH_WAVES(k4::k4_encode_fast_rest_kernel, cnt, k4::ENCODE_WAVES_PER_WG, stream, a, pa);
    if (c.seg_two_step) segments_join_launch(stream, a, sg);
    return K4LZ4_OK;
}

/* LZ4Codec.Encode below level 3 */
int launch_fast_encode(k4lz4_ctx *ctx, k4::BatchArgs b, hipStream_t stream, const DictArgs *dd, const int32_t *hostLen)
{
    const FastRoute r = fast_route(ctx, b.flags, b.n);
    Sched s{};
    int rc;
    if (r.reorder && (rc = sched_scratch(ctx, stream, (size_t)std::min<int64_t>(r.chunk_max, b.n), &s)) != K4LZ4_OK) return rc;
    b.accel = ctx->accel;
    b.flags |= g_enforce32.load(std::memory_order_relaxed) ? K4LZ4_FLAG_X32 : 0;
    b.status = ctx->d_status;
    for (int64_t first = 0; first < b.n; first += r.chunk_max) {
        const int64_t cnt = std::min<int64_t>(r.chunk_max, b.n - first);
        const FastChunk c = fast_chunk(ctx, r, cnt, hostLen ? hostLen + first : nullptr);
        k4::BatchArgs a = slice(b, first, cnt);
        a.prof = ctx->prof ? ctx->prof + k4::PROF_STRIDE * first : nullptr;
        ctx->last_encode_route |= (first > 0 ? K4LZ4_ENCODE_ROUTE_CHUNKS : 0) | (r.pcost_order ? K4LZ4_ENCODE_ROUTE_PCOST_ORDER : 0);
        if (c.pace) {
            a.pace = ctx->d_pace;
            K4_HIP(ctx, hipMemsetAsync(a.pace, 0, k4::PACE_BYTES, stream));
        }
        k4::SegArgs sg{};
        if (r.segments && (rc = segment_plan(ctx, stream, a, c.seg_items, &sg)) != K4LZ4_OK) return rc;
        if (dd && dd->dict) {
            a.dict = dd->dict; a.dictOff = dd->off + first; a.dictLen = dd->len + first;
            a.dictMode = dd->mode ? dd->mode + first : nullptr;
        }
        if (r.reorder && (rc = order_prelude(ctx, stream, a, s, r.pcost_order, 0, r.cost_sample, c.two_kernels)) != K4LZ4_OK) return rc;
        rc = c.parse_here ? two_step_chunk(ctx, r, c, a, sg, stream) : one_kernel_chunk(ctx, r, c, a, sg, stream);
        if (rc != K4LZ4_OK) return rc;
        if (r.allow_copy) allow_copy(ctx, a, stream);
        K4_HIP(ctx, hipGetLastError());
    }
    return K4LZ4_OK;
}

/* ---- pickles and wraps through the encoders ---- */

/* Is a message big enough to be cut into segments?  (A small batch without one keeps the one-kernel pickle path: the segment
 * machinery costs a plan kernel, a 4096-workgroup launch on a second queue, a join, and -- on a context's first such call --
 * 269 MB of scratch; lengths the host does not know count as "may be big".) */
bool may_cut(const k4lz4_ctx *ctx, int64_t n, const int32_t *hostLen)
{
    if (!ctx->use_segments || !hostLen || n > (int64_t)ctx->pickle_split_min) return ctx->use_segments;
    for (int64_t i = 0; i < n; i++)
        if ((uint32_t)hostLen[i] >= ctx->seg_min) return true;
    return false;
}

/* Fast-level pickles of a batch go the encoders' way: slots prepared (block = envelope + 5, cap U - 1, exactly what
 * k4_pickle_kernel hands its encoder), the batch encoded by the two encoder kernels side by side -- the expensive
 * messages with their tables in LDS, the others with tables in memory, which puts a ragged batch on all the
 * chip's wave slots instead of the nine per CU that have room for a table in LDS --, envelopes closed afterwards.
 * (Wraps take this way whatever the batch; without a message big enough to be cut, not into segments.) */
int launch_envelope(k4lz4_ctx *ctx, Envelope env, k4::BatchArgs b, hipStream_t stream, const int32_t *hostLen)
{
    const int seg_ok = env == ENV_PICKLE || may_cut(ctx, b.n, hostLen) ? FLAG_SEGMENTS_OK : 0;
    const int enc_flags = (b.flags & (K4LZ4_FLAG_NO_REORDER | K4LZ4_FLAG_X32)) | K4LZ4_FLAG_RAW_RETURN | seg_ok;
    b.accel = 1;
    b.flags |= g_enforce32.load(std::memory_order_relaxed) ? K4LZ4_FLAG_X32 : 0;
    for (int64_t first = 0; first < b.n; first += LAUNCH_CHUNK_MAX) {
        const int64_t cnt = std::min<int64_t>(LAUNCH_CHUNK_MAX, b.n - first);
        int rc = grow_after(ctx, stream, &ctx->d_pk_meta, &ctx->d_pk_meta_cap, (size_t)cnt * 16 + 64);
        if (rc != K4LZ4_OK) return rc;
        uint64_t *d_encoff = (uint64_t *)ctx->d_pk_meta;
        int32_t *d_enccap = (int32_t *)(d_encoff + cnt);
        int32_t *d_enclen = d_enccap + cnt;
        const k4::BatchArgs a = slice(b, first, cnt);
        ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_ENVELOPE;
        envelope_prep(env, a, d_encoff, d_enccap, stream);
        k4::BatchArgs e{};
        e.src = a.src; e.srcOff = a.srcOff; e.srcLen = a.srcLen; e.dst = a.dst; e.dstOff = d_encoff; e.dstCap = d_enccap; e.outLen = d_enclen;
        e.n = cnt; e.level = a.level; e.flags = enc_flags;
        rc = launch_fast_encode(ctx, e, stream, nullptr, hostLen ? hostLen + first : nullptr);
        if (rc != K4LZ4_OK) return rc;
        envelope_finish(env, a, d_enclen, stream);
        K4_HIP(ctx, hipGetLastError());
    }
    return K4LZ4_OK;
}

/* ---- decode, unpickle, the small-batch pickle kernel ---- */

int launch_decode_like(k4lz4_ctx *ctx, Kind kind, k4::BatchArgs b, hipStream_t stream, const DictArgs *dd)
{
    const int64_t cu = ctx->cu_count;
    /* cost-ordered dispatch (most expensive blocks first): pickles by default, decoders on request */
    const bool reorder = b.n > 1 &&
                         (kind == KIND_PICKLE ? !(b.flags & K4LZ4_FLAG_NO_REORDER)
                                              : ((b.flags & K4LZ4_FLAG_REORDER) != 0 ||
                                                 /* pickles are ragged by nature: start the long ones first unless told not to */
                                                 (kind == KIND_UNPICKLE && b.n > 64 && !(b.flags & K4LZ4_FLAG_NO_REORDER))));
    Sched s{};
    int rc;
    if (reorder && (rc = sched_scratch(ctx, stream, (size_t)std::min<int64_t>(LAUNCH_CHUNK_MAX, b.n), &s)) != K4LZ4_OK) return rc;
    b.accel = ctx->accel;
    b.flags |= g_enforce32.load(std::memory_order_relaxed) ? K4LZ4_FLAG_X32 : 0;
    b.status = ctx->d_status;
    for (int64_t first = 0; first < b.n; first += LAUNCH_CHUNK_MAX) {
        const int64_t cnt = std::min<int64_t>(LAUNCH_CHUNK_MAX, b.n - first);
        k4::BatchArgs a = slice(b, first, cnt);
        a.prof = ctx->prof ? ctx->prof + k4::PROF_STRIDE * first : nullptr;
        /* pair decoders: the token chain two links at a time while the launch leaves wave slots free (k4lz4_decode.hpp, follow_tokens) */
        const bool hop2 = cnt <= (int64_t)ctx->hop2_max_per_cu * cu;
        if (K4_DEC_PACE && kind != KIND_PICKLE && ctx->use_pace && ctx->d_pace && cnt > (int64_t)ctx->pace_min_per_cu * cu) {   /* k4lz4_common.hpp, Pace: more than two blocks per SIMD */
            a.pace = ctx->d_pace;
            K4_HIP(ctx, hipMemsetAsync(a.pace, 0, k4::PACE_BYTES, stream));
        }
        if (dd && dd->dict) {
            a.dict = dd->dict; a.dictOff = dd->off + first; a.dictLen = dd->len + first;
            a.dictMode = dd->mode ? dd->mode + first : nullptr;
        }
        if (reorder && (rc = order_prelude(ctx, stream, a, s, false, kind == KIND_PICKLE ? 0 : 1, k4::COST_SAMPLE, false)) != K4LZ4_OK) return rc;
        if (kind == KIND_PICKLE) {
            ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_PICKLE;
            K4_LAUNCH_WAVES(k4::k4_pickle_kernel, cnt, 1, stream, a);
        } else if (kind == KIND_DECODE) {
            ctx->last_decode_kernel = a.pace ? K4LZ4_DECODE_KERNEL_PACE : 0;
            if (a.prof && ctx->prof_pair && !ctx->prof_stamp) {
                ctx->last_decode_kernel |= K4LZ4_DECODE_KERNEL_PROF;
                hipLaunchKernelGGL(k4::k4_decode_pair_prof_kernel, dim3((unsigned)((cnt + k4::DECODE_PAIRS_PER_WG - 1) / k4::DECODE_PAIRS_PER_WG)),
                                   dim3(128 * k4::DECODE_PAIRS_PER_WG), 0, stream, a);
            }
            else if (a.prof && !ctx->prof_stamp) {
                ctx->last_decode_kernel |= K4LZ4_DECODE_KERNEL_PROF;
                K4_LAUNCH_WAVES(k4::k4_decode_prof_kernel, cnt, k4::DECODE_WAVES_PER_WG, stream, a);
            }
            else if (cnt > 24 * cu) { /* more blocks than can be resident (6 waves x 4 SIMDs per CU) */
                ctx->last_decode_kernel |= K4LZ4_DECODE_KERNEL_DENSE;
                K4_LAUNCH_WAVES(k4::k4_decode_dense_kernel, cnt, k4::DECODE_WAVES_PER_WG, stream, a);
            }
            else if (cnt <= 16 * cu && !ctx->no_pair) {
                /* at most half the chip's wave slots (8 per SIMD at 64 VGPRs) are needed: two waves per block, one
                 * parsing ahead of the one that copies */
                ctx->last_decode_kernel |= hop2 ? K4LZ4_DECODE_KERNEL_PAIR2 : K4LZ4_DECODE_KERNEL_PAIR;
                hipLaunchKernelGGL(hop2 ? k4::k4_decode_pair2_kernel : k4::k4_decode_pair_kernel, dim3((unsigned)((cnt + k4::DECODE_PAIRS_PER_WG - 1) / k4::DECODE_PAIRS_PER_WG)),
                                   dim3(128 * k4::DECODE_PAIRS_PER_WG), 0, stream, a);
            }
            else {
                ctx->last_decode_kernel |= K4LZ4_DECODE_KERNEL_SINGLE;
                K4_LAUNCH_WAVES(k4::k4_decode_kernel, cnt, k4::DECODE_WAVES_PER_WG, stream, a);
            }
        } else {
            ctx->last_decode_kernel = a.pace ? K4LZ4_DECODE_KERNEL_PACE : 0;
            if (cnt <= 64 * cu && !ctx->no_pair) {
                ctx->last_decode_kernel |= hop2 ? K4LZ4_DECODE_KERNEL_UNPICKLE_PAIR2 : K4LZ4_DECODE_KERNEL_UNPICKLE_PAIR;
                hipLaunchKernelGGL(hop2 ? k4::k4_unpickle_pair2_kernel : k4::k4_unpickle_pair_kernel, dim3((unsigned)((cnt + k4::DECODE_PAIRS_PER_WG - 1) / k4::DECODE_PAIRS_PER_WG)),
                                   dim3(128 * k4::DECODE_PAIRS_PER_WG), 0, stream, a);
            }
            else {
                ctx->last_decode_kernel |= K4LZ4_DECODE_KERNEL_UNPICKLE_SINGLE;
                K4_LAUNCH_WAVES(k4::k4_unpickle_kernel, cnt, k4::DECODE_WAVES_PER_WG, stream, a);
            }
        }
        K4_HIP(ctx, hipGetLastError());
    }
    return K4LZ4_OK;
}

/* ---- the HC levels: the route ---- */
/* what is decided per launch chunk of cnt blocks once the longest of them is known */
struct HcChunk {
    enum Chain { CHAIN_PART, CHAIN_LDS, CHAIN_MEM } chain;      /* which kernel builds the chains */
    int64_t n_lds, n_mem;           /* CHAIN_LDS: its blocks, and those the table-in-memory kernel takes beside it on the second queue */
    enum Cand { CAND_NONE, CAND_LDS, CAND_MEM } cand;           /* where the candidates' records come from */
    unsigned gy, groups, per;       /* CAND_MEM: position chunks per block, groups of eight blocks, chunks per launch */
    bool optimal, pace;             /* k4_hc_parse_opt_kernel; else the parse's late-blocks-first priorities (k4lz4_common.hpp, Pace) */
    int nseg;                       /* the parse writes sequence records by this many waves per block if there is room for them; 0: none */
};

/* longest: the chunk's longest block; chained: its blocks have a history in front of them (k4::HcArgs::hist) -- such a batch takes
 * the memory paths: the LDS kernels are built around blocks of at most 64 KiB that start at their position 0 */
HcChunk hc_chunk(const k4lz4_ctx *ctx, int64_t cnt, unsigned long long longest, int level, bool chained)
{
    const int64_t cu = ctx->cu_count;
    const bool lds_ok = longest <= 65536 && !chained;
    HcChunk c{};
    /* no block over 64 KiB: eight waves per block, each with an eighth of the hash values and of the table (round 6) */
    if (lds_ok && ctx->hc_chain_parts) c.chain = HcChunk::CHAIN_PART;
    else if (lds_ok) {
        /* (rounds 3-5, K4LZ4_HC_CHAIN_OLD) no block over 64 KiB (known from the host lengths, the reservation or the device): hash tables in LDS -- two blocks
         * per CU, a wave each, which leaves the CU's other wave slots empty; so the last third of a big chunk goes through the
         * table-in-memory kernel on the second queue at the same time (its tables: 128 KiB per block, cleared by launch_hc) */
        c.chain = HcChunk::CHAIN_LDS;
        c.n_mem = cnt >= 8 * cu ? cnt * ctx->hc_mem_pct / 100 : 0;
        c.n_lds = cnt - c.n_mem;
    } else c.chain = HcChunk::CHAIN_MEM;
    c.optimal = level >= K4LZ4_L10_OPT;              /* clTable (LL64.high.cs:1124-1138): lz4opt strategy */
    /* no block over 64 KiB: the candidates' records out of LDS (k4_hc_walk_lds_kernel, k4_hc_cand_lds_kernel; round 6) */
    if (longest >= 13 && lds_ok && !c.optimal && ctx->hc_cand_lds) c.cand = HcChunk::CAND_LDS;
    else if (longest >= 13 && !c.optimal) {
        c.cand = HcChunk::CAND_MEM;
        c.gy = (unsigned)((longest + k4::HC_CAND_POS_PER_WG - 1) / k4::HC_CAND_POS_PER_WG);
        c.groups = (unsigned)((cnt + 7) / 8);                            /* eight blocks, one per XCD (k4_hc_cand_kernel) */
        c.per = std::max(1u, (1u << 30) / (8u * c.groups));              /* chunks per launch: the grid stays below 2^31 workgroups */
    }
    if (c.optimal) return c;
    /* level 3 on blocks of at most 64 KiB: the parse writes 8-byte sequence records (the fast encoder's scratch, a slot per
     * block) and the same wave turns them into bytes afterwards; without room for them LZ4HC_encodeSequence stays in the loop */
    /* ... by two or four waves per block while the chip has the wave slots for them (k4lz4_encode_hc.hpp, HcSegs; round 6) */
    if (level <= K4LZ4_L03_HC && lds_ok && ctx->hc_records)      /* (measured, profiles/r6_hc_ab.txt: four waves per block beat two even when they take turns -- 4096 blocks: 9.5 against 12.2-13.3 ms, one wave 13.9) */
        c.nseg = longest < k4::HC_SEG_MIN_LEN ? 1 : ctx->hc_segs > 0 ? ctx->hc_segs : (cnt * 2 <= 32 * cu ? 4 : 1);
    c.pace = ctx->use_pace && ctx->d_pace && cnt > 8 * cu;
    return c;
}

/* HC levels: layout -> (sync for the scratch size) -> hash-table clear -> chain kernel -> parse kernel.
 * `env`: the same around the LZ4Pickler envelope (encoder slot = envelope + 5, cap U - 1) or LZ4Wrapper's (+ 8, cap U - 1). */
/* hostLen: the blocks' lengths when the caller has them on the host (host-pointer calls), else nullptr; hist: chained HC streams
 * (k4::HcArgs::hist, device pointer), else nullptr */
int launch_hc(k4lz4_ctx *ctx, Envelope env, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
              const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags,
              hipStream_t stream, const int32_t *hostLen, const int32_t *hist = nullptr)
{
    const int64_t chunk_max = 4096;   /* 128 KiB of hash table per block in flight */
    for (int64_t first = 0; first < n; first += chunk_max) {
        const int64_t cnt = std::min<int64_t>(chunk_max, n - first);
        int rc = grow_after(ctx, stream, &ctx->d_hc_hash, &ctx->d_hc_hash_cap, (size_t)cnt << (k4::HC_HASH_LOG + 2));
        if (rc != K4LZ4_OK) return rc;
        rc = grow_after(ctx, stream, &ctx->d_hc_meta, &ctx->d_hc_meta_cap, (size_t)(cnt + 2) * 8 + (size_t)cnt * 16 + 64);
        if (rc != K4LZ4_OK) return rc;
        unsigned long long *d_woff = (unsigned long long *)ctx->d_hc_meta;
        uint64_t *d_encoff = (uint64_t *)(d_woff + cnt + 2);
        int32_t *d_enccap = (int32_t *)(d_encoff + cnt);
        int32_t *d_enclen = d_enccap + cnt;
        k4::HcArgs h{};
        h.status = ctx->d_status;
        h.src = src; h.srcOff = srcOff + first; h.srcLen = srcLen + first;
        h.dst = dst; h.dstOff = dstOff + first; h.dstCap = dstCap + first; h.outLen = outLen + first;
        h.n = cnt; h.level = level; h.flags = flags;
        h.hash = (uint32_t *)ctx->d_hc_hash; h.workOff = d_woff;
        h.hist = hist ? hist + first : nullptr;
        k4::BatchArgs a{};
        a.src = src; a.srcOff = h.srcOff; a.srcLen = h.srcLen; a.dst = dst; a.dstOff = h.dstOff; a.dstCap = h.dstCap;
        a.outLen = h.outLen; a.n = cnt; a.level = level; a.accel = 1; a.flags = flags;
        if (env == ENV_PICKLE || env == ENV_WRAP) {
            ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_ENVELOPE;
            envelope_prep(env, a, d_encoff, d_enccap, stream);
            h.dstOff = d_encoff; h.dstCap = d_enccap; h.outLen = d_enclen; h.flags = K4LZ4_FLAG_RAW_RETURN;
        }
        /* How much work area, and how long the longest block is: from the host's copy of the lengths, from the
         * reservation (k4lz4_ctx_reserve_hc), or -- the only case that synchronises -- from the device. */
        unsigned long long tail[2] = {0, 0};   /* total work bytes, longest block */
        bool ask_device = false;
        if (hostLen) {
            for (int64_t i = 0; i < cnt; i++) {
                const int32_t len = hostLen[first + i];
                if (len > 0) {
                    tail[0] += (((unsigned long long)len + 3u) & ~3ull) * k4::HC_WORK_PER_BYTE;
                    tail[1] = std::max<unsigned long long>(tail[1], (unsigned long long)len);
                }
            }
        } else if (ctx->hc_res_total) {
            tail[0] = (ctx->hc_res_total + 4u * (unsigned long long)cnt) * k4::HC_WORK_PER_BYTE;
            tail[1] = ctx->hc_res_longest;
            h.workCap = tail[0]; h.maxLen = ctx->hc_res_longest;
        } else {
            ask_device = true;
        }
        if (!ask_device) {
            rc = grow_after(ctx, stream, &ctx->d_hc_work, &ctx->d_hc_work_cap, (size_t)tail[0] + 256);
            if (rc != K4LZ4_OK) return rc;
        }
        hipLaunchKernelGGL(k4::k4_hc_layout_kernel, dim3(1), dim3(256), 0, stream, h);
        if (ask_device) {
            K4_HIP(ctx, hipMemcpyAsync(tail, d_woff + cnt, 16, hipMemcpyDeviceToHost, stream));
            K4_HIP(ctx, hipStreamSynchronize(stream));
            rc = grow(ctx, &ctx->d_hc_work, &ctx->d_hc_work_cap, (size_t)tail[0] + 256, false);
            if (rc != K4LZ4_OK) return rc;
        }
        h.work = ctx->d_hc_work;
        const HcChunk c = hc_chunk(ctx, cnt, tail[1], level, hist != nullptr);
        if (c.chain == HcChunk::CHAIN_PART) {
            h.nChain = cnt;
            ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_HC_CHAIN_PART;
            hipLaunchKernelGGL(k4::k4_hc_chain_part_kernel, dim3((unsigned)cnt), dim3(64 * k4::HC_CHAIN_PARTS), 0, stream, h);
        } else if (c.chain == HcChunk::CHAIN_LDS) {
            if (c.n_mem > 0) {
                K4_HIP(ctx, hipEventRecord(ctx->ev_fork, stream));
                K4_HIP(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
                K4_HIP(ctx, hipMemsetAsync(ctx->d_hc_hash + ((size_t)c.n_lds << (k4::HC_HASH_LOG + 2)), 0, (size_t)c.n_mem << (k4::HC_HASH_LOG + 2), ctx->aux));
                k4::HcArgs hm = h;
                hm.blockBase = (unsigned)c.n_lds; hm.nChain = c.n_mem;
                ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_HC_CHAIN_MEM;
                K4_LAUNCH_WAVES(k4::k4_hc_chain_kernel, c.n_mem, k4::HC_CHAIN_WAVES_PER_WG, ctx->aux, hm);
                K4_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->aux));
            }
            h.nChain = c.n_lds;
            ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_HC_CHAIN_LDS;
            K4_LAUNCH_WAVES(k4::k4_hc_chain_lds_kernel, c.n_lds, k4::HC_CHAIN_LDS_WAVES_PER_WG, stream, h);
            if (c.n_mem > 0) K4_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_join, 0));
        } else {
            K4_HIP(ctx, hipMemsetAsync(ctx->d_hc_hash, 0, (size_t)cnt << (k4::HC_HASH_LOG + 2), stream));
            h.nChain = cnt;
            ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_HC_CHAIN_MEM;
            K4_LAUNCH_WAVES(k4::k4_hc_chain_kernel, cnt, k4::HC_CHAIN_WAVES_PER_WG, stream, h);
        }
        if (c.cand == HcChunk::CAND_LDS) {
            ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_HC_CAND_LDS;
            hipLaunchKernelGGL(k4::k4_hc_walk_lds_kernel, dim3((unsigned)cnt), dim3(64 * k4::HC_LDS_WAVES), 0, stream, h);
            hipLaunchKernelGGL(k4::k4_hc_cand_lds_kernel, dim3((unsigned)cnt), dim3(64 * k4::HC_CAND_LDS_WAVES), 0, stream, h);
        } else if (c.cand == HcChunk::CAND_MEM) {
            ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_HC_CAND_MEM;
            for (unsigned y0 = 0; y0 < c.gy; y0 += c.per) {
                k4::HcArgs hy = h;
                hy.posBase = y0 * (unsigned)k4::HC_CAND_POS_PER_WG;
                hy.candChunks = std::min(c.per, c.gy - y0);
                hipLaunchKernelGGL(k4::k4_hc_cand_kernel, dim3(c.groups * 8u * hy.candChunks), dim3(256), (size_t)ctx->hc_cand_dynlds, stream, hy);
            }
        }
        if (c.optimal) {
            ctx->last_encode_route |= K4LZ4_ENCODE_ROUTE_HC_PARSE_OPT;
            K4_LAUNCH_WAVES(k4::k4_hc_parse_opt_kernel, cnt, 1, stream, h);
        } else {
            int nseg = c.nseg;      /* the records the route wants: fewer waves per block, or none, where d_parse cannot grow that far */
            while (nseg) {
                const size_t need = (size_t)cnt * (nseg == 4 ? k4::hc_seg_rec_off(4, 4) : nseg == 2 ? k4::hc_seg_rec_off(2, 2) : k4::PARSE_REC_STRIDE) * sizeof(uint2);
                if (grow_after(ctx, stream, &ctx->d_parse, &ctx->d_parse_cap, need) == K4LZ4_OK) { h.recs = (uint2 *)ctx->d_parse; break; }
                { std::lock_guard<std::mutex> g(g_err_mu); ctx->error.clear(); }
                nseg = nseg > 1 ? 1 : 0;
            }
            if (c.pace) {
                h.pace = ctx->d_pace;
                K4_HIP(ctx, hipMemsetAsync(h.pace, 0, k4::PACE_BYTES, stream));
            }
            ctx->last_encode_route |= h.recs && nseg == 4 ? K4LZ4_ENCODE_ROUTE_HC_PARSE_SEG4 : h.recs && nseg == 2 ? K4LZ4_ENCODE_ROUTE_HC_PARSE_SEG2 :
                                      h.recs ? K4LZ4_ENCODE_ROUTE_HC_PARSE_REC : K4LZ4_ENCODE_ROUTE_HC_PARSE;
            if (h.recs && nseg == 4) hipLaunchKernelGGL(k4::k4_hc_parse_seg4_kernel, dim3((unsigned)((cnt + 1) / 2)), dim3(64 * k4::HC_SEG_WAVES_PER_WG), 0, stream, h);
            else if (h.recs && nseg == 2) hipLaunchKernelGGL(k4::k4_hc_parse_seg2_kernel, dim3((unsigned)((cnt + 3) / 4)), dim3(64 * k4::HC_SEG_WAVES_PER_WG), 0, stream, h);
            else if (h.recs) K4_LAUNCH_WAVES(k4::k4_hc_parse_rec_kernel, cnt, k4::HC_REC_WAVES_PER_WG, stream, h);
            else K4_LAUNCH_WAVES(k4::k4_hc_parse_kernel, cnt, k4::HC_PARSE_WAVES_PER_WG, stream, h);
        }
        envelope_finish(env, a, d_enclen, stream);
        K4_HIP(ctx, hipGetLastError());
    }
    return K4LZ4_OK;
}

/* enqueue the kernels for n blocks; all pointers are device pointers */
int launch_inner(k4lz4_ctx *ctx, Kind kind, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint8_t *dst,
                 const uint64_t *dstOff, const int32_t *dstCap, int32_t *outLen, int64_t n, int level, int flags,
                 hipStream_t stream, const DictArgs *dd, const int32_t *hostLen)
{
    const Envelope env = kind == KIND_PICKLE ? ENV_PICKLE : kind == KIND_WRAP ? ENV_WRAP : ENV_NONE;
    k4::BatchArgs b{};
    b.src = src; b.srcOff = srcOff; b.srcLen = srcLen; b.dst = dst; b.dstOff = dstOff; b.dstCap = dstCap; b.outLen = outLen;
    b.n = n; b.level = level; b.flags = flags;
    if (kind == KIND_ENCODE || env != ENV_NONE) ctx->last_encode_route = K4LZ4_ENCODE_ROUTE_NONE;
    if ((kind == KIND_ENCODE || env != ENV_NONE) && level >= K4LZ4_L03_HC) {
        const int rc = launch_hc(ctx, env, src, srcOff, srcLen, dst, dstOff, dstCap, outLen, n, level, flags, stream, hostLen);
        if (rc != K4LZ4_OK || kind != KIND_ENCODE || !(flags & K4LZ4_FLAG_ALLOW_COPY)) return rc;
        for (int64_t first = 0; first < n; first += LAUNCH_CHUNK_MAX) allow_copy(ctx, slice(b, first, std::min<int64_t>(LAUNCH_CHUNK_MAX, n - first)), stream);
        K4_HIP(ctx, hipGetLastError());
        return K4LZ4_OK;
    }
    if (kind == KIND_ENCODE) return launch_fast_encode(ctx, b, stream, dd, hostLen);
    if (kind == KIND_WRAP || (kind == KIND_PICKLE && !ctx->prof && (n > (int64_t)ctx->pickle_split_min || may_cut(ctx, n, hostLen))))
        return launch_envelope(ctx, env, b, stream, hostLen);
    return launch_decode_like(ctx, kind, b, stream, dd);
}
