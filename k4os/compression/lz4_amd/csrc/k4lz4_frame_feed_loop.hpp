/*
 * k4lz4_frame_feed_loop.hpp -- the text of k4_fr_feed_kernel's loop, included into the body of a kernel (no include guard) as
 * k4lz4_frame_reader_loop.hpp is, and for the same reason (as a function: SGPR spills 116 -> 122): into k4_fr_feed_kernel with
 * FR_LOOP_DICT 0 and into k4_fr_dict_feed_kernel (k4lz4_frame_reader_dict.hpp) with FR_LOOP_DICT 1.  The kernel provides `fa`
 * (FrFeedArgs) and `lds`, with FR_LOOP_DICT also `d` (FrDict).
 */
    const FrReadArgs &a = fa.r;
    const int lane = lane_id();
    const uint32_t wave = uni(threadIdx.x >> 6);
    const long long s = (long long)blockIdx.x * FR_WAVES_PER_WG + (long long)wave;
    if (s >= a.n) return;
    if (a.done && a.done[s] == FR_PLAN_DONE) return;
    const int64_t want = a.count ? a.count[s] : 0;
    if (want < 0) {                                          /* untouched */
        if (lane == 0) { a.outLen[s] = 0; fa.consumed[s] = 0; fa.need[s] = 0; }
        return;
    }
    FrState *st = (FrState *)(a.store + a.storeOff[s]);
    uint8_t *buf = (uint8_t *)st + FR_STATE_BYTES;
    if (a.op == FR_OP_RESET) {
        uint32_t *w = (uint32_t *)st;
        if (lane < (int)(FR_STATE_BYTES / 4)) w[lane] = 0u;
        if (lane == 0) { a.outLen[s] = 0; fa.consumed[s] = 0; fa.need[s] = 0; }
        return;
    }
    /* the state, the same in every lane */
    uint64_t bytes_read = st->bytesRead, clen = st->clen, blocks = st->blocks;
    int phase = st->phase, code = st->code;
    uint32_t flg = st->flg, bd = st->bd, pending = st->pending, tail = st->tail, direct = st->direct;
    int bs = st->bsize;
    const uint32_t fill0 = st->stashFill;
#if FR_LOOP_DICT
    uint32_t entry1 = uni(st->dictEntry);
#endif
    wave_sync();
    if (phase == FR_PHASE_FAILED) {                          /* failed streams stay failed and touch nothing */
        if (lane == 0) { a.outLen[s] = code; fa.consumed[s] = 0; fa.need[s] = 0; }
        return;
    }
    FrFeedSrc f{a.src ? a.src + a.srcOff[s] : nullptr, 0u, a.srcLen[s], (uint8_t *)st + fr_store_bytes(a.maxBlock), fill0};
    const bool fin = fa.final && fa.final[s] != 0;
    uint8_t *out = a.dst ? a.dst + a.dstOff[s] : nullptr;
    const uint32_t buf_bytes = (uint32_t)fr_buffer_bytes(a.maxBlock);
    int fail = 0;
    int64_t result = 0;
    uint32_t need = 0, awaited = 0;                          /* starved: bytes missing of the field, and the field's length */
    bool has_frame = phase == FR_PHASE_OPEN;
#if FR_LOOP_DICT
    const uint8_t *dict_end = nullptr;                       /* the open frame's kept bytes */
    uint32_t dict_len = 0u;
    if (has_frame) {
        if (entry1 > (uint32_t)d.nDict) fail = FR_DICT;      /* the set is not the one the frame was opened with */
        else dict_len = fr_dict_kept(d, entry1, dict_end);
    }
#endif

    /* ---- EnsureHeader -> ReadHeader (.async.cs:46-108): the magic, FLG / BD and the rest are three fields of one stash run */
    if (!has_frame) {
        const uint8_t *h;
        uint32_t have;
        int hw;
        for (;;) {
            h = f.fill ? f.stash : f.p + f.at;
            have = f.fill ? f.fill : (f.end - f.at > 32u ? 32u : (uint32_t)(f.end - f.at));
            hw = have ? fr_header_want(h, have) : 4;
            if (hw <= 0 || !fr_feed_field(f, (uint32_t)hw, lane)) break;
        }
        if (hw < 0) {
            fail = hw;
        } else if (hw > 0) {                                 /* the header is not all there */
            if (!fin) { awaited = (uint32_t)hw; need = fr_feed_keep(f, awaited, lane); }
            else if (have) fail = FR_EOF;                    /* nothing left is a clean end (ReaderExtensions.cs:20-21) */
        } else {
            FrHeader hd{flg, bd, 0u, bs, clen};
#if FR_LOOP_DICT
            fail = fr_parse_header_ids<true>(h, have, a.maxBlock, hd, d, entry1);
#else
            fail = fr_parse_header(h, have, a.maxBlock, hd);
#endif
            flg = hd.flg; bd = hd.bd;
            if (!fail) {
                clen = hd.clen; bs = hd.bs;
                if (flg & FLG_CONTENT_SUM) fr_xxh_update(&st->content, h, 0, true, lane);   /* InitializeContentChecksum */
                fr_feed_take(f, hd.len);
                pending = 0; tail = 0;
#if FR_LOOP_DICT
                entry1 = uni(entry1);
                dict_len = fr_dict_kept(d, entry1, dict_end);
                if (dict_len && !(flg & FLG_INDEPENDENT)) {  /* LZ4ChainDecoder.Inject(kept bytes) */
                    wave_sync();
                    wave_copy(buf, dict_end - dict_len, dict_len, lane);
                    wave_sync();
                    tail = dict_len;
                }
#endif
                phase = FR_PHASE_OPEN;
                has_frame = true;
            }
        }
    }

    if (!fail && a.op == FR_OP_OPEN) result = has_frame ? 1 : 0;
    if (!fail && a.op == FR_OP_READ && has_frame) {
        const bool chained = !(flg & FLG_INDEPENDENT);
        uint64_t offset = 0, count = (uint64_t)want;
        while (count > 0) {
            if (pending == 0) {
                /* ---- ReadBlock (.async.cs:110-137) */
                const uint8_t *rec = fr_feed_field(f, 4u, lane);
                if (!rec) {
                    if (fin) fail = FR_EOF; else { awaited = 4u; need = fr_feed_keep(f, 4u, lane); }
                    break;
                }
                const uint32_t lc = ld32u(rec);
                if (lc == 0) {                                                      /* EndMark */
                    if (flg & FLG_CONTENT_SUM) {
                        rec = fr_feed_field(f, 8u, lane);
                        if (!rec) {
                            if (fin) fail = FR_EOF; else { awaited = 8u; need = fr_feed_keep(f, 8u, lane); }
                            break;
                        }
                        const uint32_t stored = ld32u(rec + 4);
                        fr_feed_take(f, 8u);
                        if (fw_xxh32_digest(st->content) != stored) { fail = FR_CONTENT_SUM; break; }
                    } else {
                        fr_feed_take(f, 4u);
                    }
                    phase = FR_PHASE_NONE;                                          /* CloseFrame: this read ends with what it has */
                    break;
                }
                const uint32_t sn = lc & 0x7fffffffu;
                const bool raw = (lc & 0x80000000u) != 0;
                if (sn > (uint32_t)bs) { fail = FR_BLOCK; break; }                  /* does not fit AllocBuffer(blockSize) */
                const uint32_t rl = 4u + sn + ((flg & FLG_BLOCK_SUM) ? 4u : 0u);
                rec = fr_feed_field(f, rl, lane);
                if (!rec) {
                    if (fin) fail = FR_EOF; else { awaited = rl; need = fr_feed_keep(f, rl, lane); }
                    break;
                }
                const uint8_t *payload = rec + 4;
                fr_feed_take(f, rl);
                if (flg & FLG_BLOCK_SUM) {
                    const uint32_t stored = ld32u(payload + sn);
                    fr_xxh_update(&st->scratch, payload, sn, true, lane);
                    if (fw_xxh32_digest(st->scratch) != stored) { fail = FR_BLOCK_SUM; break; }
                }
                blocks++;
                /* ---- InjectOrDecode, as k4_fr_read_kernel */
                uint32_t got = 0;
                const uint8_t *made = buf;
                bool to_dst = false;
                if (chained) {
                    const uint32_t room = raw ? sn : (uint32_t)bs;
                    if (tail + room > buf_bytes) {
                        const uint32_t keep = tail < FR_HISTORY ? tail : FR_HISTORY;
                        wave_sync();
                        wave_shift_down(buf, buf + tail - keep, keep, lane);
                        tail = keep;
                    }
                    made = buf + tail;
                }
                if (raw) {
                    got = sn;
                    if (!chained && count >= sn) { to_dst = true; made = out + offset; }
                    wave_sync();
                    if (sn) wave_copy((uint8_t *)made, payload, sn, lane);
                    wave_sync();
                } else {
                    const int cap = chained ? bs : bs + 8;
                    DecodeDict dict{nullptr, 0u, 0};
                    if (chained && tail) {
                        const uint32_t hist = tail < FR_HISTORY ? tail : FR_HISTORY;
                        dict = DecodeDict{made, hist >= 65535u ? 65536u : hist, 1};
                    }
#if FR_LOOP_DICT
                    if (!chained && dict_len) dict = DecodeDict{dict_end, dict_len, 2};
#endif
                    if (!chained && count >= (uint64_t)cap) { to_dst = true; made = out + offset; }
                    wave_sync();
                    const int ret = decode_block(payload, (int)sn, (uint8_t *)made, cap, lane, lds[wave], nullptr, false, dict);
                    wave_sync();
                    if (ret < 0 || (!chained && ret == 0)) { fail = FR_BLOCK; break; }
                    got = (uint32_t)ret;
                }
                if (chained) tail += got; else if (!to_dst) tail = got;
                if ((flg & FLG_CONTENT_SUM) && got) fr_xxh_update(&st->content, made, got, false, lane);   /* UpdateContentChecksum */
                if (got == 0) break;                                                /* .async.cs:162-163: the frame stays open */
                if (to_dst) {
                    direct++;
                    bytes_read += got; offset += got; count -= got;
                    if (a.interactive) break;
                    continue;
                }
                pending = got;
            }
            /* ---- Drain (LZ4FrameReader.cs:98-112) */
            const uint32_t n = count < pending ? (uint32_t)count : pending;
            wave_sync();
            wave_copy(out + offset, buf + tail - pending, n, lane);
            bytes_read += n; pending -= n; offset += n; count -= n;
            if (a.interactive) break;
        }
        result = (int64_t)offset;
    }
    if (fail) { phase = FR_PHASE_FAILED; code = fail; result = fail; need = 0; awaited = 0; }
    wave_sync();
    if (lane == 0) {
        st->pos += f.at; st->bytesRead = bytes_read; st->clen = clen; st->blocks = blocks;
        st->phase = phase; st->code = code; st->flg = flg; st->bd = bd; st->bsize = bs;
        st->pending = pending; st->tail = tail; st->direct = direct;
        st->stashFill = need ? f.fill : 0u; st->stashWant = need ? awaited : 0u;
#if FR_LOOP_DICT
        st->dictEntry = phase == FR_PHASE_OPEN ? entry1 : 0u;
#endif
        a.outLen[s] = result;
        fa.consumed[s] = (int64_t)f.at;
        fa.need[s] = (int64_t)need;
    }
