/*
 * k4lz4_frame_reader_loop.hpp -- the text of k4_fr_read_kernel's loop, included into the body of a kernel (no include guard): into
 * k4_fr_read_kernel with FR_LOOP_DICT 0, which is that kernel as it always was, and into k4_fr_dict_read_kernel
 * (k4lz4_frame_reader_dict.hpp) with FR_LOOP_DICT 1.  Text and not a function template: wrapped in a function the
 * loop compiles to other register assignments (SGPR spills 86 -> 83) and the kernel without a set is to stay the one that was measured.
 * The kernel provides `a` (FrReadArgs) and `lds`, with FR_LOOP_DICT also `d` (FrDict).
 *
 * FR_LOOP_DICT: a DictID resolves against d; the blocks of an independent frame are decoded against the entry's kept bytes as an
 * external dictionary, a chained frame starts with them at the front of its buffer as LZ4ChainDecoder does after Inject -- never
 * drained, never counted, never hashed.
 */
    const int lane = lane_id();
    const uint32_t wave = uni(threadIdx.x >> 6);
    const long long s = (long long)blockIdx.x * FR_WAVES_PER_WG + (long long)wave;
    if (s >= a.n) return;
    if (a.done && a.done[s] == FR_PLAN_DONE) return;
    const int64_t want = a.count ? a.count[s] : 0;
    if (want < 0) {                                          /* untouched, as srcLen[s] < 0 in the writer */
        if (lane == 0) a.outLen[s] = 0;
        return;
    }
    FrState *st = (FrState *)(a.store + a.storeOff[s]);
    uint8_t *buf = (uint8_t *)st + FR_STATE_BYTES;
    if (a.op == FR_OP_RESET) {
        uint32_t *w = (uint32_t *)st;
        if (lane < (int)(FR_STATE_BYTES / 4)) w[lane] = 0u;
        if (lane == 0) a.outLen[s] = 0;
        return;
    }
    /* the state, the same in every lane */
    uint64_t pos = st->pos, bytes_read = st->bytesRead, clen = st->clen, blocks = st->blocks;
    int phase = st->phase, code = st->code;
    uint32_t flg = st->flg, bd = st->bd, pending = st->pending, tail = st->tail, direct = st->direct;
    int bs = st->bsize;
#if FR_LOOP_DICT
    uint32_t entry1 = uni(st->dictEntry);
#endif
    wave_sync();
    if (phase == FR_PHASE_FAILED) {                          /* failed streams stay failed and touch nothing */
        if (lane == 0) a.outLen[s] = code;
        return;
    }
    const uint8_t *p = a.src + a.srcOff[s];
    const uint64_t end = a.srcLen[s];
    uint8_t *out = a.dst ? a.dst + a.dstOff[s] : nullptr;
    const uint32_t buf_bytes = (uint32_t)fr_buffer_bytes(a.maxBlock);
    int fail = 0;
    int64_t result = 0;
    bool has_frame = phase == FR_PHASE_OPEN;
#if FR_LOOP_DICT
    const uint8_t *dict_end = nullptr;                       /* the open frame's kept bytes */
    uint32_t dict_len = 0u;
    if (has_frame) {
        if (entry1 > (uint32_t)d.nDict) fail = FR_DICT;      /* the set is not the one the frame was opened with */
        else dict_len = fr_dict_kept(d, entry1, dict_end);
    }
#endif

    /* ---- EnsureHeader -> ReadHeader (.async.cs:46-108) */
    if (!has_frame && pos < end) {                           /* TryPeek4: nothing left is a clean end (ReaderExtensions.cs:20-21) */
        FrHeader hd{flg, bd, 0u, bs, clen};
#if FR_LOOP_DICT
        fail = fr_parse_header_ids<true>(p + pos, end - pos, a.maxBlock, hd, d, entry1);
#else
        fail = fr_parse_header(p + pos, end - pos, a.maxBlock, hd);
#endif
        flg = hd.flg; bd = hd.bd;
        if (!fail) {
            clen = hd.clen; bs = hd.bs;
            if (flg & FLG_CONTENT_SUM) fr_xxh_update(&st->content, p + pos, 0, true, lane);   /* InitializeContentChecksum */
            pos += hd.len;
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

    if (!fail && a.op == FR_OP_OPEN) result = has_frame ? 1 : 0;
    if (!fail && a.op == FR_OP_READ && has_frame) {
        const bool chained = !(flg & FLG_INDEPENDENT);
        uint64_t offset = 0, count = (uint64_t)want;
        while (count > 0) {
            if (pending == 0) {
                /* ---- ReadBlock (.async.cs:110-137) */
                if (end - pos < 4) { fail = FR_EOF; break; }
                const uint32_t lc = ld32u(p + pos);
                pos += 4;
                if (lc == 0) {                                                      /* EndMark */
                    if (flg & FLG_CONTENT_SUM) {
                        if (end - pos < 4) { fail = FR_EOF; break; }
                        const uint32_t stored = ld32u(p + pos);
                        pos += 4;
                        if (fw_xxh32_digest(st->content) != stored) { fail = FR_CONTENT_SUM; break; }
                    }
                    phase = FR_PHASE_NONE;                                          /* CloseFrame: this read ends with what it has */
                    break;
                }
                const uint32_t sn = lc & 0x7fffffffu;
                const bool raw = (lc & 0x80000000u) != 0;
                if (sn > (uint32_t)bs) { fail = FR_BLOCK; break; }                  /* does not fit AllocBuffer(blockSize): see above */
                if (end - pos < sn) { fail = FR_EOF; break; }
                const uint8_t *payload = p + pos;
                pos += sn;
                if (flg & FLG_BLOCK_SUM) {
                    if (end - pos < 4) { fail = FR_EOF; break; }
                    const uint32_t stored = ld32u(p + pos);
                    pos += 4;
                    fr_xxh_update(&st->scratch, payload, sn, true, lane);
                    if (fw_xxh32_digest(st->scratch) != stored) { fail = FR_BLOCK_SUM; break; }
                }
                blocks++;
                /* ---- InjectOrDecode */
                uint32_t got = 0;
                const uint8_t *made = buf;                                          /* where the block's bytes are */
                bool to_dst = false;
                if (chained) {
                    /* LZ4ChainDecoder.Prepare / Inject: the block goes behind the bytes so far; the last 64 KiB move to the front first
                     * when it would not fit */
                    const uint32_t need = raw ? sn : (uint32_t)bs;
                    if (tail + need > buf_bytes) {
                        const uint32_t keep = tail < FR_HISTORY ? tail : FR_HISTORY;
                        wave_sync();
                        wave_shift_down(buf, buf + tail - keep, keep, lane);
                        tail = keep;
                    }
                    made = buf + tail;
                }
                if (raw) {
                    /* Inject: LZ4BlockDecoder.cs:58-71 (<= blockSize + 8), LZ4ChainDecoder.cs:64-93 (<= max(blockSize, 64 KiB)): the
                     * stored length is at most blockSize here.  Nothing (0x80000000) ends the read without closing the frame */
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
                    /* LZ4ChainDecoder.Decode: < 0 throws, 0 is a block of nothing; LZ4BlockDecoder.Decode through LZ4Codec.Decode: <= 0
                     * is -1 and throws (LZ4BlockDecoder.cs:49-51) */
                    if (ret < 0 || (!chained && ret == 0)) { fail = FR_BLOCK; break; }
                    got = (uint32_t)ret;
                }
                if (chained) tail += got; else if (!to_dst) tail = got;
                if ((flg & FLG_CONTENT_SUM) && got) fr_xxh_update(&st->content, made, got, false, lane);   /* UpdateContentChecksum */
                if (got == 0) break;                                                /* .async.cs:162-163: the frame stays open */
                if (to_dst) {                                                       /* decoded in place: Drain has nothing to move */
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
    if (fail) { phase = FR_PHASE_FAILED; code = fail; result = fail; }
    wave_sync();
    if (lane == 0) {
        st->pos = pos; st->bytesRead = bytes_read; st->clen = clen; st->blocks = blocks;
        st->phase = phase; st->code = code; st->flg = flg; st->bd = bd; st->bsize = bs;
        st->pending = pending; st->tail = tail; st->direct = direct;
#if FR_LOOP_DICT
        st->dictEntry = phase == FR_PHASE_OPEN ? entry1 : 0u;
#endif
        a.outLen[s] = result;
    }
