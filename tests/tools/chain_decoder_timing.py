#!/usr/bin/env python
"""Many open chained decoders advanced per call (ChainDecoderDevice, k4lz4_chain_decode_batch_device) next to
k4lz4_decode_chain_batch_device over the same streams whole, in the same run: chained L00 streams of 64 KiB blocks from
encode_fast_chain_device, drained, in runs of R blocks per call.  frame_reader_timing.py's protocol: device events around the
whole sequence of calls (the reset launch included), warm-up first, the two sides in alternating windows, median and range over
the rounds; every stream's total and a few streams' bytes are checked after the timed loops.  One JSON line per case, written to
--out (a run replaces the file).

    python tests/tools/chain_decoder_timing.py --reps 3 --rounds 3
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from k4os.compression.lz4_amd import corpus  # noqa: E402
from k4os.compression.lz4_amd.device import ChainDecoderDevice, DeviceCodec, _dp  # noqa: E402
from k4os.compression.lz4_amd.encoders import encode_fast_chain_device  # noqa: E402

GiB, K64 = 1 << 30, 65536


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def case(dc, name, S, per, R, base, a, log):
    dev = dc.device
    nb = per // K64
    host = np.resize(base, S * per)
    data = torch.from_numpy(host).to(dev)
    off = np.arange(S, dtype=np.uint64) * np.uint64(per)
    out_len, arena, boff, nblk, _ = encode_fast_chain_device(dc, data, off, np.full(S, per, np.int64), K64, 0, allow_copy=False)
    torch.cuda.synchronize()
    assert (nblk == nb).all() and bool((out_len > 0).all())
    del data
    rec_off = torch.from_numpy(boff.astype(np.int64)).to(dev)
    rec_len = out_len.contiguous()                                           # int32 > 0: the uint32 length words, bit 31 clear
    out = torch.empty(S * per + 64, dtype=torch.uint8, device=dev)
    s_idx = torch.arange(S, dtype=torch.int64, device=dev)
    steps = [(s_idx * nb + k, s_idx * per + k * K64) for k in range(0, nb, R)]
    n_rec = torch.full((S,), R, dtype=torch.int32, device=dev)
    cap = torch.full((S,), R * K64, dtype=torch.int64, device=dev)
    rec_out = torch.empty(S * nb, dtype=torch.int32, device=dev)
    total = torch.empty(S, dtype=torch.int64, device=dev)
    cd = ChainDecoderDevice([(1, K64, 0)] * S, dc)

    def runs():
        cd.reset()
        for first, d_off in steps:
            cd.run(arena, rec_off, rec_len, None, first, n_rec, rec_out, total, out, d_off, cap)

    first0, o_off = s_idx * nb, s_idx * per
    nblk_d = torch.full((S,), nb, dtype=torch.int32, device=dev)
    bsize = torch.full((S,), K64, dtype=torch.int32, device=dev)
    chained = torch.ones(S, dtype=torch.uint8, device=dev)
    wcap = torch.full((S,), per, dtype=torch.int64, device=dev)
    wout = torch.empty(S, dtype=torch.int64, device=dev)

    def whole():
        dc.ctx.check(dc.lib.k4lz4_decode_chain_batch_device(dc.ctx.handle, _dp(arena), _dp(rec_off), _dp(rec_len), _dp(first0), _dp(nblk_d), _dp(bsize),
                                                            _dp(chained), _dp(out), _dp(o_off), _dp(wcap), _dp(wout), S, C.c_void_p(dc._stream())))

    tr, tw = [], []
    for _ in range(a.rounds):
        tr.append(timed(runs, a.warmup, a.reps))
        tw.append(timed(whole, a.warmup, a.reps))
    ok = bool((wout.cpu().numpy() == per).all())
    out.zero_()
    runs()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ok &= bool((total.cpu().numpy() == R * K64).all() and (rec_out.cpu().numpy() == K64).all())
    for i in (0, S // 2, S - 1):
        ok &= got[i * per:(i + 1) * per].tobytes() == host[i * per:(i + 1) * per].tobytes()
    t_r, t_w = float(np.median(tr)), float(np.median(tw))
    line = json.dumps({"case": name, "streams": S, "kib_per_stream": per >> 10, "blocks_per_call": R, "calls": len(steps),
                       "runs_ms": round(t_r, 3), "whole_ms": round(t_w, 3), "runs_gibs": round(S * per / GiB / (t_r / 1e3), 2),
                       "whole_gibs": round(S * per / GiB / (t_w / 1e3), 2), "ratio": round(t_w / t_r, 3),
                       "runs_ms_min_max": [round(min(tr), 3), round(max(tr), 3)], "whole_ms_min_max": [round(min(tw), 3), round(max(tw), 3)], "ok": ok})
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="the two sides' windows alternate this many times")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_decoder_timing.txt"))
    a = ap.parse_args()
    dc = DeviceCodec(0)
    base = corpus.silesia_like_blocks(64, 65536, seed=7).reshape(-1)          # the eight corpus classes
    with open(a.out, "w") as log:                                            # one run per file
        case(dc, "256x4MiB_runs_of_1", 256, 4 << 20, 1, base, a, log)
        case(dc, "256x4MiB_runs_of_8", 256, 4 << 20, 8, base, a, log)
        case(dc, "4096x512KiB_runs_of_1", 4096, 512 << 10, 1, base, a, log)


if __name__ == "__main__":
    main()
