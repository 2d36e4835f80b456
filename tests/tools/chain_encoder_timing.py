#!/usr/bin/env python
"""Many open ILZ4Encoders advanced per call on the device (ChainEncoderDevice, k4lz4_chain_encode_batch_device) next to the
whole-content encoders on the same bytes in the same run: S streams x W calls x C bytes, one ALLOW_COPY record per 64 KiB block (the
bytes divide into whole blocks, so no flush is needed), against encode_batch_device over the same 64 KiB blocks (independent L00), k4lz4_encode_fast_chain_batch_device
(chained L00) and k4lz4_encode_hc_chain_batch_device (chained L03).  frame_write_timing.py's protocol: device events around the whole
call sequence (the host's planning included), warm-up, the two sides in alternating windows, median and range over the rounds.  The
per-call side's total output is checked against the whole side's after the timed loops.  One JSON line per case, appended to
profiles/chain_encoder_timing.txt with --record.

    python tests/tools/chain_encoder_timing.py --streams 1024 --calls 8 --kib 512 --chain-streams 256 --reps 3 --rounds 3 --record
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
from k4os.compression.lz4_amd.device import ChainEncoderDevice, DeviceBatch, DeviceCodec, _dp  # noqa: E402
from k4os.compression.lz4_amd.encoders import encode_fast_chain_device  # noqa: E402

GiB = 1 << 30
B = 65536


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--kib", type=int, default=512)
    ap.add_argument("--chain-streams", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--record", action="store_true")
    a = ap.parse_args()
    dc = DeviceCodec(0)
    dev = dc.device
    W, Cb = a.calls, a.kib << 10
    per = W * Cb
    base = corpus.silesia_like_blocks(64, 65536, seed=7).reshape(-1)
    lines = []
    for name, S, chaining, level in (("independent_l00", a.streams, False, 0), ("chained_l00", a.chain_streams, True, 0),
                                     ("chained_l03", a.chain_streams, True, 3)):
        data = torch.from_numpy(np.resize(base, S * per)).to(dev)
        off = np.arange(S, dtype=np.uint64) * np.uint64(per)
        slot = Cb // B * (B + B // 255 + 16)
        dst = torch.empty(S * slot + 64, dtype=torch.uint8, device=dev)
        doff, dcap = np.arange(S, dtype=np.uint64) * np.uint64(slot), np.full(S, slot, np.uint64)
        nrec = Cb // B
        loaded = torch.empty(S * nrec, dtype=torch.int32, device=dev)
        rout = torch.empty(S * nrec, dtype=torch.int32, device=dev)
        olen = [torch.empty(S, dtype=torch.int64, device=dev) for _ in range(W)]
        first, count = np.arange(S, dtype=np.uint64) * np.uint64(nrec), np.full(S, nrec, np.uint32)
        rlen, rflags = np.full(S * nrec, B, np.uint32), np.full(S * nrec, 2, np.uint32)
        enc = ChainEncoderDevice([(chaining, level, B, 0)] * S, dc)

        def per_call():
            enc.reset()
            for k in range(W):
                roff = (off[:, None] + np.uint64(k * Cb) + (np.arange(nrec, dtype=np.uint64) * np.uint64(B))[None, :]).reshape(-1)
                enc.run(data, roff, rlen, rflags, first, count, dst, doff, dcap, loaded, rout, olen[k])

        nb = S * per // B
        if not chaining:
            src = DeviceBatch(data, torch.from_numpy((np.arange(nb, dtype=np.uint64) * np.uint64(B)).view(np.int64)).to(dev), torch.full((nb,), B, dtype=torch.int32, device=dev))
            wdst = DeviceBatch.empty_slots(np.full(nb, B + B // 255 + 16, np.int32), dev)
            wout = dc.new_out_len(nb)
            whole = lambda: dc.encode(src, wdst, wout, 0, 64)  # noqa: E731
        elif level == 0:
            res = {}

            def whole():
                res["out"] = encode_fast_chain_device(dc, data, off, np.full(S, per, np.int64), B)[0]
            wout = None
        else:
            wout = torch.empty(nb, dtype=torch.int32, device=dev)
            arena = torch.empty(nb * (B + B // 255 + 16) + 64, dtype=torch.uint8, device=dev)
            slen, bs, ex, dl = np.full(S, per, np.int64), np.full(S, B, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
            aoff = np.arange(S, dtype=np.uint64) * np.uint64(per // B * (B + B // 255 + 16))

            def whole():
                dc.ctx.check(dc.lib.k4lz4_encode_hc_chain_batch_device(dc.ctx.handle, _dp(data), off.ctypes.data, slen.ctypes.data, bs.ctypes.data,
                                                                       ex.ctypes.data, dl.ctypes.data, S, _dp(arena), aoff.ctypes.data, _dp(wout), nb,
                                                                       level, 64, C.c_void_p(dc._stream())))
        per_call(); whole()
        torch.cuda.synchronize()
        tp, tw = [], []
        for _ in range(a.rounds):
            tp.append(window(per_call, a.reps))
            tw.append(window(whole, a.reps))
        torch.cuda.synchronize()
        got = sum(int(o.sum().item()) for o in olen)
        w = wout if wout is not None else res["out"]
        want = int(w.to(torch.int64).abs().sum().item())
        total = S * per
        mp, mw = float(np.median(tp)), float(np.median(tw))
        lines.append(json.dumps({"case": name, "streams": S, "calls": W, "kib": a.kib, "per_call_ms": round(mp, 3), "per_call_range": [round(min(tp), 3), round(max(tp), 3)],
                                 "whole_ms": round(mw, 3), "whole_range": [round(min(tw), 3), round(max(tw), 3)],
                                 "per_call_gibs": round(total / GiB / (mp / 1e3), 2), "whole_gibs": round(total / GiB / (mw / 1e3), 2),
                                 "ratio": round(mw / mp, 3), "ok": bool(got == want)}))
        print(lines[-1], flush=True)
        del data, dst, enc
    if a.record:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "chain_encoder_timing.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
