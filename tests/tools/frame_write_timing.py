#!/usr/bin/env python
"""The incremental frame writer on the device (FrameWriterDevice, k4lz4_frame_write_batch_device) next to whole-frame encoding of the
same contents in the same run: S streams x W writes x C bytes, then a close, against encode_frames_device over the S whole contents
(independent L00 blocks, with content checksums off and on), and the chained-L00 writer against encode_fast_chain_device.  Device
events around the whole sequence (the writers' host work included), warm-up first; a few streams' bytes are checked against the
whole-frame encoders' after the timed loops.  One JSON line per case.

    python tests/tools/frame_write_timing.py --streams 1024 --writes 8 --kib 512 --reps 3 --warmup 1
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from k4os.compression.lz4_amd import corpus  # noqa: E402
from k4os.compression.lz4_amd.device import DeviceCodec  # noqa: E402
from k4os.compression.lz4_amd.encoders import encode_fast_chain_device  # noqa: E402
from k4os.compression.lz4_amd.frames import FrameWriterDevice, LZ4EncoderSettings, encode_frames_device  # noqa: E402

GiB = 1 << 30


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--writes", type=int, default=8)
    ap.add_argument("--kib", type=int, default=512)
    ap.add_argument("--chain-streams", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    dc = DeviceCodec(0)
    S, W, C = a.streams, a.writes, a.kib << 10
    per = W * C
    # contents: stream s is its own slice of a corpus-like buffer; write k of stream s = bytes [k*C, (k+1)*C) of it
    base = corpus.silesia_like_blocks(64, 65536, seed=7).reshape(-1)
    host = np.resize(base, S * per)
    data = torch.from_numpy(host).to(dc.device)
    off = np.arange(S, dtype=np.int64) * per
    total = S * per

    def writer(settings, streams):
        def run():
            w = FrameWriterDevice(dc, streams, settings)
            outs = []
            for k in range(W):
                outs.append(w.write(data, off[:streams] + k * C, np.full(streams, C, np.int64)))
            outs.append(w.close())
            return outs
        return run

    for name, s in (("independent_l00", LZ4EncoderSettings()), ("independent_l00_content_checksum", LZ4EncoderSettings(ContentChecksum=True))):
        wr = writer(s, S)
        whole = lambda: encode_frames_device(dc, data, off, np.full(S, per, np.int64), s)  # noqa: E731
        t_w = timed(wr, a.warmup, a.reps)
        t_e = timed(whole, a.warmup, a.reps)
        outs = wr()
        fr, foff, flen = whole()
        torch.cuda.synchronize()
        ok = True
        fl = flen.cpu().numpy()
        frh = fr.cpu().numpy()
        parts = [(o.cpu().numpy(), oo, ol.cpu().numpy()) for o, oo, ol in outs]
        for i in (0, S // 2, S - 1):
            got = b"".join(p[0][int(p[1][i]):int(p[1][i]) + int(p[2][i])].tobytes() for p in parts)
            ok &= got == frh[int(foff[i]):int(foff[i]) + int(fl[i])].tobytes()
        print(json.dumps({"case": name, "streams": S, "writes": W, "kib": a.kib, "writer_ms": round(t_w, 3), "whole_ms": round(t_e, 3),
                          "writer_gibs": round(total / GiB / (t_w / 1e3), 2), "whole_gibs": round(total / GiB / (t_e / 1e3), 2),
                          "ratio": round(t_e / t_w, 3), "ok": bool(ok)}), flush=True)
    # content checksum alone: the one-shot XXH32 of every content, for the resumable kernel's share (the difference of the two rows above)
    t_x = timed(lambda: dc.xxh32(data, torch.from_numpy(off).to(dc.device), torch.full((S,), per, dtype=torch.int64, device=dc.device)),
                a.warmup, a.reps)
    print(json.dumps({"case": "xxh32_one_shot", "streams": S, "bytes": per, "ms": round(t_x, 3), "gibs": round(total / GiB / (t_x / 1e3), 2)}),
          flush=True)
    # chained L00: the writer against encode_fast_chain_device over the same contents
    Sc = min(a.chain_streams, S)
    s = LZ4EncoderSettings(ChainBlocks=True)
    wr = writer(s, Sc)
    whole = lambda: encode_fast_chain_device(dc, data, off[:Sc], np.full(Sc, per, np.int64), 65536)  # noqa: E731
    t_w = timed(wr, a.warmup, a.reps)
    t_e = timed(whole, a.warmup, a.reps)
    print(json.dumps({"case": "chained_l00", "streams": Sc, "writes": W, "kib": a.kib, "writer_ms": round(t_w, 3), "whole_ms": round(t_e, 3),
                      "writer_gibs": round(Sc * per / GiB / (t_w / 1e3), 2), "whole_gibs": round(Sc * per / GiB / (t_e / 1e3), 2),
                      "ratio": round(t_e / t_w, 3)}), flush=True)


if __name__ == "__main__":
    main()
