#!/usr/bin/env python
"""The incremental frame reader on the device (FrameReaderDevice, k4lz4_frame_read_batch_device) next to the whole-frame reader
(decode_frames_device) on the same frames in the same run: S single-frame sources of R x C bytes read in R calls of C bytes
(independent L00 frames of 64 KiB blocks, content checksums off and on; chained L00 frames from FrameWriterDevice), and the
many-small-reads case.  Device events around the whole sequence (the reader's host work included), warm-up first; every stream's
byte count and a few streams' bytes are checked after the timed loops.  One JSON line per case.

    python tests/tools/frame_reader_timing.py --streams 1024 --reads 8 --kib 512 --reps 3 --warmup 1
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
from k4os.compression.lz4_amd.frames import (FrameReaderDevice, FrameWriterDevice, LZ4EncoderSettings, decode_frames_device,  # noqa: E402
                                             encode_frames_device)

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


def case(dc, name, frames, foff, flen, S, R, C, host, a):
    per = R * C
    dev = dc.device
    out = torch.empty(S * per + 64, dtype=torch.uint8, device=dev)
    o_off = torch.arange(S, dtype=torch.int64, device=dev) * per
    cap = torch.full((S,), per, dtype=torch.int64, device=dev)
    counts = torch.full((S,), C, dtype=torch.int64, device=dev)
    steps = [o_off + k * C for k in range(R)]
    last = {}

    def reader():                      # (a reader is made per repetition: its stores' allocation and the reset launch are timed too)
        rd = FrameReaderDevice(dc, frames, foff, flen, maxBlockSize=65536)
        for k in range(R):
            last["len"] = rd.read(counts, out=(out, steps[k]), max_count=C if a.fast else 0)[2]
        last["rd"] = rd

    whole = lambda: decode_frames_device(dc, frames, foff, flen, out=(out, o_off, cap), raise_errors=False)  # noqa: E731
    # reader and whole-frame runs alternate; the spread is over the rounds
    tr, tw = [], []
    for _ in range(a.rounds):
        tr.append(timed(reader, a.warmup, a.reps))
        tw.append(timed(whole, a.warmup, a.reps))
    t_r, t_w = float(np.median(tr)), float(np.median(tw))
    q = last["rd"].query().cpu().numpy()
    got = out.cpu().numpy()
    ok = bool((q[:, 0] == per).all() and (last["len"].cpu().numpy() == C).all())
    for i in (0, S // 2, S - 1):
        ok &= got[i * per:(i + 1) * per].tobytes() == host[i * per:(i + 1) * per].tobytes()
    print(json.dumps({"case": name, "streams": S, "reads": R, "kib": C >> 10, "reader_ms": round(t_r, 3), "whole_ms": round(t_w, 3),
                      "reader_gibs": round(S * per / GiB / (t_r / 1e3), 2), "whole_gibs": round(S * per / GiB / (t_w / 1e3), 2),
                      "ratio": round(t_w / t_r, 3), "reader_ms_min_max": [round(min(tr), 3), round(max(tr), 3)],
                      "whole_ms_min_max": [round(min(tw), 3), round(max(tw), 3)], "fast_blocks": int(q[:, 6].sum()), "handed_back": int(q[:, 7].sum()),
                      "in_place_blocks": int(q[:, 5].sum()), "blocks": int(q[:, 4].sum()), "ok": ok}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reads", type=int, default=8)
    ap.add_argument("--kib", type=int, default=512)
    ap.add_argument("--chain-streams", type=int, default=256)
    ap.add_argument("--small-streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="reader and whole-frame windows alternate this many times")
    ap.add_argument("--fast", type=int, default=1, help="0: maxCount = 0, the general reader alone")
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    dc = DeviceCodec(0)
    S, R, C = a.streams, a.reads, a.kib << 10
    per = R * C
    base = corpus.silesia_like_blocks(64, 65536, seed=7).reshape(-1)          # the eight corpus classes
    host = np.resize(base, S * per)
    data = torch.from_numpy(host).to(dc.device)
    off = np.arange(S, dtype=np.int64) * per
    for name, s in (("independent_l00", LZ4EncoderSettings()), ("independent_l00_content_checksum", LZ4EncoderSettings(ContentChecksum=True))):
        frames, foff, flen = encode_frames_device(dc, data, off, np.full(S, per, np.int64), s)
        case(dc, name, frames, foff, flen, S, R, C, host, a)
        del frames
    # chained L00 frames: one write and a close per stream through the incremental writer
    Sc = min(a.chain_streams, S)
    w = FrameWriterDevice(dc, Sc, LZ4EncoderSettings(ChainBlocks=True))
    o1, f1, l1 = w.write(data, off[:Sc], np.full(Sc, per, np.int64))
    o2, f2, l2 = w.close()
    l1h, l2h = l1.cpu().numpy(), l2.cpu().numpy()
    flen = l1h + l2h
    foff = np.concatenate(([0], np.cumsum((flen + 15) // 16 * 16)))[:-1]
    frames = torch.zeros(int(foff[-1] + flen[-1]) + 64, dtype=torch.uint8, device=dc.device)
    for i in range(Sc):
        frames[int(foff[i]):int(foff[i]) + int(l1h[i])] = o1[int(f1[i]):int(f1[i]) + int(l1h[i])]
        frames[int(foff[i]) + int(l1h[i]):int(foff[i]) + int(flen[i])] = o2[int(f2[i]):int(f2[i]) + int(l2h[i])]
    case(dc, "chained_l00", frames, foff, flen, Sc, R, C, host, a)
    del frames, o1, o2
    # many small reads: every read is one 64 KiB block
    Ss, Cs = a.small_streams, 65536
    pers = 8 * Cs
    offs = np.arange(Ss, dtype=np.int64) * pers
    frames, foff, flen = encode_frames_device(dc, data, offs, np.full(Ss, pers, np.int64), LZ4EncoderSettings())
    case(dc, "small_reads_64k", frames, foff, flen, Ss, 8, Cs, host, a)


if __name__ == "__main__":
    main()
