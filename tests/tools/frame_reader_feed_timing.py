#!/usr/bin/env python
"""The fed frame reader (FrameFedReaderDevice, k4lz4_frame_read_fed_batch_device) next to the whole-source reader of 4.14
(FrameReaderDevice) on the same frames in the same run: 4.14's four cases, the source fed in P equal pieces with one read per
piece.  Every fed read asks for all that is left of the content, so it delivers the records that are whole in what it has been
given and starves; the unconsumed rest and the next piece are one contiguous range of the frame in device memory, and the ranges
are computed on the device from `consumed`, so the sequence never waits for the host.  The whole-source reader reads the same
content in R reads of C bytes.  Device events around the whole sequence (host work included), windows alternating; every stream's
byte count and a few streams' bytes are checked after the timed loops.  Then the host forms (LZ4FrameFedReaderBatch against
LZ4FrameReaderBatch, wall clock, fewer streams): the fed form sends every source byte up once, the whole-source form once per
read.  One JSON line per case.

    python tests/tools/frame_reader_feed_timing.py --streams 1024 --reads 8 --kib 512 --reps 10 --rounds 3
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from k4os.compression.lz4_amd import corpus  # noqa: E402
from k4os.compression.lz4_amd.device import DeviceCodec  # noqa: E402
from k4os.compression.lz4_amd.frames import (FrameFedReaderDevice, FrameReaderDevice, FrameWriterDevice, LZ4EncoderSettings,  # noqa: E402
                                             LZ4FrameFedReaderBatch, LZ4FrameReaderBatch, encode_frames_device)

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
    per, P, dev = R * C, a.pieces, dc.device
    out = torch.empty(S * per + 64, dtype=torch.uint8, device=dev)
    o_off = torch.arange(S, dtype=torch.int64, device=dev) * per
    counts = torch.full((S,), C, dtype=torch.int64, device=dev)
    steps = [o_off + k * C for k in range(R)]
    foff_d = torch.from_numpy(np.asarray(foff, np.int64)).to(dev)
    flen_d = torch.as_tensor(flen, dtype=torch.int64).to(dev)          # (the frame encoder hands the lengths back on the device)
    ends = [flen_d * (k + 1) // P for k in range(P)]
    fin = [torch.full((S,), int(k == P - 1), dtype=torch.int64, device=dev) for k in range(P)]
    last = {}

    def fed():                         # (a reader is made per repetition, as in 4.14's measurement)
        rd = FrameFedReaderDevice(dc, S, maxBlockSize=65536)
        taken = torch.zeros(S, dtype=torch.int64, device=dev)
        given = torch.zeros(S, dtype=torch.int64, device=dev)
        for k in range(P):
            _, _, n, consumed, need = rd.read(frames, foff_d + taken, ends[k] - taken, fin[k], per - given, out=(out, o_off + given),
                                              max_count=per if a.fast else 0)
            taken = taken + consumed
            given = given + n
        last["fed"], last["given"], last["need"] = rd, given, need

    def whole():
        rd = FrameReaderDevice(dc, frames, foff, flen, maxBlockSize=65536)
        for k in range(R):
            last["len"] = rd.read(counts, out=(out, steps[k]), max_count=C if a.fast else 0)[2]
        last["whole"] = rd

    def check(tag):
        got = out.cpu().numpy()
        ok = True
        for i in (0, S // 2, S - 1):
            ok &= got[i * per:(i + 1) * per].tobytes() == host[i * per:(i + 1) * per].tobytes()
        return ok
    tf, tw, ok = [], [], True
    for _ in range(a.rounds):
        out.zero_()
        tf.append(timed(fed, a.warmup, a.reps))
        ok &= check("fed") and bool((last["given"] == per).all()) and bool((last["need"] == 0).all())
        out.zero_()
        tw.append(timed(whole, a.warmup, a.reps))
        ok &= check("whole") and bool((last["len"] == C).all())
    t_f, t_w = float(np.median(tf)), float(np.median(tw))
    q = last["fed"].query().cpu().numpy()
    ok &= bool((q[:, 0] == per).all())
    print(json.dumps({"case": name, "form": "device", "streams": S, "pieces": P, "reads": R, "kib": C >> 10, "fed_ms": round(t_f, 3),
                      "whole_source_ms": round(t_w, 3), "fed_gibs": round(S * per / GiB / (t_f / 1e3), 2),
                      "whole_source_gibs": round(S * per / GiB / (t_w / 1e3), 2), "ratio": round(t_w / t_f, 3),
                      "fed_ms_min_max": [round(min(tf), 3), round(max(tf), 3)], "whole_source_ms_min_max": [round(min(tw), 3), round(max(tw), 3)],
                      "fast_blocks": int(q[:, 6].sum()), "handed_back": int(q[:, 7].sum()), "blocks": int(q[:, 4].sum()), "ok": bool(ok)}), flush=True)


def host_case(name, frames_h, content, R, C, a):
    """the host forms: every call of the whole-source reader sends the sources up, the fed reader sends each piece once"""
    S, P, per = len(frames_h), a.pieces, R * C

    def fed():
        rd = LZ4FrameFedReaderBatch(S, maxBlockSize=65536)
        got = [b""] * S
        for k in range(P):
            rd.Feed([f[len(f) * k // P:len(f) * (k + 1) // P] for f in frames_h], final=[k == P - 1] * S)
            got = [g + b for g, b in zip(got, rd.Read([per - len(g) for g in got]))]
        return got

    def whole():
        rd = LZ4FrameReaderBatch(frames_h, maxBlockSize=65536)
        got = [b""] * S
        for _ in range(R):
            got = [g + b for g, b in zip(got, rd.Read([C] * S))]
        return got
    tf, tw, ok = [], [], True
    for _ in range(a.rounds):
        for fn, acc in ((fed, tf), (whole, tw)):
            fn()
            t = time.perf_counter()
            for _ in range(a.host_reps):
                got = fn()
            acc.append((time.perf_counter() - t) / a.host_reps * 1e3)
            ok &= all(g == c for g, c in zip(got, content))
    t_f, t_w = float(np.median(tf)), float(np.median(tw))
    print(json.dumps({"case": name, "form": "host", "streams": S, "pieces": P, "reads": R, "kib": C >> 10, "fed_ms": round(t_f, 3),
                      "whole_source_ms": round(t_w, 3), "ratio": round(t_w / t_f, 3), "fed_ms_min_max": [round(min(tf), 3), round(max(tf), 3)],
                      "whole_source_ms_min_max": [round(min(tw), 3), round(max(tw), 3)], "ok": bool(ok)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reads", type=int, default=8)
    ap.add_argument("--pieces", type=int, default=8)
    ap.add_argument("--kib", type=int, default=512)
    ap.add_argument("--chain-streams", type=int, default=256)
    ap.add_argument("--small-streams", type=int, default=4096)
    ap.add_argument("--host-streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="fed and whole-source windows alternate this many times")
    ap.add_argument("--fast", type=int, default=1, help="0: maxCount = 0, the general readers alone")
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
        if name == "independent_l00" and a.host_streams:
            fh, fo, fl = frames.cpu().numpy(), np.asarray(foff, np.int64), np.asarray(flen.cpu().numpy() if isinstance(flen, torch.Tensor) else flen, np.int64)
            Sh = min(a.host_streams, S)
            host_case(name, [fh[int(fo[i]):int(fo[i]) + int(fl[i])].tobytes() for i in range(Sh)],
                      [host[i * per:(i + 1) * per].tobytes() for i in range(Sh)], R, C, a)
        del frames
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
    Ss, Cs = a.small_streams, 65536
    pers = 8 * Cs
    offs = np.arange(Ss, dtype=np.int64) * pers
    frames, foff, flen = encode_frames_device(dc, data, offs, np.full(Ss, pers, np.int64), LZ4EncoderSettings())
    case(dc, "small_reads_64k", frames, foff, flen, Ss, 8, Cs, host, a)


if __name__ == "__main__":
    main()
