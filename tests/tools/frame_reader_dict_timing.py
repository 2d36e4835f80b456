#!/usr/bin/env python
"""The incremental frame reader with a dictionary set on the device (FrameReaderDevice with dictionary=,
k4lz4_frame_read_dictset_batch_device) next to two yardsticks in the same run, in alternating windows: the plain
reader on plain frames of the same contents, and decode_frames_device with the set on the same dictionary frames.  The first and
third case of tests/tools/frame_reader_timing.py with frames written against a 64 KiB entry: S independent single-frame sources of
R x C bytes read in R calls of C bytes, and Sc chained ones.  Device events around the whole sequence (the reader's host work and
its stores' allocation included), warm-up first; median and range over the windows; every stream's byte count and a few streams'
bytes are checked after the timed loops.  One JSON line per case.

    python tests/tools/frame_reader_dict_timing.py --streams 1024 --chain-streams 256 --reads 8 --kib 512 --reps 3 --warmup 1 --rounds 5
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from k4os.compression.lz4_amd import DictionarySet, corpus  # noqa: E402
from k4os.compression.lz4_amd.device import DeviceCodec  # noqa: E402
from k4os.compression.lz4_amd.frames import (FrameReaderDevice, FrameWriterDevice, LZ4EncoderSettings, decode_frames_device,  # noqa: E402
                                             encode_frames_device)

GiB = 1 << 30
DICT_ID = 7


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


def plain_chained(dc, data, off, S, per):
    """chained L00 frames without a dictionary: one write and a close per stream through the incremental writer"""
    w = FrameWriterDevice(dc, S, LZ4EncoderSettings(ChainBlocks=True))
    o1, f1, l1 = w.write(data, off[:S], np.full(S, per, np.int64))
    o2, f2, l2 = w.close()
    l1h, l2h = l1.cpu().numpy(), l2.cpu().numpy()
    flen = l1h + l2h
    foff = np.concatenate(([0], np.cumsum((flen + 15) // 16 * 16)))[:-1]
    frames = torch.zeros(int(foff[-1] + flen[-1]) + 64, dtype=torch.uint8, device=dc.device)
    for i in range(S):
        frames[int(foff[i]):int(foff[i]) + int(l1h[i])] = o1[int(f1[i]):int(f1[i]) + int(l1h[i])]
        frames[int(foff[i]) + int(l1h[i]):int(foff[i]) + int(flen[i])] = o2[int(f2[i]):int(f2[i]) + int(l2h[i])]
    return frames, foff, flen


def case(dc, name, with_dict, plain, dictionary, S, R, C, host, a):
    per = R * C
    dev = dc.device
    out = torch.empty(S * per + 64, dtype=torch.uint8, device=dev)
    o_off = torch.arange(S, dtype=torch.int64, device=dev) * per
    cap = torch.full((S,), per, dtype=torch.int64, device=dev)
    counts = torch.full((S,), C, dtype=torch.int64, device=dev)
    steps = [o_off + k * C for k in range(R)]
    last = {}

    def reader(frames, d, key):        # (a reader is made per repetition: its stores' allocation and the reset launch are timed too)
        def run():
            rd = FrameReaderDevice(dc, *frames, maxBlockSize=65536, dictionary=d)
            for k in range(R):
                last[key + "_len"] = rd.read(counts, out=(out, steps[k]), max_count=C if a.fast else 0)[2]
            last[key] = rd
        return run

    def verify(key):
        q = last[key].query().cpu().numpy()
        got = out.cpu().numpy()
        ok = bool((q[:, 0] == per).all() and (last[key + "_len"].cpu().numpy() == C).all())
        for i in (0, S // 2, S - 1):
            ok &= got[i * per:(i + 1) * per].tobytes() == host[i * per:(i + 1) * per].tobytes()
        return ok, q

    sides = {"dict_reader": reader(with_dict, dictionary, "dict"), "plain_reader": reader(plain, None, "plain"),
             "whole_dict": lambda: decode_frames_device(dc, *with_dict, out=(out, o_off, cap), raise_errors=False, dictionary=dictionary)}
    t = {k: [] for k in sides}
    ok = True
    for _ in range(a.rounds):           # the three sides alternate; the spread is over the rounds
        for k, fn in sides.items():
            t[k].append(timed(fn, a.warmup, a.reps))
            if k != "whole_dict":
                ok &= verify(k.split("_")[0])[0]
    q = last["dict"].query().cpu().numpy()
    total = lambda x: int((x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).sum())  # noqa: E731
    row = {"case": name, "streams": S, "reads": R, "kib": C >> 10, "ok": ok, "fast_blocks": int(q[:, 6].sum()), "handed_back": int(q[:, 7].sum()),
           "blocks": int(q[:, 4].sum()), "dict_frame_bytes": total(with_dict[2]), "plain_frame_bytes": total(plain[2])}
    for k, v in t.items():
        row[k + "_ms"] = round(float(np.median(v)), 3)
        row[k + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
        row[k + "_gibs"] = round(S * per / GiB / (float(np.median(v)) / 1e3), 2)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--chain-streams", type=int, default=256)
    ap.add_argument("--reads", type=int, default=8)
    ap.add_argument("--kib", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="the sides' windows alternate this many times")
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
    entry = corpus.silesia_like_blocks(1, 65536, seed=8).reshape(-1)          # a full 64 KiB window of the same kind of bytes
    with DictionarySet([entry], owner=dc) as dset:
        d = (dset, [DICT_ID])
        lens = np.full(S, per, np.int64)
        with_dict = encode_frames_device(dc, data, off, lens, LZ4EncoderSettings(), dictionary=d, dict_index=[0] * S)
        plain = encode_frames_device(dc, data, off, lens, LZ4EncoderSettings())
        case(dc, "independent_l00", with_dict, plain, d, S, R, C, host, a)
        del with_dict, plain
        Sc = min(a.chain_streams, S)
        with_dict = encode_frames_device(dc, data, off[:Sc], lens[:Sc], LZ4EncoderSettings(ChainBlocks=True), dictionary=d, dict_index=[0] * Sc)
        plain = plain_chained(dc, data, off, Sc, per)
        case(dc, "chained_l00", with_dict, plain, d, Sc, R, C, host, a)


if __name__ == "__main__":
    main()
