#!/usr/bin/env python
"""decode_frames_device on 4096 single-block 64 KiB frames with and without a predefined dictionary, in the same run (DESIGN.md
4.24): the same contents written once against entry 0 of a DictionarySet and once as plain frames, both independent and chained;
the dictionary frames through k4lz4_decode_frames_dictset_device, the plain ones through k4lz4_decode_frames_device and, for the
cost of the call itself, through the dictset call as well.  Device events, warm-up first, median and range over the rounds; the
decoded bytes are checked after the timed loops.  One JSON line per case.

    python tests/tools/frame_dict_timing.py --reps 5 --warmup 2 --rounds 5
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import frame_dict_cases as FC  # noqa: E402
from frame_read_timing import timed, contents_of  # noqa: E402
from k4os.compression.lz4_amd import LZ4Frame, LZ4EncoderSettings, DictionarySet, pack_blocks  # noqa: E402
from k4os.compression.lz4_amd import frames as F  # noqa: E402
from k4os.compression.lz4_amd.device import DeviceCodec  # noqa: E402


def reader(dc, frames, dictionary):
    data, off, _ = pack_blocks([np.frombuffer(f, np.uint8) for f in frames])
    d = torch.from_numpy(data).to(dc.device)
    off_d = torch.from_numpy(off.astype(np.int64)).to(dc.device)
    len_d = torch.tensor([len(f) for f in frames], dtype=torch.int64, device=dc.device)
    size = F.frame_sizes_device(dc, d, off_d, len_d, dictionary=dictionary)[0]
    cap = size.cpu().numpy()
    o_off = np.concatenate(([0], np.cumsum((cap + 15) // 16 * 16)[:-1])).astype(np.int64)
    buf = torch.empty(int(((cap + 15) // 16 * 16).sum()) + 64, dtype=torch.uint8, device=dc.device)
    o_off_d = torch.from_numpy(o_off).to(dc.device)
    state = {}

    def run():
        state["res"] = F.decode_frames_device(dc, d, off_d, len_d, out=(buf, o_off_d, size), raise_errors=False, dictionary=dictionary)

    def ok(contents):
        n, h = state["res"][2].cpu().numpy(), buf.cpu().numpy()
        return all(int(n[f]) == c.size and np.array_equal(h[int(o_off[f]):int(o_off[f]) + c.size], c) for f, c in enumerate(contents))
    return run, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4096)
    args = ap.parse_args()
    dc = DeviceCodec(0)
    E = FC.entries()
    contents = contents_of(args.frames, 65536, 16)
    gib = args.frames * 65536 / (1 << 30)
    with DictionarySet(E, owner=dc) as dset:
        dictionary = (dset, FC.IDS)
        for chain in (False, True):
            s = LZ4EncoderSettings(ChainBlocks=chain)
            distinct = {id(c): c for c in contents}
            made = {}
            for e in (0, -1):
                frames = LZ4Frame.EncodeBatch(list(distinct.values()), s, ctx=dc.ctx, dictionary=dictionary, dict_index=[e] * len(distinct))
                made[e] = dict(zip(distinct.keys(), frames))
            sides = {"dictionary frames, dictset call": reader(dc, [made[0][id(c)] for c in contents], dictionary),
                     "plain frames, dictset call": reader(dc, [made[-1][id(c)] for c in contents], dictionary),
                     "plain frames, plain call": reader(dc, [made[-1][id(c)] for c in contents], None)}
            t = {k: [] for k in sides}
            for _ in range(args.rounds):                       # the sides in alternating windows
                for k, (run, _) in sides.items():
                    t[k].append(timed(run, args.warmup, args.reps))
            out = {"case": "chained" if chain else "independent", "frames": args.frames, "block": 65536}
            for k, (_, ok) in sides.items():
                v = sorted(t[k])
                out[k] = {"ms": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3), "gibs": round(gib / (v[len(v) // 2] / 1e3), 1),
                          "bytes_ok": bool(ok(contents))}
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
