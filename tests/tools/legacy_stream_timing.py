"""Timing of LZ4Stream piece by piece on one GPU -> profiles/legacy_stream_timing.txt.

Workload: 4.12's 64 contents of 64 MiB in 1 MiB chunks.  Code under test: LegacyWriterDevice with 8 writes and a close per stream;
LegacyReaderDevice with 8 reads per stream, with one read per chunk, and the general kernel alone (max_count = 0).  Yardsticks on
the same contents in the same session, windows alternating with the code under test: encode_legacy_streams_device and
decode_legacy_streams_device.  They are never compared with anything but themselves: the table reports each ratio with its spread
over the repetitions.  Usage: python tests/tools/legacy_stream_timing.py [--streams 64] [--mib 64] [--reps 7]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from k4os.compression.lz4_amd import corpus                       # noqa: E402
from k4os.compression.lz4_amd import legacy as L                   # noqa: E402
from k4os.compression.lz4_amd.device import DeviceCodec            # noqa: E402


def timed(fn, warm=2, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "legacy_stream_timing.txt"))
    args = ap.parse_args()
    n, size, B = args.streams, args.mib << 20, 1 << 20
    dc = DeviceCodec(0)
    one = corpus.class_bytes("dickens", size, 1)
    data = torch.from_numpy(np.tile(one, n)).to(dc.device)
    for i in range(n):                                                # distinct contents: a different byte every 64 KiB
        data[i * size:(i + 1) * size:65536] = i
    off = np.arange(n, dtype=np.int64) * size
    lens = np.full(n, size, np.int64)
    total = n * size / 2 ** 30

    def whole_write():
        return L.encode_legacy_streams_device(dc, data, off, lens, False, B)

    def pieces_write():
        wd = L.LegacyWriterDevice(dc, n, False, B)
        step = size // 8
        for k in range(8):
            wd.write(data, off + k * step, np.full(n, step, np.int64))
        wd.close()

    sbuf, soff, slen = whole_write()
    torch.cuda.synchronize()
    slen_h = slen.cpu().numpy()
    out_slots = (torch.empty(n * size + 64, dtype=torch.uint8, device=dc.device), off, lens)

    def whole_read():
        return L.decode_legacy_streams_device(dc, sbuf, soff, slen_h, out=out_slots, raise_errors=False)

    def pieces_read(per_call, max_count=None):
        def run():
            rd = L.LegacyReaderDevice(dc, sbuf, soff, slen_h, maxBlockSize=B)
            counts = torch.full((n,), per_call, dtype=torch.int64, device=dc.device)
            doff = torch.from_numpy(off).to(dc.device)
            for k in range(size // per_call):
                rd.read(counts, out=(out_slots[0], doff + k * per_call), max_count=per_call if max_count is None else max_count)
        return run

    rows = []
    for name, test, yard in (("writer: 8 writes + close", pieces_write, whole_write),
                             ("reader: 8 reads (direct path)", pieces_read(size // 8), whole_read),
                             ("reader: one read per chunk (direct path)", pieces_read(B), whole_read),
                             ("reader: 8 reads (general kernel alone)", pieces_read(size // 8, 0), whole_read)):
        t, y = [], []
        for _ in range(args.reps):                                    # windows alternate: yardstick, code under test
            y += timed(yard, warm=1, reps=1)
            t += timed(test, warm=1, reps=1)
        ratios = [b / a for a, b in zip(t, y)]
        rows.append(f"{name:44s} {total / statistics.median(t):8.2f} GiB/s   yardstick {total / statistics.median(y):8.2f} GiB/s   "
                    f"ratio {statistics.median(ratios):.2f}x (min {min(ratios):.2f}, max {max(ratios):.2f}, {args.reps} pairs)")
    text = f"legacy_stream_timing: {n} streams x {args.mib} MiB, 1 MiB chunks, {torch.cuda.get_device_name(0)}\n" + "\n".join(rows) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
