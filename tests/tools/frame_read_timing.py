#!/usr/bin/env python
"""The device frame reader (frames.decode_frames_device -> k4lz4_decode_frames_device) next to the existing path over the same
blocks in the same run: k4lz4_decode_batch_device on a host-built block table (independent blocks), k4lz4_decode_chain_batch_device
(linked frames).  Device events, warm-up first; the decoded bytes are checked after the timed loop.  One JSON line per case.

    python tests/tools/frame_read_timing.py --reps 5 --warmup 2
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
from k4os.compression.lz4_amd import LZ4EncoderSettings, LZ4Codec, corpus  # noqa: E402
from k4os.compression.lz4_amd import frames as F  # noqa: E402
from k4os.compression.lz4_amd.device import DeviceCodec, DeviceBatch  # noqa: E402

MiB = 1 << 20
CLASSES = ["dickens", "mozilla", "xml", "webster", "nci", "samba", "x-ray", "ooffice"]


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


def contents_of(n, size, distinct=8):
    d = [corpus.class_bytes(CLASSES[s % len(CLASSES)], size, 300 + s) for s in range(min(n, distinct))]
    return [d[i % len(d)] for i in range(n)]


def reader(dc, frames_d, foff, flen, total_out):
    """decode_frames_device into a preallocated target (sized once by frame_sizes_device)"""
    size, _ = F.frame_sizes_device(dc, frames_d, foff, flen)
    cap = size.cpu().numpy()
    o_off = np.concatenate(([0], np.cumsum((cap + 15) // 16 * 16)[:-1])).astype(np.int64)
    buf = torch.empty(int(((cap + 15) // 16 * 16).sum()) + 64, dtype=torch.uint8, device=dc.device)
    o_off_d = torch.from_numpy(o_off).to(dc.device)
    foff_d = torch.from_numpy(np.asarray(foff, np.int64)).to(dc.device)
    flen_d = flen if isinstance(flen, torch.Tensor) else torch.from_numpy(np.asarray(flen, np.int64)).to(dc.device)
    state = {}

    def run():
        state["res"] = F.decode_frames_device(dc, frames_d, foff_d, flen_d, out=(buf, o_off_d, size), raise_errors=False)
    return run, state


def check(state, contents):
    buf, o_off, o_len = state["res"]
    n = o_len.cpu().numpy()
    h = buf.cpu().numpy()
    o_off = o_off.cpu().numpy() if isinstance(o_off, torch.Tensor) else o_off
    return all(int(n[f]) == c.size and np.array_equal(h[int(o_off[f]):int(o_off[f]) + c.size], c) for f, c in enumerate(contents))


def block_table(frames_h, foff, flen):
    rows = []
    for f in range(len(foff)):
        info = F.parse_frame(frames_h[int(foff[f]):int(foff[f]) + int(flen[f])])
        for o, l in zip(info.block_off, info.block_len):
            rows.append((int(foff[f]) + o, l, info.descriptor.BlockSize))
    return rows


def batch_baseline(dc, frames_d, rows):
    comp = [(o, l, bs) for o, l, bs in rows if not l & 0x80000000]
    src = DeviceBatch(frames_d, torch.tensor([o for o, _, _ in comp], dtype=torch.int64, device=dc.device),
                      torch.tensor([l for _, l, _ in comp], dtype=torch.int32, device=dc.device))
    dst = DeviceBatch.empty_slots(np.array([bs for _, _, bs in comp], np.int64), dc.device)
    out = dc.new_out_len(src.n)
    return (lambda: dc.decode(src, dst, out)), len(comp), len(rows) - len(comp)


def case_independent(dc, args, nf, mib, bs, bsum, csum, label):
    contents = contents_of(nf, mib * MiB)
    data_h = np.concatenate(contents)
    off = np.arange(nf, dtype=np.int64) * (mib * MiB)
    ln = np.full(nf, mib * MiB, np.int64)
    data = torch.from_numpy(data_h).to(dc.device)
    s = LZ4EncoderSettings(BlockSize=bs, BlockChecksum=bsum, ContentChecksum=csum)
    frames_d, foff, flen = F.encode_frames_device(dc, data, off, ln, s)
    del data
    run, state = reader(dc, frames_d, foff, flen, int(ln.sum()))
    t_frames = timed(run, args.warmup, args.reps)
    ok = check(state, contents)
    rows = block_table(frames_d.cpu().numpy(), foff, flen.cpu().numpy())
    base, ncomp, nraw = batch_baseline(dc, frames_d, rows)
    t_base = timed(base, args.warmup, args.reps)
    gib = float(ln.sum()) / (1 << 30)
    return {"case": label, "frames": nf, "frame_mib": mib, "block": bs, "block_checksum": bsum, "content_checksum": csum,
            "blocks": len(rows), "raw_blocks": nraw, "frames_ms": round(t_frames, 3), "frames_gibs": round(gib / (t_frames / 1e3), 2),
            "decode_batch_ms": round(t_base, 3), "decode_batch_gibs": round(gib * ncomp / max(len(rows), 1) / (t_base / 1e3), 2),
            "ratio": round(t_base * len(rows) / max(ncomp, 1) / t_frames, 3), "bytes_ok": ok}


def case_linked(dc, args, nf, mib):
    from test_frame_layer import LZ4F
    lz = LZ4F()
    distinct = contents_of(16, mib * MiB)
    enc = [lz.compress(c, 4, True, False, False, False) for c in distinct]
    contents = [distinct[i % 16] for i in range(nf)]
    frames = [enc[i % 16] for i in range(nf)]
    flen = np.array([len(f) for f in frames], np.int64)
    foff = np.concatenate(([0], np.cumsum((flen + 15) // 16 * 16)[:-1])).astype(np.int64)
    frames_h = np.zeros(int(((flen + 15) // 16 * 16).sum()) + 64, np.uint8)
    for f, fr in enumerate(frames):
        frames_h[int(foff[f]):int(foff[f]) + len(fr)] = np.frombuffer(fr, np.uint8)
    frames_d = torch.from_numpy(frames_h).to(dc.device)
    run, state = reader(dc, frames_d, foff, flen, nf * mib * MiB)
    t_frames = timed(run, args.warmup, args.reps)
    ok = check(state, contents)
    rows = block_table(frames_h, foff, flen)
    per = len(rows) // nf
    dev = dc.device
    blk_off = torch.tensor([o for o, _, _ in rows], dtype=torch.int64, device=dev)
    blk_len = torch.tensor([l for _, l, _ in rows], dtype=torch.int64, device=dev).to(torch.int32)
    first = torch.arange(nf, dtype=torch.int64, device=dev) * per
    nblk = torch.full((nf,), per, dtype=torch.int32, device=dev)
    bsz = torch.full((nf,), 65536, dtype=torch.int32, device=dev)
    chained = torch.ones(nf, dtype=torch.uint8, device=dev)
    dst = torch.empty(nf * mib * MiB + 64, dtype=torch.uint8, device=dev)
    d_off = torch.arange(nf, dtype=torch.int64, device=dev) * (mib * MiB)
    d_cap = torch.full((nf,), mib * MiB, dtype=torch.int64, device=dev)
    t_base = timed(lambda: dc.decode_chain(frames_d, blk_off, blk_len, first, nblk, bsz, chained, dst, d_off, d_cap), args.warmup, args.reps)
    gib = nf * mib * MiB / (1 << 30)
    return {"case": "liblz4 linked", "frames": nf, "frame_mib": mib, "block": 65536, "blocks": len(rows),
            "frames_ms": round(t_frames, 3), "frames_gibs": round(gib / (t_frames / 1e3), 2), "decode_chain_ms": round(t_base, 3),
            "decode_chain_gibs": round(gib / (t_base / 1e3), 2), "ratio": round(t_base / t_frames, 3), "bytes_ok": ok}


def case_one_big(dc, args, mib):
    part = corpus.class_bytes("dickens", 4 * MiB, 77)
    content = np.tile(part, mib // 4)
    data = torch.from_numpy(content).to(dc.device)
    frames_d, foff, flen = F.encode_frames_device(dc, data, np.zeros(1, np.int64), np.array([content.size], np.int64),
                                                  LZ4EncoderSettings(BlockSize=65536))
    del data
    run, state = reader(dc, frames_d, foff, flen, content.size)
    t_frames = timed(run, args.warmup, args.reps)
    ok = check(state, [content])
    rows = block_table(frames_d.cpu().numpy(), foff, flen.cpu().numpy())
    base, ncomp, _ = batch_baseline(dc, frames_d, rows)
    t_base = timed(base, args.warmup, args.reps)
    gib = content.size / (1 << 30)
    return {"case": "one big frame", "frames": 1, "frame_mib": mib, "block": 65536, "blocks": len(rows),
            "frames_ms": round(t_frames, 3), "frames_gibs": round(gib / (t_frames / 1e3), 2), "decode_batch_ms": round(t_base, 3),
            "decode_batch_gibs": round(gib / (t_base / 1e3), 2), "ratio": round(t_base / t_frames, 3), "bytes_ok": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dc = DeviceCodec(0)
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)
    for bsum, csum, label in ((False, False, "independent"), (True, False, "independent + block checksums"),
                              (False, True, "independent + content checksum")):
        emit(case_independent(dc, args, 64, 4, 65536, bsum, csum, label))
    emit(case_linked(dc, args, 1024, 1))
    emit(case_single(dc, args))
    emit(case_one_big(dc, args, 256))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def case_single(dc, args):
    nf, size = 4096, 65536
    contents = contents_of(nf, size, 16)
    data = torch.from_numpy(np.concatenate(contents)).to(dc.device)
    off = np.arange(nf, dtype=np.int64) * size
    frames_d, foff, flen = F.encode_frames_device(dc, data, off, np.full(nf, size, np.int64), LZ4EncoderSettings(BlockSize=65536))
    del data
    run, state = reader(dc, frames_d, foff, flen, nf * size)
    t_frames = timed(run, args.warmup, args.reps)
    ok = check(state, contents)
    rows = block_table(frames_d.cpu().numpy(), foff, flen.cpu().numpy())
    base, ncomp, nraw = batch_baseline(dc, frames_d, rows)
    t_base = timed(base, args.warmup, args.reps)
    gib = nf * size / (1 << 30)
    return {"case": "single-block frames", "frames": nf, "frame_kib": size >> 10, "block": 65536, "blocks": len(rows), "raw_blocks": nraw,
            "frames_ms": round(t_frames, 3), "frames_gibs": round(gib / (t_frames / 1e3), 2), "decode_batch_ms": round(t_base, 3),
            "decode_batch_gibs": round(gib * ncomp / len(rows) / (t_base / 1e3), 2), "ratio": round(t_base * len(rows) / max(ncomp, 1) / t_frames, 3),
            "bytes_ok": ok}


if __name__ == "__main__":
    main()
