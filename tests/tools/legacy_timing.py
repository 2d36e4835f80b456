#!/usr/bin/env python
"""The legacy formats on the device next to the existing paths over the same chunks in the same run: decode_legacy_streams_device
against k4lz4_decode_batch_device on a host-built chunk table, encode_legacy_streams_device against k4lz4_encode_batch_device on
the same chunks, wrap_device against k4lz4_pickle_batch_device on the same messages.  Device events, warm-up first; outputs are
checked after the timed loops.  One JSON line per case.

    python tests/tools/legacy_timing.py --streams 64 --mib 64 --reps 3 --warmup 1
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from k4os.compression.lz4_amd import LZ4Codec, corpus  # noqa: E402
from k4os.compression.lz4_amd import legacy as L  # noqa: E402
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


def varint(b, pos):
    v, c = 0, 0
    while True:
        x = int(b[pos]); pos += 1
        v += (x & 0x7F) << c; c += 7
        if not x & 0x80 or c >= 64:
            return v, pos


def chunk_table(stream: np.ndarray, base: int):
    """host walk of a valid stream -> [(payload offset, C, U, compressed)]"""
    pos, out = 0, []
    while pos < stream.size:
        fl, pos = varint(stream, pos)
        u, pos = varint(stream, pos)
        c = u
        if fl & 1:
            c, pos = varint(stream, pos)
        out.append((base + pos, c, u, fl & 1))
        pos += c
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    dc = DeviceCodec(0)
    dev = dc.device
    n, per, bs = a.streams, a.mib * MiB, a.block
    # content: eight corpus classes, each stream a different class and offset (generated once, copied on the device)
    base = torch.from_numpy(np.concatenate([corpus.class_bytes(c, per // 8 + 4096, 7).reshape(-1) for c in CLASSES])).to(dev)
    content = torch.empty(n * per, dtype=torch.uint8, device=dev)
    for i in range(n):
        sh = (i * 7919) % 4096
        content[i * per:(i + 1) * per] = base[sh:sh + per] if base.numel() >= sh + per else base[:per]
    off = np.arange(n, dtype=np.int64) * per
    ln = np.full(n, per, np.int64)
    gib = n * per / float(1 << 30)
    res = []

    # ---- encode
    bound = np.full(n, dc.lib.k4lz4_legacy_stream_bound(per, bs), np.int64)
    buf, s_off, s_len = L.encode_legacy_streams_device(dc, content, off, ln, block_size=bs)
    t_enc = timed(lambda: L.encode_legacy_streams_device(dc, content, off, ln, block_size=bs, out=(buf, s_off, bound)), a.warmup, a.reps)
    # (the streams are checked below: they decode back to the content)
    nch = per // bs
    c_off = (np.arange(n * nch, dtype=np.int64) * bs)
    src = DeviceBatch(content, torch.from_numpy(c_off).to(dev), torch.full((n * nch,), bs, dtype=torch.int32, device=dev))
    cap = LZ4Codec.MaximumOutputSize(bs)
    dst = DeviceBatch.empty_slots(np.full(n * nch, cap), dev)
    t_bare_enc = timed(lambda: dc.encode(src, dst), a.warmup, a.reps)
    res.append(dict(case="encode", streams=n, mib=a.mib, block=bs, legacy_ms=round(t_enc, 3), bare_ms=round(t_bare_enc, 3),
                    legacy_gibs=round(gib / t_enc * 1e3, 2), bare_gibs=round(gib / t_bare_enc * 1e3, 2), ratio=round(t_bare_enc / t_enc, 3)))

    # ---- decode
    lens = s_len.cpu().numpy()
    host = buf.cpu().numpy()
    rows = []
    for i in range(n):
        rows += chunk_table(host[int(s_off[i]):int(s_off[i]) + int(lens[i])], int(s_off[i]))
    streams = buf
    out = torch.empty(n * per + 64, dtype=torch.uint8, device=dev)
    o_off = off.copy()
    t_dec = timed(lambda: L.decode_legacy_streams_device(dc, streams, s_off, lens, out=(out, o_off, ln), raise_errors=False),
                  a.warmup, a.reps)
    _, _, olen = L.decode_legacy_streams_device(dc, streams, s_off, lens, out=(out, o_off, ln), raise_errors=False)
    ok_dec = bool((olen.cpu().numpy() == per).all()) and bool(torch.equal(out[:n * per], content))
    comp = [r for r in rows if r[3]]
    cs = DeviceBatch(streams, torch.tensor([r[0] for r in comp], dtype=torch.int64, device=dev),
                     torch.tensor([r[1] for r in comp], dtype=torch.int32, device=dev))
    out2 = DeviceBatch.empty_slots(np.array([r[2] for r in comp]), dev)
    t_bare_dec = timed(lambda: dc.decode(cs, out2), a.warmup, a.reps)
    res.append(dict(case="decode", streams=n, mib=a.mib, block=bs, chunks=len(rows), compressed=len(comp), legacy_ms=round(t_dec, 3),
                    bare_ms=round(t_bare_dec, 3), legacy_gibs=round(gib / t_dec * 1e3, 2), bare_gibs=round(gib / t_bare_dec * 1e3, 2),
                    ratio=round(t_bare_dec / t_dec, 3), ok=ok_dec))

    # ---- wrap against pickle, every chunk a message
    wl = torch.full((n * nch,), bs, dtype=torch.int32, device=dev)
    wcap = np.full(n * nch, bs + 8)
    wdst = DeviceBatch.empty_slots(wcap, dev)
    t_wrap = timed(lambda: L.wrap_device(dc, content, c_off, wl, out=(wdst.data, wdst.off, wdst.length)), a.warmup, a.reps)
    pdst = DeviceBatch.empty_slots(np.full(n * nch, bs + 5), dev)
    t_pickle = timed(lambda: dc.pickle(src, pdst), a.warmup, a.reps)
    wb, wo, wlen = L.wrap_device(dc, content, c_off, wl, out=(wdst.data, wdst.off, wdst.length))
    ub, uo, ulen, udec = L.unwrap_device(dc, wb, wdst.off, wlen)
    ok_wrap = bool((ulen.cpu().numpy() == bs).all()) and bool((udec.cpu().numpy() == bs).all())
    if ok_wrap:
        ok_wrap = all(torch.equal(ub[int(uo[k]):int(uo[k]) + bs], content[k * bs:(k + 1) * bs]) for k in range(n * nch))
    res.append(dict(case="wrap", messages=n * nch, bytes=bs, wrap_ms=round(t_wrap, 3), pickle_ms=round(t_pickle, 3),
                    wrap_gibs=round(gib / t_wrap * 1e3, 2), pickle_gibs=round(gib / t_pickle * 1e3, 2), ratio=round(t_pickle / t_wrap, 3),
                    ok=ok_wrap))
    for r in res:
        print(json.dumps(r), flush=True)
    if not (ok_dec and ok_wrap):
        sys.exit(1)


if __name__ == "__main__":
    main()
