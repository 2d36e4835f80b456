"""Timing of the fed LZ4Stream reader on one GPU -> profiles/legacy_feed_timing.txt.

Workload: 4.16's 64 contents of 64 MiB in 1 MiB chunks.  Code under test: LegacyFedReaderDevice, every stream fed in eight equal
pieces with one read per piece (each read asks for everything that is left, so it takes the piece's whole chunks and is left starved
with the piece's tail in the stash), with the direct path and with the general reader alone (max_count = 0); and the host form
k4lz4_legacy_read_fed_batch the same way on a smaller set.  Yardstick on the same streams in the same session, windows alternating
with the code under test: the whole-source reader (k4lz4_legacy_read_batch_device / k4lz4_legacy_read_batch) with eight reads per
stream.  The yardstick is never compared with anything but itself: the table reports each pairwise ratio's median and spread.  The
timed direct-path case must have BATCHED == CHUNKS, or the figure would be the general reader's.
Usage: python tests/tools/legacy_feed_timing.py [--streams 64] [--mib 64] [--pairs 5] [--host-streams 8] [--host-mib 16]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from k4os.compression.lz4_amd import corpus                       # noqa: E402
from k4os.compression.lz4_amd import legacy as L                   # noqa: E402
from k4os.compression.lz4_amd.device import DeviceCodec            # noqa: E402

PIECES = 8


def once(fn, host=False):
    fn()                                                              # a warm run in front of every timed one
    torch.cuda.synchronize()
    if host:
        t = time.perf_counter()
        fn()
        return time.perf_counter() - t
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def streams_of(dc, n, size, B):
    one = corpus.class_bytes("dickens", size, 1)
    data = torch.from_numpy(np.tile(one, n)).to(dc.device)
    for i in range(n):                                                # distinct contents: a different byte every 64 KiB
        data[i * size:(i + 1) * size:65536] = i
    off = np.arange(n, dtype=np.int64) * size
    sbuf, soff, slen = L.encode_legacy_streams_device(dc, data, off, np.full(n, size, np.int64), False, B)
    torch.cuda.synchronize()
    return sbuf, np.asarray(soff, np.int64), slen.cpu().numpy().astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--host-streams", type=int, default=8)
    ap.add_argument("--host-mib", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "legacy_feed_timing.txt"))
    args = ap.parse_args()
    B = 1 << 20
    dc = DeviceCodec(0)
    dev = dc.device
    rows, checks = [], []

    def cuts_of(slen):
        return [slen * k // PIECES for k in range(PIECES + 1)]

    # ---- device forms
    n, size = args.streams, args.mib << 20
    sbuf, soff, slen = streams_of(dc, n, size, B)
    out = torch.empty(n * size + 64, dtype=torch.uint8, device=dev)
    off = np.arange(n, dtype=np.int64) * size
    cuts = cuts_of(slen)
    p_off = [torch.from_numpy(soff + cuts[k]).to(dev) for k in range(PIECES)]
    p_len = [torch.from_numpy(cuts[k + 1] - cuts[k]).to(dev) for k in range(PIECES)]
    p_fin = [torch.full((n,), int(k == PIECES - 1), dtype=torch.int64, device=dev) for k in range(PIECES)]
    last = {}

    def fed(max_count):
        def run():
            rd = L.LegacyFedReaderDevice(dc, n, B)
            doff = torch.from_numpy(off).to(dev)
            counts = torch.full((n,), size, dtype=torch.int64, device=dev)
            for k in range(PIECES):
                _, _, o, _, _ = rd.read(sbuf, p_off[k], p_len[k], p_fin[k], counts, out=(out, doff), max_count=max_count)
                doff, counts = doff + o, counts - o
            last["rd"], last["left"] = rd, counts
        return run

    def whole():
        rd = L.LegacyReaderDevice(dc, sbuf, soff, slen, maxBlockSize=B)
        counts = torch.full((n,), size // PIECES, dtype=torch.int64, device=dev)
        doff = torch.from_numpy(off).to(dev)
        for k in range(PIECES):
            rd.read(counts, out=(out, doff + k * (size // PIECES)), max_count=size // PIECES)

    def compare(name, test, yard, total, host=False):
        t, y = [], []
        for _ in range(args.pairs):                                   # windows alternate: yardstick, code under test
            y.append(once(yard, host))
            t.append(once(test, host))
        ratios = [b / a for a, b in zip(t, y)]
        rows.append(f"{name:52s} {total / statistics.median(t):8.2f} GiB/s   yardstick {total / statistics.median(y):8.2f} GiB/s   "
                    f"ratio {statistics.median(ratios):.2f}x (min {min(ratios):.2f}, max {max(ratios):.2f}, {args.pairs} pairs)")

    total = n * size / 2 ** 30
    compare("device: 8 pieces, one read each (direct path)", fed(size), whole, total)
    q = last["rd"].query().cpu().numpy()
    ok = bool((q[:, L.LSQ_BATCHED] == q[:, L.LSQ_CHUNKS]).all() and (q[:, L.LSQ_CHUNKS] == size // B).all() and
              (q[:, L.LSQ_HANDED_BACK] == 0).all() and (last["left"].cpu().numpy() == 0).all())
    checks.append(f"direct path: BATCHED == CHUNKS == {size // B} on every stream, HANDED_BACK == 0, everything delivered: {ok}")
    compare("device: 8 pieces, one read each (general reader alone)", fed(0), whole, total)
    q = last["rd"].query().cpu().numpy()
    checks.append(f"general reader alone: BATCHED == 0: {bool((q[:, L.LSQ_BATCHED] == 0).all())}, everything delivered: "
                  f"{bool((last['left'].cpu().numpy() == 0).all())}")
    del out, sbuf

    # ---- host forms, on a smaller set (every call moves its bytes between host and device)
    hn, hsize = args.host_streams, args.host_mib << 20
    hbuf, hoff, hlen = streams_of(dc, hn, hsize, B)
    src = hbuf.cpu().numpy()
    hcuts = cuts_of(hlen)
    lib = dc.lib
    fed_rec, rec = L.legacy_reader_record(B, lib, fed=True), L.legacy_reader_record(B, lib)
    st_off = (np.arange(hn, dtype=np.uint64) * np.uint64(fed_rec.storeBytes)).astype(np.uint64)
    store = torch.zeros(hn * int(fed_rec.storeBytes) + 64, dtype=torch.uint8, device=dev)
    dst = np.zeros(hn * hsize + 64, np.uint8)
    d0 = (np.arange(hn, dtype=np.uint64) * np.uint64(hsize)).astype(np.uint64)
    p = lambda a: a.ctypes.data  # noqa: E731
    res = [np.zeros(hn, np.int64) for _ in range(3)]
    zero = np.zeros(hn, np.int64)

    def host_fed():
        dc.ctx.check(lib.k4lz4_legacy_read_fed_batch(dc.ctx.handle, C.byref(fed_rec), store.data_ptr(), p(st_off), None, None, None, None, None,
                                                     None, p(zero), p(res[0]), p(res[1]), p(res[2]), hn, L.LREAD_RESET, 0))
        doff, counts = d0.copy(), np.full(hn, hsize, np.int64)
        for k in range(PIECES):
            so = (hoff + hcuts[k]).astype(np.uint64)
            sl = (hcuts[k + 1] - hcuts[k]).astype(np.uint64)
            fin = np.full(hn, int(k == PIECES - 1), np.int64)
            dc.ctx.check(lib.k4lz4_legacy_read_fed_batch(dc.ctx.handle, C.byref(fed_rec), store.data_ptr(), p(st_off), p(src), p(so), p(sl),
                                                         p(fin), p(dst), p(doff), p(counts), p(res[0]), p(res[1]), p(res[2]), hn,
                                                         L.LREAD_READ, 0))
            doff, counts = doff + res[0].astype(np.uint64), counts - res[0]
        last["left"] = counts

    def host_whole():
        dc.ctx.check(lib.k4lz4_legacy_read_batch(dc.ctx.handle, C.byref(rec), store.data_ptr(), p(st_off), None, None, None, None, None, p(zero),
                                                 p(res[0]), hn, L.LREAD_RESET, 0))
        so, sl = hoff.astype(np.uint64), hlen.astype(np.uint64)
        counts = np.full(hn, hsize // PIECES, np.int64)
        for k in range(PIECES):
            doff = d0 + np.uint64(k * (hsize // PIECES))
            dc.ctx.check(lib.k4lz4_legacy_read_batch(dc.ctx.handle, C.byref(rec), store.data_ptr(), p(st_off), p(src), p(so), p(sl), p(dst),
                                                     p(doff), p(counts), p(res[0]), hn, L.LREAD_READ, 0))

    compare(f"host: {hn} x {args.host_mib} MiB, 8 pieces, one read each", host_fed, host_whole, hn * hsize / 2 ** 30, host=True)
    checks.append(f"host form: everything delivered: {bool((last['left'] == 0).all())}")
    text = (f"legacy_feed_timing: {n} streams x {args.mib} MiB, 1 MiB chunks, {PIECES} equal pieces, {torch.cuda.get_device_name(0)}\n"
            "yardstick: the whole-source reader, 8 reads per stream (the whole source is present at every call)\n" +
            "\n".join(rows) + "\n" + "\n".join(checks) + "\n")
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
