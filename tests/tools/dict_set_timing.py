#!/usr/bin/env python
"""What a dictionary set saves per call: k4lz4_encode_dict_batch / k4lz4_encode_dict_hc_batch, which load their list
on every call, against k4lz4_encode_dictset_batch on a set created once, in the same run on the same messages -- one shared 64 KiB
dictionary (synthetic dickens), batches of 256 / 4096 / 65 536 messages of 1 KiB, levels 0 and 3, the device form and the host form.
A call is timed from the host, from before it is made until its stream has drained (the per-call calls also wait on the host, for
the previous upload of their list, which device events would not see); the two ways take turns, and the figure is the median of 5
turns after a warm-up, with the turns' range beside it.  The per-call call of no messages is the load step alone (list upload and
load kernel); k4lz4_dict_set_create is timed once per step.  Every step (one batch size at one level) runs in a child process under
a time limit of its own, and the first one that fails ends the run.  Writes profiles/dict_set_timing.txt.

    python tests/tools/dict_set_timing.py [--counts 256 4096 65536] [--levels 0 3] [--reps 5] [--limit 240] [--out profiles/dict_set_timing.txt]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZE = 1024


def messages(n):
    """n messages of 1 KiB and a 64 KiB dictionary cut from the same class: the messages' text is not the dictionary's"""
    import dict_encode_cases as DC
    base = DC.synthetic("dickens", (8 << 20) + SIZE + DC.K64, 3)
    dictionary = base[:DC.K64].copy()
    pool = base[DC.K64:]
    starts = np.random.default_rng(5).integers(0, pool.size - SIZE, n)
    return np.ascontiguousarray(pool[starts[:, None] + np.arange(SIZE)[None, :]].reshape(-1)), dictionary


def step(n, level, reps):
    import torch
    import dict_encode_cases as DC
    from k4os.compression.lz4_amd import DICT_FAST, DICT_HC, DictionarySet, LZ4Codec, LZ4Level
    from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec

    src, dictionary = messages(n)
    cap = DC.bound(SIZE)
    dc = DeviceCodec(0)
    dev = dc.device
    soff, slen = np.arange(n, dtype=np.uint64) * SIZE, np.full(n, SIZE, np.int32)
    doff, dcap = np.arange(n, dtype=np.uint64) * cap, np.full(n, cap, np.int32)
    idx = np.zeros(n, np.int32)
    dict_off, dict_len = np.zeros(1, np.uint64), np.array([dictionary.size], np.int32)
    s = DeviceBatch.from_host(src, soff, slen, dev)
    d = DeviceBatch(torch.empty(n * cap + 64, dtype=torch.uint8, device=dev), torch.from_numpy(doff.view(np.int64)).to(dev), torch.from_numpy(dcap).to(dev))
    none = DeviceBatch(s.data, s.off[:0], s.length[:0]), DeviceBatch(d.data, d.off[:0], d.length[:0])
    t_idx, t_dict = torch.from_numpy(idx).to(dev), torch.from_numpy(dictionary).to(dev)
    out_t = dc.new_out_len(n)
    h_dst = np.empty(n * cap + 64, np.uint8)
    lv = LZ4Level(level)

    t0 = time.perf_counter()
    ds = DictionarySet(dictionary, dict_off, dict_len, families=DICT_HC if level >= 3 else DICT_FAST, owner=dc)
    create_ms = (time.perf_counter() - t0) * 1e3

    def sync():
        dc.ctx.synchronize(dc._stream())

    ways = {
        ("device", "per call"): lambda: (dc.encode_dict(s, d, t_idx, t_dict, dict_off, dict_len, out_t, lv), sync()),
        ("device", "set"): lambda: (dc.encode_dictset(s, d, t_idx, ds, out_t, lv), sync()),
        ("host", "per call"): lambda: LZ4Codec.EncodeDictBatchPacked(src, soff, slen, h_dst, doff, dcap, idx, dictionary, dict_off, dict_len, lv, 0, dc.ctx),
        ("host", "set"): lambda: LZ4Codec.EncodeDictBatchPacked(src, soff, slen, h_dst, doff, dcap, idx, ds, None, None, lv, 0, dc.ctx),
        ("device", "per call, no messages"): lambda: (dc.encode_dict(none[0], none[1], t_idx[:0], t_dict, dict_off, dict_len, out_t[:0], lv), sync()),
    }
    times = {k: [] for k in ways}
    sizes = {}
    for turn in range(reps + 1):                            # the first turn is the warm-up
        for k, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            ms = (time.perf_counter() - t0) * 1e3
            if turn:
                times[k].append(ms)
            if k[0] == "host":
                sizes[k] = int(np.asarray(r).clip(min=0).sum())
            elif "no messages" not in k[1]:
                sizes[k] = int(out_t.clamp(min=0).sum().item())
    assert len(set(sizes.values())) == 1, f"the ways differ in the bytes they write: {sizes}"
    info = ds.info
    ds.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = [f"level {level}: {n} x {SIZE} B messages, one 64 KiB dictionary (synthetic dickens); ms per call, host clock to stream drained, "
             f"median of {reps} alternating turns after a warm-up [min .. max]; sum(C)/sum(U) {next(iter(sizes.values())) / (n * SIZE):.3f}",
             f"  k4lz4_dict_set_create (once): {create_ms:.3f} ms; set: {info['device_bytes']} device bytes, load launches {info['fast_loads'] + info['hc_loads']}"]
    for form in ("device", "host"):
        a, b = med[(form, "per call")], med[(form, "set")]
        for way in ("per call", "set"):
            v = times[(form, way)]
            lines.append(f"  {form:6s} form, {way:8s} {med[(form, way)]:9.3f}  [{min(v):.3f} .. {max(v):.3f}]")
        lines.append(f"  {form:6s} form, saved    {a - b:9.3f}  ({100.0 * (a - b) / a:.1f} % of the per-call call)")
    v = times[("device", "per call, no messages")]
    lines.append(f"  the load step alone (the per-call call of no messages, device form) {med[('device', 'per call, no messages')]:.3f}  [{min(v):.3f} .. {max(v):.3f}]")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", nargs="*", type=int, default=[256, 4096, 65536])
    ap.add_argument("--levels", nargs="*", type=int, default=[0, 3])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_set_timing.txt"))
    ap.add_argument("--step", nargs=2, type=int, metavar=("COUNT", "LEVEL"), help="run one step in this process and print its lines")
    a = ap.parse_args()
    if a.step:
        print("\n".join(step(a.step[0], a.step[1], a.reps)))
        return 0
    text = []
    for n in a.counts:
        for level in a.levels:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", str(n), str(level), "--reps", str(a.reps)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"step {n} x level {level}: no result within {a.limit} s; stopping", file=sys.stderr)
                return 124
            if r.returncode != 0:
                print(f"step {n} x level {level} failed with {r.returncode}; stopping\n{r.stderr[-4000:]}", file=sys.stderr)
                return r.returncode if r.returncode > 0 else 1
            print(r.stdout, flush=True)
            text += [r.stdout.rstrip("\n"), ""]
            with open(a.out, "w") as f:                     # what is measured so far is kept
                f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
