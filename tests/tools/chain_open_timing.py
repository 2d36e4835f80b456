#!/usr/bin/env python
"""Opening chained streams from a prepared dictionary set, timed on one GPU.  chain_encoder_timing.py's protocol:
device events around the calls, warm-up first, the two sides in alternating windows, median and range over the rounds; what both
sides leave is compared after the timed loops.

  decoders   S decoders (B = 1 KiB) opened from one 64 KiB entry: k4lz4_chain_decoder_open_dictset_device, one launch, next to the
             only way there was before it, in the same run -- RESET plus one Inject record of 64 KiB per stream from device memory
             (k4lz4_chain_decode_batch_device twice)
  encoders   S chained fast encoders opened from the same entry (80 KiB to move per stream: the kept bytes and the table); there
             is no earlier way to compare with, so the time is absolute
  gain       the gain case of tests/chain_prime_cases.py, compressed / uncompressed over its four 1 KiB blocks with and without the
             dictionary, from the committed goldens (the witness's sizes: no GPU in it)

One JSON line per row, written to --out (a run replaces the file).

    python tests/tools/chain_open_timing.py --streams 1024 --reps 5 --rounds 5
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
from k4os.compression.lz4_amd import DictionarySet  # noqa: E402
from k4os.compression.lz4_amd.device import ChainDecoderDevice, ChainEncoderDevice, DeviceCodec  # noqa: E402

K1, K64 = 1024, 65536


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


def stats(t):
    return round(float(np.median(t)), 4), [round(min(t), 4), round(max(t), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="the two sides' windows alternate this many times")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_open_timing.txt"))
    a = ap.parse_args()
    import chain_prime_cases as PC
    S = a.streams
    dc = DeviceCodec(0)
    dev = dc.device
    dictionary = PC.gain_dictionary()
    dset = DictionarySet([dictionary], owner=dc)
    rows = []

    # ---- decoders: open from the set | RESET + Inject from device memory
    new, old = ChainDecoderDevice([(1, K1, 0)] * S, dc), ChainDecoderDevice([(1, K1, 0)] * S, dc)
    idx = torch.zeros(S, dtype=torch.int32, device=dev)
    out_new = torch.empty(S, dtype=torch.int64, device=dev)
    out_old = torch.empty(S, dtype=torch.int64, device=dev)
    src = torch.from_numpy(dictionary).to(dev)
    rec_off = torch.zeros(S, dtype=torch.int64, device=dev)
    rec_len = torch.full((S,), K64 - (1 << 31), dtype=torch.int32, device=dev)      # 65536 with bit 31: Inject
    first = torch.arange(S, dtype=torch.int64, device=dev)
    n_rec = torch.ones(S, dtype=torch.int32, device=dev)
    rec_out = torch.empty(S, dtype=torch.int32, device=dev)

    def open_new():
        new.open(idx, dset, out_new)

    def open_old():
        old.reset(out_old)
        old.run(src, rec_off, rec_len, None, first, n_rec, rec_out, out_old)

    tn, to = [], []
    for _ in range(a.rounds):
        tn.append(timed(open_new, a.warmup, a.reps))
        to.append(timed(open_old, a.warmup, a.reps))
    torch.cuda.synchronize()
    ok = bool((out_new == K64).all().item() and (out_old == K64).all().item() and torch.equal(new.query(), old.query()))
    so, sn = old.store_off.cpu().numpy(), new.store_off.cpu().numpy()
    for i in (0, S // 2, S - 1):
        ok &= torch.equal(new.store[int(sn[i]):int(sn[i]) + 256 + K64], old.store[int(so[i]):int(so[i]) + 256 + K64])
        ok &= new.store[int(sn[i]) + 256:int(sn[i]) + 256 + K64].cpu().numpy().tobytes() == dictionary.tobytes()
    (m_new, r_new), (m_old, r_old) = stats(tn), stats(to)
    rows.append({"row": "decoders", "streams": S, "entry_bytes": K64, "open_ms": m_new, "open_ms_min_max": r_new, "reset_inject_ms": m_old,
                 "reset_inject_ms_min_max": r_old, "reset_inject_over_open": round(m_old / m_new, 3),
                 "open_gibs": round(S * K64 / (1 << 30) / (m_new / 1e3), 1), "ok": ok})
    del new, old

    # ---- encoders: chained fast streams, kept bytes and table
    enc = ChainEncoderDevice([(True, 0, K1, 0)] * S, dc)
    eidx = np.zeros(S, np.int32)
    te = [timed(lambda: enc.open(eidx, dset), a.warmup, a.reps) for _ in range(a.rounds)]
    torch.cuda.synchronize()
    want = dset.state(0)[0]
    ok = all(r.pointer == K64 and r.dictSize == K64 and r.currentOffset == K64 for r in enc.records[:S])
    base = enc._base - enc.store.data_ptr()
    for i in (0, S // 2, S - 1):
        at = int(base + enc.store_off[i])
        table = enc.store[at:at + 16384].cpu().numpy().view("<u4")
        ring = enc.store[at + 16640:at + 16640 + K64].cpu().numpy()
        ok &= bool(np.array_equal(table, want["hashTable"]) and ring.tobytes() == dictionary.tobytes())
    m_enc, r_enc = stats(te)
    rows.append({"row": "encoders", "streams": S, "bytes_per_stream": K64 + 16384 + 16, "open_ms": m_enc, "open_ms_min_max": r_enc,
                 "open_gibs": round(S * (K64 + 16400) / (1 << 30) / (m_enc / 1e3), 1), "ok": bool(ok)})

    # ---- the gain case, from the goldens
    with open(os.path.join(ROOT, "tests", "golden", "chain_prime_cases.json")) as f:
        gain = {c["name"]: c for c in json.load(f)["cases"]}["gain"]["streams"]
    case = PC.case("gain")
    for s, (setting, e) in enumerate(zip(case.settings, case.idx)):
        sizes = [abs(o) for o in gain[s]["calls"][0][0]]
        rows.append({"row": "gain", "level": setting[1], "primed": e >= 0, "block_bytes": sizes, "compressed_over_uncompressed": round(sum(sizes) / (4 * K1), 3)})
    dset.close()
    with open(a.out, "w") as log:                                              # one run per file
        for r in rows:
            line = json.dumps(r)
            print(line, flush=True)
            log.write(line + "\n")


if __name__ == "__main__":
    main()
