"""The two-step fast encoder dealt by the cost sample with its own table (k4lz4_parse.hpp, ParseCost; FastTable<3>) and the stable
order (k4lz4_encode_fast.hpp, order_by_bucket), on the GPU: the order only says which wave takes which block, so a ragged batch of 33
blocks around every length at which the code takes another path, and one of 1025 short blocks -- five workgroups of the order launch,
65 of the cost launch --, give the oracle's bytes block for block, by default and with the old order behind K4LZ4_NO_PCOST (a fresh
process per switch: the switches are read when a context is made), and the same bytes when the batch is encoded a second time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from k4os.compression.lz4_amd import LZ4Codec, corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = 2048                       # PCOST_FIT.sample
LENGTHS = [0, 1, 12, 13, 127, 128, SAMPLE - 1, SAMPLE, SAMPLE + 1, 4096, 65535, 65546, 65547]
CLASSES = ("dickens", "mozilla")            # a text class and a binary class

CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec
out = {}
dc = DeviceCodec(0)
for path in sys.argv[2:]:
    z = np.load(path)
    src = DeviceBatch.from_host(z["data"], z["off"], z["lens"], dc.device)
    runs = []
    for rep in range(2):
        comp = DeviceBatch.empty_slots(z["caps"], dc.device, fill=0xCD)
        clen = dc.encode(src, comp)
        torch.cuda.synchronize()
        runs.append((comp.data.cpu().numpy(), comp.off.cpu().numpy(), clen.cpu().numpy()))
    ch, coff, cl = runs[0]
    bad = []
    for i in range(z["lens"].size):
        w = z["want"][z["want_off"][i]:z["want_off"][i + 1]]
        if int(cl[i]) != w.size or not np.array_equal(ch[coff[i]:coff[i] + w.size], w) or not (ch[coff[i] + w.size:coff[i] + z["caps"][i]] == 0xCD).all():
            bad.append(i)
    out[path] = {"bad": bad, "same_twice": bool(np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2]))}
print(json.dumps(out))
"""


def _save(path, blocks, oracle):
    lens = np.array([b.size for b in blocks], np.int32)
    off = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.uint64)
    want = [np.frombuffer(oracle.encode(b), np.uint8) for b in blocks]
    want_off = np.concatenate([[0], np.cumsum([w.size for w in want])]).astype(np.int64)
    np.savez(path, data=np.concatenate(blocks), off=off, lens=lens, caps=np.array([LZ4Codec.MaximumOutputSize(int(n)) for n in lens], np.int64),
             want=np.concatenate(want), want_off=want_off)


@pytest.fixture(scope="module")
def batches(oracle, tmp_path_factory):
    """the oracle's bytes of both batches, computed once"""
    d = tmp_path_factory.mktemp("sample_table_order")
    base = [corpus.class_bytes(c, 1 << 20, 91) for c in CLASSES]
    rng = np.random.default_rng(92)
    ragged = []
    for i in range(33):
        ln = LENGTHS[(i * 5 + 3) % len(LENGTHS)]
        o = (i * 7919 * 64) % ((1 << 20) - ln)
        ragged.append(base[i % 2][o:o + ln])
    assert set(b.size for b in ragged) == set(LENGTHS)
    short = []
    for i, ln in enumerate(rng.integers(256, 4097, 1025)):
        o = (i * 7919 * 64) % ((1 << 20) - int(ln))
        short.append(base[i % 2][o:o + int(ln)])
    paths = [str(d / "ragged33.npz"), str(d / "short1025.npz")]
    _save(paths[0], ragged, oracle)
    _save(paths[1], short, oracle)
    return paths


@pytest.mark.parametrize("env_vars", [{}, {"K4LZ4_NO_PCOST": "1"}], ids=["default", "no_pcost"])
def test_both_batches_give_the_oracles_bytes_twice(batches, env_vars):
    env = {k: v for k, v in os.environ.items() if k not in ("K4LZ4_NO_PCOST", "K4LZ4_PCOST", "K4LZ4_PCOST_FIT")}
    env.update(env_vars)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + batches, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stderr[-2000:])
    r = json.loads(lines[-1])
    for path in batches:
        assert r[path]["bad"] == [], (env_vars, os.path.basename(path), r[path]["bad"][:10])
        assert r[path]["same_twice"], (env_vars, os.path.basename(path))
