"""Late blocks first inside k4_parse_kernel (k4lz4_parse.hpp, ParsePace): the waves of a workgroup share their
estimates in LDS and take an issue priority from them.  Nothing but timing depends on it, so every case here is the encoder's
output against the oracle, byte for byte, with the bytes behind every block untouched: with the priorities, without them
(K4LZ4_NO_PACE), and with the threshold above the batch (K4LZ4_PACE_MIN).  The switches are read when a context is made: a fresh
process per switch.  No test asserts a time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from k4os.compression.lz4_amd import LZ4Codec, corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("dickens", "mozilla")            # a text class and a binary class

CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec
z = np.load(sys.argv[2])
dc = DeviceCodec(0)
src = DeviceBatch.from_host(z["data"], z["off"], z["lens"], dc.device)
def check(clen, comp):
    torch.cuda.synchronize()
    return bool(np.array_equal(clen.cpu().numpy(), z["want_len"])) and bool(np.array_equal(comp.data.cpu().numpy()[:z["ref"].size], z["ref"]))
comp = DeviceBatch.empty_slots(z["caps"], dc.device, fill=0xCD)
assert np.array_equal(comp.off.cpu().numpy(), z["coff"])
out = {"equal": check(dc.encode(src, comp), comp)}
if sys.argv[3] == "stamps":
    comp = DeviceBatch.empty_slots(z["caps"], dc.device, fill=0xCD)
    clen, counters = dc.profile(4, src, comp)
    out["equal_stamped"] = check(clen, comp)
    st = counters.cpu().numpy()[:, 11]
    out["placements"] = {int(k): int((st == k).sum()) for k in np.unique(st)}
print(json.dumps(out))
"""


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _save(oracle, tmp_path_factory, name, blocks):
    """the batch, its output slots as DeviceBatch.empty_slots lays them out, and the oracle's bytes in a buffer filled like the slots"""
    lens = np.array([b.size for b in blocks], np.int32)
    off = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.uint64)
    data = np.concatenate(blocks)
    caps = np.array([LZ4Codec.MaximumOutputSize(int(v)) for v in lens], np.int32)
    padded = (caps.astype(np.int64) + 15) // 16 * 16
    coff = np.concatenate([[0], np.cumsum(padded[:-1])]).astype(np.int64)
    ref = np.full(int(padded.sum()), 0xCD, np.uint8)
    want_len = oracle.encode_batch(data, off, lens, ref, coff.astype(np.uint64), caps, threads=16)
    path = str(tmp_path_factory.mktemp(name) / "batch.npz")
    np.savez(path, data=data, off=off, lens=lens, caps=caps, coff=coff, ref=ref, want_len=want_len)
    return path


def _cut(lengths, seed):
    """blocks of the given lengths out of a text and a binary stretch, at offsets that differ from block to block"""
    base = [corpus.class_bytes(c, 4 << 20, seed) for c in CLASSES]
    blocks = []
    for i, ln in enumerate(lengths):
        o = (i * 7919 * 64) % ((4 << 20) - int(ln))
        blocks.append(base[i % 2][o:o + int(ln)])
    return blocks


def _child(path, env_vars, stamps=False):
    env = {k: v for k, v in os.environ.items() if k not in ("K4LZ4_NO_PACE", "K4LZ4_PACE_MIN", "K4LZ4_PACE_QUEUE", "K4LZ4_NO_MIGRATE", "K4LZ4_PARSE_QUEUE")}
    env.update(env_vars)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, path, "stamps" if stamps else "plain"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stderr[-2000:])
    r = json.loads(lines[-1])
    print(env_vars, r)
    return r


@pytest.fixture(scope="module")
def full_workgroups(oracle, tmp_path_factory):
    """(a) sixteen ragged blocks of 3 - 6 KiB per CU: every workgroup has its sixteen waves, nine tables in LDS and seven in memory,
    and a block is 48 - 96 rounds, so every wave looks at its mates' estimates three times and more"""
    rng = np.random.default_rng(50)
    return _save(oracle, tmp_path_factory, "pace_a", _cut(rng.integers(3072, 6145, 16 * _cus()), 51))


@pytest.mark.parametrize("env_vars", [{}, {"K4LZ4_NO_PACE": "1"}, {"K4LZ4_PACE_MIN": "16"}], ids=["on", "no_pace", "below_the_threshold"])
def test_sixteen_waves_per_workgroup(full_workgroups, env_vars):
    """with the priorities, without them, and with the threshold at the batch's sixteen blocks per CU (used from MORE than that on)"""
    assert _child(full_workgroups, env_vars)["equal"]


def test_ten_waves_and_all_three_placements(oracle, tmp_path_factory):
    """(b) the batch of tests/test_gpu_table_address_space.py, test_ten_waves_per_workgroup -- nine and a half blocks per CU, the tenth
    wave's table in memory, moving into an LDS table that becomes free -- with the priorities on: the estimate goes on across the
    move, and all three placements still occur by the stamps (4 LDS, 5 memory, 6 memory first and LDS from some round on)"""
    cus = _cus()
    n = 9 * cus + cus // 2
    rng = np.random.default_rng(41)
    lengths = [128, 129] * 30 + [2048] * 40
    rest = n - len(lengths)
    lengths += [32768] * (rest - 2 * (rest // 7)) + [65535] * (rest // 7) + [65546] * (rest // 7)
    lengths = [lengths[i] for i in rng.permutation(n)]
    r = _child(_save(oracle, tmp_path_factory, "pace_b", _cut(lengths, 43)), {}, stamps=True)
    assert r["equal"] and r["equal_stamped"]
    assert set(r["placements"]) == {"4", "5", "6"}


@pytest.fixture(scope="module")
def beyond_a_residency(oracle, tmp_path_factory):
    return _save(oracle, tmp_path_factory, "pace_c", _cut([3072] * (20 * _cus()), 52))


@pytest.mark.parametrize("env_vars", [{"K4LZ4_PACE_QUEUE": "1"}, {}], ids=["queue_with_priorities", "default"])
def test_queue_mode_restarts_the_clock(beyond_a_residency, env_vars):
    """(c) twenty blocks of 3 KiB per CU: more than a residency, so one workgroup per CU and every wave takes a second block from the
    queue when it is done with its first -- its estimate taken out, its clock started anew.  Queue launches use the priorities only
    with K4LZ4_PACE_QUEUE (they measured slower with them); the default is run as well."""
    assert _child(beyond_a_residency, env_vars)["equal"]


def test_early_leavers(oracle, tmp_path_factory):
    """(d) sixteen blocks per CU of which half are 128 bytes -- through in two rounds, before anybody's first look -- beside blocks of
    4 - 8 KiB: waves leave while their SIMD mates run, and whoever is left must not wait for an estimate that is gone"""
    cus = _cus()
    rng = np.random.default_rng(53)
    lengths = np.where(rng.permutation(16 * cus) % 2 == 0, 128, rng.integers(4096, 8193, 16 * cus))
    assert _child(_save(oracle, tmp_path_factory, "pace_d", _cut(lengths, 54)), {})["equal"]
