"""The fast encoder's hash table reached as an LDS table or as a memory table, never as "either" (k4lz4_parse.hpp, parse_one; DESIGN.md
section 4.7): which address space a look-up or a put goes through changes no byte.  Every case against the oracle, byte for byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from k4os.compression.lz4_amd import LZ4Codec, corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 40 blocks, lengths from {128, 129, 2 048, 32 768, 65 535, 65 546}: how many of each is fixed and not left to the draw (half the
# batch at the two block-size limits, a third in the middle, a few short ones), their order is shuffled.
LENGTHS = [128] * 2 + [129] * 2 + [2048] * 3 + [32768] * 13 + [65535] * 10 + [65546] * 10
CLASSES = ("dickens", "mozilla")            # a text class and a binary class

CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec
z = np.load(sys.argv[2])
want_stamps = sys.argv[3] == "stamps"
dc = DeviceCodec(0)
src = DeviceBatch.from_host(z["data"], z["off"], z["lens"], dc.device)
def check(clen, comp):
    torch.cuda.synchronize()
    ch, coff, cl = comp.data.cpu().numpy(), comp.off.cpu().numpy(), clen.cpu().numpy()
    bad = []
    for i in range(z["lens"].size):
        w = z["want"][z["want_off"][i]:z["want_off"][i + 1]]
        if int(cl[i]) != w.size or not np.array_equal(ch[coff[i]:coff[i] + w.size], w) or not (ch[coff[i] + w.size:coff[i] + z["caps"][i]] == 0xCD).all():
            bad.append(i)
    return bad
comp = DeviceBatch.empty_slots(z["caps"], dc.device, fill=0xCD)
out = {"bad": check(dc.encode(src, comp), comp)}
if want_stamps:
    comp = DeviceBatch.empty_slots(z["caps"], dc.device, fill=0xCD)
    clen, counters = dc.profile(4, src, comp)
    out["bad_stamped"] = check(clen, comp)
    out["stamps"] = [int(v) for v in counters.cpu().numpy()[:, 11]]
print(json.dumps(out))
"""


def _pack(blocks):
    lens = np.array([b.size for b in blocks], np.int32)
    off = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.uint64)
    return np.concatenate(blocks), off, lens


@pytest.fixture(scope="module")
def workgroup_batch(oracle, tmp_path_factory):
    rng = np.random.default_rng(40)
    blocks = [corpus.class_bytes(CLASSES[i % 2], n, 700 + i) for i, n in enumerate(LENGTHS)]
    blocks = [blocks[i] for i in rng.permutation(len(blocks))]
    data, off, lens = _pack(blocks)
    want = [np.frombuffer(oracle.encode(b), np.uint8) for b in blocks]
    want_off = np.concatenate([[0], np.cumsum([w.size for w in want])]).astype(np.int64)
    path = str(tmp_path_factory.mktemp("table_as") / "batch.npz")
    np.savez(path, data=data, off=off, lens=lens, caps=np.array([LZ4Codec.MaximumOutputSize(int(n)) for n in lens], np.int64),
             want=np.concatenate(want), want_off=want_off)
    return path, lens


def _child(path, env_vars, stamps):
    env = {k: v for k, v in os.environ.items() if k not in ("K4LZ4_NO_MIGRATE", "K4LZ4_PARSE_QUEUE")}
    env.update(env_vars)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, path, "stamps" if stamps else "plain"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stderr[-2000:])
    return json.loads(lines[-1])


@pytest.mark.parametrize("env_vars", [{}, {"K4LZ4_NO_MIGRATE": "1"}, {"K4LZ4_PARSE_QUEUE": "9"}], ids=["default", "no_migrate", "parse_queue"])
def test_one_workgroup_and_a_little_more(workgroup_batch, env_vars):
    """40 shuffled blocks (LENGTHS, over a text and a binary class) in a fresh process per switch -- the switches are read when a
    context is made --, each against the oracle byte for byte.  The default and the no-migration run also read the placement stamps
    of profile mode 4 (counters[:, 11]: 4 LDS, 5 memory, 6 memory first and an LDS table from some round on; the stamping launch
    is checked against the oracle too).  What they can show on 40 blocks is limited by the launch, not by the lengths: a batch is
    spread over the CUs first (waves per workgroup = blocks / CUs rounded up, k4lz4_launch.hpp, fast_chunk), so on a chip of 256 CUs these 40
    blocks run as 40 workgroups of ONE wave, every table in LDS, and K4LZ4_PARSE_QUEUE, which engages beyond one residency of the
    chip, repeats the default placement.  Memory tables begin at nine blocks per CU: test_ten_waves_per_workgroup below is the batch
    in which all three placements occur, and asserts it."""
    path, lens = workgroup_batch
    r = _child(path, env_vars, stamps="K4LZ4_PARSE_QUEUE" not in env_vars)
    print(env_vars, r)
    assert r["bad"] == []
    if "stamps" in r:
        assert r["bad_stamped"] == []
        assert set(r["stamps"]) <= ({4, 5} if env_vars else {4, 5, 6})


def test_ten_waves_per_workgroup(oracle, monkeypatch):
    """Nine and a half blocks per CU: workgroups of ten waves, nine with LDS tables and one -- the cheapest tenth of the cost
    order -- with its table in memory.  Sixty blocks of 128 and 129 bytes are among those and are through within two rounds, long
    before the first look at the free-table word (one look every 16 rounds): stamp 5.  The rest of that tenth are blocks of 2 048
    and of 32 768 bytes beside LDS-table blocks of their own length and class, and move into the table of the first block of their
    workgroup that finishes: stamp 6 (on an MI355X: 2 196 blocks with stamp 4, 135 with 5, 101 with 6, of both lengths).
    All three stamps must occur by default, none may say 6 with K4LZ4_NO_MIGRATE; every block against the oracle, byte for byte,
    in the ordinary launch and in the stamping one."""
    import torch
    from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 9 * cus + cus // 2
    rng = np.random.default_rng(41)
    lengths = [128, 129] * 30 + [2048] * 40
    rest = n - len(lengths)
    lengths += [32768] * (rest - 2 * (rest // 7)) + [65535] * (rest // 7) + [65546] * (rest // 7)
    lengths = [lengths[i] for i in rng.permutation(n)]
    base = [corpus.class_bytes(c, 4 << 20, 43) for c in CLASSES]
    blocks = []
    for i, ln in enumerate(lengths):
        o = (i * 7919 * 64) % ((4 << 20) - ln)
        blocks.append(base[i % 2][o:o + ln])
    data, off, lens = _pack(blocks)
    caps = np.array([LZ4Codec.MaximumOutputSize(int(v)) for v in lens], np.int32)
    for env_vars in ({}, {"K4LZ4_NO_MIGRATE": "1"}):
        monkeypatch.delenv("K4LZ4_NO_MIGRATE", raising=False)
        for k, v in env_vars.items():
            monkeypatch.setenv(k, v)
        dc = DeviceCodec(0)                                   # the switches are read when a context is created
        src = DeviceBatch.from_host(data, off, lens, dc.device)
        comp = DeviceBatch.empty_slots(caps, dc.device, fill=0xCD)
        coff = comp.off.cpu().numpy()
        if not env_vars:
            ref = np.full(comp.data.numel(), 0xCD, np.uint8)
            want = oracle.encode_batch(data, off, lens, ref, coff.astype(np.uint64), caps, threads=16)
        clen = dc.encode(src, comp)
        torch.cuda.synchronize()
        assert np.array_equal(clen.cpu().numpy(), want), env_vars
        assert np.array_equal(comp.data.cpu().numpy(), ref), env_vars
        comp2 = DeviceBatch.empty_slots(caps, dc.device, fill=0xCD)
        clen2, counters = dc.profile(4, src, comp2)
        torch.cuda.synchronize()
        assert np.array_equal(clen2.cpu().numpy(), want) and np.array_equal(comp2.data.cpu().numpy(), ref), env_vars
        stamps = counters.cpu().numpy()[:, 11]
        moved = sorted(set(int(lens[i]) for i in np.nonzero(stamps == 6)[0]))
        print(env_vars, "placements:", {int(k): int((stamps == k).sum()) for k in np.unique(stamps)}, "lengths that moved:", moved)
        assert set(int(k) for k in np.unique(stamps)) == ({4, 5} if env_vars else {4, 5, 6})


def test_byu32_forms(oracle):
    """The byU32 tables: two blocks of 65 547 bytes (the first length with one) and one of 200 000 through k4_parse_big_kernel
    -- LL64's hash5 and, with FLAG_X32, LL32's hash4 --, and a ragged pickle batch, a handful of messages of which one is 1.5 MiB
    of text and is cut into segments, through k4_parse_seg_kernel: the oracle's blocks and envelopes."""
    import torch
    from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec
    from k4os.compression.lz4_amd._native import FLAG_RAW_RETURN, FLAG_X32
    dc = DeviceCodec(0)
    blocks = [corpus.class_bytes("dickens", 65547, 31), corpus.class_bytes("mozilla", 65547, 32), corpus.class_bytes("samba", 200000, 33)]
    data, off, lens = _pack(blocks)
    src = DeviceBatch.from_host(data, off, lens, dc.device)
    for flags in (0, FLAG_X32 | FLAG_RAW_RETURN):
        comp = DeviceBatch.empty_slots([LZ4Codec.MaximumOutputSize(int(n)) for n in lens], dc.device, fill=0xCD)
        clen = dc.encode(src, comp, flags=flags)
        torch.cuda.synchronize()
        ch, coff, cl = comp.data.cpu().numpy(), comp.off.cpu().numpy(), clen.cpu().numpy()
        for i, b in enumerate(blocks):
            if flags:
                r, w = oracle.compress_fast_x32(b)
                want = w[:r].tobytes()
            else:
                want = oracle.encode(b)
            assert int(cl[i]) == len(want) and ch[coff[i]:coff[i] + cl[i]].tobytes() == want, (flags, i)
    msgs = [corpus.class_bytes("dickens", 3 << 19, 34), corpus.class_bytes("xml", 70000, 35), corpus.class_bytes("mozilla", 300000, 36),
            corpus.lorem(1337), corpus.class_bytes("osdb", 65546, 37), corpus.class_bytes("sao", 131, 38)]
    data, off, lens = _pack(msgs)
    src = DeviceBatch.from_host(data, off, lens, dc.device)
    env = DeviceBatch.empty_slots(lens.astype(np.int64) + 5, dc.device, fill=0xCD)
    plen = dc.pickle(src, env)
    torch.cuda.synchronize()
    eh, eoff, pl = env.data.cpu().numpy(), env.off.cpu().numpy(), plen.cpu().numpy()
    for i, m in enumerate(msgs):
        assert eh[eoff[i]:eoff[i] + pl[i]].tobytes() == oracle.pickle(m), f"message {i} ({m.size} B)"
