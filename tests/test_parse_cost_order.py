"""The two-step fast encoder's own cost estimate and dispatch order (k4lz4_parse.hpp: ParseCost, parse_cost_body; k4lz4_encode_fast.hpp:
k4_order_kernel's fine form with its wave-scan suffix sums) in the host wave emulator: the order is a permutation whatever the batch,
the samples stay inside their blocks (a program of its own under AddressSanitizer), and the classes whose parse takes long rank
above the one that is through in a twelfth of the time -- which the estimate by sequences in 256 bytes got wrong."""
import os
import subprocess

import numpy as np
import pytest

import emu_lib
from k4os.compression.lz4_amd import corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
COUNTS = [1, 2, 15, 16, 17, 255, 256, 257]
LENGTHS = [0, 1, 127, 128, 129, 65535, 65546, 65547]


@pytest.fixture(scope="module")
def emu():
    return emu_lib.Emu()


@pytest.fixture(scope="module")
def material():
    """one text-like and one binary-like stretch the ragged batches cut their blocks from"""
    return [corpus.class_bytes(c, 1 << 20, 77) for c in ("dickens", "mozilla")]


@pytest.mark.parametrize("n", COUNTS)
def test_order_is_a_permutation(emu, material, n):
    """n blocks whose lengths run through LENGTHS (nothing; too short for the parse; its shortest; the two block-size limits; the first
    length that is the byU32 kernel's): every index once, dearer buckets first."""
    blocks = []
    for i in range(n):
        ln = LENGTHS[(i * 5 + n) % 8]
        o = (i * 7919 * 64) % ((1 << 20) - ln)
        blocks.append(material[i % 2][o:o + ln])
    assert n < 8 or set(b.size for b in blocks) == set(LENGTHS)
    src, off, lens = emu_lib.pack(blocks)
    cost, order = emu.porder(src, off, lens, threads=4)
    assert sorted(order.tolist()) == list(range(n))
    assert (cost < 512).all()
    assert (np.diff(cost[order].astype(np.int64)) <= 0).all()
    assert (cost[lens == 0] == 0).all()


def test_long_parses_rank_above_short_ones(emu):
    """8 blocks each of ooffice, osdb, dickens, sao and x-ray: every ooffice, osdb and dickens block (928, 915 and 992 rounds of the
    parse) comes before every sao block (51 rounds) in the order.  Nothing finer: the fit decides the rest."""
    names = ("ooffice", "osdb", "dickens", "sao", "x-ray")
    blocks, cls = [], []
    for name in names:
        data = corpus.class_bytes(name, 8 * 65536, 5).reshape(8, 65536)
        blocks += list(data)
        cls += [name] * 8
    cls = np.array(cls)
    src, off, lens = emu_lib.pack(blocks)
    cost, order = emu.porder(src, off, lens, threads=4)
    assert sorted(order.tolist()) == list(range(40))
    rank = np.empty(40, np.int64)
    rank[order] = np.arange(40)
    print({name: (int(cost[cls == name].min()), int(cost[cls == name].max())) for name in names})
    for name in ("ooffice", "osdb", "dickens"):
        assert rank[cls == name].max() < rank[cls == "sao"].min(), name
        assert cost[cls == name].min() > cost[cls == "sao"].max(), name


def test_samples_stay_inside_their_blocks_under_asan(tmp_path):
    """tests/emu/parse_cost_main.cpp, a program with its own main, built with -fsanitize=address and run: the same counts and
    lengths, every block between poisoned bytes."""
    exe = str(tmp_path / "parse_cost_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas",
                           "-Wno-unused-function", "-Wno-attributes", "-pthread", "-I" + EMU_DIR, "-I" + CSRC, "-o", exe,
                           os.path.join(EMU_DIR, "parse_cost_main.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-1000:], p.stderr[-3000:])
