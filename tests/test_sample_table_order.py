"""The cost sample's own table and the stable order (k4lz4_encode_fast.hpp: FastTable<3>, order_by_bucket; k4lz4_parse.hpp:
parse_block's TT = 3, parse_cost_body) in the host wave emulator.  The order is a permutation with the dearer buckets first; inside a
bucket the block indices ascend (a stable counting sort: the place is decided by index, not by arrival), so the launch gives the same
order run by one host thread and by several -- also where a workgroup's stretch is several steps of 256 blocks and where the last
workgroups of a launch have no stretch (cost[] and order[] of exactly n words); the classes whose parse takes long still rank above the one that is through in a
twelfth of the time; and under AddressSanitizer (tests/emu/sample_order.cpp, a program of its own) the sample stays inside its block
and inside a wave's allotment of table and `seen` set."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_lib
from k4os.compression.lz4_amd import corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
SAMPLE = 2048                       # PCOST_FIT.sample (the program checks its lengths against the constant itself)
COUNTS = [1, 15, 16, 17, 255, 256, 257, 1025]
LENGTHS = [0, 1, 12, 13, 127, 128, SAMPLE - 1, SAMPLE, SAMPLE + 1, 4096, 65535, 65546, 65547]
GXX = ["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-attributes", "-pthread", "-I" + EMU_DIR, "-I" + CSRC]
SOURCES = [os.path.join(EMU_DIR, "sample_order.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sample_order") / "libsample_order.so")
    subprocess.check_call(GXX + ["-O2", "-fPIC", "-shared", "-o", so] + SOURCES)
    l = C.CDLL(so)
    l.k4emu_porder_threads.argtypes = [C.POINTER(C.c_uint8), C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return l


def porder(lib, blocks, cost_threads, order_threads):
    src, off, lens = emu_lib.pack(blocks)
    n = len(blocks)
    cost = np.zeros(n, np.uint32)
    order = np.full(n, 0xFFFFFFFF, np.uint32)
    rc = lib.k4emu_porder_threads(src.ctypes.data_as(C.POINTER(C.c_uint8)), off.ctypes.data, lens.ctypes.data, n, cost.ctypes.data, order.ctypes.data,
                                  cost_threads, order_threads)
    assert rc == 0
    return cost, order


@pytest.fixture(scope="module")
def material():
    """one text-like and one binary-like stretch the ragged batches cut their blocks from"""
    return [corpus.class_bytes(c, 1 << 20, 77) for c in ("dickens", "mozilla")]


@pytest.mark.parametrize("n", COUNTS)
def test_order_is_a_stable_permutation_whatever_the_threads(lib, material, n):
    """n blocks whose lengths run through LENGTHS (nothing; too short for the parse; around its shortest; around the sample; the two
    block-size limits; the first length that is the byU32 kernel's).  n = 1025 is five workgroups of the order launch."""
    blocks = []
    for i in range(n):
        ln = LENGTHS[(i * 5 + n) % len(LENGTHS)]
        o = (i * 7919 * 64) % ((1 << 20) - ln)
        blocks.append(material[i % 2][o:o + ln])
    assert n < len(LENGTHS) or set(b.size for b in blocks) == set(LENGTHS)
    cost, order = porder(lib, blocks, 4, 1)
    assert sorted(order.tolist()) == list(range(n))
    assert (cost < 512).all()
    lens = np.array([b.size for b in blocks])
    assert (cost[lens == 0] == 0).all()
    c = cost[order].astype(np.int64)
    assert (np.diff(c) <= 0).all()
    same = np.diff(c) == 0
    assert (np.diff(order.astype(np.int64))[same] > 0).all(), "inside a bucket the indices ascend"
    for threads in (2, 4):
        cost_t, order_t = porder(lib, blocks, 4, threads)
        assert np.array_equal(cost_t, cost) and np.array_equal(order_t, order), threads


@pytest.mark.parametrize("n,grid,fine,buckets", [(2000, 3, 1, 40), (2000, 3, 0, 7), (1793, 2, 1, 1), (70000, 256, 1, 300), (70000, 256, 0, 64),
                                                 (70000, 0, 1, 2), (513, 256, 1, 9)])
def test_order_alone_with_long_stretches_and_idle_workgroups(lib, n, grid, fine, buckets):
    """k4_order_kernel from given buckets.  A grid of 2 or 3 makes a workgroup's stretch several steps of 256 blocks (a bucket's count
    is carried from step to step); 70 000 blocks in 256 workgroups (and in the 239 the host launches: grid 0) are stretches of 512
    and workgroups without one, which read nothing; 513 blocks in 256 workgroups leave 253 idle.  Both forms of the kernel."""
    lib.k4emu_order_only.argtypes = [C.c_void_p, C.c_longlong, C.c_uint, C.c_int, C.c_int, C.c_void_p]
    cost = np.random.default_rng(n + grid).integers(0, buckets, n).astype(np.uint32)
    orders = []
    for threads in (1, 4):
        order = np.full(n, 0xFFFFFFFF, np.uint32)
        assert lib.k4emu_order_only(cost.ctypes.data, n, grid, fine, threads, order.ctypes.data) == 0
        orders.append(order)
    # the stable sort by descending bucket is the one order that is right
    assert np.array_equal(orders[0], np.argsort(-cost.astype(np.int64), kind="stable").astype(np.uint32))
    assert np.array_equal(orders[1], orders[0])


def test_long_parses_rank_above_short_ones(lib):
    """8 blocks each of osdb, dickens, ooffice and sao: every osdb, dickens and ooffice block (915, 992 and 928 rounds of the parse)
    comes before every sao block (51 rounds) -- with the sample's 12-bit table as with the block's own."""
    names = ("osdb", "dickens", "ooffice", "sao")
    blocks, cls = [], []
    for name in names:
        blocks += list(corpus.class_bytes(name, 8 * 65536, 5).reshape(8, 65536))
        cls += [name] * 8
    cls = np.array(cls)
    cost, order = porder(lib, blocks, 4, 2)
    assert sorted(order.tolist()) == list(range(32))
    rank = np.empty(32, np.int64)
    rank[order] = np.arange(32)
    print({name: (int(cost[cls == name].min()), int(cost[cls == name].max())) for name in names})
    for name in ("osdb", "dickens", "ooffice"):
        assert rank[cls == name].max() < rank[cls == "sao"].min(), name
        assert cost[cls == name].min() > cost[cls == "sao"].max(), name


def test_sample_stays_inside_block_and_allotment_under_asan(tmp_path):
    """tests/emu/sample_order.cpp as a program, built with -fsanitize=address and run directly: the same counts and lengths, every
    block between poisoned bytes, every wave's table and `seen` set a heap block of exactly its allotment."""
    exe = str(tmp_path / "sample_order_asan")
    # (no -g: the header takes twice as long to compile with it, and a report names the function all the same)
    subprocess.check_call(GXX + ["-O1", "-fsanitize=address", "-fno-omit-frame-pointer", "-o", exe] + SOURCES)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-1000:], p.stderr[-3000:])
