"""The level rule of k4_parse_kernel's late-blocks-first priorities (k4lz4_parse.hpp: parse_pace_estimate, parse_pace_level,
parse_pace_first_level) as plain functions in the host build of the product header (tests/emu/parse_pace.cpp).
A wave's estimate F is when its block will be done at the pace so far, in ticks of a 32-bit counter from the workgroup's start; its
level is how close F is to the latest estimate on its SIMD, in tiers of 1 / PARSE_PACE_DEN.  What the priorities do to the bytes --
nothing -- is the GPU suite's business (tests/test_gpu_parse_pace.py, against the oracle).  The SIMD-even deal of the issue's second
part is not built (DESIGN.md says why), so there is no deal table to test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "k4os", "compression", "lz4_amd", "csrc")
GXX = ["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-attributes", "-pthread", "-I" + EMU_DIR, "-I" + CSRC]
WAVES = 16


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("parse_pace") / "libparse_pace.so")
    subprocess.check_call(GXX + ["-O2", "-fPIC", "-shared", "-o", so, os.path.join(EMU_DIR, "parse_pace.cpp"), os.path.join(EMU_DIR, "emu_runtime.cpp")])
    l = C.CDLL(so)
    for name in ("k4emu_pace_den", "k4emu_pace_max", "k4emu_pace_estimate"):
        getattr(l, name).restype = C.c_uint32
    l.k4emu_pace_estimate.argtypes = [C.c_uint32] * 5
    l.k4emu_pace_level.argtypes = [C.c_uint32, C.c_uint32]
    l.k4emu_pace_first_level.argtypes = [C.c_uint32, C.c_int]
    l.k4emu_pace_look.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    return l


def look(lib, row, me, mine):
    r = np.array(row, np.uint32)
    assert r.size == WAVES
    lv = lib.k4emu_pace_look(r.ctypes.data, me, mine)
    return lv, r


def test_words_fit_the_cu(lib):
    """nine tables, sixteen `seen` sets, the free-table word and the priorities' words in 160 KiB; a product of an estimate and the
    tier denominator in 32 bits"""
    assert lib.k4emu_pace_lds_bytes() <= 160 * 1024
    assert lib.k4emu_pace_words() * 4 <= 8 * 1024
    assert lib.k4emu_pace_max() * lib.k4emu_pace_den() < 1 << 32


def test_one_wave_alone(lib):
    """nobody else on the SIMD: the wave is its own latest"""
    lv, row = look(lib, [0] * WAVES, 5, 300000)
    assert lv == 3 and row[5] == 300000 and int(row.sum()) == 300000


def test_mates_without_a_report(lib):
    """mates that have begun and not yet reported hold 0 and do not count; a wave with no estimate of its own keeps its level (-1)"""
    row = [0] * WAVES
    assert look(lib, row, 0, 250000)[0] == 3
    assert lib.k4emu_pace_level(0, 0) == -1 and lib.k4emu_pace_level(0, 123456) == -1
    for wave in range(WAVES):
        assert lib.k4emu_pace_first_level(wave, 0) == 3                       # starts in memory: the group that ends the launch
        assert lib.k4emu_pace_first_level(wave, 1) == (2 if wave < 4 else 1)


def test_a_mate_that_has_left(lib):
    """a late mate puts the wave at the bottom; once the mate has taken its estimate out, the wave is the latest"""
    row = [0] * WAVES
    row[9] = 310000
    lv, row = look(lib, row, 1, 250000)
    assert lv == 0
    row[9] = 0
    assert look(lib, row, 1, 250000)[0] == 3


def test_nothing_done_yet(lib):
    """c == 0: no estimate, no report"""
    assert lib.k4emu_pace_estimate(1000, 1000, 5000, 0, 65536) == 0
    assert lib.k4emu_pace_level(lib.k4emu_pace_estimate(1000, 1000, 5000, 0, 65536), 200000) == -1
    assert lib.k4emu_pace_estimate(1000, 1000, 1000, 1, 65536) >= 1            # never 0 once something is done


def test_the_counter_wraps(lib):
    """only differences of times are used: the same three times 0x200 ticks before the counter wraps and far from it"""
    U = 65536
    for c, lead, elapsed in [(1024, 16, 4000), (32768, 0, 150000), (65535, 70000, 299999)]:
        want = lib.k4emu_pace_estimate(1 << 20, (1 << 20) + lead, (1 << 20) + lead + elapsed, c, U)
        base = (1 << 32) - 0x200
        for b in (base, base - lead, (base - lead - elapsed // 2) % (1 << 32)):
            got = lib.k4emu_pace_estimate(b % (1 << 32), (b + lead) % (1 << 32), (b + lead + elapsed) % (1 << 32), c, U)
            assert got == want
        assert abs(want - (lead + elapsed * U / c)) <= 1 + want * 2.0 ** -22     # float32 arithmetic on the pace
    # an estimate never leaves the range in which the tiers are exact
    assert lib.k4emu_pace_estimate(0, 0, 0xffffffff, 1, 65546) == lib.k4emu_pace_max()
    assert lib.k4emu_pace_estimate(0, 0x80000000, 0x80000010, 64, 128) == lib.k4emu_pace_max()


def test_equal_estimates(lib):
    """equal estimates: both at the top; and the tiers, 1 / DEN of the latest apart"""
    row = [0] * WAVES
    row[2] = 280000
    assert look(lib, row, 6, 280000)[0] == 3
    den, top = lib.k4emu_pace_den(), lib.k4emu_pace_max()
    for latest in (den * 1000, 320000 // den * den, top // den * den):
        step = latest // den
        assert lib.k4emu_pace_level(latest, latest) == 3
        assert lib.k4emu_pace_level(latest - step, latest) == 3 and lib.k4emu_pace_level(latest - step - 1, latest) == 2
        assert lib.k4emu_pace_level(latest - 2 * step, latest) == 2 and lib.k4emu_pace_level(latest - 2 * step - 1, latest) == 1
        assert lib.k4emu_pace_level(latest - 3 * step, latest) == 1 and lib.k4emu_pace_level(latest - 3 * step - 1, latest) == 0
        assert lib.k4emu_pace_level(1, latest) == 0
    assert lib.k4emu_pace_level(top, top - 5) == 3                              # a stale `latest` below the wave's own
