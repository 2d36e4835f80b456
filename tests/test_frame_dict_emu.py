"""Frames with a predefined dictionary through the reader's kernels under the host wave emulator (no GPU): every case of
tests/frame_dict_cases.py against tests/golden/frame_dict_cases.json (what liblz4's LZ4F_decompress_usingDict makes of the frame) and,
where liblz4 is present, against liblz4 live.  k4lz4_frame_dict.hpp, DESIGN.md 4.24."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "tools"))

import frame_dict_cases as FC          # noqa: E402
import frame_dict_emu as FE            # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return FC.load()["cases"]


@pytest.fixture(scope="module")
def E():
    return FC.entries()


def cap_of(c):
    return None if c.cap == "size" else len(c.content) - 1


def check(c, golden, out_len, out, idx):
    """one frame's result against its case and the golden file"""
    want = golden[c.name]["decoded"]
    assert FC.xxh32(c.frame) == golden[c.name]["frame_xxh32"], c.name
    if c.expect is not None:
        assert out_len == c.expect, (c.name, out_len)
        if c.expect in (FC.BLOCK, FC.HEADER_SUM, FC.EOF, FC.LENGTH):
            assert want == "rejected", c.name           # liblz4 refuses these too
    else:
        assert want != "rejected", c.name
        assert out_len == want[0] and FC.xxh32(out) == want[1], (c.name, out_len)
        if c.content is not None:
            assert out == c.content, c.name
    if not c.null_set:
        assert idx == (c.entry if c.expect not in (FC.DICTIONARY, FC.HEADER_SUM, FC.EOF) else -1), (c.name, idx)


def test_golden_file_is_a_fresh_recording():
    if FC.liblz4() is None:
        pytest.skip("liblz4.so.1 with LZ4F_decompress_usingDict not present")
    import record_frame_dict_goldens as R
    assert R.record() == FC.load()
    assert os.path.getsize(FC.GOLDEN) < 100 << 10


def test_hand_built_frames_follow_the_format(E):
    """the cases' own model of the format agrees with what was recorded (the hand-built frames carry no witness of their own)"""
    g = FC.load()["cases"]
    blocks = [(FC.seq(b"0123456789abcdef", 16 + 1000, 40) + FC.seq(b"x" * 12), False)]
    got = FC.decode_model(blocks, E[0].tobytes(), True)
    assert got == b"0123456789abcdef" + E[0].tobytes()[-1000:-960] + b"x" * 12
    assert sum(1 for v in g.values() if v["decoded"] == "rejected") >= 10 and len(g) == len(FC.cases())


@pytest.mark.parametrize("chain_waves", [1024, 2])
def test_every_case_with_the_set(golden, E, chain_waves):
    """all cases in one batch (chain_waves = 2: one workgroup of the in-order decoder takes every frame in turns, its windows reused)"""
    cs = [c for c in FC.cases() if not c.null_set]
    out_len, outs, size, status, idx = FE.decode([c.frame for c in cs], [cap_of(c) for c in cs], E, FC.IDS, chain_waves=chain_waves)
    for c, n, o, i in zip(cs, out_len, outs, idx):
        check(c, golden, int(n), o, int(i))
    for c, s, st in zip(cs, size, status):
        if c.expect is None:
            assert st == 0 and int(s) >= golden[c.name]["decoded"][0], c.name
        if c.expect in (FC.DICTIONARY, FC.HEADER_SUM, FC.EOF):
            assert st == c.expect and s == 0, c.name


def test_without_a_set_every_dictid_is_refused(golden, E):
    """set = NULL is the plain reader: K4LZ4_FRAME_DICTIONARY behind the header checksum, whatever the id; plain frames decode"""
    cs = FC.cases()
    out_len, outs, size, status, idx = FE.decode([c.frame for c in cs], [cap_of(c) for c in cs], None)
    for c, n, o, i in zip(cs, out_len, outs, idx):
        has_id = len(c.frame) > 4 and (c.frame[4] & 1)
        if c.expect in (FC.HEADER_SUM, FC.EOF):
            assert n == c.expect, c.name
        elif has_id:
            assert n == FC.DICTIONARY, (c.name, n)
        else:
            check(c, golden, int(n), o, -1)
        assert i == -1


def test_each_case_alone_matches_liblz4_live(E):
    if FC.liblz4() is None:
        pytest.skip("liblz4.so.1 with LZ4F_decompress_usingDict not present")
    cs = [c for c in FC.cases() if not c.null_set and c.cap == "size" and c.expect != FC.DICTIONARY]
    out_len, outs, *_ = FE.decode([c.frame for c in cs], [None] * len(cs), E, FC.IDS)
    for c, n, o in zip(cs, out_len, outs):
        live = FC.lz4f_decode(c.frame, E[c.entry].tobytes() if c.entry >= 0 else b"", 4 * FC.K64 + 4096)
        assert (o is None) == (live is None) and o == live, (c.name, n)
