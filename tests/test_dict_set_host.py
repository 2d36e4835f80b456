"""k4lz4_dict_set_layout: the host arithmetic of a dictionary set -- which bytes of every entry are kept, where they lie
in the set's memory, which table an entry has in either family and how many device bytes the set holds -- against a few lines of
Python written from the rules, over the dictionary lists of tests/dict_encode_cases.py and tests/dict_hc_encode_cases.py and one list
of overlapping ranges.  No GPU."""
import numpy as np
import pytest

import dict_encode_cases as DC
import dict_hc_encode_cases as HC
from k4os.compression.lz4_amd import DICT_FAST, DICT_HC, DictionarySet, _native, pack_blocks

K64 = 65536
FAST_TABLE, HC_TABLE = 4096 * 4, 32768 * 4 + 65536 * 2


def up64(n):
    return (n + 63) // 64 * 64


def lists():
    out = []
    for mod in (DC, HC):
        for c in mod.calls():
            _, off, ln = pack_blocks(c.dicts)
            out.append((f"{mod.__name__}:{c.name}", off, ln))
    # ranges of one buffer: a long dictionary and the 64 KiB it keeps as an entry of their own, the same entry twice, short ones, empty ones
    off = np.array([0, 70000 - K64, 0, 10, 10, 12, 100, 5, 20, 20], np.uint64)
    ln = np.array([70000, K64, 70000, 5, 5, 3, 0, 0, 8, 7], np.int32)
    out.append(("ranges", off, ln))
    return out


LISTS = lists()


def expected(off, ln, families):
    """the rules, written down: an entry keeps its last min(len, 65536) bytes; every distinct kept range (empty: one for all) gets the
    next 64-byte step; the HC family's table is the range's number, the fast family's the number of the range among those of 8 bytes
    and more, everything shorter being one empty dictionary"""
    ranges, fast, at = {}, {}, 0
    kept, where, tf, th = [], [], [], []
    for o, n in zip(off.tolist(), ln.tolist()):
        k = min(n, K64)
        key = (o + n - k, k) if k else (0, 0)
        if key not in ranges:
            ranges[key] = (len(ranges), at)
            at += up64(k)
        fkey = key if n >= 8 else (0, 0)
        fast.setdefault(fkey, len(fast))
        kept.append(k)
        where.append(ranges[key][1])
        th.append(ranges[key][0] if families & DICT_HC else -1)
        tf.append(fast[fkey] if families & DICT_FAST else -1)
    nd = len(kept)
    total = at + 64 + up64(nd * 8) + up64(nd * 4)
    for bit, nt, tb in ((DICT_FAST, len(fast), FAST_TABLE), (DICT_HC, len(ranges), HC_TABLE)):
        if families & bit:
            nt = max(nt, 1)
            total += up64(nt * 8) + up64(nt * 4) + up64(nd * 8) + 2 * up64(nd * 4) + up64(nt * tb)
    return kept, where, tf, th, total


def test_the_lists_hold_the_lengths_that_matter():
    seen = set()
    for _, _, ln in LISTS:
        seen |= set(ln.tolist())
    assert {0, 3, 4, 5, 7, 8, 9, 100, 4096, 65535, 65536, 70000} <= seen
    inter = next(c for c in DC.calls() if c.name == "interleaved")
    assert inter.dicts[0].tobytes() == inter.dicts[2].tobytes()


@pytest.mark.parametrize("families", [DICT_FAST, DICT_HC, DICT_FAST | DICT_HC])
@pytest.mark.parametrize("name", [l[0] for l in LISTS])
def test_layout_equals_the_rules(name, families):
    _, off, ln = next(l for l in LISTS if l[0] == name)
    kept, at, tf, th, total = DictionarySet.layout(off, ln, families)
    want = expected(off, ln, families)
    assert kept.tolist() == want[0] and at.tolist() == want[1], name
    assert tf.tolist() == want[2] and th.tolist() == want[3], name
    assert total == want[4], name
    assert (at % 64 == 0).all()
    # no two distinct ranges overlap in the set's memory, and all of them lie in front of the words and tables
    spans = sorted({(int(a), int(k)) for a, k in zip(at, kept) if k})
    for (a0, k0), (a1, _) in zip(spans, spans[1:]):
        assert a0 + k0 <= a1
    assert not spans or spans[-1][0] + spans[-1][1] <= total


def test_equal_ranges_share_a_table_and_the_families_differ_below_eight_bytes():
    _, off, ln = next(l for l in LISTS if l[0] == "ranges")
    kept, at, tf, th, _ = DictionarySet.layout(off, ln, DICT_FAST | DICT_HC)
    # the long dictionary, the 64 KiB it keeps, and itself again: one range, one table per family
    assert at[0] == at[1] == at[2] and tf[0] == tf[1] == tf[2] and th[0] == th[1] == th[2]
    assert th[3] == th[4] and th[3] != th[5]                  # equal short ranges share; a different one does not
    assert th[6] == th[7] and kept[6] == kept[7] == 0         # empty is empty wherever it points
    assert tf[3] == tf[4] == tf[5] == tf[6] == tf[7] == tf[9] and tf[8] != tf[9]       # the fast family: below 8 bytes, the empty dictionary
    assert th[8] != th[9] and kept[9] == 7
    # over all lists: the two families tell entries apart differently exactly where a dictionary of 1 .. 7 bytes is involved
    for name, off, ln in LISTS:
        _, _, tf, th, _ = DictionarySet.layout(off, ln, DICT_FAST | DICT_HC)
        for i in range(len(ln)):
            for j in range(i):
                same_f, same_h = tf[i] == tf[j], th[i] == th[j]
                if same_f != same_h:
                    assert same_f and (0 < ln[i] < 8 or 0 < ln[j] < 8) and ln[i] < 8 and ln[j] < 8, (name, i, j)
        short = [i for i in range(len(ln)) if 0 < ln[i] < 8]
        empty = [i for i in range(len(ln)) if ln[i] == 0]
        for i in short:
            assert all(tf[i] == tf[j] for j in short + empty) and all(th[i] != th[j] for j in empty), (name, i)


def test_interleaved_keeps_equal_bytes_at_two_places_as_the_per_call_lists_do():
    """dict_list tells entries apart, in both families, by the range they keep, not by content: the set follows them, so a set call
    gives every entry the table the per-call call gives it"""
    _, off, ln = next(l for l in LISTS if l[0] == "dict_encode_cases:interleaved")
    _, at, tf, th, _ = DictionarySet.layout(off, ln, DICT_FAST | DICT_HC)
    assert tf.tolist() == [0, 1, 2, 3] and th.tolist() == [0, 1, 2, 3] and len(set(at.tolist())) == 4


def test_refusals():
    lib = _native.load_library()
    off, ln = np.array([0, 10], np.uint64), np.array([10, 5], np.int32)
    total = np.zeros(1, np.uint64)

    def rc(o, l, n, fam):
        return lib.k4lz4_dict_set_layout(o.ctypes.data if o is not None else None, l.ctypes.data if l is not None else None, n, fam,
                                         None, None, None, None, total.ctypes.data)

    assert rc(off, ln, 2, DICT_FAST) == 0 and total[0] > 0
    assert rc(off, ln, 2, 0) == _native.E_ARG                                  # no family
    assert rc(off, ln, 2, 4) == _native.E_ARG and rc(off, ln, 2, 7) == _native.E_ARG
    assert rc(off, ln, -1, DICT_HC) == _native.E_ARG
    assert rc(off, np.array([10, -1], np.int32), 2, DICT_HC) == _native.E_ARG
    assert rc(None, ln, 2, DICT_HC) == _native.E_ARG and rc(off, None, 2, DICT_HC) == _native.E_ARG
    assert rc(None, None, 0, DICT_FAST | DICT_HC) == 0                          # an empty list: one empty table per family
    assert total[0] == 64 + 2 * (64 + 64) + up64(FAST_TABLE) + up64(HC_TABLE)
    with pytest.raises(ValueError):
        DictionarySet.layout(off, ln, 0)
    lib.k4lz4_dict_set_destroy(None)                                            # a no-op
    for sym in ("k4lz4_dict_set_create", "k4lz4_dict_set_create_device", "k4lz4_dict_set_destroy", "k4lz4_dict_set_info", "k4lz4_dict_set_layout",
                "k4lz4_dict_set_state", "k4lz4_dict_set_hc_state", "k4lz4_encode_dictset_batch", "k4lz4_encode_dictset_batch_device",
                "k4lz4_decode_dictset_batch", "k4lz4_decode_dictset_batch_device"):
        assert sym in _native.SYMBOLS and getattr(lib, sym)
