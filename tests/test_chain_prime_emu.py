"""The open kernels (k4_ce_open_kernel, k4_cdec_open_kernel) under the wave emulator, with guard bytes around every
store and around the set's memory: the state after opening against LZ4_loadDict's definition (and liblz4's LZ4_stream_t where it is
present), the ring against the kept bytes, the decoder's store against reset + Inject as the emulated run kernel leaves it, the
bad-index arm, and the seam case through the emulated k4_fast_chain_kernel continuing from the opened state."""
import json
import os

import numpy as np
import pytest

from k4os.compression.lz4_amd import encoders as E
import chain_prime_cases as PC
import chain_prime_emu as PE
import chain_prime_witness as PW
from chain_decoder_emu import EmuDecoders
from dict_encode_cases import reference_table, synthetic, u8

K1, K64 = 1024, 65536
DEV_STATUS_DICT_INDEX = 4


@pytest.fixture(scope="module")
def dictionaries():
    xml = synthetic("xml", 100000, 3)
    return [xml[1000:1000 + n].copy() for n in PC.DICT_LENGTHS]


@pytest.fixture(scope="module")
def emu_set(dictionaries):
    return PE.EmuSet(dictionaries)


def test_encoder_open_leaves_the_kept_bytes_and_loadDicts_state(dictionaries, emu_set):
    kinds = [(True, 0, K1, 0), (True, 9, K1, 2), (True, 0, K64, 1), (True, 3, 4 * K1, 0)]
    settings = [k for _ in dictionaries for k in kinds] + [(True, 0, K1, 0), (True, 3, K1, 0), (False, 0, K1, 0)]
    idx = [e for e in range(len(dictionaries)) for _ in kinds] + [-1, -1, -1]
    enc = PE.EmuEncoders(settings)
    rows = enc.open(idx, emu_set)
    live = PW.available()
    if live:
        import dict_encode_witness as DW
    for s, (setting, e) in enumerate(zip(settings, idx)):
        rec = enc.records[s]
        kept = emu_set.kept[e] if e >= 0 else u8(b"")
        d = PW.primed_length(rec.kind, kept.size) if e >= 0 else 0
        assert (rec.index, rec.pointer, rec.taken, rec.blocks) == (d, d, 0, 0), (setting, e)
        assert enc.ring(s) == kept[kept.size - d:].tobytes(), (setting, e)
        enc.untouched_behind(s, rows)
        if rec.kind != 2:
            continue
        st = enc.state(s)
        assert (int(st["currentOffset"]), int(st["dictSize"])) == ((K64, d) if e >= 0 else (0, 0)), (setting, e)
        assert (rec.currentOffset, rec.dictSize) == (int(st["currentOffset"]), int(st["dictSize"]))
        assert not st["reserved"].any()
        assert np.array_equal(st["hashTable"], reference_table(kept) if e >= 0 else np.zeros(4096, np.uint32)), (setting, e)
        if live and e >= 0:
            want = DW.load_state(dictionaries[e])
            assert np.array_equal(st["hashTable"], want["hashTable"]) and int(st["currentOffset"]) == want["currentOffset"] and \
                int(st["dictSize"]) == want["dictSize"], (setting, e)


def test_reopening_a_used_store_forgets_it(emu_set):
    """a store that holds another stream's ring and state: open overwrites exactly the state and the kept bytes"""
    enc = PE.EmuEncoders([(True, 0, K1, 0), (True, 0, K1, 0)])
    enc.open([10, 8], emu_set)                    # 65 536 and 4 096 bytes
    enc.open([8, -1], emu_set)
    assert enc.ring(0) == emu_set.kept[8].tobytes() and int(enc.state(0)["dictSize"]) == 4096
    assert np.array_equal(enc.state(0)["hashTable"], reference_table(emu_set.kept[8]))
    assert enc.ring(1) == b"" and not enc.state(1)["hashTable"].any() and int(enc.state(1)["currentOffset"]) == 0


DEC_SETTINGS = [(True, K1, 0), (True, K64, 2), (False, K1, 0), (False, K64, 0), (True, 5 * K1, 1)]


def test_decoder_open_equals_reset_plus_inject(dictionaries, emu_set):
    settings = [k for _ in dictionaries for k in DEC_SETTINGS] + DEC_SETTINGS[:3]
    idx = [e for e in range(len(dictionaries)) for _ in DEC_SETTINGS] + [-1, -1, -1]
    a, b = EmuDecoders(settings), EmuDecoders(settings)
    out, status = PE.cd_open(a, idx, emu_set)
    rec_out, want, _ = b.run([[(True, emu_set.kept[e].tobytes(), 0)] if e >= 0 else [] for e in idx])
    assert status == 0
    assert out == want
    assert np.array_equal(a.query(), b.query())
    for s, (setting, e) in enumerate(zip(settings, idx)):
        oa, ob, c = int(a.store_off[s]), int(b.store_off[s]), int(a.sizes[s])
        assert np.array_equal(a.store[oa:oa + c], b.store[ob:ob + c]), (setting, e)
        n = emu_set.kept[e].size if e >= 0 else 0
        refused = e >= 0 and not setting[0] and n > setting[1] + 8
        assert out[s] == (-2 if refused else n), (setting, e)
    assert any(o == -2 for o in out) and any(o == K64 for o in out)
    # the witness's object after the same record, where the compiled reference is there
    try:
        ws = [PW.opened_decoder(*st, dictionary=dictionaries[e] if e >= 0 else None) for st, e in zip(settings, idx)]
    except (FileNotFoundError, OSError):
        return
    q = a.query()
    for s, (w, o) in enumerate(zip(ws, out)):
        assert o == w[1] and q[s, 0] == w[0].output_index and q[s, 2] == w[0].records and q[s, 3] == w[0].bytes_made and q[s, 4] == w[0].last_code
    held = a.drain([-int(q[s, 0]) for s in range(len(ws))], [int(q[s, 0]) for s in range(len(ws))])
    for s, w in enumerate(ws):
        assert held[s] == w[0].drain(-w[0].output_index, w[0].output_index)


def test_decoder_bad_index_leaves_the_store(emu_set):
    settings = [(True, K1, 0), (True, K1, 0), (False, 2 * K1, 0), (True, K1, 0)]
    a = EmuDecoders(settings)
    a.store[int(a.store_off[0]):int(a.store_off[0]) + int(a.sizes[0])] = 0x77       # a store that was never a decoder
    before = a.store.copy()
    out, status = PE.cd_open(a, [emu_set.n, -2, 2, 8], emu_set)
    assert out[:2] == [E.CDEC_DICT_INDEX, E.CDEC_DICT_INDEX] and status == DEV_STATUS_DICT_INDEX
    for s in (0, 1):
        o, c = int(a.store_off[s]), int(a.sizes[s])
        assert np.array_equal(a.store[o:o + c], before[o:o + c])
    assert out[2:] == [3, 4096]
    assert a.query()[2:, 0].tolist() == [3, 4096]
    assert a.query()[0, 4] == E.CDEC_NO_DECODER


def test_seam_through_the_emulated_fast_chain_kernel():
    """the opened state and ring, continued by k4_fast_chain_kernel: the block opens as a contiguous prefix's does and is the golden's"""
    import zlib
    import fast_chain_emu as FE
    case = PC.case("seam")
    st = PE.EmuSet([case.dictionary(0)])
    enc = PE.EmuEncoders([case.settings[0]])
    assert case.settings[0][1] == 0
    enc.open([0], st)
    state = np.zeros(1, E.FAST_CHAIN_STATE)
    state[0] = enc.state(0)
    ring = np.frombuffer(enc.ring(0), np.uint8)
    blocks, after = FE.encode([np.concatenate([ring, case.contents[0]])], K1, 0, allow_copy=False, state_in=state)
    (n, data), = blocks[0]
    assert n == len(data) and data.startswith(PC.SEAM_PREFIX_START)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_prime_cases.json")) as f:
        golden = {c["name"]: c for c in json.load(f)["cases"]}["seam"]["streams"][0]
    assert golden["calls"][0] == [[n], "%08x" % (zlib.crc32(data) & 0xFFFFFFFF)]
    st = PW.state_words(after[0])
    assert [st["table_crc32"], st["currentOffset"], st["dictSize"]] == golden["final"][2]
