"""The chain encoder's host half without a GPU: k4lz4_chain_encoder_init's rounding, the store's size, the
model's counters after every record against the witness (LZ4EncoderBase transcribed), the explicit-length block model against
hc_chain_blocks / fast_chain_blocks, TableCodec's assertions with short blocks in mid-stream, and the bound against the witness's real
block sizes."""
import ctypes as C

import numpy as np
import pytest

from k4os.compression.lz4_amd import _native, encoders as E
import hc_chain_witness as HW
import fast_chain_witness as FW
from chain_encoder_witness import WitnessEncoder, kind_of
import chain_encoder_cases as CC

K1, K64 = 1024, 65536


def plan(rec, records):
    lib = _native.load_library()
    _, _, rlen, rflags, _, _ = E.encoder_record_table([records])
    n = len(records)
    after = E.ChainEncoderRecord()
    loaded, blen = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    assert lib.k4lz4_chain_encode_plan(C.byref(rec), rlen.ctypes.data, rflags.ctypes.data, n, C.byref(after), loaded.ctypes.data, blen.ctypes.data) == 0
    bound = lib.k4lz4_chain_encode_bound(C.byref(rec), rlen.ctypes.data, rflags.ctypes.data, n)
    return after, loaded[:n].tolist(), blen[:n].tolist(), int(bound)


@pytest.mark.parametrize("chaining,level,bs,extra", [(False, 0, 1, 5), (False, 9, 65536, 0), (True, 0, 1000, -3), (True, 2, 1025, 1),
                                                      (True, 3, 65536, 3), (True, 1, 4 << 20, 0), (True, 99, 262144, 2), (True, 12, 1 << 20, 0)])
def test_init_rounding_and_store(chaining, level, bs, extra):
    r = E.chain_encoder_record(chaining, level, bs, extra)
    B = (max(bs, K1) + K1 - 1) // K1 * K1
    assert r.kind == kind_of(chaining, level)
    assert r.blockSize == B
    assert r.extraBlocks == (max(extra, 0) if chaining else 0)
    assert r.level == (min(max(level, 3), 12) if r.kind == 1 else 0 if r.kind == 2 else level)
    ring = (K64 if chaining else 0) + (1 + r.extraBlocks) * B + 32
    assert r.ringBytes == ring
    state = (E.FAST_CHAIN_STATE.itemsize + 255) // 256 * 256 if r.kind == 2 else 0
    assert r.storeBytes % 256 == 0 and state + ring + 8 <= r.storeBytes < state + ring + 8 + 256
    assert _native.load_library().k4lz4_chain_encoder_store_bytes(C.byref(r)) == r.storeBytes


def random_records(rng, B, n):
    recs = []
    for _ in range(n):
        k = int(rng.integers(0, 6))
        ln = 0 if k == 0 else int(rng.integers(1, 64)) if k == 1 else int(rng.integers(1, 3 * B))     # empty, tiny, up to past the free room
        recs.append((np.zeros(ln, np.uint8), bool(rng.integers(0, 4) == 0), bool(rng.integers(0, 2))))
    return recs


@pytest.mark.parametrize("bs", [65536, 262144, 1 << 20, 4 << 20, 1024])
@pytest.mark.parametrize("extra", [0, 1, 3])
@pytest.mark.parametrize("chaining,level", [(False, 0), (True, 0), (True, 9)])
def test_model_counters_follow_the_witness(bs, extra, chaining, level):
    rng = np.random.default_rng(bs + extra * 7 + level)
    w = WitnessEncoder(chaining, level, bs, extra, counting=True)
    rec = E.chain_encoder_record(chaining, level, bs, extra)
    runs = 0
    for _ in range(60):
        recs = random_records(rng, rec.blockSize, int(rng.integers(0, 5)))
        # record by record: the counters after every record
        cur = rec
        for r in recs:
            nb = len(w.codec.blocks)
            d0 = w.codec.dict_size
            loaded, out, _ = w.run([r])
            cur, got_loaded, got_blen, _ = plan(cur, [r])
            assert got_loaded == loaded
            assert (got_blen[0] > 0) == (out[0] != 0)
            if out[0]:
                assert got_blen[0] == w.codec.blocks[nb][0]
            assert (cur.index, cur.pointer) == (w.enc.index, w.enc.pointer)
            if rec.kind == 2:
                assert (cur.dictSize, cur.currentOffset) == (w.codec.dict_size, w.codec.cur)
                assert d0 == w.codec.blocks[nb][1] if out[0] else True
        # and the whole run at once leaves the same record
        whole, _, blen, _ = plan(rec, recs)
        assert bytes(whole) == bytes(cur)
        runs += sum(1 for b in blen if b)
        rec = cur
    assert runs > 0 and rec.blocks == len(w.codec.blocks) and rec.taken == sum(b[0] for b in w.codec.blocks) + w.enc.bytes_ready


def table_rows(lens, B, extra, D, kind, cur=None):
    """k4lz4_chain_table_rows: the library's explicit-length block table (ce_hc_rows / ce_fast_rows, what hc_chain_table_lens /
    fast_chain_table_lens fill the chained encoders' plans from) -> (start, length, dictLimit) or (start, length, dictSize, dictSmall)"""
    lib = _native.load_library()
    lens = np.ascontiguousarray(lens, np.int32)
    rows = np.zeros((max(lens.size, 1), 4), np.int64)
    assert lib.k4lz4_chain_table_rows(kind, D, D if cur is None else cur, lens.ctypes.data, lens.size, B, extra, rows.ctypes.data) == 0
    rows = rows[:lens.size]
    return [tuple(int(x) for x in r[:3]) for r in rows] if kind == 1 else [(int(r[0]), int(r[1]), int(r[2]), bool(r[3])) for r in rows]


def model_rows(rec, records):
    """k4lz4_chain_encode_blocks: the blocks ce_model yields for a run, in window coordinates"""
    lib = _native.load_library()
    _, _, rlen, rflags, _, _ = E.encoder_record_table([records])
    rows = np.zeros((len(records) + 1, 4), np.int64)
    k = lib.k4lz4_chain_encode_blocks(C.byref(rec), rlen.ctypes.data, rflags.ctypes.data, len(records), rows.ctypes.data, len(records) + 1)
    assert 0 <= k <= len(records)
    rows = rows[:k]
    return [tuple(int(x) for x in r[:3]) for r in rows] if rec.kind == 1 else [(int(r[0]), int(r[1]), int(r[2]), bool(r[3])) for r in rows]


@pytest.mark.parametrize("B,extra,D,total", [(K1, 0, 0, 200 * K1 + 5), (K64, 2, 777, 6 * K64), (4 * K1, 1, 4096, 300 * K1 + 1), (K1, 3, 0, K1)])
def test_explicit_length_tables_equal_the_cut_at_B_tables(B, extra, D, total):
    lens = [B] * ((total - D) // B) + ([(total - D) % B] if (total - D) % B else [])
    assert table_rows(lens, B, extra, D, 1) == E.hc_chain_blocks(total, B, extra, D)
    assert table_rows(lens, B, extra, D, 2) == E.fast_chain_blocks(total, B, extra, D)
    assert table_rows(lens, B, extra, D, 2, cur=D + 70000) == E.fast_chain_blocks(total, B, extra, D, currentOffset=D + 70000)


@pytest.mark.parametrize("B", [K1, K64])
@pytest.mark.parametrize("extra", [0, 2])
@pytest.mark.parametrize("D", [0, 3, 4, K64 - 1, K64])
def test_whole_stream_tables_where_the_ring_cuts(B, extra, D):
    """ce_hc_rows / ce_fast_rows (through k4lz4_chain_table_rows) over a whole stream's block lengths, formed here as the library's
    whole-stream tables form them -- B repeated, then the remainder, none for a stream that is all dictionary: the rows equal the
    package's own tables at the lengths where the ring cuts -- nothing or one byte behind the dictionary, a block less or more
    than a byte, the first Commit (pointer + B > L) a byte early and a byte late and the block behind it, and dictionaries around
    the 4 bytes below which LZ4_saveDictHC keeps nothing and around 64 KiB.  (hc_chain_table / fast_chain_table themselves fill
    plans only in front of a launch: the GPU chain tests compare their blocks with the witness; their counting pass is below.)"""
    L = K64 + (1 + extra) * B + 32
    sizes = [D, D + 1, B - 1, B, B + 1, L - B - 1, L - B + 1, L + 1]
    for N in sorted({n for n in sizes if n >= D} | {D + n for n in sizes[2:]}):
        lens = [B] * ((N - D) // B) + ([(N - D) % B] if (N - D) % B else [])
        assert table_rows(lens, B, extra, D, 1) == E.hc_chain_blocks(N, B, extra, D)
        assert table_rows(lens, B, extra, D, 2) == E.fast_chain_blocks(N, B, extra, D)
        assert table_rows(lens, B, extra, D, 2, cur=D + 70000) == E.fast_chain_blocks(N, B, extra, D, currentOffset=D + 70000)


G2 = 1 << 31


def whole_stream_answer(kind, N, B, D, cur):
    """hc_chain_table / fast_chain_table themselves, without a GPU: the host forms of the one-shot chained encoders count the
    blocks before they look at the context, so without one a stream the table accepts is answered "ctx is NULL" and one it
    refuses with the table's own message"""
    lib = _native.load_library()
    byte = (C.c_ubyte * 16)()
    off, out = np.zeros(1, np.uint64), np.zeros(1, np.int32)
    n, bs, extra, dl = np.array([N], np.int64), np.array([B], np.int32), np.zeros(1, np.int32), np.array([D], np.int32)
    streams = (None, byte, off.ctypes.data, n.ctypes.data, bs.ctypes.data, extra.ctypes.data, dl.ctypes.data, 1)
    if kind == 1:
        rc = lib.k4lz4_encode_hc_chain_batch(*streams, byte, off.ctypes.data, out.ctypes.data, 1, 9, 0)
    else:
        st = np.zeros(1, E.FAST_CHAIN_STATE)
        st["currentOffset"], st["dictSize"] = cur or 0, D
        rc = lib.k4lz4_encode_fast_chain_batch(*streams, st.ctypes.data if cur is not None else None, None, byte, off.ctypes.data,
                                               out.ctypes.data, 1, 0)
    assert rc != 0
    return lib.k4lz4_last_error(None).decode()


@pytest.mark.parametrize("B", [K64, 16 * K1])
@pytest.mark.parametrize("D,cur", [(0, None), (0, 70000), (5, 70000), (K64, 3 * K64)])
def test_whole_stream_tables_refuse_2_gb_where_the_block_walk_does(B, D, cur):
    """The refusals stand as they were: LZ4HC on 65536 + a block's start, the fast chain on currentOffset + a block's end, past
    2^31.  The model is the walk block by block; the streams end a block, a byte and nothing around the last one either accepts,
    and one is all dictionary with a state already past 2 GB (no block: nothing to refuse)."""
    def walk(kind, N):
        at = (cur or 0) if kind == 2 else K64 + D
        for pos in range(D, N, B):
            if (at + min(B, N - pos) if kind == 2 else K64 + pos) > G2:
                return True
            at += min(B, N - pos)
        return False
    for kind in (1, 2):
        edge = G2 - K64 if kind == 1 else G2 - (cur or 0) + D        # the stream position where a start (HC) or an end (fast) reaches 2^31
        seen = set()
        for N in (edge - B, edge - 1, edge, edge + 1, edge + B - 1, edge + B, edge + B + 1):
            want = walk(kind, N)
            answer = whole_stream_answer(kind, N, B, D, cur)
            assert ("longer than 2 GB" in answer) == want and (answer == "ctx is NULL") == (not want), (kind, N, answer)
            seen.add(want)
        assert seen == {False, True}
    assert whole_stream_answer(2, D, B, D, G2 + 5 if cur is not None else None) == "ctx is NULL"


@pytest.mark.parametrize("B,extra", [(K1, 0), (K1, 3), (4 * K1, 1), (K64, 0)])
def test_table_codecs_hold_with_short_blocks_in_mid_stream(B, extra):
    """4.9's argument for the new case: blocks contiguous, lowLimit == dictLimit, dictLimit <= s - 65536 after a save -- and the
    fast chain's fields -- when forced blocks shorter than B stand in mid-stream.  The library's table rows and the record model's
    blocks for the same run are both the codecs' rows."""
    rng = np.random.default_rng(B + extra)
    lens = [int(rng.integers(1, B)) if rng.random() < 0.4 else B for _ in range(max(300 * K1 // B, 12))]
    for kind, level, codec in ((1, 9, HW.TableCodec()), (2, 0, FW.FastTableCodec())):
        enc = HW.RingEncoder(codec, B, extra)
        data = np.zeros(B, np.uint8)
        saved_at = []
        for n in lens:
            assert enc.topup(data, 0, n) == n
            before = enc.pointer
            enc.encode(False)                                    # (TableCodec asserts contiguity and lowLimit == dictLimit inside)
            if enc.pointer != before:
                saved_at.append(len(codec.blocks))
        assert len(saved_at) >= 2
        want = [tuple(b) for b in codec.blocks]
        assert table_rows(lens, B, extra, 0, kind) == want
        # the record model, one forced record per block from a fresh encoder: window coordinates are the stream's
        assert model_rows(E.chain_encoder_record(True, level, B, extra), [(np.zeros(n, np.uint8), True, False) for n in lens]) == want
        if kind == 1:
            for k in saved_at:
                if k < len(codec.blocks):
                    s, _, dl = codec.blocks[k]
                    assert dl == s - K64                         # every save keeps exactly 64 KiB: the ring is past 64 KiB + 32 when it saves
        else:
            assert set(codec.arms[1:]) == {"withPrefix64k"} and codec.arms[0] == "usingExtDict"


@pytest.mark.parametrize("chaining,level,extra", [(True, 0, 0), (True, 9, 1), (True, 3, 3)])
def test_model_and_table_agree_on_continued_streams(chaining, level, extra):
    """the two pieces of host arithmetic a call is laid out with: for a stream continued over many runs, the record model's blocks
    equal the table's rows built from its block lengths, the ring's index and the fast chain's currentOffset"""
    rng = np.random.default_rng(level + extra)
    B = 2 * K1
    rec = E.chain_encoder_record(chaining, level, B, extra)
    seen = 0
    for _ in range(80):
        recs = random_records(rng, B, int(rng.integers(1, 8)))
        rows = model_rows(rec, recs)
        if rows:
            assert rows == table_rows([r[1] for r in rows], B, extra, rec.index, rec.kind, cur=rec.currentOffset)
            seen += len(rows)
        rec = plan(rec, recs)[0]
    assert seen > 50 and rec.taken > 3 * K64


@pytest.mark.parametrize("chaining,level", [(True, 0), (True, 9), (False, 0), (False, 3)])
def test_bound_covers_the_witness_blocks(chaining, level):
    rng = np.random.default_rng(level + 2 * chaining)
    B = 2 * K1
    for kind in ("text", "random"):
        data = CC.content(30 * K1, 9, kind)
        for allow in (True, False):
            recs = CC.offer_all(data, B, [int(rng.integers(1, 3 * B)) for _ in range(12)], rng, p_force=0.3, allow=allow)
            w = WitnessEncoder(chaining, level, B, 0)
            _, out, blob = w.run(recs)
            w.close()
            after, _, blen, bound = plan(E.chain_encoder_record(chaining, level, B, 0), recs)
            assert len(blob) <= bound
            assert bound == sum((b if allow else b + b // 255 + 16) for b in blen if b)
            assert [abs(o) if o < 0 else None for o in out if o < 0] == [b for o, b in zip(out, blen) if o < 0]


def test_case_list_saves_take_every_residue():
    assert CC._assert_residues() == set(range(16))
