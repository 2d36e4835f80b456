"""The incremental frame reader with a dictionary set on the GPU (k4lz4_frame_read_dictset_batch / _device, LZ4FrameReaderBatch /
FrameReaderDevice with dictionary=): every call's lengths, codes and bytes against the witness
(frame_reader_dict_witness.py), in the host form and in the device form, with guard bytes around every output slot, store and source."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

import frame_dict_cases as FC
import frame_reader_cases as K
import frame_reader_dict_cases as RC
from frame_reader_dict_gpu import DictReaders
from k4os.compression.lz4_amd import DictionarySet, DICT_HC, LZ4EncoderSettings, LZ4FrameReaderBatch, FrameReaderDevice, pack_blocks, _native
from k4os.compression.lz4_amd import frames as F
from k4os.compression.lz4_amd.device import DeviceCodec

pytestmark = pytest.mark.gpu
K64 = 65536
HOST = pytest.mark.parametrize("host", [False, True], ids=["device", "host"])


@pytest.fixture(scope="module")
def dc():
    return DeviceCodec(0)


@pytest.fixture(scope="module")
def E():
    return FC.entries()


@pytest.fixture(scope="module")
def dset(dc, E):
    with DictionarySet(E, owner=dc) as s:
        yield s


@HOST
def test_case_list_and_multi_frame_sources_in_random_counts(dc, E, dset, host):
    """the emulator's sources -- the case list, sources of several frames, header defects, offsets at and before the first kept byte --
    over twelve calls of random counts (0, 1 - 15, B - 1, B, B + 1, B + 8, 2 B, anything; every third call interactive; some streams
    sit a call out), OPENs on random subsets in between"""
    src = RC.all_sources(E)
    names, sources = [n for n, _ in src], [s for _, s in src]
    rd = DictReaders(dc, sources, (dset, FC.IDS), host=host)
    plan = K.read_plan(np.random.default_rng(7 + host), len(src), [K64] * len(src), calls=7, top=3 * K64, rest=RC.WHOLE)
    assert len(plan) == 12
    wits = [RC.witness(s, True, E) for s in sources]
    RC.check_reads(rd, wits, plan, names, opens=np.random.default_rng(3))
    RC.check_query(rd, wits, names)
    rd.check_store_guards()
    assert sum(1 for w in wits if w.failed is None and w.pos == len(w.src)) >= 40 and sum(1 for w in wits if w.failed == FC.BLOCK) >= 15


@HOST
def test_mixed_streams_take_both_routes_in_one_call(dc, E, dset, host):
    """64 streams in one call -- dictionary and plain, chained and independent, entries of every length: frames of full blocks are
    served by the fast path, the one with a short block inside the read is handed back, everything else is the general reader's"""
    pool = [(n, s, served) for n, s, served in RC.fast_path_sources(E)] + [(n, s, None) for n, s in RC.multi_frame_sources()] + \
        [(n, s, None) for n, s, with_set in RC.case_sources() if with_set and n.startswith(("lz4-", "hand-indep-first-kept", "hand-chain", "plain-"))]
    src = [pool[i % len(pool)] for i in range(64)]
    names, sources = [n for n, _, _ in src], [s for _, s, _ in src]
    lens = {E[c.entry].size for c in FC.cases() if c.entry >= 0 and any(c.name == n for n in names)}
    assert lens >= {1, 3, 4, 100, 65535, 65536, 70000} and any("empty-entry" in n for n in names)
    rd = DictReaders(dc, sources, (dset, FC.IDS), host=host)
    wits = [RC.witness(s, True, E) for s in sources]
    count = 2 * K64 + K64 // 2
    RC.check_reads(rd, wits, [(np.full(64, count, np.int64), False)], names)
    q = rd.query()
    for i, (name, _, served) in enumerate(src):
        if served is True:
            assert q[i, F.FRQ_FAST] == 3 and q[i, F.FRQ_HANDED_BACK] == 0 and q[i, F.FRQ_BLOCKS] == 3, (name, q[i])
        elif served is False:
            assert q[i, F.FRQ_FAST] == 0 and q[i, F.FRQ_HANDED_BACK] == 1, (name, q[i])
        elif not (wits[i].src[4] & 0x20):
            assert q[i, F.FRQ_FAST] == 0 and q[i, F.FRQ_HANDED_BACK] == 0, (name, q[i])       # chained: never planned
    RC.check_reads(rd, wits, [(np.full(64, count, np.int64), False)] * 5 + [(np.full(64, RC.WHOLE, np.int64), False)] * 3, names)
    RC.check_query(rd, wits, names)
    assert all(w.pos == len(w.src) for w in wits if w.failed is None) and sum(1 for w in wits if w.failed is None) >= 55
    rd.check_store_guards()


def test_a_set_of_the_hc_family_only(dc, E):
    src = RC.all_sources(E)[:43]
    with DictionarySet(E, families=DICT_HC, owner=dc) as s:
        rd = DictReaders(dc, [x for _, x in src], (s, FC.IDS))
        wits = [RC.witness(x, True, E) for _, x in src]
        RC.check_reads(rd, wits, [(np.full(len(src), K64 + 1, np.int64), False)] * 2 + [(np.full(len(src), RC.WHOLE, np.int64), False)] * 2,
                       [n for n, _ in src])


@HOST
def test_a_null_set_is_the_existing_call(dc, E, host):
    """outputs and Query() words of the new calls with a NULL set equal the existing calls' on the same sources, DictID frames
    included (K4LZ4_FRAME_DICTIONARY)"""
    sources = [s for _, s, _ in RC.case_sources()] + [s for _, s in RC.multi_frame_sources()]
    a, b = DictReaders(dc, sources, None, host=host), DictReaders(dc, sources, None, host=host, plain=True)
    for counts, inter in ((np.full(len(sources), 70000, np.int64), False), (np.full(len(sources), 9, np.int64), True),
                          (np.full(len(sources), RC.WHOLE, np.int64), False)):
        assert a.read(counts, inter) == b.read(counts, inter)
        assert a.open() == b.open()
    assert (a.query() == b.query()).all()
    assert sum(1 for row in a.query() if row[3] == FC.DICTIONARY) >= 35
    a.check_store_guards()


def test_a_set_without_the_stored_entry_fails_the_stream(dc, E, dset):
    src = [RC.by_name("hand-chain-first-kept-byte-second-block").frame, RC.fast_path_sources(E)[3][1], RC.by_name("lz4-indep-1blk-b0c0s0-e0").frame]
    with DictionarySet(E[:2], owner=dc) as small:
        rd = DictReaders(dc, src, (dset, FC.IDS))
        assert rd.open() == [1, 1, 1]
        rd.set_dictionary((small, FC.IDS[:2]))
        got = rd.read(np.full(3, 3 * K64, np.int64))
        assert got[0] == FC.DICTIONARY and got[1] == FC.DICTIONARY and len(got[2]) == 40000
        assert list(rd.query()[:, 2]) == [2, 2, 0]


def test_written_with_a_dictionary_and_read_back(dc, E, dset):
    """encode_frames_device(dictionary=) frames through FrameReaderDevice(dictionary=) in reads of 100 000 bytes and through
    LZ4FrameReaderBatch; decode_frames_device(dictionary=) gives the same bytes"""
    items = [(e, FC.content_of(E[max(e, 0)], n, 300 + k)) for k, (e, n) in enumerate(((0, 3 * K64 + 100), (6, 200_000), (-1, 70_000), (9, K64),
                                                                                     (5, 150_000), (7, 1)))]
    for chain in (False, True):
        use = [(e, c) for e, c in items if e >= 0 or not chain]
        data_h, off, _ = pack_blocks([np.frombuffer(c, np.uint8) for _, c in use])
        s = LZ4EncoderSettings(ChainBlocks=chain, ContentChecksum=True, BlockChecksum=chain)
        frames, foff, flen = F.encode_frames_device(dc, torch.from_numpy(data_h).to(dc.device), off.astype(np.int64),
                                                    np.array([len(c) for _, c in use], np.int64), s, dictionary=(dset, FC.IDS),
                                                    dict_index=[e for e, _ in use])
        rd = FrameReaderDevice(dc, frames, foff, flen, maxBlockSize=K64, dictionary=(dset, FC.IDS))
        got = [b""] * len(use)
        for _ in range(4):
            out, o_off, o_len = rd.read(np.full(len(use), 100_000, np.int64))
            h, n = out.cpu().numpy(), o_len.cpu().numpy()
            assert (n >= 0).all()
            got = [g + h[int(o):int(o) + int(k)].tobytes() for g, o, k in zip(got, o_off, n)]
        assert got == [c for _, c in use]
        q = rd.query().cpu().numpy()
        assert list(q[:, F.FRQ_BYTES_READ]) == [len(c) for _, c in use] and (chain or q[0, F.FRQ_FAST] > 0)
        dec, d_off, d_len = F.decode_frames_device(dc, frames, foff, flen, dictionary=(dset, FC.IDS))
        hd, nd = dec.cpu().numpy(), d_len.cpu().numpy()
        assert [hd[int(o):int(o) + int(k)].tobytes() for o, k in zip(d_off, nd)] == got
        hf, hn = frames.cpu().numpy(), flen.cpu().numpy()
        host_frames = [hf[int(o):int(o) + int(k)].tobytes() for o, k in zip(foff, hn)]
        hb = LZ4FrameReaderBatch(host_frames, maxBlockSize=K64, ctx=dc.ctx, dictionary=(dset, FC.IDS))
        assert hb.Read([len(c) + 5 for _, c in use]) == got and hb.Read([1] * len(use)) == [b""] * len(use)
        if any(e >= 0 for e, _ in use):
            with pytest.raises(F.NotImplementedException):               # without the set the reader refuses as before
                LZ4FrameReaderBatch(host_frames, maxBlockSize=K64, ctx=dc.ctx).Read([10] * len(use))


def test_refusals(dc, E, dset):
    """K4LZ4_E_ARG before anything is enqueued: a fed record, NULL ids with a set; the existing calls keep refusing the dictionary bit"""
    good = RC.by_name("hand-indep-match-in-dictionary").frame
    lib, h = dc.lib, dc.ctx.handle
    ids = np.array(FC.IDS, np.uint32)
    src = np.frombuffer(good, np.uint8).copy()
    zero, ln, cnt, out = np.zeros(1, np.uint64), np.array([src.size], np.uint64), np.array([100], np.int64), np.zeros(1, np.int64)
    dst = np.zeros(256, np.uint8)
    for fed, ok in ((True, False), (False, True)):
        rec = F.frame_reader_record(K64, lib, fed=fed)
        store = torch.zeros(int(rec.storeBytes) + 256, dtype=torch.uint8, device=dc.device)
        args = [h, C.byref(rec), store.data_ptr(), zero.ctypes.data, src.ctypes.data, zero.ctypes.data, ln.ctypes.data, dst.ctypes.data, zero.ctypes.data,
                cnt.ctypes.data, out.ctypes.data, 1]
        assert lib.k4lz4_frame_read_dictset_batch(*args, F.FREAD_RESET, 0, dset.handle, ids.ctypes.data) == (0 if ok else _native.E_ARG)
        if ok:
            assert lib.k4lz4_frame_read_dictset_batch(*args, F.FREAD_READ, 0, dset.handle, None) == _native.E_ARG
            assert "dictIds" in lib.k4lz4_last_error(h).decode()
            assert lib.k4lz4_frame_read_dictset_batch_device(*args, F.FREAD_READ, 0, 100, dset.handle, None, None) == _native.E_ARG
            assert lib.k4lz4_frame_read_dictset_batch(*args, F.FREAD_READ, 0, dset.handle, ids.ctypes.data) == 0 and out[0] == 68
            assert lib.k4lz4_frame_read_batch(*args, F.FREAD_RESET, 0) == 0
            assert lib.k4lz4_frame_read_batch(*args, F.FREAD_READ, 0) == 0 and out[0] == FC.DICTIONARY
    with pytest.raises(ValueError):
        LZ4FrameReaderBatch([good], ctx=dc.ctx, dictionary=(dset, [1, 2]))
