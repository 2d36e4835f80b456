"""The fed frame reader with a dictionary set on the GPU (k4lz4_frame_read_fed_dictset_batch / _device, LZ4FrameFedReaderBatch /
FrameFedReaderDevice with dictionary=), host and device form: logical reads (frame_feed_cases.FedDriver) against the
witness over the WHOLE source (frame_reader_dict_witness.py), with guard bytes around every output slot, store and piece, and every
raw call held to the contract (consumed, need, final)."""
import bisect
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  (before libk4lz4 is loaded: torch must initialise its HIP runtime first)

import frame_dict_cases as FC
import frame_feed_cases as FF
import frame_reader_cases as K
import frame_reader_dict_cases as RC
from frame_reader_dict_gpu import DictFedReaders
from k4os.compression.lz4_amd import DictionarySet, LZ4EncoderSettings, LZ4FrameFedReaderBatch, FrameFedReaderDevice, pack_blocks, _native
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
def test_random_pieces_and_random_counts(dc, E, dset, host):
    """the emulator's sources cut at random places (pieces of 0, 1 - 15, around 64 and up to 192 bytes for the small ones, around a
    block for the others), twelve calls of random counts, OPENs in between; defects come when their bytes do"""
    rng = np.random.default_rng(51 + host)
    src = RC.all_sources(E)
    names, sources = [n for n, _ in src], [s for _, s in src]
    rd = DictFedReaders(dc, len(src), (dset, FC.IDS), host=host)
    ends = [FF.random_ends(rng, len(s), K64 if len(s) > 4000 else 64) if len(s) else [0] for s in sources]
    drv = FF.FedDriver(rd, sources, ends)
    plan = K.read_plan(np.random.default_rng(19), len(src), [K64] * len(src), calls=7, top=3 * K64, rest=RC.WHOLE)
    wits = [RC.witness(s, True, E) for s in sources]
    RC.check_reads(drv, wits, plan, names, opens=np.random.default_rng(5))
    FF.check_code_timing(drv, wits, names)
    RC.check_query(rd, wits, names)
    rd.check_store_guards()
    assert len(drv.starved) > 100 and sum(1 for w in wits if w.failed is None and w.pos == len(w.src)) >= 40


@HOST
def test_every_cut_of_a_small_two_frame_source(dc, E, dset, host):
    """one stream per cut; whenever the call over [0, k) starves, need == e - k, e the end of the field that holds byte k -- inside
    the DictID the bytes that complete the header"""
    source, content, ends = RC.small_fed_source(E)
    cuts = list(range(len(source) + 1))
    n = len(cuts)
    rd = DictFedReaders(dc, n, (dset, FC.IDS), host=host)
    drv = FF.FedDriver(rd, [source] * n, [[k, len(source)] for k in cuts], lambda i, u: ends[bisect.bisect_right(ends, u)])
    wits = [RC.witness(source, True, E) for _ in cuts]
    RC.check_reads(drv, wits, RC.batch_plan([RC.plan_reads(source, True, E, 100)] * n))
    assert any(u == 16 and need == 3 for _, u, need in drv.starved) and set(range(1, 19)) <= {u for _, u, _ in drv.starved}
    q = rd.query()
    assert (q[:, 0] == len(content)).all() and (q[:, 2] == 0).all()
    rd.check_store_guards()


@HOST
def test_mixed_streams_take_both_routes_in_one_call(dc, E, dset, host):
    """64 streams, whole sources as one final piece: the fast path serves the frames of full blocks, hands back the one with a short
    block inside the read, and the general reader has the rest"""
    pool = [(n, s, served) for n, s, served in RC.fast_path_sources(E)] + [(n, s, None) for n, s in RC.multi_frame_sources()] + \
        [(n, s, None) for n, s, with_set in RC.case_sources() if with_set and n.startswith(("lz4-", "hand-chain", "plain-"))]
    src = [pool[i % len(pool)] for i in range(64)]
    names, sources = [n for n, _, _ in src], [s for _, s, _ in src]
    rd = DictFedReaders(dc, 64, (dset, FC.IDS), host=host)
    drv = FF.FedDriver(rd, sources, [[len(s)] for s in sources])
    wits = [RC.witness(s, True, E) for s in sources]
    count = 2 * K64 + K64 // 2
    RC.check_reads(drv, wits, [(np.full(64, count, np.int64), False)], names)
    q = rd.query()
    for i, (name, _, served) in enumerate(src):
        if served is True:
            assert q[i, F.FRQ_FAST] == 3 and q[i, F.FRQ_HANDED_BACK] == 0, (name, q[i])
        elif served is False:
            assert q[i, F.FRQ_FAST] == 0 and q[i, F.FRQ_HANDED_BACK] == 1, (name, q[i])
    RC.check_reads(drv, wits, [(np.full(64, count, np.int64), False)] * 5 + [(np.full(64, RC.WHOLE, np.int64), False)] * 3, names)
    RC.check_query(rd, wits, names)
    rd.check_store_guards()


@HOST
def test_a_null_set_is_the_existing_call(dc, E, host):
    sources = [s for _, s, _ in RC.case_sources()] + [s for _, s in RC.multi_frame_sources()]
    n = len(sources)
    a, b = DictFedReaders(dc, n, None, host=host), DictFedReaders(dc, n, None, host=host, plain=True)
    pieces = [s[:len(s) // 2] for s in sources]
    for p, fin, counts in ((pieces, 0, 70000), ([s[len(s) // 2:] for s in sources], 1, RC.WHOLE)):
        ra = a.call(F.FREAD_READ, p, np.full(n, fin, np.int64), np.full(n, counts, np.int64), False)
        rb = b.call(F.FREAD_READ, p, np.full(n, fin, np.int64), np.full(n, counts, np.int64), False)
        assert (ra[0] == rb[0]).all() and ra[1] == rb[1]
        ok = ra[0] >= 0
        assert (ra[2][ok] == rb[2][ok]).all() and (ra[3][ok] == rb[3][ok]).all()
    assert (a.query() == b.query()).all() and sum(1 for row in a.query() if row[3] == FC.DICTIONARY) >= 30


def test_written_with_a_dictionary_and_fed_in_thousand_byte_pieces(dc, E, dset):
    """encode_frames_device(dictionary=) frames through FrameFedReaderDevice(dictionary=) and LZ4FrameFedReaderBatch in pieces of
    1 000 bytes: the contents"""
    items = [(0, FC.content_of(E[0], 2 * K64 + 100, 400)), (9, FC.content_of(E[9], 30_000, 401)), (-1, FC.content_of(E[0], 5_000, 402)),
             (6, FC.content_of(E[6], K64, 403))]
    for chain in (False, True):
        use = [(e, c) for e, c in items if e >= 0 or not chain]
        n = len(use)
        data_h, off, _ = pack_blocks([np.frombuffer(c, np.uint8) for _, c in use])
        s = LZ4EncoderSettings(ChainBlocks=chain, ContentChecksum=True, BlockChecksum=not chain)
        frames, foff, flen = F.encode_frames_device(dc, torch.from_numpy(data_h).to(dc.device), off.astype(np.int64),
                                                    np.array([len(c) for _, c in use], np.int64), s, dictionary=(dset, FC.IDS),
                                                    dict_index=[e for e, _ in use])
        foff_h = (foff.cpu().numpy() if isinstance(foff, torch.Tensor) else np.asarray(foff)).astype(np.int64)
        flen_h = flen.cpu().numpy()
        rd = FrameFedReaderDevice(dc, n, maxBlockSize=K64, dictionary=(dset, FC.IDS))
        pos, got, left = np.zeros(n, np.int64), [b""] * n, np.array([len(c) for _, c in use], np.int64)
        for _ in range(200):
            if not (left > 0).any():
                break
            upto = np.minimum(pos // 1000 * 1000 + 1000, flen_h)
            out, o_off, o_len, consumed, need = rd.read(frames, foff_h + pos, upto - pos, (upto == flen_h).astype(np.int64), left)
            h, k, cons = out.cpu().numpy(), o_len.cpu().numpy(), consumed.cpu().numpy()
            assert (k >= 0).all()
            got = [g + h[int(o):int(o) + int(x)].tobytes() for g, o, x in zip(got, o_off, k)]
            pos, left = pos + cons, left - k
        assert got == [c for _, c in use]
        hf = frames.cpu().numpy()
        host_frames = [hf[int(o):int(o) + int(k)].tobytes() for o, k in zip(foff_h, flen_h)]
        hb = LZ4FrameFedReaderBatch(n, maxBlockSize=K64, ctx=dc.ctx, dictionary=(dset, FC.IDS))
        acc = [b""] * n
        for at in range(0, int(flen_h.max()), 1000):
            hb.Feed([f[at:at + 1000] for f in host_frames], [at + 1000 >= len(f) for f in host_frames])
            acc = [a + r for a, r in zip(acc, hb.ReadAll([len(c) + 1 - len(a) for (_, c), a in zip(use, acc)]))]
        assert acc == got


def test_refusals(dc, E, dset):
    """K4LZ4_E_ARG before anything is enqueued: a record that is not fed, NULL ids with a set"""
    lib, h = dc.lib, dc.ctx.handle
    ids = np.array(FC.IDS, np.uint32)
    src = np.frombuffer(RC.by_name("hand-indep-match-in-dictionary").frame, np.uint8).copy()
    zero, ln, cnt = np.zeros(1, np.uint64), np.array([src.size], np.uint64), np.array([100], np.int64)
    out, cons, need, fin = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64), np.ones(1, np.int64)
    dst = np.zeros(256, np.uint8)
    for fed in (False, True):
        rec = F.frame_reader_record(K64, lib, fed=fed)
        store = torch.zeros(int(rec.storeBytes) + 256, dtype=torch.uint8, device=dc.device)
        args = [h, C.byref(rec), store.data_ptr(), zero.ctypes.data, src.ctypes.data, zero.ctypes.data, ln.ctypes.data, fin.ctypes.data, dst.ctypes.data,
                zero.ctypes.data, cnt.ctypes.data, out.ctypes.data, cons.ctypes.data, need.ctypes.data, 1]
        assert lib.k4lz4_frame_read_fed_dictset_batch(*args, F.FREAD_RESET, 0, dset.handle, ids.ctypes.data) == (0 if fed else _native.E_ARG)
        if fed:
            assert lib.k4lz4_frame_read_fed_dictset_batch(*args, F.FREAD_READ, 0, dset.handle, None) == _native.E_ARG
            assert "dictIds" in lib.k4lz4_last_error(h).decode()
            assert lib.k4lz4_frame_read_fed_dictset_batch_device(*args, F.FREAD_READ, 0, 100, dset.handle, None, None) == _native.E_ARG
            assert lib.k4lz4_frame_read_fed_dictset_batch(*args, F.FREAD_READ, 0, dset.handle, ids.ctypes.data) == 0 and out[0] == 68
            assert lib.k4lz4_frame_read_fed_batch(*args, F.FREAD_RESET, 0) == 0
            assert lib.k4lz4_frame_read_fed_batch(*args, F.FREAD_READ, 0) == 0 and out[0] == FC.DICTIONARY
