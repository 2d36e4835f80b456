"""What k4lz4_chain_encoder_open_dictset[_device] and k4lz4_chain_decoder_open_dictset[_device] refuse with K4LZ4_E_ARG before
anything is enqueued -- an index outside [-1, nDict), an index >= 0 on an independent encoder, a chained fast
stream with a set that lacks the fast family or under Enforce32, a set on another device (where the machine has two), a misaligned
store -- each leaving records, stores (guard-checked) and result arrays as they were; and the device decoder's bad index: the code,
the untouched store, K4LZ4_E_ARG at the next synchronising call."""
import ctypes as C

import numpy as np
import pytest
import torch

from k4os.compression.lz4_amd import _native, DictionarySet, DICT_HC
from k4os.compression.lz4_amd import encoders as E
import chain_prime_cases as PC
from test_gpu_chain_encoder import HostForm, DeviceForm
from test_gpu_chain_decoder import HostForm as DecoderHostForm, DeviceForm as DecoderDeviceForm

pytestmark = pytest.mark.gpu
K1, K64 = 1024, 65536
SETTINGS = [(True, 0, K1, 0), (True, 9, K1, 1), (False, 0, K1, 0), (True, 0, 4 * K1, 0)]
VALID = [0, 1, -1, 1]


@pytest.fixture(scope="module")
def dicts():
    case = PC.case("first_records")            # entries of 4 096 and 65 536 bytes
    return case, DictionarySet(case.dict_buf, case.dict_off, case.dict_len)


def other_device_set(case):
    if torch.cuda.device_count() < 2:
        return None
    return DictionarySet(case.dict_buf, case.dict_off, case.dict_len, owner=_native.Context(1))


def used_encoders(form, dset, case):
    """encoders that are neither fresh nor empty: opened, and one run behind them"""
    f = (HostForm if form == "host" else DeviceForm)(SETTINGS)
    b = f.b if form == "host" else f.d
    b.open(VALID, dset)
    data = case.contents[0]
    f.run([[(data[:1500], False, True)], [(data[:700], True, True)], [(data[:1024], False, True)], [(data[:100], False, True)]])
    return f, b


def enc_open(form, b, idx, dset, base=None, store_off=None):
    idx = np.ascontiguousarray(idx, np.int32)
    ctx = b.ctx if form == "host" else b.dc.ctx
    base = b._base if base is None else base
    off = b.store_off if store_off is None else store_off
    args = [ctx.handle, b.records, C.c_void_p(base), off.ctypes.data, idx.ctypes.data, dset.handle, b.n]
    if form == "host":
        return ctx.lib.k4lz4_chain_encoder_open_dictset(*args)
    rc = ctx.lib.k4lz4_chain_encoder_open_dictset_device(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("form", ["host", "device"])
def test_encoder_refusals_leave_records_and_stores(form, dicts):
    case, dset = dicts
    f, b = used_encoders(form, dset, case)
    store = b.store
    records, before = [bytes(b.records[i]) for i in range(b.n)], store.cpu().numpy().copy()
    assert any(r.pointer for r in b.records[:b.n])

    def refused(rc, what):
        assert rc == _native.E_ARG, what
        assert [bytes(b.records[i]) for i in range(b.n)] == records, what
        assert np.array_equal(store.cpu().numpy(), before), what
        f.intact()

    for bad in (2, -2, 1 << 30, -(1 << 31)):
        refused(enc_open(form, b, [0, bad, -1, 1], dset), ("index", bad))
    refused(enc_open(form, b, [0, 1, 0, 1], dset), "an independent encoder with a dictionary")
    with DictionarySet(case.dict_buf, case.dict_off, case.dict_len, families=DICT_HC) as hc_only:
        refused(enc_open(form, b, VALID, hc_only), "a chained fast stream and a set without the fast family")
        # the HC stream alone may use it; a chained fast stream without a dictionary too
        assert enc_open(form, b, [-1, 1, -1, -1], hc_only) == 0
        assert b.records[1].pointer == K64 and b.records[0].pointer == 0
        records, before = [bytes(b.records[i]) for i in range(b.n)], store.cpu().numpy().copy()
    lib = _native.load_library()
    lib.k4lz4_set_enforce32(1)
    try:
        refused(enc_open(form, b, VALID, dset), "a chained fast stream under Enforce32")
        assert enc_open(form, b, [-1, 0, -1, -1], dset) == 0          # HC streams are not the 32-bit engine's business
    finally:
        lib.k4lz4_set_enforce32(0)
    records, before = [bytes(b.records[i]) for i in range(b.n)], store.cpu().numpy().copy()
    refused(enc_open(form, b, VALID, dset, base=b._base + 64), "a misaligned store")
    off = b.store_off.copy()
    off[1] += 128
    refused(enc_open(form, b, VALID, dset, store_off=off), "a misaligned stream")
    bad = E.ChainEncoderRecord.from_buffer_copy(b.records[1])
    b.records[1].ringBytes += 8
    records[1] = bytes(b.records[1])
    refused(enc_open(form, b, VALID, dset), "a record nobody made")
    b.records[1] = bad
    records[1] = bytes(bad)
    far = other_device_set(case)
    if far is not None:
        refused(enc_open(form, b, VALID, far), "a set on another device")
        far.close()
    ctx = b.ctx if form == "host" else b.dc.ctx
    assert ctx.lib.k4lz4_chain_encoder_open_dictset(ctx.handle, b.records, C.c_void_p(b._base), b.store_off.ctypes.data, None, dset.handle, b.n) == _native.E_ARG
    assert ctx.lib.k4lz4_chain_encoder_open_dictset(ctx.handle, b.records, C.c_void_p(b._base), b.store_off.ctypes.data,
                                                    np.array(VALID, np.int32).ctypes.data, None, b.n) == _native.E_ARG
    refused(_native.E_ARG, "NULL arguments")
    assert enc_open(form, b, VALID, dset) == 0                         # and what is valid still opens
    assert [r.pointer for r in b.records[:b.n]] == [4096, K64, 0, K64]


@pytest.mark.parametrize("form", ["host", "device"])
def test_optimal_levels_are_not_opened_from_a_dictionary(form, dicts):
    """levels from L10_OPT on with an entry: refused (no witness: DESIGN.md 4.23); without one they open as RESET does, and every
    such stream of the case list is among the refused"""
    case, dset = dicts
    f = (HostForm if form == "host" else DeviceForm)([(True, 10, K1, 0), (True, 12, K1, 2), (True, 9, K1, 0)])
    b = f.b if form == "host" else f.d
    before = b.store.cpu().numpy().copy()
    records = [bytes(b.records[i]) for i in range(b.n)]
    for idx in ([0, -1, 0], [-1, 1, 0], [1, 1, 1]):
        assert enc_open(form, b, idx, dset) == _native.E_ARG
        assert [bytes(b.records[i]) for i in range(b.n)] == records and np.array_equal(b.store.cpu().numpy(), before)
    assert enc_open(form, b, [-1, -1, 1], dset) == 0
    assert [r.pointer for r in b.records[:b.n]] == [0, 0, K64]
    f.intact()
    for name in PC.NAMES:
        c = PC.case(name)
        left_out = set(range(len(c.settings))) - set(PC.opened_streams(c))
        assert left_out == {s for s, (st, e) in enumerate(zip(c.settings, c.idx)) if st[0] and st[1] >= 10 and e >= 0}


def test_decoder_host_form_refusals(dicts):
    case, dset = dicts
    d = DecoderHostForm([(True, K1, 0), (False, K1, 0), (True, K64, 1)])
    b = d.b
    assert b.open([0, -1, 1], dset) == [4096, 0, K64]
    before = b.store.cpu().numpy().copy()
    out = np.full(3, 77, np.int64)

    def call(idx, base=None, off=None, handle=dset.handle):
        idx = np.ascontiguousarray(idx, np.int32)
        return b.lib.k4lz4_chain_decoder_open_dictset(b.ctx.handle, b.records, C.c_void_p(b._base if base is None else base),
                                                      (b.store_off if off is None else off).ctypes.data, idx.ctypes.data, handle, out.ctypes.data, 3)

    def refused(rc, what):
        assert rc == _native.E_ARG and (out == 77).all(), what
        assert np.array_equal(b.store.cpu().numpy(), before), what

    for bad in (2, -2, 1 << 30):
        refused(call([0, bad, 1]), ("index", bad))
    refused(call([0, -1, 1], base=b._base + 16), "a misaligned store")
    off = b.store_off.copy()
    off[2] += 64
    refused(call([0, -1, 1], off=off), "a misaligned stream")
    refused(call([0, -1, 1], handle=None), "no set")
    far = other_device_set(case)
    if far is not None:
        refused(call([0, -1, 1], handle=far.handle), "a set on another device")
        far.close()
    assert call([1, 0, -1]) == 0 and out.tolist() == [K64, -2, 0]      # the independent decoder holds B + 8 = 1 032 bytes


def test_device_decoder_bad_index_reports_the_code_and_leaves_the_store(dicts):
    case, dset = dicts
    d = DecoderDeviceForm([(True, K1, 0), (True, K1, 0), (False, K64, 0), (True, 4 * K1, 2)])
    cd, dev = d.cd, d.dev
    first = cd.open(torch.tensor([1, 1, 0, -1], dtype=torch.int32, device=dev), dset)
    torch.cuda.synchronize()
    assert first.cpu().tolist() == [K64, K64, 4096, 0]
    before = cd.store.cpu().numpy().copy()
    out = torch.full((4,), 77, dtype=torch.int64, device=dev)
    cd.open(torch.tensor([0, 2, -2, 0], dtype=torch.int32, device=dev), dset, out)        # enqueued: the call cannot see the indices
    with pytest.raises(ValueError):
        cd.dc.ctx.synchronize(torch.cuda.current_stream().cuda_stream)
    cd.dc.ctx.synchronize(torch.cuda.current_stream().cuda_stream)                        # the word was taken
    assert out.cpu().tolist() == [4096, E.CDEC_DICT_INDEX, E.CDEC_DICT_INDEX, 4096]
    after = cd.store.cpu().numpy()
    for s in (1, 2):
        o, c = int(d.off[s]), int(d.sizes[s])
        assert np.array_equal(after[o:o + c], before[o:o + c])
    d._stores_intact()
    q = cd.query().cpu().numpy()
    assert q[:, 0].tolist() == [4096, K64, 4096, 4096] and q[:, 2].tolist() == [1, 1, 1, 1]
    kept = case.dictionary(0).tobytes()
    held = d.drain([-4096, -4096, -4096, -4096], [4096] * 4)
    assert held[0] == kept and held[3] == kept and held[2] == kept and held[1] == case.dictionary(1)[-4096:].tobytes()
