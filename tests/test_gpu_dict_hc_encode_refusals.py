"""What k4lz4_encode_dict_hc_batch and k4lz4_encode_dict_hc_batch_device refuse with K4LZ4_E_ARG before anything runs: levels below 3
(the message names the fast entry point), levels 10 - 12, the 32-bit engine (K4LZ4_FLAG_X32 and a process under
k4lz4_set_enforce32(1)), any other flag, a negative dictLen, n or nDict, a dictIdx outside the list (host form: the device form cannot
see the indices, tests/test_gpu_dict_hc_encode.py has its answer); and that an empty dictionary, one of 1 - 3 bytes and an empty batch
are not refused."""
import ctypes as C

import numpy as np
import pytest
import torch

from k4os.compression.lz4_amd import _native, LZ4Level

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _native.Context(0)


def arrays(device_form):
    """one message of 100 bytes, two dictionaries (50 and 0 bytes): everything valid"""
    a = {"src": np.arange(100, dtype=np.uint8), "srcOff": np.zeros(1, np.uint64), "srcLen": np.full(1, 100, np.int32),
         "dst": np.zeros(200, np.uint8), "dstOff": np.zeros(1, np.uint64), "dstCap": np.full(1, 200, np.int32), "outLen": np.full(1, 77, np.int32),
         "dictIdx": np.zeros(1, np.int32), "dict": np.arange(50, dtype=np.uint8)}
    if device_form:
        a = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    return a


def call(ctx, device_form, level=LZ4Level.L03_HC, flags=0, n=1, dict_idx=None, dict_len=(50, 0), n_dict=2):
    a = arrays(device_form)
    if dict_idx is not None:
        a["dictIdx"] = torch.tensor([dict_idx], dtype=torch.int32).cuda() if device_form else np.array([dict_idx], np.int32)
    p = (lambda t: t.data_ptr()) if device_form else (lambda v: v.ctypes.data)
    dict_off = np.array([0, 50], np.uint64)
    dlen = np.array(dict_len, np.int32)
    args = [ctx.handle, p(a["src"]), p(a["srcOff"]), p(a["srcLen"]), p(a["dst"]), p(a["dstOff"]), p(a["dstCap"]), p(a["outLen"]), n, int(level),
            flags, p(a["dictIdx"]), p(a["dict"]), dict_off.ctypes.data, dlen.ctypes.data, n_dict]
    if device_form:
        rc = ctx.lib.k4lz4_encode_dict_hc_batch_device(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        out = a["outLen"].cpu().numpy()
    else:
        rc = ctx.lib.k4lz4_encode_dict_hc_batch(*args)
        out = a["outLen"]
    return rc, int(out[0]), (ctx.lib.k4lz4_last_error(ctx.handle) or b"").decode()


@pytest.mark.parametrize("device_form", [False, True])
def test_refusals(ctx, device_form):
    for level in (LZ4Level.L00_FAST, 1, 2, -1):
        rc, out, msg = call(ctx, device_form, level=level)
        assert rc == _native.E_ARG and out == 77 and "k4lz4_encode_dict_batch" in msg
    for level in (LZ4Level.L10_OPT, LZ4Level.L11_OPT, LZ4Level.L12_MAX):
        rc, out, msg = call(ctx, device_form, level=level)
        assert rc == _native.E_ARG and out == 77 and "10 - 12" in msg
    rc, out, msg = call(ctx, device_form, flags=_native.FLAG_X32)
    assert rc == _native.E_ARG and out == 77 and "32-bit" in msg
    ctx.lib.k4lz4_set_enforce32(1)
    try:
        rc, out, msg = call(ctx, device_form)
    finally:
        ctx.lib.k4lz4_set_enforce32(0)
    assert rc == _native.E_ARG and out == 77 and "32-bit" in msg
    for flags in (_native.FLAG_ALLOW_COPY, _native.FLAG_RAW_RETURN, _native.FLAG_NO_REORDER):
        rc, out, _ = call(ctx, device_form, flags=flags)
        assert rc == _native.E_ARG and out == 77
    rc, out, msg = call(ctx, device_form, dict_len=(50, -1))
    assert rc == _native.E_ARG and out == 77 and "dictLen" in msg
    rc, out, _ = call(ctx, device_form, n_dict=-1)
    assert rc == _native.E_ARG and out == 77
    rc, out, _ = call(ctx, device_form, n=-1)
    assert rc == _native.E_ARG and out == 77


def test_host_form_refuses_an_index_outside_the_list(ctx):
    for bad in (2, -1, 1 << 30):
        rc, out, msg = call(ctx, False, dict_idx=bad)
        assert rc == _native.E_ARG and out == 77 and "dictIdx" in msg


@pytest.mark.parametrize("device_form", [False, True])
def test_what_is_not_refused(ctx, device_form):
    for level in (LZ4Level.L03_HC, LZ4Level.L06_HC, LZ4Level.L09_HC):
        rc, out, _ = call(ctx, device_form, level=level)
        assert rc == 0 and 0 < out <= 116
    rc, out, _ = call(ctx, device_form, dict_idx=1)          # the empty dictionary
    assert rc == 0 and 0 < out <= 116
    for short in (0, 1, 2, 3):
        rc, out, _ = call(ctx, device_form, dict_len=(short, 0))
        assert rc == 0 and 0 < out <= 116
    rc, out, _ = call(ctx, device_form, n=0)
    assert rc == 0 and out == 77
    rc, out, _ = call(ctx, device_form, n=0, n_dict=0)
    assert rc == 0 and out == 77
    ctx.synchronize(torch.cuda.current_stream().cuda_stream)
