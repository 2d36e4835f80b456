"""Every decoder kernel the launcher can choose, on device arenas, with hostile input (tests/decoder_cases.py; proven on the CPU by
tests/test_decoder_cases_host.py).  Everything goes through the device forms on torch tensors, so the arena a kernel wrote into is
the arena that is read back: a write outside a slot -- behind it or in front of it, for an accepted or a rejected stream -- shows.

The launcher chooses by blocks per CU (k4lz4_launch.hpp, launch_decode_like): up to 12 the pair kernel that follows the token chain two links
per hop, up to 16 the one-hop pair kernel, up to 24 one wave per block, beyond that the dense build; from more than 6 the pair
kernels run with the late-blocks-first priorities.  A context reads its switches when it is created, so every variant is a
context made under its environment; `k4lz4_last_decode_kernel` says after every launch which kernel ran, and a variant that did
not get its kernel fails.  A mode's case set is larger than 6 blocks per CU, so a variant decodes it in launches of at most that
many streams (the default context's launches are then pair2 without priorities, as the variant table wants), all into one arena;
the dense variant is ONE launch of the cases of at most 8 KiB, tiled until they exceed 24 per CU."""
import os

import numpy as np
import pytest

import decoder_cases as dc
from k4os.compression.lz4_amd import _native

pytestmark = pytest.mark.gpu

K = _native
DECODE_VARIANTS = {     # name: (environment, kernel reported)
    "pair2": ({}, K.DECODE_KERNEL_PAIR2),
    "pair2+pace": ({"K4LZ4_PACE_MIN": "0"}, K.DECODE_KERNEL_PAIR2 | K.DECODE_KERNEL_PACE),
    "pair+pace": ({"K4LZ4_HOP2_MAX": "0", "K4LZ4_PACE_MIN": "0"}, K.DECODE_KERNEL_PAIR | K.DECODE_KERNEL_PACE),     # the benchmark's
    "one-wave": ({"K4LZ4_NO_PAIR": "1"}, K.DECODE_KERNEL_SINGLE),
}
UNPICKLE_VARIANTS = {
    "pair2": ({}, K.DECODE_KERNEL_UNPICKLE_PAIR2),
    "pair": ({"K4LZ4_HOP2_MAX": "0"}, K.DECODE_KERNEL_UNPICKLE_PAIR),
    "one-wave": ({"K4LZ4_NO_PAIR": "1"}, K.DECODE_KERNEL_UNPICKLE_SINGLE),
}
DECODE_MODES = ("plain", "partial", "dict")


def codec_under(env):
    """a DeviceCodec whose context was created under env (the switches are read then), the environment restored"""
    from k4os.compression.lz4_amd.device import DeviceCodec
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return DeviceCodec(0)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def run_on_device(codec, lay, chunk):
    """the layout's cases through the device form of its mode, `chunk` streams per launch, all into one arena on the device.
    Returns (out_len, the arena as it is afterwards, the set of kernels k4lz4_last_decode_kernel reported)."""
    import torch
    from k4os.compression.lz4_amd.device import DeviceBatch
    dev = codec.device
    up = lambda a, t=None: torch.from_numpy(np.array(a if t is None else a.view(t))).to(dev)      # (a copy: the prepared arrays are read-only)
    src, arena = up(lay.src), up(lay.arena)
    soff, slen, doff, dcap = up(lay.src_off, np.int64), up(lay.src_len), up(lay.dst_off, np.int64), up(lay.dst_cap)
    dict_off, dict_len = up(lay.dict_off, np.int64), up(lay.dict_len)
    out = torch.full((lay.n,), -12345, dtype=torch.int32, device=dev)
    kernels = set()
    for a in range(0, lay.n, chunk):
        b = min(a + chunk, lay.n)
        s, d = DeviceBatch(src, soff[a:b], slen[a:b]), DeviceBatch(arena, doff[a:b], dcap[a:b])
        if lay.mode == "unpickle":
            codec.unpickle(s, d, out[a:b])
        elif lay.mode == "dict":
            codec.decode_dict(s, d, arena, dict_off[a:b], dict_len[a:b], out[a:b], flags=dc.FLAGS[lay.mode])
        else:
            codec.decode(s, d, out[a:b], flags=dc.FLAGS[lay.mode])
        kernels.add(codec.ctx.last_decode_kernel())
    # the call-level status of that work: a wave pair that timed out on its partner is a failure of the test, not of a stream
    rc = codec.lib.k4lz4_synchronize(codec.ctx.handle, codec._stream())
    assert rc == _native.K4LZ4_OK, (rc, codec.lib.k4lz4_last_error(codec.ctx.handle))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), arena.cpu().numpy(), kernels


_dense, _baseline = {}, {}


def dense_prepared(mode, oracle):
    """the mode's cases of at most 8 KiB, tiled until one launch of them is the dense kernel's (more than 24 per CU), laid out
    and decoded by the oracle like the mode's own set"""
    if mode not in _dense:
        cs = dc.prepared(mode, oracle)[0]
        small = cs.subset([i for i, (_, cap, _) in enumerate(cs.cases) if cap <= 8192])
        tiled = small.tiled(24 * cu_count() // len(small.cases) + 1)
        lay = dc.layout(tiled)
        want, want_arena = dc.expect(lay, oracle.lib)
        _dense[mode] = (tiled, lay, want, want_arena)
    return _dense[mode]


def baseline(mode, oracle, dense=False):
    """the pair2 kernel without priorities (a default context, launches of at most 6 streams per CU) on the mode's arena: what every
    other variant's arena is compared with; made once"""
    if (mode, dense) not in _baseline:
        lay = (dense_prepared if dense else dc.prepared)(mode, oracle)[1]
        codec = codec_under({})
        _baseline[(mode, dense)] = run_on_device(codec, lay, 6 * cu_count())
        codec.ctx.close()
    return _baseline[(mode, dense)]


def same_as_baseline(lay, want, got_arena, base_arena, what):
    keep = dc.comparable(lay, want)
    diff = np.flatnonzero(got_arena[keep] != base_arena[keep])
    assert diff.size == 0, f"{what}: {diff.size} bytes outside rejected slots differ from the pair2 run's, first at {int(np.flatnonzero(keep)[diff[0]])}"


def run_variant(mode, oracle, env, kernel):
    cs, lay, want, want_arena = dc.prepared(mode, oracle)
    what = f"{mode} {env or 'default context'}"
    base = baseline(mode, oracle)
    if env:
        codec = codec_under(env)
        got, got_arena, kernels = run_on_device(codec, lay, 6 * cu_count())
        codec.ctx.close()
    else:
        got, got_arena, kernels = base
    assert kernels == {kernel}, f"{what}: k4lz4_last_decode_kernel reported {sorted(kernels)}, the variant is {kernel}"
    dc.check(lay, want, want_arena, got, got_arena, what)
    assert np.array_equal(got, base[0])
    same_as_baseline(lay, want, got_arena, base[1], what)


@pytest.mark.parametrize("variant", list(DECODE_VARIANTS))
@pytest.mark.parametrize("mode", DECODE_MODES)
def test_decode_variant_on_device_arena(oracle, mode, variant):
    """one decoder kernel, one mode: the kernel that ran is the variant's; out_len is the oracle's for every stream (the error
    position of a rejected one included); every accepted stream's bytes are the oracle's and the rest of its slot untouched; every
    byte of the arena outside all slots -- both guards of every slot, rejected streams included, and the dictionaries -- is what
    was uploaded; the context reports no trouble; and outside rejected slots the arena is the pair2 run's"""
    run_variant(mode, oracle, *DECODE_VARIANTS[variant])


@pytest.mark.parametrize("variant", list(UNPICKLE_VARIANTS))
def test_unpickle_variant_on_device_arena(oracle, variant):
    """the same for the envelopes' kernels (the one-wave kernel through K4LZ4_NO_PAIR; its count-only route needs more than 64
    pickles per CU and is not taken here)"""
    run_variant("unpickle", oracle, *UNPICKLE_VARIANTS[variant])


@pytest.mark.parametrize("mode", DECODE_MODES)
def test_dense_kernel_on_device_arena(oracle, mode):
    """k4_decode_dense_kernel: ONE launch of more than 24 streams per CU through a default context, against the oracle and against
    the pair2 kernel's run over the same arena (that one in launches of 6 per CU)"""
    cs, lay, want, want_arena = dense_prepared(mode, oracle)
    assert lay.n > 24 * cu_count()
    codec = codec_under({})
    got, got_arena, kernels = run_on_device(codec, lay, lay.n)
    codec.ctx.close()
    assert {k & ~K.DECODE_KERNEL_PACE for k in kernels} == {K.DECODE_KERNEL_DENSE}, f"dense {mode}: k4lz4_last_decode_kernel reported {sorted(kernels)}"
    dc.check(lay, want, want_arena, got, got_arena, f"{mode} dense")
    base_out, base_arena, base_kernels = baseline(mode, oracle, dense=True)
    assert base_kernels == {K.DECODE_KERNEL_PAIR2}, sorted(base_kernels)
    dc.check(lay, want, want_arena, base_out, base_arena, f"{mode} pair2 on the dense variant's arena")
    same_as_baseline(lay, want, got_arena, base_arena, f"{mode} dense")
