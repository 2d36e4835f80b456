"""The two-step fast encoder's blocks dealt by the parse's own cost estimate (k4lz4_parse.hpp, ParseCost; the default) and by the
one-kernel encoder's sequence count as before (K4LZ4_NO_PCOST): the order only says which wave takes which block, so both give the
oracle's bytes, block for block, and in a batch of more than nine blocks per CU both use LDS tables, memory tables and migrations."""
import numpy as np
import pytest

from k4os.compression.lz4_amd import LZ4Codec, corpus
from test_gpu_table_address_space import CLASSES, _pack

pytestmark = pytest.mark.gpu


def test_both_orders_give_the_oracles_bytes_and_all_three_placements(oracle, monkeypatch):
    """The batch of tests/test_gpu_table_address_space.py::test_ten_waves_per_workgroup (its recipe; the pieces that module exports
    are imported): nine and a half blocks per CU of 128 ... 65 546 bytes.  Encoded with the new order and with the old one behind its
    switch, in the ordinary launch and in the stamping one (profile mode 4); counters[:, 11] says where each block's table lived:
    4 LDS, 5 memory, 6 memory first and an LDS table later."""
    import torch
    from k4os.compression.lz4_amd.device import DeviceBatch, DeviceCodec
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 9 * cus + cus // 2
    rng = np.random.default_rng(41)
    lengths = [128, 129] * 30 + [2048] * 40
    rest = n - len(lengths)
    lengths += [32768] * (rest - 2 * (rest // 7)) + [65535] * (rest // 7) + [65546] * (rest // 7)
    lengths = [lengths[i] for i in rng.permutation(n)]
    base = [corpus.class_bytes(c, 4 << 20, 43) for c in CLASSES]
    blocks = []
    for i, ln in enumerate(lengths):
        o = (i * 7919 * 64) % ((4 << 20) - ln)
        blocks.append(base[i % 2][o:o + ln])
    data, off, lens = _pack(blocks)
    caps = np.array([LZ4Codec.MaximumOutputSize(int(v)) for v in lens], np.int32)
    want = ref = None
    for env_vars in ({}, {"K4LZ4_NO_PCOST": "1"}):
        monkeypatch.delenv("K4LZ4_NO_PCOST", raising=False)
        monkeypatch.delenv("K4LZ4_PCOST", raising=False)
        for k, v in env_vars.items():
            monkeypatch.setenv(k, v)
        dc = DeviceCodec(0)                                   # the switches are read when a context is created
        src = DeviceBatch.from_host(data, off, lens, dc.device)
        comp = DeviceBatch.empty_slots(caps, dc.device, fill=0xCD)
        if want is None:
            ref = np.full(comp.data.numel(), 0xCD, np.uint8)
            want = oracle.encode_batch(data, off, lens, ref, comp.off.cpu().numpy().astype(np.uint64), caps, threads=16)
        clen = dc.encode(src, comp)
        torch.cuda.synchronize()
        assert np.array_equal(clen.cpu().numpy(), want), env_vars
        assert np.array_equal(comp.data.cpu().numpy(), ref), env_vars
        comp2 = DeviceBatch.empty_slots(caps, dc.device, fill=0xCD)
        clen2, counters = dc.profile(4, src, comp2)
        torch.cuda.synchronize()
        assert np.array_equal(clen2.cpu().numpy(), want) and np.array_equal(comp2.data.cpu().numpy(), ref), env_vars
        stamps = counters.cpu().numpy()[:, 11]
        print(env_vars, "placements:", {int(k): int((stamps == k).sum()) for k in np.unique(stamps)})
        assert set(int(k) for k in np.unique(stamps)) == {4, 5, 6}, env_vars
