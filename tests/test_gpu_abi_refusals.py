"""The argument checks of the incremental readers' and the per-stream queries' entry points, in host and device form, pinned:
tests/golden/abi_refusals.json holds, per row, one defective call and the code and k4lz4_last_error text the library answered it
with before the entry points came to share their host code.  Every row is a call of n = 1 whose other arguments are small valid
buffers and whose stream sits the call out (count = -1): a row that a check let through would do nothing.  No kernel runs when every
row is refused."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from k4os.compression.lz4_amd import _native
from k4os.compression.lz4_amd import frames as F
from k4os.compression.lz4_amd import legacy as L

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_refusals.json")

READ = ["ctx", "r", "store", "storeOff", "src", "srcOff", "srcLen", "dst", "dstOff", "count", "outLen", "n", "op", "flags"]
FED = ["ctx", "r", "store", "storeOff", "src", "srcOff", "srcLen", "final", "dst", "dstOff", "count", "outLen", "consumed", "need",
       "n", "op", "flags"]
QUERY = ["ctx", "store", "storeOff", "n", "out"]
# entry point -> (its arguments in order, the family of record it takes)
ENTRIES = {}
for _name, _args, _rec in (("k4lz4_frame_read_batch", READ, "frame"), ("k4lz4_frame_read_fed_batch", FED, "frame_fed"),
                           ("k4lz4_legacy_read_batch", READ, "legacy"), ("k4lz4_legacy_read_fed_batch", FED, "legacy_fed")):
    ENTRIES[_name] = (_args, _rec)
    ENTRIES[_name + "_device"] = (_args + ["maxCount", "stream"], _rec)
for _name in ("k4lz4_frame_reader_query", "k4lz4_legacy_reader_query", "k4lz4_chain_decoder_query"):
    ENTRIES[_name] = (QUERY, None)
    ENTRIES[_name + "_device"] = (QUERY + ["stream"], None)

OTHER = {"frame": "frame_fed", "frame_fed": "frame", "legacy": "legacy_fed", "legacy_fed": "legacy"}
STORE_BYTES = 1 << 20


def make_record(lib, family):
    if family.startswith("frame"):
        return F.frame_reader_record(65536, lib, fed=family == "frame_fed")
    return L.legacy_reader_record(4096, lib, fed=family == "legacy_fed")


_buffers = {}


def buffers(device_form):
    """the valid arguments of a call, made once per form: the store is device memory, the arrays host or device memory"""
    if device_form not in _buffers:
        def words(dtype, value, count=8):
            a = np.full(count, value, dtype)
            return torch.from_numpy(a).cuda() if device_form else a
        arrays = {"store": torch.zeros(STORE_BYTES, dtype=torch.uint8, device="cuda"), "storeOff": words(np.uint64, 0),
                  "src": words(np.uint8, 0, 64), "srcOff": words(np.uint64, 0), "srcLen": words(np.uint64, 0), "final": words(np.int64, 0),
                  "dst": words(np.uint8, 0, 64), "dstOff": words(np.uint64, 0), "count": words(np.int64, -1), "outLen": words(np.int64, 0),
                  "consumed": words(np.int64, 0), "need": words(np.int64, 0), "out": words(np.int64, 0, 64)}
        torch.cuda.synchronize()
        _buffers[device_form] = arrays
    return _buffers[device_form]


def call_row(ctx, row):
    """makes the row's call: (return code, k4lz4_last_error text)"""
    lib = ctx.lib
    names, family = ENTRIES[row["fn"]]
    args = {k: a.data_ptr() if torch.is_tensor(a) else a.ctypes.data for k, a in buffers(row["fn"].endswith("_device")).items()}
    args.update({"ctx": ctx.handle, "n": 1, "op": 0, "flags": 0, "maxCount": 0, "stream": None})
    if family:
        rec = make_record(lib, OTHER[family] if row["record"] == "other" else family)
        if row["record"] == "tampered":
            rec.storeBytes += 256
        assert rec.storeBytes <= STORE_BYTES
        args["r"] = C.addressof(rec)
    for k in ("n", "op", "flags"):
        args[k] = row.get(k, args[k])
    for k in row["null"]:
        assert k in names, (row["fn"], k)
        args[k] = None
    rc = getattr(lib, row["fn"])(*[args[k] for k in names])
    text = (lib.k4lz4_last_error(args["ctx"]) or b"").decode()
    return rc, text


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def test_every_refusal_keeps_its_code_and_text(ctx):
    rows = json.load(open(GOLDEN))["rows"]
    assert {r["fn"] for r in rows} == set(ENTRIES)          # the 14 entry points, each with its rows
    wrong = []
    for row in rows:
        rc, text = call_row(ctx, row)
        assert rc != _native.K4LZ4_OK, row                  # nothing was let through, so nothing was enqueued
        if (rc, text) != (row["rc"], row["text"]):
            wrong.append((row["fn"], row["why"], (rc, text), (row["rc"], row["text"])))
    assert not wrong, wrong
