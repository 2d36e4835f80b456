"""Records tests/golden/dict_encode_cases.json from the system liblz4 (1.9.3): for every call of tests/dict_encode_cases.py an xxh32
of its inputs, and per message the size of the block with room to spare, the outLen k4lz4_encode_dict_batch has to report with the
case's cap, an xxh32 of the bytes and, under 128 bytes, the bytes themselves; per dictionary the dictSize LZ4_loadDict leaves and
an xxh32 of its hash table.  tests/test_dict_encode_emu.py asserts that the file equals a fresh recording wherever liblz4 is present.

    python tests/tools/record_dict_goldens.py          (from the repository root)"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dict_encode_cases as DC          # noqa: E402
import dict_encode_witness as W         # noqa: E402
from oracle_lib import Oracle, FrameOracle   # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "dict_encode_cases.json")
_fo = None


def xxh32(data) -> int:
    global _fo
    if _fo is None:
        _fo = FrameOracle(Oracle())
    return _fo.xxh32(np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8))


def inputs_hash(call: DC.Call) -> int:
    """the dictionaries and messages with their lengths, the messages' entries and cap rules"""
    parts = [np.array([len(call.dicts), len(call.msgs)], "<u4").view(np.uint8)]
    for d in call.dicts:
        parts += [np.array([d.size], "<u4").view(np.uint8), d]
    for m, i, c in zip(call.msgs, call.idx, call.caps):
        parts += [np.array([m.size, i, ("bound", "exact", "minus1").index(c)], "<u4").view(np.uint8), m]
    return xxh32(np.concatenate(parts))


def record_call(call: DC.Call) -> dict:
    size, out, hashes, small = [], [], [], {}
    for k, (m, d, how) in enumerate(zip(call.msgs, call.idx, call.caps)):
        r, b = W.encode(m, call.dicts[d], DC.bound(m.size))
        size.append(r)
        if how != "bound":
            r, b = W.encode(m, call.dicts[d], r - (how == "minus1"))
        out.append(W.codec_result(m.size, r))
        hashes.append(xxh32(b) if out[-1] > 0 else 0)
        if 0 < out[-1] < 128 and not call.big:
            small[str(k)] = b.hex()
    states = [W.load_state(d) for d in call.dicts]
    assert all(s["currentOffset"] == DC.K64 for s in states)
    return {"name": call.name, "inputs_xxh32": inputs_hash(call), "size": size, "outLen": out, "xxh32": hashes, "bytes": small,
            "dictSize": [s["dictSize"] for s in states], "table_xxh32": [xxh32(s["hashTable"].view(np.uint8)) for s in states]}


def record() -> dict:
    assert W.available(), "liblz4 1.9.3 is the witness"
    return {"witness": "liblz4 1.9.3: LZ4_loadDict + LZ4_compress_fast_continue(acceleration 1)", "calls": [record_call(c) for c in DC.calls()]}


def load() -> dict:
    with open(PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(PATH, "w") as f:
        json.dump(record(), f, separators=(",", ":"))
        f.write("\n")
    print(PATH, os.path.getsize(PATH), "bytes")
