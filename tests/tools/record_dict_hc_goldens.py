"""Records tests/golden/dict_hc_encode_cases.json from the system liblz4 (1.9.3): for every call of tests/dict_hc_encode_cases.py an
xxh32 of its inputs and, per level the call runs at and per message, the size of the block with room to spare, the outLen
k4lz4_encode_dict_hc_batch has to report with the case's cap, an xxh32 of the bytes and, for the first few blocks under 128 bytes, the
bytes themselves; per dictionary the kept length and an xxh32 of the hash heads and of the written chain slots that LZ4_loadDictHC
leaves (the tables do not depend on the level).  tests/test_dict_hc_encode_emu.py asserts that the file equals a fresh recording
wherever liblz4 is present.

    python tests/tools/record_dict_hc_goldens.py          (from the repository root)"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import dict_hc_encode_cases as HC          # noqa: E402
import dict_hc_encode_witness as W         # noqa: E402
from record_dict_goldens import inputs_hash, xxh32      # noqa: E402,F401

PATH = os.path.join(ROOT, "tests", "golden", "dict_hc_encode_cases.json")
BYTES_KEPT = 6      # per call and level


def table_hashes(heads: np.ndarray, chain: np.ndarray, kept: int):
    """(xxh32 of the 32768 heads, xxh32 of the chain slots k < kept - 3: the only ones LZ4_loadDictHC writes)"""
    return xxh32(np.ascontiguousarray(heads, "<u4").view(np.uint8)), xxh32(np.ascontiguousarray(chain[:max(kept - 3, 0)], "<u2").view(np.uint8))


def record_level(call, level: int) -> dict:
    size, out, hashes, small = [], [], [], {}
    for k, (m, d, how) in enumerate(zip(call.msgs, call.idx, call.caps)):
        r, b = W.encode(m, call.dicts[d], HC.DC.bound(m.size), level)
        size.append(r)
        if how != "bound":
            r, b = W.encode(m, call.dicts[d], r - (how == "minus1"), level)
        out.append(W.codec_result(m.size, r))
        hashes.append(xxh32(b) if out[-1] > 0 else 0)
        if 0 < out[-1] < 128 and len(small) < BYTES_KEPT:
            small[str(k)] = b.hex()
    return {"size": size, "outLen": out, "xxh32": hashes, "bytes": small}


def record_call(call) -> dict:
    tabs = []
    for d in call.dicts:
        st = W.load_state(d)
        tabs.append(table_hashes(st["hashTable"], st["chainTable"], min(d.size, HC.K64)))
    return {"name": call.name, "inputs_xxh32": inputs_hash(call), "levels": {str(lv): record_level(call, lv) for lv in call.levels},
            "keptLen": [min(d.size, HC.K64) for d in call.dicts], "heads_xxh32": [t[0] for t in tabs], "chain_xxh32": [t[1] for t in tabs]}


def record() -> dict:
    assert W.available(), "liblz4 1.9.3 is the witness"
    return {"witness": "liblz4 1.9.3: LZ4_resetStreamHC_fast + LZ4_loadDictHC + LZ4_compress_HC_continue", "calls": [record_call(c) for c in HC.calls()]}


def load() -> dict:
    with open(PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(PATH, "w") as f:
        json.dump(record(), f, separators=(",", ":"))
        f.write("\n")
    print(PATH, os.path.getsize(PATH), "bytes")
