"""Records tests/golden/chain_prime_cases.json from the witness (tests/chain_prime_witness.py: liblz4 1.9.3's streams after
LZ4_loadDict / LZ4_loadDictHC on the encoder's ring): for every case of tests/chain_prime_cases.py a CRC-32 of its inputs and per
stream what open leaves and what the last call leaves (the ring's length and CRC-32, a chained fast stream's table CRC-32,
currentOffset and dictSize) and per call recOut and a CRC-32 per block.  tests/test_chain_prime_host.py asserts that the file
equals a fresh recording wherever liblz4 1.9.3 is present.

    python tests/tools/record_chain_prime_goldens.py          (from the repository root)"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import chain_prime_cases as PC          # noqa: E402
import chain_prime_witness as PW        # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "chain_prime_cases.json")


def record() -> dict:
    assert PW.available(), "liblz4 1.9.3 is the witness"
    return {"witness": "liblz4 1.9.3: LZ4_loadDict / LZ4_loadDictHC on the ring, then LZ4_compress_fast_continue / LZ4_compress_HC_continue",
            "cases": [PW.summary(PC.case(n), PW.play(PC.case(n))) for n in PC.NAMES]}


def load() -> dict:
    with open(PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(PATH, "w") as f:
        json.dump(record(), f, separators=(",", ":"))
        f.write("\n")
    print(PATH, os.path.getsize(PATH), "bytes")
