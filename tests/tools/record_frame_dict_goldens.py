"""Records tests/golden/frame_dict_cases.json from the system liblz4 (1.9.3) for every case of tests/frame_dict_cases.py: what
LZ4F_decompress_usingDict, given the dictionary of the case's entry, decodes the frame to (length and XXH32, or "rejected"), an
XXH32 of the frame, and for the frames liblz4 itself makes (LZ4F_compressBegin_usingCDict + LZ4F_compressUpdate + LZ4F_flush +
LZ4F_compressEnd) the frame's bytes; their contents and every dictionary are regenerated from seeds.
tests/test_frame_dict_emu.py asserts that the file equals a fresh recording wherever liblz4 is present.

    python tests/tools/record_frame_dict_goldens.py          (from the repository root)"""
from __future__ import annotations

import base64
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import frame_dict_cases as FC          # noqa: E402


def record_case(c: FC.Case, E) -> dict:
    e = c.entry if c.witness_entry is None else c.witness_entry
    got = FC.lz4f_decode(c.frame, E[e].tobytes() if e >= 0 else b"", 4 * FC.K64 + 4096)
    if c.content is not None:
        assert got == c.content, c.name          # liblz4 reads back what it wrote
    r = {"frame_xxh32": FC.xxh32(c.frame), "decoded": "rejected" if got is None else [len(got), FC.xxh32(got)]}
    if c.make is not None:
        r["frame"] = base64.b64encode(c.frame).decode()
    return r


def record() -> dict:
    assert FC.liblz4() is not None, "liblz4 1.9.3 is the witness"
    E = FC.entries()
    return {"witness": "liblz4 1.9.3: LZ4F_compressBegin_usingCDict .. LZ4F_compressEnd, LZ4F_decompress_usingDict",
            "cases": {c.name: record_case(c, E) for c in FC.build(make_frames=True)}}


if __name__ == "__main__":
    with open(FC.GOLDEN, "w") as f:
        json.dump(record(), f, separators=(",", ":"))
        f.write("\n")
    print(FC.GOLDEN, os.path.getsize(FC.GOLDEN), "bytes")
