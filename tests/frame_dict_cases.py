"""The shared list of cases of the frame reader with a predefined dictionary (k4lz4_decode_frames_dictset): one
set of dictionary entries with their ids, and frames that name them -- made by liblz4 (LZ4F_compressBegin_usingCDict; kept in
tests/golden/frame_dict_cases.json, their contents regenerated from seeds) or assembled here from literal runs and matches, the
smallest shapes at which the reader's kernels can go wrong.  tests/tools/record_frame_dict_goldens.py records what
LZ4F_decompress_usingDict makes of every frame; the emulator test and the GPU test run the list.  Block size is 64 KiB throughout.
Test infrastructure only."""
from __future__ import annotations

import base64
import ctypes as C
import json
import os
import struct
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from dict_encode_cases import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_dict_cases.json")
K64 = 65536
MAGIC = 0x184D2204
EOF, HEADER_SUM, DICTIONARY, BLOCK, CAPACITY, LENGTH = -1, -4, -5, -6, -9, -10


# ---- XXH32 (seed 0), from its definition --------------------------------------------------------------------------------------
_P1, _P2, _P3, _P4, _P5, _M = 2654435761, 2246822519, 3266489917, 668265263, 374761393, 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & _M


def xxh32(data) -> int:
    b = bytes(data)
    n, p = len(b), 0
    if n >= 16:
        v = [(_P1 + _P2) & _M, _P2, 0, (-_P1) & _M]
        words = struct.unpack_from("<%dI" % (n // 16 * 4), b, 0)
        for i in range(0, len(words), 4):
            for k in range(4):
                v[k] = (_rotl((v[k] + words[i + k] * _P2) & _M, 13) * _P1) & _M
        p = n // 16 * 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
    else:
        h = _P5
    h = (h + n) & _M
    while p + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", b, p)[0] * _P3) & _M, 17) * _P4) & _M
        p += 4
    while p < n:
        h = (_rotl((h + b[p] * _P5) & _M, 11) * _P1) & _M
        p += 1
    h ^= h >> 15
    h = (h * _P2) & _M
    h ^= h >> 13
    h = (h * _P3) & _M
    h ^= h >> 16
    return h


# ---- blocks and frames by hand ------------------------------------------------------------------------------------------------
def _length(n: int) -> bytes:
    out = b""
    while n >= 255:
        out += b"\xff"
        n -= 255
    return out + bytes([n])


def seq(lit: bytes, offset: Optional[int] = None, mlen: int = 0) -> bytes:
    """one sequence: the literals, then a match of mlen >= 4 bytes at `offset` back; offset None: the block's last sequence"""
    ll, ml = len(lit), (mlen - 4 if offset is not None else 0)
    out = bytes([(min(ll, 15) << 4) | min(ml, 15)])
    if ll >= 15:
        out += _length(ll - 15)
    out += lit
    if offset is not None:
        out += struct.pack("<H", offset)
        if ml >= 15:
            out += _length(ml - 15)
    return out


def header(flg_bits: int, clen: Optional[int] = None, dict_id: Optional[int] = None) -> bytes:
    """magic, FLG (version 01 | flg_bits), BD (64 KiB), content size, DictID, header checksum byte"""
    flg = 0x40 | flg_bits | (0x08 if clen is not None else 0) | (0x01 if dict_id is not None else 0)
    d = bytes([flg, 0x40])
    if clen is not None:
        d += struct.pack("<Q", clen)
    if dict_id is not None:
        d += struct.pack("<I", dict_id)
    return struct.pack("<I", MAGIC) + d + bytes([(xxh32(d) >> 8) & 0xFF])


def frame(blocks, dict_id: Optional[int], indep: bool, clen: Optional[int] = None, bsum: bool = False, content: Optional[bytes] = None) -> bytes:
    """blocks: [(payload, raw)]; content (the bytes the frame decodes to): writes a content checksum"""
    out = header((0x20 if indep else 0) | (0x10 if bsum else 0) | (0x04 if content is not None else 0), clen, dict_id)
    for payload, raw in blocks:
        out += struct.pack("<I", len(payload) | (0x80000000 if raw else 0)) + payload
        if bsum:
            out += struct.pack("<I", xxh32(payload))
    out += struct.pack("<I", 0)
    if content is not None:
        out += struct.pack("<I", xxh32(content))
    return out


def decode_model(blocks, dictionary: bytes, indep: bool) -> Optional[bytes]:
    """what a frame's blocks decode to, from the format's definition: None when an offset reaches before the history"""
    kept = bytes(dictionary)[-K64:]
    out = bytearray()
    for payload, raw in blocks:
        if raw:
            out += payload
            continue
        hist = bytearray(kept if indep else (kept + bytes(out))[-K64:])
        base = len(hist)
        p = 0
        while True:
            tok = payload[p]; p += 1
            ll = tok >> 4
            if ll == 15:
                while True:
                    c = payload[p]; p += 1; ll += c
                    if c != 255:
                        break
            hist += payload[p:p + ll]; p += ll
            if p >= len(payload):
                break
            off = payload[p] | payload[p + 1] << 8; p += 2
            ml = tok & 15
            if ml == 15:
                while True:
                    c = payload[p]; p += 1; ml += c
                    if c != 255:
                        break
            ml += 4
            if off == 0 or off > len(hist):
                return None
            for _ in range(ml):
                hist.append(hist[-off])
        out += hist[base:]
    return bytes(out)


# ---- liblz4 (the witness; only the recorder and the live comparison need it) ---------------------------------------------------
class _FrameInfo(C.Structure):
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int), ("frameType", C.c_int),
                ("contentSize", C.c_ulonglong), ("dictID", C.c_uint), ("blockChecksumFlag", C.c_int)]


class _Prefs(C.Structure):
    _fields_ = [("frameInfo", _FrameInfo), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint), ("favorDecSpeed", C.c_uint),
                ("reserved", C.c_uint * 3)]


_lz4 = None


def liblz4():
    """liblz4.so.1 with the dictionary frame calls, or None"""
    global _lz4
    if _lz4 is None:
        try:
            L = C.CDLL("liblz4.so.1")
            for name in ("LZ4F_createCDict", "LZ4F_compressBegin_usingCDict", "LZ4F_decompress_usingDict"):
                getattr(L, name)
            L.LZ4F_createCDict.restype = C.c_void_p
            L.LZ4F_createCDict.argtypes = [C.c_char_p, C.c_size_t]
            L.LZ4F_freeCDict.argtypes = [C.c_void_p]
            L.LZ4F_createCompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
            L.LZ4F_createCompressionContext.restype = C.c_size_t
            L.LZ4F_freeCompressionContext.argtypes = [C.c_void_p]
            L.LZ4F_compressBegin_usingCDict.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.POINTER(_Prefs)]
            L.LZ4F_compressUpdate.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p]
            L.LZ4F_flush.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p]
            L.LZ4F_compressEnd.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p]
            for f in (L.LZ4F_compressBegin_usingCDict, L.LZ4F_compressUpdate, L.LZ4F_flush, L.LZ4F_compressEnd, L.LZ4F_decompress_usingDict):
                f.restype = C.c_size_t
            L.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
            L.LZ4F_createDecompressionContext.restype = C.c_size_t
            L.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
            L.LZ4F_decompress_usingDict.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_size_t), C.c_char_p, C.POINTER(C.c_size_t),
                                                    C.c_char_p, C.c_size_t, C.c_void_p]
            L.LZ4F_isError.argtypes = [C.c_size_t]
            _lz4 = L
        except (OSError, AttributeError):
            _lz4 = False
    return _lz4 or None


def lz4f_make(pieces: List[bytes], dictionary: bytes, dict_id: int, linked: bool, bsum: bool, csum: bool, csize: bool, level: int = 0) -> bytes:
    """LZ4F_compressBegin_usingCDict, then per piece LZ4F_compressUpdate + LZ4F_flush, then LZ4F_compressEnd"""
    L = liblz4()
    prefs = _Prefs()
    fi = prefs.frameInfo
    fi.blockSizeID, fi.blockMode, fi.contentChecksumFlag, fi.blockChecksumFlag = 4, 0 if linked else 1, int(csum), int(bsum)
    fi.contentSize, fi.dictID = (sum(len(p) for p in pieces) if csize else 0), dict_id
    prefs.compressionLevel, prefs.autoFlush = level, 1
    cctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(C.byref(cctx), 100))
    cdict = L.LZ4F_createCDict(dictionary, len(dictionary))
    cap = sum(len(p) for p in pieces) * 2 + 4096 * (len(pieces) + 2)
    buf = C.create_string_buffer(cap)
    out = b""

    def step(r):
        nonlocal out
        assert not L.LZ4F_isError(r), r
        out += buf.raw[:r]
    step(L.LZ4F_compressBegin_usingCDict(cctx, buf, cap, cdict, C.byref(prefs)))
    for p in pieces:
        step(L.LZ4F_compressUpdate(cctx, buf, cap, p, len(p), None))
        step(L.LZ4F_flush(cctx, buf, cap, None))
    step(L.LZ4F_compressEnd(cctx, buf, cap, None))
    L.LZ4F_freeCompressionContext(cctx)
    L.LZ4F_freeCDict(cdict)
    return out


def lz4f_decode(data: bytes, dictionary: bytes, cap: int) -> Optional[bytes]:
    """LZ4F_decompress_usingDict over the whole frame; None when liblz4 rejects it or wants more input"""
    L = liblz4()
    dctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(C.byref(dctx), 100))
    dst = C.create_string_buffer(cap + 64)
    out, pos, r = b"", 0, 1
    try:
        while pos < len(data):
            dn, sn = C.c_size_t(cap + 64), C.c_size_t(len(data) - pos)
            r = L.LZ4F_decompress_usingDict(dctx, dst, C.byref(dn), data[pos:], C.byref(sn), dictionary, len(dictionary), None)
            if L.LZ4F_isError(r):
                return None
            out += dst.raw[:dn.value]
            pos += sn.value
            if r == 0:
                break
            if sn.value == 0 and dn.value == 0:
                return None
        return out if r == 0 else None
    finally:
        L.LZ4F_freeDecompressionContext(dctx)


# ---- the set and the cases ----------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    frame: Optional[bytes]            # None: made by liblz4, kept in the golden file
    entry: int                        # the entry the frame has to resolve to (-1: none)
    expect: Optional[int] = None      # a K4LZ4_FRAME_* code; None: decodes to what the golden file records
    cap: str = "size"                 # the target: "size" = what frame_sizes allows, "short" = one byte less than the content
    null_set: bool = False            # the call gets no set
    witness_entry: Optional[int] = None   # the dictionary liblz4 is given (default: `entry`)
    make: Optional[dict] = None       # liblz4-made: lz4f_make's arguments but the dictionary
    content: Optional[bytes] = None   # liblz4-made: what went in


def entries() -> List[np.ndarray]:
    """the set: entry 0 a full 64 KiB window; lengths 0, 1, 3, 4, 65535, 70000 (only the tail is kept); 7 the bytes of 0 again;
    8 other bytes under the id of 0 (never chosen); 9 a hundred bytes"""
    text = synthetic("dickens", 200000, 11)
    xml = synthetic("xml", 80000, 11)
    e = [text[:K64], text[:0], text[500:501], text[600:603], text[700:704], xml[:65535], text[100000:170000], text[:K64].copy(), xml[1000:5000],
         text[180000:180100]]
    return [np.ascontiguousarray(x, np.uint8) for x in e]


IDS = [100, 101, 102, 103, 104, 105, 106, 107, 100, 109]


def content_of(dictionary: np.ndarray, n: int, seed: int) -> bytes:
    """n bytes, mostly a few long pieces of the dictionary's last 16 KiB again and again (within reach from most of a block, and the
    frames stay small) between short runs it does not hold"""
    rng = np.random.default_rng(seed)
    tail = dictionary[-16384:]
    pool = []
    for _ in range(6):
        k = int(rng.integers(1000, 6000))
        s = int(rng.integers(0, max(tail.size - k, 1)))
        pool.append(tail[s:s + k])
    out, have = [], 0
    while have < n:
        if rng.random() < 0.9:
            piece = pool[int(rng.integers(0, len(pool)))]
        else:
            piece = rng.integers(0, 256, int(rng.integers(8, 40)), dtype=np.uint8)
        out.append(piece)
        have += piece.size
    return np.concatenate(out)[:n].tobytes()


def _split(b: bytes, sizes: List[int]) -> List[bytes]:
    out, p = [], 0
    for s in sizes:
        out.append(b[p:p + s])
        p += s
    assert p == len(b)
    return out


def _made(E) -> List[Case]:
    cases = []
    combos = [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)]
    sizes = {1: 40000, 2: K64 + 30000, 4: 3 * K64 + 5000}
    k = 0
    for linked in (False, True):
        for nblk in (1, 2, 4):
            bsum, csum, csize = combos[k % len(combos)]
            entry = (0, 6, 5)[k % 3]
            data = content_of(E[entry], sizes[nblk], 40 + k)
            cases.append(Case(f"lz4-{'linked' if linked else 'indep'}-{nblk}blk-b{bsum}c{csum}s{csize}-e{entry}", None, entry,
                              make=dict(pieces=[data], dict_id=IDS[entry], linked=linked, bsum=bool(bsum), csum=bool(csum), csize=bool(csize)),
                              content=data))
            k += 1
    # short blocks (LZ4F_flush after every piece): blocks that start at 100, 3100 and 68636 bytes of output
    for linked in (False, True):
        data = content_of(E[0], 100 + 3000 + K64 + 70000, 60 + linked)
        cases.append(Case(f"lz4-{'linked' if linked else 'indep'}-short-blocks", None, 0,
                          make=dict(pieces=_split(data, [100, 3000, K64, 70000]), dict_id=IDS[0], linked=linked, bsum=True, csum=True, csize=True),
                          content=data))
    # two entries with the same bytes: the id decides; a duplicate id: the first entry; a high level's frame
    data = content_of(E[0], K64 + 2000, 70)
    cases.append(Case("lz4-linked-same-bytes-entry7", None, 7, make=dict(pieces=[data], dict_id=IDS[7], linked=True, bsum=False, csum=True, csize=False),
                      content=data))
    cases.append(Case("lz4-indep-hc9-duplicate-id", None, 0, make=dict(pieces=[data], dict_id=IDS[8], linked=False, bsum=False, csum=True, csize=False,
                                                                      level=9), content=data))
    return cases


def _hand(E) -> List[Case]:
    rng = np.random.default_rng(5)
    fresh = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    tail = fresh(12)
    cases = []

    def add(name, blocks, entry, indep, expect=None, **kw):
        model = decode_model(blocks, E[entry].tobytes() if entry >= 0 else b"", indep)
        good = expect is None
        assert (model is not None) == good or expect in (LENGTH, CAPACITY), name
        clen = kw.pop("clen", None)
        f = frame(blocks, IDS[entry] if entry >= 0 else None, indep, clen=clen, bsum=kw.pop("bsum", False),
                  content=model if (good and kw.pop("csum", True)) else None)
        cases.append(Case(name, f, entry, expect, **kw))

    for indep in (True, False):
        kind = "indep" if indep else "chain"
        add(f"hand-{kind}-match-in-dictionary", [(seq(fresh(16), 16 + 1000, 40) + seq(tail), False)], 0, indep)
        add(f"hand-{kind}-match-dictionary-into-block", [(seq(fresh(16), 16 + 10, 40) + seq(tail), False)], 0, indep, bsum=True)
    # a second block behind a 100-byte first one: a match wholly in the dictionary, one that straddles its end -> dst[0]
    first = (seq(fresh(60), 60 + 2000, 28) + seq(tail), False)                                          # 100 bytes
    second = (seq(fresh(10), 10 + 100 + 500, 30) + seq(fresh(5), 145 + 7, 50) + seq(tail), False)
    add("hand-chain-second-block-dictionary-and-seam", [first, second], 0, False, clen=100 + 10 + 30 + 5 + 50 + 12)
    add("hand-indep-short-first-block-in-order", [first, (seq(fresh(10), 10 + 500, 30) + seq(tail), False)], 0, True)
    # op of 65534 / 65535 / 65536 at the block start, offset 65535: the dictionary's last byte, dst[0], dst[1]
    for op in (65534, 65535, 65536):
        add(f"hand-chain-op{op}-offset65535", [(fresh(op), True), (seq(b"", 65535, 8) + seq(tail), False)], 0, False)
    add("hand-chain-raw-then-through-it", [(fresh(50), True), (seq(fresh(4), 4 + 50 + 200, 20) + seq(tail), False)], 0, False)
    # an independent frame whose second block reaches back past its start: the dictionary again, never the first block
    full = (seq(fresh(16), 4, K64 - 16 - 12) + seq(tail), False)
    add("hand-indep-second-block-reads-dictionary", [full, (seq(fresh(8), 8 + 300, 20) + seq(tail), False)], 0, True)
    add("hand-indep-second-block-past-small-dictionary", [full, (seq(fresh(8), 8 + 300, 20) + seq(tail), False)], 9, True, expect=BLOCK)
    # dictionary lengths: the first kept byte is reachable, the byte before it is not
    for entry in (2, 3, 4, 9, 5, 6):
        kept = min(E[entry].size, K64)
        lit = 20 if kept < 60000 else 0
        add(f"hand-indep-first-kept-byte-len{E[entry].size}", [(seq(fresh(lit), min(lit + kept, 65535), 8) + seq(tail), False)], entry, True)
        if lit + kept + 1 <= 65535:
            add(f"hand-indep-before-dictionary-len{E[entry].size}", [(seq(fresh(lit), lit + kept + 1, 8) + seq(tail), False)], entry, True, expect=BLOCK)
    add("hand-indep-empty-dictionary", [(seq(fresh(30), 7, 9) + seq(tail), False)], 1, True)
    add("hand-indep-empty-dictionary-offset-before", [(seq(fresh(30), 31, 9) + seq(tail), False)], 1, True, expect=BLOCK)
    # chained: first kept byte of a hundred-byte dictionary from the second block, and the byte before it
    small_first = (seq(fresh(88)) , False)
    add("hand-chain-first-kept-byte-second-block", [small_first, (seq(fresh(10), 10 + 88 + 100, 8) + seq(tail), False)], 9, False)
    add("hand-chain-before-dictionary-second-block", [small_first, (seq(fresh(10), 10 + 88 + 101, 8) + seq(tail), False)], 9, False, expect=BLOCK)
    # headers
    ok_blocks = [(seq(fresh(16), 16 + 1000, 40) + seq(tail), False)]
    good = frame(ok_blocks, IDS[0], True, content=decode_model(ok_blocks, E[0].tobytes(), True))
    cases.append(Case("hostile-unknown-dictid", frame(ok_blocks, 4242, True), -1, DICTIONARY))
    flipped = bytearray(good)
    flipped[6] ^= 0x01                                                      # first DictID byte, checksum as it was
    cases.append(Case("hostile-dictid-byte-flipped", bytes(flipped), -1, HEADER_SUM))
    cases.append(Case("hostile-header-cut-in-dictid", good[:8], -1, EOF))
    cases.append(Case("hostile-dict-frame-without-set", good, -1, DICTIONARY, null_set=True, witness_entry=0))
    plain = [(seq(fresh(40), 9, 30) + seq(tail), False)]
    add("plain-frame-in-dictset-call", plain, -1, True)
    content = decode_model(ok_blocks, E[0].tobytes(), True)
    add("hostile-content-length-wrong", ok_blocks, 0, True, expect=LENGTH, clen=len(content) + 1)
    return cases


def build(make_frames: bool = False) -> List[Case]:
    """every case; the liblz4-made frames come out of the golden file, or with make_frames (the recorder) from liblz4 afresh"""
    E = entries()
    made = _made(E)
    stored = {} if make_frames else load()["cases"]
    for c in made:
        c.frame = lz4f_make(dictionary=E[c.entry].tobytes(), **c.make) if make_frames else base64.b64decode(stored[c.name]["frame"])
    # a target one byte short of the content: no room for the last block
    short = Case("hostile-dstcap-one-short", made[1].frame, made[1].entry, CAPACITY, cap="short", content=made[1].content)
    out = made + [short] + _hand(E)
    assert len({c.name for c in out}) == len(out)
    return out


_cases = None


def cases() -> List[Case]:
    global _cases
    if _cases is None:
        _cases = build()
    return _cases


def load() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)
