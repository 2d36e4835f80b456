"""The witness for chained encoders and decoders opened from a dictionary (k4lz4_chain_encoder_open_dictset /
k4lz4_chain_decoder_open_dictset).  Test infrastructure only.

Encoder: chain_encoder_witness.WitnessEncoder -- hc_chain_witness.RingEncoder over liblz4 1.9.3's streams -- with this done before
its first TopupAndEncode: the dictionary's last 64 KiB copied to ring positions [0, d), _inputIndex = _inputPointer = d, and
LZ4_loadDict(stream, ring, d) (fast chain) or LZ4_loadDictHC(stream, ring, d) (HC chain).  The dictionary is the stream's prefix:
the first block follows it in the ring.  A fast chain whose dictionary keeps fewer than 8 bytes loads nothing (LZ4_loadDict leaves
the zeroed table with currentOffset 65536) and its ring stays empty.
`counting_encoder` is the same ring over the table codecs (FastTableCodec(current_offset=65536), TableCodec), no bytes.
Decoder: chain_decoder_witness's object after one leading inject."""
from __future__ import annotations

import ctypes as C

import numpy as np

import hc_chain_witness as HW
import fast_chain_witness as FW
from chain_encoder_witness import WitnessEncoder, kind_of

K64 = 65536
HASH_UNIT = 8


def available() -> bool:
    try:
        return HW.Lz4HcCodec.lib().LZ4_versionNumber() == 10903
    except OSError:
        return False


def kept_of(dictionary) -> np.ndarray:
    d = np.ascontiguousarray(np.frombuffer(bytes(dictionary), np.uint8) if isinstance(dictionary, (bytes, bytearray)) else dictionary, np.uint8)
    return d[max(d.size - K64, 0):]


def primed_length(kind: int, dict_len: int) -> int:
    """what the ring holds in front of the first block"""
    d = min(int(dict_len), K64)
    return 0 if kind == 0 or (kind == 2 and d < HASH_UNIT) else d


def _lib():
    L = FW.Lz4FastChainCodec.lib()
    L.LZ4_loadDict.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.LZ4_loadDictHC.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    return L


def prime(w: WitnessEncoder, dictionary) -> None:
    """LZ4Encoder.Create(...)'s object (w, fresh) becomes the primed one"""
    assert w.kind != 0 and w.enc.index == 0 and w.enc.pointer == 0, "a fresh chained encoder"
    kept = kept_of(dictionary)
    d = primed_length(w.kind, kept.size)
    enc, L = w.enc, _lib()
    if d:
        C.memmove(C.addressof(enc.buf), kept.ctypes.data, d)
    enc.index = enc.pointer = d
    if w.kind == 2:
        assert L.LZ4_loadDict(w.codec.ctx, C.addressof(enc.buf), kept.size if d == 0 else d) == d
    else:
        assert L.LZ4_loadDictHC(w.codec.ctx, C.addressof(enc.buf), d) == d


def primed_encoder(chaining, level, block_size, extra_blocks=0, dictionary=None) -> WitnessEncoder:
    w = WitnessEncoder(chaining, level, block_size, extra_blocks)
    if dictionary is not None:
        prime(w, dictionary)
    return w


def counting_encoder(chaining, level, block_size, extra_blocks, dict_len):
    """-> (RingEncoder over a table codec, the codec): the indices alone; dict_len None: no dictionary"""
    kind = kind_of(chaining, level)
    assert kind != 0
    codec = FW.FastTableCodec(current_offset=0 if dict_len is None else K64) if kind == 2 else HW.TableCodec()
    enc = HW.RingEncoder(codec, block_size, extra_blocks)
    if dict_len is None:
        return enc, codec
    d = primed_length(kind, dict_len)
    enc.index = enc.pointer = d
    codec.consumed = d                                        # stream coordinates: the dictionary comes first
    if kind == 2:
        if d:
            codec.dictionary, codec.dict_size = 0, d          # LZ4_loadDict: dictionary = the ring's start, dictSize = d
    else:                                                     # LZ4_loadDictHC: LZ4HC_init_internal(ring), end = ring + d
        codec.base_addr, codec.end = -K64, K64 + d
        codec.dict_limit = codec.low_limit = K64
    return enc, codec


def crc(data) -> int:
    import zlib
    return zlib.crc32(bytes(data)) & 0xFFFFFFFF


def state_words(st) -> dict:
    """a stream context (liblz4's fields, or one FAST_CHAIN_STATE record) as the goldens keep it"""
    table = np.ascontiguousarray(st["hashTable"], "<u4").reshape(-1)
    return {"table_crc32": crc(table.view(np.uint8)), "currentOffset": int(st["currentOffset"]), "dictSize": int(st["dictSize"])}


def play(case):
    """the witness over a case (chain_prime_cases.Case) -> per stream {"open": (ring, state words or None), "calls": [(loaded, out,
    bytes, ring, state words or None)]}; a stream's state is read after every call it has records in"""
    res = []
    for s, (setting, content) in enumerate(zip(case.settings, case.contents)):
        w = primed_encoder(*setting, dictionary=case.dictionary_of(s))
        row = {"open": (w.ring(), state_words(w.codec.state()) if w.kind == 2 else None), "calls": []}
        for call in case.calls:
            loaded, out, data = w.run(call[s])
            row["calls"].append((loaded, out, data, w.ring(), state_words(w.codec.state()) if w.kind == 2 and call[s] else None))
        w.close()
        res.append(row)
    return res


def summary(case, played) -> dict:
    """what the goldens keep of play()'s result, or of a device's results in the same shape: per stream what open leaves and what the
    last call leaves -- [the ring's length, its CRC-32, a fast chain's [table CRC-32, currentOffset, dictSize]] -- and per call
    [recOut, the blocks' CRC-32s as 8 hex digits each].  (recLoaded is host arithmetic: the tests hold it against the model.)"""
    def words(st):
        return None if st is None else [st["table_crc32"], st["currentOffset"], st["dictSize"]]
    streams = []
    for row in played:
        ring, st = row["open"]
        calls = []
        for _, out, data, ring_now, st_now in row["calls"]:
            at, blocks = 0, ""
            for o in out:
                if o:
                    blocks += "%08x" % crc(data[at:at + abs(o)]); at += abs(o)
            assert at == len(data)
            calls.append([[int(x) for x in out], blocks])
            ring_last, st_last = ring_now, (st_now if st_now is not None else st)
            st = st_last
        first = row["open"]
        streams.append({"open": [len(first[0]), crc(first[0]), words(first[1])], "calls": calls,
                        "final": [len(ring_last), crc(ring_last), words(st_last)]})
    return {"name": case.name, "inputs_crc32": inputs_crc(case), "streams": streams}


def inputs_crc(case) -> int:
    parts = [case.dict_buf, case.dict_off.view(np.uint8), case.dict_len.view(np.uint8)]
    for setting, e in zip(case.settings, case.idx):
        parts.append(np.array([int(x) for x in setting] + [e], "<i4").view(np.uint8))
    for call in case.calls:
        for recs in call:
            for data, force, allow in recs:
                parts += [np.array([len(data), int(force), int(allow)], "<u4").view(np.uint8), np.frombuffer(bytes(data), np.uint8)]
    return crc(np.concatenate(parts))


def opened_decoder(chaining, block_size, extra_blocks=0, dictionary=None):
    """LZ4Decoder.Create(...)'s object after one Inject(kept bytes), counted as one applied record -> (decoder, outLen of the open)"""
    import chain_decoder_witness as DW
    dec = DW.create(chaining, block_size, extra_blocks)
    if dictionary is None:
        return dec, 0
    _, out, _ = DW.run(dec, [(True, kept_of(dictionary).tobytes(), 0)])
    return dec, out
