"""The witness for many open ILZ4Decoders (k4lz4_chain_decode_batch): frame_reader_witness's transcriptions of
LZ4ChainDecoder (Encoders/LZ4ChainDecoder.cs, its ring and LZ4_streamDecode_t as LL64.LZ4_decompress_safe_continue keeps it) and
LZ4BlockDecoder (Encoders/LZ4BlockDecoder.cs) over the reference's compiled engine, extended by
  * the per-call blockSize (LZ4ChainDecoder.cs:47-52, LZ4BlockDecoder.cs:43-47),
  * Drain / Peek with the reference's range checks (:96-115),
  * DecodeAndDrain (Encoders/LZ4EncoderExtensions.cs:305-323),
  * the state after a throwing call: the object as the exception leaves it (Prepare's move applied, nothing else),
and by the library's own rules: a run of records (run()), the codes, and the refusal of a chained blockSize above
(1 + extraBlocks) * B + 32, with which the reference would write past its buffer after CopyDict.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C

import numpy as np

import frame_reader_witness as FRW
from frame_reader_witness import K1, K64, Defect

DECODE, INJECT, BLOCK_SIZE, TARGET, NOT_RUN, RANGE, NO_DECODER = -1, -2, -3, -4, -5, -6, -7
CDQ_WORDS = 8
INJECT_BIT = 0x80000000


class Code(Exception):
    """the reference's InvalidOperationException (or the library's refusal), as the code the library reports for it"""

    def __init__(self, code):
        self.code = code


class _Common:
    records = bytes_made = last_code = 0

    def drain(self, offset: int, length: int) -> bytes:               # Drain: LZ4ChainDecoder.cs:96-103, LZ4BlockDecoder.cs:75-85
        at = self.output_index + offset
        if at < 0 or length < 0 or at + length > self.output_index:
            raise Code(RANGE)
        return C.string_at(self.base + at, length)

    def peek(self, offset: int) -> bytes:                             # Peek: :106-115 -- the pointer; here the bytes up to the index
        at = self.output_index + offset
        if at < 0 or at > self.output_index:
            raise Code(RANGE)
        return C.string_at(self.base + at, self.output_index - at)

    def fill(self, value: int):
        """what lies behind the index is not the decoder's: a mutant whose output depends on it is one the reference leaves undefined"""
        C.memset(self.base + self.output_index, value, len(self.buf) - self.output_index)

    @property
    def bytes_ready(self):
        return self.output_index


class ChainDecoder(_Common, FRW.ChainDecoder):
    chaining = 1

    def __init__(self, block_size: int, extra_blocks: int = 0):
        FRW.ChainDecoder.__init__(self, block_size, extra_blocks)
        self.extra_blocks = max(extra_blocks, 0)

    def decode(self, src: bytes, block_size: int = 0) -> int:         # :45-61
        if block_size <= 0:
            block_size = self.block_size
        if block_size > (1 + self.extra_blocks) * self.block_size + 32:
            raise Code(BLOCK_SIZE)                                    # the library's own refusal
        if self.output_index + block_size > self.output_length:       # Prepare :117-123
            self.output_index = self._copy_dict(self.output_index)
        decoded = self._continue(bytes(src), self.base + self.output_index, block_size)
        if decoded < 0:
            raise Code(DECODE)
        self.output_index += decoded
        return decoded

    def inject(self, src: bytes) -> int:
        try:
            return FRW.ChainDecoder.inject(self, bytes(src))
        except Defect:
            raise Code(INJECT)

    def prefix(self) -> bytes:
        """what the next block sees in front of it, from the context's own words"""
        n = min(self.prefix_size, K64)
        return C.string_at(self.prefix_end - n, n) if n else b""


class BlockDecoder(_Common, FRW.BlockDecoder):
    chaining = 0
    extra_blocks = 0

    def decode(self, src: bytes, block_size: int = 0) -> int:         # :39-55
        if block_size <= 0:
            block_size = self.block_size
        if block_size > self.block_size:
            raise Code(BLOCK_SIZE)                                    # :46-47
        try:
            return FRW.BlockDecoder.decode(self, bytes(src))
        except Defect:
            raise Code(DECODE)

    def inject(self, src: bytes) -> int:
        try:
            return FRW.BlockDecoder.inject(self, bytes(src))
        except Defect:
            raise Code(INJECT)


def create(chaining, block_size: int, extra_blocks: int = 0):
    """LZ4Decoder.Create"""
    return ChainDecoder(block_size, extra_blocks) if chaining else BlockDecoder(block_size)


def decode_and_drain(decoder, src: bytes, target_length: int):
    """LZ4EncoderExtensions.DecodeAndDrain: (ok, decoded, bytes)"""
    if len(src) <= 0:
        return False, 0, b""
    decoded = decoder.decode(src)
    if decoded <= 0 or target_length < decoded:
        return False, decoded, b""
    return True, decoded, decoder.drain(-decoded, decoded)


def run(decoder, records, drain: bool = False, cap: int = 0):
    """records: [(inject, bytes, blockSize)] applied in order -> (recOut, outLen, the drained bytes)"""
    if not records:
        return [], 0, b""
    rec_out, out, total, fail = [], bytearray(), 0, 0
    for inject, data, bs in records:
        try:
            if inject:
                got = decoder.inject(data)
            elif drain and len(data) == 0:
                rec_out.append(0)                                     # DecodeAndDrain: nothing is decoded
                continue
            else:
                got = decoder.decode(data, bs)
        except Code as c:
            fail = c.code
            break
        decoder.records += 1
        decoder.bytes_made += got
        total += got
        if drain and got:
            if cap - len(out) < got:
                fail = TARGET                                         # DecodeAndDrain's false: the block stays
                break
            out += decoder.drain(-got, got)
        rec_out.append(got)
    if fail:
        rec_out += [fail] + [NOT_RUN] * (len(records) - len(rec_out) - 1)
    decoder.last_code = fail
    return rec_out, (fail or total), bytes(out)


class WitnessDecoders:
    """n decoders behind the interface the emulator and the GPU drivers offer (chain_decoder_cases.play)"""

    def __init__(self, settings):
        self.settings = list(settings)
        self.d = [create(c, b, e) for c, b, e in self.settings]

    def reset(self, which=None):
        for i in (range(len(self.d)) if which is None else which):
            self.d[i] = create(*self.settings[i])

    def run(self, records, drain=False, caps=None):
        res = [run(d, r, drain, caps[i] if caps is not None else 0) for i, (d, r) in enumerate(zip(self.d, records))]
        return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]

    def drain(self, offsets, lengths):
        out = []
        for d, o, n in zip(self.d, offsets, lengths):
            try:
                out.append(d.drain(o, n))
            except Code as c:
                out.append(c.code)
        return out

    def query(self):
        return np.array([[d.output_index, d.block_size, d.records, d.bytes_made, d.last_code, d.chaining, d.extra_blocks, 0] for d in self.d],
                        np.int64)


def record_table(records, guard: int = 0, fill: int = 0xEE):
    """per-stream record lists -> (src, recOff, recLen, recBlockSize, firstRec, nRec), with `guard` bytes around every source"""
    flat = [r for rs in records for r in rs]
    n_rec = np.array([len(rs) for rs in records], np.uint32)
    first = np.zeros(len(records), np.uint64)
    if len(records) > 1:
        first[1:] = np.cumsum(n_rec[:-1].astype(np.uint64))
    lens = np.array([len(r[1]) for r in flat], np.uint64)
    off = np.full(len(flat), guard, np.uint64)
    if len(flat) > 1:
        off[1:] += np.cumsum(lens[:-1] + np.uint64(guard))
    src = np.full(int(lens.sum()) + guard * (len(flat) + 1) + 16, fill, np.uint8)
    for r, o in zip(flat, off):
        src[int(o):int(o) + len(r[1])] = np.frombuffer(bytes(r[1]), np.uint8)
    rec_len = np.array([len(r[1]) | (INJECT_BIT if r[0] else 0) for r in flat], np.uint32)
    rec_bs = np.array([int(r[2]) for r in flat], np.int32)
    return src, off, rec_len, rec_bs, first, n_rec
