"""The chain encoder's staging, write-back and placement kernels under the wave emulator, given the witness's encoded blocks
(DESIGN.md 4.19): the case list's calls with guard bytes around every store and target here and around every window and slot in
the emulator's scratch; the output bytes, recLoaded, recOut and the ring equal the witness's.  Also the placement kernel's own arm
for a target that is too small or a block that did not encode, which the host's bound otherwise keeps from it."""
import ctypes as C

import numpy as np
import pytest

from k4os.compression.lz4_amd import encoders as E
import chain_encoder_cases as CC
import chain_encoder_emu as EMU
from chain_encoder_witness import WitnessEncoder

K1, K64 = 1024, 65536
GUARD = 256

CASES = {
    "records": CC.record_cases,
    "b64k_x0": lambda: CC.big_case(K64, 0, [0, 3]),
    "b64k_x2": lambda: CC.big_case(K64, 2, [0, 9]),
    "b64k_ind": lambda: CC.big_case(K64, 0, [0, 0], chaining=False),
    "small": lambda: tuple(x if k == 0 else [c[:12:2] for c in x] for k, x in enumerate(_small())),
    "mixed": lambda: CC.mixed_case(16, 6, seed=5),
}


def _small():
    settings, calls = CC.small_case()
    return settings[:12:2], calls


class Emu:
    def __init__(self, settings):
        self.n = n = len(settings)
        self.records = (E.ChainEncoderRecord * n)(*[E.chain_encoder_record(*s) for s in settings])
        self.sizes = np.array([r.storeBytes for r in self.records], np.int64)
        self.off = (GUARD + np.concatenate(([0], np.cumsum(self.sizes[:-1] + GUARD)))).astype(np.uint64)
        self.store = np.full(int(self.sizes.sum()) + GUARD * (n + 1), 0xA5, np.uint8)

    def intact(self):
        mask = np.ones(self.store.size, bool)
        for o, c in zip(self.off, self.sizes):
            mask[int(o):int(o) + int(c)] = False
        assert (self.store[mask] == 0xA5).all(), "a write outside a stream's store"

    def ring(self, i):
        r = self.records[i]
        at = int(self.off[i]) + E._ring_at(r)
        return self.store[at:at + r.pointer].tobytes()

    def run(self, records, raw, caps=None, honour=1):
        """raw[s]: the witness's EncodeBlock results of this call, [(encoded, bytes)]"""
        n = self.n
        src, roff, rlen, rflags, first, nrec = E.encoder_record_table(records)
        lib = E._native.load_library()
        if caps is None:
            caps = [lib.k4lz4_chain_encode_bound(C.byref(self.records[i]), rlen[int(f):].ctypes.data, rflags[int(f):].ctypes.data, int(k)) if k else 0
                    for i, (f, k) in enumerate(zip(first, nrec))]
        caps = np.asarray(caps, np.uint64)
        doff = (GUARD + np.concatenate(([0], np.cumsum(caps[:-1] + np.uint64(GUARD))))).astype(np.uint64)
        dst = np.full(int(caps.sum()) + GUARD * (n + 1), 0xCD, np.uint8)
        flat = [b for rs in raw for b in rs]
        enc_len = np.array([b[0] for b in flat] + [0], np.int32)
        blobs = [np.frombuffer(b[1], np.uint8) for b in flat]
        arena, enc_off, _ = E.pack_blocks(blobs) if blobs else (np.zeros(1, np.uint8), np.zeros(1, np.uint64), None)
        nr = max(int(rlen.size), 1)
        loaded, out, olen = np.full(nr, -77, np.int32), np.full(nr, -77, np.int32), np.full(n, -77, np.int64)
        p = lambda a: a.ctypes.data  # noqa: E731
        rc = EMU.lib().k4emu_ce_call(self.records, p(self.store), p(self.off), p(src), p(roff), p(rlen), p(rflags), int(rlen.size), p(first), p(nrec), n,
                                     p(enc_len), p(arena), p(np.ascontiguousarray(enc_off, np.uint64)), len(flat), p(dst), p(doff), p(caps), honour,
                                     p(loaded), p(out), p(olen), 0)
        assert rc == len(flat), rc
        self.intact()
        mask = np.ones(dst.size, bool)
        data = []
        for i in range(n):
            mask[int(doff[i]):int(doff[i]) + int(caps[i])] = False
            used = max(int(olen[i]), 0)
            data.append(dst[int(doff[i]):int(doff[i]) + used].tobytes())
            if olen[i] >= 0:      # (a run the kernel stopped has written the blocks that fitted, inside its target)
                assert (dst[int(doff[i]) + used:int(doff[i]) + int(caps[i])] == 0xCD).all(), "bytes behind the run's total"
        assert (dst[mask] == 0xCD).all(), "a write outside a stream's target"
        cut = lambda a: [a[int(f):int(f) + int(k)].tolist() for f, k in zip(first, nrec)]  # noqa: E731
        return cut(loaded), cut(out), olen.tolist(), data


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_place_the_witness_blocks(name):
    settings, calls = CASES[name]()
    ws = [WitnessEncoder(*s) for s in settings]
    emu = Emu(settings)
    for c, call in enumerate(calls):
        want, raw = [], []
        for w, recs in zip(ws, call):
            k = len(w.codec.raw)
            want.append(w.run(recs) + (w.ring(),))
            raw.append(w.codec.raw[k:])
        fresh_fast = [i for i, r in enumerate(emu.records) if r.kind == 2 and r.currentOffset == 0 and raw[i]]
        loaded, out, olen, data = emu.run(call, raw)
        for i, (wl, wo, wd, wring) in enumerate(want):
            tag = (name, c, i, settings[i])
            assert loaded[i] == wl and out[i] == wo, tag
            assert olen[i] == len(wd) and data[i] == wd, tag
            assert emu.ring(i) == wring, tag
            r = emu.records[i]
            assert (r.index, r.pointer) == (ws[i].enc.index, ws[i].enc.pointer), tag
        for i in fresh_fast:      # a fresh fast chain starts from a zeroed state (the encoders' stand-in hands it through)
            assert not emu.store[int(emu.off[i]):int(emu.off[i]) + E.FAST_CHAIN_STATE.itemsize].any(), (name, c, i)
    for w in ws:
        w.close()


def test_placement_stops_at_the_target_and_at_a_block_that_did_not_encode():
    settings = [(True, 9, K1, 0), (False, 0, K1, 0), (True, 0, K1, 0)]
    data = CC.content(4 * K1, 8)
    run = [[(data[:K1], False, False), (data[K1:K1 + 100], True, False)] for _ in settings]
    ws = [WitnessEncoder(*s) for s in settings]
    want = [w.run(r) for w, r in zip(ws, run)]
    raw = [list(w.codec.raw) for w in ws]
    emu = Emu(settings)
    total = [len(w[2]) for w in want]
    raw[2][1] = (0, b"")                                        # a block the encoder reported as failed
    loaded, out, olen, got = emu.run(run, raw, caps=[total[0] - 1, total[1], total[2]], honour=0)
    assert olen[0] == E.CENC_TARGET and out[0] == [want[0][1][0], 0]          # the first block fits, the second would pass the target
    assert (out[1], olen[1], got[1]) == (want[1][1], total[1], want[1][2])
    assert olen[2] == E.CENC_TARGET and out[2] == [want[2][1][0], 0]
    for w in ws:
        w.close()
