"""The incremental frame readers with a dictionary set through the C ABI on the GPU, for tests/test_gpu_frame_reader_dict.py and
tests/test_gpu_frame_feed_dict.py: n readers with guard bytes around every output slot, store, source / piece, in the host form or
the device form.  dictionary=(DictionarySet, ids): the _dictset calls; dictionary=None with plain=False: the _dictset calls with a
NULL set; plain=True: the calls that take no set.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from k4os.compression.lz4_amd import frames as F

GUARD = 64


def _up(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


def _guarded(items):
    """byte strings -> (buffer with 0xEE guards in front of, between and behind them, offsets, lengths)"""
    lens = np.array([len(p) for p in items], np.uint64)
    off = np.full(len(items), GUARD, np.uint64)
    off[1:] += np.cumsum(lens[:-1] + np.uint64(GUARD))
    buf = np.full(int(lens.sum()) + GUARD * (len(items) + 1), 0xEE, np.uint8)
    for o, p in zip(off, items):
        buf[int(o):int(o) + len(p)] = np.frombuffer(bytes(p), np.uint8)
    return buf, off, lens


class _Readers:
    def __init__(self, dc, n, max_block, host, fast, fed, dictionary, plain):
        self.dc, self.host, self.n, self.fast, self.fed, self.plain = dc, host, n, fast, fed, plain
        self.rec = F.frame_reader_record(max_block, dc.lib, fed=fed)
        self.sb = int(self.rec.storeBytes)
        self.step = self.sb + 256
        self.store = torch.full((n * self.step + 512,), 0xA5, dtype=torch.uint8, device=dc.device)
        self.store_off = 256 + np.arange(n, dtype=np.uint64) * np.uint64(self.step)
        self.d_store_off = _up(self.store_off, dc.device)
        self.set_dictionary(dictionary)
        torch.cuda.synchronize()            # the host form works on the context's own stream: the fill is over before RESET

    def set_dictionary(self, dictionary):
        assert not (self.plain and dictionary is not None)
        self.dset, self.ids = (None, None) if dictionary is None else (dictionary[0], np.ascontiguousarray(dictionary[1], np.uint32))

    def _tail(self):
        return [] if self.plain else [None if self.dset is None else self.dset.handle, None if self.ids is None else self.ids.ctypes.data]

    def _run(self, op, src, soff, lens, final, counts, interactive, d_src=None):
        """one call -> (outLen, [bytes], consumed, need); src / soff / lens host arrays (d_src: the source already on the device)"""
        n, dev = self.n, self.dc.device
        counts = np.ascontiguousarray(counts, np.int64)
        final = np.ascontiguousarray(final, np.int64)
        caps = np.maximum(counts, 0).astype(np.uint64) if op == F.FREAD_READ else np.zeros(n, np.uint64)
        doff = np.full(n, GUARD, np.uint64)
        doff[1:] += np.cumsum(caps[:-1] + np.uint64(GUARD))
        total = int(caps.sum()) + GUARD * (n + 1)
        flags = F.FREAD_INTERACTIVE if interactive else 0
        lib, ctx = self.dc.lib, self.dc.ctx
        name = "k4lz4_frame_read" + ("_fed" if self.fed else "") + ("" if self.plain else "_dictset") + "_batch" + ("" if self.host else "_device")
        fn = getattr(lib, name)
        if self.host:
            dst = np.full(total, 0xCD, np.uint8)
            out, consumed, need = (np.full(n, -999, np.int64) for _ in range(3))
            fed_in = [final.ctypes.data] if self.fed else []
            fed_out = [consumed.ctypes.data, need.ctypes.data] if self.fed else []
            ctx.check(fn(ctx.handle, C.byref(self.rec), self.store.data_ptr(), self.store_off.ctypes.data, src.ctypes.data, soff.ctypes.data,
                         lens.ctypes.data, *fed_in, dst.ctypes.data, doff.ctypes.data, counts.ctypes.data, out.ctypes.data, *fed_out, n, op, flags,
                         *self._tail()))
        else:
            if d_src is None:
                d_src = _up(src, dev)
            d_soff, d_len, d_fin, d_cnt, d_doff = (_up(a, dev) for a in (soff, lens, final, counts, doff))
            d_dst = torch.full((total,), 0xCD, dtype=torch.uint8, device=dev)
            d_out, d_cons, d_need = (torch.full((n,), -999, dtype=torch.int64, device=dev) for _ in range(3))
            fed_in = [d_fin.data_ptr()] if self.fed else []
            fed_out = [d_cons.data_ptr(), d_need.data_ptr()] if self.fed else []
            ctx.check(fn(ctx.handle, C.byref(self.rec), self.store.data_ptr(), self.d_store_off.data_ptr(), d_src.data_ptr(), d_soff.data_ptr(),
                         d_len.data_ptr(), *fed_in, d_dst.data_ptr(), d_doff.data_ptr(), d_cnt.data_ptr(), d_out.data_ptr(), *fed_out, n, op, flags,
                         int(max(counts.max(), 0)) if self.fast else 0, *self._tail(), C.c_void_p(self.dc._stream())))
            dst, out, consumed, need = d_dst.cpu().numpy(), d_out.cpu().numpy(), d_cons.cpu().numpy(), d_need.cpu().numpy()
        mask = np.ones(dst.size, bool)
        for i in range(n):
            mask[int(doff[i]):int(doff[i] + caps[i])] = False
        assert (dst[mask] == 0xCD).all(), "a write outside a stream's slot"
        data = [dst[int(doff[i]):int(doff[i]) + max(int(out[i]), 0)].tobytes() if op == F.FREAD_READ else b"" for i in range(n)]
        return out, data, consumed, need

    def query(self):
        q = np.zeros(self.n * F.FRQ_WORDS, np.int64)
        self.dc.ctx.check(self.dc.lib.k4lz4_frame_reader_query(self.dc.ctx.handle, self.store.data_ptr(), self.store_off.ctypes.data, self.n,
                                                               q.ctypes.data))
        return q.reshape(self.n, F.FRQ_WORDS)

    def check_store_guards(self):
        s = self.store
        body = s[256:256 + self.n * self.step].view(self.n, self.step)
        assert bool((s[:256] == 0xA5).all()) and bool((body[:, self.sb:] == 0xA5).all()) and bool((s[256 + self.n * self.step:] == 0xA5).all()), \
            "a write outside a stream's store"


class DictReaders(_Readers):
    """readers over whole sources: k4lz4_frame_read[_dictset]_batch[_device]"""

    def __init__(self, dc, sources, dictionary=None, max_block=65536, host=False, fast=True, plain=False):
        super().__init__(dc, len(sources), max_block, host, fast, False, dictionary, plain)
        self.src, self.src_off, self.src_len = _guarded(sources)
        self.d_src = None if host else _up(self.src, dc.device)
        self.call(F.FREAD_RESET, np.zeros(self.n, np.int64), False)

    def call(self, op, counts, interactive):
        out, data, _, _ = self._run(op, self.src, self.src_off, self.src_len, np.zeros(self.n, np.int64), counts, interactive, self.d_src)
        return out, data

    def read(self, counts, interactive=False):
        out, data = self.call(F.FREAD_READ, counts, interactive)
        return [None if counts[i] < 0 else (int(out[i]) if out[i] < 0 else data[i]) for i in range(self.n)]

    def open(self, which=None):
        counts = np.array([0 if which is None or i in which else -1 for i in range(self.n)], np.int64)
        out, _ = self.call(F.FREAD_OPEN, counts, False)
        return [None if counts[i] < 0 else int(out[i]) for i in range(self.n)]


class DictFedReaders(_Readers):
    """fed readers: k4lz4_frame_read_fed[_dictset]_batch[_device]; call() is what frame_feed_cases.FedDriver drives"""

    def __init__(self, dc, n, dictionary=None, max_block=65536, host=False, fast=True, plain=False):
        super().__init__(dc, n, max_block, host, fast, True, dictionary, plain)
        self.call(F.FREAD_RESET, [b""] * n, np.zeros(n, np.int64), np.zeros(n, np.int64), False)

    def call(self, op, pieces, final, counts, interactive):
        src, soff, lens = _guarded(pieces)
        return self._run(op, src, soff, lens, final, counts, interactive)
