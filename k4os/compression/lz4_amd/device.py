"""Device-resident batches: the roofline path.  Buffers are torch tensors on the GPU (torch is
used for device memory and streams only); the kernels are reached through the *_device entry
points of the C ABI with raw device pointers."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native
from .codec import LZ4Level


def _dp(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


@dataclass
class DeviceBatch:
    """n independent blocks in one packed device buffer"""
    data: torch.Tensor      # uint8
    off: torch.Tensor       # int64 holding uint64 offsets
    length: torch.Tensor    # int32 (lengths for a source batch, capacities for a target batch)

    @property
    def n(self) -> int:
        return int(self.length.numel())

    @staticmethod
    def from_host(data: np.ndarray, off: np.ndarray, length: np.ndarray, device) -> "DeviceBatch":
        d = torch.from_numpy(np.ascontiguousarray(data)).to(device, non_blocking=False)
        o = torch.from_numpy(np.ascontiguousarray(off).view(np.int64)).to(device)
        ln = torch.from_numpy(np.ascontiguousarray(length, dtype=np.int32)).to(device)
        return DeviceBatch(d, o, ln)

    @staticmethod
    def empty_slots(caps: np.ndarray, device, align: int = 16, fill: Optional[int] = None) -> "DeviceBatch":
        caps = np.asarray(caps, dtype=np.int64).clip(min=0)
        padded = (caps + (align - 1)) // align * align
        off = np.zeros(len(caps), dtype=np.int64)
        if len(caps) > 1:
            off[1:] = np.cumsum(padded[:-1])
        total = int(padded.sum()) + 64
        if fill is None:
            data = torch.empty(total, dtype=torch.uint8, device=device)
        else:
            data = torch.full((total,), fill, dtype=torch.uint8, device=device)
        return DeviceBatch(data, torch.from_numpy(off).to(device), torch.from_numpy(caps.astype(np.int32)).to(device))


class DeviceCodec:
    """Batched LZ4Codec / LZ4Pickler on HBM-resident data; asynchronous on the current torch stream."""

    def __init__(self, device: Optional[int] = None):
        if not torch.cuda.is_available():
            raise _native.NativeLibraryError("no GPU visible: the device path has no CPU fallback")
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.ctx = _native.Context(self.device_index)
        self.lib = self.ctx.lib

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _call(self, fn, src: DeviceBatch, dst: DeviceBatch, out_len: torch.Tensor, *tail):
        assert src.n == dst.n == out_len.numel() and out_len.dtype == torch.int32
        rc = fn(self.ctx.handle, _dp(src.data), _dp(src.off), _dp(src.length), _dp(dst.data), _dp(dst.off),
                _dp(dst.length), _dp(out_len), src.n, *tail, C.c_void_p(self._stream()))
        self.ctx.check(rc)
        return out_len

    def new_out_len(self, n: int) -> torch.Tensor:
        return torch.empty(n, dtype=torch.int32, device=self.device)

    def encode(self, src: DeviceBatch, dst: DeviceBatch, out_len: Optional[torch.Tensor] = None,
               level: LZ4Level = LZ4Level.L00_FAST, flags: int = 0) -> torch.Tensor:
        out_len = self.new_out_len(src.n) if out_len is None else out_len
        return self._call(self.lib.k4lz4_encode_batch_device, src, dst, out_len, int(level), flags)

    def decode(self, src: DeviceBatch, dst: DeviceBatch, out_len: Optional[torch.Tensor] = None,
               flags: int = 0) -> torch.Tensor:
        out_len = self.new_out_len(src.n) if out_len is None else out_len
        return self._call(self.lib.k4lz4_decode_batch_device, src, dst, out_len, flags)

    def decode_dict(self, src: DeviceBatch, dst: DeviceBatch, dictionaries: torch.Tensor, dict_off: torch.Tensor, dict_len: torch.Tensor,
                    out_len: Optional[torch.Tensor] = None, flags: int = 0) -> torch.Tensor:
        """block i decoded against dictionaries[dict_off[i]:+dict_len[i]] (k4lz4_decode_dict_batch_device; device tensors: uint8,
        int64 holding uint64 offsets, int32)"""
        out_len = self.new_out_len(src.n) if out_len is None else out_len
        assert dict_off.numel() == dict_len.numel() == src.n and dict_len.dtype == torch.int32
        return self._call(lambda *a: self.lib.k4lz4_decode_dict_batch_device(*a[:-1], _dp(dictionaries), _dp(dict_off), _dp(dict_len), a[-1]),
                          src, dst, out_len, flags)

    def encode_dict(self, src: DeviceBatch, dst: DeviceBatch, dict_idx: torch.Tensor, dictionaries: torch.Tensor, dict_off: np.ndarray,
                    dict_len: np.ndarray, out_len: Optional[torch.Tensor] = None, level: LZ4Level = LZ4Level.L00_FAST,
                    flags: int = 0) -> torch.Tensor:
        """message i encoded against entry dict_idx[i] (device int32 tensor) of the list dictionaries[dict_off[d]:+dict_len[d]]
        (device bytes; the list's two arrays are HOST arrays): k4lz4_encode_dict_batch_device below L03_HC,
        k4lz4_encode_dict_hc_batch_device at L03_HC .. L09_HC"""
        out_len = self.new_out_len(src.n) if out_len is None else out_len
        doff = np.ascontiguousarray(dict_off, dtype=np.uint64)
        dlen = np.ascontiguousarray(dict_len, dtype=np.int32)
        assert doff.size == dlen.size and dict_idx.numel() == src.n and dict_idx.dtype == torch.int32
        if doff.size and int((doff + dlen.clip(min=0).astype(np.uint64)).max()) > dictionaries.numel():
            raise ValueError("a dictionary exceeds the dictionary buffer")
        fn = self.lib.k4lz4_encode_dict_hc_batch_device if int(level) >= int(LZ4Level.L03_HC) else self.lib.k4lz4_encode_dict_batch_device
        return self._call(fn, src, dst, out_len, int(level), flags, _dp(dict_idx), _dp(dictionaries),
                          doff.ctypes.data if doff.size else None, dlen.ctypes.data if dlen.size else None, int(doff.size))

    def encode_dictset(self, src: DeviceBatch, dst: DeviceBatch, dict_idx: torch.Tensor, dictionaries, out_len: Optional[torch.Tensor] = None,
                       level: LZ4Level = LZ4Level.L00_FAST, flags: int = 0) -> torch.Tensor:
        """encode_dict with the list being a codec.DictionarySet (k4lz4_encode_dictset_batch_device): the same blocks, and nothing is
        loaded per call -- the cost, order and encode kernels run on the set's memory"""
        out_len = self.new_out_len(src.n) if out_len is None else out_len
        assert dict_idx.numel() == src.n and dict_idx.dtype == torch.int32
        return self._call(self.lib.k4lz4_encode_dictset_batch_device, src, dst, out_len, int(level), flags, _dp(dict_idx), dictionaries.handle)

    def decode_dictset(self, src: DeviceBatch, dst: DeviceBatch, dict_idx: torch.Tensor, dictionaries, out_len: Optional[torch.Tensor] = None,
                       flags: int = 0) -> torch.Tensor:
        """block i decoded against entry dict_idx[i] (device int32 tensor; -1: no dictionary) of a codec.DictionarySet
        (k4lz4_decode_dictset_batch_device)"""
        out_len = self.new_out_len(src.n) if out_len is None else out_len
        assert dict_idx.numel() == src.n and dict_idx.dtype == torch.int32
        return self._call(self.lib.k4lz4_decode_dictset_batch_device, src, dst, out_len, flags, _dp(dict_idx), dictionaries.handle)

    def dict_hc_state(self, d: int):
        """what LZ4_loadDictHC left for entry d of the most recent encode_dict call's list at an HC level (k4lz4_encode_dict_hc_state):
        (hashTable: 32768 x uint32, chainTable: 65536 x uint16, kept length).  Waits for that call."""
        heads, chain, kept = np.zeros(32768, np.uint32), np.zeros(65536, np.uint16), np.zeros(1, np.int32)
        self.ctx.check(self.lib.k4lz4_encode_dict_hc_state(self.ctx.handle, int(d), heads.ctypes.data, chain.ctypes.data, kept.ctypes.data))
        return heads, chain, int(kept[0])

    def dict_state(self, d: int) -> np.ndarray:
        """the stream context LZ4_loadDict left for entry d of the most recent encode_dict call's list (k4lz4_encode_dict_state):
        one FAST_CHAIN_STATE record.  Waits for that call."""
        from .encoders import FAST_CHAIN_STATE
        st = np.zeros(1, FAST_CHAIN_STATE)
        self.ctx.check(self.lib.k4lz4_encode_dict_state(self.ctx.handle, int(d), st.ctypes.data))
        return st

    def pickle(self, src: DeviceBatch, dst: DeviceBatch, out_len: Optional[torch.Tensor] = None,
               level: LZ4Level = LZ4Level.L00_FAST, flags: int = 0) -> torch.Tensor:
        out_len = self.new_out_len(src.n) if out_len is None else out_len
        return self._call(self.lib.k4lz4_pickle_batch_device, src, dst, out_len, int(level), flags)

    def unpickle(self, src: DeviceBatch, dst: DeviceBatch, out_len: Optional[torch.Tensor] = None) -> torch.Tensor:
        out_len = self.new_out_len(src.n) if out_len is None else out_len
        return self._call(self.lib.k4lz4_unpickle_batch_device, src, dst, out_len, 0)

    def unpickle_sizes(self, src: DeviceBatch) -> torch.Tensor:
        out = self.new_out_len(src.n)
        rc = self.lib.k4lz4_unpickle_sizes_device(self.ctx.handle, _dp(src.data), _dp(src.off), _dp(src.length),
                                                  _dp(out), src.n, C.c_void_p(self._stream()))
        self.ctx.check(rc)
        return out

    def xxh32(self, data: torch.Tensor, off: torch.Tensor, length: torch.Tensor, seed: int = 0) -> torch.Tensor:
        """XXH32 of n HBM-resident buffers (off, length: int64/uint64 tensors) -> uint32 digests as an int64 tensor's low half
        (torch has no uint32 arithmetic; the tensor is int32 storage, view it as uint32 on the host)"""
        n = off.numel()
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        rc = self.lib.k4lz4_xxh32_batch_device(self.ctx.handle, _dp(data), _dp(off), _dp(length), _dp(out), n, seed,
                                               C.c_void_p(self._stream()))
        self.ctx.check(rc)
        return out

    def decode_chain(self, src: torch.Tensor, blk_off: torch.Tensor, blk_len: torch.Tensor, first: torch.Tensor, nblk: torch.Tensor,
                     block_size: torch.Tensor, chained: torch.Tensor, dst: torch.Tensor, dst_off: torch.Tensor,
                     dst_cap: torch.Tensor) -> torch.Tensor:
        """block streams decoded in order, one stream per wavefront (k4lz4_decode_chain_batch_device)"""
        n = first.numel()
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        rc = self.lib.k4lz4_decode_chain_batch_device(self.ctx.handle, _dp(src), _dp(blk_off), _dp(blk_len), _dp(first), _dp(nblk),
                                                      _dp(block_size), _dp(chained), _dp(dst), _dp(dst_off), _dp(dst_cap), _dp(out), n,
                                                      C.c_void_p(self._stream()))
        self.ctx.check(rc)
        return out

    def profile(self, decode: bool, src: DeviceBatch, dst: DeviceBatch, out_len: Optional[torch.Tensor] = None):
        """instrumented twin kernels: returns (out_len, counters[n, 16] int64 tensor); decode == 2: the two-waves-per-block
        decoder, counters[n, 32] (parsing wave, copying wave); decode == 4 / 5: the ordinary encode / decode kernels, which
        then only stamp every block's start, end and placement (counters[:, 8:12])"""
        out_len = self.new_out_len(src.n) if out_len is None else out_len
        counters = torch.zeros((src.n, 32 if int(decode) == 2 else 16), dtype=torch.int64, device=self.device)
        rc = self.lib.k4lz4_profile_batch_device(self.ctx.handle, int(decode), _dp(src.data), _dp(src.off),
                                                 _dp(src.length), _dp(dst.data), _dp(dst.off), _dp(dst.length),
                                                 _dp(out_len), src.n, _dp(counters), C.c_void_p(self._stream()))
        self.ctx.check(rc)
        return out_len, counters


class DevicePickleBackend:
    """per-rank work of sharding.sharded_pickle_roundtrip on one GPU: HBM-resident Pickle + Unpickle of a share of messages"""

    def __init__(self, device: int):
        self.dc = DeviceCodec(device)

    def time_alone(self, message: np.ndarray) -> float:
        """Pickle + Unpickle seconds of ONE message with the GPU to itself (the critical path of a ragged batch)"""
        import time
        dc = self.dc
        lens = np.array([message.size], np.int32)
        src = DeviceBatch.from_host(message, np.zeros(1, np.uint64), lens, dc.device)
        env = DeviceBatch.empty_slots(lens.astype(np.int64) + 5, dc.device)
        back = DeviceBatch.empty_slots(lens, dc.device)
        plen, ulen = dc.new_out_len(1), dc.new_out_len(1)
        best = float("inf")
        for _ in range(2):
            torch.cuda.synchronize(dc.device)
            t = time.perf_counter()
            dc.pickle(src, env, plen)
            dc.unpickle(DeviceBatch(env.data, env.off, plen), back, ulen)
            torch.cuda.synchronize(dc.device)
            best = min(best, time.perf_counter() - t)
        return best

    def pickle_unpickle(self, data: np.ndarray, off: np.ndarray, lens: np.ndarray):
        import time
        dc = self.dc
        n = int(lens.size)
        if n == 0:
            return torch.zeros(0, dtype=torch.int32, device=dc.device), 0.0, 0.0, True
        src = DeviceBatch.from_host(data, off, lens, dc.device)
        env = DeviceBatch.empty_slots(lens.astype(np.int64) + 5, dc.device)
        plen = dc.new_out_len(n)
        back = DeviceBatch.empty_slots(lens, dc.device)
        ulen = dc.new_out_len(n)
        dc.pickle(src, env, plen)                      # warm-up (scratch allocation)
        torch.cuda.synchronize(dc.device)
        t = time.perf_counter(); dc.pickle(src, env, plen); torch.cuda.synchronize(dc.device); t_p = time.perf_counter() - t
        psrc = DeviceBatch(env.data, env.off, plen)
        dc.unpickle(psrc, back, ulen)
        torch.cuda.synchronize(dc.device)
        t = time.perf_counter(); dc.unpickle(psrc, back, ulen); torch.cuda.synchronize(dc.device); t_u = time.perf_counter() - t
        ok = bool((ulen == torch.from_numpy(lens).to(dc.device)).all().item())
        if ok:                                         # every byte back, compared on the device
            boff = back.off.cpu().numpy()
            want = torch.from_numpy(np.ascontiguousarray(data)).to(dc.device)
            pos = 0
            if all(int(boff[i]) == int(off[i]) for i in range(0, n, max(1, n // 64))) and int(boff[-1]) == int(off[-1]):
                ok = bool(torch.equal(back.data[:want.numel()], want))
            else:                                      # slots are 16-byte aligned: compare message by message
                for i in range(n):
                    ln = int(lens[i])
                    if not torch.equal(back.data[int(boff[i]):int(boff[i]) + ln], want[int(off[i]):int(off[i]) + ln]):
                        ok = False
                        break
        return plen, t_p, t_u, ok


class ChainDecoderDevice:
    """Many open ILZ4Decoders over device tensors (k4lz4_chain_decode_batch_device / k4lz4_chain_drain_batch_device /
    k4lz4_chain_decoder_query_device): settings is one (chaining, blockSize, extraBlocks) per decoder, as
    LZ4Decoder.Create takes them.  Every array of a call is a device tensor, every call is enqueued on the current torch stream and
    returns; nothing is read back."""

    def __init__(self, settings, dc: Optional[DeviceCodec] = None):
        from .encoders import chain_decoder_record, ChainDecoderRecord
        self.dc = dc or DeviceCodec()
        self.n = len(settings)
        recs = (ChainDecoderRecord * max(self.n, 1))(*[chain_decoder_record(c, b, e, self.dc.lib) for c, b, e in settings])
        self.block_size = [int(r.blockSize) for r in recs[:self.n]]
        self.store_bytes = np.array([r.storeBytes for r in recs[:self.n]], np.int64)
        off = np.concatenate(([0], np.cumsum(self.store_bytes[:-1]))).astype(np.int64) if self.n else np.zeros(0, np.int64)
        dev = self.dc.device
        self.store = torch.empty(int(self.store_bytes.sum()) + 256, dtype=torch.uint8, device=dev)
        self.store_off = torch.from_numpy(off + (-self.store.data_ptr()) % 256).to(dev)
        self.records = torch.from_numpy(np.frombuffer(bytes(recs), np.uint8)[:self.n * C.sizeof(ChainDecoderRecord)].copy()).to(dev)
        self.reset()

    def reset(self, out_len: Optional[torch.Tensor] = None) -> torch.Tensor:
        """every store becomes a fresh decoder"""
        out_len = torch.empty(self.n, dtype=torch.int64, device=self.dc.device) if out_len is None else out_len
        self.dc.ctx.check(self.dc.lib.k4lz4_chain_decode_batch_device(
            self.dc.ctx.handle, _dp(self.records), _dp(self.store), _dp(self.store_off), None, None, None, None, None, None, None, None, None, None,
            _dp(out_len), self.n, 1, 0, C.c_void_p(self.dc._stream())))
        return out_len

    def open(self, dict_idx: torch.Tensor, dictionaries, out_len: Optional[torch.Tensor] = None) -> torch.Tensor:
        """k4lz4_chain_decoder_open_dictset_device: every store becomes a fresh decoder, and decoder s with dict_idx[s] = e >= 0 (an
        int32 device tensor; -1: none) one after Inject(the bytes entry e of `dictionaries`, a DictionarySet, keeps).  out_len[s]: the
        bytes injected or a code; an index outside the set leaves its store untouched and reports CDEC_DICT_INDEX"""
        out_len = torch.empty(self.n, dtype=torch.int64, device=self.dc.device) if out_len is None else out_len
        self.dc.ctx.check(self.dc.lib.k4lz4_chain_decoder_open_dictset_device(
            self.dc.ctx.handle, _dp(self.records), _dp(self.store), _dp(self.store_off), _dp(dict_idx), dictionaries.handle, _dp(out_len), self.n,
            C.c_void_p(self.dc._stream())))
        return out_len

    def run(self, src, rec_off, rec_len, rec_block_size, first_rec, n_rec, rec_out, out_len, dst=None, dst_off=None, dst_cap=None):
        """one run per decoder: decoder s owns records first_rec[s] .. + n_rec[s] of the table (rec_off uint64, rec_len uint32 with
        bit 31 = Inject, rec_block_size int32 or None).  With dst / dst_off / dst_cap (uint64) the records' bytes are drained.
        rec_out (int32 per record) and out_len (int64 per decoder) are written on the device."""
        drain = dst is not None
        self.dc.ctx.check(self.dc.lib.k4lz4_chain_decode_batch_device(
            self.dc.ctx.handle, None, _dp(self.store), _dp(self.store_off), _dp(src), _dp(rec_off), _dp(rec_len), _dp(rec_block_size),
            _dp(first_rec), _dp(n_rec), _dp(dst), _dp(dst_off), _dp(dst_cap), _dp(rec_out), _dp(out_len), self.n, 0, 1 if drain else 0,
            C.c_void_p(self.dc._stream())))
        return out_len

    def drain(self, offset, length, dst, dst_off, out_len):
        """Drain(target, offset, length) per decoder (offset, length int64; offset relative to BytesReady)"""
        self.dc.ctx.check(self.dc.lib.k4lz4_chain_drain_batch_device(
            self.dc.ctx.handle, _dp(self.store), _dp(self.store_off), _dp(offset), _dp(length), _dp(dst), _dp(dst_off), _dp(out_len), self.n,
            C.c_void_p(self.dc._stream())))
        return out_len

    def query(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(n, 8) int64 on the device: BytesReady, BlockSize, records applied, bytes decoded, the last code, ..."""
        out = torch.empty((self.n, 8), dtype=torch.int64, device=self.dc.device) if out is None else out
        self.dc.ctx.check(self.dc.lib.k4lz4_chain_decoder_query_device(self.dc.ctx.handle, _dp(self.store), _dp(self.store_off), self.n, _dp(out),
                                                                       C.c_void_p(self.dc._stream())))
        return out


class ChainEncoderDevice:
    """Many open ILZ4Encoders over device tensors (k4lz4_chain_encode_batch_device): settings is one (chaining, level,
    blockSize, extraBlocks) per encoder, as LZ4Encoder.Create takes them.  The sources, the target and the result arrays of a call
    are device tensors, the plan arrays (record offsets, lengths and flags, the streams' first records and counts, the target's
    offsets and capacities) host arrays; the counters live in the host records.  Every call is enqueued on the current torch stream
    and returns; nothing is read back."""

    def __init__(self, settings, dc: Optional[DeviceCodec] = None):
        from .encoders import chain_encoder_record, ChainEncoderRecord
        self.dc = dc or DeviceCodec()
        self.n = len(settings)
        self.records = (ChainEncoderRecord * max(self.n, 1))(*[chain_encoder_record(c, int(l), b, e, self.dc.lib) for c, l, b, e in settings])
        self.store_bytes = np.array([r.storeBytes for r in self.records[:self.n]], np.int64)
        off = np.concatenate(([0], np.cumsum(self.store_bytes[:-1]))).astype(np.int64) if self.n else np.zeros(0, np.int64)
        self.store = torch.empty(int(self.store_bytes.sum()) + 256, dtype=torch.uint8, device=self.dc.device)
        self._base = (self.store.data_ptr() + 255) // 256 * 256
        self.store_off = np.ascontiguousarray(off, np.uint64)

    def bytes_ready(self, i: int) -> int:
        return int(self.records[i].pointer - self.records[i].index)

    def bound(self, i: int, rec_len, rec_flags) -> int:
        rec_len, rec_flags = np.ascontiguousarray(rec_len, np.uint32), np.ascontiguousarray(rec_flags, np.uint32)
        return int(self.dc.lib.k4lz4_chain_encode_bound(C.byref(self.records[i]), rec_len.ctypes.data, rec_flags.ctypes.data, rec_len.size))

    def reset(self) -> None:
        """every encoder becomes a fresh one"""
        self.dc.ctx.check(self.dc.lib.k4lz4_chain_encode_batch_device(
            self.dc.ctx.handle, self.records, C.c_void_p(self._base), self.store_off.ctypes.data, None, None, None, None, 0, None, None, None, None,
            None, None, None, None, self.n, 1, 0, C.c_void_p(self.dc._stream())))

    def open(self, dict_idx, dictionaries) -> None:
        """k4lz4_chain_encoder_open_dictset_device: every encoder becomes a fresh one, and encoder s with dict_idx[s] = e >= 0 (a host
        array; -1: none) starts with the bytes entry e of `dictionaries` (a DictionarySet) keeps as its prefix"""
        idx = np.ascontiguousarray(dict_idx, np.int32)
        if idx.size != self.n:
            raise ValueError("dict_idx must have one entry per encoder")
        self.dc.ctx.check(self.dc.lib.k4lz4_chain_encoder_open_dictset_device(
            self.dc.ctx.handle, self.records, C.c_void_p(self._base), self.store_off.ctypes.data, idx.ctypes.data, dictionaries.handle, self.n,
            C.c_void_p(self.dc._stream())))

    def run(self, src, rec_off, rec_len, rec_flags, first_rec, n_rec, dst, dst_off, dst_cap, rec_loaded, rec_out, out_len, flags: int = 0):
        """one run per encoder: encoder s owns records first_rec[s] .. + n_rec[s] of the table (rec_off uint64, rec_len and rec_flags
        uint32, first_rec uint64, n_rec uint32, dst_off and dst_cap uint64: host arrays).  src, dst (uint8), rec_loaded, rec_out (int32 per
        record) and out_len (int64 per encoder) are device tensors."""
        h = [np.ascontiguousarray(a, t) for a, t in ((rec_off, np.uint64), (rec_len, np.uint32), (rec_flags, np.uint32), (first_rec, np.uint64),
                                                     (n_rec, np.uint32), (dst_off, np.uint64), (dst_cap, np.uint64))]
        self.dc.ctx.check(self.dc.lib.k4lz4_chain_encode_batch_device(
            self.dc.ctx.handle, self.records, C.c_void_p(self._base), self.store_off.ctypes.data, _dp(src), h[0].ctypes.data, h[1].ctypes.data,
            h[2].ctypes.data, int(h[1].size), h[3].ctypes.data, h[4].ctypes.data, _dp(dst), h[5].ctypes.data, h[6].ctypes.data, _dp(rec_loaded),
            _dp(rec_out), _dp(out_len), self.n, 0, flags, C.c_void_p(self.dc._stream())))
        return out_len
