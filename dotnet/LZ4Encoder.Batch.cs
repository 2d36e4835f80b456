// K4os.Compression.LZ4/Encoders/LZ4Encoder.Batch.cs -- many open ILZ4Encoders (LZ4Encoder.Create(chaining, level, blockSize,
// extraBlocks): LZ4BlockEncoder, LZ4FastChainEncoder or LZ4HighChainEncoder) advanced together, a run of TopupAndEncode /
// FlushAndEncode records each per call, through k4lz4_chain_encode_batch (include/k4lz4.h, DESIGN.md 4.19).  Per encoder a call gives
// what the reference's object gives for the same sequence of calls: per record what Topup took and `encoded` before the sign is
// dropped, and the blocks' bytes behind each other.  The rings (and the fast chains' states) live in device stores allocated here with
// hipMalloc; the counters are the host records.  Compile-unverified.
using System;
using System.Runtime.InteropServices;

namespace K4os.Compression.LZ4.Encoders
{
	internal static unsafe class ChainEncoderNative
	{
		private const string Lib = "k4lz4";

		[StructLayout(LayoutKind.Sequential)]
		public struct Settings { public int chaining, level, blockSize, extraBlocks; }

		[StructLayout(LayoutKind.Sequential)]
		public struct Record
		{
			public int kind, level, blockSize, extraBlocks, ringBytes, index, pointer;
			public uint currentOffset, dictSize;
			public int reserved;
			public long taken, blocks, storeBytes;
		}

		public const int RUN = 0, RESET = 1, TARGET = -1;
		public const uint FORCE = 1, ALLOW_COPY = 2;

		[DllImport(Lib)] public static extern int k4lz4_chain_encoder_init(Record* e, Settings* settings);
		[DllImport(Lib)] public static extern long k4lz4_chain_encoder_store_bytes(Record* e);
		[DllImport(Lib)] public static extern long k4lz4_chain_encode_bound(Record* e, uint* recLen, uint* recFlags, long nRec);
		[DllImport(Lib)] public static extern int k4lz4_chain_encode_batch(IntPtr ctx, Record* enc, byte* store, ulong* storeOff, byte* src,
			ulong* recOff, uint* recLen, uint* recFlags, long nRecords, ulong* firstRec, uint* nRec, byte* dst, ulong* dstOff, ulong* dstCap,
			int* recLoaded, int* recOut, long* outLen, long n, int op, int flags);
		[DllImport(Lib)] public static extern int k4lz4_chain_encode_batch_device(IntPtr ctx, Record* enc, byte* store, ulong* storeOff, byte* src,
			ulong* recOff, uint* recLen, uint* recFlags, long nRecords, ulong* firstRec, uint* nRec, byte* dst, ulong* dstOff, ulong* dstCap,
			int* recLoaded, int* recOut, long* outLen, long n, int op, int flags, IntPtr stream);

		[DllImport("amdhip64")] public static extern int hipMalloc(byte** p, UIntPtr bytes);
		[DllImport("amdhip64")] public static extern int hipFree(byte* p);
	}

	/// <summary>One record of a run: TopupAndEncode(source, forceEncode, allowCopy); no bytes with forceEncode is FlushAndEncode.</summary>
	public readonly struct ChainEncoderRecord
	{
		public readonly ArraySegment<byte> Source;
		public readonly bool ForceEncode, AllowCopy;

		public ChainEncoderRecord(ArraySegment<byte> source, bool forceEncode = false, bool allowCopy = true)
		{
			Source = source; ForceEncode = forceEncode; AllowCopy = allowCopy;
		}
	}

	/// <summary>What a record did: Loaded is what Topup took, Encoded the reference's value before the sign is dropped.</summary>
	public readonly struct ChainEncoderResult
	{
		public readonly int Loaded, Encoded;
		public ChainEncoderResult(int loaded, int encoded) { Loaded = loaded; Encoded = encoded; }
		public EncoderAction Action =>
			Encoded > 0 ? EncoderAction.Encoded : Encoded < 0 ? EncoderAction.Copied : Loaded > 0 ? EncoderAction.Loaded : EncoderAction.None;
	}

	/// <summary>Many open encoders; every call advances all of them.</summary>
	public sealed unsafe partial class LZ4EncoderBatch: IDisposable
	{
		private readonly IntPtr _ctx;
		private readonly ChainEncoderNative.Record[] _records;
		private readonly ulong[] _storeOff;
		private byte* _store;

		/// <param name="ctx">a k4lz4 context (NativeContext.Handle)</param>
		/// <param name="settings">per encoder what LZ4Encoder.Create takes</param>
		public LZ4EncoderBatch(IntPtr ctx, (bool chaining, LZ4Level level, int blockSize, int extraBlocks)[] settings)
		{
			_ctx = ctx;
			_records = new ChainEncoderNative.Record[settings.Length];
			_storeOff = new ulong[settings.Length];
			ulong total = 0;
			for (var i = 0; i < settings.Length; i++)
			{
				var s = new ChainEncoderNative.Settings {
					chaining = settings[i].chaining ? 1 : 0, level = (int) settings[i].level, blockSize = settings[i].blockSize,
					extraBlocks = settings[i].extraBlocks };
				fixed (ChainEncoderNative.Record* r = &_records[i])
					if (ChainEncoderNative.k4lz4_chain_encoder_init(r, &s) != 0)
						throw new ArgumentException("block size above the input size limit");
				_storeOff[i] = total;
				total += (ulong) _records[i].storeBytes;
			}
			byte* p;
			if (ChainEncoderNative.hipMalloc(&p, (UIntPtr) Math.Max(total, 256UL)) != 0) throw new OutOfMemoryException();
			_store = p;                         // hipMalloc's allocations are 256-byte aligned, and so is every storeBytes
		}

		public int Count => _records.Length;
		public int BlockSize(int i) => _records[i].blockSize;
		public int BytesReady(int i) => _records[i].pointer - _records[i].index;

		/// <summary>Every encoder becomes a fresh one.</summary>
		public void Reset()
		{
			fixed (ChainEncoderNative.Record* r = _records)
			fixed (ulong* so = _storeOff)
				Check(ChainEncoderNative.k4lz4_chain_encode_batch(_ctx, r, _store, so, null, null, null, null, 0, null, null, null, null, null,
					null, null, null, _records.Length, ChainEncoderNative.RESET, 0));
		}

		/// <summary>The most the run can emit for encoder i.</summary>
		public long Bound(int i, ChainEncoderRecord[] run)
		{
			var len = new uint[Math.Max(run.Length, 1)];
			var flg = new uint[Math.Max(run.Length, 1)];
			for (var k = 0; k < run.Length; k++) { len[k] = (uint) run[k].Source.Count; flg[k] = Flags(run[k]); }
			fixed (ChainEncoderNative.Record* r = &_records[i])
			fixed (uint* l = len, f = flg)
				return ChainEncoderNative.k4lz4_chain_encode_bound(r, l, f, run.Length);
		}

		/// <summary>records[s]: the run of encoder s (empty: it sits the call out); targets[s] takes its blocks behind each other.
		/// results[s][r]: what record r did; the return value per encoder is the bytes written, or K4LZ4_CENC_TARGET (-1).</summary>
		public long[] Run(ChainEncoderRecord[][] records, byte[][] targets, out ChainEncoderResult[][] results)
		{
			var n = _records.Length;
			long nRecords = 0, srcBytes = 0, dstBytes = 0;
			foreach (var run in records) { nRecords += run.Length; foreach (var rec in run) srcBytes += rec.Source.Count; }
			foreach (var t in targets) dstBytes += t?.Length ?? 0;
			var src = new byte[Math.Max(srcBytes, 1)];
			var dst = new byte[Math.Max(dstBytes, 1)];
			var recOff = new ulong[Math.Max(nRecords, 1)];
			var recLen = new uint[Math.Max(nRecords, 1)];
			var recFlags = new uint[Math.Max(nRecords, 1)];
			var loaded = new int[Math.Max(nRecords, 1)];
			var encoded = new int[Math.Max(nRecords, 1)];
			var first = new ulong[n];
			var count = new uint[n];
			var dstOff = new ulong[n];
			var dstCap = new ulong[n];
			var outLen = new long[n];
			long k = 0, at = 0, to = 0;
			for (var s = 0; s < n; s++)
			{
				first[s] = (ulong) k; count[s] = (uint) records[s].Length;
				foreach (var rec in records[s])
				{
					recOff[k] = (ulong) at; recLen[k] = (uint) rec.Source.Count; recFlags[k] = Flags(rec);
					if (rec.Source.Count > 0) Buffer.BlockCopy(rec.Source.Array, rec.Source.Offset, src, (int) at, rec.Source.Count);
					at += rec.Source.Count; k++;
				}
				dstOff[s] = (ulong) to; dstCap[s] = (ulong) (targets[s]?.Length ?? 0); to += targets[s]?.Length ?? 0;
			}
			fixed (ChainEncoderNative.Record* r = _records)
			fixed (ulong* so = _storeOff, ro = recOff, fr = first, dof = dstOff, dc = dstCap)
			fixed (uint* rl = recLen, rf = recFlags, nr = count)
			fixed (byte* sp = src, dp = dst)
			fixed (int* lo = loaded, en = encoded)
			fixed (long* ol = outLen)
				Check(ChainEncoderNative.k4lz4_chain_encode_batch(_ctx, r, _store, so, sp, ro, rl, rf, nRecords, fr, nr, dp, dof, dc, lo, en, ol, n,
					ChainEncoderNative.RUN, 0));
			results = new ChainEncoderResult[n][];
			for (var s = 0; s < n; s++)
			{
				results[s] = new ChainEncoderResult[records[s].Length];
				for (var j = 0; j < records[s].Length; j++)
					results[s][j] = new ChainEncoderResult(loaded[(long) first[s] + j], encoded[(long) first[s] + j]);
				if (outLen[s] > 0) Buffer.BlockCopy(dst, (int) dstOff[s], targets[s], 0, (int) outLen[s]);
			}
			return outLen;
		}

		private static uint Flags(ChainEncoderRecord rec) =>
			(rec.ForceEncode ? ChainEncoderNative.FORCE : 0u) | (rec.AllowCopy ? ChainEncoderNative.ALLOW_COPY : 0u);

		private static void Check(int rc)
		{
			if (rc != 0) throw new InvalidOperationException($"k4lz4_chain_encode_batch failed: {rc}");
		}

		public void Dispose()
		{
			if (_store != null) { ChainEncoderNative.hipFree(_store); _store = null; }
		}
	}
}
