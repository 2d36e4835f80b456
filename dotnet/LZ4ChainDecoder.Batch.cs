// K4os.Compression.LZ4/Encoders/LZ4ChainDecoder.Batch.cs -- many open ILZ4Decoders (LZ4Decoder.Create(chaining, blockSize,
// extraBlocks): LZ4ChainDecoder or LZ4BlockDecoder) advanced together, a run of Decode / Inject records each per call, through
// k4lz4_chain_decode_batch, k4lz4_chain_drain_batch and k4lz4_chain_decoder_query (include/k4lz4.h, DESIGN.md 4.18).  Per decoder a
// call gives what the reference's object gives for the same sequence of calls: Decode's / Inject's return values, DecodeAndDrain's
// bytes, BytesReady, and Drain / Peek over the reference's own ring geometry.  The decoders' state and ring buffers live in device
// stores allocated here with hipMalloc; the host keeps the settings.  Compile-unverified.
using System;
using System.Runtime.InteropServices;

namespace K4os.Compression.LZ4.Encoders
{
	internal static unsafe class ChainDecoderNative
	{
		private const string Lib = "k4lz4";

		[StructLayout(LayoutKind.Sequential)]
		public struct Settings { public int blockSize, extraBlocks, chaining; }

		[StructLayout(LayoutKind.Sequential)]
		public struct Record { public int blockSize, extraBlocks, chaining, reserved; public long storeBytes; }

		public const int RUN = 0, RESET = 1, DRAIN = 1, QUERY_WORDS = 8;
		public const uint INJECT = 0x80000000u;
		public const int DECODE_THREW = -1, INJECT_THREW = -2, BLOCK_SIZE = -3, TARGET = -4, NOT_RUN = -5, RANGE = -6, NO_DECODER = -7;

		[DllImport(Lib)] public static extern int k4lz4_chain_decoder_init(Record* d, Settings* settings);
		[DllImport(Lib)] public static extern long k4lz4_chain_decoder_store_bytes(Record* d);
		[DllImport(Lib)] public static extern int k4lz4_chain_decode_batch(IntPtr ctx, Record* dec, byte* store, ulong* storeOff, byte* src,
			ulong* recOff, uint* recLen, int* recBlockSize, long nRecords, ulong* firstRec, uint* nRec, byte* dst, ulong* dstOff, ulong* dstCap,
			int* recOut, long* outLen, long n, int op, int flags);
		[DllImport(Lib)] public static extern int k4lz4_chain_decode_batch_device(IntPtr ctx, Record* dec, byte* store, ulong* storeOff, byte* src,
			ulong* recOff, uint* recLen, int* recBlockSize, ulong* firstRec, uint* nRec, byte* dst, ulong* dstOff, ulong* dstCap, int* recOut,
			long* outLen, long n, int op, int flags, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_chain_drain_batch(IntPtr ctx, byte* store, ulong* storeOff, long* offset, long* length,
			byte* dst, ulong* dstOff, long* outLen, long n);
		[DllImport(Lib)] public static extern int k4lz4_chain_drain_batch_device(IntPtr ctx, byte* store, ulong* storeOff, long* offset, long* length,
			byte* dst, ulong* dstOff, long* outLen, long n, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_chain_decoder_query(IntPtr ctx, byte* store, ulong* storeOff, long n, long* @out);
		[DllImport(Lib)] public static extern int k4lz4_chain_decoder_query_device(IntPtr ctx, byte* store, ulong* storeOff, long n, long* @out,
			IntPtr stream);

		[DllImport("amdhip64")] public static extern int hipMalloc(byte** p, UIntPtr bytes);
		[DllImport("amdhip64")] public static extern int hipFree(byte* p);
	}

	/// <summary>One record of a run: Decode(source, length, blockSize), or Inject(source, length).</summary>
	public readonly struct ChainDecoderRecord
	{
		public readonly ArraySegment<byte> Source;
		public readonly bool Inject;
		public readonly int BlockSize;

		public ChainDecoderRecord(ArraySegment<byte> source, bool inject = false, int blockSize = 0)
		{
			Source = source; Inject = inject; BlockSize = blockSize;
		}
	}

	/// <summary>Many open decoders; every call advances all of them.</summary>
	public sealed unsafe partial class LZ4ChainDecoderBatch: IDisposable
	{
		private readonly IntPtr _ctx;
		private readonly ChainDecoderNative.Record[] _records;
		private readonly ulong[] _storeOff;
		private byte* _store;

		/// <param name="ctx">a k4lz4 context (NativeContext.Handle)</param>
		/// <param name="settings">per decoder what LZ4Decoder.Create takes: (chaining, blockSize, extraBlocks)</param>
		public LZ4ChainDecoderBatch(IntPtr ctx, (bool chaining, int blockSize, int extraBlocks)[] settings)
		{
			_ctx = ctx;
			_records = new ChainDecoderNative.Record[settings.Length];
			_storeOff = new ulong[settings.Length];
			ulong total = 0;
			for (var i = 0; i < settings.Length; i++)
			{
				var s = new ChainDecoderNative.Settings {
					blockSize = settings[i].blockSize, extraBlocks = settings[i].extraBlocks, chaining = settings[i].chaining ? 1 : 0 };
				fixed (ChainDecoderNative.Record* r = &_records[i])
					if (ChainDecoderNative.k4lz4_chain_decoder_init(r, &s) != 0)
						throw new ArgumentException("the decoder's ring buffer is too large");
				_storeOff[i] = total;
				total += (ulong) _records[i].storeBytes;
			}
			byte* p;
			if (ChainDecoderNative.hipMalloc(&p, (UIntPtr) Math.Max(total, 256)) != 0) throw new OutOfMemoryException();
			_store = p;
			Reset();
		}

		public int Count => _records.Length;

		/// <summary>Every store becomes a fresh decoder.</summary>
		public void Reset()
		{
			var outLen = new long[Count];
			fixed (ChainDecoderNative.Record* r = _records)
			fixed (ulong* so = _storeOff)
			fixed (long* ol = outLen)
				Check(ChainDecoderNative.k4lz4_chain_decode_batch(_ctx, r, _store, so, null, null, null, null, 0, null, null, null, null, null, null,
					ol, Count, ChainDecoderNative.RESET, 0));
		}

		/// <summary>Applies records[s] to decoder s in order (an empty run leaves it untouched).  With targets, every record's bytes are
		/// appended to targets[s] as DecodeAndDrain does.  results[s][k]: the bytes record k produced or a code
		/// (ChainDecoderNative.*); returns per decoder the run's total or the failing record's code.</summary>
		public long[] Run(ChainDecoderRecord[][] records, out int[][] results, byte[][] targets = null)
		{
			var n = Count;
			long nr = 0, bytes = 0, room = 0;
			foreach (var run in records) { nr += run.Length; foreach (var rec in run) bytes += rec.Source.Count; }
			var src = new byte[Math.Max(bytes, 1)];
			var recOff = new ulong[Math.Max(nr, 1)]; var recLen = new uint[Math.Max(nr, 1)]; var recBs = new int[Math.Max(nr, 1)];
			var first = new ulong[n]; var nRec = new uint[n]; var dstOff = new ulong[n]; var dstCap = new ulong[n];
			long at = 0, k = 0;
			for (var s = 0; s < n; s++)
			{
				first[s] = (ulong) k; nRec[s] = (uint) records[s].Length;
				foreach (var rec in records[s])
				{
					Buffer.BlockCopy(rec.Source.Array ?? Array.Empty<byte>(), rec.Source.Offset, src, (int) at, rec.Source.Count);
					recOff[k] = (ulong) at; recLen[k] = (uint) rec.Source.Count | (rec.Inject ? ChainDecoderNative.INJECT : 0u); recBs[k] = rec.BlockSize;
					at += rec.Source.Count; k++;
				}
				if (targets != null) { dstOff[s] = (ulong) room; dstCap[s] = (ulong) targets[s].Length; room += targets[s].Length; }
			}
			var dst = new byte[Math.Max(room, 1)];
			var recOut = new int[Math.Max(nr, 1)]; var outLen = new long[n];
			fixed (ulong* so = _storeOff, ro = recOff, fr = first, dof = dstOff, dc = dstCap)
			fixed (uint* rl = recLen, nrp = nRec)
			fixed (int* rb = recBs, rout = recOut)
			fixed (byte* sp = src, dp = dst)
			fixed (long* ol = outLen)
				Check(ChainDecoderNative.k4lz4_chain_decode_batch(_ctx, null, _store, so, sp, ro, rl, rb, nr, fr, nrp, targets != null ? dp : null,
					targets != null ? dof : null, targets != null ? dc : null, rout, ol, n, ChainDecoderNative.RUN,
					targets != null ? ChainDecoderNative.DRAIN : 0));
			results = new int[n][];
			for (var s = 0; s < n; s++)
			{
				results[s] = new int[nRec[s]];
				Array.Copy(recOut, (long) first[s], results[s], 0, nRec[s]);
				long given = 0;
				foreach (var got in results[s]) { if (got < 0) break; given += got; }
				if (targets != null) Buffer.BlockCopy(dst, (int) dstOff[s], targets[s], 0, (int) given);
			}
			return outLen;
		}

		/// <summary>Drain(target, offset, length) per decoder; offset is relative to BytesReady (negative).  Throws what the reference
		/// throws for the lowest-index decoder whose range check fails.</summary>
		public void Drain(byte[][] targets, long[] offsets, long[] lengths)
		{
			var n = Count;
			var dstOff = new ulong[n]; var outLen = new long[n];
			long room = 0;
			for (var s = 0; s < n; s++) { dstOff[s] = (ulong) room; room += Math.Max(lengths[s], 0); }
			var dst = new byte[Math.Max(room, 1)];
			fixed (ulong* so = _storeOff, dof = dstOff)
			fixed (long* of = offsets, ln = lengths, ol = outLen)
			fixed (byte* dp = dst)
				Check(ChainDecoderNative.k4lz4_chain_drain_batch(_ctx, _store, so, of, ln, dp, dof, ol, n));
			for (var s = 0; s < n; s++)
			{
				if (outLen[s] < 0) throw new InvalidOperationException();
				Buffer.BlockCopy(dst, (int) dstOff[s], targets[s], 0, (int) outLen[s]);
			}
		}

		/// <summary>Per decoder QUERY_WORDS words: BytesReady, BlockSize, records applied, bytes decoded, the last code, ...</summary>
		public long[] Query()
		{
			var q = new long[Count * ChainDecoderNative.QUERY_WORDS];
			fixed (ulong* so = _storeOff)
			fixed (long* qp = q)
				Check(ChainDecoderNative.k4lz4_chain_decoder_query(_ctx, _store, so, Count, qp));
			return q;
		}

		private static void Check(int rc)
		{
			if (rc != 0) throw new InvalidOperationException($"k4lz4 call failed ({rc})");
		}

		public void Dispose()
		{
			if (_store != null) ChainDecoderNative.hipFree(_store);
			_store = null;
		}
	}
}
