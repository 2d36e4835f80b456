// Streams/Frames/LZ4FrameFedReaderBatch.cs -- many LZ4FrameReaders whose sources arrive in pieces, advanced together through
// k4lz4_frame_read_fed_batch (DESIGN.md 4.15): what LZ4DecoderStream does over a socket or a pipe.  Feed(pieces, final) appends to a
// per-stream host queue; Read(counts) presents each stream's unconsumed bytes to one ReadManyBytes(count) per stream
// (Frames/LZ4FrameReader.async.cs:150-172), drops what was consumed and returns the bytes delivered.  Need[s] > 0 then says that the
// read is starved: the field it stands at wants that many further bytes (Streams/Internal/ReaderExtensions.cs:10-28 loops at that
// point), and the same read is to be issued again, with the count reduced by what it delivered, once more has been fed.  Every
// source byte goes up once; an incomplete header or record waits in the stream's device store.
// Compile-unverified: this C# has not been compiled.
using System;
using System.Collections.Generic;
using System.Runtime.InteropServices;
using K4os.Compression.LZ4.Engine;

namespace K4os.Compression.LZ4.Streams.Frames
{
	public sealed unsafe partial class LZ4FrameFedReaderBatch: IDisposable
	{
		[DllImport("amdhip64")] private static extern int hipSetDevice(int device);
		[DllImport("amdhip64")] private static extern int hipMalloc(out IntPtr ptr, UIntPtr size);
		[DllImport("amdhip64")] private static extern int hipFree(IntPtr ptr);

		private LLNative.k4lz4_frame_reader _record;
		private readonly ulong[] _storeOff;
		private readonly List<byte>[] _queue;
		private readonly long[] _final;
		private readonly NativeContext.Lease _lease;
		private IntPtr _store;

		/// <summary>Per-stream codes of the last call: 0, or a K4LZ4_FRAME_* code for a stream that failed (it stays failed).</summary>
		public long[] LastCodes { get; private set; }
		/// <summary>Per stream after the last call: the further bytes with which the field a starved read stands at is complete; 0: not starved.</summary>
		public long[] Need { get; private set; }

		public LZ4FrameFedReaderBatch(int n, int maxBlockSize = 4 << 20): this(n, maxBlockSize, null, default) { }

		// (the form with a dictionary set is in LZ4FrameFedReaderBatch.DictSet.cs)
		private LZ4FrameFedReaderBatch(int n, int maxBlockSize, LZ4DictionarySet dictionaries, ReadOnlySpan<uint> dictionaryIds)
		{
			SetDictionaries(dictionaries, dictionaryIds);
			_lease = NativeContext.Rent();
			var settings = new LLNative.k4lz4_frame_reader_settings { maxBlockSize = maxBlockSize, flags = LLNative.FREADER_FED };
			fixed (LLNative.k4lz4_frame_reader* r = &_record)
				LLNative.ThrowIfFailed(LLNative.k4lz4_frame_reader_init(r, &settings), IntPtr.Zero);
			_storeOff = new ulong[n]; _final = new long[n]; _queue = new List<byte>[n];
			for (var i = 0; i < n; i++) { _storeOff[i] = (ulong) (i * _record.storeBytes); _queue[i] = new List<byte>(); }
			if (hipSetDevice(_lease.Device) != 0 || hipMalloc(out _store, (UIntPtr) (ulong) (n * _record.storeBytes + 64)) != 0)
				throw new OutOfMemoryException("device memory for the frame readers' stores");
			LastCodes = new long[n]; Need = new long[n];
			Call(new long[n], LLNative.FREAD_OP_RESET, false, out _);
		}

		/// <summary>pieces[s]: the next bytes of stream s's source (null: none now); final[s]: no byte follows them.</summary>
		public void Feed(byte[][] pieces, bool[] final = null)
		{
			if (pieces.Length != _queue.Length || (final != null && final.Length != _queue.Length)) throw new ArgumentException("one piece (or null) per stream");
			for (var i = 0; i < pieces.Length; i++)
			{
				if (pieces[i] != null && pieces[i].Length > 0)
				{
					if (_final[i] != 0) throw new InvalidOperationException("the stream was fed its final piece already");
					_queue[i].AddRange(pieces[i]);
				}
				if (final != null && final[i]) _final[i] = 1;
			}
		}

		private long[] Call(long[] counts, int op, bool interactive, out byte[] dst)
		{
			var n = _storeOff.Length;
			if (counts.Length != n) throw new ArgumentException("one count per stream (negative: the stream sits the call out)");
			var srcOff = new ulong[n]; var srcLen = new ulong[n]; var dstOff = new ulong[n];
			long total = 0, cap = 0;
			for (var i = 0; i < n; i++)
			{
				srcOff[i] = (ulong) total; srcLen[i] = op == LLNative.FREAD_OP_RESET ? 0UL : (ulong) _queue[i].Count; total += (long) srcLen[i];
				dstOff[i] = (ulong) cap; if (op == LLNative.FREAD_OP_READ) cap += Math.Max(counts[i], 0);
			}
			var src = new byte[Math.Max(total, 1)];
			for (var i = 0; i < n; i++) if (srcLen[i] > 0) _queue[i].CopyTo(0, src, (int) srcOff[i], (int) srcLen[i]);
			dst = new byte[Math.Max(cap, 1)];
			var outLen = new long[n]; var consumed = new long[n]; var need = new long[n];
			fixed (LLNative.k4lz4_frame_reader* r = &_record)
			fixed (byte* ps = src, pd = dst)
			fixed (ulong* pso = srcOff, psl = srcLen, pdo = dstOff, pst = _storeOff)
			fixed (long* pc = counts, pol = outLen, pf = _final, pcs = consumed, pn = need)
			fixed (uint* ids = _dictionaryIds)
				LLNative.ThrowIfFailed(_dictionaries is null
					? LLNative.k4lz4_frame_read_fed_batch(_lease.Handle, r, _store, pst, ps, pso, psl, pf, pd, pdo, pc, pol, pcs, pn, n,
						op, interactive ? LLNative.FREAD_INTERACTIVE : 0)
					: LLNative.k4lz4_frame_read_fed_dictset_batch(_lease.Handle, r, _store, pst, ps, pso, psl, pf, pd, pdo, pc, pol, pcs, pn, n,
						op, interactive ? LLNative.FREAD_INTERACTIVE : 0, _dictionaries.Handle, ids), _lease.Handle);
			GC.KeepAlive(_dictionaries);
			var codes = new long[n];
			for (var i = 0; i < n; i++)
			{
				codes[i] = counts[i] < 0 ? 0 : Math.Min(outLen[i], 0);
				if (counts[i] >= 0 && outLen[i] >= 0 && consumed[i] > 0) _queue[i].RemoveRange(0, (int) consumed[i]);
				if (outLen[i] < 0) need[i] = 0;
			}
			LastCodes = codes; Need = need;
			return outLen;
		}

		/// <summary>ReadManyBytes(counts[s]) per stream over what has been fed: the bytes delivered; null for a stream that sat the call
		/// out or failed (LastCodes says which).  Need[s] > 0: starved, read again with counts[s] - result[s].Length after feeding.</summary>
		public byte[][] Read(long[] counts, bool interactive = false)
		{
			var outLen = Call(counts, LLNative.FREAD_OP_READ, interactive, out var dst);
			var result = new byte[counts.Length][];
			long at = 0;
			for (var i = 0; i < counts.Length; i++)
			{
				if (counts[i] >= 0 && outLen[i] >= 0)
				{
					result[i] = new byte[outLen[i]];
					Buffer.BlockCopy(dst, (int) at, result[i], 0, (int) outLen[i]);
				}
				at += Math.Max(counts[i], 0);
			}
			return result;
		}

		/// <summary>OpenFrame per stream: 1 a frame is open, 0 the source is at its end or (Need[s] > 0) the header is not all there yet,
		/// or a K4LZ4_FRAME_* code.</summary>
		public long[] Open() => Call(new long[_storeOff.Length], LLNative.FREAD_OP_OPEN, false, out _);

		/// <summary>As LZ4FrameReaderBatch.Query (LLNative.FRQ_*).</summary>
		public long[] Query()
		{
			var q = new long[Math.Max(_storeOff.Length, 1) * LLNative.FRQ_WORDS];
			fixed (ulong* pst = _storeOff)
			fixed (long* pq = q)
				LLNative.ThrowIfFailed(LLNative.k4lz4_frame_reader_query(_lease.Handle, _store, pst, _storeOff.Length, pq), _lease.Handle);
			return q;
		}

		public void Dispose()
		{
			if (_store != IntPtr.Zero) { LLNative.k4lz4_synchronize(_lease.Handle, IntPtr.Zero); hipFree(_store); _store = IntPtr.Zero; }
			_lease.Dispose();
		}
	}
}
