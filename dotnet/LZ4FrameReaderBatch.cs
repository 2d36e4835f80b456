// Streams/Frames/LZ4FrameReaderBatch.cs -- many LZ4FrameReaders advanced together through k4lz4_frame_read_batch (DESIGN.md 4.14):
// Read(counts) is one ReadManyBytes(count) per stream (Frames/LZ4FrameReader.async.cs:150-172), Open one OpenFrame
// (LZ4FrameReader.cs:138-139).  Each source is held whole in host memory (the ReadOnlyMemory adapter's case); the readers' state --
// position, open frame, checksum, history, the undrained rest of a block -- lives in one device allocation owned by this object.
// Compile-unverified: this C# has not been compiled.
using System;
using System.IO;
using System.Runtime.InteropServices;
using K4os.Compression.LZ4.Engine;

namespace K4os.Compression.LZ4.Streams.Frames
{
	public sealed unsafe partial class LZ4FrameReaderBatch: IDisposable
	{
		[DllImport("amdhip64")] private static extern int hipSetDevice(int device);
		[DllImport("amdhip64")] private static extern int hipMalloc(out IntPtr ptr, UIntPtr size);
		[DllImport("amdhip64")] private static extern int hipFree(IntPtr ptr);

		private LLNative.k4lz4_frame_reader _record;
		private readonly ulong[] _storeOff, _srcOff, _srcLen;
		private readonly byte[] _src;
		private readonly NativeContext.Lease _lease;
		private IntPtr _store;

		/// <summary>Per-stream codes of the last call: 0, or a K4LZ4_FRAME_* code for a stream that failed (it stays failed).</summary>
		public long[] LastCodes { get; private set; }

		public LZ4FrameReaderBatch(byte[][] sources, int maxBlockSize = 4 << 20): this(sources, maxBlockSize, null, default) { }

		// (the form with a dictionary set is in LZ4FrameReaderBatch.DictSet.cs)
		private LZ4FrameReaderBatch(byte[][] sources, int maxBlockSize, LZ4DictionarySet dictionaries, ReadOnlySpan<uint> dictionaryIds)
		{
			SetDictionaries(dictionaries, dictionaryIds);
			var n = sources.Length;
			_lease = NativeContext.Rent();
			var settings = new LLNative.k4lz4_frame_reader_settings { maxBlockSize = maxBlockSize };
			fixed (LLNative.k4lz4_frame_reader* r = &_record)
				LLNative.ThrowIfFailed(LLNative.k4lz4_frame_reader_init(r, &settings), IntPtr.Zero);
			_storeOff = new ulong[n]; _srcOff = new ulong[n]; _srcLen = new ulong[n];
			long total = 0;
			for (var i = 0; i < n; i++)
			{
				_storeOff[i] = (ulong) (i * _record.storeBytes);
				_srcOff[i] = (ulong) total; _srcLen[i] = (ulong) sources[i].Length;
				total += (sources[i].Length + 15) / 16 * 16;
			}
			_src = new byte[Math.Max(total, 1)];
			for (var i = 0; i < n; i++) Buffer.BlockCopy(sources[i], 0, _src, (int) _srcOff[i], sources[i].Length);
			if (hipSetDevice(_lease.Device) != 0 || hipMalloc(out _store, (UIntPtr) (ulong) (n * _record.storeBytes + 64)) != 0)
				throw new OutOfMemoryException("device memory for the frame readers' stores");
			LastCodes = new long[n];
			Call(new long[n], LLNative.FREAD_OP_RESET, false, out _);
		}

		private long[] Call(long[] counts, int op, bool interactive, out byte[] dst)
		{
			var n = _storeOff.Length;
			if (counts.Length != n) throw new ArgumentException("one count per stream (negative: the stream sits the call out)");
			var dstOff = new ulong[n];
			long cap = 0;
			for (var i = 0; i < n; i++) { dstOff[i] = (ulong) cap; if (op == LLNative.FREAD_OP_READ) cap += Math.Max(counts[i], 0); }
			dst = new byte[Math.Max(cap, 1)];
			var outLen = new long[n];
			fixed (LLNative.k4lz4_frame_reader* r = &_record)
			fixed (byte* ps = _src, pd = dst)
			fixed (ulong* pso = _srcOff, psl = _srcLen, pdo = dstOff, pst = _storeOff)
			fixed (long* pc = counts, pol = outLen)
			fixed (uint* ids = _dictionaryIds)
				LLNative.ThrowIfFailed(_dictionaries is null
					? LLNative.k4lz4_frame_read_batch(_lease.Handle, r, _store, pst, ps, pso, psl, pd, pdo, pc, pol, n, op,
						interactive ? LLNative.FREAD_INTERACTIVE : 0)
					: LLNative.k4lz4_frame_read_dictset_batch(_lease.Handle, r, _store, pst, ps, pso, psl, pd, pdo, pc, pol, n, op,
						interactive ? LLNative.FREAD_INTERACTIVE : 0, _dictionaries.Handle, ids), _lease.Handle);
			GC.KeepAlive(_dictionaries);
			var codes = new long[n];
			for (var i = 0; i < n; i++) codes[i] = counts[i] < 0 ? 0 : Math.Min(outLen[i], 0);
			LastCodes = codes;
			return outLen;
		}

		/// <summary>ReadManyBytes(counts[s]) per stream: the bytes delivered (empty at the end of a frame and of the source); null for
		/// a stream that sat the call out or failed (LastCodes says which).</summary>
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

		/// <summary>OpenFrame per stream: 1 a frame is open, 0 the source is at its end, or a K4LZ4_FRAME_* code.</summary>
		public long[] Open() => Call(new long[_storeOff.Length], LLNative.FREAD_OP_OPEN, false, out _);

		/// <summary>GetBytesRead / the open frame's ContentLength (-1: none) / phase / code per stream (LLNative.FRQ_*).</summary>
		public long[] Query()
		{
			var q = new long[Math.Max(_storeOff.Length, 1) * LLNative.FRQ_WORDS];
			fixed (ulong* pst = _storeOff)
			fixed (long* pq = q)
				LLNative.ThrowIfFailed(LLNative.k4lz4_frame_reader_query(_lease.Handle, _store, pst, _storeOff.Length, pq), _lease.Handle);
			return q;
		}

		/// <summary>The exception LZ4FrameReader throws for a code.</summary>
		public static Exception ExceptionFor(long code) => code switch {
			-1 => new EndOfStreamException("Unexpected end of stream. Data might be corrupted."),
			-2 => new InvalidDataException("LZ4 frame magic number expected"),
			-3 => new InvalidDataException("LZ4 frame version is not supported"),
			-4 => new InvalidDataException("Invalid LZ4 frame header checksum"),
			-5 => new NotImplementedException("Feature 'Predefined dictionaries feature is not implemented' is not implemented"),
			-6 => new InvalidOperationException(),
			-7 => new InvalidDataException("Invalid block checksum"),
			-8 => new InvalidDataException("Invalid content checksum"),
			_ => new InvalidDataException("LZ4 frame block size is above the reader's maxBlockSize"),
		};

		public void Dispose()
		{
			if (_store != IntPtr.Zero) { LLNative.k4lz4_synchronize(_lease.Handle, IntPtr.Zero); hipFree(_store); _store = IntPtr.Zero; }
			_lease.Dispose();
		}
	}
}
