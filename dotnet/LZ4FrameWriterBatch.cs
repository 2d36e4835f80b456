// Streams/Frames/LZ4FrameWriterBatch.cs -- many LZ4FrameWriters advanced together through k4lz4_frame_write_batch (DESIGN.md 4.13):
// Write(chunks) is one WriteManyBytes per stream (Frames/LZ4FrameWriter.async.cs:29-47), Open one OpenFrame (LZ4FrameWriter.cs:217),
// Close one CloseFrame (LZ4FrameWriter.async.cs:59-90).  Each returns, per stream, the bytes the reference's writer pushes to its
// inner stream during that call; a caller that holds one output stream per writer appends them there.  The records live in host
// memory (an array of k4lz4_frame_writer), the encoders' rings in one device allocation owned by this object.
// Compile-unverified: this C# has not been compiled.
using System;
using System.Runtime.InteropServices;
using K4os.Compression.LZ4.Engine;

namespace K4os.Compression.LZ4.Streams.Frames
{
	public sealed unsafe class LZ4FrameWriterBatch: IDisposable
	{
		[DllImport("amdhip64")] private static extern int hipSetDevice(int device);
		[DllImport("amdhip64")] private static extern int hipMalloc(out IntPtr ptr, UIntPtr size);
		[DllImport("amdhip64")] private static extern int hipFree(IntPtr ptr);

		private readonly LLNative.k4lz4_frame_writer[] _records;
		private readonly ulong[] _storeOff;
		private readonly NativeContext.Lease _lease;
		private IntPtr _store;                    // device memory of the context's GPU: every stream's ring, XXH32 state, fast-chain state

		/// <summary>Per-stream codes of the last call: 0, or LLNative.FWRITE_* for a stream the call refused.</summary>
		public long[] LastCodes { get; private set; }

		public LZ4FrameWriterBatch(LZ4EncoderSettings[] settings)
		{
			var n = settings.Length;
			_lease = NativeContext.Rent();
			_records = new LLNative.k4lz4_frame_writer[n];
			_storeOff = new ulong[n];
			long total = 0;
			for (var i = 0; i < n; i++)
			{
				var s = settings[i];
				var ws = new LLNative.k4lz4_frame_writer_settings {
					contentLength = s.ContentLength.HasValue ? (long) s.ContentLength.Value : -1,
					blockSize = s.BlockSize, level = (int) s.CompressionLevel, chainBlocks = s.ChainBlocks ? 1 : 0,
					blockChecksum = s.BlockChecksum ? 1 : 0, contentChecksum = s.ContentChecksum ? 1 : 0, extraMemory = s.ExtraMemory,
				};
				fixed (LLNative.k4lz4_frame_writer* r = &_records[i])
				{
					LLNative.ThrowIfFailed(LLNative.k4lz4_frame_writer_init(r, &ws), IntPtr.Zero);
					_storeOff[i] = (ulong) total;
					total += LLNative.k4lz4_frame_writer_store_bytes(r);
				}
			}
			if (hipSetDevice(_lease.Device) != 0 || hipMalloc(out _store, (UIntPtr) (ulong) (total + 64)) != 0)
				throw new OutOfMemoryException("device memory for the frame writers' stores");
			LastCodes = new long[n];
		}

		private byte[][] Call(byte[][] chunks, int op)
		{
			var n = _records.Length;
			if (chunks.Length != n) throw new ArgumentException("one chunk (or null) per stream");
			var srcOff = new ulong[n];
			var srcLen = new long[n];
			long total = 0;
			for (var i = 0; i < n; i++) { srcOff[i] = (ulong) total; srcLen[i] = chunks[i]?.Length ?? -1; total += Math.Max(srcLen[i], 0); }
			var src = new byte[Math.Max(total, 1)];
			for (var i = 0; i < n; i++) if (chunks[i] != null) Buffer.BlockCopy(chunks[i], 0, src, (int) srcOff[i], chunks[i].Length);
			var dstOff = new ulong[n];
			var dstCap = new ulong[n];
			long cap = 0;
			fixed (LLNative.k4lz4_frame_writer* r = _records)
				for (var i = 0; i < n; i++)
				{
					dstOff[i] = (ulong) cap;
					dstCap[i] = (ulong) LLNative.k4lz4_frame_write_bound(r + i, srcLen[i], op == LLNative.FWRITE_OP_CLOSE ? 1 : 0);
					cap += (long) dstCap[i];
				}
			var dst = new byte[Math.Max(cap, 1)];
			var outLen = new long[n];
			fixed (LLNative.k4lz4_frame_writer* r = _records)
			fixed (byte* ps = src, pd = dst)
			fixed (ulong* pso = srcOff, pdo = dstOff, pdc = dstCap, pst = _storeOff)
			fixed (long* psl = srcLen, pol = outLen)
				LLNative.ThrowIfFailed(LLNative.k4lz4_frame_write_batch(_lease.Handle, r, _store, pst, ps, pso, psl, pd, pdo, pdc, pol, n, op,
					LZ4Codec.Enforce32 ? LLNative.FLAG_X32 : 0), _lease.Handle);
			var result = new byte[n][];
			var codes = new long[n];
			for (var i = 0; i < n; i++)
			{
				codes[i] = Math.Min(outLen[i], 0);
				if (srcLen[i] < 0 || outLen[i] < 0) continue;
				result[i] = new byte[outLen[i]];
				Buffer.BlockCopy(dst, (int) dstOff[i], result[i], 0, (int) outLen[i]);
			}
			LastCodes = codes;
			return result;
		}

		/// <summary>WriteManyBytes per stream; a null chunk leaves its stream untouched (null result).</summary>
		public byte[][] Write(byte[][] chunks) => Call(chunks, LLNative.FWRITE_OP_WRITE);

		/// <summary>OpenFrame per stream: the header, or nothing for a frame already open.</summary>
		public byte[][] Open() => Call(Empties(), LLNative.FWRITE_OP_OPEN);

		/// <summary>CloseFrame per stream: the last partial block, EndMark, content checksum; nothing for a frame never opened.</summary>
		public byte[][] Close() => Call(Empties(), LLNative.FWRITE_OP_CLOSE);

		private byte[][] Empties()
		{
			var e = new byte[_records.Length][];
			for (var i = 0; i < e.Length; i++) e[i] = Array.Empty<byte>();
			return e;
		}

		public void Dispose()
		{
			if (_store != IntPtr.Zero) { LLNative.k4lz4_synchronize(_lease.Handle, IntPtr.Zero); hipFree(_store); _store = IntPtr.Zero; }
			_lease.Dispose();
		}
	}
}
