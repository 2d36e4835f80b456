// LZ4LegacyBatch: batch forms of K4os.Compression.LZ4.Legacy's LZ4Wrapper (Wrap / WrapHC / Unwrap) and of LZ4Stream written whole
// and read to its end (LZ4Legacy.Encode / Decode), over the host calls of include/k4lz4.h (k4lz4_wrap_batch, k4lz4_unwrap_batch,
// k4lz4_encode_legacy_streams, k4lz4_legacy_stream_sizes + k4lz4_decode_legacy_streams; DESIGN.md 4.12).  Every item behaves as
// the reference does for it; a batch throws what the reference throws for its lowest-index failing item.  Compile-unverified.
using System;
using System.IO;
using K4os.Compression.LZ4.Engine;

namespace K4os.Compression.LZ4.Legacy
{
	public static unsafe class LZ4LegacyBatch
	{
		private static Exception Thrown(int code) => code switch {
			LLNative.LEGACY_END_OF_STREAM => new EndOfStreamException("Unexpected end of stream"),
			LLNative.LEGACY_OVERFLOW => new OverflowException(),
			LLNative.LEGACY_NOT_SUPPORTED => new NotSupportedException("Chunks with multiple passes are not supported."),
			LLNative.LEGACY_INVALID_DATA => new InvalidDataException("Compressed data corrupted"),
			LLNative.LEGACY_ARGUMENT => new ArgumentException("inputBuffer size is invalid or has been corrupted"),
			_ => new InvalidOperationException($"libk4lz4 legacy result {code}"),
		};

		private static byte[] Pack(byte[][] items, out ulong[] off, out long total)
		{
			off = new ulong[items.Length];
			total = 0;
			for (var i = 0; i < items.Length; i++) { off[i] = (ulong) total; total += items[i].Length; }
			var packed = new byte[Math.Max(total, 1)];
			for (var i = 0; i < items.Length; i++) Buffer.BlockCopy(items[i], 0, packed, (int) off[i], items[i].Length);
			return packed;
		}

		/// <summary>LZ4Wrapper.Wrap (high: WrapHC) of every source: L00_FAST or L09_HC, LZ4Codec.Enforce32 applies.</summary>
		public static byte[][] WrapBatch(byte[][] sources, bool high = false)
		{
			var n = sources.Length;
			var src = Pack(sources, out var srcOff, out _);
			var srcLen = new int[n];
			var dstCap = new int[n];
			var dstOff = new ulong[n];
			long total = 0;
			for (var i = 0; i < n; i++)
			{
				srcLen[i] = sources[i].Length;
				dstCap[i] = LLNative.k4lz4_wrap_bound(srcLen[i]);
				dstOff[i] = (ulong) total;
				total += dstCap[i];
			}
			var dst = new byte[Math.Max(total, 1)];
			var outLen = new int[n];
			using var lease = NativeContext.Rent();
			fixed (byte* s = src) fixed (ulong* so = srcOff) fixed (int* sl = srcLen) fixed (byte* d = dst) fixed (ulong* dof = dstOff)
			fixed (int* dc = dstCap) fixed (int* ol = outLen)
				LLNative.ThrowIfFailed(LLNative.k4lz4_wrap_batch(lease.Handle, s, so, sl, d, dof, dc, ol, n, high ? 1 : 0,
					LZ4Codec.Enforce32 ? LLNative.FLAG_X32 : 0), lease.Handle);
			var result = new byte[n][];
			for (var i = 0; i < n; i++) result[i] = dst.AsSpan((int) dstOff[i], outLen[i]).ToArray();
			return result;
		}

		/// <summary>LZ4Wrapper.Unwrap of every buffer.  decodeOk[i] is false where LZ4Codec.Decode did not return the wrapped
		/// length; Unwrap ignores that and so does this (the result has the wrapped length all the same).</summary>
		public static byte[][] UnwrapBatch(byte[][] buffers, out bool[] decodeOk)
		{
			var n = buffers.Length;
			var src = Pack(buffers, out var srcOff, out _);
			var srcLen = new int[n];
			var dstCap = new int[n];
			var dstOff = new ulong[n];
			long total = 0;
			for (var i = 0; i < n; i++)
			{
				srcLen[i] = buffers[i].Length;
				fixed (byte* b = buffers[i]) dstCap[i] = LLNative.k4lz4_unwrap_size(b, buffers[i].Length);
				if (dstCap[i] < 0) throw Thrown(dstCap[i]);
				dstOff[i] = (ulong) total;
				total += dstCap[i];
			}
			var dst = new byte[Math.Max(total, 1)];
			var outLen = new int[n];
			var decoded = new int[n];
			using var lease = NativeContext.Rent();
			fixed (byte* s = src) fixed (ulong* so = srcOff) fixed (int* sl = srcLen) fixed (byte* d = dst) fixed (ulong* dof = dstOff)
			fixed (int* dc = dstCap) fixed (int* ol = outLen) fixed (int* de = decoded)
				LLNative.ThrowIfFailed(LLNative.k4lz4_unwrap_batch(lease.Handle, s, so, sl, d, dof, dc, ol, de, n), lease.Handle);
			var result = new byte[n][];
			decodeOk = new bool[n];
			for (var i = 0; i < n; i++)
			{
				if (outLen[i] < 0) throw Thrown(outLen[i]);
				result[i] = dst.AsSpan((int) dstOff[i], outLen[i]).ToArray();
				decodeOk[i] = decoded[i] == outLen[i];
			}
			return result;
		}

		/// <summary>What LZ4Legacy.Encode(stream, highCompression, blockSize) writes for each content written whole, then disposed.</summary>
		public static byte[][] EncodeBatch(byte[][] contents, bool highCompression = false, int blockSize = 1024 * 1024)
		{
			var n = contents.Length;
			var src = Pack(contents, out var srcOff, out _);
			var srcLen = new ulong[n];
			var dstCap = new ulong[n];
			var dstOff = new ulong[n];
			long total = 0;
			for (var i = 0; i < n; i++)
			{
				srcLen[i] = (ulong) contents[i].Length;
				dstCap[i] = (ulong) LLNative.k4lz4_legacy_stream_bound(contents[i].Length, blockSize);
				dstOff[i] = (ulong) total;
				total += (long) dstCap[i];
			}
			var dst = new byte[Math.Max(total, 1)];
			var outLen = new long[n];
			using var lease = NativeContext.Rent();
			fixed (byte* s = src) fixed (ulong* so = srcOff) fixed (ulong* sl = srcLen) fixed (byte* d = dst) fixed (ulong* dof = dstOff)
			fixed (ulong* dc = dstCap) fixed (long* ol = outLen)
				LLNative.ThrowIfFailed(LLNative.k4lz4_encode_legacy_streams(lease.Handle, s, so, sl, n, blockSize, highCompression ? 1 : 0,
					LZ4Codec.Enforce32 ? LLNative.FLAG_X32 : 0, d, dof, dc, ol), lease.Handle);
			var result = new byte[n][];
			for (var i = 0; i < n; i++)
			{
				if (outLen[i] < 0) throw Thrown((int) outLen[i]);
				result[i] = dst.AsSpan((int) dstOff[i], (int) outLen[i]).ToArray();
			}
			return result;
		}

		/// <summary>What reading LZ4Legacy.Decode(stream) to its end returns for each stream (two native calls: the sizes, without
		/// trusting a chunk's header beyond what its payload can decode to, then the walk, checks and decoding on the device).</summary>
		public static byte[][] DecodeBatch(byte[][] streams)
		{
			var n = streams.Length;
			var src = Pack(streams, out var srcOff, out _);
			var srcLen = new ulong[n];
			for (var i = 0; i < n; i++) srcLen[i] = (ulong) streams[i].Length;
			var size = new ulong[n];
			var status = new int[n];
			var dstOff = new ulong[n];
			var outLen = new long[n];
			using var lease = NativeContext.Rent();
			fixed (byte* s = src) fixed (ulong* so = srcOff) fixed (ulong* sl = srcLen) fixed (ulong* sz = size) fixed (int* st = status)
				LLNative.ThrowIfFailed(LLNative.k4lz4_legacy_stream_sizes(lease.Handle, s, so, sl, n, sz, st), lease.Handle);
			long total = 0;
			for (var i = 0; i < n; i++) { dstOff[i] = (ulong) total; total += (long) size[i]; }
			var dst = new byte[Math.Max(total, 1)];
			fixed (byte* s = src) fixed (ulong* so = srcOff) fixed (ulong* sl = srcLen) fixed (byte* d = dst) fixed (ulong* dof = dstOff)
			fixed (ulong* dc = size) fixed (long* ol = outLen)
				LLNative.ThrowIfFailed(LLNative.k4lz4_decode_legacy_streams(lease.Handle, s, so, sl, n, d, dof, dc, ol), lease.Handle);
			var result = new byte[n][];
			for (var i = 0; i < n; i++)
			{
				if (outLen[i] < 0) throw Thrown((int) outLen[i]);
				result[i] = dst.AsSpan((int) dstOff[i], (int) outLen[i]).ToArray();
			}
			return result;
		}
	}
}
