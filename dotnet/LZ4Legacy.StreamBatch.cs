// K4os.Compression.LZ4.Legacy/LZ4Legacy.StreamBatch.cs -- many open LZ4Streams advanced together, one Write / Flush / Dispose or one
// Read(count) each per call, through k4lz4_legacy_write_batch and k4lz4_legacy_read_batch (include/k4lz4.h, DESIGN.md 4.16).
// Per stream a call returns exactly what LZ4Stream pushes to (LZ4Stream.cs:209-243, :313-316, :414-450) or returns from
// (:248-294, :349-377) its inner stream during that call; the lazy flush is the reference's: a buffer that a Write fills exactly
// goes out with the next byte, or at Flush / Dispose.  The writer's record is host memory advanced from lengths alone; the pending
// bytes and the readers' state live in device stores allocated here with hipMalloc.  Compile-unverified.
using System;
using System.IO;
using System.Runtime.InteropServices;

namespace K4os.Compression.LZ4.Legacy
{
	internal static unsafe class LegacyStreamNative
	{
		private const string Lib = "k4lz4";

		[StructLayout(LayoutKind.Sequential)]
		public struct Writer { public int blockSize, high, pending, closed; }

		[StructLayout(LayoutKind.Sequential)]
		public struct Reader { public int maxBlockSize, flags; public long storeBytes; }

		public const int WRITE = 0, FLUSH = 1, CLOSE = 2;
		public const int READ = 0, RESET = 1, INTERACTIVE = 1, QUERY_WORDS = 8;
		public const int END_OF_STREAM = -1, OVERFLOW = -2, NOT_SUPPORTED = -3, INVALID_DATA = -4, CAPACITY = -6, NOT_ENCODED = -7,
			BLOCK_SIZE = -8, CLOSED = -9;

		[DllImport(Lib)] public static extern int k4lz4_legacy_writer_init(Writer* w, int blockSize, int high);
		[DllImport(Lib)] public static extern long k4lz4_legacy_writer_store_bytes(Writer* w);
		[DllImport(Lib)] public static extern long k4lz4_legacy_write_bound(Writer* w, long srcLen, int op);
		[DllImport(Lib)] public static extern int k4lz4_legacy_write_batch(IntPtr ctx, Writer* w, byte* store, ulong* storeOff, byte* src,
			ulong* srcOff, long* srcLen, byte* dst, ulong* dstOff, ulong* dstCap, long* outLen, long n, int op, int flags);
		[DllImport(Lib)] public static extern int k4lz4_legacy_write_batch_device(IntPtr ctx, Writer* w, byte* store, ulong* storeOff, byte* src,
			ulong* srcOff, long* srcLen, byte* dst, ulong* dstOff, ulong* dstCap, long* outLen, long n, int op, int flags, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_legacy_reader_init(Reader* r, int maxBlockSize);
		[DllImport(Lib)] public static extern long k4lz4_legacy_reader_store_bytes(Reader* r);
		[DllImport(Lib)] public static extern long k4lz4_legacy_read_table_rows(Reader* r, long maxCount);
		[DllImport(Lib)] public static extern int k4lz4_legacy_read_batch(IntPtr ctx, Reader* r, byte* store, ulong* storeOff, byte* src,
			ulong* srcOff, ulong* srcLen, byte* dst, ulong* dstOff, long* count, long* outLen, long n, int op, int flags);
		[DllImport(Lib)] public static extern int k4lz4_legacy_read_batch_device(IntPtr ctx, Reader* r, byte* store, ulong* storeOff, byte* src,
			ulong* srcOff, ulong* srcLen, byte* dst, ulong* dstOff, long* count, long* outLen, long n, int op, int flags, long maxCount,
			IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_legacy_reader_query(IntPtr ctx, byte* store, ulong* storeOff, long n, long* @out);
		[DllImport(Lib)] public static extern int k4lz4_legacy_reader_query_device(IntPtr ctx, byte* store, ulong* storeOff, long n, long* @out,
			IntPtr stream);

		[DllImport("amdhip64")] public static extern int hipMalloc(byte** p, UIntPtr bytes);
		[DllImport("amdhip64")] public static extern int hipFree(byte* p);

		public static Exception Thrown(long code) => code switch {
			END_OF_STREAM => new EndOfStreamException("Unexpected end of stream"),
			OVERFLOW => new OverflowException(),
			NOT_SUPPORTED => new NotSupportedException("Chunks with multiple passes are not supported."),
			INVALID_DATA => new InvalidDataException("Compressed data corrupted"),
			CAPACITY => new ArgumentException("the target is too small"),
			NOT_ENCODED => new OutOfMemoryException("HC scratch reserved with k4lz4_ctx_reserve_hc was too small"),
			BLOCK_SIZE => new ArgumentException("a chunk is larger than the reader's maxBlockSize"),
			CLOSED => new ObjectDisposedException(nameof(LZ4Stream)),
			_ => new InvalidOperationException($"unknown legacy result {code}"),
		};

		public static byte* Alloc(long bytes)
		{
			byte* p;
			if (hipMalloc(&p, (UIntPtr) (ulong) Math.Max(bytes, 1)) != 0) throw new OutOfMemoryException("hipMalloc");
			return p;
		}
	}

	/// <summary>n LZ4Streams in Compress mode.  Write / Flush / Close return, per stream, the bytes the reference's stream pushes to
	/// its inner stream during that call (null where the chunk is null: the stream sits the call out).</summary>
	public sealed unsafe class LZ4StreamWriterBatch: IDisposable
	{
		private readonly LegacyStreamNative.Writer[] _records;
		private readonly ulong[] _storeOff;
		private byte* _store;

		public LZ4StreamWriterBatch(int n, bool highCompression = false, int blockSize = 1024 * 1024)
		{
			_records = new LegacyStreamNative.Writer[n];
			_storeOff = new ulong[n];
			long at = 0;
			fixed (LegacyStreamNative.Writer* w = _records)
				for (var i = 0; i < n; i++)
				{
					if (LegacyStreamNative.k4lz4_legacy_writer_init(w + i, blockSize, highCompression ? 1 : 0) != 0)
						throw new ArgumentException("blockSize is too large", nameof(blockSize));
					_storeOff[i] = (ulong) at;
					at += (LegacyStreamNative.k4lz4_legacy_writer_store_bytes(w + i) + 255) / 256 * 256;
				}
			_store = LegacyStreamNative.Alloc(at + 64);
		}

		public byte[][] Write(byte[][] chunks) => Call(chunks, LegacyStreamNative.WRITE);
		public byte[][] Flush() => Call(Empty(), LegacyStreamNative.FLUSH);
		public byte[][] Close(byte[][] chunks = null) => Call(chunks ?? Empty(), LegacyStreamNative.CLOSE);

		private byte[][] Empty()
		{
			var e = new byte[_records.Length][];
			for (var i = 0; i < e.Length; i++) e[i] = Array.Empty<byte>();
			return e;
		}

		private byte[][] Call(byte[][] chunks, int op)
		{
			var n = _records.Length;
			if (chunks.Length != n) throw new ArgumentException("one chunk (or null) per stream");
			var srcOff = new ulong[n]; var srcLen = new long[n]; var dstOff = new ulong[n]; var dstCap = new ulong[n]; var outLen = new long[n];
			long total = 0, room = 0;
			for (var i = 0; i < n; i++) { srcOff[i] = (ulong) total; srcLen[i] = chunks[i]?.Length ?? -1; total += Math.Max(srcLen[i], 0); }
			var src = new byte[Math.Max(total, 1)];
			for (var i = 0; i < n; i++) if (srcLen[i] > 0) Buffer.BlockCopy(chunks[i], 0, src, (int) srcOff[i], (int) srcLen[i]);
			using var lease = NativeContext.Rent();
			fixed (LegacyStreamNative.Writer* w = _records)
			{
				for (var i = 0; i < n; i++)
				{
					dstOff[i] = (ulong) room;
					dstCap[i] = (ulong) LegacyStreamNative.k4lz4_legacy_write_bound(w + i, srcLen[i], op);
					room += (long) dstCap[i];
				}
				var dst = new byte[Math.Max(room, 1)];
				fixed (byte* s = src, d = dst)
				fixed (ulong* so = srcOff, sto = _storeOff, dof = dstOff, dc = dstCap)
				fixed (long* sl = srcLen, ol = outLen)
					LLNative.ThrowIfFailed(LegacyStreamNative.k4lz4_legacy_write_batch(lease.Handle, w, _store, sto, s, so, sl, d, dof, dc, ol, n, op, 0),
						lease.Handle);
				var result = new byte[n][];
				for (var i = 0; i < n; i++)
				{
					if (srcLen[i] < 0) continue;
					if (outLen[i] < 0) throw LegacyStreamNative.Thrown(outLen[i]);
					result[i] = new byte[outLen[i]];
					Buffer.BlockCopy(dst, (int) dstOff[i], result[i], 0, (int) outLen[i]);
				}
				return result;
			}
		}

		public void Dispose()
		{
			if (_store != null) LegacyStreamNative.hipFree(_store);
			_store = null;
		}
	}

	/// <summary>n LZ4Streams in Decompress mode over sources held in host memory.  Read(counts) is one Read(count) per stream
	/// (a negative count: the stream sits the call out); it throws what the reference's Read throws for the lowest-index failing
	/// stream, and such a stream stays failed.</summary>
	public sealed unsafe class LZ4StreamReaderBatch: IDisposable
	{
		private LegacyStreamNative.Reader _record;
		private readonly byte[] _src;
		private readonly ulong[] _srcOff, _srcLen, _storeOff;
		private byte* _store;

		public LZ4StreamReaderBatch(byte[][] sources, int maxBlockSize = 1024 * 1024)
		{
			var n = sources.Length;
			fixed (LegacyStreamNative.Reader* r = &_record)
				if (LegacyStreamNative.k4lz4_legacy_reader_init(r, maxBlockSize) != 0)
					throw new ArgumentException("maxBlockSize is too large", nameof(maxBlockSize));
			_srcOff = new ulong[n]; _srcLen = new ulong[n]; _storeOff = new ulong[n];
			long total = 0;
			for (var i = 0; i < n; i++) { _srcOff[i] = (ulong) total; _srcLen[i] = (ulong) sources[i].Length; total += sources[i].Length; _storeOff[i] = (ulong) (i * _record.storeBytes); }
			_src = new byte[Math.Max(total, 1)];
			for (var i = 0; i < n; i++) Buffer.BlockCopy(sources[i], 0, _src, (int) _srcOff[i], sources[i].Length);
			_store = LegacyStreamNative.Alloc(n * _record.storeBytes + 64);
			Call(new long[n], LegacyStreamNative.RESET, false, out _);
		}

		public byte[][] Read(long[] counts, bool interactive = false)
		{
			var outLen = Call(counts, LegacyStreamNative.READ, interactive, out var dst);
			var result = new byte[counts.Length][];
			long at = 0;
			for (var i = 0; i < counts.Length; i++)
			{
				if (counts[i] >= 0)
				{
					if (outLen[i] < 0) throw LegacyStreamNative.Thrown(outLen[i]);
					result[i] = new byte[outLen[i]];
					Buffer.BlockCopy(dst, (int) at, result[i], 0, (int) outLen[i]);
				}
				at += Math.Max(counts[i], 0);
			}
			return result;
		}

		/// <summary>the K4LZ4_LSQ_* words of every stream</summary>
		public long[] Query()
		{
			var q = new long[Math.Max(_storeOff.Length, 1) * LegacyStreamNative.QUERY_WORDS];
			using var lease = NativeContext.Rent();
			fixed (ulong* sto = _storeOff)
			fixed (long* o = q)
				LLNative.ThrowIfFailed(LegacyStreamNative.k4lz4_legacy_reader_query(lease.Handle, _store, sto, _storeOff.Length, o), lease.Handle);
			return q;
		}

		private long[] Call(long[] counts, int op, bool interactive, out byte[] dst)
		{
			var n = _storeOff.Length;
			if (counts.Length != n) throw new ArgumentException("one count per stream");
			var dstOff = new ulong[n]; var outLen = new long[n];
			long room = 0;
			for (var i = 0; i < n; i++) { dstOff[i] = (ulong) room; room += op == LegacyStreamNative.READ ? Math.Max(counts[i], 0) : 0; }
			dst = new byte[Math.Max(room, 1)];
			using var lease = NativeContext.Rent();
			fixed (LegacyStreamNative.Reader* r = &_record)
			fixed (byte* s = _src, d = dst)
			fixed (ulong* so = _srcOff, sl = _srcLen, sto = _storeOff, dof = dstOff)
			fixed (long* c = counts, ol = outLen)
				LLNative.ThrowIfFailed(LegacyStreamNative.k4lz4_legacy_read_batch(lease.Handle, r, _store, sto, s, so, sl, d, dof, c, ol, n, op,
					interactive ? LegacyStreamNative.INTERACTIVE : 0), lease.Handle);
			return outLen;
		}

		public void Dispose()
		{
			if (_store != null) LegacyStreamNative.hipFree(_store);
			_store = null;
		}
	}
}
