// K4os.Compression.LZ4.Legacy/LZ4Legacy.FedStreamBatch.cs -- many open LZ4Streams in Decompress mode whose sources arrive in pieces
// (sockets, pipes, files read as they grow), advanced together through k4lz4_legacy_read_fed_batch (include/k4lz4.h, DESIGN.md 4.17).
// The reference reads a chunk's varints one byte at a time (LZ4Stream.cs:133-155) and loops until a payload is complete (:176-191),
// so how a source is cut is invisible in what Read returns; here a read that meets an incomplete field comes back starved (need > 0)
// with the field's bytes kept in the stream's device store, and is issued again with the count reduced once more bytes are fed.
// Only the pieces travel to the device.  Compile-unverified.
using System;
using System.Collections.Generic;
using System.Runtime.InteropServices;

namespace K4os.Compression.LZ4.Legacy
{
	internal static unsafe class LegacyFedStreamNative
	{
		private const string Lib = "k4lz4";
		public const int READER_FED = 1;

		[DllImport(Lib)] public static extern int k4lz4_legacy_reader_init_fed(LegacyStreamNative.Reader* r, int maxBlockSize);
		[DllImport(Lib)] public static extern int k4lz4_legacy_read_fed_batch(IntPtr ctx, LegacyStreamNative.Reader* r, byte* store, ulong* storeOff,
			byte* src, ulong* srcOff, ulong* srcLen, long* final, byte* dst, ulong* dstOff, long* count, long* outLen, long* consumed, long* need,
			long n, int op, int flags);
		[DllImport(Lib)] public static extern int k4lz4_legacy_read_fed_batch_device(IntPtr ctx, LegacyStreamNative.Reader* r, byte* store,
			ulong* storeOff, byte* src, ulong* srcOff, ulong* srcLen, long* final, byte* dst, ulong* dstOff, long* count, long* outLen,
			long* consumed, long* need, long n, int op, int flags, long maxCount, IntPtr stream);
	}

	/// <summary>n LZ4Streams in Decompress mode fed piece by piece.  Feed appends a stream's next bytes behind what it has not consumed
	/// yet; Read(counts) is one k4lz4_legacy_read_fed_batch over what is held: per stream the bytes delivered, and in Need the number
	/// of further source bytes a starved read waits for (0: the read is complete).  The bytes, total and exception of a read issued
	/// again until it is no longer starved are those of one LZ4Stream.Read(count) over the whole source.</summary>
	public sealed unsafe class LZ4StreamFedReaderBatch: IDisposable
	{
		private LegacyStreamNative.Reader _record;
		private readonly List<byte>[] _held;
		private readonly long[] _final;
		private readonly ulong[] _storeOff;
		private byte* _store;

		public long[] Consumed { get; private set; }
		public long[] Need { get; private set; }

		public LZ4StreamFedReaderBatch(int n, int maxBlockSize = 1024 * 1024)
		{
			fixed (LegacyStreamNative.Reader* r = &_record)
				if (LegacyFedStreamNative.k4lz4_legacy_reader_init_fed(r, maxBlockSize) != 0)
					throw new ArgumentException("maxBlockSize is too large", nameof(maxBlockSize));
			_held = new List<byte>[n]; _final = new long[n]; _storeOff = new ulong[n];
			for (var i = 0; i < n; i++) { _held[i] = new List<byte>(); _storeOff[i] = (ulong) (i * _record.storeBytes); }
			_store = LegacyStreamNative.Alloc(n * _record.storeBytes + 64);
			Consumed = new long[n]; Need = new long[n];
			Call(new long[n], LegacyStreamNative.RESET, false, out _);
		}

		/// <summary>stream i's next bytes (null: none); final: nothing will follow</summary>
		public void Feed(int i, byte[] piece, bool final = false)
		{
			if (piece != null && piece.Length > 0)
			{
				if (_final[i] != 0) throw new InvalidOperationException("the stream was fed its final piece already");
				_held[i].AddRange(piece);
			}
			if (final) _final[i] = 1;
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
					_held[i].RemoveRange(0, (int) Consumed[i]);
				}
				at += Math.Max(counts[i], 0);
			}
			return result;
		}

		/// <summary>the K4LZ4_LSQ_* words of every stream; the position is the sum of Consumed</summary>
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
			var srcOff = new ulong[n]; var srcLen = new ulong[n]; var dstOff = new ulong[n]; var outLen = new long[n];
			long room = 0, total = 0;
			for (var i = 0; i < n; i++)
			{
				srcOff[i] = (ulong) total; srcLen[i] = (ulong) _held[i].Count; total += _held[i].Count;
				dstOff[i] = (ulong) room; room += op == LegacyStreamNative.READ ? Math.Max(counts[i], 0) : 0;
			}
			var src = new byte[Math.Max(total, 1)];
			for (var i = 0; i < n; i++) _held[i].CopyTo(src, (int) srcOff[i]);
			dst = new byte[Math.Max(room, 1)];
			using var lease = NativeContext.Rent();
			fixed (LegacyStreamNative.Reader* r = &_record)
			fixed (byte* s = src, d = dst)
			fixed (ulong* so = srcOff, sl = srcLen, sto = _storeOff, dof = dstOff)
			fixed (long* c = counts, ol = outLen, fin = _final, cons = Consumed, need = Need)
				LLNative.ThrowIfFailed(LegacyFedStreamNative.k4lz4_legacy_read_fed_batch(lease.Handle, r, _store, sto, s, so, sl, fin, d, dof, c, ol,
					cons, need, n, op, interactive ? LegacyStreamNative.INTERACTIVE : 0), lease.Handle);
			return outLen;
		}

		public void Dispose()
		{
			if (_store != null) LegacyStreamNative.hipFree(_store);
			_store = null;
		}
	}
}
