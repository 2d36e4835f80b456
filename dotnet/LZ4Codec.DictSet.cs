// LZ4Codec.DictSet.cs -- dictionaries that stay prepared on the device across calls: k4lz4_dict_set (include/k4lz4.h, DESIGN.md 4.22).
// LZ4Codec.EncodeBatch(..., dictionaries, dictionaryIndex) of LZ4Codec.DictBatch.cs loads its list of dictionaries on every call; an
// LZ4DictionarySet is the same list loaded once (the dictionaries' last 64 KiB and the tables LL64.LZ4_loadDict / LL.LZ4_loadDictHC
// leave), read by any number of later EncodeBatch / DecodeBatch calls and freed by Dispose.  The blocks are byte for byte those of the
// per-call form; DecodeBatch is Decode(source, target, dictionary) for many blocks, dictionaryIndex[i] == -1 meaning no dictionary.
// Not under LZ4Codec.Enforce32, not at L10_OPT and up.  Compile-unverified.
using System;
using System.Runtime.InteropServices;
using K4os.Compression.LZ4.Engine;

namespace K4os.Compression.LZ4
{
	internal static unsafe class DictSetNative
	{
		private const string Lib = "k4lz4";

		[DllImport(Lib)] public static extern int k4lz4_dict_set_create(
			IntPtr ctx, byte* dict, ulong* dictOff, int* dictLen, int nDict, int families, out IntPtr set);
		[DllImport(Lib)] public static extern int k4lz4_dict_set_create_device(
			IntPtr ctx, byte* dict, ulong* dictOff, int* dictLen, int nDict, int families, out IntPtr set, IntPtr stream);
		[DllImport(Lib)] public static extern void k4lz4_dict_set_destroy(IntPtr set);
		[DllImport(Lib)] public static extern int k4lz4_dict_set_info(IntPtr set, long* out8);
		[DllImport(Lib)] public static extern int k4lz4_dict_set_layout(
			ulong* dictOff, int* dictLen, int nDict, int families, int* keptLen, ulong* keptAt, int* tableFast, int* tableHc, ulong* bytes);
		[DllImport(Lib)] public static extern int k4lz4_dict_set_state(IntPtr set, int d, void* fastChainState);
		[DllImport(Lib)] public static extern int k4lz4_dict_set_hc_state(IntPtr set, int d, uint* hashTable, ushort* chainTable, int* keptLen);
		[DllImport(Lib)] public static extern int k4lz4_encode_dictset_batch(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int level, int flags,
			int* dictIdx, IntPtr set);
		[DllImport(Lib)] public static extern int k4lz4_encode_dictset_batch_device(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int level, int flags,
			int* dictIdx, IntPtr set, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_decode_dictset_batch(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int flags,
			int* dictIdx, IntPtr set);
		[DllImport(Lib)] public static extern int k4lz4_decode_dictset_batch_device(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int flags,
			int* dictIdx, IntPtr set, IntPtr stream);
	}

	/// <summary>Which tables a set prepares: Fast serves levels below L03_HC (16 KiB per distinct dictionary), High L03_HC .. L09_HC
	/// (256 KiB per distinct dictionary).  Decoding needs neither.</summary>
	[Flags]
	public enum LZ4DictionaryFamilies { Fast = 1, High = 2, Both = 3 }

	/// <summary>A list of dictionaries prepared on the device once.  Immutable; any thread may encode and decode against it at the
	/// same time (every call rents a context of its own); Dispose waits for the calls that still read it.</summary>
	public sealed unsafe class LZ4DictionarySet: IDisposable
	{
		private IntPtr _handle;

		public int Count { get; }
		public LZ4DictionaryFamilies Families { get; }
		internal IntPtr Handle => _handle != IntPtr.Zero ? _handle : throw new ObjectDisposedException(nameof(LZ4DictionarySet));

		/// <summary>Dictionary d is dictionaries[dictionaryOffsets[d] .. +dictionaryLengths[d]).  The set copies what it keeps: the
		/// buffers are the caller's again when the constructor returns.</summary>
		public LZ4DictionarySet(
			ReadOnlySpan<byte> dictionaries, ReadOnlySpan<ulong> dictionaryOffsets, ReadOnlySpan<int> dictionaryLengths,
			LZ4DictionaryFamilies families = LZ4DictionaryFamilies.Both)
		{
			if (dictionaryOffsets.Length != dictionaryLengths.Length) throw new ArgumentException("dictionary vectors differ in length");
			for (var d = 0; d < dictionaryLengths.Length; d++)
				if (dictionaryLengths[d] < 0 || dictionaryOffsets[d] + (ulong) dictionaryLengths[d] > (ulong) dictionaries.Length)
					throw new ArgumentException($"dictionary {d}: range outside the buffer");
			using var lease = NativeContext.Rent();
			var ctx = lease.Handle;
			fixed (byte* dc = dictionaries)
			fixed (ulong* dof = dictionaryOffsets)
			fixed (int* dl = dictionaryLengths)
				LLNative.ThrowIfFailed(
					DictSetNative.k4lz4_dict_set_create(ctx, dc, dof, dl, dictionaryLengths.Length, (int) families, out _handle), ctx);
			Count = dictionaryLengths.Length;
			Families = families;
		}

		public LZ4DictionarySet(byte[][] dictionaries, LZ4DictionaryFamilies families = LZ4DictionaryFamilies.Both)
			: this(Pack(dictionaries, out var off, out var len), off, len, families) { }

		// only the last 64 KiB of a dictionary are ever looked at
		private static byte[] Pack(byte[][] dictionaries, out ulong[] off, out int[] len)
		{
			if (dictionaries is null) throw new ArgumentNullException(nameof(dictionaries));
			long total = 0;
			for (var d = 0; d < dictionaries.Length; d++)
				total += Math.Min((dictionaries[d] ?? throw new ArgumentNullException($"{nameof(dictionaries)}[{d}]")).Length, 65536);
			if (total > int.MaxValue - 64) throw new ArgumentException("the dictionaries do not fit one packed buffer");
			var buf = new byte[Math.Max(1, total)];
			off = new ulong[dictionaries.Length]; len = new int[dictionaries.Length];
			var at = 0;
			for (var d = 0; d < dictionaries.Length; d++)
			{
				var kept = Math.Min(dictionaries[d].Length, 65536);
				off[d] = (ulong) at; len[d] = kept;
				Buffer.BlockCopy(dictionaries[d], dictionaries[d].Length - kept, buf, at, kept);
				at += kept;
			}
			return buf;
		}

		/// <summary>k4lz4_dict_set_info: nDict, tables of the fast family, of the high family, device bytes, families, device ordinal,
		/// load launches of either family (fixed at construction: no call loads anything).</summary>
		public long[] Info()
		{
			var v = new long[8];
			fixed (long* p = v)
				if (DictSetNative.k4lz4_dict_set_info(Handle, p) != 0) throw new InvalidOperationException("k4lz4_dict_set_info failed");
			return v;
		}

		public void Dispose()
		{
			var h = System.Threading.Interlocked.Exchange(ref _handle, IntPtr.Zero);
			if (h != IntPtr.Zero) DictSetNative.k4lz4_dict_set_destroy(h);
			GC.SuppressFinalize(this);
		}

		~LZ4DictionarySet() => Dispose();
	}

	public static partial class LZ4Codec
	{
		/// <summary>EncodeBatch(..., dictionaries, dictionaryIndex) with the list being a set: the same blocks, and only the messages
		/// travel to the device.</summary>
		public static unsafe void EncodeBatch(
			ReadOnlySpan<byte> source, ReadOnlySpan<ulong> sourceOffsets, ReadOnlySpan<int> sourceLengths,
			Span<byte> target, ReadOnlySpan<ulong> targetOffsets, ReadOnlySpan<int> targetLengths,
			Span<int> encodedLengths, LZ4DictionarySet dictionaries, ReadOnlySpan<int> dictionaryIndex, LZ4Level level = LZ4Level.L00_FAST)
		{
			if (dictionaries is null) throw new ArgumentNullException(nameof(dictionaries));
			var n = ValidateBatch(source.Length, sourceOffsets, sourceLengths, target.Length, targetOffsets, targetLengths, encodedLengths.Length);
			if (level >= LZ4Level.L10_OPT) throw new ArgumentException("levels 10 - 12 with a dictionary are not supported", nameof(level));
			if (dictionaryIndex.Length != n) throw new ArgumentException("one dictionary index per message");
			if (n == 0) return;
			using var lease = NativeContext.Rent();
			var ctx = lease.Handle;
			fixed (byte* s = source, t = target)
			fixed (ulong* so = sourceOffsets, to = targetOffsets)
			fixed (int* sl = sourceLengths, tl = targetLengths, ol = encodedLengths, di = dictionaryIndex)
				LLNative.ThrowIfFailed(
					DictSetNative.k4lz4_encode_dictset_batch(ctx, s, so, sl, t, to, tl, ol, n, (int) level, 0, di, dictionaries.Handle), ctx);
			GC.KeepAlive(dictionaries);
		}

		/// <summary>Decode(source, target, dictionary) for n blocks, block i against entry dictionaryIndex[i] of the set (-1: no
		/// dictionary).  decodedLengths[i]: bytes written, or -1 where Decode returns a negative value.</summary>
		public static unsafe void DecodeBatch(
			ReadOnlySpan<byte> source, ReadOnlySpan<ulong> sourceOffsets, ReadOnlySpan<int> sourceLengths,
			Span<byte> target, ReadOnlySpan<ulong> targetOffsets, ReadOnlySpan<int> targetLengths,
			Span<int> decodedLengths, LZ4DictionarySet dictionaries, ReadOnlySpan<int> dictionaryIndex)
		{
			if (dictionaries is null) throw new ArgumentNullException(nameof(dictionaries));
			var n = ValidateBatch(source.Length, sourceOffsets, sourceLengths, target.Length, targetOffsets, targetLengths, decodedLengths.Length);
			if (dictionaryIndex.Length != n) throw new ArgumentException("one dictionary index per block");
			if (n == 0) return;
			using var lease = NativeContext.Rent();
			var ctx = lease.Handle;
			fixed (byte* s = source, t = target)
			fixed (ulong* so = sourceOffsets, to = targetOffsets)
			fixed (int* sl = sourceLengths, tl = targetLengths, ol = decodedLengths, di = dictionaryIndex)
				LLNative.ThrowIfFailed(
					DictSetNative.k4lz4_decode_dictset_batch(ctx, s, so, sl, t, to, tl, ol, n, 0, di, dictionaries.Handle), ctx);
			GC.KeepAlive(dictionaries);
		}
	}
}
