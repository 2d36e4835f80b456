// LZ4Codec.DictBatch.cs -- batches of messages encoded against shared dictionaries, the counterpart of
// LZ4Codec.Decode(source, target, dictionary): k4lz4_encode_dict_batch (include/k4lz4.h, DESIGN.md 4.20).  Message i is encoded
// against dictionaries[dictionaryIndex[i]]; its block is what LL64.LZ4_loadDict followed by LL64.LZ4_compress_fast_continue on that
// stream writes (Engine/x64/LL64.tools.cs:175-206, LL64.fast.cs:582-667) and decodes with Decode(source, target, dictionary) given
// the same dictionary.  At L03_HC .. L09_HC the call is k4lz4_encode_dict_hc_batch (DESIGN.md 4.21) and the block is what
// LL.LZ4_loadDictHC followed by LL64.LZ4_compress_HC_continue writes; L10_OPT and up are refused (no sound witness for the optimal
// parser with a dictionary).  Not under LZ4Codec.Enforce32.  Compile-unverified.
using System;
using System.Runtime.InteropServices;
using K4os.Compression.LZ4.Engine;

namespace K4os.Compression.LZ4
{
	internal static unsafe class DictBatchNative
	{
		private const string Lib = "k4lz4";

		[DllImport(Lib)] public static extern int k4lz4_encode_dict_batch(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int level, int flags,
			int* dictIdx, byte* dict, ulong* dictOff, int* dictLen, int nDict);
		[DllImport(Lib)] public static extern int k4lz4_encode_dict_batch_device(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int level, int flags,
			int* dictIdx, byte* dict, ulong* dictOff, int* dictLen, int nDict, IntPtr stream);
	}

	public static partial class LZ4Codec
	{
		/// <summary>Compresses n messages, message i against dictionaries[dictionaryOffsets[d] .. +dictionaryLengths[d]) with
		/// d = dictionaryIndex[i].  encodedLengths[i]: bytes written, 0 for an empty message, -1 when the block does not fit its
		/// target.  Only a dictionary's last 64 KiB count; at the fast levels one of fewer than 8 bytes is an empty dictionary.</summary>
		public static unsafe void EncodeBatch(
			ReadOnlySpan<byte> source, ReadOnlySpan<ulong> sourceOffsets, ReadOnlySpan<int> sourceLengths,
			Span<byte> target, ReadOnlySpan<ulong> targetOffsets, ReadOnlySpan<int> targetLengths,
			Span<int> encodedLengths,
			ReadOnlySpan<byte> dictionaries, ReadOnlySpan<ulong> dictionaryOffsets, ReadOnlySpan<int> dictionaryLengths,
			ReadOnlySpan<int> dictionaryIndex, LZ4Level level = LZ4Level.L00_FAST)
		{
			var n = ValidateBatch(source.Length, sourceOffsets, sourceLengths, target.Length, targetOffsets, targetLengths, encodedLengths.Length);
			if (level >= LZ4Level.L10_OPT) throw new ArgumentException("levels 10 - 12 with a dictionary are not supported", nameof(level));
			if (dictionaryIndex.Length != n || dictionaryOffsets.Length != dictionaryLengths.Length)
				throw new ArgumentException("dictionary vectors differ in length");
			for (var d = 0; d < dictionaryLengths.Length; d++)
				if (dictionaryLengths[d] < 0 || dictionaryOffsets[d] + (ulong) dictionaryLengths[d] > (ulong) dictionaries.Length)
					throw new ArgumentException($"dictionary {d}: range outside the buffer");
			for (var i = 0; i < n; i++)
				if (dictionaryIndex[i] < 0 || dictionaryIndex[i] >= dictionaryLengths.Length)
					throw new ArgumentException($"message {i}: no dictionary {dictionaryIndex[i]}");
			if (n == 0) return;
			using var lease = NativeContext.Rent();
			var ctx = lease.Handle;
			fixed (byte* s = source, t = target, dc = dictionaries)
			fixed (ulong* so = sourceOffsets, to = targetOffsets, dof = dictionaryOffsets)
			fixed (int* sl = sourceLengths, tl = targetLengths, ol = encodedLengths, dl = dictionaryLengths, di = dictionaryIndex)
				LLNative.ThrowIfFailed(
					level >= LZ4Level.L03_HC
						? LLNative.k4lz4_encode_dict_hc_batch(ctx, s, so, sl, t, to, tl, ol, n, (int) level, 0, di, dc, dof, dl, dictionaryLengths.Length)
						: DictBatchNative.k4lz4_encode_dict_batch(ctx, s, so, sl, t, to, tl, ol, n, (int) level, 0, di, dc, dof, dl, dictionaryLengths.Length), ctx);
		}

		/// <summary>Convenience form: every message compressed into a fresh array against dictionaries[dictionaryIndex[i]].</summary>
		public static byte[][] EncodeBatch(byte[][] messages, byte[][] dictionaries, int[] dictionaryIndex, LZ4Level level = LZ4Level.L00_FAST)
		{
			if (messages is null) throw new ArgumentNullException(nameof(messages));
			if (dictionaries is null) throw new ArgumentNullException(nameof(dictionaries));
			if (dictionaryIndex is null) throw new ArgumentNullException(nameof(dictionaryIndex));
			var n = messages.Length;
			long st = 0, dt = 0, ct = 0;
			for (var i = 0; i < n; i++)
			{
				if (messages[i] is null) throw new ArgumentNullException($"{nameof(messages)}[{i}]");
				st += messages[i].Length; dt += MaximumOutputSize(messages[i].Length);
			}
			for (var d = 0; d < dictionaries.Length; d++)
			{
				if (dictionaries[d] is null) throw new ArgumentNullException($"{nameof(dictionaries)}[{d}]");
				ct += Math.Min(dictionaries[d].Length, 65536);
			}
			if (st > MaxPackedBytes || dt > MaxPackedBytes || ct > MaxPackedBytes)
				throw new ArgumentException("the batch does not fit one packed call: split it");
			var src = new byte[Math.Max(1, st)]; var dst = new byte[Math.Max(1, dt)]; var dct = new byte[Math.Max(1, ct)];
			var srcOff = new ulong[n]; var srcLen = new int[n]; var dstOff = new ulong[n]; var dstCap = new int[n]; var outLen = new int[n];
			var dictOff = new ulong[dictionaries.Length]; var dictLen = new int[dictionaries.Length];
			int sp = 0, dp = 0, cp = 0;
			for (var i = 0; i < n; i++)
			{
				srcOff[i] = (ulong) sp; srcLen[i] = messages[i].Length;
				Buffer.BlockCopy(messages[i], 0, src, sp, messages[i].Length);
				sp += messages[i].Length;
				dstOff[i] = (ulong) dp; dstCap[i] = MaximumOutputSize(messages[i].Length); dp += dstCap[i];
			}
			for (var d = 0; d < dictionaries.Length; d++)
			{
				var kept = Math.Min(dictionaries[d].Length, 65536);      // LZ4_loadDict and LZ4_loadDictHC keep the last 64 KiB
				dictOff[d] = (ulong) cp; dictLen[d] = kept;
				Buffer.BlockCopy(dictionaries[d], dictionaries[d].Length - kept, dct, cp, kept);
				cp += kept;
			}
			EncodeBatch(src, srcOff, srcLen, dst, dstOff, dstCap, outLen, dct, dictOff, dictLen, dictionaryIndex, level);
			var result = new byte[n][];
			for (var i = 0; i < n; i++)
			{
				if (outLen[i] < 0) throw new InvalidOperationException($"message {i} did not fit into MaximumOutputSize bytes"); // cannot happen
				result[i] = new byte[outLen[i]];
				Buffer.BlockCopy(dst, (int) dstOff[i], result[i], 0, outLen[i]);
			}
			return result;
		}
	}
}
