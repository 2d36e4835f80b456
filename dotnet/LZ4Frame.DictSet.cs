// K4os.Compression.LZ4.Streams/Frames/LZ4Frame.DictSet.cs -- frames with a predefined dictionary (FLG bit 0, DictID) read against an
// LZ4DictionarySet: k4lz4_frame_sizes_dictset / k4lz4_decode_frames_dictset (include/k4lz4.h, DESIGN.md 4.24).  The reader of
// LZ4FrameBatch.DecodeBatch with a set and one id per entry beside it: a frame's DictID resolves to the first entry whose id equals it,
// a frame without the bit decodes without a dictionary, and a DictID that nothing answers to throws what every DictID throws without
// a set (NotImplementedException).  The writer: Encode / EncodeBatch name the entry's id as the frame's DictID and take the blocks
// from LZ4Codec.EncodeBatch(..., set, dictionaryIndex) with the allowCopy rule (independent frames) or from an LZ4EncoderBatch opened
// from the entry, one record -- Topup and a forced Encode -- per block (chained frames); the layout is LZ4FrameBatch.Assemble's.  Not
// at L10_OPT and up, not under LZ4Codec.Enforce32.  The incremental readers take a set of their own (LZ4FrameReaderBatch.DictSet.cs,
// LZ4FrameFedReaderBatch.DictSet.cs, DESIGN.md 4.25); the incremental writer (LZ4FrameWriterBatch) keeps refusing the dictionary bit.
// The executable form of all of it is frames.py.  Compile-unverified.
using System;
using K4os.Compression.LZ4.Encoders;
using K4os.Compression.LZ4.Engine;

namespace K4os.Compression.LZ4.Engine
{
	internal static unsafe partial class LLNative
	{
		// dictIds: a HOST array of one uint per entry of the set in all four; outDictIdx may be null
		[System.Runtime.InteropServices.DllImport(Lib)] public static extern int k4lz4_frame_sizes_dictset(
			IntPtr ctx, byte* src, ulong* frameOff, ulong* frameLen, long n, ulong* outSize, int* outStatus, int* outDictIdx, IntPtr set,
			uint* dictIds);
		[System.Runtime.InteropServices.DllImport(Lib)] public static extern int k4lz4_decode_frames_dictset(
			IntPtr ctx, byte* src, ulong* frameOff, ulong* frameLen, long n, byte* dst, ulong* dstOff, ulong* dstCap, long* outLen, IntPtr set,
			uint* dictIds);
		[System.Runtime.InteropServices.DllImport(Lib)] public static extern int k4lz4_frame_sizes_dictset_device(
			IntPtr ctx, byte* src, ulong* frameOff, ulong* frameLen, long n, ulong* outSize, int* outStatus, int* outDictIdx, IntPtr set,
			uint* dictIds, IntPtr stream);
		[System.Runtime.InteropServices.DllImport(Lib)] public static extern int k4lz4_decode_frames_dictset_device(
			IntPtr ctx, byte* src, ulong* frameOff, ulong* frameLen, long n, byte* dst, ulong* dstOff, ulong* dstCap, long* outLen, IntPtr set,
			uint* dictIds, IntPtr stream);
	}
}

namespace K4os.Compression.LZ4.Streams.Frames
{
	public static unsafe class LZ4FrameDictSet
	{
		/// <summary>One frame around content whose header names dictionaryIds[dictionaryIndex] and whose blocks are encoded against
		/// that entry of the set; dictionaryIndex -1: LZ4FrameBatch.Encode's plain frame.</summary>
		public static byte[] Encode(
			ReadOnlySpan<byte> content, LZ4EncoderSettings settings, LZ4DictionarySet dictionaries, ReadOnlySpan<uint> dictionaryIds,
			int dictionaryIndex)
		{
			if (dictionaries is null) throw new ArgumentNullException(nameof(dictionaries));
			if (dictionaryIds.Length != dictionaries.Count) throw new ArgumentException("one id per entry of the set", nameof(dictionaryIds));
			if (dictionaryIndex < -1 || dictionaryIndex >= dictionaries.Count) throw new ArgumentOutOfRangeException(nameof(dictionaryIndex));
			if (dictionaryIndex < 0) return LZ4FrameBatch.Encode(content, settings);
			if (settings.CompressionLevel >= LZ4Level.L10_OPT || LZ4Codec.Enforce32)
				throw new NotImplementedException("frames with a predefined dictionary: L00_FAST .. L09_HC of the 64-bit engine");
			var chained = settings.ChainBlocks;
			var blockSize = LZ4FrameBatch.MaxBlockSize(settings.BlockSize, out var bdCode);
			var encoderBlock = chained ? (Math.Max(blockSize, 1024) + 1023) / 1024 * 1024 : blockSize;
			var n = (int) (((long) content.Length + encoderBlock - 1) / encoderBlock);
			var slot = LZ4Codec.MaximumOutputSize(encoderBlock);
			var arena = new byte[Math.Max(1, (long) n * slot)];
			var encoded = new int[Math.Max(1, n)];
			var source = content.ToArray();
			if (n > 0 && !chained)
			{
				// every block one message of k4lz4_encode_dictset_batch; then LZ4EncoderBase.Encode(allowCopy: true)'s rule
				var so = new ulong[n]; var sl = new int[n]; var to = new ulong[n]; var tl = new int[n]; var di = new int[n];
				for (var i = 0; i < n; i++)
				{
					so[i] = (ulong) ((long) i * encoderBlock); sl[i] = Math.Min(encoderBlock, source.Length - i * encoderBlock);
					to[i] = (ulong) ((long) i * slot); tl[i] = slot; di[i] = dictionaryIndex;
				}
				LZ4Codec.EncodeBatch(source, so, sl, arena, to, tl, encoded, dictionaries, di, settings.CompressionLevel);
				for (var i = 0; i < n; i++)
				{
					if (encoded[i] <= 0) throw new InvalidOperationException("Failed to encode chunk. Target buffer too small.");
					if (encoded[i] < sl[i]) continue;
					source.AsSpan((int) so[i], sl[i]).CopyTo(arena.AsSpan((int) to[i]));
					encoded[i] = -sl[i];
				}
			}
			else if (n > 0)
			{
				var extra = Math.Max(settings.ExtraMemory > 0 ? blockSize : 0, settings.ExtraMemory) / blockSize;
				using var lease = NativeContext.Rent();
				using var encoder = LZ4EncoderBatch.Create(
					lease.Handle, new[] { (true, settings.CompressionLevel, blockSize, extra) }, dictionaries, new[] { dictionaryIndex });
				var run = new ChainEncoderRecord[n];
				for (var i = 0; i < n; i++)
					run[i] = new ChainEncoderRecord(
						new ArraySegment<byte>(source, i * encoderBlock, Math.Min(encoderBlock, source.Length - i * encoderBlock)), true, true);
				var packed = new byte[encoder.Bound(0, run)];
				var written = encoder.Run(new[] { run }, new[] { packed }, out var results);
				if (written[0] < 0) throw new InvalidOperationException("Failed to encode chunk. Target buffer too small.");
				var at = 0;
				for (var i = 0; i < n; i++)
				{   // the blocks lie packed behind each other
					encoded[i] = results[0][i].Encoded;
					packed.AsSpan(at, Math.Abs(encoded[i])).CopyTo(arena.AsSpan(i * slot));
					at += Math.Abs(encoded[i]);
				}
			}
			return LZ4FrameBatch.Assemble(content, settings, bdCode, arena, slot, encoded, n, dictionaryIds[dictionaryIndex]);
		}

		/// <summary>Encode for every content; dictionaryIndex[i] is content i's entry (-1: a plain frame).</summary>
		public static byte[][] EncodeBatch(
			byte[][] contents, LZ4EncoderSettings settings, LZ4DictionarySet dictionaries, ReadOnlySpan<uint> dictionaryIds, int[] dictionaryIndex)
		{
			if (dictionaryIndex is null || dictionaryIndex.Length != contents.Length) throw new ArgumentException("one dictionary index per content");
			var frames = new byte[contents.Length][];
			for (var i = 0; i < contents.Length; i++) frames[i] = Encode(contents[i], settings, dictionaries, dictionaryIds, dictionaryIndex[i]);
			return frames;
		}

		/// <summary>Decodes one frame against the set; see DecodeBatch.</summary>
		public static byte[] Decode(ReadOnlySpan<byte> frame, LZ4DictionarySet dictionaries, ReadOnlySpan<uint> dictionaryIds) =>
			DecodeBatch(new[] { frame.ToArray() }, dictionaries, dictionaryIds, out _)[0];

		/// <summary>LZ4FrameBatch.DecodeBatch with dictionaries: entry e of the set answers to DictID dictionaryIds[e].
		/// dictionaryIndex[i]: the entry frame i resolved to, -1 for a frame without a DictID.  Throws for the lowest-index frame that
		/// fails, in the reader's defect order (an unknown DictID after the header checksum, before the first block).</summary>
		public static byte[][] DecodeBatch(byte[][] frames, LZ4DictionarySet dictionaries, ReadOnlySpan<uint> dictionaryIds, out int[] dictionaryIndex)
		{
			if (dictionaries is null) throw new ArgumentNullException(nameof(dictionaries));
			if (dictionaryIds.Length != dictionaries.Count) throw new ArgumentException("one id per entry of the set", nameof(dictionaryIds));
			var n = frames.Length;
			var frameOff = new ulong[n];
			var frameLen = new ulong[n];
			long total = 0;
			for (var i = 0; i < n; i++) { frameOff[i] = (ulong) total; frameLen[i] = (ulong) frames[i].Length; total += frames[i].Length; }
			var packed = new byte[Math.Max(total, 1)];
			for (var i = 0; i < n; i++) Buffer.BlockCopy(frames[i], 0, packed, (int) frameOff[i], frames[i].Length);
			var size = new ulong[n];
			var status = new int[n];
			var outLen = new long[n];
			dictionaryIndex = new int[n];
			var ids = dictionaryIds.Length == 0 ? new uint[1] : dictionaryIds.ToArray();
			using var lease = NativeContext.Rent();
			fixed (byte* src = packed)
			fixed (ulong* fo = frameOff, fl = frameLen, sz = size)
			fixed (int* st = status, di = dictionaryIndex)
			fixed (uint* id = ids)
				LLNative.ThrowIfFailed(
					LLNative.k4lz4_frame_sizes_dictset(lease.Handle, src, fo, fl, n, sz, st, di, dictionaries.Handle, id), lease.Handle);
			var dstOff = new ulong[n];
			ulong outTotal = 0;
			for (var i = 0; i < n; i++) { dstOff[i] = outTotal; outTotal += size[i]; }
			var dst = new byte[Math.Max(outTotal, 1UL)];
			fixed (byte* src = packed, d = dst)
			fixed (ulong* fo = frameOff, fl = frameLen, doff = dstOff, cap = size)
			fixed (long* ol = outLen)
			fixed (uint* id = ids)
				LLNative.ThrowIfFailed(
					LLNative.k4lz4_decode_frames_dictset(lease.Handle, src, fo, fl, n, d, doff, cap, ol, dictionaries.Handle, id), lease.Handle);
			GC.KeepAlive(dictionaries);
			var result = new byte[n][];
			for (var i = 0; i < n; i++)
			{
				if (outLen[i] < 0) throw LZ4FrameBatch.FrameError(outLen[i]);
				result[i] = dst.AsSpan((int) dstOff[i], (int) outLen[i]).ToArray();
			}
			return result;
		}
	}
}
