// Streams/Frames/LZ4FrameReaderBatch.DictSet.cs -- LZ4FrameReaderBatch against an LZ4DictionarySet: k4lz4_frame_read_dictset_batch
// (include/k4lz4.h, DESIGN.md 4.25).  Frames with a predefined dictionary (FLG bit 0, DictID) are read a piece at a time: a frame's
// DictID resolves to the first entry whose id equals it, a frame without the bit is read as ever, and a DictID that nothing answers
// to is the code every DictID has without a set (-5, NotImplementedException), reported by Open too.  The set and the ids stay the
// same for as long as a frame is open; the kept bytes are never delivered and never counted.  Without a set the class calls
// k4lz4_frame_read_batch, unchanged.  The executable form is frames.py (LZ4FrameReaderBatch(dictionary=)).  Compile-unverified.
using System;
using K4os.Compression.LZ4.Engine;

namespace K4os.Compression.LZ4.Engine
{
	internal static unsafe partial class LLNative
	{
		// dictIds: a HOST array of one uint per entry of the set in both forms
		[System.Runtime.InteropServices.DllImport(Lib)] public static extern int k4lz4_frame_read_dictset_batch(
			IntPtr ctx, k4lz4_frame_reader* r, IntPtr store, ulong* storeOff, byte* src, ulong* srcOff, ulong* srcLen, byte* dst, ulong* dstOff,
			long* count, long* outLen, long n, int op, int flags, IntPtr set, uint* dictIds);
		[System.Runtime.InteropServices.DllImport(Lib)] public static extern int k4lz4_frame_read_dictset_batch_device(
			IntPtr ctx, k4lz4_frame_reader* r, IntPtr store, IntPtr storeOff, IntPtr src, IntPtr srcOff, IntPtr srcLen, IntPtr dst, IntPtr dstOff,
			IntPtr count, IntPtr outLen, long n, int op, int flags, long maxCount, IntPtr set, uint* dictIds, IntPtr stream);
	}
}

namespace K4os.Compression.LZ4.Streams.Frames
{
	public sealed unsafe partial class LZ4FrameReaderBatch
	{
		private LZ4DictionarySet _dictionaries;
		private uint[] _dictionaryIds = new uint[1];

		/// <summary>Readers over sources whose frames may name dictionaries: entry e of the set answers to DictID dictionaryIds[e].</summary>
		public static LZ4FrameReaderBatch WithDictionaries(
			byte[][] sources, LZ4DictionarySet dictionaries, ReadOnlySpan<uint> dictionaryIds, int maxBlockSize = 4 << 20)
		{
			if (dictionaries is null) throw new ArgumentNullException(nameof(dictionaries));
			return new LZ4FrameReaderBatch(sources, maxBlockSize, dictionaries, dictionaryIds);
		}

		private void SetDictionaries(LZ4DictionarySet dictionaries, ReadOnlySpan<uint> dictionaryIds)
		{
			if (dictionaries is null) return;
			if (dictionaryIds.Length != dictionaries.Count) throw new ArgumentException("one id per entry of the set", nameof(dictionaryIds));
			_dictionaries = dictionaries;
			if (dictionaryIds.Length > 0) _dictionaryIds = dictionaryIds.ToArray();
		}
	}
}
