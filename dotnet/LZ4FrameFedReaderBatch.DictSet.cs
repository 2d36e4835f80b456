// Streams/Frames/LZ4FrameFedReaderBatch.DictSet.cs -- LZ4FrameFedReaderBatch against an LZ4DictionarySet:
// k4lz4_frame_read_fed_dictset_batch (include/k4lz4.h, DESIGN.md 4.25).  The rules are LZ4FrameReaderBatch.DictSet.cs's; a stream
// that is not final and ends inside the DictID starves there, Need[s] being the bytes that complete the header.  Without a set the
// class calls k4lz4_frame_read_fed_batch, unchanged.  The executable form is frames.py (LZ4FrameFedReaderBatch(dictionary=)).
// Compile-unverified.
using System;
using K4os.Compression.LZ4.Engine;

namespace K4os.Compression.LZ4.Engine
{
	internal static unsafe partial class LLNative
	{
		// dictIds: a HOST array of one uint per entry of the set in both forms
		[System.Runtime.InteropServices.DllImport(Lib)] public static extern int k4lz4_frame_read_fed_dictset_batch(
			IntPtr ctx, k4lz4_frame_reader* r, IntPtr store, ulong* storeOff, byte* src, ulong* srcOff, ulong* srcLen, long* final, byte* dst,
			ulong* dstOff, long* count, long* outLen, long* consumed, long* need, long n, int op, int flags, IntPtr set, uint* dictIds);
		[System.Runtime.InteropServices.DllImport(Lib)] public static extern int k4lz4_frame_read_fed_dictset_batch_device(
			IntPtr ctx, k4lz4_frame_reader* r, IntPtr store, IntPtr storeOff, IntPtr src, IntPtr srcOff, IntPtr srcLen, IntPtr final, IntPtr dst,
			IntPtr dstOff, IntPtr count, IntPtr outLen, IntPtr consumed, IntPtr need, long n, int op, int flags, long maxCount, IntPtr set,
			uint* dictIds, IntPtr stream);
	}
}

namespace K4os.Compression.LZ4.Streams.Frames
{
	public sealed unsafe partial class LZ4FrameFedReaderBatch
	{
		private LZ4DictionarySet _dictionaries;
		private uint[] _dictionaryIds = new uint[1];

		/// <summary>n fed readers whose frames may name dictionaries: entry e of the set answers to DictID dictionaryIds[e].</summary>
		public static LZ4FrameFedReaderBatch WithDictionaries(
			int n, LZ4DictionarySet dictionaries, ReadOnlySpan<uint> dictionaryIds, int maxBlockSize = 4 << 20)
		{
			if (dictionaries is null) throw new ArgumentNullException(nameof(dictionaries));
			return new LZ4FrameFedReaderBatch(n, maxBlockSize, dictionaries, dictionaryIds);
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
