// K4os.Compression.LZ4/Encoders/LZ4Encoder.DictSet.cs -- chained encoders and decoders opened from an LZ4DictionarySet
// (k4lz4_chain_encoder_open_dictset / k4lz4_chain_decoder_open_dictset, include/k4lz4.h, DESIGN.md 4.23).  "Open" makes fresh streams,
// as Reset does, and primes those that name an entry of the set: an encoder starts with the entry's last 64 KiB as its prefix
// (LL.LZ4_loadDict / LL.LZ4_loadDictHC on its ring buffer, the first block right behind it), a decoder as one that was given
// Inject(those bytes).  The bytes never leave the device.  Both batch classes become `partial`; the two Create overloads make the
// streams and open them in one step.  Not for independent encoders, not at L10_OPT and up, a chained fast encoder needs a set with
// LZ4DictionaryFamilies.Fast and is not offered under LZ4Codec.Enforce32.  Compile-unverified.
using System;
using System.Runtime.InteropServices;

namespace K4os.Compression.LZ4.Encoders
{
	internal static unsafe class ChainOpenNative
	{
		private const string Lib = "k4lz4";

		public const int DICT_INDEX = -8;   // K4LZ4_CDEC_DICT_INDEX (the _device decoder form only)

		[DllImport(Lib)] public static extern int k4lz4_chain_encoder_open_plan(ChainEncoderNative.Record* e, int dictLen);
		[DllImport(Lib)] public static extern int k4lz4_chain_encoder_open_dictset(
			IntPtr ctx, ChainEncoderNative.Record* enc, byte* store, ulong* storeOff, int* dictIdx, IntPtr set, long n);
		[DllImport(Lib)] public static extern int k4lz4_chain_encoder_open_dictset_device(
			IntPtr ctx, ChainEncoderNative.Record* enc, byte* store, ulong* storeOff, int* dictIdx, IntPtr set, long n, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_chain_decoder_open_dictset(
			IntPtr ctx, ChainDecoderNative.Record* dec, byte* store, ulong* storeOff, int* dictIdx, IntPtr set, long* outLen, long n);
		[DllImport(Lib)] public static extern int k4lz4_chain_decoder_open_dictset_device(
			IntPtr ctx, ChainDecoderNative.Record* dec, byte* store, ulong* storeOff, int* dictIdx, IntPtr set, long* outLen, long n,
			IntPtr stream);
	}

	public sealed unsafe partial class LZ4EncoderBatch
	{
		/// <summary>LZ4Encoder.Create(chaining, level, blockSize, extraBlocks) per entry of settings, encoder s starting from entry
		/// dictionaryIndex[s] of the set (-1: no dictionary).</summary>
		public static LZ4EncoderBatch Create(
			IntPtr ctx, (bool chaining, LZ4Level level, int blockSize, int extraBlocks)[] settings, LZ4DictionarySet dictionaries,
			int[] dictionaryIndex)
		{
			var batch = new LZ4EncoderBatch(ctx, settings);
			try { batch.Open(dictionaries, dictionaryIndex); }
			catch { batch.Dispose(); throw; }
			return batch;
		}

		/// <summary>Every encoder becomes a fresh one; encoder s with dictionaryIndex[s] >= 0 starts with that entry's kept bytes in
		/// front of its first block.  Refused as a whole (ArgumentException, nothing changes): an index outside the set, an index on
		/// an independent encoder or at L10_OPT and up, a chained fast encoder and a set without the fast family.</summary>
		public void Open(LZ4DictionarySet dictionaries, int[] dictionaryIndex)
		{
			if (dictionaries is null) throw new ArgumentNullException(nameof(dictionaries));
			if (dictionaryIndex is null || dictionaryIndex.Length != _records.Length) throw new ArgumentException("one dictionary index per encoder");
			fixed (ChainEncoderNative.Record* r = _records)
			fixed (ulong* so = _storeOff)
			fixed (int* di = dictionaryIndex)
			{
				var rc = ChainOpenNative.k4lz4_chain_encoder_open_dictset(_ctx, r, _store, so, di, dictionaries.Handle, _records.Length);
				if (rc == -2) throw new ArgumentException("k4lz4_chain_encoder_open_dictset refused the call");
				Check(rc);
			}
			GC.KeepAlive(dictionaries);
		}
	}

	public sealed unsafe partial class LZ4ChainDecoderBatch
	{
		/// <summary>LZ4Decoder.Create(chaining, blockSize, extraBlocks) per entry of settings, decoder s being the one after
		/// Inject(the kept bytes of entry dictionaryIndex[s]) (-1: no dictionary).</summary>
		public static LZ4ChainDecoderBatch Create(
			IntPtr ctx, (bool chaining, int blockSize, int extraBlocks)[] settings, LZ4DictionarySet dictionaries, int[] dictionaryIndex)
		{
			var batch = new LZ4ChainDecoderBatch(ctx, settings);
			try
			{
				var injected = batch.Open(dictionaries, dictionaryIndex);
				for (var s = 0; s < injected.Length; s++)
					if (injected[s] < 0) throw new InvalidOperationException($"decoder {s}: the dictionary does not fit (code {injected[s]})");
			}
			catch { batch.Dispose(); throw; }
			return batch;
		}

		/// <summary>Every store becomes a fresh decoder; decoder s with dictionaryIndex[s] >= 0 is then given that entry's kept bytes
		/// as Inject gives them.  Per decoder: the bytes injected, or INJECT_THREW (-2) for an independent decoder whose buffer is
		/// shorter than the entry.</summary>
		public long[] Open(LZ4DictionarySet dictionaries, int[] dictionaryIndex)
		{
			if (dictionaries is null) throw new ArgumentNullException(nameof(dictionaries));
			if (dictionaryIndex is null || dictionaryIndex.Length != _records.Length) throw new ArgumentException("one dictionary index per decoder");
			var injected = new long[_records.Length];
			fixed (ChainDecoderNative.Record* r = _records)
			fixed (ulong* so = _storeOff)
			fixed (int* di = dictionaryIndex)
			fixed (long* ol = injected)
			{
				var rc = ChainOpenNative.k4lz4_chain_decoder_open_dictset(_ctx, r, _store, so, di, dictionaries.Handle, ol, _records.Length);
				if (rc == -2) throw new ArgumentException("k4lz4_chain_decoder_open_dictset refused the call");
				Check(rc);
			}
			GC.KeepAlive(dictionaries);
			return injected;
		}
	}
}
