// Engine/LLNative.cs -- P/Invoke table of libk4lz4.so (include/k4lz4.h).  Compile-unverified (no dotnet in the build image).
// Every entry mirrors one K4LZ4_API declaration; the per-block calls have the argument order and return values of the
// LLxx members they stand in for (Engine/LLxx.cs:17-26, :29-39, :41-55, :65-75, :94-103).
using System;
using System.IO;
using System.Runtime.InteropServices;

namespace K4os.Compression.LZ4.Engine
{
	internal static unsafe partial class LLNative      // (the other part: LZ4Frame.DictSet.cs)
	{
		private const string Lib = "k4lz4"; // libk4lz4.so on the probing path

		// k4lz4_status
		public const int OK = 0, E_HIP = -1, E_ARG = -2, E_NOMEM = -3, E_NO_DEVICE = -4, E_UNSUPPORTED = -5;

		// k4lz4_flags
		public const int FLAG_RAW_RETURN = 1, FLAG_PICKLE_WRITER = 2, FLAG_NO_REORDER = 4, FLAG_REORDER = 8, FLAG_NO_SPLIT = 16,
			FLAG_PARTIAL = 32, FLAG_ALLOW_COPY = 64, FLAG_X32 = 128, FLAG_SEGMENTS = 256;

		[DllImport(Lib)] public static extern int k4lz4_version();
		[DllImport(Lib)] public static extern int k4lz4_device_count();
		[DllImport(Lib)] public static extern long k4lz4_recommended_min_batch(int kind, int blockBytes, double hostGiBs);
		[DllImport(Lib)] public static extern int k4lz4_ctx_create(out IntPtr ctx, int device);
		[DllImport(Lib)] public static extern void k4lz4_ctx_destroy(IntPtr ctx);
		[DllImport(Lib)] public static extern IntPtr k4lz4_last_error(IntPtr ctx);
		[DllImport(Lib)] public static extern int k4lz4_ctx_device(IntPtr ctx);
		[DllImport(Lib)] public static extern int k4lz4_synchronize(IntPtr ctx, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_ctx_reserve_hc(IntPtr ctx, long totalSrcBytes, int longestBlock);
		[DllImport(Lib)] public static extern int k4lz4_host_register(IntPtr ptr, UIntPtr bytes);
		[DllImport(Lib)] public static extern int k4lz4_host_unregister(IntPtr ptr);
		[DllImport(Lib)] public static extern void k4lz4_set_enforce32(int on);
		[DllImport(Lib)] public static extern int k4lz4_get_enforce32();
		[DllImport(Lib)] public static extern int k4lz4_compress_bound(int n);
		[DllImport(Lib)] public static extern int k4lz4_last_status();

		// ---- the LLxx seam, one block per call
		[DllImport(Lib)] public static extern int k4lz4_compress_fast(byte* src, byte* dst, int srcLen, int dstCap, int acceleration);
		[DllImport(Lib)] public static extern int k4lz4_compress_hc(byte* src, byte* dst, int srcLen, int dstCap, int level);
		[DllImport(Lib)] public static extern int k4lz4_decompress_safe(byte* src, byte* dst, int srcLen, int dstCap);
		[DllImport(Lib)] public static extern int k4lz4_decompress_safe_partial(byte* src, byte* dst, int srcLen, int targetLen);
		[DllImport(Lib)] public static extern int k4lz4_decompress_safe_using_dict(
			byte* src, byte* dst, int srcLen, int dstCap, byte* dict, int dictLen);

		// ---- batches of independent blocks (host pointers)
		[DllImport(Lib)] public static extern int k4lz4_encode_batch(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int level, int flags);
		[DllImport(Lib)] public static extern int k4lz4_decode_batch(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int flags);
		[DllImport(Lib)] public static extern int k4lz4_decode_dict_batch(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int flags,
			byte* dict, ulong* dictOff, int* dictLen);
		// messages against shared dictionaries at L03_HC .. L09_HC (DESIGN.md 4.21); the fast levels' pair is in LZ4Codec.DictBatch.cs
		[DllImport(Lib)] public static extern int k4lz4_encode_dict_hc_batch(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int level, int flags,
			int* dictIdx, byte* dict, ulong* dictOff, int* dictLen, int nDict);
		[DllImport(Lib)] public static extern int k4lz4_encode_dict_hc_batch_device(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int level, int flags,
			int* dictIdx, byte* dict, ulong* dictOff, int* dictLen, int nDict, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_encode_dict_hc_state(IntPtr ctx, int d, uint* hashTable, ushort* chainTable, int* keptLen);

		// ---- LZ4Pickler envelope
		[DllImport(Lib)] public static extern int k4lz4_pickle_bound(int srcLen);
		[DllImport(Lib)] public static extern int k4lz4_unpickle_size(byte* pickle, int pickleLen);
		[DllImport(Lib)] public static extern int k4lz4_pickle_batch(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int level, int flags);
		[DllImport(Lib)] public static extern int k4lz4_unpickle_batch(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int flags);

		// ---- frame layer
		[DllImport(Lib)] public static extern int k4lz4_xxh32_batch(IntPtr ctx, byte* data, ulong* off, ulong* len, uint* digests, long n, uint seed);
		[DllImport(Lib)] public static extern int k4lz4_decode_chain_batch(
			IntPtr ctx, byte* src, ulong* blkOff, uint* blkLen, long nBlocks, ulong* firstBlk, uint* nBlk, int* blockSize, byte* chained,
			byte* dst, ulong* dstOff, ulong* dstCap, long* outLen, long nStreams);
		// frame reader (LZ4FrameReader over whole frames, DESIGN.md 4.11): outSize = the most frame f can decode to, outStatus /
		// outLen < 0 = the FRAME_* codes below.  The _device forms take device pointers; k4lz4_decode_frames_device waits for its
		// stream once (it reads the block count back).
		public const int FRAME_EOF = -1, FRAME_MAGIC = -2, FRAME_VERSION = -3, FRAME_HEADER_SUM = -4, FRAME_DICTIONARY = -5,
			FRAME_BLOCK = -6, FRAME_BLOCK_SUM = -7, FRAME_CONTENT_SUM = -8, FRAME_CAPACITY = -9, FRAME_LENGTH = -10;
		[DllImport(Lib)] public static extern int k4lz4_frame_sizes(
			IntPtr ctx, byte* src, ulong* frameOff, ulong* frameLen, long n, ulong* outSize, int* outStatus);
		[DllImport(Lib)] public static extern int k4lz4_decode_frames(
			IntPtr ctx, byte* src, ulong* frameOff, ulong* frameLen, long n, byte* dst, ulong* dstOff, ulong* dstCap, long* outLen);
		[DllImport(Lib)] public static extern int k4lz4_frame_sizes_device(
			IntPtr ctx, byte* src, ulong* frameOff, ulong* frameLen, long n, ulong* outSize, int* outStatus, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_decode_frames_device(
			IntPtr ctx, byte* src, ulong* frameOff, ulong* frameLen, long n, byte* dst, ulong* dstOff, ulong* dstCap, long* outLen,
			IntPtr stream);
		// legacy formats (K4os.Compression.LZ4.Legacy: LZ4Wrapper, LZ4Stream; DESIGN.md 4.12).  Per-item results < 0 are the
		// LEGACY_* codes: the exception the reference throws.  unwrap: decoded[i] = what LZ4Codec.Decode returned (Unwrap ignores it).
		public const int LEGACY_END_OF_STREAM = -1, LEGACY_OVERFLOW = -2, LEGACY_NOT_SUPPORTED = -3, LEGACY_INVALID_DATA = -4,
			LEGACY_ARGUMENT = -5, LEGACY_CAPACITY = -6, LEGACY_NOT_ENCODED = -7;
		[DllImport(Lib)] public static extern int k4lz4_wrap_bound(int srcLen);
		[DllImport(Lib)] public static extern int k4lz4_wrap_batch(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int high, int flags);
		[DllImport(Lib)] public static extern int k4lz4_wrap_batch_device(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, long n, int high, int flags,
			IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_unwrap_size(byte* buf, long len);
		[DllImport(Lib)] public static extern int k4lz4_unwrap_sizes_device(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, int* outLen, long n, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_unwrap_batch(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, int* decoded, long n);
		[DllImport(Lib)] public static extern int k4lz4_unwrap_batch_device(
			IntPtr ctx, byte* src, ulong* srcOff, int* srcLen, byte* dst, ulong* dstOff, int* dstCap, int* outLen, int* decoded, long n,
			IntPtr stream);
		[DllImport(Lib)] public static extern long k4lz4_legacy_stream_bound(long srcLen, int blockSize);
		[DllImport(Lib)] public static extern int k4lz4_encode_legacy_streams(
			IntPtr ctx, byte* src, ulong* srcOff, ulong* srcLen, long n, int blockSize, int high, int flags, byte* dst, ulong* dstOff,
			ulong* dstCap, long* outLen);
		[DllImport(Lib)] public static extern int k4lz4_encode_legacy_streams_device(
			IntPtr ctx, byte* src, ulong* srcOff, ulong* srcLen, long n, int blockSize, int high, int flags, byte* dst, ulong* dstOff,
			ulong* dstCap, long* outLen, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_legacy_stream_sizes(
			IntPtr ctx, byte* src, ulong* streamOff, ulong* streamLen, long n, ulong* outSize, int* outStatus);
		[DllImport(Lib)] public static extern int k4lz4_legacy_stream_sizes_device(
			IntPtr ctx, byte* src, ulong* streamOff, ulong* streamLen, long n, ulong* outSize, int* outStatus, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_decode_legacy_streams(
			IntPtr ctx, byte* src, ulong* streamOff, ulong* streamLen, long n, byte* dst, ulong* dstOff, ulong* dstCap, long* outLen);
		[DllImport(Lib)] public static extern int k4lz4_decode_legacy_streams_device(
			IntPtr ctx, byte* src, ulong* streamOff, ulong* streamLen, long n, byte* dst, ulong* dstOff, ulong* dstCap, long* outLen,
			IntPtr stream);
		// chained HC streams: LZ4HighChainEncoder(level, blockSize, extraBlocks) over whole contents, every block of every stream in
		// one launch sequence; dictLen (may be null): ring-buffer bytes in front of each content's first new block
		[DllImport(Lib)] public static extern int k4lz4_encode_hc_chain_batch(
			IntPtr ctx, byte* src, ulong* srcOff, long* srcLen, int* blockSize, int* extraBlocks, int* dictLen, long nStreams,
			byte* dst, ulong* dstOff, int* outLen, long nBlocks, int level, int flags);
		[DllImport(Lib)] public static extern int k4lz4_encode_hc_chain_batch_device(
			IntPtr ctx, IntPtr src, ulong* srcOff, long* srcLen, int* blockSize, int* extraBlocks, int* dictLen, long nStreams,
			IntPtr dst, ulong* dstOff, IntPtr outLen, long nBlocks, int level, int flags, IntPtr stream);

		// chained fast streams: LZ4FastChainEncoder(blockSize, extraBlocks) over whole contents, one wavefront per stream; stateIn /
		// stateOut (may be null): one k4lz4_fast_chain_state per stream (LZ4_stream_t's hashTable, currentOffset, dictSize) to continue
		// a stream across calls, with dictLen = stateIn.dictSize ring-buffer bytes in front of each content's first new block
		[StructLayout(LayoutKind.Sequential)]
		public struct k4lz4_fast_chain_state
		{
			public fixed uint hashTable[4096];
			public uint currentOffset;
			public uint dictSize;
			public fixed uint reserved[2];
		}
		[DllImport(Lib)] public static extern int k4lz4_encode_fast_chain_batch(
			IntPtr ctx, byte* src, ulong* srcOff, long* srcLen, int* blockSize, int* extraBlocks, int* dictLen, long nStreams,
			k4lz4_fast_chain_state* stateIn, k4lz4_fast_chain_state* stateOut, byte* dst, ulong* dstOff, int* outLen, long nBlocks, int flags);
		[DllImport(Lib)] public static extern int k4lz4_encode_fast_chain_batch_device(
			IntPtr ctx, IntPtr src, ulong* srcOff, long* srcLen, int* blockSize, int* extraBlocks, int* dictLen, long nStreams,
			IntPtr stateIn, IntPtr stateOut, IntPtr dst, ulong* dstOff, IntPtr outLen, long nBlocks, int flags, IntPtr stream);

		// incremental frame writer (DESIGN.md 4.13): many LZ4FrameWriters, one Write / OpenFrame / CloseFrame each per call; the records
		// in host memory, the stores (rings, XXH32 states, fast-chain states) in device memory
		[StructLayout(LayoutKind.Sequential)]
		public struct k4lz4_frame_writer_settings
		{
			public long contentLength;            // < 0: no content size in the header
			public int blockSize, level, chainBlocks, blockChecksum, contentChecksum, extraMemory;
		}
		[StructLayout(LayoutKind.Sequential)]
		public struct k4lz4_frame_writer
		{
			public k4lz4_frame_writer_settings settings;
			public int kind, encBlock, extraBlocks, ringBytes;
			public long written;
			public int index, pointer;
			public uint currentOffset, dictSize;
			public int phase, reserved;
		}
		public const int FWRITE_OP_WRITE = 0, FWRITE_OP_OPEN = 1, FWRITE_OP_CLOSE = 2;
		public const int FWRITE_TARGET = -1, FWRITE_CLOSED = -2, FWRITE_LENGTH = -3;
		[DllImport(Lib)] public static extern int k4lz4_frame_writer_init(k4lz4_frame_writer* w, k4lz4_frame_writer_settings* settings);
		[DllImport(Lib)] public static extern long k4lz4_frame_writer_store_bytes(k4lz4_frame_writer* w);
		[DllImport(Lib)] public static extern long k4lz4_frame_write_bound(k4lz4_frame_writer* w, long srcLen, int closing);
		[DllImport(Lib)] public static extern int k4lz4_frame_write_batch(
			IntPtr ctx, k4lz4_frame_writer* w, IntPtr store, ulong* storeOff, byte* src, ulong* srcOff, long* srcLen, byte* dst, ulong* dstOff,
			ulong* dstCap, long* outLen, long n, int op, int flags);
		[DllImport(Lib)] public static extern int k4lz4_frame_write_batch_device(
			IntPtr ctx, k4lz4_frame_writer* w, IntPtr store, ulong* storeOff, IntPtr src, ulong* srcOff, long* srcLen, IntPtr dst, ulong* dstOff,
			ulong* dstCap, IntPtr outLen, long n, int op, int flags, IntPtr stream);

		// incremental frame reader (DESIGN.md 4.14): many LZ4FrameReaders, one ReadManyBytes / OpenFrame each per call; the record holds
		// the settings and the per-stream store size, everything a reader keeps between calls is in the device store
		[StructLayout(LayoutKind.Sequential)]
		public struct k4lz4_frame_reader_settings { public int maxBlockSize, flags; }
		[StructLayout(LayoutKind.Sequential)]
		public struct k4lz4_frame_reader { public k4lz4_frame_reader_settings settings; public long storeBytes; }
		public const int FREAD_OP_READ = 0, FREAD_OP_OPEN = 1, FREAD_OP_RESET = 2, FREAD_INTERACTIVE = 1;
		public const int FRAME_BLOCK_SIZE = -11, FRQ_BYTES_READ = 0, FRQ_FRAME_LENGTH = 1, FRQ_PHASE = 2, FRQ_CODE = 3, FRQ_BLOCKS = 4, FRQ_DIRECT = 5, FRQ_FAST = 6, FRQ_HANDED_BACK = 7, FRQ_WORDS = 8;
		[DllImport(Lib)] public static extern int k4lz4_frame_reader_init(k4lz4_frame_reader* r, k4lz4_frame_reader_settings* settings);
		[DllImport(Lib)] public static extern long k4lz4_frame_reader_store_bytes(k4lz4_frame_reader* r);
		[DllImport(Lib)] public static extern int k4lz4_frame_read_batch(
			IntPtr ctx, k4lz4_frame_reader* r, IntPtr store, ulong* storeOff, byte* src, ulong* srcOff, ulong* srcLen, byte* dst, ulong* dstOff,
			long* count, long* outLen, long n, int op, int flags);
		[DllImport(Lib)] public static extern int k4lz4_frame_read_batch_device(
			IntPtr ctx, k4lz4_frame_reader* r, IntPtr store, IntPtr storeOff, IntPtr src, IntPtr srcOff, IntPtr srcLen, IntPtr dst, IntPtr dstOff,
			IntPtr count, IntPtr outLen, long n, int op, int flags, long maxCount, IntPtr stream);
		[DllImport(Lib)] public static extern long k4lz4_frame_read_table_rows(long maxCount);
		// the same readers fed their sources in pieces (DESIGN.md 4.15): a record made with FREADER_FED, per call the unconsumed part of
		// each source and whether it is final; consumed and need come back beside outLen
		public const int FREADER_FED = 1;
		[DllImport(Lib)] public static extern int k4lz4_frame_read_fed_batch(
			IntPtr ctx, k4lz4_frame_reader* r, IntPtr store, ulong* storeOff, byte* src, ulong* srcOff, ulong* srcLen, long* final, byte* dst,
			ulong* dstOff, long* count, long* outLen, long* consumed, long* need, long n, int op, int flags);
		[DllImport(Lib)] public static extern int k4lz4_frame_read_fed_batch_device(
			IntPtr ctx, k4lz4_frame_reader* r, IntPtr store, IntPtr storeOff, IntPtr src, IntPtr srcOff, IntPtr srcLen, IntPtr final, IntPtr dst,
			IntPtr dstOff, IntPtr count, IntPtr outLen, IntPtr consumed, IntPtr need, long n, int op, int flags, long maxCount, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_frame_reader_query(IntPtr ctx, IntPtr store, ulong* storeOff, long n, long* @out);
		[DllImport(Lib)] public static extern int k4lz4_frame_reader_query_device(IntPtr ctx, IntPtr store, IntPtr storeOff, long n, IntPtr @out, IntPtr stream);

		// ---- device-resident variants: every pointer is a device pointer of the context's GPU, stream = hipStream_t
		[DllImport(Lib)] public static extern int k4lz4_encode_batch_device(
			IntPtr ctx, IntPtr src, IntPtr srcOff, IntPtr srcLen, IntPtr dst, IntPtr dstOff, IntPtr dstCap, IntPtr outLen, long n, int level, int flags, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_decode_batch_device(
			IntPtr ctx, IntPtr src, IntPtr srcOff, IntPtr srcLen, IntPtr dst, IntPtr dstOff, IntPtr dstCap, IntPtr outLen, long n, int flags, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_pickle_batch_device(
			IntPtr ctx, IntPtr src, IntPtr srcOff, IntPtr srcLen, IntPtr dst, IntPtr dstOff, IntPtr dstCap, IntPtr outLen, long n, int level, int flags, IntPtr stream);
		[DllImport(Lib)] public static extern int k4lz4_unpickle_batch_device(
			IntPtr ctx, IntPtr src, IntPtr srcOff, IntPtr srcLen, IntPtr dst, IntPtr dstOff, IntPtr dstCap, IntPtr outLen, long n, int flags, IntPtr stream);

		/// <summary>Call-level status -> the exception type the managed code base uses for the same situation.</summary>
		internal static void ThrowIfFailed(int status, IntPtr ctx)
		{
			if (status == OK) return;
			var msg = Marshal.PtrToStringAnsi(k4lz4_last_error(ctx)) ?? "libk4lz4 call failed";
			switch (status)
			{
				case E_ARG: throw new ArgumentException(msg); // Internal/Extensions.cs:37-52 semantics
				case E_NOMEM: throw new OutOfMemoryException(msg);
				case E_UNSUPPORTED: throw new NotImplementedException(msg);
				case E_NO_DEVICE: throw new PlatformNotSupportedException(msg); // never a silent fall back to LL64
				default: throw new InvalidOperationException(msg); // E_HIP, incl. "decoder wave pair timed out"
			}
		}

		/// <summary>After an LLxx-shaped call, whose int return cannot carry an infrastructure failure.</summary>
		internal static int Checked(int result)
		{
			ThrowIfFailed(k4lz4_last_status(), IntPtr.Zero);
			return result; // LLxx-level value: bytes, 0 = did not fit, decode error = -(pos) - 1
		}
	}
}
