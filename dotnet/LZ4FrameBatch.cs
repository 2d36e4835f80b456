// Streams/Frames/LZ4FrameBatch.cs -- whole-buffer frames through the batch calls: what LZ4FrameWriter / LZ4FrameReader do one
// block at a time (Frames/LZ4FrameWriter.async.cs:15-90: length word with raw bit, payload, optional block checksum, EndMark,
// optional content checksum; Frames/LZ4FrameReader.async.cs:108-136), done for all blocks of a frame -- or of many frames -- with
// one encode / decode launch and one XXH32 launch.  Chained frames (ChainBlocks = true, the reference's default) at L03_HC and up
// are LZ4HighChainEncoder's blocks, from k4lz4_encode_hc_chain_batch: a chained HC block needs the bytes before it, not the parse
// of the block before it (DESIGN.md).  Chained L00_FAST frames stay with LZ4FrameWriter (LZ4FastChainEncoder's table depends on
// its parse: serial per stream).  The reader side (Decode / DecodeBatch) is k4lz4_frame_sizes + k4lz4_decode_frames: the frames are
// walked, checked and decoded on the device, both kinds.
// Byte layout and header arithmetic are LZ4FrameWriter.cs:57-108,:159-189.  Compile-unverified.
using System;
using System.Buffers.Binary;
using K4os.Compression.LZ4.Encoders;
using K4os.Compression.LZ4.Engine;

namespace K4os.Compression.LZ4.Streams.Frames
{
	public static unsafe class LZ4FrameBatch
	{
		private const uint Magic = 0x184D2204;

		/// <summary>One LZ4 frame (independent blocks) around content, byte-identical to what LZ4FrameWriter writes for the same
		/// settings when its input arrives in one piece.</summary>
		/// <summary>LZ4HighChainEncoder(level, blockSize, extraBlocks) over the whole content (Streams/Extensions.cs:18-36), one native
		/// call: block i to arena[i * slot], encoded[i] as LZ4EncoderBase.Encode(allowCopy: true) returns it.</summary>
		private static void EncodeChained(ReadOnlySpan<byte> content, LZ4EncoderSettings settings, int blockSize, byte[] arena, int[] encoded, int n)
		{
			if (n == 0) return;
			var extra = Math.Max(settings.ExtraMemory > 0 ? blockSize : 0, settings.ExtraMemory) / blockSize;
			ulong srcOff = 0, dstOff = 0;
			long srcLen = content.Length;
			using var lease = NativeContext.Rent();
			fixed (byte* src = content)
			fixed (byte* dst = arena)
			fixed (int* outLen = encoded)
				LLNative.ThrowIfFailed(LLNative.k4lz4_encode_hc_chain_batch(lease.Handle, src, &srcOff, &srcLen, &blockSize, &extra, null, 1,
					dst, &dstOff, outLen, n, (int) settings.CompressionLevel, LLNative.FLAG_ALLOW_COPY), lease.Handle);
		}

		/// <summary>LZ4FastChainEncoder's blocks of one content (the frame writer's ChainBlocks at levels below L03_HC):
		/// block j in arena[j * slot ..], encoded[j] its length (negative: stored raw).  Encode below still refuses chained
		/// L00_FAST frames; this is the block half of such a frame.</summary>
		public static void EncodeFastChained(ReadOnlySpan<byte> content, LZ4EncoderSettings settings, int blockSize, byte[] arena, int[] encoded, int n)
		{
			if (n == 0) return;
			var extra = Math.Max(settings.ExtraMemory > 0 ? blockSize : 0, settings.ExtraMemory) / blockSize;
			ulong srcOff = 0, dstOff = 0;
			long srcLen = content.Length;
			using var lease = NativeContext.Rent();
			fixed (byte* src = content)
			fixed (byte* dst = arena)
			fixed (int* outLen = encoded)
				LLNative.ThrowIfFailed(LLNative.k4lz4_encode_fast_chain_batch(lease.Handle, src, &srcOff, &srcLen, &blockSize, &extra, null, 1,
					null, null, dst, &dstOff, outLen, n, LLNative.FLAG_ALLOW_COPY), lease.Handle);
		}

		public static byte[] Encode(ReadOnlySpan<byte> content, LZ4EncoderSettings settings)
		{
			var chained = settings.ChainBlocks;
			if (chained && settings.CompressionLevel < LZ4Level.L03_HC)
				throw new NotSupportedException("chained L00_FAST blocks depend on each other's parse: use LZ4FrameWriter");
			var blockSize = MaxBlockSize(settings.BlockSize, out var bdCode);
			// the chained encoder's blocks are its ring buffer's: the block size rounded up to a whole KiB (LZ4EncoderBase.cs:23)
			var encoderBlock = chained ? (Math.Max(blockSize, 1024) + 1023) / 1024 * 1024 : blockSize;
			var n = (int) (((long) content.Length + encoderBlock - 1) / encoderBlock);
			var slot = LZ4Codec.MaximumOutputSize(encoderBlock);
			var arena = new byte[Math.Max(1, (long) n * slot)];
			var encoded = new int[Math.Max(1, n)];
			if (chained)
				EncodeChained(content, settings, blockSize, arena, encoded, n);
			else
				using (var encoder = new LZ4BlockEncoder(settings.CompressionLevel, blockSize))
					encoder.EncodeBlocks(content, arena, encoded, allowCopy: true);
			return Assemble(content, settings, bdCode, arena, slot, encoded, n, null);
		}

		/// <summary>The frame around n encoded blocks (block i in arena[i * slot ..], encoded[i] negative: stored raw): header, records
		/// with their checksums, EndMark, content checksum.  dictId: the DictID the header names (FLG bit 0, after the content size) --
		/// only LZ4FrameDictSet passes one.</summary>
		internal static byte[] Assemble(
			ReadOnlySpan<byte> content, LZ4EncoderSettings settings, int bdCode, byte[] arena, int slot, int[] encoded, int n, uint? dictId)
		{
			var chained = settings.ChainBlocks;
			// sizes: header 7 (+8 content length, +4 DictID), per block 4 + stored (+4), EndMark 4 (+4)
			long total = 7 + (settings.ContentLength.HasValue ? 8 : 0) + (dictId.HasValue ? 4 : 0) + 4 + (settings.ContentChecksum ? 4 : 0);
			for (var i = 0; i < n; i++) total += 4 + Math.Abs(encoded[i]) + (settings.BlockChecksum ? 4 : 0);
			var frame = new byte[total];
			var at = 0;
			BinaryPrimitives.WriteUInt32LittleEndian(frame.AsSpan(at), Magic); at += 4;
			var headerStart = at;
			frame[at++] = (byte) ((1 << 6) | (chained ? 0 : 1 << 5) /* FLG bit 5: independent blocks */ | (settings.BlockChecksum ? 1 << 4 : 0) |
				(settings.ContentLength.HasValue ? 1 << 3 : 0) | (settings.ContentChecksum ? 1 << 2 : 0) | (dictId.HasValue ? 1 : 0));
			frame[at++] = (byte) (bdCode << 4);
			if (settings.ContentLength.HasValue) { BinaryPrimitives.WriteUInt64LittleEndian(frame.AsSpan(at), (ulong) settings.ContentLength.Value); at += 8; }
			if (dictId.HasValue) { BinaryPrimitives.WriteUInt32LittleEndian(frame.AsSpan(at), dictId.Value); at += 4; }
			frame[at] = (byte) (Digest(frame.AsSpan(headerStart, at - headerStart)) >> 8); at++;          // LZ4FrameWriter.cs:100

			// payloads first, then every block checksum of the frame in one XXH32 launch
			var payloadAt = new ulong[n]; var payloadLen = new ulong[n];
			for (var i = 0; i < n; i++)
			{
				var stored = Math.Abs(encoded[i]);
				BinaryPrimitives.WriteUInt32LittleEndian(frame.AsSpan(at), (uint) stored | (encoded[i] < 0 ? 0x80000000u : 0u)); at += 4;   // :159-160
				arena.AsSpan(i * slot, stored).CopyTo(frame.AsSpan(at));
				payloadAt[i] = (ulong) at; payloadLen[i] = (ulong) stored; at += stored;
				if (settings.BlockChecksum) at += 4;
			}
			if (settings.BlockChecksum && n > 0)
			{
				var digests = Digests(frame, payloadAt, payloadLen);
				for (var i = 0; i < n; i++) BinaryPrimitives.WriteUInt32LittleEndian(frame.AsSpan((int) (payloadAt[i] + payloadLen[i])), digests[i]);
			}
			BinaryPrimitives.WriteUInt32LittleEndian(frame.AsSpan(at), 0); at += 4;                          // EndMark
			if (settings.ContentChecksum) { BinaryPrimitives.WriteUInt32LittleEndian(frame.AsSpan(at), Digest(content)); at += 4; }
			return frame;
		}

		/// <summary>Decodes one frame (independent or chained blocks) into a fresh array, throwing what LZ4FrameReader throws for the
		/// first defect it meets in stream order (bad magic / version / header checksum, dictionary, end of stream, a block checksum,
		/// a block that does not decode, the content checksum, ContentLength).  Bytes after the frame are ignored.</summary>
		public static byte[] Decode(ReadOnlySpan<byte> frame) => DecodeBatch(new[] { frame.ToArray() })[0];

		/// <summary>Decodes whole frames, one per element, with two native calls (k4lz4_frame_sizes sizes the output without trusting
		/// the headers, k4lz4_decode_frames walks, checks and decodes every frame on the device); throws for the lowest-index frame
		/// that fails.</summary>
		public static byte[][] DecodeBatch(byte[][] frames)
		{
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
			using var lease = NativeContext.Rent();
			fixed (byte* src = packed)
			fixed (ulong* fo = frameOff)
			fixed (ulong* fl = frameLen)
			fixed (ulong* sz = size)
			fixed (int* st = status)
				LLNative.ThrowIfFailed(LLNative.k4lz4_frame_sizes(lease.Handle, src, fo, fl, n, sz, st), lease.Handle);
			var dstOff = new ulong[n];
			ulong outTotal = 0;
			for (var i = 0; i < n; i++) { dstOff[i] = outTotal; outTotal += size[i]; }
			var dst = new byte[Math.Max(outTotal, 1UL)];
			fixed (byte* src = packed)
			fixed (ulong* fo = frameOff)
			fixed (ulong* fl = frameLen)
			fixed (byte* d = dst)
			fixed (ulong* doff = dstOff)
			fixed (ulong* cap = size)
			fixed (long* ol = outLen)
				LLNative.ThrowIfFailed(LLNative.k4lz4_decode_frames(lease.Handle, src, fo, fl, n, d, doff, cap, ol), lease.Handle);
			var result = new byte[n][];
			for (var i = 0; i < n; i++)
			{
				if (outLen[i] < 0) throw FrameError(outLen[i]);
				result[i] = dst.AsSpan((int) dstOff[i], (int) outLen[i]).ToArray();
			}
			return result;
		}

		/// <summary>The reference reader's exception for a K4LZ4_FRAME_* code (Frames/LZ4FrameReader.blocking.cs ReadHeader / ReadBlock,
		/// Internal/Stash: EndOfStream).</summary>
		internal static Exception FrameError(long code) => code switch {
			LLNative.FRAME_EOF => new System.IO.EndOfStreamException("Unexpected end of stream"),
			LLNative.FRAME_MAGIC => new System.IO.InvalidDataException("LZ4 frame magic number expected"),
			LLNative.FRAME_VERSION => new System.IO.InvalidDataException("LZ4 frame version unknown: 0"),
			LLNative.FRAME_HEADER_SUM => new System.IO.InvalidDataException("Invalid LZ4 frame header checksum"),
			LLNative.FRAME_DICTIONARY => new NotImplementedException("Predefined dictionaries feature is not implemented"),
			LLNative.FRAME_BLOCK => new System.IO.InvalidDataException("LZ4 block does not decode"),
			LLNative.FRAME_BLOCK_SUM => new System.IO.InvalidDataException("Invalid block checksum"),
			LLNative.FRAME_CONTENT_SUM => new System.IO.InvalidDataException("Invalid content checksum"),
			LLNative.FRAME_CAPACITY => new System.IO.InvalidDataException("Decoded frame does not fit its target"),
			LLNative.FRAME_LENGTH => new System.IO.InvalidDataException("Content length does not match the frame header"),
			_ => new InvalidOperationException($"unknown frame result {code}"),
		};

		internal static int MaxBlockSize(int requested, out int bdCode)
		{   // LZ4FrameWriter.cs:176-189
			if (requested <= 1 << 16) { bdCode = 4; return 1 << 16; }
			if (requested <= 1 << 18) { bdCode = 5; return 1 << 18; }
			if (requested <= 1 << 20) { bdCode = 6; return 1 << 20; }
			bdCode = 7; return 1 << 22;
		}

		private static uint Digest(ReadOnlySpan<byte> bytes)
		{
			var off = new ulong[] { 0 }; var len = new ulong[] { (ulong) bytes.Length };
			var pad = bytes.Length == 0 ? new byte[1] : bytes.ToArray();
			return Digests(pad, off, len)[0];
		}

		private static uint[] Digests(byte[] data, ulong[] off, ulong[] len)
		{
			var digests = new uint[off.Length];
			using var lease = NativeContext.Rent();
			fixed (byte* d = data)
			fixed (ulong* o = off, l = len)
			fixed (uint* r = digests)
				LLNative.ThrowIfFailed(LLNative.k4lz4_xxh32_batch(lease.Handle, d, o, l, r, off.Length, 0), lease.Handle);
			return digests;
		}
	}
}
