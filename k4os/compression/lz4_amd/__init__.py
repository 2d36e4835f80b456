"""k4os.compression.lz4_amd -- MI355X (gfx950) LZ4 block codec behind the K4os.Compression.LZ4
block API: LZ4Codec.Encode / Decode, LZ4Pickler.Pickle / Unpickle and their batch forms.
All compute runs in hand-written HIP kernels (csrc/) reached through the C ABI of libk4lz4.so
(include/k4lz4.h).  There is no CPU fallback."""
from .codec import LZ4Codec, LZ4Level, pack_blocks, make_arena, encode_dict_packed, encode_dict_device, encode_dictset_device, DictionarySet, DICT_FAST, DICT_HC
from .pickler import LZ4Pickler, InvalidDataException
from .encoders import (LZ4BlockEncoder, LZ4HighChainEncoder, LZ4FastChainEncoder, LZ4BlockDecoder, EncoderAction, InvalidOperationException, TopupAndEncode,
                       FlushAndEncode, DecodeAndDrain, encode_fast_chain_packed, encode_fast_chain_device, fast_chain_blocks,
                       FAST_CHAIN_STATE, LZ4ChainDecoder, LZ4Decoder, LZ4ChainDecoderBatch, LZ4EncoderBatch, LZ4ChainEncoder, LZ4Encoder)
from .frames import (LZ4Frame, LZ4EncoderSettings, LZ4Descriptor, parse_frame, xxh32_many, encode_fast_chain_frames,
                     frame_sizes_device, decode_frames_device, frame_exception, LZ4FrameWriterBatch, FrameWriterDevice,
                     LZ4FrameReaderBatch, FrameReaderDevice, LZ4FrameFedReaderBatch, FrameFedReaderDevice)
from .legacy import (LZ4Legacy, EndOfStreamException, OverflowException, NotSupportedException, ArgumentException, legacy_exception,
                     wrap_device, unwrap_device, encode_legacy_streams_device, legacy_stream_sizes_device, decode_legacy_streams_device,
                     LZ4StreamWriterBatch, LegacyWriterDevice, LZ4StreamReaderBatch, LegacyReaderDevice,
                     LZ4StreamFedReaderBatch, LegacyFedReaderDevice)
from ._native import NativeLibraryError, Context, load_library, default_context, host_register, host_unregister

__all__ = ["LZ4Codec", "LZ4Level", "LZ4Pickler", "InvalidDataException", "NativeLibraryError", "Context",
           "load_library", "default_context", "host_register", "host_unregister", "pack_blocks", "make_arena", "LZ4BlockEncoder", "LZ4HighChainEncoder", "LZ4FastChainEncoder", "LZ4BlockDecoder",
           "EncoderAction", "InvalidOperationException", "TopupAndEncode", "FlushAndEncode", "DecodeAndDrain", "LZ4Frame",
           "LZ4EncoderSettings", "LZ4Descriptor", "parse_frame", "xxh32_many", "encode_fast_chain_packed", "encode_fast_chain_device",
           "fast_chain_blocks", "FAST_CHAIN_STATE", "encode_fast_chain_frames",
           "frame_sizes_device", "decode_frames_device", "frame_exception", "LZ4FrameWriterBatch", "FrameWriterDevice", "LZ4FrameReaderBatch", "FrameReaderDevice",
           "LZ4FrameFedReaderBatch", "FrameFedReaderDevice",
           "LZ4Legacy", "EndOfStreamException", "OverflowException", "NotSupportedException", "ArgumentException", "legacy_exception",
           "wrap_device", "unwrap_device", "encode_legacy_streams_device", "legacy_stream_sizes_device", "decode_legacy_streams_device",
           "LZ4StreamWriterBatch", "LegacyWriterDevice", "LZ4StreamReaderBatch", "LegacyReaderDevice",
           "LZ4StreamFedReaderBatch", "LegacyFedReaderDevice", "LZ4ChainDecoder", "LZ4Decoder", "LZ4ChainDecoderBatch",
           "LZ4EncoderBatch", "LZ4ChainEncoder", "LZ4Encoder", "encode_dict_packed", "encode_dict_device", "encode_dictset_device", "DictionarySet",
           "DICT_FAST", "DICT_HC"]
