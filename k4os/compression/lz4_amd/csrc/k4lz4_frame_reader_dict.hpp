/*
 * k4lz4_frame_reader_dict.hpp -- the incremental frame readers against a k4lz4_dict_set (k4lz4_frame_read_dictset_batch,
 * k4lz4_frame_read_fed_dictset_batch): frames with a predefined dictionary (FLG bit 0, DictID) read a piece at a
 * time.  The loops are the readers' own -- the wave loops are one text (k4lz4_frame_reader_loop.hpp, k4lz4_frame_feed_loop.hpp),
 * plan and commit one body each (fr_plan_body / fr_commit_body and the fed pair in k4lz4_frame_reader.hpp and k4lz4_frame_feed.hpp,
 * whose <false> instances are the kernels without a set) -- with three things added:
 *
 *   header       where fr_parse_header refuses the dictionary bit the DictID is looked up in the call's id table (the first entry
 *                whose id equals it, FR_DICT when there is none: behind the header checksum, in front of the first block).  The
 *                entry, + 1, is FrState::dictEntry while the frame is open; a later call whose set does not have that entry fails
 *                the stream with FR_DICT and reads nothing of the set.
 *   independent  every compressed block is decoded against the entry's kept bytes as an external dictionary (DecodeDict mode 2),
 *                into the buffer or straight into dst.  On the fast path the plan writes the batch decoder's dictOff / dictLen /
 *                dictMode 2 for every row and for the straddling block, and the commit stores the entry with the state.
 *   chained      when the header is accepted the wave copies the kept bytes to the front of the stream's buffer: tail = their length,
 *                pending = 0.  From there the reader's prefix logic (the last min(tail, 64 KiB) bytes, DecodeDict mode 1) and its
 *                sliding are LZ4ChainDecoder's after Inject(kept bytes); the kept bytes are never drained, never counted in
 *                bytesRead and never enter the content checksum.  The buffer holds 64 KiB + maxBlockSize + 64 bytes.
 *
 * An offset that reaches before the first kept byte is FR_BLOCK; an entry of no bytes reads as a plain frame whose id resolved.
 * Included last by k4lz4_capi.hip: device code that comes in front of other kernels renumbers their registers.
 */
#pragma once
#include "k4lz4_frame_feed.hpp"

namespace k4 {

struct FrDictReadArgs { FrReadArgs r; FrDict d; };
struct FrDictFastArgs { FrFastArgs f; FrDictRows w; };
struct FrDictFeedArgs { FrFeedArgs f; FrDict d; };
struct FrDictFeedFastArgs { FrFeedFastArgs f; FrDictRows w; };

__global__ __launch_bounds__(64 * FR_WAVES_PER_WG) void k4_fr_dict_read_kernel(FrDictReadArgs da)
{
    __shared__ uint32_t lds[FR_WAVES_PER_WG][DECODE_LDS_DWORDS];
    const FrReadArgs &a = da.r;
    const FrDict &d = da.d;
#define FR_LOOP_DICT 1
#include "k4lz4_frame_reader_loop.hpp"
#undef FR_LOOP_DICT
}

__global__ __launch_bounds__(256) void k4_fr_dict_plan_kernel(FrDictFastArgs a)
{
    fr_plan_body<true>(a.f, a.w);
}

__global__ __launch_bounds__(64 * FR_WAVES_PER_WG) void k4_fr_dict_commit_kernel(FrDictFastArgs a)
{
    fr_commit_body<true>(a.f, a.w.entry);
}

__global__ __launch_bounds__(64 * FR_WAVES_PER_WG) void k4_fr_dict_feed_kernel(FrDictFeedArgs da)
{
    __shared__ uint32_t lds[FR_WAVES_PER_WG][DECODE_LDS_DWORDS];
    const FrFeedArgs &fa = da.f;
    const FrDict &d = da.d;
#define FR_LOOP_DICT 1
#include "k4lz4_frame_feed_loop.hpp"
#undef FR_LOOP_DICT
}

__global__ __launch_bounds__(256) void k4_fr_dict_feed_plan_kernel(FrDictFeedFastArgs a)
{
    fr_feed_plan_body<true>(a.f, a.w);
}

__global__ __launch_bounds__(64 * FR_WAVES_PER_WG) void k4_fr_dict_feed_commit_kernel(FrDictFeedFastArgs a)
{
    fr_feed_commit_body<true>(a.f, a.w.entry);
}

}  // namespace k4
