/* tests/emu/parse_pace.cpp -- the level rule of k4_parse_kernel's late-blocks-first priorities (k4lz4_parse.hpp: parse_pace_estimate,
 * parse_pace_level, parse_pace_first_level, ParsePace::latest_of) as the host build of the product header has it: plain functions of
 * a few words, called by tests/test_parse_pace.py through the functions below.  The issue priority itself exists on the GPU only
 * (tests/test_gpu_parse_pace.py).  Test infrastructure only. */
#include "hip/hip_runtime.h"
#include "k4lz4_decode.hpp"
#include "k4lz4_encode_fast.hpp"
#include "k4lz4_parse.hpp"

extern "C" {
uint32_t k4emu_pace_den() { return k4::PARSE_PACE_DEN; }
uint32_t k4emu_pace_max() { return k4::PARSE_PACE_MAX; }
int k4emu_pace_words() { return k4::PARSE_PACE_DWORDS; }
int k4emu_pace_lds_bytes() { return (k4::PARSE_LDS_DWORDS + k4::PARSE_PACE_DWORDS) * 4; }
uint32_t k4emu_pace_estimate(uint32_t wg_start, uint32_t start, uint32_t now, uint32_t c, uint32_t U) { return k4::parse_pace_estimate(wg_start, start, now, c, U); }
int k4emu_pace_level(uint32_t mine, uint32_t latest) { return k4::parse_pace_level(mine, latest); }
int k4emu_pace_first_level(uint32_t wave, int in_lds) { return k4::parse_pace_first_level(wave, in_lds != 0); }
/* a wave's look: the sixteen words of its SIMD as they stand (`row`, its own word among them at `me`), its new estimate `mine`;
 * the word is stored before the row is read, as ParsePace::report does */
int k4emu_pace_look(uint32_t *row, int me, uint32_t mine)
{
    row[me] = mine;
    return k4::parse_pace_level(mine, k4::ParsePace::latest_of(row, 0));
}
}
