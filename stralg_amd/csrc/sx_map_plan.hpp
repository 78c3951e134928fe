// sx_map_plan.hpp -- what the read mapper's loop (sx_map.hip) decides without looking at the device: how much room a batch's
// hits get, when that room grows and when the batch is halved instead, how many reads a batch holds, the text's window,
// the rows of a located run.  Plain arithmetic on the free memory, four of the context's switches and counts: host only,
// no HIP, no context, so that tests/test_map_plan.py checks it without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef SX_SAM_WINDOW_BYTES
#define SX_SAM_WINDOW_BYTES (32u << 20) // window of the streamed form: one pinned staging buffer
#endif

namespace sx {

// The largest room for the hits of a batch's searches: 2^27 hits or what a quarter of the free memory holds (72 bytes a hit:
// the searches' array, the merged one, the byte offsets); 2^26 where the free memory is unknown or given as 0.
// room_flag: SX_FLAG_SAM_ROOM_HITS, a test switch; > 0: that many hits, whatever the memory
static inline uint64_t map_room_largest(bool free_known, uint64_t free_bytes, int64_t room_flag = 0)
{
    if (room_flag > 0) return (uint64_t)room_flag;
    uint64_t largest = 1ull << 26;
    if (free_known && free_bytes) largest = free_bytes / 4 / 72 < (1ull << 27) ? free_bytes / 4 / 72 : 1ull << 27;
    return largest < (1u << 16) ? 1u << 16 : largest;
}

// the room to start with: a guess of four hits a (read, record), 2^16 hits at least (with the test switch set: 1)
static inline uint64_t map_room_first(uint32_t batch_max, uint32_t n_records, uint64_t largest, int64_t room_flag = 0)
{
    const uint64_t guess = (uint64_t)batch_max * n_records * 4, least = room_flag > 0 ? 1u : 1u << 16;
    return guess < least ? least : guess > largest ? largest : guess;
}

// A batch of `groups` groups needs room for `need` hits and has `cap`: the room grows where that is allowed (one group alone
// gets whatever it needs) -- a search over few reads leaves most of its lanes idle; otherwise halve, and cap stays
struct map_room_step {
    bool halve;
    uint64_t cap;
};
static inline map_room_step map_room_next(uint64_t cap, uint64_t largest, uint64_t need, uint32_t groups)
{
    if (need > largest && groups > 1) return {true, cap};
    cap = need + need / 4 > 2 * cap ? need + need / 4 : 2 * cap;
    if (cap > largest && need <= largest) cap = largest;
    return {false, cap};
}

// reads of a batch; flag: SX_FLAG_SAM_BATCH_READS.  group 2: a batch holds whole groups, both strands of a read (n_reads is
// even then)
static inline uint32_t map_batch_max(int64_t flag, uint32_t group, uint32_t n_reads)
{
    uint32_t batch_max = flag > 0 ? (uint32_t)flag : (1u << 20);
    if (group == 2) batch_max += batch_max & 1u;
    return batch_max > n_reads ? n_reads : batch_max;
}

// half the groups of a batch, rounded up (g: reads a group, 1 where there are none)
static inline uint32_t map_batch_halved(uint32_t batch, uint32_t g) { return (batch / g + 1) / 2 * g; }

// bytes of a window of the text; flag: SX_FLAG_SAM_WINDOW_BYTES.  A window leaves through one staging buffer
static inline size_t map_window_bytes(int64_t flag, size_t stage_bytes)
{
    const size_t window = flag > 0 ? ((size_t)flag + 15) & ~(size_t)15 : (size_t)SX_SAM_WINDOW_BYTES;
    return window > stage_bytes ? stage_bytes : window;
}

// Paired reads.  Reads of a batch: whole pairs, four reads each (n_reads is a multiple of four); here
// the flag, SX_FLAG_SAM_BATCH_READS, counts pairs; 2^18 pairs where it is not set
static inline uint32_t map_pairs_batch_max(int64_t flag, uint32_t n_reads)
{
    const uint64_t pairs = flag > 0 ? (uint64_t)flag : 1u << 18;
    return pairs * 4 > n_reads ? n_reads : (uint32_t)(pairs * 4);
}

// The lines of a batch, and the line descriptors of its proper combinations, that a batch of several pairs may have before
// it is halved (a pair alone gets whatever it needs): 2^27, or what a quarter of the free memory holds at 28 bytes each (a
// line: position, span, hit, count; a descriptor: 20 bytes and its byte offset), 2^16 at least.  room_flag:
// SX_FLAG_PAIRS_ROOM_LINES, or where that is 0 SX_FLAG_SAM_ROOM_HITS, the test switch of the hits' room; > 0: that many
static inline uint64_t map_pairs_largest(bool free_known, uint64_t free_bytes, int64_t room_flag = 0)
{
    if (room_flag > 0) return (uint64_t)room_flag;
    uint64_t largest = 1ull << 26;
    if (free_known && free_bytes) largest = free_bytes / 4 / 28 < (1ull << 27) ? free_bytes / 4 / 28 : 1ull << 27;
    return largest < (1u << 16) ? 1u << 16 : largest;
}

// lines a located run may have; flag: SX_FLAG_LOCATE_CHUNK_ROWS
static inline uint64_t map_located_rows(int64_t flag) { return flag > 0 ? (uint64_t)flag : 1ull << 28; }

} // namespace sx
