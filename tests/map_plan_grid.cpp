// The read mapper's batch plan (stralg_amd/csrc/sx_map_plan.hpp) over a grid of free memory, counts and switches, one line
// a case: what tests/test_map_plan.py compares with tests/golden/map_plans.txt.  No GPU, no library: the plan is arithmetic.
#include <inttypes.h>
#include <stdio.h>

#include <initializer_list>

#include "sx_map_plan.hpp"

using namespace sx;

struct mem_kind {
    const char *name;
    bool known;
    uint64_t bytes;
};

// one step of a room's chain: what a batch of `groups` groups that needs `need` hits makes of the room
static void step(uint64_t &cap, uint64_t largest, uint64_t need, uint32_t groups)
{
    const map_room_step s = map_room_next(cap, largest, need, groups);
    if (s.halve) printf(" %" PRIu64 "/%u->halve", need, groups);
    else printf(" %" PRIu64 "/%u->%" PRIu64, need, groups, s.cap);
    cap = s.cap;
}

static void next_row(uint64_t cap, uint64_t largest, uint64_t need, uint32_t groups, const char *kind = "next")
{
    const map_room_step s = map_room_next(cap, largest, need, groups);
    printf("%s cap=%" PRIu64 " largest=%" PRIu64 " need=%" PRIu64 " groups=%u : halve=%d cap=%" PRIu64 "\n", kind, cap, largest, need, groups,
           (int)s.halve, s.cap);
}

// The rows of the room switch (SX_FLAG_SAM_ROOM_HITS), behind everything else: the lines above are what they were without it
static void room_switch_rows(const mem_kind *mems, const uint32_t *records, const uint32_t *reads, const uint32_t *groups,
                             const int64_t *batch_flags)
{
    const int64_t room_flags[6] = {1, 4, 100, 400, (int64_t)1 << 20, (int64_t)1 << 40};
    // the largest room is the switch, whatever the memory
    for (int64_t s : room_flags) {
        printf("switch_largest switch=%" PRId64 " :", s);
        for (int m = 0; m < 5; ++m) printf(" free=%s->%" PRIu64, mems[m].name, map_room_largest(mems[m].known, mems[m].bytes, s));
        printf("\n");
    }
    // the room to start with: a line a (switch, memory, records), reads x group x flag in the order of the lines above
    for (int64_t s : room_flags)
        for (int m = 0; m < 5; ++m)
            for (int r = 0; r < 3; ++r) {
                const uint64_t largest = map_room_largest(mems[m].known, mems[m].bytes, s);
                printf("switch_first switch=%" PRId64 " free=%s n_records=%u :", s, mems[m].name, records[r]);
                for (int n = 0; n < 4; ++n)
                    for (int g = 0; g < 3; ++g)
                        for (int f = 0; f < 4; ++f)
                            printf(" %" PRIu64, map_room_first(map_batch_max(batch_flags[f], groups[g], reads[n]), records[r], largest, s));
                printf("\n");
            }
    // A room's chain from those rooms: a need below twice the room, one above it, one above the largest for several groups
    // (halve) and for one (it gets what it needs: the room is above the largest from here on), several groups where the need fits
    for (int64_t s : room_flags)
        for (int r = 0; r < 3; ++r)
            for (int64_t f : {(int64_t)0, (int64_t)8}) {
                const uint64_t largest = map_room_largest(true, 1ull << 30, s);
                uint64_t cap = map_room_first(map_batch_max(f, 0, 240), records[r], largest, s);
                printf("switch_chain switch=%" PRId64 " n_records=%u flag=%" PRId64 " largest=%" PRIu64 " cap=%" PRIu64 " :", s, records[r], f, largest, cap);
                step(cap, largest, cap + cap / 2, 4);
                step(cap, largest, 3 * cap, 4);
                step(cap, largest, largest + 1000, 3);
                step(cap, largest, largest + 1000, 1);
                step(cap, largest, largest, 2);
                printf("\n");
            }
}

int main()
{
    const mem_kind mems[5] = {{"unknown", false, 0}, {"0", true, 0}, {"2^20", true, 1ull << 20}, {"2^30", true, 1ull << 30}, {"80*2^30", true, 80ull << 30}};
    const uint32_t records[3] = {1, 2, 200}, reads[4] = {1, 7, 1u << 20, (1u << 21) + 1}, groups[3] = {0, 1, 2};
    const int64_t batch_flags[4] = {0, 1, 7, 8}, window_flags[4] = {0, 1, 4096, (int64_t)1 << 40};

    for (const mem_kind &m : mems) printf("largest free=%s : %" PRIu64 "\n", m.name, map_room_largest(m.known, m.bytes));

    // reads of a batch: a line a (reads, group), the four flags
    for (uint32_t n_reads : reads)
        for (uint32_t group : groups) {
            printf("batch_max n_reads=%u group=%u :", n_reads, group);
            for (int64_t f : batch_flags) printf(" flag%" PRId64 "=%u", f, map_batch_max(f, group, n_reads));
            printf("\n");
        }

    // the room to start with: a line a (memory, records, reads), group x flag in the order above
    for (const mem_kind &m : mems)
        for (uint32_t n_records : records)
            for (uint32_t n_reads : reads) {
                const uint64_t largest = map_room_largest(m.known, m.bytes);
                printf("first free=%s n_records=%u n_reads=%u :", m.name, n_records, n_reads);
                for (uint32_t group : groups)
                    for (int64_t f : batch_flags) printf(" %" PRIu64, map_room_first(map_batch_max(f, group, n_reads), n_records, largest));
                printf("\n");
            }

    // A room's chain: a need below twice the room, one above it, one between 4/5 of the largest room and the largest
    // (growing by a quarter would pass it), one above the largest for several groups (halve) and for one (it gets what it
    // needs), and several groups again where the need fits
    for (const mem_kind &m : mems)
        for (uint32_t n_records : records)
            for (int64_t f : {(int64_t)0, (int64_t)7}) {
                const uint64_t largest = map_room_largest(m.known, m.bytes);
                uint64_t cap = map_room_first(map_batch_max(f, 0, 1u << 20), n_records, largest);
                printf("chain free=%s n_records=%u flag=%" PRId64 " largest=%" PRIu64 " cap=%" PRIu64 " :", m.name, n_records, f, largest, cap);
                step(cap, largest, cap + cap / 2, 4);
                step(cap, largest, 3 * cap, 4);
                step(cap, largest, largest / 10 * 9, 4);
                step(cap, largest, largest + 1000, 3);
                step(cap, largest, largest + 1000, 1);
                step(cap, largest, largest, 2);
                printf("\n");
            }

    for (int64_t f : window_flags)
        printf("window flag=%" PRId64 " : stage4096=%zu stage2^25=%zu stage2^26=%zu\n", f, map_window_bytes(f, 4096), map_window_bytes(f, (size_t)1 << 25),
               map_window_bytes(f, (size_t)1 << 26));

    printf("located_rows :");
    for (int64_t f : {(int64_t)0, (int64_t)5, (int64_t)64, (int64_t)1 << 40}) printf(" flag%" PRId64 "=%" PRIu64, f, map_located_rows(f));
    printf("\n");

    for (uint32_t g : {1u, 2u}) {
        printf("halved g=%u :", g);
        for (uint32_t batch : {2u, 3u, 4u, 6u, 7u, 8u, 10u, 1u << 20, (1u << 21) + 2}) printf(" %u->%u", batch, map_batch_halved(batch, g));
        printf("\n");
    }

    // the rows that tests/test_map_plan.py asserts by value
    const uint64_t L = 1ull << 27;
    next_row(1u << 16, L, 70000, 1);
    next_row(1u << 16, L, 200000, 1);
    next_row(1ull << 26, L, 120000000, 1);
    next_row(1ull << 26, L, 140000000, 1);
    next_row(1ull << 26, L, 140000000, 2);

    room_switch_rows(mems, records, reads, groups, batch_flags);
    // ... and its rows that the test asserts by value: batches of 8 and of 240 reads on two records
    for (int64_t sw : {(int64_t)1, (int64_t)100, (int64_t)400, (int64_t)1 << 20})
        for (uint32_t batch_max : {8u, 240u})
            printf("room_first switch=%" PRId64 " batch_max=%u n_records=2 : %" PRIu64 "\n", sw, batch_max,
                   map_room_first(batch_max, 2, map_room_largest(true, 80ull << 30, sw), sw));
    next_row(1, 1, 5, 2, "room_next");
    next_row(1, 1, 5, 1, "room_next");
    next_row(6, 1, 7, 1, "room_next");
    next_row(64, 100, 90, 4, "room_next");
    next_row(100, 100, 332, 2, "room_next");
    next_row(100, 100, 332, 1, "room_next");
    next_row(64, 1ull << 20, 200, 4, "room_next");
    return 0;
}
