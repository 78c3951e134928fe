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

static void next_row(uint64_t cap, uint64_t largest, uint64_t need, uint32_t groups)
{
    const map_room_step s = map_room_next(cap, largest, need, groups);
    printf("next cap=%" PRIu64 " largest=%" PRIu64 " need=%" PRIu64 " groups=%u : halve=%d cap=%" PRIu64 "\n", cap, largest, need, groups,
           (int)s.halve, s.cap);
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
    return 0;
}
