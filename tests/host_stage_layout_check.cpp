// CPU check of the staging buffer's layout arithmetic (csrc/host_stage_layout.hpp), the header the C ABI's host-in /
// host-out wrappers size and carve their one device buffer with.  Own main, no GPU: random slot lists -- wanted and
// unwanted (a NULL optional argument) slots, zero counts, slots that ask for float4 alignment -- and for each list
//   - offsets increase in declaration order; a slot that asks for an alignment (1 or kVec4 = 4 floats) starts at a
//     multiple of it, and no further from the end of the slot before than that alignment needs (align 1: packed),
//   - slots are disjoint: one starts at or after the end of the one before,
//   - the total is the end of the last slot that takes space (0 when none does),
//   - an unwanted or empty slot resolves to a null pointer and moves nothing,
//   - resolving against a real allocation of `total` floats stays inside it (the sanitizer build writes every slot),
//   - the seventeenth slot is refused.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <vector>

#include "../blackbox_mpc_amd/csrc/host_stage_layout.hpp"

using bbmpc::StageLayout;
static_assert(StageLayout::kVec4 * sizeof(float) == 16, "kVec4 is what a float4 access needs");

static int g_failed = 0;
#define EXPECT(cond, ...)                                      \
    do {                                                       \
        if (!(cond)) {                                         \
            ++g_failed;                                        \
            std::printf("FAILED %s:%d: %s | ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                          \
            std::printf("\n");                                 \
        }                                                      \
    } while (0)

struct Want {
    size_t count;
    bool wanted;
    size_t align = 1;
};

static void check_list(const std::vector<Want>& list, int id) {
    StageLayout lay;
    std::vector<int> slot;
    for (const Want& w : list) {
        const size_t before = lay.total;
        const int s = lay.add(w.count, w.wanted, w.align);
        slot.push_back(s);
        if (!w.wanted || w.count == 0) EXPECT(lay.total == before, "list %d: an empty slot moved the total", id);
    }
    EXPECT(lay.n == (int)list.size(), "list %d", id);
    size_t end = 0;              // end of the last slot that takes space
    bool any = false;
    for (size_t i = 0; i < list.size(); ++i) {
        const int s = slot[i];
        EXPECT(s == (int)i, "list %d: slots are numbered in declaration order", id);
        const bool empty = !list[i].wanted || list[i].count == 0;
        if (empty) {
            EXPECT(lay.off[s] == StageLayout::kNone && lay.len[s] == 0, "list %d slot %d", id, s);
            continue;
        }
        EXPECT(lay.len[s] == list[i].count, "list %d slot %d", id, s);
        EXPECT(lay.off[s] % list[i].align == 0, "list %d slot %d: offset %zu", id, s, lay.off[s]);
        EXPECT(lay.off[s] >= end, "list %d slot %d: offset %zu inside the slot before (ends %zu)", id, s, lay.off[s], end);
        EXPECT(lay.off[s] < end + list[i].align, "list %d slot %d: more than the alignment's padding", id, s);
        if (any) EXPECT(lay.off[s] > 0, "list %d slot %d", id, s);
        end = lay.off[s] + lay.len[s];
        any = true;
    }
    EXPECT(lay.total == end, "list %d: total %zu, last slot ends %zu", id, lay.total, end);

    // against a real allocation: null slots give null, the others lie inside [base, base + total)
    std::vector<float> buf(lay.total);
    float* base = buf.data();
    for (size_t i = 0; i < list.size(); ++i) {
        float* p = lay.at(base, slot[i]);
        if (!list[i].wanted || list[i].count == 0) {
            EXPECT(p == nullptr, "list %d slot %zu: an empty slot resolves to a pointer", id, i);
            continue;
        }
        EXPECT(p == base + lay.off[slot[i]], "list %d slot %zu", id, i);
        for (size_t j = 0; j < list[i].count; ++j) p[j] = (float)(i + 1);      // (out of bounds -> the sanitizer build stops here)
    }
    for (size_t i = 0; i < list.size(); ++i) {                                  // nobody wrote into anybody else's slot
        const float* p = lay.at((const float*)base, slot[i]);
        if (!p) continue;
        bool own = true;
        for (size_t j = 0; j < list[i].count; ++j) own = own && p[j] == (float)(i + 1);
        EXPECT(own, "list %d slot %zu was overwritten", id, i);
    }
}

int main() {
    std::mt19937 rng(20240607u);
    const size_t edge[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 4096};
    int lists = 0;
    for (; lists < 400; ++lists) {
        const int n = 1 + (int)(rng() % StageLayout::kMaxSlots);
        std::vector<Want> list;
        for (int i = 0; i < n; ++i) {
            const unsigned kind = rng() % 8;
            Want w;
            w.align = rng() % 3 == 0 ? StageLayout::kVec4 : 1;
            w.wanted = kind != 0;                                               // one in eight: a NULL optional argument
            w.count = kind == 1 ? 0 : (kind < 5 ? edge[rng() % (sizeof(edge) / sizeof(edge[0]))] : 1 + rng() % 3000);
            list.push_back(w);
        }
        check_list(list, lists);
    }
    check_list({}, lists++);
    check_list({{0, true}, {5, false}}, lists++);                               // nothing takes space: total 0
    check_list({{5, false}, {7, true}}, lists++);                               // the first real slot starts at 0
    {
        StageLayout lay;
        lay.add(5, false);
        EXPECT(lay.add(7) == 1 && lay.off[1] == 0 && lay.total == 7, "first real slot");
        EXPECT(lay.add(1) == 2 && lay.off[2] == 7 && lay.total == 8, "packed behind the first");
        EXPECT(lay.add(2, true, StageLayout::kVec4) == 3 && lay.off[3] == 8 && lay.total == 10, "already aligned: no padding");
        EXPECT(lay.add(3, true, StageLayout::kVec4) == 4 && lay.off[4] == 12 && lay.total == 15, "padded to 4 floats");
        EXPECT(lay.add(1) == 5 && lay.off[5] == 15 && lay.total == 16, "packed again");
    }
    {
        StageLayout lay;
        for (int i = 0; i < StageLayout::kMaxSlots; ++i) lay.add(1);
        bool refused = false;
        try {
            lay.add(1);
        } catch (const std::logic_error&) {
            refused = true;
        }
        EXPECT(refused, "a slot past kMaxSlots was accepted");
    }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("%d slot lists, all checks held\n", lists);
    return 0;
}
