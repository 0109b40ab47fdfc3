// Stand-alone check of the completion line's host side (blackbox_mpc_amd/csrc/completion_line.hpp): built and run by
// tests/test_completion_line_cpu.py.  Exit status 0 = every check held; otherwise the failed check is printed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../blackbox_mpc_amd/csrc/completion_line.hpp"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static uint32_t bits_of(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}
static float float_of(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}

int main() {
    using namespace bbmpc;
    // -0.0, a NaN with a payload, a denormal, an ordinary value, the largest finite one
    const float rec[5] = {-0.0f, float_of(0x7fc12345u), float_of(0x00000123u), -1.2345678f, float_of(0x7f7fffffu)};
    const float sentinel = 42.0f;
    const uint32_t seqs[] = {1u, 0xffffu, 0x10000u, 0x10001u, 0xfffeffffu, 0x12345678u};
    for (uint32_t seq : seqs) {
        alignas(64) uint32_t line[16];
        completion_line_encode(line, seq, rec);
        float out[5];
        for (float& o : out) o = sentinel;
        CHECK(completion_line_decode(line, seq, out));
        for (int f = 0; f < 5; ++f) CHECK(bits_of(out[f]) == bits_of(rec[f]));
        // the line of the call before is refused whole, and leaves the destination alone
        for (float& o : out) o = sentinel;
        CHECK(!completion_line_decode(line, seq + 1u, out));
        uint32_t prev[16];
        completion_line_encode(prev, seq - 1u, rec);
        CHECK(!completion_line_decode(prev, seq, out));
        for (int f = 0; f < 5; ++f) CHECK(out[f] == sentinel);
        // one stale word (still the previous call's), whichever word it is: refused; a stale filler word does not matter
        for (int i = 0; i < 16; ++i) {
            uint32_t torn[16];
            memcpy(torn, line, sizeof(torn));
            torn[i] = prev[i];
            const bool looked_at = i < 10 || i == 15;
            for (float& o : out) o = sentinel;
            CHECK(completion_line_decode(torn, seq, out) == !looked_at);
            if (looked_at)
                for (int f = 0; f < 5; ++f) CHECK(out[f] == sentinel);
        }
        // same 16-bit tag, another call (65536 numbers earlier): word 15 decides
        uint32_t old[16];
        completion_line_encode(old, seq - 0x10000u, rec);
        CHECK(!completion_line_decode(old, seq, out));
    }
    if (failures == 0) printf("completion line: all checks held\n");
    return failures == 0 ? 0 : 1;
}
