// csrc/dcr_row_patch.h alone, with nothing of the library: random sequences of edge additions that carry nodes across both class
// limits, the patched plan compared with a full rebuild after every edit.  Built with -fsanitize=address,undefined and run by
// tests/test_fosr_cpu.py.  Prints the number of edits checked, of class changes seen at the lower and at the upper limit.
#include <cstdio>
#include <cstdlib>

#include "dcr_row_patch.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t draw(uint32_t below) {  // xorshift64*
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return (uint32_t)(((state * 0x2545F4914F6CDD1Dull) >> 33) % below);
}

int main() {
    long edits = 0, crossed[2] = {0, 0};
    // small limits, so that a few hundred additions cross both of them many times; and the library's own
    const int limits[3][2] = {{2, 5}, {1, 2}, {32, 2048}};
    for (int round = 0; round < 60; ++round) {
        const int *lim = limits[round % 3];
        const int n = round % 3 == 2 ? 2300 : 2 + (int)draw(40);
        dcr::HostRowPlan plan;
        plan.short_deg = lim[0];
        plan.long_deg = lim[1];
        plan.deg.assign((size_t)n, 0);
        if (round % 3 == 2)  // nodes waiting at either side of both limits
            for (int v = 0; v < n; ++v) plan.deg[(size_t)v] = v % 7 == 0 ? 2047 + (int)draw(3) : v % 5 == 0 ? 31 + (int)draw(3) : (int)draw(4);
        plan.rebuild();
        const int steps = round % 3 == 2 ? 400 : 6 * n;
        for (int s = 0; s < steps; ++s) {
            const int32_t u = (int32_t)draw((uint32_t)n);
            int32_t v = (int32_t)draw((uint32_t)n - 1);
            if (v >= u) ++v;
            const int cu = plan.cls(plan.deg[(size_t)u]), cv = plan.cls(plan.deg[(size_t)v]);
            const bool changed = plan.add_edge(u, v);
            const int du = plan.cls(plan.deg[(size_t)u]), dv = plan.cls(plan.deg[(size_t)v]);
            crossed[0] += (cu == 2 && du == 1) + (cv == 2 && dv == 1);
            crossed[1] += (cu == 1 && du == 0) + (cv == 1 && dv == 0);
            dcr::HostRowPlan full;
            full.short_deg = lim[0];
            full.long_deg = lim[1];
            full.deg = plan.deg;
            full.rebuild();
            const bool same = full.rows == plan.rows && full.count[0] == plan.count[0] && full.count[1] == plan.count[1] &&
                              full.count[2] == plan.count[2];
            if (!same || changed != (cu != du || cv != dv)) {
                std::fprintf(stderr, "round %d step %d: the patched plan differs from the rebuilt one\n", round, s);
                return 1;
            }
            ++edits;
        }
    }
    std::printf("%ld %ld %ld\n", edits, crossed[0], crossed[1]);
    return 0;
}
