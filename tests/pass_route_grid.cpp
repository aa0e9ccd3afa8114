// Stand-alone walk of plan_pass (csrc/dcr_pass_route.h) over the boundary grid of tests/test_pass_route_cpu.py, for a build
// with -fsanitize=address,undefined: the header alone, no HIP, no library.  Prints how many plans took each route, how many
// list by rows, how many carry the hub supplement, and the sum of the three estimates' bit patterns; the test compares the
// line with what the library gives over the same grid.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "dcr_pass_route.h"

using namespace dcr;

int main() {
    const int64_t ns[] = {2999, 3000, 1000000};
    const int64_t es[] = {10000, 80000};
    const int32_t degs[] = {H2_MAXDEG, H2_MAXDEG + 1, NC_MAXD, NC_MAXD + 1};
    const int64_t caps[] = {3999999, 4000000, ((int64_t)1 << 30) - 1, (int64_t)1 << 30};
    const int edits[] = {DIRTY_EDITS, DIRTY_EDITS + 1};
    long long routes[4] = {0, 0, 0, 0}, by_rows = 0, hubs = 0;
    uint64_t bits = 0;
    for (int64_t n : ns)
        for (int over = 0; over < 2; ++over)
            for (int64_t E : es)
                for (int32_t deg : degs)
                    for (int64_t cap : caps)
                        for (int pending : edits)
                            for (int curv = DCR_CURV_BFC; curv <= DCR_CURV_HAANTJES; ++curv)
                                for (int impl = 0; impl < 4; ++impl)
                                    for (int inc = 0; inc < 2; ++inc)
                                        for (int fine = 0; fine < 2; ++fine)
                                            for (int full = -2; full < 2; ++full)       // unset, cap - 1, cap, cap + 1
                                                for (int sweep = -1; sweep < 2; ++sweep) {
                                                    // the largest sum of squared degrees with share <= 0.045, or one more
                                                    const double sd2 = (double)(int64_t)(0.045 * (double)n * (double)n) + over;
                                                    const PassFacts f{n, E, cap, sd2, deg, pending};
                                                    const PassSwitches sw{impl, fine != 0, full != -2, full == -2 ? 0 : cap + full, sweep};
                                                    const PassPlan p = plan_pass(f, sw, curv, inc != 0);
                                                    routes[p.route] += 1;
                                                    by_rows += p.list_by_rows;
                                                    hubs += p.hub_supplement;
                                                    for (double t : {p.t_h2, p.t_nc, p.t_edges}) {
                                                        uint64_t u;
                                                        memcpy(&u, &t, sizeof u);
                                                        bits += u;
                                                    }
                                                }
    printf("%lld %lld %lld %lld %lld %lld %" PRIu64 "\n", routes[0], routes[1], routes[2], routes[3], by_rows, hubs, bits);
    return 0;
}
