// The row plan kept on the host across edge additions (dcr_fosr.hip): a copy of the degrees, the class counts and the list of rows
// by class as dcr_analysis.hip::classify_rows makes it.  Adding an edge moves two degrees up by one; the list changes only when
// one of them crosses a class limit, and then only that node changes its place.  Pure host code with no HIP include, so that
// tests/row_patch_check.cpp can run it alone under the sanitizers against a full rebuild.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace dcr {

struct HostRowPlan {
    int short_deg = 0, long_deg = 0;  // SP_SHORT_DEG and SP_LONG_DEG of dcr_analysis.h
    std::vector<int32_t> deg;         // [n]
    std::vector<int32_t> rows;        // [n]: the long rows, then the medium ones, then the short ones, each by node id
    int64_t count[3] = {0, 0, 0};     // long, medium, short

    int cls(int d) const { return d > long_deg ? 0 : d > short_deg ? 1 : 2; }

    void rebuild() {
        const int64_t n = (int64_t)deg.size();
        rows.resize((size_t)n);
        count[0] = count[1] = count[2] = 0;
        for (int64_t v = 0; v < n; ++v) ++count[cls(deg[(size_t)v])];
        int64_t at[3] = {0, count[0], count[0] + count[1]};
        for (int64_t v = 0; v < n; ++v) rows[(size_t)at[cls(deg[(size_t)v])]++] = (int32_t)v;
    }

    // deg[v] += 1.  Returns true where v changed its class: it has then left its place in `rows` and taken the one its id gives
    // it in the class above (a rotation of the entries between the two places), and the counts have followed.
    bool bump(int32_t v) {
        const int from = cls(deg[(size_t)v]), to = cls(++deg[(size_t)v]);
        if (from == to) return false;  // (to == from - 1: one more neighbour crosses one limit at most)
        const int64_t begin_from = from == 2 ? count[0] + count[1] : count[0], begin_to = to == 0 ? 0 : count[0];
        const auto first = rows.begin();
        const auto old_at = std::lower_bound(first + begin_from, first + begin_from + count[from], v);
        const auto new_at = std::lower_bound(first + begin_to, first + begin_to + count[to], v);
        std::rotate(new_at, old_at, old_at + 1);
        --count[from];
        ++count[to];
        return true;
    }

    // the edge {u, v} was added; true where `rows` and the counts changed (the device copy is then stale)
    bool add_edge(int32_t u, int32_t v) {
        const bool a = bump(u), b = bump(v);
        return a || b;
    }
};

}  // namespace dcr
