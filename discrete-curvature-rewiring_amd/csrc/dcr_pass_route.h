// Which kernels run a curvature pass: one pure host function of six facts about the graph and four switches.  Plain C++, no
// HIP and no environment: launch_curvature_pass (dcr_bfc.hip) fills the two structs and switches over the plan,
// dcr_pass_plan (include/dcr.h) exposes the same function to tests/test_pass_route_cpu.py.
#pragma once
#include <stdint.h>

#include "dcr.h"

namespace dcr {

// limits of the kernels that the route depends on
constexpr int H2_MAXDEG = 5000;   // two-hop pass: flagged neighbours live in every partition's table (5,500 keys in the largest
                                  // class: a hub near the limit is split into many partitions, one workgroup each)
constexpr int NC_MAXD = 8190;     // node-centric pass: largest degree whose neighbour table fits the biggest class
constexpr int DIRTY_EDITS = 3;    // edits between two passes that get exact dirty flags (dcr_internal.h); later ones are coarse

struct PassFacts {
    int64_t n;
    int64_t n_edges;        // undirected
    int64_t cap_total;      // adjacency slots allocated
    double sum_deg2;        // sum of squared degrees when the graph was created
    int32_t max_deg_bound;  // upper bound on every degree
    int pending_edits;      // edits flagged since the last pass
};

struct PassSwitches {
    int pass_impl;            // DCR_PASS, fixed when the graph is created: 0 automatic, 1 edge, 2 nc, 3 h2
    bool fine_on;             // DCR_NC_FINE != 0: the edge-by-edge kernels may be used
    bool fine_full_set;       // DCR_NC_FINE_FULL=<slots> is set: full passes go edge by edge up to that many adjacency slots (A/B aid)
    int64_t fine_full_slots;
    int fine_sweep;           // DCR_NC_FINE_SWEEP: -1 unset, 0 the edge list from the flagged nodes' rows, 1 from a sweep (A/B aid)
};

enum PassRoute { ROUTE_TWO_HOP = 0, ROUTE_EDGE_CENTRIC = 1, ROUTE_NC_CLASSES = 2, ROUTE_NC_EDGES = 3 };

struct PassPlan {
    PassRoute route;
    bool list_by_rows;    // incremental edge-by-edge pass: the edge list from the rows of the flagged nodes, not from a sweep
    bool hub_supplement;  // node-centric routes: the edge-centric kernels for the rest and process_hub_edges follow
    double t_h2, t_nc, t_edges;  // the three estimates below, ms
};

// Estimates of a full Balanced Forman pass, milliseconds on one MI355X.  Round 4: two fitted cost models instead of two
// thresholds from one graph family.  tools/probe_engine_choice.py times the engines on 31 graphs of four families
// (preferential attachment m = 2 / 5 / 10 / 20 at 2k-500k nodes, uniform random graphs of mean degree 6-20, grids, a dense
// random graph; profiles/r04_engine_choice.txt, profiles/r05_engine_choice.txt) and the pass times are, within 11-15 % on average,
//     node-centric:  0.127 + 0.438e-6 E + 1.135e-9 E s + 0.201 min(dmax, 400) / 400
//     two-hop:       0.120 + 1.193e-6 n + 4.498e-9 (sum d^2) (1 + 60 s / n)          (0.190 until round 5)
//     edge by edge:  0.012 + E (5.0e-6 + 4.2e-9 s)                                   (round 5)
// with E edges, n nodes, s = sum d^2 / n (the mean size of a 2-hop neighbourhood), dmax the largest degree: the class kernels
// of the node-centric engine stream about s entries per edge and lose a tenth of a millisecond to the tail of their hub units;
// the two-hop engine reads sum d^2 entries per pass, pays per node, and slows down as neighbourhoods overlap (s / n: the share
// of the graph a 2-hop neighbourhood covers — repeated keys, fuller tables, more partitions); a workgroup per edge costs its
// chain of dependent reads plus what it streams.  (Round 5: the fixed cost of a two-hop pass went from 0.19 to about 0.10 ms
// with the three-stream layout — re-fitted, kept a little above the measurements: on a 500 k-node graph of two edges per node
// the per-node cost is underestimated.)
//
// The two-hop engine takes a full Balanced Forman pass when its estimate is the lowest (DCR_PASS=h2: always), and never for
// graphs under 3,000 nodes (every engine is launch-bound there and the node-centric one has fewer launches), for s / n above
// 0.045 (measured 1.5-5 x slower there), hubs beyond its tables or 2^30 adjacency slots.  Otherwise the edge-centric kernels
// take the '1d' curvature and everything under DCR_PASS=edge, the node-centric ones the rest: edge by edge behind a few
// exactly flagged edits and for full passes of small graphs — the class kernels are launch-bound there (plans, four
// persistent grids and their joins: 0.17-0.4 ms whatever the graph holds), a workgroup per edge is not: Cora's size (5 k
// edges) 0.19 -> 0.04 ms, 25 k edges 0.31 -> 0.17, break-even near 50 k edges — automatic choice only, DCR_PASS=nc keeps the
// class kernels.  The edge list of an incremental pass: a sweep over every slot costs 11 us per 2.6 M slots, the rows of the
// flagged nodes a chain of five dependent reads, 14 us whatever the graph's size (S100k 0.203 / 0.208 ms per iteration sweep /
// rows, S1M 0.540 / 0.452): by rows from 4 M slots.
inline PassPlan plan_pass(const PassFacts &f, const PassSwitches &sw, int curv_type, bool incremental) {
    PassPlan p{};
    const double n = (double)f.n, nn = (double)(f.n > 0 ? f.n : 1), E = (double)f.n_edges, sd2 = f.sum_deg2;
    const double s = sd2 / nn, share = s / nn;
    const double dmax = (double)(f.max_deg_bound < 400 ? f.max_deg_bound : 400);
    p.t_h2 = 0.120 + 1.193e-6 * n + 4.498e-9 * sd2 * (1.0 + 60.0 * share);
    p.t_nc = 0.127 + 0.438e-6 * E + 1.135e-9 * E * s + 0.201 * dmax / 400.0;
    p.t_edges = 0.012 + E * (5.0e-6 + 4.2e-9 * s);

    const bool h2_able = curv_type == DCR_CURV_BFC && !incremental && f.max_deg_bound <= H2_MAXDEG && f.cap_total < (int64_t)1 << 30;
    const bool h2_cheapest = f.n >= 3000 && share <= 0.045 && !(sw.fine_on && p.t_edges < p.t_h2) && p.t_h2 < p.t_nc;
    if (h2_able && (sw.pass_impl == 3 || (sw.pass_impl == 0 && h2_cheapest))) {
        p.route = ROUTE_TWO_HOP;
        return p;
    }
    if (curv_type == DCR_CURV_1D || sw.pass_impl == 1) {
        p.route = ROUTE_EDGE_CENTRIC;
        return p;
    }
    // node-centric kernels; the edge-centric ones only for edges beyond their degree limits (two hubs with more than NC_MAXD
    // neighbours each), which cannot exist while the largest degree is within the limit
    p.hub_supplement = f.max_deg_bound > NC_MAXD;
    p.route = ROUTE_NC_CLASSES;
    if (sw.fine_on && incremental && f.pending_edits <= DIRTY_EDITS) {
        p.route = ROUTE_NC_EDGES;
        p.list_by_rows = sw.fine_sweep >= 0 ? sw.fine_sweep == 0 : f.cap_total >= 4000000;
    } else if (sw.fine_on && !incremental) {
        if (sw.fine_full_set ? f.cap_total <= sw.fine_full_slots : sw.pass_impl == 0 && p.t_edges < p.t_nc) p.route = ROUTE_NC_EDGES;
    }
    return p;
}

}  // namespace dcr
