// Node and edge betweenness centrality on the device-resident graph: Brandes' algorithm for unweighted graphs, pull-style and
// level-synchronous.  include/dcr.h has the rule; the reference has no counterpart, tests/betweenness_ref.py restates it in numpy.
//
// A batch holds BTW_B = 16 sources, a column each.  Three node-major arrays per batch: dist int32 [n][16] (-1: not reached),
// sigma fp64 [n][16] (the number of shortest paths from the column's source) and delta fp64 [n][16] (the dependency of the source
// on the node).  A lane owns two adjacent columns (8-byte loads of dist, 16-byte loads of sigma and delta), eight lanes cover a
// node, so the gather of one neighbour reads one 64-byte and up to two 128-byte lines.  Across batches: node_acc fp64 [n] and,
// where edge values are asked for, slot_acc fp64 per adjacency slot.  Nothing is n x n and there is no floating-point atomic.
//
// Kernels (rows through walk_rows in the three degree classes, geometry as the resistance mat-vec):
//   k_btw_init        dist[s][b] = 0, sigma[s][b] = 1 for the source s of column b; a duplicated source has a column of its own
//   k_btw_forward     level L: for every column b of row v with dist[v][b] == -1 the sum of sigma[w][b] over the neighbours w
//                     with dist[w][b] == L - 1; where one matched (the sum is positive: sigma >= 1) dist[v][b] = L and sigma[v][b]
//                     = the sum.  A row whose columns are all reached returns after its own 64 bytes of dist.  The number of
//                     newly reached (node, column) entries and the largest sigma go to the control block with integer atomics
//                     (a non-negative double orders as its bit pattern).
//   k_btw_backward    level l: for every column of row v with dist[v][b] == l, acc = sum over the neighbours w with dist[w][b]
//                     == l + 1 of (1 + delta[w][b]) / sigma[w][b], delta[v][b] = sigma[v][b] acc.  With edge values the slot v -> w
//                     adds sigma[v][b] (1 + delta[w][b]) / sigma[w][b], summed over the 16 columns by a butterfly over the eight
//                     lanes of the slot, to slot_acc[slot]: by the row that owns the slot, so without atomics.  A row with no
//                     column at level l returns after its own 64 bytes of dist.
//   k_btw_accumulate  node_acc[v] += sum of delta[v][b] over the columns, the column of a source skipped at the source itself:
//                     the two columns of a lane, then the butterfly over the eight lanes
//
// In place.  k_btw_forward reads and writes dist and sigma in one launch.  Row v alone writes dist[v][b] and sigma[v][b], and only
// where dist[v][b] is -1.  A reader compares dist[v][b] with L - 1: whether it sees -1 or L there, neither matches, so it does
// not read sigma[v][b], which level L + 1 reads first, in a later launch.  k_btw_backward at level l reads delta, sigma and dist of
// nodes at level l + 1, which an earlier launch wrote, and writes delta[v][b] only where dist[v][b] == l, which no row of the
// launch reads.  slot_acc[slot] is read and written by the row that owns the slot only.
//
// Order of the sums.  A lane adds its slots of a row in slot order, the lanes of a scope are added by the scope's butterfly, the
// columns by the butterfly over the eight lanes of a node, the batches in call order: the graph and the call fix every order, and
// two calls on the same graph return the same bits.
//
// The host runs the forward levels as HopRun::batch does: per level one launch and one download of the control block, until a
// level reaches nothing.  The backward levels and the accumulation follow back to back without a synchronisation in between.  No
// kernel waits for another workgroup.
#include <algorithm>
#include <cmath>

#include "dcr_analysis.h"

namespace dcr {

constexpr int BTW_B = 16;                // sources (columns) of a batch
constexpr int BTW_CP = BTW_B / 2;        // lanes across a node: two columns each
constexpr int BTW_SHORT_LANES = 32;      // lanes of a short row's group
constexpr int BTW_SHORT_ROWS = 64;       // short rows a workgroup takes: 8 groups x 8 turns
using BtwRows = RowGeom<BTW_SHORT_LANES, BTW_SHORT_ROWS / 8, BTW_CP>;
constexpr int BTW_ACC_BLOCKS = 1024;     // most workgroups of k_btw_accumulate

struct BtwCtl {
    unsigned long long reached;     // (node, column) entries the forward levels of the batch have reached, the sources not counted
    unsigned long long sigma_bits;  // the bits of the largest sigma of the call so far
    int32_t src[BTW_B];             // the source of each column; -1: padding
};

__device__ inline int2 btw_ldi(const int32_t *base, int64_t node, int cp) { return *reinterpret_cast<const int2 *>(base + node * BTW_B + 2 * cp); }
__device__ inline double2 btw_ld2(const double *base, int64_t node, int cp) {
    return *reinterpret_cast<const double2 *>(base + node * BTW_B + 2 * cp);
}

// true in all eight lanes of a node where it is true in one of them
__device__ inline bool node_any(bool x) {
    int f = x ? 1 : 0;
#pragma unroll
    for (int off = BTW_CP / 2; off >= 1; off >>= 1) f |= __shfl_xor(f, off);
    return f != 0;
}

__global__ void __launch_bounds__(64) k_btw_init(const BtwCtl *__restrict__ ctl, int32_t *dist, double *sigma) {
    const int b = threadIdx.x;
    if (b >= BTW_B) return;
    const int64_t s = ctl->src[b];
    if (s < 0) return;
    dist[s * BTW_B + b] = 0;
    sigma[s * BTW_B + b] = 1.0;
}

// used: the columns of the batch that hold a source; the others stay -1 everywhere and keep no row open
__global__ void __launch_bounds__(256) k_btw_forward(RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                      int32_t level, int used, int32_t *dist, double *sigma, BtwCtl *ctl) {
    __shared__ double2 sh[4 * BTW_CP];
    const int cp = threadIdx.x % BTW_CP;
    int fresh = 0;      // entries this thread has reached
    double top = 0.0;   // the largest sigma it has written
    walk_rows<BtwRows>(plan, rowinfo, sh, [=](auto scope, int32_t v, int2 ri, int &fresh, double &top) {
        const int2 dv = btw_ldi(dist, v, cp);
        const bool open0 = dv.x < 0 && 2 * cp < used, open1 = dv.y < 0 && 2 * cp + 1 < used;
        if (!node_any(open0 || open1)) return;  // the same in every lane of the scope: all of them read this row's dist
        const int32_t want = level - 1;
        double2 acc = make_double2(0.0, 0.0);
        for (int j = scope.first(); j < ri.y; j += scope.stride) {
            const int32_t w = col[ri.x + j];
            const int2 dw = btw_ldi(dist, w, cp);
            if (dw.x != want && dw.y != want) continue;
            const double2 sw = btw_ld2(sigma, w, cp);
            if (dw.x == want) acc.x += sw.x;
            if (dw.y == want) acc.y += sw.y;
        }
        acc = scope.sum(acc);
        if (!scope.owner()) return;
        if (open0 && acc.x > 0.0) {
            dist[(int64_t)v * BTW_B + 2 * cp] = level;
            sigma[(int64_t)v * BTW_B + 2 * cp] = acc.x;
            top = fmax(top, acc.x);
            ++fresh;
        }
        if (open1 && acc.y > 0.0) {
            dist[(int64_t)v * BTW_B + 2 * cp + 1] = level;
            sigma[(int64_t)v * BTW_B + 2 * cp + 1] = acc.y;
            top = fmax(top, acc.y);
            ++fresh;
        }
    }, fresh, top);
    fresh = wave_sum(fresh);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) top = fmax(top, __shfl_xor(top, off));
    if ((threadIdx.x & 63) == 0 && fresh > 0) {
        atomicAdd(&ctl->reached, (unsigned long long)fresh);
        atomicMax(&ctl->sigma_bits, (unsigned long long)__double_as_longlong(top));
    }
}

template <bool EDGES>
__global__ void __launch_bounds__(256) k_btw_backward(RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                       int32_t level, const int32_t *__restrict__ dist, const double *__restrict__ sigma,
                                                       double *delta, double *slot_acc) {
    __shared__ double2 sh[4 * BTW_CP];
    const int cp = threadIdx.x % BTW_CP;
    walk_rows<BtwRows>(plan, rowinfo, sh, [=](auto scope, int32_t v, int2 ri) {
        const int2 dv = btw_ldi(dist, v, cp);
        const bool at0 = dv.x == level, at1 = dv.y == level;
        if (!node_any(at0 || at1)) return;  // the same in every lane of the scope
        const double2 sv = btw_ld2(sigma, v, cp);  // read only where at0 / at1
        const int32_t want = level + 1;
        double2 acc = make_double2(0.0, 0.0);
        for (int j = scope.first(); j < ri.y; j += scope.stride) {  // the eight lanes of a slot run this loop together
            const int32_t w = col[ri.x + j];
            const int2 dw = btw_ldi(dist, w, cp);
            const bool m0 = at0 && dw.x == want, m1 = at1 && dw.y == want;
            double2 t = make_double2(0.0, 0.0);
            if (m0 || m1) {
                const double2 sw = btw_ld2(sigma, w, cp), dl = btw_ld2(delta, w, cp);
                if (m0) t.x = (1.0 + dl.x) / sw.x;
                if (m1) t.y = (1.0 + dl.y) / sw.y;
            }
            acc.x += t.x;
            acc.y += t.y;
            if (EDGES) {
                const double e = group_sum<BTW_CP, 1>((m0 ? sv.x * t.x : 0.0) + (m1 ? sv.y * t.y : 0.0));
                if (cp == 0 && e > 0.0) slot_acc[ri.x + j] += e;
            }
        }
        acc = scope.sum(acc);
        if (!scope.owner()) return;
        if (at0) delta[(int64_t)v * BTW_B + 2 * cp] = sv.x * acc.x;
        if (at1) delta[(int64_t)v * BTW_B + 2 * cp + 1] = sv.y * acc.y;
    });
}

__global__ void __launch_bounds__(256) k_btw_accumulate(int64_t n, const BtwCtl *__restrict__ ctl, const double *__restrict__ delta,
                                                         double *node_acc) {
    const int cp = threadIdx.x % BTW_CP;
    const int32_t s0 = ctl->src[2 * cp], s1 = ctl->src[2 * cp + 1];
    const int64_t total = n * BTW_CP;  // the eight lanes of a node stay together: 256 is a multiple of BTW_CP
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t node = e / BTW_CP;
        const double2 d = btw_ld2(delta, node, cp);
        const double x = group_sum<BTW_CP, 1>((node == s0 ? 0.0 : d.x) + (node == s1 ? 0.0 : d.y));
        if (cp == 0) node_acc[node] += x;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct BtwRun {
    dcr_graph *g;
    int64_t n;
    RowPlan plan;
    std::vector<int2> info;  // rowinfo on the host
    int32_t *dist;
    double *sigma, *delta, *node_acc, *slot_acc;  // slot_acc: nullptr without edge values
    BtwCtl *ctl;
    int32_t levels_max = 0;
    int32_t batches = 0;
    double sigma_max = 0.0;

    int setup(bool want_edges) {
        n = g->n;
        AnalysisState &A = analysis_of(g);
        DCR_TRY(A.btw_dist.grow(n * BTW_B));
        DCR_TRY(A.btw_f64.grow(2 * n * BTW_B + n));
        DCR_TRY(A.btw_ctl.grow((int64_t)sizeof(BtwCtl)));
        if (want_edges) DCR_TRY(A.btw_slot.grow(g->cap_total));
        dist = A.btw_dist.p;
        sigma = A.btw_f64.p;  // 16-byte aligned each
        delta = sigma + n * BTW_B;
        node_acc = delta + n * BTW_B;
        slot_acc = want_edges ? A.btw_slot.p : nullptr;
        ctl = reinterpret_cast<BtwCtl *>(A.btw_ctl.p);
        DCR_TRY(build_row_plan(g, &plan, &info));
        hipStream_t st = g->stream;
        DCR_HIP(hipMemsetAsync(node_acc, 0, sizeof(double) * (size_t)n, st));
        if (slot_acc && g->cap_total > 0) DCR_HIP(hipMemsetAsync(slot_acc, 0, sizeof(double) * (size_t)g->cap_total, st));
        return DCR_OK;
    }

    // B sources (sources, or the nodes first, first + 1, ... where it is nullptr) as one batch
    int batch(const int32_t *sources, int64_t first, int B) {
        hipStream_t st = g->stream;
        BtwCtl h;
        h.reached = 0;
        h.sigma_bits = 0x3ff0000000000000ull;  // 1.0, the sigma of a source
        if (sigma_max > 1.0) std::memcpy(&h.sigma_bits, &sigma_max, sizeof(double));
        for (int b = 0; b < BTW_B; ++b) h.src[b] = b >= B ? -1 : sources ? sources[b] : (int32_t)(first + b);
        DCR_HIP(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, st));
        DCR_HIP(hipMemsetAsync(dist, 0xff, sizeof(int32_t) * (size_t)(n * BTW_B), st));
        DCR_HIP(hipMemsetAsync(delta, 0, sizeof(double) * (size_t)(n * BTW_B), st));
        hipLaunchKernelGGL(k_btw_init, dim3(1), dim3(64), 0, st, ctl, dist, sigma);
        DCR_HIP(hipGetLastError());

        const dim3 grid(row_grid<BtwRows>(plan));
        int64_t last = 0;  // the last level that holds a node
        unsigned long long before = 0;
        for (int64_t level = 1;; ++level) {
            if (level > n) DCR_FAIL(DCR_ESTATE, "betweenness: more levels than nodes");
            hipLaunchKernelGGL(k_btw_forward, grid, dim3(256), 0, st, plan, g->rowinfo.p, g->col.p, (int32_t)level, B, dist, sigma, ctl);
            DCR_HIP(hipGetLastError());
            DCR_HIP(hipMemcpyAsync(&h, ctl, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            DCR_HIP(hipStreamSynchronize(st));
            if (h.reached == before) break;
            before = h.reached;
            last = level;
        }
        std::memcpy(&sigma_max, &h.sigma_bits, sizeof(double));
        if (!(sigma_max <= 1.79769313486231570815e308))
            DCR_FAIL(DCR_ESTATE, "betweenness: the number of shortest paths of a pair exceeds the float64 range");
        for (int64_t level = last - 1; level >= 0; --level) {
            if (slot_acc)
                hipLaunchKernelGGL(k_btw_backward<true>, grid, dim3(256), 0, st, plan, g->rowinfo.p, g->col.p, (int32_t)level, dist, sigma, delta,
                                   slot_acc);
            else
                hipLaunchKernelGGL(k_btw_backward<false>, grid, dim3(256), 0, st, plan, g->rowinfo.p, g->col.p, (int32_t)level, dist, sigma, delta,
                                   slot_acc);
        }
        hipLaunchKernelGGL(k_btw_accumulate, dim3(std::min(blocks_of(n * BTW_CP), (unsigned)BTW_ACC_BLOCKS)), dim3(256), 0, st, n, ctl, delta,
                           node_acc);
        DCR_HIP(hipGetLastError());
        levels_max = std::max(levels_max, (int32_t)last);
        ++batches;
        return DCR_OK;
    }

    // edge {u, v} = slot_acc[u -> v] + slot_acc[v -> u], in the order and orientation of dcr_graph_edges (row by row, the slots with
    // col > row).  The slot v -> u of an edge u < v comes from the list of such slots grouped by u (a counting sort): O(n + E).
    int edges_out(double *out_edge) {
        hipStream_t st = g->stream;
        const int64_t cap = g->cap_total;
        std::vector<int32_t> col((size_t)cap);
        std::vector<double> acc((size_t)cap);
        if (cap > 0) {
            DCR_HIP(hipMemcpyAsync(col.data(), g->col.p, sizeof(int32_t) * (size_t)cap, hipMemcpyDeviceToHost, st));
            DCR_HIP(hipMemcpyAsync(acc.data(), slot_acc, sizeof(double) * (size_t)cap, hipMemcpyDeviceToHost, st));
        }
        DCR_HIP(hipStreamSynchronize(st));
        std::vector<int64_t> start((size_t)n + 1, 0);  // the slots v -> u with u < v, grouped by u
        for (int64_t v = 0; v < n; ++v)
            for (int32_t i = 0; i < info[(size_t)v].y; ++i) {
                const int32_t u = col[(size_t)info[(size_t)v].x + i];
                if (u < v) ++start[(size_t)u + 1];
            }
        for (int64_t u = 0; u < n; ++u) start[(size_t)u + 1] += start[(size_t)u];
        std::vector<int64_t> back_slot((size_t)start[(size_t)n]), fill(start.begin(), start.end() - 1);
        std::vector<int32_t> back_row((size_t)start[(size_t)n]);
        for (int64_t v = 0; v < n; ++v)
            for (int32_t i = 0; i < info[(size_t)v].y; ++i) {
                const int64_t slot = (int64_t)info[(size_t)v].x + i;
                const int32_t u = col[(size_t)slot];
                if (u >= v) continue;
                const int64_t k = fill[(size_t)u]++;
                back_slot[(size_t)k] = slot;
                back_row[(size_t)k] = (int32_t)v;
            }
        std::vector<int64_t> mate((size_t)n, -1);  // mate[v]: the slot v -> u for the row u at hand
        int64_t p = 0;
        for (int64_t u = 0; u < n; ++u) {
            for (int64_t k = start[(size_t)u]; k < start[(size_t)u + 1]; ++k) mate[(size_t)back_row[(size_t)k]] = back_slot[(size_t)k];
            for (int32_t i = 0; i < info[(size_t)u].y; ++i) {
                const int64_t slot = (int64_t)info[(size_t)u].x + i;
                const int32_t v = col[(size_t)slot];
                if (v <= u) continue;
                if (p >= g->n_edges || mate[(size_t)v] < 0) DCR_FAIL(DCR_ESTATE, "betweenness: the adjacency is not symmetric");
                out_edge[p++] = acc[(size_t)slot] + acc[(size_t)mate[(size_t)v]];
                mate[(size_t)v] = -1;
            }
        }
        if (p != g->n_edges) DCR_FAIL(DCR_ESTATE, "edge count drifted");
        return DCR_OK;
    }
};

}  // namespace dcr

using namespace dcr;

extern "C" {

int dcr_betweenness(dcr_graph *g, const int32_t *sources, int64_t P, double *out_node, double *out_edge, dcr_betweenness_info *out_info) {
    if (!g) DCR_FAIL(DCR_EINVAL, "null graph");
    if (!out_node) DCR_FAIL(DCR_EINVAL, "null argument");
    if (P < 0) DCR_FAIL(DCR_EINVAL, "negative source count");
    if (!sources && P != g->n) DCR_FAIL(DCR_EINVAL, "sources NULL stands for every node: P must be num_nodes");
    if (sources)
        for (int64_t i = 0; i < P; ++i)
            if (sources[i] < 0 || sources[i] >= g->n) DCR_FAIL(DCR_EINVAL, "source outside 0 .. num_nodes - 1");
    if (out_info) *out_info = dcr_betweenness_info{0, 0, 0.0};
    if (P == 0) {  // an empty sum
        std::fill(out_node, out_node + g->n, 0.0);
        if (out_edge) std::fill(out_edge, out_edge + g->n_edges, 0.0);
        return DCR_OK;
    }
    DCR_HIP(hipSetDevice(g->device));
    BtwRun R;
    R.g = g;
    DCR_TRY(R.setup(out_edge != nullptr));
    for (int64_t first = 0; first < P; first += BTW_B)
        DCR_TRY(R.batch(sources ? sources + first : nullptr, first, (int)std::min<int64_t>(P - first, BTW_B)));
    DCR_HIP(hipMemcpyAsync(out_node, R.node_acc, sizeof(double) * (size_t)g->n, hipMemcpyDeviceToHost, g->stream));
    DCR_HIP(hipStreamSynchronize(g->stream));
    if (out_edge) DCR_TRY(R.edges_out(out_edge));
    if (out_info) *out_info = dcr_betweenness_info{R.levels_max, R.batches, R.sigma_max};
    return DCR_OK;
}

}  // extern "C"
