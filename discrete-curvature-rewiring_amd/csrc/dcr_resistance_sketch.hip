// Sketched effective resistance of every edge (and of given pairs) on the device-resident graph: Spielman and Srivastava's
// estimator with Rademacher signs.  include/dcr.h has the rule; tests/resistance_sketch_ref.py restates it in numpy.
//
// With B the incidence matrix (an edge oriented from its smaller to its larger endpoint), R(u, v) = |B L^+ (e_u - e_v)|^2.  For k
// sign vectors q_j in {-1, +1}^E:  b_j = B^T q_j,  L z_j = b_j,  R~(u, v) = 1/k sum_j (z_j[u] - z_j[v])^2.  In the normalised
// operator of dcr_resistance.hip the system is 𝓛 y_j = s ⊙ b_j with z_j = s ⊙ y_j, s = 1 / sqrt(deg): the batched column CG of
// dcr_analysis.h with SketchProblem below, COL_B columns a batch, up to SKT_MAX_GROUPS batches a launch as blockIdx.y.  Z (k x n)
// is never stored: after every launch of groups the squared differences go into one float64 per adjacency slot and per pair.
//
// The sign of edge {lo, hi}, lo < hi, in column COL_B b + i is bit i of word 0 of philox4x32_10(lo | hi << 32, 0x5253 << 48 | b,
// seed), a 0 meaning +1: keyed by the endpoints, so a row finds the sign of each of its slots by itself and the signs move with
// neither the row order nor an edit elsewhere in the graph.
//
// Kernels (rows through walk_rows<ColRows>, the geometry of the column CG's mat-vec; no floating-point atomics):
//   k_sketch_rhs         per row w the COL_CP lanes of a slot (w, x) draw the slot's Philox word (the same call in each of them: the
//                        lanes of a slot run in lockstep, a broadcast would save no cycle) and add (w < x ? +1 : -1) sign to their
//                        two columns; the scope's sum (integers in float64: exact in any order), then the owners store s_w b[w]
//                        (and b[w] itself for dcr_resistance_sketch_rhs) node-major and add (s_w b[w])^2 to the partials of |rhs|^2,
//                        which the last arriver closes into the control block.  Padding columns are written as zeros.
//   col_cg_solve<SketchProblem>   the solve; its closing launches leave z = s ⊙ y = z_j in the group's z vector and the true
//                        residual |s ⊙ b_j - 𝓛 y_j| per column in the control block
//   k_sketch_accumulate  per slot (w, x) with w < x, the slot G.edges() lists the edge at: sum over the groups of the launch, in
//                        batch order, and over the columns (the lane's two, then the butterfly over the COL_CP lanes) of
//                        (z[w] - z[x])^2, one 128-byte gather of z[x] a group; added to slot_acc[slot] by the row that owns the slot.
//                        The slots x -> w hold the same value mathematically and are skipped.
//   k_sketch_pairs       the same sum for each given pair into pair_acc[i]
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "dcr_analysis.h"
#include "dcr_philox.h"

namespace dcr {

constexpr int SKT_MAX_GROUPS = 4;           // batches solved side by side in the same launches: 64 columns a launch
constexpr int64_t SKT_GROUP_NODES = 65536;  // as many groups as keep groups x nodes within this (the rule of dcr_diffusion.hip)
constexpr uint64_t SKT_STREAM = 0x5253ull << 48;  // the Philox offset of batch b is SKT_STREAM | b
constexpr int SKT_PAIR_BLOCKS = 1024;       // most workgroups of k_sketch_pairs

struct SktCtl {
    ColCg cg;
    double cc[COL_B];     // |s ⊙ b|^2 (k_sketch_rhs)
    double resid[COL_B];  // the closing mat-vec's |s ⊙ b - 𝓛 y|_2
    double tol;
    int32_t used;         // columns of the batch that hold a sign vector; the others are padding
    int32_t pad_;
};

struct SketchProblem {  // 𝓛 y = s ⊙ b for the column CG of dcr_analysis.h
    using Ctl = SktCtl;
    static constexpr bool closing_dot = false;  // the residual alone
    SktCtl *ctl;
    const double *c;  // group 0's right-hand side [n][COL_B]
    int64_t gstride;
    __device__ auto rhs(int cp) const {
        const double *mine = c + (int64_t)blockIdx.y * gstride;
        return [=](int32_t node, double) { return ld2(mine, node, cp); };
    }
    __device__ auto entry() const {  // a zero row at an isolated node
        return [](int deg, double x, double su, double acc, double) { return deg > 0 ? x - su * acc : 0.0; };
    }
    __device__ void start(int k, const double *) const {  // the column stops at |r| <= tol |rhs|; an all-zero one starts frozen
        const double cc = ctl->cc[k];
        ctl->cg.rr[k] = cc;
        ctl->cg.stop[k] = ctl->tol * sqrt(cc);
        if (!(cc > 0.0)) ctl->cg.frozen[k] = 1;
    }
    __device__ void close(int k, const double *, const double *, double, double dev) const { ctl->resid[k] = sqrt(dev); }
};

// groups blockIdx.y = 0 .. of batches batch0, batch0 + 1, ...; b_out: nullptr, or where group 0's integer b goes
__global__ void __launch_bounds__(256) k_sketch_rhs(RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                     const double *__restrict__ s, uint64_t seed, int64_t batch0, SktCtl *ctl,
                                                     double *__restrict__ c, double *__restrict__ b_out, double *part, int64_t gstride,
                                                     int64_t pstride) {
    __shared__ double2 sh[4 * COL_CP];
    const int t = threadIdx.x, cp = t % COL_CP;
    ctl += blockIdx.y, c += (int64_t)blockIdx.y * gstride, part += (int64_t)blockIdx.y * pstride;
    const uint64_t offset = SKT_STREAM | (uint64_t)(batch0 + blockIdx.y);
    const bool on0 = 2 * cp < ctl->used, on1 = 2 * cp + 1 < ctl->used;
    double2 cc = make_double2(0.0, 0.0);
    walk_rows<ColRows>(plan, rowinfo, sh, [=](auto scope, int32_t w, int2 ri, double2 &cc) {
        double2 acc = make_double2(0.0, 0.0);
        for (int j = scope.first(); j < ri.y; j += scope.stride) {
            const int32_t x = col[ri.x + j];
            const uint32_t lo = (uint32_t)(w < x ? w : x), hi = (uint32_t)(w < x ? x : w);
            uint32_t word[4];
            philox4x32_10((uint64_t)lo | (uint64_t)hi << 32, offset, seed, word);
            const double out = w < x ? 1.0 : -1.0;  // the edge leaves its smaller endpoint
            acc.x += (word[0] >> (2 * cp)) & 1u ? -out : out;
            acc.y += (word[0] >> (2 * cp + 1)) & 1u ? -out : out;
        }
        acc = scope.sum(acc);
        if (!scope.owner()) return;
        if (!on0) acc.x = 0.0;
        if (!on1) acc.y = 0.0;
        const double sw = s[w];
        const double2 cw = make_double2(sw * acc.x, sw * acc.y);
        st2(c, w, cp, cw);
        if (b_out) st2(b_out, w, cp, acc);
        cc.x += cw.x * cw.x;
        cc.y += cw.y * cw.y;
    }, cc);
    cc = block_sum<COL_CP>(cc, sh);
    if (t < COL_CP) store_partial(part, blockIdx.x, cc);
    if (!last_arriver(&ctl->cg.ticket, (unsigned)gridDim.x)) return;
    const double2 a = close_partials(part, gridDim.x, sh);
    if (t < COL_CP) {
        ctl->cc[2 * t] = a.x;
        ctl->cc[2 * t + 1] = a.y;
    }
    if (t == 0) __hip_atomic_store(&ctl->cg.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the lane's share of sum over the groups and its two columns of (z[a] - z[b])^2
__device__ inline double skt_diff2(const double *__restrict__ z, int ng, int64_t gstride, int32_t a, int32_t b, int cp) {
    double e = 0.0;
    for (int i = 0; i < ng; ++i) {
        const double2 za = ld2(z + i * gstride, a, cp), zb = ld2(z + i * gstride, b, cp);
        const double d0 = za.x - zb.x, d1 = za.y - zb.y;
        e += d0 * d0 + d1 * d1;
    }
    return e;
}

__global__ void __launch_bounds__(256) k_sketch_accumulate(RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                            const double *__restrict__ z, int ng, int64_t gstride, double *slot_acc) {
    __shared__ double2 sh[4 * COL_CP];
    const int cp = threadIdx.x % COL_CP;
    walk_rows<ColRows>(plan, rowinfo, sh, [=](auto scope, int32_t w, int2 ri) {
        for (int j = scope.first(); j < ri.y; j += scope.stride) {  // the COL_CP lanes of a slot run this loop together
            const int32_t x = col[ri.x + j];
            if (x < w) continue;  // the edge is kept at the slot of its smaller endpoint
            const double e = group_sum<COL_CP, 1>(skt_diff2(z, ng, gstride, w, x, cp));
            if (cp == 0) slot_acc[ri.x + j] += e;
        }
    });
}

__global__ void __launch_bounds__(256) k_sketch_pairs(const int32_t *__restrict__ u, const int32_t *__restrict__ v, int64_t P,
                                                       const double *__restrict__ z, int ng, int64_t gstride, double *pair_acc) {
    const int cp = threadIdx.x % COL_CP;
    const int64_t total = P * COL_CP;  // the COL_CP lanes of a pair stay together: 256 is a multiple of COL_CP
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / COL_CP;
        const double x = group_sum<COL_CP, 1>(skt_diff2(z, ng, gstride, u[i], v[i], cp));
        if (cp == 0) pair_acc[i] += x;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
static int sketch_groups(int64_t n, int64_t batches) {
    int64_t cap = SKT_MAX_GROUPS;
    if (const char *e = getenv("DCR_SKETCH_GROUPS")) {  // for tools/probe_resistance_sketch.py: 1 .. SKT_MAX_GROUPS
        const int w = atoi(e);
        if (w >= 1 && w <= SKT_MAX_GROUPS) cap = w;
    }
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(cap, batches), SKT_GROUP_NODES / std::max<int64_t>(n, 1)));
}

struct SketchRun {
    dcr_graph *g;
    int64_t n;
    RowPlan plan;
    std::vector<int2> info;  // rowinfo on the host
    int groups;
    ColLayout L;
    SketchProblem prob;
    double *c, *slot_acc, *pair_acc;
    int32_t *pair_u, *pair_v;

    // buffers for `groups` batches side by side; slot and pair accumulators only where asked for, cleared
    int setup(int64_t batches, bool want_edges, const int32_t *u, const int32_t *v, int64_t P) {
        n = g->n;
        DCR_TRY(build_row_plan(g, &plan, &info));
        groups = sketch_groups(n, batches);
        const int nb_mv = (int)row_grid<ColRows>(plan);
        const int nb_el = (int)std::min<int64_t>(COL_UPDATE_BLOCKS, blocks_of(n * COL_CP));
        const int64_t gstride = 6 * n * COL_B, pstride = (int64_t)COL_B * std::max(nb_mv, nb_el);
        AnalysisState &A = analysis_of(g);
        DCR_TRY(A.skt_vec.grow(n + groups * gstride));
        DCR_TRY(A.skt_part.grow(groups * pstride));
        DCR_TRY(A.skt_ctl.grow((int64_t)sizeof(SktCtl) * groups));
        double *z = A.skt_vec.p, *p = z + n * COL_B, *r = p + n * COL_B, *y = r + n * COL_B, *q = y + n * COL_B;  // 16-byte aligned each
        c = q + n * COL_B;
        double *s = z + groups * gstride;
        L = ColLayout{z, p, r, y, q, s, A.skt_part.p, gstride, pstride, nb_mv, nb_el};
        prob = SketchProblem{reinterpret_cast<SktCtl *>(A.skt_ctl.p), c, gstride};
        hipStream_t st = g->stream;
        inv_sqrt_degree(g, s);
        DCR_HIP(hipGetLastError());
        slot_acc = pair_acc = nullptr;
        pair_u = pair_v = nullptr;
        if (want_edges && g->cap_total > 0) {
            DCR_TRY(A.skt_slot.grow(g->cap_total));
            slot_acc = A.skt_slot.p;
            DCR_HIP(hipMemsetAsync(slot_acc, 0, sizeof(double) * (size_t)g->cap_total, st));
        }
        if (P > 0) {
            DCR_TRY(A.skt_pair.grow(P));
            DCR_TRY(A.skt_pair_idx.grow(2 * P));
            pair_acc = A.skt_pair.p;
            pair_u = A.skt_pair_idx.p;
            pair_v = pair_u + P;
            DCR_HIP(hipMemsetAsync(pair_acc, 0, sizeof(double) * (size_t)P, st));
            DCR_HIP(hipMemcpyAsync(pair_u, u, sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, st));
            DCR_HIP(hipMemcpyAsync(pair_v, v, sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, st));
            DCR_HIP(hipStreamSynchronize(st));  // u and v are the caller's
        }
        return DCR_OK;
    }

    // the control blocks of batches first .. first + ng - 1 of a sketch of `columns` columns, and their right-hand sides
    int rhs(uint64_t seed, int64_t first, int ng, int64_t columns, double tol, std::vector<SktCtl> &h, double *b_out) {
        std::memset(h.data(), 0, sizeof(SktCtl) * (size_t)ng);
        for (int i = 0; i < ng; ++i) {
            SktCtl &hc = h[(size_t)i];
            hc.tol = tol;
            hc.used = (int32_t)std::min<int64_t>(COL_B, columns - (first + i) * COL_B);
            for (int k = hc.used; k < COL_B; ++k) hc.cg.frozen[k] = 1;  // padding columns start frozen
            hc.cg.active = hc.used;
        }
        DCR_HIP(hipMemcpyAsync(prob.ctl, h.data(), sizeof(SktCtl) * (size_t)ng, hipMemcpyHostToDevice, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));  // h is reused by the solve
        hipLaunchKernelGGL(k_sketch_rhs, dim3((unsigned)L.nb_mv, (unsigned)ng), dim3(256), 0, g->stream, plan, g->rowinfo.p, g->col.p, L.s, seed,
                           first, prob.ctl, c, b_out, L.part, L.gstride, L.pstride);
        DCR_HIP(hipGetLastError());
        return DCR_OK;
    }

    // edge {u, v}, u < v, from the slot u -> v: the order and orientation of dcr_graph_edges (row by row, the slots with col > row)
    int edges_out(double *out_edge, double scale) {
        const int64_t cap = g->cap_total;
        std::vector<int32_t> col((size_t)cap);
        std::vector<double> acc((size_t)cap);
        if (cap > 0) {
            DCR_HIP(hipMemcpyAsync(col.data(), g->col.p, sizeof(int32_t) * (size_t)cap, hipMemcpyDeviceToHost, g->stream));
            DCR_HIP(hipMemcpyAsync(acc.data(), slot_acc, sizeof(double) * (size_t)cap, hipMemcpyDeviceToHost, g->stream));
        }
        DCR_HIP(hipStreamSynchronize(g->stream));
        int64_t p = 0;
        for (int64_t u = 0; u < n; ++u)
            for (int32_t i = 0; i < info[(size_t)u].y; ++i) {
                const int64_t slot = (int64_t)info[(size_t)u].x + i;
                if (col[(size_t)slot] <= u) continue;
                if (p >= g->n_edges) DCR_FAIL(DCR_ESTATE, "resistance sketch: the adjacency is not symmetric");
                out_edge[p++] = acc[(size_t)slot] / scale;
            }
        if (p != g->n_edges) DCR_FAIL(DCR_ESTATE, "edge count drifted");
        return DCR_OK;
    }
};

}  // namespace dcr

using namespace dcr;

extern "C" {

int dcr_resistance_sketch(dcr_graph *g, const dcr_sketch_opts *opts, double *out_edge, const int32_t *u, const int32_t *v, int64_t P,
                          double *out_pair, double *out_residual, dcr_sketch_info *out_info) {
    if (!g) DCR_FAIL(DCR_EINVAL, "null graph");
    dcr_sketch_opts o = {256, 0, 1e-6, 20000};
    if (opts) o = *opts;
    if (o.columns < 1) DCR_FAIL(DCR_EINVAL, "columns must be >= 1");
    if (!(o.tol >= 0.0) || o.max_steps < 1) DCR_FAIL(DCR_EINVAL, "tol must be >= 0, max_steps >= 1");
    if (P < 0) DCR_FAIL(DCR_EINVAL, "the number of pairs must be >= 0");
    if (P > 0 && (!u || !v || !out_pair)) DCR_FAIL(DCR_EINVAL, "null argument");
    for (int64_t i = 0; i < P; ++i)
        if (u[i] < 0 || u[i] >= g->n || v[i] < 0 || v[i] >= g->n) DCR_FAIL(DCR_EINVAL, "pair " + std::to_string(i) + ": endpoint outside 0 .. num_nodes - 1");
    const int64_t k = o.columns, batches = (k + COL_B - 1) / COL_B;
    dcr_sketch_info info = {o.columns, (int32_t)batches, 0, 0.0};
    if (out_info) *out_info = info;
    if (out_residual) std::fill(out_residual, out_residual + k, 0.0);
    DCR_HIP(hipSetDevice(g->device));

    // decided from the components alone, as dcr_effective_resistance does: the same node, or no path between the two
    std::vector<int32_t> labels;
    if (P > 0) DCR_TRY(graph_components(g, labels));
    const bool solve = g->n_edges > 0 && (out_edge || P > 0 || out_residual || out_info);  // without an edge every b is zero
    SketchRun R;
    R.g = g;
    if (solve) {
        DCR_TRY(R.setup(batches, out_edge != nullptr, u, v, P));
        std::vector<SktCtl> h((size_t)R.groups);
        hipStream_t st = g->stream;
        for (int64_t first = 0; first < batches; first += R.groups) {
            const int ng = (int)std::min<int64_t>(R.groups, batches - first);
            DCR_TRY(R.rhs(o.seed, first, ng, k, o.tol, h, nullptr));
            DCR_TRY(col_cg_solve(g, R.plan, R.L, ng, R.prob, h.data(), o.max_steps));
            if (R.slot_acc)
                hipLaunchKernelGGL(k_sketch_accumulate, dim3((unsigned)R.L.nb_mv), dim3(256), 0, st, R.plan, g->rowinfo.p, g->col.p, R.L.z, ng,
                                   R.L.gstride, R.slot_acc);
            if (P > 0)
                hipLaunchKernelGGL(k_sketch_pairs, dim3(std::min(blocks_of(P * COL_CP), (unsigned)SKT_PAIR_BLOCKS)), dim3(256), 0, st, R.pair_u,
                                   R.pair_v, P, R.L.z, ng, R.L.gstride, R.pair_acc);
            DCR_HIP(hipGetLastError());
            DCR_HIP(hipMemcpyAsync(h.data(), R.prob.ctl, sizeof(SktCtl) * (size_t)ng, hipMemcpyDeviceToHost, st));
            DCR_HIP(hipStreamSynchronize(st));
            for (int i = 0; i < ng; ++i)
                for (int c = 0; c < h[(size_t)i].used; ++c) {
                    const double resid = h[(size_t)i].resid[c];
                    if (out_residual) out_residual[(first + i) * COL_B + c] = resid;
                    info.steps_total += h[(size_t)i].cg.steps[c];
                    if (!(resid <= info.residual_max)) info.residual_max = resid;  // a NaN shows
                }
        }
        if (out_edge) DCR_TRY(R.edges_out(out_edge, (double)k));
        if (P > 0) {
            DCR_HIP(hipMemcpyAsync(out_pair, R.pair_acc, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, st));
            DCR_HIP(hipStreamSynchronize(st));
        }
    }
    for (int64_t i = 0; i < P; ++i) {
        if (u[i] == v[i])
            out_pair[i] = 0.0;
        else if (labels[(size_t)u[i]] != labels[(size_t)v[i]])
            out_pair[i] = INFINITY;
        else
            out_pair[i] /= (double)k;
    }
    if (out_info) *out_info = info;
    return DCR_OK;
}

int dcr_resistance_sketch_rhs(dcr_graph *g, uint64_t seed, int64_t batch, double *out) {
    if (!g || !out) DCR_FAIL(DCR_EINVAL, "null argument");
    if (batch < 0 || batch >= (int64_t)1 << 48) DCR_FAIL(DCR_EINVAL, "batch must be in 0 .. 2^48 - 1");
    if (g->n == 0) return DCR_OK;
    DCR_HIP(hipSetDevice(g->device));
    SketchRun R;
    R.g = g;
    DCR_TRY(R.setup(1, false, nullptr, nullptr, 0));
    std::vector<SktCtl> h(1);
    DCR_TRY(R.rhs(seed, batch, 1, (batch + 1) * COL_B, 0.0, h, R.L.z));  // every column of the batch holds a sign vector
    DCR_HIP(hipMemcpyAsync(out, R.L.z, sizeof(double) * (size_t)(g->n * COL_B), hipMemcpyDeviceToHost, g->stream));
    DCR_HIP(hipStreamSynchronize(g->stream));
    return DCR_OK;
}

}  // extern "C"
