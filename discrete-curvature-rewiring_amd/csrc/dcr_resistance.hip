// Effective resistance of node pairs on the device-resident graph.
//
// R(u, v) = (e_u - e_v)^T L^+ (e_u - e_v), L = D - A.  In the normalised operator the spectral code uses, 𝓛 = I - Â with
// Â = D^-1/2 A D^-1/2 (a zero row at an isolated node), and c = s_u e_u - s_v e_v, s = 1 / sqrt(deg), the same number is
// R = c^T 𝓛^+ c = c^T y* with 𝓛 y* = c: c is orthogonal to 𝓛's null space whenever u and v share a component.  The solve is
// conjugate gradients on 𝓛 from y = 0, i.e. Jacobi-preconditioned CG on L.  What is returned is not c^T y but
//     lower = 2 c^T y - y^T 𝓛 y            for the y the iteration ended with,
// because R - lower = (y* - y)^T 𝓛 (y* - y) >= 0 for ANY y: a lower bound also when the solve was cut short, and
// R - lower = r^T 𝓛^+ r <= |r|^2 / lambda_1 with the true residual r = c - 𝓛 y.  lower and |r|_2 come from one extra mat-vec on y
// at the end, not from the recurrences.
//
// COL_B pairs are solved at a time by the batched column CG of dcr_analysis.h (the layout, the freeze rule and why a column's bits
// depend on its own pair only are described there), in one group.  ResProblem below is all this file adds to it: the operator's
// row entry x - s ⊙ (A z), zero at an isolated node; c as the right-hand side; the stop threshold tol |c|; and what the close makes of the closing mat-vec's two sums.
//
// Kernels (dcr_analysis.h; the iterate x there is y here):
//   k_col_start<ResProblem>      r = p = c, z = s ⊙ p, y = 0 for all columns; |c|^2 and tol |c| per column
//   k_col_matvec<ResProblem, 0>  q = 𝓛 p = p - s ⊙ (A z); the last arriver sets the step length |r|^2 / p^T q or freezes the column
//   k_col_update<ResCtl>         y += gain p, r -= gain q; the last arriver sets beta, counts the step and freezes what has converged
//   k_col_direction<ResCtl>      p = r + beta p, z = s ⊙ p
//   k_col_scale                  z = s ⊙ y, then
//   k_col_matvec<ResProblem, 1>  w = 𝓛 y (not stored), partials of y^T w and |c - w|^2; the last arriver writes lower and |c - 𝓛 y|_2
// Three launches a step; the host synchronises every SP_CHECK_EVERY steps to read the control block (col_cg_solve).
#include <algorithm>
#include <cmath>

#include "dcr_analysis.h"

namespace dcr {

struct ResCtl {
    ColCg cg;
    double cc[COL_B];                   // |c|^2
    double lower[COL_B], resid[COL_B];  // the closing mat-vec's results
    double tol;
    int32_t u[COL_B], v[COL_B];         // the pair of each column; -1: padding
};

// the entry of c = s_u e_u - s_v e_v at `node` for the column of pair (u, v)
__device__ inline double c_entry(int32_t node, int32_t u, int32_t v, double s_node) { return node == u ? s_node : node == v ? -s_node : 0.0; }

struct ResProblem {  // 𝓛 y = c for the column CG of dcr_analysis.h
    using Ctl = ResCtl;
    static constexpr bool closing_dot = true;  // lower needs y^T 𝓛 y
    ResCtl *ctl;
    __device__ auto rhs(int cp) const {
        const int32_t u0 = ctl->u[2 * cp], v0 = ctl->v[2 * cp], u1 = ctl->u[2 * cp + 1], v1 = ctl->v[2 * cp + 1];
        return [=](int32_t node, double sn) { return make_double2(c_entry(node, u0, v0, sn), c_entry(node, u1, v1, sn)); };
    }
    __device__ auto entry() const {  // a zero row at an isolated node
        return [](int deg, double x, double su, double acc, double) { return deg > 0 ? x - su * acc : 0.0; };
    }
    __device__ void start(int k, const double *s) const {  // |c|^2, and the column stops at |r| <= tol |c|
        const int32_t u = ctl->u[k], v = ctl->v[k];
        const double su = u >= 0 ? s[u] : 0.0, sv = v >= 0 ? s[v] : 0.0;
        const double cc = su * su + sv * sv;
        ctl->cc[k] = cc;
        ctl->cg.rr[k] = cc;
        ctl->cg.stop[k] = ctl->tol * sqrt(cc);
    }
    __device__ void close(int k, const double *y, const double *s, double ywy, double dev) const {  // y^T 𝓛 y and |c - 𝓛 y|^2
        const int32_t u = ctl->u[k], v = ctl->v[k];
        double lower = 0.0, resid = 0.0;
        if (u >= 0) {
            const double cty = s[u] * y[(int64_t)u * COL_B + k] - s[v] * y[(int64_t)v * COL_B + k];
            lower = 2.0 * cty - ywy;
            resid = sqrt(dev);
        }
        ctl->lower[k] = lower;
        ctl->resid[k] = resid;
    }
};

// ---- host --------------------------------------------------------------------------------------------------------------------------
static int resistance_batches(dcr_graph *g, const int32_t *u, const int32_t *v, const std::vector<int64_t> &todo,
                              const dcr_resistance_opts &o, double *out_lower, double *out_residual, int32_t *out_steps) {
    const int64_t n = g->n;
    RowPlan plan;
    DCR_TRY(build_row_plan(g, &plan, nullptr));
    const int nb_mv = (int)row_grid<ColRows>(plan);
    const int nb_el = (int)std::min<int64_t>(COL_UPDATE_BLOCKS, blocks_of(n * COL_CP));

    AnalysisState &A = analysis_of(g);
    DCR_TRY(A.res_vec.grow(n + 5 * n * COL_B));
    DCR_TRY(A.res_part.grow((int64_t)COL_B * std::max(2 * nb_mv, nb_el)));
    DCR_TRY(A.res_ctl.grow((int64_t)sizeof(ResCtl)));
    double *z = A.res_vec.p, *p = z + n * COL_B, *r = p + n * COL_B, *y = r + n * COL_B, *q = y + n * COL_B;  // 16-byte aligned each
    double *s = q + n * COL_B;
    const ColLayout L = {z, p, r, y, q, s, A.res_part.p, 0, 0, nb_mv, nb_el};  // one group
    const ResProblem prob = {reinterpret_cast<ResCtl *>(A.res_ctl.p)};
    inv_sqrt_degree(g, s);
    DCR_HIP(hipGetLastError());

    ResCtl h;
    for (size_t first = 0; first < todo.size(); first += COL_B) {
        const int used = (int)std::min<size_t>(COL_B, todo.size() - first);
        std::memset(&h, 0, sizeof(h));
        h.tol = o.tol;
        for (int k = 0; k < COL_B; ++k) {
            const bool pad = k >= used;
            h.u[k] = pad ? -1 : u[todo[first + (size_t)k]];
            h.v[k] = pad ? -1 : v[todo[first + (size_t)k]];
            h.cg.frozen[k] = pad ? 1 : 0;  // padding columns start frozen
        }
        h.cg.active = used;
        DCR_HIP(hipMemcpyAsync(prob.ctl, &h, sizeof(h), hipMemcpyHostToDevice, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));  // h is reused below
        DCR_TRY(col_cg_solve(g, plan, L, 1, prob, &h, o.max_steps));
        DCR_HIP(hipMemcpyAsync(&h, prob.ctl, sizeof(h), hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));
        for (int k = 0; k < used; ++k) {
            const int64_t i = todo[first + (size_t)k];
            out_lower[i] = h.lower[k];
            out_residual[i] = h.resid[k];
            if (out_steps) out_steps[i] = h.cg.steps[k];
        }
    }
    return DCR_OK;
}

}  // namespace dcr

using namespace dcr;

extern "C" {

int dcr_effective_resistance(dcr_graph *g, const int32_t *u, const int32_t *v, int64_t P, const dcr_resistance_opts *opts,
                             double *out_lower, double *out_residual, int32_t *out_steps) {
    if (!g || !u || !v || !out_lower || !out_residual) DCR_FAIL(DCR_EINVAL, "null argument");
    if (P < 0) DCR_FAIL(DCR_EINVAL, "the number of pairs must be >= 0");
    dcr_resistance_opts o = {1e-10, 20000};
    if (opts) o = *opts;
    if (!(o.tol >= 0.0) || o.max_steps < 1) DCR_FAIL(DCR_EINVAL, "tol must be >= 0, max_steps >= 1");
    for (int64_t i = 0; i < P; ++i)
        if (u[i] < 0 || u[i] >= g->n || v[i] < 0 || v[i] >= g->n) DCR_FAIL(DCR_EINVAL, "pair " + std::to_string(i) + ": endpoint outside 0 .. num_nodes - 1");
    if (P == 0) return DCR_OK;
    DCR_HIP(hipSetDevice(g->device));

    // decided from the components alone: the same node, or no path between the two (an isolated node is its own component)
    std::vector<int32_t> labels;
    DCR_TRY(graph_components(g, labels));
    std::vector<int64_t> todo;
    for (int64_t i = 0; i < P; ++i) {
        const bool same = u[i] == v[i];
        if (!same && labels[(size_t)u[i]] == labels[(size_t)v[i]]) {
            todo.push_back(i);
            continue;
        }
        out_lower[i] = same ? 0.0 : INFINITY;
        out_residual[i] = 0.0;
        if (out_steps) out_steps[i] = 0;
    }
    if (todo.empty()) return DCR_OK;
    return resistance_batches(g, u, v, todo, o, out_lower, out_residual, out_steps);
}

}  // extern "C"
