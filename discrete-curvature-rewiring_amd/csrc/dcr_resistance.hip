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
// RES_B pairs are solved at a time as RES_B independent CGs in step (not a block CG): every vector is node-major [n][RES_B], so
// the gather of one neighbour reads RES_B contiguous doubles (a whole 128-byte line at 16 columns) where k_spec_matvec reads 8
// bytes of one.  A lane owns two adjacent columns (16-byte loads and stores); RES_B / 2 lanes cover a node.  Each column has its own
// alpha, beta, |r|^2, step count and frozen flag in device memory (ResCtl).  A column freezes, on the device, in the step where
// |r| <= tol |c|, or where p^T 𝓛 p is not a positive finite number; a frozen column's y, r and p are no longer written.  Every
// sum runs over rows or nodes in an order that the graph alone fixes and treats all columns alike, so a column's bits depend on
// its own pair only: not on its column index, not on what else shares the batch, not on when the others freeze.
//
// Kernels (all fp64, no floating-point atomics: per-workgroup partials through the L2, closed in index order by the last arriver):
//   k_res_start      r = p = c, z = s ⊙ p, y = 0 for all columns; |c|^2 per column
//   k_res_matvec<0>  q = 𝓛 p = p - s ⊙ (A z) for all columns in one sweep of the rows, through walk_rows in the three degree classes
//                    (<= 32: 32 lanes a row, 64 rows a workgroup; <= 2048: a wave a row; above: a workgroup a row, those first); the
//                    per-column partials of p^T q; the last arriver sets alpha = |r|^2 / p^T q or freezes the column
//   k_res_update     y += alpha p, r -= alpha q, partials of the new |r|^2; the last arriver sets beta, counts the step and freezes
//                    the columns that have converged
//   k_res_direction  p = r + beta p, z = s ⊙ p
//   k_res_scale_y    z = s ⊙ y, then
//   k_res_matvec<1>  w = 𝓛 y (not stored), partials of y^T w and |c - w|^2; the last arriver writes lower and |c - 𝓛 y|_2 per column
// Three launches a step; the host synchronises every SP_CHECK_EVERY steps to read the control block.
#include <algorithm>
#include <cmath>

#include "dcr_analysis.h"

#ifndef DCR_RES_B
#define DCR_RES_B 16  // columns of a batch: 8 or 16 (DESIGN §4.8 has the timings of both)
#endif

namespace dcr {

constexpr int RES_B = DCR_RES_B;
constexpr int RES_CP = RES_B / 2;        // lanes across a node: two columns each
constexpr int RES_SHORT_LANES = 32;      // lanes of a short row's group
constexpr int RES_SHORT_ROWS = 64;       // short rows a workgroup takes: 8 groups x 8 turns
using ResRows = RowGeom<RES_SHORT_LANES, RES_SHORT_ROWS / 8, RES_CP>;
constexpr int RES_UPDATE_BLOCKS = 1024;  // most workgroups of the element-wise kernels with a reduction
static_assert(RES_B == 8 || RES_B == 16, "a batch has 8 or 16 columns");

struct ResCtl {
    double rr[RES_B];     // |r|^2 of the recurrence
    double cc[RES_B];     // |c|^2
    double alpha[RES_B], beta[RES_B];
    double lower[RES_B], resid[RES_B];  // the closing mat-vec's results
    double tol;
    int32_t u[RES_B], v[RES_B];  // the pair of each column; -1: padding
    int32_t frozen[RES_B];
    int32_t steps[RES_B];
    int32_t active;       // columns not frozen
    unsigned ticket;
};

__device__ inline double2 ld2(const double *base, int64_t node, int cp) {
    return *reinterpret_cast<const double2 *>(base + node * RES_B + 2 * cp);
}
__device__ inline void st2(double *base, int64_t node, int cp, double2 x) { *reinterpret_cast<double2 *>(base + node * RES_B + 2 * cp) = x; }

// the entry of c = s_u e_u - s_v e_v at `node` for the column of pair (u, v)
__device__ inline double c_entry(int32_t node, int32_t u, int32_t v, double s_node) { return node == u ? s_node : node == v ? -s_node : 0.0; }

// x summed per column pair (lane % RES_CP) over the workgroup: butterflies over the offsets 32 .. RES_CP, then the four wave sums
// in wave order.  sh: 4 RES_CP entries, free again on return.
__device__ inline double2 cols_block_sum(double2 x, double2 *sh) { return block_sum<RES_CP>(x, sh); }

// partials part[workgroup][RES_B] of `count` workgroups: thread t adds those of workgroups t / RES_CP, + 256 / RES_CP, ... for its
// column pair in order, then cols_block_sum
__device__ inline double2 cols_close_partials(const double *part, int count, double2 *sh) {
    const int cp = threadIdx.x % RES_CP;
    double2 acc = make_double2(0.0, 0.0);
    for (int i = threadIdx.x / RES_CP; i < count; i += 256 / RES_CP) {
        acc.x += ld_agent(part + (int64_t)i * RES_B + 2 * cp);
        acc.y += ld_agent(part + (int64_t)i * RES_B + 2 * cp + 1);
    }
    return cols_block_sum(acc, sh);
}

__device__ inline void cols_store_partial(double *part, int block, double2 x) {  // threads 0 .. RES_CP - 1
    st_agent(part + (int64_t)block * RES_B + 2 * threadIdx.x, x.x);
    st_agent(part + (int64_t)block * RES_B + 2 * threadIdx.x + 1, x.y);
}

// ---- start -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_res_start(const double *__restrict__ s, int64_t n, ResCtl *ctl, double *__restrict__ z,
                                                    double *__restrict__ p, double *__restrict__ r, double *__restrict__ y) {
    const int cp = threadIdx.x % RES_CP;
    const int32_t u0 = ctl->u[2 * cp], v0 = ctl->v[2 * cp], u1 = ctl->u[2 * cp + 1], v1 = ctl->v[2 * cp + 1];
    const int64_t total = n * RES_CP;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t node = e / RES_CP;
        const double sn = s[node];
        const double2 c = make_double2(c_entry((int32_t)node, u0, v0, sn), c_entry((int32_t)node, u1, v1, sn));
        st2(p, node, cp, c);
        st2(r, node, cp, c);
        st2(z, node, cp, make_double2(sn * c.x, sn * c.y));
        st2(y, node, cp, make_double2(0.0, 0.0));
    }
    if (blockIdx.x == 0 && threadIdx.x < RES_B) {
        const int k = threadIdx.x;
        const int32_t u = ctl->u[k], v = ctl->v[k];
        const double su = u >= 0 ? s[u] : 0.0, sv = v >= 0 ? s[v] : 0.0;
        const double cc = su * su + sv * sv;
        ctl->cc[k] = cc;
        ctl->rr[k] = cc;
    }
}

// ---- mat-vec ---------------------------------------------------------------------------------------------------------------------
// MODE 0: x = p, q = 𝓛 p stored, partials of p^T q.  MODE 1: x = y, w = 𝓛 y not stored, partials of y^T w and, behind them, of |c - w|^2.
template <int MODE>
__global__ void __launch_bounds__(256) k_res_matvec(RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                     const double *__restrict__ x, const double *__restrict__ z,
                                                     const double *__restrict__ s, double *__restrict__ q, ResCtl *ctl, double *part) {
    __shared__ double2 sh[4 * RES_CP];
    const int t = threadIdx.x, cp = t % RES_CP;
    const int b = blockIdx.x;
    int32_t u0 = -1, v0 = -1, u1 = -1, v1 = -1;
    if (MODE == 1) {
        u0 = ctl->u[2 * cp];
        v0 = ctl->v[2 * cp];
        u1 = ctl->u[2 * cp + 1];
        v1 = ctl->v[2 * cp + 1];
    }
    double2 dot = make_double2(0.0, 0.0), dev = make_double2(0.0, 0.0);
    walk_rows<ResRows>(plan, rowinfo, sh, [=](auto scope, int32_t row, int2 ri, double2 &xw, double2 &ee) {
        double2 acc = make_double2(0.0, 0.0);  // (A z)_row
        for (int j = scope.first(); j < ri.y; j += scope.stride) {
            const double2 zv = ld2(z, col[ri.x + j], cp);
            acc.x += zv.x;
            acc.y += zv.y;
        }
        acc = scope.sum(acc);
        if (!scope.owner()) return;
        // the row's entry of 𝓛 x, by the RES_CP lanes that own the row
        const double2 xu = ld2(x, row, cp);
        const double su = s[row];
        double2 w;
        w.x = ri.y > 0 ? xu.x - su * acc.x : 0.0;
        w.y = ri.y > 0 ? xu.y - su * acc.y : 0.0;
        xw.x += xu.x * w.x;
        xw.y += xu.y * w.y;
        if (MODE == 0) {
            st2(q, row, cp, w);
        } else {
            const double e0 = c_entry(row, u0, v0, su) - w.x, e1 = c_entry(row, u1, v1, su) - w.y;
            ee.x += e0 * e0;
            ee.y += e1 * e1;
        }
    }, dot, dev);
    dot = cols_block_sum(dot, sh);
    if (t < RES_CP) cols_store_partial(part, b, dot);
    if (MODE == 1) {
        dev = cols_block_sum(dev, sh);
        if (t < RES_CP) cols_store_partial(part + (int64_t)gridDim.x * RES_B, b, dev);
    }
    if (!last_arriver(&ctl->ticket, (unsigned)gridDim.x)) return;
    const double2 a = cols_close_partials(part, gridDim.x, sh);
    double2 d = make_double2(0.0, 0.0);
    if (MODE == 1) d = cols_close_partials(part + (int64_t)gridDim.x * RES_B, gridDim.x, sh);
    if (t < RES_CP) {
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * t + h;
            const double sum = h ? a.y : a.x;
            if (MODE == 0) {
                if (ctl->frozen[k]) continue;
                if (sum > 0.0 && sum <= 1.79769313486231570815e308) {
                    ctl->alpha[k] = ctl->rr[k] / sum;
                } else {  // p^T 𝓛 p zero, negative or not finite: nothing more to gain along p
                    ctl->alpha[k] = 0.0;
                    ctl->frozen[k] = 1;
                }
            } else {
                const int32_t u = ctl->u[k], v = ctl->v[k];
                double lower = 0.0, resid = 0.0;
                if (u >= 0) {
                    const double cty = s[u] * x[(int64_t)u * RES_B + k] - s[v] * x[(int64_t)v * RES_B + k];
                    lower = 2.0 * cty - sum;
                    resid = sqrt(h ? d.y : d.x);
                }
                ctl->lower[k] = lower;
                ctl->resid[k] = resid;
            }
        }
    }
    if (t == 0) __hip_atomic_store(&ctl->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- update, direction -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_res_update(int64_t n, ResCtl *ctl, const double *__restrict__ p, const double *__restrict__ q,
                                                     double *__restrict__ y, double *__restrict__ r, double *part) {
    __shared__ double2 sh[4 * RES_CP];
    const int t = threadIdx.x, cp = t % RES_CP;
    const double a0 = ctl->alpha[2 * cp], a1 = ctl->alpha[2 * cp + 1];
    const bool f0 = ctl->frozen[2 * cp] != 0, f1 = ctl->frozen[2 * cp + 1] != 0;
    double2 acc = make_double2(0.0, 0.0);
    if (!(f0 && f1)) {
        const int64_t total = n * RES_CP;
        for (int64_t e = (int64_t)blockIdx.x * 256 + t; e < total; e += (int64_t)gridDim.x * 256) {
            const int64_t node = e / RES_CP;
            const double2 pv = ld2(p, node, cp), qv = ld2(q, node, cp);
            double2 yv = ld2(y, node, cp), rv = ld2(r, node, cp);
            if (!f0) {
                yv.x += a0 * pv.x;
                rv.x -= a0 * qv.x;
            }
            if (!f1) {
                yv.y += a1 * pv.y;
                rv.y -= a1 * qv.y;
            }
            st2(y, node, cp, yv);
            st2(r, node, cp, rv);
            acc.x += rv.x * rv.x;
            acc.y += rv.y * rv.y;
        }
    }
    acc = cols_block_sum(acc, sh);
    if (t < RES_CP) cols_store_partial(part, blockIdx.x, acc);
    if (!last_arriver(&ctl->ticket, (unsigned)gridDim.x)) return;
    const double2 a = cols_close_partials(part, gridDim.x, sh);
    if (t < RES_CP) {
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * t + h;
            if (ctl->frozen[k]) continue;
            const double rr = h ? a.y : a.x;
            ctl->beta[k] = rr / ctl->rr[k];
            ctl->rr[k] = rr;
            ctl->steps[k] += 1;
            if (!(rr <= 1.79769313486231570815e308) || sqrt(rr) <= ctl->tol * sqrt(ctl->cc[k])) ctl->frozen[k] = 1;
        }
    }
    __syncthreads();
    if (t == 0) {
        int active = 0;
        for (int k = 0; k < RES_B; ++k) active += ctl->frozen[k] == 0;
        ctl->active = active;
        __hip_atomic_store(&ctl->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(256) k_res_direction(int64_t n, const ResCtl *__restrict__ ctl, const double *__restrict__ s,
                                                        const double *__restrict__ r, double *__restrict__ p, double *__restrict__ z) {
    const int cp = threadIdx.x % RES_CP;
    const double b0 = ctl->beta[2 * cp], b1 = ctl->beta[2 * cp + 1];
    const bool f0 = ctl->frozen[2 * cp] != 0, f1 = ctl->frozen[2 * cp + 1] != 0;
    if (f0 && f1) return;
    const int64_t total = n * RES_CP;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t node = e / RES_CP;
        const double2 rv = ld2(r, node, cp);
        double2 pv = ld2(p, node, cp);
        if (!f0) pv.x = rv.x + b0 * pv.x;
        if (!f1) pv.y = rv.y + b1 * pv.y;
        const double sn = s[node];
        st2(p, node, cp, pv);
        st2(z, node, cp, make_double2(sn * pv.x, sn * pv.y));
    }
}

__global__ void __launch_bounds__(256) k_res_scale_y(int64_t n, const double *__restrict__ s, const double *__restrict__ y,
                                                      double *__restrict__ z) {
    const int cp = threadIdx.x % RES_CP;
    const int64_t total = n * RES_CP;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t node = e / RES_CP;
        const double sn = s[node];
        const double2 yv = ld2(y, node, cp);
        st2(z, node, cp, make_double2(sn * yv.x, sn * yv.y));
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
static int resistance_batches(dcr_graph *g, const int32_t *u, const int32_t *v, const std::vector<int64_t> &todo,
                              const dcr_resistance_opts &o, double *out_lower, double *out_residual, int32_t *out_steps) {
    const int64_t n = g->n;
    RowPlan plan;
    DCR_TRY(build_row_plan(g, &plan, nullptr));
    const int nb_mv = (int)row_grid<ResRows>(plan);
    const int nb_el = (int)std::min<int64_t>(RES_UPDATE_BLOCKS, blocks_of(n * RES_CP));

    AnalysisState &A = analysis_of(g);
    DCR_TRY(dev_regrow(&A.res_vec, &A.res_vec_cap, n + 5 * n * RES_B));
    DCR_TRY(dev_regrow(&A.res_part, &A.res_part_cap, (int64_t)RES_B * std::max(2 * nb_mv, nb_el)));
    DCR_TRY(dev_regrow(&A.res_ctl, &A.res_ctl_cap, (int64_t)sizeof(ResCtl)));
    double *z = A.res_vec, *p = z + n * RES_B, *r = p + n * RES_B, *y = r + n * RES_B, *q = y + n * RES_B;  // 16-byte aligned each
    double *s = q + n * RES_B;
    ResCtl *ctl = reinterpret_cast<ResCtl *>(A.res_ctl);
    inv_sqrt_degree(g, s);
    DCR_HIP(hipGetLastError());

    ResCtl h;
    for (size_t first = 0; first < todo.size(); first += RES_B) {
        const int used = (int)std::min<size_t>(RES_B, todo.size() - first);
        std::memset(&h, 0, sizeof(h));
        h.tol = o.tol;
        for (int k = 0; k < RES_B; ++k) {
            const bool pad = k >= used;
            h.u[k] = pad ? -1 : u[todo[first + (size_t)k]];
            h.v[k] = pad ? -1 : v[todo[first + (size_t)k]];
            h.frozen[k] = pad ? 1 : 0;  // padding columns start frozen
        }
        h.active = used;
        DCR_HIP(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));  // h is reused below
        hipLaunchKernelGGL(k_res_start, dim3((unsigned)nb_el), dim3(256), 0, g->stream, s, n, ctl, z, p, r, y);
        for (int64_t step = 0; step < o.max_steps; ++step) {
            hipLaunchKernelGGL(k_res_matvec<0>, dim3((unsigned)nb_mv), dim3(256), 0, g->stream, plan, g->rowinfo, g->col, p, z, s, q, ctl,
                               A.res_part);
            hipLaunchKernelGGL(k_res_update, dim3((unsigned)nb_el), dim3(256), 0, g->stream, n, ctl, p, q, y, r, A.res_part);
            hipLaunchKernelGGL(k_res_direction, dim3((unsigned)nb_el), dim3(256), 0, g->stream, n, ctl, s, r, p, z);
            if ((step + 1) % SP_CHECK_EVERY != 0 && step + 1 != o.max_steps) continue;
            DCR_HIP(hipGetLastError());
            DCR_HIP(hipMemcpyAsync(&h.active, &ctl->active, sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
            DCR_HIP(hipStreamSynchronize(g->stream));
            if (h.active == 0) break;
        }
        hipLaunchKernelGGL(k_res_scale_y, dim3((unsigned)nb_el), dim3(256), 0, g->stream, n, s, y, z);
        hipLaunchKernelGGL(k_res_matvec<1>, dim3((unsigned)nb_mv), dim3(256), 0, g->stream, plan, g->rowinfo, g->col, y, z, s, q, ctl,
                           A.res_part);
        DCR_HIP(hipGetLastError());
        DCR_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));
        for (int k = 0; k < used; ++k) {
            const int64_t i = todo[first + (size_t)k];
            out_lower[i] = h.lower[k];
            out_residual[i] = h.resid[k];
            if (out_steps) out_steps[i] = h.steps[k];
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
