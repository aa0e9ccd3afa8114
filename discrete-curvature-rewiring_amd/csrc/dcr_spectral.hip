// Spectral gap of the normalised Laplacian on the device-resident graph (the connected components it needs: dcr_analysis.hip).
//
// Replaces the dense eigh of the reference's experiment/cheeger_bounds.py:11-21 (normalized_laplacian_matrix, :13; eigh, :15; "the
// first eigenvalue > 0", :16).  What :16 means is the smallest eigenvalue above the null space of L = I - Â, Â = D^-1/2 A D^-1/2;
// with c connected components (an isolated node is one) that null space has dimension exactly c, so lambda_1 is the (c+1)-th
// smallest eigenvalue.  (What :16 does is take the first value floating point left strictly positive, which is rounding noise of
// a zero eigenvalue about half the time; experiment/cheeger_bounds.py of this package states the deviation.)
//
// Method: Lanczos with full reorthogonalisation on B = I + Â (positive semidefinite, spectrum in [0, 2]), restricted to the
// complement of L's null space, which is known in closed form: k_C = D^1/2 1_C / sqrt(vol C) per component with an edge, e_v per
// isolated node v.  lambda_1 = 2 - theta_max(B on that complement).  Every vector of a call is zero on the isolated nodes (the
// start vector is, and B keeps it so: their scale is 0), so only the components with an edge are deflated explicitly.
//
// Kernels (all fp64, no floating-point atomics: every reduction is per-workgroup partials closed in index order, so the same
// seed on the same graph returns the same bits):
//   k_spec_start               start vector from Philox, counter (node, restart)
//   k_spec_matvec              w = v + s ⊙ (A z), z = s ⊙ v kept next to v; rows through walk_rows (dcr_analysis.h): <= 32 eight
//                              lanes a row, <= 2048 a wave a row, above that a workgroup a row (those launch first); alpha = v . w
//   k_spec_defl_dot / _apply   w -= sum_C (k_C . w) k_C over chunks of 1024 nodes: one reduction when there is one component,
//                              the nodes taken through a by-component order otherwise; run before and after Gram-Schmidt, the
//                              second time with |w|^2 -> beta
//   k_spec_gs_coef / _apply    classical Gram-Schmidt against every column at once (run twice per step): one read of w and of
//                              each column for all coefficients, then the update
//   k_spec_normalise           v_next = w / beta (beta read from device memory), z_next = s ⊙ v_next
//   k_spec_combine             Ritz vector = basis x coefficients
// The driver lives in dcr_spectral_gap: explicit restarts from the best Ritz vector, alpha and beta on the device, one host
// synchronisation per 8 steps (and after steps 1, 2 and 4 of a cycle, where a breakdown on a graph of few distinct eigenvalues
// shows), the small tridiagonal problem solved on the host (implicit QL).  A Ritz vector is accepted on its
// TRUE residual only: it becomes column 0 of a fresh cycle, whose first step yields alpha_0 = its Rayleigh quotient and beta_0 =
// |P(B y) - alpha_0 y| by the same kernels.
#include <algorithm>
#include <cmath>

#include "dcr_analysis.h"
#include "dcr_philox.h"

namespace dcr {

constexpr int SP_WAVE_ELEMS = 512;  // elements of w a wave of k_spec_gs_coef keeps in registers
constexpr int SP_CHUNK = 1024;      // nodes per deflation chunk
constexpr double SP_BREAKDOWN = 0x1p-40;

// ---- vectors ---------------------------------------------------------------------------------------------------------------------
// uniform in (-1, 1) from 53 bits of philox4x32_10(node, restart, seed); 0 on isolated nodes
__global__ void __launch_bounds__(256) k_spec_start(const int2 *__restrict__ rowinfo, double *__restrict__ w, int64_t n, uint64_t restart,
                                                     uint64_t seed) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    uint32_t r[4];
    philox4x32_10((uint64_t)v, restart, seed, r);
    const uint64_t bits = ((uint64_t)r[0] | ((uint64_t)r[1] << 32)) >> 11;
    w[v] = rowinfo[v].y > 0 ? ((double)bits + 0.5) * 0x1p-52 - 1.0 : 0.0;
}

using SpecRows = RowGeom<>;  // eight lanes a short row, 32 short rows a workgroup

__global__ void __launch_bounds__(256) k_spec_matvec(RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                      const double *__restrict__ v, const double *__restrict__ z,
                                                      const double *__restrict__ s, double *__restrict__ w, double *part,
                                                      unsigned *ticket, double *alpha_out) {
    __shared__ double sh[4];
    const int t = threadIdx.x;
    double dot = 0.0;  // v_u w_u of the row this thread finishes
    walk_rows<SpecRows>(plan, rowinfo, sh, [=](auto scope, int32_t u, int2 ri, double &vw) {
        double acc = 0.0;
        for (int j = scope.first(); j < ri.y; j += scope.stride) acc += z[col[ri.x + j]];
        acc = scope.sum(acc);
        if (scope.owner()) {
            const double vu = v[u], wu = vu + s[u] * acc;
            w[u] = wu;
            vw = vu * wu;
        }
    }, dot);
    dot = block_sum(dot, sh);
    if (t == 0) st_agent(part + blockIdx.x, dot);
    if (!last_arriver(ticket, (unsigned)gridDim.x)) return;
    const double a = close_partials(part, gridDim.x, sh);
    if (t == 0) {
        *alpha_out = a;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- deflation -------------------------------------------------------------------------------------------------------------------
// chunk: {first position, end position, first chunk of its component, chunks of its component}; positions index `order`, or are
// the node ids themselves when ONE (one component with an edge: the common case)
template <bool ONE>
__global__ void __launch_bounds__(256) k_spec_defl_dot(const int4 *__restrict__ chunks, const int32_t *__restrict__ order,
                                                        const double *__restrict__ kd, const double *__restrict__ w, double *__restrict__ part) {
    __shared__ double sh[4];
    const int4 ch = chunks[blockIdx.x];
    double acc = 0.0;
    for (int p = ch.x + (int)threadIdx.x; p < ch.y; p += 256) {
        const int32_t v = ONE ? p : order[p];
        acc += kd[v] * w[v];
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// the update, and |w|^2 of the deflated w: per-chunk partials (behind the dots in `part`) closed into *beta_out = |w|
template <bool ONE>
__global__ void __launch_bounds__(256) k_spec_defl_apply(const int4 *__restrict__ chunks, const int32_t *__restrict__ order,
                                                          const double *__restrict__ kd, double *__restrict__ w, double *part, unsigned *ticket,
                                                          double *beta_out) {
    __shared__ double sh[4];
    const int4 ch = chunks[blockIdx.x];
    double acc = 0.0;
    for (int i = threadIdx.x; i < ch.w; i += 256) acc += part[ch.z + i];  // (written by the launch before this one)
    const double tot = block_sum(acc, sh);  // the same bits in every chunk of the component
    double sq = 0.0;
    for (int p = ch.x + (int)threadIdx.x; p < ch.y; p += 256) {
        const int32_t v = ONE ? p : order[p];
        const double x = w[v] - tot * kd[v];
        w[v] = x;
        sq += x * x;
    }
    if (!beta_out) return;
    sq = block_sum(sq, sh);
    double *part2 = part + gridDim.x;
    if (threadIdx.x == 0) st_agent(part2 + blockIdx.x, sq);
    if (!last_arriver(ticket, (unsigned)gridDim.x)) return;
    const double nrm2 = close_partials(part2, gridDim.x, sh);
    if (threadIdx.x == 0) {
        *beta_out = sqrt(nrm2);
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- classical Gram-Schmidt against columns 0 .. jc - 1 --------------------------------------------------------------------------
// A wave keeps 512 consecutive elements of w in registers and walks the columns; partial (column, wave) at part[column * n_waves + wave].
// The last workgroup closes them a wave per column: lane l adds partials l, l + 64, ... in order, then the butterfly: coef[column].
__global__ void __launch_bounds__(256) k_spec_gs_coef(const double *__restrict__ basis, const double *__restrict__ w, int64_t n, int jc,
                                                       int n_waves, double *part, double *__restrict__ coef, unsigned *ticket) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * 4 + wave;
    if (gw < n_waves) {
        const int64_t x0 = (int64_t)gw * SP_WAVE_ELEMS + lane;
        double wr[SP_WAVE_ELEMS / 64];
#pragma unroll
        for (int q = 0; q < SP_WAVE_ELEMS / 64; ++q) wr[q] = x0 + 64 * q < n ? w[x0 + 64 * q] : 0.0;
        for (int i = 0; i < jc; ++i) {
            const double *__restrict__ c = basis + (int64_t)i * n;
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < SP_WAVE_ELEMS / 64; ++q) a += wr[q] * (x0 + 64 * q < n ? c[x0 + 64 * q] : 0.0);
            a = wave_sum(a);
            if (lane == 0) st_agent(part + (int64_t)i * n_waves + gw, a);
        }
    }
    if (!last_arriver(ticket, (unsigned)gridDim.x)) return;
    for (int i = wave; i < jc; i += 4) {
        const double *col_part = part + (int64_t)i * n_waves;
        double acc = 0.0;
        for (int p = lane; p < n_waves; p += 64) acc += ld_agent(col_part + p);
        acc = wave_sum(acc);
        if (lane == 0) coef[i] = acc;
    }
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// w -= sum_i coef[i] column_i, the columns in index order
__global__ void __launch_bounds__(256) k_spec_gs_apply(const double *__restrict__ basis, double *__restrict__ w, int64_t n, int jc,
                                                        const double *__restrict__ coef) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    double acc = w[x];
    for (int i = 0; i < jc; ++i) acc -= coef[i] * basis[(int64_t)i * n + x];
    w[x] = acc;
}

// a beta below the breakdown threshold leaves a zero column: the host stops at that step
__global__ void __launch_bounds__(256) k_spec_normalise(const double *__restrict__ w, const double *__restrict__ beta, const double *__restrict__ s,
                                                         double *__restrict__ vout, double *__restrict__ zout, int64_t n) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const double b = *beta;
    const double y = b >= SP_BREAKDOWN ? w[x] / b : 0.0;
    vout[x] = y;
    zout[x] = s[x] * y;
}

__global__ void __launch_bounds__(256) k_spec_combine(const double *__restrict__ basis, const double *__restrict__ coef, int64_t n, int k,
                                                       double *__restrict__ w) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    double acc = 0.0;
    for (int i = 0; i < k; ++i) acc += coef[i] * basis[(int64_t)i * n + x];
    w[x] = acc;
}

// ---- host: symmetric tridiagonal eigenproblem, implicit QL (EISPACK tql2) ----------------------------------------------------------
// d[0 .. k): diagonal, e[0 .. k - 1): off-diagonal.  zt holds `rows` tracked rows of the eigenvector matrix, transposed: on entry
// zt[i * rows + r] = Z0[r][i], on return column i of Z (eigenvalue d[i]) is zt[i * rows .. i * rows + rows).  Returns false if a
// value takes more than 60 sweeps.
static bool tridiag_ql(std::vector<double> &d, std::vector<double> &e_in, int k, std::vector<double> &zt, int rows) {
    std::vector<double> e((size_t)k, 0.0);
    for (int i = 0; i + 1 < k; ++i) e[(size_t)i] = e_in[(size_t)i];
    double f = 0.0, tst1 = 0.0;
    const double eps = 0x1p-52;
    for (int l = 0; l < k; ++l) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < k - 1 && std::fabs(e[m]) > eps * tst1) ++m;
        if (m > l) {
            int iter = 0;
            do {
                if (++iter > 60) return false;
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = std::hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < k; ++i) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
                const double el1 = e[l + 1];
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2;
                    c2 = c;
                    s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = std::hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    double *za = &zt[(size_t)i * rows], *zb = &zt[(size_t)(i + 1) * rows];
                    for (int q = 0; q < rows; ++q) {
                        const double hb = zb[q];
                        zb[q] = s * za[q] + c * hb;
                        za[q] = c * za[q] - s * hb;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1);
        }
        d[l] += f;
        e[l] = 0.0;
    }
    return true;
}

// largest eigenvalue of T_k (alpha, beta) and, per `full`, its whole eigenvector or only the last component (in vec[0])
static bool top_ritz(const double *alpha, const double *beta, int k, bool full, double *theta, std::vector<double> &vec) {
    std::vector<double> d(alpha, alpha + k), e(beta, beta + (k > 1 ? k - 1 : 0));
    const int rows = full ? k : 1;
    std::vector<double> zt((size_t)k * rows, 0.0);
    if (full)
        for (int i = 0; i < k; ++i) zt[(size_t)i * k + i] = 1.0;
    else
        zt[(size_t)(k - 1)] = 1.0;  // row k - 1 of the identity
    if (!tridiag_ql(d, e, k, zt, rows)) return false;
    int best = 0;
    for (int i = 1; i < k; ++i)
        if (d[i] > d[best]) best = i;
    *theta = d[best];
    vec.assign(zt.begin() + (size_t)best * rows, zt.begin() + (size_t)(best + 1) * rows);
    return true;
}

// ---- host: plan, driver ------------------------------------------------------------------------------------------------------------
void spectral_release_basis(dcr_graph *g) {
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->analysis) g->analysis->spc_basis.free();
}

struct SpecRun {
    dcr_graph *g;
    AnalysisState *A;
    int64_t n;
    RowPlan plan;
    int n_chunks, n_waves;
    bool one;
    double *s, *kd, *z, *w;         // [n] each, in spc_vec
    double *alpha, *beta, *scal, *coef, *ritz;  // in spc_small
    int32_t *order;
    unsigned *ticket;

    double *col(int j) const { return A->spc_basis.p + (int64_t)j * n; }
    // w -= sum_C (k_C . w) k_C; with beta_out also *beta_out = |w| afterwards
    void deflate(double *beta_out) const {
        if (one) {
            hipLaunchKernelGGL(k_spec_defl_dot<true>, dim3(n_chunks), dim3(256), 0, g->stream, A->spc_chunks.p, order, kd, w, A->spc_part.p);
            hipLaunchKernelGGL(k_spec_defl_apply<true>, dim3(n_chunks), dim3(256), 0, g->stream, A->spc_chunks.p, order, kd, w, A->spc_part.p,
                               ticket, beta_out);
        } else {
            hipLaunchKernelGGL(k_spec_defl_dot<false>, dim3(n_chunks), dim3(256), 0, g->stream, A->spc_chunks.p, order, kd, w, A->spc_part.p);
            hipLaunchKernelGGL(k_spec_defl_apply<false>, dim3(n_chunks), dim3(256), 0, g->stream, A->spc_chunks.p, order, kd, w, A->spc_part.p,
                               ticket, beta_out);
        }
    }
    // w orthogonal to columns 0 .. jc - 1: classical Gram-Schmidt, twice
    void orthogonalise(int jc) const {
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(k_spec_gs_coef, dim3(blocks_of(n_waves, 4)), dim3(256), 0, g->stream, A->spc_basis.p, w, n, jc,
                               n_waves, A->spc_part.p, coef, ticket);
            hipLaunchKernelGGL(k_spec_gs_apply, dim3(blocks_of(n)), dim3(256), 0, g->stream, A->spc_basis.p, w, n, jc, coef);
        }
    }
    void normalise(const double *beta_in, int j) const {
        hipLaunchKernelGGL(k_spec_normalise, dim3(blocks_of(n)), dim3(256), 0, g->stream, w, beta_in, s, col(j), z, n);
    }
    // column 0 from what is in w
    void first_column() const {
        deflate(scal);
        normalise(scal, 0);
    }
    // Lanczos step j: alpha[j], beta[j], and column j + 1 when there is room for it
    void step(int j, int m) const {
        hipLaunchKernelGGL(k_spec_matvec, dim3(row_grid<SpecRows>(plan)), dim3(256), 0, g->stream, plan, g->rowinfo.p, g->col.p, col(j), z, s, w,
                           A->spc_part.p, ticket, alpha + j);
        // The deflation comes LAST.  Each column carries a rounding-size component along the k_C; Gram-Schmidt hands w the sum
        // of those, weighted by alpha and beta, and with nothing behind it that component obeys the Lanczos recurrence of an
        // eigenvalue inside the spectrum (P B P k = 0) and doubles per step, while alpha = v . B v goes on treating k as
        // B's eigenvalue 2: T stops being the projection of one operator after some 50 steps.
        deflate(nullptr);
        orthogonalise(j + 1);
        deflate(beta + j);
        if (j + 1 < m) normalise(beta + j, j + 1);
    }
};

// The whole of dcr_spectral_gap but for the download of the vector: the accepted Ritz vector stays in column 0 of the basis, which
// stays allocated until spectral_release_basis.
int spectral_solve(dcr_graph *g, const dcr_spectral_opts *opts, dcr_spectral_result *out, SpectralKept *kept, RowPlan *plan) {
    if (!g || !out) DCR_FAIL(DCR_EINVAL, "null argument");
    dcr_spectral_opts o = {1e-10, 20000, 0, 0};
    if (opts) o = *opts;
    if (!(o.tol >= 0.0) || o.max_steps < 1 || o.max_basis < 0) DCR_FAIL(DCR_EINVAL, "tol must be >= 0, max_steps >= 1, max_basis >= 0");
    if (g->n_edges <= 0) DCR_FAIL(DCR_EINVAL, "no positive eigenvalue: the graph has no edges");
    DCR_HIP(hipSetDevice(g->device));
    const int64_t n = g->n;

    // components, degrees, the null-space vectors
    std::vector<int32_t> labels;
    DCR_TRY(graph_components(g, labels));
    std::vector<int2> info;
    DCR_TRY(build_row_plan(g, plan, &info));
    int64_t components = 0;
    std::vector<int32_t> cidx((size_t)n, -1);  // component with an edge -> its index, by smallest node id
    std::vector<int64_t> vol;
    for (int64_t v = 0; v < n; ++v) {
        if (labels[(size_t)v] != v) continue;
        ++components;
        if (info[(size_t)v].y > 0) {
            cidx[(size_t)v] = (int32_t)vol.size();
            vol.push_back(0);
        }
    }
    for (int64_t v = 0; v < n; ++v)
        if (info[(size_t)v].y > 0) vol[(size_t)cidx[(size_t)labels[(size_t)v]]] += info[(size_t)v].y;
    const int64_t n_comp = (int64_t)vol.size();
    std::vector<double> kd((size_t)n, 0.0);
    for (int64_t v = 0; v < n; ++v)
        if (info[(size_t)v].y > 0) kd[(size_t)v] = std::sqrt((double)info[(size_t)v].y) / std::sqrt((double)vol[(size_t)cidx[(size_t)labels[(size_t)v]]]);

    AnalysisState &A = analysis_of(g);
    SpecRun R;
    R.g = g;
    R.A = &A;
    R.n = n;
    R.plan = *plan;
    R.one = n_comp == 1;
    // deflation chunks
    std::vector<int4> chunks;
    std::vector<int32_t> order;
    if (R.one) {
        const int nc = (int)((n + SP_CHUNK - 1) / SP_CHUNK);
        for (int c = 0; c < nc; ++c) chunks.push_back(make_int4(c * SP_CHUNK, (int)std::min<int64_t>(n, (int64_t)(c + 1) * SP_CHUNK), 0, nc));
    } else {
        std::vector<int64_t> first((size_t)n_comp + 1, 0);
        for (int64_t v = 0; v < n; ++v)
            if (info[(size_t)v].y > 0) ++first[(size_t)cidx[(size_t)labels[(size_t)v]] + 1];
        for (int64_t c = 0; c < n_comp; ++c) first[(size_t)c + 1] += first[(size_t)c];
        order.resize((size_t)first[(size_t)n_comp]);
        std::vector<int64_t> fill(first.begin(), first.end() - 1);
        for (int64_t v = 0; v < n; ++v)
            if (info[(size_t)v].y > 0) order[(size_t)fill[(size_t)cidx[(size_t)labels[(size_t)v]]]++] = (int32_t)v;
        for (int64_t c = 0; c < n_comp; ++c) {
            const int64_t b = first[(size_t)c], e = first[(size_t)c + 1];
            const int nc = (int)((e - b + SP_CHUNK - 1) / SP_CHUNK), c0 = (int)chunks.size();
            for (int i = 0; i < nc; ++i)
                chunks.push_back(make_int4((int)(b + (int64_t)i * SP_CHUNK), (int)std::min<int64_t>(e, b + (int64_t)(i + 1) * SP_CHUNK), c0, nc));
        }
    }
    R.n_chunks = (int)chunks.size();
    // basis capacity
    const int64_t by_memory = ((int64_t)4 << 30) / (8 * n);
    int64_t m = o.max_basis > 0 ? std::min(o.max_basis, std::max<int64_t>(by_memory, 16)) : std::max<int64_t>(std::min<int64_t>(256, by_memory), 16);
    if (m < 2) m = 2;  // one column could only restart from itself
    m = std::max<int64_t>(1, std::min(m, n - components));  // the deflated space has n - c dimensions
    R.n_waves = (int)((n + SP_WAVE_ELEMS - 1) / SP_WAVE_ELEMS);

    // buffers
    DCR_TRY(A.spc_vec.grow(4 * n));
    DCR_TRY(A.spc_basis.grow(m * n));
    DCR_TRY(A.spc_rows.grow(n));
    DCR_TRY(A.spc_chunks.grow((int64_t)chunks.size()));
    const int64_t part_need = std::max<int64_t>({(int64_t)R.n_waves * m, (int64_t)row_grid<SpecRows>(*plan), 2 * (int64_t)R.n_chunks});
    DCR_TRY(A.spc_part.grow(part_need));
    DCR_TRY(A.spc_small.grow(4 * m + 8));
    DCR_TRY(A.spc_ctl.grow(4));
    R.s = A.spc_vec.p;
    R.kd = R.s + n;
    R.z = R.s + 2 * n;
    R.w = R.s + 3 * n;
    R.alpha = A.spc_small.p;
    R.beta = R.alpha + m;
    R.scal = R.alpha + 2 * m;  // 8 scalars
    R.coef = R.alpha + 2 * m + 8;
    R.ritz = R.alpha + 3 * m + 8;
    R.order = A.spc_rows.p;
    R.ticket = A.spc_ctl.p + 1;
    DCR_HIP(hipMemsetAsync(A.spc_ctl.p, 0, 4 * sizeof(unsigned), g->stream));
    DCR_HIP(hipMemcpyAsync(R.kd, kd.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, g->stream));
    if (!order.empty())
        DCR_HIP(hipMemcpyAsync(R.order, order.data(), sizeof(int32_t) * order.size(), hipMemcpyHostToDevice, g->stream));
    DCR_HIP(hipMemcpyAsync(A.spc_chunks.p, chunks.data(), sizeof(int4) * chunks.size(), hipMemcpyHostToDevice, g->stream));
    inv_sqrt_degree(g, R.s);
    hipLaunchKernelGGL(k_spec_start, dim3(blocks_of(n)), dim3(256), 0, g->stream, g->rowinfo.p, R.w, n, (uint64_t)0, o.seed);
    R.first_column();
    DCR_HIP(hipGetLastError());

    // Lanczos cycles
    std::vector<double> ab((size_t)(2 * m)), vec;
    int64_t total = 0, restarts = 0;
    bool last_cycle = false, converged = false;
    double theta = 0.0, residual = INFINITY;
    for (bool done = false; !done;) {
        for (int j = 0;; ++j) {
            R.step(j, (int)m);
            ++total;
            const bool forced = total >= o.max_steps - 1;
            // The host also looks after steps 1, 2 and 4 of a cycle.  With two or three distinct eigenvalues on the deflated space
            // (a star, a union of cliques) the recurrence breaks down there, and every step up to the next look would be spent
            // on a zero column.
            const bool early = j + 1 < SP_CHECK_EVERY && ((j + 1) & j) == 0;
            if (!(early || (j + 1) % SP_CHECK_EVERY == 0 || j + 1 == m || forced)) continue;
            DCR_HIP(hipGetLastError());
            DCR_HIP(hipMemcpyAsync(ab.data(), A.spc_small.p, sizeof(double) * (size_t)(2 * m), hipMemcpyDeviceToHost, g->stream));
            DCR_HIP(hipStreamSynchronize(g->stream));
            const double *alpha = ab.data(), *beta = ab.data() + m;
            if (j == 0) {  // column 0 is a unit vector of the deflated space: its Rayleigh quotient and its true residual
                theta = alpha[0];
                residual = beta[0];
                if (!std::isfinite(theta) || !std::isfinite(residual)) DCR_FAIL(DCR_ESTATE, "spectral gap: non-finite Lanczos coefficients");
                converged = residual <= o.tol;
                if (converged || last_cycle || total >= o.max_steps) {
                    done = true;
                    break;
                }
            }
            int k = j + 1;
            bool breakdown = false;
            for (int i = 0; i <= j; ++i)
                if (!(beta[i] >= SP_BREAKDOWN)) {  // an invariant subspace: solve what is there and finish
                    k = i + 1;
                    breakdown = true;
                    break;
                }
            double th = 0.0;
            bool restart = breakdown || k == m || forced;
            if (!restart) {
                if (!top_ritz(alpha, beta, k, false, &th, vec)) DCR_FAIL(DCR_ESTATE, "spectral gap: the tridiagonal QL iteration did not converge");
                restart = std::fabs(beta[k - 1] * vec[0]) <= 0.5 * o.tol;  // the Lanczos estimate only decides when to look
            }
            if (!restart) continue;
            if (!top_ritz(alpha, beta, k, true, &th, vec)) DCR_FAIL(DCR_ESTATE, "spectral gap: the tridiagonal QL iteration did not converge");
            DCR_HIP(hipMemcpyAsync(R.ritz, vec.data(), sizeof(double) * (size_t)k, hipMemcpyHostToDevice, g->stream));
            DCR_HIP(hipStreamSynchronize(g->stream));
            hipLaunchKernelGGL(k_spec_combine, dim3(blocks_of(n)), dim3(256), 0, g->stream, A.spc_basis.p, R.ritz, n, k, R.w);
            R.first_column();
            ++restarts;
            last_cycle = breakdown || forced;
            break;
        }
    }
    DCR_HIP(hipStreamSynchronize(g->stream));
    kept->y = R.col(0);
    kept->s = R.s;
    out->lambda1 = 2.0 - theta;
    out->residual = residual;
    out->steps = total;
    out->restarts = restarts;
    out->components = components;
    out->converged = converged ? 1 : 0;
    return DCR_OK;
}

}  // namespace dcr

using namespace dcr;

extern "C" {

int dcr_spectral_gap(dcr_graph *g, const dcr_spectral_opts *opts, dcr_spectral_result *out, double *out_vector) {
    SpectralKept kept;
    RowPlan plan;
    int rc = spectral_solve(g, opts, out, &kept, &plan);
    if (rc == DCR_OK && out_vector) {
        hipError_t e = hipMemcpyAsync(out_vector, kept.y, sizeof(double) * (size_t)g->n, hipMemcpyDeviceToHost, g->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
        if (e != hipSuccess) {
            set_error(std::string("spectral gap: the vector did not come back: ") + hipGetErrorString(e));
            rc = DCR_EHIP;
        }
    }
    // an occasional analysis call: the basis (up to 4 GiB) does not stay on the handle; the O(n) buffers do
    if (g) spectral_release_basis(g);
    return rc;
}

}  // extern "C"
