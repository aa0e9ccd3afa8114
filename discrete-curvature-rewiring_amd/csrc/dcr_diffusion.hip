// PageRank diffusion rewiring (DIGL / GDC) on the device-resident graph: columns of the personalised-PageRank matrix, sparsified.
//
// With Ã = A + I, d̃ = deg + 1, H = D̃^-1/2 Ã D̃^-1/2 and 0 < α < 1:  M = I - (1 - α) H,  S = α M^-1.  H is symmetric with spectrum in
// (-1, 1], so M is symmetric positive definite with spectrum in [α, 2 - α]; column j of S solves M x = α e_j.  An isolated node
// has M_jj = α and S_jj = 1.  The reference never forms this matrix; utils/adjacency_matrix_ops.py:26-39 holds the two sparsifiers
// that were written for it, on dense N x N arrays, and they are restated here per column: keep the k largest entries, or the
// entries >= eps, then divide the kept entries by their sum.
//
// The solve: COL_B columns at a time by the batched column CG of dcr_analysis.h (the layout, the freeze rule and why a column's bits
// depend on its own source only, padding and neighbours in the batch notwithstanding, are described there).  DifProblem below
// is all this file adds to it: the operator's row entry, α e_j as the right-hand side, the stop threshold tol α (α = |α e_j|) and the
// true residual the close writes.
//
// The selection runs on the batch's [n][COL_B] result where it lies, a workgroup a column.  Values go through the order-preserving
// map of fp64 onto uint64 (negative: all bits flipped, else the sign bit set): entries of S are positive, but an entry below the
// solve's error can come out negative, and the order has to be that of the values whatever the solve left.  Larger value first;
// among equal bits, the smaller node id first.
//
// Kernels (all fp64, no floating-point atomics: per-workgroup partials through the L2, closed in index order by the last arriver):
//   k_dif_scale      s̃ = 1 / sqrt(deg + 1)
//   k_col_start<DifProblem>      r = p = α e_j, z = s̃ ⊙ p, x = 0 for all columns
//   k_col_matvec<DifProblem, 0>  q = M p = p - (1 - α) s̃ ⊙ ((A + I) z): the row's neighbours summed over the scope, the row's own z
//                    added by the owner lanes; the last arriver sets the step length |r|^2 / p^T q or freezes the column
//   k_col_update<DifCtl>, k_col_direction<DifCtl>, k_col_scale   as they are in dcr_analysis.h, then
//   k_col_matvec<DifProblem, 1>  w = M x (not stored), partials of |α e_j - w|^2; the last arriver writes the true residual per column
//   k_dif_select     top-k: a radix select per column, 8-bit digit histograms in LDS from the top digit down over the keys that
//                    share the digits chosen so far, until the k-th key and the count above it are known (or a whole bucket is
//                    kept and no tie is left to break); threshold: the count of keys >= key(eps)
//   k_dif_fill       the kept entries of a column in node order: every key above the threshold key and the first `take` node ids
//                    among the keys equal to it (two workgroup scans per 256 nodes); the kept values are added in that order by one
//                    thread, then every kept value is divided by the sum
// Three launches a solver step; the host synchronises every SP_CHECK_EVERY steps to read the control blocks.  A small graph does not
// fill the device with one batch, so up to DIF_MAX_GROUPS batches share every launch as blockIdx.y (while groups x nodes stays
// within DIF_GROUP_NODES), each with its own vectors, partials, ticket and control block: the arithmetic of a column is that of
// its batch alone, however many batches run beside it.
//
// The heat kernel, GDC's other diffusion: S = exp(-t (I - H)) = e^-t Σ_k t^k / k! H^k for 0 < t <= 256.  Every term is non-negative,
// so nothing cancels and a partial sum is an entrywise lower bound of the column; H √d̃ = √d̃, so with r = √d̃ the mass the partial sum
// x = Σ_{k <= K} θ_k H^k e_j (θ_k = e^-t t^k / k!) still lacks is r_j - Σ_i r_i x_i = r_j ρ_K, ρ_K = Σ_{k > K} θ_k, and
// 0 <= S_ij - x_i <= deficit_j / r_i.  K is fixed on the host before the first launch (heat_terms: the smallest K with ρ_K <= tol / 2,
// the tail added term by term from its small end, or max_terms where that is lower): no data-dependent stop, no ticket and no
// read-back between terms.  The recurrence v_0 = e^-t e_j, v_{k+1} = t / (k + 1) s̃ ⊙ ((A + I)(s̃ ⊙ v_k)), x += v_{k+1} keeps only
// z = s̃ ⊙ v between terms, in two buffers by turns (z and p of the PageRank layout): other rows read z_in during the sweep.
//   k_heat_start     x = e^-t e_j, z = s̃ ⊙ x for all columns (padding columns are zero and stay zero)
//   k_heat_term      one launch a term, the row walk and gather of k_col_matvec: v = c (s̃_u (Σ z_in[col] + z_in[u])), x[u] += v,
//                    z_out[u] = s̃_u v, with c = t / (k + 1) an argument
//   k_heat_mass      partials of Σ_i r_i x_i per column; the last arriver writes deficit_j = r_j - Σ_i r_i x_i
// K + 2 launches a batch, then k_dif_select / k_dif_fill as they are.  A column's bits depend on its source, t and K only.
#include <algorithm>
#include <cmath>

#include "dcr_analysis.h"

namespace dcr {

constexpr int DIF_MAX_GROUPS = 8;        // batches solved side by side in the same launches (blockIdx.y), each on its own
constexpr int64_t DIF_GROUP_NODES = 65536;  // vectors and control block: as many as keep groups x nodes within this

struct DifCtl {
    ColCg cg;
    double resid[COL_B];   // the closing mat-vec's |α e_j - M x|_2; heat: the deficit r_j - Σ_i r_i x_i
    double teleport, damp; // α, 1 - α
    uint64_t thr[COL_B];   // selection: the threshold key
    int64_t base[COL_B];   // where the column's kept entries start in the batch's output
    int32_t src[COL_B];    // the source node of each column; -1: padding
    int32_t take[COL_B];   // how many of the keys equal to thr are kept, in node order
    int32_t count[COL_B];  // kept entries
};

// the entry of α e_src at `node`
__device__ inline double dif_rhs(int32_t node, int32_t src, double teleport) { return node == src ? teleport : 0.0; }

struct DifProblem {  // M x = α e_j for the column CG of dcr_analysis.h; the host sets the stop threshold tol α
    using Ctl = DifCtl;
    static constexpr bool closing_dot = false;  // the close needs |α e_j - M x|^2 only
    DifCtl *ctl;
    __device__ auto rhs(int cp) const {
        const int32_t j0 = ctl->src[2 * cp], j1 = ctl->src[2 * cp + 1];
        const double teleport = ctl->teleport;
        return [=](int32_t node, double) { return make_double2(dif_rhs(node, j0, teleport), dif_rhs(node, j1, teleport)); };
    }
    __device__ auto entry() const {  // the row's own z is the I of A + I
        const double damp = ctl->damp;
        return [=](int, double v, double su, double acc, double zu) { return v - damp * (su * (acc + zu)); };
    }
    __device__ void start(int k, const double *) const { ctl->cg.rr[k] = ctl->src[k] >= 0 ? ctl->teleport * ctl->teleport : 0.0; }
    __device__ void close(int k, const double *, const double *, double, double dev) const { ctl->resid[k] = ctl->src[k] >= 0 ? sqrt(dev) : 0.0; }
};

__global__ void __launch_bounds__(256) k_dif_scale(const int2 *__restrict__ rowinfo, double *__restrict__ s, int64_t n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) s[v] = 1.0 / sqrt((double)rowinfo[v].y + 1.0);
}

// ---- heat kernel -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_heat_start(const double *__restrict__ s, int64_t n, const DifCtl *__restrict__ ctl, double start,
                                                     double *__restrict__ z, double *__restrict__ x, int64_t gstride) {
    const int cp = threadIdx.x % COL_CP;
    const int64_t go = (int64_t)blockIdx.y * gstride;
    ctl += blockIdx.y, z += go, x += go;
    const int32_t j0 = ctl->src[2 * cp], j1 = ctl->src[2 * cp + 1];
    const int64_t total = n * COL_CP;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t node = e / COL_CP;
        const double sn = s[node];
        const double2 c = make_double2(dif_rhs((int32_t)node, j0, start), dif_rhs((int32_t)node, j1, start));  // e^-t e_src
        st2(x, node, cp, c);
        st2(z, node, cp, make_double2(sn * c.x, sn * c.y));
    }
}

// x += v, z_out = s̃ ⊙ v with v = c s̃ ⊙ ((A + I) z_in) for all columns in one sweep of the rows; a row's x and z_out are written by its
// owner lanes alone, z_in by nobody
__global__ void __launch_bounds__(256) k_heat_term(RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                    const double *__restrict__ z_in, const double *__restrict__ s, double c,
                                                    double *__restrict__ z_out, double *__restrict__ x, int64_t gstride) {
    __shared__ double2 sh[4 * COL_CP];
    const int cp = threadIdx.x % COL_CP;
    const int64_t go = (int64_t)blockIdx.y * gstride;
    z_in += go, z_out += go, x += go;
    walk_rows<ColRows>(plan, rowinfo, sh, [=](auto scope, int32_t row, int2 ri) {
        const double2 acc = gather(scope, col, ri, z_in, cp);
        if (!scope.owner()) return;
        const double2 zu = ld2(z_in, row, cp);
        const double su = s[row];
        const double2 v = make_double2(c * (su * (acc.x + zu.x)), c * (su * (acc.y + zu.y)));
        double2 xu = ld2(x, row, cp);
        xu.x += v.x;
        xu.y += v.y;
        st2(x, row, cp, xu);
        st2(z_out, row, cp, make_double2(su * v.x, su * v.y));
    });
}

__global__ void __launch_bounds__(256) k_heat_mass(const int2 *__restrict__ rowinfo, int64_t n, DifCtl *ctl, const double *__restrict__ x,
                                                    double *part, int64_t gstride, int64_t pstride) {
    __shared__ double2 sh[4 * COL_CP];
    const int t = threadIdx.x, cp = t % COL_CP;
    ctl += blockIdx.y, x += (int64_t)blockIdx.y * gstride, part += (int64_t)blockIdx.y * pstride;
    double2 acc = make_double2(0.0, 0.0);
    const int64_t total = n * COL_CP;
    for (int64_t e = (int64_t)blockIdx.x * 256 + t; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t node = e / COL_CP;
        const double rn = sqrt((double)rowinfo[node].y + 1.0);
        const double2 xv = ld2(x, node, cp);
        acc.x += rn * xv.x;
        acc.y += rn * xv.y;
    }
    acc = block_sum<COL_CP>(acc, sh);
    if (t < COL_CP) store_partial(part, blockIdx.x, acc);
    if (!last_arriver(&ctl->cg.ticket, (unsigned)gridDim.x)) return;
    const double2 a = close_partials(part, gridDim.x, sh);
    if (t < COL_CP) {
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * t + h;
            const int32_t j = ctl->src[k];
            ctl->resid[k] = j >= 0 ? sqrt((double)rowinfo[j].y + 1.0) - (h ? a.y : a.x) : 0.0;
        }
    }
    if (t == 0) __hip_atomic_store(&ctl->cg.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------
// fp64 -> uint64 in the order of the values (-0.0 below +0.0; the solve never produces it)
__host__ __device__ inline uint64_t dif_key(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof(b));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// 256 threads: the exclusive prefix of x in thread order, and the workgroup's total.  sh: 4 entries, free again on return.
__device__ inline int dif_excl_scan(int x, int *sh, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(incl, off);
        if (lane >= off) incl += y;
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    const int w0 = sh[0], w1 = sh[1], w2 = sh[2], w3 = sh[3];
    __syncthreads();
    total = w0 + w1 + w2 + w3;
    return incl - x + (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0);
}

// A workgroup a column.  mode 0: thr = the k-th largest key of the column and take = how many of the keys equal to it belong to
// the k largest (k <= n); or, where a whole bucket of keys is kept, thr = the bucket's smallest possible key and take = n.
// mode 1: thr is given (the key of eps), take = n, count = the keys >= thr.
__global__ void __launch_bounds__(256) k_dif_select(const double *__restrict__ x, int64_t n, DifCtl *ctl, int mode, int k, int64_t gstride) {
    __shared__ int hist[256];
    __shared__ int sh[4];
    __shared__ int pick[3];
    const int t = threadIdx.x, c = blockIdx.x;
    ctl += blockIdx.y, x += (int64_t)blockIdx.y * gstride;
    if (ctl->src[c] < 0) {  // padding
        if (t == 0) ctl->count[c] = 0;
        return;
    }
    if (mode == 1) {
        const uint64_t thr = ctl->thr[c];
        int mine = 0, total;
        for (int64_t i = t; i < n; i += 256) mine += dif_key(x[i * COL_B + c]) >= thr;
        dif_excl_scan(mine, sh, total);
        if (t == 0) {
            ctl->count[c] = total;
            ctl->take[c] = (int32_t)n;
        }
        return;
    }
    uint64_t prefix = 0, mask = 0;
    int need = k, take = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[t] = 0;
        __syncthreads();
        for (int64_t i = t; i < n; i += 256) {
            const uint64_t key = dif_key(x[i * COL_B + c]);
            if ((key & mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
        }
        __syncthreads();
        // thread t looks at digit 255 - t: `above` counts the keys of this round with a larger digit
        const int d = 255 - t, h = hist[d];
        int total;
        const int above = dif_excl_scan(h, sh, total);
        if (above < need && need <= above + h) {  // one thread: the digit of the need-th largest key
            pick[0] = d;
            pick[1] = above;
            pick[2] = h;
        }
        __syncthreads();
        const int digit = pick[0], bucket = pick[2];
        need -= pick[1];
        __syncthreads();
        prefix |= (uint64_t)digit << shift;
        mask |= (uint64_t)255 << shift;
        if (bucket == need) {  // the whole bucket is kept: every key >= prefix, no tie to break
            take = (int)n;
            break;
        }
        take = need;  // after the last digit: `need` of the keys equal to prefix
    }
    if (t == 0) {
        ctl->thr[c] = prefix;
        ctl->take[c] = take;
        ctl->count[c] = k;
    }
}

// A workgroup a column: the kept entries in node order into row / val at base[c], never more than count[c] of them; then
// wgt = val / sum, the sum taken in node order (1 where it is not positive, as the reference's helpers divide).
__global__ void __launch_bounds__(256) k_dif_fill(const double *__restrict__ x, int64_t n, DifCtl *ctl, int32_t *__restrict__ row,
                                                   double *__restrict__ val, double *__restrict__ wgt, int64_t gstride) {
    __shared__ double kept_val[256];
    __shared__ int sh[4];
    __shared__ double norm;
    const int t = threadIdx.x, c = blockIdx.x;
    ctl += blockIdx.y, x += (int64_t)blockIdx.y * gstride;
    if (ctl->src[c] < 0) return;
    const uint64_t thr = ctl->thr[c];
    const int take = ctl->take[c], count = ctl->count[c];
    const int64_t base = ctl->base[c];
    int eq_seen = 0, kept = 0;
    double sum = 0.0;  // thread 0
    for (int64_t first = 0; first < n; first += 256) {
        const int64_t i = first + t;
        const bool valid = i < n;
        const double v = valid ? x[i * COL_B + c] : 0.0;
        const uint64_t key = dif_key(v);
        const bool eq = valid && key == thr;
        int n_eq, n_keep;
        const int eq_pos = dif_excl_scan(eq ? 1 : 0, sh, n_eq);
        const bool keep = valid && (key > thr || (eq && eq_seen + eq_pos < take));
        const int pos = dif_excl_scan(keep ? 1 : 0, sh, n_keep);
        if (keep && kept + pos < count) {
            row[base + kept + pos] = (int32_t)i;
            val[base + kept + pos] = v;
            kept_val[pos] = v;
        }
        __syncthreads();
        const int fits = min(n_keep, count - kept);
        if (t == 0)
            for (int j = 0; j < fits; ++j) sum += kept_val[j];
        __syncthreads();
        eq_seen += n_eq;
        kept += fits;
    }
    if (t == 0) norm = sum > 0.0 ? sum : 1.0;
    __syncthreads();  // val of this column was written by this workgroup
    const double by = norm;
    for (int p = t; p < kept; p += 256) wgt[base + p] = val[base + p] / by;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
struct DifSparse {  // the caller's buffers of dcr_diffusion_sparsify; mode 0: the k largest, 1: the entries >= eps
    int mode;
    int64_t k;
    double eps;
    int64_t *ptr, cap;
    int32_t *row;
    double *weight, *value;
    int64_t nnz;  // out: entries of all columns, also where they did not fit
};

struct HeatPlan {  // the heat solve of a call: t and the number of terms after the first
    double t;
    int64_t K;
};

// K of the heat kernel: the smallest K whose tail ρ_K = Σ_{k > K} θ_k is <= tol / 2, or max_terms where that is lower.  θ_k by its
// recurrence until it has underflowed to zero (t <= 256: within 2,000 terms); the tail is the sum of its terms, small end first,
// never 1 - the partial sum, which could say nothing below 2^-53.
static int64_t heat_terms(double t, double tol, int64_t max_terms) {
    std::vector<double> theta;
    for (double th = std::exp(-t); th > 0.0 && theta.size() < 65536; th *= t / (double)theta.size()) theta.push_back(th);
    int64_t K = (int64_t)theta.size() - 1;  // nothing above it is left to add
    double tail = 0.0;                      // ρ_K
    while (K > 0 && tail + theta[(size_t)K] <= 0.5 * tol) tail += theta[(size_t)K--];
    return std::min(K, max_terms);
}

// sources NULL: column i is node i.  dense: host [P][n], or NULL with `sp` set.  Up to DIF_MAX_GROUPS batches go through the same
// launches as blockIdx.y, each with its own vectors, partials and control block: a column's arithmetic is that of a batch alone.
// heat NULL: the PageRank solve with `o`; else the heat kernel's partial sum, out_residual takes the deficits and `o` plays no part.
static int diffusion_batches(dcr_graph *g, const int32_t *sources, int64_t P, const dcr_diffusion_opts &o, const HeatPlan *heat,
                             double *dense, DifSparse *sp, double *out_residual, int32_t *out_steps) {
    const int64_t n = g->n;
    RowPlan plan;
    DCR_TRY(build_row_plan(g, &plan, nullptr));
    const int nb_mv = (int)row_grid<ColRows>(plan);
    const int nb_el = (int)std::min<int64_t>(COL_UPDATE_BLOCKS, blocks_of(n * COL_CP));
    // batches of a launch: a small graph does not fill the device with one
    const int64_t batches = (P + COL_B - 1) / COL_B;
    const int groups = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(DIF_MAX_GROUPS, batches), DIF_GROUP_NODES / std::max<int64_t>(n, 1)));
    const int64_t gstride = 5 * n * COL_B, pstride = (int64_t)COL_B * std::max(nb_mv, nb_el);

    AnalysisState &A = analysis_of(g);
    DCR_TRY(A.dif_vec.grow(n + groups * gstride));
    DCR_TRY(A.dif_part.grow(groups * pstride));
    DCR_TRY(A.dif_ctl.grow((int64_t)sizeof(DifCtl) * groups));
    // per group z, p, r, x, q (16-byte aligned each), then the scale once; the heat kernel has z by turns in z and p, and x
    double *z = A.dif_vec.p, *p = z + n * COL_B, *r = p + n * COL_B, *x = r + n * COL_B, *q = x + n * COL_B;
    double *s = z + groups * gstride;
    DifCtl *ctl = reinterpret_cast<DifCtl *>(A.dif_ctl.p);
    const ColLayout L = {z, p, r, x, q, s, A.dif_part.p, gstride, pstride, nb_mv, nb_el};
    hipLaunchKernelGGL(k_dif_scale, dim3(blocks_of(n)), dim3(256), 0, g->stream, g->rowinfo.p, s, n);
    DCR_HIP(hipGetLastError());

    const int kk = sp ? (int)std::min<int64_t>(sp->k, n) : 0;
    std::vector<double> host_x;
    if (dense) host_x.resize((size_t)(n * COL_B));
    if (sp) {
        sp->nnz = 0;
        sp->ptr[0] = 0;
    }
    bool fits = true;
    std::vector<DifCtl> h((size_t)groups);
    for (int64_t first = 0; first < P; first += (int64_t)groups * COL_B) {
        const int ng = (int)std::min<int64_t>(groups, (P - first + COL_B - 1) / COL_B);  // groups of this launch
        const dim3 grid_mv((unsigned)nb_mv, (unsigned)ng), grid_el((unsigned)nb_el, (unsigned)ng), grid_col(COL_B, (unsigned)ng);
        std::memset(h.data(), 0, sizeof(DifCtl) * (size_t)ng);
        for (int64_t c = 0; c < (int64_t)ng * COL_B; ++c) {
            DifCtl &hc = h[(size_t)(c / COL_B)];
            const int k = (int)(c % COL_B);
            const bool pad = first + c >= P;
            hc.teleport = o.alpha;
            hc.damp = 1.0 - o.alpha;
            hc.cg.stop[k] = o.tol * o.alpha;
            hc.src[k] = pad ? -1 : sources ? sources[first + c] : (int32_t)(first + c);
            hc.cg.frozen[k] = pad ? 1 : 0;  // padding columns start frozen
            hc.cg.active += pad ? 0 : 1;
            if (sp && sp->mode == 1) hc.thr[k] = dif_key(sp->eps + 0.0);
        }
        DCR_HIP(hipMemcpyAsync(ctl, h.data(), sizeof(DifCtl) * (size_t)ng, hipMemcpyHostToDevice, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));  // h is reused below
        if (heat) {
            hipLaunchKernelGGL(k_heat_start, grid_el, dim3(256), 0, g->stream, s, n, ctl, std::exp(-heat->t), z, x, gstride);
            double *z_in = z, *z_out = p;
            for (int64_t k = 0; k < heat->K; ++k, std::swap(z_in, z_out))
                hipLaunchKernelGGL(k_heat_term, grid_mv, dim3(256), 0, g->stream, plan, g->rowinfo.p, g->col.p, z_in, s, heat->t / (double)(k + 1),
                                   z_out, x, gstride);
            hipLaunchKernelGGL(k_heat_mass, grid_el, dim3(256), 0, g->stream, g->rowinfo.p, n, ctl, x, L.part, gstride, pstride);
        } else {
            DCR_TRY(col_cg_solve(g, plan, L, ng, DifProblem{ctl}, h.data(), o.max_steps));
        }
        if (sp) hipLaunchKernelGGL(k_dif_select, grid_col, dim3(256), 0, g->stream, x, n, ctl, sp->mode, kk, gstride);
        DCR_HIP(hipGetLastError());
        DCR_HIP(hipMemcpyAsync(h.data(), ctl, sizeof(DifCtl) * (size_t)ng, hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));
        int64_t batch = 0;  // entries the columns of this launch keep
        for (int64_t c = 0; c < (int64_t)ng * COL_B; ++c) {
            DifCtl &hc = h[(size_t)(c / COL_B)];
            const int k = (int)(c % COL_B);
            hc.base[k] = batch;
            batch += hc.count[k];
            if (first + c >= P) continue;
            out_residual[first + c] = hc.resid[k];
            if (out_steps) out_steps[first + c] = hc.cg.steps[k];
            if (sp) sp->ptr[first + c + 1] = sp->ptr[first + c] + hc.count[k];
        }
        if (dense) {
            for (int i = 0; i < ng; ++i) {
                DCR_HIP(hipMemcpyAsync(host_x.data(), x + i * gstride, sizeof(double) * (size_t)(n * COL_B), hipMemcpyDeviceToHost, g->stream));
                DCR_HIP(hipStreamSynchronize(g->stream));
                for (int k = 0; k < COL_B && first + (int64_t)i * COL_B + k < P; ++k)
                    for (int64_t v = 0; v < n; ++v) dense[(first + (int64_t)i * COL_B + k) * n + v] = host_x[(size_t)(v * COL_B + k)];
            }
            continue;
        }
        const int64_t at = sp->nnz;
        sp->nnz += batch;
        fits = fits && sp->nnz <= sp->cap;
        if (!fits || batch == 0) continue;  // the remaining columns are still counted
        DCR_TRY(A.dif_row.grow(batch));
        DCR_TRY(A.dif_val.grow(2 * batch));
        int32_t *row = A.dif_row.p;  // both taken after this launch's grow
        double *val = A.dif_val.p, *wgt = val + batch;
        for (int i = 0; i < ng; ++i)
            DCR_HIP(hipMemcpyAsync(ctl[i].base, h[(size_t)i].base, sizeof(h[0].base), hipMemcpyHostToDevice, g->stream));
        hipLaunchKernelGGL(k_dif_fill, grid_col, dim3(256), 0, g->stream, x, n, ctl, row, val, wgt, gstride);
        DCR_HIP(hipGetLastError());
        DCR_HIP(hipMemcpyAsync(sp->row + at, row, sizeof(int32_t) * (size_t)batch, hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipMemcpyAsync(sp->value + at, val, sizeof(double) * (size_t)batch, hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipMemcpyAsync(sp->weight + at, wgt, sizeof(double) * (size_t)batch, hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));
    }
    if (!fits) DCR_FAIL(DCR_ECAPACITY, "diffusion: " + std::to_string(sp->nnz) + " entries kept, room for " + std::to_string(sp->cap));
    return DCR_OK;
}

static int diffusion_opts(const dcr_diffusion_opts *opts, dcr_diffusion_opts *o) {
    *o = {0.15, 1e-10, 20000};
    if (opts) *o = *opts;
    if (!(o->alpha > 0.0 && o->alpha < 1.0)) DCR_FAIL(DCR_EINVAL, "alpha must lie in (0, 1)");
    if (!(o->tol >= 0.0) || o->max_steps < 1) DCR_FAIL(DCR_EINVAL, "tol must be >= 0, max_steps >= 1");
    return DCR_OK;
}

static int heat_opts(const dcr_heat_opts *opts, dcr_heat_opts *o) {
    *o = {5.0, 1e-10, 4096};
    if (opts) *o = *opts;
    if (!(o->t > 0.0 && o->t <= 256.0)) DCR_FAIL(DCR_EINVAL, "t must lie in (0, 256]");
    if (!(o->tol >= 0.0) || o->max_terms < 1) DCR_FAIL(DCR_EINVAL, "tol must be >= 0, max_terms >= 1");
    return DCR_OK;
}

static int diffusion_sources(const dcr_graph *g, const int32_t *sources, int64_t P) {
    if (P < 0) DCR_FAIL(DCR_EINVAL, "the number of sources must be >= 0");
    if (!sources && P != g->n) DCR_FAIL(DCR_EINVAL, "sources NULL stands for all nodes: P must be num_nodes");
    for (int64_t i = 0; sources && i < P; ++i)
        if (sources[i] < 0 || sources[i] >= g->n) DCR_FAIL(DCR_EINVAL, "source " + std::to_string(i) + " outside 0 .. num_nodes - 1");
    return DCR_OK;
}

// what dcr_diffusion_sparsify and dcr_heat_sparsify share once their options are read: the remaining argument checks, the
// capacity of a top-k call, the solve and selection
static int sparsify_call(dcr_graph *g, const int32_t *sources, int64_t P, const dcr_diffusion_opts &o, const HeatPlan *heat, DifSparse *sp,
                         double *out_residual, int32_t *out_steps, int64_t *out_nnz) {
    if (sp->cap < 0 || (sp->cap > 0 && (!sp->row || !sp->weight || !sp->value)))
        DCR_FAIL(DCR_EINVAL, "cap entries of row, weight and value are needed");
    if (sp->mode != 0 && sp->mode != 1) DCR_FAIL(DCR_EINVAL, "mode must be 0 (top-k) or 1 (threshold)");
    if (sp->mode == 0 && sp->k < 1) DCR_FAIL(DCR_EINVAL, "k must be >= 1");
    if (sp->mode == 1 && !(sp->eps == sp->eps)) DCR_FAIL(DCR_EINVAL, "eps must not be NaN");
    DCR_TRY(diffusion_sources(g, sources, P));
    if (P == 0) return DCR_OK;
    if (sp->mode == 0) {  // the size is known before any solve
        const int64_t need = P * std::min<int64_t>(sp->k, g->n);
        if (need > sp->cap) {
            *out_nnz = need;
            DCR_FAIL(DCR_ECAPACITY, "diffusion: " + std::to_string(need) + " entries kept, room for " + std::to_string(sp->cap));
        }
    }
    DCR_HIP(hipSetDevice(g->device));
    const int rc = diffusion_batches(g, sources, P, o, heat, nullptr, sp, out_residual, out_steps);
    if (rc == DCR_OK || rc == DCR_ECAPACITY) *out_nnz = sp->nnz;
    return rc;
}

}  // namespace dcr

using namespace dcr;

extern "C" {

int dcr_ppr_columns(dcr_graph *g, const int32_t *sources, int64_t P, const dcr_diffusion_opts *opts, double *out, double *out_residual,
                    int32_t *out_steps) {
    if (!g || !sources || !out || !out_residual) DCR_FAIL(DCR_EINVAL, "null argument");
    dcr_diffusion_opts o;
    DCR_TRY(diffusion_opts(opts, &o));
    DCR_TRY(diffusion_sources(g, sources, P));
    if (P == 0) return DCR_OK;
    DCR_HIP(hipSetDevice(g->device));
    return diffusion_batches(g, sources, P, o, nullptr, out, nullptr, out_residual, out_steps);
}

int dcr_diffusion_sparsify(dcr_graph *g, const int32_t *sources, int64_t P, const dcr_diffusion_opts *opts, int mode, int64_t k, double eps,
                           int64_t *out_ptr, int64_t cap, int32_t *out_row, double *out_weight, double *out_value, double *out_residual,
                           int32_t *out_steps, int64_t *out_nnz) {
    if (!g || !out_ptr || !out_residual || !out_nnz) DCR_FAIL(DCR_EINVAL, "null argument");
    dcr_diffusion_opts o;
    DCR_TRY(diffusion_opts(opts, &o));
    DifSparse sp = {mode, k, eps, out_ptr, cap, out_row, out_weight, out_value, 0};
    return sparsify_call(g, sources, P, o, nullptr, &sp, out_residual, out_steps, out_nnz);
}

int dcr_heat_columns(dcr_graph *g, const int32_t *sources, int64_t P, const dcr_heat_opts *opts, double *out, double *out_deficit,
                     int64_t *out_terms) {
    if (!g || !sources || !out || !out_deficit) DCR_FAIL(DCR_EINVAL, "null argument");
    dcr_heat_opts o;
    DCR_TRY(heat_opts(opts, &o));
    DCR_TRY(diffusion_sources(g, sources, P));
    if (P == 0) return DCR_OK;
    const HeatPlan heat = {o.t, heat_terms(o.t, o.tol, o.max_terms)};
    if (out_terms) *out_terms = heat.K;
    DCR_HIP(hipSetDevice(g->device));
    return diffusion_batches(g, sources, P, {}, &heat, out, nullptr, out_deficit, nullptr);
}

int dcr_heat_sparsify(dcr_graph *g, const int32_t *sources, int64_t P, const dcr_heat_opts *opts, int mode, int64_t k, double eps,
                      int64_t *out_ptr, int64_t cap, int32_t *out_row, double *out_weight, double *out_value, double *out_deficit,
                      int64_t *out_terms, int64_t *out_nnz) {
    if (!g || !out_ptr || !out_deficit || !out_nnz) DCR_FAIL(DCR_EINVAL, "null argument");
    dcr_heat_opts o;
    DCR_TRY(heat_opts(opts, &o));
    const HeatPlan heat = {o.t, heat_terms(o.t, o.tol, o.max_terms)};
    DifSparse sp = {mode, k, eps, out_ptr, cap, out_row, out_weight, out_value, 0};
    const int rc = sparsify_call(g, sources, P, {}, &heat, &sp, out_deficit, nullptr, out_nnz);
    if (out_terms && P > 0 && (rc == DCR_OK || rc == DCR_ECAPACITY)) *out_terms = heat.K;
    return rc;
}

}  // extern "C"
