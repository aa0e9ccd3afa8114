// What the graph-analysis translation units share (dcr_cheeger.hip, dcr_spectral.hip, dcr_sweep.hip, dcr_resistance.hip,
// dcr_resistance_sketch.hip, dcr_diffusion.hip, dcr_fosr.hip, dcr_hops.hip, dcr_betweenness.hip) and the
// curvature pass, SDRF and the GCN do not need: the deterministic reductions, the row plan and the row walker, the Cheeger ratio,
// the analysis buffers of a graph, and the batched column CG that the resistance and diffusion solves share.  A new analysis
// feature adds its buffers (one line each in AnalysisState, of the owning DevBuf type of dcr_internal.h) and declarations here;
// dcr_internal.h and dcr_graph.hip stay as they are.
#pragma once
#include "dcr_internal.h"

namespace dcr {

constexpr int SP_SHORT_DEG = 32;    // rows up to this degree: a lane group a row
constexpr int SP_LONG_DEG = 2048;   // rows above this degree: a workgroup a row
constexpr int SP_CHECK_EVERY = 8;   // solver steps between host synchronisations

inline unsigned blocks_of(int64_t n, int64_t per = 256) { return (unsigned)((n + per - 1) / per); }
__device__ inline double inv_sqrt_deg(int d) { return d > 0 ? 1.0 / sqrt((double)d) : 0.0; }  // the scale s of a node of degree d

// ---- deterministic reductions: no floating-point atomics; per-workgroup partials go through the L2 (st_agent), the last arriver
// closes them in index order (ld_agent) -------------------------------------------------------------------------------------------
__device__ inline double ld_agent(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_agent(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename T>
__device__ inline T xor_add(T x, int off) {
    return x + __shfl_xor(x, off);
}
__device__ inline double2 xor_add(double2 x, int off) {  // two columns, each on its own
    x.x += __shfl_xor(x.x, off);
    x.y += __shfl_xor(x.y, off);
    return x;
}

// x summed over LANES consecutive lanes of a wave; with NODE > 1 over those of them that hold the same column (lane % NODE).
// A butterfly: every lane ends with the same bits (a + b == b + a).
template <int LANES, int NODE, typename T>
__device__ inline T group_sum(T x) {
#pragma unroll
    for (int off = LANES / 2; off >= NODE; off >>= 1) x = xor_add(x, off);
    return x;
}
template <typename T>
__device__ inline T wave_sum(T x) {
    return group_sum<64, 1>(x);
}

// 256 threads: the same over the workgroup, the four wave sums added in wave order.  sh: 4 NODE entries, free again on return.
template <int NODE = 1, typename T>
__device__ inline T block_sum(T x, T *sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane % NODE;
    x = group_sum<64, NODE>(x);
    if (lane < NODE) sh[wave * NODE + lane] = x;
    __syncthreads();
    const T r = ((sh[c] + sh[NODE + c]) + sh[2 * NODE + c]) + sh[3 * NODE + c];
    __syncthreads();
    return r;
}

// sum of other workgroups' partials part[0 .. count): thread t takes t, t + 256, ... in order, then block_sum
__device__ inline double close_partials(const double *part, int64_t count, double *sh) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += 256) acc += ld_agent(part + i);
    return block_sum(acc, sh);
}

// ---- the ratio of a node set from its edge counts (experiment/compute_cheeger.py:40-45) --------------------------------------------
// in / lo / hi: edges a < b with both ends inside, only a inside, only b inside.  definition 0: lo / min(2 in, 2 out);
// 1: (lo + hi) / min(2 in + lo + hi, 2 out + lo + hi).  inf where the smaller volume is zero.  One IEEE float64 division of two
// integers below 2^53.
__device__ inline double cheeger_ratio(int64_t in, int64_t lo, int64_t hi, int64_t n_edges, int definition) {
    const int64_t outside = n_edges - in - lo - hi;
    const int64_t cut = definition ? lo + hi : lo, extra = definition ? lo + hi : 0;
    const int64_t va = 2 * in + extra, vb = 2 * outside + extra, m = va < vb ? va : vb;
    return m == 0 ? __builtin_inf() : (double)cut / (double)m;
}

// ---- rows by degree class ----------------------------------------------------------------------------------------------------------
// The device list holds the long rows (degree above SP_LONG_DEG), then the medium ones, then the short ones (up to SP_SHORT_DEG),
// each by node id.  A kernel that walks it gives a workgroup to a long row, a wave to a medium one and a lane group to a short
// one; workgroups come in the same order, so the longest work starts first.
struct RowPlan {
    const int32_t *rows;
    int n_long, n_mid, n_short;
};

// How a kernel of 256 threads walks the short rows: groups of SHORT_LANES lanes, TURNS rows per group one after the other; and,
// for every class, NODE adjacent lanes on the same slot (each with its own columns of a node-major vector).
template <int SHORT_LANES = 8, int TURNS = 1, int NODE = 1>
struct RowGeom {
    static constexpr int short_lanes = SHORT_LANES, turns = TURNS, node = NODE;
    static constexpr int short_rows = 256 / SHORT_LANES * TURNS;  // per workgroup
};

template <class G>
inline unsigned row_grid(const RowPlan &p) {
    return (unsigned)p.n_long + blocks_of(p.n_mid, 4) + blocks_of(p.n_short, G::short_rows);
}

// The lanes on one row: LANES consecutive lanes of a wave, or the workgroup (256).  Lane l takes slots first(), first() + stride,
// ...; sum() adds over the scope (per column where NODE > 1), the same bits in every lane; owner() marks the NODE lanes that
// finish the row.  sh is the kernel's 4 NODE entries of LDS, used by the workgroup scope only.
template <int LANES, int NODE, typename S>
struct RowScope {
    S *sh;
    static constexpr int stride = LANES / NODE;
    __device__ int first() const { return (int)(threadIdx.x & (LANES - 1)) / NODE; }
    __device__ bool owner() const { return (int)(threadIdx.x & (LANES - 1)) < NODE; }
    __device__ S sum(S x) const {
        if constexpr (LANES == 256)
            return block_sum<NODE>(x, sh);
        else
            return group_sum<LANES, NODE>(x);
    }
};

// Calls body(scope, row, {start, degree}, acc...) for every row this thread works on: the class from blockIdx.x, the row from the
// plan, nothing for the waves and groups past the end of a class.  body is a lambda that captures BY VALUE (pointers and
// scalars); what it accumulates comes in as reference parameters, as in ext_take: everything inlines and stays in registers.
// All lanes of a scope reach body together, so it may call scope.sum().
template <class G, typename S, class Body, typename... Acc>
__device__ __forceinline__ void walk_rows(const RowPlan &plan, const int2 *__restrict__ rowinfo, S *sh, Body body, Acc &...acc) {
    const int t = threadIdx.x;
    const int b_mid = (int)blockIdx.x - plan.n_long, b_short = b_mid - (plan.n_mid + 3) / 4;
    if (b_mid < 0) {
        const int32_t row = plan.rows[blockIdx.x];
        body(RowScope<256, G::node, S>{sh}, row, rowinfo[row], acc...);
    } else if (b_short < 0) {
        const int i = b_mid * 4 + (t >> 6);
        if (i >= plan.n_mid) return;
        const int32_t row = plan.rows[plan.n_long + i];
        body(RowScope<64, G::node, S>{sh}, row, rowinfo[row], acc...);
    } else {
        for (int turn = 0; turn < G::turns; ++turn) {
            const int i = b_short * G::short_rows + turn * (256 / G::short_lanes) + t / G::short_lanes;
            if (i >= plan.n_short) return;
            const int32_t row = plan.rows[plan.n_long + plan.n_mid + i];
            body(RowScope<G::short_lanes, G::node, S>{sh}, row, rowinfo[row], acc...);
        }
    }
}

// ---- the analysis buffers of a graph, grown on demand; dcr_graph::analysis, created on first use (analysis_of) ----------------------
struct AnalysisState {
    DevBuf<int32_t> rows;         // [n] rows by degree class (build_row_plan)

    // Monte-Carlo Cheeger estimate (dcr_cheeger.hip): membership words [n][W], counts [3][64 W], ratios [64 W]
    DevBuf<uint64_t> chg_members;
    DevBuf<unsigned long long> chg_counts;
    DevBuf<double> chg_values;

    // connected components (dcr_analysis.hip) and the spectral gap (dcr_spectral.hip)
    DevBuf<int32_t> spc_label;    // [n] smallest node id of the node's component
    DevBuf<unsigned> spc_ctl;     // {a sweep of the components changed a label, reduction ticket, -, -}
    DevBuf<double> spc_vec;       // [4][n]: scale s, null-space weights k, z = s ⊙ v of the newest column, work vector w
    DevBuf<double> spc_basis;     // [columns][n] Lanczos basis
    DevBuf<int32_t> spc_rows;     // [n]: nodes by component
    DevBuf<int4> spc_chunks;      // deflation chunks
    DevBuf<double> spc_part;      // per-workgroup (per-wave) partial sums
    DevBuf<double> spc_small;     // alpha [m], beta [m], 8 scalars, Gram-Schmidt coefficients [m], Ritz coefficients [m]

    // effective resistance (dcr_resistance.hip): O(n B), B the columns of a batch
    DevBuf<double> res_vec;       // z, p, r, y, q as [n][B] each, then s [n]
    DevBuf<double> res_part;      // per-workgroup partial sums, B per workgroup (2 B in the closing mat-vec)
    DevBuf<unsigned char> res_ctl;  // the batch's control block (ResCtl of dcr_resistance.hip)

    // sweep cut (dcr_sweep.hip): all O(n)
    DevBuf<uint64_t> swp_keys;    // [2][n] sort keys, ping and pong
    DevBuf<int32_t> swp_idx;      // [6][n]: node ids ping and pong, rank, the three difference arrays (in, lo, hi)
    DevBuf<int32_t> swp_table;    // [256][tiles] digit counts of a sort pass, then the scans' per-block sums and offsets
    DevBuf<double> swp_f64;       // [2][n]: the score, the profile
    DevBuf<unsigned> swp_ctl;     // tickets, NaN flag, the [8][256] digit histogram of the keys, the result block, arg-min partials

    // PageRank diffusion (dcr_diffusion.hip): O(n B) for the solve, O(entries kept by one batch) for the selection
    DevBuf<double> dif_vec;       // z, p, r, x, q as [n][B] each, then the scale [n]
    DevBuf<double> dif_part;      // per-workgroup partial sums, B per workgroup
    DevBuf<unsigned char> dif_ctl;  // the batch's control block (DifCtl of dcr_diffusion.hip)
    DevBuf<int32_t> dif_row;     // the node ids a batch keeps, column after column
    DevBuf<double> dif_val;       // their values, then their weights

    // FoSR (dcr_fosr.hip): all O(n)
    DevBuf<double> fsr_vec;       // [4][n]: the iterate x, its projection, s ⊙ projection, z
    DevBuf<double> fsr_part;      // per-workgroup partials: sums, or (product, {u, partner}) pairs of the pick
    DevBuf<unsigned char> fsr_ctl;  // tickets and the result block (FsrCtl of dcr_fosr.hip)

    // hop distances (dcr_hops.hip): O(n W) words, W <= 4 the words of a batch of 64 W sources; O(64 W n) only where rows are asked for
    DevBuf<uint64_t> hop_bits;    // visited, frontier, next as [n][W] each
    DevBuf<unsigned char> hop_ctl;  // the batch's running totals [256] (64-bit), then its sources [256]
    DevBuf<int32_t> hop_dist;     // [64 W][n] distance rows of a batch

    // betweenness (dcr_betweenness.hip): O(16 n) for a batch of 16 sources; O(adjacency slots) only where edge values are asked for
    DevBuf<int32_t> btw_dist;     // [n][16] the level of the node for each source of the batch, -1: not reached
    DevBuf<double> btw_f64;       // sigma, delta as [n][16] each, then the sum over the batches [n]
    DevBuf<double> btw_slot;      // [cap_total] the sum over the batches per adjacency slot
    DevBuf<unsigned char> btw_ctl;  // the batch's control block (BtwCtl of dcr_betweenness.hip)

    // resistance sketch (dcr_resistance_sketch.hip): O(n B) per group of a launch; O(adjacency slots) only where edge values are asked for
    DevBuf<double> skt_vec;       // per group z, p, r, y, q and the right-hand side s ⊙ b as [n][B] each, then s [n]
    DevBuf<double> skt_part;      // per-workgroup partial sums, B per workgroup, per group
    DevBuf<unsigned char> skt_ctl;  // the groups' control blocks (SktCtl of dcr_resistance_sketch.hip)
    DevBuf<double> skt_slot;     // [cap_total] the sum over the columns per adjacency slot
    DevBuf<double> skt_pair;      // [P] the same per given pair
    DevBuf<int32_t> skt_pair_idx;  // [2][P] the pairs' endpoints
};

AnalysisState &analysis_of(dcr_graph *g);  // dcr_analysis.hip: the graph's state, created on first use

// ---- batched column conjugate gradients (dcr_resistance.hip, dcr_resistance_sketch.hip, dcr_diffusion.hip) ----------------------------------------------------
// COL_B right-hand sides are solved at a time as COL_B independent CGs in step (not a block CG), from the iterate x = 0.  Every
// vector is node-major [n][COL_B]: the gather of one neighbour reads COL_B contiguous doubles (a whole 128-byte line at 16 columns).
// A lane owns two adjacent columns (16-byte loads and stores); COL_CP lanes cover a node.  Each column has its own step length,
// beta, |r|^2, stop threshold, step count and frozen flag in device memory (ColCg).  A column freezes, on the device, in the step
// where |r| <= its threshold, or where p^T (operator) p is not a positive finite number; a frozen column's x, r and p are no longer
// written.  Every sum runs over rows or nodes in an order that the graph alone fixes and treats all columns alike, so a column's
// bits depend on its own right-hand side only: not on its column index, not on what shares the batch, not on when the others
// freeze.  Several batches ("groups") share a launch as blockIdx.y, each with its own vectors, partials and control block.
//
// A problem type P says what is solved.  It holds `Ctl *ctl`, the groups' control blocks, each with a ColCg member `cg`, and gives
//   P::closing_dot        whether the closing mat-vec also reduces x^T w
//   rhs(cp)               a lambda (node, s_node) -> the lane's two entries of the right-hand side
//   entry()               a lambda (degree, x_row, s_row, (A z)_row, z_row) -> the row's entry of the operator on x, for one column
//   start(k, s)           sets cg.rr[k] = |rhs|^2 of column k (and cg.stop[k], where the host has not)
//   close(k, x, s, dot, dev)  takes column k's sums of the closing mat-vec: x^T w (with closing_dot) and |rhs - w|^2
// in the style of walk_rows: the lambdas capture what they read from the control block by value, once per thread.
#ifndef DCR_COL_B
#define DCR_COL_B 16  // columns of a batch: 8 or 16 (DESIGN §4.8 has the code-object figures of both)
#endif
constexpr int COL_B = DCR_COL_B;
constexpr int COL_CP = COL_B / 2;        // lanes across a node: two columns each
constexpr int COL_SHORT_LANES = 32;      // lanes of a short row's group
constexpr int COL_SHORT_ROWS = 64;       // short rows a workgroup takes: 8 groups x 8 turns
using ColRows = RowGeom<COL_SHORT_LANES, COL_SHORT_ROWS / 8, COL_CP>;
constexpr int COL_UPDATE_BLOCKS = 1024;  // most workgroups of the element-wise kernels with a reduction
static_assert(COL_B == 8 || COL_B == 16, "a batch has 8 or 16 columns");

struct ColCg {  // the CG part of a batch's control block
    double rr[COL_B];    // |r|^2 of the recurrence
    double gain[COL_B];  // the step length (CG's "alpha")
    double beta[COL_B];
    double stop[COL_B];  // the column freezes at |r| <= stop
    int32_t frozen[COL_B];
    int32_t steps[COL_B];
    int32_t active;      // columns not frozen
    unsigned ticket;
};

__device__ inline double2 ld2(const double *base, int64_t node, int cp) {
    return *reinterpret_cast<const double2 *>(base + node * COL_B + 2 * cp);
}
__device__ inline void st2(double *base, int64_t node, int cp, double2 x) { *reinterpret_cast<double2 *>(base + node * COL_B + 2 * cp) = x; }

// partials part[workgroup][COL_B] of `count` workgroups: thread t adds those of workgroups t / COL_CP, + 256 / COL_CP, ... for its
// column pair in order, then the workgroup's sum per column pair.  sh: 4 COL_CP entries, free again on return.
__device__ inline double2 close_partials(const double *part, int count, double2 *sh) {
    const int cp = threadIdx.x % COL_CP;
    double2 acc = make_double2(0.0, 0.0);
    for (int i = threadIdx.x / COL_CP; i < count; i += 256 / COL_CP) {
        acc.x += ld_agent(part + (int64_t)i * COL_B + 2 * cp);
        acc.y += ld_agent(part + (int64_t)i * COL_B + 2 * cp + 1);
    }
    return block_sum<COL_CP>(acc, sh);
}

__device__ inline void store_partial(double *part, int block, double2 x) {  // threads 0 .. COL_CP - 1
    st_agent(part + (int64_t)block * COL_B + 2 * threadIdx.x, x.x);
    st_agent(part + (int64_t)block * COL_B + 2 * threadIdx.x + 1, x.y);
}

// (A z)_row for the lane's column pair: the row's neighbours over the lanes of the scope, then the scope's sum
template <class Scope>
__device__ __forceinline__ double2 gather(Scope scope, const int32_t *__restrict__ col, int2 ri, const double *__restrict__ z, int cp) {
    double2 acc = make_double2(0.0, 0.0);
    for (int j = scope.first(); j < ri.y; j += scope.stride) {
        const double2 zv = ld2(z, col[ri.x + j], cp);
        acc.x += zv.x;
        acc.y += zv.y;
    }
    return scope.sum(acc);
}

// r = p = rhs, z = s ⊙ p, x = 0 for all columns; |rhs|^2 per column
template <class P>
__global__ void __launch_bounds__(256) k_col_start(P prob, const double *__restrict__ s, int64_t n, double *__restrict__ z,
                                                    double *__restrict__ p, double *__restrict__ r, double *__restrict__ x, int64_t gstride) {
    const int cp = threadIdx.x % COL_CP;
    const int64_t go = (int64_t)blockIdx.y * gstride;  // this group's vectors and control block
    prob.ctl += blockIdx.y, z += go, p += go, r += go, x += go;
    const auto rhs = prob.rhs(cp);
    const int64_t total = n * COL_CP;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t node = e / COL_CP;
        const double sn = s[node];
        const double2 c = rhs((int32_t)node, sn);
        st2(p, node, cp, c);
        st2(r, node, cp, c);
        st2(z, node, cp, make_double2(sn * c.x, sn * c.y));
        st2(x, node, cp, make_double2(0.0, 0.0));
    }
    if (blockIdx.x == 0 && threadIdx.x < COL_B) prob.start(threadIdx.x, s);
}

// MODE 0: v = p, q = (operator) p stored for all columns in one sweep of the rows, through walk_rows in the three degree classes
// (<= 32: 32 lanes a row, 64 rows a workgroup; <= 2048: a wave a row; above: a workgroup a row, those first); partials of p^T q;
// the last arriver sets the step length |r|^2 / p^T q or freezes the column.  MODE 1, the close: v = x, w = (operator) x not stored,
// partials of x^T w (with P::closing_dot) and, behind them, of |rhs - w|^2; the last arriver hands the sums to P::close.
template <class P, int MODE>
__global__ void __launch_bounds__(256) k_col_matvec(P prob, RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                     const double *__restrict__ v, const double *__restrict__ z,
                                                     const double *__restrict__ s, double *__restrict__ q, double *part, int64_t gstride,
                                                     int64_t pstride) {
    constexpr bool DOT = MODE == 0 || P::closing_dot;
    __shared__ double2 sh[4 * COL_CP];
    const int t = threadIdx.x, cp = t % COL_CP;
    const int64_t go = (int64_t)blockIdx.y * gstride;
    prob.ctl += blockIdx.y, v += go, z += go, q += go, part += (int64_t)blockIdx.y * pstride;
    ColCg *cg = &prob.ctl->cg;
    const auto entry = prob.entry();
    const auto rhs = prob.rhs(cp);
    double2 dot = make_double2(0.0, 0.0), dev = make_double2(0.0, 0.0);
    walk_rows<ColRows>(plan, rowinfo, sh, [=](auto scope, int32_t row, int2 ri, double2 &vw, double2 &ee) {
        const double2 acc = gather(scope, col, ri, z, cp);
        if (!scope.owner()) return;
        // the row's entry of the operator on v, by the COL_CP lanes that own the row
        const double2 vu = ld2(v, row, cp), zu = ld2(z, row, cp);
        const double su = s[row];
        const double2 w = make_double2(entry(ri.y, vu.x, su, acc.x, zu.x), entry(ri.y, vu.y, su, acc.y, zu.y));
        if (DOT) {
            vw.x += vu.x * w.x;
            vw.y += vu.y * w.y;
        }
        if (MODE == 0) {
            st2(q, row, cp, w);
        } else {
            const double2 c = rhs(row, su);
            const double e0 = c.x - w.x, e1 = c.y - w.y;
            ee.x += e0 * e0;
            ee.y += e1 * e1;
        }
    }, dot, dev);
    double *part_dev = part + (DOT ? (int64_t)gridDim.x * COL_B : 0);
    if (DOT) {
        dot = block_sum<COL_CP>(dot, sh);
        if (t < COL_CP) store_partial(part, blockIdx.x, dot);
    }
    if (MODE == 1) {
        dev = block_sum<COL_CP>(dev, sh);
        if (t < COL_CP) store_partial(part_dev, blockIdx.x, dev);
    }
    if (!last_arriver(&cg->ticket, (unsigned)gridDim.x)) return;
    double2 a = make_double2(0.0, 0.0), d = make_double2(0.0, 0.0);
    if (DOT) a = close_partials(part, gridDim.x, sh);
    if (MODE == 1) d = close_partials(part_dev, gridDim.x, sh);
    if (t < COL_CP) {
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * t + h;
            const double sum = h ? a.y : a.x;
            if (MODE == 1) {
                prob.close(k, v, s, sum, h ? d.y : d.x);
            } else if (!cg->frozen[k]) {
                if (sum > 0.0 && sum <= 1.79769313486231570815e308) {
                    cg->gain[k] = cg->rr[k] / sum;
                } else {  // p^T (operator) p zero, negative or not finite: nothing more to gain along p
                    cg->gain[k] = 0.0;
                    cg->frozen[k] = 1;
                }
            }
        }
    }
    if (t == 0) __hip_atomic_store(&cg->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// x += gain p, r -= gain q, partials of the new |r|^2; the last arriver sets beta, counts the step, freezes the columns that have
// converged and counts the active ones
template <class Ctl>
__global__ void __launch_bounds__(256) k_col_update(int64_t n, Ctl *ctl, const double *__restrict__ p, const double *__restrict__ q,
                                                     double *__restrict__ x, double *__restrict__ r, double *part, int64_t gstride,
                                                     int64_t pstride) {
    __shared__ double2 sh[4 * COL_CP];
    const int t = threadIdx.x, cp = t % COL_CP;
    const int64_t go = (int64_t)blockIdx.y * gstride;
    p += go, q += go, x += go, r += go, part += (int64_t)blockIdx.y * pstride;
    ColCg *cg = &ctl[blockIdx.y].cg;
    const double a0 = cg->gain[2 * cp], a1 = cg->gain[2 * cp + 1];
    const bool f0 = cg->frozen[2 * cp] != 0, f1 = cg->frozen[2 * cp + 1] != 0;
    double2 acc = make_double2(0.0, 0.0);
    if (!(f0 && f1)) {
        const int64_t total = n * COL_CP;
        for (int64_t e = (int64_t)blockIdx.x * 256 + t; e < total; e += (int64_t)gridDim.x * 256) {
            const int64_t node = e / COL_CP;
            const double2 pv = ld2(p, node, cp), qv = ld2(q, node, cp);
            double2 xv = ld2(x, node, cp), rv = ld2(r, node, cp);
            if (!f0) {
                xv.x += a0 * pv.x;
                rv.x -= a0 * qv.x;
            }
            if (!f1) {
                xv.y += a1 * pv.y;
                rv.y -= a1 * qv.y;
            }
            st2(x, node, cp, xv);
            st2(r, node, cp, rv);
            acc.x += rv.x * rv.x;
            acc.y += rv.y * rv.y;
        }
    }
    acc = block_sum<COL_CP>(acc, sh);
    if (t < COL_CP) store_partial(part, blockIdx.x, acc);
    if (!last_arriver(&cg->ticket, (unsigned)gridDim.x)) return;
    const double2 a = close_partials(part, gridDim.x, sh);
    if (t < COL_CP) {
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * t + h;
            if (cg->frozen[k]) continue;
            const double rr = h ? a.y : a.x;
            cg->beta[k] = rr / cg->rr[k];
            cg->rr[k] = rr;
            cg->steps[k] += 1;
            if (!(rr <= 1.79769313486231570815e308) || sqrt(rr) <= cg->stop[k]) cg->frozen[k] = 1;
        }
    }
    __syncthreads();
    if (t == 0) {
        int active = 0;
        for (int k = 0; k < COL_B; ++k) active += cg->frozen[k] == 0;
        cg->active = active;
        __hip_atomic_store(&cg->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// p = r + beta p, z = s ⊙ p
template <class Ctl>
__global__ void __launch_bounds__(256) k_col_direction(int64_t n, const Ctl *__restrict__ ctl, const double *__restrict__ s,
                                                        const double *__restrict__ r, double *__restrict__ p, double *__restrict__ z,
                                                        int64_t gstride) {
    const int cp = threadIdx.x % COL_CP;
    const int64_t go = (int64_t)blockIdx.y * gstride;
    r += go, p += go, z += go;
    const ColCg *cg = &ctl[blockIdx.y].cg;
    const double b0 = cg->beta[2 * cp], b1 = cg->beta[2 * cp + 1];
    const bool f0 = cg->frozen[2 * cp] != 0, f1 = cg->frozen[2 * cp + 1] != 0;
    if (f0 && f1) return;
    const int64_t total = n * COL_CP;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t node = e / COL_CP;
        const double2 rv = ld2(r, node, cp);
        double2 pv = ld2(p, node, cp);
        if (!f0) pv.x = rv.x + b0 * pv.x;
        if (!f1) pv.y = rv.y + b1 * pv.y;
        const double sn = s[node];
        st2(p, node, cp, pv);
        st2(z, node, cp, make_double2(sn * pv.x, sn * pv.y));
    }
}

// z = s ⊙ x, ahead of the closing mat-vec (a template like the others so that only the files that solve instantiate it)
template <class P>
__global__ void __launch_bounds__(256) k_col_scale(int64_t n, const double *__restrict__ s, const double *__restrict__ x,
                                                    double *__restrict__ z, int64_t gstride) {
    const int cp = threadIdx.x % COL_CP;
    x += (int64_t)blockIdx.y * gstride, z += (int64_t)blockIdx.y * gstride;
    const int64_t total = n * COL_CP;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t node = e / COL_CP;
        const double sn = s[node];
        const double2 xv = ld2(x, node, cp);
        st2(z, node, cp, make_double2(sn * xv.x, sn * xv.y));
    }
}

struct ColLayout {  // where a solve's vectors lie and how its kernels are launched; the caller owns every buffer
    double *z, *p, *r, *x, *q;  // group 0: [n][COL_B] each, 16-byte aligned; z = s ⊙ p, the iterate x, q = (operator) p
    const double *s;            // [n] the scale, the same for every group
    double *part;               // group 0: COL_B partials per workgroup (2 COL_B in a closing mat-vec with closing_dot)
    int64_t gstride, pstride;   // from a group's vectors and partials to the next group's
    int nb_mv, nb_el;           // workgroups per group: the row sweep, the element-wise kernels
};

// The solve of `ng` groups whose control blocks the caller has filled: the start, three launches a step (mat-vec, update,
// direction), then the scale and the closing mat-vec.  Every SP_CHECK_EVERY steps and at max_steps the control blocks come back
// into host[0 .. ng), and the steps end when no column of any group is active.
template <class P>
int col_cg_solve(dcr_graph *g, const RowPlan &plan, const ColLayout &L, int ng, P prob, typename P::Ctl *host, int64_t max_steps) {
    const dim3 grid_mv((unsigned)L.nb_mv, (unsigned)ng), grid_el((unsigned)L.nb_el, (unsigned)ng);
    const int64_t n = g->n;
    hipLaunchKernelGGL(k_col_start<P>, grid_el, dim3(256), 0, g->stream, prob, L.s, n, L.z, L.p, L.r, L.x, L.gstride);
    for (int64_t step = 0; step < max_steps; ++step) {
        hipLaunchKernelGGL((k_col_matvec<P, 0>), grid_mv, dim3(256), 0, g->stream, prob, plan, g->rowinfo.p, g->col.p, L.p, L.z, L.s, L.q, L.part,
                           L.gstride, L.pstride);
        hipLaunchKernelGGL(k_col_update<typename P::Ctl>, grid_el, dim3(256), 0, g->stream, n, prob.ctl, L.p, L.q, L.x, L.r, L.part, L.gstride,
                           L.pstride);
        hipLaunchKernelGGL(k_col_direction<typename P::Ctl>, grid_el, dim3(256), 0, g->stream, n, prob.ctl, L.s, L.r, L.p, L.z, L.gstride);
        if ((step + 1) % SP_CHECK_EVERY != 0 && step + 1 != max_steps) continue;
        DCR_HIP(hipGetLastError());
        DCR_HIP(hipMemcpyAsync(host, prob.ctl, sizeof(*host) * (size_t)ng, hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));
        int active = 0;
        for (int i = 0; i < ng; ++i) active += host[i].cg.active;
        if (active == 0) break;
    }
    hipLaunchKernelGGL(k_col_scale<P>, grid_el, dim3(256), 0, g->stream, n, L.s, L.x, L.z, L.gstride);
    hipLaunchKernelGGL((k_col_matvec<P, 1>), grid_mv, dim3(256), 0, g->stream, prob, plan, g->rowinfo.p, g->col.p, L.x, L.z, L.s, L.q, L.part,
                       L.gstride, L.pstride);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

// dcr_analysis.hip
// one download of rowinfo (into *info_out too when given), the classification, one upload into AnalysisState::rows
int build_row_plan(dcr_graph *g, RowPlan *plan, std::vector<int2> *info_out);
int graph_components(dcr_graph *g, std::vector<int32_t> &labels);  // labels (smallest node id of the component) into spc_label and onto the host
void inv_sqrt_degree(dcr_graph *g, double *s);  // launches s = 1 / sqrt(deg), 0 at degree 0, on the graph's stream

// dcr_sweep.hip: the sweep's order for another call.  *score: the [n] device buffer the caller's kernel fills; sweep_order then
// sorts it as the sweep cut does (ascending by (score, node id), -0.0 == +0.0) and leaves *order (the node at each position) and
// *rank (its inverse) on the device.  One host synchronisation; a NaN in the score is DCR_ESTATE.
int sweep_score_buffer(dcr_graph *g, double **score);
int sweep_order(dcr_graph *g, const int32_t **order, const int32_t **rank);

// dcr_spectral.hip
struct SpectralKept {  // what spectral_solve leaves in device memory: the unit Ritz vector y, the scale s = 1 / sqrt(deg)
    const double *y, *s;
};
// *plan: the row plan the solver built, for the caller's own kernels on the same graph
int spectral_solve(dcr_graph *g, const dcr_spectral_opts *opts, dcr_spectral_result *out, SpectralKept *kept, RowPlan *plan);
void spectral_release_basis(dcr_graph *g);  // synchronises the stream and frees the Lanczos basis (y with it)

}  // namespace dcr
