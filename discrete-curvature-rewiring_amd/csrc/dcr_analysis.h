// What the graph-analysis translation units share (dcr_cheeger.hip, dcr_spectral.hip, dcr_sweep.hip, dcr_resistance.hip,
// dcr_diffusion.hip, dcr_fosr.hip, dcr_hops.hip, dcr_betweenness.hip) and the
// curvature pass, SDRF and the GCN do not need: the deterministic reductions, the row plan and the row walker, the Cheeger ratio,
// and the analysis buffers of a graph.  A new analysis feature adds its buffers and declarations here; dcr_internal.h and
// dcr_graph.hip stay as they are.
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
    int32_t *rows = nullptr;        // [n] rows by degree class (build_row_plan)
    int64_t rows_cap = 0;

    // Monte-Carlo Cheeger estimate (dcr_cheeger.hip): membership words [n][W], counts [3][64 W], ratios [64 W]
    uint64_t *chg_members = nullptr;
    int64_t chg_members_cap = 0;
    unsigned long long *chg_counts = nullptr;
    int64_t chg_counts_cap = 0;
    double *chg_values = nullptr;
    int64_t chg_values_cap = 0;

    // connected components (dcr_analysis.hip) and the spectral gap (dcr_spectral.hip)
    int32_t *spc_label = nullptr;   // [n] smallest node id of the node's component
    int64_t spc_label_cap = 0;
    unsigned *spc_ctl = nullptr;    // {a sweep of the components changed a label, reduction ticket, -, -}
    int64_t spc_ctl_cap = 0;
    double *spc_vec = nullptr;      // [4][n]: scale s, null-space weights k, z = s ⊙ v of the newest column, work vector w
    int64_t spc_vec_cap = 0;
    double *spc_basis = nullptr;    // [columns][n] Lanczos basis
    int64_t spc_basis_cap = 0;
    int32_t *spc_rows = nullptr;    // [n]: nodes by component
    int64_t spc_rows_cap = 0;
    int4 *spc_chunks = nullptr;     // deflation chunks
    int64_t spc_chunks_cap = 0;
    double *spc_part = nullptr;     // per-workgroup (per-wave) partial sums
    int64_t spc_part_cap = 0;
    double *spc_small = nullptr;    // alpha [m], beta [m], 8 scalars, Gram-Schmidt coefficients [m], Ritz coefficients [m]
    int64_t spc_small_cap = 0;

    // effective resistance (dcr_resistance.hip): O(n B), B the columns of a batch
    double *res_vec = nullptr;      // z, p, r, y, q as [n][B] each, then s [n]
    int64_t res_vec_cap = 0;
    double *res_part = nullptr;     // per-workgroup partial sums, B per workgroup (2 B in the closing mat-vec)
    int64_t res_part_cap = 0;
    unsigned char *res_ctl = nullptr;  // the batch's control block (ResCtl of dcr_resistance.hip)
    int64_t res_ctl_cap = 0;

    // sweep cut (dcr_sweep.hip): all O(n)
    uint64_t *swp_keys = nullptr;   // [2][n] sort keys, ping and pong
    int64_t swp_keys_cap = 0;
    int32_t *swp_idx = nullptr;     // [6][n]: node ids ping and pong, rank, the three difference arrays (in, lo, hi)
    int64_t swp_idx_cap = 0;
    int32_t *swp_table = nullptr;   // [256][tiles] digit counts of a sort pass, then the scans' per-block sums and offsets
    int64_t swp_table_cap = 0;
    double *swp_f64 = nullptr;      // [2][n]: the score, the profile
    int64_t swp_f64_cap = 0;
    unsigned *swp_ctl = nullptr;    // tickets, NaN flag, the [8][256] digit histogram of the keys, the result block, arg-min partials
    int64_t swp_ctl_cap = 0;

    // PageRank diffusion (dcr_diffusion.hip): O(n B) for the solve, O(entries kept by one batch) for the selection
    double *dif_vec = nullptr;      // z, p, r, x, q as [n][B] each, then the scale [n]
    int64_t dif_vec_cap = 0;
    double *dif_part = nullptr;     // per-workgroup partial sums, B per workgroup
    int64_t dif_part_cap = 0;
    unsigned char *dif_ctl = nullptr;  // the batch's control block (DifCtl of dcr_diffusion.hip)
    int64_t dif_ctl_cap = 0;
    int32_t *dif_row = nullptr;     // the node ids a batch keeps, column after column
    int64_t dif_row_cap = 0;
    double *dif_val = nullptr;      // their values, then their weights
    int64_t dif_val_cap = 0;

    // FoSR (dcr_fosr.hip): all O(n)
    double *fsr_vec = nullptr;      // [4][n]: the iterate x, its projection, s ⊙ projection, z
    int64_t fsr_vec_cap = 0;
    double *fsr_part = nullptr;     // per-workgroup partials: sums, or (product, {u, partner}) pairs of the pick
    int64_t fsr_part_cap = 0;
    unsigned char *fsr_ctl = nullptr;  // tickets and the result block (FsrCtl of dcr_fosr.hip)
    int64_t fsr_ctl_cap = 0;

    // hop distances (dcr_hops.hip): O(n W) words, W <= 4 the words of a batch of 64 W sources; O(64 W n) only where rows are asked for
    uint64_t *hop_bits = nullptr;   // visited, frontier, next as [n][W] each
    int64_t hop_bits_cap = 0;
    unsigned char *hop_ctl = nullptr;  // the batch's running totals [256] (64-bit), then its sources [256]
    int64_t hop_ctl_cap = 0;
    int32_t *hop_dist = nullptr;    // [64 W][n] distance rows of a batch
    int64_t hop_dist_cap = 0;

    // betweenness (dcr_betweenness.hip): O(16 n) for a batch of 16 sources; O(adjacency slots) only where edge values are asked for
    int32_t *btw_dist = nullptr;    // [n][16] the level of the node for each source of the batch, -1: not reached
    int64_t btw_dist_cap = 0;
    double *btw_f64 = nullptr;      // sigma, delta as [n][16] each, then the sum over the batches [n]
    int64_t btw_f64_cap = 0;
    double *btw_slot = nullptr;     // [cap_total] the sum over the batches per adjacency slot
    int64_t btw_slot_cap = 0;
    unsigned char *btw_ctl = nullptr;  // the batch's control block (BtwCtl of dcr_betweenness.hip)
    int64_t btw_ctl_cap = 0;

    void release();  // frees every buffer
};

// dcr_analysis.hip
AnalysisState &analysis_of(dcr_graph *g);  // the graph's state, created on first use
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
