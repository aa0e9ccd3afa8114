// FoSR, first-order spectral rewiring (Karhadkar, Banerjee, Montufar, ICLR 2023) on the device-resident graph: add the edge that
// raises the spectral gap most, to first order.  include/dcr.h has the definitions (power step, pick, loop); the reference has no
// counterpart, tests/fosr_ref.py restates them in numpy.
//
// The published code takes the arg-min of the dense n x n outer product y y^T.  Here the choice is exact in O(n log n + E): with
// the nodes sorted by (y, id), the best partner of a node u of degree d is the first node of the order (the last, for y_u < 0)
// that is neither u nor a neighbour of u, and that node has rank below d + 2.  So a row needs a bitmap of d + 2 bits and a
// find-first-zero, and the arg-min over the rows closes the pick.  No n x n array exists.
//
// Kernels (all fp64, no floating-point atomics, every reduction per-workgroup partials closed in index order by the last
// workgroup behind the agent-scope ticket of dcr_internal.h):
//   k_fosr_start     x0 from Philox, counter (node, 0)
//   k_fosr_dot       the projection coefficient (x . r) / vol, r = sqrt(deg)                  reads 16 n bytes
//   k_fosr_project   xp = x - coef r, zs = s ⊙ xp                                             reads 16 n, writes 16 n
//   k_fosr_matvec    z = xp + s ⊙ A zs over walk_rows, |z|                                    reads 4 (2 E) + 8 (2 E) gathered + 24 n
//   k_fosr_scale     x = z / |z|; raises `stopped` and leaves x alone where |z| is 0 or not finite
//   k_fosr_y         y = x / sqrt(deg + 1) into the sweep's score buffer
//   (the sweep's keys, radix passes and rank: dcr_sweep.hip, sweep_order)
//   k_fosr_pick      per row the first unset rank among the first d + 2 from its end of the order, the product, the arg-min
#include <cmath>

#include "dcr_analysis.h"
#include "dcr_philox.h"
#include "dcr_row_patch.h"

namespace dcr {

constexpr int FSR_WINDOW = 4096;  // ranks a workgroup's LDS bitmap covers at a time (long rows)
constexpr int FSR_WAVE_WORDS = (SP_LONG_DEG + 2 + 31) / 32;  // 32-bit words of a medium row's bitmap: d + 2 <= 2,050 bits
constexpr int FSR_BM_WORDS = 4 * FSR_WAVE_WORDS > FSR_WINDOW / 32 ? 4 * FSR_WAVE_WORDS : FSR_WINDOW / 32;
constexpr int FSR_DOT_BLOCKS = 1024;  // most workgroups of k_fosr_dot

struct FsrCtl {
    unsigned ticket[4];  // dot, mat-vec, pick
    double coef;         // (x . r) / vol of the running step
    double norm;         // |z| of the last mat-vec
    double product;      // the pick: y_u y_v, u, v; found = 0 where no row has a candidate
    int32_t u, v, found;
    int32_t stopped;     // a step met |z| = 0 or not finite: x is the iterate before that step
};

struct FsrPart {  // a workgroup's best row; u < 0: none
    double product;
    unsigned long long uv;  // u | v << 32
};

// ---- the power step ----------------------------------------------------------------------------------------------------------------
// uniform in (-1, 1): ((53 bits of r[0], r[1]) + 1/2) 2^-52 - 1, the spectral solver's construction (on every node)
__global__ void __launch_bounds__(256) k_fosr_start(double *__restrict__ x, int64_t n, uint64_t seed) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    uint32_t r[4];
    philox4x32_10((uint64_t)v, (uint64_t)0, seed, r);
    const uint64_t bits = ((uint64_t)r[0] | ((uint64_t)r[1] << 32)) >> 11;
    x[v] = ((double)bits + 0.5) * 0x1p-52 - 1.0;
}

__global__ void __launch_bounds__(256) k_fosr_dot(const int2 *__restrict__ rowinfo, const double *__restrict__ x, int64_t n, double vol,
                                                   double *part, FsrCtl *ctl) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) acc += x[v] * sqrt((double)rowinfo[v].y);
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) st_agent(part + blockIdx.x, acc);
    if (!last_arriver(&ctl->ticket[0], (unsigned)gridDim.x)) return;
    const double dot = close_partials(part, gridDim.x, sh);
    if (threadIdx.x == 0) {
        ctl->coef = dot / vol;
        __hip_atomic_store(&ctl->ticket[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(256) k_fosr_project(const int2 *__restrict__ rowinfo, const double *__restrict__ x, const FsrCtl *__restrict__ ctl,
                                                       double *__restrict__ xp, double *__restrict__ zs, int64_t n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int d = rowinfo[v].y;
    const double p = x[v] - ctl->coef * sqrt((double)d);
    xp[v] = p;
    zs[v] = inv_sqrt_deg(d) * p;
}

using FsrRows = RowGeom<>;  // eight lanes a short row, 32 short rows a workgroup

__global__ void __launch_bounds__(256) k_fosr_matvec(RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                      const double *__restrict__ xp, const double *__restrict__ zs, double *__restrict__ z,
                                                      double *part, FsrCtl *ctl) {
    __shared__ double sh[4];
    double sq = 0.0;  // z_u^2 of the row this thread finishes
    walk_rows<FsrRows>(plan, rowinfo, sh, [=](auto scope, int32_t u, int2 ri, double &zz) {
        double acc = 0.0;
        for (int j = scope.first(); j < ri.y; j += scope.stride) acc += zs[col[ri.x + j]];
        acc = scope.sum(acc);
        if (scope.owner()) {
            const double zu = xp[u] + inv_sqrt_deg(ri.y) * acc;
            z[u] = zu;
            zz = zu * zu;
        }
    }, sq);
    sq = block_sum(sq, sh);
    if (threadIdx.x == 0) st_agent(part + blockIdx.x, sq);
    if (!last_arriver(&ctl->ticket[1], (unsigned)gridDim.x)) return;
    const double tot = close_partials(part, gridDim.x, sh);
    if (threadIdx.x == 0) {
        ctl->norm = sqrt(tot);
        __hip_atomic_store(&ctl->ticket[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(256) k_fosr_scale(const double *__restrict__ z, FsrCtl *ctl, double *__restrict__ x, int64_t n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const double nrm = ctl->norm;
    if (!(nrm > 0.0 && nrm < __builtin_inf())) {
        if (v == 0) ctl->stopped = 1;
        return;
    }
    if (v < n) x[v] = z[v] / nrm;
}

__global__ void __launch_bounds__(256) k_fosr_y(const int2 *__restrict__ rowinfo, const double *__restrict__ x, double *__restrict__ y, int64_t n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) y[v] = x[v] / sqrt((double)(rowinfo[v].y + 1));
}

// ---- the pick ----------------------------------------------------------------------------------------------------------------------
// (bp, bu, bv) <- the better of it and (p, u, v): the smaller product, among equal ones (-0.0 == 0.0) the smaller u; u < 0: none
__device__ inline void pick_take(double &bp, int32_t &bu, int32_t &bv, double p, int32_t u, int32_t v) {
    const bool better = bu < 0 || p < bp || (p == bp && u < bu);
    if (u >= 0 && better) {
        bp = p;
        bu = u;
        bv = v;
    }
}

// over the workgroup; shp / shu / shv: one entry per wave.  The result in every thread.
__device__ inline void pick_block_reduce(double &bp, int32_t &bu, int32_t &bv, double *shp, int32_t *shu, int32_t *shv) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) pick_take(bp, bu, bv, __shfl_xor(bp, off), __shfl_xor(bu, off), __shfl_xor(bv, off));
    if (lane == 0) {
        shp[wave] = bp;
        shu[wave] = bu;
        shv[wave] = bv;
    }
    __syncthreads();
    bu = -1;
    for (int w = 0; w < 4; ++w) pick_take(bp, bu, bv, shp[w], shu[w], shv[w]);
    __syncthreads();
}

// lanes of one wave meet around their LDS words: the wave's LDS instructions run in order, the fences keep the compiler's order
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(256) k_fosr_pick(RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                    const double *__restrict__ y, const int32_t *__restrict__ rank,
                                                    const int32_t *__restrict__ order, int32_t n, FsrPart *part, FsrCtl *ctl) {
    __shared__ unsigned bm[FSR_BM_WORDS];  // a medium row's bitmap per wave, or the long row's window
    __shared__ int32_t sh[4], shu[4], shv[4];
    __shared__ double shp[4];
    double bp = 0.0;
    int32_t bu = -1, bv = -1;
    walk_rows<FsrRows>(plan, rowinfo, sh, [=](auto scope, int32_t u, int2 ri, double &tp, int32_t &tu, int32_t &tv) {
        constexpr int L = decltype(scope)::stride;
        const int d = ri.y;
        if (d >= n - 1) return;  // adjacent to every other node: no candidate (the same in every lane of the scope)
        const double yu = y[u];
        const bool top = yu < 0.0;           // which end of the order the partner comes from
        const int32_t lim = d + 2;           // u and its neighbours cannot fill the first d + 2 ranks; lim <= n
        const int32_t own = top ? n - 1 - rank[u] : rank[u];
        int32_t f = -1;                      // the first free rank, counted from that end
        if constexpr (L < 64) {              // lim <= 34: one register mask, OR-ed across the lane group
            unsigned long long m = 0ull;
            for (int j = scope.first(); j < d; j += L) {
                const int32_t r = rank[col[ri.x + j]], q = top ? n - 1 - r : r;
                if (q < lim) m |= 1ull << q;
            }
#pragma unroll
            for (int off = L / 2; off > 0; off >>= 1) m |= __shfl_xor(m, off);
            if (own < lim) m |= 1ull << own;
            f = __ffsll(~m) - 1;
        } else if constexpr (L == 64) {      // lim <= 2,050: the wave's LDS bitmap
            const int lane = threadIdx.x & 63;
            unsigned *w = bm + (threadIdx.x >> 6) * FSR_WAVE_WORDS;
            const int words = (lim + 31) >> 5;
            for (int i = lane; i < words; i += 64) __hip_atomic_store(w + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            wave_lds_sync();
            for (int j = lane; j < d; j += 64) {
                const int32_t r = rank[col[ri.x + j]], q = top ? n - 1 - r : r;
                if (q < lim) atomicOr(w + (q >> 5), 1u << (q & 31));
            }
            if (lane == 0 && own < lim) atomicOr(w + (own >> 5), 1u << (own & 31));
            wave_lds_sync();
            int32_t best = INT32_MAX;        // (bits from lim up are unset: the first unset bit is below lim all the same)
            for (int i = lane; i < words; i += 64) {
                const unsigned free_bits = ~__hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                if (free_bits && best == INT32_MAX) best = i * 32 + __ffs(free_bits) - 1;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off));
            f = best;
        } else {                             // a window of FSR_WINDOW ranks at a time until one has a free rank
            const int t = threadIdx.x;
            for (int32_t base = 0; base < lim && f < 0; base += FSR_WINDOW) {
                const int32_t end = min(lim - base, FSR_WINDOW);
                const int words = (end + 31) >> 5;
                for (int i = t; i < words; i += 256) bm[i] = 0u;
                __syncthreads();
                for (int j = t; j < d; j += 256) {
                    const int32_t r = rank[col[ri.x + j]], q = (top ? n - 1 - r : r) - base;
                    if (q >= 0 && q < end) atomicOr(bm + (q >> 5), 1u << (q & 31));
                }
                if (t == 0 && own >= base && own - base < end) atomicOr(bm + ((own - base) >> 5), 1u << ((own - base) & 31));
                __syncthreads();
                int32_t best = INT32_MAX;
                for (int i = t; i < words; i += 256) {
                    unsigned free_bits = ~bm[i];
                    if (i == words - 1 && (end & 31)) free_bits &= (1u << (end & 31)) - 1u;  // a full window ends inside this word
                    if (free_bits && best == INT32_MAX) best = i * 32 + __ffs(free_bits) - 1;
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off));
                if ((t & 63) == 0) scope.sh[t >> 6] = best;
                __syncthreads();
                best = min(min(scope.sh[0], scope.sh[1]), min(scope.sh[2], scope.sh[3]));
                __syncthreads();
                if (best != INT32_MAX) f = base + best;
            }
        }
        if (scope.owner() && f >= 0 && f < lim) {
            const int32_t partner = order[top ? n - 1 - f : f];
            const double p = yu * y[partner];
            if (p == p) pick_take(tp, tu, tv, p, u, partner);  // (0 x inf: not a candidate)
        }
    }, bp, bu, bv);
    pick_block_reduce(bp, bu, bv, shp, shu, shv);
    if (threadIdx.x == 0) {
        st_agent(&part[blockIdx.x].product, bp);
        __hip_atomic_store(&part[blockIdx.x].uv, (unsigned long long)(uint32_t)bu | ((unsigned long long)(uint32_t)bv << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!last_arriver(&ctl->ticket[2], (unsigned)gridDim.x)) return;
    bu = -1;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += 256) {
        const double p = ld_agent(&part[i].product);
        const unsigned long long uv = __hip_atomic_load(&part[i].uv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pick_take(bp, bu, bv, p, (int32_t)(uint32_t)uv, (int32_t)(uint32_t)(uv >> 32));
    }
    pick_block_reduce(bp, bu, bv, shp, shu, shv);
    if (threadIdx.x == 0) {
        ctl->product = bu >= 0 ? bp : 0.0;
        ctl->u = bu;
        ctl->v = bu >= 0 ? bv : -1;
        ctl->found = bu >= 0;
        __hip_atomic_store(&ctl->ticket[2], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
struct FsrRun {
    dcr_graph *g;
    int64_t n;
    double *x, *xp, *zs, *z, *y;  // [n] each; y is the sweep's score buffer
    double *part;
    FsrCtl *ctl;
    HostRowPlan host;             // degrees and rows by class, patched edge by edge (dcr_row_patch.h)
    RowPlan plan;

    int setup() {
        n = g->n;
        AnalysisState &A = analysis_of(g);
        DCR_TRY(A.fsr_vec.grow(4 * n));
        DCR_TRY(A.fsr_part.grow(2 * n + FSR_DOT_BLOCKS));  // a workgroup of a row kernel holds a row at least
        DCR_TRY(A.fsr_ctl.grow((int64_t)sizeof(FsrCtl)));
        DCR_TRY(sweep_score_buffer(g, &y));
        x = A.fsr_vec.p;
        xp = x + n;
        zs = x + 2 * n;
        z = x + 3 * n;
        part = A.fsr_part.p;
        ctl = (FsrCtl *)A.fsr_ctl.p;
        DCR_HIP(hipMemsetAsync(ctl, 0, sizeof(FsrCtl), g->stream));
        std::vector<int2> info;
        DCR_TRY(build_row_plan(g, &plan, &info));
        host.short_deg = SP_SHORT_DEG;
        host.long_deg = SP_LONG_DEG;
        host.deg.resize((size_t)n);
        for (int64_t v = 0; v < n; ++v) host.deg[(size_t)v] = info[(size_t)v].y;
        host.rebuild();
        return DCR_OK;
    }
    // the edge {u, v} has been added: the host plan follows; the device list only where a node changed its class.  (A row that
    // moved in a relayout needs nothing: the plan holds node ids, and every launch takes g->rowinfo as it is then.)
    int edge_added(int32_t u, int32_t v) {
        if (!host.add_edge(u, v)) return DCR_OK;
        DCR_HIP(hipMemcpyAsync(analysis_of(g).rows.p, host.rows.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));
        plan.n_long = (int)host.count[0];
        plan.n_mid = (int)host.count[1];
        plan.n_short = (int)host.count[2];
        return DCR_OK;
    }
    void power_step() const {
        hipStream_t st = g->stream;
        hipLaunchKernelGGL(k_fosr_dot, dim3(std::min(blocks_of(n), (unsigned)FSR_DOT_BLOCKS)), dim3(256), 0, st, g->rowinfo.p, x, n,
                           2.0 * (double)g->n_edges, part, ctl);
        hipLaunchKernelGGL(k_fosr_project, dim3(blocks_of(n)), dim3(256), 0, st, g->rowinfo.p, x, ctl, xp, zs, n);
        hipLaunchKernelGGL(k_fosr_matvec, dim3(row_grid<FsrRows>(plan)), dim3(256), 0, st, plan, g->rowinfo.p, g->col.p, xp, zs, z, part, ctl);
        hipLaunchKernelGGL(k_fosr_scale, dim3(blocks_of(n)), dim3(256), 0, st, z, ctl, x, n);
    }
    // y of what is in x, the order, the pick; *c: the control block as the pick left it (one small read)
    int pick(FsrCtl *c) const {
        hipStream_t st = g->stream;
        hipLaunchKernelGGL(k_fosr_y, dim3(blocks_of(n)), dim3(256), 0, st, g->rowinfo.p, x, y, n);
        const int32_t *order, *rank;
        DCR_TRY(sweep_order(g, &order, &rank));
        hipLaunchKernelGGL(k_fosr_pick, dim3(row_grid<FsrRows>(plan)), dim3(256), 0, st, plan, g->rowinfo.p, g->col.p, y, rank, order,
                           (int32_t)n, (FsrPart *)part, ctl);
        DCR_HIP(hipGetLastError());
        DCR_HIP(hipMemcpyAsync(c, ctl, sizeof(FsrCtl), hipMemcpyDeviceToHost, st));
        DCR_HIP(hipStreamSynchronize(st));
        return DCR_OK;
    }
};

static int fosr_vector_ok(const double *x, int64_t n) {
    for (int64_t v = 0; v < n; ++v)
        if (std::isnan(x[v])) DCR_FAIL(DCR_EINVAL, "the vector holds a NaN");
    return DCR_OK;
}

}  // namespace dcr

using namespace dcr;

extern "C" {

int dcr_fosr_pick(dcr_graph *g, const double *x, int32_t *out_u, int32_t *out_v, double *out_product, double *out_y, int *out_found) {
    if (!g || !x || !out_u || !out_v || !out_product || !out_found) DCR_FAIL(DCR_EINVAL, "null argument");
    if (g->n < 2) DCR_FAIL(DCR_EINVAL, "a pick needs at least two nodes");
    DCR_TRY(fosr_vector_ok(x, g->n));
    DCR_HIP(hipSetDevice(g->device));
    FsrRun R;
    R.g = g;
    DCR_TRY(R.setup());
    DCR_HIP(hipMemcpyAsync(R.x, x, sizeof(double) * (size_t)R.n, hipMemcpyHostToDevice, g->stream));
    FsrCtl c;
    DCR_TRY(R.pick(&c));
    if (out_y) {
        DCR_HIP(hipMemcpyAsync(out_y, R.y, sizeof(double) * (size_t)R.n, hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));
    }
    *out_found = c.found;
    *out_u = c.u;
    *out_v = c.v;
    *out_product = c.product;
    return DCR_OK;
}

int dcr_fosr(dcr_graph *g, const dcr_fosr_opts *opts, const double *x0, int32_t *out_u, int32_t *out_v, int64_t *out_added, double *out_x) {
    if (!g || !opts || !out_added) DCR_FAIL(DCR_EINVAL, "null argument");
    if (opts->num_iterations < 0 || opts->initial_power_iters < 0) DCR_FAIL(DCR_EINVAL, "num_iterations and initial_power_iters must be >= 0");
    if (opts->num_iterations > 0 && (!out_u || !out_v)) DCR_FAIL(DCR_EINVAL, "null argument");
    if (g->n < 2) DCR_FAIL(DCR_EINVAL, "FoSR needs at least two nodes");
    if (g->n_edges <= 0) DCR_FAIL(DCR_EINVAL, "FoSR needs a graph with an edge");
    if (x0) DCR_TRY(fosr_vector_ok(x0, g->n));
    *out_added = 0;
    DCR_HIP(hipSetDevice(g->device));
    FsrRun R;
    R.g = g;
    DCR_TRY(R.setup());
    const int64_t n = R.n;
    if (x0)
        DCR_HIP(hipMemcpyAsync(R.x, x0, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, g->stream));
    else
        hipLaunchKernelGGL(k_fosr_start, dim3(blocks_of(n)), dim3(256), 0, g->stream, R.x, n, opts->seed);
    for (int64_t i = 0; i < opts->initial_power_iters; ++i) R.power_step();
    DCR_HIP(hipGetLastError());
    for (int64_t it = 0; it < opts->num_iterations; ++it) {
        FsrCtl c;
        DCR_TRY(R.pick(&c));  // (brings the last step's `stopped` along)
        if (c.stopped || !c.found) break;
        const int64_t before = g->n_edges;
        DCR_TRY(dcr_graph_add_edge(g, c.u, c.v));
        if (g->n_edges != before + 1) DCR_FAIL(DCR_ESTATE, "FoSR: the picked pair was already an edge");
        DCR_TRY(R.edge_added(c.u, c.v));
        out_u[*out_added] = c.u;
        out_v[*out_added] = c.v;
        ++*out_added;
        R.power_step();
        DCR_HIP(hipGetLastError());
    }
    if (out_x) DCR_HIP(hipMemcpyAsync(out_x, R.x, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
    DCR_HIP(hipStreamSynchronize(g->stream));
    return DCR_OK;
}

}  // extern "C"
