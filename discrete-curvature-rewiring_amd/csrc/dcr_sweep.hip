// Sweep cut on the device-resident graph: the constructive half of Cheeger's inequality.
//
// Given a score per node, the nodes are ordered ascending by (score, node id) and every prefix S_k of that order, k = 1 .. n - 1, is
// valued by one of the two ratios of k_cheeger_values (cheeger_ratio, dcr_analysis.h); the smallest value and the smallest k that has it are
// returned.  With the score x = D^-1/2 y, y the eigenvector dcr_spectral.hip accepts for lambda_1, the best prefix is a set with
// lambda_1 / 2 <= h <= conductance(S_k) <= sqrt(2 lambda_1): a certificate for the bracket of experiment/cheeger_bounds.py.  The
// reference has no counterpart.  Everything up to the one division per prefix is integer arithmetic, so the result does not depend
// on any order of execution and matches a numpy restatement (tests/sweep_ref.py) bit for bit.
//
// Kernels:
//   k_sweep_score     x = s ⊙ y for the Fiedler path (s = 1 / sqrt(deg), 0 at degree 0: the solver's own)
//   k_sweep_keys      fp64 -> order-preserving uint64 (-0.0 canonicalised to +0.0; negative: all bits flipped, else the sign bit),
//                     payload = node id; the [8][256] digit histogram of all keys (order-independent), from which the host drops
//                     every pass whose digit is the same in all keys; a NaN raises a flag
//   k_sweep_hist      a sort pass, step 1: a wave owns a contiguous tile of keys and counts its digits: table[digit][tile]
//   k_scan_reduce / k_scan_apply   prefix sums of an int32 array in blocks of 2,048: block sums, closed into block offsets by the
//                     last workgroup (last_arriver), then the blocks themselves; exclusive for the sort table, inclusive (three
//                     arrays in one launch) for the difference arrays
//   k_sweep_scatter   step 3: the wave walks its tile 64 keys at a time; lanes with the same digit are ranked by a match mask (8
//                     ballots) and a popcount of the lower lanes on top of the wave's running per-digit offset: a STABLE scatter, so
//                     ties keep the input's id order through every pass
//   k_sweep_rank      rank[order[p]] = p
//   k_sweep_edges     every live slot with col > row, rows through walk_rows in the three degree classes; with p = rank[row],
//                     q = rank[col]: p < q: the edge is `lo` for k in [p + 1, q], q < p: `hi` for k in [q + 1, p], `in` from
//                     k = max(p, q) + 1, as +-1 into three int32 difference arrays indexed by k - 1 (integer atomics); what lands on
//                     the row's own rank is summed over the row first and added once
//   k_sweep_value     the ratio of every prefix, the profile, and the (value, k) lexicographic minimum: per-workgroup partials closed
//                     by the last workgroup
// Counts are int32: the limit is fewer than 2^31 live adjacency slots, which dcr_graph_create keeps.
#include <algorithm>
#include <cmath>

#include "dcr_analysis.h"

namespace dcr {

constexpr int SW_SCAN_BLOCK = 2048;  // elements a workgroup of the scans takes (8 per thread)
constexpr int SW_VALUE_BLOCKS = 1024;  // most workgroups of k_sweep_value (one arg-min partial each)
constexpr int64_t SW_TILE = 1024;    // keys per wave of a sort pass, up to 4,096 tiles; more keys per tile beyond that
// words of swp_ctl
constexpr int SW_CTL_TICKETS = 0;    // three scan tickets, the arg-min ticket
constexpr int SW_CTL_NAN = 4;
constexpr int SW_CTL_HIST = 8;       // [8][256]
constexpr int SW_CTL_RESULT = SW_CTL_HIST + 8 * 256;  // SweepDev
constexpr int SW_CTL_PARTS = SW_CTL_RESULT + 8;       // Ext[SW_VALUE_BLOCKS]
constexpr int SW_CTL_WORDS = SW_CTL_PARTS + 4 * SW_VALUE_BLOCKS;

struct SweepDev {
    double value;
    int32_t k, in, lo, hi;
    int32_t pad[2];
};
static_assert(sizeof(SweepDev) == 32, "result block is 8 words");

__device__ inline int32_t wave_incl_scan(int32_t x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    return x;
}

// 256 threads: the exclusive prefix of x over the workgroup, and the workgroup's total.  sh is free again on return.
__device__ inline int32_t block_excl_scan(int32_t x, int32_t *sh, int32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t incl = wave_incl_scan(x, lane);
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    const int32_t w0 = sh[0], w1 = sh[1], w2 = sh[2], w3 = sh[3];
    __syncthreads();
    const int32_t base = wave == 0 ? 0 : wave == 1 ? w0 : wave == 2 ? w0 + w1 : w0 + w1 + w2;
    *total = w0 + w1 + w2 + w3;
    return base + incl - x;
}

// ---- score and keys ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sweep_score(const double *__restrict__ s, const double *__restrict__ y, double *__restrict__ x, int64_t n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) x[v] = s[v] * y[v];
}

__global__ void __launch_bounds__(256) k_sweep_keys(const double *__restrict__ score, int64_t n, uint64_t *__restrict__ keys, int32_t *__restrict__ ids,
                                                     unsigned *hist, unsigned *nan_flag) {
    __shared__ unsigned sh[8 * 256];
    for (int i = threadIdx.x; i < 8 * 256; i += 256) sh[i] = 0;
    __syncthreads();
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const double x = score[v];
        if (x != x) atomicOr(nan_flag, 1u);
        uint64_t b = x == 0.0 ? 0ull : (uint64_t)__double_as_longlong(x);
        b = (b >> 63) ? ~b : b | 0x8000000000000000ull;
        keys[v] = b;
        ids[v] = (int32_t)v;
#pragma unroll
        for (int d = 0; d < 8; ++d) atomicAdd(&sh[d * 256 + (int)((b >> (8 * d)) & 255)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 8 * 256; i += 256)
        if (sh[i]) atomicAdd(hist + i, sh[i]);
}

// ---- a sort pass -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sweep_hist(const uint64_t *__restrict__ keys, int64_t n, int shift, int tile, int tiles,
                                                     int32_t *__restrict__ table) {
    __shared__ int32_t h[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * 4 + wave;
    for (int d = lane; d < 256; d += 64) h[wave][d] = 0;
    __syncthreads();
    if (gw < tiles) {
        const int64_t t0 = (int64_t)gw * tile;
        for (int i = lane; i < tile; i += 64) {
            const int64_t x = t0 + i;
            if (x < n) atomicAdd(&h[wave][(int)((keys[x] >> shift) & 255)], 1);
        }
    }
    __syncthreads();
    if (gw < tiles)
        for (int d = lane; d < 256; d += 64) table[(int64_t)d * tiles + gw] = h[wave][d];
}

// table: exclusive prefix sums over [digit][tile], so table[d][t] is where tile t's first key of digit d goes
__global__ void __launch_bounds__(256) k_sweep_scatter(const uint64_t *__restrict__ kin, const int32_t *__restrict__ vin, uint64_t *__restrict__ kout,
                                                        int32_t *__restrict__ vout, int64_t n, int shift, int tile, int tiles,
                                                        const int32_t *__restrict__ table) {
    __shared__ int32_t off[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * 4 + wave;
    const bool live = gw < tiles;
    for (int d = lane; d < 256; d += 64) off[wave][d] = live ? table[(int64_t)d * tiles + gw] : 0;
    __syncthreads();
    const int64_t t0 = (int64_t)gw * tile;
    const uint64_t lower = (1ull << lane) - 1ull;
    for (int i = 0; i < tile; i += 64) {  // the same trip count in every wave of the workgroup
        const int64_t x = t0 + i + lane;
        const bool ok = live && x < n;
        const uint64_t key = ok ? kin[x] : 0ull;
        const int32_t val = ok ? vin[x] : 0;
        const int d = (int)((key >> shift) & 255);
        uint64_t mask = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const uint64_t m = __ballot(ok && bit);
            mask &= bit ? m : ~m;
        }
        const int below = __popcll(mask & lower), count = __popcll(mask);
        const int32_t base = ok ? off[wave][d] : 0;
        __syncthreads();
        if (ok) {
            const int64_t pos = (int64_t)base + below;
            if (pos >= 0 && pos < n) {
                kout[pos] = key;
                vout[pos] = val;
            }
            if (below == count - 1) off[wave][d] = base + count;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_sweep_rank(const int32_t *__restrict__ order, int32_t *__restrict__ rank, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int32_t v = order[p];
    if (v >= 0 && v < n) rank[v] = (int32_t)p;
}

// ---- prefix sums -------------------------------------------------------------------------------------------------------------------
// grid (blocks, arrays); array y is data + y * stride.  part / boff: [arrays][blocks].
__global__ void __launch_bounds__(256) k_scan_reduce(const int32_t *__restrict__ data, int64_t len, int64_t stride, int nb, int32_t *part,
                                                      int32_t *__restrict__ boff, unsigned *ticket) {
    __shared__ int32_t sh[4];
    const int t = threadIdx.x, y = blockIdx.y;
    const int32_t *a = data + (int64_t)y * stride;
    const int64_t i0 = (int64_t)blockIdx.x * SW_SCAN_BLOCK + t * 8;
    int32_t acc = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) acc += i0 + q < len ? a[i0 + q] : 0;
    acc = wave_sum(acc);
    if ((t & 63) == 0) sh[t >> 6] = acc;
    __syncthreads();
    if (t == 0) __hip_atomic_store(part + (int64_t)y * nb + blockIdx.x, sh[0] + sh[1] + sh[2] + sh[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (!last_arriver(ticket + y, (unsigned)nb)) return;
    int32_t carry = 0;
    for (int c = 0; c < nb; c += 256) {
        const bool ok = c + t < nb;
        const int32_t v = ok ? __hip_atomic_load(part + (int64_t)y * nb + c + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        int32_t total;
        const int32_t ex = block_excl_scan(v, sh, &total);
        if (ok) boff[(int64_t)y * nb + c + t] = carry + ex;
        carry += total;
    }
    if (t == 0) __hip_atomic_store(ticket + y, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool INCLUSIVE>
__global__ void __launch_bounds__(256) k_scan_apply(int32_t *data, int64_t len, int64_t stride, int nb, const int32_t *__restrict__ boff) {
    __shared__ int32_t sh[4];
    const int t = threadIdx.x, y = blockIdx.y;
    int32_t *a = data + (int64_t)y * stride;
    const int64_t i0 = (int64_t)blockIdx.x * SW_SCAN_BLOCK + t * 8;
    int32_t v[8], acc = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        v[q] = i0 + q < len ? a[i0 + q] : 0;
        acc += v[q];
    }
    int32_t total;
    int32_t run = boff[(int64_t)y * nb + blockIdx.x] + block_excl_scan(acc, sh, &total);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int32_t before = run;
        run += v[q];
        if (i0 + q < len) a[i0 + q] = INCLUSIVE ? run : before;
    }
}

// ---- edges -------------------------------------------------------------------------------------------------------------------------
// one slot of row u (rank p): the far end's updates go out at once; the row's own are counted by the caller.  Returns 1 where the
// far end comes later in the order, 2 where it comes earlier, 0 for a slot that does not hold the edge.
__device__ inline int sweep_slot(int32_t u, int32_t p, int32_t v, const int32_t *__restrict__ rank, int32_t *d_in, int32_t *d_lo, int32_t *d_hi) {
    if (v <= u) return 0;
    const int32_t q = rank[v];
    if (p < q) {  // lo for k - 1 in [p, q - 1], in from k - 1 = q
        atomicAdd(d_lo + q, -1);
        atomicAdd(d_in + q, 1);
        return 1;
    }
    atomicAdd(d_hi + q, 1);  // hi for k - 1 in [q, p - 1], in from k - 1 = p
    return 2;
}

__device__ inline void sweep_row_own(int32_t p, int up, int down, int32_t *d_in, int32_t *d_lo, int32_t *d_hi) {
    if (up) atomicAdd(d_lo + p, up);
    if (down) {
        atomicAdd(d_hi + p, -down);
        atomicAdd(d_in + p, down);
    }
}

using SweepRows = RowGeom<>;  // eight lanes a short row, 32 short rows a workgroup

__global__ void __launch_bounds__(256) k_sweep_edges(RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                      const int32_t *__restrict__ rank, int32_t *d_in, int32_t *d_lo, int32_t *d_hi) {
    __shared__ int32_t sh[4];
    walk_rows<SweepRows>(plan, rowinfo, sh, [=](auto scope, int32_t u, int2 ri) {
        const int32_t p = rank[u];
        int32_t up = 0, down = 0;
        for (int j = scope.first(); j < ri.y; j += scope.stride) {
            const int r = sweep_slot(u, p, col[ri.x + j], rank, d_in, d_lo, d_hi);
            up += r == 1;
            down += r == 2;
        }
        up = scope.sum(up);
        down = scope.sum(down);
        if (scope.owner()) sweep_row_own(p, up, down, d_in, d_lo, d_hi);
    });
}

// ---- values and the arg-min --------------------------------------------------------------------------------------------------------
// c_*: inclusive prefix sums, element k - 1 = the count of S_k; n1 = n - 1 prefixes.
__global__ void __launch_bounds__(256) k_sweep_value(const int32_t *__restrict__ c_in, const int32_t *__restrict__ c_lo, const int32_t *__restrict__ c_hi,
                                                      int64_t n1, int64_t n_edges, int definition, double *__restrict__ profile, Ext *part,
                                                      unsigned *ticket, SweepDev *result) {
    __shared__ double shv[4];
    __shared__ int shs[4];
    double bv = 0.0;
    int bs = -1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n1; i += (int64_t)gridDim.x * 256) {
        const double val = cheeger_ratio(c_in[i], c_lo[i], c_hi[i], n_edges, definition);
        profile[i] = val;
        ext_take(bv, bs, val, (int)i, 0);
    }
    ext_block_reduce(bv, bs, 0, shv, shs);
    if (threadIdx.x == 0) {
        __hip_atomic_store(&part[blockIdx.x].val, bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&part[blockIdx.x].slot, bs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last_arriver(ticket, (unsigned)gridDim.x)) return;
    bv = 0.0;
    bs = -1;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) {
        const double v = __hip_atomic_load(&part[i].val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int s = __hip_atomic_load(&part[i].slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ext_take(bv, bs, v, s, 0);
    }
    ext_block_reduce(bv, bs, 0, shv, shs);
    if (threadIdx.x == 0) {
        result->value = bv;
        result->k = bs + 1;
        result->in = bs >= 0 ? c_in[bs] : 0;
        result->lo = bs >= 0 ? c_lo[bs] : 0;
        result->hi = bs >= 0 ? c_hi[bs] : 0;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
struct SweepPlan {
    int64_t n;
    int tile, tiles, nb_table, nb_diff;
    uint64_t *keys[2];
    int32_t *ids[2], *rank, *diff, *table, *part, *boff;
    double *score, *profile;
    unsigned *ctl;
};

static int sweep_buffers(dcr_graph *g, SweepPlan *P) {
    const int64_t n = g->n;
    P->n = n;
    int64_t tile = SW_TILE;
    if (n > 4096 * SW_TILE) tile = ((n + 4095) / 4096 + 63) / 64 * 64;
    P->tile = (int)tile;
    P->tiles = (int)((n + tile - 1) / tile);
    const int64_t table_len = (int64_t)256 * P->tiles;
    P->nb_table = (int)blocks_of(table_len, SW_SCAN_BLOCK);
    P->nb_diff = (int)blocks_of(n, SW_SCAN_BLOCK);
    const int64_t nb_most = std::max<int64_t>(P->nb_table, 3 * (int64_t)P->nb_diff);
    AnalysisState &A = analysis_of(g);
    DCR_TRY(A.swp_keys.grow(2 * n));
    DCR_TRY(A.swp_idx.grow(6 * n));
    DCR_TRY(A.swp_table.grow(table_len + 2 * nb_most));
    DCR_TRY(A.swp_f64.grow(2 * n));
    DCR_TRY(A.swp_ctl.grow(SW_CTL_WORDS));
    P->keys[0] = A.swp_keys.p;
    P->keys[1] = A.swp_keys.p + n;
    P->ids[0] = A.swp_idx.p;
    P->ids[1] = A.swp_idx.p + n;
    P->rank = A.swp_idx.p + 2 * n;
    P->diff = A.swp_idx.p + 3 * n;
    P->table = A.swp_table.p;
    P->part = A.swp_table.p + table_len;
    P->boff = P->part + nb_most;
    P->score = A.swp_f64.p;
    P->profile = A.swp_f64.p + n;
    P->ctl = A.swp_ctl.p;
    return DCR_OK;
}

// keys, the sort passes and the rank of what is in P.score; *order_out: the node at each position
static int sweep_sort(dcr_graph *g, const SweepPlan &P, const int32_t **order_out) {
    const int64_t n = P.n;
    hipStream_t st = g->stream;
    DCR_HIP(hipMemsetAsync(P.ctl, 0, sizeof(unsigned) * SW_CTL_WORDS, st));
    hipLaunchKernelGGL(k_sweep_keys, dim3(std::min(blocks_of(n), 1024u)), dim3(256), 0, st, P.score, n, P.keys[0], P.ids[0],
                       P.ctl + SW_CTL_HIST, P.ctl + SW_CTL_NAN);
    DCR_HIP(hipGetLastError());
    std::vector<unsigned> head((size_t)SW_CTL_RESULT);
    DCR_HIP(hipMemcpyAsync(head.data(), P.ctl, sizeof(unsigned) * head.size(), hipMemcpyDeviceToHost, st));
    DCR_HIP(hipStreamSynchronize(st));
    if (head[SW_CTL_NAN]) DCR_FAIL(DCR_ESTATE, "sweep cut: the score holds a NaN");
    int cur = 0;
    for (int pass = 0; pass < 8; ++pass) {
        bool one_digit = false;
        for (int d = 0; d < 256; ++d) one_digit = one_digit || head[(size_t)(SW_CTL_HIST + pass * 256 + d)] == (unsigned)n;
        if (one_digit) continue;  // the pass would move nothing
        hipLaunchKernelGGL(k_sweep_hist, dim3(blocks_of(P.tiles, 4)), dim3(256), 0, st, P.keys[cur], n, 8 * pass, P.tile, P.tiles, P.table);
        hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)P.nb_table, 1), dim3(256), 0, st, P.table, (int64_t)256 * P.tiles, (int64_t)0,
                           P.nb_table, P.part, P.boff, P.ctl + SW_CTL_TICKETS);
        hipLaunchKernelGGL(k_scan_apply<false>, dim3((unsigned)P.nb_table, 1), dim3(256), 0, st, P.table, (int64_t)256 * P.tiles, (int64_t)0,
                           P.nb_table, P.boff);
        hipLaunchKernelGGL(k_sweep_scatter, dim3(blocks_of(P.tiles, 4)), dim3(256), 0, st, P.keys[cur], P.ids[cur], P.keys[cur ^ 1],
                           P.ids[cur ^ 1], n, 8 * pass, P.tile, P.tiles, P.table);
        cur ^= 1;
    }
    hipLaunchKernelGGL(k_sweep_rank, dim3(blocks_of(n)), dim3(256), 0, st, P.ids[cur], P.rank, n);
    DCR_HIP(hipGetLastError());
    *order_out = P.ids[cur];
    return DCR_OK;
}

// the score is in P.score; rows: the graph's row plan
static int sweep_run(dcr_graph *g, const SweepPlan &P, int definition, const RowPlan &rows, dcr_sweep_result *out, int32_t *out_order,
                     double *out_profile) {
    const int64_t n = P.n;
    hipStream_t st = g->stream;
    const int32_t *order;
    DCR_TRY(sweep_sort(g, P, &order));
    int32_t *d_in = P.diff, *d_lo = P.diff + n, *d_hi = P.diff + 2 * n;
    DCR_HIP(hipMemsetAsync(P.diff, 0, sizeof(int32_t) * 3 * (size_t)n, st));
    if (g->n_edges > 0)
        hipLaunchKernelGGL(k_sweep_edges, dim3(row_grid<SweepRows>(rows)), dim3(256), 0, st, rows, g->rowinfo.p, g->col.p, P.rank, d_in, d_lo, d_hi);
    hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)P.nb_diff, 3), dim3(256), 0, st, P.diff, n, n, P.nb_diff, P.part, P.boff,
                       P.ctl + SW_CTL_TICKETS);
    hipLaunchKernelGGL(k_scan_apply<true>, dim3((unsigned)P.nb_diff, 3), dim3(256), 0, st, P.diff, n, n, P.nb_diff, P.boff);
    SweepDev *res_dev = (SweepDev *)(P.ctl + SW_CTL_RESULT);
    hipLaunchKernelGGL(k_sweep_value, dim3(std::min(blocks_of(n - 1), (unsigned)SW_VALUE_BLOCKS)), dim3(256), 0, st, d_in, d_lo, d_hi, n - 1,
                       g->n_edges, definition, P.profile, (Ext *)(P.ctl + SW_CTL_PARTS), P.ctl + SW_CTL_TICKETS + 3, res_dev);
    DCR_HIP(hipGetLastError());
    SweepDev res;
    DCR_HIP(hipMemcpyAsync(&res, res_dev, sizeof(res), hipMemcpyDeviceToHost, st));
    if (out_order) DCR_HIP(hipMemcpyAsync(out_order, order, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (out_profile) DCR_HIP(hipMemcpyAsync(out_profile, P.profile, sizeof(double) * (size_t)(n - 1), hipMemcpyDeviceToHost, st));
    DCR_HIP(hipStreamSynchronize(st));
    out->value = res.value;
    out->size = res.k;
    out->in = res.in;
    out->lo = res.lo;
    out->hi = res.hi;
    return DCR_OK;
}

// the order alone, for the other analysis calls (dcr_analysis.h): the caller's kernel writes the score, then asks for the sort
int sweep_score_buffer(dcr_graph *g, double **score) {
    SweepPlan P;
    DCR_TRY(sweep_buffers(g, &P));
    *score = P.score;
    return DCR_OK;
}

int sweep_order(dcr_graph *g, const int32_t **order, const int32_t **rank) {
    SweepPlan P;
    DCR_TRY(sweep_buffers(g, &P));
    *rank = P.rank;
    return sweep_sort(g, P, order);
}

static int sweep_args(const dcr_graph *g, int definition, const void *out) {
    if (!g || !out) DCR_FAIL(DCR_EINVAL, "null argument");
    if (definition != 0 && definition != 1) DCR_FAIL(DCR_EINVAL, "unknown definition");
    if (g->n < 2) DCR_FAIL(DCR_EINVAL, "a sweep needs at least two nodes");
    return DCR_OK;
}

}  // namespace dcr

using namespace dcr;

extern "C" {

int dcr_sweep_cut(dcr_graph *g, const double *score, int definition, dcr_sweep_result *out, int32_t *out_order, double *out_profile) {
    DCR_TRY(sweep_args(g, definition, out));
    if (!score) DCR_FAIL(DCR_EINVAL, "null argument");
    const int64_t n = g->n;
    for (int64_t v = 0; v < n; ++v)
        if (std::isnan(score[v])) DCR_FAIL(DCR_EINVAL, "the score holds a NaN");
    DCR_HIP(hipSetDevice(g->device));
    SweepPlan P;
    DCR_TRY(sweep_buffers(g, &P));
    RowPlan rows;
    DCR_TRY(build_row_plan(g, &rows, nullptr));
    DCR_HIP(hipMemcpyAsync(P.score, score, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, g->stream));
    return sweep_run(g, P, definition, rows, out, out_order, out_profile);
}

int dcr_fiedler_sweep(dcr_graph *g, const dcr_spectral_opts *opts, int definition, dcr_spectral_result *out_gap, dcr_sweep_result *out,
                      int32_t *out_order, double *out_score) {
    DCR_TRY(sweep_args(g, definition, out));
    if (!out_gap) DCR_FAIL(DCR_EINVAL, "null argument");
    SpectralKept kept;
    RowPlan rows;  // the solver's
    int rc = spectral_solve(g, opts, out_gap, &kept, &rows);
    if (rc == DCR_OK) {
        SweepPlan P;
        rc = sweep_buffers(g, &P);
        if (rc == DCR_OK) {
            hipLaunchKernelGGL(k_sweep_score, dim3(blocks_of(g->n)), dim3(256), 0, g->stream, kept.s, kept.y, P.score, g->n);
            rc = sweep_run(g, P, definition, rows, out, out_order, nullptr);
        }
        if (rc == DCR_OK && out_score) {
            hipError_t e = hipMemcpyAsync(out_score, P.score, sizeof(double) * (size_t)g->n, hipMemcpyDeviceToHost, g->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
            if (e != hipSuccess) {
                set_error(std::string("fiedler sweep: the score did not come back: ") + hipGetErrorString(e));
                rc = DCR_EHIP;
            }
        }
    }
    spectral_release_basis(g);
    return rc;
}

}  // extern "C"
