// Hop distances on the device-resident graph: bit-parallel multi-source breadth-first search.  include/dcr.h has the rule; the
// reference has no counterpart, tests/hops_ref.py restates it in numpy.
//
// A batch holds 64 W sources (W = 1, 2 or 4 words).  Every node carries one bit per source in three node-major uint64 [n][W]
// arrays: visited (the source has reached the node), frontier (it reached it at the previous level) and next (at this one).  One
// sweep of the adjacency advances every source of the batch by one hop; nothing is n x n unless distance rows are asked for, and
// then it is the batch's [64 W][n] block.  Everything is integer: any schedule gives the same bits.
//
// Kernels:
//   k_hop_init<W>   the source bits into visited and frontier (64-bit atomic OR: two sources may be the same node), distance 0
//   k_hop_level<W>  pull, rows through walk_rows in the three degree classes: a row ORs the frontier words of its live neighbours
//                   across its scope, next = acc & ~visited, visited |= next.  A row writes its own words only: no atomics, no
//                   ordering between rows (frontier is read, visited and next are written, each by its own row).  A row whose
//                   visited words cover `live` (the batch's sources that still advance) returns before it reads a neighbour.
//                   reads 4 (2 E) + 8 W (2 E) gathered + 8 W n, writes up to 16 W n; the full rows cost 8 W read + 8 W written
//   k_hop_count<W>  per source the nodes of `next`, added to the running totals with 64-bit integer atomics; the distance rows
//                   where asked for.  A wave takes 64 nodes at a time, a node a lane; lane b keeps the count of bit b
//                   (ballot + popcount), only for the bits some lane has.  reads 8 W n
// The host runs the levels: per level one launch of each, one download of the 64 W totals, one synchronisation.  No kernel
// waits for another workgroup.
#include <algorithm>
#include <cstdlib>

#include "dcr_analysis.h"

namespace dcr {

constexpr int HOP_MAX_W = 4;           // words of the widest batch: 256 sources a sweep
constexpr int HOP_COUNT_BLOCKS = 1024; // most workgroups of k_hop_count

template <int W>
struct HopWords {  // one bit per source of a batch
    uint64_t w[W];
};

// ---- OR over a row's scope (RowScope::sum adds) --------------------------------------------------------------------------------
template <int LANES>
__device__ inline uint64_t group_or(uint64_t x) {  // over LANES consecutive lanes of a wave, the same bits in every lane
#pragma unroll
    for (int off = LANES / 2; off >= 1; off >>= 1) x |= (uint64_t)__shfl_xor((unsigned long long)x, off);
    return x;
}

// sh: 4 W words of LDS, used by the workgroup scope only and free again on return
template <int W, class Scope>
__device__ inline void scope_or(const Scope &scope, uint64_t (&acc)[W]) {
    constexpr int L = Scope::stride;
    if constexpr (L == 256) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            acc[w] = group_or<64>(acc[w]);
            if (lane == 0) scope.sh[wave * W + w] = acc[w];
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = (scope.sh[w] | scope.sh[W + w]) | (scope.sh[2 * W + w] | scope.sh[3 * W + w]);
        __syncthreads();
    } else {
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = group_or<L>(acc[w]);
    }
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------
// source i of the batch gets bit i & 63 of word i >> 6.  sources == nullptr: source i is node first + i.
template <int W>
__global__ void __launch_bounds__(256) k_hop_init(const int32_t *__restrict__ sources, int64_t first, int B, int64_t n, uint64_t *visited,
                                                   uint64_t *frontier, int32_t *dist) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= B) return;
    const int64_t s = sources ? (int64_t)sources[i] : first + i;
    const unsigned long long bit = 1ull << (i & 63);
    atomicOr((unsigned long long *)visited + s * W + (i >> 6), bit);
    atomicOr((unsigned long long *)frontier + s * W + (i >> 6), bit);
    if (dist) dist[(int64_t)i * n + s] = 0;
}

using HopRows = RowGeom<>;  // eight lanes a short row, 32 short rows a workgroup

template <int W>
__global__ void __launch_bounds__(256) k_hop_level(RowPlan plan, const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                    const uint64_t *__restrict__ frontier, uint64_t *visited, uint64_t *next,
                                                    HopWords<W> live) {
    __shared__ uint64_t sh[4 * W];
    walk_rows<HopRows>(plan, rowinfo, sh, [=](auto scope, int32_t v, int2 ri) {
        uint64_t vis[W], acc[W];
        bool full = true;  // the same in every lane of the scope
#pragma unroll
        for (int w = 0; w < W; ++w) {
            vis[w] = visited[(int64_t)v * W + w];
            acc[w] = 0;
            full = full && (vis[w] & live.w[w]) == live.w[w];
        }
        if (full) {  // no source that still advances can enter this row
            if (scope.owner()) {
#pragma unroll
                for (int w = 0; w < W; ++w) next[(int64_t)v * W + w] = 0;
            }
            return;
        }
        for (int j = scope.first(); j < ri.y; j += scope.stride) {
            const uint64_t *f = frontier + (int64_t)col[ri.x + j] * W;
#pragma unroll
            for (int w = 0; w < W; ++w) acc[w] |= f[w];
        }
        scope_or<W>(scope, acc);
        if (scope.owner()) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const uint64_t fresh = acc[w] & ~vis[w];
                next[(int64_t)v * W + w] = fresh;
                if (fresh) visited[(int64_t)v * W + w] = vis[w] | fresh;
            }
        }
    });
}

// totals[64 w + b] += the nodes whose bit b of word w of `bits` is set; dist (or nullptr): dist[64 w + b][v] = level for them
template <int W>
__global__ void __launch_bounds__(256) k_hop_count(const uint64_t *__restrict__ bits, int64_t n, int32_t level, int32_t *dist,
                                                    unsigned long long *totals) {
    __shared__ uint32_t sh[4][64 * W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t cnt[W];  // lane b: the nodes with bit b of word w, of this wave's chunks (a workgroup sees fewer than 2^32 nodes)
#pragma unroll
    for (int w = 0; w < W; ++w) cnt[w] = 0;
    const int64_t chunks = (n + 63) / 64;
    for (int64_t c = (int64_t)blockIdx.x * 4 + wave; c < chunks; c += (int64_t)gridDim.x * 4) {
        const int64_t v = c * 64 + lane;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint64_t word = v < n ? bits[v * W + w] : 0ull;
            const uint64_t any = group_or<64>(word);
            uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)any), hi = __builtin_amdgcn_readfirstlane((uint32_t)(any >> 32));
            for (uint64_t left = (uint64_t)lo | ((uint64_t)hi << 32); left; left &= left - 1) {  // the same in every lane
                const int b = __builtin_ctzll(left);
                const bool set = (word >> b) & 1ull;
                const uint32_t c1 = (uint32_t)__popcll(__ballot(set));
                if (lane == b) cnt[w] += c1;
                if (dist && set) dist[((int64_t)64 * w + b) * n + v] = level;
            }
        }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) sh[wave][64 * w + lane] = cnt[w];
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * W; i += 256) {
        const unsigned long long t = (unsigned long long)sh[0][i] + sh[1][i] + sh[2][i] + sh[3][i];
        if (t) atomicAdd(totals + i, t);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct HopRun {
    dcr_graph *g;
    int64_t n;
    RowPlan plan;
    uint64_t *visited, *frontier, *next;   // [n][W] each
    unsigned long long *totals;            // [64 HOP_MAX_W] nodes reached so far per source, the source not counted
    int32_t *src;                          // [64 HOP_MAX_W] the batch's sources on the device
    int32_t *dist;                         // [64 W][n] of the batch, or nullptr

    int setup(bool want_dist, int max_w) {
        n = g->n;
        AnalysisState &A = analysis_of(g);
        DCR_TRY(A.hop_bits.grow(3 * n * max_w));
        DCR_TRY(A.hop_ctl.grow((int64_t)64 * HOP_MAX_W * (int64_t)(sizeof(unsigned long long) + sizeof(int32_t))));
        if (want_dist) DCR_TRY(A.hop_dist.grow((int64_t)64 * max_w * n));
        totals = (unsigned long long *)A.hop_ctl.p;
        src = (int32_t *)(totals + 64 * HOP_MAX_W);
        dist = want_dist ? A.hop_dist.p : nullptr;
        return build_row_plan(g, &plan, nullptr);
    }

    // B sources (sources, or the nodes first, first + 1, ... where it is nullptr) as one batch of W words; the four outputs at
    // the batch's first source, each may be nullptr
    template <int W>
    int batch(const int32_t *sources, int64_t first, int B, int64_t max_hops, int32_t *out_dist, int32_t *out_ecc, int64_t *out_reached,
              int64_t *out_total) {
        hipStream_t st = g->stream;
        visited = g->analysis->hop_bits.p;
        frontier = visited + n * W;
        next = frontier + n * W;
        DCR_HIP(hipMemsetAsync(visited, 0, sizeof(uint64_t) * (size_t)(2 * n * W), st));  // (every row writes `next` in every level)
        DCR_HIP(hipMemsetAsync(totals, 0, sizeof(unsigned long long) * 64 * HOP_MAX_W, st));
        if (dist) DCR_HIP(hipMemsetAsync(dist, 0xff, sizeof(int32_t) * (size_t)((int64_t)B * n), st));
        if (sources) DCR_HIP(hipMemcpyAsync(src, sources, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_hop_init<W>, dim3(blocks_of(B)), dim3(256), 0, st, sources ? src : nullptr, first, B, n, visited, frontier, dist);
        DCR_HIP(hipGetLastError());

        HopWords<W> live;
        for (int w = 0; w < W; ++w) live.w[w] = B >= 64 * (w + 1) ? ~0ull : B > 64 * w ? (1ull << (B - 64 * w)) - 1 : 0ull;
        std::vector<int32_t> ecc((size_t)B, 0);
        std::vector<int64_t> reached((size_t)B, 1), total((size_t)B, 0);
        unsigned long long now[64 * HOP_MAX_W], before[64 * HOP_MAX_W] = {};
        for (int64_t level = 1; max_hops < 0 || level <= max_hops; ++level) {
            if (level > n) DCR_FAIL(DCR_ESTATE, "hop distances: more levels than nodes");
            hipLaunchKernelGGL(k_hop_level<W>, dim3(row_grid<HopRows>(plan)), dim3(256), 0, st, plan, g->rowinfo.p, g->col.p, frontier, visited,
                               next, live);
            hipLaunchKernelGGL(k_hop_count<W>, dim3(std::min(blocks_of((n + 63) / 64, 4), (unsigned)HOP_COUNT_BLOCKS)), dim3(256), 0, st, next,
                               n, (int32_t)level, dist, totals);
            DCR_HIP(hipGetLastError());
            DCR_HIP(hipMemcpyAsync(now, totals, sizeof(unsigned long long) * 64 * W, hipMemcpyDeviceToHost, st));
            DCR_HIP(hipStreamSynchronize(st));
            bool any = false;
            for (int i = 0; i < B; ++i) {
                const int64_t c = (int64_t)(now[i] - before[i]);
                before[i] = now[i];
                if (c > 0) {
                    ecc[(size_t)i] = (int32_t)level;
                    reached[(size_t)i] += c;
                    total[(size_t)i] += level * c;
                    any = true;
                } else {
                    live.w[i >> 6] &= ~(1ull << (i & 63));  // this source has its component: no row waits for it any more
                }
            }
            if (!any) break;
            std::swap(frontier, next);
        }
        if (out_dist) DCR_HIP(hipMemcpyAsync(out_dist, dist, sizeof(int32_t) * (size_t)((int64_t)B * n), hipMemcpyDeviceToHost, st));
        DCR_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < B; ++i) {
            if (out_ecc) out_ecc[i] = ecc[(size_t)i];
            if (out_reached) out_reached[i] = reached[(size_t)i];
            if (out_total) out_total[i] = total[(size_t)i];
        }
        return DCR_OK;
    }
};

// DCR_HOPS_W=1 | 2 | 4 fixes the words of a batch for a call (tools/probe_hops.py times them against each other); otherwise the
// narrowest that holds what is left of the call, 4 at most
static int hops_forced_words() {
    const char *e = getenv("DCR_HOPS_W");
    const int w = e ? atoi(e) : 0;
    return w == 1 || w == 2 || w == 4 ? w : 0;
}

}  // namespace dcr

using namespace dcr;

extern "C" {

int dcr_hop_distances(dcr_graph *g, const int32_t *sources, int64_t P, const dcr_hops_opts *opts, int32_t *out_dist, int32_t *out_ecc,
                      int64_t *out_reached, int64_t *out_total) {
    if (!g) DCR_FAIL(DCR_EINVAL, "null graph");
    if (P < 0) DCR_FAIL(DCR_EINVAL, "negative source count");
    if (!sources && P != g->n) DCR_FAIL(DCR_EINVAL, "sources NULL stands for every node: P must be num_nodes");
    if (sources)
        for (int64_t i = 0; i < P; ++i)
            if (sources[i] < 0 || sources[i] >= g->n) DCR_FAIL(DCR_EINVAL, "source outside 0 .. num_nodes - 1");
    if (P == 0) return DCR_OK;
    const int64_t max_hops = opts && opts->max_hops >= 0 ? opts->max_hops : -1;
    DCR_HIP(hipSetDevice(g->device));
    const int forced = hops_forced_words();
    HopRun R;
    R.g = g;
    DCR_TRY(R.setup(out_dist != nullptr, forced ? forced : P <= 64 ? 1 : P <= 128 ? 2 : HOP_MAX_W));
    for (int64_t first = 0; first < P;) {
        const int64_t left = P - first;
        const int W = forced ? forced : left <= 64 ? 1 : left <= 128 ? 2 : HOP_MAX_W;
        const int B = (int)std::min<int64_t>(left, 64 * W);
        const int32_t *s = sources ? sources + first : nullptr;
        int32_t *od = out_dist ? out_dist + first * g->n : nullptr, *oe = out_ecc ? out_ecc + first : nullptr;
        int64_t *orr = out_reached ? out_reached + first : nullptr, *ot = out_total ? out_total + first : nullptr;
        if (W == 1)
            DCR_TRY(R.batch<1>(s, first, B, max_hops, od, oe, orr, ot));
        else if (W == 2)
            DCR_TRY(R.batch<2>(s, first, B, max_hops, od, oe, orr, ot));
        else
            DCR_TRY(R.batch<4>(s, first, B, max_hops, od, oe, orr, ot));
        first += B;
    }
    return DCR_OK;
}

}  // extern "C"
