// Monte-Carlo Cheeger estimate on the device-resident graph: edge counts of many random node subsets in one sweep of the rows.
//
// Replaces the inner work of the reference's experiment/compute_cheeger.py: random_subset (:19-24), boundary_size (:32-37),
// vol (:27-29) and cheeger_S (:40-45) for every draw of estimate_cheeger (:48-64).  For a subset S and every undirected edge
// a < b the reference needs three integers,
//     in = #{a in S, b in S}     lo = #{a in S, b not in S}     hi = #{a not in S, b in S}
// (out = E - in - lo - hi): boundary_size counts lo only, vol(G.subgraph(S)) = 2 in, vol(G - S) = 2 out.  Subsets are packed
// 64 to a machine word: the membership matrix is node-major uint64 [n][W], bit k of word w of node v = v is a member of subset
// 64 w + k.  Everything up to the final division is integer arithmetic, so any order of summation gives the same bits; the
// counts of a workgroup are added to the totals with 64-bit integer atomics.
//
// Two kernels compute the same counts (DESIGN §4.5 has the measurements; DCR_CHEEGER=lane | sliced picks one per call):
//   * k_cheeger_lane    a lane per subset: a wave walks a run of adjacency slots, the two endpoints' words are the same address
//                       in every lane, each lane extracts its own bit of both and adds three counters;
//   * k_cheeger_sliced  a lane per (slot stream, word): the three 64-bit products mu & mv, mu & ~mv, ~mu & mv are added into
//                       bit-sliced counters (plane p holds bit p of 64 counters at once), a 3-plane counter taking seven slots and
//                       then being added into a 10-plane one; the planes are turned into integers once per workgroup, in LDS.
// Both take every undirected edge at the slot where col > row, as the curvature array does, and skip the slack of the rows.
#include <cstdlib>

#include "dcr_analysis.h"
#include "dcr_philox.h"

namespace dcr {

// ---- shape (a): a lane per subset ---------------------------------------------------------------------------------------------
// grid (slot chunks, W); the four waves of a workgroup share the chunk, four slots of a wave in flight together.
__global__ void __launch_bounds__(256) k_cheeger_lane(const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                       const int32_t *__restrict__ slot_row, int64_t cap_total,
                                                       const uint64_t *__restrict__ mem, int W, int64_t slots_per_wg,
                                                       unsigned long long *counts, int64_t n_sub) {
    __shared__ uint32_t sh[3][256];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int w = blockIdx.y;
    const int64_t s_begin = (int64_t)blockIdx.x * slots_per_wg;
    const int64_t s_end = s_begin + slots_per_wg < cap_total ? s_begin + slots_per_wg : cap_total;
    uint32_t n_in = 0, n_a = 0, n_b = 0;
    for (int64_t s0 = s_begin + 4 * wave; s0 < s_end; s0 += 16) {
        int u[4], v[4];
        int2 ri[4];
        bool ok[4];
        uint64_t mu[4], mv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t s = s0 + q;
            ok[q] = s < s_end;
            u[q] = ok[q] ? slot_row[s] : 0;
            v[q] = ok[q] ? col[s] : -1;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) ri[q] = ok[q] ? rowinfo[u[q]] : make_int2(0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ok[q] = ok[q] && (s0 + q - ri[q].x) < (int64_t)ri[q].y && v[q] > u[q];  // a live slot holding the edge's upper end
            mu[q] = ok[q] ? mem[(int64_t)u[q] * W + w] : 0ull;
            mv[q] = ok[q] ? mem[(int64_t)v[q] * W + w] : 0ull;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!ok[q]) continue;
            const uint32_t a = (uint32_t)(mu[q] >> lane) & 1u, b = (uint32_t)(mv[q] >> lane) & 1u;
            n_a += a;
            n_b += b;
            n_in += a & b;
        }
    }
    sh[0][threadIdx.x] = n_in;
    sh[1][threadIdx.x] = n_a - n_in;  // lower end inside, upper end outside
    sh[2][threadIdx.x] = n_b - n_in;
    __syncthreads();
    if (threadIdx.x < 192) {  // wave c adds category c: 512 contiguous bytes per atomic instruction
        const int c = threadIdx.x >> 6;
        const unsigned long long t = (unsigned long long)sh[c][lane] + sh[c][64 + lane] + sh[c][128 + lane] + sh[c][192 + lane];
        if (t) atomicAdd(&counts[(int64_t)c * n_sub + 64 * (int64_t)w + lane], t);
    }
}

// ---- shape (b): bit-sliced counters ---------------------------------------------------------------------------------------------
constexpr int CH_LOW = 3, CH_HIGH = 10, CH_RUN = 7;       // 3 planes count a run of 7 slots; 10 planes count to 1023
constexpr int CH_MAX_ROUNDS = ((1 << CH_HIGH) - 1) / CH_RUN;  // runs of one lane in a launch: 146

__device__ inline void planes_add1(uint64_t (&L)[CH_LOW], uint64_t x) {  // L += x, x one bit per counter; at most 7 times
    uint64_t t = L[0] & x;
    L[0] ^= x;
    x = t;
    t = L[1] & x;
    L[1] ^= x;
    L[2] ^= t;
}

__device__ inline void planes_fold(uint64_t (&H)[CH_HIGH], uint64_t (&L)[CH_LOW]) {  // H += L; L = 0
    uint64_t carry = 0;
#pragma unroll
    for (int p = 0; p < CH_LOW; ++p) {
        const uint64_t a = H[p], b = L[p], s = a ^ b;
        H[p] = s ^ carry;
        carry = (a & b) | (s & carry);
        L[p] = 0;
    }
#pragma unroll
    for (int p = CH_LOW; p < CH_HIGH; ++p) {
        const uint64_t t = H[p] & carry;
        H[p] ^= carry;
        carry = t;
    }
}

// WL adjacent lanes take WL adjacent words of the same slot (one 8 WL-byte piece of each endpoint's row); the workgroup's
// 256 / WL slot streams take adjacent slots.  grid (slot chunks of (256 / WL) * 7 * rounds, W / WL rounded up).
template <int WL>
__global__ void __launch_bounds__(256) k_cheeger_sliced(const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                         const int32_t *__restrict__ slot_row, int64_t cap_total,
                                                         const uint64_t *__restrict__ mem, int W, int rounds,
                                                         unsigned long long *counts, int64_t n_sub) {
    constexpr int NS = 256 / WL;
    __shared__ uint64_t sh[CH_HIGH][256];
    const int t = threadIdx.x, wsub = t & (WL - 1), stream = t / WL;
    const int w = blockIdx.y * WL + wsub;
    const bool active = w < W;
    const int64_t s_begin = (int64_t)blockIdx.x * ((int64_t)NS * CH_RUN * rounds);
    uint64_t L[3][CH_LOW], H[3][CH_HIGH];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int p = 0; p < CH_LOW; ++p) L[c][p] = 0;
#pragma unroll
        for (int p = 0; p < CH_HIGH; ++p) H[c][p] = 0;
    }
    for (int r = 0; r < rounds; ++r) {
        const int64_t s_run = s_begin + (int64_t)r * CH_RUN * NS + stream;
        if (s_run - stream >= cap_total) break;  // the same for every thread of the workgroup
#pragma unroll
        for (int i = 0; i < CH_RUN; ++i) {
            const int64_t s = s_run + (int64_t)i * NS;
            bool ok = active && s < cap_total;
            const int u = ok ? slot_row[s] : 0;
            const int v = ok ? col[s] : -1;
            const int2 ri = ok ? rowinfo[u] : make_int2(0, 0);
            ok = ok && (s - ri.x) < (int64_t)ri.y && v > u;
            const uint64_t mu = ok ? mem[(int64_t)u * W + w] : 0ull;
            const uint64_t mv = ok ? mem[(int64_t)v * W + w] : 0ull;
            planes_add1(L[0], mu & mv);
            planes_add1(L[1], mu & ~mv);
            planes_add1(L[2], ~mu & mv);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) planes_fold(H[c], L[c]);
    }
    // planes -> integers, a category at a time: thread t owns outputs [t * NB, t * NB + NB) of the workgroup's 64 * WL
    constexpr int NB = WL >= 4 ? WL / 4 : 1;
    const int o0 = t * NB;
    const bool owner = o0 < 64 * WL;
    const int ow = owner ? o0 >> 6 : 0, bit0 = o0 & 63;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c) __syncthreads();
#pragma unroll
        for (int p = 0; p < CH_HIGH; ++p) sh[p][t] = H[c][p];
        __syncthreads();
        if (!owner) continue;
        uint32_t cnt[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) cnt[j] = 0;
        for (int st = 0; st < NS; ++st) {
#pragma unroll
            for (int p = 0; p < CH_HIGH; ++p) {
                const uint64_t word = sh[p][st * WL + ow] >> bit0;
#pragma unroll
                for (int j = 0; j < NB; ++j) cnt[j] += ((uint32_t)(word >> j) & 1u) << p;
            }
        }
        const int wo = blockIdx.y * WL + ow;
        if (wo < W) {
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if (cnt[j]) atomicAdd(&counts[(int64_t)c * n_sub + 64 * (int64_t)wo + bit0 + j], (unsigned long long)cnt[j]);
        }
    }
}

// ---- membership from Philox ---------------------------------------------------------------------------------------------------
// include/dcr.h states the mapping: subset j, node v -> bit (j & 31) of word (j >> 5) & 3 of philox4x32_10(v, j >> 7, seed).
__global__ void __launch_bounds__(256) k_cheeger_draw(uint64_t *mem, int64_t n, int W, int64_t first_word, uint64_t seed) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * W) return;
    const int64_t v = i / W, wa = first_word + (i - v * W);
    uint32_t r[4];
    philox4x32_10((uint64_t)v, (uint64_t)(wa >> 1), seed, r);
    const int h = (int)(wa & 1) * 2;
    mem[i] = (uint64_t)r[h] | ((uint64_t)r[h + 1] << 32);
}

// ---- counts -> ratios ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cheeger_values(const unsigned long long *counts, int64_t n_sub, int64_t B, int64_t n_edges,
                                                         int definition, double *out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    out[j] = cheeger_ratio((int64_t)counts[j], (int64_t)counts[n_sub + j], (int64_t)counts[2 * n_sub + j], n_edges, definition);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static bool cheeger_use_lane() {
    const char *e = getenv("DCR_CHEEGER");
    return e && strcmp(e, "lane") == 0;
}

static int cheeger_buffers(dcr_graph *g, int64_t W) {
    DCR_HIP(hipSetDevice(g->device));
    AnalysisState &A = analysis_of(g);
    DCR_TRY(A.chg_members.grow(g->n * W));
    DCR_TRY(A.chg_counts.grow(3 * 64 * W));
    DCR_TRY(A.chg_values.grow(64 * W));
    return DCR_OK;
}

template <int WL>
static void launch_sliced(dcr_graph *g, int W) {
    const int64_t per_round = (int64_t)(256 / WL) * CH_RUN;
    const int groups = (W + WL - 1) / WL;
    // about four workgroups per CU in all, a workgroup at least four runs long
    int64_t rounds = (g->cap_total * groups) / (per_round * 4 * (g->num_cu > 0 ? g->num_cu : 256)) + 1;
    if (rounds < 4) rounds = 4;
    if (rounds > CH_MAX_ROUNDS) rounds = CH_MAX_ROUNDS;
    const int64_t chunk = per_round * rounds;
    const unsigned gx = (unsigned)((g->cap_total + chunk - 1) / chunk);
    hipLaunchKernelGGL(k_cheeger_sliced<WL>, dim3(gx, (unsigned)groups), dim3(256), 0, g->stream, g->rowinfo.p, g->col.p, g->slot_row.p,
                       g->cap_total, g->analysis->chg_members.p, W, (int)rounds, g->analysis->chg_counts.p, (int64_t)64 * W);
}

// counts of the subsets in chg_members [n][W] -> chg_counts [3][64 W] (after cheeger_buffers), on the graph's stream (no synchronisation)
static int cheeger_run(dcr_graph *g, int W) {
    const int64_t n_sub = (int64_t)64 * W;
    DCR_HIP(hipMemsetAsync(g->analysis->chg_counts.p, 0, sizeof(unsigned long long) * 3 * (size_t)n_sub, g->stream));
    if (g->cap_total <= 0 || g->n <= 0) return DCR_OK;
    if (cheeger_use_lane()) {
        int64_t per = g->cap_total * W / (8 * (g->num_cu > 0 ? g->num_cu : 256)) + 1;
        per = (per + 15) / 16 * 16;
        if (per < 512) per = 512;
        const unsigned gx = (unsigned)((g->cap_total + per - 1) / per);
        hipLaunchKernelGGL(k_cheeger_lane, dim3(gx, (unsigned)W), dim3(256), 0, g->stream, g->rowinfo.p, g->col.p, g->slot_row.p,
                           g->cap_total, g->analysis->chg_members.p, W, per, g->analysis->chg_counts.p, n_sub);
    } else if (W >= 16) {
        launch_sliced<16>(g, W);
    } else if (W > 4) {
        launch_sliced<8>(g, W);
    } else if (W > 2) {
        launch_sliced<4>(g, W);
    } else if (W == 2) {
        launch_sliced<2>(g, W);
    } else {
        launch_sliced<1>(g, W);
    }
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

static int cheeger_draw(dcr_graph *g, uint64_t seed, int64_t first, int W) {
    const int64_t total = g->n * W;
    if (total <= 0) return DCR_OK;
    hipLaunchKernelGGL(k_cheeger_draw, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, g->stream, g->analysis->chg_members.p, g->n, W,
                       first / 64, seed);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

// counts [3][n_sub] on the device -> out [B][3] on the host
static int cheeger_fetch_counts(dcr_graph *g, int64_t n_sub, int64_t B, int64_t *out) {
    std::vector<unsigned long long> h((size_t)(3 * n_sub));
    DCR_HIP(hipMemcpyAsync(h.data(), g->analysis->chg_counts.p, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, g->stream));
    DCR_HIP(hipStreamSynchronize(g->stream));
    for (int64_t j = 0; j < B; ++j)
        for (int c = 0; c < 3; ++c) out[3 * j + c] = (int64_t)h[(size_t)(c * n_sub + j)];
    return DCR_OK;
}

constexpr int64_t CHEEGER_MAX_WORDS = 65535;  // grid.y of the lane kernel

static int philox_args(const dcr_graph *g, int64_t first, int64_t B) {
    if (!g) DCR_FAIL(DCR_EINVAL, "null graph");
    if (first < 0 || (first & 63)) DCR_FAIL(DCR_EINVAL, "first subset must be a non-negative multiple of 64");
    if (B <= 0 || (B + 63) / 64 > CHEEGER_MAX_WORDS) DCR_FAIL(DCR_EINVAL, "subset count out of range");
    return DCR_OK;
}

}  // namespace dcr

using namespace dcr;

extern "C" {

int dcr_cheeger_counts(dcr_graph *g, const uint64_t *members, int64_t W, int64_t *out_counts) {
    if (!g || !members || !out_counts) DCR_FAIL(DCR_EINVAL, "null argument");
    if (W <= 0 || W > CHEEGER_MAX_WORDS) DCR_FAIL(DCR_EINVAL, "W out of range");
    DCR_TRY(cheeger_buffers(g, W));
    if (g->n > 0)
        DCR_HIP(hipMemcpyAsync(g->analysis->chg_members.p, members, sizeof(uint64_t) * (size_t)(g->n * W), hipMemcpyHostToDevice, g->stream));
    DCR_TRY(cheeger_run(g, (int)W));
    return cheeger_fetch_counts(g, 64 * W, 64 * W, out_counts);
}

int dcr_cheeger_philox_members(dcr_graph *g, uint64_t seed, int64_t first, int64_t W, uint64_t *out_members) {
    if (!out_members) DCR_FAIL(DCR_EINVAL, "null argument");
    if (W <= 0 || W > CHEEGER_MAX_WORDS) DCR_FAIL(DCR_EINVAL, "W out of range");
    DCR_TRY(philox_args(g, first, 64 * W));
    DCR_TRY(cheeger_buffers(g, W));
    DCR_TRY(cheeger_draw(g, seed, first, (int)W));
    if (g->n > 0)
        DCR_HIP(hipMemcpyAsync(out_members, g->analysis->chg_members.p, sizeof(uint64_t) * (size_t)(g->n * W), hipMemcpyDeviceToHost, g->stream));
    DCR_HIP(hipStreamSynchronize(g->stream));
    return DCR_OK;
}

int dcr_cheeger_philox_counts(dcr_graph *g, uint64_t seed, int64_t first, int64_t B, int64_t *out_counts) {
    if (!out_counts) DCR_FAIL(DCR_EINVAL, "null argument");
    DCR_TRY(philox_args(g, first, B));
    const int64_t W = (B + 63) / 64;
    DCR_TRY(cheeger_buffers(g, W));
    DCR_TRY(cheeger_draw(g, seed, first, (int)W));
    DCR_TRY(cheeger_run(g, (int)W));
    return cheeger_fetch_counts(g, 64 * W, B, out_counts);
}

int dcr_cheeger_philox_values(dcr_graph *g, uint64_t seed, int64_t first, int64_t B, int definition, double *out_values) {
    if (!out_values) DCR_FAIL(DCR_EINVAL, "null argument");
    if (definition != 0 && definition != 1) DCR_FAIL(DCR_EINVAL, "unknown definition");
    DCR_TRY(philox_args(g, first, B));
    const int64_t W = (B + 63) / 64;
    DCR_TRY(cheeger_buffers(g, W));
    DCR_TRY(cheeger_draw(g, seed, first, (int)W));
    DCR_TRY(cheeger_run(g, (int)W));
    hipLaunchKernelGGL(k_cheeger_values, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, g->stream, g->analysis->chg_counts.p, 64 * W, B,
                       g->n_edges, definition, g->analysis->chg_values.p);
    DCR_HIP(hipGetLastError());
    DCR_HIP(hipMemcpyAsync(out_values, g->analysis->chg_values.p, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, g->stream));
    DCR_HIP(hipStreamSynchronize(g->stream));
    return DCR_OK;
}

}  // extern "C"
