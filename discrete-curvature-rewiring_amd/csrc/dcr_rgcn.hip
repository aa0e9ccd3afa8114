// R-GCN typed sparse aggregation of libdcr_hip.so (models/rgcn.py): the mean-per-relation layer of Schlichtkrull et al. eq. 2,
// evaluated transform-first.  One GEMM gives Zall = X·[W_0 | … | W_{R-1} | W_root]; ONE sweep of a typed CSR then forms the
// layer's output (k_spmm_typed, the gather) and, on the CSR of the transposed pattern, the whole gradient of Zall
// (k_spmm_typed_expand, the expand).
//
// Typed CSR: rowptr int64, col int32, val float32 (1/|N_r(i)|), rel uint8 per slot.  PRECONDITION of both kernels: inside a row
// the slots are sorted by relation (stably within one), every rel[e] < n_rel.  A larger rel[e] is read as n_rel - 1, so a CSR
// that breaks the precondition gives wrong sums but no access outside the operands.
//
// Both kernels have the shape of k_spmm_csr (csrc/dcr_gcn.hip): a group of LPR lanes per row, each lane VEC consecutive
// features, U gathers in flight per group, rows above SPMM_LONG slots parked in LDS and taken by the whole workgroup in a
// fixed strided order.  Like it they are gather-bound: a slot pulls n_feat floats of one row of the operand.  No atomics on
// floats anywhere: the results are the same bits on every run.
#include <cstdint>
#include "dcr_internal.h"

namespace dcr {

constexpr int TSPMM_LONG = 96;    // = SPMM_LONG of csrc/dcr_gcn.hip: the n_rel = 1 gather is bit-identical to k_spmm_csr
constexpr int TSPMM_MAX_REL = 8;

template <int VEC>
__device__ inline void load_vec(const float *__restrict__ src, float (&b)[VEC]) {
    if (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(src);
        b[0] = t.x; b[1 % VEC] = t.y; b[2 % VEC] = t.z; b[3 % VEC] = t.w;
    } else if (VEC == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(src);
        b[0] = t.x; b[1 % VEC] = t.y;
    } else {
        b[0] = src[0];
    }
}

// (the expand only: its dispatch asks for a 16- / 8-byte aligned C before it picks VEC 4 / 2)
template <int VEC>
__device__ inline void store_vec(float *__restrict__ dst, const float (&b)[VEC]) {
    if (VEC == 4) *reinterpret_cast<float4 *>(dst) = make_float4(b[0], b[1 % VEC], b[2 % VEC], b[3 % VEC]);
    else if (VEC == 2) *reinterpret_cast<float2 *>(dst) = make_float2(b[0], b[1 % VEC]);
    else dst[0] = b[0];
}

// U slots e, e + stride, ... of one row: weight, relation and the VEC floats each gathers from row col[.] of M at column
// f0 + rel[.] * blk (blk = n_feat: the gather's typed column block; 0: the expand, which reads plain rows of G).
template <int VEC, int U>
struct SlotBatch {
    float w[U];
    int r[U];
    bool ok[U];
    float b[U][VEC];
};

// MASKED: slots at or past e1 are switched off (the last batch of a row): one batch with its loads side by side, not one
// slot after another with two memory latencies each (k_spmm_csr's tail, for the same reason).
template <int VEC, int U, bool MASKED>
__device__ inline void load_batch(const int32_t *__restrict__ col, const float *__restrict__ val, const uint8_t *__restrict__ rel,
                                  const float *__restrict__ M, int64_t ld, int blk, int rmax, int f0, int64_t e, int64_t e1,
                                  int64_t stride, SlotBatch<VEC, U> &t) {
    int c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t eu = e + u * stride;
        t.ok[u] = !MASKED || eu < e1;
        c[u] = t.ok[u] ? col[eu] : 0;
        t.w[u] = t.ok[u] ? val[eu] : 0.f;
        const int r = t.ok[u] ? (int)rel[eu] : 0;
        t.r[u] = r < rmax ? r : rmax;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (t.ok[u]) {
            load_vec<VEC>(M + (int64_t)c[u] * ld + (int64_t)t.r[u] * blk + f0, t.b[u]);
        } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q) t.b[u][q] = 0.f;
        }
    }
}

// acc += Σ val·M[col, f0 + rel·blk ...] over slots e0, e0 + stride, ... < e1, one fmaf per slot in that order: the operations
// and the order of spmm_accumulate (csrc/dcr_gcn.hip).
template <int VEC, int U>
__device__ inline void typed_accumulate(const int32_t *__restrict__ col, const float *__restrict__ val,
                                        const uint8_t *__restrict__ rel, const float *__restrict__ M, int64_t ld, int blk, int rmax,
                                        int f0, int64_t e0, int64_t e1, int64_t stride, float (&acc)[VEC]) {
    SlotBatch<VEC, U> t;
    int64_t e = e0;
    for (; e + (U - 1) * stride < e1; e += U * stride) {
        load_batch<VEC, U, false>(col, val, rel, M, ld, blk, rmax, f0, e, e1, stride, t);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc[q] = fmaf(t.w[u], t.b[u][q], acc[q]);
    }
    if (e < e1) {
        load_batch<VEC, U, true>(col, val, rel, M, ld, blk, rmax, f0, e, e1, stride, t);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc[q] = t.ok[u] ? fmaf(t.w[u], t.b[u][q], acc[q]) : acc[q];
    }
}

// ---- the gather (forward): C[i,:] = Σ_e val[e]·B[col[e], rel[e]·n_feat + :] (+ B[i, n_rel·n_feat + :]) (+ bias) (ReLU) ----------
template <int LPR, int VEC>
__global__ void __launch_bounds__(256) k_spmm_typed(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                     const float *__restrict__ val, const uint8_t *__restrict__ rel,
                                                     const float *__restrict__ B, float *__restrict__ C, int64_t n_rows, int n_feat,
                                                     int n_rel, int64_t ldb, int64_t ldc, int self_block,
                                                     const float *__restrict__ bias, int relu) {
    constexpr int G = 256 / LPR;             // rows per workgroup / lane groups per workgroup
    constexpr int U = LPR <= 8 ? 8 : 4;
    __shared__ int long_rows[G];
    __shared__ int n_long;
    __shared__ float red[256 * VEC];
    const int sub = threadIdx.x / LPR;
    const int sl = threadIdx.x % LPR;
    const int64_t row = (int64_t)sub * gridDim.x + blockIdx.x;   // (k_spmm_csr's deal: consecutive hub rows in different workgroups)
    const int rmax = n_rel - 1;
    // the sum of one row's slots, then the row's own block, then the bias: one rounding each
    auto finish = [&](int64_t i, int f0, const float (&sum)[VEC]) {
        float own[VEC];
        if (self_block) load_vec<VEC>(B + i * ldb + (int64_t)n_rel * n_feat + f0, own);
        float *dst = C + i * ldc + f0;
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            float r = sum[q];
            if (self_block) r += own[q];
            if (bias) r += bias[f0 + q];
            if (relu) r = r > 0.f ? r : 0.f;
            dst[q] = r;
        }
    };
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
    if (row < n_rows) {
        const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
        if (e1 - e0 > TSPMM_LONG) {
            if (sl == 0) long_rows[atomicAdd(&n_long, 1)] = sub;
        } else {
            for (int f0 = sl * VEC; f0 < n_feat; f0 += LPR * VEC) {
                float acc[VEC];
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
                typed_accumulate<VEC, U>(col, val, rel, B, ldb, n_feat, rmax, f0, e0, e1, 1, acc);
                finish(row, f0, acc);
            }
        }
    }
    __syncthreads();
    const int nl = n_long;  // uniform
    for (int li = 0; li < nl; ++li) {
        const int64_t lrow = (int64_t)long_rows[li] * gridDim.x + blockIdx.x;
        const int64_t e0 = rowptr[lrow], e1 = rowptr[lrow + 1];
        for (int fb = 0; fb < n_feat; fb += LPR * VEC) {  // uniform trip count
            const int f0 = fb + sl * VEC;
            float acc[VEC];
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
            if (f0 < n_feat) typed_accumulate<VEC, U>(col, val, rel, B, ldb, n_feat, rmax, f0, e0 + sub, e1, G, acc);
#pragma unroll
            for (int q = 0; q < VEC; ++q) red[threadIdx.x * VEC + q] = acc[q];
            __syncthreads();
            if (sub == 0 && f0 < n_feat) {
                float sum[VEC];
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    float r = 0.f;
                    for (int g = 0; g < G; ++g) r += red[(g * LPR + sl) * VEC + q];
                    sum[q] = r;
                }
                finish(lrow, f0, sum);
            }
            __syncthreads();
        }
    }
}

// ---- the expand (backward, on the CSR of the transposed pattern) ---------------------------------------------------------
// C[j, r·n_feat + :] = Σ_{e in row j, rel[e] = r} val[e]·G[col[e], :] for EVERY r (zeros where row j has no slot of r), and
// C[j, n_rel·n_feat + :] = G[j, :] with self_block: every element of C's (n_rel + self_block)·n_feat columns is written.
// The slots of a row are sorted by relation, so a row needs ONE accumulator, stored and cleared when the relation moves on.
template <int LPR, int VEC>
__global__ void __launch_bounds__(256) k_spmm_typed_expand(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                            const float *__restrict__ val, const uint8_t *__restrict__ rel,
                                                            const float *__restrict__ Gm, float *__restrict__ C, int64_t n_rows,
                                                            int n_feat, int n_rel, int64_t ldg, int64_t ldc, int self_block) {
    constexpr int G = 256 / LPR;
    constexpr int U = LPR <= 8 ? 8 : 4;
    __shared__ int long_rows[G];
    __shared__ int n_long;
    __shared__ float red[256 * VEC];
    __shared__ int64_t seg[TSPMM_MAX_REL + 1];   // a hub row's slots of relation r: seg[r] .. seg[r + 1]
    const int sub = threadIdx.x / LPR;
    const int sl = threadIdx.x % LPR;
    const int64_t row = (int64_t)sub * gridDim.x + blockIdx.x;
    const int rmax = n_rel - 1;
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
    if (row < n_rows) {
        const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
        if (e1 - e0 > TSPMM_LONG) {
            if (sl == 0) long_rows[atomicAdd(&n_long, 1)] = sub;
        } else {
            for (int f0 = sl * VEC; f0 < n_feat; f0 += LPR * VEC) {
                float *dst = C + row * ldc + f0;
                float acc[VEC];
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
                int cur = 0;   // the relation acc belongs to; blocks below it are written
                // a slot of a later relation: store the finished block and the empty ones before the slot's (cur <= rmax always)
                auto add = [&](const SlotBatch<VEC, U> &t, int u) {
                    while (cur < t.r[u]) {
                        store_vec<VEC>(dst + (int64_t)cur * n_feat, acc);
#pragma unroll
                        for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
                        ++cur;
                    }
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[q] = fmaf(t.w[u], t.b[u][q], acc[q]);
                };
                SlotBatch<VEC, U> t;
                int64_t e = e0;
                for (; e + (U - 1) < e1; e += U) {
                    load_batch<VEC, U, false>(col, val, rel, Gm, ldg, 0, rmax, f0, e, e1, 1, t);
#pragma unroll
                    for (int u = 0; u < U; ++u) add(t, u);
                }
                if (e < e1) {
                    load_batch<VEC, U, true>(col, val, rel, Gm, ldg, 0, rmax, f0, e, e1, 1, t);
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (t.ok[u]) add(t, u);
                }
                for (; cur < n_rel; ++cur) {
                    store_vec<VEC>(dst + (int64_t)cur * n_feat, acc);
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
                }
                if (self_block) {
                    load_vec<VEC>(Gm + row * ldg + f0, acc);
                    store_vec<VEC>(dst + (int64_t)n_rel * n_feat, acc);
                }
            }
        }
    }
    __syncthreads();
    const int nl = n_long;  // uniform
    for (int li = 0; li < nl; ++li) {
        const int64_t lrow = (int64_t)long_rows[li] * gridDim.x + blockIdx.x;
        const int64_t e0 = rowptr[lrow], e1 = rowptr[lrow + 1];
        // where each relation's slots start: seg[q] = the first slot of relation >= q (e1: none)
        if (threadIdx.x <= n_rel) seg[threadIdx.x] = e1;
        __syncthreads();
        for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
            const int r = min((int)rel[e], rmax);
            const int before = e == e0 ? -1 : min((int)rel[e - 1], rmax);
            for (int q = before + 1; q <= r; ++q) seg[q] = e;
        }
        __syncthreads();
        float *dst0 = C + lrow * ldc;
        for (int fb = 0; fb < n_feat; fb += LPR * VEC) {  // uniform trip count
            const int f0 = fb + sl * VEC;
            for (int r = 0; r < n_rel; ++r) {
                // relation r's slots as k_spmm_csr takes a hub row: group g the slots g, g + G, ... of them, partial sums
                // added in group order
                const int64_t s0 = seg[r], s1 = seg[r + 1];
                float acc[VEC];
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
                if (f0 < n_feat) typed_accumulate<VEC, U>(col, val, rel, Gm, ldg, 0, rmax, f0, s0 + sub, s1, G, acc);
#pragma unroll
                for (int q = 0; q < VEC; ++q) red[threadIdx.x * VEC + q] = acc[q];
                __syncthreads();
                if (sub == 0 && f0 < n_feat) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        float s = 0.f;
                        for (int g = 0; g < G; ++g) s += red[(g * LPR + sl) * VEC + q];
                        acc[q] = s;
                    }
                    store_vec<VEC>(dst0 + (int64_t)r * n_feat + f0, acc);
                }
                __syncthreads();   // (red is free again; after the last relation, so is seg)
            }
            if (self_block && sub == 0 && f0 < n_feat) {
                float own[VEC];
                load_vec<VEC>(Gm + lrow * ldg + f0, own);
                store_vec<VEC>(dst0 + (int64_t)n_rel * n_feat + f0, own);
            }
        }
    }
}

}  // namespace dcr

using namespace dcr;

// the (LPR, VEC) table of spmm_dispatch (csrc/dcr_gcn.hip): LPR from the number of VEC-wide pieces of one row
#define DCR_TYPED_PICK(GO, F, v4, v2)             \
    do {                                          \
        if (v4) {                                 \
            const int lanes = (F) / 4;            \
            if (lanes <= 4) GO(4, 4);             \
            else if (lanes <= 8) GO(8, 4);        \
            else if (lanes <= 16) GO(16, 4);      \
            else if (lanes <= 32) GO(32, 4);      \
            else GO(64, 4);                       \
        } else if (v2) {                          \
            const int lanes = (F) / 2;            \
            if (lanes <= 4) GO(4, 2);             \
            else if (lanes <= 8) GO(8, 2);        \
            else if (lanes <= 16) GO(16, 2);      \
            else if (lanes <= 32) GO(32, 2);      \
            else GO(64, 2);                       \
        } else {                                  \
            if ((F) <= 4) GO(4, 1);               \
            else if ((F) <= 8) GO(8, 1);          \
            else if ((F) <= 16) GO(16, 1);        \
            else if ((F) <= 32) GO(32, 1);        \
            else GO(64, 1);                       \
        }                                         \
    } while (0)

// what spmm_dispatch rejects, for a typed call: `wide` is the operand with (n_rel + self_block) column blocks
static int typed_check(const void *rowptr, const void *col, const void *val, const void *rel, const void *in, const void *out,
                       int64_t n_rows, int64_t n_feat, int64_t n_rel, int64_t ld_narrow, int64_t ld_wide, int self_block) {
    if (!rowptr || !col || !val || !rel || !in || !out || n_rows < 0 || n_feat <= 0 || n_rel < 1 || n_rel > TSPMM_MAX_REL ||
        (self_block != 0 && self_block != 1))
        DCR_FAIL(DCR_EINVAL, "bad typed SpMM arguments");
    if (n_feat > INT32_MAX / 2 / (TSPMM_MAX_REL + 1)) DCR_FAIL(DCR_EINVAL, "n_feat too large");
    if (ld_narrow < n_feat || ld_wide < (n_rel + self_block) * n_feat) DCR_FAIL(DCR_EINVAL, "bad typed SpMM arguments (leading dimension)");
    return DCR_OK;
}

extern "C" int dcr_spmm_csr_typed_f32_dev(const int64_t *rowptr, const int32_t *col, const float *val, const uint8_t *rel,
                                          const float *B, float *C, int64_t n_rows, int64_t n_feat, int64_t n_rel, int64_t ldb,
                                          int64_t ldc, int self_block, const float *bias, int relu, void *hip_stream) {
    DCR_TRY(typed_check(rowptr, col, val, rel, B, C, n_rows, n_feat, n_rel, ldc, ldb, self_block));
    if (n_rows == 0) return DCR_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const int F = (int)n_feat;
    // (exactly spmm_dispatch's choice, which does not look at C's alignment: the stores are scalar, as k_spmm_csr's)
    const bool v4 = (F % 4 == 0) && (ldb % 4 == 0) && (ldc % 4 == 0) && (((uintptr_t)B & 15) == 0);
    const bool v2 = (F % 2 == 0) && (ldb % 2 == 0) && (ldc % 2 == 0) && (((uintptr_t)B & 7) == 0);
#define GO(L, V)                                                                                                                 \
    hipLaunchKernelGGL((k_spmm_typed<L, V>), dim3((unsigned)((n_rows + 256 / L - 1) / (256 / L))), dim3(256), 0, st, rowptr, col, \
                       val, rel, B, C, n_rows, F, (int)n_rel, ldb, ldc, self_block, bias, relu)
    DCR_TYPED_PICK(GO, F, v4, v2);
#undef GO
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

extern "C" int dcr_spmm_csr_typed_expand_f32_dev(const int64_t *rowptr, const int32_t *col, const float *val, const uint8_t *rel,
                                                 const float *G, float *C, int64_t n_rows, int64_t n_feat, int64_t n_rel,
                                                 int64_t ldg, int64_t ldc, int self_block, void *hip_stream) {
    DCR_TRY(typed_check(rowptr, col, val, rel, G, C, n_rows, n_feat, n_rel, ldg, ldc, self_block));
    if (n_rows == 0) return DCR_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const int F = (int)n_feat;
    // (the column blocks of C start n_feat apart: with n_feat and ldc multiples of VEC every vector store is aligned when C is)
    const bool v4 = (F % 4 == 0) && (ldg % 4 == 0) && (ldc % 4 == 0) && (((uintptr_t)G & 15) == 0) && (((uintptr_t)C & 15) == 0);
    const bool v2 = (F % 2 == 0) && (ldg % 2 == 0) && (ldc % 2 == 0) && (((uintptr_t)G & 7) == 0) && (((uintptr_t)C & 7) == 0);
#define GO(L, V)                                                                                                                   \
    hipLaunchKernelGGL((k_spmm_typed_expand<L, V>), dim3((unsigned)((n_rows + 256 / L - 1) / (256 / L))), dim3(256), 0, st, rowptr, \
                       col, val, rel, G, C, n_rows, F, (int)n_rel, ldg, ldc, self_block)
    DCR_TYPED_PICK(GO, F, v4, v2);
#undef GO
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}
