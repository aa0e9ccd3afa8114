// Sparse aggregation of libdcr_hip.so on CSR, fp32: three kernels on one set of pieces.
//
//   k_spmm_csr           C = Â · B (+ bias, ReLU): the GCN propagate (replaces the scatter-add of torch_geometric GCNConv,
//                        call site models/gcn.py), over all rows or a row list, one or two column blocks of B in one sweep.
//   k_spmm_typed         the R-GCN gather (models/rgcn.py; Schlichtkrull et al. eq. 2, transform-first): one GEMM gives
//                        Zall = X·[W_0 | … | W_{R-1} | W_root], ONE sweep of a typed CSR then forms the layer's output.
//   k_spmm_typed_expand  its backward on the CSR of the transposed pattern: the whole gradient of Zall in one sweep.
//
// CSR: rowptr int64, col int32, val float32.  Typed CSR: also rel uint8 per slot.  PRECONDITION of the typed kernels: inside a
// row the slots are sorted by relation (stably within one), every rel[e] < n_rel.  A larger rel[e] is read as n_rel - 1, so a
// CSR that breaks the precondition gives wrong sums but no access outside the operands.
//
// HBM / Infinity-Cache gather-bound: every slot pulls one row of the operand (n_feat floats).  A row of the matrix is owned by a
// group of LPR lanes, each lane holding VEC consecutive features, so one wave-instruction reads (64/LPR) operand rows in 16-byte
// pieces (full 128-B lines for n_feat >= 32) and a wave covers 64/LPR output rows.  MFMA has nothing to do here: the dense
// contraction (X·Wᵀ) is done before these kernels on the matrix cores by the GEMM library.
//
// The order of every sum is fixed and the same in all three (tests/spmm_order_ref.py restates it, tests/test_spmm_order_gpu.py
// compares the bits): one fmaf per slot in slot order; a row above SPMM_LONG slots as G strided partial sums added in group
// order; then the row's own block, the bias, ReLU, one rounding each.  No atomics on floats: the same bits on every run, and the
// n_rel = 1 gather is the plain product bit for bit.
#include <cstdint>
#include <initializer_list>
#include <type_traits>
#include "dcr_internal.h"
#include "dcr_spmm_pieces.h"   // SPMM_LONG, Deal, load_vec, store_vec, deal_rows, sum_groups (shared with csrc/dcr_gat.hip)

namespace dcr {

constexpr int SPMM_MAX_REL = 8;

// U slots e, e + stride, ... of one row: weight, (TYPED) relation and, per column block, the VEC floats each gathers
template <int VEC, int U, int NBLK, bool TYPED>
struct SlotBatch {
    float w[U];
    int r[TYPED ? U : 1];
    bool ok[U];
    float b[U][NBLK][VEC];
};

// Slot u reads row col[.] of M at column f0 + k·blk (plain: NBLK column blocks `blk` floats apart) or f0 + rel[.]·blk (TYPED;
// blk = n_feat: the gather's typed column block; 0: the expand, which reads plain rows).  MASKED: slots at or past e1 are
// switched off (the last batch of a row).
template <int VEC, int U, int NBLK, bool TYPED, bool MASKED>
__device__ inline void load_batch(const int32_t *__restrict__ col, const float *__restrict__ val, const uint8_t *__restrict__ rel,
                                  const float *__restrict__ M, int64_t ld, int blk, int rmax, int f0, int64_t e, int64_t e1,
                                  int64_t stride, SlotBatch<VEC, U, NBLK, TYPED> &t) {
    int c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t eu = e + u * stride;
        t.ok[u] = !MASKED || eu < e1;
        c[u] = t.ok[u] ? col[eu] : 0;
        if constexpr (TYPED) {
            const int r = t.ok[u] ? (int)rel[eu] : 0;
            t.r[u] = r < rmax ? r : rmax;
        }
        t.w[u] = t.ok[u] ? val[eu] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int k = 0; k < NBLK; ++k) {
            if (t.ok[u]) {
                const float *row = M + (int64_t)c[u] * ld;
                if constexpr (TYPED) load_vec<VEC>(row + (int64_t)t.r[u] * blk + f0, t.b[u][k]);
                else load_vec<VEC>(row + f0 + k * blk, t.b[u][k]);
            } else {
#pragma unroll
                for (int q = 0; q < VEC; ++q) t.b[u][k][q] = 0.f;
            }
        }
    }
}

// Slots e0, e0 + stride, ... < e1 of one row, U at a time with their loads side by side; add(t, u) once per slot, in slot order.
// What is left at the end (fewer than U slots) goes as ONE more batch with the missing slots masked off, and add sees
// t.ok[u] = false for them: it must add nothing.  One slot at a time, each with its index load and its gather behind one another,
// cost two memory latencies per slot, and on a graph of average degree 20 that was most of the plain kernel's time.
// Two column blocks halve U: the same number of gathers in flight.
template <int VEC, int U, int NBLK, bool TYPED, class Add>
__device__ inline void for_slots(const int32_t *__restrict__ col, const float *__restrict__ val, const uint8_t *__restrict__ rel,
                                 const float *__restrict__ M, int64_t ld, int blk, int rmax, int f0, int64_t e0, int64_t e1,
                                 int64_t stride, Add &&add) {
    constexpr int UU = NBLK > 1 ? U / 2 : U;
    SlotBatch<VEC, UU, NBLK, TYPED> t;
    int64_t e = e0;
    for (; e + (UU - 1) * stride < e1; e += UU * stride) {
        load_batch<VEC, UU, NBLK, TYPED, false>(col, val, rel, M, ld, blk, rmax, f0, e, e1, stride, t);
#pragma unroll
        for (int u = 0; u < UU; ++u) add(t, u);
    }
    if (e < e1) {
        load_batch<VEC, UU, NBLK, TYPED, true>(col, val, rel, M, ld, blk, rmax, f0, e, e1, stride, t);
#pragma unroll
        for (int u = 0; u < UU; ++u) add(t, u);
    }
}

// acc[k] += Σ val·M[col, block k ...]: one fmaf per slot and block in slot order, so every block of a two-block call is
// accumulated with exactly the operations, in exactly the order, of a sweep of its own
template <int VEC, int U, int NBLK, bool TYPED>
__device__ inline void accumulate(const int32_t *__restrict__ col, const float *__restrict__ val, const uint8_t *__restrict__ rel,
                                  const float *__restrict__ M, int64_t ld, int blk, int rmax, int f0, int64_t e0, int64_t e1,
                                  int64_t stride, float (&acc)[NBLK][VEC]) {
    for_slots<VEC, U, NBLK, TYPED>(col, val, rel, M, ld, blk, rmax, f0, e0, e1, stride, [&](const auto &t, int u) {
#pragma unroll
        for (int k = 0; k < NBLK; ++k)
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc[k][q] = t.ok[u] ? fmaf(t.w[u], t.b[u][k][q], acc[k][q]) : acc[k][q];
    });
}

// the sum of one row's slots, then the row's own block (own: where it starts, or nullptr), then the bias: one rounding each
template <int VEC>
__device__ inline void finish_row(float *__restrict__ dst, const float (&sum)[VEC], const float *__restrict__ own,
                                  const float *__restrict__ bias, int f0, int relu) {
    float o[VEC];
    if (own) load_vec<VEC>(own, o);
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        float r = sum[q];
        if (own) r += o[q];
        if (bias) r += bias[f0 + q];
        if (relu) r = r > 0.f ? r : 0.f;
        dst[q] = r;
    }
}

// ---- the plain product ---------------------------------------------------------------------------------------------------
// rows: nullptr, or the n_rows rows of the matrix to compute (output row k = row rows[k] of the product); output rows from
// `split` on take their operand b_off2 floats further into B (two row lists over two column blocks in one launch).
// NBLK = 2: B holds two column blocks `blk` floats apart (two operands aggregated in one sweep of the indices, models/gcn.py
// forward_pair), C two blocks blk_c apart.
// This kernel keeps its own walk over the rows, long-row sum and closing steps, written out, and shares the accumulator, the deal
// and the dispatch.  Measured on the 1M-node graph of the benchmark at its class width (<4, 4, 1>, 452 us): through sum_groups it
// takes 70 registers for 74, a seventh wave per SIMD runs, and the kernel, bound by the rate of row requests, is 2 % slower;
// finish_row costs another 1 %; deal_rows brings the 70 registers back by itself.
template <int LPR, int VEC, int NBLK>
__global__ void __launch_bounds__(256) k_spmm_csr(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                   const float *__restrict__ val, const float *__restrict__ B,
                                                   float *__restrict__ C, int64_t n_rows, int n_feat, int64_t ldb,
                                                   int64_t ldc, const float *__restrict__ bias, int relu, int blk, int64_t blk_c,
                                                   const int64_t *__restrict__ rows, int64_t split, int64_t b_off2) {
    using D = Deal<LPR>;
    __shared__ int long_rows[D::G];
    __shared__ int n_long;
    __shared__ float red[256 * VEC];
    const int sub = D::sub(), sl = D::sl();
    const int64_t row = D::row(sub);
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
    if (row < n_rows) {
        const int64_t mrow = rows ? rows[row] : row;
        const float *Bk = row >= split ? B + b_off2 : B;
        const int64_t e0 = rowptr[mrow], e1 = rowptr[mrow + 1];
        if (e1 - e0 > SPMM_LONG) {
            if (sl == 0) long_rows[atomicAdd(&n_long, 1)] = sub;
        } else {
            for (int f0 = sl * VEC; f0 < n_feat; f0 += LPR * VEC) {
                float acc[NBLK][VEC];
#pragma unroll
                for (int k = 0; k < NBLK; ++k)
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[k][q] = 0.f;
                accumulate<VEC, D::U, NBLK, false>(col, val, nullptr, Bk, ldb, blk, 0, f0, e0, e1, 1, acc);
#pragma unroll
                for (int k = 0; k < NBLK; ++k) {
                    float *dst = C + row * ldc + f0 + k * blk_c;
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        float r = acc[k][q];
                        if (bias) r += bias[f0 + q];
                        if (relu) r = r > 0.f ? r : 0.f;
                        dst[q] = r;
                    }
                }
            }
        }
    }
    __syncthreads();
    const int nl = n_long;  // uniform
    for (int li = 0; li < nl; ++li) {
        const int64_t lrow = D::row(long_rows[li]);
        const int64_t lmrow = rows ? rows[lrow] : lrow;
        const float *Bk = lrow >= split ? B + b_off2 : B;
        const int64_t e0 = rowptr[lmrow], e1 = rowptr[lmrow + 1];
        for (int fb = 0; fb < n_feat; fb += LPR * VEC) {  // uniform trip count
            const int f0 = fb + sl * VEC;
            float acc[NBLK][VEC];
#pragma unroll
            for (int k = 0; k < NBLK; ++k)
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[k][q] = 0.f;
            if (f0 < n_feat) accumulate<VEC, D::U, NBLK, false>(col, val, nullptr, Bk, ldb, blk, 0, f0, e0 + sub, e1, D::G, acc);
#pragma unroll
            for (int k = 0; k < NBLK; ++k) {
#pragma unroll
                for (int q = 0; q < VEC; ++q) red[threadIdx.x * VEC + q] = acc[k][q];
                __syncthreads();
                if (sub == 0 && f0 < n_feat) {
                    float *dst = C + lrow * ldc + f0 + k * blk_c;
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        float r = 0.f;
                        for (int g = 0; g < D::G; ++g) r += red[(g * LPR + sl) * VEC + q];   // in group order
                        if (bias) r += bias[f0 + q];
                        if (relu) r = r > 0.f ? r : 0.f;
                        dst[q] = r;
                    }
                }
                __syncthreads();
            }
        }
    }
}

// ---- the typed gather (forward): C[i,:] = Σ_e val[e]·B[col[e], rel[e]·n_feat + :] (+ B[i, n_rel·n_feat + :]) (+ bias) (ReLU) ---
template <int LPR, int VEC>
__global__ void __launch_bounds__(256) k_spmm_typed(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                     const float *__restrict__ val, const uint8_t *__restrict__ rel,
                                                     const float *__restrict__ B, float *__restrict__ C, int64_t n_rows, int n_feat,
                                                     int n_rel, int64_t ldb, int64_t ldc, int self_block,
                                                     const float *__restrict__ bias, int relu) {
    using D = Deal<LPR>;
    __shared__ alignas(16) float red[256 * VEC];   // (sum_groups reads it VEC floats at a time)
    const int sub = D::sub(), sl = D::sl();
    const int rmax = n_rel - 1;
    auto finish = [&](int64_t i, int f0, const float (&sum)[VEC]) {
        finish_row<VEC>(C + i * ldc + f0, sum, self_block ? B + i * ldb + (int64_t)n_rel * n_feat + f0 : nullptr, bias, f0, relu);
    };
    deal_rows<LPR>(
        rowptr, n_rows, [](int64_t i) { return i; },
        [&](int64_t row, int64_t e0, int64_t e1) {
            for (int f0 = sl * VEC; f0 < n_feat; f0 += LPR * VEC) {
                float acc[1][VEC] = {};
                accumulate<VEC, D::U, 1, true>(col, val, rel, B, ldb, n_feat, rmax, f0, e0, e1, 1, acc);
                finish(row, f0, acc[0]);
            }
        },
        [&](int64_t lrow, int64_t e0, int64_t e1) {
            for (int fb = 0; fb < n_feat; fb += LPR * VEC) {  // uniform trip count
                const int f0 = fb + sl * VEC;
                float acc[1][VEC] = {};
                if (f0 < n_feat) accumulate<VEC, D::U, 1, true>(col, val, rel, B, ldb, n_feat, rmax, f0, e0 + sub, e1, D::G, acc);
                sum_groups<LPR, VEC>(red, sub == 0 && f0 < n_feat, acc[0], [&](const float (&sum)[VEC]) { finish(lrow, f0, sum); });
            }
        });
}

// ---- the typed expand (backward, on the CSR of the transposed pattern) ---------------------------------------------------
// C[j, r·n_feat + :] = Σ_{e in row j, rel[e] = r} val[e]·G[col[e], :] for EVERY r (zeros where row j has no slot of r), and
// C[j, n_rel·n_feat + :] = G[j, :] with self_block: every element of C's (n_rel + self_block)·n_feat columns is written.
// The slots of a row are sorted by relation, so a short row needs ONE accumulator, stored and cleared when the relation moves on.
template <int LPR, int VEC>
__global__ void __launch_bounds__(256) k_spmm_typed_expand(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                            const float *__restrict__ val, const uint8_t *__restrict__ rel,
                                                            const float *__restrict__ Gm, float *__restrict__ C, int64_t n_rows,
                                                            int n_feat, int n_rel, int64_t ldg, int64_t ldc, int self_block) {
    using D = Deal<LPR>;
    __shared__ alignas(16) float red[256 * VEC];   // (sum_groups reads it VEC floats at a time)
    __shared__ int64_t seg[SPMM_MAX_REL + 1];   // a hub row's slots of relation r: seg[r] .. seg[r + 1]
    const int sub = D::sub(), sl = D::sl();
    const int rmax = n_rel - 1;
    deal_rows<LPR>(
        rowptr, n_rows, [](int64_t i) { return i; },
        [&](int64_t row, int64_t e0, int64_t e1) {
            for (int f0 = sl * VEC; f0 < n_feat; f0 += LPR * VEC) {
                float *dst = C + row * ldc + f0;
                float acc[VEC] = {};
                int cur = 0;   // the relation acc belongs to; blocks below it are written
                auto flush = [&]() {
                    store_vec<VEC>(dst + (int64_t)cur * n_feat, acc);
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
                    ++cur;
                };
                // a slot of a later relation: store the finished block and the empty ones before the slot's (cur <= rmax always)
                for_slots<VEC, D::U, 1, true>(col, val, rel, Gm, ldg, 0, rmax, f0, e0, e1, 1, [&](const auto &t, int u) {
                    if (!t.ok[u]) return;
                    while (cur < t.r[u]) flush();
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[q] = fmaf(t.w[u], t.b[u][0][q], acc[q]);
                });
                while (cur < n_rel) flush();
                if (self_block) {   // (through acc's registers: a copy of its own cost the VEC 2 kernels on 4 and 8 lanes a wave per SIMD)
                    load_vec<VEC>(Gm + row * ldg + f0, acc);
                    store_vec<VEC>(dst + (int64_t)n_rel * n_feat, acc);
                }
            }
        },
        [&](int64_t lrow, int64_t e0, int64_t e1) {
            // where each relation's slots start: seg[q] = the first slot of relation >= q (e1: none)
            if (threadIdx.x <= n_rel) seg[threadIdx.x] = e1;
            __syncthreads();
            for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
                const int r = min((int)rel[e], rmax);
                const int before = e == e0 ? -1 : min((int)rel[e - 1], rmax);
                for (int q = before + 1; q <= r; ++q) seg[q] = e;
            }
            __syncthreads();
            for (int fb = 0; fb < n_feat; fb += LPR * VEC) {  // uniform trip count
                const int f0 = fb + sl * VEC;
                const bool lead = sub == 0 && f0 < n_feat;
                for (int r = 0; r < n_rel; ++r) {
                    // relation r's slots as a long row of their own: the stride starts at the segment's first slot
                    const int64_t s0 = seg[r], s1 = seg[r + 1];
                    float acc[1][VEC] = {};
                    if (f0 < n_feat) accumulate<VEC, D::U, 1, true>(col, val, rel, Gm, ldg, 0, rmax, f0, s0 + sub, s1, D::G, acc);
                    // (on return red is free again; after the last relation, so is seg)
                    sum_groups<LPR, VEC>(red, lead, acc[0],
                                         [&](const float (&sum)[VEC]) { store_vec<VEC>(C + lrow * ldc + (int64_t)r * n_feat + f0, sum); });
                }
                if (self_block && lead) {
                    float own[VEC];
                    load_vec<VEC>(Gm + lrow * ldg + f0, own);
                    store_vec<VEC>(C + lrow * ldc + (int64_t)n_rel * n_feat + f0, own);
                }
            }
        });
}

}  // namespace dcr

using namespace dcr;

template <int N>
using Int = std::integral_constant<int, N>;

// Whether 16- and 8-byte accesses are possible: the width and both leading dimensions multiples of 4 / 2 floats, every pointer
// in `ptrs` aligned.  Which pointers count is the caller's: an output written with scalar stores does not.
struct VecOk {
    bool v4, v2;
};
static VecOk vec_ok(int F, int64_t ld_in, int64_t ld_out, std::initializer_list<const void *> ptrs) {
    auto ok = [&](int vec) {
        bool all = F % vec == 0 && ld_in % vec == 0 && ld_out % vec == 0;
        for (const void *p : ptrs) all = all && ((uintptr_t)p & (4 * vec - 1)) == 0;
        return all;
    };
    return {ok(4), ok(2)};
}

// The (LPR, VEC) table: the widest VEC allowed, then the first LPR of 4 .. 64 lanes that holds the VEC-wide pieces of one row
// (wider rows take more than one trip of the f0 loop on 64 lanes).  go(Int<LPR>, Int<VEC>) launches the instantiation.
template <class Go>
static void pick_lpr_vec(int F, VecOk v, Go &&go) {
    auto lpr = [&](auto vec) {
        const int pieces = F / decltype(vec)::value;
        if (pieces <= 4) go(Int<4>{}, vec);
        else if (pieces <= 8) go(Int<8>{}, vec);
        else if (pieces <= 16) go(Int<16>{}, vec);
        else if (pieces <= 32) go(Int<32>{}, vec);
        else go(Int<64>{}, vec);
    };
    if (v.v4) lpr(Int<4>{});
    else if (v.v2) lpr(Int<2>{});
    else lpr(Int<1>{});
}

static int spmm_dispatch(const int64_t *rowptr, const int32_t *col, const float *val, const float *B, float *C,
                         int64_t n_rows, int64_t n_feat, int64_t n_blocks, int64_t ldb, int64_t ldc, const float *bias, int relu,
                         void *hip_stream, int64_t blk_c = -1, const int64_t *rows = nullptr, int64_t split = INT64_MAX,
                         int64_t b_off2 = 0) {
    // blk_c: where the second block of the output starts relative to the first (floats); -1: next to it (n_feat)
    if (!rowptr || !B || !C || n_rows < 0 || n_feat <= 0 || n_blocks < 1 || n_blocks > 2 || ldb < n_feat * n_blocks ||
        ldc < (blk_c < 0 ? n_feat * n_blocks : n_feat))
        DCR_FAIL(DCR_EINVAL, "bad SpMM arguments");
    if (blk_c < 0) blk_c = n_feat;
    if (n_rows == 0) return DCR_OK;
    if (n_feat > INT32_MAX / 2) DCR_FAIL(DCR_EINVAL, "n_feat too large");
    hipStream_t st = (hipStream_t)hip_stream;
    const int F = (int)n_feat;
    // (the template is chosen by the width of ONE block: a block of a two-block call is accumulated exactly like a call of its
    //  own.  C does not count: its stores are scalar)
    VecOk v = vec_ok(F, ldb, ldc, {B});
    // (rows from `split` on read B + b_off2: the 8-byte path needs that operand aligned too, and falls back to scalar loads
    //  where it is not; the 16-byte path's second operand is dcr_spmm_csr_rows2_f32_dev's own check)
    v.v2 = v.v2 && (split >= n_rows || b_off2 % 2 == 0);
    pick_lpr_vec(F, v, [&](auto L, auto V) {
        constexpr int LPR = decltype(L)::value, VEC = decltype(V)::value;
        if (n_blocks == 2)
            hipLaunchKernelGGL((k_spmm_csr<LPR, VEC, 2>), Deal<LPR>::grid(n_rows), dim3(256), 0, st, rowptr, col, val, B, C, n_rows, F,
                               ldb, ldc, bias, relu, F, blk_c, rows, split, b_off2);
        else
            hipLaunchKernelGGL((k_spmm_csr<LPR, VEC, 1>), Deal<LPR>::grid(n_rows), dim3(256), 0, st, rowptr, col, val, B, C, n_rows, F,
                               ldb, ldc, bias, relu, 0, (int64_t)0, rows, split, b_off2);
    });
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

extern "C" int dcr_spmm_csr_f32_dev(const int64_t *rowptr, const int32_t *col, const float *val, const float *B,
                                    float *C, int64_t n_rows, int64_t n_feat, int64_t ldb, int64_t ldc,
                                    const float *bias, int relu, void *hip_stream) {
    return spmm_dispatch(rowptr, col, val, B, C, n_rows, n_feat, 1, ldb, ldc, bias, relu, hip_stream);
}

extern "C" int dcr_spmm_csr_f32_pair_dev(const int64_t *rowptr, const int32_t *col, const float *val, const float *B,
                                         float *C, int64_t n_rows, int64_t n_feat, int64_t ldb, int64_t ldc,
                                         const float *bias, int relu, void *hip_stream) {
    return spmm_dispatch(rowptr, col, val, B, C, n_rows, n_feat, 2, ldb, ldc, bias, relu, hip_stream);
}

extern "C" int dcr_spmm_csr_f32_pair_split_dev(const int64_t *rowptr, const int32_t *col, const float *val, const float *B,
                                               float *C0, float *C1, int64_t n_rows, int64_t n_feat, int64_t ldb, int64_t ldc,
                                               const float *bias, int relu, void *hip_stream) {
    if (!C0 || !C1 || ((C1 - C0) % 4) != 0) DCR_FAIL(DCR_EINVAL, "bad SpMM arguments (the two outputs 16 bytes apart modulo 16)");
    return spmm_dispatch(rowptr, col, val, B, C0, n_rows, n_feat, 2, ldb, ldc, bias, relu, hip_stream, (int64_t)(C1 - C0));
}

// Rows rows_dev[0..n_sel) of Â·B (+ bias) only, output row k = row rows_dev[k]: the last layer of a training epoch is read at
// the training rows (loss) and the validation rows (accuracy) and nowhere else (experiment/training_loop.py:50-51,64-71 index
// the model's output with the split masks).  Every computed row is accumulated exactly as dcr_spmm_csr_f32_dev does it.
extern "C" int dcr_spmm_csr_rows_f32_dev(const int64_t *rowptr, const int32_t *col, const float *val, const int64_t *rows,
                                         int64_t n_sel, const float *B, float *C, int64_t n_feat, int64_t ldb, int64_t ldc,
                                         const float *bias, int relu, void *hip_stream) {
    if (!rows && n_sel > 0) DCR_FAIL(DCR_EINVAL, "bad SpMM arguments (no row list)");
    return spmm_dispatch(rowptr, col, val, B, C, n_sel, n_feat, 1, ldb, ldc, bias, relu, hip_stream, -1, rows);
}

// Two row lists over two column blocks of one operand in ONE launch: output rows [0, n_first) are rows rows_dev[k] of Â·B0,
// rows [n_first, n_sel) those of Â·B1 with B1 = B0 + b_off2 floats (the training rows of Â·Z_train and the validation rows of
// Â·Z_eval of an epoch, Z = [Z_train | Z_eval]).  Each row as dcr_spmm_csr_rows_f32_dev computes it; where B1 is only 4-byte
// aligned and B0 would take 8-byte loads, BOTH lists are computed as that call computes B1's (scalar loads).
extern "C" int dcr_spmm_csr_rows2_f32_dev(const int64_t *rowptr, const int32_t *col, const float *val, const int64_t *rows,
                                          int64_t n_first, int64_t n_sel, const float *B, int64_t b_off2, float *C, int64_t n_feat,
                                          int64_t ldb, int64_t ldc, const float *bias, int relu, void *hip_stream) {
    if ((!rows && n_sel > 0) || n_first < 0 || n_first > n_sel || b_off2 < 0 || b_off2 + n_feat > ldb)
        DCR_FAIL(DCR_EINVAL, "bad SpMM arguments (row lists)");
    // (the 16-byte path needs both operands aligned: decided on B0, so B1 must keep its alignment)
    if ((b_off2 % 4) != 0 && (n_feat % 4) == 0) DCR_FAIL(DCR_EINVAL, "bad SpMM arguments (second operand not 16 bytes apart)");
    return spmm_dispatch(rowptr, col, val, B, C, n_sel, n_feat, 1, ldb, ldc, bias, relu, hip_stream, -1, rows, n_first, b_off2);
}

// the argument checks of a typed call: `wide` is the operand with (n_rel + self_block) column blocks
static int typed_check(const void *rowptr, const void *col, const void *val, const void *rel, const void *in, const void *out,
                       int64_t n_rows, int64_t n_feat, int64_t n_rel, int64_t ld_narrow, int64_t ld_wide, int self_block) {
    if (!rowptr || !col || !val || !rel || !in || !out || n_rows < 0 || n_feat <= 0 || n_rel < 1 || n_rel > SPMM_MAX_REL ||
        (self_block != 0 && self_block != 1))
        DCR_FAIL(DCR_EINVAL, "bad typed SpMM arguments");
    if (n_feat > INT32_MAX / 2 / (SPMM_MAX_REL + 1)) DCR_FAIL(DCR_EINVAL, "n_feat too large");
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
    // (the plain product's choice, so that n_rel = 1 is that product bit for bit: C's stores are scalar here too)
    pick_lpr_vec(F, vec_ok(F, ldb, ldc, {B}), [&](auto L, auto V) {
        constexpr int LPR = decltype(L)::value, VEC = decltype(V)::value;
        hipLaunchKernelGGL((k_spmm_typed<LPR, VEC>), Deal<LPR>::grid(n_rows), dim3(256), 0, st, rowptr, col, val, rel, B, C, n_rows, F,
                           (int)n_rel, ldb, ldc, self_block, bias, relu);
    });
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
    // (vector stores: the column blocks of C start n_feat apart, so with n_feat and ldc multiples of VEC every one is aligned
    //  when C is)
    pick_lpr_vec(F, vec_ok(F, ldg, ldc, {G, C}), [&](auto L, auto V) {
        constexpr int LPR = decltype(L)::value, VEC = decltype(V)::value;
        hipLaunchKernelGGL((k_spmm_typed_expand<LPR, VEC>), Deal<LPR>::grid(n_rows), dim3(256), 0, st, rowptr, col, val, rel, G, C,
                           n_rows, F, (int)n_rel, ldg, ldc, self_block);
    });
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}
