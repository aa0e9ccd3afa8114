// The device-side pieces every gather over a CSR is built from (csrc/dcr_spmm.hip: the plain and typed aggregation;
// csrc/dcr_gat.hip: the attention aggregation): the deal of lanes to rows, the 16- / 8- / 4-byte accesses, the walk of a
// workgroup over its rows with the parking of long ones, and the group-order sum of a long row's partial sums.
#pragma once
#include <cstdint>
#include "dcr_internal.h"

namespace dcr {

// Rows up to SPMM_LONG slots: one LPR-lane group per row, slots in order.  Longer rows (the hubs of a power-law graph:
// thousands of slots, which one group would chew through long after the rest of the grid has finished) are parked in LDS and
// then taken by the whole workgroup: group g accumulates slots g, g + G, ... and the partial sums are added in group order, so
// the result is deterministic.
constexpr int SPMM_LONG = 96;

// how the 256 lanes of a workgroup are dealt to rows
template <int LPR>
struct Deal {
    static constexpr int G = 256 / LPR;          // lane groups per workgroup = rows per workgroup
    static constexpr int U = LPR <= 8 ? 8 : 4;   // gathers in flight per group; narrow operand rows: more
    __device__ static int sub() { return threadIdx.x / LPR; }   // which row of the workgroup / which group
    __device__ static int sl() { return threadIdx.x % LPR; }    // lane inside the group
    // group `sub` of workgroup b owns row sub * gridDim + b: consecutive (hub) rows land in different workgroups
    __device__ static int64_t row(int sub) { return (int64_t)sub * gridDim.x + blockIdx.x; }
    static dim3 grid(int64_t n_rows) { return dim3((unsigned)((n_rows + G - 1) / G)); }
};

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

// The walk of a workgroup over its rows.  row_of(i): the row of the matrix behind output row i.  short_row(i, e0, e1) runs in
// the row's own group; long_row(i, e0, e1) afterwards in the WHOLE workgroup, once per parked row (it may use barriers).
template <int LPR, class RowOf, class Short, class Long>
__device__ inline void deal_rows(const int64_t *__restrict__ rowptr, int64_t n_rows, RowOf &&row_of, Short &&short_row,
                                 Long &&long_row) {
    using D = Deal<LPR>;
    __shared__ int long_rows[D::G];
    __shared__ int n_long;
    const int sub = D::sub();
    const int64_t row = D::row(sub);
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
    if (row < n_rows) {
        const int64_t mrow = row_of(row);
        const int64_t e0 = rowptr[mrow], e1 = rowptr[mrow + 1];
        if (e1 - e0 > SPMM_LONG) {
            if (D::sl() == 0) long_rows[atomicAdd(&n_long, 1)] = sub;
        } else {
            short_row(row, e0, e1);
        }
    }
    __syncthreads();
    const int nl = n_long;  // uniform
    for (int li = 0; li < nl; ++li) {
        const int64_t lrow = D::row(long_rows[li]);
        const int64_t mrow = row_of(lrow);
        long_row(lrow, rowptr[mrow], rowptr[mrow + 1]);
    }
}

// A long row's partial sums (one per group in `part`, lanes of equal sl hold the same features) added in group order onto 0.f by
// group 0, whose lanes with lead = true then call done(sum).  Called by the whole workgroup; red is free again on return.
template <int LPR, int VEC, class Done>
__device__ inline void sum_groups(float *__restrict__ red, bool lead, const float (&part)[VEC], Done &&done) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) red[threadIdx.x * VEC + q] = part[q];
    __syncthreads();
    if (lead) {
        float sum[VEC] = {};
        // (a few groups at a time: all G reads in flight at once took 4·G registers at VEC 4, and set the kernel's occupancy)
#pragma unroll 4
        for (int g = 0; g < Deal<LPR>::G; ++g) {
            float p[VEC];
            load_vec<VEC>(red + (g * LPR + Deal<LPR>::sl()) * VEC, p);
#pragma unroll
            for (int q = 0; q < VEC; ++q) sum[q] += p[q];
        }
        done(sum);
    }
    __syncthreads();
}

}  // namespace dcr
