// Attention aggregation of libdcr_hip.so on CSR, fp32: the GAT layer of Veličković et al. as torch_geometric's GATConv evaluates
// it (models/gat.py), on the pieces of csrc/dcr_spmm_pieces.h.  H heads, C channels per head, flow source -> target.
//
//   k_gat_gather    forward, ONE sweep of the CSR by target: per (row, head) the softmax over the row's slots of
//                   e = leaky(s_src[col] + s_dst[row]) fused into the gather of Z[col, head, :]; writes O and the record (m, den).
//   k_gat_rowdot    backward, row-local: D[i,h] = <dO[i,h,:], O[i,h,:]> (= Σ_j α_ij·dα_ij, so no second softmax pass), packed with
//                   what a slot of the expand needs of its target into one 16-byte record (s_dst, m, den, D).
//   k_gat_expand    backward, ONE sweep of the CSR of the transposed pattern: row j keeps Z[j] in registers, gathers dO[i] and i's
//                   record per slot, writes dZ[j], dS_src[j] and g at the slot's position in the target CSR.
//   k_gat_dst_sum   backward, the closing sum: dS_dst[i,h] = Σ g over the slots of target row i.
//
// A unit is a (row, head) pair, taken by a group of LPH lanes that covers the head's C channels VEC at a time (C / VEC <= LPH: one
// trip).  Units are dealt so that the heads of one row sit in neighbouring lane groups of one wave: their gathers are neighbouring
// pieces of one operand row.
//
// The order of every sum is fixed.  A unit of at most GAT_LONG slots: den and every acc element one operation per slot in slot
// order from 0.f.  A longer one is parked and taken by the whole workgroup: group g takes slots g, g + G, ... in order, the G
// partial sums are added in group order onto 0.f (sum_groups).  The maximum is order-free.  Dots over a head's channels: each
// lane fmaf's its VEC products in channel order from 0.f, then a butterfly over the LPH lanes (xor 1, 2, 4, ...), which gives
// every lane the same bits.  No atomics on floats, no scratch: the same bits on every call.
//
// expf is the library's (not a fast-math variant), every multiply-add an explicit fmaf (the file is built -ffp-contract=off), the
// closing acc / den and the backward's w / den are true divisions.
//
// Attention dropout (the DROP = true instantiations; DROP = false is the code above and never reads GatDrop): the keep weight
// k in {0, scale} of slot `pos` of the target CSR under head h multiplies alpha AFTER the softmax, so m and den run over every
// slot and D = <dO, O> stays as it is.  No mask is stored: the decision is element E = h * S8 + pos (S8 = nnz rounded up to 8)
// of the dropout stream of include/dcr.h, and both sweeps draw it again.  One Philox call holds the 8 slots pos & ~7 .. of one
// head: the forward's slot-order sweep draws once per 8 slots (KeepDraw), the expand, which meets positions in the order of
// the transposed pattern, once per slot.  The stream offset o = offset + *offset_dev is resolved by the gather, which leaves
// it in a device word for the expand: a replayed graph whose counter moved on between the two still redraws the same mask.
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <type_traits>
#include "dcr_internal.h"
#include "dcr_philox.h"
#include "dcr_spmm_pieces.h"

namespace dcr {

// units above GAT_LONG slots are parked (deal_rows parks by SPMM_LONG: one threshold for every gather of the library)
constexpr int GAT_LONG = 96;
static_assert(GAT_LONG == SPMM_LONG, "deal_rows parks rows by SPMM_LONG");
constexpr int GAT_MAX_HEADS = 64;

__device__ inline float leaky(float pre, float slope) { return pre > 0.f ? pre : slope * pre; }

// what the DROP = true kernels read (a DROP = false kernel is passed one and touches none of it)
struct GatDrop {
    uint64_t seed = 0, offset = 0;
    const int64_t *offset_dev = nullptr;   // gather: the caller's call counter, may be null; expand: the word the gather wrote
    int64_t *offset_used = nullptr;        // gather: receives o = offset + *offset_dev
    int64_t s8 = 0;                        // nnz rounded up to a multiple of 8: the stream's elements per head
    uint32_t threshold = 0;                // kept: 16-bit draw >= threshold
    float scale = 1.f;                     // (float)(1 / (1 - p))
};

// The keep decision of element E = h * s8 + pos: call E >> 3, word E & 3, half (E >> 2) & 1 (philox_quad16's rule).  The four
// words of the last call stay in registers (named, not indexed: no scratch), so a sweep in slot order draws once per 8 slots.
struct KeepDraw {
    uint64_t call = ~(uint64_t)0;   // (no element reaches call 2^64 - 1)
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
    __device__ bool keep(uint64_t E, uint64_t o, uint64_t seed, uint32_t threshold) {
        if ((E >> 3) != call) {
            call = E >> 3;
            uint32_t r[4];
            philox4x32_10(call, o, seed, r);
            r0 = r[0]; r1 = r[1]; r2 = r[2]; r3 = r[3];
        }
        const uint32_t lo = (E & 1) ? r1 : r0, hi = (E & 1) ? r3 : r2;
        const uint32_t word = (E & 2) ? hi : lo;
        return ((word >> ((uint32_t)((E >> 2) & 1) * 16u)) & 0xFFFFu) >= threshold;
    }
};

// deal_rows numbers the group `sub` of workgroup b as i = sub * gridDim + b (Deal::row).  Here the unit of that group is
// b * G + sub: the heads of one row (units row * H .. row * H + H - 1) sit in neighbouring groups of one workgroup.
template <int LPH>
__device__ inline int64_t unit_of(int64_t i) {
    return (i % gridDim.x) * Deal<LPH>::G + i / gridDim.x;
}

// Slots e0, e0 + stride, ... < e1, U at a time: load(u, e, ok) for the U slots of a batch first (their gathers side by side), then
// use(u) once per slot in slot order.  What is left at the end goes as one more batch with the missing slots' ok = false: use must
// add nothing for them.
template <int U, class Load, class Use>
__device__ inline void slot_batches(int64_t e0, int64_t e1, int64_t stride, Load &&load, Use &&use) {
    int64_t e = e0;
    for (; e + (U - 1) * stride < e1; e += U * stride) {
#pragma unroll
        for (int u = 0; u < U; ++u) load(u, e + u * stride, true);
#pragma unroll
        for (int u = 0; u < U; ++u) use(u);
    }
    if (e < e1) {
#pragma unroll
        for (int u = 0; u < U; ++u) load(u, e + u * stride, e + u * stride < e1);
#pragma unroll
        for (int u = 0; u < U; ++u) use(u);
    }
}

// the sum over the LPH lanes of a group, neighbours first; every lane gets the same bits (each step adds the same two values)
template <int LPH>
__device__ inline float group_sum(float p) {
#pragma unroll
    for (int k = 1; k < LPH; k <<= 1) p += __shfl_xor(p, k, LPH);
    return p;
}

// ---- forward --------------------------------------------------------------------------------------------------------------
// O[i, h·C + :] = Σ_slots w·Z[col, h·C + :] / den, w = expf(e − m), e = leaky(s_src[col, h] + s_dst[i, h]), m = max e, den = Σ w.
// rec[(i·H + h)·2 ..] = (m, den); a row without slots: O = 0, rec = (0, 1).
// DROP: O = (Σ_kept slots w·Z / den)·scale — den over every slot, the numerator's fmaf for kept slots only, in slot order from
// 0.f, a true division, then one multiply; rec as without.
template <int LPH, int VEC, bool DROP>
__global__ void __launch_bounds__(256) k_gat_gather(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                     const float *__restrict__ Z, const float *__restrict__ s_src,
                                                     const float *__restrict__ s_dst, float *__restrict__ O, float *__restrict__ rec,
                                                     int64_t n, int H, int C, int64_t ldz, int64_t lds, int64_t ldo, float slope,
                                                     GatDrop drop) {
    using D = Deal<LPH>;
    __shared__ alignas(16) float red[256 * VEC];   // (sum_groups reads it VEC floats at a time)
    __shared__ float wave_max[4];
    const int sub = D::sub(), sl = D::sl();
    const int f0 = sl * VEC;
    const bool mine = f0 < C;   // (C / VEC <= LPH: the lanes past the head's last piece only help with the scores)
    const int64_t n_units = n * H;
    uint64_t o = 0;
    if constexpr (DROP) {
        o = drop.offset + (drop.offset_dev ? (uint64_t)*drop.offset_dev : 0);
        if (blockIdx.x == 0 && threadIdx.x == 0) *drop.offset_used = (int64_t)o;
    }
    // sub-sweep 2 of one unit over slots e0, e0 + stride, ...: den and acc in slot order
    auto sweep2 = [&](const float *zh, const float *ss, float sd, float m, int64_t e0, int64_t e1, int64_t stride, float &den,
                      float (&acc)[VEC], uint64_t head0) {   // (head0 = h * s8: element 0 of the head's stream; DROP only)
        float s[D::U], b[D::U][VEC];
        bool ok[D::U];
        int64_t at[D::U];
        KeepDraw draw;
        slot_batches<D::U>(
            e0, e1, stride,
            [&](int u, int64_t e, bool on) {
                ok[u] = on;
                if constexpr (DROP) at[u] = e;
                const int64_t c = on ? col[e] : 0;
                s[u] = on ? ss[c * lds] : 0.f;
                if (on && mine) {
                    load_vec<VEC>(zh + c * ldz, b[u]);
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) b[u][q] = 0.f;
                }
            },
            [&](int u) {
                if (!ok[u]) return;
                const float w = expf(leaky(s[u] + sd, slope) - m);
                den += w;
                if constexpr (DROP) {
                    if (!draw.keep(head0 + (uint64_t)at[u], o, drop.seed, drop.threshold)) return;
                }
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[q] = fmaf(w, b[u][q], acc[q]);
            });
    };
    auto close = [&](int64_t unit, float *dst, const float (&acc)[VEC], float m, float den, bool any) {
        if (mine) {
            float v[VEC];
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                v[q] = any ? acc[q] / den : 0.f;
                if constexpr (DROP) v[q] *= drop.scale;
            }
            store_vec<VEC>(dst, v);
        }
        if (sl == 0) {
            rec[unit * 2] = any ? m : 0.f;
            rec[unit * 2 + 1] = any ? den : 1.f;
        }
    };
    deal_rows<LPH>(
        rowptr, (int64_t)D::G * gridDim.x,
        [&](int64_t i) {   // (a group past the last unit reads the last row's extent and then does nothing)
            const int64_t unit = unit_of<LPH>(i);
            return unit < n_units ? unit / H : n - 1;
        },
        [&](int64_t i, int64_t e0, int64_t e1) {
            const int64_t unit = unit_of<LPH>(i);
            if (unit >= n_units) return;
            const int64_t row = unit / H;
            const int h = (int)(unit % H);
            const float sd = s_dst[row * lds + h];
            const float *ss = s_src + h;
            // sub-sweep 1: the lanes of the group share the slots, the maximum is joined across them
            float m = -INFINITY;
#pragma unroll 4
            for (int64_t e = e0 + sl; e < e1; e += LPH) m = fmaxf(m, leaky(ss[(int64_t)col[e] * lds] + sd, slope));
#pragma unroll
            for (int k = 1; k < LPH; k <<= 1) m = fmaxf(m, __shfl_xor(m, k, LPH));
            float den = 0.f, acc[VEC] = {};
            sweep2(Z + (int64_t)h * C + f0, ss, sd, m, e0, e1, 1, den, acc, (uint64_t)h * (uint64_t)drop.s8);
            close(unit, O + row * ldo + (int64_t)h * C + f0, acc, m, den, e1 > e0);
        },
        [&](int64_t i, int64_t e0, int64_t e1) {
            const int64_t unit = unit_of<LPH>(i);
            if (unit >= n_units) return;   // uniform
            const int64_t row = unit / H;
            const int h = (int)(unit % H);
            const float sd = s_dst[row * lds + h];
            const float *ss = s_src + h;
            float m = -INFINITY;
            for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) m = fmaxf(m, leaky(ss[(int64_t)col[e] * lds] + sd, slope));
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) m = fmaxf(m, __shfl_xor(m, k, 64));
            if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
            __syncthreads();   // (wave_max is free again after the barriers of sum_groups below)
            m = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
            float den_p[1] = {0.f}, acc[VEC] = {};
            sweep2(Z + (int64_t)h * C + f0, ss, sd, m, e0 + sub, e1, D::G, den_p[0], acc, (uint64_t)h * (uint64_t)drop.s8);
            float den = 1.f;
            sum_groups<LPH, 1>(red, sub == 0, den_p, [&](const float (&sum)[1]) { den = sum[0]; });
            sum_groups<LPH, VEC>(red, sub == 0, acc,
                                 [&](const float (&sum)[VEC]) { close(unit, O + row * ldo + (int64_t)h * C + f0, sum, m, den, true); });
        });
}

// ---- backward -------------------------------------------------------------------------------------------------------------
// rec4[i·H + h] = (s_dst[i,h], m, den, D[i,h]), D = <dO[i,h,:], O[i,h,:]>
template <int LPH, int VEC>
__global__ void __launch_bounds__(256) k_gat_rowdot(const float *__restrict__ O, const float *__restrict__ dO,
                                                     const float *__restrict__ s_dst, const float *__restrict__ rec,
                                                     float4 *__restrict__ rec4, int64_t n, int H, int C, int64_t lds, int64_t ldo) {
    using D = Deal<LPH>;
    const int sl = D::sl();
    const int f0 = sl * VEC;
    const int64_t unit = (int64_t)blockIdx.x * D::G + D::sub();
    if (unit >= n * H) return;   // (whole groups leave: the butterfly below stays inside one group)
    const int64_t row = unit / H;
    const int h = (int)(unit % H);
    float p = 0.f;
    if (f0 < C) {
        float o[VEC], g[VEC];
        load_vec<VEC>(O + row * ldo + (int64_t)h * C + f0, o);
        load_vec<VEC>(dO + row * ldo + (int64_t)h * C + f0, g);
#pragma unroll
        for (int q = 0; q < VEC; ++q) p = fmaf(g[q], o[q], p);
    }
    p = group_sum<LPH>(p);
    if (sl == 0) rec4[unit] = make_float4(s_dst[row * lds + h], rec[unit * 2], rec[unit * 2 + 1], p);
}

// Row j of the transposed pattern, head h; per slot (target i = col_t, position pos = slot_t in the target CSR):
//   pre = s_src[j,h] + s_dst[i,h]; α = expf(leaky(pre) − m_i) / den_i; t = <dO[i,h,:], Z[j,h,:]>
//   g = α·(t − D_i)·(pre > 0 ? 1 : slope) -> gbuf[pos·H + h];  dZ[j,h,:] = Σ fmaf(α, dO[i,h,:], ·);  dS_src[j,h] = Σ g
// DROP: k = scale or 0 from (pos, h), drawn once per slot:  g = α·(k·t − D)·(pre > 0 ? 1 : slope);  dZ = Σ_kept fmaf(α·k, dO, ·)
template <int LPH, int VEC, bool DROP>
__global__ void __launch_bounds__(256) k_gat_expand(const int64_t *__restrict__ rowptr_t, const int32_t *__restrict__ col_t,
                                                     const int64_t *__restrict__ slot_t, const float *__restrict__ Z,
                                                     const float *__restrict__ s_src, const float *__restrict__ dO,
                                                     const float4 *__restrict__ rec4, float *__restrict__ dZ,
                                                     float *__restrict__ dS_src, float *__restrict__ gbuf, int64_t n, int H, int C,
                                                     int64_t ldz, int64_t lds, int64_t ldo, float slope, GatDrop drop) {
    using D = Deal<LPH>;
    __shared__ alignas(16) float red[256 * VEC];   // (sum_groups reads it VEC floats at a time)
    const int sub = D::sub(), sl = D::sl();
    const int f0 = sl * VEC;
    const bool mine = f0 < C;
    const int64_t n_units = n * H;
    uint64_t o = 0;
    if constexpr (DROP) o = (uint64_t)*drop.offset_dev;
    auto sweep = [&](int h, const float (&z)[VEC], float ssj, int64_t e0, int64_t e1, int64_t stride, float &gs, float (&acc)[VEC]) {
        float4 r[D::U];
        float d[D::U][VEC];
        int64_t pos[D::U];
        bool ok[D::U];
        const float *dh = dO + (int64_t)h * C + f0;
        slot_batches<D::U>(
            e0, e1, stride,
            [&](int u, int64_t e, bool on) {
                ok[u] = on;
                const int64_t i = on ? col_t[e] : 0;
                pos[u] = on ? slot_t[e] : 0;
                r[u] = on ? rec4[i * H + h] : make_float4(0.f, 0.f, 1.f, 0.f);
                if (on && mine) {
                    load_vec<VEC>(dh + i * ldo, d[u]);
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) d[u][q] = 0.f;
                }
            },
            [&](int u) {
                float t = 0.f;
#pragma unroll
                for (int q = 0; q < VEC; ++q) t = fmaf(d[u][q], z[q], t);
                t = group_sum<LPH>(t);   // (ok[u] is the same in the whole group)
                if (!ok[u]) return;
                const float pre = ssj + r[u].x;
                const float a = expf(leaky(pre, slope) - r[u].y) / r[u].z;
                float g;
                if constexpr (DROP) {
                    KeepDraw draw;
                    const bool kept = draw.keep((uint64_t)h * (uint64_t)drop.s8 + (uint64_t)pos[u], o, drop.seed, drop.threshold);
                    g = a * ((kept ? drop.scale * t : 0.f) - r[u].w) * (pre > 0.f ? 1.f : slope);
                    if (kept) {
                        const float ak = a * drop.scale;
#pragma unroll
                        for (int q = 0; q < VEC; ++q) acc[q] = fmaf(ak, d[u][q], acc[q]);
                    }
                } else {
                    g = a * (t - r[u].w) * (pre > 0.f ? 1.f : slope);
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[q] = fmaf(a, d[u][q], acc[q]);
                }
                gs += g;
                if (sl == 0) gbuf[pos[u] * H + h] = g;
            });
    };
    deal_rows<LPH>(
        rowptr_t, (int64_t)D::G * gridDim.x,
        [&](int64_t i) {
            const int64_t unit = unit_of<LPH>(i);
            return unit < n_units ? unit / H : n - 1;
        },
        [&](int64_t i, int64_t e0, int64_t e1) {
            const int64_t unit = unit_of<LPH>(i);
            if (unit >= n_units) return;
            const int64_t row = unit / H;
            const int h = (int)(unit % H);
            float z[VEC] = {}, acc[VEC] = {}, gs = 0.f;
            if (mine) load_vec<VEC>(Z + row * ldz + (int64_t)h * C + f0, z);
            sweep(h, z, s_src[row * lds + h], e0, e1, 1, gs, acc);
            if (mine) store_vec<VEC>(dZ + row * ldz + (int64_t)h * C + f0, acc);
            if (sl == 0) dS_src[row * lds + h] = gs;
        },
        [&](int64_t i, int64_t e0, int64_t e1) {
            const int64_t unit = unit_of<LPH>(i);
            if (unit >= n_units) return;   // uniform
            const int64_t row = unit / H;
            const int h = (int)(unit % H);
            float z[VEC] = {}, acc[VEC] = {}, gs_p[1] = {0.f};
            if (mine) load_vec<VEC>(Z + row * ldz + (int64_t)h * C + f0, z);
            sweep(h, z, s_src[row * lds + h], e0 + sub, e1, D::G, gs_p[0], acc);
            sum_groups<LPH, 1>(red, sub == 0 && sl == 0, gs_p, [&](const float (&sum)[1]) { dS_src[row * lds + h] = sum[0]; });
            sum_groups<LPH, VEC>(red, sub == 0 && mine, acc,
                                 [&](const float (&sum)[VEC]) { store_vec<VEC>(dZ + row * ldz + (int64_t)h * C + f0, sum); });
        });
}

// dS_dst[i, h] = Σ gbuf[e·H + h] over the slots e of target row i, in slot order; a group of 4 lanes per row, lane sl the heads
// sl, sl + 4, ...; a row above GAT_LONG slots in the strided order of every long row here.
constexpr int DST_LPR = 4;
__global__ void __launch_bounds__(256) k_gat_dst_sum(const int64_t *__restrict__ rowptr, const float *__restrict__ gbuf,
                                                      float *__restrict__ dS_dst, int64_t n, int H, int64_t lds) {
    using D = Deal<DST_LPR>;
    __shared__ alignas(16) float red[256];
    const int sub = D::sub(), sl = D::sl();
    deal_rows<DST_LPR>(
        rowptr, n, [](int64_t i) { return i; },
        [&](int64_t row, int64_t e0, int64_t e1) {
            for (int h = sl; h < H; h += DST_LPR) {
                float s = 0.f;
#pragma unroll 4
                for (int64_t e = e0; e < e1; ++e) s += gbuf[e * H + h];
                dS_dst[row * lds + h] = s;
            }
        },
        [&](int64_t row, int64_t e0, int64_t e1) {
            for (int hb = 0; hb < H; hb += DST_LPR) {   // uniform trip count
                const int h = hb + sl;
                float s[1] = {0.f};
                if (h < H)
                    for (int64_t e = e0 + sub; e < e1; e += D::G) s[0] += gbuf[e * H + h];
                sum_groups<DST_LPR, 1>(red, sub == 0 && h < H, s, [&](const float (&sum)[1]) { dS_dst[row * lds + h] = sum[0]; });
            }
        });
}

}  // namespace dcr

using namespace dcr;

template <int N>
using Int = std::integral_constant<int, N>;

// The widest VEC in {4, 2, 1} that C, every leading dimension and every pointer allow (a head starts h·C floats into its row, so
// C % VEC == 0 keeps every head aligned and no lane straddles two), then the first LPH of 4 .. 64 lanes that holds the head's
// C / VEC pieces.  false: more than 64 pieces.
template <class Go>
static bool pick_lph_vec(int C, std::initializer_list<int64_t> lds, std::initializer_list<const void *> ptrs, Go &&go) {
    auto ok = [&](int vec) {
        bool all = C % vec == 0;
        for (int64_t ld : lds) all = all && ld % vec == 0;
        for (const void *p : ptrs) all = all && ((uintptr_t)p & (4 * vec - 1)) == 0;
        return all;
    };
    auto lph = [&](auto vec) {
        const int pieces = C / decltype(vec)::value;
        if (pieces <= 4) go(Int<4>{}, vec);
        else if (pieces <= 8) go(Int<8>{}, vec);
        else if (pieces <= 16) go(Int<16>{}, vec);
        else if (pieces <= 32) go(Int<32>{}, vec);
        else if (pieces <= 64) go(Int<64>{}, vec);
        else return false;
        return true;
    };
    if (ok(4)) return lph(Int<4>{});
    if (ok(2)) return lph(Int<2>{});
    return lph(Int<1>{});
}

static int gat_check(int64_t n, int64_t H, int64_t C, int64_t ldz, int64_t lds, int64_t ldo) {
    if (n < 0 || H < 1 || H > GAT_MAX_HEADS || C < 1) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (n >= 0, 1 <= H <= 64, C >= 1)");
    if (C > 256) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (C above 256)");
    if (ldz < H * C || ldo < H * C || lds < H) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (leading dimension)");
    if (n > (INT32_MAX - 1) / H) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (n * H above 2^31 - 2)");
    return DCR_OK;
}

// p, nnz and the output word of the DROP = true entry points -> GatDrop (threshold and scale as every dropout kernel forms them)
static int gat_drop_args(int64_t nnz, double p, uint64_t seed, uint64_t offset, const int64_t *offset_dev, int64_t *offset_used,
                         GatDrop &drop) {
    if (!(p >= 0.0 && p < 1.0)) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (attention dropout p outside [0, 1))");
    if (nnz < 0) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (nnz < 0)");
    drop.seed = seed;
    drop.offset = offset;
    drop.offset_dev = offset_dev;
    drop.offset_used = offset_used;
    drop.s8 = (nnz + 7) / 8 * 8;
    drop.threshold = dropout_threshold16(p);
    drop.scale = (float)(1.0 / (1.0 - p));
    return DCR_OK;
}

template <bool DROP>
static int gat_gather(const int64_t *rowptr, const int32_t *col, const float *Z, const float *s_src, const float *s_dst, float *O,
                      float *rec, int64_t n, int64_t H, int64_t C, int64_t ldz, int64_t lds, int64_t ldo, double negative_slope,
                      void *hip_stream, const GatDrop &drop) {
    if (!rowptr || !col || !Z || !s_src || !s_dst || !O || !rec) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (null pointer)");
    DCR_TRY(gat_check(n, H, C, ldz, lds, ldo));
    if (n == 0) return DCR_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const bool fits = pick_lph_vec((int)C, {ldz, ldo}, {Z, O}, [&](auto L, auto V) {
        constexpr int LPH = decltype(L)::value, VEC = decltype(V)::value;
        hipLaunchKernelGGL((k_gat_gather<LPH, VEC, DROP>), Deal<LPH>::grid(n * H), dim3(256), 0, st, rowptr, col, Z, s_src, s_dst, O,
                           rec, n, (int)H, (int)C, ldz, lds, ldo, (float)negative_slope, drop);
    });
    if (!fits) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (C above 64 lanes of the widest access the operands allow)");
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

template <bool DROP>
static int gat_expand(const int64_t *rowptr, const int64_t *rowptr_t, const int32_t *col_t, const int64_t *slot_t, const float *Z,
                      const float *s_src, const float *s_dst, const float *O, const float *dO, const float *rec, float *dZ,
                      float *dS_src, float *dS_dst, float *work_rec, float *work_g, int64_t n, int64_t H, int64_t C, int64_t ldz,
                      int64_t lds, int64_t ldo, double negative_slope, void *hip_stream, const GatDrop &drop) {
    if (!rowptr || !rowptr_t || !col_t || !slot_t || !Z || !s_src || !s_dst || !O || !dO || !rec || !dZ || !dS_src || !dS_dst ||
        !work_rec || !work_g)
        DCR_FAIL(DCR_EINVAL, "bad GAT arguments (null pointer)");
    DCR_TRY(gat_check(n, H, C, ldz, lds, ldo));
    if (((uintptr_t)work_rec & 15) != 0) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (work_rec not 16-byte aligned)");
    if (n == 0) return DCR_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const bool fits = pick_lph_vec((int)C, {ldz, ldo}, {Z, O, dO, dZ}, [&](auto L, auto V) {
        constexpr int LPH = decltype(L)::value, VEC = decltype(V)::value;
        hipLaunchKernelGGL((k_gat_rowdot<LPH, VEC>), Deal<LPH>::grid(n * H), dim3(256), 0, st, O, dO, s_dst, rec, (float4 *)work_rec, n,
                           (int)H, (int)C, lds, ldo);
        hipLaunchKernelGGL((k_gat_expand<LPH, VEC, DROP>), Deal<LPH>::grid(n * H), dim3(256), 0, st, rowptr_t, col_t, slot_t, Z, s_src,
                           dO, (const float4 *)work_rec, dZ, dS_src, work_g, n, (int)H, (int)C, ldz, lds, ldo, (float)negative_slope,
                           drop);
    });
    if (!fits) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (C above 64 lanes of the widest access the operands allow)");
    hipLaunchKernelGGL(k_gat_dst_sum, Deal<DST_LPR>::grid(n), dim3(256), 0, st, rowptr, (const float *)work_g, dS_dst, n, (int)H, lds);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

extern "C" int dcr_gat_gather_f32_dev(const int64_t *rowptr, const int32_t *col, const float *Z, const float *s_src,
                                      const float *s_dst, float *O, float *rec, int64_t n, int64_t H, int64_t C, int64_t ldz,
                                      int64_t lds, int64_t ldo, double negative_slope, void *hip_stream) {
    return gat_gather<false>(rowptr, col, Z, s_src, s_dst, O, rec, n, H, C, ldz, lds, ldo, negative_slope, hip_stream, GatDrop{});
}

extern "C" int dcr_gat_gather_drop_f32_dev(const int64_t *rowptr, const int32_t *col, const float *Z, const float *s_src,
                                           const float *s_dst, float *O, float *rec, int64_t n, int64_t H, int64_t C, int64_t ldz,
                                           int64_t lds, int64_t ldo, double negative_slope, void *hip_stream, int64_t nnz, double p,
                                           uint64_t seed, uint64_t offset, const int64_t *offset_dev, int64_t *offset_used_dev) {
    if (!offset_used_dev) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (null pointer)");
    GatDrop drop;
    DCR_TRY(gat_drop_args(nnz, p, seed, offset, offset_dev, offset_used_dev, drop));
    return gat_gather<true>(rowptr, col, Z, s_src, s_dst, O, rec, n, H, C, ldz, lds, ldo, negative_slope, hip_stream, drop);
}

extern "C" int dcr_gat_expand_f32_dev(const int64_t *rowptr, const int64_t *rowptr_t, const int32_t *col_t, const int64_t *slot_t,
                                      const float *Z, const float *s_src, const float *s_dst, const float *O, const float *dO,
                                      const float *rec, float *dZ, float *dS_src, float *dS_dst, float *work_rec, float *work_g,
                                      int64_t n, int64_t H, int64_t C, int64_t ldz, int64_t lds, int64_t ldo, double negative_slope,
                                      void *hip_stream) {
    return gat_expand<false>(rowptr, rowptr_t, col_t, slot_t, Z, s_src, s_dst, O, dO, rec, dZ, dS_src, dS_dst, work_rec, work_g, n, H,
                             C, ldz, lds, ldo, negative_slope, hip_stream, GatDrop{});
}

extern "C" int dcr_gat_expand_drop_f32_dev(const int64_t *rowptr, const int64_t *rowptr_t, const int32_t *col_t,
                                           const int64_t *slot_t, const float *Z, const float *s_src, const float *s_dst,
                                           const float *O, const float *dO, const float *rec, float *dZ, float *dS_src, float *dS_dst,
                                           float *work_rec, float *work_g, int64_t n, int64_t H, int64_t C, int64_t ldz, int64_t lds,
                                           int64_t ldo, double negative_slope, void *hip_stream, int64_t nnz, double p, uint64_t seed,
                                           const int64_t *offset_used_dev) {
    if (!offset_used_dev) DCR_FAIL(DCR_EINVAL, "bad GAT arguments (null pointer)");
    GatDrop drop;
    DCR_TRY(gat_drop_args(nnz, p, seed, 0, offset_used_dev, nullptr, drop));
    return gat_expand<true>(rowptr, rowptr_t, col_t, slot_t, Z, s_src, s_dst, O, dO, rec, dZ, dS_src, dS_dst, work_rec, work_g, n, H, C,
                            ldz, lds, ldo, negative_slope, hip_stream, drop);
}
