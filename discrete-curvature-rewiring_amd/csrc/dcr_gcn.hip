// What a GCN training step of libdcr_hip.so does around its sparse aggregation (csrc/dcr_spmm.hip), fp32: ReLU + dropout
// between the layers, the activation fused into the next layer's dense contraction, loss and accuracy on the selected rows,
// the head of an epoch in one kernel per direction, and the Adam step as one launch.
#include <cstdint>
#include "dcr_internal.h"
#include "dcr_philox.h"

using namespace dcr;

// ---------------------------------------------------------------------------------------------------------------------
// ReLU + dropout between the GCN layers (models/gcn.py:38-42: x = act_fn(x); x = dropout(x)) as ONE pass over the
// activations in each direction, with the keep mask packed to one bit per element: forward reads x, writes y and the
// bits (N*F/8 bytes); backward reads the gradient and the bits.  The stock path is four element-wise kernels and a
// byte mask (4.9 GB of traffic per training step at 1M x 128; this is 2.1 GB).  Random numbers: Philox-4x32-10 keyed by
// (seed, call offset), counter = element-quad index >> 1 (two quads share a call: dcr_philox.h, philox_quad16; the rule is
// written out in include/dcr.h), so a run is reproducible for a given torch seed.
namespace dcr {

// thread t owns elements 4t .. 4t+3; wave w stores the four keep-ballots of its 256 elements in bits[4w .. 4w+3]
__global__ void __launch_bounds__(256) k_relu_dropout_fwd(const float *__restrict__ x, float *__restrict__ y,
                                                           unsigned long long *__restrict__ bits, int64_t n, float scale,
                                                           uint32_t threshold, uint64_t seed, uint64_t offset,
                                                           const uint64_t *__restrict__ offset_dev) {
    if (offset_dev) offset += *offset_dev;  // call counter kept in device memory: the launch can be replayed from a hipGraph
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e0 = t * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (e0 + 3 < n) {
        const float4 q = *reinterpret_cast<const float4 *>(x + e0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        for (int j = 0; j < 4; ++j)
            if (e0 + j < n) v[j] = x[e0 + j];
    }
    uint32_t r[4];
    philox_quad16((uint64_t)t, offset, seed, r);
    bool keep[4];
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        keep[j] = v[j] > 0.f && r[j] >= threshold;  // P(r >= threshold) = 1 - p
        o[j] = keep[j] ? v[j] * scale : 0.f;
    }
    if (e0 + 3 < n) {
        *reinterpret_cast<float4 *>(y + e0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        for (int j = 0; j < 4; ++j)
            if (e0 + j < n) y[e0 + j] = o[j];
    }
    const int64_t wave = t >> 6;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long m = __ballot(keep[j]);
        if ((threadIdx.x & 63) == 0) bits[wave * 4 + j] = m;
    }
}

__global__ void __launch_bounds__(256) k_relu_dropout_bwd(const float *__restrict__ g, float *__restrict__ gin,
                                                           const unsigned long long *__restrict__ bits, int64_t n,
                                                           float scale) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e0 = t * 4;
    if (e0 >= n) return;
    const int64_t wave = t >> 6;
    const int lane = threadIdx.x & 63;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (e0 + 3 < n) {
        const float4 q = *reinterpret_cast<const float4 *>(g + e0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        for (int j = 0; j < 4; ++j)
            if (e0 + j < n) v[j] = g[e0 + j];
    }
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = ((bits[wave * 4 + j] >> lane) & 1ull) ? v[j] * scale : 0.f;
    if (e0 + 3 < n) {
        *reinterpret_cast<float4 *>(gin + e0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        for (int j = 0; j < 4; ++j)
            if (e0 + j < n) gin[e0 + j] = o[j];
    }
}

}  // namespace dcr

extern "C" int dcr_relu_dropout_bits_words(int64_t n, int64_t *out_words) {
    if (!out_words || n < 0) DCR_FAIL(DCR_EINVAL, "bad argument");
    const int64_t threads = (n + 3) / 4, blocks = (threads + 255) / 256;
    *out_words = blocks * 4 * 4;  // 4 waves per workgroup, 4 ballots per wave
    return DCR_OK;
}

extern "C" int dcr_relu_dropout_fwd_f32_ctr_dev(const float *x, float *y, uint64_t *bits, int64_t n, double p,
                                                uint64_t seed, uint64_t offset, const uint64_t *offset_dev,
                                                void *hip_stream) {
    if (!x || !y || !bits || n < 0 || !(p >= 0.0 && p < 1.0)) DCR_FAIL(DCR_EINVAL, "bad relu_dropout arguments");
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15)) DCR_FAIL(DCR_EINVAL, "relu_dropout: 16-byte aligned tensors expected");
    if (n == 0) return DCR_OK;
    const int64_t threads = (n + 3) / 4, blocks = (threads + 255) / 256;
    const uint32_t threshold = dcr::dropout_threshold16(p);
    hipLaunchKernelGGL(k_relu_dropout_fwd, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, x, y,
                       (unsigned long long *)bits, n, (float)(1.0 / (1.0 - p)), threshold, seed, offset, offset_dev);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

extern "C" int dcr_relu_dropout_fwd_f32_dev(const float *x, float *y, uint64_t *bits, int64_t n, double p, uint64_t seed,
                                            uint64_t offset, void *hip_stream) {
    return dcr_relu_dropout_fwd_f32_ctr_dev(x, y, bits, n, p, seed, offset, nullptr, hip_stream);
}

extern "C" int dcr_relu_dropout_bwd_f32_dev(const float *grad_out, float *grad_in, const uint64_t *bits, int64_t n,
                                            double p, void *hip_stream) {
    if (!grad_out || !grad_in || !bits || n < 0 || !(p >= 0.0 && p < 1.0)) DCR_FAIL(DCR_EINVAL, "bad relu_dropout arguments");
    if (((uintptr_t)grad_out & 15) || ((uintptr_t)grad_in & 15))
        DCR_FAIL(DCR_EINVAL, "relu_dropout: 16-byte aligned tensors expected");
    if (n == 0) return DCR_OK;
    const int64_t threads = (n + 3) / 4, blocks = (threads + 255) / 256;
    hipLaunchKernelGGL(k_relu_dropout_bwd, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, grad_out, grad_in,
                       (const unsigned long long *)bits, n, (float)(1.0 / (1.0 - p)));
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

// ---- activation fused into the next layer's dense contraction ---------------------------------------------------------
// models/gcn.py:36-42 between two layers: x = relu(x); x = dropout(x); then the next GCNConv's lin (x·Wᵀ, W = [C, H] with C
// classes).  As separate passes the hidden activation (N x H floats: 512 MB at the 1M-node bench shape) was read by the
// ReLU/dropout kernel, written, read again by the GEMM library — and once more each for the evaluation operand of the
// one-pass epoch (relu, GEMM) — 0.68 ms of a 4.6 ms epoch for 8 GFLOP.  Here one pass reads the pre-activation row, applies
// ReLU (+ dropout with the SAME Philox stream and keep-bit layout as k_relu_dropout_fwd: element 4t..4t+3 belongs to
// thread t, wave w of 64 threads stores its four ballots in bits[4w..4w+3]), stores the training activation (the weight
// gradient needs it) and contracts both operands with W on the spot: LPR = H / 4 lanes hold one row (4 floats each) and
// their 4-column block of W in registers (64 floats), each forms its partial of the 16 + 16 outputs, and a
// reduce-scatter over the row's lanes (halve the values, exchange, add: 31 shuffles for 32 values instead of 160) leaves
// every lane with 32 / LPR finished outputs.  Memory-bound: N·H·4 read + N·H·4 written + 2·N·C·4.
namespace dcr {

// MFMA form.  A wave takes 16 rows at a time; lane (i = lane & 15, g = lane >> 4) loads, for m = 0 .. H/16 - 1, the four
// floats x[row i][16m + 4g ..] — exactly the A-operand shape of v_mfma_f32_16x16x4_f32 (lane l supplies A[l & 15][k = l >> 4])
// when step (m, q) takes the k index g to be hidden column 16m + 4g + q; the matching B operand W[class i][16m + 4g + q] sits
// in 4·H/16 registers per lane for the whole kernel.  Two accumulator tiles (training, evaluation) of 4 registers each hold
// z[row 4g + r][class i]: no cross-lane reduction at all (the VALU version spent more on its reduce-scatter than on the
// products, and both on top of Philox made it ALU-bound at 0.36 ms for 1.2 GB).  The float4 a lane holds is element
// t = row·H/4 + 4m + g of k_relu_dropout_fwd's numbering: same Philox counter, same place in the bit words
// (word 4·(t >> 6) + q, bit t & 63), assembled here with two OR-exchanges across g and one or two across neighbouring rows.
template <int HM, bool TRAIN, bool EVAL>
__global__ void __launch_bounds__(256) k_act_linear_fwd(const float *__restrict__ x, const float *__restrict__ w, float *__restrict__ h_train,
                                                         float *__restrict__ z_train, float *__restrict__ z_eval, int64_t ldz,
                                                         unsigned long long *__restrict__ bits, int64_t n_rows, int C, float scale,
                                                         uint32_t threshold, uint64_t seed, uint64_t offset,
                                                         const uint64_t *__restrict__ offset_dev) {
    constexpr int H = 16 * HM, LPR = H / 4, RPW = 64 / LPR;  // RPW rows share one set of four bit words
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    if (TRAIN && offset_dev) offset += *offset_dev;
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    float wb[HM][4];
#pragma unroll
    for (int m = 0; m < HM; ++m) {
        const float4 t = i < C ? *reinterpret_cast<const float4 *>(w + (int64_t)i * H + 16 * m + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
        wb[m][0] = t.x; wb[m][1] = t.y; wb[m][2] = t.z; wb[m][3] = t.w;
    }
    const int64_t n_tiles = (n_rows + 15) / 16;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t row = tile * 16 + i;
        const bool live = row < n_rows;
        float v[HM][4];
#pragma unroll
        for (int m = 0; m < HM; ++m) {
            const float4 t = live ? *reinterpret_cast<const float4 *>(x + row * H + 16 * m + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[m][0] = t.x; v[m][1] = t.y; v[m][2] = t.z; v[m][3] = t.w;
        }
        f32x4 acc_tr = {0.f, 0.f, 0.f, 0.f}, acc_ev = {0.f, 0.f, 0.f, 0.f};
        if (TRAIN) {
            uint32_t part[4] = {0u, 0u, 0u, 0u};  // keep bits of this lane's elements, bit 4m + g of column q's word
#pragma unroll
            for (int m = 0; m < HM; ++m) {
                const int64_t t = row * LPR + 4 * m + g;
                uint32_t r[4];
                philox_quad16((uint64_t)t, offset, seed, r);
                float o[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool keep = v[m][q] > 0.f && r[q] >= threshold;
                    o[q] = keep ? v[m][q] * scale : 0.f;
                    part[q] |= keep ? (1u << (4 * m + g)) : 0u;
                }
                if (live && h_train) *reinterpret_cast<float4 *>(h_train + row * H + 16 * m + 4 * g) = make_float4(o[0], o[1], o[2], o[3]);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc_tr = __builtin_amdgcn_mfma_f32_16x16x4f32(o[q], wb[m][q], acc_tr, 0, 0, 0);
            }
            // bit words: OR over the four g of a row, then over the RPW rows of a word (row s of them shifted by s·LPR)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t p = part[q];
                p |= (uint32_t)__shfl_xor((int)p, 16);
                p |= (uint32_t)__shfl_xor((int)p, 32);
                unsigned long long word = (unsigned long long)p << ((i % RPW) * LPR);
                uint32_t lo = (uint32_t)word, hi = (uint32_t)(word >> 32);
#pragma unroll
                for (int d = 1; d < RPW; d <<= 1) {
                    lo |= (uint32_t)__shfl_xor((int)lo, d);
                    hi |= (uint32_t)__shfl_xor((int)hi, d);
                }
                if (g == 0 && (i % RPW) == 0 && live) bits[(row / RPW) * 4 + q] = ((unsigned long long)hi << 32) | lo;
            }
        }
        if (EVAL) {
#pragma unroll
            for (int m = 0; m < HM; ++m)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    acc_ev = __builtin_amdgcn_mfma_f32_16x16x4f32(v[m][q] > 0.f ? v[m][q] : 0.f, wb[m][q], acc_ev, 0, 0, 0);
        }
        // accumulator register r of lane (i, g) is z[row 4g + r of the tile][class i]
        if (i < C) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t orow = tile * 16 + 4 * g + r;
                if (orow < n_rows) {
                    if (TRAIN) z_train[orow * ldz + i] = acc_tr[r];
                    if (EVAL) z_eval[orow * ldz + i] = acc_ev[r];
                }
            }
        }
    }
}

// dx = keep ? (dz · W) / (1 - p) : 0 — the backward of the training operand above in one pass (it was a GEMM writing
// N x H floats and the ReLU/dropout backward reading and writing them again).  A workgroup takes 256 rows: their dz rows
// (256·C floats, contiguous) and bit words go through LDS in one coalesced sweep, then every wave walks its 64 rows with
// LPR lanes per row (4 columns each, their block of W in registers), reading dz as LDS broadcasts: the first version
// loaded the 16 gradients of a row with 16 dependent global loads per two rows and ran at 2.1 TB/s.
template <int LPR>
__global__ void __launch_bounds__(256) k_act_linear_bwd(const float *__restrict__ dz, const float *__restrict__ w,
                                                         const unsigned long long *__restrict__ bits, float *__restrict__ dx,
                                                         int64_t n_rows, int C, float scale, float *__restrict__ colpart) {
    // colpart (nullable): [gridDim.x][H] column sums of the rows this workgroup wrote — the bias gradient of the layer that
    // produced x is the column sum of dx, and dx is in registers here (k_colsum_finish adds the workgroups' parts in order)
    constexpr int H = 4 * LPR, RPW = 64 / LPR, TR = 256, WORDS = TR / RPW * 4;
    __shared__ float tile[TR * 16];
    __shared__ unsigned long long tbits[WORDS];
    const int lane = threadIdx.x & 63, sl = lane % LPR, sub = lane / LPR, wave = threadIdx.x >> 6;
    float cs[4] = {0.f, 0.f, 0.f, 0.f};
    float wr[16][4];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float4 t = j < C ? *reinterpret_cast<const float4 *>(w + (int64_t)j * H + 4 * sl) : make_float4(0.f, 0.f, 0.f, 0.f);
        wr[j][0] = t.x; wr[j][1] = t.y; wr[j][2] = t.z; wr[j][3] = t.w;
    }
    const int64_t n_tiles = (n_rows + TR - 1) / TR;
    const bool vec = (C & 3) == 0 && ((uintptr_t)dz & 15) == 0;
    for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int64_t row0 = tl * TR;
        const int nrow = (int)(n_rows - row0 < TR ? n_rows - row0 : TR);
        const int nfl = nrow * C;
        const float *src = dz + row0 * C;
        if (vec) {
            for (int k = threadIdx.x; k < nfl / 4; k += 256) reinterpret_cast<float4 *>(tile)[k] = reinterpret_cast<const float4 *>(src)[k];
        } else {
            for (int k = threadIdx.x; k < nfl; k += 256) tile[k] = src[k];
        }
        const int nwords = (nrow + RPW - 1) / RPW * 4;
        for (int k = threadIdx.x; k < nwords; k += 256) tbits[k] = bits[row0 / RPW * 4 + k];
        __syncthreads();
#pragma unroll 4
        for (int st = 0; st < 64 / RPW; ++st) {
            const int r = wave * 64 + st * RPW + sub;
            if (r >= nrow) continue;
            float g[16];
            if (C == 16) {
#pragma unroll
                for (int j4 = 0; j4 < 4; ++j4) {
                    const float4 t = reinterpret_cast<const float4 *>(tile)[r * 4 + j4];
                    g[4 * j4] = t.x; g[4 * j4 + 1] = t.y; g[4 * j4 + 2] = t.z; g[4 * j4 + 3] = t.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) g[j] = j < C ? tile[r * C + j] : 0.f;
            }
            float o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float acc = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) acc = fmaf(g[j], wr[j][q], acc);
                const bool keep = (tbits[(wave * (64 / RPW) + st) * 4 + q] >> lane) & 1ull;
                o[q] = keep ? acc * scale : 0.f;
                cs[q] += o[q];
            }
            *reinterpret_cast<float4 *>(dx + ((row0 + r) * LPR + sl) * 4) = make_float4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();
    }
    if (colpart) {  // uniform
        __shared__ float red[4][H];
#pragma unroll
        for (int m = LPR; m < 64; m <<= 1)
#pragma unroll
            for (int q = 0; q < 4; ++q) cs[q] += __shfl_xor(cs[q], m, 64);
        if (sub == 0)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[threadIdx.x >> 6][4 * sl + q] = cs[q];
        __syncthreads();
        if (threadIdx.x < H)
            colpart[(int64_t)blockIdx.x * H + threadIdx.x] =
                (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
}

// The whole backward of the fused activation + contraction in ONE pass, on the matrix cores: dx = keep ? (dz·W)/(1-p) : 0,
// its column sums (bias gradient of the previous layer) and dW = dzᵀ·h with h = keep ? x/(1-p) : 0 rebuilt from x and the
// keep bits — the forward pass then need not store h (N x H floats written and read back), and the separate weight-gradient
// reduction over all rows (0.26 ms at 1M x 128 x 16) goes away.  A workgroup stages 256 rows of dz and their bit words in LDS
// (k_act_linear_bwd); a wave takes 16 rows at a time with v_mfma_f32_16x16x4_f32, lane (i = lane & 15, g = lane >> 4):
//   dx tile:  A[row i][k = g] = dz[row i][class 4s + g] (LDS), B[k = g][n = i] = W[class 4s + g][col(i)] (registers),
//             D register r = dx[row 4g + r][col(i)], with col(i) = 64b + 4i + q for MFMA (b, q): the four q of one b are four
//             consecutive columns, so every lane stores float4s and a wave writes 256 contiguous bytes of each of 4 rows;
//   dW tile:  A[class i][k = g] = dz[row 4s + g][class i] (LDS), B[k = g][n = i] = h[row 4s + g][col(i)] from a float4 load
//             of x[row 4s + g][64b + 4i ..] (a wave reads 256 contiguous bytes of each of 4 rows), D register r =
//             dW[class 4g + r][col(i)], accumulated in registers over all tiles of the wave.
// Element (row, column 4·sl + q) keeps bit (row % RPW)·LPR + sl of word 4·(row / RPW) + q, as everywhere else.
template <int HB>  // H = 64 * HB
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) k_act_linear_bwd_fused(const float *__restrict__ dz, const float *__restrict__ w,
                                                               const unsigned long long *__restrict__ bits, const float *__restrict__ x,
                                                               float *__restrict__ dx, int64_t n_rows, int C, float scale,
                                                               float *__restrict__ part) {
    // part: [gridDim.x][H + 16 * H]: column sums of dx, then the workgroup's dW (class-major, 16 rows)
    constexpr int H = 64 * HB, LPR = H / 4, RPW = 64 / LPR, TR = 256, WORDS = TR / RPW * 4;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    __shared__ float tile[TR * 16];
    __shared__ unsigned long long tbits[WORDS];
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    float wb[4][HB][4];  // W[class 4s + g][64b + 4i + q]
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int b = 0; b < HB; ++b) {
            const int cls = 4 * s4 + g;
            const float4 t = cls < C ? *reinterpret_cast<const float4 *>(w + (int64_t)cls * H + 64 * b + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
            wb[s4][b][0] = t.x; wb[s4][b][1] = t.y; wb[s4][b][2] = t.z; wb[s4][b][3] = t.w;
        }
    f32x4 dw[HB][4];
    float cs[HB][4];
#pragma unroll
    for (int b = 0; b < HB; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            dw[b][q] = f32x4{0.f, 0.f, 0.f, 0.f};
            cs[b][q] = 0.f;
        }
    const int64_t n_tiles = (n_rows + TR - 1) / TR;
    const bool vec = (C & 3) == 0 && ((uintptr_t)dz & 15) == 0;
    for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int64_t row0 = tl * TR;
        const int nrow = (int)(n_rows - row0 < TR ? n_rows - row0 : TR);
        const int nfl = nrow * C;
        const float *src = dz + row0 * C;
        if (vec) {
            for (int k = threadIdx.x; k < TR * C / 4; k += 256)
                reinterpret_cast<float4 *>(tile)[k] = k < nfl / 4 ? reinterpret_cast<const float4 *>(src)[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int k = threadIdx.x; k < TR * C; k += 256) tile[k] = k < nfl ? src[k] : 0.f;
        }
        const int nwords = (nrow + RPW - 1) / RPW * 4;
        for (int k = threadIdx.x; k < WORDS; k += 256) tbits[k] = k < nwords ? bits[row0 / RPW * 4 + k] : 0ull;
        __syncthreads();
        for (int st = 0; st < 4; ++st) {  // the wave's four 16-row tiles
            const int r0 = wave * 64 + st * 16;
            if (r0 >= nrow) break;  // uniform
            // one 64-column block at a time: its x rows are requested first, the dx block is formed and stored while they
            // travel, then the block's part of dW (register budget: two waves per SIMD need the kernel under 256 per lane,
            // 72 of them persistent: W, dW, column sums)
#pragma unroll
            for (int b = 0; b < HB; ++b) {
                float xv[4][4];  // x[row 4s + g][64b + 4i + q]
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    const int64_t row = row0 + r0 + 4 * s4 + g;
                    const float4 t = row < n_rows ? *reinterpret_cast<const float4 *>(x + row * H + 64 * b + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
                    xv[s4][0] = t.x; xv[s4][1] = t.y; xv[s4][2] = t.z; xv[s4][3] = t.w;
                }
                // ---- dx = mask · scale · (dz · W) ----
                f32x4 acc[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    const int cls = 4 * s4 + g;
                    const float a = cls < C ? tile[(r0 + i) * C + cls] : 0.f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wb[s4][b][q], acc[q], 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rl = r0 + 4 * g + r;  // row of accumulator register r
                    const int wbase = rl / RPW * 4, sh = (rl % RPW) * LPR + i + 16 * b;
                    float o[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bool keep = (tbits[wbase + q] >> sh) & 1ull;
                        o[q] = keep ? acc[q][r] * scale : 0.f;
                        cs[b][q] += o[q];
                    }
                    if (rl < nrow) *reinterpret_cast<float4 *>(dx + (row0 + rl) * H + 64 * b + 4 * i) = make_float4(o[0], o[1], o[2], o[3]);
                }
                // ---- dW += dzᵀ · h ----
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    const int rl = r0 + 4 * s4 + g;
                    const float a = i < C ? tile[rl * C + i] : 0.f;
                    const int wbase = rl / RPW * 4, sh = (rl % RPW) * LPR + i + 16 * b;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bool keep = (tbits[wbase + q] >> sh) & 1ull;
                        const float hv = keep ? xv[s4][q] * scale : 0.f;
                        dw[b][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, hv, dw[b][q], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
    }
    // ---- the workgroup's parts: waves added in wave order through LDS (reusing the dz tile: 4 x (H + 16 H) floats > 16 KB
    //      for H = 128, so two rounds) ----
    float *out = part + (int64_t)blockIdx.x * (H + 16 * H);
    // column sums: over g inside the wave, then over the waves
#pragma unroll
    for (int b = 0; b < HB; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cs[b][q] += __shfl_xor(cs[b][q], 16, 64);
            cs[b][q] += __shfl_xor(cs[b][q], 32, 64);
        }
    __syncthreads();
    if (g == 0)
#pragma unroll
        for (int b = 0; b < HB; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) tile[wave * H + 64 * b + 4 * i + q] = cs[b][q];
    __syncthreads();
    if (threadIdx.x < H) out[threadIdx.x] = (tile[threadIdx.x] + tile[H + threadIdx.x]) + (tile[2 * H + threadIdx.x] + tile[3 * H + threadIdx.x]);
    __syncthreads();
    // dW: register r of (b, q) is dW[class 4g + r][64b + 4i + q]; waves 0,1 then 2,3 through the 16 KB tile
    for (int round = 0; round < 2; ++round) {
        if ((wave >> 1) == round) {
#pragma unroll
            for (int b = 0; b < HB; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r) tile[(wave & 1) * 16 * H + (4 * g + r) * H + 64 * b + 4 * i + q] = dw[b][q][r];
        }
        __syncthreads();
        for (int k = threadIdx.x; k < 16 * H; k += 256) {
            const float v = tile[k] + tile[16 * H + k];
            out[H + k] = round == 0 ? v : out[H + k] + v;
        }
        __syncthreads();
    }
}

// out[c] = sum over the parts of column c, in a fixed order (one workgroup per column)
__global__ void __launch_bounds__(256) k_colsum_finish(const float *__restrict__ part, int64_t n_parts, int H, float *__restrict__ out) {
    __shared__ float red[256];
    const int c = blockIdx.x;
    float a = 0.f;
    for (int64_t i = threadIdx.x; i < n_parts; i += 256) a += part[i * H + c];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = red[0];
}

// out0[c] (c < split) and out1[c - split] = sum over the parts of column c of a [n_parts][stride] array, in a fixed order
__global__ void __launch_bounds__(256) k_parts_finish(const float *__restrict__ part, int64_t n_parts, int stride, int split,
                                                       float *__restrict__ out0, float *__restrict__ out1) {
    __shared__ float red[256];
    const int c = blockIdx.x;
    float a = 0.f;
    for (int64_t k = threadIdx.x; k < n_parts; k += 256) a += part[k * stride + c];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (c < split) out0[c] = red[0];
        else out1[c - split] = red[0];
    }
}

void launch_parts_finish(const float *part, int64_t n_parts, int stride, int split, int columns, float *out0, float *out1, hipStream_t st) {
    hipLaunchKernelGGL(k_parts_finish, dim3((unsigned)columns), dim3(256), 0, st, part, n_parts, stride, split, out0, out1);
}

template <int HM>
static void launch_act_linear_fwd(bool train, bool eval, const float *x, const float *w, float *h_train, float *z_train, float *z_eval,
                                  int64_t ldz, unsigned long long *bits, int64_t n_rows, int C, float scale, uint32_t threshold, uint64_t seed,
                                  uint64_t offset, const uint64_t *offset_dev, hipStream_t st) {
    const int64_t n_waves = (n_rows + 15) / 16;        // a wave per 16-row tile
    int64_t blocks = (n_waves + 3) / 4;
    if (blocks > 256 * 8) blocks = 256 * 8;            // grid-stride: the weights are loaded into registers once per wave
    if (blocks < 1) blocks = 1;
    if (train && eval)
        hipLaunchKernelGGL((k_act_linear_fwd<HM, true, true>), dim3((unsigned)blocks), dim3(256), 0, st, x, w, h_train, z_train, z_eval, ldz, bits,
                           n_rows, C, scale, threshold, seed, offset, offset_dev);
    else if (train)
        hipLaunchKernelGGL((k_act_linear_fwd<HM, true, false>), dim3((unsigned)blocks), dim3(256), 0, st, x, w, h_train, z_train, z_eval, ldz, bits,
                           n_rows, C, scale, threshold, seed, offset, offset_dev);
    else
        hipLaunchKernelGGL((k_act_linear_fwd<HM, false, true>), dim3((unsigned)blocks), dim3(256), 0, st, x, w, h_train, z_train, z_eval, ldz, bits,
                           n_rows, C, scale, threshold, seed, offset, offset_dev);
}

}  // namespace dcr

// ---- loss and accuracy on the selected rows (experiment/training_loop.py:51 F.nll_loss(log_probs[mask], y[mask]); :64-71
// log_probs[mask].max(1)[1].eq(y[mask]).sum()) — a dozen stock element-wise / reduction launches of a few microseconds each per
// epoch, as three kernels.  The gradient is -g / m at the picked entries and zero elsewhere, as the stock kernels give it.
namespace dcr {

// Round 4: many workgroups, each a fixed slice of the rows, and the LAST one to finish adds the slices' sums in slice order
// (deterministic).  As one workgroup of 1,024 threads every thread walked ~100 rows of the bench's training split one
// dependent pair of loads after the other: 92 us per epoch for a 100k-element gather.  The partial sums live in a buffer of
// the library (one per device and process: calls are expected on one stream at a time, as the epoch's graph issues them).
// Round 5 (advisor, round 4): the partial sums and the ticket live in the CALLER's workspace (the head kernels' HeadWs below:
// one buffer per device and stream, tickets zero before the first use and left zero by every launch) — as process-global
// device variables two loss calls in flight on different streams mixed their partials.
constexpr int PICKED_BLOCKS = 256;
constexpr int HEAD_MAXC = 32, HEAD_MAXB = 1024;
struct HeadWs {
    double loss_part[HEAD_MAXB];
    unsigned long long hit_part[HEAD_MAXB];
    float col_part[HEAD_MAXB][HEAD_MAXC];
    unsigned ticket_fwd, ticket_bwd;
    unsigned pad[2];
};

__global__ void __launch_bounds__(256) k_picked_mean_fwd(const float *__restrict__ lp, int64_t ld, const int64_t *__restrict__ y,
                                                          int64_t m, int C, float *__restrict__ out, HeadWs *ws) {
    double *picked_partial = ws->loss_part;
    unsigned &picked_ticket = ws->ticket_fwd;
    __shared__ double red[256];
    const int64_t per = (m + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < m ? lo + per : m;
    double a = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const int64_t t = y[i];
        if (t >= 0 && t < C) a += (double)lp[i * ld + t];
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) __hip_atomic_store(&picked_partial[blockIdx.x], red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!last_arriver(&picked_ticket, gridDim.x)) return;
    red[threadIdx.x] = (int)threadIdx.x < (int)gridDim.x
                           ? __hip_atomic_load(&picked_partial[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (float)(-red[0] / (double)m);
        picked_ticket = 0u;  // (for the next call)
    }
}

__global__ void __launch_bounds__(256) k_picked_mean_bwd(const int64_t *__restrict__ y, int64_t m, int C, const float *__restrict__ g,
                                                          float *__restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one element of the [m, C] gradient
    if (i >= m * C) return;
    const int64_t row = i / C;
    const int c = (int)(i - row * C);
    grad[i] = y[row] == c ? -(g[0] / (float)m) : 0.f;
}

__global__ void __launch_bounds__(256) k_count_argmax_equal(const float *__restrict__ lp, int64_t ld, const int64_t *__restrict__ y,
                                                             int64_t m, int C, unsigned long long *__restrict__ out) {
    __shared__ int red[256];
    int hits = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
        const float *r = lp + i * ld;
        float best = r[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {  // first maximum; a NaN counts as the maximum (torch.max)
            const float v = r[c];
            if (!(best != best) && (v > best || v != v)) {
                best = v;
                arg = c;
            }
        }
        hits += (int64_t)arg == y[i] ? 1 : 0;
    }
    red[threadIdx.x] = hits;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0]) atomicAdd(out, (unsigned long long)red[0]);
}


// ---- Round 5: the head of an epoch in ONE kernel per direction ------------------------------------------------------------------
// experiment/training_loop.py:50-51 F.nll_loss(model(data)[train_mask], y[train_mask]) with models/gcn.py:44 log_softmax in front
// of it, and :64-71 the arg-max accuracy on the evaluated split, from the RAW outputs of the last aggregation (the arg-max of a row
// of log-probabilities is the arg-max of its logits).  Before: two softmax launches, the picked-mean kernel, the arg-max count and
// two fills forward; a fill, the picked-mean backward, the softmax backward, a fill and a column-sum reduction (the last layer's
// bias gradient) backward — eleven launches of 4-12 us each for a few hundred KB.  A thread per row (at most 32 classes):
//   forward:  nll_i = lse_i - o[i, y_i],  lse_i = max_c o[i, c] + log(sum_c exp(o[i, c] - max)); loss = mean_i nll_i (float64 sum
//             of per-block sums in block order); correct = number of evaluated rows whose first maximum is their label;
//   backward: grad[i, c] = (exp(o[i, c] - lse_i) - [c == y_i]) * g / m, and its column sums (per-block partials added in block
//             order: deterministic) = the gradient of the last layer's bias.
// The last block to finish (last_arriver) closes each reduction; partials and tickets live in a workspace of the CALLER (as
// process-global device variables they were shared by every stream) whose tickets are zero before the first use and left
// zero by every launch.

template <int C>
__device__ __forceinline__ float head_lse(const float (&o)[C], int classes) {
    float mx = o[0];
#pragma unroll
    for (int c = 1; c < C; ++c)
        if (c < classes) mx = fmaxf(mx, o[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (c < classes) s += expf(o[c] - mx);
    return mx + logf(s);
}

// a row of raw outputs into registers: 16-byte loads where the row stride and the width allow (a thread reads its own 64-byte row:
// one instruction per 16 bytes instead of one per float — the loads are what the kernel's time is)
template <int C>
__device__ __forceinline__ void head_load_row(const float *__restrict__ base, int64_t i, int64_t ld, int classes, bool vec, float (&o)[C]) {
    if (vec) {
#pragma unroll
        for (int q = 0; q < C / 4; ++q) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (4 * q < classes) v = *reinterpret_cast<const float4 *>(base + i * ld + 4 * q);
            o[4 * q] = v.x; o[4 * q + 1] = v.y; o[4 * q + 2] = v.z; o[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = c < classes ? base[i * ld + c] : 0.f;
    }
}

template <int C>
__global__ void __launch_bounds__(256) k_head_fwd(const float *__restrict__ o_tr, int64_t ld_tr, const int64_t *__restrict__ y_tr, int64_t m_tr,
                                                  int nb_tr, const float *__restrict__ o_ev, int64_t ld_ev, const int64_t *__restrict__ y_ev,
                                                  int64_t m_ev, int nb_ev, int classes, float *__restrict__ out_loss,
                                                  long long *__restrict__ out_correct, HeadWs *__restrict__ ws) {
    __shared__ double red[256];
    __shared__ unsigned long long redh[256];
    const int b = blockIdx.x;
    double a = 0.0;
    unsigned long long hits = 0ull;
    if (b < nb_tr) {
        const int64_t per = (m_tr + nb_tr - 1) / nb_tr, lo = (int64_t)b * per, hi = lo + per < m_tr ? lo + per : m_tr;
        const bool vec = (classes & 3) == 0 && (ld_tr & 3) == 0 && (((uintptr_t)o_tr) & 15) == 0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
            float o[C];
            head_load_row<C>(o_tr, i, ld_tr, classes, vec, o);
            const int64_t t = y_tr[i];
            float pick = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c)
                if ((int64_t)c == t) pick = o[c];
            if (t >= 0 && t < classes) a += (double)(head_lse<C>(o, classes) - pick);
        }
    } else {
        const int be = b - nb_tr;
        const int64_t per = (m_ev + nb_ev - 1) / nb_ev, lo = (int64_t)be * per, hi = lo + per < m_ev ? lo + per : m_ev;
        const bool vec = (classes & 3) == 0 && (ld_ev & 3) == 0 && (((uintptr_t)o_ev) & 15) == 0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
            float r[C];
            head_load_row<C>(o_ev, i, ld_ev, classes, vec, r);
            float best = r[0];
            int arg = 0;
#pragma unroll
            for (int c = 1; c < C; ++c) {  // first maximum; a NaN counts as the maximum (torch.max)
                if (c >= classes) break;
                const float v = r[c];
                if (!(best != best) && (v > best || v != v)) {
                    best = v;
                    arg = c;
                }
            }
            hits += (int64_t)arg == y_ev[i] ? 1ull : 0ull;
        }
    }
    red[threadIdx.x] = a;
    redh[threadIdx.x] = hits;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[threadIdx.x] += red[threadIdx.x + s];
            redh[threadIdx.x] += redh[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&ws->loss_part[b], red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&ws->hit_part[b], redh[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!last_arriver(&ws->ticket_fwd, gridDim.x)) return;
    // at most 256 partials of each kind (head_blocks): one per thread, then the same fixed tree as above.  (First version: one
    // thread adding them one after the other — 782 dependent L2 round trips, 111 us for a kernel whose work is 5 us.)
    red[threadIdx.x] = (int)threadIdx.x < nb_tr ? __hip_atomic_load(&ws->loss_part[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    redh[threadIdx.x] = (int)threadIdx.x < nb_ev ? __hip_atomic_load(&ws->hit_part[nb_tr + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[threadIdx.x] += red[threadIdx.x + s];
            redh[threadIdx.x] += redh[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (out_loss) out_loss[0] = m_tr > 0 ? (float)(red[0] / (double)m_tr) : 0.f;
        if (out_correct) out_correct[0] = (long long)redh[0];
        ws->ticket_fwd = 0u;
    }
}

template <int C>
__global__ void __launch_bounds__(256) k_head_bwd(const float *__restrict__ o_tr, int64_t ld_tr, const int64_t *__restrict__ y_tr, int64_t m_tr,
                                                  int classes, const float *__restrict__ g, float *__restrict__ grad,
                                                  float *__restrict__ grad_bias, HeadWs *__restrict__ ws) {
    __shared__ float red[4][HEAD_MAXC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float scale = g[0] / (float)m_tr;
    const int64_t per = (m_tr + gridDim.x - 1) / gridDim.x, lo = (int64_t)blockIdx.x * per, hi = lo + per < m_tr ? lo + per : m_tr;
    float cs[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cs[c] = 0.f;
    const bool vec = (classes & 3) == 0 && (ld_tr & 3) == 0 && (((uintptr_t)o_tr) & 15) == 0 && (((uintptr_t)grad) & 15) == 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        float o[C], gv[C];
        head_load_row<C>(o_tr, i, ld_tr, classes, vec, o);
        const float lse = head_lse<C>(o, classes);
        const int64_t t = y_tr[i];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            gv[c] = c < classes ? (expf(o[c] - lse) - ((int64_t)c == t ? 1.f : 0.f)) * scale : 0.f;
            cs[c] += gv[c];
        }
        if (vec) {
#pragma unroll
            for (int q = 0; q < C / 4; ++q)
                if (4 * q < classes) *reinterpret_cast<float4 *>(grad + i * classes + 4 * q) = make_float4(gv[4 * q], gv[4 * q + 1], gv[4 * q + 2], gv[4 * q + 3]);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (c < classes) grad[i * classes + c] = gv[c];
        }
    }
    // column sums: inside a wave by a fixed butterfly, the four waves in wave order, the blocks in block order
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float v = cs[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) red[wave][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)HEAD_MAXC)
        __hip_atomic_store(&ws->col_part[blockIdx.x][threadIdx.x],
                           threadIdx.x < (unsigned)C ? ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x] : 0.f,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!last_arriver(&ws->ticket_bwd, gridDim.x)) return;
    // the blocks' column sums: thread (column c, group j) adds blocks j, j + 8, ... (at most 32 independent loads), the eight
    // groups are then added in group order
    __shared__ float fin[8][HEAD_MAXC];
    {
        const int c = threadIdx.x & 31, j = threadIdx.x >> 5;
        float acc = 0.f;
        for (int k0 = j; k0 < (int)gridDim.x; k0 += 64) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int k = k0 + 8 * q;
                v[q] = k < (int)gridDim.x ? __hip_atomic_load(&ws->col_part[k][c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) acc += v[q];
        }
        fin[j][c] = acc;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)classes && grad_bias) {
        float sum = fin[0][threadIdx.x];
#pragma unroll
        for (int j = 1; j < 8; ++j) sum += fin[j][threadIdx.x];
        grad_bias[threadIdx.x] = sum;
    }
    if (threadIdx.x == 0) ws->ticket_bwd = 0u;
}

static int head_blocks(int64_t m) {
    int64_t b = (m + 255) / 256;
    if (b > 256) b = 256;   // (one partial per thread of the closing block)
    return (int)b;
}


// ---- Round 5: the optimiser step of an epoch as ONE launch --------------------------------------------------------------------
// experiment/save_models.py:78-82: Adam over two parameter groups that differ in their weight decay only (L2 added to the
// gradient).  torch's implementations take 2-3 launches per group (step counters, the update; ~45 without `fused`); the four
// tensors of the 2-layer model are 33k + 2k elements: one grid over all of them.  The update is torch.optim.Adam's
// (amsgrad off, maximize off), in float32, with the step count in device memory so that a captured epoch advances it:
//     g += wd * p;  m += (1 - b1) (g - m);  v = b2 v + (1 - b2) g g;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
constexpr int ADAM_MAXT = 8;
struct AdamArgs {
    float *p[ADAM_MAXT];
    const float *g[ADAM_MAXT];
    float *m[ADAM_MAXT];
    float *v[ADAM_MAXT];
    int64_t start[ADAM_MAXT + 1];   // tensor t holds the flat elements start[t] .. start[t + 1]
    float wd[ADAM_MAXT];
    int nt;
    float lr, b1, b2, eps;
};
__global__ void __launch_bounds__(256) k_adam_multi(AdamArgs A, float *__restrict__ step, unsigned *__restrict__ ticket) {
    const float t = step[0] + 1.f;   // (every block reads it before the last one to finish advances it)
    const float bc1 = 1.f - powf(A.b1, t), bc2 = 1.f - powf(A.b2, t);
    const float step_size = A.lr / bc1, bc2_sqrt = sqrtf(bc2);
    const int64_t total = A.start[A.nt];
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        int k = 0;
#pragma unroll
        for (int j = 1; j < ADAM_MAXT; ++j)
            if (j < A.nt && e >= A.start[j]) k = j;
        // (selects, not A.p[k]: indexing a kernel argument with a run-time value puts the struct into scratch)
        float *pp = A.p[0], *mm = A.m[0], *vv = A.v[0];
        const float *gg = A.g[0];
        float wd = A.wd[0];
        int64_t s0 = A.start[0];
#pragma unroll
        for (int j = 1; j < ADAM_MAXT; ++j)
            if (k == j) {
                pp = A.p[j]; mm = A.m[j]; vv = A.v[j]; gg = A.g[j]; wd = A.wd[j]; s0 = A.start[j];
            }
        const int64_t i = e - s0;
        const float p0 = pp[i];
        float g = gg[i];
        if (wd != 0.f) g = g + wd * p0;
        float m = mm[i], v = vv[i];
        m = m + (1.f - A.b1) * (g - m);
        v = A.b2 * v + (1.f - A.b2) * g * g;
        mm[i] = m;
        vv[i] = v;
        pp[i] = p0 - step_size * (m / (sqrtf(v) / bc2_sqrt + A.eps));
    }
    if (last_arriver(ticket, gridDim.x) && threadIdx.x == 0) {
        step[0] = t;
        *ticket = 0u;
    }
}

}  // namespace dcr

extern "C" int dcr_nll_picked_mean_fwd_f32_dev(const float *lp, int64_t ld, const int64_t *y, int64_t m, int classes, float *out_loss,
                                               void *ws, void *hip_stream) {
    if (!lp || !y || !out_loss || !ws || ((uintptr_t)ws & 7) || m <= 0 || classes < 1 || ld < classes)
        DCR_FAIL(DCR_EINVAL, "bad nll arguments (a workspace of dcr_head_workspace bytes)");
    int64_t blocks = (m + 255) / 256;
    if (blocks > dcr::PICKED_BLOCKS) blocks = dcr::PICKED_BLOCKS;
    hipLaunchKernelGGL(dcr::k_picked_mean_fwd, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, lp, ld, y, m, classes,
                       out_loss, (dcr::HeadWs *)ws);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

extern "C" int dcr_nll_picked_mean_bwd_f32_dev(const int64_t *y, int64_t m, int classes, const float *g, float *grad, void *hip_stream) {
    if (!y || !g || !grad || m <= 0 || classes < 1) DCR_FAIL(DCR_EINVAL, "bad nll arguments");
    const int64_t blocks = (m * classes + 255) / 256;
    hipLaunchKernelGGL(dcr::k_picked_mean_bwd, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, y, m, classes, g, grad);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

extern "C" int dcr_count_argmax_equal_f32_dev(const float *lp, int64_t ld, const int64_t *y, int64_t m, int classes, int64_t *out_count,
                                              void *hip_stream) {
    if (!out_count || m < 0 || classes < 1 || ld < classes || (m > 0 && (!lp || !y))) DCR_FAIL(DCR_EINVAL, "bad accuracy arguments");
    DCR_HIP(hipMemsetAsync(out_count, 0, sizeof(int64_t), (hipStream_t)hip_stream));
    if (m == 0) return DCR_OK;
    int64_t blocks = (m + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(dcr::k_count_argmax_equal, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, lp, ld, y, m, classes,
                       (unsigned long long *)out_count);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

extern "C" int dcr_adam_step_f32_dev(int n_tensors, void *const *params, const void *const *grads, void *const *exp_avg, void *const *exp_avg_sq,
                                     const int64_t *numel, const float *weight_decay, double lr, double beta1, double beta2, double eps,
                                     float *step_dev, uint32_t *ticket_dev, void *hip_stream) {
    if (n_tensors < 1 || n_tensors > dcr::ADAM_MAXT || !params || !grads || !exp_avg || !exp_avg_sq || !numel || !weight_decay || !step_dev || !ticket_dev)
        DCR_FAIL(DCR_EINVAL, "bad adam_step arguments (1..8 tensors per call)");
    dcr::AdamArgs A;
    A.nt = n_tensors;
    A.start[0] = 0;
    for (int t = 0; t < dcr::ADAM_MAXT; ++t) {
        const bool live = t < n_tensors;
        if (live && (!params[t] || !grads[t] || !exp_avg[t] || !exp_avg_sq[t] || numel[t] < 0)) DCR_FAIL(DCR_EINVAL, "bad adam_step tensor");
        A.p[t] = live ? (float *)params[t] : nullptr;
        A.g[t] = live ? (const float *)grads[t] : nullptr;
        A.m[t] = live ? (float *)exp_avg[t] : nullptr;
        A.v[t] = live ? (float *)exp_avg_sq[t] : nullptr;
        A.wd[t] = live ? weight_decay[t] : 0.f;
        A.start[t + 1] = A.start[t] + (live ? numel[t] : 0);
    }
    A.lr = (float)lr; A.b1 = (float)beta1; A.b2 = (float)beta2; A.eps = (float)eps;
    int64_t blocks = (A.start[n_tensors] + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(dcr::k_adam_multi, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, A, step_dev, ticket_dev);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

extern "C" int dcr_head_workspace(int64_t *bytes) {
    if (!bytes) DCR_FAIL(DCR_EINVAL, "bad head_workspace arguments");
    *bytes = (int64_t)sizeof(dcr::HeadWs);
    return DCR_OK;
}

extern "C" int dcr_head_fwd_f32_dev(const float *o_train, int64_t ld_train, const int64_t *y_train, int64_t m_train, const float *o_eval,
                                    int64_t ld_eval, const int64_t *y_eval, int64_t m_eval, int classes, float *out_loss,
                                    int64_t *out_correct, void *ws, int64_t ws_bytes, void *hip_stream) {
    if (m_train < 0 || m_eval < 0 || (m_train == 0 && m_eval == 0) || classes < 1 || classes > dcr::HEAD_MAXC || !ws ||
        ws_bytes < (int64_t)sizeof(dcr::HeadWs) || ((uintptr_t)ws & 7))
        DCR_FAIL(DCR_EINVAL, "bad head_fwd arguments (1..32 classes, a workspace of dcr_head_workspace bytes)");
    if ((m_train > 0 && (!o_train || !y_train || !out_loss || ld_train < classes)) || (m_eval > 0 && (!o_eval || !y_eval || !out_correct || ld_eval < classes)))
        DCR_FAIL(DCR_EINVAL, "bad head_fwd arguments");
    const int nb_tr = m_train > 0 ? dcr::head_blocks(m_train) : 0, nb_ev = m_eval > 0 ? dcr::head_blocks(m_eval) : 0;
    hipStream_t st = (hipStream_t)hip_stream;
    if (classes <= 8)
        hipLaunchKernelGGL((dcr::k_head_fwd<8>), dim3((unsigned)(nb_tr + nb_ev)), dim3(256), 0, st, o_train, ld_train, y_train, m_train, nb_tr, o_eval,
                           ld_eval, y_eval, m_eval, nb_ev, classes, out_loss, (long long *)out_correct, (dcr::HeadWs *)ws);
    else if (classes <= 16)
        hipLaunchKernelGGL((dcr::k_head_fwd<16>), dim3((unsigned)(nb_tr + nb_ev)), dim3(256), 0, st, o_train, ld_train, y_train, m_train, nb_tr, o_eval,
                           ld_eval, y_eval, m_eval, nb_ev, classes, out_loss, (long long *)out_correct, (dcr::HeadWs *)ws);
    else
        hipLaunchKernelGGL((dcr::k_head_fwd<32>), dim3((unsigned)(nb_tr + nb_ev)), dim3(256), 0, st, o_train, ld_train, y_train, m_train, nb_tr, o_eval,
                           ld_eval, y_eval, m_eval, nb_ev, classes, out_loss, (long long *)out_correct, (dcr::HeadWs *)ws);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

extern "C" int dcr_head_bwd_f32_dev(const float *o_train, int64_t ld_train, const int64_t *y_train, int64_t m_train, int classes, const float *g,
                                    float *grad, float *grad_bias, void *ws, int64_t ws_bytes, void *hip_stream) {
    if (!o_train || !y_train || !g || !grad || m_train <= 0 || classes < 1 || classes > dcr::HEAD_MAXC || ld_train < classes || !ws ||
        ws_bytes < (int64_t)sizeof(dcr::HeadWs) || ((uintptr_t)ws & 7))
        DCR_FAIL(DCR_EINVAL, "bad head_bwd arguments");
    const int nb = dcr::head_blocks(m_train);
    hipStream_t st = (hipStream_t)hip_stream;
    if (classes <= 8)
        hipLaunchKernelGGL((dcr::k_head_bwd<8>), dim3((unsigned)nb), dim3(256), 0, st, o_train, ld_train, y_train, m_train, classes, g, grad, grad_bias,
                           (dcr::HeadWs *)ws);
    else if (classes <= 16)
        hipLaunchKernelGGL((dcr::k_head_bwd<16>), dim3((unsigned)nb), dim3(256), 0, st, o_train, ld_train, y_train, m_train, classes, g, grad, grad_bias,
                           (dcr::HeadWs *)ws);
    else
        hipLaunchKernelGGL((dcr::k_head_bwd<32>), dim3((unsigned)nb), dim3(256), 0, st, o_train, ld_train, y_train, m_train, classes, g, grad, grad_bias,
                           (dcr::HeadWs *)ws);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

extern "C" int dcr_act_linear_fwd_f32_dev(const float *x, const float *w, float *h_train, float *z_train, float *z_eval, int64_t ldz,
                                          uint64_t *bits, int64_t n_rows, int hidden, int classes, double p, uint64_t seed,
                                          uint64_t offset, const uint64_t *offset_dev, void *hip_stream) {
    const bool train = z_train != nullptr, eval = z_eval != nullptr;
    if (!x || !w || n_rows < 0 || (!train && !eval)) DCR_FAIL(DCR_EINVAL, "bad act_linear arguments");
    if (train && (!bits || !(p >= 0.0 && p < 1.0))) DCR_FAIL(DCR_EINVAL, "act_linear: training output needs bits and 0 <= p < 1");
    if ((hidden != 64 && hidden != 128) || classes < 1 || classes > 16 || ldz < classes)
        DCR_FAIL(DCR_EINVAL, "act_linear: hidden width 64 or 128, at most 16 classes, ldz >= classes (other shapes take the separate kernels)");
    if (((uintptr_t)x & 15) || ((uintptr_t)w & 15) || (h_train && ((uintptr_t)h_train & 15)))
        DCR_FAIL(DCR_EINVAL, "act_linear: 16-byte aligned tensors expected");
    if (n_rows == 0) return DCR_OK;
    const uint32_t threshold = dcr::dropout_threshold16(p);
    const float scale = (float)(1.0 / (1.0 - p));
    if (hidden == 128)
        dcr::launch_act_linear_fwd<8>(train, eval, x, w, h_train, z_train, z_eval, ldz, (unsigned long long *)bits, n_rows, classes, scale, threshold,
                                       seed, offset, offset_dev, (hipStream_t)hip_stream);
    else
        dcr::launch_act_linear_fwd<4>(train, eval, x, w, h_train, z_train, z_eval, ldz, (unsigned long long *)bits, n_rows, classes, scale, threshold,
                                       seed, offset, offset_dev, (hipStream_t)hip_stream);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

static int64_t act_linear_bwd_blocks(int64_t n_rows, int hidden) {
    (void)hidden;
    int64_t blocks = (n_rows + 255) / 256;  // a workgroup per 256-row tile
    if (blocks > 256 * 64) blocks = 256 * 64;
    return blocks < 1 ? 1 : blocks;
}

extern "C" int dcr_act_linear_bwd_workspace(int64_t n_rows, int hidden, int64_t *floats) {
    if (!floats || n_rows < 0 || (hidden != 64 && hidden != 128)) DCR_FAIL(DCR_EINVAL, "bad act_linear_bwd_workspace arguments");
    *floats = act_linear_bwd_blocks(n_rows, hidden) * hidden;
    return DCR_OK;
}

static int64_t act_linear_bwd_fused_blocks(int64_t n_rows) {
    int64_t blocks = (n_rows + 255) / 256;
    if (blocks > 1024) blocks = 1024;  // grid-stride: a part of H + 16 H floats per workgroup
    return blocks < 1 ? 1 : blocks;
}

extern "C" int dcr_act_linear_bwd_fused_workspace(int64_t n_rows, int hidden, int64_t *floats) {
    if (!floats || n_rows < 0 || (hidden != 64 && hidden != 128)) DCR_FAIL(DCR_EINVAL, "bad act_linear_bwd_fused_workspace arguments");
    *floats = act_linear_bwd_fused_blocks(n_rows) * 17 * hidden;
    return DCR_OK;
}

extern "C" int dcr_act_linear_bwd_fused_f32_dev(const float *dz, const float *w, const uint64_t *bits, const float *x, float *dx,
                                                float *dw, float *colsum, float *ws, int64_t ws_floats, int64_t n_rows, int hidden,
                                                int classes, double p, void *hip_stream) {
    if (!dz || !w || !bits || !x || !dx || !dw || !colsum || !ws || n_rows < 0 || !(p >= 0.0 && p < 1.0))
        DCR_FAIL(DCR_EINVAL, "bad act_linear_bwd_fused arguments");
    if ((hidden != 64 && hidden != 128) || classes < 1 || classes > 16) DCR_FAIL(DCR_EINVAL, "act_linear_bwd_fused: unsupported shape");
    if (((uintptr_t)dx & 15) || ((uintptr_t)w & 15) || ((uintptr_t)x & 15)) DCR_FAIL(DCR_EINVAL, "act_linear_bwd_fused: 16-byte aligned tensors expected");
    const int64_t blocks = act_linear_bwd_fused_blocks(n_rows);
    if (ws_floats < blocks * 17 * hidden) DCR_FAIL(DCR_EINVAL, "act_linear_bwd_fused: workspace too small (dcr_act_linear_bwd_fused_workspace)");
    hipStream_t st = (hipStream_t)hip_stream;
    if (n_rows == 0) {
        DCR_HIP(hipMemsetAsync(colsum, 0, sizeof(float) * hidden, st));
        DCR_HIP(hipMemsetAsync(dw, 0, sizeof(float) * hidden * classes, st));
        return DCR_OK;
    }
    const float scale = (float)(1.0 / (1.0 - p));
    if (hidden == 128)
        hipLaunchKernelGGL((dcr::k_act_linear_bwd_fused<2>), dim3((unsigned)blocks), dim3(256), 0, st, dz, w, (const unsigned long long *)bits, x,
                           dx, n_rows, classes, scale, ws);
    else
        hipLaunchKernelGGL((dcr::k_act_linear_bwd_fused<1>), dim3((unsigned)blocks), dim3(256), 0, st, dz, w, (const unsigned long long *)bits, x,
                           dx, n_rows, classes, scale, ws);
    // parts -> colsum[hidden] and dw[classes][hidden]: the first hidden * (1 + classes) columns of the [blocks][17 * hidden] parts
    hipLaunchKernelGGL(dcr::k_parts_finish, dim3((unsigned)(hidden * (1 + classes))), dim3(256), 0, st, ws, blocks, 17 * hidden, hidden, colsum, dw);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

static int act_linear_bwd(const float *dz, const float *w, const uint64_t *bits, float *dx, float *colsum, float *ws, int64_t ws_floats,
                          int64_t n_rows, int hidden, int classes, double p, void *hip_stream);

extern "C" int dcr_act_linear_bwd_f32_dev(const float *dz, const float *w, const uint64_t *bits, float *dx, int64_t n_rows, int hidden,
                                          int classes, double p, void *hip_stream) {
    return act_linear_bwd(dz, w, bits, dx, nullptr, nullptr, 0, n_rows, hidden, classes, p, hip_stream);
}

extern "C" int dcr_act_linear_bwd_colsum_f32_dev(const float *dz, const float *w, const uint64_t *bits, float *dx, float *colsum,
                                                 float *ws, int64_t ws_floats, int64_t n_rows, int hidden, int classes, double p,
                                                 void *hip_stream) {
    if (!colsum || !ws) DCR_FAIL(DCR_EINVAL, "act_linear_bwd_colsum: colsum and workspace expected");
    return act_linear_bwd(dz, w, bits, dx, colsum, ws, ws_floats, n_rows, hidden, classes, p, hip_stream);
}

static int act_linear_bwd(const float *dz, const float *w, const uint64_t *bits, float *dx, float *colsum, float *ws, int64_t ws_floats,
                          int64_t n_rows, int hidden, int classes, double p, void *hip_stream) {
    if (!dz || !w || !bits || !dx || n_rows < 0 || !(p >= 0.0 && p < 1.0)) DCR_FAIL(DCR_EINVAL, "bad act_linear_bwd arguments");
    if ((hidden != 64 && hidden != 128) || classes < 1 || classes > 16) DCR_FAIL(DCR_EINVAL, "act_linear_bwd: unsupported shape");
    if (((uintptr_t)dx & 15) || ((uintptr_t)w & 15)) DCR_FAIL(DCR_EINVAL, "act_linear_bwd: 16-byte aligned tensors expected");
    const int64_t blocks = act_linear_bwd_blocks(n_rows, hidden);
    if (colsum && ws_floats < blocks * hidden) DCR_FAIL(DCR_EINVAL, "act_linear_bwd_colsum: workspace too small (dcr_act_linear_bwd_workspace)");
    if (n_rows == 0) {
        if (colsum) DCR_HIP(hipMemsetAsync(colsum, 0, sizeof(float) * hidden, (hipStream_t)hip_stream));
        return DCR_OK;
    }
    const float scale = (float)(1.0 / (1.0 - p));
    if (hidden == 128)
        hipLaunchKernelGGL((dcr::k_act_linear_bwd<32>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, dz, w,
                           (const unsigned long long *)bits, dx, n_rows, classes, scale, colsum ? ws : nullptr);
    else
        hipLaunchKernelGGL((dcr::k_act_linear_bwd<16>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, dz, w,
                           (const unsigned long long *)bits, dx, n_rows, classes, scale, colsum ? ws : nullptr);
    if (colsum)
        hipLaunchKernelGGL(dcr::k_colsum_finish, dim3((unsigned)hidden), dim3(256), 0, (hipStream_t)hip_stream, ws, blocks, hidden, colsum);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}
