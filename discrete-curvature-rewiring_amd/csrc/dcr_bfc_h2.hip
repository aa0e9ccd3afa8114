// Two-hop curvature pass of libdcr_hip.so: full Balanced Forman passes from row u of A·A instead of per-edge
// neighbourhood streaming (round 3: rebuilt around Bloom bitmaps; the round-2 hash-map version of this file was slower
// than the node-centric kernels and is gone).
//
// Replaces compute_curvature_graph(G, 'bfc') at rewiring/sdrf_no_cuda.py:24, i.e. E calls of bfc_naive.bfc_edge
// (curvature/bfc_naive.py:7-40), with the same integers and the same float64 closing expression as the other two
// implementations (dcr_bfc_nc.hip, dcr_bfc.hip) — only the way the integers are counted differs.
//
// For an edge {u,v}: DX = N(u) \ N(v) \ {v}, DY = N(v) \ N(u) \ {u}.  bfc_naive.py:26-29,36-37 needs, for every w in DY,
// c(w) = |N(w) ∩ DX| (|sq2| = how many are positive, gamma = the largest; the same from v's side gives |sq1|).  Now
//
//     c(w) = |N(w) ∩ N(u)|  -  1  -  |N(w) ∩ N(u) ∩ N(v)|
//
// (v itself is a common neighbour of w and u; the last term are the triangle partners of {u,v} adjacent to w).  The first
// term M_u(w) does not depend on v: it is row u of A·A, the number of times w is met when the rows of the neighbours of
// u are read once.  The node-centric kernels find it by intersecting N(w) with N(u) for every (edge, w): 1.05 G adjacency
// entries per pass on the 100k-node bench graph; here every node reads its neighbours' rows: Σ d² = 0.117 G entries.
//
// 97.6 % of the 2-hop keys of a node occur once (c = 0: nothing to count) and only 5 % of the entries belong to keys
// that repeat, so exact state is kept for those only:
//   A. first sweep of the neighbours' rows: test-and-set one bit per entry in a Bloom bitmap B1 (LDS, ~16 bits per
//      entry); an entry that finds its bit set is a repeat (or, rarely, a collision) and sets the bit of a second,
//      smaller bitmap B2.  No table, no queue, one LDS atomic per entry;
//   B. second sweep: an entry whose B2 bit is set — every occurrence of every repeated key, first ones included, plus a
//      few collisions — goes to an exact table EX of (key → rows that hold it); the members of N(u) are seeded into
//      B1, B2 and EX beforehand, flagged, so a hit on one of them is a triangle (bfc_naive.py:25);
//   C. with EX complete, c(w) for the occurrence of w in row i is |rows(w) \ {i} \ rows adjacent to row i|.
// Nodes of at most 64 neighbours (97 % of the bench graph's nodes, 85 % of its entries) are taken by one wave each:
// rows(w) is a 64-bit mask, the rows adjacent to row i (the triangle partners of edge {u, v_i}) another, the B-sweep
// leaves a short list of candidate occurrences and step C is one pass over that list — no third sweep, no edge-set
// probes.  Larger nodes are taken by a workgroup with a counting table (key → occurrences) and a third sweep for the
// per-row statistics; the triangle term is subtracted per edge with triangles AND positive counts by probing an edge
// hash set in device memory; hubs whose repeated keys exceed the table are split by key hash into partitions (units of
// their own, results met by integer atomics).  A node whose tables fill up (dense neighbourhoods: sizes are typical,
// not worst case) is put on a retry list and redone by the largest class with worst-case partitions; only if that fails
// too does the whole pass fall back to the node-centric kernels.
// Each node writes, per adjacency slot u->v, {|sq| on v's side, max count, T, reverse slot}; a final kernel joins the two
// records of an edge and evaluates the float64 closing expression in the reference's order (bfc_naive.py:31-40).
// Bounds: HBM / L2 row streaming (2-3 x 4 B x Σ d² per pass) and LDS atomics; no MFMA (integer set counting).
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dcr_bfc_common.h"

namespace dcr {

constexpr unsigned H2_EMPTY = 0xFFFFFFFFu;
constexpr unsigned H2_NBR = 0x80000000u;  // on a key of the small classes' EX: member of N(u) (node ids stay below 2^30)
constexpr int H2_CLASSES = 5;             // 0-2: one wave per node (<= 64 neighbours), 3-4: one workgroup per unit
constexpr int H2_WB = 4;                  // weight buckets per class (units are laid out heaviest bucket first)
// third word of an edge's record: the triangle count with the degree of the row's node above it (both below 2^16: H2_MAXDEG).
// The closing kernel reads the OTHER endpoint's degree out of the partner record it fetches anyway, instead of a random read of
// that node's row header: one random read per edge is left of the four it made in round 3.
__device__ inline unsigned h2_rec_t(int T, int deg) { return (unsigned)T | ((unsigned)deg << 16); }
static_assert(H2_MAXDEG < 65536, "record packing");
constexpr int H2_SMALL_DEG = 64;
#ifndef H2_Q
#define H2_Q 2                            // 16-byte pieces per lane in flight in the streaming loops
#endif
#ifndef H2_QL
#define H2_QL 2                           // the same for the split class (16 waves per unit, a few pieces per lane and sweep)
#endif
constexpr int H2_QCAP = 128;              // queued exact-path items per wave (worked off when fewer than 64 slots are left)
__host__ __device__ constexpr int h2_wpb(int c) { return c == 2 ? 2 : 4; }  // waves (= nodes in flight) per workgroup of the wave classes

// per class: log2 of the bits of B1; largest weight W = Σ neighbour degrees (the entries of one sweep)
__host__ __device__ constexpr int h2_l1(int c) { return c == 0 ? 14 : c == 1 ? 15 : c == 2 ? 16 : c == 3 ? 16 : 17; }
__host__ __device__ constexpr int h2_maxw(int c) { return c == 0 ? 1024 : c == 1 ? 2048 : c == 2 ? 4096 : c == 3 ? 8192 : INT_MAX; }
__host__ __device__ constexpr int h2_exs(int c) { return c == 0 ? 128 : c == 1 ? 256 : c == 2 ? 512 : c == 3 ? 4096 : 8192; }
__host__ __device__ constexpr int h2_clcap(int c) { return c == 0 ? 192 : c == 1 ? 384 : 768; }
__host__ __device__ constexpr int h2_waves(int c) { return c == 3 ? 4 : 16; }
__host__ __device__ constexpr int h2_keycap(int c) { return c == 3 ? 2800 : 5500; }  // keys a block table takes (4-slot buckets)
constexpr int H2_PLCAP = 192;              // triangle partners of one batch of rows kept in LDS (more: their rows are read again)
constexpr int H2_WALK = 32;                // longest probe sequence of the exact tables

__device__ inline void h2_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int NW>
__device__ inline void h2_sync() {
    if (NW == 1) h2_wave_sync();
    else __syncthreads();
}

// ---- hashing: Fibonacci hashing of the low 24 bits with the full-rate 24-bit multiply (see dcr_bfc_nc.hip) ----------
__device__ inline unsigned h2_mul24(unsigned key) {
    unsigned prod;
    asm("v_mul_u32_u24 %0, 0x9e3779, %1" : "=v"(prod) : "v"(key));
    return prod;
}
__device__ inline unsigned h2_mul24b(unsigned key) {  // an independent multiplier for the exact tables
    unsigned prod;
    asm("v_mul_u32_u24 %0, 0x85ebcb, %1" : "=v"(prod) : "v"(key));
    return prod;
}
template <int L1>
__device__ inline unsigned h2_bit(unsigned key) {
    return (h2_mul24(key) >> (24 - L1)) & ((1u << L1) - 1u);
}
// which partition of a split node a key belongs to: a hash independent of the others (NOT a multiplier whose leading digits
// equal those of h2_mul24b: the keys of one partition then share the leading bits of their bucket index and fill 1 / nparts
// of the table)
__device__ inline int h2_part(unsigned key, int nparts) {
    return (int)((((key * 0xC2B2AE35u) >> 16) * (unsigned)nparts) >> 16);
}

// ---- the bitmaps ------------------------------------------------------------------------------------------------------
// B1: TWO bits per 2-hop entry in ONE 32-bit word — the word and the first bit from the first hash, the second bit from an
// independent one (a blocked Bloom filter); "seen" = both were set; B2 (a quarter of the bits, indexed by the first hash):
// seen again.  (Round 4: with one bit per entry in 16, one key in sixteen that occurs ONCE found its bit set by another key
// and went down the exact path — half of all exact-path items, and the exact tables of the heaviest nodes of every wave class
// ran at 85 % load; with two bits a singleton needs both taken: 1-2 %.  Both bits go in ONE atomic: two atomics were tried
// first and were WRONG — two lanes holding the same key in one instruction are served in an order of the hardware's choosing,
// not necessarily the same for the second atomic, and then neither lane sees both bits set.)
__device__ inline unsigned h2_mul24c(unsigned key) {  // a third multiplier: independent of the bitmaps' first hash and of the tables'
    unsigned prod;
    asm("v_mul_u32_u24 %0, 0xb55a4f, %1" : "=v"(prod) : "v"(key));
    return prod;
}
// the entry's bits inside word (bit index >> 5) of B1
__device__ inline unsigned h2_word_mask(unsigned key, unsigned b) {
    unsigned m = 1u << (b & 31u);
    m |= 1u << ((h2_mul24c(key) >> 19) & 31u);
    return m;
}
template <int L1>
__device__ inline void h2_seed(unsigned *b1, unsigned *b2, unsigned key) {  // a member of N(u): every occurrence is exact
    const unsigned b = h2_bit<L1>(key);
    atomicOr(&b1[b >> 5], h2_word_mask(key, b));
    const unsigned c = b >> 2;
    atomicOr(&b2[c >> 5], 1u << (c & 31u));
}
__device__ inline bool h2_again(const unsigned *b2, unsigned b) {
    const unsigned c = b >> 2;
    return (b2[c >> 5] >> (c & 31u)) & 1u;
}
// The four entries of a piece at once, branch-free up to the rare second step: entry by entry, every returning atomic was
// followed by a wait and a branch (20 round trips of LDS latency per sweep of a small node).  `valid`: 4-bit mask.
template <int L1>
__device__ inline void h2_mark4(unsigned *b1, unsigned *b2, const unsigned kk[4], unsigned valid) {
    unsigned b[4], m[4], old[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        b[jj] = h2_bit<L1>(kk[jj]);
        m[jj] = ((valid >> jj) & 1u) ? h2_word_mask(kk[jj], b[jj]) : 0u;  // (no bit for an entry that does not count: the atomic changes nothing)
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) old[jj] = atomicOr(&b1[b[jj] >> 5], m[jj]);
    unsigned any = 0u;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        old[jj] = (m[jj] != 0u && (old[jj] & m[jj]) == m[jj]) ? 1u : 0u;
        any |= old[jj];
    }
    if (any) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            if (old[jj]) {
                const unsigned c = b[jj] >> 2;
                atomicOr(&b2[c >> 5], 1u << (c & 31u));
            }
    }
}
// which of the four entries have their B2 bit set (four independent reads)
template <int L1>
__device__ inline unsigned h2_again4(const unsigned *b2, const unsigned kk[4], unsigned valid) {
    unsigned c[4], wd[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        c[jj] = h2_bit<L1>(kk[jj]) >> 2;
        wd[jj] = b2[c[jj] >> 5];
    }
    unsigned f = 0u;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) f |= ((wd[jj] >> (c[jj] & 31u)) & 1u) << jj;
    return f & valid;
}
__device__ inline unsigned h2_eq4(const unsigned kk[4], unsigned u) {
    return (kk[0] == u ? 1u : 0u) | (kk[1] == u ? 2u : 0u) | (kk[2] == u ? 4u : 0u) | (kk[3] == u ? 8u : 0u);
}

// the entry of a piece that the one-hot 4-bit `b` names: three selects (written as a chain of b == 1, b == 2, ... it is
// compiled into a switch: three branches per entry)
__device__ inline unsigned h2_pick4(const int4 w, unsigned b) {
    const int lo = (b & 1u) ? w.x : w.y, hi = (b & 4u) ? w.z : w.w;
    return (unsigned)((b & 3u) ? lo : hi);
}

__device__ inline unsigned h2_piece_mask(int a, int lo, int hi) {
    const int s = lo - a, t = hi - a;
    const unsigned head = s > 0 ? (0xFu << s) & 0xFu : 0xFu;
    const unsigned tail = t < 4 ? (1u << t) - 1u : 0xFu;
    return head & tail;
}

// row of piece j of the flat piece list of a batch (same scheme as dcr_bfc_nc.hip: two ballots bracket the rows of a
// 64-piece step, a few shuffles or a short bisection settle the lane's own)
__device__ inline int h2_piece_row(const int *poff, int poff_lane, int j, int j_first, int j_last) {
    const int rf = __popcll(__ballot(poff_lane <= j_first)) - 1;
    const int rl = __popcll(__ballot(poff_lane <= j_last)) - 1;
    int r = rf;
    const int span = rl - rf;
    if (span <= 4) {
        for (int b = rf + 1; b <= rl; ++b) r += (__shfl(poff_lane, b) <= j);
    } else {
        for (int step = span >= 32 ? 32 : span >= 16 ? 16 : span >= 8 ? 8 : 4; step > 0; step >>= 1)
            if (r + step <= rl && poff[r + step] <= j) r += step;
    }
    return r;
}

// The rows of a batch (descriptors and piece prefix sums in LDS) as one flat list of aligned 16-byte pieces shared evenly
// by the 64 lanes.  body(piece, valid-entry mask, row, slot of the piece's first entry) is called by ALL lanes, converged
// (lanes without a piece pass mask 0, row -1).
template <typename Body>
__device__ inline void h2_for_pieces(const int32_t *col, const int2 *desc, const int *poff, int poff_lane, int P, Body body) {
    const int lane = threadIdx.x & 63;
    for (int j0 = 0; j0 < P; j0 += 64 * H2_Q) {
        int4 w[H2_Q];
        int rr[H2_Q], aa[H2_Q];
        unsigned vm[H2_Q];
#pragma unroll
        for (int q = 0; q < H2_Q; ++q) {
            const int j = j0 + 64 * q + lane;
            rr[q] = -1;
            aa[q] = 0;
            vm[q] = 0u;
            w[q] = make_int4(0, 0, 0, 0);
            const int jf = j0 + 64 * q, jl = jf + 63 < P ? jf + 63 : P - 1;
            if (jf >= P) continue;  // uniform
            const int r = h2_piece_row(poff, poff_lane, j < P ? j : jl, jf, jl);
            if (j < P) {
                const int2 d = desc[r];
                const int a = (d.x & ~3) + 4 * (j - poff[r]);
                w[q] = load_piece(col, a);
                rr[q] = r;
                aa[q] = a;
                vm[q] = h2_piece_mask(a, d.x, d.x + d.y);
            }
        }
#pragma unroll
        for (int q = 0; q < H2_Q; ++q) {
            if (j0 + 64 * q >= P) continue;  // uniform
            body(w[q], vm[q], rr[q], aa[q]);
        }
    }
}

// The same with the exact-path queue: flags(piece, mask, row, slot) -> which of the four entries go to the queue;
// push(index, key, row) stores one; drain() works the queue off and resets qn.  The drain is called from ONE place per
// iteration (inlined at every entry position it was 4 x H2_Q copies of the table walks per sweep, and the kernels
// outgrew the instruction cache: 135-190 KB each).
template <int Q, typename Flags, typename Push, typename Drain>
__device__ inline void h2_for_pieces_queued(const int32_t *col, const int2 *desc, const int *poff, int poff_lane, int P, int &qn,
                                            Flags flags, Push push, Drain drain) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll 1
    for (int j0 = 0; j0 < P; j0 += 64 * Q) {
        int4 w[Q];
        int rr[Q];
        unsigned fl[Q];
        unsigned anyf = 0u;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int j = j0 + 64 * q + lane;
            rr[q] = -1;
            fl[q] = 0u;
            w[q] = make_int4(0, 0, 0, 0);
            const int jf = j0 + 64 * q, jl = jf + 63 < P ? jf + 63 : P - 1;
            if (jf >= P) continue;  // uniform
            const int r = h2_piece_row(poff, poff_lane, j < P ? j : jl, jf, jl);
            int a = 0;
            unsigned vm = 0u;
            if (j < P) {
                const int2 d = desc[r];
                a = (d.x & ~3) + 4 * (j - poff[r]);
                w[q] = load_piece(col, a);
                rr[q] = r;
                vm = h2_piece_mask(a, d.x, d.x + d.y);
            }
            fl[q] = flags(w[q], vm, rr[q], a);
            anyf |= fl[q];
        }
        if (__ballot(anyf != 0u) == 0ull) continue;  // uniform
#pragma unroll 1
        while (true) {
            bool stop = false;  // uniform: the queue is full, the rest waits for the drain
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const unsigned kk[4] = {(unsigned)w[q].x, (unsigned)w[q].y, (unsigned)w[q].z, (unsigned)w[q].w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const bool p = (fl[q] >> jj) & 1u;
                    const unsigned long long m = __ballot(p);
                    if (m == 0ull) continue;  // uniform
                    if (stop || qn + __popcll(m) > H2_QCAP) {
                        stop = true;
                        continue;
                    }
                    if (p) {
                        push(qn + __popcll(m & below), kk[jj], rr[q]);
                        fl[q] &= ~(1u << jj);
                    }
                    qn += __popcll(m);
                }
            }
            if (!stop) break;
            drain();
        }
    }
}

// piece counts of the rows held by the lanes -> exclusive prefix in `excl`, total returned
__device__ inline int h2_prefix(int np, int &excl) {
    const int lane = threadIdx.x & 63;
    int incl = np;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    excl = incl - np;
    return __shfl(incl, 63);
}

// The same for the exact-path queue's per-lane counts, in registers alone (h2_prefix goes six times through ds_bpermute, and
// the queue wants its prefix once per node and sweep): shifts by 1, 2, 4, 8 inside each row of 16 lanes, then lane 15 of
// rows 0 and 2 into rows 1 and 3, then lane 31 into rows 2 and 3.
__device__ inline int h2_prefix_dpp(int np, int &excl) {
    int incl = np;
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, false);  // row_shr:1 (lanes without a source add 0)
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, false);  // row_shr:2
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, false);  // row_shr:4
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, false);  // row_shr:8
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xA, 0xF, false);  // row_bcast:15, rows 1 and 3
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xC, 0xF, false);  // row_bcast:31, rows 2 and 3
    excl = incl - np;
    return __builtin_amdgcn_readlane(incl, 63);
}

// ---- the retry list: nodes whose tables filled up in their class -------------------------------------------------------
// partitions of a node in the largest class: `safe` sizes them for the worst case (every key repeats: W / 2 keys, a
// quarter of slack for the partition hash), else for what power-law graphs need (W / 4)
__host__ __device__ inline int h2_parts_for(int d, int64_t W, bool safe) {
    const int64_t room = h2_keycap(4) - d;  // the flagged neighbours live in every partition's table
    if (room <= 0) return 65536;
    const int64_t keys = safe ? W / 2 + W / 8 + 64 : W / 3 + 64;
    int64_t p = (keys + room - 1) / room;
    // ... and B1 wants 8 (16) bits per entry of the partition, or its collisions fill B2 and the table with keys that occur once
    const int64_t per = safe ? (1 << h2_l1(4)) / 16 : (1 << h2_l1(4)) / 8;
    if (p < (W + per - 1) / per) p = (W + per - 1) / per;
    if (p < 1) p = 1;
    if (p > 65535) p = 65536;
    return (int)p;
}
struct H2Retry {
    int4 *units;
    int64_t cap;
    int32_t *weight;  // bit 31: the node is on the list already (several partitions of a split node may fail)
    DevResult *res;
};
__device__ inline void h2_retry_push(const H2Retry rt, int u, int d, int cls) {  // one lane calls this
    atomicAdd(&rt.res->h2_failed[cls], 1);
    const unsigned old = atomicOr(reinterpret_cast<unsigned *>(&rt.weight[u]), 0x80000000u);
    if (old & 0x80000000u) return;
    const int nparts = h2_parts_for(d, (int64_t)old, true);
    const int first = atomicAdd(&rt.res->h2_retry, nparts);
    if (nparts > 65535 || first < 0 || (int64_t)first + nparts > rt.cap) {
        rt.res->h2_status = 1;  // not even the retry list takes it: the pass is redone by the node-centric kernels
        return;
    }
    for (int j = 0; j < nparts; ++j) rt.units[first + j] = make_int4(u, (nparts << 16) | j, 0, 0);
}

// =====================================================================================================================
// wave classes: a node of at most 64 neighbours, by one wave
// =====================================================================================================================
// The LDS of one wave is used in two phases that never overlap (round 4: the arrays of both phases side by side held
// occupancy at 6 / 12 / 20 waves per CU): up to the end of sweep A the first-level bitmap and the row descriptors the
// pieces are addressed with (the pieces themselves are in registers from then on), from sweep B on the exact table, the
// row masks, the queue and the candidate list.  Only the second-level bitmap lives through both.
template <int L1, int EXS, int CLCAP>
struct __attribute__((aligned(16))) H2Small {
    unsigned b2[(1 << (L1 - 2)) / 32];
    union {
        struct {
            unsigned b1[(1 << L1) / 32];   // (directly behind b2: the two are cleared as one range)
            int2 desc[64];
            int poff[66];
        } a;
        struct {
            unsigned exkey[EXS];            // candidate key, or a member of N(u) | H2_NBR
            unsigned exlo[EXS], exhi[EXS];  // candidate: the rows that hold it (64-bit mask); member of N(u): its position in row u
            unsigned adjlo[64], adjhi[64];  // per row i: the rows adjacent to it = triangle partners of edge {u, v_i}
            int pos[64], mx[64];
            unsigned qk[H2_QCAP];
            unsigned short cls[CLCAP];     // candidate occurrences: EX slot ...
            unsigned char qr[H2_QCAP];
            unsigned char clr[CLCAP];      // ... and row
        } b;
    };
    int rev[64];  // per row i: the slot of u in it (found in sweep A, published at the end of the node: outside the phases)
};

template <int EXS>
__device__ inline unsigned h2s_home(unsigned key) {
    constexpr int BITS = __builtin_ctz(EXS);
    return (h2_mul24b(key) >> (24 - BITS)) & (unsigned)(EXS - 1);
}
// slot of w (a plain id), inserting it if absent; -1: table full
template <int EXS>
__device__ inline int h2s_find_or_insert(unsigned *exkey, unsigned w) {
    unsigned s = h2s_home<EXS>(w);
#pragma unroll 1
    for (int walk = 0; walk < EXS; ++walk) {
        const unsigned e = exkey[s];
        if ((e & ~H2_NBR) == w && e != H2_EMPTY) return (int)s;
        if (e == H2_EMPTY) {
            const unsigned old = atomicCAS(&exkey[s], H2_EMPTY, w);
            if (old == H2_EMPTY || (old & ~H2_NBR) == w) return (int)s;
        }
        s = (s + 1) & (unsigned)(EXS - 1);
    }
    return -1;
}
template <int EXS>
__device__ inline int h2s_insert_nbr(unsigned *exkey, unsigned k) {  // the members of N(u) are distinct
    unsigned s = h2s_home<EXS>(k);
#pragma unroll 1
    for (int walk = 0; walk < EXS; ++walk) {
        if (atomicCAS(&exkey[s], H2_EMPTY, k | H2_NBR) == H2_EMPTY) return (int)s;
        s = (s + 1) & (unsigned)(EXS - 1);
    }
    return -1;
}

// ---- the wave classes' forms of h2_mark4 and h2_again4 -----------------------------------------------------------------
// The SAME hashes, words and bits (h2_bit, h2_word_mask, h2_again; the block classes keep the forms above), formed with fewer
// instructions — the three wave-class kernels sit at their vector-issue limit (profiles/h2_sweep_reuse_ab.txt):
//  - the word index and the bit of either bitmap are bit fields of ONE product, h2_mul24(key): one extract each, where
//    h2_bit, a shift and a mask stood;
//  - an entry that does not count takes mask 0 by an AND with its sign-extended valid bit: written as a conditional the
//    second multiply (an asm statement, never speculated) kept it a branch of its own per entry;
//  - the B2 bit of an entry seen before goes in with mask 0 for the other entries of the piece, under the one branch
//    "any of the four": no branch per entry.
template <int L1>
__device__ inline void h2s_mark4(unsigned *b1, unsigned *b2, const unsigned kk[4], unsigned valid) {
    unsigned p[4], m[4], old[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        p[jj] = h2_mul24(kk[jj]);
        const unsigned both = (1u << ((p[jj] >> (24 - L1)) & 31u)) | (1u << ((h2_mul24c(kk[jj]) >> 19) & 31u));
        m[jj] = both & (unsigned)__builtin_amdgcn_sbfe((int)valid, (unsigned)jj, 1u);
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) old[jj] = atomicOr(&b1[__builtin_amdgcn_ubfe(p[jj], 29 - L1, L1 - 5)], m[jj]);
    bool seen[4], any = false;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        seen[jj] = m[jj] != 0u && (old[jj] & m[jj]) == m[jj];
        any |= seen[jj];
    }
    if (any) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            atomicOr(&b2[__builtin_amdgcn_ubfe(p[jj], 31 - L1, L1 - 7)], seen[jj] ? 1u << ((p[jj] >> (26 - L1)) & 31u) : 0u);
    }
}
// the B2 bits of the four entries (the caller masks them with the entries that count)
template <int L1>
__device__ inline unsigned h2s_again4(const unsigned *b2, const unsigned kk[4]) {
    unsigned p[4], wd[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        p[jj] = h2_mul24(kk[jj]);
        wd[jj] = b2[__builtin_amdgcn_ubfe(p[jj], 31 - L1, L1 - 7)];
    }
    unsigned f = 0u;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) f |= __builtin_amdgcn_ubfe(wd[jj], __builtin_amdgcn_ubfe(p[jj], 26 - L1, 5), 1u) << jj;
    return f;
}
// (The piece-to-row search stays h2_piece_row, from scratch per 64-piece step: bracketing step q + 1 from the last row of step
//  q saves a ballot and RAISED the vector + scalar instructions per launch of all three kernels — built, measured, dropped.)

// k, rk: the lane's member of N(u) and its row (loaded ahead by the caller); NP: 64-piece steps a node of this class can
// have — all pieces of the node stay in registers and serve both sweeps; mid(): called once between the sweeps (the
// caller's prefetch of the next node)
template <int L1, int EXS, int CLCAP, int NP, typename Mid>
__device__ inline void h2s_node(const View &g, int u, int2 ru, int k, int2 rk, H2Small<L1, EXS, CLCAP> *s, uint4 *rec,
                                const H2Retry rt, Mid mid) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    {   // clear: both bitmaps to zero (the second phase's arrays are set up between the sweeps)
        uint4 *z = reinterpret_cast<uint4 *>(s->b2);
        constexpr int NZ = ((1 << L1) / 32 + (1 << (L1 - 2)) / 32) / 4;  // b2, then b1 directly behind it
        using Lds = H2Small<L1, EXS, CLCAP>;
        static_assert(__builtin_offsetof(Lds, a) == sizeof(unsigned) * ((1 << (L1 - 2)) / 32), "b1 directly behind b2");
        for (int i = lane; i < NZ; i += 64) z[i] = make_uint4(0u, 0u, 0u, 0u);
        s->rev[lane] = -1;  // (written in sweep A, read when the node is published: no clear in between resets it)
    }
    h2_wave_sync();
    // the members of N(u): seeded into both bitmaps (into the exact table between the sweeps)
    bool full = false;
    if (lane >= ru.y || k < 0 || k >= g.n || k == u) {
        k = -1;
        rk = make_int2(0, 0);
    } else {
        if (!row_ok(g, rk, 32, k, u)) rk = make_int2(0, 0);
        h2_seed<L1>(s->a.b1, s->b2, (unsigned)k);
    }
    const int np = rk.y > 0 ? ((rk.x + rk.y + 3) >> 2) - (rk.x >> 2) : 0;
    int poff_lane;
    const int P = h2_prefix(np, poff_lane);
    s->a.desc[lane] = rk;
    s->a.poff[lane] = poff_lane;
    if (lane == 0) s->a.poff[64] = P;
    h2_wave_sync();
    if (P > 64 * NP) full = true;  // (cannot happen: the class bounds the weight; such a node would be redone elsewhere)
    // every piece of the node is requested at once and kept: meta = valid-entry mask | row << 4.  (The piece's first slot is
    // wanted once per ROW, where u sits in it: sweep A works it out again from the descriptors, still in LDS then, instead of
    // every piece carrying it through both sweeps and the queue loop in a register of its own.)
    int4 w[NP];
    unsigned meta[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int j = 64 * q + lane;
        w[q] = make_int4(0, 0, 0, 0);
        meta[q] = 0u;
        const int jf = 64 * q, jl = jf + 63 < P ? jf + 63 : P - 1;
        if (jf >= P) continue;  // uniform
        const int r = h2_piece_row(s->a.poff, poff_lane, j < P ? j : jl, jf, jl);
        if (j < P) {
            const int2 d = s->a.desc[r];
            const int a = (d.x & ~3) + 4 * (j - s->a.poff[r]);
            w[q] = load_piece(g.col, a);
            meta[q] = h2_piece_mask(a, d.x, d.x + d.y) | ((unsigned)r << 4);
        }
    }
    // sweep A (and, once per row, where u sits in it: the reverse slot of edge {u, v_row})
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        if (64 * q >= P) continue;  // uniform
        const unsigned kk[4] = {(unsigned)w[q].x, (unsigned)w[q].y, (unsigned)w[q].z, (unsigned)w[q].w};
        const unsigned isu = h2_eq4(kk, (unsigned)u) & meta[q] & 0xFu;
        if (isu) {  // (the lane has piece 64 q + lane of row meta >> 4)
            const int r = (int)(meta[q] >> 4);
            s->rev[r] = (s->a.desc[r].x & ~3) + 4 * (64 * q + lane - s->a.poff[r]) + __ffs((int)isu) - 1;
        }
        // u's own entry leaves the piece's valid mask here, for both sweeps: the reverse slot is taken, nothing later reads
        // that bit, and sweep B need not look for u a second time
        meta[q] &= ~isu;
        h2s_mark4<L1>(s->a.b1, s->b2, kk, meta[q] & 0xFu);
    }
    mid();
    h2_wave_sync();  // sweep A is through: b1 and the descriptors are dead, their space becomes the second phase's arrays
    {
        uint4 *k4 = reinterpret_cast<uint4 *>(s->b.exkey);
        for (int i = lane; i < EXS / 4; i += 64) k4[i] = make_uint4(H2_EMPTY, H2_EMPTY, H2_EMPTY, H2_EMPTY);
        uint4 *m4 = reinterpret_cast<uint4 *>(s->b.exlo);  // exlo and exhi are adjacent
        for (int i = lane; i < 2 * EXS / 4; i += 64) m4[i] = make_uint4(0u, 0u, 0u, 0u);
        s->b.adjlo[lane] = 0u;
        s->b.adjhi[lane] = 0u;
        s->b.pos[lane] = 0;
        s->b.mx[lane] = 0;
    }
    h2_wave_sync();
    if (k >= 0) {  // the members of N(u) into the exact table, flagged, with their position in row u
        const int slot = h2s_insert_nbr<EXS>(s->b.exkey, (unsigned)k);
        if (slot < 0) full = true;
        else s->b.exlo[slot] = (unsigned)lane;
    }
    h2_wave_sync();
    // sweep B: entries whose B2 bit is set are queued and settled against the exact table 64 at a time
    int qn = 0, cln = 0;  // uniform
    auto drain = [&]() {
        h2_wave_sync();
        for (int base = 0; base < qn; base += 64) {
            const int i = base + lane;
            bool cand = false;
            int slot = -1, row = 0;
            if (i < qn) {
                const unsigned w = s->b.qk[i];
                row = s->b.qr[i];
                slot = h2s_find_or_insert<EXS>(s->b.exkey, w);
                if (slot < 0) {
                    full = true;
                } else if (s->b.exkey[slot] & H2_NBR) {  // a member of N(u) in row `row`: rows `row` and exlo[slot] are adjacent
                    const unsigned x = s->b.exlo[slot];
                    atomicOr(x < 32u ? &s->b.adjlo[row] : &s->b.adjhi[row], 1u << (x & 31u));
                } else {
                    atomicOr(row < 32 ? &s->b.exlo[slot] : &s->b.exhi[slot], 1u << (row & 31));
                    cand = true;
                }
            }
            const unsigned long long m = __ballot(cand);
            if (cand) {
                const int idx = cln + __popcll(m & below);
                if (idx < CLCAP) {
                    s->b.cls[idx] = (unsigned short)slot;
                    s->b.clr[idx] = (unsigned char)row;
                } else {
                    full = true;
                }
            }
            cln += __popcll(m);
        }
        h2_wave_sync();
        qn = 0;
    };
    unsigned fl[NP];
    int nfl = 0;  // this lane's flagged entries
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        fl[q] = 0u;
        if (64 * q >= P) continue;  // uniform
        const unsigned kk[4] = {(unsigned)w[q].x, (unsigned)w[q].y, (unsigned)w[q].z, (unsigned)w[q].w};
        fl[q] = h2s_again4<L1>(s->b2, kk) & meta[q] & 0xFu;  // (the valid mask is without u's entry since sweep A)
        nfl += __popc(fl[q]);
    }
    // The flagged entries are queued by LANE, not by entry position (one ballot, count and branch per position cost the
    // same 4 x NP times per node whether one entry in twenty is flagged, as on the bench graph, or all of them): one prefix
    // over the lanes' flag counts gives each lane the queue indices of its own entries, which it writes walking the set bits
    // of its flags.  The queue's ORDER is all this changes (lane by lane instead of position by position).  More than H2_QCAP
    // entries go in rounds cut by queue index: round r takes the indices [r x H2_QCAP, (r + 1) x H2_QCAP), and a lane whose
    // run of indices crosses the cut goes on in the next round where it stopped.  The drain has ONE call site (inlined per
    // entry position the kernels outgrew the instruction cache).
    int qi;  // queue index of this lane's next entry, counted from the start of the round; all before it are queued
    const int qtotal = h2_prefix_dpp(nfl, qi);
#pragma unroll 1
    for (int left = qtotal; left > 0; left -= H2_QCAP) {  // uniform
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            if (64 * q >= P) continue;  // uniform
            while (fl[q] != 0u && qi < H2_QCAP) {
                const unsigned b = fl[q] & (0u - fl[q]);  // the lowest flagged entry of the piece
                s->b.qk[qi] = h2_pick4(w[q], b);
                s->b.qr[qi] = (unsigned char)(meta[q] >> 4);
                fl[q] ^= b;
                ++qi;
            }
        }
        qn = left < H2_QCAP ? left : H2_QCAP;
        drain();
        qi -= H2_QCAP;  // (a lane with entries left stands at H2_QCAP or beyond: never below 0 while it has any)
    }
    h2_wave_sync();
    if (__ballot(full) != 0ull) {  // a table or the list filled up: nothing is published, the node is redone elsewhere
        if (lane == 0) h2_retry_push(rt, u, ru.y, L1 == 14 ? 0 : L1 == 15 ? 1 : 2);
        h2_wave_sync();
        return;
    }
    // step C: c(w) for the occurrence of w in row i = the rows that hold w, less row i, less the rows adjacent to row i
    const int cl_n = cln < CLCAP ? cln : CLCAP;
    for (int e = lane; e < cl_n; e += 64) {
        const int slot = s->b.cls[e], row = s->b.clr[e];
        const int c = __popc(s->b.exlo[slot] & ~s->b.adjlo[row]) + __popc(s->b.exhi[slot] & ~s->b.adjhi[row]) - 1;
        if (c > 0) {
            atomicAdd(&s->b.pos[row], 1);
            atomicMax(&s->b.mx[row], c);
        }
    }
    h2_wave_sync();
    if (k >= 0) {
        const int rev = s->rev[lane];
        if (rev < 0 || rev >= g.cap_total) {
            row_ok(g, make_int2(-1, rev), 33, u, k);  // adjacency not symmetric: report, never publish
        } else {
            const int T = __popc(s->b.adjlo[lane]) + __popc(s->b.adjhi[lane]);
            rec[(int64_t)ru.x + lane] = make_uint4((unsigned)s->b.pos[lane], (unsigned)s->b.mx[lane], h2_rec_t(T, ru.y), (unsigned)rev);
        }
    }
    h2_wave_sync();  // the arrays are rewritten by the next node
}

// Units are taken grid-stride from a list laid out heaviest first: every wave gets a similar mix.  A node is a chain of
// dependent device-memory reads (unit -> row of u -> rows of its members -> their pieces) with little to do in between,
// so the chain of the NEXT node is started while the current one is worked on: its unit two nodes ahead, its row at the
// start of this node, the rows' descriptors between the sweeps.
// waves per SIMD the three wave-class kernels are compiled for (registers; their LDS allows as many since the two phases
// share it).  Measured one class at a time (us, S100k; profiles/r04_occupancy_ab.txt): lightest class 5 / 6 / 7 / 8 waves:
// 155 / 153 / 144 / 162 (near its vector-issue limit: more waves buy little); middle 3 / 4 / 5: 158 / 150 / 147;
// heaviest 2 / 3: 142 / 106 (latency-bound: a third wave per SIMD is worth its 40 spilled registers).
#ifndef H2_OCC0
#define H2_OCC0 7
#endif
#ifndef H2_OCC1
#define H2_OCC1 4
#endif
#ifndef H2_OCC2
#define H2_OCC2 3
#endif
template <int L1, int EXS, int CLCAP, int WPB, int NP>
__global__ void __launch_bounds__(64 * WPB, (L1 == 14 ? H2_OCC0 : L1 == 15 ? H2_OCC1 : H2_OCC2)) k_h2_small(View g, const int4 *units, const int32_t *count, int64_t unit_cap,
                                                       uint4 *rec, H2Retry rt) {
    __shared__ H2Small<L1, EXS, CLCAP> sm[WPB];
    // (the wave's index as a scalar in the two lighter classes: the unit walk — `it`, the units two nodes ahead — then lives in
    //  scalar registers instead of vector registers spilled around every node; the heaviest class spilled one more with it)
    const int wid = L1 == 16 ? (int)(threadIdx.x >> 6) : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int total = *count;
    if (total < 0 || total > unit_cap) {
        row_ok(g, make_int2(-1, total), 34, 0, 0);
        return;
    }
    const int64_t stride = (int64_t)gridDim.x * WPB;
    int64_t it = (int64_t)blockIdx.x * WPB + wid;
    const int4 none = make_int4(-1, 0, 0, 0);
    auto unit_ok = [&](const int4 un) {
        return un.x >= 0 && un.x < g.n && un.w > 0 && un.w <= H2_SMALL_DEG && un.z >= 0 && (int64_t)un.z + un.w <= g.cap_total;
    };
    // prologue: this node's unit, row and row descriptors; the next node's unit and row
    int4 un = it < total ? units[it] : none;
    int4 un1 = it + stride < total ? units[it + stride] : none;
    int k = (unit_ok(un) && lane < un.w) ? g.col[un.z + lane] : -1;
    int2 rk = (k >= 0 && k < g.n) ? g.rowinfo[k] : make_int2(0, 0);
    int k1 = (unit_ok(un1) && lane < un1.w) ? g.col[un1.z + lane] : -1;
    for (; it < total; it += stride) {
        const int4 un2 = it + 2 * stride < total ? units[it + 2 * stride] : none;  // two nodes ahead
        int2 rk1 = make_int2(0, 0);
        if (unit_ok(un)) {
            // (the plan read the row of u in this same pass: {start, degree} travel with the unit)
            h2s_node<L1, EXS, CLCAP, NP>(g, un.x, make_int2(un.z, un.w), k, rk, &sm[wid], rec, rt, [&]() {
                rk1 = (k1 >= 0 && k1 < g.n) ? g.rowinfo[k1] : make_int2(0, 0);
            });
        } else {
            if (un.x != -1 || it < total) row_ok(g, make_int2(-1, un.x), 35, (int)it, total);
            rk1 = (k1 >= 0 && k1 < g.n) ? g.rowinfo[k1] : make_int2(0, 0);
        }
        un = un1;
        k = k1;
        rk = rk1;
        un1 = un2;
        k1 = (unit_ok(un1) && lane < un1.w) ? g.col[un1.z + lane] : -1;
    }
}

// =====================================================================================================================
// block classes: a unit (node, key partition) by a workgroup; counting table, third sweep, edge-set probes
// =====================================================================================================================
// ---- the table: open addressing over 4-slot buckets (one 16-byte LDS read settles almost every access) -------------
template <int CAP>
__device__ inline unsigned h2_bucket(unsigned key) {
    constexpr int BITS = __builtin_ctz(CAP / 4);
    return (h2_mul24b(key) >> (24 - BITS)) & ((1u << BITS) - 1);
}
__device__ inline int h2_match(const uint4 e, unsigned w) {
    return e.x == w ? 0 : e.y == w ? 1 : e.z == w ? 2 : e.w == w ? 3 : -1;
}
// slot of w; -1: absent
template <int CAP>
__device__ inline int h2_find(const unsigned *key, unsigned w) {
    const uint4 *tb = reinterpret_cast<const uint4 *>(key);
    unsigned b = h2_bucket<CAP>(w);
#pragma unroll 1
    for (int walk = 0; walk < H2_WALK; ++walk) {  // (insertion never walks further than this)
        const uint4 e = tb[b];
        const int pos = h2_match(e, w);
        if (pos >= 0) return (int)(b * 4) + pos;
        if (e.w == H2_EMPTY) return -1;  // slots of a bucket fill in order: a free last slot means the key never spilled
        b = (b + 1) & (CAP / 4 - 1);
    }
    return -1;
}
// slot of w, inserting it if absent; -1: the table is full (reported by the caller, never loops forever).
// A lane claims the first free slot it saw; slots never empty again, so filled slots always form a prefix of a bucket and a
// key is never stored twice (a racing lane with the same key meets it on its way up).
template <int CAP>
__device__ inline int h2_insert(unsigned *key, unsigned w) {
    const uint4 *tb = reinterpret_cast<const uint4 *>(key);
    unsigned b = h2_bucket<CAP>(w);
#pragma unroll 1
    for (int walk = 0; walk < H2_WALK; ++walk) {  // (a longer walk: too full, treated as full)
        const uint4 e = tb[b];
        const int pos = h2_match(e, w);
        if (pos >= 0) return (int)(b * 4) + pos;
        int ep = e.x == H2_EMPTY ? 0 : e.y == H2_EMPTY ? 1 : e.z == H2_EMPTY ? 2 : e.w == H2_EMPTY ? 3 : 4;
        for (; ep < 4; ++ep) {
            const unsigned old = atomicCAS(&key[b * 4 + ep], H2_EMPTY, w);
            if (old == H2_EMPTY || old == w) return (int)(b * 4) + ep;
        }
        b = (b + 1) & (CAP / 4 - 1);
    }
    return -1;
}
// per-slot state, two 16-bit halves per word: bit 15 = member of N(u), bits 0-14 = occurrences in the neighbours' rows
__device__ inline void h2_cnt_flag(unsigned *cnt, int s) { atomicOr(&cnt[s >> 1], 0x8000u << ((s & 1) * 16)); }
__device__ inline void h2_cnt_add(unsigned *cnt, int s) { atomicAdd(&cnt[s >> 1], 1u << ((s & 1) * 16)); }
__device__ inline unsigned h2_cnt_get(const unsigned *cnt, int s) { return (cnt[s >> 1] >> ((s & 1) * 16)) & 0xFFFFu; }

struct H2Scratch {
    int2 desc[64];   // {start, length} of the rows of the current batch
    int poff[66];    // exclusive prefix of their piece counts; poff[64] = total
    int rowT[64], rowPos[64], rowMx[64], rowRev[64];  // third-sweep accumulators per row of the batch
    unsigned qw[H2_QCAP];       // queued exact-path work: key ...
    unsigned char qr[H2_QCAP];  // ... row of the batch ...
    unsigned char qb[H2_QCAP];  // ... and batch (the second sweep's queue runs across batches)
    unsigned plt[H2_PLCAP];       // third sweep: the members of N(u) met in the rows of the batch (triangle partners) ...
    unsigned char plr[H2_PLCAP];  // ... and the row each was met in
    int pln;                      // how many (counting past the capacity)
    unsigned char trank[64];      // rank of each row of the batch among the rows present (its task is tbase + rank)
};

// the LDS arrays of a unit
struct H2Tab {
    unsigned *b1, *b2;
    unsigned *key;  // [EXS] 4-slot buckets
    unsigned *cnt;  // [EXS / 2] their state, 16 bits each
    int *full;      // set when the table fills up
    int *wsum;      // [waves of the unit] per-wave totals of the join's slot scan
};

// M_u(w) and whether w is a member of N(u); {1, false} for a key this unit keeps no exact state for
template <int L1, int EXS>
__device__ inline int h2_query(const H2Tab t, unsigned w, bool &nbr) {
    nbr = false;
    if (!h2_again(t.b2, h2_bit<L1>(w))) return 1;
    const int s = h2_find<EXS>(t.key, w);
    if (s < 0) return 1;
    const unsigned c16 = h2_cnt_get(t.cnt, s);
    nbr = (c16 & 0x8000u) != 0u;
    return (int)(c16 & 0x7FFFu);
}

// ---- the edge set: every undirected edge as one 64-bit key in an open-addressing table in device memory -------------------
// The triangle step asks it "is w adjacent to t?" a few times per edge with triangles.  Built once (one CAS per edge) and
// then KEPT across passes (round 4): the SDRF loop changes one or two edges between two passes, the edit kernels journal them
// (DevResult::edit_log) and h2_eset_apply, one thread of k_h2_plan<1>, brings the set up to date — an insertion, or a tombstone in place of a removed
// key (probes walk over tombstones; the bitmap in front of the table keeps the removed edge's bit: a false positive the
// table then answers).  Rebuilt when the journal overflowed, the table was re-sized, or tombstones have piled up.
constexpr unsigned long long H2_ESET_EMPTY = ~0ull;
constexpr unsigned long long H2_ESET_TOMB = ~0ull - 1ull;
__device__ inline unsigned long long h2_edge_key(int a, int b) {
    return a < b ? ((unsigned long long)(unsigned)a << 32) | (unsigned)b : ((unsigned long long)(unsigned)b << 32) | (unsigned)a;
}
__device__ inline unsigned long long h2_eset_slot(unsigned long long key, int bits) {
    return (key * 0x9E3779B97F4A7C15ull) >> (64 - bits);
}
struct H2EdgeSet {
    unsigned long long *tab;
    int bits;
    unsigned *bloom;  // one bit per edge in a bitmap small enough for an XCD's L2: most probes end there
    int bloom_bits;
};
__device__ inline unsigned h2_bloom_bit(unsigned long long key, int bits) {
    return (unsigned)((key * 0xD6E8FEB86659FD93ull) >> (64 - bits));
}
__device__ inline bool h2_eset_has(const H2EdgeSet es, int a, int b) {
    const unsigned long long key = h2_edge_key(a, b), mask = (1ull << es.bits) - 1ull;
    unsigned long long h = h2_eset_slot(key, es.bits);
#pragma unroll 1
    for (unsigned long long walk = 0; walk <= mask; ++walk) {
        const unsigned long long k = es.tab[h];
        if (k == key) return true;
        if (k == H2_ESET_EMPTY) return false;
        h = (h + 1) & mask;
    }
    return false;
}
// the journaled edits, in order, by ONE thread of the pass (a handful per SDRF iteration): see k_h2_plan
__device__ inline void h2_eset_apply(const H2EdgeSet es, DevResult *res, int32_t *status) {
    const int n = res->edit_n;
    res->edit_n = 0;
    if (n < 0 || n > EDIT_LOG_CAP) {  // (the host counts the edit launches and rebuilds instead: cannot happen)
        *status = 1;
        return;
    }
    const unsigned long long mask = (1ull << es.bits) - 1ull;
    for (int e = 0; e < n; ++e) {
        const int op = res->edit_log[3 * e], u = res->edit_log[3 * e + 1], v = res->edit_log[3 * e + 2];
        const unsigned long long key = h2_edge_key(u, v);
        unsigned long long h = h2_eset_slot(key, es.bits), free_at = ~0ull;
        bool found = false;
        for (unsigned long long walk = 0; walk <= mask; ++walk) {
            const unsigned long long k = es.tab[h];
            if (k == key) {
                found = true;
                break;
            }
            if (k == H2_ESET_TOMB && free_at == ~0ull) free_at = h;
            if (k == H2_ESET_EMPTY) {
                if (free_at == ~0ull) free_at = h;
                break;
            }
            h = (h + 1) & mask;
        }
        if (op > 0) {
            if (!found) {
                if (free_at == ~0ull) {
                    *status = 1;
                    return;
                }
                es.tab[free_at] = key;
            }
            const unsigned bb = h2_bloom_bit(key, es.bloom_bits);
            es.bloom[bb >> 5] |= 1u << (bb & 31u);
        } else if (found) {
            es.tab[h] = H2_ESET_TOMB;
        }
    }
}
__global__ void __launch_bounds__(256) k_h2_eset_build(View g, H2EdgeSet es, int32_t *status, DevResult *res) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s == 0) res->edit_n = 0;  // the set is built from the rows as they are: every journaled edit is in it
    if (s >= g.cap_total) return;
    const int u = g.slot_row[s];
    if (u < 0 || u >= g.n) return;
    const int2 ru = g.rowinfo[u];
    if (s < ru.x || (int)(s - ru.x) >= ru.y) return;
    const int v = g.col[s];
    if (v <= u || v >= g.n) return;
    const unsigned long long key = h2_edge_key(u, v), mask = (1ull << es.bits) - 1ull;
    const unsigned bb = h2_bloom_bit(key, es.bloom_bits);
    atomicOr(&es.bloom[bb >> 5], 1u << (bb & 31u));
    unsigned long long h = h2_eset_slot(key, es.bits);
#pragma unroll 1
    for (unsigned long long walk = 0; walk <= mask; ++walk) {
        const unsigned long long old = atomicCAS(&es.tab[h], H2_ESET_EMPTY, key);
        if (old == H2_ESET_EMPTY || old == key) return;
        h = (h + 1) & mask;
    }
    *status = 1;
}

// ---- triangle step ------------------------------------------------------------------------------------------------------
// An edge {u,v} with triangles AND candidates (w in row v, outside N(u), M_u(w) >= 2): c(w) = M_u(w) - 1 - |N(w) ∩ Tset|,
// Tset = N(u) ∩ N(v).  Every (candidate, partner) pair is one probe of the edge set, and nearly all the pairs (98 % on the
// bench graph: 13.5 M) belong to a few thousand hub-to-hub edges with hundreds of candidates and partners each, up to
// 57 k pairs for one edge.  Probed on the spot by the wave that owns the row, they were 1.2 ms of a 2.6 ms pass (one
// dependent device-memory read per lane and round, the heavy rows of one hub in the same workgroup).  So the units only
// LIST the work — per such edge a task {record slot, candidates (w, M - 1), partners} in device-memory pools — and one
// dense kernel over all candidates of all tasks (k_h2_triangles) probes and publishes, spread over the whole chip.
struct H2Tasks {
    uint4 *task;   // per row of a block-class unit: {record slot, first partner, partners (0xFFFFFFFF: nothing to correct, its
                   // candidates are skipped), node | 0x80000000 when listed by the retry launch}
    int4 *cand;    // {w, M_u(w) - 1, task, unused}
    int32_t *part;
    int64_t task_cap, cand_cap, part_cap;
    int32_t *n_task, *n_cand, *n_part, *n_done;  // this pool's counters in the result block
    DevResult *res;
    const int32_t *weight;  // bit 31: the node went to the retry list (what its first attempt listed is void)
    unsigned retry_flag;    // 0x80000000 in the retry launch
    unsigned *lists;        // per-wave lists of the third step (H2_LIST_WORDS each, one per wave of the launch; nullptr: none)
    H2EdgeSet es;           // probed by the units that join their triangle term themselves (h2_batch_join)
};
// Pool space is handed out in chunks per wave (a reservation per edge on three shared counters cost more than the whole
// step: same-address atomics serialise); what a wave leaves of a candidate chunk is marked void.  All members are uniform.
constexpr int H2_CHUNK_C = 256, H2_CHUNK_P = 128, H2_CHUNK_T = 64;
struct H2Alloc {
    int c_cur = 0, c_end = 0, p_cur = 0, p_end = 0, t_cur = 0, t_end = 0;
};
__device__ inline int h2_pool_grab(int32_t *counter, int n) {  // all lanes call this
    int v = 0;
    if ((threadIdx.x & 63) == 0) v = atomicAdd(counter, n);
    return __shfl(v, 0);
}
__device__ inline void h2_void_candidates(const H2Tasks tk, int from, int to) {
    for (int64_t i = (int64_t)from + (threadIdx.x & 63); i < to && i < tk.cand_cap; i += 64) tk.cand[i] = make_int4(0, 0, -1, 0);
}
constexpr unsigned H2_TASK_VOID = 0xFFFFFFFFu;
__device__ inline void h2_void_tasks(const H2Tasks tk, int from, int to) {
    for (int64_t i = (int64_t)from + (threadIdx.x & 63); i < to && i < tk.task_cap; i += 64)
        tk.task[i] = make_uint4(0u, 0u, H2_TASK_VOID, 0u);
}

// nt tasks, nc candidates and np partners, each contiguous (all lanes call this; false: the pools are too small)
__device__ inline bool h2_pool_reserve(const H2Tasks tk, H2Alloc &al, int nt, int nc, int np, int &t0, int &c0, int &p0) {
    if (al.t_end - al.t_cur < nt) {
        h2_void_tasks(tk, al.t_cur, al.t_end);
        const int n = nt > H2_CHUNK_T ? nt : H2_CHUNK_T;
        al.t_cur = h2_pool_grab(tk.n_task, n);
        al.t_end = al.t_cur + n;
    }
    if (al.c_end - al.c_cur < nc) {
        h2_void_candidates(tk, al.c_cur, al.c_end);
        const int n = nc > H2_CHUNK_C ? nc : H2_CHUNK_C;
        al.c_cur = h2_pool_grab(tk.n_cand, n);
        al.c_end = al.c_cur + n;
    }
    if (al.p_end - al.p_cur < np) {
        const int n = np > H2_CHUNK_P ? np : H2_CHUNK_P;
        al.p_cur = h2_pool_grab(tk.n_part, n);
        al.p_end = al.p_cur + n;
    }
    t0 = al.t_cur;
    c0 = al.c_cur;
    p0 = al.p_cur;
    al.t_cur += nt;
    al.c_cur += nc;
    al.p_cur += np;
    if (t0 < 0 || (int64_t)t0 + nt > tk.task_cap || c0 < 0 || (int64_t)c0 + nc > tk.cand_cap || p0 < 0 || (int64_t)p0 + np > tk.part_cap) {
        // the pools are too small (or the 31-bit counters wrapped): the counters keep counting, the host grows the pools
        // to what they say and runs the pass again
        if ((threadIdx.x & 63) == 0) {
            if (c0 < 0 || p0 < 0 || t0 < 0) tk.res->h2_status = 1;
            else atomicCAS(&tk.res->h2_status, 0, 2);  // (a table failure elsewhere, 1, stays)
        }
        return false;
    }
    return true;
}

// Fallback when the partner list of a batch did not fit in LDS (rows of hubs: hundreds of partners each): the members of
// N(u) in row v are read again, by one wave (long rows) or one LANE per row (rows of at most H2_SHORT_ROW entries).
template <int L1, int EXS>
__device__ inline void h2_partners_of_row(const View &g, const H2Tasks tk, int u, int2 rv, int p0, int npart, const H2Tab t) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int32_t *rowv = g.col + rv.x;
    int np = 0;  // running total (uniform)
    for (int base = 0; base < rv.y; base += 64) {
        const int i = base + lane;
        const int w = i < rv.y ? rowv[i] : -1;
        bool isT = false;
        if (w >= 0 && w != u) (void)h2_query<L1, EXS>(t, (unsigned)w, isT);
        const unsigned long long mT = __ballot(isT);
        const int it = np + __popcll(mT & below);
        if (isT && it < npart) tk.part[p0 + it] = w;
        np += __popcll(mT);
    }
    if (lane == 0 && np != npart) row_ok(g, make_int2(-1, np), 43, npart, u);  // cannot happen
}
constexpr int H2_SHORT_ROW = 32;
template <int L1, int EXS>
__device__ inline void h2_partners_short(const View &g, const H2Tasks tk, int u, int2 rv, int p0, int npart, const H2Tab t) {
    int pi = p0;
    const int pend = p0 + npart;
    for (int q0 = 0; q0 < rv.y; q0 += 8) {  // (eight loads in flight: a lane walks its row alone)
        int ww[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) ww[q] = q0 + q < rv.y ? g.col[rv.x + q0 + q] : -1;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int w = ww[q];
            if (w < 0 || w == u) continue;
            bool isT;
            (void)h2_query<L1, EXS>(t, (unsigned)w, isT);
            if (isT) {
                if (pi < pend) tk.part[pi] = w;
                ++pi;
            }
        }
    }
    if (pi != pend) row_ok(g, make_int2(-1, pi - pend), 43, npart, u);  // cannot happen
}

// ---- the third sweep from a list (round 4) ---------------------------------------------------------------------------------
// The third sweep used to stream every row again, test every entry against B2 again, queue and LOOK UP every exact-path entry
// again — for the per-row statistics of the few entries that matter (10 % of them in the middle class).  The second sweep has
// those entries in its hands, table slot included: it now appends {slot, row, batch} to a per-wave list in device memory (and
// where u sits in each row to a per-wave array), and the third step is one pass over that list once the counts are complete.
// A wave whose list would overflow, or with more batches than the array holds, falls back to streaming (the old path).
constexpr int H2_ITEMS = 2048;       // items per wave and unit
constexpr int H2_REV_BATCHES = 16;   // batches of 64 rows per wave whose "position of u" the array holds
constexpr int H2_LIST_OWN = H2_ITEMS + H2_REV_BATCHES * 64;  // a wave's own items and row array
// ... plus, per workgroup, one array of as many words as its waves have items: the rows of the repeated keys grouped by key
// (h2_join_prepare).  Layout of a workgroup's part of the pool: the waves' own parts, then that array.
constexpr int H2_LIST_WORDS = H2_LIST_OWN + H2_ITEMS;  // 32-bit words per wave
struct H2List {       // all members uniform over the wave
    unsigned *items;  // slot | row << 13 | batch << 19
    int *revs;        // [batch][row of the batch]: slot of u inside that row, -1: not found
    int32_t *srt;     // the workgroup's: for every key that repeats, the members of N(u) whose rows hold it, one run per table slot
    int n;            // items appended (counts past the capacity)
    bool over;        // the list does not describe the unit: stream the third sweep
    bool join;        // uniform over the workgroup: no wave's list overflowed, the unit joins its triangle term itself
};
__device__ inline H2List h2_list_of(unsigned *pool, int waves_per_group) {
    H2List ls;
    unsigned *group = pool ? pool + (int64_t)blockIdx.x * waves_per_group * H2_LIST_WORDS : nullptr;
    unsigned *mine = group ? group + (int64_t)(threadIdx.x >> 6) * H2_LIST_OWN : nullptr;
    ls.items = mine;
    ls.revs = reinterpret_cast<int *>(mine ? mine + H2_ITEMS : nullptr);
    ls.srt = reinterpret_cast<int32_t *>(group ? group + (int64_t)waves_per_group * H2_LIST_OWN : nullptr);
    ls.n = 0;
    ls.over = mine == nullptr;
    ls.join = false;
    return ls;
}

// ---- the three sweeps: the rows of the neighbours of u, in batches of 64 rows per wave -----------------------------------
// the queued exact-path work of one wave: n is uniform and lives in a register
// PHASE 2 also LISTS what the triangle step needs, on the spot (no row is read again for it): every candidate occurrence
// (w outside N(u), c = M_u(w) - 1 > 0) goes to the device-memory pool with the task of its row (tbase + row: a task
// per row of the batch, filled in when the batch is complete), every member of N(u) met (a triangle partner of its row)
// to the batch's LDS list.
// what the third step does with ONE exact-path entry per lane: `have` (the lane holds one), its table slot, its row of the
// batch, its key.  pln (uniform) counts the batch's triangle partners.
template <int L1, int EXS>
__device__ inline void h2_settle(const H2Tab t, H2Scratch *sc, bool have, int s, int r, unsigned w, int &pln, const H2Tasks tk,
                                 H2Alloc &al, int tbase) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    bool cand = false, partner = false;
    int c = 0;
    if (have && s >= 0) {
        const unsigned c16 = h2_cnt_get(t.cnt, s);
        if (c16 & 0x8000u) {
            atomicAdd(&sc->rowT[r], 1);
            partner = true;
        } else {
            c = (int)(c16 & 0x7FFFu) - 1;
            if (c > 0) {
                atomicAdd(&sc->rowPos[r], 1);
                atomicMax(&sc->rowMx[r], c);
                cand = true;
            }
        }
    }
    const unsigned long long mC = __ballot(cand), mT = __ballot(partner);
    if (mC != 0ull && tbase >= 0) {  // uniform
        const int nc = __popcll(mC);
        if (al.c_end - al.c_cur < nc) {
            h2_void_candidates(tk, al.c_cur, al.c_end);
            al.c_cur = h2_pool_grab(tk.n_cand, H2_CHUNK_C);
            al.c_end = al.c_cur + H2_CHUNK_C;
        }
        const int c0 = al.c_cur;
        al.c_cur += nc;
        if (c0 < 0 || (int64_t)c0 + nc > tk.cand_cap) {
            if (lane == 0) {
                if (c0 < 0) tk.res->h2_status = 1;
                else atomicCAS(&tk.res->h2_status, 0, 2);  // the pool is too small: the host grows it and runs the pass again
            }
        } else if (cand) {
            tk.cand[c0 + __popcll(mC & below)] = make_int4((int)w, c, tbase + (int)sc->trank[r], 0);
        }
    }
    if (mT != 0ull) {  // uniform
        if (partner) {
            const int idx = pln + __popcll(mT & below);
            if (idx < H2_PLCAP) {
                sc->plt[idx] = w;
                sc->plr[idx] = (unsigned char)r;
            }
        }
        pln += __popcll(mT);
    }
}

// PHASE 1: occurrences of the repeated keys (and the list of the third step); PHASE 2 (streaming fallback): per-row statistics.
// PARTS: the unit is one key partition of a split node — only its own keys are counted, but the flagged members of N(u), which
// live in every partition's table, are met (and listed) whatever their partition: T and the partner lists are whole.
template <int L1, int EXS, int PHASE, bool PARTS>
__device__ inline void h2_drain(const H2Tab t, H2Scratch *sc, int &n, const H2Tasks tk, H2Alloc &al, int tbase, H2List &ls, int part,
                                int nparts) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    h2_wave_sync();
    int pln = PHASE == 2 ? sc->pln : 0;  // uniform
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const unsigned w = i < n ? sc->qw[i] : 0u;
        if (PHASE == 1) {
            int s = -1;
            if (i < n) {
                const bool own = !PARTS || h2_part(w, nparts) == part;
                if (own) {
                    s = h2_insert<EXS>(t.key, w);
                    if (s < 0) *t.full = 1;
                    else h2_cnt_add(t.cnt, s);
                } else {  // another partition's key: of interest only as a member of N(u)
                    s = h2_find<EXS>(t.key, w);
                    if (s >= 0 && !(h2_cnt_get(t.cnt, s) & 0x8000u)) s = -1;
                }
            }
            if (!ls.over) {  // uniform
                const unsigned long long m = __ballot(s >= 0);
                const int cnt = __popcll(m);
                if (ls.n + cnt > H2_ITEMS) {
                    ls.over = true;
                } else if (s >= 0) {
                    ls.items[ls.n + __popcll(m & below)] = (unsigned)s | ((unsigned)sc->qr[i] << 13) | ((unsigned)sc->qb[i] << 19);
                }
                ls.n += cnt;
            }
        } else {
            int s = -1, r = 0;
            if (i < n) {
                s = h2_find<EXS>(t.key, w);
                r = sc->qr[i];
            }
            h2_settle<L1, EXS>(t, sc, i < n, s, r, w, pln, tk, al, tbase);
        }
    }
    if (PHASE == 2 && lane == 0) sc->pln = pln;
    h2_wave_sync();
    n = 0;
}

// the third step from the list: the items of batch `bidx` (they are batch-monotone: the second sweep's queue is first in, first out)
template <int L1, int EXS>
__device__ inline void h2_settle_items(const H2Tab t, H2Scratch *sc, const H2List &ls, int &lcur, int bidx, const H2Tasks tk, H2Alloc &al,
                                       int tbase) {
    const int lane = threadIdx.x & 63;
    int pln = sc->pln;  // uniform
#pragma unroll 1
    while (true) {
        const int i = lcur + lane;
        const unsigned item = i < ls.n ? ls.items[i] : 0xFFFFFFFFu;
        const bool mine = i < ls.n && (int)(item >> 19) == bidx;
        const int cnt = __popcll(__ballot(mine));
        if (cnt == 0) break;  // uniform
        const int s = (int)(item & 0x1FFFu), r = (int)((item >> 13) & 63u);
        const unsigned w = mine ? t.key[s] : 0u;
        h2_settle<L1, EXS>(t, sc, mine, mine ? s : -1, r, w, pln, tk, al, tbase);
        lcur += cnt;
        if (cnt < 64) break;
    }
    if (lane == 0) sc->pln = pln;
    h2_wave_sync();
}

// third sweep, start of a batch of rows: row accumulators, partner list, a task per row present
__device__ inline void h2_batch_begin(const H2Tasks tk, H2Alloc &al, H2Scratch *sc, int k, int &tbase, int &trow, int rev = -1) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    sc->rowT[lane] = 0;
    sc->rowPos[lane] = 0;
    sc->rowMx[lane] = 0;
    sc->rowRev[lane] = rev;  // (-1: found by the sweep that follows; list mode: what the second sweep found)
    if (lane == 0) sc->pln = 0;
    int dummy_c, dummy_p;
    const unsigned long long rows = __ballot(k >= 0);  // a task per row of the batch
    if (!h2_pool_reserve(tk, al, __popcll(rows), 0, 0, tbase, dummy_c, dummy_p)) tbase = -1;
    trow = __popcll(rows & below);  // rank of this lane's row among them (the drain needs rank by row: sc->trank)
    sc->trank[lane] = (unsigned char)trow;
    trow += tbase;
}

// third sweep, end of a batch (the queue is drained): partners to the pool, tasks, records.  i: this lane's position in
// row u; k, rk: its member of N(u) and that one's row
// items / [ifrom, ito): in list mode, the wave's exact-path items of this batch ({slot, row, batch}: h2_settle_items has just walked
// them) — round 5: when the batch has more triangle partners than the LDS list holds, they are taken from these items in a second
// pass instead of reading the rows again (a wave per long row, one after the other: 186 of the 407 us of the longest unit of the
// bench graph, the unit that sets the length of the split class's kernel).  items == nullptr: streaming mode, rows are read again.
template <int L1, int EXS, bool PARTS>
__device__ inline void h2_batch_end(const View &g, const H2Tasks tk, H2Alloc &al, int u, int2 ru, int i, int k, int2 rk, int tbase,
                                    int trow, int part, const H2Tab t, H2Scratch *sc, uint4 *rec, const unsigned *items = nullptr,
                                    int ifrom = 0, int ito = 0) {
    const int lane = threadIdx.x & 63;
    int T = sc->rowT[lane], pos = sc->rowPos[lane], mx = sc->rowMx[lane];
    const int rev = sc->rowRev[lane];
    // Triangles AND positive counts: the counts of this edge still include the triangle partners.  Its candidates
    // are in the pool already (listed by the drain); its partners go there now and its task says where they are:
    // k_h2_triangles publishes its counts, here it contributes none.  The tasks of all other rows are void.
    bool listed = tbase >= 0 && k >= 0 && T > 0 && pos > 0 && rev >= 0 && rev < g.cap_total;
    int ep;
    const int Pn = h2_prefix(listed ? T : 0, ep);
    int p0 = 0;
    if (Pn > 0) {  // uniform
        int dummy_t, dummy_c;
        if (!h2_pool_reserve(tk, al, 0, 0, Pn, dummy_t, dummy_c, p0)) listed = false;
    }
    if (__ballot(listed) != 0ull) {
        const int pln = sc->pln;
        if (pln <= H2_PLCAP) {
            // the partners were kept: each goes to the range of its row (sc->poff is free now: a cursor per row)
            sc->poff[lane] = listed ? p0 + ep : -1;
            h2_wave_sync();
            for (int j = lane; j < pln; j += 64) {
                const int r = sc->plr[j];
                if (sc->poff[r] >= 0) tk.part[atomicAdd(&sc->poff[r], 1)] = (int32_t)sc->plt[j];
            }
            h2_wave_sync();
        } else if (items) {
            // too many for the LDS list (rows of hubs): a second pass over the batch's items — every flagged one is a partner of its row
            sc->poff[lane] = listed ? p0 + ep : -1;
            h2_wave_sync();
            for (int j = ifrom + lane; j < ito; j += 64) {
                const unsigned item = items[j];
                const int s2 = (int)(item & 0x1FFFu), r = (int)((item >> 13) & 63u);
                if ((h2_cnt_get(t.cnt, s2) & 0x8000u) && sc->poff[r] >= 0) tk.part[atomicAdd(&sc->poff[r], 1)] = (int32_t)t.key[s2];
            }
            h2_wave_sync();
        } else {
            // too many for the list (rows of hubs): the rows are read again for their partners
            const bool shortrow = listed && rk.y <= H2_SHORT_ROW;
            if (shortrow) h2_partners_short<L1, EXS>(g, tk, u, rk, p0 + ep, T, t);
            unsigned long long todo = __ballot(listed && !shortrow);
            while (todo) {
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int2 rv = make_int2(__shfl(rk.x, l), __shfl(rk.y, l));
                h2_partners_of_row<L1, EXS>(g, tk, u, rv, __shfl(p0 + ep, l), __shfl(T, l), t);
            }
        }
    }
    if (tbase >= 0 && k >= 0) {
        tk.task[trow] = listed ? make_uint4((unsigned)(ru.x + i), (unsigned)(p0 + ep), (unsigned)T, (unsigned)u | tk.retry_flag)
                               : make_uint4(0u, 0u, H2_TASK_VOID, 0u);
    }
    if (listed) {
        pos = 0;
        mx = 0;
    }
    if (k >= 0) {
        const int64_t slot = (int64_t)ru.x + i;
        if (rev < 0 || rev >= g.cap_total) {
            row_ok(g, make_int2(-1, rev), 33, u, k);  // adjacency not symmetric: report, never publish
        } else if (!PARTS) {
            rec[slot] = make_uint4((unsigned)pos, (unsigned)mx, h2_rec_t(T, ru.y), (unsigned)rev);
        } else {
            unsigned *r4 = reinterpret_cast<unsigned *>(rec + slot);
            if (pos) atomicAdd(&r4[0], (unsigned)pos);
            if (mx) atomicMax(&r4[1], (unsigned)mx);
            if (part == 0) {  // the flagged neighbours live in every partition's table: T and the slot are whole
                r4[2] = h2_rec_t(T, ru.y);
                r4[3] = (unsigned)rev;
            }
        }
    }
}

// ---- the triangle term joined inside the unit -----------------------------------------------------------------------------
// c(w) for the occurrence of w in row r (edge {u, v_r}) is M_u(w) - 1 - |{ t in N(u) ∩ N(v_r) : t adjacent to w }|.  Every such t
// is itself a row j of u, and "t adjacent to w" is "w occurs in row j": the second sweep has listed exactly these occurrences
// (an item {slot of w, row j} per occurrence of a repeated key).  So the last term is
//     |{ j in rows(w), j != r : v_j adjacent to v_r }|,
// M_u(w) - 1 probes of the edge set for a candidate instead of one per triangle partner of its edge (hundreds on a hub-to-hub
// edge, nearly all of them misses), asked by the unit itself with the counts at hand: it publishes final records and lists
// nothing for k_h2_triangles.  rows(w) comes from a counting sort of the unit's items by table slot: the counts are the
// table's own, the cursors live in B1 (dead after the first sweep, and exactly EXS 16-bit words large), the sorted members go
// to the workgroup's array in device memory.  Needs every wave's list complete: a unit with an overflowed list keeps the old
// path (pools and k_h2_triangles) and is counted in DevResult::h2_fallback.
// Cost: a key met in M rows is a candidate in up to M of them and each asks M times: M (M - 1) probes per key, against T_r per
// candidate on the old path — far fewer on power-law graphs (M <= 43 on S100k, <= 54 on S1M, T_r in the hundreds on hub-to-hub
// edges), but quadratic where two hubs share thousands of neighbours.  A unit with a key in more than H2_JOIN_MAXM rows therefore
// keeps the old path as well: a candidate's serial loop stays at most 32 rounds of 8 probes in flight, what the old path spends on an
// edge with 256 partners.
constexpr int H2_JOIN_MAXM = 256;
__device__ inline int h2_probe_partners(const H2EdgeSet es, int w, const int32_t *pt, int np);

// all threads of the unit; the table is complete, no wave's list overflowed.  false (uniform, nothing written but B1): some key is
// in more rows than the join takes
template <int L1, int EXS, int NW>
__device__ inline bool h2_join_prepare(const View &g, const H2Tab t, int2 ru, const H2List &ls) {
    constexpr int NT = 64 * NW, PER = EXS / NT;  // consecutive table slots per thread
    static_assert(PER >= 2 && PER % 2 == 0, "a thread owns whole cursor words");
    static_assert(EXS / 2 <= (1 << L1) / 32, "the cursors fit B1");
    static_assert(NW * H2_ITEMS < 65536 && EXS <= 8192, "16-bit cursors, 13-bit slots");
    const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
    unsigned *cur = t.b1;
    int n[PER], sum = 0, most = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const unsigned c16 = h2_cnt_get(t.cnt, tid * PER + q);
        n[q] = ((c16 & 0x8000u) || c16 < 2u) ? 0 : (int)c16;  // (members of N(u) and keys met once are no candidates)
        sum += n[q];
        most = n[q] > most ? n[q] : most;
    }
    if (__syncthreads_or(most > H2_JOIN_MAXM)) return false;
    int excl;
    const int wtot = h2_prefix(sum, excl);
    if (lane == 0) t.wsum[wid] = wtot;
    __syncthreads();
    int off = excl;
    for (int w = 0; w < wid; ++w) off += t.wsum[w];
#pragma unroll
    for (int q = 0; q < PER; q += 2) {
        const unsigned lo = (unsigned)off;
        off += n[q];
        const unsigned hi = (unsigned)off;
        off += n[q + 1];
        cur[(tid * PER + q) >> 1] = lo | (hi << 16);
    }
    __syncthreads();
    for (int base = 0; base < ls.n; base += 64) {
        const int j = base + lane;
        if (j >= ls.n) continue;
        const unsigned item = ls.items[j];
        const int s = (int)(item & 0x1FFFu), r = (int)((item >> 13) & 63u), b = (int)(item >> 19);
        const unsigned c16 = h2_cnt_get(t.cnt, s);
        if ((c16 & 0x8000u) || c16 < 2u) continue;
        const int row = (b * 64 + r) * NW + wid;  // (see h2_stream: lane r of batch b of wave wid)
        if (row >= ru.y) {
            row_ok(g, make_int2(-1, row), 44, ru.y, (int)item);  // an item of a row the node does not have: report, the pass fails
            continue;
        }
        const int v = g.col[ru.x + row];
        const unsigned old = atomicAdd(&cur[s >> 1], 1u << ((s & 1) * 16));
        const int p = (int)((old >> ((s & 1) * 16)) & 0xFFFFu);
        if (p < NW * H2_ITEMS) ls.srt[p] = v;
        else row_ok(g, make_int2(-1, p), 45, s, (int)c16);  // more occurrences listed than counted: report, never write
    }
    __syncthreads();  // every cursor now stands at the END of its slot's run
    return true;
}

// One batch of rows of one wave in join mode: triangle counts, corrected candidate counts, records.  lcur: the wave's next item.
template <int L1, int EXS, int NW, bool PARTS>
__device__ inline void h2_batch_join(const View &g, const H2Tasks tk, H2Alloc &al, int u, int2 ru, int i, int k, int2 rk, int part,
                                     const H2Tab t, H2Scratch *sc, uint4 *rec, const H2List &ls, int &lcur, int bidx, int rev) {
    const int lane = threadIdx.x & 63;
    sc->rowT[lane] = 0;
    sc->rowPos[lane] = 0;
    sc->rowMx[lane] = 0;
    sc->rowRev[lane] = rev;
    if (lane == 0) sc->pln = 0;
    h2_wave_sync();
    const int lfrom = lcur;
#pragma unroll 1
    while (true) {  // the batch's items (batch-monotone): a flagged one is a triangle partner of its row
        const int j = lcur + lane;
        const unsigned item = j < ls.n ? ls.items[j] : 0xFFFFFFFFu;
        const bool mine = j < ls.n && (int)(item >> 19) == bidx;
        const int cnt = __popcll(__ballot(mine));
        if (cnt == 0) break;  // uniform
        if (mine && (h2_cnt_get(t.cnt, (int)(item & 0x1FFFu)) & 0x8000u)) atomicAdd(&sc->rowT[(item >> 13) & 63u], 1);
        lcur += cnt;
        if (cnt < 64) break;
    }
    h2_wave_sync();
    const unsigned *cur = t.b1;
#pragma unroll 1
    for (int base = lfrom; base < lcur; base += 64) {
        const int j = base + lane;
        const bool have = j < lcur;
        const unsigned item = have ? ls.items[j] : 0u;
        const int s = (int)(item & 0x1FFFu), r = (int)((item >> 13) & 63u);
        const int vr = __shfl(k, r);
        if (!have) continue;
        const unsigned c16 = h2_cnt_get(t.cnt, s);
        if (c16 & 0x8000u) continue;
        const int m = (int)(c16 & 0x7FFFu);
        int c = m - 1;
        if (c <= 0) continue;
        if (sc->rowT[r] > 0 && vr >= 0) {
            const int end = (int)((cur[s >> 1] >> ((s & 1) * 16)) & 0xFFFFu);
            if (end >= m && end <= NW * H2_ITEMS) {
                c -= h2_probe_partners(tk.es, vr, ls.srt + (end - m), m);  // (v_r itself is in the run: no edge)
            } else {
                row_ok(g, make_int2(-1, end), 46, s, m);  // the cursor is not at the end of its run: report, never publish uncorrected
                c = 0;
            }
        }
        if (c > 0) {
            atomicAdd(&sc->rowPos[r], 1);
            atomicMax(&sc->rowMx[r], c);
        }
    }
    h2_wave_sync();
    h2_batch_end<L1, EXS, PARTS>(g, tk, al, u, ru, i, k, rk, -1, 0, part, t, sc, rec);  // (no task base: lists nothing, publishes)
}

// Wave `wid` of NW takes the rows i = wid, wid + NW, ... of row u (strided: a hub's heaviest rows, adjacent at the
// front of its row, spread over the waves); lane l of the batch starting at `base` stands for row base + l * NW + wid.
// PHASE 0: bitmaps; 1: occurrences of the repeated keys; 2: per-row statistics, triangle step, records.
// k0, rk0: this lane's row of the FIRST batch (member of N(u) and its row header, validated), read once by the caller for all
// three sweeps: a unit of the streaming path is a chain of dependent device-memory reads (row of u -> headers of its
// members' rows -> their pieces) with a handful of pieces per lane behind it, and two of its three links do not change
// between the sweeps (round 4: the split class spent most of every sweep waiting for them).
template <int L1, int EXS, int NW, bool PARTS, int PHASE>
__device__ inline void h2_stream(const View &g, const H2Tasks tk, H2Alloc &al, int u, int2 ru, int part, int nparts,
                                 const H2Tab t, H2Scratch *sc, uint4 *rec, int k0, int2 rk0, H2List &ls) {
    const int lane = threadIdx.x & 63;
    const int wid = (int)(threadIdx.x >> 6);
    int qn = 0;  // queued items (uniform)
    int lcur = 0;  // third step from the list: next item (uniform)
    if (PHASE == 0 && ru.y > 64 * NW * H2_REV_BATCHES) ls.over = true;  // more batches than the list's row array holds
    for (int base = 0; base < ru.y; base += 64 * NW) {
        const int i = base + lane * NW + wid;
        int k = k0;
        int2 rk = rk0;
        if (base > 0) {  // uniform
            k = -1;
            rk = make_int2(0, 0);
            if (i < ru.y) {
                k = g.col[ru.x + i];
                if (k >= 0 && k < g.n && k != u) {
                    rk = g.rowinfo[k];
                    if (!row_ok(g, rk, 32, k, u)) rk = make_int2(0, 0);
                } else {
                    k = -1;
                }
            }
        }
        const int np = rk.y > 0 ? ((rk.x + rk.y + 3) >> 2) - (rk.x >> 2) : 0;
        int poff_lane;
        const int P = h2_prefix(np, poff_lane);
        if (P == 0) continue;  // uniform: no row in this wave's share of the batch
        const int bidx = base / (64 * NW);
        int tbase = -1, trow = 0;  // third sweep: the tasks of this batch's rows (tbase uniform; trow: this lane's row)
        if (PHASE == 2 && !ls.over) {
            // the third step from the second sweep's list: no row is streamed, no entry tested or looked up again
            if (ls.join) {
                h2_batch_join<L1, EXS, NW, PARTS>(g, tk, al, u, ru, i, k, rk, part, t, sc, rec, ls, lcur, bidx, ls.revs[bidx * 64 + lane]);
                h2_wave_sync();  // the scratch is rewritten by the next batch
                continue;
            }
            h2_batch_begin(tk, al, sc, k, tbase, trow, ls.revs[bidx * 64 + lane]);
            h2_wave_sync();
            const int lfrom = lcur;
            h2_settle_items<L1, EXS>(t, sc, ls, lcur, bidx, tk, al, tbase);
            h2_batch_end<L1, EXS, PARTS>(g, tk, al, u, ru, i, k, rk, tbase, trow, part, t, sc, rec, ls.items, lfrom, lcur);
            h2_wave_sync();  // the scratch is rewritten by the next batch
            continue;
        }
        if (PHASE == 0 && !ls.over) ls.revs[bidx * 64 + lane] = -1;
        sc->desc[lane] = rk;
        sc->poff[lane] = poff_lane;
        if (lane == 0) sc->poff[64] = P;
        if (PHASE == 2) h2_batch_begin(tk, al, sc, k, tbase, trow);
        h2_wave_sync();
        const bool listing = PHASE == 1 && !ls.over;  // uniform
        auto flags = [&](const int4 w, unsigned vm, int r, int a) -> unsigned {
            const unsigned kk[4] = {(unsigned)w.x, (unsigned)w.y, (unsigned)w.z, (unsigned)w.w};
            const unsigned isu = h2_eq4(kk, (unsigned)u) & vm;
            if (PHASE == 2 && isu) sc->rowRev[r] = a + __ffs((int)isu) - 1;
            if (listing && isu) ls.revs[bidx * 64 + r] = a + __ffs((int)isu) - 1;  // (where u sits in that row: the third step's)
            unsigned valid = vm & ~isu;
            // (third sweep: no partition test — a key of another partition is simply not in the table, and the flagged
            //  members of N(u), which are in every partition's table, must all be met: T and the partner lists are whole.
            //  The same holds for the second sweep while it lists for the third step: its drain tells the partitions apart.)
            if (PARTS && PHASE != 2 && !listing) {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    if (h2_part(kk[jj], nparts) != part) valid &= ~(1u << jj);
            }
            if (PHASE == 0) {
                h2_mark4<L1>(t.b1, t.b2, kk, valid);
                return 0u;
            }
            return h2_again4<L1>(t.b2, kk, valid);
        };
        h2_for_pieces_queued<(PARTS ? H2_QL : H2_Q)>(g.col, sc->desc, sc->poff, poff_lane, P, qn, flags,
                             [&](int idx, unsigned key, int r) {
                                 sc->qw[idx] = key;
                                 if (PHASE != 0) sc->qr[idx] = (unsigned char)r;
                                 if (PHASE == 1) sc->qb[idx] = (unsigned char)bidx;
                             },
                             [&]() { h2_drain<L1, EXS, PHASE, PARTS>(t, sc, qn, tk, al, tbase, ls, part, nparts); });
        if (PHASE == 2) {
            h2_drain<L1, EXS, PHASE, PARTS>(t, sc, qn, tk, al, tbase, ls, part, nparts);  // the row totals are read next
            h2_batch_end<L1, EXS, PARTS>(g, tk, al, u, ru, i, k, rk, tbase, trow, part, t, sc, rec);
        }
        h2_wave_sync();  // the scratch is rewritten by the next batch
    }
    if (qn > 0) h2_drain<L1, EXS, PHASE, PARTS>(t, sc, qn, tk, al, -1, ls, part, nparts);  // (after the loop: a wave's last batches may be empty; PHASE 1 only)
}

// ---- class M's row-mask path ------------------------------------------------------------------------------------------------
// A unit of at most 128 rows whose pieces fit the registers (h2_node_fast) is settled the way the wave classes settle a node
// (h2s_node), with the workgroup where that function has a wave and 128-bit masks where it has 64-bit ones: sweep B's flagged
// entries are looked up in a small exact table; a hit on a member of N(u) sets the bit of that member's position in row u in the
// adjacency mask of the entry's row, any other key gets the entry's row into its row mask and the occurrence {slot, row} onto a
// candidate list; step C is one pass over that list, c = |rows(w) \ adj(row)| - 1.  No item list in device memory, no counting
// sort, no probe of the edge set, no third sweep: per entry the block path cost nine times what a wave class pays.
// The arrays alias what the block path keeps in LDS and this path does not use: the row masks lie in the counting table's keys,
// the exact keys, the adjacency masks and the per-row results in its counts, the candidate list in B1 (dead once sweep A is
// through).  Sizes are typical, not worst case (tools/count_rowmask_keys.py, profiles/h2_rowmask_ab.txt): a unit whose table or
// list fills up publishes nothing here — h2_rows_unit returns false — and the block path takes it: its own tables cleared and seeded,
// then its sweep B, behind the sweep A the two paths share (B2 is as that sweep left it; see h2_node_fast).
constexpr int H2_ROWS_MAX = 128;   // rows of a unit: four 32-bit mask words
constexpr int H2_ROWS_EXS = 1024;  // slots of the exact table: {key, four mask words}
constexpr int H2_ROWS_CL = 2048;   // candidate occurrences: slot | row << 16
// diagnostic (tools/h2_rowmask_coverage.py): class-M units published by the row-mask path / handed over to the block path
__device__ unsigned h2_rows_units[2];

// h2s_find_or_insert with the walk cut at H2_WALK slots: a longer one counts as "full".  (Walked to the end, as the wave classes'
// small tables are, the one unit of the bench graph with more keys than slots took 1,024 dependent LDS reads per missing key and
// round, and units near a full table not many fewer: the iteration was a fifth slower than without the path,
// profiles/h2_rowmask_ab.txt.)
__device__ inline int h2r_find_or_insert(unsigned *exkey, unsigned w) {
    unsigned s = h2s_home<H2_ROWS_EXS>(w);
#pragma unroll 1
    for (int walk = 0; walk < H2_WALK; ++walk) {
        const unsigned e = exkey[s];
        if ((e & ~H2_NBR) == w && e != H2_EMPTY) return (int)s;
        if (e == H2_EMPTY) {
            const unsigned old = atomicCAS(&exkey[s], H2_EMPTY, w);
            if (old == H2_EMPTY || (old & ~H2_NBR) == w) return (int)s;
        }
        s = (s + 1) & (unsigned)(H2_ROWS_EXS - 1);
    }
    return -1;
}

// From sweep B on.  w, meta: the pieces of this wave's rows as h2_node_fast holds them after sweep A; i, k: this lane's position in
// row u and its member of N(u).  The caller has cleared the arrays below, seeded the members of N(u) into the exact table (*t.full
// set if one found no slot) and run sweep A, which is the block path's own; every thread is past it.
template <int L1, int EXS, int NW, int NP>
__device__ inline bool h2_rows_unit(const View &g, int u, int2 ru, int i, int k, int P, const int4 (&w)[NP], unsigned long long (&meta)[NP],
                                    const H2Tab t, H2Scratch *sc, uint4 *rec) {
    static_assert(EXS >= 4 * H2_ROWS_EXS, "the row masks fit the counting table's keys");
    static_assert(EXS / 2 >= H2_ROWS_EXS + 6 * H2_ROWS_MAX, "the exact keys, adjacency masks and row results fit its counts");
    static_assert((1 << L1) / 32 >= H2_ROWS_CL, "the candidate list fits B1");
    static_assert(64 * NW >= H2_ROWS_MAX && H2_ROWS_MAX <= 256 && H2_ROWS_EXS <= 65536, "a row per lane; 8-bit rows, 16-bit slots");
    const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
    constexpr int NT = 64 * NW;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned *exm = t.key;                           // [slot][4] candidate: the rows that hold it; member of N(u): word 0 = its position in row u
    unsigned *exkey = t.cnt;                         // [slot] candidate key, or a member of N(u) | H2_NBR
    unsigned *adj = t.cnt + H2_ROWS_EXS;             // [row][4] the rows adjacent to it = triangle partners of edge {u, v_row}
    int *pos = reinterpret_cast<int *>(adj + 4 * H2_ROWS_MAX), *mx = pos + H2_ROWS_MAX;
    unsigned *cl = t.b1;                             // (from sweep B on)
    int *cln = t.wsum;                               // candidate occurrences so far (counts past the capacity)
    bool full = *t.full != 0;  // (a member of N(u) found no slot in the exact table)
    // sweep B: the flagged entries are queued by lane (see h2s_node) and settled against the exact table 64 at a time
    int qn = 0;  // uniform over the wave
    auto drain = [&]() {
        h2_wave_sync();
        for (int base = 0; base < qn; base += 64) {
            const int j = base + lane;
            bool cand = false;
            int slot = -1, row = 0;
            if (j < qn) {
                row = sc->qr[j];
                slot = h2r_find_or_insert(exkey, sc->qw[j]);
                if (slot < 0) {
                    full = true;
                } else if (row >= ru.y) {
                    row_ok(g, make_int2(-1, row), 47, u, ru.y);  // an entry of a row the node does not have: report, the pass fails
                } else if (exkey[slot] & H2_NBR) {  // a member of N(u) in row `row`: rows `row` and exm[slot] are adjacent
                    const unsigned x = exm[4 * slot];
                    if (x >= (unsigned)ru.y) row_ok(g, make_int2(-1, (int)x), 48, u, ru.y);  // a position row u does not have: the same
                    else atomicOr(&adj[4 * row + (int)(x >> 5)], 1u << (x & 31u));
                } else {
                    atomicOr(&exm[4 * slot + (row >> 5)], 1u << (row & 31));
                    cand = true;
                }
            }
            const unsigned long long m = __ballot(cand);
            if (m == 0ull) continue;  // uniform
            int first = 0;
            if (lane == 0) first = atomicAdd(cln, __popcll(m));
            first = __shfl(first, 0);
            if (cand) {
                const int idx = first + __popcll(m & below);
                if (idx < H2_ROWS_CL) cl[idx] = (unsigned)slot | ((unsigned)row << 16);
                else full = true;
            }
        }
        h2_wave_sync();
        qn = 0;
    };
    {
        // (the flags of a piece's entries ride in bits 48-51 of its meta word, free in every piece: an array of their own raised the
        //  kernel's spills)
        constexpr int FL = 48;
        int nfl = 0;  // this lane's flagged entries
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            if (64 * q >= P) continue;  // uniform
            const unsigned kk[4] = {(unsigned)w[q].x, (unsigned)w[q].y, (unsigned)w[q].z, (unsigned)w[q].w};
            // (where u sits in the row, the reverse slot of edge {u, v_row}, found while the pieces are at hand)
            const unsigned isu = h2_eq4(kk, (unsigned)u) & (unsigned)meta[q] & 0xFu;
            if (isu) sc->rowRev[(int)((meta[q] >> 8) & 0xFFull)] = (int)(meta[q] >> 16) + __ffs((int)isu) - 1;
            const unsigned f = h2_again4<L1>(t.b2, kk, (unsigned)(meta[q] >> 4) & 0xFu);
            meta[q] |= (unsigned long long)f << FL;
            nfl += __popc(f);
        }
        int qi;  // queue index of this lane's next entry, counted from the start of the round
        const int qtotal = h2_prefix_dpp(nfl, qi);
#pragma unroll 1
        for (int left = qtotal; left > 0; left -= H2_QCAP) {  // uniform
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                if (64 * q >= P) continue;  // uniform
                while ((meta[q] >> FL) != 0ull && qi < H2_QCAP) {
                    const unsigned f = (unsigned)(meta[q] >> FL), b = f & (0u - f);  // the lowest flagged entry of the piece
                    sc->qw[qi] = h2_pick4(w[q], b);
                    sc->qr[qi] = (unsigned char)((int)((meta[q] >> 8) & 0xFFull) * NW + wid);  // (lane r of wave wid holds row r * NW + wid)
                    meta[q] ^= (unsigned long long)b << FL;
                    ++qi;
                }
            }
            qn = left < H2_QCAP ? left : H2_QCAP;
            drain();
            if (__ballot(full) != 0ull) break;  // uniform over the wave: the unit is handed over, the rest of the queue is not looked at
            qi -= H2_QCAP;
        }
    }
    if (__syncthreads_or(full)) return false;  // the table or the list filled up: nothing is published, the block path takes the unit
    // step C: c(w) for the occurrence of w in row r = the rows that hold w, less row r, less the rows adjacent to row r
    const int cl_n = *cln;
    const uint4 *exm4 = reinterpret_cast<const uint4 *>(exm), *adj4 = reinterpret_cast<const uint4 *>(adj);
    for (int e = tid; e < cl_n; e += NT) {
        const unsigned item = cl[e];
        const int row = (int)(item >> 16);
        const uint4 m = exm4[item & 0xFFFFu], a = adj4[row];
        const int c = __popc(m.x & ~a.x) + __popc(m.y & ~a.y) + __popc(m.z & ~a.z) + __popc(m.w & ~a.w) - 1;
        if (c > 0) {
            atomicAdd(&pos[row], 1);
            atomicMax(&mx[row], c);
        }
    }
    __syncthreads();
    if (k >= 0) {
        const int rev = sc->rowRev[lane];
        if (rev < 0 || rev >= g.cap_total) {
            row_ok(g, make_int2(-1, rev), 33, u, k);  // adjacency not symmetric: report, never publish
        } else {
            const uint4 a = adj4[i];
            const int T = __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w);
            rec[(int64_t)ru.x + i] = make_uint4((unsigned)pos[i], (unsigned)mx[i], h2_rec_t(T, ru.y), (unsigned)rev);
        }
    }
    return true;
}

// A unit whose rows fit one batch (at most 64 per wave) and whose pieces fit NPB per lane: rows, descriptors and pieces
// are read ONCE and stay in registers for all three sweeps (the streaming version pays the chain unit -> row of u -> rows'
// descriptors -> pieces three times, with a handful of pieces per wave to hide it behind).  false: does not fit (decided
// before anything is written; the caller streams).  `ok` is set like h2_node's return value.
// Class M (one partition, four waves) tries the row-mask path first for a unit of at most H2_ROWS_MAX rows.
constexpr int H2_NPB = 12;
template <int L1, int EXS, int NW, bool PARTS>
__device__ inline bool h2_node_fast(const View &g, const H2Tasks tk, H2Alloc &al, int u, int2 ru, int part, int nparts,
                                    const H2Tab t, H2Scratch *sc, uint4 *rec, bool &ok, H2List &ls) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
    constexpr int NT = 64 * NW, NP = H2_NPB;
    constexpr bool ROWS = !PARTS && NW == 4 && EXS >= 4 * H2_ROWS_EXS;
    const unsigned long long below = (1ull << lane) - 1ull;
    if (ru.y > 64 * NW) return false;  // uniform
    const bool rows = ROWS && ru.y <= H2_ROWS_MAX;  // uniform
    const int i = lane * NW + wid;
    int k = -1;
    int2 rk = make_int2(0, 0);
    if (i < ru.y) {
        k = g.col[ru.x + i];
        if (k >= 0 && k < g.n && k != u) {
            rk = g.rowinfo[k];
            if (!row_ok(g, rk, 32, k, u)) rk = make_int2(0, 0);
        } else {
            k = -1;
        }
    }
    const int np = rk.y > 0 ? ((rk.x + rk.y + 3) >> 2) - (rk.x >> 2) : 0;
    int poff_lane;
    const int P = h2_prefix(np, poff_lane);
    if (__syncthreads_or(P > 64 * NP)) return false;  // some wave's share is too long for the registers
    // the bitmaps and the tables of the path named: the block path's (key empty, counts zero) or the row-mask path's, which lie in
    // the same arrays (row masks zero where the keys are; exact keys empty, adjacency masks and row results zero where the counts are)
    auto clear = [&](bool for_rows) {
        const uint4 zero = make_uint4(0u, 0u, 0u, 0u), none = make_uint4(H2_EMPTY, H2_EMPTY, H2_EMPTY, H2_EMPTY);
        uint4 *z = reinterpret_cast<uint4 *>(t.b1);  // b1 and b2 are adjacent
        constexpr int NZ = ((1 << L1) / 32 + (1 << (L1 - 2)) / 32) / 4;
        for (int j = tid; j < NZ; j += NT) z[j] = zero;
        uint4 *k4 = reinterpret_cast<uint4 *>(t.key);
        for (int j = tid; j < EXS / 4; j += NT) k4[j] = for_rows ? zero : none;
        uint4 *c4 = reinterpret_cast<uint4 *>(t.cnt);
        for (int j = tid; j < EXS / 8; j += NT) c4[j] = (for_rows && j < H2_ROWS_EXS / 4) ? none : zero;
        if (tid == 0) {
            *t.full = 0;
            t.wsum[0] = 0;  // (the row-mask path's candidate count; the join writes its own before it reads)
        }
    };
    clear(rows);
    sc->desc[lane] = rk;
    sc->poff[lane] = poff_lane;
    if (lane == 0) sc->poff[64] = P;
    h2_wave_sync();
    // every piece of this wave's rows: meta = entries inside the row | those of this unit's key partition << 4 | row << 8 |
    // first slot of the piece << 16
    int4 w[NP];
    unsigned long long meta[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int j = 64 * q + lane;
        w[q] = make_int4(0, 0, 0, 0);
        meta[q] = 0ull;
        const int jf = 64 * q, jl = jf + 63 < P ? jf + 63 : P - 1;
        if (jf >= P) continue;  // uniform
        const int r = h2_piece_row(sc->poff, poff_lane, j < P ? j : jl, jf, jl);
        if (j < P) {
            const int2 d = sc->desc[r];
            const int a = (d.x & ~3) + 4 * (j - sc->poff[r]);
            w[q] = load_piece(g.col, a);
            meta[q] = (unsigned long long)h2_piece_mask(a, d.x, d.x + d.y) | ((unsigned long long)r << 8) | ((unsigned long long)(unsigned)a << 16);
        }
    }
    __syncthreads();  // the tables are cleared
    // the members of N(u): flagged table entries (in every partition's tables); both paths seed the same bits into the bitmaps
    auto seed_table = [&]() {
        const int sl = h2_insert<EXS>(t.key, (unsigned)k);
        if (sl < 0) *t.full = 1;
        else h2_cnt_flag(t.cnt, sl);
    };
    if (k >= 0) {
        if (rows) {  // uniform: the row-mask path's exact table, flagged too, with the member's position in row u
            const int sl = h2s_insert_nbr<H2_ROWS_EXS>(t.cnt, (unsigned)k);
            if (sl < 0) *t.full = 1;
            else t.key[4 * sl] = (unsigned)i;
        } else {
            seed_table();
        }
        h2_seed<L1>(t.b1, t.b2, (unsigned)k);
    }
    if (rows) sc->rowRev[lane] = -1;
    __syncthreads();
    // sweep A
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        if (64 * q >= P) continue;  // uniform
        const unsigned kk[4] = {(unsigned)w[q].x, (unsigned)w[q].y, (unsigned)w[q].z, (unsigned)w[q].w};
        unsigned valid = (unsigned)meta[q] & 0xFu & ~h2_eq4(kk, (unsigned)u);
        if (PARTS) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                if (h2_part(kk[jj], nparts) != part) valid &= ~(1u << jj);
        }
        meta[q] |= (unsigned long long)valid << 4;
        h2_mark4<L1>(t.b1, t.b2, kk, valid);
    }
    __syncthreads();
    if constexpr (ROWS) {
        if (rows) {  // uniform
            const bool done = h2_rows_unit<L1, EXS, NW, NP>(g, u, ru, i, k, P, w, meta, t, sc, rec);
            if (tid == 0) atomicAdd(&h2_rows_units[done ? 0 : 1], 1u);
            __syncthreads();  // the tables are rewritten: by the next unit, or right here
            if (done) {
                ok = true;
                return true;
            }
            // Its table or its list filled up and nothing is published: the block path takes the unit — no retry, no fallback, the
            // unit is counted where it would have been without the row-mask path.  Sweep A is common to both paths and B2 is as it
            // left it (B1, the candidate list since, is dead on the block path as well: the join's cursors are written before they
            // are read), so the block path starts from its own tables, cleared and seeded, and goes on with its sweep B.
            {
                uint4 *k4 = reinterpret_cast<uint4 *>(t.key);
                for (int j = tid; j < EXS / 4; j += NT) k4[j] = make_uint4(H2_EMPTY, H2_EMPTY, H2_EMPTY, H2_EMPTY);
                uint4 *c4 = reinterpret_cast<uint4 *>(t.cnt);
                for (int j = tid; j < EXS / 8; j += NT) c4[j] = make_uint4(0u, 0u, 0u, 0u);
                if (tid == 0) *t.full = 0;
            }
            __syncthreads();
            if (k >= 0) seed_table();
            __syncthreads();
        }
    }
    // Sweep B: flagged entries are queued, the drain has one call site.  It lists its exact-path entries (slot and row) and
    // where u sits in each row; the third step is then one pass over that list (h2_settle_items) — unless the list overflowed:
    // that wave streams its rows for the third sweep (h2_stream, the path of the units that do not fit the registers).
    int qn = 0, tbase = -1, trow = 0;
    sc->rowRev[lane] = -1;
    h2_wave_sync();
    {
        unsigned fl[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            fl[q] = 0u;
            if (64 * q >= P) continue;  // uniform
            const unsigned kk[4] = {(unsigned)w[q].x, (unsigned)w[q].y, (unsigned)w[q].z, (unsigned)w[q].w};
            const unsigned valid = (unsigned)(meta[q] >> 4) & 0xFu;
            // (where u sits in the row: the third step's, found while the pieces are at hand)
            const unsigned isu = h2_eq4(kk, (unsigned)u) & (unsigned)meta[q] & 0xFu;
            if (isu) sc->rowRev[(int)((meta[q] >> 8) & 0xFFull)] = (int)(meta[q] >> 16) + __ffs((int)isu) - 1;
            fl[q] = h2_again4<L1>(t.b2, kk, valid);
        }
#pragma unroll 1
        while (true) {
            bool stop = false;  // uniform: the queue is full, the rest waits for the drain
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                if (64 * q >= P) continue;  // uniform
                const unsigned kk[4] = {(unsigned)w[q].x, (unsigned)w[q].y, (unsigned)w[q].z, (unsigned)w[q].w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const bool p = (fl[q] >> jj) & 1u;
                    const unsigned long long m = __ballot(p);
                    if (m == 0ull) continue;  // uniform
                    if (stop || qn + __popcll(m) > H2_QCAP) {
                        stop = true;
                        continue;
                    }
                    if (p) {
                        const int idx = qn + __popcll(m & below);
                        sc->qw[idx] = kk[jj];
                        sc->qr[idx] = (unsigned char)((meta[q] >> 8) & 0xFFull);
                        sc->qb[idx] = 0;
                        fl[q] &= ~(1u << jj);
                    }
                    qn += __popcll(m);
                }
            }
            if (qn > 0) h2_drain<L1, EXS, 1, PARTS>(t, sc, qn, tk, al, -1, ls, part, nparts);
            if (!stop) break;
        }
    }
    __syncthreads();
    ok = *t.full == 0;  // uniform
    ls.join = !__syncthreads_or(ls.over) && ok;
    if (ls.join) ls.join = h2_join_prepare<L1, EXS, NW>(g, t, ru, ls);
    if (ls.join) {
        int lcur = 0;
        const int myrev = sc->rowRev[lane];
        h2_wave_sync();
        h2_batch_join<L1, EXS, NW, PARTS>(g, tk, al, u, ru, i, k, rk, part, t, sc, rec, ls, lcur, 0, myrev);
    } else if (ok) {
        if (tid == 0) atomicAdd(&tk.res->h2_fallback, 1);
        if (!ls.over) {  // uniform over the wave
            int lcur = 0;
            const int myrev = sc->rowRev[lane];
            h2_wave_sync();
            h2_batch_begin(tk, al, sc, k, tbase, trow, myrev);
            h2_wave_sync();
            h2_settle_items<L1, EXS>(t, sc, ls, lcur, 0, tk, al, tbase);
            h2_batch_end<L1, EXS, PARTS>(g, tk, al, u, ru, i, k, rk, tbase, trow, part, t, sc, rec, ls.items, 0, lcur);
        } else {
            h2_stream<L1, EXS, NW, PARTS, 2>(g, tk, al, u, ru, part, nparts, t, sc, rec, k, rk, ls);
        }
    }
    __syncthreads();  // the tables are rewritten by the next unit
    return true;
}

// one unit: node u, key partition `part` of `nparts`, by NW waves sharing the tables `t`; false: the table filled up
template <int L1, int EXS, int NW, bool PARTS>
__device__ inline bool h2_node(const View &g, const H2Tasks tk, H2Alloc &al, int u, int2 ru, int part, int nparts,
                               const H2Tab t, H2Scratch *sc, uint4 *rec, H2List &ls) {
    const int tid = (int)threadIdx.x;
    constexpr int NT = 64 * NW;
    if constexpr (!PARTS) {  // (with 16 waves per unit the registers it needs spill: measured slower for the split class)
        bool ok_fast = true;
        if (h2_node_fast<L1, EXS, NW, PARTS>(g, tk, al, u, ru, part, nparts, t, sc, rec, ok_fast, ls)) return ok_fast;
    }
    // this lane's row of the first batch of every sweep (requested before the tables are cleared)
    int k0 = -1;
    int2 rk0 = make_int2(0, 0);
    {
        const int i0 = (tid & 63) * NW + (tid >> 6);
        if (i0 < ru.y) {
            k0 = g.col[ru.x + i0];
            if (k0 >= 0 && k0 < g.n && k0 != u) {
                rk0 = g.rowinfo[k0];
                if (!row_ok(g, rk0, 32, k0, u)) rk0 = make_int2(0, 0);
            } else {
                k0 = -1;
            }
        }
    }
    {
        uint4 *z = reinterpret_cast<uint4 *>(t.b1);  // b1 and b2 are adjacent
        constexpr int NZ = ((1 << L1) / 32 + (1 << (L1 - 2)) / 32) / 4;
        for (int i = tid; i < NZ; i += NT) z[i] = make_uint4(0u, 0u, 0u, 0u);
        uint4 *k4 = reinterpret_cast<uint4 *>(t.key);
        for (int i = tid; i < EXS / 4; i += NT) k4[i] = make_uint4(H2_EMPTY, H2_EMPTY, H2_EMPTY, H2_EMPTY);
        uint4 *c4 = reinterpret_cast<uint4 *>(t.cnt);
        for (int i = tid; i < EXS / 8; i += NT) c4[i] = make_uint4(0u, 0u, 0u, 0u);
        if (tid == 0) *t.full = 0;
    }
    __syncthreads();
    for (int i = tid; i < ru.y; i += NT) {  // the members of N(u): flagged table entries (in every partition's tables)
        const int k = g.col[ru.x + i];
        if (k >= 0 && k < g.n && k != u) {
            const int s = h2_insert<EXS>(t.key, (unsigned)k);
            if (s < 0) *t.full = 1;
            else h2_cnt_flag(t.cnt, s);
            h2_seed<L1>(t.b1, t.b2, (unsigned)k);
        }
    }
    __syncthreads();
    h2_stream<L1, EXS, NW, PARTS, 0>(g, tk, al, u, ru, part, nparts, t, sc, rec, k0, rk0, ls);
    __syncthreads();
    h2_stream<L1, EXS, NW, PARTS, 1>(g, tk, al, u, ru, part, nparts, t, sc, rec, k0, rk0, ls);
    __syncthreads();
    const bool ok = *t.full == 0;  // uniform
    ls.join = !__syncthreads_or(ls.over) && ok;
    if (ls.join) ls.join = h2_join_prepare<L1, EXS, NW>(g, t, ru, ls);
    if (!ls.join && ok && tid == 0) atomicAdd(&tk.res->h2_fallback, 1);
    if (ok) h2_stream<L1, EXS, NW, PARTS, 2>(g, tk, al, u, ru, part, nparts, t, sc, rec, k0, rk0, ls);
    __syncthreads();  // the tables are rewritten by the next unit
    return ok;
}

// RETRY: the units come from the retry list (whose tables must not fill up again: the pass falls back then)
// (at least three waves per SIMD: class M's fast path wanted 232 registers, i.e. two of its 4-wave workgroups per CU where its
//  LDS lets three live; at 168 registers and 136 bytes of spills the pass was 2.6 % faster on S100k, 4.3 % on S1M.  With the
//  row-mask path class M stands at 168 registers, 41 spilled and 192 bytes of scratch per lane, 23 and 96 before it:
//  profiles/h2_rowmask_resources.txt, and profiles/h2_rowmask_ab.txt for what that costs the units of the other paths)
template <int L1, int EXS, int NW, bool PARTS>
__global__ void __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(3))) k_h2_block(View g, H2Tasks tk, const int4 *units, const int32_t *count, int64_t unit_cap,
                                                       uint4 *rec, H2Retry rt, int is_retry) {
    __shared__ __attribute__((aligned(16))) unsigned bits[(1 << L1) / 32 + (1 << (L1 - 2)) / 32];
    __shared__ __attribute__((aligned(16))) unsigned key[EXS];
    __shared__ __attribute__((aligned(16))) unsigned cnt[EXS / 2];
    __shared__ H2Scratch sc_all[NW];
    __shared__ int full;
    __shared__ int wsum[NW];
    const int wid = threadIdx.x >> 6;
    const int total = *count;
    if (total < 0 || total > unit_cap) {  // uniform
        row_ok(g, make_int2(-1, total), 37, 0, 0);
        return;
    }
    const H2Tab t{bits, bits + (1 << L1) / 32, key, cnt, &full, wsum};
    H2Alloc al;
    for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {  // every value steering the barriers is uniform
        const int4 un = units[it];
        const int u = un.x;
        const int nparts = PARTS ? (int)((unsigned)un.y >> 16) : 1, part = PARTS ? (un.y & 0xFFFF) : 0;
        bool ok = u >= 0 && u < g.n && nparts >= 1 && part < nparts;
        int2 ru = make_int2(0, 0);
        if (ok) {
            ru = g.rowinfo[u];
            ok = row_ok(g, ru, 38, u, (int)it) && ru.y > 0 && ru.y <= H2_MAXDEG;
        }
        if (!ok) continue;
        H2List ls = h2_list_of(tk.lists, NW);  // (fresh per unit)
        const bool unit_ok = h2_node<L1, EXS, NW, PARTS>(g, tk, al, u, ru, part, nparts, t, &sc_all[wid], rec, ls);
        if (!unit_ok) {
            if (threadIdx.x == 0) {  // every partition of the node is redone (the retry starts from zeroed records)
                if (is_retry) {
                    rt.res->h2_status = 1;
                    atomicAdd(&rt.res->h2_failed[5], 1);
                } else {
                    h2_retry_push(rt, u, ru.y, PARTS ? 4 : 3);
                }
            }
        }
    }
    h2_void_candidates(tk, al.c_cur, al.c_end);
    h2_void_tasks(tk, al.t_cur, al.t_end);
}

// how many of the partners pt[0..np) are adjacent to w: one probe of the edge set per pair, eight in flight, most of
// them settled by the edge bitmap
__device__ inline int h2_probe_partners(const H2EdgeSet es, int w, const int32_t *pt, int np) {
    int found = 0;
    for (int j = 0; j < np; j += 8) {
        int tt[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) tt[q] = j + q < np ? pt[j + q] : -1;
        unsigned long long key[8], k0[8], h[8];
        unsigned bw[8], bb[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            key[q] = h2_edge_key(w, tt[q] < 0 ? w : tt[q]);
            bb[q] = h2_bloom_bit(key[q], es.bloom_bits);
            bw[q] = es.bloom[bb[q] >> 5];
        }
        // few pairs pass the bitmap; those that do read their home slot of the edge set together, not one after the other
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const bool maybe = tt[q] >= 0 && ((bw[q] >> (bb[q] & 31u)) & 1u);
            h[q] = h2_eset_slot(key[q], es.bits);
            k0[q] = maybe ? es.tab[h[q]] : H2_ESET_EMPTY;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            bool hit = k0[q] == key[q];
            if (!hit && k0[q] != H2_ESET_EMPTY) hit = h2_eset_has(es, w, tt[q]);  // (rare: the home slot is someone else's)
            found += hit ? 1 : 0;
        }
    }
    return found;
}

// the listed (candidate, partner) pairs: a thread per candidate probes the edge set for each partner of its edge
// and adds its corrected count to the record of the edge; the candidates of an edge are adjacent, so lanes that share a
// record reduce first
// Launched twice: `second` = 0 as soon as the block classes have finished (beside the wave classes, which list nothing),
// for the candidates there are then; `second` = 1 after the retry launch for what that one listed.  (The split is read
// from / left in the result block: h2_ncand_done is only written by the kernel that marks the first launch's end.)
// (Round 4: the first launch of a pool takes the candidates there are and records their number itself — a one-thread kernel did
//  that before, and behind the split class on the main stream it took 20-50 us to get a wave.)
__global__ void __launch_bounds__(256) k_h2_triangles(H2EdgeSet es, H2Tasks tk, uint4 *rec, const int32_t *status, int second) {
    const int cand_now = *tk.n_cand;  // (stable: the kernels that list into this pool are through)
    const int first = second ? *tk.n_done : 0;
    // Round 5 (found by the randomised sweep, one pass in ~1,500 on a graph whose pools had just been grown to what the pass before
    // had counted): the counter advances by whole CHUNKS, so it can pass the end of the pool although every reservation fitted —
    // no status is raised then (h2_pool_reserve fails only when c0 + nc exceeds the pool) and nothing lies beyond the pool.  This
    // kernel used to take "counter beyond the pool" for a failed pass and return: a pass that was NOT run again lost every
    // correction of this launch.  A reservation that did not fit has set the status, which is checked right below.
    const int total = cand_now < tk.cand_cap ? cand_now : (int)tk.cand_cap;
    if (!second && blockIdx.x == 0 && threadIdx.x == 0) *tk.n_done = cand_now;  // read by the retry stage's launch only
    if (*status != 0) return;
    if (total <= first || first < 0) return;
    const int lane = threadIdx.x & 63;
    for (int64_t base = first + (((int64_t)blockIdx.x * 256 + threadIdx.x) & ~63ll); base < total; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + lane;
        int c = 0;
        unsigned slot = 0xFFFFFFFFu;
        if (i < total) {
            const int4 cd = tk.cand[i];
            const uint4 ts = (cd.z >= 0 && cd.z < tk.task_cap) ? tk.task[cd.z] : make_uint4(0u, 0u, H2_TASK_VOID, 0u);  // (void: the tail of a wave's chunk)
            // (a split node some partition of which failed is redone as a whole: what its other partitions listed is void)
            const bool skip = ts.z == H2_TASK_VOID || (!(ts.w & 0x80000000u) && ((unsigned)tk.weight[ts.w & 0x7FFFFFFFu] & 0x80000000u));
            if (!skip) {
                slot = ts.x;
                c = cd.y - h2_probe_partners(es, cd.x, tk.part + ts.y, (int)ts.z);
            }
        }
        // the candidates of an edge are adjacent: one pair of atomics per run of equal record slots (segmented scan)
        const unsigned prev = (unsigned)__shfl_up((int)slot, 1);
        const bool head = lane == 0 || prev != slot;
        const unsigned long long heads = __ballot(head);
        const int seg = __popcll(heads & ((2ull << lane) - 1ull));
        int n = c > 0 ? 1 : 0, mx = c > 0 ? c : 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int s2 = __shfl_up(seg, off), n2 = __shfl_up(n, off), m2 = __shfl_up(mx, off);
            if (lane >= off && s2 == seg) {
                n += n2;
                mx = m2 > mx ? m2 : mx;
            }
        }
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (tail && n > 0 && slot != 0xFFFFFFFFu) {
            unsigned *r4 = reinterpret_cast<unsigned *>(rec + slot);
            atomicAdd(&r4[0], (unsigned)n);
            atomicMax(&r4[1], (unsigned)mx);
        }
    }
}

// Σ_{k in N(u)} deg(k) for every u: a thread per adjacency slot, run-length sums inside a wave (rows are contiguous),
// one atomic per run
__global__ void __launch_bounds__(256) k_h2_weight(View g, int32_t *weight) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int u = -1, val = 0;
    if (s < g.cap_total) {
        // two rounds of loads, not four: the slot's row and neighbour first (both in bounds for every slot), then the two
        // row headers; what the slot holds is validated afterwards (slack behind a row holds -1)
        const int us = g.slot_row[s];
        const int v = g.col[s];
        const bool uok = us >= 0 && us < g.n, vok = v >= 0 && v < g.n;
        const int2 ru = g.rowinfo[uok ? us : 0];
        const int dv = g.rowinfo[vok ? v : 0].y;
        if (uok) {
            u = us;
            if (vok && s >= ru.x && (int)(s - ru.x) < ru.y) val = dv;
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(val, off), uu = __shfl_up(u, off);
        if (lane >= off && uu == u) val += t;
    }
    const int un = __shfl_down(u, 1);
    if (u >= 0 && val > 0 && (lane == 63 || un != u)) atomicAdd(&weight[u], val);
}

// ---- plan: class, partitions and weight bucket per node; units laid out heaviest bucket first inside each class -------
constexpr int H2_NB = H2_CLASSES * H2_WB;
// the per-pass fields of the result block and bucket half `half`, by the first threads of one workgroup (tid: at least H2_NB)
__device__ inline void h2_clear_result(DevResult *res, int tid, int half, bool flags_cleared) {
    if (tid == 0 && flags_cleared) res->touched_n = 0;   // (the list of flagged nodes goes with the flags)
    if (tid < 8) res->misc[tid] = 0;
    if (tid < H2_NB) {
        res->h2_bucket[half][tid] = 0;
        res->h2_fill[half][tid] = 0;
    }
    if (tid < H2_CLASSES) res->h2_count[tid] = 0;
    if (tid == 0) {
        res->h2_status = 0;
        res->h2_retry = 0;
        for (int p = 0; p < 2; ++p) res->h2_ntask[p] = res->h2_ncand[p] = res->h2_npart[p] = res->h2_ncand_done[p] = 0;
        for (int c = 0; c < 6; ++c) res->h2_failed[c] = 0;
        res->h2_fallback = 0;
        res->flag_too_big = 0;
    }
}
struct H2Lists {
    int4 *units[H2_CLASSES];  // {node, partitions << 16 | partition, row start, degree}
    int64_t cap[H2_CLASSES];
};
constexpr int H2_PLAN_THREADS = 1024;

__device__ inline void h2_classify(int d, int S, int &cls, int &wb, int &nparts) {
    nparts = 1;
    int lo = 0;
    if (d <= H2_SMALL_DEG && S <= h2_maxw(2)) {
        cls = S <= h2_maxw(0) ? 0 : S <= h2_maxw(1) ? 1 : 2;
        lo = cls == 0 ? 0 : h2_maxw(cls - 1);
        wb = (int)((int64_t)(S - lo) * H2_WB / (h2_maxw(cls) - lo + 1));
    } else if (S <= h2_maxw(3) && d + S / 4 <= h2_keycap(3)) {
        cls = 3;
        wb = S < 2048 ? 0 : S < 4096 ? 1 : S < 6144 ? 2 : 3;
    } else {
        cls = 4;
        nparts = h2_parts_for(d, S, false);
        wb = S < 16384 ? 0 : S < 32768 ? 1 : S < 65536 ? 2 : 3;
    }
    if (wb > H2_WB - 1) wb = H2_WB - 1;
    if (wb < 0) wb = 0;
}

// PHASE 0 counts the units per bucket, PHASE 1 places them.  Both work in half `parity` of DevResult::h2_bucket / h2_fill.
// PHASE 0 also takes the retry mark of the last pass (bit 31, h2_retry_push) off the weights it reads: the weights are kept from
// pass to pass (dev_weight_edit), the mark belongs to one.
// `head` != 0: the pass has no k_h2_clear and no k_h2_retry_zero ahead of the class kernels, their work is done here.  PHASE 0
// zeroes the node flags of the incremental pass, and its workgroup 0 the bucket half of the NEXT pass and the per-pass fields of
// the result block (none is read or written before PHASE 1; this half was left zero by the pass before, or by k_h2_clear);
// PHASE 1 zeroes the records of the nodes it puts into the split class (their partitions add into them), a wave per row.
// `journal` != 0 (PHASE 1 only, with either head): the edge set is kept and edits are pending.  The launch then has ONE
// workgroup more than the nodes need — none of its threads has a node to place — and that workgroup's first thread applies the
// journal before anything else.  No plan kernel reads the edge set, the block classes that probe it are launched behind this
// kernel on every stream, and the per-pass fields of the result block (the status among them) were cleared by the kernel before.
template <int PHASE>
__global__ void __launch_bounds__(H2_PLAN_THREADS) k_h2_plan(View g, int32_t *weight, H2Lists L, DevResult *res, int parity, int head,
                                                             unsigned *dirty_words, int64_t n_dirty_words, uint4 *rec, H2EdgeSet es,
                                                             int journal) {
    __shared__ int blk_count[H2_NB];
    __shared__ int blk_base[H2_NB];
    const int u = blockIdx.x * H2_PLAN_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (PHASE == 1 && journal && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) h2_eset_apply(es, res, &res->h2_status);
    if (threadIdx.x < H2_NB) blk_count[threadIdx.x] = 0;
    __syncthreads();
    int bkt = -1, cls = -1, wb = 0, nparts = 0;
    int2 ru = make_int2(0, 0);
    if (u < g.n) {
        ru = g.rowinfo[u];
        const int d = ru.y;
        const int wraw = weight[u];
        if (PHASE == 0 && wraw < 0) weight[u] = wraw & 0x7FFFFFFF;
        if (d > 0 && d <= H2_MAXDEG) {
            h2_classify(d, wraw & 0x7FFFFFFF, cls, wb, nparts);
            bkt = cls * H2_WB + wb;
        }
    }
    if (PHASE == 0 && head) {
        const int64_t stride = (int64_t)gridDim.x * H2_PLAN_THREADS;
        for (int64_t i = (int64_t)blockIdx.x * H2_PLAN_THREADS + threadIdx.x; i < n_dirty_words; i += stride) dirty_words[i] = 0u;
        if (blockIdx.x == 0) h2_clear_result(res, (int)threadIdx.x, 1 - parity, n_dirty_words > 0);
    }
    const int nunits = bkt < 0 ? 0 : nparts;
    int my_off = 0;
    for (int b = 0; b < H2_NB; ++b) {
        const unsigned long long m = __ballot(bkt == b);
        if (m == 0) continue;
        int incl = bkt == b ? nunits : 0;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        const int tot = __shfl(incl, 63);
        int wave_off = 0;
        if (lane == 0) wave_off = atomicAdd(&blk_count[b], tot);
        wave_off = __shfl(wave_off, 0);
        if (bkt == b) my_off = wave_off + incl - nunits;
    }
    __syncthreads();
    if (threadIdx.x < H2_NB) {
        const int b = threadIdx.x, c = blk_count[b];
        if (PHASE == 0) {
            if (c) atomicAdd(&res->h2_bucket[parity][b], c);
        } else {
            int before = 0;
            for (int h = b + 1; h < H2_NB; ++h)  // heavier buckets of the same class come first
                if (h / H2_WB == b / H2_WB) before += res->h2_bucket[parity][h];
            blk_base[b] = before + (c ? atomicAdd(&res->h2_fill[parity][b], c) : 0);
        }
    }
    if (PHASE == 0) return;
    if (blockIdx.x == 0 && threadIdx.x >= 64 && threadIdx.x < 64 + H2_CLASSES) {
        const int c = (int)threadIdx.x - 64;
        int64_t tot = 0;
        for (int b = c * H2_WB; b < (c + 1) * H2_WB; ++b) tot += res->h2_bucket[parity][b];
        if (tot > (c == 0 ? L.cap[0] : c == 1 ? L.cap[1] : c == 2 ? L.cap[2] : c == 3 ? L.cap[3] : L.cap[4])) {  // the list cannot hold them: nothing of this class runs, the pass is redone elsewhere
            res->h2_status = 1;
            tot = 0;
        }
        res->h2_count[c] = (int)tot;
    }
    __syncthreads();
    if (bkt >= 0) {
        const int64_t first = (int64_t)blk_base[bkt] + my_off;
        // (selects, not L.units[cls]: indexing a kernel argument with a run-time value puts the whole struct into scratch)
        int4 *dst = cls == 0 ? L.units[0] : cls == 1 ? L.units[1] : cls == 2 ? L.units[2] : cls == 3 ? L.units[3] : L.units[4];
        const int64_t cap = cls == 0 ? L.cap[0] : cls == 1 ? L.cap[1] : cls == 2 ? L.cap[2] : cls == 3 ? L.cap[3] : L.cap[4];
        static_assert(H2_CLASSES == 5, "the selects above list the classes");
        if (nparts <= 65535 && first >= 0 && first + nunits <= cap) {
            for (int j = 0; j < nunits; ++j) dst[first + j] = make_int4(u, (nparts << 16) | j, ru.x, ru.y);
        } else if (nparts > 65535) {
            res->h2_status = 1;
        }  // (else: reported through h2_count / h2_status above)
    }
    if (!head) return;  // (uniform: k_h2_retry_zero follows)
    // Not the nodes this thread's wave has just placed: the split nodes of a power-law graph are its first few hundred ids, one
    // workgroup's, whose 16 waves then zero every long row of the graph one after the other (measured: 39 us for this kernel
    // instead of 10).  The nodes are dealt out again for this step, eight consecutive ids (one 64-byte piece of the row headers)
    // to eight lanes and the pieces round-robin over the workgroups, then the waves, then the lane groups: a run of 8 * G * 16
    // consecutive ids has no two pieces in one wave.  Every node below 1,024 * G is looked at by exactly one lane.
    const int64_t piece = (int64_t)((lane >> 3) * (H2_PLAN_THREADS / 64) + (int)(threadIdx.x >> 6)) * gridDim.x + blockIdx.x;
    const int64_t z = piece * 8 + (lane & 7);
    int2 rz = make_int2(0, 0);
    bool is_split = false;
    if (z < g.n) {
        rz = g.rowinfo[z];
        if (rz.y > 0 && rz.y <= H2_MAXDEG) {
            int zc, zb, zp;
            h2_classify(rz.y, weight[z] & 0x7FFFFFFF, zc, zb, zp);
            is_split = zc == 4;
        }
    }
    unsigned long long split = __ballot(is_split);
    while (split) {
        const int src = __ffsll((long long)split) - 1;
        split &= split - 1ull;
        const int2 rs = make_int2(__shfl(rz.x, src), __shfl(rz.y, src));
        if (!row_ok(g, rs, 42, __shfl((int)z, src), -1)) continue;
        for (int i = lane; i < rs.y; i += 64) rec[(int64_t)rs.x + i] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// (round 4: also zeroes the weights — a fill launch of its own before; n = 0 when the weights are kept: dcr_graph::h2_weight_valid)
// The stand-alone head of a pass whose result block is not known to be ready (dcr_graph::h2_head_clean) or whose weights have to
// be computed: both bucket halves start from zero.
__global__ void __launch_bounds__(256) k_h2_clear(DevResult *res, int32_t *weight, int64_t n, unsigned *dirty_words, int64_t n_dirty_words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) weight[i] = 0;
    // (the incremental pass's per-node flags: a full pass recomputes every edge, so they can go now — a fill launch at the
    //  tail of every pass before)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_dirty_words; i += (int64_t)gridDim.x * 256) dirty_words[i] = 0u;
    if (blockIdx.x != 0) return;
    h2_clear_result(res, (int)threadIdx.x, 0, n_dirty_words > 0);
    h2_clear_result(res, (int)threadIdx.x, 1, n_dirty_words > 0);
}

// the records of the nodes on the retry list start from zero again (a split node's partitions add into them)
__global__ void __launch_bounds__(256) k_h2_retry_zero(View g, const int4 *units, const int32_t *count, int64_t unit_cap, uint4 *rec) {
    const int total = *count;
    if (total <= 0 || total > unit_cap) return;
    for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const int4 un = units[it];
        if ((un.y & 0xFFFF) != 0 || un.x < 0 || un.x >= g.n) continue;
        const int2 ru = g.rowinfo[un.x];
        if (!row_ok(g, ru, 42, un.x, (int)it)) continue;
        for (int i = threadIdx.x; i < ru.y; i += 256) rec[(int64_t)ru.x + i] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// ---- join the two records of every edge and evaluate the closing expression ------------------------------------------
// Round 4: a fixed grid walks the slots and every WAVE leaves the first minimum and the first maximum (value, slot) of what
// it wrote: the arg-min that follows every pass of the SDRF loop (sdrf_no_cuda.py:27) and the stale arg-max of its removal
// step (:57-61) are then one small reduction each instead of two more sweeps over the slots.  (Per wave, not per workgroup:
// with a barrier at the end a workgroup holds its place until its slowest wave's gathers are back — measured, the kernel
// took 137-268 us instead of 60, growing with the number of workgroups.)  The partner slot's record is only fetched by the
// lanes whose slot holds a value (neighbour id above the row id) — under the execution mask, not from a clamped index:
// half the lanes of every wave asking for element 0 of five arrays is a hot spot of its own.
#ifndef H2_FINAL_Q
#define H2_FINAL_Q 1
#endif
#ifndef H2_FINAL_BLOCKS
#define H2_FINAL_BLOCKS 1024   // (x 4 waves = 4,096 pairs of partial extrema: the reduction that follows is one workgroup)
#endif
// `when` = 0: the pass was launched WITHOUT its retry stage (no pass of this graph has needed it so far: three launches and a
// stream join less on the critical path of every pass); should the retry list turn out not to be empty, nothing is written,
// status 3 is left and the host runs the pass again with the stage.  `when` = 1: behind the retry stage, unconditionally.
// `tri_stage` = 0: the pass was launched WITHOUT its k_h2_triangles launches (no pass of this graph has had a block-class unit on
// the probe path so far); should some unit have listed for them after all, its records lack their corrections: nothing is
// written, status 4 is left and the host runs the pass again with the launches.
__global__ void __launch_bounds__(256) k_h2_final(View g, const uint4 *rec, double *curv, const int32_t *status, Ext *part_min,
                                                  Ext *part_max, const int32_t *retry_count, int when, const int32_t *fallback_count,
                                                  int tri_stage) {
    if (when == 0 && *retry_count > 0) {  // uniform (the count is final once the class kernels are through)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicCAS(const_cast<int32_t *>(status), 0, 3);
        return;
    }
    if (tri_stage == 0 && *fallback_count > 0) {  // uniform (final as well: the class kernels and the retry launch are through)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicCAS(const_cast<int32_t *>(status), 0, 4);
        return;
    }
    double lo_v = 0.0, hi_v = 0.0;
    int lo_s = -1, hi_s = -1;
    const bool live = *status == 0;  // (else some records are missing: the whole pass is redone by the node-centric kernels)
    const int64_t stride = (int64_t)gridDim.x * 256;
    constexpr int Q = H2_FINAL_Q;
    for (int64_t s0 = (int64_t)blockIdx.x * 256 + threadIdx.x; live && s0 < g.cap_total; s0 += Q * stride) {
        // Round one: everything addressed by the slot itself (its row, its neighbour, its record — all in bounds for every
        // slot, slack included).  Round two, for the slots that may hold a value: the two row headers, the partner slot's
        // neighbour, row and record.  Validity is decided afterwards.
        int u[Q], v[Q];
        uint4 a[Q];
        bool want[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int64_t s = s0 + q * stride;
            const bool in = s < g.cap_total;
            u[q] = in ? g.slot_row[s] : -1;
            v[q] = in ? g.col[s] : -1;
            a[q] = in ? rec[s] : make_uint4(0u, 0u, 0u, 0u);  // from u's side: statistics over N(v) \ N(u) \ {u}
        }
        int2 ru[Q];
        int dv[Q], rcol[Q], rrow[Q];
        uint4 b[Q];
        bool rok[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            // the value lives at the slot whose neighbour id exceeds the row id
            want[q] = u[q] >= 0 && u[q] < g.n && v[q] > u[q] && v[q] < g.n;
            const int64_t r = (int64_t)a[q].w;
            rok[q] = want[q] && r >= 0 && r < g.cap_total;
            ru[q] = make_int2(0, 0);
            dv[q] = 0;
            rcol[q] = rrow[q] = -1;
            b[q] = make_uint4(0u, 0u, 0u, 0u);
            if (want[q]) ru[q] = g.rowinfo[u[q]];   // (consecutive slots share it; v's degree comes with the partner record)
            if (rok[q]) {
                // (the partner slot's record points back at this slot — its own sweep found u in v's row where this one found v
                //  in u's: checked below in place of reading the partner slot's row and neighbour, two more random reads per
                //  edge of the four this kernel made; slot 0 alone keeps the old check, a record of zeros would point at it)
                b[q] = rec[r];  // from v's side: statistics over N(u) \ N(v) \ {v}
                dv[q] = (int)(b[q].z >> 16);
                if (s0 + q * stride == 0) {
                    rcol[q] = g.col[r];
                    rrow[q] = g.slot_row[r];
                } else {
                    rcol[q] = (int64_t)b[q].w == s0 + q * stride ? u[q] : -1;
                    rrow[q] = v[q];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int64_t s = s0 + q * stride;
            if (!want[q]) continue;
            if (s < ru[q].x || (int)(s - ru[q].x) >= ru[q].y) continue;  // slack behind the row
            double val;
            if (ru[q].y == 1 || (rok[q] && dv[q] == 1)) {  // bfc_naive.py:18-19
                val = 0.0;
            } else {
                if (!rok[q] || rcol[q] != u[q] || rrow[q] != v[q]) {
                    row_ok(g, make_int2(-1, (int)a[q].w), 39, u[q], v[q]);
                    continue;
                }
                if ((a[q].z & 0xFFFFu) != (b[q].z & 0xFFFFu) || (int)(a[q].z >> 16) != ru[q].y) {  // both sides count the same triangles
                    row_ok(g, make_int2(-1, (int)a[q].z), 40, u[q], v[q]);
                    continue;
                }
                const int gam = (int)(a[q].y > b[q].y ? a[q].y : b[q].y);
                val = bfc_formula(ru[q].y, dv[q], (int)(a[q].z & 0xFFFFu), (int)b[q].x, (int)a[q].x, gam);
            }
            curv[s] = val;
            ext_take(lo_v, lo_s, val, (int)s, 0);
            ext_take(hi_v, hi_s, val, (int)s, 1);
        }
    }
    ext_wave_reduce(lo_v, lo_s, 0);
    ext_wave_reduce(hi_v, hi_s, 1);
    if ((threadIdx.x & 63) == 0) {
        const int w = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
        part_min[w] = ext_make(lo_v, lo_s);
        part_max[w] = ext_make(hi_v, hi_s);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// the pools of the triangle step were too small for the last pass: remember what it asked for (the counters kept counting)
bool h2_grow_pools(dcr_graph *g) {
    const DevResult &h = *g->hres.p;  // (per pool; both pools have the same size)
    const int64_t t = std::max(h.h2_ntask[0], h.h2_ntask[1]), c = std::max(h.h2_ncand[0], h.h2_ncand[1]), p = std::max(h.h2_npart[0], h.h2_npart[1]);
    if (h.h2_ntask[0] < 0 || h.h2_ntask[1] < 0 || h.h2_ncand[0] < 0 || h.h2_ncand[1] < 0 || h.h2_npart[0] < 0 || h.h2_npart[1] < 0) return false;
    if (t < 0 || c < 0 || p < 0) return false;  // the 31-bit counters wrapped: not a case for this engine
    // (a pass that ran out of one pool stopped listing into the others too: ask for twice what it counted)
    g->h2_want[0] = std::max<int64_t>(g->h2_want[0], 2 * t + 4096);
    g->h2_want[1] = std::max<int64_t>(g->h2_want[1], 2 * c + 65536);
    g->h2_want[2] = std::max<int64_t>(g->h2_want[2], 2 * p + 65536);
    return true;
}

static int ensure_h2(dcr_graph *g) {
    if (g->h2_weight.cap < g->n + 64) g->h2_weight_valid = false;  // a new array: k_h2_weight fills it
    DCR_TRY(g->h2_weight.grow(g->n + 64));
    DCR_TRY(g->h2_rec.grow(g->cap_total + 64));
    // edge set: at most cap_total / 2 undirected edges, load <= 1/2
    int bits = 10;
    while ((1ll << bits) < g->cap_total) ++bits;
    if (g->h2_eset_bits != bits || !g->h2_eset.p) {
        DCR_TRY(g->h2_eset.alloc((int64_t)1 << bits));
        g->h2_eset_bits = bits;
        g->h2_eset_valid = false;
    }
    int bbits = 16;
    while ((1ll << bbits) < 4 * g->cap_total) ++bbits;
    if (g->h2_bloom_bits != bbits || !g->h2_bloom.p) {
        DCR_TRY(g->h2_bloom.alloc(((int64_t)1 << bbits) / 32));
        g->h2_bloom_bits = bbits;
        g->h2_eset_valid = false;
    }
    const int64_t need[H2_CLASSES] = {g->n + 64, g->n + 64, g->n + 64, g->n + 64, g->n + g->cap_total / 4 + 64};
    for (int c = 0; c < H2_CLASSES; ++c) DCR_TRY(g->h2_units[c].grow(need[c]));
    DCR_TRY(g->h2_retry.grow(g->n + g->cap_total / 4 + 64));
    // triangle step pools: tasks are edges (with the partitions of split nodes: a few times that), candidates and partners
    // adjacency entries of theirs
    // (sized for power-law graphs; a pass that needs more says how much — h2_grow_pools — and is run again)
    // (two pools of each kind, the arrays hold both: see DevResult)
    DCR_TRY(g->h2_task.grow(2 * std::max<int64_t>(g->cap_total + 4096, g->h2_want[0])));
    DCR_TRY(g->h2_cand.grow(2 * std::max<int64_t>(2 * g->cap_total + 65536, g->h2_want[1])));
    DCR_TRY(g->h2_part.grow(2 * std::max<int64_t>(g->cap_total + 65536, g->h2_want[2])));
    // the third step's per-wave lists: the split class (one workgroup of 16 waves per CU; the retry launch reuses its part)
    // and class M (three workgroups of 4 waves per CU)
    const int cus = g->num_cu > 0 ? g->num_cu : 256;
    DCR_TRY(g->h2_lists.grow((int64_t)cus * (16 + 12) * H2_LIST_WORDS));
    return DCR_OK;
}

template <int C>
static void launch_h2_small(dcr_graph *g, const View &vw, const H2Retry &rt, hipStream_t st) {
    constexpr int H2_WPB = h2_wpb(C);
    constexpr int NP = h2_maxw(C) / 256 + 1;  // 64-piece steps: W / 4 pieces and at most one more per row (alignment)
    auto kern = k_h2_small<h2_l1(C), h2_exs(C), h2_clcap(C), H2_WPB, NP>;
    // workgroups a CU holds at once (LDS and registers): the units are dealt to the workgroups up front (grid-stride), so a
    // workgroup that has to wait for a place still has its whole share ahead of it — launch what is resident, no more
    static int per_cu_res = 0;
    if (per_cu_res == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 64 * H2_WPB, 0) != hipSuccess || nb < 1) {
            (void)hipGetLastError();
            nb = (160 * 1024) / (H2_WPB * (int)sizeof(H2Small<h2_l1(C), h2_exs(C), h2_clcap(C)>));
            if (nb > 32 / H2_WPB) nb = 32 / H2_WPB;
        }
        per_cu_res = nb < 1 ? 1 : nb;
    }
    int64_t grid = (int64_t)g->num_cu * per_cu_res;
    const int64_t units = g->h2_last_count[C] >= 0 ? (int64_t)g->h2_last_count[C] + g->h2_last_count[C] / 32 + 8 : g->n;
    if (grid > (units + H2_WPB - 1) / H2_WPB) grid = (units + H2_WPB - 1) / H2_WPB;  // small graphs: no idle workgroups
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * H2_WPB), 0, st, vw,
                       g->h2_units[C].p, &g->dres.p->h2_count[C], g->h2_units[C].cap, g->h2_rec.p, rt);
}

template <int C, bool PARTS>
static void launch_h2_block(dcr_graph *g, const View &vw, const H2Tasks &tk, const H2Retry &rt, const int4 *units,
                            const int32_t *count, int64_t cap, int64_t units_hint, int is_retry, hipStream_t st) {
    // (at most the workgroups the list pool has places for: one of the split class, three of class M per CU)
    int64_t grid = units_hint;
    const int64_t most = (int64_t)g->num_cu * (C == 3 ? 3 : 1);
    if (grid > most) grid = most;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL((k_h2_block<h2_l1(C), h2_exs(C), h2_waves(C), PARTS>), dim3((unsigned)grid), dim3(64 * h2_waves(C)), 0,
                       st, vw, tk, units, count, cap, g->h2_rec.p, rt, is_retry);
}

int launch_curvature_pass_h2(dcr_graph *g) {
    if (g->num_cu <= 0) {
        g->num_cu = 256;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, g->device) == hipSuccess && prop.multiProcessorCount > 0)
            g->num_cu = prop.multiProcessorCount;
    }
    DCR_TRY(ensure_h2(g));
    View vw{g->rowinfo.p, g->col.p, g->slot_row.p, g->cap_total, g->dres.p->misc, nullptr, (int32_t)g->n, 0};
    H2Lists L;
    for (int c = 0; c < H2_CLASSES; ++c) {
        L.units[c] = g->h2_units[c].p;
        L.cap[c] = g->h2_units[c].cap;
    }
    int32_t *status = &g->dres.p->h2_status;
    const H2Retry rt{g->h2_retry.p, g->h2_retry.cap, g->h2_weight.p, g->dres.p};
    const int64_t tcap = g->h2_task.cap / 2, ccap = g->h2_cand.cap / 2, pcap = g->h2_part.cap / 2;
    DevResult *dr = g->dres.p;
    unsigned *lists_L = g->h2_lists.p, *lists_M = g->h2_lists.p + (int64_t)g->num_cu * 16 * H2_LIST_WORDS;
    const H2EdgeSet es{g->h2_eset.p, g->h2_eset_bits, g->h2_bloom.p, g->h2_bloom_bits};
    H2Tasks tk{g->h2_task.p, g->h2_cand.p, g->h2_part.p, tcap, ccap, pcap, &dr->h2_ntask[0], &dr->h2_ncand[0], &dr->h2_npart[0],
               &dr->h2_ncand_done[0], g->dres.p, g->h2_weight.p, 0u, lists_L, es};  // pool 0: the split class and the retry launch
    const H2Tasks tkM{g->h2_task.p + tcap, g->h2_cand.p + ccap, g->h2_part.p + pcap, tcap, ccap, pcap, &dr->h2_ntask[1], &dr->h2_ncand[1],
                      &dr->h2_npart[1], &dr->h2_ncand_done[1], g->dres.p, g->h2_weight.p, 0u, lists_M, es};  // pool 1: class M
    // The head of the pass.  Steady state (the weights are kept by the edit kernels and the last pass left the result block
    // ready): the two plan kernels and nothing else, they clear what has to be cleared on their way.  Otherwise the stand-alone
    // k_h2_clear first (both bucket halves, and the weights when they have to be computed), k_h2_weight if so, the plan kernels
    // and k_h2_retry_zero.  Like SdrfScratch::table_dirty, h2_head_clean is dropped here and set again once everything that
    // makes it true is enqueued; whoever reads a status behind the pass drops it again (curvature_pass_impl).
    const int64_t sblocks = (g->cap_total + 255) / 256;
    const int64_t pblocks = (g->n + H2_PLAN_THREADS - 1) / H2_PLAN_THREADS;
    // (dirty: n bytes, allocated in whole words? — only the whole words are zeroed here, the caller's fill takes the rest)
    const bool whole = g->n % 4 == 0;
    unsigned *dirty_words = reinterpret_cast<unsigned *>(g->dirty.p);
    const int64_t n_dirty_words = whole ? g->n / 4 : (int64_t)0;
    const bool run_weight = !g->h2_weight_valid;
    const bool fast_head = !run_weight && g->h2_head_clean && pblocks > 0;
    const int parity = g->h2_parity & 1;
    g->h2_head_clean = false;
    if (!fast_head) {
        const int64_t cb = (g->n + 255) / 256;
        hipLaunchKernelGGL(k_h2_clear, dim3((unsigned)(cb < 1 ? 1 : cb > 2048 ? 2048 : cb)), dim3(256), 0, g->stream, g->dres.p, g->h2_weight.p,
                           run_weight ? g->n : (int64_t)0, dirty_words, n_dirty_words);
        if (run_weight && sblocks > 0) hipLaunchKernelGGL(k_h2_weight, dim3((unsigned)sblocks), dim3(256), 0, g->stream, vw, g->h2_weight.p);
        g->h2_weight_valid = true;  // (from here on the edit kernels keep them)
    }
    g->h2_cleared_dirty = whole;
    // the edge set (probed by the block classes only): kept from the last pass and patched with the journaled edits by one
    // thread of k_h2_plan<1>, ahead of the fork, or rebuilt on the aux stream beside the class kernels (32 MB of fill and a
    // million atomics: 0.17 ms of chip time per pass on the bench graph).  (No plan kernel, no nodes: nothing to patch with.)
    const bool patch = pblocks > 0 && g->h2_eset_valid && g->h2_eset_pending <= EDIT_LOG_CAP &&
                       g->h2_eset_tombs + g->h2_eset_pending <= ((int64_t)1 << g->h2_eset_bits) / 16;
    const bool journal = patch && g->h2_eset_pending > 0;
    if (pblocks > 0) {
        hipLaunchKernelGGL(k_h2_plan<0>, dim3((unsigned)pblocks), dim3(H2_PLAN_THREADS), 0, g->stream, vw, g->h2_weight.p, L,
                           g->dres.p, parity, fast_head ? 1 : 0, dirty_words, n_dirty_words, g->h2_rec.p, es, 0);
        hipLaunchKernelGGL(k_h2_plan<1>, dim3((unsigned)(pblocks + (journal ? 1 : 0))), dim3(H2_PLAN_THREADS), 0, g->stream, vw,
                           g->h2_weight.p, L, g->dres.p, parity, fast_head ? 1 : 0, dirty_words, n_dirty_words, g->h2_rec.p, es, journal ? 1 : 0);
    }
    // records of split nodes are accumulated with atomics: start from zero (the fast head: k_h2_plan<1> has done it)
    if (!fast_head)
        hipLaunchKernelGGL(k_h2_retry_zero, dim3(1024), dim3(256), 0, g->stream, vw, g->h2_units[4].p, &g->dres.p->h2_count[4], g->h2_units[4].cap,
                           g->h2_rec.p);
    g->h2_parity = 1 - parity;  // (the half of this pass is used; the other one is zero: k_h2_clear, or k_h2_plan<0> of this pass)
    g->h2_weight_launches += run_weight ? 1 : 0;
    g->h2_clear_launches += fast_head ? 0 : 1;
    // The stream each class kernel is launched on ({split class, class M, wave classes 2, 1, 0}: an index into `pool`; kernels on
    // one stream run one after the other).  The split class stays on the main stream, launched first: its workgroups need most
    // of a CU's LDS and find no CU free once the other kernels are resident (measured: started 60 us late, finished last).
    // Round 5: five persistent full-chip kernels on five streams do not run five abreast anyway (the runtime maps streams onto
    // four hardware queues, and the split class's workgroups hold 125 KB of a CU's LDS), and every stream the closing kernel has
    // to join costs a barrier packet of 10-15 us on the critical path (the 48-75 us hole in front of k_h2_final in the round-4
    // timelines).  Measured (profiles/r05_layouts.txt, interleaved rounds, pass ms): S100k five streams 1.020, {0,1,2,2,1} 0.962,
    // {0,1,1,2,2} 0.962, {0,1,2,2,2} 0.984, {0,1,2,3,3} 0.983, {0,1,1,1,1} 1.094; S1M five streams 10.10, {0,1,2,2,1} 10.70 —
    // the fixed costs do not matter there and five abreast packs the chip better.
    // Re-dealt once the triangle launches were gone from the pass (profiles/tristage_layouts.txt, the same method): behind the
    // split class the main stream stood idle from about 400 us on while wave class 0 waited behind class M until 564 us and
    // ended the pass.  S100k pass ms, medians of three interleaved rounds: {0,1,2,2,1} 0.818, {0,1,2,2,0} 0.809, {0,1,2,0,1}
    // 0.799, {0,1,2,0,2} 0.791 (spread of each below 0.003) — wave class 1 behind the split class, classes 2 and 0 share the
    // second side stream, class M has the first to itself.  With the triangle stage (h2_expect_triangles) each block class's
    // triangle launch stays right behind it on its stream, ahead of whatever the table puts there next.
    static const int three_streams[H2_CLASSES] = {0, 1, 2, 0, 2}, five_streams[H2_CLASSES] = {0, 1, 2, 3, 4};
    const int *lay = g->n < 400000 ? three_streams : five_streams;
    hipStream_t pool[5] = {g->stream, g->side[1], g->low[0], g->low[1], g->side[2]};
    hipEvent_t done[5] = {nullptr, g->ev_join[1], g->ev_join[2], g->ev_join[3], g->ev_aux2};
    bool used[5] = {true, false, false, false, false};
    DCR_HIP(hipEventRecord(g->ev_fork, g->stream));
    auto on = [&](int c) {
        const int si = lay[c];
        if (!used[si]) {
            used[si] = true;
            (void)hipStreamWaitEvent(pool[si], g->ev_fork, 0);   // (an error surfaces at hipGetLastError below)
        }
        return pool[si];
    };
    bool eset_on_aux = false;
    if (patch) {
        if (journal) g->h2_eset_tombs += g->h2_eset_pending;  // (applied by k_h2_plan<1> above, ahead of the fork)
    } else {
        DCR_HIP(hipStreamWaitEvent(g->aux, g->ev_fork, 0));
        DCR_HIP(hipMemsetAsync(g->h2_eset.p, 0xFF, sizeof(unsigned long long) << g->h2_eset_bits, g->aux));
        DCR_HIP(hipMemsetAsync(g->h2_bloom.p, 0, sizeof(unsigned) * (((size_t)1 << g->h2_bloom_bits) / 32), g->aux));
        if (sblocks > 0) hipLaunchKernelGGL(k_h2_eset_build, dim3((unsigned)sblocks), dim3(256), 0, g->aux, vw, es, status, g->dres.p);
        g->h2_eset_tombs = 0;
        DCR_HIP(hipEventRecord(g->ev_aux, g->aux));
        eset_on_aux = true;
    }
    g->h2_eset_valid = true;
    g->h2_eset_pending = 0;
    const int64_t hint4 = g->h2_last_count[4] >= 0 ? (int64_t)g->h2_last_count[4] + 8 : g->num_cu;
    const int64_t hint3 = g->h2_last_count[3] >= 0 ? (int64_t)g->h2_last_count[3] + 8 : 3 * (int64_t)g->num_cu;
    // (the block classes probe the edge set themselves: a set that is being rebuilt has to be complete before they start)
    hipStream_t st_split = on(0), st_mid = on(1);
    if (eset_on_aux) {
        DCR_HIP(hipStreamWaitEvent(st_split, g->ev_aux, 0));
        if (st_mid != st_split) DCR_HIP(hipStreamWaitEvent(st_mid, g->ev_aux, 0));
    }
    launch_h2_block<4, true>(g, vw, tk, rt, g->h2_units[4].p, &g->dres.p->h2_count[4], g->h2_units[4].cap, hint4, 0, st_split);
    launch_h2_block<3, false>(g, vw, tkM, rt, g->h2_units[3].p, &g->dres.p->h2_count[3], g->h2_units[3].cap, hint3, 0, st_mid);
    // The triangle stage (both launches here and the one behind the retry launch) goes with the pass only once some pass of this
    // graph has had a block-class unit on the probe path: the units join their triangle term themselves, and on a graph where all
    // of them can the launches found nothing to do, yet each pushed a full-chip grid through a full chip (32 us on average on the
    // bench graph, the one behind class M ahead of the kernel that ends the pass).  k_h2_final checks the expectation (status 4).
    const bool tri_stage = g->h2_expect_triangles;
    if (tri_stage) {
        // each block class's triangle step right behind it on its own stream (class M's behind the split class's: 292 us beside
        // the other classes, 60 alone — it started 90 us after M's end and sat on the critical path)
        hipLaunchKernelGGL(k_h2_triangles, dim3((unsigned)(g->num_cu * 4)), dim3(256), 0, pool[lay[0]], es, tk, g->h2_rec.p, status, 0);
        hipLaunchKernelGGL(k_h2_triangles, dim3((unsigned)(g->num_cu * 8)), dim3(256), 0, pool[lay[1]], es, tkM, g->h2_rec.p, status, 0);
    }
    launch_h2_small<2>(g, vw, rt, on(2));
    launch_h2_small<1>(g, vw, rt, on(3));
    launch_h2_small<0>(g, vw, rt, on(4));
    for (int si = 1; si < 5; ++si)
        if (used[si]) {
            DCR_HIP(hipEventRecord(done[si], pool[si]));
            DCR_HIP(hipStreamWaitEvent(g->stream, done[si], 0));
        }
    if (!g->ext_part.p) DCR_TRY(g->ext_part.alloc(2 * EXT_PART_BLOCKS));
    int64_t fblocks = (sblocks + H2_FINAL_Q - 1) / H2_FINAL_Q;
    if (fblocks > H2_FINAL_BLOCKS) fblocks = H2_FINAL_BLOCKS;
    if (fblocks > EXT_PART_BLOCKS / 4) fblocks = EXT_PART_BLOCKS / 4;  // (a pair of partial extrema per WAVE)
    if (fblocks < 1) fblocks = 1;
    const bool retry_stage = g->h2_expect_retry;
    if (retry_stage) {
        // nodes whose tables filled up in their class: zero their records, redo them with worst-case partitions
        hipLaunchKernelGGL(k_h2_retry_zero, dim3(1024), dim3(256), 0, g->stream, vw, g->h2_retry.p, &g->dres.p->h2_retry, g->h2_retry.cap,
                           g->h2_rec.p);
        tk.retry_flag = 0x80000000u;
        launch_h2_block<4, true>(g, vw, tk, rt, g->h2_retry.p, &g->dres.p->h2_retry, g->h2_retry.cap, 64, 1, g->stream);
        if (tri_stage)
            hipLaunchKernelGGL(k_h2_triangles, dim3((unsigned)(g->num_cu * 2)), dim3(256), 0, g->stream, es, tk, g->h2_rec.p, status, 1);
    }
    hipLaunchKernelGGL(k_h2_final, dim3((unsigned)fblocks), dim3(256), 0, g->stream, vw, g->h2_rec.p, g->curv.p, status, g->ext_part.p,
                       g->ext_part.p + EXT_PART_BLOCKS, &g->dres.p->h2_retry, retry_stage ? 1 : 0, &g->dres.p->h2_fallback,
                       tri_stage ? 1 : 0);
    g->h2_launches += 1;
    g->h2_last_retry_stage = retry_stage;
    g->h2_last_tri_stage = tri_stage;
    g->ext_part_n = (int)fblocks * 4;
    g->ext_part_valid = true;  // (dropped again by the caller if the pass reports a failure, and by every edit)
    DCR_HIP(hipGetLastError());
    g->h2_head_clean = pblocks > 0;  // (everything that leaves the other bucket half zero is enqueued)
    return DCR_OK;
}

// diagnostic: W recomputed from the rows into an array of its own and compared with the kept one (bit 31 aside)
__global__ void __launch_bounds__(256) k_h2_weight_diff(const int32_t *kept, const int32_t *fresh, int64_t n, int32_t *out) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        bad += (kept[i] & 0x7FFFFFFF) != fresh[i];
    if (bad) atomicAdd(out, bad);
}

int h2_weight_check(dcr_graph *g, int64_t *mismatches) {
    *mismatches = -1;
    if (!g->h2_weight_valid || !g->h2_weight.p) return DCR_OK;
    DCR_TRY(g->h2_weight_chk.grow(g->n + 64));
    int32_t *fresh = g->h2_weight_chk.p, *count = g->h2_weight_chk.p + g->n;  // (the array has 64 words of slack)
    DCR_HIP(hipMemsetAsync(fresh, 0, sizeof(int32_t) * (size_t)(g->n + 1), g->stream));
    View vw{g->rowinfo.p, g->col.p, g->slot_row.p, g->cap_total, g->dres.p->misc, nullptr, (int32_t)g->n, 0};
    const int64_t sblocks = (g->cap_total + 255) / 256, cb = (g->n + 255) / 256;
    if (sblocks > 0) hipLaunchKernelGGL(k_h2_weight, dim3((unsigned)sblocks), dim3(256), 0, g->stream, vw, fresh);
    hipLaunchKernelGGL(k_h2_weight_diff, dim3((unsigned)(cb < 1 ? 1 : cb > 2048 ? 2048 : cb)), dim3(256), 0, g->stream, g->h2_weight.p, fresh,
                       g->n, count);
    DCR_HIP(hipGetLastError());
    int32_t bad = 0;
    DCR_HIP(hipMemcpyAsync(&bad, count, sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
    DCR_HIP(hipStreamSynchronize(g->stream));
    *mismatches = bad;
    return DCR_OK;
}

}  // namespace dcr

// diagnostic, for tools/h2_rowmask_coverage.py alone (not part of include/dcr.h): the class-M units of the current device that
// the row-mask path published (out[0]) and handed over to the block path (out[1]) since the last call; the counters start again.
// Call it with the device idle.
extern "C" int dcr_h2_rowmask_units(uint32_t out[2]) {
    const unsigned zero[2] = {0u, 0u};
    if (!out || hipMemcpyFromSymbol(out, HIP_SYMBOL(dcr::h2_rows_units), sizeof zero) != hipSuccess) return DCR_EHIP;
    return hipMemcpyToSymbol(HIP_SYMBOL(dcr::h2_rows_units), zero, sizeof zero) == hipSuccess ? DCR_OK : DCR_EHIP;
}
