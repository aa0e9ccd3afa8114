// SDRF-side kernels of libdcr_hip.so: arg-min/arg-max over edges, the candidate/improvement tensor and the
// add/remove tail of one iteration (rewiring/sdrf_no_cuda.py:27-66).
//
// Improvements.  The reference evaluates bfc_edge(x,y) twice per candidate (sdrf_no_cuda.py:41-46).  Here the
// integer ingredients of bfc_edge(x,y) on G + (i,j) are derived exactly from per-neighbour counters of the base
// graph, and the float64 closing expression (bfc_naive.py:31-40) is evaluated on those integers, so
// after - before is bit-identical to the reference while the work per candidate is O(1):
//   c1[a] = |N(i_a) ∩ DY| for i_a in DX = N(x) \ N(y) \ {y};  c2[b] = |N(j_b) ∩ DX| for j_b in DY.
//   * i in N(x), j in N(y) (neither is x or y): only (i in DX, j in DY) changes anything: c1[a]+1, c2[b]+1.
//   * i == x, j in DY: deg(x)+1, T+1, j leaves DY: c1[k] drops by [k ~ j]; needs one scan of row j.
//   * j == y, i in DX: mirrored.
//   * every other admissible pair leaves all ingredients unchanged: improvement = +0.0.
#include <cstdlib>
#include "dcr_internal.h"
#include <cstdio>

namespace dcr {

struct RowView {
    const int2 *rowinfo;
    const int32_t *col;
    const int32_t *slot_row;
};

__device__ __host__ inline double bfc_formula(int d1, int d2, int T, int s1, int s2, int gamma) {
    int dmax = d1 > d2 ? d1 : d2, dmin = d1 < d2 ? d1 : d2;
    double r = 2.0 / (double)d1;
    r = r + 2.0 / (double)d2;
    r = r - 2.0;
    r = r + (double)(2 * (int64_t)T) / (double)dmax;
    r = r + (double)T / (double)dmin;
    if (s1 == 0 || s2 == 0) return r;
    double q = 1.0 / (double)gamma;
    q = q / (double)dmax;
    q = q * (double)(s1 + s2);
    return r + q;
}

__device__ inline double bfc_value(int d1, int d2, int T, int s1, int s2, int gamma) {
    if ((d1 < d2 ? d1 : d2) == 1) return 0.0;  // bfc_naive.py:18-19
    return bfc_formula(d1, d2, T, s1, s2, gamma);
}

// ---------------------------------------------------------------------------------------------
// arg-extremum over undirected edges, first in G.edges order (= smallest slot) on ties
// ---------------------------------------------------------------------------------------------
// (Ext, ext_better and the reductions live in dcr_internal.h: the two-hop pass's closing kernel leaves per-block extrema too)

// Calls body(slot, u, v, value, acc...) for every live slot of this thread that holds an undirected edge (u < v), in increasing
// slot order: ext_take's "first slot wins" rests on that order.  Four slots per thread and round, their chains of dependent loads
// (owner row -> row extent; neighbour; value) in flight together: everything addressed by the slot itself in one round (all in
// bounds for every slot, slack included), the row extent in a second one.  body is a lambda that captures BY VALUE; what it
// accumulates comes in as reference parameters (as walk_rows of dcr_analysis.h): the running extrema stay in plain registers.
template <class Body, typename... Acc>
__device__ __forceinline__ void walk_edge_slots(const RowView &g, int64_t cap_total, const double *curv, Body body, Acc &...acc) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s0 < cap_total; s0 += 4 * stride) {
        int u[4], v[4];
        int2 ru[4];
        bool ok[4];
        double cv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t s = s0 + q * stride;
            ok[q] = s < cap_total;
            u[q] = ok[q] ? g.slot_row[s] : 0;
            v[q] = ok[q] ? g.col[s] : -1;
            cv[q] = ok[q] ? curv[s] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) ru[q] = ok[q] ? g.rowinfo[u[q]] : make_int2(0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t s = s0 + q * stride;
            if (!ok[q] || (int)(s - ru[q].x) >= ru[q].y || v[q] <= u[q]) continue;
            body((int)s, u[q], v[q], cv[q], acc...);
        }
    }
}

__global__ void __launch_bounds__(256) k_argext_edges(RowView g, int64_t cap_total, const double *curv, int want_max,
                                                       int excl_u, int excl_v, const DevResult *res, Ext *partial) {
    __shared__ double shv[4];
    __shared__ int shs[4];
    if (excl_u == -2) {  // the edge picked on the device (dcr_sdrf_tail_at)
        excl_u = res->cand_i;
        excl_v = res->cand_j;
    }
    double best_v = 0.0;
    int best_s = -1;
    walk_edge_slots(
        g, cap_total, curv,
        [=](int s, int u, int v, double cv, double &bv, int &bs) {
            if (u == excl_u && v == excl_v) return;
            ext_take(bv, bs, cv, s, want_max);
        },
        best_v, best_s);
    ext_block_reduce(best_v, best_s, want_max, shv, shs);
    if (threadIdx.x == 0) partial[blockIdx.x] = ext_make(best_v, best_s);
}

// both extrema in ONE sweep, left as per-workgroup partials where the two-hop pass's closing kernel leaves its per-wave ones
// (g->ext_part): after a node-centric or incremental pass the arg-min of the loop (sdrf_no_cuda.py:27) and the stale arg-max of
// its removal step (:57-61) were two sweeps of 13 us each
// (clear_words: the incremental pass's node flags, which nothing reads between the pass and this sweep: their fill launch rode
//  in front of it before)
__global__ void __launch_bounds__(256) k_argext_edges_both(RowView g, int64_t cap_total, const double *curv, Ext *part_min, Ext *part_max,
                                                            unsigned *clear_words, int64_t n_clear_words, DevResult *res) {
    __shared__ double shv[4];
    __shared__ int shs[4];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_clear_words; i += (int64_t)gridDim.x * blockDim.x) clear_words[i] = 0u;
    if (n_clear_words > 0 && blockIdx.x == 0 && threadIdx.x == 0) res->touched_n = 0;   // (the list of flagged nodes goes with the flags)
    double lo_v = 0.0, hi_v = 0.0;
    int lo_s = -1, hi_s = -1;
    walk_edge_slots(
        g, cap_total, curv,
        [](int s, int, int, double cv, double &lv, int &ls, double &hv, int &hs) {
            ext_take(lv, ls, cv, s, 0);
            ext_take(hv, hs, cv, s, 1);
        },
        lo_v, lo_s, hi_v, hi_s);
    ext_block_reduce(lo_v, lo_s, 0, shv, shs);
    if (threadIdx.x == 0) part_min[blockIdx.x] = ext_make(lo_v, lo_s);
    __syncthreads();
    ext_block_reduce(hi_v, hi_s, 1, shv, shs);
    if (threadIdx.x == 0) part_max[blockIdx.x] = ext_make(hi_v, hi_s);
}

// partial[0 .. nparts) reduced to (best_v, best_s) in every thread of ONE workgroup of any size up to 1,024 (16 waves)
__device__ inline void reduce_partials(const Ext *partial, int nparts, int want_max, double &best_v, int &best_s) {
    __shared__ double shv[16];
    __shared__ int shs[16];
    best_v = 0.0;
    best_s = -1;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
        const Ext e = partial[i];
        ext_take(best_v, best_s, e.val, e.slot, want_max);
    }
    ext_block_reduce(best_v, best_s, want_max, shv, shs);
}

// the one-workgroup reduction of the partial extrema into the result block
__device__ inline void argext_final_body(const RowView &g, const Ext *partial, int nparts, int want_max, DevResult *res) {
    double best_v;
    int best_s;
    reduce_partials(partial, nparts, want_max, best_v, best_s);
    if (threadIdx.x == 0) {
        res->ext_val = best_v;
        res->ext_slot = best_s;
        const int eu = best_s >= 0 ? g.slot_row[best_s] : -1, ev = best_s >= 0 ? g.col[best_s] : -1;
        res->ext_u = eu;
        res->ext_v = ev;
        res->ext_du = best_s >= 0 ? g.rowinfo[eu].y : 0;
        res->ext_dv = best_s >= 0 ? g.rowinfo[ev].y : 0;
    }
}

__global__ void __launch_bounds__(1024) k_argext_final(RowView g, const Ext *partial, int nparts, int want_max,
                                                        DevResult *res) {
    argext_final_body(g, partial, nparts, want_max, res);
}

// first maximum of a plain array (np.argmax of the improvements, utils/softmax.py:7): of a[0 .. n), or of a[0 .. res->n_cand)
// when res is given (the device-side draw: nothing there needs a host value)
__global__ void __launch_bounds__(256) k_argmax_array(const double *a, int64_t n, const DevResult *res, Ext *partial) {
    __shared__ double shv[4];
    __shared__ int shs[4];
    if (res) n = res->n_cand;
    double best_v = 0.0;
    int best_s = -1;
    // indices may exceed int32 only beyond 2^31 candidates, which the row capacity already excludes
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        ext_take(best_v, best_s, a[i], (int)i, 1);
    }
    ext_block_reduce(best_v, best_s, 1, shv, shs);
    if (threadIdx.x == 0) partial[blockIdx.x] = ext_make(best_v, best_s);
}

__global__ void __launch_bounds__(256) k_argmax_final(const Ext *partial, int nparts, DevResult *res) {
    double best_v;
    int best_s;
    reduce_partials(partial, nparts, 1, best_v, best_s);
    if (threadIdx.x == 0) res->imp_argmax = best_s;
}

// the candidate at index idx of the emitted list, as the sorted pair the tail kernels add
__device__ inline void store_candidate(DevResult *res, const int32_t *ci, const int32_t *cj, int64_t idx) {
    const int32_t a = ci[idx], b = cj[idx];
    res->cand_i = a < b ? a : b;
    res->cand_j = a < b ? b : a;
}

// ---------------------------------------------------------------------------------------------
// improvement pipeline
// ---------------------------------------------------------------------------------------------
constexpr unsigned T_EMPTY = 0xFFFFFFFFu;

__device__ inline unsigned g_hash(unsigned key, unsigned mask) { return (key * 0x9E3779B1u >> 7) & mask; }

// slot index of key in the global table, or -1
__device__ inline int g_find(const int32_t *keys, unsigned mask, int key) {
    unsigned h = g_hash((unsigned)key, mask);
    while (true) {
        const int e = keys[h];
        if (e == key) return (int)h;
        if ((unsigned)e == T_EMPTY) return -1;
        h = (h + 1) & mask;
    }
}

// four look-ups with their first probes in flight together (the rows swept by the improvement kernels are walked by one
// wave each: the longest row sets the kernel's duration, and its steps are chains of dependent loads)
__device__ inline void g_find4(const int32_t *keys, unsigned mask, const int (&key)[4], const bool (&valid)[4], int (&out)[4]) {
    unsigned h[4];
    int e[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        h[q] = g_hash((unsigned)key[q], mask);
        e[q] = valid[q] ? keys[h[q]] : (int)T_EMPTY;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        out[q] = -1;
        if (!valid[q]) continue;
        while (true) {
            if (e[q] == key[q]) { out[q] = (int)h[q]; break; }
            if ((unsigned)e[q] == T_EMPTY) break;
            h[q] = (h[q] + 1) & mask;
            e[q] = keys[h[q]];
        }
    }
}

struct ImpBuf {
    int32_t *keys, *posx, *posy;  // hash table over N(x) ∪ N(y) minus {x,y}
    int32_t *c1, *c2;             // [dx], [dy]
    int32_t *clsx, *clsy;         // 0: only in own row (DX / DY), 1: in both rows (triangle), 2: the other endpoint
    int4 *descx, *descy;          // [dx+1], [dy]: {member, start of its row, its degree, its table slot (-1: an endpoint)} of row x
                                  // (entry dx: x itself) and of row y, left by k_imp_insert
    int32_t *rowcount, *rowoff;   // [dx+1]
    uint32_t *adjbits;            // [dx+1][words]
    ImpStats *st;
};

// K1 (round 4: one launch for both rows; the pipeline was eleven launch-bound kernels, 45 us of launch gaps in 115): row x and
// row y go into the table concurrently — a key met in both rows (a triangle node) is inserted by whichever thread comes first
// and found by the other; which of the two it was does not matter, posx / posy are separate arrays.  The classes (0: in its
// own row only, 1: in both, 2: the other endpoint) are resolved by the next kernel, when the table is complete.
// Round 5: the removal step's stale arg-max (the reduction of the partial maxima the pass's closing kernel left; it depends on
// nothing in the pipeline and writes other fields of the result block) rides on this launch as ONE MORE workgroup instead of
// being a launch of its own between the pipeline and the draw (5.4 us of the iteration: profiles/r05_step_timeline.txt).
__global__ void __launch_bounds__(256) k_imp_insert(RowView g, ImpBuf B, int x, int y, unsigned mask, const Ext *amax_parts, int amax_n,
                                                     DevResult *res) {
    const int nblocks = (int)gridDim.x - (amax_parts ? 1 : 0);
    if ((int)blockIdx.x == nblocks) {  // (uniform: the extra workgroup)
        argext_final_body(g, amax_parts, amax_n, 1, res);
        return;
    }
    const int2 rx = g.rowinfo[x], ry = g.rowinfo[y];
    const int total = rx.y + ry.y;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += nblocks * blockDim.x) {
        const bool isx = t < rx.y;
        const int p = isx ? t : t - rx.y;
        const int k = g.col[(isx ? rx.x : ry.x) + p];
        const int2 rk = g.rowinfo[k];  // (in flight beside the probes: the descriptor the later kernels start from)
        if (isx) {
            B.c1[p] = 0;
            B.clsx[p] = k == y ? 2 : 0;
        } else {
            B.c2[p] = 0;
            B.clsy[p] = k == x ? 2 : 0;
            if (k == x) B.st->pos_x_in_y = p;
        }
        int slot = -1;
        if (k != (isx ? y : x)) {  // the endpoints themselves are never in the table
            unsigned h = g_hash((unsigned)k, mask);
            while (true) {
                const unsigned old = atomicCAS((unsigned *)&B.keys[h], T_EMPTY, (unsigned)k);
                if (old == T_EMPTY || old == (unsigned)k) break;
                h = (h + 1) & mask;
            }
            if (isx) B.posx[h] = p;
            else B.posy[h] = p;
            slot = (int)h;  // (a triangle node: both rows' threads end their walk at the one slot that holds it)
        }
        (isx ? B.descx : B.descy)[p] = make_int4(k, rk.x, rk.y, slot);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        B.st->x = x;
        B.st->y = y;
        B.st->dx = rx.y;
        B.st->dy = ry.y;
        B.st->table_mask = (int)mask;
        B.st->T = 0;
        B.st->deg_min_is_one = (rx.y < ry.y ? rx.y : ry.y) == 1;
        B.st->done_rows = 0;
        B.st->done_draw = 0;
        B.descx[rx.y] = make_int4(x, rx.x, rx.y, -1);  // the candidate row of x itself
        // (pos_x_in_y: written above by the thread that meets x in row y; reset to -1 by the pipeline's last kernel)
    }
}

// empty table (only after a fresh allocation or a pipeline that did not run to its end: k_imp_emit leaves the table empty)
__global__ void __launch_bounds__(256) k_imp_clear(ImpBuf B, int64_t ts) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < ts; i += nth) {
        B.keys[i] = -1;
        B.posx[i] = -1;
        B.posy[i] = -1;
    }
    if (tid == 0) B.st->pos_x_in_y = -1;
}

struct Mx {
    int m, c, s;  // maximum, how many attain it, largest value below it
};

__device__ inline Mx mx_join(Mx a, Mx b) {
    Mx r;
    if (a.m == b.m) {
        r.m = a.m;
        r.c = a.c + b.c;
        r.s = a.s > b.s ? a.s : b.s;
    } else if (a.m > b.m) {
        r.m = a.m;
        r.c = a.c;
        r.s = a.s > b.m ? a.s : b.m;
    } else {
        r.m = b.m;
        r.c = b.c;
        r.s = b.s > a.m ? b.s : a.m;
    }
    return r;
}

__device__ inline Mx mx_add(Mx a, int v) {
    Mx b;
    b.m = v;
    b.c = 1;
    b.s = -1;
    return mx_join(a, b);
}

__device__ inline void block_stats(const int32_t *c, int n, int *cnt_pos, Mx *mx, int *shi) {
    int pos = 0;
    Mx m;
    m.m = -1;
    m.c = 0;
    m.s = -1;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int v = c[i];
        pos += v > 0;
        m = mx_add(m, v);
    }
    for (int off = 32; off > 0; off >>= 1) {
        pos += __shfl_xor(pos, off);
        Mx o;
        o.m = __shfl_xor(m.m, off);
        o.c = __shfl_xor(m.c, off);
        o.s = __shfl_xor(m.s, off);
        m = mx_join(m, o);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) {
        shi[wid * 4 + 0] = pos;
        shi[wid * 4 + 1] = m.m;
        shi[wid * 4 + 2] = m.c;
        shi[wid * 4 + 3] = m.s;
    }
    __syncthreads();
    pos = 0;
    m.m = -1;
    m.c = 0;
    m.s = -1;
    for (int w = 0; w < nw; ++w) {
        pos += shi[w * 4];
        Mx o;
        o.m = shi[w * 4 + 1];
        o.c = shi[w * 4 + 2];
        o.s = shi[w * 4 + 3];
        m = mx_join(m, o);
    }
    *cnt_pos = pos;
    *mx = m;
}

// |sq1|, |sq2|, maxima (with multiplicity and runner-up), triangles and the base curvature; called by one whole workgroup
__device__ inline void imp_close_stats(ImpBuf B, int curv_type, int *shi) {
    ImpStats *st = B.st;
    const int dx = st->dx, dy = st->dy;
    int s1, s2;
    Mx m1, m2;
    block_stats(B.c1, dx, &s1, &m1, shi);
    block_stats(B.c2, dy, &s2, &m2, shi);
    // triangles: the members of row x that are in row y too (class 1)
    int T = 0;
    for (int a = threadIdx.x; a < dx; a += blockDim.x) T += B.clsx[a] == 1;
    for (int off = 32; off > 0; off >>= 1) T += __shfl_xor(T, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) shi[threadIdx.x >> 6] = T;
    __syncthreads();
    if (threadIdx.x == 0) {
        T = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) T += shi[w];
        st->T = T;
        st->s1 = s1;
        st->s2 = s2;
        st->max1 = m1.m < 0 ? 0 : m1.m;
        st->cnt1 = m1.c;
        st->sec1 = m1.s < 0 ? 0 : m1.s;
        st->max2 = m2.m < 0 ? 0 : m2.m;
        st->cnt2 = m2.c;
        st->sec2 = m2.s < 0 ? 0 : m2.s;
        const int gam = st->max1 > st->max2 ? st->max1 : st->max2;
        double before;
        switch (curv_type) {
            case DCR_CURV_1D: before = (double)(4 - dx - dy); break;
            case DCR_CURV_AUGMENTED: before = (double)(4 - dx - dy + 3 * T); break;
            case DCR_CURV_HAANTJES: before = (double)T; break;
            default: before = bfc_value(dx, dy, T, s1, s2, gam);
        }
        st->before = before;
    }
    __syncthreads();
}

// K2 (round 4: one launch for what were k_imp_count, k_imp_stats, k_imp_rows and k_imp_scan).  One workgroup per candidate row
// a (i = x_nb[a]; a == dx: i = x) streams row i ONCE: every entry is looked up in the table; an entry that is in row y only is
// a 4-cycle x - i - w - y (c1[a] grows, and c2 of the node it lands on: bfc_naive.py:26-29,36-37), an entry that is in
// row y at all rules the pair (i, that neighbour) out (sdrf_no_cuda.py:35: has_edge) — a bit in the row's bitmap, as do i == j,
// w == y and w == x.  The workgroup also settles the classes of its row and of a share of row y.  The LAST workgroup to
// finish closes the stage: statistics of c1 / c2, triangles, base curvature, exclusive scan of the rows' candidate counts.
// The grid is dx + 1 workgroups and dy comes as an argument (the host sized the launch by both).  A workgroup starts from the
// descriptor k_imp_insert left for its row — member, row extent, table slot — so the row's entries are the second link of its
// chain of dependent reads, not the sixth (statistics block, rowinfo of x, col, probe walk, rowinfo of i came before them), and
// its class is one read at a known slot, in flight beside them.
__global__ void __launch_bounds__(256) k_imp_rows_count(RowView g, ImpBuf B, int x, int y, int dy, unsigned mask, int words,
                                                         int curv_type, DevResult *res) {
    extern __shared__ uint32_t bits[];
    __shared__ int cnt_sh, c1_sh;
    __shared__ int shi[16 * 4];
    ImpStats *stp = B.st;
    const int dx = (int)gridDim.x - 1;
    const int a = blockIdx.x;
    const int4 d = B.descx[a];
    const int pos_x_in_y = stp->pos_x_in_y;  // x is an endpoint, so it is not in the table
    for (int w = threadIdx.x; w < words; w += blockDim.x) bits[w] = 0u;
    // class of row a: 2 = the other endpoint, 1 = also in row y (a triangle node), 0 = in row x only.  Every thread reads the
    // slot itself (one address: a broadcast) — behind one thread and a barrier the whole workgroup waited for it.
    int cls = 3, b_i = -1;  // b_i: position of i in row y + [y] (the pair (i, i) is ruled out: sdrf_no_cuda.py:35, i != j)
    if (a == dx) {
        b_i = pos_x_in_y;
    } else if (d.w < 0) {  // i == y
        cls = 2;
        b_i = dy;
    } else {
        b_i = B.posy[d.w];  // (complete: every posy was written by the launch before)
        cls = b_i >= 0 ? 1 : 0;
    }
    if (threadIdx.x == 0) {
        cnt_sh = 0;
        c1_sh = 0;
        // (what the closing workgroup reads of this one — clsx, rowcount, c1 — is stored through the L2 with agent-scope relaxed
        //  atomics, as last_arriver asks; c2 is updated by device-scope atomics)
        if (a < dx) __hip_atomic_store(&B.clsx[a], cls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const bool counting = curv_type == DCR_CURV_BFC && cls == 0;
    const int2 ri = make_int2(d.y, d.z);
    int c = 0;
    for (int base = 0; base < ri.y; base += 4 * 256) {  // four look-ups in flight per thread (a hub's row is 1,400 entries)
        int w[4], h[4];
        bool in[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int t = base + 256 * q + (int)threadIdx.x;
            in[q] = t < ri.y;
            w[q] = in[q] ? g.col[ri.x + t] : -1;
            in[q] = in[q] && w[q] != x && w[q] != y;  // (the endpoints are not in the table)
        }
        g_find4(B.keys, mask, w, in, h);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int b = -1;
            if (w[q] == y && base + 256 * q + (int)threadIdx.x < ri.y) b = dy;
            else if (w[q] == x && base + 256 * q + (int)threadIdx.x < ri.y) b = pos_x_in_y;
            else if (in[q] && h[q] >= 0) {
                b = B.posy[h[q]];
                if (counting && b >= 0 && B.posx[h[q]] < 0) {  // in N(y) only
                    ++c;
                    atomicAdd(&B.c2[b], 1);
                }
            }
            if (b >= 0) atomicOr(&bits[b >> 5], 1u << (b & 31));
        }
    }
    if (threadIdx.x == 0 && b_i >= 0) atomicOr(&bits[b_i >> 5], 1u << (b_i & 31));  // i == j
    // classes of a share of row y (every position is settled by exactly one workgroup; nothing in this kernel reads them)
    // (the slot of its member is in the row's descriptor: one posx read per position, no probe walk; -1: x itself, class 2)
    for (int b = a + (int)threadIdx.x * (int)gridDim.x; b < dy; b += (int)blockDim.x * (int)gridDim.x) {
        const int h = B.descy[b].w;
        if (h >= 0) B.clsy[b] = B.posx[h] >= 0 ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&c1_sh, c);
    __syncthreads();
    int adm = 0;
    const int nb = dy + 1;
    for (int w = threadIdx.x; w < words; w += blockDim.x) {
        uint32_t v = bits[w];
        const int lo = w * 32;
        const uint32_t live = (nb - lo >= 32) ? 0xFFFFFFFFu : ((1u << (nb - lo)) - 1u);
        adm += __popc(~v & live);
        B.adjbits[(size_t)a * words + w] = v;
    }
    for (int off = 32; off > 0; off >>= 1) adm += __shfl_xor(adm, off);
    if ((threadIdx.x & 63) == 0 && adm) atomicAdd(&cnt_sh, adm);
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(&B.rowcount[a], cnt_sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a < dx) __hip_atomic_store(&B.c1[a], counting ? c1_sh : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!last_arriver(&stp->done_rows, (int)gridDim.x)) return;
    // imp_close_stats reads c1, c2 and clsx with plain loads, hence the agent-scope acquire (buffer_inv: drops this CU's stale
    // lines, no write-back of the L2 as __threadfence() has it)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    imp_close_stats(B, curv_type, shi);
    // exclusive scan of rowcount[0 .. rows): the candidates are emitted row by row (sdrf_no_cuda.py:32-37: outer loop over x_nb)
    const int rows = (int)gridDim.x;
    // 1,024 rows per step: a thread takes four consecutive rows (their loads in flight together), a wave scans its threads'
    // totals, the waves' totals cross through LDS; the carry is a register every thread keeps, and the waves' totals alternate
    // between two LDS sets, so a step has ONE barrier (256 rows a step, the carry through LDS: three).
    __shared__ int wsum[2][4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0, par = 0; base < rows; base += 4 * 256, par ^= 1) {
        const int r0 = base + 4 * (int)threadIdx.x;
        int v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            v[q] = r0 + q < rows ? __hip_atomic_load(&B.rowcount[r0 + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        const int mine = v[0] + v[1] + v[2] + v[3];
        int incl = mine;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wsum[par][wid] = incl;
        __syncthreads();
        int woff = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int s = wsum[par][w];
            woff += w < wid ? s : 0;
            all += s;
        }
        int o = carry + woff + incl - mine;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (r0 + q < rows) B.rowoff[r0 + q] = o;
            o += v[q];
        }
        carry += all;
    }
    if (threadIdx.x == 0) res->n_cand = carry;
}

// the closing expressions of class B (i == x, j = y_nb[b] in DY joins row x) and class C (j == y, i = x_nb[a] in DX joins
// row y): the side that gains the edge loses one member (own: its counter c_own), every counter of the other side adjacent to
// it drops by one (n_dec0 of them stood at 1, n_maxadj of them at the maximum)
__device__ inline double bfc_after_b(const ImpStats &st, int cb, int n_dec0, int n_maxadj) {
    const int s1 = st.s1 - n_dec0;
    const int m1 = (st.max1 > 0 && n_maxadj == st.cnt1) ? st.max1 - 1 : st.max1;
    const int s2 = st.s2 - (cb > 0);
    const int m2 = (cb == st.max2 && st.cnt2 == 1) ? st.sec2 : st.max2;
    return bfc_value(st.dx + 1, st.dy, st.T + 1, s1, s2, m1 > m2 ? m1 : m2);
}

__device__ inline double bfc_after_c(const ImpStats &st, int ca, int n_dec0, int n_maxadj) {
    const int s2 = st.s2 - n_dec0;
    const int m2 = (st.max2 > 0 && n_maxadj == st.cnt2) ? st.max2 - 1 : st.max2;
    const int s1 = st.s1 - (ca > 0);
    const int m1 = (ca == st.max1 && st.cnt1 == 1) ? st.sec1 : st.max1;
    return bfc_value(st.dx, st.dy + 1, st.T + 1, s1, s2, m1 > m2 ? m1 : m2);
}

// 4 - d1 - d2 (+3T): one degree grows, one triangle appears (classical_curvatures.py:14-28)
__device__ inline double classical_bc(int curv_type) {
    return curv_type == DCR_CURV_1D ? -1.0 : curv_type == DCR_CURV_AUGMENTED ? 2.0 : 1.0;
}

// K7: write the admitted candidates, row by row in j order, with their improvements.  Workgroups [0, dx): row a (i = x_nb[a]).
// Workgroups [dx, dx + words): the row of x itself (i == x, class B), 32 positions b each.
// Classes B and C were a launch of their own that streamed the row of every j in DY and every i in DX through the table again
// (9.7 us and a launch boundary).  The admissibility bitmap already holds what they looked up: for i_a in DX and j_b in DY, bit
// (a, b) is set exactly when i_a ~ j_b.  Class C of row a is therefore a count over the bits of its own bitmap row, which the
// row's threads read anyway; class B of 32 positions is a count over one word column of the bitmap.  Same integers into the
// same closing expression, no row is streamed, and the table is not read here:
// (Round 4: the pipeline's last kernel leaves the hash table EMPTY for the next iteration; the separate clearing kernel at the
//  head of the pipeline is gone.)
__global__ void __launch_bounds__(256) k_imp_emit(ImpBuf B, int x, int y, int dx, int dy, int words, int curv_type,
                                                   double *out, int32_t *ci, int32_t *cj, int64_t ts) {
    __shared__ int wsum[2][4];
    __shared__ int dec_sh[32], mxa_sh[32];
    const ImpStats st = *B.st;
    const int a = blockIdx.x;
    for (int64_t i = (int64_t)a * 256 + threadIdx.x; i < ts; i += (int64_t)gridDim.x * 256) {
        B.keys[i] = -1;
        B.posx[i] = -1;
        B.posy[i] = -1;
    }
    if (a == 0 && threadIdx.x == 0) B.st->pos_x_in_y = -1;
    const int nb = dy + 1;
    const bool bfc = curv_type == DCR_CURV_BFC;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (a >= dx) {  // (uniform) class B: positions [32 wc, 32 wc + 32) of the row of x itself
        const int wc = a - dx, lo = wc * 32;
        const uint32_t *rowx = B.adjbits + (size_t)dx * words;
        const uint32_t live = (nb - lo >= 32) ? 0xFFFFFFFFu : ((1u << (nb - lo)) - 1u);
        const uint32_t adm = ~rowx[wc] & live;  // admitted: j in DY (triangle nodes, x and y have their bits set)
        if (adm == 0u) return;
        if (threadIdx.x < 32) dec_sh[threadIdx.x] = mxa_sh[threadIdx.x] = 0;
        // place in the output: the admitted positions of this row in the words before (all of their bits are live)
        int before = 0;
        for (int w = threadIdx.x; w < wc; w += 256) before += __popc(~rowx[w]);
        for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
        if (lane == 0) wsum[0][wid] = before;
        __syncthreads();
        before = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
        if (bfc) {
            // the members of DX adjacent to j_b lose a 4-cycle: only those whose counter stands at 1 or at the maximum matter
            for (int r = threadIdx.x; r < dx; r += 256) {
                const int c = B.c1[r];
                if (B.clsx[r] != 0 || (c != 1 && c != st.max1)) continue;
                uint32_t m = B.adjbits[(size_t)r * words + wc] & adm;
                while (m) {
                    const int bit = __ffs(m) - 1;
                    m &= m - 1u;
                    if (c == 1) atomicAdd(&dec_sh[bit], 1);
                    if (c == st.max1) atomicAdd(&mxa_sh[bit], 1);
                }
            }
            __syncthreads();
        }
        if (threadIdx.x < 32 && ((adm >> threadIdx.x) & 1u)) {
            const int b = lo + (int)threadIdx.x;
            const int64_t o = (int64_t)B.rowoff[dx] + before + __popc(adm & ((1u << threadIdx.x) - 1u));
            const int j = b < dy ? B.descy[b].x : y;
            out[o] = bfc ? bfc_after_b(st, B.c2[b], dec_sh[threadIdx.x], mxa_sh[threadIdx.x]) - st.before : classical_bc(curv_type);
            ci[o] = x < j ? x : j;  // sorted((i, j)), sdrf_no_cuda.py:37
            cj[o] = x < j ? j : x;
        }
        return;
    }
    if (B.rowcount[a] == 0) return;
    const int i = B.descx[a].x;
    const int cls_a = B.clsx[a];
    const int c1a = cls_a == 0 ? B.c1[a] : 0;
    const int gam = st.max1 > st.max2 ? st.max1 : st.max2;
    const int64_t row_base = B.rowoff[a];
    const bool general = bfc && cls_a == 0;  // (a row of DX: its pairs with DY and with y change the ingredients)
    // one thread per candidate position b (256 per round): its place in the output is the number of admitted positions
    // before it (ballots inside the wave, wave totals through LDS, alternating between two sets: one barrier a round).  (One
    // thread per 32-bit bitmap word, as this kernel first did it, leaves 5 of 256 threads busy for a typical 150-neighbour
    // endpoint, 32 closing expressions each.)
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int carry = 0, n_dec0 = 0, n_maxadj = 0;  // class C: the members of DY adjacent to i, counted as the rounds pass them
    int64_t o_y = -1;                          // where the pair (i, y) goes (the thread of b == dy, in the last round)
    for (int bbase = 0, par = 0; bbase < nb; bbase += 256, par ^= 1) {
        const int b = bbase + threadIdx.x;
        bool ok = false;
        if (b < nb) ok = ((B.adjbits[(size_t)a * words + (b >> 5)] >> (b & 31)) & 1u) == 0u;
        int clsyb = 3, c2b = 0;
        if (general && b < dy) {
            clsyb = B.clsy[b];
            c2b = B.c2[b];
        }
        const bool adj = general && b < dy && !ok && clsyb == 0;  // j_b in DY, i ~ j_b
        n_dec0 += __popcll(__ballot(adj && c2b == 1));
        n_maxadj += __popcll(__ballot(adj && c2b == st.max2));
        const unsigned long long m = __ballot(ok);
        if (lane == 0) wsum[par][wid] = __popcll(m);
        __syncthreads();
        int woff = 0, all = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int s = wsum[par][q];
            woff += q < wid ? s : 0;
            all += s;
        }
        if (ok) {
            const int64_t o = row_base + carry + woff + __popcll(m & lt);
            const int j = b < dy ? B.descy[b].x : y;
            if (b == dy) {
                o_y = o;  // j == y: admitted only for i in DX; its value needs the whole row's counts (below)
            } else if (general && clsyb == 0) {
                const int mm = (c1a + 1 > c2b + 1 ? c1a + 1 : c2b + 1);
                const double after = bfc_value(st.dx, st.dy, st.T, st.s1 + (c1a == 0), st.s2 + (c2b == 0),
                                               mm > gam ? mm : gam);
                out[o] = after - st.before;
            } else {
                out[o] = 0.0;
            }
            ci[o] = i < j ? i : j;  // sorted((i, j)), sdrf_no_cuda.py:37
            cj[o] = i < j ? j : i;
        }
        carry += all;
    }
    // class C: the per-wave counts (uniform over a wave) summed over the workgroup, for the one thread that holds (i, y)
    __syncthreads();
    if (threadIdx.x == 0) dec_sh[0] = mxa_sh[0] = 0;
    __syncthreads();
    if (lane == 0 && general) {
        if (n_dec0) atomicAdd(&dec_sh[0], n_dec0);
        if (n_maxadj) atomicAdd(&mxa_sh[0], n_maxadj);
    }
    __syncthreads();
    if (o_y >= 0)
        out[o_y] = cls_a != 0 ? 0.0 : bfc ? bfc_after_c(st, c1a, dec_sh[0], mxa_sh[0]) - st.before : classical_bc(curv_type);
}

// the candidate drawn on the host, by index: (k, l) never leaves the device (dcr_sdrf_tail_at)
__global__ void k_pick_candidate(const int32_t *ci, const int32_t *cj, int64_t index, DevResult *res) {
    store_candidate(res, ci, cj, index);
    res->draw_status = 0;
}

// ---- the draw of sdrf_no_cuda.py:49-50 on the device -------------------------------------------------------------------
// np.random.choice(n, p = softmax(improvements, tau)) is: cdf = cumsum(p); cdf /= cdf[-1]; searchsorted(cdf, u, 'right') with
// ONE uniform u from the global stream (the host draws it: it does not depend on anything computed here).  The index is the
// first i with cdf_i / t > u, i.e. with P_i > u · P_n for the exact prefix sums P of e_i = exp(tau · improvement_i): numpy's
// floating-point chain (its exp, the pairwise sum S, e / S, the sequential cumsum, the division by t) and the sums formed
// here each stay within (n + 64) · 2^-53 · P_n of those exact values, so when u · P_n is further than a margin of
// (n + 1024) · 2^-51 · P_n from both P_{i-1} and P_i the comparison numpy makes at i - 1 and at i has the outcome found here
// and i IS the index numpy returns.  When it is closer (probability ~ 1e-10 per draw), or anything is not finite, or there is
// no candidate, nothing is decided here: draw_status says so, the tail kernels leave the graph alone, and the host runs the
// exact path (numpy's own exp and sums) for this iteration.
constexpr int DRAW_BLOCKS = 256;

// tau = +inf: softmax is one-hot at the first arg-max of the improvements (utils/softmax.py:5-8), so the index np.random.choice
// returns is that arg-max whatever the uniform (which it still consumes: the caller has taken it).
__global__ void k_draw_from_argmax(const int32_t *ci, const int32_t *cj, DevResult *res) {
    const int64_t n = res->n_cand, idx = res->imp_argmax;
    if (n <= 0) {
        res->draw_status = 2;
        res->draw_idx = -1;
        return;
    }
    if (idx < 0 || idx >= n) {  // (not a number anywhere: the host path decides what numpy does with it)
        res->draw_status = 1;
        res->draw_idx = -1;
        return;
    }
    store_candidate(res, ci, cj, idx);
    res->draw_idx = idx;
    res->draw_status = 0;
}

// The n candidates are cut into DRAW_BLOCKS blocks of L, a block into 256 segments of l: [t0, t1) is segment t of block b
// (empty behind the end of the block or of the list).
__device__ inline void draw_segment(int64_t n, int b, int t, int64_t &t0, int64_t &t1) {
    const int64_t L = (n + DRAW_BLOCKS - 1) / DRAW_BLOCKS, l = (L + 255) / 256;
    const int64_t b0 = (int64_t)b * L, bend = b0 + L < n ? b0 + L : n;
    t0 = b0 + (int64_t)t * l;
    t1 = t0 + l < bend ? t0 + l : bend;
}

// the sum of exp(tau * improvement) over that segment, added in index order
__device__ inline double draw_segment_sum(const double *__restrict__ imp, int64_t n, double tau, int b, int t) {
    int64_t t0, t1;
    draw_segment(n, b, t, t0, t1);
    double s = 0.0;
    for (int64_t k = t0; k < t1; ++k) s += exp(imp[k] * tau);
    return s;
}

__device__ void draw_block_sum(const double *__restrict__ imp, const DevResult *res, double tau, double *__restrict__ bsum) {
    __shared__ double red[256];
    red[threadIdx.x] = draw_segment_sum(imp, res->n_cand, tau, (int)blockIdx.x, (int)threadIdx.x);
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) __hip_atomic_store(&bsum[blockIdx.x], red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (through the L2: last_arriver)
}

__device__ void draw_pick_block(const double *__restrict__ imp, const int32_t *__restrict__ ci, const int32_t *__restrict__ cj,
                                DevResult *res, double tau, double u, const double *bsum, double margin_scale) {
    __shared__ double pre[256];
    __shared__ int found;
    const int t = threadIdx.x;
    const int64_t n = res->n_cand;
    if (n <= 0) {
        if (t == 0) {
            res->draw_status = 2;
            res->draw_idx = -1;
        }
        return;
    }
    // inclusive prefix of the block sums (256 values: one thread adds them in order)
    pre[t] = __hip_atomic_load(&bsum[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (other workgroups' sums)
    __syncthreads();
    if (t == 0) {
        double a = 0.0;
        for (int k = 0; k < DRAW_BLOCKS; ++k) {
            a += pre[k];
            pre[k] = a;
        }
        found = DRAW_BLOCKS;
    }
    __syncthreads();
    const double total = pre[DRAW_BLOCKS - 1];
    const double T = u * total;
    // (false for NaN too; far from the subnormal range, where the relative error bounds behind the margin do not hold)
    const bool fine = total > 1e-250 && total < 1e300;
    if (fine && pre[t] > T) atomicMin(&found, t);
    __syncthreads();
    const int bs = found;
    if (!fine || bs >= DRAW_BLOCKS) {
        if (t == 0) {
            res->draw_status = 1;
            res->draw_idx = -1;
            res->draw_total = total;
        }
        return;
    }
    const double base = bs == 0 ? 0.0 : pre[bs - 1];
    __syncthreads();
    // inside block bs: the threads' segment sums, then the segment that crosses T is walked element by element
    pre[t] = draw_segment_sum(imp, n, tau, bs, t);
    __syncthreads();
    if (t == 0) {
        const double margin = (double)(n + 1024) * 0x1p-51 * total * margin_scale;
        double run = base;
        int64_t idx = -1;
        double below = 0.0, above = 0.0;
        for (int k = 0; k < 256 && idx < 0; ++k) {
            if (run + pre[k] > T) {
                int64_t s0, s1;
                draw_segment(n, bs, k, s0, s1);
                for (int64_t q = s0; q < s1; ++q) {
                    const double prev = run;
                    run += exp(imp[q] * tau);
                    if (run > T) {
                        idx = q;
                        below = T - prev;
                        above = run - T;
                        break;
                    }
                }
                break;  // (not found inside a segment whose sum crosses: rounding; left undecided)
            }
            run += pre[k];
        }
        const bool ok = idx >= 0 && above > margin && (idx == 0 || below > margin);
        res->draw_total = total;
        res->draw_gap = idx >= 0 ? (above < below || idx == 0 ? above : below) / total : 0.0;
        res->draw_idx = ok ? idx : -1;
        res->draw_status = ok ? 0 : 1;
        if (ok) store_candidate(res, ci, cj, idx);
    }
}

// Block sums of exp(tau * improvement); the LAST block to finish picks the index.
__global__ void __launch_bounds__(256) k_draw_partial(const double *__restrict__ imp, const int32_t *__restrict__ ci,
                                                       const int32_t *__restrict__ cj, DevResult *res, double tau, double u,
                                                       double *bsum, double margin_scale, ImpStats *st) {
    draw_block_sum(imp, res, tau, bsum);
    if (!last_arriver(&st->done_draw, (int)gridDim.x)) return;
    // (the block sums are read with sc1 loads in draw_pick_block; everything else it reads was written by earlier kernels)
    draw_pick_block(imp, ci, cj, res, tau, u, bsum, margin_scale);
}

// ---------------------------------------------------------------------------------------------
// host side: the scratch of a graph, the launches other translation units call
// ---------------------------------------------------------------------------------------------
// Every buffer the SDRF step needs beyond the graph itself: dcr_graph::sdrf, created with the graph (sdrf_scratch_create),
// grown on demand.  Nothing outside this file looks inside.
struct SdrfScratch {
    // what the improvement kernels see as an ImpBuf (imp_view): the table, three arrays of one capacity; the row arrays, eight of
    // one capacity; the admissibility bitmap; one ImpStats
    DevBuf<int32_t> keys, posx, posy;
    DevBuf<int32_t> c1, c2, rowcount, rowoff, clsx, clsy;
    DevBuf<int4> descx, descy;
    DevBuf<uint32_t> adjbits;
    DevBuf<ImpStats> st;
    bool table_dirty = true;      // the table is not all-empty (fresh allocation, or a pipeline that did not reach its last kernel)
    DevBuf<double> out;           // compacted improvements and their candidate pairs, three arrays of one capacity
    DevBuf<int32_t> ci, cj;
    PinnedBuf<double> out_h;      // pinned host mirrors
    PinnedBuf<int32_t> ci_h, cj_h;
    int64_t n = 0;                // candidates of the last pipeline that was read back
    DevBuf<Ext> red_scratch;      // [ARGEXT_BLOCKS] per-workgroup partial extrema, allocated on first use (red_scratch_of)
    DevBuf<double> draw_bsum;     // [DRAW_BLOCKS] device-side draw: block sums of exp(tau * improvement)
};

constexpr int ARGEXT_BLOCKS = 1024;  // (8192 blocks: 92 us instead of 33 on S100k, the per-block reduction dominates)

static ImpBuf imp_view(const SdrfScratch &S) {  // the raw pointers as they are now: taken again after any growth
    return ImpBuf{S.keys.p, S.posx.p, S.posy.p, S.c1.p, S.c2.p, S.clsx.p, S.clsy.p, S.descx.p, S.descy.p, S.rowcount.p, S.rowoff.p,
                  S.adjbits.p, S.st.p};
}

// Buffers that share one capacity: nothing when `need` fits; otherwise every one is freed, then allocated again with `next`
// elements.  A failure halfway leaves the whole group empty, which the next call accepts.
template <typename First, typename... Rest>
static int regrow_group(int64_t need, int64_t next, First &first, Rest &...rest) {
    if (need <= first.cap) return DCR_OK;
    first.free();
    (rest.free(), ...);
    int rc = first.alloc(next);
    ((rc = rc == DCR_OK ? rest.alloc(next) : rc), ...);
    if (rc != DCR_OK) {
        first.free();
        (rest.free(), ...);
    }
    return rc;
}

int sdrf_scratch_create(dcr_graph *g) {
    SdrfScratch *S = g->sdrf = new SdrfScratch();
    DCR_TRY(S->st.alloc(1));
    DCR_HIP(hipMemsetAsync(S->st.p, 0xFF, sizeof(ImpStats), g->stream));  // (pos_x_in_y = -1)
    DCR_TRY(S->draw_bsum.alloc(DRAW_BLOCKS));
    return DCR_OK;
}

void sdrf_scratch_destroy(dcr_graph *g) {
    delete g->sdrf;
    g->sdrf = nullptr;
}

static int red_scratch_of(dcr_graph *g, Ext **out) {  // allocated on first use
    SdrfScratch &S = *g->sdrf;
    if (!S.red_scratch.p) DCR_TRY(S.red_scratch.alloc(ARGEXT_BLOCKS));
    *out = S.red_scratch.p;
    return DCR_OK;
}

static inline int nparts_threads(int nparts) { return nparts > 1024 ? 1024 : nparts > 256 ? 512 : 256; }  // threads of the one-workgroup reduction

static inline unsigned argext_blocks(int64_t cap_total) {  // workgroups of an edge sweep
    const int64_t blocks = (cap_total + 255) / 256;
    return (unsigned)(blocks > ARGEXT_BLOCKS ? ARGEXT_BLOCKS : blocks < 1 ? 1 : blocks);
}

int launch_argext(dcr_graph *g, int want_max, int excl_u, int excl_v, hipStream_t st) {
    if (!st) st = g->stream;
    g->amax_valid = false;  // the ext fields of the result block are about to be overwritten
    Ext *partial = nullptr;
    DCR_TRY(red_scratch_of(g, &partial));
    RowView vw{g->rowinfo.p, g->col.p, g->slot_row.p};
    const unsigned blocks = argext_blocks(g->cap_total);
    hipLaunchKernelGGL(k_argext_edges, dim3(blocks), dim3(256), 0, st, vw, g->cap_total, g->curv.p, want_max, excl_u, excl_v, g->dres.p,
                       partial);
    hipLaunchKernelGGL(k_argext_final, dim3(1), dim3(nparts_threads((int)blocks)), 0, st, vw, (const Ext *)partial, (int)blocks,
                       want_max, g->dres.p);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

// one sweep for both extrema; the partials stay valid until the next edit (as the closing kernel's of the two-hop pass)
int launch_argext_both(dcr_graph *g, hipStream_t st, bool clear_dirty) {
    if (!st) st = g->stream;
    if (!g->ext_part.p) DCR_TRY(g->ext_part.alloc(2 * EXT_PART_BLOCKS));
    RowView vw{g->rowinfo.p, g->col.p, g->slot_row.p};
    const unsigned blocks = argext_blocks(g->cap_total);
    hipLaunchKernelGGL(k_argext_edges_both, dim3(blocks), dim3(256), 0, st, vw, g->cap_total, g->curv.p, g->ext_part.p,
                       g->ext_part.p + EXT_PART_BLOCKS, reinterpret_cast<unsigned *>(g->dirty.p),
                       clear_dirty ? (int64_t)(g->n + 3) / 4 : (int64_t)0, g->dres.p);   // (the flags hold n + 4 bytes)
    DCR_HIP(hipGetLastError());
    g->ext_part_n = (int)blocks;
    g->ext_part_valid = true;
    return DCR_OK;
}

int launch_argext_from_parts(dcr_graph *g, int want_max, hipStream_t st) {
    if (!st) st = g->stream;
    g->amax_valid = false;  // the ext fields of the result block are about to be overwritten
    RowView vw{g->rowinfo.p, g->col.p, g->slot_row.p};
    const Ext *parts = g->ext_part.p + (want_max ? EXT_PART_BLOCKS : 0);
    hipLaunchKernelGGL(k_argext_final, dim3(1), dim3(nparts_threads(g->ext_part_n)), 0, st, vw, parts, g->ext_part_n, want_max, g->dres.p);
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

}  // namespace dcr

using namespace dcr;

// the improvement pipeline of one edge (x, y), enqueued on the library stream: candidates and their improvements end up in
// the scratch's out / ci / cj, their number in the result block (n_cand); *upper_out = the bound (dx + 1)(dy + 1) on it
// amax_from_parts: the stale arg-max of the removal step reduced from the pass's partial maxima by one more workgroup of the
// first launch (the caller has checked g->ext_part_valid and sets g->amax_valid)
static int imp_enqueue(dcr_graph *g, int32_t x, int32_t y, int curv_type, int64_t *upper_out, bool amax_from_parts = false) {
    int dx, dy;
    if (g->am_valid && g->am_x == x && g->am_y == y) {  // the arg-min step already brought the degrees over
        dx = g->am_dx;
        dy = g->am_dy;
    } else {
        int2 rxy[2];
        DCR_HIP(hipMemcpyAsync(&rxy[0], g->rowinfo.p + x, sizeof(int2), hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipMemcpyAsync(&rxy[1], g->rowinfo.p + y, sizeof(int2), hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));
        dx = rxy[0].y;
        dy = rxy[1].y;
    }
    const int64_t keys = (int64_t)dx + dy;
    int64_t ts = 64;
    while (ts < 4 * keys) ts <<= 1;
    const unsigned mask = (unsigned)(ts - 1);
    const int rows = dx + 1;
    const int words = (dy + 1 + 31) / 32;
    if ((size_t)words * 4 > 150 * 1024) DCR_FAIL(DCR_ECAPACITY, "deg(y) too large for the candidate bitmap");
    const int64_t upper = (int64_t)(dx + 1) * (dy + 1);
    if (upper > INT32_MAX) DCR_FAIL(DCR_ECAPACITY, "more than 2^31 candidate pairs");

    // scratch: the table exactly as large as asked for; the row arrays and the output doubled (a re-allocation is a device
    // synchronisation + two driver calls, ~0.3 ms — a few of them inside a 20-iteration measurement are 1-2 % of it)
    SdrfScratch &S = *g->sdrf;
    if (ts > S.keys.cap) S.table_dirty = true;
    DCR_TRY(regrow_group(ts, ts, S.keys, S.posx, S.posy));
    const int64_t rows_need = (int64_t)(dx > dy ? dx : dy) + 2;
    DCR_TRY(regrow_group(rows_need, 2 * rows_need + 64, S.c1, S.c2, S.rowcount, S.rowoff, S.clsx, S.clsy, S.descx, S.descy));
    if ((int64_t)rows * words > S.adjbits.cap) DCR_TRY(S.adjbits.grow(2 * (int64_t)rows * words));
    DCR_TRY(regrow_group(upper, 2 * upper + 1024, S.out, S.ci, S.cj));
    const ImpBuf B = imp_view(S);
    RowView vw{g->rowinfo.p, g->col.p, g->slot_row.p};

    // Four launches: insert both rows and leave a descriptor per member | per candidate row: classes, 4-cycle counters,
    // admissibility bitmap, and the stage's closing statistics + scan by its last workgroup | emit, classes B and C from the
    // bitmap (and leave the table empty) | the draw (its caller).  The table is only cleared here when the previous pipeline did not leave it empty.
    if (S.table_dirty) {
        const unsigned blocks = (unsigned)((S.keys.cap + 255) / 256 > 1024 ? 1024 : (S.keys.cap + 255) / 256);
        hipLaunchKernelGGL(k_imp_clear, dim3(blocks ? blocks : 1), dim3(256), 0, g->stream, B, S.keys.cap);
    }
    S.table_dirty = true;  // (until k_imp_emit below has been enqueued)
    const int gi = (dx + dy + 255) / 256 > 0 ? (dx + dy + 255) / 256 : 1;
    const Ext *amax_parts = amax_from_parts ? g->ext_part.p + EXT_PART_BLOCKS : nullptr;
    hipLaunchKernelGGL(k_imp_insert, dim3(gi + (amax_parts ? 1 : 0)), dim3(256), 0, g->stream, vw, B, x, y, mask, amax_parts,
                       amax_parts ? g->ext_part_n : 0, g->dres.p);
    hipLaunchKernelGGL(k_imp_rows_count, dim3(rows), dim3(256), (size_t)words * 4, g->stream, vw, B, x, y, dy, mask, words,
                       curv_type, g->dres.p);
    hipLaunchKernelGGL(k_imp_emit, dim3(dx + words), dim3(256), 0, g->stream, B, x, y, dx, dy, words, curv_type, S.out.p, S.ci.p, S.cj.p, ts);
    S.table_dirty = false;
    DCR_HIP(hipGetLastError());
    *upper_out = upper;
    return DCR_OK;
}

static int check_edge_args(const dcr_graph *g, int32_t x, int32_t y, int curv_type) {
    if (x < 0 || y < 0 || x >= g->n || y >= g->n || x == y) DCR_FAIL(DCR_EINVAL, "bad node ids");
    if (curv_type < DCR_CURV_BFC || curv_type > DCR_CURV_HAANTJES) DCR_FAIL(DCR_EINVAL, "unknown curvature type");
    return DCR_OK;
}

// the candidate drawn on the host goes into the result block by its index: the tail then adds the pair (-2, -2)
static int pick_candidate(dcr_graph *g, int64_t cand_index) {
    if (!g) DCR_FAIL(DCR_EINVAL, "null graph");
    if (cand_index < 0 || cand_index >= g->sdrf->n) DCR_FAIL(DCR_EINVAL, "candidate index out of range");
    DCR_HIP(hipSetDevice(g->device));
    hipLaunchKernelGGL(k_pick_candidate, dim3(1), dim3(1), 0, g->stream, g->sdrf->ci.p, g->sdrf->cj.p, cand_index, g->dres.p);
    return DCR_OK;
}

static void fill_added(const dcr_graph *g, int32_t out_added[2]) {  // after a synchronisation: the pair the tail added
    if (!out_added) return;
    out_added[0] = g->hres.p->cand_i;
    out_added[1] = g->hres.p->cand_j;
}

extern "C" {

int dcr_argext(dcr_graph *g, int want_max, int32_t excl_u, int32_t excl_v, int32_t *out_u, int32_t *out_v,
               double *out_val) {
    if (!g) DCR_FAIL(DCR_EINVAL, "null graph");
    if (!g->curv_valid) DCR_FAIL(DCR_ESTATE, "dcr_argext needs a curvature pass first");
    DCR_HIP(hipSetDevice(g->device));
    if (excl_u > excl_v) {
        int32_t t = excl_u;
        excl_u = excl_v;
        excl_v = t;
    }
    DCR_TRY(launch_argext(g, want_max, excl_u, excl_v));
    DCR_TRY(sync_result(g));
    if (g->hres.p->ext_slot < 0) DCR_FAIL(DCR_ENOTFOUND, "graph has no (eligible) edges");
    if (out_u) *out_u = g->hres.p->ext_u;
    if (out_v) *out_v = g->hres.p->ext_v;
    if (out_val) *out_val = g->hres.p->ext_val;
    return DCR_OK;
}

int dcr_improvements(dcr_graph *g, int32_t x, int32_t y, int curv_type, int want_candidates, int64_t *n_out,
                     const double **out_improvement, const int32_t **out_ci, const int32_t **out_cj) {
    if (!g || !n_out) DCR_FAIL(DCR_EINVAL, "null argument");
    DCR_TRY(check_edge_args(g, x, y, curv_type));
    DCR_HIP(hipSetDevice(g->device));
    SdrfScratch &S = *g->sdrf;
    int64_t upper = 0;
    DCR_TRY(imp_enqueue(g, x, y, curv_type, &upper));
    // one host sync: the result block and the values go out together; the candidate count is not known yet, so the
    // copy is sized by its upper bound (dx+1)(dy+1), which the real count nearly reaches on a sparse graph
    if (upper > 0 && out_improvement) {
        if (upper > S.out_h.cap) DCR_TRY(S.out_h.alloc(upper + upper / 4 + 1024));
        DCR_HIP(hipMemcpyAsync(S.out_h.p, S.out.p, sizeof(double) * (size_t)upper, hipMemcpyDeviceToHost, g->stream));
    }
    if (upper > 0 && want_candidates) {
        if (upper > S.ci_h.cap) DCR_TRY(S.ci_h.alloc(upper + upper / 4 + 1024));
        if (upper > S.cj_h.cap) DCR_TRY(S.cj_h.alloc(upper + upper / 4 + 1024));
        DCR_HIP(hipMemcpyAsync(S.ci_h.p, S.ci.p, sizeof(int32_t) * (size_t)upper, hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipMemcpyAsync(S.cj_h.p, S.cj.p, sizeof(int32_t) * (size_t)upper, hipMemcpyDeviceToHost, g->stream));
    }
    DCR_TRY(sync_result(g));
    const int64_t n = g->hres.p->n_cand;
    if (n < 0 || n > upper) DCR_FAIL(DCR_ESTATE, "candidate count outside its bound");
    S.n = n;
    *n_out = n;
    // The removal step looks for the highest STALE curvature (sdrf_no_cuda.py:57-61), which does not depend on the edge
    // about to be drawn (that one is excluded there only because it has no stale value): compute it now, while the host
    // draws, and let dcr_sdrf_tail* pick it up.  Any pass or edit in between drops it.
    if (g->curv_valid && n > 0) {
        if (g->ext_part_valid) DCR_TRY(launch_argext_from_parts(g, 1));  // left by the two-hop pass's closing kernel
        else DCR_TRY(launch_argext(g, 1, -1, -1));
        g->amax_valid = true;
    }
    if (out_improvement) *out_improvement = n > 0 ? S.out_h.p : nullptr;
    if (out_ci) *out_ci = (n > 0 && want_candidates) ? S.ci_h.p : nullptr;
    if (out_cj) *out_cj = (n > 0 && want_candidates) ? S.cj_h.p : nullptr;
    return DCR_OK;
}

int dcr_improvements_argmax(dcr_graph *g, int64_t *out_index) {
    if (!g || !out_index) DCR_FAIL(DCR_EINVAL, "null argument");
    const int64_t n = g->sdrf->n;
    if (n <= 0) DCR_FAIL(DCR_ESTATE, "no candidates from the last dcr_improvements call");
    DCR_HIP(hipSetDevice(g->device));
    Ext *partial = nullptr;
    DCR_TRY(red_scratch_of(g, &partial));
    const int64_t blocks = (n + 255) / 256 > ARGEXT_BLOCKS ? ARGEXT_BLOCKS : (n + 255) / 256;
    hipLaunchKernelGGL(k_argmax_array, dim3((unsigned)blocks), dim3(256), 0, g->stream, g->sdrf->out.p, n, (const DevResult *)nullptr,
                       partial);
    hipLaunchKernelGGL(k_argmax_final, dim3(1), dim3(256), 0, g->stream, (const Ext *)partial, (int)blocks, g->dres.p);
    DCR_HIP(hipGetLastError());
    DCR_TRY(sync_result(g));
    *out_index = g->hres.p->imp_argmax;
    return DCR_OK;
}

int dcr_candidate_at(dcr_graph *g, int64_t index, int32_t *out_i, int32_t *out_j) {
    if (!g || !out_i || !out_j) DCR_FAIL(DCR_EINVAL, "null argument");
    if (index < 0 || index >= g->sdrf->n) DCR_FAIL(DCR_EINVAL, "candidate index out of range");
    DCR_HIP(hipSetDevice(g->device));
    DCR_HIP(hipMemcpyAsync(out_i, g->sdrf->ci.p + index, sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
    DCR_HIP(hipMemcpyAsync(out_j, g->sdrf->cj.p + index, sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
    DCR_HIP(hipStreamSynchronize(g->stream));
    return DCR_OK;
}

}  // extern "C"

// The tail of an iteration: prepare (argument checks, host bookkeeping), enqueue (add, dirty flags, stale arg-max, conditional
// remove), then — after some synchronisation has brought the result block over — finish (edge count, degree bound, outputs).
// run_tail holds the three together; with a TailPass the synchronisation is the NEXT iteration's curvature pass and first
// minimum, enqueued right behind the edit without a host round trip in between.
struct TailCall {
    int32_t add_k, add_l;
    int do_remove;
    double bound;
    bool adding, have_amax;
    int edit_add, edit_rem;
};

struct TailPass {  // arguments of dcr_curvature_pass_argmin
    int curv_type, incremental;
    int32_t *out_u, *out_v;
    double *out_val;
};

static int tail_prepare(dcr_graph *g, int32_t add_k, int32_t add_l, int do_remove, double removal_bound, TailCall *tc) {
    if (!g) DCR_FAIL(DCR_EINVAL, "null graph");
    if (do_remove && !g->curv_valid) DCR_FAIL(DCR_ESTATE, "removal needs a curvature pass first");
    tc->adding = add_k >= 0 || add_k == -2;  // -2: the pair k_pick_candidate or the device-side draw left in the result block
    if (add_k >= 0) {
        if (add_l < 0 || add_k >= g->n || add_l >= g->n || add_k == add_l) DCR_FAIL(DCR_EINVAL, "bad edge to add");
        if (add_k > add_l) {
            int32_t t = add_k;
            add_k = add_l;
            add_l = t;
        }
    }
    tc->add_k = add_k;
    tc->add_l = add_l;
    tc->do_remove = do_remove;
    tc->bound = removal_bound;
    DCR_HIP(hipSetDevice(g->device));
    g->am_valid = false;
    tc->have_amax = g->amax_valid;  // computed on this graph before the add: nothing to exclude
    g->amax_valid = false;
    // edit numbers for the incremental pass's flags (edge_dirty): the add, then the removal
    tc->edit_add = g->pending_edits;
    tc->edit_rem = g->pending_edits + (tc->adding ? 1 : 0);
    g->pending_edits += (tc->adding ? 1 : 0) + (do_remove ? 1 : 0);
    return DCR_OK;
}

static int tail_enqueue(dcr_graph *g, const TailCall &tc, bool first_attempt) {
    if (tc.adding && (!tc.do_remove || (tc.have_amax && first_attempt))) {  // nothing to compute in between: one launch
        launch_sdrf_tail(g, tc.add_k, tc.add_l, tc.edit_add, tc.do_remove, tc.bound, tc.edit_rem);
        DCR_HIP(hipGetLastError());
        return DCR_OK;
    }
    launch_add_edge(g, tc.add_k, tc.add_l);
    launch_mark_dirty(g, tc.add_k, tc.add_l, tc.edit_add);  // after the append: the new neighbours are flagged too
    if (tc.do_remove) {
        if (!(tc.have_amax && first_attempt))
            DCR_TRY(launch_argext(g, 1, tc.adding ? tc.add_k : -1, tc.adding ? tc.add_l : -1));
        launch_remove_if_above(g, tc.bound, tc.edit_rem);
    }
    DCR_HIP(hipGetLastError());
    return DCR_OK;
}

// after a synchronisation that brought the result block over: host-side bookkeeping and outputs (out_max_val: the stale
// maximum, for the callers whose result block still holds it — a pass behind the tail overwrites the ext fields)
static void tail_finish(dcr_graph *g, const TailCall &tc, int32_t out_removed[2], double *out_max_val) {
    if (tc.adding && g->hres.p->add_status == 0) {
        g->n_edges++;
        g->max_deg_bound++;
    }
    int32_t ru = -1, rv = -1;
    if (tc.do_remove) {
        ru = g->hres.p->removed_u;
        rv = g->hres.p->removed_v;
        if (ru >= 0) g->n_edges--;
        if (out_max_val) *out_max_val = g->hres.p->ext_slot >= 0 ? g->hres.p->ext_val : 0.0;
    }
    if (out_removed) {
        out_removed[0] = ru;
        out_removed[1] = rv;
    }
}

// Enqueue, synchronise (pass: through the next curvature pass and its first minimum), finish.  A row overflow of the add —
// rare: rows carry slack — is seen only after the synchronisation; nothing was edited then (the removal is skipped when the add
// overflows): the rows are laid out again and the tail replayed once, the pass with it.  add_status == 3 (the device-side draw
// left nothing to add: nothing was edited) skips the bookkeeping; it cannot occur behind k_pick_candidate or an explicit pair,
// which never leave a draw status other than 0, so the one check serves every caller.
static int run_tail(dcr_graph *g, const TailCall &tc, const TailPass *pass, int32_t out_removed[2], double *out_max_val) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        DCR_TRY(tail_enqueue(g, tc, attempt == 0));
        int rc = DCR_OK;
        if (pass) {
            // the pass sizes its launches by this upper bound (which class kernels run at all): count the pending add in, on the
            // replay too — relayout() has just reset the bound to the exact maximum BEFORE the add
            g->max_deg_bound++;
            rc = dcr_curvature_pass_argmin(g, pass->curv_type, pass->incremental, pass->out_u, pass->out_v, pass->out_val);  // synchronises
            g->max_deg_bound--;  // (tail_finish counts it once the add is known to have happened)
        } else {
            DCR_TRY(sync_result(g));
        }
        if (g->hres.p->add_status != 1) {
            if (rc == DCR_OK) break;
            // the edit did happen on the device (the result block is from a completed synchronisation unless the failure was
            // the HIP call itself): keep the host's edge count and degree bound in step before reporting
            if (rc != DCR_EHIP && g->hres.p->add_status != 3) tail_finish(g, tc, out_removed, out_max_val);
            return rc;
        }
        if (attempt == 1) DCR_FAIL(DCR_ECAPACITY, "row still full after relayout");
        DCR_TRY(relayout(g));
    }
    if (g->hres.p->add_status != 3) tail_finish(g, tc, out_removed, out_max_val);
    return DCR_OK;
}

extern "C" {

int dcr_sdrf_tail(dcr_graph *g, int32_t add_k, int32_t add_l, int do_remove, double removal_bound,
                  int32_t out_removed[2], double *out_max_val) {
    TailCall tc;
    DCR_TRY(tail_prepare(g, add_k, add_l, do_remove, removal_bound, &tc));
    return run_tail(g, tc, nullptr, out_removed, out_max_val);
}

int dcr_sdrf_tail_at(dcr_graph *g, int64_t cand_index, int do_remove, double removal_bound, int32_t out_added[2],
                     int32_t out_removed[2], double *out_max_val) {
    DCR_TRY(pick_candidate(g, cand_index));
    TailCall tc;
    DCR_TRY(tail_prepare(g, -2, -2, do_remove, removal_bound, &tc));
    DCR_TRY(run_tail(g, tc, nullptr, out_removed, out_max_val));
    fill_added(g, out_added);
    return DCR_OK;
}

// Tail of iteration i and the head of iteration i + 1 in one call with ONE host synchronisation: add the drawn
// candidate, conditional removal (sdrf_no_cuda.py:51,56-66), then the curvature pass of the next iteration and its first
// minimum (:24,:27).  The result block carries the tail's outcome and the arg-min over together.
int dcr_sdrf_tail_at_pass_argmin(dcr_graph *g, int64_t cand_index, int do_remove, double removal_bound, int curv_type,
                                 int incremental, int32_t out_added[2], int32_t out_removed[2], int32_t *out_u, int32_t *out_v,
                                 double *out_val) {
    DCR_TRY(pick_candidate(g, cand_index));
    TailCall tc;
    DCR_TRY(tail_prepare(g, -2, -2, do_remove, removal_bound, &tc));
    const TailPass pass{curv_type, incremental, out_u, out_v, out_val};
    DCR_TRY(run_tail(g, tc, &pass, out_removed, nullptr));
    fill_added(g, out_added);
    return DCR_OK;
}

// One whole iteration of the loop body for finite tau without moving the improvements to the host: the improvement pipeline
// of the edge (x, y) found by the previous call, the draw on the device (k_draw_*: the host supplies the uniform it has taken
// from numpy's stream), the tail (add, conditional removal) and the NEXT iteration's curvature pass and first minimum
// (sdrf_no_cuda.py:29-66, then :24,:27).  Two host round trips, each carrying the 1 KB result block only.  *out_status: 0
// done; 1 the draw was left undecided, 2 there was no candidate — in both cases NOTHING was edited (and no pass run) and the
// caller runs the iteration through dcr_improvements / dcr_sdrf_tail* instead.
int dcr_sdrf_iteration_device_draw(dcr_graph *g, int32_t x, int32_t y, int curv_type, double tau, double uniform, int do_remove,
                                   double removal_bound, int incremental, int *out_status, int64_t *out_n_cand,
                                   int32_t out_added[2], int32_t out_removed[2], int32_t *out_u, int32_t *out_v, double *out_val) {
    if (!g || !out_status || !out_n_cand) DCR_FAIL(DCR_EINVAL, "null argument");
    DCR_TRY(check_edge_args(g, x, y, curv_type));
    const bool tau_inf = tau > 1.7e308;  // +inf: the first arg-max
    if (!(tau == tau) || tau < -1.7e308 || !(uniform >= 0.0 && uniform < 1.0))
        DCR_FAIL(DCR_EINVAL, "device draw: tau finite or +inf and a uniform in [0, 1) expected");
    if (do_remove && !g->curv_valid) DCR_FAIL(DCR_ESTATE, "removal needs a curvature pass first");
    DCR_HIP(hipSetDevice(g->device));
    SdrfScratch &S = *g->sdrf;
    // the stale arg-max of the removal step does not depend on the edge about to be drawn (see dcr_improvements), nor on the
    // improvement pipeline: beside it, on a stream of its own (it writes other fields of the result block)
    const bool amax = g->curv_valid && do_remove;
    const bool amax_parts = amax && g->ext_part_valid;  // one small reduction over what the pass's closing kernel left: in line
    if (amax && !amax_parts) {
        DCR_HIP(hipEventRecord(g->ev_fork, g->stream));
        DCR_HIP(hipStreamWaitEvent(g->side[0], g->ev_fork, 0));
        DCR_TRY(launch_argext(g, 1, -1, -1, g->side[0]));
        DCR_HIP(hipEventRecord(g->ev_join[0], g->side[0]));
    }
    int64_t upper = 0;
    if (amax_parts) g->amax_valid = false;  // the ext fields of the result block are about to be overwritten
    DCR_TRY(imp_enqueue(g, x, y, curv_type, &upper, amax_parts));
    if (amax_parts) {
        g->amax_valid = true;   // (reduced by one more workgroup of the pipeline's first launch)
    } else if (amax) {
        DCR_HIP(hipStreamWaitEvent(g->stream, g->ev_join[0], 0));
        g->amax_valid = true;
    }
    // (DCR_DRAW_MARGIN_SCALE widens the margin: the tests use it to send draws down the undecided path)
    const double margin_scale = getenv("DCR_DRAW_MARGIN_SCALE") ? atof(getenv("DCR_DRAW_MARGIN_SCALE")) : 1.0;
    if (tau_inf && margin_scale <= 1.0) {
        Ext *partial = nullptr;
        DCR_TRY(red_scratch_of(g, &partial));
        // (red_scratch is free again: the stale arg-max beside the pipeline has been joined above)
        hipLaunchKernelGGL(k_argmax_array, dim3(256), dim3(256), 0, g->stream, S.out.p, (int64_t)0, (const DevResult *)g->dres.p, partial);
        hipLaunchKernelGGL(k_argmax_final, dim3(1), dim3(256), 0, g->stream, (const Ext *)partial, 256, g->dres.p);
        hipLaunchKernelGGL(k_draw_from_argmax, dim3(1), dim3(1), 0, g->stream, S.ci.p, S.cj.p, g->dres.p);
    } else {
        hipLaunchKernelGGL(k_draw_partial, dim3(DRAW_BLOCKS), dim3(256), 0, g->stream, S.out.p, S.ci.p, S.cj.p, g->dres.p, tau, uniform,
                           S.draw_bsum.p, margin_scale >= 1.0 ? margin_scale : 1.0, S.st.p);
    }
    const auto nothing_edited = [&]() {
        if (out_removed) out_removed[0] = out_removed[1] = -1;
        if (out_added) out_added[0] = out_added[1] = -1;
        return DCR_OK;
    };
    // A host round trip here, without any transfer or host arithmetic: enqueuing the tail and the pass behind a stream that
    // is still working through the small kernels above cost 0.2 ms per iteration more than enqueuing them on an idle one
    // (measured, interleaved in one run: 1.89 against 1.59 ms), and the draw's verdict comes over with it, so an undecided
    // draw costs no wasted pass.
    // (Not in front of an INCREMENTAL pass — three launches on this one stream, 0.08 ms: there the round trip costs a tenth of
    //  the iteration and saves nothing; an undecided draw makes the tail a no-op (it reads the verdict in the result block), the
    //  pass then finds nothing flagged, and the verdict comes over with the pass's result.)
    if (!incremental) {
        DCR_TRY(sync_result(g));
        S.n = *out_n_cand = g->hres.p->n_cand;
        *out_status = g->hres.p->draw_status;
        if (g->hres.p->draw_status != 0) return nothing_edited();
    }
    TailCall tc;
    DCR_TRY(tail_prepare(g, -2, -2, do_remove, removal_bound, &tc));
    const TailPass pass{curv_type, incremental, out_u, out_v, out_val};
    DCR_TRY(run_tail(g, tc, &pass, out_removed, nullptr));
    S.n = *out_n_cand = g->hres.p->n_cand;
    *out_status = g->hres.p->draw_status;
    if (g->hres.p->draw_status != 0 || g->hres.p->add_status == 3) {  // nothing was edited; the pass ran on the same graph
        if (g->hres.p->draw_status == 0) DCR_FAIL(DCR_ESTATE, "device draw: edit skipped without a draw status");
        return nothing_edited();
    }
    fill_added(g, out_added);
    return DCR_OK;
}

}  // extern "C"
