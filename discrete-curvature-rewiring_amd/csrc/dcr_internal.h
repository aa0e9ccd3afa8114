// Internal declarations shared by the translation units of libdcr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "dcr.h"
#include "dcr_pass_route.h"

namespace dcr {

void set_error(const std::string &msg);

#define DCR_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            ::dcr::set_error(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" + (strrchr(__FILE__, '/') ? strrchr(__FILE__, '/') + 1 : __FILE__) + ":" + std::to_string(__LINE__) + ")"); \
            return DCR_EHIP;                                                                   \
        }                                                                                      \
    } while (0)

#define DCR_TRY(expr)                 \
    do {                              \
        int _rc = (expr);             \
        if (_rc != DCR_OK) return _rc; \
    } while (0)

#define DCR_FAIL(code, msg)       \
    do {                          \
        ::dcr::set_error(msg);    \
        return (code);            \
    } while (0)

// ---- curvature-pass work bins ----------------------------------------------
// An undirected edge (u,v) needs an LDS hash set over N(u) ∪ N(v) ∪ {u,v}; the bin is chosen by
// that size so the table keeps a load factor <= 1/4 (1/2 in the last bin).  Threads per edge ("team") grow with the bin.
constexpr int NBINS = 5;
constexpr int GIANT_LIST_CAP = 65536;  // edges beyond every LDS table that one pass can list
constexpr int BIN_SLOTS[NBINS] = {128, 512, 2048, 4096, 32768};
constexpr int BIN_TEAM[NBINS] = {64, 64, 256, 512, 1024};
constexpr int MAX_TABLE_KEYS = BIN_SLOTS[NBINS - 1] / 2;  // du + dv + 2 must not exceed this
constexpr int32_t MAX_NODES = (1 << 30) - 2;              // two tag bits live above the key

// small result block mirrored in pinned host memory
struct DevResult {
    double ext_val;       // argext value
    int32_t ext_slot;     // argext slot (-1: none)
    int32_t ext_u, ext_v;
    int32_t ext_du, ext_dv;  // their degrees (saves dcr_improvements a round trip)
    int32_t add_status;   // 0 ok, 1 row overflow (nothing changed), 2 already present, 3 no edge drawn on the device (nothing changed)
    int32_t removed_u, removed_v;
    int32_t overflow_row;
    int32_t max_keys;     // largest du+dv+2 seen by classify
    int32_t work_count[NBINS];
    int32_t work_next[NBINS];  // dequeue cursors of the persistent bin kernels
    int32_t nc_count[5];       // node-centric pass: units per degree class
    int32_t nc_next[5];        // dequeue cursors of its kernels
    int32_t nc_bucket[16];     // units per degree bucket (plan phase 0)
    int32_t nc_fill[16];       // placement cursors per bucket (plan phase 1)
    int32_t flag_too_big; // an edge exceeded MAX_TABLE_KEYS and could not be put on the giant list either
    int32_t giant_count;  // edges beyond every LDS table, listed for the device-memory path (dcr_bfc_giant.hip)
    int32_t hub_count;    // nodes with more neighbours than the largest table (k_find_hubs)
    int64_t n_cand;
    int64_t imp_argmax;
    int32_t cand_i, cand_j;
    // device-side draw (dcr_sdrf_iteration_device_draw): the index np.random.choice would return, and whether the margins
    // that make it certain held (0 ok; 1 undecided / not finite: the host draws; 2 no candidates)
    int64_t draw_idx;
    double draw_total, draw_gap;
    int32_t draw_status;
    int32_t draw_pad;
    int32_t misc[8];  // scratch: has_edge/remove status, and the kernels' invariant guard record
    // two-hop pass (dcr_bfc_h2.hip): units per (class, weight bucket), placement cursors, units per class.  Two halves, used in turn
    // (the parity of the pass, dcr_graph::h2_parity): the plan kernels count and place in one half, the first of them leaves the
    // other half zero for the next pass
    int32_t h2_bucket[2][24];
    int32_t h2_fill[2][24];
    int32_t h2_count[5];
    int32_t h2_failed[6];  // diagnostic: nodes whose tables filled up, per class (5: on the retry list itself)
    // triangle step, one pool per block class (0: the split class and the retry launch, 1: class M), so that the candidates of
    // a class can be taken as soon as THAT class is done: listed edges, candidates, partners; candidates the first
    // k_h2_triangles launch of the pool has taken
    int32_t h2_ntask[2], h2_ncand[2], h2_npart[2];
    int32_t h2_ncand_done[2];
    int32_t h2_fallback;  // block-class units that listed their triangle work for k_h2_triangles instead of joining it themselves
    // Edit journal (round 4): every edge the device adds or removes since the two-hop pass last brought its edge set up to
    // date: {+1 / -1, u, v} per edit, in order; edit_n keeps counting past the capacity (the host then knows the bound on
    // its own and rebuilds the set).  Written by dev_add_edge / dev_remove_edge, consumed by k_h2_plan<1> (h2_eset_apply).
    int32_t edit_n;
    int32_t edit_log[3 * 8];
    int32_t touched_n;  // nodes on the graph's touched list (every node whose dirty byte went from zero to non-zero since the flags
                        // were last cleared: dev_mark_dirty appends, whoever clears the flags resets this)
    int32_t h2_retry;   // units on the retry list (nodes whose tables filled up in their class, redone by the largest class)
    int32_t h2_status;  // 0 ok; 1: a table filled up or a list overflowed (the pass is then redone by the node-centric kernels);
                        // 2: the triangle step's pools were too small (run again with larger ones); 3: the pass was launched
                        // without its retry stage and some node needed it (run again with the stage); 4: the pass was launched
                        // without its triangle stage and some block-class unit listed for it (h2_fallback > 0: run again with
                        // the stage).  3 and 4 are only ever put in place of 0, and the closing kernel asks for the retry stage
                        // first: a pass that misses both stages leaves 3, and the host reads h2_fallback next to it
};

// Incremental pass: which edges an edit can have changed.  BFC(a,b) is a function of deg a, deg b, N(a) ∩ N(b) and the
// adjacency between DX = N(a) \ N(b) and DY = N(b) \ N(a).  Adding or removing the edge {x,l} changes the first three
// only for edges incident to x or l, and that adjacency only for the pair {x,l} itself, i.e. only for edges {a,b} with
// a in N(x) and b in N(l) (or the other way round).  Per node, one byte: DIRTY_ENDPOINT on x and l, bit A_e on the
// members of N(x) and B_e on those of N(l) for the e-th edit since the last pass (three edits fit; dcr_sdrf_tail makes
// two); further edits fall back to DIRTY_COARSE on {x,l} ∪ N(x) ∪ N(l) (every edge with a flagged endpoint).
constexpr int EDIT_LOG_CAP = 8;
constexpr int EXT_PART_BLOCKS = 16384;  // capacity of the per-block extrema arrays
__device__ inline void journal_edit(DevResult *res, int op, int32_t u, int32_t v) {  // one thread of a single-workgroup edit kernel
    const int i = res->edit_n;
    if (i >= 0 && i < EDIT_LOG_CAP) {
        res->edit_log[3 * i] = op;
        res->edit_log[3 * i + 1] = u;
        res->edit_log[3 * i + 2] = v;
    }
    res->edit_n = i + 1;
}
constexpr unsigned DIRTY_COARSE = 0x80u, DIRTY_ENDPOINT = 0x40u;
__device__ __host__ inline bool edge_dirty(unsigned du, unsigned dv) {
    if ((du | dv) & (DIRTY_COARSE | DIRTY_ENDPOINT)) return true;
    return ((((du >> 1) & dv) | ((dv >> 1) & du)) & 0x15u) != 0u;  // some edit has its A bit on one side, its B bit on the other
}

// ---- (value, slot) extrema: first in G.edges order (= smallest slot) on ties (sdrf_no_cuda.py:27,59,61) ----
struct Ext {  // how a partial result is stored; the running pair lives in two plain registers (ext_take): passed around as a
              // struct it ended up in scratch memory (88-117 scratch accesses per kernel, round 4)
    double val;
    int32_t slot;
    int32_t pad;
};

// (bv, bs) <- the better of (bv, bs) and (v, sl); a slot < 0 means "none"
__device__ inline void ext_take(double &bv, int &bs, double v, int sl, int want_max) {
    const bool better = bs < 0 || (want_max ? v > bv : v < bv) || (v == bv && sl < bs);
    if (sl >= 0 && better) {
        bv = v;
        bs = sl;
    }
}

__device__ inline void ext_wave_reduce(double &bv, int &bs, int want_max) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int os = __shfl_xor(bs, off);
        ext_take(bv, bs, ov, os, want_max);
    }
}

// shv / shs: one entry per wave of the workgroup
__device__ inline void ext_block_reduce(double &bv, int &bs, int want_max, double *shv, int *shs) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    ext_wave_reduce(bv, bs, want_max);
    if (lane == 0) {
        shv[wid] = bv;
        shs[wid] = bs;
    }
    __syncthreads();
    if (wid == 0) {
        double tv = lane < nw ? shv[lane] : 0.0;
        int ts = lane < nw ? shs[lane] : -1;
        ext_wave_reduce(tv, ts, want_max);
        if (lane == 0) {
            shv[0] = tv;
            shs[0] = ts;
        }
    }
    __syncthreads();
    bv = shv[0];
    bs = shs[0];
}
__device__ inline Ext ext_make(double v, int sl) {
    Ext e;
    e.val = v;
    e.slot = sl;
    e.pad = 0;
    return e;
}

// ---- last-workgroup ticket: the workgroup that arrives last closes a reduction over every workgroup's partial ----------
// Call from every thread of the workgroup after its payload stores, which are agent-scope relaxed atomics (sc1: through the L2).
// Every wave drains its stores (written out: a wait the compiler inserts can be dropped), the workgroup meets, and one lane
// takes the ticket with a relaxed agent-scope add.  Returns true, in every thread, in the workgroup that arrived last; that
// workgroup reads the partials with agent-scope relaxed (sc1) loads, or with plain loads behind fence(acquire, "agent").
// A workgroup-scope fence or a bare barrier is no release for other CUs: it waits for no store (MI355X_MICROARCH.md,
// § Workgroup dispatch ... inter-workgroup visibility, Valid forms and the first row of its hand-off table).
template <typename T>
__device__ inline bool last_arriver(T *ticket, T arrivals) {
    __shared__ int last;
    asm volatile("s_waitcnt vmcnt(0) ; dcr ticket drain" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) last = __hip_atomic_fetch_add(ticket, (T)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == arrivals - 1;
    __syncthreads();
    return last;
}

struct ImpStats {  // per (x,y) statistics for the improvement kernels; lives in device memory
    int32_t x, y, dx, dy;
    int32_t T, s1, s2;
    int32_t max1, cnt1, max2, cnt2, sec1, sec2;  // maxima of c1/c2, their multiplicity, runner-up
    int32_t table_mask;
    int32_t deg_min_is_one;
    int32_t pos_x_in_y;  // position of x inside row y
    int32_t done_rows;   // workgroups of k_imp_rows_count that are through (the last one closes the stage: statistics, scan)
    double before;
    int32_t done_draw;   // the same for k_draw_partial (the last one picks)
    int32_t pad_;
};

template <typename T>
int dev_alloc(T **p, int64_t count, bool pinned = false) {  // pinned: page-locked host memory instead of device memory
    void *q = nullptr;
    const size_t bytes = (size_t)(count > 0 ? count : 1) * sizeof(T);
    hipError_t e = pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
    if (e != hipSuccess) {
        set_error(std::string(pinned ? "hipHostMalloc: " : "hipMalloc: ") + hipGetErrorString(e));
        return DCR_ENOMEM;
    }
    *p = (T *)q;
    return DCR_OK;
}

// A device array that owns its memory (PinnedBuf: the same in pinned host memory).  It is never copied: a copy handed to a kernel
// launch or a helper would free the memory at the end of the call, with the kernel still queued.  Kernels, helpers and the structs
// a launch takes by value get the raw pointer p, which holds until the next alloc(), grow() or swap().
template <typename T, bool PINNED = false>
struct DevBuf {
    T *p = nullptr;
    int64_t cap = 0;  // elements

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { free(); }

    void free() {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    // a new array of exactly `count` elements in place of what is there (empty if that fails); the contents are lost
    int alloc(int64_t count) {
        free();
        DCR_TRY(dev_alloc(&p, count, PINNED));
        cap = count;
        return DCR_OK;
    }
    // room for `need` elements: what is there when it is enough, else a new array of need + need / 4 + 64; the contents are lost
    int grow(int64_t need) { return need <= cap ? DCR_OK : alloc(need + need / 4 + 64); }
    void swap(DevBuf &o) {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
};
template <typename T>
using PinnedBuf = DevBuf<T, true>;

struct AnalysisState;  // dcr_analysis.h
struct SdrfScratch;    // dcr_sdrf.hip

}  // namespace dcr

struct dcr_graph {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0;
    int64_t n_edges = 0;    // undirected, tracked on the host
    int64_t cap_total = 0;  // adjacency slots allocated

    // HBM-resident graph: rows in insertion order, slack-padded
    dcr::DevBuf<int2> rowinfo;      // [n] {start slot, degree}
    dcr::DevBuf<int32_t> rowcap;    // [n] capacity of each row
    dcr::DevBuf<int32_t> col;       // [cap_total + 64] neighbour ids (padded: rows are read in aligned 16-byte pieces)
    dcr::DevBuf<int32_t> slot_row;  // [cap_total] owning row of each slot
    dcr::DevBuf<double> curv;       // [cap_total] curvature of the undirected edge stored at slot (col > row)

    // degrees of the last arg-min edge as seen by the device; dropped by any edit
    int32_t am_x = -1, am_y = -1, am_dx = 0, am_dy = 0;
    bool am_valid = false;
    bool amax_valid = false;  // the result block holds the stale arg-max of the current graph (computed ahead of the tail)

    int curv_type_last = -1;
    bool curv_valid = false;
    dcr::DevBuf<uint8_t> dirty;  // [n + 4] node flags: an incident edge was added/removed at this node or a neighbour
    bool dirty_tracked = false;  // flags cover every edit since the last pass
    int pending_edits = 0;       // edits flagged since the last pass (the first DIRTY_EDITS get exact flags)

    // node-centric pass (dcr_bfc_nc.hip): unit lists per degree class
    dcr::DevBuf<int2> nc_units[5];      // {node, first sub-unit}
    dcr::DevBuf<int32_t> nc_queues;     // dequeue cursors of the two wave-class kernels, one cache line each (allocated on first use)
    dcr::DevBuf<uint8_t> nc_touch;      // [n + 64] incremental pass: node has a flagged neighbour
    dcr::DevBuf<int2> nc_fine_list;     // incremental pass behind a few exactly flagged edits: the edges to recompute {owner, position}
    dcr::DevBuf<int32_t> touched;       // [n + 64] the flagged nodes, each once (DevResult::touched_n of them)
    double sum_deg2 = 0.0;        // sum of squared degrees when the graph was created (engine choice: size of the 2-hop neighbourhoods)
    int32_t max_deg_bound = 0;    // host-side upper bound on the largest degree (exact after create / relayout)
    int pass_impl = 0;            // 0: automatic (default: two-hop kernels for full Balanced Forman passes of graphs large enough to
                                  // pay for their fixed cost, node-centric otherwise); 1: edge-centric kernels only (DCR_PASS=edge);
                                  // 2: node-centric (DCR_PASS=nc); 3: two-hop
                                  // kernels for full Balanced Forman passes, node-centric otherwise (DCR_PASS=h2)
    int last_engine = -1;         // which implementation ran the last pass: 0 two-hop, 1 edge-centric, 2 node-centric

    // two-hop pass (dcr_bfc_h2.hip)
    dcr::DevBuf<int32_t> h2_weight;   // [n] sum of the neighbours' degrees
    dcr::DevBuf<int4> h2_units[5];    // per class {node, partitions << 16 | partition, row start, degree}
    dcr::DevBuf<uint4> h2_task;       // triangle step pools (dcr_bfc_h2.hip): two of each kind in one array, so each pool has half
    dcr::DevBuf<int4> h2_cand;        // of the array's cap
    dcr::DevBuf<int32_t> h2_part;
    dcr::DevBuf<unsigned> h2_lists;   // per-wave lists of the block classes' third step (dcr_bfc_h2.hip: H2List)
    int64_t h2_want[3] = {0, 0, 0};   // pool sizes a pass asked for (tasks, candidates, partners)
    dcr::DevBuf<unsigned> h2_bloom;   // one bit per edge (prefilter of the edge set)
    int h2_bloom_bits = 0;            // 2^bits bits in the filter: keys its reallocation, and the kernels hash with it
    dcr::DevBuf<int4> h2_retry;       // units of nodes whose tables filled up in their class (redone by the largest class)
    dcr::DevBuf<uint4> h2_rec;        // [cap_total] per directed slot {|sq| on the far side, max count, triangles, reverse slot}
    // h2_weight holds W of the CURRENT rows (bit 31 aside): k_h2_weight has filled this array and every writer of a degree since
    // has kept it (dev_add_edge / dev_remove_edge, the only writers behind dcr_graph_create; relayout() moves rows and changes no
    // degree).  False for a new graph and whenever the array is (re)allocated; a pass then runs k_h2_weight.
    bool h2_weight_valid = false;
    // the head of the last two-hop launch left the result block ready for a head without k_h2_clear: the bucket half of the other
    // parity is zero.  False for a new graph (fresh DevResult) and behind a pass that reported a status or an invariant.
    bool h2_head_clean = false;
    int h2_parity = 0;                 // the bucket half the next pass counts in
    int h2_weight_launches = 0, h2_clear_launches = 0;  // of the h2_launches: those that ran k_h2_weight / the stand-alone k_h2_clear
    dcr::DevBuf<int32_t> h2_weight_chk;  // dcr_h2_weight_check: W recomputed (diagnostic, allocated on first use)
    dcr::DevBuf<unsigned long long> h2_eset;  // [2^h2_eset_bits] every undirected edge as one 64-bit key (open addressing), rebuilt per pass
    int h2_eset_bits = 0;
    bool h2_expect_retry = false;      // some pass of this graph had nodes on the retry list: the retry stage is launched with every pass
    bool h2_expect_triangles = false;  // some pass of this graph had a block-class unit on the probe path (DevResult::h2_fallback):
                                       // the k_h2_triangles launches go with every pass
    int h2_launches = 0;               // two-hop launches of the last dcr_curvature_pass* call, and which stages the last of them carried
    bool h2_last_retry_stage = false, h2_last_tri_stage = false;
    bool h2_cleared_dirty = false;     // the last two-hop launch zeroed the incremental pass's node flags itself
    bool h2_eset_valid = false;        // the set holds the graph's edges as of the last two-hop pass; later edits are in the journal
    int h2_eset_pending = 0;           // upper bound of the edits journaled since (host-side count of the edit launches)
    int64_t h2_eset_tombs = 0;         // upper bound of the tombstones in the set (removals applied since the last rebuild)
    int32_t h2_last_count[5] = {-1, -1, -1, -1, -1};  // units per class of the previous pass (sizes the next grids)

    // edges beyond every LDS table (dcr_bfc_giant.hip): records {slot, u, v, deg u, deg v}; position map over all ids
    // (all allocated on first use)
    dcr::DevBuf<int32_t> giant_list;
    dcr::DevBuf<int32_t> giant_pos;
    dcr::DevBuf<uint32_t> giant_cnt;
    dcr::DevBuf<int32_t> giant_acc;
    dcr::DevBuf<int32_t> hub_list;  // {node, degree} pairs of the nodes above every table size
    int64_t hub_list_cap = 0;       // in pairs: the array holds twice as many elements
    dcr::DevBuf<uint32_t> hub_cnt;  // per-wave slot counters of k_hub_edges (kept all-zero between edges)

    // curvature-pass work lists (edge-centric kernels)
    dcr::DevBuf<int32_t> work[dcr::NBINS];
    int64_t work_cap = 0;  // of each of the five lists; 0 behind a relayout, which drops them (they are sized by slots)

    // per-block (value, slot) minima and maxima left by the two-hop pass's closing kernel (k_h2_final) or by the one sweep for
    // both (launch_argext_both): the first minimum after the pass and the stale first maximum of the removal step then need no
    // sweep of their own.  Valid until the next edit (a removal moves values between slots) or pass.
    dcr::DevBuf<dcr::Ext> ext_part;  // [2][EXT_PART_BLOCKS]: minima, then maxima (allocated on first use)
    int ext_part_n = 0;
    bool ext_part_valid = false;

    dcr::SdrfScratch *sdrf = nullptr;        // every buffer of the SDRF step (dcr_sdrf.hip), created with the graph
    dcr::AnalysisState *analysis = nullptr;  // every buffer of the graph-analysis calls (dcr_analysis.h), created on first use

    dcr::DevBuf<dcr::DevResult> dres;     // device
    dcr::PinnedBuf<dcr::DevResult> hres;  // its mirror in pinned host memory

    // side streams: the work bins of a curvature pass run concurrently
    hipStream_t side[dcr::NBINS - 1] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr;
    hipStream_t aux = nullptr;   // two-hop pass: the edge set is rebuilt here while the plan runs
    hipEvent_t ev_aux = nullptr;
    hipStream_t low[2] = {nullptr, nullptr};  // low priority (with side[2]): the fine-grained kernels of the two-hop pass
    hipEvent_t ev_aux2 = nullptr;
    hipEvent_t ev_join[dcr::NBINS - 1] = {nullptr, nullptr, nullptr, nullptr};
    int num_cu = 0;

    // profiling
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double pass_ms_total = 0.0;
    int64_t pass_count = 0;
    bool profile = false;

    dcr_graph() = default;
    ~dcr_graph();  // dcr_graph.hip: drains the stream, then the SDRF scratch, the analysis state, streams and events; the buffers go with the members
};
static_assert(!std::is_copy_constructible_v<dcr_graph>, "dcr_graph owns its device buffers");

namespace dcr {

// dcr_graph.hip
int relayout(dcr_graph *g);
int sync_result(dcr_graph *g);  // D2H of DevResult + stream sync
void launch_add_edge(dcr_graph *g, int32_t u, int32_t v);          // u < 0: no-op that clears add_status
void launch_remove_if_above(dcr_graph *g, double bound, int edit);  // acts on the last argext result
// add + dirty flags + conditional removal of the arg-max already in the result block, one launch (dcr_graph.hip: k_sdrf_tail)
void launch_sdrf_tail(dcr_graph *g, int32_t u, int32_t v, int edit_add, int do_remove, double bound, int edit_rem);
void launch_mark_dirty(dcr_graph *g, int32_t u, int32_t v, int edit);  // flag the edges edit number `edit` can change (>= 3: coarse)

// dcr_sdrf.hip
int sdrf_scratch_create(dcr_graph *g);    // g->sdrf and the two buffers every iteration needs
void sdrf_scratch_destroy(dcr_graph *g);  // deletes g->sdrf and with it what it holds
int launch_argext(dcr_graph *g, int want_max, int excl_u, int excl_v, hipStream_t st = nullptr);  // st: default the library stream
// the same from the per-block extrema of the last two-hop pass (g->ext_part_valid), without sweeping the edges again
int launch_argext_from_parts(dcr_graph *g, int want_max, hipStream_t st = nullptr);
int launch_argext_both(dcr_graph *g, hipStream_t st = nullptr, bool clear_dirty = false);
// reductions of per-workgroup partial results shared by the GCN kernels (csrc/dcr_gemm.hip, csrc/dcr_gcn.hip)
void launch_slab_reduce(const float *part, float *C, int64_t mn, int N, int64_t ldc, int splits, hipStream_t st);
void launch_slab_reduce_cols(const float *part, float *C, int64_t mn, int N, int ncols, int64_t ldc, int splits, hipStream_t st);
void launch_parts_finish(const float *part, int64_t n_parts, int stride, int split, int columns, float *out0, float *out1, hipStream_t st);
int process_giant_edges(dcr_graph *g, int curv_type);  // dcr_bfc_giant.hip; syncs once
int process_hub_edges(dcr_graph *g, int curv_type, bool incremental);  // dcr_bfc_giant.hip; syncs once
int giant_edge(dcr_graph *g, int u, int v, int du, int dv, int64_t slot, int curv_type, bool need_cycles, int64_t *d_out6);  // result in DevResult after the next sync

// dcr_bfc.hip: plans the pass (dcr_pass_route.h) and launches the plan; node_centric_only: planned as under DCR_PASS=nc
int launch_curvature_pass(dcr_graph *g, int curv_type, bool incremental, bool node_centric_only = false);
// dcr_bfc_nc.hip: the class kernels, or a workgroup per edge (its edge list from the flagged nodes' rows or from a sweep)
int launch_curvature_pass_nc(dcr_graph *g, int curv_type, bool incremental, bool edge_by_edge, bool list_by_rows);
// dcr_bfc_h2.hip
int launch_curvature_pass_h2(dcr_graph *g);
// what the edit kernels get: the weights they keep current, or null while there are none to keep
inline int32_t *h2_kept_weight(dcr_graph *g) { return g->h2_weight_valid ? g->h2_weight.p : nullptr; }
bool h2_grow_pools(dcr_graph *g);
int h2_weight_check(dcr_graph *g, int64_t *mismatches);  // -1: no kept weights; else the nodes whose kept W differs from the rows' 

// dcr_analysis.hip
void analysis_destroy(dcr_graph *g);  // frees g->analysis and what it holds

}  // namespace dcr
