// The parts of graph analysis that belong to no single method: the analysis buffers of a graph, the connected components, the
// scale 1 / sqrt(deg), and the plan of the rows by degree class that the row walker of dcr_analysis.h follows.
//
// Kernels:
//   k_cc_hook / k_cc_compress  min-label hooking + pointer jumping over the live slots; integer only, any schedule, same labels
//   k_inv_sqrt_degree          s = 1 / sqrt(deg) from rowinfo
#include "dcr_analysis.h"

namespace dcr {

// ---- connected components --------------------------------------------------------------------------------------------------------
__device__ inline int32_t cc_find(const int32_t *label, int32_t x) {
    for (;;) {  // label[x] <= x always, so this ends at a root
        const int32_t p = __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}

__global__ void __launch_bounds__(256) k_cc_init(int32_t *label, int64_t n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) label[v] = (int32_t)v;
}

// every live slot with col > row: hook the larger root under the smaller.  An atomicMin that lands on a node hooked meanwhile
// may drop that node's earlier link; the sweeps repeat until one changes nothing, and that last sweep has seen every edge with
// both ends under one root.
__global__ void __launch_bounds__(256) k_cc_hook(const int2 *__restrict__ rowinfo, const int32_t *__restrict__ col,
                                                  const int32_t *__restrict__ slot_row, int64_t cap_total, int32_t *label, int32_t *changed) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= cap_total) return;
    const int32_t u = slot_row[s];
    const int2 ri = rowinfo[u];
    if (s - ri.x >= (int64_t)ri.y) return;  // slack
    const int32_t v = col[s];
    if (v <= u) return;
    const int32_t ru = cc_find(label, u), rv = cc_find(label, v);
    if (ru == rv) return;
    const int32_t hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
    if (atomicMin(label + hi, lo) > lo) *changed = 1;
}

__global__ void __launch_bounds__(256) k_cc_compress(int32_t *label, int64_t n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int32_t r = cc_find(label, (int32_t)v);
    __hip_atomic_store(label + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int graph_components(dcr_graph *g, std::vector<int32_t> &labels) {
    const int64_t n = g->n;
    labels.resize((size_t)n);
    if (n == 0) return DCR_OK;
    AnalysisState &A = analysis_of(g);
    DCR_TRY(A.spc_label.grow(n));
    DCR_TRY(A.spc_ctl.grow(4));
    int32_t *const label = A.spc_label.p, *const flag = (int32_t *)A.spc_ctl.p;
    hipLaunchKernelGGL(k_cc_init, dim3(blocks_of(n)), dim3(256), 0, g->stream, label, n);
    for (int sweep = 0; g->cap_total > 0; ++sweep) {
        if (sweep > 100000) DCR_FAIL(DCR_ESTATE, "connected components did not settle");
        DCR_HIP(hipMemsetAsync(flag, 0, 4 * sizeof(int32_t), g->stream));
        hipLaunchKernelGGL(k_cc_hook, dim3(blocks_of(g->cap_total)), dim3(256), 0, g->stream, g->rowinfo.p, g->col.p, g->slot_row.p,
                           g->cap_total, label, flag);
        hipLaunchKernelGGL(k_cc_compress, dim3(blocks_of(n)), dim3(256), 0, g->stream, label, n);
        DCR_HIP(hipGetLastError());
        int32_t changed = 0;
        DCR_HIP(hipMemcpyAsync(&changed, flag, sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
        DCR_HIP(hipStreamSynchronize(g->stream));
        if (!changed) break;
    }
    DCR_HIP(hipMemcpyAsync(labels.data(), label, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
    DCR_HIP(hipStreamSynchronize(g->stream));
    return DCR_OK;
}

// ---- the scale -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_inv_sqrt_degree(const int2 *__restrict__ rowinfo, double *__restrict__ s, int64_t n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    s[v] = inv_sqrt_deg(rowinfo[v].y);
}

void inv_sqrt_degree(dcr_graph *g, double *s) {
    hipLaunchKernelGGL(k_inv_sqrt_degree, dim3(blocks_of(g->n)), dim3(256), 0, g->stream, g->rowinfo.p, s, g->n);
}

// ---- the row plan ----------------------------------------------------------------------------------------------------------------
// rows: the long rows (degree above SP_LONG_DEG), then the medium ones, then the short ones (up to SP_SHORT_DEG), each by node id
static void classify_rows(const std::vector<int2> &info, std::vector<int32_t> &rows, RowPlan *plan) {
    const int64_t n = (int64_t)info.size();
    rows.resize((size_t)n);
    int64_t nl = 0, nm = 0, ns = 0;
    for (int64_t v = 0; v < n; ++v) {
        const int d = info[(size_t)v].y;
        (d > SP_LONG_DEG ? nl : d > SP_SHORT_DEG ? nm : ns)++;
    }
    int64_t pl = 0, pm = nl, ps = nl + nm;
    for (int64_t v = 0; v < n; ++v) {
        const int d = info[(size_t)v].y;
        rows[(size_t)(d > SP_LONG_DEG ? pl : d > SP_SHORT_DEG ? pm : ps)++] = (int32_t)v;
    }
    plan->n_long = (int)nl;
    plan->n_mid = (int)nm;
    plan->n_short = (int)ns;
}

int build_row_plan(dcr_graph *g, RowPlan *plan, std::vector<int2> *info_out) {
    const int64_t n = g->n;
    std::vector<int2> own;
    std::vector<int2> &info = info_out ? *info_out : own;
    info.resize((size_t)n);
    DCR_HIP(hipMemcpyAsync(info.data(), g->rowinfo.p, sizeof(int2) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
    DCR_HIP(hipStreamSynchronize(g->stream));
    std::vector<int32_t> rows;
    classify_rows(info, rows, plan);
    AnalysisState &A = analysis_of(g);
    DCR_TRY(A.rows.grow(n));
    DCR_HIP(hipMemcpyAsync(A.rows.p, rows.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, g->stream));
    DCR_HIP(hipStreamSynchronize(g->stream));  // `rows` goes out of scope
    plan->rows = A.rows.p;
    return DCR_OK;
}

// ---- the state -------------------------------------------------------------------------------------------------------------------
AnalysisState &analysis_of(dcr_graph *g) {
    if (!g->analysis) g->analysis = new AnalysisState();
    return *g->analysis;
}

void analysis_destroy(dcr_graph *g) {
    delete g->analysis;  // every DevBuf frees its own array
    g->analysis = nullptr;
}

}  // namespace dcr

using namespace dcr;

extern "C" {

int dcr_connected_components(dcr_graph *g, int32_t *out_labels, int64_t *out_count) {
    if (!g || !out_labels || !out_count) DCR_FAIL(DCR_EINVAL, "null argument");
    DCR_HIP(hipSetDevice(g->device));
    std::vector<int32_t> labels;
    DCR_TRY(graph_components(g, labels));
    int64_t c = 0;
    for (int64_t v = 0; v < g->n; ++v) {
        out_labels[v] = labels[(size_t)v];
        c += labels[(size_t)v] == v;
    }
    *out_count = c;
    return DCR_OK;
}

}  // extern "C"
