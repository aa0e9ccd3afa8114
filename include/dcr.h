/*
 * dcr.h — C ABI of libdcr_hip.so: MI355X (gfx950) Balanced Forman curvature,
 * SDRF rewiring primitives and the GCN sparse aggregation.
 *
 * The reference (jakubbober/discrete-curvature-rewiring) is pure Python and has
 * no FFI of its own; its only native launches are numba kernels taking torch
 * CUDA tensors (curvature/bfc_cuda.py:64,157).  This header is the boundary a
 * maintainer binds with ctypes underneath the reference's Python call surface
 * (see INTEGRATION.md).  Each entry point names the reference code it replaces
 * (file:line into the reference tree).
 *
 * Conventions
 *   - every function returns 0 on success, a negative DCR_E* code on failure;
 *     dcr_last_error() returns a thread-local message for the last failure;
 *   - plain pointers and sizes only; HOST pointers unless the name says _dev;
 *   - the caller owns every buffer it passes in; buffers returned through
 *     `const T**` are library-owned pinned host memory, valid until the next
 *     call on the same handle;
 *   - a dcr_graph handle is not thread-safe; distinct handles are independent;
 *   - all calls are synchronous on return (the library owns one HIP stream
 *     per handle) unless documented otherwise.
 */
#ifndef DCR_H
#define DCR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dcr_graph dcr_graph;

enum {
    DCR_OK = 0,
    DCR_EINVAL = -1,   /* bad argument (self-loop, id out of range, ...)        */
    DCR_ENOMEM = -2,   /* host or device allocation failed                      */
    DCR_EHIP = -3,     /* a HIP runtime call or kernel failed                   */
    DCR_ECAPACITY = -4,/* caller buffer too small / degree beyond kernel limit  */
    DCR_ENOTFOUND = -5,/* edge not present                                      */
    DCR_ESTATE = -6    /* call sequence error (e.g. argext before a pass)       */
};

/* curvature kinds: curvature/bfc_naive.py:7 and curvature/classical_curvatures.py:14-28 */
enum { DCR_CURV_BFC = 0, DCR_CURV_1D = 1, DCR_CURV_AUGMENTED = 2, DCR_CURV_HAANTJES = 3 };

const char *dcr_last_error(void);
int dcr_device_count(int *out);

/* ---- graph container ------------------------------------------------------
 * Replaces the nx.Graph built by torch_geometric.utils.to_networkx(data,
 * to_undirected=True) at rewiring/sdrf_no_cuda.py:20: walks (src[e], dst[e]) in
 * order, keeps pairs with dst <= src, appends each new neighbour at the end of
 * both adjacency rows (insertion order is part of the contract: SURVEY §8 A5).
 * Rows live in HBM as slack-padded int32 arrays in insertion order. */
int dcr_graph_create(int device, int64_t num_nodes, int64_t m_directed, const int64_t *src, const int64_t *dst,
                     dcr_graph **out);
int dcr_graph_destroy(dcr_graph *g);
int dcr_graph_num_nodes(const dcr_graph *g, int64_t *out);
int dcr_graph_num_edges(const dcr_graph *g, int64_t *out_undirected);

/* G.add_edge / G.remove_edge / G.has_edge / G.degree — sdrf_no_cuda.py:35,43,46,51,63 */
int dcr_graph_add_edge(dcr_graph *g, int32_t u, int32_t v);
int dcr_graph_remove_edge(dcr_graph *g, int32_t u, int32_t v);
int dcr_graph_has_edge(dcr_graph *g, int32_t u, int32_t v, int *out);
int dcr_graph_degree(dcr_graph *g, int32_t u, int32_t *out);
/* list(G.neighbors(u)) in insertion order — sdrf_no_cuda.py:29-30 */
int dcr_graph_neighbors(dcr_graph *g, int32_t u, int64_t cap, int32_t *out, int64_t *n_out);

/* G.edges enumeration order — sdrf_no_cuda.py:27,59,61; out_u/out_v sized num_edges */
int dcr_graph_edges(dcr_graph *g, int32_t *out_u, int32_t *out_v);
/* from_networkx(G).edge_index — sdrf_no_cuda.py:68; out is int64 [2][2*num_edges] */
int dcr_graph_export_edge_index(dcr_graph *g, int64_t *out2xM);

/* ---- curvature ------------------------------------------------------------ */
/* One full pass: compute_curvature_graph(G, curv_type), sdrf_no_cuda.py:24
 * (classical_curvatures.py:38-46; 'bfc' = bfc_naive.bfc(G), bfc_naive.py:43-52).
 * Values stay in HBM, keyed by adjacency slot; the stale-read semantics of
 * sdrf_no_cuda.py:57-61 follow from later calls reading that buffer. */
int dcr_curvature_pass(dcr_graph *g, int curv_type);
/* Same result, less work: recompute only the edges whose value can have changed since the previous pass of the same
 * kind, i.e. those with an endpoint in {a,b} ∪ N(a) ∪ N(b) of an edge (a,b) added or removed meanwhile (every edit
 * through this API is tracked).  Falls back to a full pass when there is no complete buffer to build on.  The
 * reference recomputes everything each iteration (sdrf_no_cuda.py:24); this is an optional mode. */
int dcr_curvature_pass_incremental(dcr_graph *g, int curv_type);
/* A pass followed by min(G.edges, key=curvature) — sdrf_no_cuda.py:24 and :27 — with one host synchronisation. */
int dcr_curvature_pass_argmin(dcr_graph *g, int curv_type, int incremental, int32_t *out_u, int32_t *out_v,
                              double *out_val);
/* Copy the last pass out in G.edges order (float64 per undirected edge). */
int dcr_curvature_read(dcr_graph *g, double *out_curv, int32_t *out_u, int32_t *out_v);
/* bfc_edge(G, v1, v2), bfc_naive.py:7-40 / compute_curvature_edge, classical_curvatures.py:6 */
int dcr_curvature_edge(dcr_graph *g, int32_t u, int32_t v, int curv_type, double *out);
/* integer ingredients of bfc_edge: d1,d2,triangles,|sq1|,|sq2|,gamma (diagnostic / tests) */
int dcr_bfc_ingredients(dcr_graph *g, int32_t u, int32_t v, int64_t out6[6]);

/* min(G.edges, key=curv) / max([e for e in G.edges if e != (k,l)], key=curv):
 * first extremum in G.edges order over the buffer of the last pass
 * (sdrf_no_cuda.py:27,59,61).  excl_u < 0 means no exclusion. */
int dcr_argext(dcr_graph *g, int want_max, int32_t excl_u, int32_t excl_v, int32_t *out_u, int32_t *out_v,
               double *out_val);

/* Candidate set and improvements for edge (x, y): sdrf_no_cuda.py:29-46.
 * Candidates are produced in the reference's nested-loop order (duplicates
 * kept) as sorted pairs; improvement[c] = curv(x,y | G + cand[c]) - curv(x,y | G).
 * *n_out is the candidate count; the three arrays are library-owned pinned
 * host buffers (cand arrays are filled only if want_candidates != 0). */
int dcr_improvements(dcr_graph *g, int32_t x, int32_t y, int curv_type, int want_candidates, int64_t *n_out,
                     const double **out_improvement, const int32_t **out_ci, const int32_t **out_cj);
/* first index of the maximum improvement of the last dcr_improvements call
 * (np.argmax, utils/softmax.py:7) and the candidate pair at any index */
int dcr_improvements_argmax(dcr_graph *g, int64_t *out_index);
int dcr_candidate_at(dcr_graph *g, int64_t index, int32_t *out_i, int32_t *out_j);

/* Tail of one SDRF iteration, sdrf_no_cuda.py:51,56-66, fused on the device:
 * add (k,l) if add_k >= 0; then, if do_remove, take the first maximum of the
 * stale buffer (excluding (k,l) when it was added) and remove that edge iff
 * its value > removal_bound.  out_removed = {u, v} or {-1,-1}; out_max_val =
 * the maximum examined. */
int dcr_sdrf_tail(dcr_graph *g, int32_t add_k, int32_t add_l, int do_remove, double removal_bound,
                  int32_t out_removed[2], double *out_max_val);
/* The same with the edge to add given as an index into the candidate list of the last dcr_improvements call (the
 * index np.random.choice returned, sdrf_no_cuda.py:49-51): the pair is looked up on the device, out_added receives it. */
int dcr_sdrf_tail_at(dcr_graph *g, int64_t cand_index, int do_remove, double removal_bound, int32_t out_added[2],
                     int32_t out_removed[2], double *out_max_val);

/* Which implementation ran the last curvature pass: 0 two-hop kernels (csrc/dcr_bfc_h2.hip: full Balanced Forman passes of
 * graphs whose 2-hop neighbourhoods are a small part of the graph — the default there — or always with DCR_PASS=h2 when the
 * graph is created), 2 node-centric kernels (csrc/dcr_bfc_nc.hip: everything else, or DCR_PASS=nc), 1 edge-centric kernels
 * (DCR_PASS=edge); -1 before the first pass.  All three produce the same bits. */
int dcr_pass_engine(dcr_graph *g, int *out);
/* Diagnostics of the last two-hop pass: candidates listed for the triangle kernel by the split class's pool and by class
 * M's, block-class units that took that probe path (their item list overflowed) instead of joining the triangle term
 * themselves, units of class M, units of the split class, units on the retry list.  Zeros after a pass of another engine. */
int dcr_h2_stats(dcr_graph *g, int32_t out[6]);
/* How the last dcr_curvature_pass* call ran the two-hop pass: how many times it was launched (0: another engine; more than 1: a
 * launch found that it needed a stage it was launched without, or larger pools, and was run again), and whether the last of the
 * launches carried the retry stage and the triangle stage (k_h2_triangles).  Both stages are left out until a pass of the graph
 * needs them and go with every pass from then on.  out[3], out[4]: how many of the launches ran k_h2_weight (the node weights
 * were computed from the rows, not kept by the edit kernels) and the stand-alone k_h2_clear (the full head, not the two plan
 * kernels alone). */
int dcr_h2_launch_info(dcr_graph *g, int32_t out[5]);
/* Diagnostic: recomputes the two-hop pass's node weights from the rows and counts the nodes whose kept weight (maintained by the
 * edit kernels since the last pass that computed them) differs.  *mismatches = -1 while no weights are kept (no two-hop pass
 * has run on the graph).  Synchronises; no part of a pass. */
int dcr_h2_weight_check(dcr_graph *g, int64_t *mismatches);
/* The route a pass with these facts and switches takes (csrc/dcr_pass_route.h: plan_pass, the function every pass calls): no
 * handle, no environment, no GPU.  Facts: nodes, undirected edges, adjacency slots, sum of squared degrees, upper bound on the
 * degrees, edits since the last pass.  Switches: pass_impl 0 automatic / 1 edge / 2 nc / 3 h2 (DCR_PASS), fine_on (DCR_NC_FINE),
 * fine_full_set and fine_full_slots (DCR_NC_FINE_FULL), fine_sweep -1 unset / 0 / 1 (DCR_NC_FINE_SWEEP).  *out_route: 0 two-hop,
 * 1 edge-centric, 2 node-centric class kernels, 3 node-centric edge by edge (dcr_pass_engine reports 2 for both);
 * *out_list_by_rows: the edge list of an incremental edge-by-edge pass comes from the flagged nodes' rows, not from a sweep;
 * *out_hub_supplement: the kernels for hubs above the node-centric tables follow; out_ms: the estimates two-hop, class
 * kernels, edge by edge. */
int dcr_pass_plan(int64_t n, int64_t n_edges, int64_t cap_total, double sum_deg2, int32_t max_deg_bound, int pending_edits,
                  int pass_impl, int fine_on, int fine_full_set, int64_t fine_full_slots, int fine_sweep, int curv_type,
                  int incremental, int *out_route, int *out_list_by_rows, int *out_hub_supplement, double out_ms[3]);

/* dcr_sdrf_tail_at followed by dcr_curvature_pass_argmin of the NEXT iteration (sdrf_no_cuda.py:51,56-66 then :24,:27) with
 * one host synchronisation instead of two: the pass is enqueued right behind the edit.  Same results as the two calls. */
int dcr_sdrf_tail_at_pass_argmin(dcr_graph *g, int64_t cand_index, int do_remove, double removal_bound, int curv_type,
                                 int incremental, int32_t out_added[2], int32_t out_removed[2], int32_t *out_u, int32_t *out_v,
                                 double *out_val);

/* One whole loop iteration for finite tau or tau = +inf (then the draw is the first arg-max, utils/softmax.py:5-8) (sdrf_no_cuda.py:29-66 for the edge (x, y) the previous call returned, then :24,:27 of
 * the next iteration) with the improvements staying on the device (two host round trips of the 1 KB result block; no
 * transfer of the improvements, no host arithmetic).  The draw np.random.choice(n, p=softmax(improvements, tau)) (:49-50) runs
 * on the device from `uniform`, the one double the caller has taken from numpy's global stream: the index is the first i whose
 * prefix sum of exp(tau * improvement) exceeds uniform * total, accepted only when that comparison is decided by a margin wider
 * than every rounding difference between numpy's arithmetic and the device's.  *out_status: 0 done (outputs as
 * dcr_sdrf_tail_at_pass_argmin); 1 undecided or not finite, 2 no candidates: nothing was edited, no pass was run (out_u /
 * out_v / out_val untouched), and the caller runs this iteration through dcr_improvements + the host draw instead (after
 * putting the uniform back into the stream). */
int dcr_sdrf_iteration_device_draw(dcr_graph *g, int32_t x, int32_t y, int curv_type, double tau, double uniform, int do_remove,
                                   double removal_bound, int incremental, int *out_status, int64_t *out_n_cand,
                                   int32_t out_added[2], int32_t out_removed[2], int32_t *out_u, int32_t *out_v, double *out_val);

/* Timing hooks for bench.py: accumulated device time (HIP events on the
 * handle's stream) of the curvature-pass kernels since the last reset. */
int dcr_profile_reset(dcr_graph *g);
int dcr_profile_read(dcr_graph *g, double *pass_ms_total, int64_t *pass_count);
/* SURVEY §8(d) algorithmic bytes of one BFC pass on the current graph (both difference sets of every edge charged). */
int dcr_bfc_algorithmic_bytes(dcr_graph *g, double *out_bytes);
/* The same with only the cheaper difference set's rows charged per edge: 4(d_u+d_v) + 4*sum of the row lengths of that
 * side + 8(2 + its size) + 8.  sq1, sq2 and gamma (bfc_naive.py:26-29,36-37) are degree statistics of ONE bipartite
 * graph, so a pass has to read one side only; this is the byte count bench.py's roofline fraction is quoted on. */
int dcr_bfc_algorithmic_bytes_one_sided(dcr_graph *g, double *out_bytes);

/* ---- Monte-Carlo Cheeger estimate: experiment/compute_cheeger.py ------------------------------------------------------
 * For a node subset S and every undirected edge a < b (G.edges of to_networkx(data, to_undirected=True), :55, yields each
 * edge once in that orientation) the reference's cheeger_S (:40-45) is a function of three integers:
 *     in = #{a in S, b in S}     lo = #{a in S, b not in S}     hi = #{a not in S, b in S}     out = E - in - lo - hi
 * boundary_size (:32-37) = lo (only the edges whose SMALLER endpoint is inside), vol(G.subgraph(S)) (:27-29, :60) = 2 in,
 * vol(G - S) (:42-44) = 2 out.  The calls below count many subsets in one sweep of the graph's rows (csrc/dcr_cheeger.hip).
 * Subsets are packed 64 to a word: a membership matrix is node-major uint64 [num_nodes][W], bit k of word w of node v set
 * iff v is a member of subset 64 w + k.  All of them are READ-ONLY on the graph (curvature buffer, incremental flags,
 * edit journal, two-hop edge set and extremum caches untouched), run on the graph's stream and are synchronous on return.
 * Bad arguments (null pointers, W <= 0, B <= 0, first not a non-negative multiple of 64) return DCR_EINVAL before any
 * device call.
 *   dcr_cheeger_counts           members: host [num_nodes][W]; out_counts: host int64 [64 W][3] = (in, lo, hi) per subset
 *                                (the loop body of estimate_cheeger, :59-60, for 64 W draws of random_subset, :19-24)
 *   dcr_cheeger_philox_counts    the same for subsets first .. first + B - 1 of the Philox family of `seed`, drawn on the
 *                                device; out_counts: host int64 [B][3]
 *   dcr_cheeger_philox_values    their ratios, out_values: host double [B].  definition 0: cheeger_S as the reference
 *                                computes it (:40-45), lo / min(2 in, 2 out); 1: conductance, (lo + hi) / min(2 in + lo + hi,
 *                                2 out + lo + hi).  +inf where the smaller volume is 0.  One IEEE float64 division of two
 *                                exactly represented integers.
 *   dcr_cheeger_philox_members   the membership words themselves, words first / 64 .. first / 64 + W - 1: host [num_nodes][W]
 * Philox family: with r[0..3] = Philox-4x32-10 of counter words {v low, v high, (j >> 7) low, (j >> 7) high} under key
 * {seed low, seed high} (the generator of csrc/dcr_philox.h), node v is a member of subset j iff bit (j & 31) of
 * r[(j >> 5) & 3] is set.  Membership probability 1/2; a subset depends on (seed, j) only, not on first or B. */
int dcr_cheeger_counts(dcr_graph *g, const uint64_t *members, int64_t W, int64_t *out_counts);
int dcr_cheeger_philox_counts(dcr_graph *g, uint64_t seed, int64_t first, int64_t B, int64_t *out_counts);
int dcr_cheeger_philox_values(dcr_graph *g, uint64_t seed, int64_t first, int64_t B, int definition, double *out_values);
int dcr_cheeger_philox_members(dcr_graph *g, uint64_t seed, int64_t first, int64_t W, uint64_t *out_members);

/* ---- spectral gap and Cheeger bounds: experiment/cheeger_bounds.py:11-21 ------------------------------------------------
 * The reference brackets the Cheeger constant by lambda_1 / 2 <= h <= sqrt(2 lambda_1), lambda_1 the smallest eigenvalue of
 * the normalised Laplacian L = I - D^-1/2 A D^-1/2 above its null space (:13-19, from a dense eigh).  With c connected
 * components (an isolated node is one; its row of L is zero, as networkx has it) the null space of L has dimension exactly
 * c, so lambda_1 is the (c+1)-th smallest eigenvalue.  The calls below compute c and lambda_1 on the live graph
 * (csrc/dcr_spectral.hip: Lanczos with full reorthogonalisation on I + D^-1/2 A D^-1/2 with the null space deflated in
 * closed form); both are read-only on the graph and leave the curvature buffer alone.  All arithmetic is fp64 and every
 * reduction has a fixed order: the same seed on the same graph returns the same bits.
 *   dcr_connected_components  out_labels: host int32 [num_nodes], the smallest node id of each node's component; out_count: c
 *   dcr_spectral_gap          opts NULL = defaults: tol 1e-10, max_steps 20000, max_basis 0 = min of 256 columns and
 *                             4 GiB / 8 num_nodes, at least 16; seed 0: the start vector is Philox-4x32-10 of counter
 *                             {node, restart} under key seed, csrc/dcr_philox.h.
 *                             out->converged: the TRUE residual |L y - lambda_1 y|_2 of the returned unit vector, recomputed
 *                             with a mat-vec of its own, is <= tol; out->residual is that norm.  steps counts mat-vecs and
 *                             never exceeds max_steps; when they run out the call still returns DCR_OK, with converged = 0
 *                             and the last checked value, which is never below the true lambda_1.
 *                             out_vector, host double [num_nodes] or NULL: that eigenvector of L in node order, the Fiedler
 *                             vector in D^1/2 scaling.
 *                             max_basis 1 is taken as 2 (one column could only restart from itself).  The basis, max_basis
 *                             x num_nodes doubles, is allocated for the call and freed before it returns; O(num_nodes)
 *                             work buffers stay on the handle until dcr_graph_destroy.
 * A graph without edges has no positive eigenvalue: DCR_EINVAL, where the reference raises IndexError.  Null g or out, tol
 * negative or NaN, max_steps < 1, max_basis < 0: DCR_EINVAL. */
typedef struct { double tol; int64_t max_steps; int64_t max_basis; uint64_t seed; } dcr_spectral_opts;
typedef struct { double lambda1, residual; int64_t steps, restarts, components; int converged; } dcr_spectral_result;
int dcr_connected_components(dcr_graph *g, int32_t *out_labels /* host [n] */, int64_t *out_count);
int dcr_spectral_gap(dcr_graph *g, const dcr_spectral_opts *opts /* NULL = defaults */,
                     dcr_spectral_result *out, double *out_vector /* host [n] or NULL */);

/* ---- sweep cut: the constructive half of Cheeger's inequality (csrc/dcr_sweep.hip; no counterpart in the reference) ------
 * The nodes are ordered ascending by (score, node id): -0.0 and +0.0 are the same score, +-inf are ordinary values, i.e.
 * np.lexsort((ids, np.where(score == 0, 0.0, score))).  S_k is the first k nodes of that order, k = 1 .. num_nodes - 1.  With
 * in / lo / hi / out of S_k counted as above (each undirected edge a < b once), the value of S_k is, by `definition`, one of the
 * two ratios of dcr_cheeger_philox_values: 0: lo / min(2 in, 2 out); 1: (lo + hi) / min(2 in + lo + hi, 2 out + lo + hi); +inf
 * where the smaller volume is 0; one IEEE float64 division of exact integers.  The result is the smallest value and, among
 * equal values, the smallest k (numpy's argmin of the profile; k = 1 when every value is +inf).  Sort, counts and arg-min run on
 * the device over the live adjacency (a hand-written stable LSD radix sort on an order-preserving uint64 image of the score,
 * integer difference arrays and prefix sums); the calls are READ-ONLY on the graph as the Cheeger and spectral calls are, run on
 * the graph's stream and are synchronous on return.  Counts are int32 on the device: fewer than 2^31 live adjacency slots.
 * O(num_nodes) work buffers stay on the handle until dcr_graph_destroy.
 *   dcr_sweep_cut      score: host double [num_nodes].  out_order, host int32 [num_nodes] or NULL: the node at each position;
 *                      out_profile, host double [num_nodes - 1] or NULL: the value of S_1 .. S_{n-1}.  A NaN in the score is
 *                      DCR_EINVAL, found on the host before any device call.
 *   dcr_fiedler_sweep  runs the solver of dcr_spectral_gap (same opts, same out_gap bits), keeps the eigenvector y on the
 *                      device, forms the score x = s ⊙ y with the solver's own s = 1 / sqrt(deg) (0 at degree 0) -- the Fiedler
 *                      vector in D^-1/2 scaling -- and sweeps it with no host round trip of the vector.  out_score, host
 *                      double [num_nodes] or NULL: the score that was swept.  With `definition` 1 the result satisfies
 *                      lambda_1 / 2 <= h <= value <= sqrt(2 lambda_1).  A graph without edges: DCR_EINVAL, as dcr_spectral_gap.
 * Null g, out (or out_gap), score; a definition outside {0, 1}; num_nodes < 2: DCR_EINVAL. */
typedef struct { double value; int64_t size, in, lo, hi; } dcr_sweep_result;   /* size = best k */
int dcr_sweep_cut(dcr_graph *g, const double *score /* host [n] */, int definition, dcr_sweep_result *out,
                  int32_t *out_order /* host [n] or NULL */, double *out_profile /* host [n-1] or NULL */);
int dcr_fiedler_sweep(dcr_graph *g, const dcr_spectral_opts *opts, int definition,
                      dcr_spectral_result *out_gap, dcr_sweep_result *out,
                      int32_t *out_order, double *out_score /* host [n] or NULL */);

/* ---- effective resistance of node pairs (csrc/dcr_resistance.hip; no counterpart in the reference) ------------------------
 * R(u, v) = (e_u - e_v)^T L^+ (e_u - e_v), L = D - A the combinatorial Laplacian of the live graph: the commute time between u
 * and v divided by 2 E.  Solved in the normalised operator of the spectral calls: with L' = I - D^-1/2 A D^-1/2 and
 * c = s_u e_u - s_v e_v, s = 1 / sqrt(deg), R = c^T y* where L' y* = c, by conjugate gradients from y = 0 (Jacobi-preconditioned
 * CG on L), 8 or 16 pairs at a time as independent columns of one multi-column mat-vec over the live adjacency.
 *   out_lower     host double [P]: 2 c^T y - y^T L' y for the y the iteration ended with.  For ANY y this is a LOWER bound:
 *                 R - out_lower = (y* - y)^T L' (y* - y) >= 0, also when the solve was cut short by max_steps, and
 *                 R - out_lower <= out_residual^2 / lambda_1, lambda_1 the spectral gap of dcr_spectral_gap (of the whole graph: it
 *                 is the smallest over the components with an edge).  Computed with a mat-vec of its own, not from the recurrences.
 *   out_residual  host double [P]: the true residual |c - L' y|_2 from that same mat-vec.  A pair has converged when it is
 *                 <= tol |c|_2, |c|_2^2 = 1 / deg u + 1 / deg v.
 *   out_steps     host int32 [P] or NULL: CG steps the pair's column took.  A column stops, on the device, in the step where the
 *                 recurrence's |r| <= tol |c|, or where p^T L' p is not a positive finite number.
 * Decided from the connected components before any solve: u == v gives 0 (residual 0, steps 0); u and v in different
 * components, an isolated node included, give +inf (residual 0, steps 0).
 * opts NULL = defaults: tol 1e-10, max_steps 20000.  A pair that ran out of steps is still DCR_OK; its residual says so.
 * All arithmetic is fp64 without floating-point atomics and every reduction has a fixed order in which the columns of a batch
 * do not meet: a pair's three outputs are the same bits whatever else is in the call and wherever in it the pair stands.
 * READ-ONLY on the graph as the Cheeger and spectral calls are, runs on the graph's stream and is synchronous on return; work
 * buffers of O(16 num_nodes) doubles stay on the handle until dcr_graph_destroy.
 * Null g, u, v, out_lower or out_residual; P < 0; an endpoint outside 0 .. num_nodes - 1; tol negative or NaN; max_steps < 1:
 * DCR_EINVAL before any device call.  P == 0: DCR_OK, nothing written. */
typedef struct { double tol; int64_t max_steps; } dcr_resistance_opts;
int dcr_effective_resistance(dcr_graph *g, const int32_t *u, const int32_t *v, int64_t P,
                             const dcr_resistance_opts *opts /* NULL = defaults */,
                             double *out_lower /* host [P] */, double *out_residual /* host [P] */,
                             int32_t *out_steps /* host [P] or NULL */);

/* ---- sketched effective resistance of every edge (csrc/dcr_resistance_sketch.hip; no counterpart in the reference) -----------
 * With B the incidence matrix of the live graph, an edge oriented from its smaller to its larger endpoint, R(u, v) =
 * |B L^+ (e_u - e_v)|^2.  For k = opts.columns sign vectors q_j in {-1, +1}^E (Spielman and Srivastava, with Rademacher signs):
 *     b_j = B^T q_j,  b_j[w] = sum over the neighbours x of w of q_j({w, x}) (w < x ? +1 : -1),      L z_j = b_j,
 *     R~(u, v) = 1/k sum_j (z_j[u] - z_j[v])^2.
 * R~ is unbiased with Var R~(u, v) <= 2 R(u, v)^2 / k, so its relative standard deviation is at most sqrt(2 / k) for every pair at
 * once; the sum over the edges has mean n - c and variance <= 2 (n - c) / k, c the connected components; on a bridge R~ = 1 for
 * any signs.  One set of k solves serves every edge and every pair: 16 columns a batch in the column CG of
 * dcr_effective_resistance, on L' y_j = s ⊙ b_j with z_j = s ⊙ y_j, from y = 0.
 * Signs: the sign of edge {lo, hi}, lo < hi, in column 16 b + i is bit i of output word 0 of Philox-4x32-10 with counter
 * {lo, hi, b low, 0x52530000 | b high} and key {seed low, seed high}; a bit of 0 means +1.  Keyed by the endpoints: the signs
 * of an edge do not depend on the order of the rows or on edits elsewhere in the graph.
 *   out_edge      host double [num_edges] or NULL: R~ of every edge in the order of dcr_graph_edges.  Without it no per-slot
 *                 buffer exists.
 *   u, v, out_pair   P pairs and host double [P], or NULL with P = 0: R~ of each pair; 0 for u == v and +inf across components
 *                 (an isolated node included), both decided from the connected components.
 *   out_residual  host double [columns] or NULL: the true residual |s ⊙ b_j - L' y_j|_2 of each column from a mat-vec of its own
 *                 at the end of its batch.  The error a column's solve leaves in sqrt(R~) is at most residual_j / sqrt(lambda_1).
 *   out_info      or NULL: columns; batches of 16 that ran; steps_total, the CG steps of all columns; residual_max.
 * A column stops in the step where the recurrence's |r| <= tol |s ⊙ b_j|, or where p^T L' p is not a positive finite number; an
 * all-zero b_j takes no step.  opts NULL = defaults: columns 256, seed 0, tol 1e-6 (the solve error only has to sit well below
 * the sketch's own sqrt(2 / k)), max_steps 20000.  columns need not be a multiple of 16: the padding columns of the last batch
 * are zero and add nothing.  A column that ran out of steps is still DCR_OK; its residual says so.
 * All arithmetic is fp64 without floating-point atomics and every sum has an order that the graph and the call fix: a column's
 * residual depends on (seed, j) and the graph alone, and two calls return the same bits.
 * READ-ONLY on the graph, runs on the graph's stream and is synchronous on return; work buffers of 768 bytes per node and group
 * of a launch (at most 4 groups, and 1 above 65,536 nodes), and 8 bytes per adjacency slot where out_edge is given, stay on the
 * handle until dcr_graph_destroy.  The k x n matrix Z is never stored.
 * Null g; columns < 1; tol negative or NaN; max_steps < 1; P < 0; P > 0 with a null u, v or out_pair; an endpoint outside
 * 0 .. num_nodes - 1: DCR_EINVAL before any device call.
 *   dcr_resistance_sketch_rhs   for the tests: the integers b_j[w] of the 16 columns of batch `batch`, host double [num_nodes][16]. */
typedef struct { int32_t columns; uint64_t seed; double tol; int64_t max_steps; } dcr_sketch_opts;   /* NULL: 256, 0, 1e-6, 20000 */
typedef struct { int32_t columns, batches; int64_t steps_total; double residual_max; } dcr_sketch_info;
int dcr_resistance_sketch(dcr_graph *g, const dcr_sketch_opts *opts,
                          double *out_edge /* host [n_edges], G.edges() order, or NULL */,
                          const int32_t *u, const int32_t *v, int64_t P, double *out_pair /* host [P], or NULL with P = 0 */,
                          double *out_residual /* host [columns] true residual per column, or NULL */, dcr_sketch_info *out_info);
int dcr_resistance_sketch_rhs(dcr_graph *g, uint64_t seed, int64_t batch, double *out /* host [n][16], the integer b */);

/* ---- PageRank diffusion rewiring, DIGL / GDC (csrc/dcr_diffusion.hip) -------------------------------------------------------
 * With A~ = A + I, d~ = deg + 1, H = D~^-1/2 A~ D~^-1/2 of the live graph and 0 < alpha < 1:  M = I - (1 - alpha) H, symmetric
 * positive definite with spectrum in [alpha, 2 - alpha], and S = alpha M^-1, the personalised-PageRank matrix.  Column j of S
 * solves M x = alpha e_j; S_jj = 1 at an isolated node.  The reference never builds S; utils/adjacency_matrix_ops.py:26-39 holds
 * the two sparsifiers written for it (get_top_k_matrix, get_clipped_matrix) on dense N x N arrays, restated here per column.
 * Columns are solved 16 at a time as independent conjugate-gradient iterations from x = 0 in one multi-column mat-vec.
 *   dcr_ppr_columns         out: host double [P][num_nodes], row i = column sources[i] of S.
 *   dcr_diffusion_sparsify  per column, mode 0: the k largest entries (all of them where k >= num_nodes); larger value first,
 *                           among equal bits the smaller node id first.  mode 1: the entries >= eps.  sources NULL stands for all
 *                           nodes in order, and P must then be num_nodes.  The output is grouped by column in the order of
 *                           `sources`, within a column by node id ascending:
 *                             out_ptr     host int64 [P + 1], column i holds entries out_ptr[i] .. out_ptr[i + 1] - 1
 *                             out_row     host int32 [cap], the node ids
 *                             out_value   host double [cap], the raw S_ij
 *                             out_weight  host double [cap], out_value divided by the sum of the column's kept values, the sum
 *                                         added in node-id order (divided by 1 where that sum is not positive, as the reference
 *                                         does).  A column with nothing kept has no entries.
 *                             out_nnz     the number of entries of all columns
 *                           When cap is smaller than that number the call returns DCR_ECAPACITY with *out_nnz set to the number
 *                           needed and out_ptr complete; out_row, out_weight and out_value then hold nothing of use (they may be
 *                           NULL when cap is 0: a counting call).  In mode 0 the number is P min(k, num_nodes) and the call
 *                           returns before any solve; in mode 1 every column is solved to be counted.
 *   out_residual  host double [P]: the true residual |alpha e_j - M x|_2 of the returned column, from a mat-vec of its own.  A
 *                 column has converged when it is <= tol alpha.  |x_i - S_ij| <= out_residual / alpha for every i.
 *   out_steps     host int32 [P] or NULL: CG steps of the column.  A column stops, on the device, in the step where the
 *                 recurrence's |r| <= tol alpha, or where p^T M p is not a positive finite number.
 * opts NULL = defaults: alpha 0.15, tol 1e-10, max_steps 20000.  A column that ran out of steps is still DCR_OK.
 * All arithmetic is fp64 without floating-point atomics and every reduction has a fixed order in which the columns of a batch
 * do not meet: a column's outputs are the same bits whatever else is in the call and wherever in it the source stands.
 * READ-ONLY on the graph, runs on the graph's stream and is synchronous on return; O(16 num_nodes) doubles of work buffers
 * and the entries one batch keeps stay on the handle until dcr_graph_destroy.  No num_nodes x num_nodes buffer exists.
 * Null g, out, out_ptr, out_residual, out_nnz (sources too in dcr_ppr_columns); P < 0; a source outside 0 .. num_nodes - 1;
 * alpha outside (0, 1); tol negative or NaN; max_steps < 1; a mode outside {0, 1}; k < 1 in mode 0; eps NaN in mode 1; cap < 0, or
 * cap > 0 with a NULL entry array: DCR_EINVAL before any device call.  P == 0: DCR_OK, nothing written. */
typedef struct { double alpha, tol; int64_t max_steps; } dcr_diffusion_opts;
int dcr_ppr_columns(dcr_graph *g, const int32_t *sources, int64_t P, const dcr_diffusion_opts *opts /* NULL = defaults */,
                    double *out /* host [P][n] */, double *out_residual /* host [P] */, int32_t *out_steps /* host [P] or NULL */);
int dcr_diffusion_sparsify(dcr_graph *g, const int32_t *sources /* NULL = all nodes */, int64_t P,
                           const dcr_diffusion_opts *opts /* NULL = defaults */, int mode /* 0 top-k, 1 threshold */, int64_t k,
                           double eps, int64_t *out_ptr /* host [P + 1] */, int64_t cap, int32_t *out_row, double *out_weight,
                           double *out_value, double *out_residual /* host [P] */, int32_t *out_steps /* host [P] or NULL */,
                           int64_t *out_nnz);

/* ---- Heat-kernel diffusion, GDC's other kernel (csrc/dcr_diffusion.hip; upstream's get_heat_matrix, which the reference did not
 * take over) ---------------------------------------------------------------------------------------------------------------------
 * With A~, d~ = deg + 1, s~ = 1 / sqrt(d~), r = sqrt(d~) and H = D~^-1/2 A~ D~^-1/2 of the live graph as above, and 0 < t <= 256:
 * S = exp(-t (I - H)) = sum_k theta_k H^k with theta_k = e^-t t^k / k!.  Column j is computed as the partial sum
 * x = sum_{k = 0 .. K} theta_k H^k e_j by the recurrence
 *   v_0 = e^-t e_j;   v_{k+1} = (t / (k + 1)) s~ ⊙ ((A + I)(s~ ⊙ v_k));   x += v_{k+1}
 * 16 columns at a time, one launch a term.  K is chosen on the host before any launch: the smallest K whose tail
 * rho_K = sum_{k > K} theta_k, added term by term, is <= tol / 2; or max_terms where that is lower: the call is then still DCR_OK
 * and the deficit says that the sum was cut short.  Nothing on the device decides when to stop and the host reads nothing back
 * between terms.  An isolated node has H_jj = 1 and S_jj = 1.
 * Every term is non-negative, so nothing cancels and x <= S_j entrywise; H r = r, so the mass that x lacks is known exactly:
 *   out_deficit  host double [P]: r_j - sum_i r_i x_i, in exact arithmetic r_j rho_K >= 0.  0 <= S_ij - x_i <= out_deficit / r_i
 *                for every i.  A column has converged when it is <= tol r_j.
 *   out_terms    one host int64 or NULL: K, the same for every column of the call.
 *   dcr_heat_columns   out: host double [P][num_nodes], row i = the partial sum of column sources[i] of S.
 *   dcr_heat_sparsify  the selection of dcr_diffusion_sparsify on these columns: mode, k, eps, out_ptr, cap, out_row, out_weight,
 *                      out_value, out_nnz, DCR_ECAPACITY and the counting call are as stated there.
 * opts NULL = defaults: t 5.0, tol 1e-10, max_terms 4096.  fp64 without floating-point atomics, every sum in an order the graph
 * alone fixes: the bits of a column depend on its source, t and K only, not on its place in the call, on the other columns or on
 * how many batches share a launch.  READ-ONLY on the graph, on the graph's stream, synchronous on return; the work buffers are
 * those of the PageRank solve.
 * Null g, out, out_ptr, out_deficit, out_nnz (sources too in dcr_heat_columns); t outside (0, 256] or NaN; tol negative or NaN;
 * max_terms < 1; and what dcr_diffusion_sparsify rejects in P, sources, mode, k, eps and cap: DCR_EINVAL before any device call.
 * P == 0: DCR_OK, nothing written. */
typedef struct { double t, tol; int64_t max_terms; } dcr_heat_opts;
int dcr_heat_columns(dcr_graph *g, const int32_t *sources, int64_t P, const dcr_heat_opts *opts /* NULL = defaults */,
                     double *out /* host [P][n] */, double *out_deficit /* host [P] */, int64_t *out_terms /* one, or NULL */);
int dcr_heat_sparsify(dcr_graph *g, const int32_t *sources /* NULL = all nodes */, int64_t P,
                      const dcr_heat_opts *opts /* NULL = defaults */, int mode /* 0 top-k, 1 threshold */, int64_t k, double eps,
                      int64_t *out_ptr /* host [P + 1] */, int64_t cap, int32_t *out_row, double *out_weight, double *out_value,
                      double *out_deficit /* host [P] */, int64_t *out_terms /* one, or NULL */, int64_t *out_nnz);

/* ---- FoSR, first-order spectral rewiring (csrc/dcr_fosr.hip; Karhadkar, Banerjee, Montufar, ICLR 2023; no counterpart in the
 * reference) ------------------------------------------------------------------------------------------------------------------
 * Adds, one at a time, the edge that raises the spectral gap most to first order.  With deg the current degrees, r = sqrt(deg),
 * vol = sum deg and s = 1 / sqrt(deg) (0 at degree 0):
 *   power step on x:   x <- x - (x . r / vol) r;   z <- x + s ⊙ A (s ⊙ x);   x <- z / |z|_2
 *                      All fp64, no floating-point atomics, every reduction in a fixed order: the same input gives the same bits.
 *                      Where |z| is 0 or not finite the loop stops there: x stays the iterate before that step, the call is still
 *                      DCR_OK and reports the edges added so far.
 *   pick on x:         y_i = x_i / sqrt(deg_i + 1).  The nodes are ordered as the sweep cut orders them: ascending by (y, node id),
 *                      -0.0 equal to +0.0 (np.lexsort((ids, np.where(y == 0, 0.0, y)))).  For a node u the eligible nodes are those
 *                      that are neither u nor adjacent to u; partner(u) is the LAST eligible node of the order where y_u < 0 and
 *                      the FIRST one otherwise (zero included); none where nothing is eligible.  p(u) = fl(y_u y_partner(u)).  The
 *                      pick is the u with the smallest p(u), among equal values (-0.0 == 0.0) the smallest u, as (u, partner(u)).
 *                      Rounded multiplication is monotone, so p is the exact minimum of fl(y_u y_v) over all non-adjacent pairs
 *                      u != v.  It is found in O(n log n + E): partner(u) has rank below deg_u + 2 from its end of the order, a
 *                      bitmap of that many bits per row; no num_nodes x num_nodes array exists.  (A product 0 x inf is NaN and no
 *                      candidate.)
 *   loop:              initial_power_iters power steps; then num_iterations times: pick, add the edge, one power step with the
 *                      new degrees.  A disconnected graph needs no special case: after the projection the iterate has both
 *                      signs, components are joined first.
 * One deliberate difference from the published code: that code zeroes the products of existing edges and of the diagonal and
 * takes the arg-min of the dense outer product, so when every free product is positive it re-adds an existing edge or adds a
 * self-loop.  Here only free pairs are candidates; a graph without a free pair gives "none" and the loop stops.
 *   dcr_fosr_pick  x: host double [num_nodes].  *out_found 0: no free pair (out_u = out_v = -1, out_product 0).  out_y, host
 *                  double [num_nodes] or NULL: the y that was ordered.  READ-ONLY on the graph as the sweep is.  A NaN in x is
 *                  DCR_EINVAL, found on the host.
 *   dcr_fosr       x0: host double [num_nodes], or NULL: x0_v = ((53 bits) + 1/2) 2^-52 - 1, uniform in (-1, 1), the 53 bits being
 *                  ((r[0] | r[1] << 32) >> 11) of Philox-4x32-10 with counter {v, 0} under key seed (csrc/dcr_philox.h), the
 *                  construction of the spectral solver's start vector, on every node.  out_u / out_v: host int32
 *                  [num_iterations], the added edges in order, *out_added of them; out_x, host double [num_nodes] or NULL: the
 *                  final iterate.  MUTATES the graph: every edge goes through dcr_graph_add_edge, so the incremental flags, the
 *                  edit journal and the caches behave as for any added edge.  The pick comes back to the host once per iteration
 *                  (one 56-byte block).  A graph without edges, or a NaN in x0: DCR_EINVAL.
 * Both run on the graph's stream and are synchronous on return; O(num_nodes) work buffers stay on the handle until
 * dcr_graph_destroy.  Null g, opts, x or a null output other than out_y / out_x (out_u / out_v may be NULL where num_iterations is
 * 0); a negative count; num_nodes < 2: DCR_EINVAL before any device call. */
typedef struct { int64_t num_iterations, initial_power_iters; uint64_t seed; } dcr_fosr_opts;
int dcr_fosr_pick(dcr_graph *g, const double *x /* host [n] */, int32_t *out_u, int32_t *out_v, double *out_product,
                  double *out_y /* host [n] or NULL */, int *out_found);
int dcr_fosr(dcr_graph *g, const dcr_fosr_opts *opts, const double *x0 /* host [n] or NULL */, int32_t *out_u,
             int32_t *out_v /* host [num_iterations] */, int64_t *out_added, double *out_x /* host [n] or NULL */);

/* ---- hop distances, eccentricities and ball sizes (csrc/dcr_hops.hip; no counterpart in the reference) ----------------------
 * d(s, v) is the number of edges of a shortest path from s to v in the live graph, unweighted and undirected: d(s, s) = 0, and
 * level L = 1, 2, ... holds the nodes that have a neighbour at level L - 1 and are in no earlier level.  With a hop limit H
 * (max_hops >= 0) the levels stop at H.  Per source s, over the nodes its levels hold (s itself included, at distance 0):
 *   out_dist     host int32 [P][num_nodes] or NULL: row i holds d(sources[i], v); -1 where v was not reached (another
 *                component, or beyond max_hops).  Without it no distance row exists anywhere.
 *   out_ecc      host int32 [P] or NULL: the largest distance reached, the last level that holds a node.  0 for an isolated source.
 *   out_reached  host int64 [P] or NULL: the nodes at distance <= max_hops, the source included: the ball size |B_H(s)|; the size
 *                of the source's component where there is no limit.
 *   out_total    host int64 [P] or NULL: the sum of the distances of those nodes.
 * An isolated source gives ecc 0, reached 1, total 0, and so does every source at max_hops = 0.
 * Breadth-first search from 64 W sources at a time (W = 1, 2 or 4: the narrowest that holds what is left of the call, so a call
 * of up to 64 sources runs at W = 1 and a long one 256 sources a sweep): every node carries one bit per
 * source in W 64-bit words, one sweep of the live adjacency advances every source of the batch by one hop, and the host reads
 * the 64 W per-source counts once per level and stops when all are zero.  Duplicated sources are legal, each is a source of its
 * own.  sources NULL stands for every node in order, and P must then be num_nodes.  All arithmetic is integer: a source's outputs
 * are the same bits whatever else is in the call and wherever in it the source stands.
 * READ-ONLY on the graph, runs on the graph's stream and is synchronous on return; 24 W num_nodes bytes of work buffers, and
 * 256 W num_nodes more where out_dist is given, stay on the handle until dcr_graph_destroy.  No num_nodes x num_nodes buffer
 * exists on the device.
 * Null g; P < 0; sources NULL with P != num_nodes; a source outside 0 .. num_nodes - 1: DCR_EINVAL before any device call.
 * P == 0: DCR_OK, nothing written.  More levels than nodes (a corrupted graph): DCR_ESTATE. */
typedef struct { int32_t max_hops; /* < 0: no limit */ } dcr_hops_opts;
int dcr_hop_distances(dcr_graph *g, const int32_t *sources /* NULL = every node, P must then be n */, int64_t P,
                      const dcr_hops_opts *opts /* NULL = no limit */,
                      int32_t *out_dist    /* host [P][n] or NULL; -1 = not reached (other component, or beyond max_hops) */,
                      int32_t *out_ecc     /* host [P]: largest distance reached */,
                      int64_t *out_reached /* host [P]: nodes at distance <= max_hops, the source included */,
                      int64_t *out_total   /* host [P]: sum of the distances of those nodes */);

/* ---- node and edge betweenness centrality (csrc/dcr_betweenness.hip; no counterpart in the reference) ------------------------
 * For a source s, sigma_s(v) is the number of shortest paths from s to v in the live graph (unweighted, undirected; distances as in
 * the hop-distance section above), and the dependency of s is, from the deepest level upwards,
 *     delta_s(v)    = sum over the neighbours w of v one level further from s of  sigma_s(v) / sigma_s(w) (1 + delta_s(w)),
 *     delta_s(v, w) = sigma_s(v) / sigma_s(w) (1 + delta_s(w))   for such an edge, 0 for every other edge
 * (Brandes 2001).  The values are the RAW sums over the given sources:
 *   out_node  host double [num_nodes]: sum over s in sources of delta_s(v), the term s == v left out: endpoints are not counted.
 *   out_edge  host double [num_edges] or NULL: sum over s in sources of delta_s(u, v) + delta_s(v, u), in the order and orientation
 *             of dcr_graph_edges.  Without it no per-slot buffer exists.
 * With every node a source this is the ORDERED-pair convention, every pair (s, t) and (t, s) counted: twice the unnormalised value
 * networkx gives for an undirected graph.  A duplicated source counts as often as it is given.  Nodes in other components than the
 * source contribute nothing and receive nothing; an isolated node and a graph without edges give zeros.
 *   out_info  or NULL: levels_max, the largest eccentricity of a source; batches, the batches of 16 sources that ran; sigma_max,
 *             the largest path count met.  sigma is float64: sigma_max > 2^53 means that path counts were ROUNDED (the values then
 *             carry that rounding, relative 2^-53 per addition, and stay finite and non-negative).  A path count beyond the float64
 *             range is DCR_ESTATE with a message: no NaN or infinity is ever returned, and the handle stays usable.
 * 16 sources a batch, a column each, in node-major int32 / float64 [num_nodes][16] arrays; one sweep of the adjacency per level
 * forward (the host reads one count per level and stops at zero) and one per level backward, so about 2 (levels) sweeps a batch.
 * Every sum has an order that the graph and the call fix, no floating-point atomic is used: two calls on the same graph return
 * the same bits.  Relative error of a value: at most (2 D (maxdeg + 3) + P) 2^-53, D = levels_max + 1, all summands non-negative.
 * READ-ONLY on the graph, runs on the graph's stream and is synchronous on return; 328 num_nodes bytes of work buffers, and 8 bytes
 * per adjacency slot more where out_edge is given, stay on the handle until dcr_graph_destroy.  No num_nodes x num_nodes buffer
 * exists on the device.
 * Null g or out_node; P < 0; sources NULL with P != num_nodes; a source outside 0 .. num_nodes - 1: DCR_EINVAL before any device
 * call.  P == 0: DCR_OK, zeros.  More levels than nodes (a corrupted graph): DCR_ESTATE. */
typedef struct { int32_t levels_max; int32_t batches; double sigma_max; } dcr_betweenness_info;
int dcr_betweenness(dcr_graph *g, const int32_t *sources /* NULL = every node, P must then be n */, int64_t P,
                    double *out_node /* host [n] */, double *out_edge /* host [E] or NULL */,
                    dcr_betweenness_info *out_info /* or NULL */);

/* ---- dense float32 Balanced Forman curvature: the numerics of the reference's numba path (device pointers, caller's
 * stream).  curvature/bfc_cuda.py computes a different number from curvature/bfc_naive.py (float32 dense formula, other
 * 4-cycle term, no degree-1 rule) and it is what rewire('bfc') runs in the reference (rewiring/rewire.py:8-10), so results
 * obtained with the reference can only be reproduced with these.  A, A2 = A·A, C: row-major N x N float32; d_in / d_out:
 * column / row sums of A; pairs: the (i, j) of the non-zero entries of A as int64 [nnz][2] (C must be zero elsewhere:
 * the caller clears it).  Float64 closing expression rounded to float32 twice, as numba types the kernel.
 *   dcr_bfc_dense_f32_dev              replaces _balanced_forman_curvature   (curvature/bfc_cuda.py:11-48, launch :64)
 *   dcr_bfc_dense_post_delta_f32_dev   replaces _balanced_forman_post_delta  (curvature/bfc_cuda.py:68-141, launch :157):
 *       D[I][J] = curvature of (x, y) once (i_neighbors[I], j_neighbors[J]) is added; -1000 where the two are equal or
 *       already adjacent (:77-79); d_in_x = A[:, x].sum(), d_out_y = A[y].sum() (:147-148). */
int dcr_bfc_dense_f32_dev(const float *A_dev, const float *A2_dev, const float *d_in_dev, const float *d_out_dev, int64_t N,
                          const int64_t *pairs_dev, int64_t nnz, float *C_dev, void *hip_stream);
int dcr_bfc_dense_post_delta_f32_dev(const float *A_dev, const float *A2_dev, float d_in_x, float d_out_y, int64_t N,
                                     float *D_dev, int32_t x, int32_t y, const int32_t *i_neighbors_dev,
                                     const int32_t *j_neighbors_dev, int64_t dim_i, int64_t dim_j, void *hip_stream);

/* ---- host helper for np.random.choice(n, p=softmax(a, tau)) — sdrf_no_cuda.py:49-50, utils/softmax.py:9-10
 * Given e = exp(a * tau) and its sum S (both computed by the caller's numpy: their rounding is part of the bit-exact
 * contract), fill cdf[i] = the SEQUENTIAL float64 running sum of p_i = e_i / S, i.e. numpy.cumsum(e / S), in one fused
 * pass with numpy's operations in numpy's order, and return cdf[n-1].  The caller validates the total, draws ONE uniform
 * from the legacy stream and bisects cdf / total exactly as RandomState.choice does.  Plain host code, no GPU. */
int dcr_host_cdf_from_exp(const double *e, int64_t n, double S, double *out_cdf, double *out_total);
/* The same through the plain sequential loop only.  dcr_host_cdf_from_exp evaluates the recurrence eight elements at a
 * time in integer-valued float64 arithmetic where that is exact (csrc/dcr_host_draw.cpp) and falls back to this loop
 * elsewhere; the two must agree bit for bit (tests/test_host_cpu.py). */
int dcr_host_cdf_from_exp_plain(const double *e, int64_t n, double S, double *out_cdf, double *out_total);

/* ---- GCN aggregation (csrc/dcr_spmm.hip; device pointers, caller's stream) ---
 * Replaces the propagate/scatter step of torch_geometric GCNConv (third-party,
 * call site models/gcn.py:36): C[i,:] = (bias ? bias : 0) + sum_e val[e] * B[col[e],:]
 * over CSR row i, optionally followed by ReLU.  fp32, row-major; ldb/ldc in
 * elements.  Rows are accumulated with fused multiply-adds in CSR order (rows
 * above 96 non-zeros: in a fixed strided order), so the result is deterministic
 * for a given CSR.  Asynchronous on hip_stream. */
int dcr_spmm_csr_f32_dev(const int64_t *rowptr_dev, const int32_t *col_dev, const float *val_dev,
                         const float *B_dev, float *C_dev, int64_t n_rows, int64_t n_feat, int64_t ldb, int64_t ldc,
                         const float *bias_dev, int relu, void *hip_stream);

/* Two operands in one sweep of the indices: B = [B0 | B1] and C = [C0 | C1] hold two blocks of n_feat columns side by
 * side (ldb, ldc >= 2 * n_feat); C0 = Â·B0 + bias, C1 = Â·B1 + bias, every block accumulated with the operations and in
 * the order of a dcr_spmm_csr_f32_dev call of its own (bit-identical to two calls).  The training forward of one epoch and
 * the validation forward of the previous one see the same weights, so their aggregations (models/gcn.py:36, called from
 * experiment/training_loop.py:50 and :67) share one pass over the graph: the gathers are bound by the number of row
 * requests, and a 128-byte request costs what a 64-byte one does. */
int dcr_spmm_csr_f32_pair_dev(const int64_t *rowptr_dev, const int32_t *col_dev, const float *val_dev, const float *B_dev,
                              float *C_dev, int64_t n_rows, int64_t n_feat, int64_t ldb, int64_t ldc, const float *bias_dev,
                              int relu, void *hip_stream);
/* the same with the two output blocks in matrices of their own (C1 - C0 a multiple of 4 floats; ldc the row stride of both) */
int dcr_spmm_csr_f32_pair_split_dev(const int64_t *rowptr_dev, const int32_t *col_dev, const float *val_dev, const float *B_dev,
                                    float *C0_dev, float *C1_dev, int64_t n_rows, int64_t n_feat, int64_t ldb, int64_t ldc,
                                    const float *bias_dev, int relu, void *hip_stream);
/* Only the rows rows_dev[0..n_sel) of the product: C[k,:] = row rows_dev[k] of Â·B (+ bias), each accumulated exactly as
 * dcr_spmm_csr_f32_dev accumulates it.  The reference indexes the model's output with the split masks and reads nothing else
 * (experiment/training_loop.py:50-51 log_probs[train_mask]; :64-71 log_probs[mask] of the evaluated split): the last layer's
 * aggregation (models/gcn.py:36) is evaluated at those rows. */
int dcr_spmm_csr_rows_f32_dev(const int64_t *rowptr_dev, const int32_t *col_dev, const float *val_dev, const int64_t *rows_dev,
                              int64_t n_sel, const float *B_dev, float *C_dev, int64_t n_feat, int64_t ldb, int64_t ldc,
                              const float *bias_dev, int relu, void *hip_stream);
/* Two row lists over two column blocks of one operand in one launch: output rows [0, n_first) = rows rows_dev[k] of Â·B0,
 * rows [n_first, n_sel) = rows rows_dev[k] of Â·B1, B1 = B0 + b_off2 floats (the training rows of Â·Z_train and the validation
 * rows of Â·Z_eval of one epoch, Z = [Z_train | Z_eval]: experiment/training_loop.py:50-51 and :64-71 on the same weights). */
int dcr_spmm_csr_rows2_f32_dev(const int64_t *rowptr_dev, const int32_t *col_dev, const float *val_dev, const int64_t *rows_dev,
                               int64_t n_first, int64_t n_sel, const float *B_dev, int64_t b_off2, float *C_dev, int64_t n_feat,
                               int64_t ldb, int64_t ldc, const float *bias_dev, int relu, void *hip_stream);

/* ---- R-GCN typed aggregation (csrc/dcr_spmm.hip; device pointers, caller's stream)
 * The mean-per-relation layer of Schlichtkrull et al. eq. 2 with c_{i,r} = |N_r(i)| (torch_geometric's RGCNConv with
 * aggr='mean'; models/rgcn.py), evaluated transform-first: one GEMM forms Zall = X·[W_0 | ... | W_{R-1} | W_root], one
 * sweep of a typed CSR forms the output.  Typed CSR: rowptr int64, col int32, val float32 (1 / |N_r(i)|) and rel uint8,
 * one entry per slot.  PRECONDITION: inside every row the slots are sorted by relation (stably within a relation) and
 * every rel[e] < n_rel; both kernels rely on it (a larger rel[e] is read as n_rel - 1: wrong sums, no stray access).
 * 1 <= n_rel <= 8; that and every argument error dcr_spmm_csr_f32_dev rejects (null pointers, n_rows < 0, n_feat <= 0,
 * a leading dimension below its row) return DCR_EINVAL without a launch.  fp32, row-major, leading dimensions in
 * elements.  Every output element is accumulated with fused multiply-adds over the slots that feed it in CSR order; a
 * row above 96 slots in the fixed strided order of dcr_spmm_csr_f32_dev, partial sums added in group order.  No
 * floating-point atomics: the same bits on every run for a given CSR.  Asynchronous on hip_stream.
 *
 * The gather (forward), rows = targets:
 *   C[i,:] = sum_e val[e] * B[col[e], rel[e]*n_feat + :]  (+ B[i, n_rel*n_feat + :] with self_block)  (+ bias)  (ReLU)
 * the slot sum first, then the row's own block, then the bias, one rounding each.  ldb >= (n_rel + self_block) * n_feat,
 * ldc >= n_feat; with self_block B has a row for every output row.  With n_rel = 1 and self_block = 0 the result is
 * dcr_spmm_csr_f32_dev's on the same CSR, bit for bit. */
int dcr_spmm_csr_typed_f32_dev(const int64_t *rowptr_dev, const int32_t *col_dev, const float *val_dev, const uint8_t *rel_dev,
                               const float *B_dev, float *C_dev, int64_t n_rows, int64_t n_feat, int64_t n_rel, int64_t ldb,
                               int64_t ldc, int self_block, const float *bias_dev, int relu, void *hip_stream);
/* The expand (backward), run on the typed CSR of the TRANSPOSED pattern (rows = sources, the same val and rel per edge,
 * slots again sorted by relation):
 *   C[j, r*n_feat + :]     = sum_{e in row j, rel[e] = r} val[e] * G[col[e], :]        for every r in [0, n_rel)
 *   C[j, n_rel*n_feat + :] = G[j, :]                                                    with self_block
 * Every element of the (n_rel + self_block) * n_feat columns of C is written (zeros where row j has no slot of r), so the
 * gradient of Zall is complete after one launch and needs no memset.  ldg >= n_feat, ldc >= (n_rel + self_block) * n_feat;
 * with self_block G has a row for every output row. */
int dcr_spmm_csr_typed_expand_f32_dev(const int64_t *rowptr_dev, const int32_t *col_dev, const float *val_dev,
                                      const uint8_t *rel_dev, const float *G_dev, float *C_dev, int64_t n_rows, int64_t n_feat,
                                      int64_t n_rel, int64_t ldg, int64_t ldc, int self_block, void *hip_stream);

/* ---- GAT attention aggregation (csrc/dcr_gat.hip; device pointers, caller's stream)
 * The layer of Velickovic et al. as torch_geometric's GATConv evaluates it (models/gat.py), H heads of C channels, flow
 * source -> target, on Z = X*W [n, H*C] and the scores s_src[j,h] = <Z[j,h,:], att_src[h,:]>, s_dst likewise:
 *   pre = s_src[j,h] + s_dst[i,h]     e = pre > 0 ? pre : negative_slope * pre
 *   w = expf(e - m[i,h])              m = max of e, den = sum of w over the slots of row i
 *   O[i,h,:] = (sum_slots w * Z[col,h,:]) / den[i,h]
 * CSR by target: rowptr int64 [n + 1], col int32 (sources; every value in [0, n)).  A duplicated column is two slots; a row
 * without slots gives O = 0 and the record (0, 1).  fp32, row-major, leading dimensions in elements: ldz for Z and dZ
 * (>= H*C), lds for s_src, s_dst, dS_src and dS_dst (>= H), ldo for O and dO (>= H*C).  rec [n*H*2] receives (m, den) per
 * (row, head) for the backward pass.
 * Supported: 1 <= H <= 64; 1 <= C <= 64 always, up to 128 / 256 where C, ldz, ldo and the pointers of Z, O (expand: also dO,
 * dZ) allow 8- / 16-byte accesses (C / VEC <= 64); n * H <= 2^31 - 2.  Outside that, a null pointer, n < 0, H or C < 1, a
 * leading dimension below its width: DCR_EINVAL without a launch.  n = 0 is DCR_OK.
 * Order: den and every element of the slot sum one operation per slot (fmaf for the products) in CSR order; a (row, head)
 * above 96 slots as G strided partial sums added in group order, G = 256 / LPH, LPH the first of 4, 8, .., 64 lanes that
 * holds C / VEC.  One true division per output element.  No floating-point atomics: the same bits on every call.
 * Asynchronous on hip_stream. */
int dcr_gat_gather_f32_dev(const int64_t *rowptr_dev, const int32_t *col_dev, const float *Z_dev, const float *s_src_dev,
                           const float *s_dst_dev, float *O_dev, float *rec_dev, int64_t n, int64_t H, int64_t C, int64_t ldz,
                           int64_t lds, int64_t ldo, double negative_slope, void *hip_stream);
/* The backward pass in three launches.  With D[i,h] = <dO[i,h,:], O[i,h,:]> and alpha = expf(e - m) / den recomputed from
 * the scores and rec with the forward's operations:
 *   g_ij,h      = alpha * (<dO[i,h,:], Z[j,h,:]> - D[i,h]) * (pre > 0 ? 1 : negative_slope)
 *   dZ[j,h,:]   = sum_i alpha * dO[i,h,:]      dS_src[j,h] = sum_i g_ij,h      dS_dst[i,h] = sum_j g_ij,h
 * rowptr_dev is the target CSR's; rowptr_t / col_t (targets, in [0, n)) the CSR of the transposed pattern and slot_t
 * (int64) the position of each of its slots in the target CSR (a permutation of [0, E)).  O and rec are the gather's
 * outputs for the same operands.  work_rec [n*H*4] (16-byte aligned, else DCR_EINVAL) and work_g [E*H] (at least one
 * element) are overwritten.  Every element of dZ's H*C columns and of dS_src's and dS_dst's H columns is written: no
 * memset is needed.  Sums over slots in slot order of the CSR each runs on, long rows as above. */
int dcr_gat_expand_f32_dev(const int64_t *rowptr_dev, const int64_t *rowptr_t_dev, const int32_t *col_t_dev,
                           const int64_t *slot_t_dev, const float *Z_dev, const float *s_src_dev, const float *s_dst_dev,
                           const float *O_dev, const float *dO_dev, const float *rec_dev, float *dZ_dev, float *dS_src_dev,
                           float *dS_dst_dev, float *work_rec_dev, float *work_g_dev, int64_t n, int64_t H, int64_t C,
                           int64_t ldz, int64_t lds, int64_t ldo, double negative_slope, void *hip_stream);
/* Attention dropout (torch_geometric's GATConv(dropout = p) in training): the keep weight k in {0, scale},
 * scale = float32(1 / (1 - p)), multiplies alpha AFTER the softmax, so m and den run over every slot:
 *   O[i,h,:]  = ((sum_kept slots w * Z[col,h,:]) / den[i,h]) * scale        rec as without dropout
 *   g_ij,h    = alpha * (k * <dO[i,h,:], Z[j,h,:]> - D[i,h]) * (pre > 0 ? 1 : negative_slope)
 *   dZ[j,h,:] = sum_kept i (alpha * k) * dO[i,h,:]                          D, dS_src and dS_dst as without dropout
 * The stream is the one of the dropout section below, and NO mask is stored: with nnz = rowptr[n] and S8 = nnz rounded up to
 * a multiple of 8, the slot at position pos of the target CSR under head h is element E = h * S8 + pos of an (H * S8)-element
 * tensor under that rule (call E >> 3, word E & 3, half (E >> 2) & 1, key seed, o = offset + *offset_dev; kept when the 16-bit
 * draw >= min(floor(p * 65536), 65535)), so the host's decisions are dropout_ref.decisions(H * S8, p, seed, o) reshaped
 * [H, S8] and cut to [:, :nnz].  The gather redraws it per 8 slots, the expand per slot through slot_t.
 * The gather resolves o (offset_dev may be null: o = offset) and writes it to offset_used_dev [1]; the expand reads o from
 * that word, so a replayed hipGraph whose counter has moved on between the two still applies the forward's mask.
 * nnz must be rowptr[n] (it only sizes S8; nothing on the device checks it).  p outside [0, 1), nnz < 0, a null
 * offset_used_dev: DCR_EINVAL.  At p = 0 every slot is kept and scale is 1: the bits of the entry points above.
 * Every other argument, limit and order: as dcr_gat_gather_f32_dev / dcr_gat_expand_f32_dev. */
int dcr_gat_gather_drop_f32_dev(const int64_t *rowptr_dev, const int32_t *col_dev, const float *Z_dev, const float *s_src_dev,
                                const float *s_dst_dev, float *O_dev, float *rec_dev, int64_t n, int64_t H, int64_t C,
                                int64_t ldz, int64_t lds, int64_t ldo, double negative_slope, void *hip_stream, int64_t nnz,
                                double p, uint64_t seed, uint64_t offset, const int64_t *offset_dev /* nullable */,
                                int64_t *offset_used_dev);
int dcr_gat_expand_drop_f32_dev(const int64_t *rowptr_dev, const int64_t *rowptr_t_dev, const int32_t *col_t_dev,
                                const int64_t *slot_t_dev, const float *Z_dev, const float *s_src_dev, const float *s_dst_dev,
                                const float *O_dev, const float *dO_dev, const float *rec_dev, float *dZ_dev, float *dS_src_dev,
                                float *dS_dst_dev, float *work_rec_dev, float *work_g_dev, int64_t n, int64_t H, int64_t C,
                                int64_t ldz, int64_t lds, int64_t ldo, double negative_slope, void *hip_stream, int64_t nnz,
                                double p, uint64_t seed, const int64_t *offset_used_dev);

/* ---- GCN weight gradient on the matrix cores (device pointers, caller's stream)
 * C[M x N] = A^T * B with A [K x M] and B [K x N] row-major fp32 (lda/ldb/ldc in
 * elements), K = number of nodes: the backward of GCNConv's bias-free Linear,
 * dW = dZ^T * X (third-party torch_geometric; call site models/gcn.py:36 through
 * autograd).  Exact f32 MFMA (v_mfma_f32_32x32x2_f32), K split across workgroups,
 * partial tiles summed in a fixed order: deterministic.  The caller provides a
 * scratch buffer of dcr_atb_f32_workspace() floats.  Asynchronous on hip_stream. */
int dcr_atb_f32_workspace(int64_t K, int64_t M, int64_t N, int64_t *out_floats);
int dcr_atb_f32_dev(const float *A_dev, const float *B_dev, float *C_dev, int64_t K, int64_t M, int64_t N, int64_t lda,
                    int64_t ldb, int64_t ldc, float *workspace_dev, int64_t workspace_floats, void *hip_stream);

/* ---- ReLU + dropout between the GCN layers (device pointers, caller's stream) ------------------------------------
 * models/gcn.py:38-42 (x = act_fn(x); x = dropout(x)) as one pass per direction: y = x > 0 and kept ? x / (1 - p) : 0,
 * the keep decisions packed one bit per element into `bits` (dcr_relu_dropout_bits_words(n) 64-bit words); backward
 * scales the incoming gradient by the same bits.  Philox-4x32-10 keyed by (seed, offset): reproducible for a seed.
 * Sixteen random bits per element: an element is kept with probability 1 - floor(p * 65536) / 65536 (exact at p = 0.5).
 *
 * The stream, for every kernel of this section and the next (tests/dropout_ref.py restates it; tests/test_dropout_stream_gpu.py
 * compares every bit).  For a tensor of n elements in row-major order, element e = 4t + j (quad t, j in 0..3), with
 * o = offset + *offset_dev as a 64-bit sum (offset alone where there is no offset_dev):
 *     r        = Philox-4x32-10(counter = {lo32(t >> 1), hi32(t >> 1), lo32(o), hi32(o)}, key = {lo32(seed), hi32(seed)})
 *     draw     = (r[j] >> 16 * (t & 1)) & 0xFFFF
 *     decision = draw >= min(floor(p * 65536), 65535)
 *     keep     = decision && x[e] > 0
 *     y[e]     = keep ? x[e] * float32(1 / (1 - p)) : 0
 *     bit t & 63 of word 4 * (t >> 6) + j of `bits` is keep
 *     bits that belong to no element are 0 in every word a forward kernel writes
 * For a row-structured [n_rows x H] activation this is the same rule with t = row * H/4 + col/4 and j = col % 4 (RPW = 256 / H
 * rows share four words; a forward kernel writes the ceil(n_rows / RPW) * 4 words its rows reach, dcr_relu_dropout_fwd all
 * dcr_relu_dropout_bits_words(n) of them).  dcr_dropout_words_dev writes `decision` without the sign test in the same places,
 * then the four-word stamp {o, seed, threshold, n_rows} at word ceil(n_rows / RPW) * 4.  The backward kernels read `bits` by
 * this layout alone: any mask packed this way is theirs to apply. */
int dcr_relu_dropout_bits_words(int64_t n, int64_t *out_words);
int dcr_relu_dropout_fwd_f32_dev(const float *x_dev, float *y_dev, uint64_t *bits_dev, int64_t n, double p, uint64_t seed,
                                 uint64_t offset, void *hip_stream);
/* the same with the stream offset = offset + *offset_dev (a call counter the caller keeps in device memory and bumps
 * after each call): the launch parameters are then constants, so the call can be captured in a hipGraph and replayed */
int dcr_relu_dropout_fwd_f32_ctr_dev(const float *x_dev, float *y_dev, uint64_t *bits_dev, int64_t n, double p,
                                     uint64_t seed, uint64_t offset, const uint64_t *offset_dev, void *hip_stream);
int dcr_relu_dropout_bwd_f32_dev(const float *grad_out_dev, float *grad_in_dev, const uint64_t *bits_dev, int64_t n,
                                 double p, void *hip_stream);

/* ---- the same activation fused into the next layer's dense contraction ------------------------------------------------
 * models/gcn.py:36-42 between two layers (x = relu(x); x = dropout(x); next GCNConv's lin: x·W^T, W = [classes, hidden]) in
 * ONE pass over the hidden activation: z_train = dropout(relu(x))·W^T (with h_train = dropout(relu(x)) stored for the weight
 * gradient and the keep bits as above, same Philox stream as dcr_relu_dropout_fwd_f32_ctr_dev) and / or z_eval = relu(x)·W^T.
 * A null z_train (z_eval) skips that operand; a null h_train skips the stored training activation.  hidden 64 or 128, classes <= 16 (other shapes: the separate entry points).
 * Backward of the training operand: dx = keep ? (dz·W) / (1 - p) : 0. */
int dcr_act_linear_fwd_f32_dev(const float *x_dev, const float *w_dev, float *h_train_dev, float *z_train_dev, float *z_eval_dev,
                               int64_t ldz, uint64_t *bits_dev, int64_t n_rows, int hidden, int classes, double p, uint64_t seed,
                               uint64_t offset, const uint64_t *offset_dev, void *hip_stream);  /* ldz: row stride of both z */
int dcr_act_linear_bwd_f32_dev(const float *dz_dev, const float *w_dev, const uint64_t *bits_dev, float *dx_dev, int64_t n_rows,
                               int hidden, int classes, double p, void *hip_stream);
/* The same pass, also returning colsum_dev[hidden] = the column sums of dx: the bias gradient of the layer that produced x
 * (models/gcn.py:36, `bias` of the previous GCNConv) without reading dx again.  ws_dev: dcr_act_linear_bwd_workspace floats;
 * the parts are added in a fixed order (deterministic). */
int dcr_act_linear_bwd_workspace(int64_t n_rows, int hidden, int64_t *floats);
int dcr_act_linear_bwd_colsum_f32_dev(const float *dz_dev, const float *w_dev, const uint64_t *bits_dev, float *dx_dev,
                                      float *colsum_dev, float *ws_dev, int64_t ws_floats, int64_t n_rows, int hidden, int classes,
                                      double p, void *hip_stream);
/* The first GCNConv (models/gcn.py:36, on a precomputed Â·X), the activation and dropout after it (models/gcn.py:38-42) and the
 * second GCNConv's lin in ONE kernel on the matrix cores (csrc/dcr_gcn_first.hip):
 *     pre = ax · W1ᵀ + b1   [n_rows x hidden]   (written when pre_dev != NULL: the backward pass reads it)
 *     z_train = dropout_p(relu(pre)) · W2ᵀ,  z_eval = relu(pre) · W2ᵀ   [n_rows x classes, row stride ldz]; either may be NULL
 * Keep bits, Philox stream and the order of operations of the second contraction are those of dcr_act_linear_fwd_f32_dev on
 * the same pre, so dcr_act_linear_bwd_fused_f32_dev(dz, W2, bits, pre, ...) is its backward.  b1_dev may be NULL.  Shapes:
 * dcr_first_layer_fits(in_features, hidden, classes) != 0: hidden 64 or 128, classes <= 16, any input width (round 5).  Two
 * kernels behind one entry point:
 *   - W1 resident in one CU's LDS (in_features a multiple of 16, hidden x in_features floats + W2 + b1 within 160 KB: the
 *     synthetic bench shape 256 -> 128): dcr_first_layer_fwd_workspace gives 0, ws_dev may be NULL;
 *   - K-chunked (everything else, the reference's own datasets among them — Cora 1,433 -> 128, Citeseer 3,703 -> 64,
 *     utils/hyperparams.py:2-21): W1 streamed through LDS in chunks of 16384 / hidden columns, a workgroup per (64 rows, chunk),
 *     partial tiles in ws_dev, the last workgroup of a row group to arrive adds them in chunk order and runs the epilogue.
 *     ws_dev: dcr_first_layer_fwd_workspace floats, 16-byte aligned; its trailing (n_rows / 64 rounded up) words are tickets:
 *     ZERO before the first use, left zero by every launch (one launch at a time per workspace).
 * ax_dev: n_rows x ldx, ldx >= in_features rounded up to a multiple of 16, the pad columns zero (W1's pad is zero inside the
 * kernel; 0 x NaN would still be NaN).  w1_dev: hidden x in_features, row stride in_features (any alignment for the K-chunked
 * kernel).  dcr_first_layer_fwd_f32_dev is the round-4 entry point: the same call without a workspace (resident shapes only). */
int dcr_first_layer_fits(int in_features, int hidden, int classes);
int dcr_first_layer_fwd_workspace(int64_t n_rows, int in_features, int hidden, int64_t *floats);
int dcr_first_layer_fwd_ws_f32_dev(const float *ax_dev, int64_t ldx, const float *w1_dev, const float *b1_dev, const float *w2_dev,
                                   float *pre_dev, float *z_train_dev, float *z_eval_dev, int64_t ldz, uint64_t *bits_dev,
                                   uint64_t *dwords_dev, int64_t n_rows, int in_features, int hidden, int classes, double p,
                                   uint64_t seed, uint64_t offset, const uint64_t *offset_dev, float *ws_dev, int64_t ws_floats,
                                   void *hip_stream);
/* The dropout decisions of one training call of the kernels above, drawn ahead of it (round 5): dwords_dev
 * [dcr_dropout_words_count words, 8-byte aligned] gets one bit per element of the n_rows x hidden activation, packed as
 * bits_dev is — 1 where the Philox stream of (seed, offset + *offset_dev) keeps the element (F.dropout's mask,
 * models/gcn.py:40, before the activation's sign is known) — followed by a stamp of the call it belongs to (offset + *offset_dev,
 * seed, p, n_rows).  Handed to dcr_first_layer_fwd_ws_f32_dev as dwords_dev, a call with that very stamp reads its decisions
 * there and gives bit for bit what it gives with dwords_dev == NULL; a call with any other stamp draws in line as if it had
 * been given none.  Every training call given a dwords_dev also leaves, in word [dcr_dropout_words_count - 4], its own
 * offset + 1: pointing the next dcr_dropout_words_dev's offset_dev there (offset 0) draws for the call expected next without
 * reading a counter that other work may be moving.  models/gcn.py draws the next epoch's words on a side stream while the
 * current epoch's aggregations run. */
int dcr_dropout_words_count(int64_t n_rows, int hidden, int64_t *words);
int dcr_dropout_words_dev(uint64_t *dwords_dev, int64_t n_rows, int hidden, double p, uint64_t seed, uint64_t offset,
                          const uint64_t *offset_dev, void *hip_stream);
int dcr_first_layer_fwd_f32_dev(const float *ax_dev, int64_t ldx, const float *w1_dev, const float *b1_dev, const float *w2_dev,
                                float *pre_dev, float *z_train_dev, float *z_eval_dev, int64_t ldz, uint64_t *bits_dev, int64_t n_rows,
                                int in_features, int hidden, int classes, double p, uint64_t seed, uint64_t offset,
                                const uint64_t *offset_dev, void *hip_stream);

/* Backward of dcr_first_layer_fwd_f32_dev's training operand in ONE kernel (the backward of models/gcn.py:36-42 for the first
 * two layers' dense parts): from dz = d loss / d z_train [n_rows x classes, contiguous] to
 *     dw1 [hidden x in_features] = dpreᵀ · ax,  db1 [hidden] = column sums of dpre,  dw2 [classes x hidden] = dzᵀ · dropout(relu(pre)),
 * with dpre = keep ? (dz · W2) / (1 - p) : 0 never written to memory (the first layer's input needs no gradient).  bits, pre:
 * as dcr_first_layer_fwd_f32_dev left them.  ws_dev: dcr_first_layer_bwd_workspace floats.  Any in_features (round 5: the true
 * width of W1 / dW1, row stride in_features; ax_dev as in the forward call, ldx >= in_features rounded up to 16), hidden 64 or
 * 128, classes <= 16.  The input width is tiled by 256 columns (grid y), the rows by about one workgroup per CU in total.
 * Partial results are added in a fixed order: deterministic. */
int dcr_first_layer_bwd_workspace(int64_t n_rows, int in_features, int hidden, int64_t *floats);
int dcr_first_layer_bwd_f32_dev(const float *dz_dev, const float *w2_dev, const uint64_t *bits_dev, const float *pre_dev,
                                const float *ax_dev, int64_t ldx, float *dw1_dev, float *db1_dev, float *dw2_dev, float *ws_dev,
                                int64_t ws_floats, int64_t n_rows, int in_features, int hidden, int classes, double p, void *hip_stream);

/* The whole backward of dcr_act_linear_fwd_f32_dev's training operand in one pass over x, on the matrix cores: dx as above,
 * colsum_dev[hidden] = its column sums, dw_dev[classes x hidden] = dz^T · h with h = keep ? x / (1 - p) : 0 rebuilt from x and
 * the keep bits (the forward call may then pass h_train_dev = NULL and store no activation).  Replaces the weight-gradient
 * reduction of the next layer's Linear (models/gcn.py:36, dW = dz^T · h) as well.  Deterministic (fixed-order sums). */
int dcr_act_linear_bwd_fused_workspace(int64_t n_rows, int hidden, int64_t *floats);
int dcr_act_linear_bwd_fused_f32_dev(const float *dz_dev, const float *w_dev, const uint64_t *bits_dev, const float *x_dev,
                                     float *dx_dev, float *dw_dev, float *colsum_dev, float *ws_dev, int64_t ws_floats,
                                     int64_t n_rows, int hidden, int classes, double p, void *hip_stream);

/* ---- loss and accuracy on the rows an epoch reads (device pointers, caller's stream) ----
 * experiment/training_loop.py:51 F.nll_loss(log_probs[mask], y[mask]) as out_loss[0] = -mean_i lp[i, y_i] over m rows of
 * log-probabilities (row stride ld), and its backward grad[i, c] = (c == y_i) ? -g[0] / m : 0 over the contiguous [m, classes]
 * gradient (what the stock kernels produce); :64-71 log_probs[mask].max(1)[1].eq(y[mask]).sum() as out_count[0] (first maximum
 * per row). */
int dcr_nll_picked_mean_fwd_f32_dev(const float *lp_dev, int64_t ld, const int64_t *y_dev, int64_t m, int classes, float *out_loss_dev,
                                    void *ws_dev, void *hip_stream);   /* ws_dev: as dcr_head_fwd_f32_dev's (may be the same buffer) */
/* Round 5: the head of an epoch in ONE kernel per direction, from the RAW outputs o = (Â·Z + b)[rows] of the last aggregation
 * (models/gcn.py:44 log_softmax + experiment/training_loop.py:51 F.nll_loss on the training rows; :64-71 arg-max accuracy on the
 * evaluated rows — the arg-max of log-probabilities is the arg-max of the logits):
 *     out_loss[0]    = mean_i (lse_i - o_train[i, y_i]),  lse_i = log sum_c exp o_train[i, c]
 *     out_correct[0] = #{i : first arg-max of o_eval[i, :] == y_eval[i]}
 * and backward  grad[i, c] = (exp(o_train[i, c] - lse_i) - [c == y_i]) * g[0] / m_train  (contiguous [m_train, classes]) with
 * grad_bias[c] = its column sums (the gradient of the last GCNConv's bias; may be NULL).  Either half of the forward call may be
 * absent (m = 0).  classes <= 32.  Labels must be class ids in [0, classes) (what F.nll_loss accepts without ignore_index).
 * ws_dev: dcr_head_workspace bytes, 8-byte aligned, ZERO before the first use; every launch leaves its tickets zero (one launch
 * at a time per workspace).  Sums in a fixed order: deterministic. */
/* Round 5: torch.optim.Adam's update (experiment/save_models.py:78-82; amsgrad off, L2 weight decay added to the gradient) for up
 * to 8 float32 tensors in ONE launch: params / grads / exp_avg / exp_avg_sq are host arrays of device pointers, numel and
 * weight_decay host arrays.  step_dev: the step count as one float in device memory (read, then advanced by one: a captured
 * epoch replays the increment); ticket_dev: one zero word, left zero. */
int dcr_adam_step_f32_dev(int n_tensors, void *const *params_dev, const void *const *grads_dev, void *const *exp_avg_dev,
                          void *const *exp_avg_sq_dev, const int64_t *numel, const float *weight_decay, double lr, double beta1,
                          double beta2, double eps, float *step_dev, uint32_t *ticket_dev, void *hip_stream);
int dcr_head_workspace(int64_t *bytes);
int dcr_head_fwd_f32_dev(const float *o_train_dev, int64_t ld_train, const int64_t *y_train_dev, int64_t m_train, const float *o_eval_dev,
                         int64_t ld_eval, const int64_t *y_eval_dev, int64_t m_eval, int classes, float *out_loss_dev,
                         int64_t *out_correct_dev, void *ws_dev, int64_t ws_bytes, void *hip_stream);
int dcr_head_bwd_f32_dev(const float *o_train_dev, int64_t ld_train, const int64_t *y_train_dev, int64_t m_train, int classes,
                         const float *g_dev, float *grad_dev, float *grad_bias_dev, void *ws_dev, int64_t ws_bytes, void *hip_stream);
int dcr_nll_picked_mean_bwd_f32_dev(const int64_t *y_dev, int64_t m, int classes, const float *g_dev, float *grad_dev, void *hip_stream);
int dcr_count_argmax_equal_f32_dev(const float *lp_dev, int64_t ld, const int64_t *y_dev, int64_t m, int classes, int64_t *out_count_dev,
                                   void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* DCR_H */
