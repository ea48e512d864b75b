/*
 * mgp_hip.h -- C-ABI of libmgp_hip.so: the MI355X (gfx950) implementation of manifold-gp's
 * sparse graph-Laplacian GP hot path.
 *
 * Boundary contract (every entry point):
 *   - extern "C", plain device pointers + sizes + a hipStream_t passed as void*; no torch types;
 *   - returns int: 0 = ok, <0 = argument error (MGP_ERR_*), >0 = hipError_t from the runtime;
 *   - never allocates or frees caller memory: scratch comes from an explicit `work` buffer whose
 *     size the matching *_workspace_bytes() query returns; a `work_bytes` below that size is
 *     MGP_ERR_WORKSPACE before any launch, also where the carve would fit in less (docs/memory_contract.md);
 *   - asynchronous on `stream` unless the comment says it synchronises (graph-build calls that
 *     must report a data-dependent size do).  In tested terms (docs/stream_contract.md): every launch, copy and memset of
 *     a call is ordered on `stream` and on no other; a call issued behind pending work of `stream` reads its inputs
 *     only once that work is done, and its results are those of the same call on an idle null stream (bit for bit wherever two such calls agree bit for bit);
 *     work on other streams neither waits for it nor is waited for; a plan replays its captured graphs on the stream
 *     it was created with;
 *   - all matrices of right-hand sides are row-major [N, C] fp32, indices int32, values fp32.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * nash169/manifold-gp checkout; third-party call sites are the reference's, the arithmetic
 * lived in faiss / torch_sparse / linear_operator / ATen).
 */
#ifndef MGP_HIP_H
#define MGP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGP_OK 0
#define MGP_ERR_ARG (-1)        /* null pointer / bad size / bad enum */
#define MGP_ERR_WORKSPACE (-2)  /* work buffer too small */
#define MGP_ERR_UNSUPPORTED (-3)
#define MGP_ERR_NOT_CONVERGED (-4)
#define MGP_ERR_KNN_AMBIGUOUS (-5)
#define MGP_ERR_TIMEOUT (-6)      /* a multi-rank solve's stream did not drain within MGP_DIST_TIMEOUT_S seconds (default 300):
                                      a peer rank is gone or a collective hangs; the caller must exit, not retry */

#define MGP_PAD 4 /* CSR rows are padded to a multiple of 4 entries (16-byte vector loads) */

/* library / device probes ------------------------------------------------------------------ */
int mgp_version(void);                       /* 100*major + minor */
int mgp_device_info(int* cu_count, int* wave_size, size_t* hbm_bytes); /* hipGetDeviceProperties */

/* ---------------------------------------------------------------------------------------------
 * k-NN: exact brute-force squared-L2 top-k, ascending (d2, index).
 * Replaces faiss IndexFlatL2 / IndexIVFFlat(nlist=1) / Gpu* `search` as called at
 * manifold_gp/utils/nearest_neighbors.py:35-37 (index built at :17-33).
 *   db [N,d] f32 row-major (the indexed points), q [n,d] f32 (queries), k <= min(N, 1024)
 *   D [n,k] f32 = (float) of the fp64 distance, I [n,k] i32
 * Distances/ties follow the rule in oracle/knn_oracle.c (fp64 sum in ascending feature order,
 * no FMA contraction, lower index wins exact ties): fp32 tiles select a padded candidate set,
 * an fp64 re-rank orders it, a per-row bound check proves the set sufficient, rows that fail
 * are redone with a wider set and finally by an exact fp64 scan.  For d <= 3 and N >= 4096 no
 * N x n distance slab is formed: points are Morton-sorted, a window around the query gives a provable
 * upper bound on its k-th neighbour distance, one fused pass over the chunks of points whose bounding box
 * meets the workgroup's search box keeps the points under that bound and the fp64 re-rank orders them (knn_lowd.hip); rows whose candidate list overflows go
 * through the slab pipeline.  Same results bit for bit.  Synchronises `stream`.
 * stats (nullable, host int64[4]): rows redone wide, rows redone exact, chunks, candidates K'
 * (-1 when the low-dimensional path ran; [0] then counts its overflow rows). */
size_t mgp_knn_workspace_bytes(int64_t N, int64_t n, int d, int k);
int mgp_knn_search(const float* db, int64_t N, int d, const float* q, int64_t n, int k,
                   float* D, int32_t* I, void* work, size_t work_bytes, int64_t* stats,
                   void* stream);
/* d >= 32 and >= 1024 queries: the candidate keys of the slab pipeline come from the matrix cores (centred bf16 two-term
 * split, GEMM form, knn_mfma.hip) with an absolute error bound in the sufficiency check; a chunk in which
 * many rows fail that check is redone with the direct-difference tiles.  0 forces the direct tiles
 * (default 1).  mgp_knn_last_direct_chunks: chunks of the last slab search that were redone. */
int mgp_knn_set_mfma(int on);
int64_t mgp_knn_last_direct_chunks(void);
/* Self-search (q == db, n == N: the graph build, nearest_neighbors.py:35-37 called on the training inputs) with the whole
 * N x N key matrix inside the workspace (N <= 92k: 32 GiB): key(x, y) = key(y, x), so the matrix-core kernel computes the
 * tile pairs on and above the diagonal only and stores each off-diagonal tile twice (as it is and transposed): half the
 * MFMA work, the same selection, the same results bit for bit.  Default 1; 0 computes every tile (tests, A/B runs). */
int mgp_knn_set_symmetric(int on);
/* Candidate filter of the matrix-core searches (round 5).  A large search does not write its keys to an N x n slab for the
 * select kernel to read back (60k x 60k: 14.4 GB each way): the keys of every row to a 1/stride sample of the points
 * (stride 16 up to k = 64) give a per-row bound >= the row's K'-th smallest key; the key pass appends the ~stride K' keys
 * per row under the bounds to a log (one returning atomic per WORKGROUP and tile pair draws its range; a self-search logs
 * each key of an off-diagonal tile for both of its rows); regroup_kernel deals the log to per-row candidate lists (3840
 * entries of {key, index}) with LDS counters; the select kernel takes the exact K'-th smallest key, the candidates, the fp64
 * re-rank and the sufficiency check from the list.  Rows whose list overflows or whose check fails are gathered and redone
 * by the slab pipeline (which ends in the exact scan); a chunk whose log fills up is redone there whole: the results are
 * the oracle's bit for bit, as before.  Workspace at 60k x 784: 4.9 GB instead of 14.8.  mode 0: key slab (rounds 1-4);
 * 1 (default): searches of >= 4096 queries against >= 16384 points; 2: every matrix-core search whose k the lists can serve
 * (tests).  Lab / test switch: read once per call.
 * mgp_knn_last_filter_failover: rows of the last search handed to the slab pipeline; -1 when the search ran on the slab. */
int mgp_knn_set_filter(int mode);
int64_t mgp_knn_last_filter_failover(void);
/* Prepared index (d >= 32): the part of a search that depends on the points alone -- column means, the centred bf16 split
 * in the key kernel's tile layout, norms -- built once (faiss: index.train / index.add, nearest_neighbors.py:20-33) and
 * handed to every search.  Without it a search prepares the points itself (~1 ms at 60k x 784) and therefore keeps small
 * query batches (< 1024 rows) on the fp32 direct-difference tiles; with it the matrix cores rank the candidates of any batch
 * (600 queries against 60k x 784: 1.3 -> 0.5 ms).  The index is a SNAPSHOT of db at build time (faiss copies its vectors):
 * rebuild it when db changes.  Results are the oracle's bit for bit either way.  mgp_knn_index_bytes: 0 when d < 32. */
size_t mgp_knn_index_bytes(int64_t N, int d);
int mgp_knn_index_build(const float* db, int64_t N, int d, void* index, size_t index_bytes, void* stream);
int mgp_knn_search_indexed(const float* db, int64_t N, int d, const void* index, size_t index_bytes, const float* q,
                           int64_t n, int k, float* D, int32_t* I, void* work, size_t work_bytes, int64_t* stats,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Graph: k-NN lists -> symmetrised graph.  Replaces NearestNeighbors.graph
 * (manifold_gp/utils/nearest_neighbors.py:39-55: drop column 0, orient row<col,
 * torch_sparse.coalesce(op='mean')).
 * Outputs (caller allocates the upper bounds, actual sizes returned through host pointers):
 *   reference view: tri_row/tri_col i32 [<= n(k-1)], tri_val f32 -- sorted unique (row<=col) COO,
 *                   value = fp32 mean of the duplicates;  *M = number of undirected edges
 *   kernel view   : full symmetric padded CSR of the same graph: rowptr i32 [n+1] (every row
 *                   start a multiple of MGP_PAD), col i32 / d2 f32 / eid i32 [<= 2n(k-1)+4n]
 *                   (eid = index into tri_*; padding entries: col = own row, d2 = +inf, eid = -1)
 *                   *nnz = rowptr[n].  A (i,i) edge (duplicate points) appears twice in row i,
 *                   exactly as the reference scatters it twice.
 * Synchronises `stream` (needs M on the host). */
size_t mgp_graph_workspace_bytes(int64_t n, int k);
/* The edge list of NearestNeighbors.graph for ANY flag combination (nearest_neighbors.py:39-55), without the CSR that
 * mgp_graph_build adds for the default one (symmetric, no self loops): self_loop keeps column 0 of the lists (an (i, i) entry
 * at distance 0), symmetric orients every pair as (min, max), sorts and merges duplicates with the fp32 mean
 * (torch_sparse.coalesce(op='mean')); not symmetric: the n (k - first) directed pairs in row-major order.  out_* hold
 * n (k - first) entries (first = 0 with self_loop, else 1); *M = the number written.  Workspace (symmetric only):
 * mgp_graph_workspace_bytes(n, k + 1). */
int mgp_graph_edges(const float* D, const int32_t* I, int64_t n, int k, int symmetric, int self_loop, int32_t* out_row,
                    int32_t* out_col, float* out_val, int64_t* M, void* work, size_t work_bytes, void* stream);
int mgp_graph_build(const float* D, const int32_t* I, int64_t n, int k, int32_t* tri_row, int32_t* tri_col,
                    float* tri_val, int64_t* M, int32_t* rowptr, int32_t* col, float* d2, int32_t* eid,
                    int64_t* nnz, void* work, size_t work_bytes, void* stream);
/* same CSR from an existing reference-style edge list (idx[2,M] given as two i32 arrays) */
size_t mgp_graph_coo_workspace_bytes(int64_t n, int64_t M);
int mgp_graph_from_coo(const int32_t* tri_row, const int32_t* tri_col, const float* tri_val,
                       int64_t M, int64_t n, int32_t* rowptr, int32_t* col, float* d2, int32_t* eid,
                       int64_t* nnz, void* work, size_t work_bytes, void* stream);

/* Row-tile column dictionaries for the C == 1 SpMV.  A tile is `tile_rows` consecutive rows of the padded
 * CSR; tile_cols lists the distinct columns the tile references (ascending), lid maps every entry to
 * its column's position in that list.  The SpMV stages x[tile_cols] in LDS once per tile, so the
 * texture path sees one access per DISTINCT column instead of one per entry and the matrix stream
 * shrinks to 6 bytes per entry.  No reference counterpart (the reference scatters with atomics,
 * graph_laplacian_operator.py:117-120).
 *   tile_ptr [ceil(n/tile_rows)+1], tile_cols [capacity nnz], lid [nnz]  (device, caller allocated)
 *   total_cols / max_cols / max_entries: host outputs.  MGP_ERR_UNSUPPORTED when a tile references
 *   more than 65536 distinct columns (use a smaller tile or leave the dictionaries off). */
size_t mgp_graph_tiles_workspace_bytes(int64_t n, int64_t nnz);
/* row_order (nullable): a permutation of the rows; tile t then holds rows row_order[64 t .. 64 t + 63]
 * (locality order for inputs that arrive unordered).  With it the tile view is a second CSR in that
 * order: tile_rowptr [n+1] (entry offsets), emap [nnz] (tile-order entry -> entry of the CSR: gather
 * the values through it, mgp_csr_t.tile_vals), lid in tile order; column ids stay the original ones. */
int mgp_graph_tiles(int64_t n, const int32_t* rowptr, const int32_t* col, int64_t nnz, int tile_rows,
                    const int32_t* row_order, int32_t* tile_rowptr, int32_t* emap, int32_t* tile_ptr,
                    int32_t* tile_cols, uint16_t* lid, int64_t* total_cols, int32_t* max_cols,
                    int32_t* max_entries, void* work, size_t work_bytes, void* stream);

/* Breadth-first (Cuthill-McKee style) locality order of the graph: order [n] = node ids level by level,
 * a level sorted by (position of the first-numbered parent, node id); components are appended one
 * after the other.  Deterministic.  For inputs whose node order carries no locality (random point
 * order) the tile dictionaries built on this order recover the reuse a spatially sorted input has.
 * Synchronises `stream` (one host round trip per BFS level). */
/* Morton (Z-curve) order of points with d <= 3: int32 [n] permutation, ascending code.  The cheaper and
 * tighter alternative to the BFS order when coordinates of low dimension are at hand.  Synchronises. */
size_t mgp_morton_order_workspace_bytes(int64_t n);
int mgp_morton_order(const float* x, int64_t n, int d, int32_t* order, void* work, size_t work_bytes, void* stream);
/* Nearest-neighbour chain order (round 5): from the node in hand step to its nearest not-yet-numbered neighbour (by d2), else to
 * that of one of the last 64 chain nodes, else to the unnumbered node of smallest index.  For k-NN graphs whose given order keeps
 * clusters together but not the order inside them (rotation orbits in random angle order) it makes the rows of a tile share most
 * of their columns: 2.5 x fewer distinct columns per 16-row tile on the 60k RMNIST-like graph, which is what the matrix-core SpMM's
 * work is proportional to.  Sequential walk on the HOST over a copy of the CSR (one-off per graph); deterministic; synchronises. */
int mgp_graph_chain_order(int64_t n, const int32_t* rowptr, const int32_t* col, const float* d2, int32_t* order, void* stream);
/* dst[p, :] = src[order[p], :] for a row-major float32 block [n, C] (order: int32 [n], any row list with entries in [0, n_src);
 * src != dst).  What the solvers that iterate on P A P^T (graph.RelabelledGraph) permute right-hand sides in and solutions out
 * with; no counterpart in the reference. */
int mgp_permute_rows(const float* src, const int32_t* order, int64_t n, int C, float* dst, void* stream);
size_t mgp_graph_bfs_workspace_bytes(int64_t n);
int mgp_graph_bfs_order(int64_t n, const int32_t* rowptr, const int32_t* col, int32_t* order, void* work,
                        size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Laplacian build: diffusion-maps normalisation of the kernel weights, fused row passes.
 * Replaces the cached properties adjacency_unnorm_mat / degree_unnorm_mat / adjacency_mat /
 * degree_mat / laplacian_diag / laplacian_triu of
 * manifold_gp/operators/graph_laplacian_operator.py:52-106.
 *   in : padded CSR (rowptr, col, d2), eps (graph bandwidth), self_loops
 *   out: degree_unnorm D~ [n], degree D [n], diag [n], dsqrt = sqrt(D) [n], dinvsqrt [n],
 *        vals [nnz] = S_ij = A_ij / (sqrt(D_i) sqrt(D_j)) / eps^2  (positive; L_ij = -S_ij) */
int mgp_laplacian_build(int64_t n, const int32_t* rowptr, const int32_t* col, const float* d2,
                        float eps, int self_loops, float* degree_unnorm, float* degree,
                        float* diag, float* dsqrt, float* dinvsqrt, float* vals, void* stream);
/* Forward-mode tangent of mgp_laplacian_build wrt the graph bandwidth: d/d eps of D~, D, diag, sqrt(D),
 * 1/sqrt(D) and the CSR values (same three row passes).  With it d(u^T L v)/d eps = u^T L' v is one more
 * fused SpMV on (d_vals, d_diag): the hyper-parameter gradient path the reference obtains by autograd
 * through graph_laplacian_operator.py:52-124 (pinned by test/_test_functions.py:59-74). */
int mgp_laplacian_tangent(int64_t n, const int32_t* rowptr, const int32_t* col, const float* d2,
                          float eps, int self_loops, const float* degree_unnorm, const float* degree,
                          const float* diag, float* d_degree_unnorm, float* d_degree, float* d_diag,
                          float* d_dsqrt, float* d_dinvsqrt, float* d_vals, void* stream);
/* The reductions of the differentiable fused SpMM's backward pass in one launch (autograd through graph_laplacian_operator.py:108-124 /
 * precision_matern_operator.py:26-37 wrt bandwidth, length scale and the node vectors; `_test_functions.py:59-104`).  Blocks are
 * [n, C] row-major float32: h = cov post (.) g (upstream gradient), xs = pre (.) X, dlx = L' xs (tangent product), lx = L xs,
 * gxs = a h + b L h.  Writes partial[mgp_spmm_backward_blocks(n)][2] = per-workgroup sums of <h, dlx> and <h, xs> (the caller adds
 * them up), gpre[r] = sum_c gxs X and gpost[r] = cov sum_c g (a xs + b lx).  Null dlx / gpre / gpost switch that output off. */
int mgp_spmm_backward_blocks(int64_t n);
int mgp_spmm_backward_sums(int64_t n, int C, const float* h, const float* dlx, const float* xs, const float* gxs, const float* X,
                           const float* g, const float* lx, float av, float bv, float cov, float* partial, float* gpre,
                           float* gpost, void* stream);
/* per-edge values in the reference's COO order: which = 0 W (adjacency_unnorm_mat :54-56),
 * 1 A (adjacency_mat :73-75), 2 S (laplacian_triu :104-106) */
int mgp_edge_values(const int32_t* tri_row, const int32_t* tri_col, const float* tri_val,
                    int64_t M, const float* degree_unnorm, const float* degree, float eps,
                    int which, float* out, void* stream);

/* Entry-balanced row tiles for the single-column tile kernels (graph.py c1_balanced_tiles; docs/kernels/spmm.md, round 8): a
 * second tile set over the SAME col / vals of a CSR (mgp_csr_t, below) in natural row order, whose tiles are at most 64
 * consecutive rows and at most MGP_C1_TILE_CAP padded entries (a single heavier row is a tile of its own).  Tile t owns positions 64 t .. 64 t + 63 of a padded
 * position space: its rows first, then empty positions.  A HOST struct of device pointers and host numbers, named by
 * mgp_csr_t.c1_tiles.  Taken at C == 1 only, on a CSR without a row order, without a row offset, one tile per workgroup
 * (csrc/spmm_policy.h c1_balanced); the 64-row set of the CSR stays what every other kernel reads. */
typedef struct {
  int64_t n;                 /* rows of the CSR the set was cut for (== mgp_csr_t.n) */
  const int32_t* tile_ptr;   /* [tiles + 1] offsets into tile_cols */
  const int32_t* tile_cols;  /* distinct column ids of each balanced tile, ascending */
  const uint16_t* lid;       /* [nnz] position of every entry's column in its balanced tile's list */
  const int32_t* rowptr_pad; /* [64 tiles + 1] entry offsets of the positions (an empty position repeats its offset) */
  const int32_t* tile_shift; /* [tiles + 1] empty positions in front of tile t: its first row is 64 t - tile_shift[t];
                                tile_shift[tiles] = 64 tiles - n.  ONE allocation with the offsets: tile_shift == rowptr_pad +
                                64 tiles + 1, else the set is not taken (the kernels have no scalar register for another pointer) */
  int32_t tiles;             /* T */
  int32_t max_cols;          /* max over balanced tiles of the list length */
  int32_t max_entries;       /* max over balanced tiles of the padded entry count */
  int32_t reserved;
} mgp_c1_tiles_t;

/* ---------------------------------------------------------------------------------------------
 * The hot kernel: fused CSR SpMV / SpMM with the symmetric Laplacian.
 *   xs_j = pre ? pre[j] * X[j,:] : X[j,:]
 *   lx_i = diag[i] * xs_i - sum_j vals[ij] * xs_j
 *   t_i  = (post ? post[i] : 1) * (a * xs_i + b * lx_i)
 *   Y[i,:] = (base ? cb * base[i,:] : 0) + co * t_i
 *   dot_partials (nullable) [dot_blocks, C]: per-workgroup partial sums of dotw[i,:] * Y[i,:]
 * Replaces GraphLaplacianOperator._matmul (graph_laplacian_operator.py:108-124: two
 * torch_sparse.spmm calls + diagonal + random-walk scalings) and is the building block of the
 * precision / wrapper operators below.  pre/post/base/dotw/dot_partials may be NULL. */
typedef struct {
  int64_t n;
  const int32_t* rowptr;
  const int32_t* col;
  const float* vals;
  const float* diag;
  int64_t ncols;           /* length of the vectors the columns index (0 = n; > n for a row slice) */
  /* row-tile column dictionaries (mgp_graph_tiles); all NULL / 0 = gather straight from memory */
  const int32_t* tile_ptr;   /* [ntiles + 1] offsets into tile_cols, ntiles = ceil(n / tile_rows) */
  const int32_t* tile_cols;  /* distinct column ids of each tile, ascending */
  const uint16_t* lid;       /* [nnz] position of every entry's column in its tile's list */
  int32_t tile_rows;
  int32_t tile_max_cols;     /* max over tiles of the list length (LDS floats per workgroup) */
  int32_t tile_max_entries;  /* max over tiles of the padded entry count */
  int32_t spmv_lanes;        /* C == 1 row-group kernel: lanes per row for THIS matrix, one of 4, 8, 16, 32, 64; 0 = the process
                                default (mgp_spmm_set_group_hint, initially 16).  Any other value: MGP_ERR_ARG */
  /* tiles over a row ORDER (mgp_graph_tiles with row_order): all NULL = tile t is rows 64 t .. 64 t + 63.
   * Three DEVICE arrays, all three or none: a partial order selects no dictionary kernel */
  const int32_t* tile_rowptr;  /* [n+1] entry offsets in tile order */
  const float* tile_vals;      /* [nnz] vals gathered through emap */
  const int32_t* tile_rowid;   /* [n] original row of every tile-order position (= row_order) */
  /* dense 16-row tiles for the matrix-core SpMM at 48 <= C <= 256 (mgp_spmm_mt_fill); all NULL / 0 = not built */
  const int32_t* mt_sptr;      /* [mt_tiles + 1] steps (of four distinct columns) before tile t; multiples of 16 */
  const int32_t* mt_dcol;      /* [4 mt_steps + 192] the tiles' distinct columns, padded per tile to whole bodies of 64 */
  const float* mt_img;         /* [64 (mt_steps + 32)] tile values in MFMA operand order */
  int32_t mt_tiles;            /* ceil(n / 16) */
  int32_t mt_steps;            /* mt_sptr[mt_tiles] */
  /* entry-balanced tile set for the single-column tile kernels (mgp_c1_tiles_t, above); NULL = none.  A HOST pointer: the
   * descriptor must live as long as the struct and every plan made from it are used */
  const mgp_c1_tiles_t* c1_tiles;
} mgp_csr_t;

/* Padded entries a workgroup of the single-column tile kernels holds in registers (4 entries x NQ = 4 quads x 256 lanes): what
 * the balanced cut caps a tile at.  csrc/spmm.hip asserts it against the kernel's constants. */
#define MGP_C1_TILE_CAP 4096

/* workgroups that write dot partials for this CSR (format aware; use this one to size dot_partials) */
int mgp_spmm_dot_blocks_csr(const mgp_csr_t* L, int C);
int mgp_spmm_set_tile_mode(int on);          /* C == 1: use the tile dictionaries when present (default 1) */
/* C == 1 tile kernel, lab: 1 = run the tile-loop form of the kernel even where every workgroup owns one tile (default 0: such
 * graphs, up to 4096 row tiles, run the single-tile form).  Both forms give the same bits (tests/test_gpu_tile_head.py). */
int mgp_spmm_set_tile_loop_mode(int on);
int mgp_spmm_set_tile_small_mode(int on);    /* C in {4,8,12,16}: LDS-dictionary multi-column kernel on 64-row tiles
                                                (default 1; 0 = the per-entry gather kernel) */
/* 16 < C <= 256 with C % 4 == 0 on 64-row tiles: LDS-dictionary kernel in 16-column chunks where it wins (an X block of
 * 96 MB and more: default 1); 0 = never; 2 = whenever the shape allows (tests, A/B runs). */
int mgp_spmm_set_tile_wide_mode(int on);
/* 16 < C <= 256 with C % 4 == 0 on 64-row tiles (round 3): the dictionary kernel with LANES OVER COLUMNS
 * (csrc/spmm.hip spmm_dict_kernel) -- a tile's distinct X rows cross the vector memory path once per tile, staged in
 * double-buffered slices of 256-byte-aligned LDS slots that every entry then reads conflict-free.  Default 1: taken
 * where it was measured to win (from 64 columns up, an X block of 96 MB and more); 0 = never; 2 = wherever the shape allows.
 * Requires what the graph
 * builders guarantee: within a row the entries' columns ascend (padding entries, value 0, at the row's end).
 * Replaces torch_sparse.spmm at manifold_gp/operators/graph_laplacian_operator.py:118-119 for the [N, 100] right-hand
 * sides of precision_matern_operator.py:50-53 and the eigensolver's blocks. */
int mgp_spmm_set_dict_mode(int on);
/* 48 <= C <= 256 with C % 4 == 0 (round 4): the SpMM on the fp32 MATRIX CORES over 16-row tiles stored dense in their own distinct
 * columns (csrc/spmm.hip spmm_mt_kernel): a tile's distinct X rows cross the vector memory path once per tile and 64-column
 * block, straight into the MFMA operand layout; no LDS, no barrier.  Taken when the CSR
 * carries mt_* and the call has no row offset (weighted dot-product partials included: one row of partials per workgroup of four
 * (tile, block) waves, mgp_spmm_dot_blocks_csr counts them); a row's sum is taken in ascending column order.
 * N = 60k, C = 128: 60 us against 94 for the gather kernel.  mgp_spmm_set_mt_mode(0) = never; returns the previous setting.
 * mgp_spmm_mt_fill builds mt_dcol / mt_img from a CSR in natural row order and its 16-row tile dictionaries
 * (mgp_graph_tiles with tile_rows = 16: tile_ptr16, tile_cols16, lid16) and the step offsets sptr (per tile
 * 16 ceil(D / 64) steps -- whole bodies of four blocks --, exclusive prefix sum, `steps` = the total).
 * Replaces torch_sparse.spmm at manifold_gp/operators/graph_laplacian_operator.py:118-119 for the eigensolver's blocks and
 * the [N, 100] right-hand sides of precision_matern_operator.py:50-53. */
int mgp_spmm_set_mt_mode(int on);
/* which kernel mgp_spmm_fused would launch for this CSR / width (tests, docs).  The precedence order, the one of spmm_plan in
 * csrc/spmm.hip rule for rule; the first rule that matches decides, and the returned number is the one in brackets
 * (4 was a round-4 kernel, removed):
 *   1. [1] C == 1, tile dictionaries of 32 / 64 / 128 rows that fit the LDS (tile mode 1): the C == 1 tile kernel
 *   2. [2] C in {4, 8, 12, 16}, 64-row tiles within the LDS budget (tile mode 1, tile-small mode 1): the small-C tile kernel
 *   3. [3] 48 <= C <= 256, C % 4 == 0, the CSR carries mt_* (mt mode 1), no row offset: matrix-core tiles.  With a row offset
 *          the image is ignored and rules 4-7 apply -- except with dot partials, whose count mgp_spmm_dot_blocks_csr sized for
 *          the matrix-core kernel: MGP_ERR_UNSUPPORTED from this function and from mgp_spmm_fused_rows alike (strip mt_* from
 *          the struct for such a call)
 *   4. [5] 16 < C <= 256, C % 4 == 0, 64-row tiles, C >= 64, X block >= 96 MB (dict mode 1; 2: any size): lanes-over-columns dictionary
 *   5. [6] the same shapes, X block >= 96 MB (tile-wide mode 1; 2: any size): chunked dictionary
 *   6. [0] C == 1: row groups of spmv_lanes lanes
 *   7. [0] C > 1: gather from memory; the member (row16, float4 lanes under v4 mode, per-column) by pointer alignment at launch --
 *          all three write the same dot-partial blocks
 * Rules 2-5: X / Y / base / dotw that are not 16-byte aligned are MGP_ERR_ARG at launch, never a fall-through to another kernel. */
int mgp_spmm_kernel_choice(const mgp_csr_t* L, int C, int with_dot, int64_t row_offset);
int mgp_spmm_mt_fill(int64_t n, const int32_t* rowptr, const float* vals, const uint16_t* lid16, const int32_t* tile_ptr16,
                     const int32_t* tile_cols16, const int32_t* sptr, int64_t steps, int32_t* dcol, float* img, void* stream);
/* Measurement hook (bench.py `roofline`): between begin and end every EAGER launch of the C == 1 tile kernel carries
 * its own start / stop event pair (hipExtLaunchKernelGGL: the dispatch's begin / end timestamps); end returns the sum of
 * the kernel durations and the number of launches timed (at most max_launches).  No effect on results. */
int mgp_spmm_timing_begin(int max_launches);
int mgp_spmm_timing_end(float* total_ms, int* launches);
/* 16 < C <= 256 with C % 4 == 0 on a quad-padded CSR (what the graph builder produces), 16-byte aligned operands: a
 * lane owns one float4 of the row instead of one column; used where it wins (C <= 64, or an X block of 96 MB and more:
 * default 1); 0 = never (the per-column gather kernel); 2 = always (tests, A/B runs). */
int mgp_spmm_set_v4_mode(int on);

int mgp_spmm_dot_blocks(int64_t n, int C);   /* workgroups that write dot partials */
int mgp_spmm_set_group_hint(int lanes);      /* C == 1: lanes per row, one of 4,8,16,32,64: the default for structs whose
                                                spmv_lanes is 0 (a struct that sets the field is not affected) */
int mgp_spmm_set_rows_in_flight(int rows);   /* C == 1 fallback kernel: rows a lane group loads at once: 1,2,4,8 */
int mgp_spmm_fused(const mgp_csr_t* L, const float* X, int C, float* Y, float a, float b,
                   const float* pre, const float* post, const float* base, float cb, float co,
                   const float* dotw, float* dot_partials, void* stream);

/* row-partitioned form: L_local = rows [row_offset, row_offset + L_local->n) of the operator (column
 * ids global), vectors of global length; writes only the local rows of Y (and local dot partials) */
int mgp_spmm_fused_rows(const mgp_csr_t* L_local, int64_t row_offset, const float* X, int C, float* Y,
                        float a, float b, const float* pre, const float* post, const float* base,
                        float cb, float co, const float* dotw, float* dot_partials, void* stream);

/* measurement helper: `reps` back-to-back launches of Y = L X replayed as one hipGraph; elapsed_ms
 * (nullable, host) = HIP-event time of the launches on `stream`.  Synchronises `stream`. */
int mgp_spmm_repeat(const mgp_csr_t* L, const float* X, int C, float* Y, int reps, float* elapsed_ms,
                    void* stream);

/* L @ X in the three flavours of graph_laplacian_operator.py:108-124:
 * mode 0 symmetric, 1 randomwalk (D^-1/2 L_sym D^1/2), 2 randomwalk transposed */
int mgp_laplacian_matmul(const mgp_csr_t* L, const float* dsqrt, const float* dinvsqrt, int mode,
                         const float* X, int C, float* Y, float* work_nc, void* stream);

/* GMRF noise for exact sampling (csrc/sampling.hip, docs/kernels/sampling.md): tau I + L_sym = G G^T with
 * G = [sqrt(tau) I | E], E[a, e] = +sqrt(S_ab dsqrt_b / dsqrt_a), E[b, e] = -sqrt(S_ab dsqrt_a / dsqrt_b) for the
 * undirected edge e = (a < b).  Writes Y [n, S] row-major = node_coef w_tag (+ E w_edge when with_edges), the noise of
 * global sample index sample_offset + j in column j: Philox4x32-10 keyed on seed, node counter (i, 0, s >> 2, tag), edge
 * counter (a, b, s >> 2, 1), Box-Muller on the output words.  L: the natural-order CSR of mgp_laplacian_build (row and
 * column ids are the noise keys; entries with col == row or S_ij == 0 are skipped); tiles are not read.  Deterministic,
 * no atomics.  MGP_ERR_ARG for S < 1, null pointers, n >= 2^31, tag < 0, sample_offset < 0. */
int mgp_gmrf_noise(const mgp_csr_t* L, const float* dsqrt, float node_coef, int tag, int with_edges,
                   uint64_t seed, int64_t sample_offset, int S, float* Y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Precision-side operator family, applied matrix-free as a chain of fused SpMMs:
 *   Q2  = scale * diag(post) (tau I + L_sym)^nu diag(pre)          tau = 2 nu / kappa^2
 *         - symmetric normalisation: pre = post = NULL
 *           (PrecisionMaternOperator._matmul, precision_matern_operator.py:26-37)
 *         - random walk: pre = post = sqrt(D), because
 *           D (tau I + L_rw)^nu = D^1/2 (tau I + L_sym)^nu D^1/2   (same file, :36-37)
 *         - scale = outputscale or 1/outputscale (ScaleWrapperOperator,
 *           scale_wrapper_operator.py:27)
 *         - a 0/1 mask multiplied into pre / post gives the MaskedLinearOperator blocks
 *           Q_ll, Q_lu, Q_ul, Q_uu of schur_complement_operator.py:26-30 on full-length
 *           zero-padded vectors
 *   A   = form 0: Q2
 *         form 1: Q2 - s Q2^2 + s^2 Q2^3   (NoiseWrapperOperator, noise_wrapper_operator.py:22,
 *                                           evaluated as Q2(v - s Q2(v - s Q2 v)))
 *         form 2: I + s Q2                 ((K + s I) in precision form with K = Q2^-1:
 *                                           K (K + s I)^-1 y = (I + s Q2)^-1 y)
 *         form 3: diag(w) + s Q2           w = obs_w >= 0: observation precisions relative to the reference noise s
 *                                           (w_i = s / sigma_i^2 on observed nodes, 0 elsewhere).  The GMRF posterior
 *                                           on a subset of nodes / with per-node noise: precision P = Q2 + W / s,
 *                                           mean (W + s Q2)^-1 W y; form 2 is w = 1 (docs/kernels/sampling.md).
 *                                           Evaluated in the epilogue of the chain's last SpMM (w_i X_i + s Q2 X).
 * obs_w is read ONLY when form == 3 (a caller built against the struct without it never has it read); form 3 with
 * obs_w == NULL is MGP_ERR_ARG.  The weights live on the device and are not validated (the Python layer does).
 * Form 3 is supported by: mgp_operator_apply / _apply_dot / _jacobi, the single-GPU CG (mgp_cg_solve, mgp_cg_plan_*
 * incl. refinement and rebind; never the complex-shift or init-free starts), the Lanczos tridiagonalisations
 * (mgp_lanczos_tridiag, mgp_lanczos_tridiag_block: A is SPD).  MGP_ERR_UNSUPPORTED from the row-partitioned and
 * distributed paths: mgp_operator_apply_part, mgp_cg_plan_create_dist, mgp_pcg_plan_create. */
typedef struct {
  mgp_csr_t L;
  const float* pre;   /* nullable [n] */
  const float* post;  /* nullable [n] */
  int32_t nu;
  float kappa;        /* lengthscale */
  float scale;        /* 1 = none */
  int32_t form;       /* 0, 1, 2, 3 above */
  float noise;        /* s */
  const float* obs_w; /* form 3 only: [n] non-negative observation weights w (device); not read for forms 0-2 */
} mgp_operator_t;

size_t mgp_operator_workspace_bytes(const mgp_operator_t* op, int C);
int mgp_operator_apply(const mgp_operator_t* op, const float* X, int C, float* Y, void* work,
                       size_t work_bytes, void* stream);
/* as above, additionally writing per-workgroup partials of dotw . Y (used by CG/Lanczos) */
int mgp_operator_apply_dot(const mgp_operator_t* op, const float* X, int C, float* Y,
                           const float* dotw, float* dot_partials, void* work, size_t work_bytes,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * (Preconditioned) conjugate gradients on A x = b, multi right-hand side, single-reduction
 * (Chronopoulos-Gear) recurrence, whole iterations captured in a hipGraph.
 * Replaces linear_operator.utils.linear_cg as reached from
 * precision_matern_operator.py:53 (`inv_quad_logdet`), schur_complement_operator.py:28
 * (`.solve`) and train_model.py:68.
 *   B [n,C] rhs, X [n,C] solution (in: ignored, start from 0), minv (nullable) Jacobi 1/diag(A)
 *   stop: mode 0 = linear_cg's rule (rhs columns normalised; >= min_iter(10) iterations; stop
 *         when the mean over columns of ||r||_2 < tol; columns with ||r|| < 1e-10 freeze),
 *         mode 1 = every column ||r||_2 <= tol * ||b||_2
 *   out (host): iters, resid[C] relative residual norms (recurrence residual).
 * A solve that needs k steps is ONE hipGraph launch (cg_init + k x (operator apply, fused update);
 * the rhs pointer is patched into the graph, its length follows the previous solves).  The call
 * returns when the stopping decision has reached the host (host-mapped flag); X is complete in
 * stream order: consume it on `stream` or synchronise before reading it from elsewhere. */
typedef struct {
  float tol;
  int32_t max_iter;
  int32_t min_iter;
  int32_t stop_mode;
  int32_t check_every; /* iterations per graph launch / host convergence poll (0 = default) */
  int32_t use_graph;   /* 1 = hipGraph replay (default), 0 = eager launches */
  int32_t max_refine;  /* stop_mode 1 only: iterative-refinement rounds on the TRUE residual B - A x
                          (0 = off); `resid` then reports true relative residuals.  A refined solve stops (status 1)
                          once every true relative residual is <= 2 tol: the fp32 evaluation of B - A x scatters by about
                          that factor around the tolerance */
} mgp_cg_params_t;

/* what a plan on (op, C) carves from `work` (csrc/cg_policy.h: cg_carve), plus slack; 0 for arguments a plan would refuse */
size_t mgp_cg_workspace_bytes(const mgp_operator_t* op, int C);
/* ---- Lab-only switches (every mgp_*_set_* in this header): process-wide words for A/B measurements and tests (std::atomic<int>;
 * the CG family's seven are the plain ints of one struct, CgKnobs in csrc/cg_policy.h).
 * The SpMM family reads them once per call, into the plan value that the call passes down; the CG
 * switches are read at plan creation (mgp_cg_set_poll_spin: once per chunk of a solve); the kernel-block switch once per call; the k-NN / eigensolver switches where a call
 * branches on them.  They are not part of the path's contract and are not meant to be flipped while another thread is inside a
 * call of the same family: two calls that size and launch the same product (mgp_spmm_dot_blocks_csr, then mgp_spmm_fused; the
 * k-NN workspace query, then the search) must see the same setting. */
/* C == 1 plans: the LAST update launch of a plan's first graph also takes the stopping decision of the step behind it and
 * leaves the end-of-graph mark, instead of a single-workgroup decision launch + a marker launch behind it.  Hand-off inside the
 * launch (no release / acquire fence -- a fence writes back every dirty L2 line of the vectors the launch has just stored, measured
 * +3.4 us per solve): lane 0 of every workgroup stores its ||r||^2 partial with a write-through (sc1) relaxed agent-scope atomic
 * store, drains it (s_waitcnt vmcnt(0)) and makes one returning relaxed agent-scope atomic add on its group's arrival counter
 * (two levels: eight groups, one top word); the workgroup whose add completes the count reads all partials with sc1 relaxed
 * agent-scope atomic loads, sums them in the decision kernel's order and takes the decision (MI355X_MICROARCH.md, inter-workgroup
 * visibility: sc1 stores reach the shared level before vmcnt retires them, sc1 loads miss the non-coherent levels).  Same sums in
 * the same order, same rule, same flags: bit-identical to the separate launches (tests/test_gpu_parity.py::
 * test_cg_decide_in_update_matches_separate_launches).  Default 1; 0 = the separate launches; returns the previous setting; read
 * at plan creation. */
int mgp_cg_set_decide_in_update(int on);
/* Complex-shift solve (round 5).  C == 1 plans on A = I + s Q2 (form 2) with nu = 2 and no pre / post vectors (symmetric
 * normalisation), stop_mode 1, no preconditioner: A = I + c B^2 = (I + i sigma B)(I - i sigma B) with B = tau I + L_sym,
 * c = noise * scale, sigma = sqrt(c), and x = Re[(I + i sigma B)^-1 b].  The plan then runs COCG (the CG recurrences with the
 * unconjugated bilinear form) on the complex symmetric system, whose condition is ~sqrt(cond(A)): ONE product with B (the
 * 4-column tile SpMM over (re, im, re, im)) per iteration and about the square root of CG's iteration count -- 1M-node swiss
 * roll: 58 iterations against 688 of two SpMVs each.  `iters` counts COCG iterations, `resid` is the relative norm of the
 * COMPLEX residual (refined solves report the true residual of A x = b as before).  The reference's call is the unpreconditioned
 * linear_cg of precision_matern_operator.py:53 / riemann_gp.py:45-75 on the same system.
 * mgp_cg_set_complex_shift(0): CG on A as in rounds 1-4 (A/B runs, tests, the in-solve SpMV profile); returns the previous
 * setting; read at plan creation.  mgp_cg_plan_is_complex_shift: 1 when the plan took that form. */
int mgp_cg_set_complex_shift(int on);
int mgp_cg_plan_is_complex_shift(void* plan);
/* Folded CG step (round 6).  C == 1 plans with nu = 2, form 0 or 2, no preconditioner, ONE vector P as pre and post (op->pre ==
 * op->post as pointers: sqrt(D) of the random-walk normalisation, or both NULL), on the 64-row tile SpMV with the init-free
 * start: A = [I +] c P B^2 P and u = r give u . A u = [gamma +] c |B P u|^2, which the FIRST SpMV of the apply can sum
 * (t = B P u is its output).  Every scalar of the step is then known when the second SpMV starts, and the row-local update
 * (s, p, x, r, pre (.) r, the partials of the new ||r||^2) runs in its epilogue, in the lane that holds (A u)_i: a step is two
 * launches, spmv_tile_kernel<.., true> and spmv_tile_cgstep_kernel, with no update launch.  Every other plan keeps the
 * (apply, update) launches.  Every SpMV workgroup of the step kernel re-reduces the step's partials, so the gain is for graphs
 * of up to 1024 SpMV workgroups (65,536 nodes; measured at 60k: 54.0 -> 48.2 us per 3-step solve) and turns into a loss
 * beyond (300k nodes, 2345 workgroups: 34.3 -> 36.7 us per iteration).  1 (default) = up to 1024 workgroups; 2 = wherever the
 * shape allows (tests, A/B runs); 0 = the update launches everywhere; returns the previous setting; read at plan creation.
 * mgp_cg_plan_is_folded: 1 when the plan took that form. */
int mgp_cg_set_fold_update(int on);
int mgp_cg_plan_is_folded(void* plan);
/* Plans with more than 16 columns sum the dot-product partials of a step ONCE (cg_reduce_kernel, one small launch
 * ahead of the update) instead of in every workgroup of the update kernel.  Default 1; 0 = the every-workgroup
 * scheme at any C (A/B measurements, tests); affects plans created afterwards. */
int mgp_cg_set_reduce_once(int on);
/* Plans whose column count is a multiple of four (the 12 probes, the 32 / 100 one-hot columns of training) run their vector update
 * on float4 streams (cg_update_q_kernel: a lane owns a column QUAD of a row, every access a dwordx4; cg_update_kernel gives a lane
 * one element and idles tile_cols(C) - C lanes of every row).  Default 1; 0 = the element form at every column count (A/B runs,
 * tests); read at plan creation. */
int mgp_cg_set_update_quads(int on);
/* The host learns of the end of a solve from a host-mapped word the deciding kernel writes.  While the first graph of
 * a plan runs -- it is sized to end in the stopping decision -- the host reads only that word, for up to twice the
 * time the previous solve took (`spins` reads between two looks at the clock, default 64); hipStreamQuery, the guard
 * against a chunk that ends undecided, comes after that window and for continuation chunks.  0: no window, one
 * query per read as in round 1. */
int mgp_cg_set_poll_spin(int spins);
/* C == 1 plans on the tile SpMV without a preconditioner start WITHOUT a cg_init launch: the first operator apply
 * reads the right-hand side itself, copies it to r and leaves ||b||^2 as partials; the first update treats p, s, x
 * as zero.  One launch (~3.8 us at N = 60k) less per solve.  Default 1; 0 restores the classic start (plans created
 * afterwards). */
int mgp_cg_set_init_free(int on);
/* reusable solver: owns the captured iteration graph; `work` must outlive the plan */
int mgp_cg_plan_create(const mgp_operator_t* op, int C, const float* minv,
                       const mgp_cg_params_t* params, void* work, size_t work_bytes, void* stream,
                       void** plan_out);
int mgp_cg_plan_solve(void* plan, const float* B, float* X, int32_t* iters, float* resid,
                      int32_t* status); /* status 1 converged, 2 max_iter, 3 breakdown (NaN) */
/* Point an existing single-GPU plan at another operator of the SAME structure -- same sizes, tile / dense-tile layouts, nu, form,
 * the same of pre / post / minv present --, e.g. the same graph at the next epoch's bandwidth and length scale (the reference
 * rebuilds its operators every epoch, train_model.py:63-67; a fresh plan costs ~0.9 ms of host time between its creation, its
 * first eager solve, the capture at its second and its destruction).  Pointers and scalars may all differ.  The workspace, the
 * host-mapped flags and the executable graphs are kept: the next solve records its launches again and updates the graphs in
 * place (hipGraphExecUpdate).  MGP_ERR_UNSUPPORTED when the structure differs (create a new plan), for distributed plans, and for a
 * complex-shift plan whose new operator no longer factorises.  The old operator's arrays are not touched after this call. */
int mgp_cg_plan_rebind(void* plan, const mgp_operator_t* op, const float* minv);
float* mgp_cg_plan_x(void* plan);    /* device pointer of the plan's own solution buffer [n,C]; pass
                                         X = NULL to mgp_cg_plan_solve to skip the copy into X */
/* refined solves (max_refine > 0, single GPU) accumulate the solution in float64 and form the true residual
 * from it; the float32 buffer above holds its rounding.  Device pointer of that float64 solution [n,C]
 * (valid after a refined solve, until the next solve); NULL for a distributed plan. */
double* mgp_cg_plan_x64(void* plan);
/* operator applies the last solve actually ran (refinement off).  A plan's first graph is captured for the
 * step count its previous solves needed; for C = 1 its last step -- the one that would only notice
 * ||r|| <= tol after running one more apply for nothing -- is a single-workgroup decision launch, so a
 * solve that takes k iterations runs k applies, not k + 1.  Same iterates, residuals and flags. */
int mgp_cg_plan_last_applies(void* plan);
int mgp_cg_plan_destroy(void* plan);
/* 1 after a solve of this plan returned MGP_ERR_TIMEOUT (a dead peer / hung collective of a multi-rank job): kernels and
 * collectives that reference the plan's buffers are still queued, so the plan is POISONED -- further solves return
 * MGP_ERR_TIMEOUT at once and mgp_cg_plan_destroy frees and synchronises nothing (the memory is leaked on purpose; the
 * caller must keep the workspace alive and exit non-zero). */
int mgp_cg_plan_poisoned(void* plan);
int mgp_cg_plan_poison(void* plan);     /* mark it so by hand: the caller has learnt by other means that a peer rank is gone */
int mgp_cg_solve(const mgp_operator_t* op, const float* B, int C, float* X, const float* minv,
                 const mgp_cg_params_t* params, int32_t* iters, float* resid, void* work,
                 size_t work_bytes, void* stream);
/* cheap Jacobi preconditioner: minv_i = 1 / A_ii with the polynomial's off-diagonal
 * contributions to the diagonal ignored for nu > 2 (exact for nu <= 2, forms 0 / 2 / 3; entries with col == row, the self
 * edges of a graph with coincident points, count as part of the row's diagonal: A_ii = tau + diag_i - sum S_ii) */
int mgp_operator_jacobi(const mgp_operator_t* op, float* minv, void* stream);

/* The operator in float64 from the float32 matrix: Y = A X for X, Y [n,C] float64 (device, X != Y), every product and sum of
 * the chain in float64 (the kernels behind the true residual of the refined CG solves).  Reads the natural-order CSR only.
 * For callers that need A x to the rounding of its result, not of the chain: with tau I + L_sym applied nu times in float32 a
 * smooth x loses up to a few thousand float32 roundings against A x (docs/kernels/classification.md).
 * work: mgp_operator_apply_double_workspace_bytes(op, C) bytes (4 n C doubles), 8-byte aligned; MGP_ERR_WORKSPACE otherwise. */
size_t mgp_operator_apply_double_workspace_bytes(const mgp_operator_t* op, int C);
int mgp_operator_apply_double(const mgp_operator_t* op, const double* X, int C, double* Y, void* work, size_t work_bytes,
                              void* stream);

/* Marginal posterior variances in precision form (csrc/variance.hip, docs/kernels/sampling.md "Marginal variances"): the two
 * kernels of the single-site Rao-Blackwell estimator  var_i = s / d_i + E[(delta_i - p_i / d_i)^2],  d = diag(W + s Q2).
 *
 * The EXACT diagonal of operator forms 0 (q_i), 2 (1 + s q_i) and 3 (w_i + s q_i), q_i = scale pre_i post_i diag((tau I + L_sym)^nu)_i,
 * for nu = 1, 2, 3 in float64: diag_out [n] (device).  nu = 3 counts the triangles through every node (a wave per row, the row's
 * own entries in LDS); the Jacobi routine above keeps its pure diagonal power there.  Reads the natural-order CSR only (rowptr, col,
 * vals, diag; no tiles), pre / post and, for form 3, obs_w; the CSR is taken as symmetric (S_ji = S_ij, as the graph builders
 * write it); entries with col == row or S_ij == 0 are skipped as in the GMRF noise routine; a row's columns may come in any
 * order.  Products and sums in float64 from the float32 values; tau, scale and s enter as the doubles of the struct's floats.
 * Deterministic, no atomics.  The kernel needs no scratch today: the workspace query returns 0 and `work` may be NULL (the
 * pair is there so that a later layout can take one without a new signature).
 * MGP_ERR_UNSUPPORTED for nu > 3 and form 1; MGP_ERR_ARG for null pointers, form 3 without obs_w and n >= 2^31. */
size_t mgp_operator_diag_exact_workspace_bytes(const mgp_operator_t* op);
int mgp_operator_diag_exact(const mgp_operator_t* op, double* diag_out, void* work, size_t work_bytes, void* stream);
/* Row moments of a block of samples: for every row i of the row-major float32 blocks U, V, Pm [n, C], 1 <= C <= 256,
 *   u_c = U_ic - (Pm ? Pm_ic rdiag_i : 0),  v_c likewise from V (V == NULL or V == U: v = u),
 *   acc[i, 0] += sum_c u_c v_c,   acc[i, 1] += sum_c (u_c v_c)^2,
 * all arithmetic in float64.  acc [n, 2] float64 is read-modify-written: the chunks of a larger sample count add into one
 * state, which the caller zeroes first.  rdiag [n] float64 (read only with Pm).  U == V, Pm == NULL: the plain second and
 * fourth moments; distinct U and V: cross moments.  A lane group per row, float4 loads where C % 4 == 0 and the blocks are
 * 16-byte aligned, scalar loads otherwise; fixed reduction tree, one lane writes: deterministic.
 * MGP_ERR_ARG for C < 1, C > 256, n < 1, null U or acc, Pm without rdiag. */
int mgp_row_moments(const float* U, const float* V, const double* rdiag, const float* Pm, int64_t n, int C, double* acc,
                    void* stream);

/* Laplace approximation for 0/1 labels with a Bernoulli-logit likelihood (csrc/laplace.hip, docs/kernels/classification.md):
 * the two per-node kernels of classification.laplace_fit.
 *
 * The likelihood stage of one Newton step.  f [n] latent values, qf [n] = Q2 f (NULL: zeros, the start at f = 0), y [n]
 * labels (class 1 where y > 0.5; read at observed nodes only, NaN allowed elsewhere), obs [n] bytes (non-zero: observed; NULL:
 * every node), all on the device.  Per node in float64 from the float32 inputs, with t in {0, 1}, a = (2 t - 1) f, e = exp(-|f|):
 *   log p = min(a, 0) - log1p(e),   pi = f >= 0 ? 1 / (1 + e) : e / (1 + e),   g = t - pi,   h = e / (1 + e)^2
 * (g = h = 0 at unobserved nodes), and
 *   w_i = (float)(s_ref h_i),   rhs_i = (float)(s_ref (g_i - qf_i)),
 *   sums [4] float64 (device) = { sum_obs log p,  sum_i f_i qf_i,  max_i |g_i - qf_i|,  sum_i (g_i - qf_i)^2 }.
 * w is the obs_w of operator form 3 with noise = s_ref, rhs the Newton right-hand side; finite for any finite f (|f| = 1e4:
 * log p = -1e4, h = 0).  The sums go through one partial per workgroup and a second launch that adds the partials: fixed order,
 * no atomics, repeated calls are bitwise equal.  `work`: mgp_bernoulli_site_workspace_bytes(n) bytes, 8-byte aligned.
 * float4 loads and stores where f, qf, y, w, rhs are 16-byte and obs 4-byte aligned, scalar ones otherwise.
 * link: 0 = logit; any other MGP_ERR_UNSUPPORTED.  MGP_ERR_ARG for null f, y, w, rhs or sums and n < 1; MGP_ERR_WORKSPACE for
 * a null, misaligned or short `work`. */
size_t mgp_bernoulli_site_workspace_bytes(int64_t n);
int mgp_bernoulli_site(const float* f, const float* qf, const float* y, const uint8_t* obs, int64_t n, double s_ref, int link,
                       float* w, float* rhs, double* sums, void* work, size_t work_bytes, void* stream);
/* Predictive class probability  prob_i = int sigma(mean_i + sqrt(var_i) u) phi(u) du  by the `points`-point trapezoid rule
 * on [-8, 8]: sum_k D phi(u_k) sigma(mean_i + sqrt(var_i) u_k), u_k = -8 + k D, D = 16 / (points - 1), k ascending, all in
 * float64 (classification.md has the rule's error against 30-digit quadrature).  mean [n] float32, var [n] float64, prob [n]
 * float64, on the device.  var < 0 counts as 0 (prob = sigma(mean)); NaN in mean or var gives NaN; prob <= 1.
 * MGP_ERR_ARG for null pointers, n < 1 and points even or outside 9 .. 1025. */
int mgp_bernoulli_predict(const float* mean, const double* var, int64_t n, int points, double* prob, void* stream);

/* Counts at the nodes (csrc/laplace.hip, docs/kernels/counts.md): the likelihood stage of one Newton step of
 * counts.laplace_fit_counts, with the contract of mgp_bernoulli_site.  f, qf (NULL: zeros), obs (NULL: every node) as there;
 * y [n] counts and aux [n] are read at observed nodes only (NaN allowed elsewhere).  Per observed node in float64 from the
 * float32 inputs, eta = f + mean + (family 0 ? aux : 0):
 *   family 0, Poisson, aux = log-exposure (NULL: zeros):
 *     mu = exp(min(eta, 700)),   l = y eta - mu,   g = y - mu,   h = mu       (-lgamma(y + 1) is left to the caller)
 *   family 1, binomial, aux = trials N (NULL: MGP_ERR_ARG), e = exp(-|eta|), d = 1 + e:
 *     pi = eta >= 0 ? 1 / d : e / d,   1 - pi = eta >= 0 ? e / d : 1 / d,
 *     l = -(N - y)(max(eta, 0) + log1p(e)) - y (max(-eta, 0) + log1p(e)),   g = y (1 - pi) - (N - y) pi,   h = N e / d^2
 *                                                                             (log C(N, y) is left to the caller)
 * (g = h = 0 at unobserved nodes), and
 *   w_i = (float)(s_ref h_i),   rhs_i = (float)(s_ref (g_i - qf_i)),   both saturated at +-FLT_MAX,
 *   sums [4] float64 (device) = { sum_obs l,  sum_i f_i qf_i,  max_i |g_i - qf_i|,  sum_i (g_i - qf_i)^2 }.
 * For finite inputs with |f| <= 1e4 and counts <= 2^24 the first three sums are finite term by term; the fourth may be +inf.
 * One partial per workgroup and a second launch that adds them: fixed order, no atomics, repeated calls are bitwise equal.
 * `work`: mgp_count_site_workspace_bytes(n) bytes, 8-byte aligned.  float4 / uchar4 accesses where f, qf, y, aux, w, rhs
 * are 16-byte and obs 4-byte aligned, scalar ones otherwise.  MGP_ERR_ARG for null f, y, w, rhs or sums and n < 1;
 * MGP_ERR_UNSUPPORTED for any other family; MGP_ERR_WORKSPACE for a null, misaligned or short `work`.  The checks precede
 * every launch. */
size_t mgp_count_site_workspace_bytes(int64_t n);
int mgp_count_site(const float* f, const float* qf, const float* y, const float* aux, const uint8_t* obs, int64_t n,
                   double s_ref, double mean, int family, float* w, float* rhs, double* sums, void* work, size_t work_bytes,
                   void* stream);
/* Overdispersed counts (csrc/laplace.hip, docs/kernels/counts.md): the likelihood stage of one Newton step of
 * counts.laplace_fit_counts(family="negative_binomial"), y_i ~ NB(mean mu_i = E_i exp(f_i + mean), dispersion r),
 * Var y = mu + mu^2 / r, with the contract of mgp_count_site.  f, qf (NULL: zeros), obs (NULL: every node) as there; y [n] counts
 * and aux [n], the float32 log-exposure (NULL: zeros), are read at observed nodes only (NaN allowed elsewhere).  dispersion: one
 * finite scalar in [2^-10, 2^20].  Per observed node in float64 from the float32 inputs, z = f + mean + aux - log r (so that
 * pi = sigma(z) = mu / (r + mu)), e = exp(-|z|), d = 1 + e:
 *     pi = z >= 0 ? 1 / d : e / d,   1 - pi = z >= 0 ? e / d : 1 / d,
 *     l = -r (max(z, 0) + log1p(e)) - y (max(-z, 0) + log1p(e)),   g = y (1 - pi) - r pi,   h = (y + r) e / d^2,
 *     0 < h <= (y + r) / 4      (c(y, r) = lgamma(y + r) - lgamma(r) - lgamma(y + 1) is left to the caller)
 * the binomial arithmetic of mgp_count_site with y + r trials and r failures at a shifted predictor: no exp of an unclamped
 * argument, nothing saturates for finite inputs.  (g = h = 0 at unobserved nodes), and
 *   w_i = (float)(s_ref h_i),   rhs_i = (float)(s_ref (g_i - qf_i)),   both saturated at +-FLT_MAX,
 *   sums [4] float64 (device) = { sum_obs l,  sum_i f_i qf_i,  max_i |g_i - qf_i|,  sum_i (g_i - qf_i)^2 }.
 * For finite inputs with |f| <= 1e4 and counts <= 2^24 the first three sums are finite term by term; the fourth may be +inf.
 * One partial per workgroup and a second launch that adds them: fixed order, no atomics, repeated calls are bitwise equal.
 * `work`: mgp_nb_site_workspace_bytes(n) bytes, 8-byte aligned.  float4 / uchar4 accesses where f, qf, y, aux, w, rhs
 * are 16-byte and obs 4-byte aligned, scalar ones otherwise.  MGP_ERR_ARG for null f, y, w, rhs or sums, n < 1 and a dispersion
 * outside [2^-10, 2^20] (NaN included); MGP_ERR_WORKSPACE for a null, misaligned or short `work`.  The checks precede every
 * launch. */
size_t mgp_nb_site_workspace_bytes(int64_t n);
int mgp_nb_site(const float* f, const float* qf, const float* y, const float* aux, const uint8_t* obs, int64_t n, double s_ref,
                double mean, double dispersion, float* w, float* rhs, double* sums, void* work, size_t work_bytes, void* stream);

/* Ordered categories at the nodes (csrc/laplace.hip, docs/kernels/ordinal.md): the likelihood stage of one Newton step of
 * ordinal.laplace_fit_ordinal, a cumulative-logit model with one latent function, with the contract of mgp_bernoulli_site.
 * f, qf (NULL: zeros), obs (NULL: every node) as there; lo [n] and hi [n] are the float32 ends of the node's interval of
 * cutpoints, lo < hi, -inf and +inf allowed (the end categories); read at observed nodes only (NaN allowed elsewhere).  The
 * kernel sees intervals, never labels: no table is indexed.  Per observed node in float64 from the float32 inputs, with
 * u = hi - f, l = lo - f, logsig(x) = -(max(-x, 0) + log1p(exp(-|x|))) and sigma(x) = 1 / (1 + e) (x >= 0), e / (1 + e) (x < 0),
 * e = exp(-|x|):
 *   P(y | f) = sigma(u) - sigma(l) = sigma(u) sigma(-l) (1 - exp(-(hi - lo)))                  (no cancellation)
 *   log p = logsig(u) + logsig(-l)            (log(-expm1(-(hi - lo))) does not depend on f and is left to the caller)
 *   g = sigma(l) - sigma(-u),   h = e_u / (1 + e_u)^2 + e_l / (1 + e_l)^2,   0 < h <= 1/2
 * (g = h = 0 at unobserved nodes), and
 *   w_i = (float)(s_ref h_i),   rhs_i = (float)(s_ref (g_i - qf_i)),
 *   sums [4] float64 (device) = { sum_obs log p,  sum_i f_i qf_i,  max_i |g_i - qf_i|,  sum_i (g_i - qf_i)^2 }.
 * Finite for any finite f and any lo < hi, infinite ends included.  One partial per workgroup and the second launch of
 * mgp_bernoulli_site: fixed order, no atomics, repeated calls are bitwise equal.  `work`: mgp_ordinal_site_workspace_bytes(n)
 * bytes, 8-byte aligned.  float4 / uchar4 accesses where f, qf, lo, hi, w, rhs are 16-byte and obs 4-byte aligned, scalar ones
 * otherwise.  MGP_ERR_ARG for null f, lo, hi, w, rhs or sums and n < 1; MGP_ERR_WORKSPACE for a null, misaligned or short `work`.
 * The checks precede every launch. */
size_t mgp_ordinal_site_workspace_bytes(int64_t n);
int mgp_ordinal_site(const float* f, const float* qf, const float* lo, const float* hi, const uint8_t* obs, int64_t n,
                     double s_ref, float* w, float* rhs, double* sums, void* work, size_t work_bytes, void* stream);
/* The predictive probabilities of the K ordered categories, 2 <= K <= 64, under a Gaussian latent marginal:
 *   out [n, K] row-major,   out_ik = int P(y = k | f) N(f; eta_i, var_i) df,
 * by the `points`-point trapezoid rule of mgp_bernoulli_predict, u_j = -8 + j D, D = 16 / (points - 1), f_j = eta_i + sqrt(var_i) u_j,
 * weights D phi(u_j), j ascending, all in float64, with the integrand in the product form
 *   c_k sigma(b_{k+1} - f_j) sigma(f_j - b_k),   c_k = -expm1(-(b_{k+1} - b_k)),
 * one factor and c = 1 for an end category (b_0 = -inf, b_K = +inf): every term is positive, so a tail category keeps its
 * relative accuracy.  The sum is divided by the sum of the weights, so a row sums to 1 up to rounding at every `points` (the
 * weights of 9 points sum to 1.014, those of 65 and more to 1 - 1.3e-15).  cuts [K - 1] float64 on the device, strictly
 * increasing (not validated here); eta, var [n] float64.  var <= 2^-76 (zero and negative variances included) gives the plain
 * probability at eta; NaN in eta or var gives a row of NaN.  log_out non-zero: the logarithm of the same number (-inf where it
 * underflows).  A group of TK lanes (the least power of two >= K) per node, lane k its category.  No workspace, no atomics:
 * repeated calls are bitwise equal.  Element alignment only.  MGP_ERR_ARG for null eta, var, cuts or out, n < 1, K outside
 * 2 .. 64 and points even or outside 9 .. 1025.  The checks precede the launch. */
int mgp_ordinal_predict(const double* eta, const double* var, const double* cuts, int64_t n, int K, int points, int log_out,
                        double* out, void* stream);

/* The predictive pmf of a count fit (csrc/count_predict.hip, docs/kernels/count_predict.md): per node and count k,
 *   pmf(k) = (2 pi v)^-1/2 int exp(g(x)) dx,   Poisson   g = k (x + a) - exp(x + a) - lgamma(k + 1) - (x - m)^2 / 2v,
 *                                              binomial  g = log C(N, k) - k softplus(-x) - (N - k) softplus(x) - (x - m)^2 / 2v,
 * with m = eta_i (the linear predictor at the mode WITHOUT the exposure, float64), v = var_i (float64) and aux as
 * mgp_count_site: the float32 log-exposure a (family 0; NULL: zeros) or the float32 trials N (family 1; NULL: MGP_ERR_ARG).
 * The quadrature is placed per (node, k), all in float64: the mode x* of g by a safeguarded Newton iteration, a window
 * [x* - t_L, x* + t_R] at whose ends g has dropped by 40 (doubling from (-g''(x*))^-1/2, six bisections), and the `points`-point
 * trapezoid rule of exp(g(x* + t) - g(x*)) there, t ascending, the difference formed without cancellation;
 * log pmf = g(x*) + log(h sum / sqrt(2 pi v)).  v <= 2^-76 (zero and negative variances included) is the plain log pmf at
 * x = m; k > N gives pmf 0 (log: -inf); NaN in eta, var or y gives NaN.  exp(x + a) is taken at min(x + a, 700).
 * mgp_count_predict_pmf writes the counts k0 .. k0 + K - 1 of every node to out [n, K] row-major: the pmf, or its log when
 * log_out is non-zero; 1 <= K <= 65536, 0 <= k0, k0 + K - 1 <= 2^24.  A wave per (node, 64 counts).
 * mgp_count_predict_logpmf writes the log pmf of the one count y_i (a float32 integer in [0, 2^24], not validated) per node to
 * out [n]; y is read only where `at` [n] bytes is non-zero (NULL: every node), out is NaN at the other nodes.  It is bitwise
 * the matching entry of mgp_count_predict_pmf with log_out.
 * points: odd, 17 .. 257.  No workspace, no atomics: repeated calls are bitwise equal.  Element alignment only.
 * MGP_ERR_ARG for null eta, var, out (y), n < 1, K, k0 or points out of range and family 1 without aux; MGP_ERR_UNSUPPORTED for
 * any other family.  The checks precede every launch. */
int mgp_count_predict_pmf(const double* eta, const double* var, const float* aux, int64_t n, int family, int64_t k0, int K,
                          int points, int log_out, double* out, void* stream);
int mgp_count_predict_logpmf(const double* eta, const double* var, const float* aux, const float* y, const uint8_t* at,
                             int64_t n, int family, int points, double* out, void* stream);
/* The predictive pmf of a negative-binomial fit (csrc/count_predict.hip, docs/kernels/count_predict.md): per node and count k,
 *   pmf(k) = (2 pi v)^-1/2 int exp(g(x)) dx,   g = c(k, r) - k softplus(-z) - r softplus(z) - (x - m)^2 / 2v,   z = x + a - log r,
 *   c(k, r) = lgamma(k + r) - lgamma(r) - lgamma(k + 1),
 * with m = eta_i (the linear predictor at the mode WITHOUT the exposure, float64), v = var_i (float64), a the float32
 * log-exposure aux_i (NULL: zeros) and r = dispersion, one finite scalar in [2^-10, 2^20].  In the variable z this is the binomial
 * integrand of mgp_count_predict_pmf with k + r in the place of N, r in the place of N - k and m + a - log r in the place of m, and
 * the same rule runs on it, all in float64: the mode x* by the safeguarded Newton iteration (bracket: m and log k - a for k > 0,
 * m - v r and m for k = 0; a step that leaves the bracket or does not halve the last one is a bisection), the window at whose ends
 * g has dropped by 40, and the `points`-point trapezoid rule of exp(g(x* + t) - g(x*)), t ascending, the difference formed
 * without cancellation; log pmf = g(x*) + log(h sum / sqrt(2 pi v)).  There is no upper end of the count range.  c(k, r) is formed
 * from terms of the size of the result: sum_{j < k} log((r + j) / (j + 1)) for k < 32, beyond it Stirling's formula with the two
 * leading terms of lgamma(k + r) and of the larger of lgamma(r), lgamma(k + 1) combined through log1p (count_predict.md has the
 * error).  v <= 2^-76 (zero and negative variances included) is the plain log pmf at x = m; NaN in eta, var or y gives NaN.
 * mgp_nb_predict_pmf writes the counts k0 .. k0 + K - 1 of every node to out [n, K] row-major: the pmf, or its log when
 * log_out is non-zero; 1 <= K <= 65536, 0 <= k0, k0 + K - 1 <= 2^24.  A wave per (node, 64 counts).
 * mgp_nb_predict_logpmf writes the log pmf of the one count y_i (a float32 integer in [0, 2^24], not validated) per node to
 * out [n]; y is read only where `at` [n] bytes is non-zero (NULL: every node), out is NaN at the other nodes.  It is bitwise
 * the matching entry of mgp_nb_predict_pmf with log_out.
 * points: odd, 17 .. 257.  No workspace, no atomics: repeated calls are bitwise equal.  Element alignment only.
 * MGP_ERR_ARG for null eta, var, out (y), n < 1, K, k0 or points out of range and a dispersion outside [2^-10, 2^20] (NaN
 * included).  The checks precede every launch. */
int mgp_nb_predict_pmf(const double* eta, const double* var, const float* aux, int64_t n, double dispersion, int64_t k0, int K,
                       int points, int log_out, double* out, void* stream);
int mgp_nb_predict_logpmf(const double* eta, const double* var, const float* aux, const float* y, const uint8_t* at, int64_t n,
                          double dispersion, int points, double* out, void* stream);

/* The Laplace evidence at the mode (csrc/laplace.hip, docs/kernels/evidence.md): the per-node stage of
 * evidence.laplace_evidence.  f [n] the mode, y, aux, obs as mgp_count_site (read in quads that hold an observed node only; NaN
 * allowed elsewhere); family 0 Poisson, 1 binomial, 2 Bernoulli-logit (class 1 where y > 0.5 as mgp_bernoulli_site; aux is not
 * read); var [n] float64 the latent marginal variances diag((Q2 + H)^-1), nullable.  Per observed node in float64 from the float32
 * inputs, eta, l and h as mgp_count_site (family 2: one trial), and h' = dh / df:
 *   Poisson  h' = mu;     binomial, Bernoulli  h' = h ((1 - pi) - pi),  (1 - pi) - pi = -+(-expm1(-|eta|)) / (1 + e)  (- for eta >= 0)
 * and, on the observed nodes with h >= h_floor (0 at every other node),
 *   root_h_i = (float) sqrt(h_i),   corr_i = (float)(var_i h'_i),   both saturated at +-FLT_MAX;
 *   sums [4] float64 (device) = { sum_obs l,  m = nodes kept,  sum_i corr_i,  max_i |corr_i| }   (corr before the float cast).
 * corr is not written, and sums 2 and 3 are 0, when var or corr is NULL.  One partial per workgroup and the second launch of
 * mgp_bernoulli_site: fixed order, no atomics, repeated calls are bitwise equal.  `work`:
 * mgp_laplace_evidence_site_workspace_bytes(n) bytes, 8-byte aligned.  float4 / uchar4 / double2 accesses where f, y, aux,
 * var, root_h, corr are 16-byte and obs 4-byte aligned, scalar ones otherwise.  MGP_ERR_ARG for null f, y, root_h or sums, n < 1,
 * h_floor negative or NaN and family 1 without aux; MGP_ERR_UNSUPPORTED for any other family; MGP_ERR_WORKSPACE for a null,
 * misaligned or short `work`.  The checks precede every launch. */
size_t mgp_laplace_evidence_site_workspace_bytes(int64_t n);
int mgp_laplace_evidence_site(const float* f, const float* y, const float* aux, const uint8_t* obs, const double* var, int64_t n,
                              double mean, int family, double h_floor, float* root_h, float* corr, double* sums, void* work,
                              size_t work_bytes, void* stream);
/* The same stage for a negative-binomial fit with the dispersion r in [2^-10, 2^20] (mgp_nb_site): f, y, aux (the float32
 * log-exposure, NULL: zeros), obs, var as above.  Per observed node in float64, z, pi, l and h as mgp_nb_site, and
 *   h' = dh / df = h ((1 - pi) - pi),  (1 - pi) - pi = -+(-expm1(-|z|)) / (1 + e)  (- for z >= 0),
 * and, on the observed nodes with h >= h_floor (0 at every other node),
 *   root_h_i = (float) sqrt(h_i),   corr_i = (float)(var_i h'_i),   both saturated at +-FLT_MAX;
 *   sums [4] float64 (device) = { sum_obs l,  m = nodes kept,  sum_i corr_i,  max_i |corr_i| }   (corr before the float cast).
 * corr is not written, and sums 2 and 3 are 0, when var or corr is NULL.  One partial per workgroup and the second launch of
 * mgp_bernoulli_site: fixed order, no atomics, repeated calls are bitwise equal.  `work`:
 * mgp_nb_evidence_site_workspace_bytes(n) bytes, 8-byte aligned.  float4 / uchar4 / double2 accesses where f, y, aux, var,
 * root_h, corr are 16-byte and obs 4-byte aligned, scalar ones otherwise.  MGP_ERR_ARG for null f, y, root_h or sums, n < 1,
 * h_floor negative or NaN and a dispersion outside [2^-10, 2^20] (NaN included); MGP_ERR_WORKSPACE for a null, misaligned or
 * short `work`.  The checks precede every launch. */
size_t mgp_nb_evidence_site_workspace_bytes(int64_t n);
int mgp_nb_evidence_site(const float* f, const float* y, const float* aux, const uint8_t* obs, const double* var, int64_t n,
                         double mean, double dispersion, double h_floor, float* root_h, float* corr, double* sums, void* work,
                         size_t work_bytes, void* stream);
/* The derivative of the negative-binomial Laplace evidence with respect to the dispersion r in [2^-10, 2^20], the mean and the
 * exposure held fixed, as three sums over the nodes (docs/kernels/counts.md, "Learning the dispersion"): out [3] float64 (device).
 * f, y, aux (NULL: zeros), obs (NULL: every node) as mgp_nb_evidence_site; var [n] float64 (NULL: row 1 is 0): diag(A^-1); u [n]
 * float64 (NULL: row 2 is 0): A^-1 (var o h').  y, aux, var and u are read only in quads that hold an observed node (NaN allowed
 * elsewhere).  Per observed node in float64, with z, pi, 1 - pi, h and h' as mgp_nb_evidence_site forms them,
 *   row 0:   psi(y + r) - psi(r) + log(1 - pi) + pi - y (1 - pi) / r     the likelihood with d c(y, r) / dr, every observed node
 *   row 1:   -1/2 var (pi (1 - pi) - h' / r)                             the curvature at fixed f, dh / dr
 *   row 2:   -1/2 u (h / r - pi)                                         through the mode, dg / dr = h / r - pi
 * rows 1 and 2 only where h >= h_floor; their sum is d log Z / dr.  log(1 - pi) = -(max(z, 0) + log1p(e)).  The digamma
 * difference is formed from positive terms no larger than itself: sum_{j < y} 1 / (r + j), j ascending, for y <= 32; beyond it,
 * with k = 32 for r < 32 and 0 otherwise, b = r + k, a = y + r and t(x) = 1/12 x^-2 - 1/120 x^-4 + 1/252 x^-6 - 1/240 x^-8 +
 * 1/132 x^-10 - 691/32760 x^-12,
 *   sum_{j < k} 1 / (r + j) + log1p((y - k) / b) + (y - k) / (2 a b) + (t(b) - t(a));
 * y = 0 gives exactly 0; the first sum depends on r alone and is formed once on the host.  The node loop, the partials (one per workgroup, at most 1024) and the second launch are those of
 * mgp_nb_evidence_site: fixed order, no atomics, repeated calls are bitwise equal.  `work`:
 * mgp_nb_dispersion_sums_workspace_bytes(n) bytes, 8-byte aligned.  float4 / uchar4 / double2 accesses where f, y, aux, var, u
 * are 16-byte and obs 4-byte aligned, scalar ones otherwise.  MGP_ERR_ARG for null f, y or out, n < 1, h_floor negative or NaN
 * and a dispersion outside [2^-10, 2^20] (NaN included); MGP_ERR_WORKSPACE for a null, misaligned or short `work`.  The checks
 * precede every launch. */
size_t mgp_nb_dispersion_sums_workspace_bytes(int64_t n);
int mgp_nb_dispersion_sums(const float* f, const float* y, const float* aux, const uint8_t* obs, const double* var,
                           const double* u, int64_t n, double mean, double dispersion, double h_floor, double* out, void* work,
                           size_t work_bytes, void* stream);
/* The same stage for an ordered-category fit (ordinal.laplace_fit_ordinal, docs/kernels/ordinal.md) with the contract of
 * mgp_laplace_evidence_site: lo [n] and hi [n], the float32 ends of the node's interval of cutpoints as mgp_ordinal_site reads
 * them (lo < hi, -inf / +inf at the end categories), in the place of (y, aux); read only in quads that hold an observed node (NaN
 * allowed elsewhere), as var.  Per observed node in float64, with u = hi - f, l = lo - f, e_x = exp(-|x|), a_x = e_x / (1 + e_x)^2
 * and gap_x = sigma(-x) - sigma(x) = -+(-expm1(-|x|)) / (1 + e_x) (- for x >= 0; an infinite end has a = 0 and adds nothing),
 *   l = log sigma(u) + log sigma(-l),   h = a_u + a_l in (0, 1/2],   h' = dh / df = -(a_u gap_u + a_l gap_l);
 * at the observed nodes with h >= h_floor (the m nodes kept; 0 elsewhere)
 *   root_h_i = (float) sqrt(h_i),   corr_i = (float)(var_i h'_i),
 *   sums [4] float64 (device) = { sum_obs l,  m,  sum_i corr_i,  max_i |corr_i| }.
 * corr is not written, and sums 2 and 3 are 0, when var or corr is NULL.  Partials, second launch, vector accesses and `work`
 * (mgp_ordinal_evidence_site_workspace_bytes(n) bytes, 8-byte aligned) as mgp_laplace_evidence_site: repeated calls are bitwise
 * equal.  MGP_ERR_ARG for null f, lo, hi, root_h or sums, n < 1, h_floor negative or NaN; MGP_ERR_WORKSPACE for a null, misaligned
 * or short `work`.  The checks precede every launch. */
size_t mgp_ordinal_evidence_site_workspace_bytes(int64_t n);
int mgp_ordinal_evidence_site(const float* f, const float* lo, const float* hi, const uint8_t* obs, const double* var, int64_t n,
                              double h_floor, float* root_h, float* corr, double* sums, void* work, size_t work_bytes,
                              void* stream);
/* The derivative of the ordinal Laplace evidence with respect to the K - 1 cutpoints, 2 <= K <= 64, as three rows of sums over the
 * observed nodes (docs/kernels/ordinal.md): out [3, K - 1] float64 row-major (device), column k - 1 the cutpoint b_k.  f, lo, hi,
 * obs (NULL: every node) as above; cat [n] uint8: the node's category c (lo = b_c, hi = b_{c+1}); var [n] float64 (NULL: row 1 is
 * 0): diag(A^-1); u [n] float64 (NULL: row 2 is 0): A^-1 (var o h').  lo, hi, cat, var and u are read at observed nodes only; a
 * node with cat >= K adds nothing, and cat is compared, never used as an index.  With w = hi - lo and the notation above, a node
 * of category c adds to column c (its upper cut, c <= K - 2) and to column c - 1 (its lower cut, c >= 1)
 *   row 0:   sigma(-u) + 1 / expm1(w)              -(sigma(l) + 1 / expm1(w))           the likelihood (1 / expm1(inf) = 0)
 *   row 1:   -1/2 var a_u gap_u                     -1/2 var a_l gap_l                    the curvature at fixed f
 *   row 2:   -1/2 u a_u                             -1/2 u a_l                            through the mode
 * rows 1 and 2 only where h >= h_floor.  One partial [3, K - 1] per workgroup, every entry summed in node order by one lane, and
 * a second launch that adds the partials in workgroup order: no atomics, repeated calls are bitwise equal.  `work`:
 * mgp_ordinal_cut_sums_workspace_bytes(n, K) bytes (0 for n < 1 or K outside 2 .. 64), 8-byte aligned.  Element alignment only.
 * MGP_ERR_ARG for null f, lo, hi, cat or out, n < 1, K outside 2 .. 64, h_floor negative or NaN; MGP_ERR_WORKSPACE for a null,
 * misaligned or short `work`.  The checks precede every launch. */
size_t mgp_ordinal_cut_sums_workspace_bytes(int64_t n, int K);
int mgp_ordinal_cut_sums(const float* f, const float* lo, const float* hi, const uint8_t* cat, const uint8_t* obs,
                         const double* var, const double* u, int64_t n, int K, double h_floor, double* out, void* work,
                         size_t work_bytes, void* stream);
/* Row scaling of a row-major [n, P] float32 block, 1 <= P <= 256:  out_ij = s_i V_ij  (X NULL)  or  fmaf(s_i, X_ij, V_ij).
 * out may be V or X.  float4 accesses where P % 4 == 0 and V, X, out are 16-byte aligned.  MGP_ERR_ARG for null s, V or out,
 * n < 1 and P outside 1 .. 256. */
int mgp_scale_rows(const float* s, const float* V, const float* X, int64_t n, int P, float* out, void* stream);

/* C-class labels with a softmax likelihood (csrc/laplace.hip, csrc/softmax_cg.hip, docs/kernels/classification.md): the kernels of
 * classification.laplace_fit_multiclass.  Blocks are row-major [n, C] float32, 2 <= C <= 64; the C latent functions share the
 * form-0 precision Q2.
 *
 * The likelihood stage of one Newton step.  f [n, C] latent values, qf [n, C] = Q2 F (NULL: zeros), labels [n] int32 (read at
 * observed nodes only), obs [n] bytes (non-zero: observed; NULL: every node).  Per row in float64 from the float32 inputs:
 *   m = max_c f_c,  e_c = exp(f_c - m),  Z = sum_c e_c,  pi_c = e_c / Z,  log p = f_t - m - log Z,  G = onehot(t) - pi
 * (pi = G = 0 on unobserved rows; G_t = 1 - pi_t is formed as sum_{c != t} e_c / Z, without the cancellation), and
 *   pi [n, C] = (float) pi,   rhs [n, C] = (float)(G - qf),
 *   sums [4] float64 (device) = { sum_obs log p,  sum f . qf,  max |G - qf|,  sum (G - qf)^2 }.
 * Finite for |f| up to 1e4.  A label is only compared with the class index, never used as an address: a label outside [0, C)
 * gives a row with G = -pi and no log p term (the Python layer validates labels).  A group of TC lanes (least power of two
 * >= C) owns a row; the sums go through one partial per workgroup and a second launch, fixed order, no atomics: repeated calls
 * are bitwise equal.  `work`: mgp_softmax_site_workspace_bytes(n, C) bytes, 8-byte aligned.
 * MGP_ERR_ARG for null f, labels, pi, rhs or sums, n < 1 and C outside 2 .. 64; MGP_ERR_WORKSPACE for a null, misaligned or
 * short `work`.  The checks precede every launch. */
size_t mgp_softmax_site_workspace_bytes(int64_t n, int C);
int mgp_softmax_site(const float* f, const float* qf, const int32_t* labels, const uint8_t* obs, int64_t n, int C, float* pi,
                     float* rhs, double* sums, void* work, size_t work_bytes, void* stream);
/* Y_i += pi_i o x_i - pi_i (pi_i . x_i) for every row: the softmax Hessian H(pi) X added to Y (X != Y), float32, the row's dot
 * product by an xor tree over its lane group.  A row of zeros in pi leaves its row of Y as it is.  The epilogue of a step of
 * mgp_softmax_cg, exported for tests and restatements.  MGP_ERR_ARG for null pointers, X == Y, n < 1, C outside 2 .. 64. */
int mgp_softmax_hessian_add(const float* pi, const float* X, int64_t n, int C, float* Y, void* stream);
/* CG on (Q2 (x) I_C + H(pi)) X = B as ONE system of size n C: one alpha and one beta per step (cg_rule.h on one column of
 * length n C), the Chronopoulos-Gear single-reduction recurrence, float32 vectors, float64 per-workgroup partials summed in a
 * fixed order (no atomics: a repeated solve, or one with another check_every, is bitwise equal).  A step is the operator chain
 * on C columns, mgp_softmax_hessian_add with the partials of R . R and R . W, and one update launch that forms the scalars,
 * updates P, S, X, R and decides  ||r||_2 <= tol ||b||_2  over all n C entries.  Eager launches; a device flag turns the
 * launches behind the decision into no-ops; the host reads the state once per check_every steps (0 = 8) and the call
 * returns when it has seen the decision (it synchronises `stream`).  op: form 0 only (MGP_ERR_UNSUPPORTED otherwise);
 * pi [n, C] rows of a softmax or zeros; X starts from 0 (B = 0: X = 0, status 1).  Host outputs (nullable): iters = updates
 * made, resid = the recurrence's relative residual at the decision, status 1 converged / 2 max_iter / 3 not finite, as
 * mgp_cg_plan_solve.  No preconditioner, no hipGraph.  `work`: mgp_softmax_cg_workspace_bytes(op, C) bytes (0 for arguments
 * the solve refuses), 16-byte aligned.  MGP_ERR_ARG for null op, pi, B, X, B == X, C outside 2 .. 64, tol < 0 or NaN,
 * max_iter < 1, check_every < 0 and an invalid operator; the checks precede every launch. */
size_t mgp_softmax_cg_workspace_bytes(const mgp_operator_t* op, int C);
int mgp_softmax_cg(const mgp_operator_t* op, const float* pi, int C, const float* B, float* X, float tol, int max_iter,
                   int check_every, int32_t* iters, float* resid, int32_t* status, void* work, size_t work_bytes, void* stream);
/* S right-hand sides of that system at once (csrc/softmax_cg_block.hip, layout in csrc/softmax_block.h): A X_s = B_s, s = 0 .. S - 1,
 * with A = Q2 (x) I_C + H(pi) and pi [n, C] shared.  B and X are row-major [n, S, C] (node i, sample s, class c at (i S + s) C + c),
 * so the operator chain runs once per step on S C columns; 2 <= C <= 64, S >= 1, S C <= 256.  Every sample keeps the scalars of
 * its own CG (gamma_s, delta_s, alpha_s, beta_s, ||b_s||^2, rel_s; cg_rule.h with a sample in the place of a column).  A step is
 * the chain, the block epilogue (W_is += H(pi_i) r_is with float64 partials of gamma_s and delta_s per workgroup), a reduce launch
 * (one workgroup per sample, fixed order) and the update.  A sample with rel_s <= tol is frozen: alpha_s = beta_s = 0 and X_s, R_s
 * are not written again.  The solve ends when every sample is frozen (status 1), at step > max_iter (2) or on a non-finite
 * residual (3).  No atomics: sample s depends on (op, pi, C, S, B_s, tol, max_iter) and its slot alone -- not on the other
 * (finite) right-hand sides, on check_every or on repetition.  Eager launches, a device flag, one host read per check_every steps
 * (0 = 8), as mgp_softmax_cg.  Host outputs (nullable): iters [S] = updates applied to each sample, resid [S] = its last rel_s
 * (B_s = 0: X_s = 0, iters 0, resid 0), status one word.  `work`: mgp_softmax_cg_block_workspace_bytes(op, C, S) bytes (0 for
 * arguments the solve refuses), 16-byte aligned.  MGP_ERR_ARG for null op, pi, B, X, B == X, C outside 2 .. 64, S < 1,
 * S C > 256, tol < 0 or NaN, max_iter < 1, check_every < 0 and an invalid operator; MGP_ERR_UNSUPPORTED for forms 1-3;
 * MGP_ERR_WORKSPACE for a null, misaligned or short `work`.  The checks precede every launch. */
size_t mgp_softmax_cg_block_workspace_bytes(const mgp_operator_t* op, int C, int S);
int mgp_softmax_cg_block(const mgp_operator_t* op, const float* pi, int C, int S, const float* B, float* X, float tol,
                         int max_iter, int check_every, int32_t* iters, float* resid, int32_t* status, void* work,
                         size_t work_bytes, void* stream);
/* The block epilogue alone, for tests: Y_is += pi_i o x_is - pi_i (pi_i . x_is) on X, Y [n, S, C] with pi [n, C], and, when `sums`
 * (device [S][2] float64) is given, the reduce launch: sums[s] = { sum x_s . x_s, sum x_s . y_s } with y the updated Y.  `work`:
 * mgp_softmax_hessian_add_block_workspace_bytes(n, C, S) bytes, 16-byte aligned, read only when sums is given.  MGP_ERR_ARG for
 * null pi, X, Y, X == Y, n < 1 and a shape the solver refuses (workspace size 0); MGP_ERR_WORKSPACE as above. */
size_t mgp_softmax_hessian_add_block_workspace_bytes(int64_t n, int C, int S);
int mgp_softmax_hessian_add_block(const float* pi, const float* X, int64_t n, int C, int S, float* Y, double* sums, void* work,
                                  size_t work_bytes, void* stream);
/* The symmetric factor of the softmax Hessian (csrc/laplace.hip, docs/kernels/evidence.md "The softmax family"): with
 * s_i = sqrt(pi_i),  R_i = diag(s_i)(I - s_i s_i^T),  R_i R_i^T = H_i = diag(pi_i) - pi_i pi_i^T  where the row sums to 1.
 *   transpose == 0:  out = R V          (R v)_c   = s_c v_c - pi_c sum_k s_k v_k               (X must be NULL)
 *   transpose != 0:  out = V + R^T X    (R^T x)_c = s_c (x_c - sum_k pi_k x_k)                 (V NULL: out = R^T X)
 * on S vectors of [n, C] float32, 2 <= C <= 64, S >= 1, C S <= 256: entry (i, c, s) of V, X and out lies at
 * i C S + c class_stride + s sample_stride, so (S, 1) is the layout [n, C, S] of a block of Lanczos vectors and (1, C) the
 * [n, S, C] of mgp_softmax_cg_block.  pi [n, C] is shared by the samples.  A group of lanes owns a (node, sample) row; sqrt(pi), the
 * row's dot product and the combination are float64 from the float32 inputs, rounded once at the store.  Where pi_ic = 0 the
 * entry is exactly 0 (forward) or exactly V (0 without V) whatever V and X hold there, NaN included.  out may be V or X.  No
 * atomics, no workspace: repeated calls are bitwise equal.  Element alignment only.
 * MGP_ERR_ARG for null pi or out, null V (forward) or X (transposed), X given forward, n < 1, C outside 2 .. 64, S < 1, C S > 256,
 * and strides that are not positive, let two entries of a row overlap or reach beyond its C S floats.  The checks precede the
 * launch. */
int mgp_softmax_root_apply(const float* pi, const float* V, const float* X, int64_t n, int C, int S, int64_t class_stride,
                           int64_t sample_stride, int transpose, float* out, void* stream);
/* The curvature term of the softmax evidence's gradient from latent deviations: for delta [n, S, C] float32 (the solution of
 * mgp_softmax_cg_block for S perturb-and-MAP right-hand sides: delta_s ~ N(0, A^-1)) and pi [n, C],
 *   d = delta_is - (pi_i . delta_is),   g_s = pi_ic (d_c^2 - sum_a pi_ia d_a^2),   acc_ic += sum_s g_s,   acc2_ic += sum_s g_s^2
 * in float64 from the float32 inputs, the samples added in the order s = 0 .. S - 1 and then to the entry: E g_s =
 * tr(V_i dH_i / df_ic) with V_i the C x C diagonal block of A^-1.  acc, acc2 [n, C] float64, distinct.  A row of zeros in pi is not
 * written.  One writer per entry, no atomics: a second run over the same blocks is bitwise equal.
 * MGP_ERR_ARG for null pointers, acc == acc2, n < 1, C outside 2 .. 64, S < 1, C S > 256. */
int mgp_softmax_curvature(const float* pi, const float* delta, int64_t n, int C, int S, double* acc, double* acc2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Eigensolve: the m smallest eigenpairs of L_sym by a Chebyshev-filtered block Krylov iteration
 * with Rayleigh-Ritz on L_sym itself (csrc/eigen.hip explains why not single-vector Lanczos; the
 * plain Lanczos tridiagonalisation is mgp_lanczos_tridiag below).
 * Replaces torch.linalg.eigh on the densified N x N matrix at
 * manifold_gp/kernels/riemann_kernel.py:121-125 and
 * GraphLaplacianOperator.diagonalization (graph_laplacian_operator.py:132-144).
 *   evals [m] ascending (host), evecs [n,m] row-major (device, orthonormal), resid [m] (host)
 *   = ||L v - lambda v||_2.  Synchronises `stream`.
 * Width: the block of b = min(mgp_lanczos_block_size(m, p), n) columns may have up to 512 columns -- with the default rule
 * m <= 455, with max_basis = 512 m <= 510 --; block products run in balanced column chunks of at most 256 per SpMM launch.
 * A wider block is MGP_ERR_UNSUPPORTED. */
typedef struct {
  int32_t max_basis;   /* block size b (0 = default: next multiple of 64 above m + max(m/8, 12)); at least m + 2, at most 512 */
  int32_t degree;      /* Chebyshev filter degree (0 = adaptive 8..200; no filter where the block is the whole space, b = n) */
  int32_t max_restarts;/* outer filter + Rayleigh-Ritz rounds (0 = 40) */
  float tol;           /* residual tolerance relative to lambda_max */
  uint64_t seed;
} mgp_lanczos_params_t;

/* host-only helper of the block eigensolver: eigendecomposition of a small dense symmetric matrix in
 * fp64 (Householder tridiagonalisation + implicit QL).  A [n x n] row-major, evals ascending,
 * eigenvectors = columns of V [n x n] row-major.  No device work. */
int mgp_host_symeig(int n, const double* A, double* evals, double* V);
size_t mgp_lanczos_workspace_bytes(int64_t n, int m, const mgp_lanczos_params_t* p);
int mgp_lanczos_smallest(const mgp_csr_t* L, int m, const mgp_lanczos_params_t* p, float* evals,
                         float* evecs, float* resid, int32_t* info, void* work, size_t work_bytes,
                         void* stream);
/* The same solve, also handing out the WHOLE Rayleigh-Ritz block it ended with -- the m wanted pairs plus the guard
 * columns behind them (b = mgp_lanczos_block_size(m, p) columns, Ritz values ascending): block_evals [b] (host),
 * block_evecs [n, b] row-major (device), block_resid [b] (host); any of the three may be NULL.  What an independent
 * check of the spectral stage needs (tests/test_gpu_configs.py: float64 Rayleigh-Ritz of the block with the oracle's
 * matrix, the gap behind the kept modes, a Davis-Kahan bound).
 * Return value of both: MGP_OK when all m residuals are <= tol * lambda_max, and ALSO when the iteration has reached the
 * fp32 residual floor (a few ulp of |L|: a round with the filter at its degree cap that does not even halve the largest
 * residual and converges no further pair), or when the measured gap between the wanted block and its last guard column says
 * that a further round at the degree cap would not even halve the residual: info[2] (pairs under tol) < m tells these
 * from convergence and `resid` holds what was reached.  Both early exits require the largest residual to be within
 * max(50 tol, 2e-5) * lambda_max (2e-5 = 10 x the measured fp32 floor); the Python wrapper warns (EigenFloorWarning) whenever
 * info[2] < m.  MGP_ERR_NOT_CONVERGED: max_restarts rounds without either. */
int mgp_lanczos_block_size(int m, const mgp_lanczos_params_t* p);
int mgp_lanczos_smallest_ex(const mgp_csr_t* L, int m, const mgp_lanczos_params_t* p, float* evals, float* evecs,
                            float* resid, int32_t* info, float* block_evals, float* block_evecs, float* block_resid,
                            void* work, size_t work_bytes, void* stream);
/* Warm start (round 5).  The reference re-runs the whole eigendecomposition on every eval() (riemann_kernel.py:117-130); while
 * the graph bandwidth moves a little per training step the previous Rayleigh-Ritz block is already close.  warm_block [n, b]
 * (device: the block_evecs of an earlier call on the SAME sparsity pattern and row order) replaces the random start, warm_evals
 * [b] (host: its block_evals) set the first round's filter, so that the first round is already a full-strength one.  Same
 * outputs, return values and tolerances as mgp_lanczos_smallest_ex. */
int mgp_lanczos_smallest_warm(const mgp_csr_t* L, int m, const mgp_lanczos_params_t* p, float* evals, float* evecs, float* resid,
                              int32_t* info, float* block_evals, float* block_evecs, float* block_resid, const float* warm_block,
                              const float* warm_evals, void* work, size_t work_bytes, void* stream);
/* Upper end of the eigensolver's Chebyshev filter: 1 (default) = lambda_max estimated from a 32-dimensional Krylov space
 * (+ 3 % or more), checked against the Ritz values of every round, with the Gershgorin bound as the fallback; 0 = the
 * Gershgorin bound (rigorous; about twice lambda_max on k-NN graph Laplacians, i.e. ~40 % more filter applies).  The residual
 * test uses the Gershgorin bound as its norm of L in both modes.  2 (tests only): half the estimate, a bound that is
 * certainly short, so that the fallback is exercised.  Process-wide. */
int mgp_lanczos_set_bound_mode(int mode);

/* k-step Lanczos tridiagonalisation of a precision-family operator with full re-orthogonalisation
 * (classical Gram-Schmidt against all previous vectors, twice).  Replaces
 * linear_operator.utils.lanczos.lanczos_tridiag as reached from
 * GraphLaplacianOperator.diagonalization (graph_laplacian_operator.py:132-135, Lanczos branch)
 * and from the stochastic-Lanczos-quadrature log-determinant of inv_quad_logdet
 * (train_model.py:68).  q0 [n] device start vector; alpha[steps], beta[steps] host;
 * Q_out (nullable) device [steps, n], row j = q_j.  Synchronises `stream`. */
/* P independent Lanczos runs at once (the probes of the stochastic log-determinant): Q0 [n, P] row-major,
 * P <= 16, steps <= 47; alpha / beta host [steps][P].  Same arithmetic per column as mgp_lanczos_tridiag,
 * one P-column SpMM chain per step instead of P single-vector chains.  Synchronises `stream`. */
size_t mgp_lanczos_tridiag_block_workspace_bytes(const mgp_operator_t* op, int P, int steps);
int mgp_lanczos_tridiag_block(const mgp_operator_t* op, const float* Q0, int P, int steps, float* alpha, float* beta,
                              void* work, size_t work_bytes, void* stream);
/* The same P runs for an operator the CALLER applies (round 5) -- the inverse of a Schur complement, every product of which is a CG
 * solve of its own: the stochastic log-determinant of the semi-supervised loss (train_model.py:68 through
 * schur_complement_operator.py:12-36).  mgp_blz_begin normalises the start block Q0 [n, P]; per step j = 0 .. steps - 1 the caller
 * reads q_j (mgp_blz_q: device pointer of the [n, P] block inside `work`), applies its operator and hands W = A q_j [n, P] to
 * mgp_blz_step (two passes of classical Gram-Schmidt against q_0 .. q_j, alpha_j, beta_j, q_j+1; W is overwritten);
 * mgp_blz_end copies alpha / beta (host [steps][P]) and synchronises `stream` -- nothing before it synchronises or reads back.
 * `work` (mgp_blz_workspace_bytes; 0 = unsupported shape: P <= 16, steps <= 47) is laid out identically at every call and must
 * not be touched in between. */
size_t mgp_blz_workspace_bytes(int64_t n, int P, int steps);
int mgp_blz_begin(const float* Q0, int64_t n, int P, int steps, void* work, size_t work_bytes, void* stream);
float* mgp_blz_q(int64_t n, int P, int steps, int j, void* work, size_t work_bytes);
int mgp_blz_step(float* W, int64_t n, int P, int steps, int j, void* work, size_t work_bytes, void* stream);
int mgp_blz_end(int64_t n, int P, int steps, float* alpha, float* beta, void* work, size_t work_bytes, void* stream);
size_t mgp_lanczos_tridiag_workspace_bytes(const mgp_operator_t* op, int steps);
int mgp_lanczos_tridiag(const mgp_operator_t* op, const float* q0, int steps, float* alpha,
                        float* beta, float* Q_out, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spectral features and the kernel block.
 * mgp_features_insample: Z = sqrt(N s / sum s) * Phi, s = (2 nu/kappa^2 + lambda)^-nu
 *   (riemann_kernel.py:134-136, riemann_matern_kernel.py:21-22); also the eval()-time
 *   post-processing Phi = normalise_cols(D^-1/2 U), lambda_0 = 0 (riemann_kernel.py:126-128)
 *   via mgp_eigvec_postprocess.
 * mgp_features_oos: fused Nystrom extension (graph_laplacian_operator.py:146-157) + bump
 *   modulation (riemann_kernel.py:138-147, torch_utils.py:38-41) without the [T,k,m] temporary.
 *   Limits (MGP_ERR_ARG beyond them, nothing written): m <= 1024 modes (mgp_features_insample too), k <= 1024 neighbours,
 *   normalization 0 (symmetric) or 1 (random walk).  A test point with sqrt(knn_d2[t][0]) >= bump_scale * eps gets a row of
 *   exact zeros, whatever its weights.  A test point INSIDE the support whose k weights exp(-d2 / (4 eps^2)) all underflow
 *   float32 to zero (d2 > ~415 eps^2: inside the support only with a bump scale above 20) has test degree 0 and gets a row of NaN (0 / 0), as the reference's
 *   float32 arithmetic does: tests/test_gpu_spectral_kernels.py pins the pattern against a float32 numpy restatement.
 * mgp_kernel_block: K = Z1 Z2^T on the fp32 MFMA (v_mfma_f32_32x32x2_f32)
 *   (MatmulLinearOperator / LowRankRootLinearOperator evaluation, riemann_kernel.py:92-100). */
size_t mgp_eigvec_postprocess_work_floats(int m);   /* size of colnorm_work in floats */
int mgp_eigvec_postprocess(float* evecs, int64_t n, int m, const float* degree, float* colnorm_work,
                           void* stream);
int mgp_features_insample(const float* evals_dev, const float* evecs, int64_t n, int m, int nu,
                          float kappa, float* Z, void* stream);
int mgp_features_oos(const float* evals_dev, const float* evecs, int64_t n, int m, int nu,
                     float kappa, float eps, int normalization, const float* degree_unnorm,
                     const float* degree, const float* knn_d2, const int32_t* knn_idx, int64_t T,
                     int k, float bump_scale, float bump_decay, float* Z, void* stream);
int mgp_kernel_block(const float* Z1, int64_t n1, const float* Z2, int64_t n2, int m, float scale,
                     float* K, void* stream);
/* K = scale * Z1 Z2^T on the fp32 MFMA.  Which kernel runs (A/B and test knob; results agree to fp32 rounding, the three
 * LDS kernels bit for bit with each other): 0 (default) = by shape: the resident-operand kernel where the operands allow it
 * (16 <= m <= 128, m and n2 multiples of 4, n1 >= 64, n2 >= 32, 16-byte aligned: a wave keeps 64 rows of Z1 in registers and
 * streams Z2, no LDS), else the lean one-tile kernel, else the general one; 1 = one 128x128 tile per workgroup, by the lean
 * kernel (single-instruction staging loads, 16-byte stores) where the operands allow it (n1, n2 >= 128, m and n2 multiples of
 * 4, 16-byte aligned) and by the general one elsewhere; 2 = where they allow it, one 512-thread workgroup per CU whose two
 * halves walk tiles and take turns on the matrix pipe; 3 = as 2 with every store dropped (timing only); 4 = the general kernel
 * always; 5 = as 0; 6 = as 5 with every store dropped (timing only). */
int mgp_kernel_block_set_pipe(int mode);
int mgp_kernel_diag(const float* Z1, const float* Z2, int64_t n, int m, float scale, float* out,
                    void* stream);
/* y = alpha * Z (Z^T x) + beta * x : the low-rank covariance K + sigma^2 I applied matrix-free */
size_t mgp_lowrank_workspace_bytes(int m, int C);
int mgp_lowrank_apply(const float* Z, int64_t n, int m, const float* X, int C, float alpha,
                      float beta, float* Y, void* work, size_t work_bytes, void* stream);
/* Woodbury solve of (s Z Z^T + noise I) x = v, the way gpytorch evaluates the reference's spectral kernel
 * (LowRankRootAddedDiagLinearOperator), in two device steps around an m x m fp64 system:
 *   mgp_gram_f64          G = A^T A for a tall block A [n,b] (b <= 512), fp64 accumulation -> device double [b,b];
 *                         with A = [Z | v] one pass gives Z^T Z, Z^T v (and v^T v)
 *   mgp_lowrank_residual  out = scale * (V - Z T), T device double [m,C] (m C <= 6144), row sums in fp64 */
size_t mgp_gram_workspace_bytes(int64_t n, int b);
int mgp_gram_f64(const float* A, int64_t n, int b, double* G, void* work, size_t work_bytes, void* stream);
/* the partial Gram blocks of mgp_gram_f64 and of the eigensolver on the fp64 matrix cores (v_mfma_f64_16x16x4_f64; default 1) or by
 * fp64 vector FMAs (0: A/B runs, tests); returns the previous setting */
int mgp_gram_set_mfma(int on);
int mgp_lowrank_residual(const float* Z, int64_t n, int m, const double* T, const float* V, int C, double scale,
                         float* out, void* stream);
/* One Newton evaluation of a Laplace fit on the spectral features (csrc/spectral_laplace.hip, docs/kernels/spectral_laplace.md;
 * spectral_laplace.spectral_laplace_fit): the latent function is f = Z w + mean with Z [n, m] row-major float32 (any alignment:
 * 16-byte loads where m % 4 == 0 and Z is 16-byte aligned, scalar ones otherwise; 1 <= m <= 512, finite entries) and w [m]
 * float64.  family: 0 Bernoulli-logit (a = labels, class 1 where a > 0.5), 1 Poisson (a = counts, b = log-exposure or NULL:
 * zeros), 2 binomial (b = trials), 3 negative binomial (b = log-exposure or NULL, dispersion in [2^-10, 2^20]), 4 ordinal (a, b =
 * the row's interval (lo, hi] of cutpoints, infinite ends allowed).  a and b [n] float32 are read at observed rows only (NaN
 * allowed elsewhere); obs [n] bytes, NULL: every row.  f_i = z_i . w is formed in float64 (fma's and a fixed tree) and goes
 * straight into the family's formulas, those of mgp_bernoulli_site, mgp_count_site, mgp_nb_site and mgp_ordinal_site, at
 * f_i + mean (l, g = dl / df, h = -dg / df; the Poisson exp at min(eta, 700); 0 at unobserved rows).  Outputs, float64 on the
 * device:
 *   f [n] (nullable) = z_i . w without the mean,   grad [m] = Z^T g,   hess [m, m] (nullable) = Z^T diag(h) Z,
 *   sums [2] = { sum_obs l_i (without the families' f-independent constants),  max_i |f_i| over every row }.
 * The prior's terms (-w / s, I / s, -w . w / (2 s)) are the caller's.  hess comes from the fp64 matrix cores in a second pass
 * over Z that skips 32-row stages without an observed row; it is bitwise symmetric.  Sums are one partial per workgroup or row
 * chunk and a second launch that adds them in a fixed order: no atomics, repeated calls are bitwise equal, and f, grad and sums
 * of a call with hess == NULL equal those of a call with it bit for bit.  Finite outputs for finite inputs with |f| <= 1e4.
 * `work`: mgp_spectral_site_workspace_bytes(n, m, with_hessian) bytes, 8-byte aligned (0 for arguments the entry point refuses).
 * MGP_ERR_ARG for null Z, w, a, grad or sums, n < 1, m outside 1 .. 512, a missing b (families 2, 4), a dispersion out of range
 * (family 3) or a misaligned array; MGP_ERR_UNSUPPORTED for any other family; MGP_ERR_WORKSPACE for a null, misaligned or short
 * `work`.  The checks precede every launch. */
size_t mgp_spectral_site_workspace_bytes(int64_t n, int m, int with_hessian);
int mgp_spectral_site(const float* Z, int64_t n, int m, const double* w, int family, const float* a, const float* b,
                      const uint8_t* obs, double mean, double dispersion, double* f, double* grad, double* hess, double* sums,
                      void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU (one process per GPU, RCCL over xGMI): row-partitioned operator apply and CG.
 * The reference has no distributed code; this is the north-star's
 * "CG SpMV row-partitions across the 8 GPUs of one node with one RCCL collective per iteration".
 *   - rank p owns global rows [p*n_loc, (p+1)*n_loc) of L (op_local->L: local CSR slice whose
 *     column ids are global; op_local->pre/post and every vector have GLOBAL length world*n_loc and
 *     are replicated on every rank);
 *   - per SpMM launch each rank computes its row slice, then ONE grouped ncclAllGather assembles
 *     the output on every rank; on the last launch of a chain the dot-product partials ride in the
 *     same group, so CG needs no separate scalar reduction (the vector updates are replicated and
 *     every rank takes bit-identical decisions);
 *   - the communicator comes from ncclCommInitRank over a unique id the host distributes. */
int mgp_dist_unique_id_bytes(void);
int mgp_dist_unique_id(void* id_out);                          /* rank 0 */
int mgp_dist_init(int rank, int world, const void* id_bytes, void** comm_out);
int mgp_dist_destroy(void* comm);
/* size of the communicator, this process's rank in it and its HIP device, as RCCL reports them (ncclCommCount /
 * ncclCommUserRank / ncclCommCuDevice): what bench.py's N > 1 line carries as `rccl_ranks` */
int mgp_dist_comm_info(void* comm, int32_t* count, int32_t* user_rank, int32_t* device);
int mgp_dist_allgather(void* comm, int rank, int world, float* buf, int64_t count_per_rank,
                       void* stream);                          /* in place, slice p at p*count */
int mgp_operator_apply_part(const mgp_operator_t* op_local, void* comm, int rank, int world,
                            const float* X, int C, float* Y, void* work, size_t work_bytes,
                            void* stream);                     /* work: 4 global-length buffers */
size_t mgp_cg_dist_workspace_bytes(const mgp_operator_t* op_local, int C, int world);
int mgp_cg_plan_create_dist(const mgp_operator_t* op_local, int C, const float* minv,
                            const mgp_cg_params_t* params, void* comm, int rank, int world,
                            void* work, size_t work_bytes, void* stream, void** plan_out);
/* solve / x / destroy: mgp_cg_plan_solve, mgp_cg_plan_x, mgp_cg_plan_destroy (B, X global length) */

/* ---------------------------------------------------------------------------------------------
 * Partitioned pipelined CG (csrc/pcg.hip): the multi-GPU form that can scale -- vectors AND rows partitioned,
 * ONE grouped RCCL all-gather per iteration (the w slices + the dot partials), ghost layers instead of a second
 * exchange for nu >= 2, the iteration loop captured in a hipGraph.  C = 1, forms 0 and 2.  Same call sites as
 * mgp_cg_plan_* above (the (K + s I) x = y solve in precision form).
 *   op->L        tile view of the WHOLE padded graph over this rank's row order [own rows, ghost layer 1, ...,
 *                rest] (mgp_graph_tiles with `order`: tile_rowptr / tile_vals / tile_rowid set); L.n = global
 *                (padded) node count; pre / post / diag at the global length
 *   launch_rows  [nu]: rows of that view launch s of the SpMV chain covers = own rows + (nu - 1 - s) ghost layers,
 *                rounded up to the tile height; launch_rows[nu - 1] >= n_loc
 *   row0, n_loc  this rank's contiguous row block (row0 = rank * n_loc, equal blocks); n_real: rows >= n_real are
 *                padding
 *   comm         ncclComm_t, or NULL: world == 1, or VIRTUAL ranks of one process sharing `shared`
 *                (mgp_pcg_shared_floats floats: gathered w and partials, double-buffered), driven phase by phase
 *                with mgp_pcg_plan_enqueue -- what the single-GPU tests of the partition logic use
 *   B            right-hand side at the global length on every rank; the solution's own rows are valid in
 *                mgp_pcg_plan_x()[row0 .. row0 + n_loc) and copied to X_loc when given */
size_t mgp_pcg_shared_floats(int64_t n_glob, int64_t n_loc, int world);
size_t mgp_pcg_workspace_bytes(int64_t n_glob, int64_t n_loc, int world);
/* recurrence: 0 = pipelined (ONE grouped all-gather per iteration; stagnates early on ill-conditioned systems in
 *             fp32: residual replacement for chunks >= 16 iterations, refinement rounds with max_refine),
 *             1 = Chronopoulos-Gear, the recurrence of mgp_cg_plan_* (robust; TWO collectives per iteration: the
 *             gathered vector + gamma partials, and ~n_loc / 64 delta partials per rank) */
int mgp_pcg_plan_create(const mgp_operator_t* op, const int64_t* launch_rows, int64_t row0, int64_t n_loc,
                        int64_t n_real, void* comm, int rank, int world, float* shared, int recurrence,
                        const mgp_cg_params_t* params, void* work, size_t work_bytes, void* stream,
                        void** plan_out);
int mgp_pcg_plan_solve(void* plan, const float* B, float* X_loc, int32_t* iters, float* resid, int32_t* status);
int mgp_pcg_plan_enqueue(void* plan, int phase, int par, const float* B); /* 0: start; 1: iteration (recurrence 1: its
                                                                             SpMV chain); 2: recurrence 1: its update */
int mgp_pcg_plan_poll(void* plan, int32_t* iters, float* resid, int32_t* status); /* 1 = undecided */
float* mgp_pcg_plan_x(void* plan);
int mgp_pcg_plan_destroy(void* plan);
int mgp_pcg_plan_poisoned(void* plan);   /* as mgp_cg_plan_poisoned */

#ifdef __cplusplus
}
#endif
#endif /* MGP_HIP_H */
