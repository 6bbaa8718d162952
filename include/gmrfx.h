/*
 * gmrfx.h -- C ABI of libgmrfx.so, the MI355X-native sparse-Cholesky / triangular-solve /
 * selected-inverse backend for GaussianMarkovRandomFields.jl's GMRF precision-matrix path.
 *
 * Every entry point replaces one call the reference makes into CHOLMOD / SelectedInversion.jl
 * behind its two solver seams (file:line relative to the reference repository):
 *
 *   seam B  WorkspaceBackend protocol            src/workspace/backend.jl:8-30
 *   seam A  LinearSolve algorithm + GMRF hooks   src/solvers/{selinv,backward_solve,logdet}.jl,
 *                                                ext/GaussianMarkovRandomFieldsPardiso.jl:10-80
 *
 * Conventions: plain C types only; int64 indices (Julia `Int`); `index_base` 0 or 1; dense
 * blocks are column-major with explicit leading dimension; every array is caller-owned and
 * only read/written during the call (the library copies what it keeps). A handle owns one HIP
 * stream; a handle is not re-entrant, distinct handles may be used from different threads
 * (the WorkspacePool contract, src/workspace/workspace_pool.jl:15-20). No callbacks, no
 * global mutable state except a thread-local error string for failed gmrfx_create calls.
 *
 * All numeric work runs on the GPU. There is no CPU fallback: without a usable HIP device the
 * numeric entry points return GMRFX_ERR_NO_DEVICE.
 */
#ifndef GMRFX_H
#define GMRFX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gmrfx_handle gmrfx_handle;

enum {
    GMRFX_OK = 0,
    GMRFX_ERR_INVALID_ARG = 1,   /* -> Julia ArgumentError / DimensionMismatch */
    GMRFX_ERR_NO_DEVICE = 2,     /* no HIP device or handle created symbolic_only */
    GMRFX_ERR_HIP = 3,           /* HIP runtime error, text in gmrfx_last_error */
    GMRFX_ERR_NOT_FACTORIZED = 4,/* numeric op before the first gmrfx_refactorize */
    GMRFX_ERR_NOT_POSDEF = 5,    /* only from gmrfx_refactorize when opts.check_posdef != 0 */
    GMRFX_ERR_ALLOC = 6
};

enum { GMRFX_UPLO_UPPER = 0, GMRFX_UPLO_LOWER = 1 };
enum { GMRFX_ORDER_AUTO = 0, GMRFX_ORDER_NATURAL = 1 };

typedef struct gmrfx_opts {
    int32_t struct_size;    /* = sizeof(gmrfx_opts); lets the struct grow compatibly */
    int32_t uplo;           /* which stored triangle defines Q when both are present.
                               GMRFX_UPLO_UPPER mirrors Symmetric(ws.Q) (default :U),
                               src/workspace/gmrf_workspace.jl:176 */
    int32_t ordering;       /* used when perm == NULL: AUTO = nested dissection (geometric if
                               coords != NULL, graph-based otherwise), NATURAL = identity */
    int32_t device;         /* HIP device ordinal; -1 = current device */
    int32_t symbolic_only;  /* 1: host symbolic analysis only (ordering, supernodes, stats,
                               gmrfx_get_perm); numeric entry points fail loudly */
    int32_t check_posdef;   /* 0: seam-B behaviour, never fail on indefiniteness
                               (cholesky!(...; check=false), src/workspace/backend.jl:184);
                               1: seam-A behaviour, return GMRFX_ERR_NOT_POSDEF */
    int32_t nd_leaf;        /* nested-dissection leaf size (0 = default) */
    int32_t relax_cols;     /* supernode amalgamation: merge while width <= relax_cols ... */
    double  relax_zeros;    /* ... or added explicit-zero fraction <= relax_zeros (0 = default) */
    int32_t coord_dim;      /* 0, 2 or 3 */
    int32_t reserved0;
    const double *coords;   /* optional n x coord_dim row-major node coordinates (mesh nodes),
                               enables geometric nested dissection; NULL otherwise */
    /* Sharding ONE factorisation over shard_world processes (one GPU each): every process creates
     * its handle with the same pattern / options and its own shard_rank. The supernodal tree is cut
     * into subtrees dealt to the ranks; every front above them (the "top") is owned by ONE rank of the
     * group whose subtrees it joins (the least loaded owner of its children). See the
     * gmrfx_shard_* entry points. shard_world <= 1: unsharded (default). */
    int32_t shard_rank, shard_world;
    /* Force at least this many fronts into the top of the sharded plan (0 = the cost model decides). With shard_world == 1 a
     * value > 0 makes the handle a SHARDED handle of one rank: the phase entry points, the top levels and the (empty or
     * self-addressed) exchange lists of the protocol below run on a single GPU -- how tests/test_rccl_world1.py executes the
     * RCCL device path of gmrfx/shard.py on the one-GPU boxes of the test pool. */
    int32_t shard_min_top;
    int32_t reserved1;
} gmrfx_opts;

typedef struct gmrfx_stats {
    int64_t n, nnz_q_tri, nnz_l, nnz_l_stored; /* true fill / fill incl. amalgamation zeros */
    int64_t nsuper, nlevels, max_cols, max_rows, sum_rows;
    int64_t n_small_fronts, n_big_fronts;
    double  factor_flops;          /* sum_s c^3/3 + c^2 (r-c) + c (r-c)^2                  */
    double  bytes_factor, bytes_cb_arena, bytes_device_total;
    double  ms_symbolic;           /* host wall time of gmrfx_create's analysis             */
    /* GPU times of the most recent call of each kind, HIP events on the handle's stream    */
    double  ms_factor, ms_solve, ms_solve_fwd, ms_solve_bwd, ms_solve_perm, ms_backward_solve,
            ms_logdet, ms_selinv;
    int64_t last_nrhs;
    int64_t fail_col;              /* -1, or first (permuted, 0-based) non-positive pivot   */
    /* the dominant kernel of the factorisation (contribution-block SYRK, k_syrk_cb): summed device
     * time of its launches in the most recent refactorisation -- per launch the latest end minus the
     * earliest start that its own workgroups read from the device's wall clock (no event on the
     * stream) --, their number, and the flops they do
     * (sum over big fronts of c m (m + 1), m = r - c: lower triangle only)                  */
    double  ms_syrk, syrk_flops;
    int64_t syrk_launches;
    double  ms_quadform;           /* most recent gmrfx_quadform(_dev): kernels only             */
    /* widest diagonal block the sweeps use as an explicit inverse (2048 by default; 64 once the handle's first factorisation
     * found a front with pivot growth above 1e4), and the host wall time that one-time check took (0 before it ran) */
    int64_t inv_cap;
    double  ms_inv_decide;
    double  ms_rbmc;               /* most recent gmrfx_rbmc_var(_dev): GPU time, backward sweeps included */
} gmrfx_stats;

/* Message for the most recent failed gmrfx_create on this thread. */
const char *gmrfx_last_create_error(void);
/* Message for the most recent failure on this handle. */
const char *gmrfx_last_error(const gmrfx_handle *h);

/* Symbolic analysis (+ device upload). Replaces `cholesky(Q; perm=...)`'s analyse phase:
 * CHOLMODBackend ctor src/workspace/backend.jl:147-153, ordering_permutation :73-133.
 * colptr/rowval: CSC pattern of Q, either one triangle or both (both is what ws.Q holds).
 * perm (nullable): user elimination order, perm[k] = index (index_base-based) of the k-th
 * pivot. The pattern is fixed for the life of the handle; nzval passed later must follow the
 * same CSC order (the workspace guarantees it: gmrf_workspace.jl:131-143). */
int32_t gmrfx_create(int64_t n, const int64_t *colptr, const int64_t *rowval, int32_t index_base,
                     const int64_t *perm, const gmrfx_opts *opts, gmrfx_handle **out);
void    gmrfx_destroy(gmrfx_handle *h);
/* deepcopy(cache) at the start of Newton loops: arithmetic/condition/gaussian_approximation.jl:103-109 */
int32_t gmrfx_clone(const gmrfx_handle *h, gmrfx_handle **out);

/* Numeric refactorisation on the fixed pattern. Replaces
 * `_copy_sparse_values!` + `cholesky!(F, S; check=false)`: src/workspace/backend.jl:165-189.
 * Drops the selected-inverse cache. info (nullable) <- 0, or 1 + first failing pivot column
 * in the elimination order. */
int32_t gmrfx_refactorize(gmrfx_handle *h, const double *nzval, int64_t *info);
int32_t gmrfx_refactorize_dev(gmrfx_handle *h, const double *d_nzval, int64_t *info);
/* Numeric refactorisation AND solve Q X = B in one call. Replaces `workspace_solve(ws, B)` on a workspace whose values have
 * just been updated (src/workspace/gmrf_workspace.jl:170-178 `ensure_numeric!` -> `refactorize!`, :207-215 `backend_solve`):
 * the Newton / hyper-parameter loops always run the two back to back. Same results, bit for bit, as gmrfx_refactorize followed
 * by gmrfx_solve -- but pipelined: the forward sweep follows the factorisation up the elimination tree on a second stream
 * (level l of the sweep starts when level l is factored), so the bottom of the sweep fills the chip while the top of the
 * factorisation is a chain of small dependent launches. X is only meaningful when *info == 0. B / X column-major n x nrhs. */
int32_t gmrfx_refactorize_solve(gmrfx_handle *h, const double *nzval, const double *B, int64_t ldb, int64_t nrhs, double *X, int64_t ldx,
                                int64_t *info);
int32_t gmrfx_refactorize_solve_dev(gmrfx_handle *h, const double *d_nzval, const double *d_B, int64_t ldb, int64_t nrhs, double *d_X,
                                    int64_t ldx, int64_t *info);

/* One evaluation of the hyper-parameter loop (docs/src/literate-tutorials/workspace_factorization_reuse.jl:94-102) in ONE call:
 * new values -> numeric factorisation, quad[k] = (x_k - mu)' Q (x_k - mu) for nvec vectors and *logdet = log det Q, i.e. everything
 * `logpdf(::WorkspaceGMRF, z)` needs (src/workspace/workspace_gmrf.jl:288-292 with `ensure_numeric!` inside,
 * gmrf_workspace.jl:170-178). Device pointers for Q's values, X (column-major n x nvec) and mu (nullable); the quadratic forms run
 * beside the factorisation, one synchronisation, both results arrive through pinned memory. Same bits as gmrfx_refactorize_dev +
 * gmrfx_quadform_dev + gmrfx_logdet. */
int32_t gmrfx_refactorize_logpdf_dev(gmrfx_handle *h, const double *d_nzval, const double *d_X, int64_t ldx, int64_t nvec,
                                     const double *d_mu, double *quad /* host, nvec */, double *logdet /* host */, int64_t *info);

/* ---- Newton loop with Q resident on the device -----------------------------------
 * Replaces `_update_hessian!` + `ensure_numeric!` of the Gaussian-approximation loop
 * (src/workspace/gaussian_approximation.jl:103-129: copyto!(ws.Q.nzval, prior_nzval); nzval[map[k]] -= H.nzval[k]).
 * gmrfx_set_prior uploads the prior's values (same CSC order as the pattern) and the Hessian -> Q index map
 * (`diag_idx` or `_sparse_hessian_map`, index_base-based positions into nzval) ONCE; every iterate then sends
 * only the cnt Hessian values and refactorises: Q_k = Q_prior - H_k is formed on the device. */
int32_t gmrfx_set_prior(gmrfx_handle *h, const double *prior_nzval, const int64_t *map, int64_t cnt, int32_t index_base);
int32_t gmrfx_refactorize_update(gmrfx_handle *h, const double *hvals, int64_t *info);
int32_t gmrfx_refactorize_update_dev(gmrfx_handle *h, const double *d_hvals, int64_t *info);
/* One whole Newton iterate (gaussian_approximation.jl:103-129: `_update_hessian!`, `ensure_numeric!`, the solve for the new mean) as
 * one pipelined call: gmrfx_refactorize_update followed by gmrfx_solve, with the forward sweep running beside the factorisation
 * like gmrfx_refactorize_solve; same bits as the two calls. */
int32_t gmrfx_refactorize_update_solve(gmrfx_handle *h, const double *hvals, const double *B, int64_t ldb, int64_t nrhs, double *X, int64_t ldx,
                                       int64_t *info);
int32_t gmrfx_refactorize_update_solve_dev(gmrfx_handle *h, const double *d_hvals, const double *d_B, int64_t ldb, int64_t nrhs, double *d_X,
                                           int64_t ldx, int64_t *info);

/* ---- sharded factorisation (opts.shard_world > 1); SURVEY section 8(e) -------------------------------
 * ONE factorisation over several GPUs, one process each, driven by the host language over its collective library
 * (RCCL through torch.distributed in the Python binding, gmrfx/shard.py). Every process runs the same analysis: the
 * supernodal tree is cut into subtrees dealt to the ranks, and every front ABOVE them (the "top") is owned by one
 * rank of the group whose subtrees it joins -- independent top fronts run on different GPUs, and data crosses ranks
 * only along the tree edges whose two ends have different owners (gmrfx_shard_edges: child, src, dst, level of the
 * parent, the contribution block's place in the arena gmrfx_device_ptr(h, 0), the update vector's rows in
 * gmrfx_device_ptr(h, 3)). X / W rows are laid out identically on all ranks; the contribution-block ARENA has its own
 * layout on every rank (round 6: a rank only gives slots -- shared by lifetime -- to the blocks it produces or receives),
 * so cb_offset / zb_offset / gmrfx_shard_transfers' offset are THIS rank's offsets (-1 when the rank is neither end):
 * the sender builds its view from its own handle's table, the receiver from its own. K = nlevels - shard_level top levels.
 *   refactorisation  gmrfx_refactorize_phase(h, nzval, 0)      the subtrees this rank owns
 *                    for k = 0 .. K-1:  [contribution blocks of the edges with level = shard_level + k: src -> dst]
 *                                       gmrfx_refactorize_phase(h, nzval, 1 + k)   this rank's fronts of top level k
 *   log det Q        all-reduce (sum) of gmrfx_logdet_partial; pivot failures: all-reduce (min) of gmrfx_stats.fail_col
 *   solve (1..64 right-hand sides, device buffers)
 *                    gmrfx_solve_phase(.., 0)                  transpose in + forward sweep over the own subtrees. Of d_B a rank
 *                                                              READS only the rows of the columns it owns (its subtrees' and its
 *                                                              own top fronts': gmrfx_shard_rows kinds 3 and 2 with owner = rank,
 *                                                              through gmrfx_get_perm): B may be row-sharded over the ranks
 *                    for k = 0 .. K-1:  [update vectors W of the level's edges: src -> dst]   gmrfx_solve_phase(.., 100 + k)
 *                    for k = K-1 .. 0:  gmrfx_solve_phase(.., 200 + k)   [x of that level's top fronts: owner -> all,
 *                                       gmrfx_shard_rows(kind 2)]
 *                    gmrfx_solve_phase(.., 2)                  backward sweep over the own subtrees
 *                    [x of every assigned subtree -> rank 0, gmrfx_shard_rows(kind 3)]   gmrfx_solve_phase(.., 3) on rank 0
 *   selected inversion (top-down)   gmrfx_selinv_phase(h, 0, 0, 0) begin; for every level l from the top: (h, 1, l, 0) the
 *                    owners of the PARENTS gather the trailing inverse blocks of the other ranks' fronts at level l;
 *                    [those blocks (zb_offset / cb_count of the edges with child_level = l, in gmrfx_device_ptr(h, 0)):
 *                    owner of the parent -> owner of the child]; (h, 2, l + 1, l) this rank's fronts of level l
 *                    (levels without cross-rank edges may be run as one range); (h, 3, 0, 0) end. The getters
 *                    (gmrfx_selinv_diag / _extract / _dot ...) then return this rank's PART (zeros for the entries of
 *                    other ranks' fronts): sum over the ranks = the selected inverse. */
int32_t gmrfx_refactorize_phase(gmrfx_handle *h, const double *d_nzval, int32_t phase);
int32_t gmrfx_shard_info(const gmrfx_handle *h, int64_t *n_edges, int64_t *n_top_fronts, int64_t *shard_level);
int32_t gmrfx_shard_edges(const gmrfx_handle *h, int64_t *child, int64_t *src, int64_t *dst, int64_t *level,
                          int64_t *cb_offset, int64_t *cb_count, int64_t *w_row0, int64_t *w_nrows,
                          int64_t *zb_offset /* nullable */, int64_t *child_level /* nullable */);
int32_t gmrfx_selinv_phase(gmrfx_handle *h, int32_t what, int32_t level_hi, int32_t level_lo);
int32_t gmrfx_shard_owner(const gmrfx_handle *h, int64_t *owner /* nsuper, >= 0 */, int64_t *is_top /* nsuper, nullable */);
void   *gmrfx_device_ptr(gmrfx_handle *h, int32_t which /* 0: contribution-block arena, 1: factor panels, 2: X, 3: W */);
int32_t gmrfx_solve_phase(gmrfx_handle *h, const double *d_B, int64_t ldb, int64_t nrhs, double *d_X, int64_t ldx, int32_t phase);
/* Backward-only sharded solve, X = P' L^-T Z (`F.UP \ z`, src/workspace/backend.jl:281-284), through the same entry point:
 * phase 10 = take Z in elimination order (a rank reads the rows of its own columns only, as above); 300 + k = backward over top level k [then broadcast that
 * level's x rows, as after 200 + k]; 12 = backward over the own subtrees; [gather on rank 0]; 3 = transpose out.
 *
 * gmrfx_set_stream: the caller's HIP stream becomes the handle's main stream (use_external = 1; 0 restores the handle's
 * own). A sharded driver passes the stream its communication library orders its operations on (torch's current stream for
 * torch.distributed / RCCL): kernels, copies and transfers are then ordered by the stream, and with async_phases = 1 the
 * phase entry points (gmrfx_refactorize_phase / _solve_phase / _selinv_phase) return after enqueueing -- no host-side
 * synchronisation between a phase and the exchange behind it (their HIP-event timings are not collected then). */
int32_t gmrfx_set_stream(gmrfx_handle *h, void *hip_stream, int32_t use_external, int32_t async_phases);
/* DISTRIBUTED TOP FRONTS (sharded handles; csrc/symbolic.h Symbolic::dist_fronts): a top front with at least 4096 columns
 * (GMRFX_DIST_MIN overrides; 0 = never) whose group -- the ranks owning the subtrees below it -- has more than one rank is
 * factored by the WHOLE GROUP: the dense top fronts of a 3-D problem hold most of the flops (cfg 4: the root alone has 47 628
 * columns) and the single-address-space call this replaces, `cholesky!(F, S; check = false)` (src/workspace/backend.jl:165-189),
 * has no notion of it. Panel columns and contribution-block columns are cut into 256-column blocks dealt cyclically over the
 * group (panel block b -> group[b mod g], contribution-block block q -> group[(panel blocks + q) mod g]); a front WITH a contribution
 * block is stored whole by every member, one without (the root) only by its owner (gmrfx_dist_front_block below); sweeps and
 * selected inversion of the front stay on its owner.
 *   gmrfx_shard_dist_fronts: counts[0] fronts, [1] group entries, [2] transfers, [3] world; per front (nullable): supernode,
 *     columns, rows, panel offset in gmrfx_device_ptr(h, 1), panel leading dimension, tree level; gptr / grank: its group.
 *   gmrfx_shard_transfers: every contribution-block transfer of the factorisation, ordered by the parent's level: `count`
 *     doubles (whole columns of `child`'s block) at `offset` of THIS rank's gmrfx_device_ptr(h, 0) (-1 when this rank is neither
 *     src nor dst; the two ends have different offsets) go src -> dst before level `level` is assembled (col0: the first of
 *     these columns). Replaces the cb_offset / cb_count columns of gmrfx_shard_edges for the factorisation.
 *   gmrfx_dist_front_phase(h, d_nzval, front, what, block): 0 = assemble this rank's panel blocks; 1 = factor panel block
 *     `block` (its owner; a no-op elsewhere) [then broadcast columns 256 block .. of the panel inside the group]; 2 = apply
 *     block `block` to this rank's later panel blocks (4 = to block + 1 only, 5 = to the later blocks except block + 1: the
 *     LOOK-AHEAD split -- the owner of block + 1 applies 4, factors and starts the broadcast of block + 1, and everybody
 *     applies 5 while that broadcast is in flight); 3 = this rank's blocks of the contribution block. A no-op on ranks
 *     outside the group. Same kernels, same sums in the same order as an unsharded handle: bit-identical factor. */
int32_t gmrfx_shard_dist_fronts(const gmrfx_handle *h, int64_t *counts /* 4 */, int64_t *front, int64_t *cols, int64_t *rows,
                                int64_t *panel_offset, int64_t *panel_ld, int64_t *level, int64_t *gptr, int64_t *grank);
int32_t gmrfx_shard_transfers(const gmrfx_handle *h, int64_t *child, int64_t *src, int64_t *dst, int64_t *level,
                              int64_t *offset, int64_t *count, int64_t *col0);
int32_t gmrfx_dist_front_phase(gmrfx_handle *h, const double *d_nzval, int32_t front, int32_t what, int32_t block);
/* Block-cyclic STORAGE of a distributed front without trailing rows (the root; round 6): only the front's owner -- which sweeps and
 * inverts it -- stores the whole panel; every other member keeps its own 256-column blocks and a window of two received blocks
 * (cfg 4 at world 8: 18 GB -> 2.5 GB on seven of eight ranks). gmrfx_dist_front_block tells a rank where IT keeps panel block
 * `block` -- offset into gmrfx_device_ptr(h, 1) and doubles (whole columns) --: the buffer it hands to the broadcast of that block
 * (the ends of a broadcast have different offsets). -1 / 0 outside the group. Fronts with a contribution block stay replicated
 * (every member needs all of L21 for its own column blocks of that block). */
int32_t gmrfx_dist_front_block(const gmrfx_handle *h, int32_t front, int32_t block, int64_t *offset, int64_t *count);
/* Profiling aid (handles created under GMRFX_LEVEL_MARK=1): HIP-event time of every tree level of the most recent
 * factorisation (which = 0), forward (1) or backward (2) sweep: ms[0] = the sweep tasks, ms[1 + l] = level l; *count = entries
 * written (0 when the marks are off). gmrfx/shard.py turns them into the TIME bound of a sharding plan (plan_summary). */
int32_t gmrfx_level_times(gmrfx_handle *h, int32_t which, double *ms, int64_t cap, int64_t *count);
int32_t gmrfx_shard_rows(const gmrfx_handle *h, int32_t kind, int64_t *nblocks, int64_t *owner, int64_t *row0, int64_t *nrows,
                         int64_t *level);
int32_t gmrfx_logdet_partial(gmrfx_handle *h, double *out);

/* How the HOST entry points (gmrfx_solve, gmrfx_refactorize_solve, ... with pageable B / X: what `workspace_solve(ws, B::Matrix)`
 * hands over, src/workspace/gmrf_workspace.jl:207-215) cut a column-major n x nrhs array into slices for the handle's
 * page-locked staging ring of 8 slots (download = 0: B in, 1: X out). plan[0] columns per slice, [1] row pieces per column
 * (> 1 once a column exceeds a slice), [2] rows per piece, [3] doubles per ring slot, [4] slices, [5] doubles reserved
 * (= min(slices, 8) x slot). Slice k covers columns [k plan[0], ...) when plan[1] == 1, else column k / plan[1], rows
 * [(k mod plan[1]) plan[2], ...). Arithmetic only (no handle, no device) -- exported so that the invariant "every slice fits
 * its slot, the slices tile the array" is checked on the CPU for sizes no test box holds. */
int32_t gmrfx_host_io_plan(int64_t n, int64_t nrhs, int32_t download, int64_t *plan /* 6 */);

/* ---- Layout of B, X and Z (every solve-family call: gmrfx_solve, gmrfx_backward_solve, gmrfx_refactorize_solve,
 * gmrfx_refactorize_update_solve, gmrfx_quadform, gmrfx_refactorize_logpdf_dev and their _dev forms) ------------------------------
 * A dense argument is a column-major n x nrhs WINDOW: element (i, j) at ptr[i + j ld], ld >= n (GMRFX_ERR_INVALID_ARG otherwise,
 * and for a null array, whenever nrhs > 0; nrhs == 0 touches neither array). The window may sit anywhere inside a larger array -- a
 * `@view` of a taller matrix: the base pointer and the column starts need the alignment of a double (8 bytes), nothing more. The
 * rows n .. ld-1 between two columns and everything before and behind the window are never read into a result and never written;
 * the input window is only read. Results do not depend on ld or on the alignment: a padded call returns the bits of the
 * contiguous one (tests/test_gpu_layout.py).
 * ALIASING: X may BE the input (X == B, or X == Z, the same pointer) when ldx == ldb: the solve then runs in place -- every pass of
 * 64 columns reads its columns before it writes them. Any other overlap of the two windows is not allowed and not detected. */
/* Q X = B. Replaces `F \ b` / `F \ B`: src/workspace/backend.jl:191-209. */
int32_t gmrfx_solve(gmrfx_handle *h, const double *B, int64_t ldb, int64_t nrhs, double *X, int64_t ldx);
int32_t gmrfx_solve_dev(gmrfx_handle *h, const double *d_B, int64_t ldb, int64_t nrhs, double *d_X, int64_t ldx);

/* X = P' L^-T Z (sampling). Replaces `F.UP \ z`: src/workspace/backend.jl:281-284,
 * src/solvers/backward_solve.jl:50-60. Batched over nrhs samples (the reference loops). */
int32_t gmrfx_backward_solve(gmrfx_handle *h, const double *Z, int64_t ldz, int64_t nrhs, double *X, int64_t ldx);
int32_t gmrfx_backward_solve_dev(gmrfx_handle *h, const double *d_Z, int64_t ldz, int64_t nrhs, double *d_X, int64_t ldx);

/* +log det Q = 2 sum log L_jj. Replaces `logdet(F)`: src/workspace/backend.jl:211-213
 * (seam A negates: src/solvers/logdet.jl:27-31). */
int32_t gmrfx_logdet(gmrfx_handle *h, double *out);

/* out[v] = (x_v - mu)' Q (x_v - mu) for the nvec columns of the column-major n x nvec X (mu: n values or NULL for a
 * zero mean), on Q's CSC values `nzval` (same order as the pattern given to gmrfx_create; NULL = the values of the
 * last refactorisation when the handle holds them, i.e. after gmrfx_refactorize or gmrfx_refactorize_update).
 * Replaces `dot(r, d.precision * r)` in logpdf(::WorkspaceGMRF, z), src/workspace/workspace_gmrf.jl:288-292, and
 * sqmahal, src/gmrf.jl:94-97; with gmrfx_refactorize_dev + gmrfx_logdet the hyper-parameter loop of
 * docs/src/literate-tutorials/workspace_factorization_reuse.jl:94-102 keeps Q and z in HBM. Only the stored triangle
 * that defines Q (gmrfx_opts.uplo) is read. Does not need a factorisation. The _dev form takes device pointers for
 * nzval, X and mu; out is a host array of nvec doubles in both. nvec <= 65535. */
int32_t gmrfx_quadform(gmrfx_handle *h, const double *nzval, const double *X, int64_t ldx, int64_t nvec,
                       const double *mu, double *out);
int32_t gmrfx_quadform_dev(gmrfx_handle *h, const double *d_nzval, const double *d_X, int64_t ldx, int64_t nvec,
                           const double *d_mu, double *out);

/* ---- dense-operator leg of the separable (Kronecker) path ---------------------------
 * `Q = kron(Q_1, Q_2)` (SeparableModel, src/latent_models/separable.jl:143-156; logdet rule :122-141): a solve / a sample of all
 * n1 n2 unknowns is ONE sweep over the large factor with n1 right-hand sides (the flat vector x[i1 n2 + i2] is its column-major
 * n2 x n1 panel) followed by the small factor applied as a DENSE n1 x n1 operator D (Q_1^-1, or P_1' L_1^-T for samples) to the
 * row-major n1 x n2 result T:  R = D T.  gmrfx_dense_apply_dev computes that product on the FP64 matrix cores with the library's
 * own kernels (csrc/dense.hip; no vendor GEMM). All three arrays are row-major device arrays, T and R must not overlap, and T
 * must be followed by at least 8 readable bytes when n2 is odd (16-byte operand loads). gmrfx_transpose_dev writes the
 * transpose of a row-major rows x cols device array (dst: cols x rows) -- the layout change between the two sweeps when BOTH
 * factors are large. `h` is any numeric handle of the device the arrays live on; both calls return when the result is complete. */
int32_t gmrfx_dense_apply_dev(gmrfx_handle *h, int64_t n1, int64_t n2, const double *d_D, const double *d_T, double *d_R);
int32_t gmrfx_transpose_dev(gmrfx_handle *h, int64_t rows, int64_t cols, const double *d_src, double *d_dst);

/* Takahashi selected inverse; computed lazily once per refactorisation and cached on the
 * device. Replaces SelectedInversion.selinv / selinv_diag: src/workspace/backend.jl:215-257,
 * src/solvers/selinv.jl:70-125. */
int32_t gmrfx_selinv_compute(gmrfx_handle *h);
int32_t gmrfx_selinv_diag(gmrfx_handle *h, double *out /* n, original ordering */);
/* Full selected inverse, original ordering, both triangles, rows sorted: the pattern of
 * (L+L') de-permuted (a superset of pattern(Q)). Two-call protocol: nnz, then fill. */
int32_t gmrfx_selinv_nnz(gmrfx_handle *h, int64_t *nnz);
int32_t gmrfx_selinv_csc(gmrfx_handle *h, int32_t index_base, int64_t *colptr, int64_t *rowval, double *nzval);
/* Sigma on a caller pattern, 0.0 outside the factor pattern. Replaces
 * SelectedInversion.selinv_extract(Z, B): src/workspace/backend.jl:275-279. */
int32_t gmrfx_selinv_extract(gmrfx_handle *h, int64_t ncol, const int64_t *colptr, const int64_t *rowval,
                             int32_t index_base, double *out_nzval);
/* Contractions with the selected inverse, reduced on the device (only the results cross PCIe).
 * gmrfx_selinv_dot: *out = sum over the stored entries of B (n columns, CSC) of Sigma_ij * B_ij = tr(Q^-1 B) for a
 * symmetric B whose pattern lies inside the factor pattern (entries outside it contribute 0). Replaces
 * selinv_dot(b, B) for Float64 B: src/workspace/backend.jl:258-267 (Dual-valued B: use gmrfx_selinv_extract and
 * contract in Julia).
 * gmrfx_selinv_row_diag: out[i] = sum_{p,q in row i} A_ip A_iq Sigma[j_p, j_q] = (A Sigma A')_ii for the m rows of a
 * sparse design matrix given by rows (CSR arrays = the CSC arrays of A'). Replaces _row_diag_AΣAt(A, Σ) /
 * selinv_extract_at(ws, A' * A): src/linear_predictor_marginals.jl:125-165. */
int32_t gmrfx_selinv_dot(gmrfx_handle *h, int64_t ncol, const int64_t *colptr, const int64_t *rowval,
                         const double *nzval, int32_t index_base, double *out);
int32_t gmrfx_selinv_row_diag(gmrfx_handle *h, int64_t m, const int64_t *rowptr, const int64_t *colind,
                              const double *values, int32_t index_base, double *out);
/* The same in two steps for a design matrix whose PATTERN stays fixed while Q changes (the hyper-parameter loop):
 * _plan looks the pairs up once and keeps them on the device (valid for the lifetime of the handle, across
 * refactorisations), _apply sends A's values (same order as colind) and returns the m variances, _free drops the plan. */
int32_t gmrfx_selinv_row_diag_plan(gmrfx_handle *h, int64_t m, const int64_t *rowptr, const int64_t *colind,
                                   int32_t index_base, int64_t *plan);
int32_t gmrfx_selinv_row_diag_apply(gmrfx_handle *h, int64_t plan, const double *values, double *out);
int32_t gmrfx_selinv_row_diag_free(gmrfx_handle *h, int64_t plan);

/* Elimination order actually used (index_base-based), so CHOLMOD can be run on the identical
 * P Q P' (`CHOLMODBackend(Q; ordering = perm)`, src/workspace/backend.jl:147-149). */
int32_t gmrfx_get_perm(const gmrfx_handle *h, int32_t index_base, int64_t *perm);
int32_t gmrfx_get_stats(const gmrfx_handle *h, gmrfx_stats *out, int32_t struct_size);

/* Symbolic structure, for tests and for tools that want the supernodal layout.
 * sizes[0..7] = {nsuper, sum_rows, nnz_l_stored, n_levels, cb_arena, nnz_q_used, 0, 0}. */
int32_t gmrfx_symbolic_sizes(const gmrfx_handle *h, int64_t *sizes);
/* Any pointer may be NULL. super_first: nsuper+1; super_parent: nsuper; row_ptr: nsuper+1;
 * rows: sum_rows (permuted indices); rel: sum_rows (position in parent's row list for the
 * rows below the diagonal block, -1 elsewhere); panel_ptr: nsuper+1 (offset in doubles);
 * panel_ld: nsuper; level: nsuper; q_src/q_dst: nnz_q_used (index into nzval -> offset in
 * panel storage). */
int32_t gmrfx_symbolic_get(const gmrfx_handle *h, int64_t *super_first, int64_t *super_parent,
                           int64_t *row_ptr, int64_t *rows, int64_t *rel, int64_t *panel_ptr,
                           int64_t *panel_ld, int64_t *level, int64_t *q_src, int64_t *q_dst);
/* Copy the numeric factor panels (nnz_l_stored doubles) to the host: tests compare them
 * with the oracle's L (unique for a given permutation). */
/* Sweep tasks (host analysis; testing / inspection): maximal bottom subtrees of the supernodal tree whose forward /
 * backward substitution one workgroup runs on an LDS-resident local vector (csrc/sweep_task.hip), so the update
 * vectors between their fronts never touch HBM. first / last: supernode range of each task (last = root), lrow: for
 * every entry of the supernode row lists, the local row inside its task (-1 outside tasks / for own rows). */
int32_t gmrfx_symbolic_sweep_tasks(const gmrfx_handle *h, int64_t *ntasks, int64_t *rows_cap, int64_t *first,
                                   int64_t *last, int64_t *lrow);
/* The tasks' CHUNKS (csrc/sweep_chunk.hip; host analysis, testing / inspection): every task front cut into column blocks
 * of at most 16 columns, each a narrow front of its own (targets = the panel rows below its diagonal block). nchunks (two
 * values: forward records -- a chunk with more than 128 target rows is several records -- and backward records = chunks) /
 * nrows always; when non-null: task_ptr (2 per task + 2: first forward / backward record of a task), slot (8 per task: chunks in the backward
 * program of row-tile slot 0..3, then the barriers each slot passes behind its last chunk), fwd / bwd (8 per chunk:
 * offset of (first target row, first column) in the factor storage, panel ld, local row of the first own column,
 * columns, target rows, offset of its padded target-row list in rows, barriers passed before it (backward programs),
 * number of the chunk; fwd = task by task in postorder, bwd = per task the programs of slot 0, 1, 2, 3), rows
 * (nrows: local rows of the targets, every list padded with -1 to a multiple of 32). */
int32_t gmrfx_symbolic_sweep_chunks(const gmrfx_handle *h, int64_t *nchunks, int64_t *nrows, int64_t *task_ptr,
                                    int64_t *slot, int64_t *fwd, int64_t *bwd, int64_t *rows);
int32_t gmrfx_get_factor_values(gmrfx_handle *h, double *out);

/* ---- batched handles: B precisions with ONE pattern, factored in one pass ------------------------------------------------------
 * The hyper-parameter loop evaluates logpdf for many values of one pattern (docs/src/literate-tutorials/workspace_factorization_reuse.jl:
 * 50 values of a 100 x 100 grid; INLA / marginal-likelihood / HMC loops), and WorkspacePool (src/workspace/workspace_pool.jl:5-22)
 * exists to run such evaluations side by side -- CHOLMOD serialises them behind a global lock. A batched handle holds B MEMBERS:
 * one pattern Q and one elimination order, B sets of values. Internally it is an ordinary handle of the block-diagonal matrix
 * diag(Q_1 .. Q_B), whose elimination forest is B copies of the member's tree on the same levels: every level launch does B times
 * the work of one member, with the same kernels.
 * gmrfx_create_batched: n, colptr, rowval, perm and opts.coords describe ONE member (the order is computed once, on the member, and
 * replicated: perm[k n + i] = k n + perm_1[i]). INVALID_ARG (message in gmrfx_last_create_error, nothing allocated) for nbatch < 1,
 * nbatch n > INT32_MAX, or sharding options (shard_world > 1, shard_min_top > 0). gmrfx_stats then describe the forest: n, nnz_l,
 * nsuper, factor_flops, bytes_factor and bytes_cb_arena are B times the member's (also for symbolic_only handles: size B with them
 * before building a numeric handle), nlevels is the member's.
 * gmrfx_batch_size: *nbatch = B, *n_member = n (1 and n for a plain handle; the batch entry points treat it as a batch of one).
 * gmrfx_batch_refactorize(_dev): nzval = nnz x B column-major, member k's values in the member's CSC order at nzval + k nnz (which
 *   is the forest's CSC value array). info[k] <- 0, or 1 + the first member-local pivot column (elimination order) that failed --
 *   what a plain handle reports for that member's values alone. A failing member does not disturb the others. check_posdef = 1:
 *   GMRFX_ERR_NOT_POSDEF when any member fails; info is filled in either way.
 * gmrfx_batch_logdet: out[k] = log det Q_k.
 * gmrfx_batch_solve(_dev): X_k = Q_k^-1 B_k; gmrfx_batch_backward_solve(_dev): X_k = P' L_k^-T Z_k (Z_k in the member's elimination
 *   order). Member k's n x nrhs block of B (Z) / X at B + k sb / X + k sx, leading dimension ldb / ldx >= n, stride >= ld nrhs.
 * gmrfx_batch_quadform(_dev): quad[k nvec + v] = (x_vk - mu_k)' Q_k (x_vk - mu_k) (quad: host array nvec x B), x_vk at X + k sx + v ldx,
 *   mu_k at mu + k n (mu: n x B, nullable), Q_k's values at nzval + k nnz (NULL: the values of the last host refactorisation), the
 *   stored triangle chosen by opts.uplo as in gmrfx_quadform; one launch for all members.
 * gmrfx_batch_refactorize_logpdf_dev: the batched gmrfx_refactorize_logpdf_dev -- refactorisation of all members, their quadratic forms
 *   beside it on the side stream, per-member log det and info, one synchronisation; quad (nvec x B), logdet (B), info (B) are host
 *   arrays. Same bits as gmrfx_batch_refactorize_dev + gmrfx_batch_quadform_dev + gmrfx_batch_logdet.
 * Every other entry point keeps its meaning on a batched handle and acts on the block-diagonal matrix of size B n: gmrfx_logdet is
 * the sum over the members, gmrfx_selinv_diag returns the n x B matrix of member variances, gmrfx_get_perm the forest's order,
 * gmrfx_clone copies the batch (Newton loops clone). The Newton entry points (gmrfx_set_prior, gmrfx_refactorize_update*) take
 * forest-wide index maps. */
int32_t gmrfx_create_batched(int64_t n, const int64_t *colptr, const int64_t *rowval, int32_t index_base, const int64_t *perm,
                             int64_t nbatch, const gmrfx_opts *opts, gmrfx_handle **out);
int32_t gmrfx_batch_size(const gmrfx_handle *h, int64_t *nbatch, int64_t *n_member);
int32_t gmrfx_batch_refactorize(gmrfx_handle *h, const double *nzval, int64_t *info /* nbatch, nullable */);
int32_t gmrfx_batch_refactorize_dev(gmrfx_handle *h, const double *d_nzval, int64_t *info /* nbatch, nullable */);
int32_t gmrfx_batch_logdet(gmrfx_handle *h, double *out /* nbatch */);
int32_t gmrfx_batch_solve(gmrfx_handle *h, const double *B, int64_t ldb, int64_t sb, int64_t nrhs, double *X, int64_t ldx, int64_t sx);
int32_t gmrfx_batch_solve_dev(gmrfx_handle *h, const double *d_B, int64_t ldb, int64_t sb, int64_t nrhs, double *d_X, int64_t ldx, int64_t sx);
int32_t gmrfx_batch_backward_solve(gmrfx_handle *h, const double *Z, int64_t ldz, int64_t sz, int64_t nrhs, double *X, int64_t ldx, int64_t sx);
int32_t gmrfx_batch_backward_solve_dev(gmrfx_handle *h, const double *d_Z, int64_t ldz, int64_t sz, int64_t nrhs, double *d_X, int64_t ldx,
                                       int64_t sx);
int32_t gmrfx_batch_quadform(gmrfx_handle *h, const double *nzval, const double *X, int64_t ldx, int64_t sx, int64_t nvec,
                             const double *mu, double *quad);
int32_t gmrfx_batch_quadform_dev(gmrfx_handle *h, const double *d_nzval, const double *d_X, int64_t ldx, int64_t sx, int64_t nvec,
                                 const double *d_mu, double *quad);
int32_t gmrfx_batch_refactorize_logpdf_dev(gmrfx_handle *h, const double *d_nzval, const double *d_X, int64_t ldx, int64_t sx, int64_t nvec,
                                           const double *d_mu, double *quad /* host, nvec x nbatch */, double *logdet /* host, nbatch */,
                                           int64_t *info /* host, nbatch, nullable */);

/* ---- linear equality constraints A x = e, computed on the device -----------------------------------------------------------------
 * Conditioning by kriging (Rue & Held 2005, section 2.3.3) as `ConstraintInfo` / `WorkspaceGMRF` do it on the host,
 * src/workspace/workspace_gmrf.jl:22-56 (the blocked solve A~' = Q^-1 A', the m x m Cholesky L_c of W = A A~', the constrained mean and
 * the log-density correction), :260-273 (variance correction), :280-284 (per-sample correction). A constraint is STATE of a handle,
 * like the prior of the Newton loop: set once, everything derived from it is computed lazily on the device once per factorisation
 * (zero + scatter of A' on the device, ONE blocked solve through the gmrfx_solve_dev path -- gmrfx_stats.last_nrhs then reads m --,
 * W by a deterministic reduction, L_c and L_c^-1 on the host, B = A~' L_c^-T on the device), kept there (A~' and B, 2 x 8 n m bytes)
 * and dropped by every refactorisation, like the selected-inverse cache. A handle without constraints behaves exactly as before.
 * LIMIT: m <= 64 rows -- the blocked solve is then one sweep pass and the m x m operands of the correction kernels live in LDS.
 * Callers with more rows keep their host path. Every sum is formed in a fixed order without atomics: results are bit-reproducible
 * from run to run and do not depend on leading dimensions or on the alignment of the caller's arrays.
 *
 * gmrfx_constraints_set: A as m sparse rows (CSR arrays = the CSC arrays of A', what `sparse(A')` holds), e: m values; duplicates within
 *   a row are summed; m = 0 removes the constraint. The handle keeps A (on the device with 32-bit columns), e and the host-computed
 *   log det(A A') (:51). GMRFX_ERR_INVALID_ARG with a message and NOTHING changed for: a column outside [0, n), a non-monotone rowptr,
 *   m > 64, an empty row, a batched handle (gmrfx_batch_size > 1; see gmrfx_batch_constraints_set), a sharded handle. Works on symbolic_only handles (validation;
 *   numeric use there returns GMRFX_ERR_NO_DEVICE). gmrfx_clone carries A and e; the clone recomputes what is derived.
 * gmrfx_constraints_info: *m (0 without a constraint, the other outputs are then 0), *logdet_AAt, and -- these two trigger the
 *   preparation when they are asked for (non-null) -- *logdet_W = log det(A Q^-1 A') = logdet(L_c) (:50) and *ms = GPU time of the most
 *   recent preparation. Any pointer may be NULL. gmrfx_stats is unchanged.
 * gmrfx_constraints_get: host copies of A~' (n x m column-major, leading dimension ld) and W (m x m), either nullable: the fields
 *   A_tilde_T and L_c (= cholesky(Symmetric(W))) of the Julia ConstraintInfo (:37-40).
 * gmrfx_constraints_mean: mean_c = mu - A~' W^-1 (A mu - e) (:43-44; mu NULL = 0, mean_c nullable) and *log_correction =
 *   0.5 (m log 2 pi + log det W + r' W^-1 r) - 0.5 log det(A A'), r = e - A mu (:46-51). Host arrays.
 * gmrfx_constraints_correct(_dev): in place X <- X - A~' W^-1 (A X - e) on all nvec >= 1 columns (column-major, ldx >= n): :280-284
 *   applied to a block. A no-op without a constraint.
 * gmrfx_constraints_var: out[i] = max(Sigma_ii - sum_j B_ij^2, 0), B = A~' L_c^-T (:260-273); uses the cached selected inverse and
 *   computes it if absent. Without a constraint: gmrfx_selinv_diag, bit for bit.
 * gmrfx_sample(_dev): `_rand!` (:275-286) in one call: X = P' L^-T Z + mu (mu nullable, n values), then the correction when a
 *   constraint is set. Without a constraint and with mu = NULL the result has the bits of gmrfx_backward_solve(_dev).
 * Errors: GMRFX_ERR_NOT_FACTORIZED before the first factorisation; GMRFX_ERR_NOT_POSDEF when W is not positive definite -- a
 *   rank-deficient A, where the reference throws PosDefException from cholesky (:40); a pivot below 16 m eps W_jj counts as zero.
 *   The handle stays usable. */
int32_t gmrfx_constraints_set(gmrfx_handle *h, int64_t m, const int64_t *rowptr, const int64_t *colind, const double *values,
                              int32_t index_base, const double *e);
int32_t gmrfx_constraints_info(gmrfx_handle *h, int64_t *m, double *logdet_W, double *logdet_AAt, double *ms);
int32_t gmrfx_constraints_get(gmrfx_handle *h, double *A_tilde_T /* n x m, nullable */, int64_t ld, double *W /* m x m, nullable */);
int32_t gmrfx_constraints_mean(gmrfx_handle *h, const double *mu /* n, nullable = 0 */, double *mean_c /* n, nullable */,
                               double *log_correction /* nullable */);
int32_t gmrfx_constraints_correct(gmrfx_handle *h, double *X, int64_t ldx, int64_t nvec);
int32_t gmrfx_constraints_correct_dev(gmrfx_handle *h, double *d_X, int64_t ldx, int64_t nvec);
int32_t gmrfx_constraints_var(gmrfx_handle *h, double *out /* n */);
int32_t gmrfx_sample(gmrfx_handle *h, const double *Z, int64_t ldz, int64_t nrhs, const double *mu /* nullable */, double *X, int64_t ldx);
int32_t gmrfx_sample_dev(gmrfx_handle *h, const double *d_Z, int64_t ldz, int64_t nrhs, const double *d_mu /* nullable */, double *d_X,
                         int64_t ldx);

/* ---- the same constraint for every member of a batched handle ---------------------------------------------------------------------
 * The intrinsic latent models of the hyper-parameter loop (Besag, RW1, RW2, BYM2) come with a sum-to-zero constraint, and its
 * log-density term log_constraint_correction (src/workspace/workspace_gmrf.jl:46-51, 288-305) depends on Q through W = A Q^-1 A':
 * it differs for every member. A batched handle therefore takes ONE A (m <= 64 sparse rows over the MEMBER's n columns) and ONE e,
 * shared by all B members, and computes everything derived from them PER MEMBER on the device, once per factorisation: memset +
 * scatter of A' into B blocks in one launch, ONE forest solve of m columns (the gmrfx_batch_solve_dev path), W_k = A A~'_k by the
 * deterministic chunked reduction, then one workgroup per member for the Cholesky factor L_ck of W_k, its inverse, log det W_k and the
 * status word (no download of W, no host loop over the members), and B_k = A~'_k L_ck^-T. Member k's A~'_k and B_k are n x m
 * column-major blocks at k n m of two device arrays (2 x 8 n B m bytes). Cached per factorisation and dropped by every
 * refactorisation. Same determinism as above: fixed summation orders, no atomics, bits independent of ldx, sx and alignment.
 * A plain (unsharded) handle is a batch of one, as for the other gmrfx_batch_* calls. A handle holds at most ONE kind of constraint:
 * gmrfx_batch_constraints_set while a plain constraint is set, or gmrfx_constraints_set while a batch constraint is set, is
 * GMRFX_ERR_INVALID_ARG. gmrfx_constraints_set keeps refusing handles with more than one member.
 *
 * gmrfx_batch_constraints_set: CSR conventions and validation of gmrfx_constraints_set, columns in [0, n_member); duplicates are
 *   summed; m = 0 clears. GMRFX_ERR_INVALID_ARG with a message and NOTHING changed for invalid input or a sharded handle;
 *   GMRFX_ERR_ALLOC, nothing changed, when the two operand arrays do not fit. Works on symbolic_only handles. gmrfx_clone carries A
 *   and e; the clone recomputes what is derived.
 * gmrfx_batch_constraints_info: *m, *logdet_AAt, and -- these trigger the preparation when asked for -- logdet_W[k] = log det W_k,
 *   cinfo[k] = 0, or 1 + j when pivot j of W_k fails (a pivot not above 16 m eps |W_jj|), or -1 when member k's factorisation itself
 *   failed (member k's outputs are then NaN everywhere), *ms = GPU time of the most recent preparation. Any pointer may be NULL.
 * gmrfx_batch_constraints_get: host copies of member `member`'s A~' (n x m, leading dimension ld) and W (m x m), either nullable.
 * gmrfx_batch_constraints_mean: per member the two quantities of gmrfx_constraints_mean: mean_c (n x B) = mu_k - A~'_k W_k^-1 (A mu_k - e)
 *   (mu: n x B, NULL = 0) and log_correction[k]; r_k' W_k^-1 r_k = |L_ck^-1 r_k|^2 is formed on the device. Host arrays, each nullable.
 * gmrfx_batch_constraints_correct(_dev): in place X_k <- X_k - A~'_k W_k^-1 (A X_k - e) on the members' n x nvec blocks at X + k sx,
 *   leading dimension ldx (layout of gmrfx_batch_solve). A no-op without a constraint.
 * gmrfx_batch_sample(_dev): X_k = P' L_k^-T Z_k + mu_k (mu: n x B, nullable), then the correction. Without a constraint and with
 *   mu = NULL the result has the bits of gmrfx_batch_backward_solve(_dev).
 * gmrfx_batch_constraints_var: out (n x B) = max(Sigma_ii - sum_j B_ij^2, 0) per member; without a constraint gmrfx_selinv_diag,
 *   bit for bit.
 * gmrfx_batch_constrained_logpdf_dev: the constrained twin of gmrfx_batch_refactorize_logpdf_dev: refactorisation, the quadratic forms
 *   beside it, per-member log det and info, the preparation above, and log_correction[k] with r_k = e - A mu_k. quad, logdet and info
 *   have the bits of gmrfx_batch_refactorize_logpdf_dev, log_correction those of gmrfx_batch_constraints_mean after the same
 *   refactorisation. log_correction (B), info (B) and cinfo (B) are host arrays, each nullable.
 * Errors: GMRFX_ERR_NOT_FACTORIZED before the first factorisation, GMRFX_ERR_NO_DEVICE on symbolic_only handles.
 *   GMRFX_ERR_NOT_POSDEF when W_k fails for a member whose factorisation succeeded (a rank-deficient A): cinfo is filled in either
 *   way and the handle stays usable. A member whose factorisation failed is reported through cinfo only (and through info / the
 *   handle's check_posdef by the factorising call); it never disturbs another member. */
int32_t gmrfx_batch_constraints_set(gmrfx_handle *h, int64_t m, const int64_t *rowptr, const int64_t *colind, const double *values,
                                    int32_t index_base, const double *e);
int32_t gmrfx_batch_constraints_info(gmrfx_handle *h, int64_t *m, double *logdet_W /* nbatch */, double *logdet_AAt,
                                     int64_t *cinfo /* nbatch */, double *ms);
int32_t gmrfx_batch_constraints_get(gmrfx_handle *h, int64_t member, double *A_tilde_T /* n x m, nullable */, int64_t ld,
                                    double *W /* m x m, nullable */);
int32_t gmrfx_batch_constraints_mean(gmrfx_handle *h, const double *mu /* n x nbatch, nullable = 0 */, double *mean_c /* n x nbatch, nullable */,
                                     double *log_correction /* nbatch, nullable */);
int32_t gmrfx_batch_constraints_correct(gmrfx_handle *h, double *X, int64_t ldx, int64_t sx, int64_t nvec);
int32_t gmrfx_batch_constraints_correct_dev(gmrfx_handle *h, double *d_X, int64_t ldx, int64_t sx, int64_t nvec);
int32_t gmrfx_batch_constraints_var(gmrfx_handle *h, double *out /* n x nbatch */);
int32_t gmrfx_batch_sample(gmrfx_handle *h, const double *Z, int64_t ldz, int64_t sz, int64_t nrhs, const double *mu /* n x nbatch, nullable */,
                           double *X, int64_t ldx, int64_t sx);
int32_t gmrfx_batch_sample_dev(gmrfx_handle *h, const double *d_Z, int64_t ldz, int64_t sz, int64_t nrhs,
                               const double *d_mu /* n x nbatch, nullable */, double *d_X, int64_t ldx, int64_t sx);
int32_t gmrfx_batch_constrained_logpdf_dev(gmrfx_handle *h, const double *d_nzval, const double *d_X, int64_t ldx, int64_t sx, int64_t nvec,
                                           const double *d_mu, double *quad /* host, nvec x nbatch */, double *logdet /* host, nbatch */,
                                           double *log_correction /* host, nbatch, nullable */, int64_t *info /* host, nbatch, nullable */,
                                           int64_t *cinfo /* host, nbatch, nullable */);

/* KL-optimal sparse approximate Cholesky factor, L L' ~ Theta^-1: a batch of small dense problems, one
 * workgroup each. A task = local rows R (task_rows[task_rowptr[t] .. task_rowptr[t+1]), in the caller's local order)
 * + the columns of L it fills (task_cols[task_colptr[t] ..)): M = Theta[R, R] + reg I = U'U, and for every member
 * column k with N_k = nnz(L[:, k]) <= |R|: U x = e_{N_k}, nzval[column k] = x[N_k : -1 : 1].
 *   - sparse_approximate_cholesky!(Theta, L), src/kl_cholesky/kl_cholesky.jl:32-55: one task per column, R = the
 *     column's row indices in DESCENDING order, reg = 1e-6;
 *   - sparse_approximate_cholesky(Theta, sc::SupernodeClustering), :74-113: one task per supernode, R = its rows
 *     (descending), member columns = sc.column_indices[s], reg = 1e-8.
 * Theta: dense n x n column-major (leading dimension ldt), host or device memory (theta_on_device); L_colptr: the n+1
 * column pointers of the pattern of L; nzval: host array of nnz(L) doubles, written in L's storage order. A local block
 * that is not positive definite gives GMRFX_ERR_NOT_POSDEF and *info = 1 + task index (the reference throws
 * PosDefException from cholesky!). No handle: errors are reported through gmrfx_last_create_error(). GPU only. */
int32_t gmrfx_kl_cholesky(int64_t n, const double *theta, int64_t ldt, int32_t theta_on_device,
                          const int64_t *L_colptr, int64_t ntasks, const int64_t *task_rowptr, const int64_t *task_rows,
                          const int64_t *task_colptr, const int64_t *task_cols, int32_t index_base, double reg,
                          int32_t device, double *nzval, int64_t *info);

/* ---- Rao-Blackwellised Monte Carlo marginal variances ---------------------------------------------------------------------------
 * The reference's second way to marginal variances beside selected inversion, "in large-scale regimes where Takahashi recursions
 * may be too expensive": `var(d, RBMCStrategy(k))` and `var(d, BlockRBMCStrategy(k; enclosure_size))`, src/solvers/rbmc.jl:71-87
 * and :90-158, reached on seam A through src/gmrf.jl:318-332. There: k single-vector rand! calls, a host SpMM, and for the block
 * form one CHOLMOD factorisation per block. Here: the k-column backward sweep in blocks of 64 samples, a symmetric SpMM fused with
 * a per-row running variance, and one workgroup per block (gather Q_BB, Cholesky, substitutions, reduction over the samples).
 * X = P' L^-T Z are the centred samples (`rand!` minus the mean, gmrf.jl:275-281); the caller supplies the standard normals Z
 * (n x nsamples column-major, leading dimension ldz) -- there is no RNG in the library, as for gmrfx_sample. Variances over samples
 * are corrected (divisor nsamples - 1, Julia's `var(...; dims = 2)`).
 *   plain (enclosure_size = -1):  out_i = 1 / D_i + Var_s( (sum_{j != i} Q_ij X_js) / D_i ),  D = diag(Q)
 *   block (enclosure_size >= 0):  `_build_disjoint_subsets` (:106-117) walks i = 1..n; an unvisited i opens a subset S = all stored
 *     neighbours of i (row i of Q: i itself and explicit zeros included), visited or not -- the subsets OVERLAP, and
 *     `var_estimate[interior] .=` (:151) lets the LAST subset that holds a node decide its value. B = S + enclosure_size
 *     breadth-first rings (`_build_enclosure_idcs`, :93-104); out_i = (Q_BB^-1)_ii + Var_s( [Q_BB^-1 Q_{B,out} X_out]_i ), i in S.
 *     (The two symamd calls, :140-144, reorder rows inside a block and do not change these values: not reproduced.)
 * Q is Symmetric(Q) with the handle's uplo, as for gmrfx_quadform: neighbours and values come from the stored triangle that defines
 * Q, mirrored; the other triangle is ignored even where it is stored. nzval: Q's CSC values (NULL = the values of the last
 * refactorisation when the handle holds them, as gmrfx_quadform; a clone does not hold them).
 * Device memory is O(64 n) for any nsamples. Every sum is formed in an order that depends on indices only, without atomics: results
 * are bit-reproducible from run to run and do not depend on ldz or on the alignment of Z; the host and the _dev form agree bit for
 * bit. A non-positive pivot in a block (rounding only: a principal block of a positive definite Q is positive definite) makes that
 * block's outputs NaN. On a batched handle the calls act on the block-diagonal forest: Z and out have B n rows.
 * LIMIT: a block of more than 512 rows is GMRFX_ERR_INVALID_ARG (the message names the block and its size); the limit of
 * gmrfx_kl_cholesky. Also INVALID_ARG, with a message and nothing changed: nsamples < 2 (the reference would return NaN), ldz < n,
 * enclosure_size < -1, a sharded handle, a handle with a constraint set (plain or batch: the constrained estimator is not
 * implemented). GMRFX_ERR_NOT_FACTORIZED before the first factorisation, GMRFX_ERR_NOT_POSDEF when the last factorisation reported
 * a failed pivot, GMRFX_ERR_NO_DEVICE for numeric use of a symbolic_only handle. gmrfx_stats.ms_rbmc: GPU time of the last call. */
/* enclosure_size = -1: RBMCStrategy; >= 0: BlockRBMCStrategy with that enclosure. nzval: Q's CSC values
 * (NULL = the values of the last refactorisation when the handle holds them, as gmrfx_quadform). */
int32_t gmrfx_rbmc_var(gmrfx_handle *h, const double *nzval, const double *Z, int64_t ldz, int64_t nsamples,
                       int32_t enclosure_size, double *out /* n, host */);
int32_t gmrfx_rbmc_var_dev(gmrfx_handle *h, const double *d_nzval, const double *d_Z, int64_t ldz, int64_t nsamples,
                           int32_t enclosure_size, double *d_out /* n, device */);
/* Host analysis only (works on symbolic_only handles). Two-call protocol like gmrfx_symbolic_sweep_chunks:
 * counts[0] blocks, [1] total rows, [2] largest block; block_ptr (blocks+1), rows (S first, index_base-based),
 * n_interior (blocks), owner (total rows: 1 where this block writes the node, else 0; 0 for enclosure rows). */
int32_t gmrfx_rbmc_plan(gmrfx_handle *h, int32_t enclosure_size, int32_t index_base, int64_t *counts,
                        int64_t *block_ptr, int64_t *rows, int64_t *n_interior, int64_t *owner);

/* ---- Log-density gradients on Q's own pattern -------------------------------------------------------------------------------------
 * The array arithmetic of the reference's logpdf / logdetcov pullbacks (src/autodiff/logpdf.jl:63-90, src/autodiff/logdetcov.jl:14-18,
 * src/autodiff/precision_gradient.jl, src/workspace/autodiff.jl:14-50), formed on the device and only on the stored entries of Q --
 * the cotangent is contracted with a dQ/dtheta that lives there:
 *   Qbar[e] = c (Sigma_ij - r_i r_j) - c (sum_k B_ik B_jk - u_i u_j)     e = (i, j) a stored entry,  c = ybar / 2,  r = z - mu
 *   mubar   = ybar Q r - ybar A' W^-1 (e - A mu)                          (zbar = -mubar)
 * Sigma = Q^-1 (the selected inverse: computed if absent, cached per factorisation), and with a constraint A x = e set
 * (gmrfx_constraints_set or gmrfx_batch_constraints_set; the second terms exist only then) B = Q^-1 A' L_c^-T, L_c L_c' = W = A Q^-1 A',
 * u = B L_c^-1 (e - A mu): the outputs are then the gradient of logpdf + log_correction (gmrfx_constraints_mean), src/workspace/
 * autodiff.jl:24-37. An entry gets its value whichever triangle it lies in (opts.uplo does not matter for Qbar); the first term is
 * computed as c * (Sigma_ij - r_i * r_j), in that association. mubar uses Symmetric(Q) as gmrfx_quadform does: the triangle not in use
 * is never read. nzval: Q's CSC values, only read for mubar (NULL = the values of the last refactorisation when the handle holds them,
 * as gmrfx_quadform; INVALID_ARG when it holds none). mu NULL = zero mean. Qbar (nnz, in the pattern's order) and mubar (n) are each
 * nullable (not computed), not both.
 * gmrfx_pattern_dot: out[k] = sum_e w_e G[e] J[e + k ldj], k < p -- dlogpdf/dtheta_k from G = Qbar and the Jacobian J of Q's stored
 * values (nnz x p column-major, ldj >= nnz); w_e are the weights of gmrfx_quadform: 1 on the diagonal, 2 off the diagonal in the
 * triangle that defines Q and 0 in the other one. Only p numbers cross PCIe. Needs no factorisation.
 * Batch forms: member k's values / Qbar at + k nnz, mu / mubar at + k n, z at + k sz, J at + k sj; ybar, info and out (p x nbatch) are
 * host arrays. A plain handle is a batch of one. A member whose factorisation or whose W_k failed gets NaN in its own outputs and
 * info[k] = -1 resp. 1 + the failing pivot of W_k (as gmrfx_batch_constraints_info); nobody else's outputs are disturbed. With
 * info = NULL such a member makes the call return GMRFX_ERR_NOT_POSDEF, as a failed factorisation or W does for the plain forms.
 * No atomics: every sum is formed in an order that depends on indices only; results are bit-reproducible, independent of sz and of the
 * alignment of the operands, the host and the _dev forms agree bit for bit, and member k of a batch equals a plain handle on Q_k.
 * Errors: GMRFX_ERR_INVALID_ARG with a message for sharded handles, the plain forms on a batched handle, p < 1, ldj < nnz, member
 * strides that overlap, null required pointers; GMRFX_ERR_NOT_FACTORIZED before the first factorisation (gradient forms);
 * GMRFX_ERR_NO_DEVICE for symbolic_only handles. LIMITS: one z per call, m <= 64 constraint rows, p <= 65535. */
int32_t gmrfx_pattern_nnz(const gmrfx_handle *h, int64_t *nnz /* stored entries of the (member's) pattern: the length of Qbar / G */);
int32_t gmrfx_logpdf_grad(gmrfx_handle *h, const double *nzval /* nullable */, const double *z, const double *mu /* nullable */, double ybar,
                          double *Qbar /* nnz, nullable */, double *mubar /* n, nullable */);
int32_t gmrfx_logpdf_grad_dev(gmrfx_handle *h, const double *d_nzval, const double *d_z, const double *d_mu, double ybar, double *d_Qbar,
                              double *d_mubar);
int32_t gmrfx_pattern_dot(gmrfx_handle *h, const double *G /* nnz */, const double *J, int64_t ldj, int64_t p, double *out /* host, p */);
int32_t gmrfx_pattern_dot_dev(gmrfx_handle *h, const double *d_G, const double *d_J, int64_t ldj, int64_t p, double *out /* host, p */);
int32_t gmrfx_batch_logpdf_grad(gmrfx_handle *h, const double *nzval /* nnz x nbatch, nullable */, const double *z, int64_t sz,
                                const double *mu /* n x nbatch, nullable */, const double *ybar /* host, nbatch */,
                                double *Qbar /* nnz x nbatch, nullable */, double *mubar /* n x nbatch, nullable */,
                                int64_t *info /* host, nbatch, nullable */);
int32_t gmrfx_batch_logpdf_grad_dev(gmrfx_handle *h, const double *d_nzval, const double *d_z, int64_t sz, const double *d_mu,
                                    const double *ybar /* host, nbatch */, double *d_Qbar, double *d_mubar, int64_t *info /* host, nbatch, nullable */);
int32_t gmrfx_batch_pattern_dot(gmrfx_handle *h, const double *G /* nnz x nbatch */, const double *J, int64_t ldj, int64_t sj, int64_t p,
                                double *out /* host, p x nbatch */);
int32_t gmrfx_batch_pattern_dot_dev(gmrfx_handle *h, const double *d_G, const double *d_J, int64_t ldj, int64_t sj, int64_t p,
                                    double *out /* host, p x nbatch */);

/* ---- Fisher scoring on the device: the observation likelihood as state of a plain handle, one fused evaluation ----------------------
 * What the reference's Gaussian-approximation loop (src/workspace/gaussian_approximation.jl:191-313, line search and merit:
 * src/arithmetic/condition/gaussian_approximation.jl:231-409) computes on the host at every iterate besides the factorisation --
 * loggrad, loghessian, loglik, Q_p x - h -- for the pointwise exponential-family likelihoods with a canonical or log link
 * (src/observation_models/exponential_family/canonical_implementations.jl:146-327, helpers.jl:5-31). eta_i = x[indices[i]]:
 *   family  0 Normal / identity      param sigma                  g = (y - eta) / sigma^2          d = -1 / sigma^2
 *           1 Poisson / log          aux = log exposure (NULL 0)  g = y - mu, mu = exp(eta + aux)  d = -mu
 *           2 Bernoulli / logit                                   g = y - mu, mu = logistic(eta)   d = -mu (1 - mu)
 *           3 Binomial / logit       aux = trials (required)      g = y - n mu                     d = -n mu (1 - mu)
 *           4 NegBinomial / log      aux = log exposure, param r  g = r (y - mu) / (r + mu)        d = -r mu (r + y) / (r + mu)^2
 *           5 Gamma / log            param phi                    g = phi (y / mu - 1)             d = -phi y / mu
 * g = dl/deta, d = d2l/deta2, l the log density of one observation; a node without an observation has g = d = l = 0 exactly
 * (_embed_grad, _embed_diag). Every term is evaluated in a form that is stable for every eta (csrc/fisher_point.h, "STABLE FORMS").
 * gmrfx_obs_set validates, sums the terms of loglik that do not depend on x in long double (loglik_const: -lgamma(y + 1), the
 * binomial coefficients, the Normal / NegBinomial / Gamma constants) and expands y, aux and an observed mask to one value per node
 * on the device. indices NULL = nodes 1 .. n in order (needs nobs == n). nobs = 0 removes the likelihood. gmrfx_clone carries it.
 * Works on symbolic_only handles (validation and loglik_const only). gmrfx_obs_info: family (-1: none), nobs, loglik_const; each nullable.
 * Refused with GMRFX_ERR_INVALID_ARG, a message and nothing changed: an unknown family, nobs outside [0, n], an index outside the
 * range, a node observed twice (the reference's g[indices] .= g_obs would silently keep the last), indices == NULL with nobs != n,
 * no aux for the binomial family, sigma / r / phi not positive, y (or aux) not finite, a negative count, a Bernoulli y above 1,
 * y above the number of trials, a Gamma y that is not positive, a batched handle (gmrfx_batch_size > 1), a sharded handle.
 * gmrfx_fisher_eval: at the point x, with Q_p the values gmrfx_set_prior keeps, h = Q_p mu (mu NULL: h = 0), in one pass over
 * Symmetric(Q_p) (the triangle not in use is never read):
 *   score_i = ((Q_p x)_i - h_i) - g_i(x_i)     the reference's neg_score_k; n values, nullable (not computed)
 *   hess_i  = d_i(x_i)                          n values, nullable: the hvals of gmrfx_refactorize_update under the diagonal map
 *   out[0]  = sum_i (0.5 x_i (Q_p x)_i - x_i h_i) = 1/2 x' Q_p x - x' h;   out[1] = loglik(x), loglik_const included
 * in these associations. No atomics: every sum is formed in an order that depends on indices only; results are bit-reproducible,
 * independent of the alignment of the operands, and the host and the _dev forms agree bit for bit. Needs no factorisation and leaves
 * the handle's factorisation as it is.
 * Errors: GMRFX_ERR_INVALID_ARG with a message when x or out is null, no likelihood is set, gmrfx_set_prior has not been called or
 * was called with a map that is not "the position of (i, i) for every i" (cnt == n: diagonal Hessians only), a batched or sharded
 * handle; GMRFX_ERR_NO_DEVICE for symbolic_only handles (after the argument checks that need no device state).
 * LIMITS: plain handles, n < 2^31; pointwise likelihoods with a diagonal Hessian here, Hessians A' D A in the design form below.
 * Student-t (not concave), LatentPrior and generic likelihoods stay on the gmrfx_refactorize_update path, driven from the host. */
int32_t gmrfx_obs_set(gmrfx_handle *h, int32_t family, int64_t nobs, const int64_t *indices /* nobs, nullable */, int32_t index_base,
                      const double *y /* nobs */, const double *aux /* nobs, nullable */, double param);
int32_t gmrfx_obs_info(const gmrfx_handle *h, int32_t *family, int64_t *nobs, double *loglik_const);
int32_t gmrfx_fisher_eval(gmrfx_handle *h, const double *x, const double *mu /* nullable */, double *score /* n, nullable */,
                          double *hess /* n (design form: cnt), nullable */, double *out /* host, 2: energy, loglik */);
int32_t gmrfx_fisher_eval_dev(gmrfx_handle *h, const double *d_x, const double *d_mu, double *d_score, double *d_hess,
                              double *out /* host, 2: energy, loglik */);
/* ---- the same through a sparse design matrix: eta = A x + b (LinearlyTransformedLikelihood, src/observation_models/
 * linearly_transformed.jl:313-340: loggrad = A' g(eta), loghessian = Symmetric(A' (D(eta) A))) ---------------------------------------
 * gmrfx_obs_set_design: A is nobs x n in CSC as Julia holds it (colptr n + 1, row indices sorted and unique within a column), offset
 * the nobs values of b (NULL: 0). Families, aux, param, loglik_const and every refusal are those of gmrfx_obs_set, except that two
 * rows may observe the same node, empty rows (eta_i = b_i) and untouched columns are allowed, nobs may exceed n (nobs >= 1) and
 * explicit zeros of A are kept as entries. Refused in addition (INVALID_ARG, a message, nothing changed): a colptr that is not
 * monotone or does not start at index_base, a row index outside [0, nobs), unsorted or repeated row indices within a column, a
 * non-finite value of A or offset, n / nobs / nnz(A) / the term count at 2^31 or above, and a pattern(A'A) that the handle's pattern
 * does not contain (the first missing (j, k) is named; the reference's _sparse_hessian_map throws there too).
 * The Hessian's positions are computed on the host, once: for every unordered pair (j, k) with a common row in A (j = k included) the
 * position in the handle's nzval of that entry in the triangle the handle reads, each pair once, in ascending position order.
 * gmrfx_obs_hess_map returns the list (cnt; map nullable, cnt values, 0-based): it is the map to give gmrfx_set_prior. With it the
 * plan keeps, for every position p, the terms (i_t, w_t = A[i_t, j] A[i_t, k]) in ascending i_t.
 * Setting one form replaces the other; gmrfx_obs_set with nobs = 0 removes either; gmrfx_clone carries the design form; symbolic_only
 * handles validate, give loglik_const and the map. gmrfx_obs_info keeps its meaning; gmrfx_obs_design_info: nnz(A), cnt and the term
 * count, each nullable, -1 each in node form or with no likelihood.
 * gmrfx_fisher_eval[_dev] in design form needs gmrfx_set_prior with exactly that map (INVALID_ARG otherwise) and returns
 *   score_j = ((Q_p x)_j - h_j) - (A' g(eta))_j    n values;        hess[p] = sum_t w_t d(eta_{i_t})    cnt values, the hvals of
 *   gmrfx_refactorize_update under that map;  out[0] as above;  out[1] = sum_i l_i(eta_i) + loglik_const.
 * No atomics; every sum in an order fixed by indices only (csrc/fisher_design.hip). With A = rows of the identity and no offset,
 * score, energy and the entries of hess have the bits of the node form. gmrfx_gaussian_approximation[_dev] runs the same loop; its
 * hess / d_hess output is then the cnt values in map order.
 * Memory of the plan on the device: A by rows and by columns, 12 B per entry each, and 12 B per term (32-bit observation, weight).
 * LIMITS: plain handles; sparse A; a theta-dependent A is set again by the caller (same pattern, same map). */
int32_t gmrfx_obs_set_design(gmrfx_handle *h, int32_t family, int64_t nobs, const int64_t *colptr /* n + 1 */, const int64_t *rowval,
                             const double *nzval, int32_t index_base, const double *offset /* nobs, nullable */, const double *y /* nobs */,
                             const double *aux /* nobs, nullable */, double param);
int32_t gmrfx_obs_hess_map(const gmrfx_handle *h, int64_t *cnt, int64_t *map /* nullable; cnt values, index base 0 */);
int32_t gmrfx_obs_design_info(const gmrfx_handle *h, int64_t *nnz_a, int64_t *cnt, int64_t *terms);
/* ---- composite likelihoods: several observation families on one handle (CompositeObservationModel / CompositeLikelihood,
 * src/observation_models/composite/: loglik, loggrad and loghessian are sums over the components, pointwise_loglik their
 * concatenation) -- Normal measurements next to Poisson counts, a Bernoulli presence part next to a Gamma amount part, two Normal data
 * sets with different sigmas ----------------------------------------------------------------------------------------------------------
 * gmrfx_obs_set_composite: A is the STACKED nobs x n design matrix [A_1; ...; A_C] in CSC, exactly as gmrfx_obs_set_design takes it
 * (offset, y and aux go with its rows; a component observed at nodes is a block of identity rows, and two components may observe the
 * same nodes). Component c owns rows rowptr[c] .. rowptr[c + 1] (index base 0): rowptr[0] = 0, rowptr[ncomp] = nobs, strictly
 * increasing (no empty component), 1 <= ncomp <= GMRFX_OBS_MAX_COMPONENTS. family[c]: one of the six ids of gmrfx_obs_set; param[c]:
 * that component's sigma / r / phi, ignored for the families without one. aux has one value per row; it is read and validated only on
 * the rows of Poisson, Binomial and NegBinomial components (the other rows may hold anything, NaN included); NULL is refused when a
 * Binomial component exists. Every check and refusal of gmrfx_obs_set_design applies, the value checks per component under that
 * component's family; the messages name the component and the observation;
 * what is refused about A carries the entry point's name and the column). Refused in addition (INVALID_ARG, a message, nothing
 * changed): ncomp out of range, a null family / param / rowptr, a rowptr that does not start at 0, is not strictly increasing or does
 * not end at nobs.
 * loglik_const is the sum of the components' constants over their own rows, taken in component order in long double; gmrfx_obs_info
 * returns the total and family = GMRFX_OBS_COMPOSITE, gmrfx_obs_composite_info the components (ncomp = 0 when none is set; family,
 * param, loglik_const: ncomp values, one per component, rowptr ncomp + 1; each nullable). The plan, the map and the term tables are those of
 * gmrfx_obs_set_design on the same A: gmrfx_obs_hess_map, gmrfx_obs_design_info, gmrfx_obs_design_rows and gmrfx_set_prior with that
 * map work unchanged; one component gives the state of gmrfx_obs_set_design and every result bit for bit. Setting any of the three
 * forms replaces the others; gmrfx_obs_set with nobs = 0 removes the likelihood; gmrfx_clone carries the composite; symbolic_only
 * handles validate it and give the constants and the map.
 * gmrfx_obs_composite_set_param replaces the parameters in place (the positivity checks again; on refusal nothing is changed) and
 * recomputes the constants and the cached pointwise constants; the plan and the device tables are untouched.
 * On a handle holding a composite gmrfx_fisher_eval[_dev], gmrfx_gaussian_approximation[_dev] (with and without a constraint set),
 * gmrfx_obs_pointwise_const, gmrfx_predictor_marginals[_dev] and gmrfx_predictive_scores[_dev] run the composite: every row's g, d and
 * l under its own component (csrc/fisher_design.hip: k_design_eta_comp, one byte per observation and a table of ncomp entries in
 * device memory; csrc/predictive.hip), every sum in the order of the design form. No atomics; bit-reproducible; the host and the _dev
 * forms agree bit for bit. gmrfx_ga_pullback[_dev] is refused (INVALID_ARG): its single parameter cotangent has no composite meaning;
 * gmrfx_ga_pullback_composite[_dev] (below) returns one per component.
 * The batched entry points refuse the handle as they refuse the design form.
 * LIMITS: plain handles; at most 16 components; pointwise exponential-family components only. */
#define GMRFX_OBS_MAX_COMPONENTS 16
#define GMRFX_OBS_COMPOSITE (-2)
int32_t gmrfx_obs_set_composite(gmrfx_handle *h, int32_t ncomp, const int32_t *family /* ncomp */, const double *param /* ncomp */,
                                const int64_t *rowptr /* ncomp + 1, index base 0 */, int64_t nobs, const int64_t *colptr /* n + 1 */,
                                const int64_t *rowval, const double *nzval, int32_t index_base, const double *offset /* nobs, nullable */,
                                const double *y /* nobs */, const double *aux /* nobs, nullable */);
int32_t gmrfx_obs_composite_info(const gmrfx_handle *h, int32_t *ncomp, int32_t *family, double *param, int64_t *rowptr,
                                 double *loglik_const /* ncomp: per component */);
int32_t gmrfx_obs_composite_set_param(gmrfx_handle *h, const double *param /* ncomp */);
/* The loop itself: gaussian_approximation(prior::WorkspaceGMRF, obs_lik) of the reference (src/workspace/gaussian_approximation.jl:191-313)
 * with _ga_line_search, _predict_converged and _frozen_finish of src/arithmetic/condition/gaussian_approximation.jl:231-409 restated
 * line by line in host C++; every vector (x_k, step, score, hess, the line search's candidates) stays in HBM, the host reads a handful
 * of scalars per iterate. Per iterate: gmrfx_fisher_eval at x_k, gmrfx_refactorize_update_solve_dev with its hess and score, with a
 * constraint set the projection step - A~' W^-1 (A step) (the correction of gmrfx_constraints_correct with e = 0), the line search on
 * merit = energy - loglik (accepting up to obj + 64 eps max(|energy| + |loglik|, 1); the full step is probed first under retry_full
 * when alpha < 1; x0.1 per backtrack, alpha <- sqrt(alpha) on acceptance, exit when alpha |step|_inf < newton_dec_tol / 1000; NaN or
 * +Inf merits are rejections), the three-way convergence test (Newton decrement dot(score, step), |x_new - x_k|, the same relative to
 * |x_k|), the look-ahead and three chord steps on the factorisation in hand, of which only the first decides.
 * mu NULL = zero prior mean; x0 NULL = mu. flags: bit 0 adaptive_stepsize, 1 step_recovery == :retry_full, 2 predictive_convergence,
 * 3 leave the handle factorised at Q_prior - H(x_final) (without it the handle holds the last iterate's factor, as the reference's
 * workspace does). x: the mode, n. hess: H(x_final), n, nullable. result (host, 8) = {iterations, converged, final alpha, last Newton
 * decrement, factorisations, solves, merit evaluations, 1 if the frozen finish produced the result}. dec_trace / alpha_trace (host,
 * max_iter + 1 each, nullable): per iterate, the frozen finish's deciding step after the last; unused entries are NaN.
 * Errors: those of gmrfx_fisher_eval; INVALID_ARG for negative max_iter / max_linesearch_iter and unknown flag bits;
 * GMRFX_ERR_NOT_POSDEF when a factorisation fails, with *info as gmrfx_refactorize reports it, x = the last accepted iterate and the
 * handle usable afterwards (also when A Q^-1 A' fails, *info = 0). LIMITS: as gmrfx_fisher_eval. */
int32_t gmrfx_gaussian_approximation(gmrfx_handle *h, const double *mu /* nullable */, const double *x0 /* nullable */, int64_t max_iter,
                                     int64_t max_linesearch_iter, double mean_change_tol, double newton_dec_tol, int32_t flags,
                                     double *x /* n */, double *hess /* n (design form: cnt), nullable */, double *result /* host, 8 */,
                                     double *dec_trace /* host, max_iter + 1, nullable */, double *alpha_trace /* same */, int64_t *info);
int32_t gmrfx_gaussian_approximation_dev(gmrfx_handle *h, const double *d_mu, const double *d_x0, int64_t max_iter,
                                         int64_t max_linesearch_iter, double mean_change_tol, double newton_dec_tol, int32_t flags,
                                         double *d_x, double *d_hess, double *result /* host, 8 */, double *dec_trace /* host */,
                                         double *alpha_trace /* host */, int64_t *info);

/* ---- Fisher scoring and the Gaussian approximation for every member of a batched handle ---------------------------------------------
 * The hyper-parameter sweep of a model with non-Gaussian observations: one Gaussian approximation per theta_k, all in one pass over the
 * forest of gmrfx_create_batched. Node form (eta_i = x_i) or design form (eta = A x + b, gmrfx_batch_obs_set_design), the six families of
 * gmrfx_obs_set, no constraints; a plain handle is a batch of one. gmrfx_obs_set, gmrfx_fisher_eval and gmrfx_gaussian_approximation keep refusing batched handles; the state set here is separate
 * from theirs.
 *   gmrfx_batch_set_prior    keeps the nnz x nbatch values (member-major, as gmrfx_batch_refactorize takes them) on the device and
 *                            installs the Hessian map of the batch likelihood in place at the time of the call, for every member: the
 *                            position of (i, i) in member k's values (no likelihood, or the node form), or the map of
 *                            gmrfx_batch_obs_hess_map shifted by k nnz (design form). The caller builds no forest-wide map. After changing
 *                            the likelihood's FORM call it again: the evaluation refuses a map that is not the one the likelihood in
 *                            place needs. INVALID_ARG for a pattern without a stored diagonal.
 *   gmrfx_batch_obs_set      ONE data set for all members (y, aux, indices as in gmrfx_obs_set; stored once, n values) and one param
 *                            (sigma, r, phi) per member. The same validation and refusals as gmrfx_obs_set, applied to every param[k];
 *                            loglik_const is summed per member in long double. nobs = 0 removes it; gmrfx_clone carries it; works on
 *                            symbolic_only handles.
 *   gmrfx_batch_obs_set_design   the same through a design matrix, eta = A x + b: A (nobs x n, CSC), offset, y and aux as in
 *                            gmrfx_obs_set_design, ONE copy for all members, and one param per member. Every check of gmrfx_obs_set_design
 *                            (the first pair of pattern(A'A) that Q does not store is named in the caller's base; the 2^31 limits) and,
 *                            member by member, every check of gmrfx_batch_obs_set. The plan is built on the member's pattern. nobs = 0
 *                            removes the likelihood; setting either batch form replaces the other. Works on symbolic_only handles.
 *   gmrfx_batch_obs_hess_map     the member's map: cnt positions (index base 0) in ONE member's value array, the list gmrfx_obs_hess_map
 *                            returns on a plain handle of that pattern (map nullable; cap: its capacity, INVALID_ARG when below cnt). A
 *                            member's Hessian vector then has cnt entries in that order, in gmrfx_batch_fisher_eval and the loop.
 *   gmrfx_batch_obs_design_info  nnz(A), cnt and the term count of the plan (-1 each without one), as gmrfx_obs_design_info.
 *   gmrfx_batch_obs_info     family (-1: none), nobs, loglik_const (nbatch values), each nullable.
 *   gmrfx_batch_fisher_eval  per member exactly what gmrfx_fisher_eval returns for Q_p,k, param[k] and x_k, bit for bit: member k's point
 *                            at x + k sx, its mean at mu + k smu (mu nullable; smu = 0: one mean for all), score and hess (either nullable)
 *                            at + k ss, out[2 k ..] = {energy, loglik}. active (host, nbatch bytes, nullable = all): a member whose byte
 *                            is 0 is skipped; its slices of score and hess and its pair of out are left untouched. Design form: per
 *                            member what gmrfx_fisher_eval returns in design form, bit for bit; hess has cnt entries per member, and ss
 *                            must be at least n when score is non-null and at least cnt when hess is.
 *   gmrfx_batch_gaussian_approximation   the loop of gmrfx_gaussian_approximation (same flags, same rules) for all members in lockstep:
 *                            one forest-wide launch per step, every member taking its own line search, look-ahead and frozen finish and
 *                            stopping at its own iterate. x0 nullable (= mu, or 0), member k's at + k sx0; x (sx) the modes; hess (sh,
 *                            nullable) H(x_k). result (host, 10 per member): the plain call's eight numbers, counted as that member's own
 *                            plain loop would count them, then energy and loglik at x_k. totals (host, 3, nullable): the forest-level
 *                            factorisations, solves and evaluations actually launched. dec_trace / alpha_trace (host, (max_iter + 1) per
 *                            member, nullable). info (nbatch, nullable). Returns GMRFX_ERR_NOT_POSDEF when any member's factorisation
 *                            failed: info[k] is then as gmrfx_batch_refactorize reports it, x_k that member's last accepted iterate and
 *                            its hess slice untouched; every other member is complete and correct, and the handle stays usable. A
 *                            stopped member's values no longer change, so without flag bit 3 it ends holding the factor of its own last
 *                            iterate; with it, one more forest factorisation at H(x_k) covers every member that did not fail. Design
 *                            form: hess has cnt entries per member (sh >= cnt); a plan with cnt = 0 runs with Q_post = Q_p.
 *   gmrfx_batch_obs_set_param    replaces the members' parameters (sigma, r, phi) of the likelihood in place, in node or design form: the
 *                            validation of gmrfx_batch_obs_set on every param[k], loglik_const per member in long double from the data
 *                            the handle keeps. No data goes up and no plan is rebuilt; a following evaluation has the bits it has after
 *                            a full gmrfx_batch_obs_set with the same parameters. Works with a batch constraint held and on symbolic_only
 *                            handles. INVALID_ARG without a likelihood or with a null param.
 *   gmrfx_batch_constrained_gaussian_approximation   the same loop under the batch constraint A x = e of gmrfx_batch_constraints_set
 *                            (Besag, RW1, RW2, BYM2 under sum-to-zero): every step is projected, s_k <- s_k - At_k W_k^-1 (A s_k), where
 *                            the plain loop projects it under gmrfx_constraints_set -- once per iterate and once per chord step of the
 *                            frozen finish -- with At_k, W_k refreshed per iterate for all members in one forest solve. The arguments of
 *                            gmrfx_batch_gaussian_approximation, then cinfo (nbatch, nullable): 0, 1 + the failing pivot of W_k, or -1
 *                            beside a failed factorisation; residual (host, nbatch, nullable): max_r |(A x_k - e)_r| of the members that
 *                            did not fail, NaN for the others. The iterates keep A x_k = A x0_k, so x0 (or mu) must satisfy the
 *                            constraint for the modes to. A member whose W_k fails stops alone like one whose factorisation fails: x_k its
 *                            last accepted iterate, everybody else complete; GMRFX_ERR_NOT_POSDEF when any member failed either way.
 *                            INVALID_ARG when no batch constraint is held (call gmrfx_batch_gaussian_approximation) or a plain one is,
 *                            then every refusal of the unconstrained call. gmrfx_batch_set_prior accepts a handle holding a batch
 *                            constraint; gmrfx_batch_obs_set[_design], gmrfx_batch_fisher_eval and gmrfx_batch_gaussian_approximation[_dev]
 *                            keep refusing one: the unconstrained loop would silently ignore the constraint.
 * No atomics; bit-reproducible; the host and the _dev forms agree bit for bit; a member's results do not depend on the other members.
 * Device memory: the data set (17 n bytes), the member's row structure, 6 n nbatch doubles of work vectors on the first loop. Design
 * form: the plan's tables and the data set once, (2 nobs + ncc + nct + design blocks) nbatch doubles of evaluation work (ncc + nct: the
 * chunks of the columns and term lists longer than 512 entries), (5 n + cnt) nbatch doubles of work vectors on the first loop.
 * Errors (INVALID_ARG with a message, nothing changed): a sharded handle, more than 65535 members, a constraint set (gmrfx_constraints_set
 * everywhere; gmrfx_batch_constraints_set for gmrfx_batch_obs_set[_design], gmrfx_batch_fisher_eval and the unconstrained loop; none held
 * for the constrained loop), a plain handle holding the design form of gmrfx_obs_set_design, null x / out / result, a stride below n
 * (smu = 0 excepted; hess: below cnt in design form), no likelihood, no prior, a prior whose map is not the likelihood's.
 * GMRFX_ERR_NO_DEVICE for symbolic_only handles after these checks.
 * LIMITS: constraints through gmrfx_batch_constrained_gaussian_approximation only (one A and e for all members, m <= 64 rows); no batched
 * pullback or predictive scores (left to follow-ups); nbatch <= 65535; n < 2^31. */
int32_t gmrfx_batch_set_prior(gmrfx_handle *h, const double *prior_nzval /* nnz x nbatch */);
int32_t gmrfx_batch_obs_set(gmrfx_handle *h, int32_t family, int64_t nobs, const int64_t *indices /* nobs, nullable */, int32_t index_base,
                            const double *y /* nobs */, const double *aux /* nobs, nullable */, const double *param /* nbatch */);
int32_t gmrfx_batch_obs_set_design(gmrfx_handle *h, int32_t family, int64_t nobs, const int64_t *colptr /* n + 1 */, const int64_t *rowval,
                                   const double *nzval, int32_t index_base, const double *offset /* nobs, nullable */,
                                   const double *y /* nobs */, const double *aux /* nobs, nullable */, const double *param /* nbatch */);
int32_t gmrfx_batch_obs_set_param(gmrfx_handle *h, const double *param /* nbatch */);
int32_t gmrfx_batch_obs_hess_map(const gmrfx_handle *h, int64_t *map /* nullable; cnt values, index base 0 */, int64_t cap, int64_t *cnt);
int32_t gmrfx_batch_obs_design_info(const gmrfx_handle *h, int64_t *nnz_a, int64_t *cnt, int64_t *terms);
int32_t gmrfx_batch_obs_info(const gmrfx_handle *h, int32_t *family, int64_t *nobs, double *loglik_const /* nbatch */);
int32_t gmrfx_batch_fisher_eval(gmrfx_handle *h, const double *x, int64_t sx, const double *mu /* nullable */, int64_t smu,
                                const uint8_t *active /* host, nbatch, nullable */, double *score /* nullable */, double *hess /* nullable */,
                                int64_t ss, double *out /* host, 2 x nbatch */);
int32_t gmrfx_batch_fisher_eval_dev(gmrfx_handle *h, const double *d_x, int64_t sx, const double *d_mu, int64_t smu,
                                    const uint8_t *active /* host */, double *d_score, double *d_hess, int64_t ss, double *out /* host */);
int32_t gmrfx_batch_gaussian_approximation(gmrfx_handle *h, const double *mu /* nullable */, int64_t smu, const double *x0 /* nullable */,
                                           int64_t sx0, int64_t max_iter, int64_t max_linesearch_iter, double mean_change_tol,
                                           double newton_dec_tol, int32_t flags, double *x, int64_t sx, double *hess /* nullable */,
                                           int64_t sh, double *result /* host, 10 x nbatch */, double *totals /* host, 3, nullable */,
                                           double *dec_trace /* host, (max_iter + 1) x nbatch, nullable */, double *alpha_trace /* same */,
                                           int64_t *info /* nbatch, nullable */);
int32_t gmrfx_batch_gaussian_approximation_dev(gmrfx_handle *h, const double *d_mu, int64_t smu, const double *d_x0, int64_t sx0,
                                               int64_t max_iter, int64_t max_linesearch_iter, double mean_change_tol, double newton_dec_tol,
                                               int32_t flags, double *d_x, int64_t sx, double *d_hess, int64_t sh, double *result /* host */,
                                               double *totals /* host */, double *dec_trace /* host */, double *alpha_trace /* host */,
                                               int64_t *info);
int32_t gmrfx_batch_constrained_gaussian_approximation(gmrfx_handle *h, const double *mu /* nullable */, int64_t smu, const double *x0 /* nullable */,
                                                       int64_t sx0, int64_t max_iter, int64_t max_linesearch_iter, double mean_change_tol,
                                                       double newton_dec_tol, int32_t flags, double *x, int64_t sx, double *hess /* nullable */,
                                                       int64_t sh, double *result /* host, 10 x nbatch */, double *totals /* host, 3, nullable */,
                                                       double *dec_trace /* host, (max_iter + 1) x nbatch, nullable */, double *alpha_trace /* same */,
                                                       int64_t *info /* nbatch, nullable */, int64_t *cinfo /* nbatch, nullable */,
                                                       double *residual /* host, nbatch, nullable */);
int32_t gmrfx_batch_constrained_gaussian_approximation_dev(gmrfx_handle *h, const double *d_mu, int64_t smu, const double *d_x0, int64_t sx0,
                                                           int64_t max_iter, int64_t max_linesearch_iter, double mean_change_tol,
                                                           double newton_dec_tol, int32_t flags, double *d_x, int64_t sx, double *d_hess, int64_t sh,
                                                           double *result /* host */, double *totals /* host */, double *dec_trace /* host */,
                                                           double *alpha_trace /* host */, int64_t *info, int64_t *cinfo, double *residual /* host */);

/* ---- The pullback of the Gaussian approximation (implicit-function rule) -------------------------------------------------------------
 * Reverse-mode rule of gaussian_approximation(prior, obs_lik) at its mode x (src/workspace/autodiff.jl:140-202; for plain GMRFs
 * src/autodiff/gaussian_approximation.jl:278-347), the step between gmrfx_logpdf_grad and gmrfx_pattern_dot when hyper-parameters are
 * fitted on the Laplace marginal likelihood. Inputs: the cotangent of the posterior mean, mubar (n), and of the posterior precision
 * Q_post = Q_prior - H(x), Qbar: a symmetric matrix on the stored entries of the pattern, nnz values in the pattern's order, an entry
 * carrying its value whichever triangle it lies in (the convention of gmrfx_logpdf_grad: dL = sum_ij Qbar_ij dQ_ij over all (i, j)).
 * Either may be NULL (zero), not both. With r = x - mu, a_i row i of A (node form: a unit vector), g, d as above, d3 = dd/deta and
 * gp, dp the derivatives of g and d by the family's parameter (sigma, r, phi; 0 for Poisson, Bernoulli, Binomial):
 *   c_i  = a_i' Qbar a_i          node form: the diagonal entry Qbar[map[i]]; design form: the sum over the pairs (j <= k) of row i of
 *                                 (j == k ? 1 : 2) A_ij A_ik Qbar[position of (j, k)], the positions of gmrfx_obs_hess_map
 *   xbar = mubar - A' (c . d3(eta))
 *   lam  = Q_post^-1 xbar         the handle's factor; flags bit 0 and a constraint set: lam <- lam - A~' W^-1 (A lam), the correction
 *                                 the loop applies to its steps (e = 0); without the bit the plain solve of the workspace rule
 *   Qbar_prior[e = (i, j)] = Qbar[e] - 0.5 (lam_i r_j + lam_j r_i)        nnz, in that association, no contraction; Qbar NULL: 0 - ...
 *   mubar_prior = Q_p lam                                                 n; Symmetric(Q_p), the values gmrfx_set_prior keeps
 *   out[0] = sum_i (A lam)_i gp_i - sum_i c_i dp_i                        the cotangent of sigma / r / phi
 *   out[1] = lam' xbar                                                    a check value
 *   family   d3                       gp                           dp                                     (m the mean, q = 1 - m)
 *   Normal   0                        -2 (y - eta) / sigma^3       2 / sigma^3
 *   Poisson  -m                       0                            0
 *   Bern/Bin -n m q (q - m)           0                            0
 *   NegBin   -(r + y) s q (q - s)     s ((r + y) q / r - 1)        -s q + (r + y) s q (q - s) / r        s = mu / (r + mu), q = 1 - s
 *   Gamma    phi w                    w - 1                        -w                                     w = y exp(-eta)
 * in the stable forms of csrc/fisher_point.h. Qbar_prior, mubar_prior and lambda (= lam, n) are each nullable, not all three;
 * Qbar_prior may be Qbar itself. flags bit 1: refactorise at Q_prior - H(x) first (gmrfx_fisher_eval, then gmrfx_refactorize_update);
 * without it the handle must hold that factor already -- gmrfx_gaussian_approximation with its flag bit 3 leaves it.
 * No atomics: every sum is formed in an order that depends on indices only; results are bit-reproducible, independent of the
 * alignment of the operands (8 bytes suffice), the host and the _dev forms agree bit for bit, and a selection matrix A without offset
 * gives the arrays of the node form bit for bit. Work memory on the device: 2 n + nobs doubles, and in design form the plan's
 * transposed term table, 12 B per term, uploaded on the first call; gmrfx_clone carries nothing new.
 * gmrfx_obs_design_rows reads that table: ptr (nobs + 1), and per term the position in nzval and the weight (doubled off the diagonal),
 * positions ascending within a row; each nullable.
 * Errors: those of gmrfx_fisher_eval (x or out null, no likelihood, no prior, a map that is not the likelihood's, a batched or sharded
 * handle; GMRFX_ERR_NO_DEVICE for symbolic_only handles after the argument checks that need no device state); INVALID_ARG for unknown
 * flag bits, mubar and Qbar both null, every output null, bit 0 without a constraint; GMRFX_ERR_NOT_FACTORIZED without bit 1 before
 * the first factorisation; GMRFX_ERR_NOT_POSDEF when the factorisation of bit 1 or the constraint's W fails (outputs untouched).
 * LIMITS: as gmrfx_fisher_eval. The tangents of y, aux, the offset and the values of A are not computed. A row's term list is summed
 * by one lane group whatever its length (a row of k entries has k (k + 1) / 2 terms). */
int32_t gmrfx_ga_pullback(gmrfx_handle *h, const double *x, const double *mu /* nullable */, const double *mubar /* n, nullable */,
                          const double *Qbar /* nnz, nullable */, int32_t flags, double *Qbar_prior /* nnz, nullable */,
                          double *mubar_prior /* n, nullable */, double *lambda /* n, nullable */, double *out /* host, 2 */);
int32_t gmrfx_ga_pullback_dev(gmrfx_handle *h, const double *d_x, const double *d_mu, const double *d_mubar, const double *d_Qbar, int32_t flags,
                              double *d_Qbar_prior, double *d_mubar_prior, double *d_lambda, double *out /* host, 2 */);
int32_t gmrfx_obs_design_rows(const gmrfx_handle *h, int64_t *ptr /* nobs + 1 */, int64_t *pos /* terms */, double *w /* terms */);

/* ---- The same pullback for every member of a batched handle ------------------------------------------------------------------------------
 * The middle link of the batched gradient chain gmrfx_batch_logpdf_grad_dev -> gmrfx_batch_ga_pullback_dev -> gmrfx_batch_pattern_dot_dev:
 * the formulas of gmrfx_ga_pullback, member by member, with Q_p,k the values of gmrfx_batch_set_prior, the ONE likelihood of
 * gmrfx_batch_obs_set / gmrfx_batch_obs_set_design (node or design form) and param[k]. ONE forest solve and one launch per step for
 * all members.
 * STRIDES. Member k's mode at x + k sx (sx >= n) and prior mean at mu + k smu (smu >= n, or 0: one mean for all), as in
 * gmrfx_batch_fisher_eval. The cotangents and the outputs are dense per member, as gmrfx_batch_logpdf_grad has them: mubar, mubar_prior
 * and lambda at + k n, Qbar and Qbar_prior at + k nnz (nnz of the member's pattern); the Qbar of gmrfx_batch_logpdf_grad_dev is passed
 * straight in and Qbar_prior straight on to gmrfx_batch_pattern_dot_dev. Qbar_prior may be Qbar itself. out[2 k], out[2 k + 1]: member
 * k's parameter cotangent and lam_k' xbar_k.
 * FLAGS. Bit 0: lam_k <- lam_k - A~_k' W_k^-1 (A lam_k) with the batch constraint (gmrfx_batch_constraints_set). A handle that holds a
 * batch constraint is not refused without the bit: bit clear is the plain solve, as on a plain handle. Bit 1: one batched evaluation of
 * every member's Hessian at its x, then the forest's gmrfx_refactorize_update; without it the handle must hold the factor of every
 * Q_p,k - H(x_k) already -- gmrfx_batch_gaussian_approximation with its flag bit 3 leaves it.
 * INFO (host, nbatch, nullable), the convention of gmrfx_batch_logpdf_grad: 0; -1 when member k's factorisation failed (under bit 1, or
 * held); 1 + the failing pivot when its W_k did (bit 0). Such a member is masked out of every launch: its requested output slices and
 * its two entries of out are NaN, nothing else of it is touched, and every other member is computed as if it were not there. With info
 * NULL such a member makes the call return GMRFX_ERR_NOT_POSDEF; the healthy members' outputs are written all the same.
 * BITS. No atomics; member k's sums are formed in the plain call's orders whatever the other members hold. Without bit 0, member k's
 * outputs and its two results have the bits of gmrfx_ga_pullback on a plain handle of Q_p,k, param[k], x_k, mu_k and its cotangents,
 * whichever members share the batch; host and _dev forms agree bit for bit, whatever the alignment of the operands (8 bytes suffice).
 * Under bit 0 the preparation of W_k is the batch constraint's own (see gmrfx_batch_constraints_set): close to, not bitwise, the plain one.
 * Work memory on the device, allocated on the first call, on the handle's books and dropped with the likelihood by
 * gmrfx_batch_obs_set*: nbatch (2 n + nobs) doubles, the partial sums and nbatch results, and in design form ONE transposed term table
 * (12 B per term); under bit 1 the loop's work area (5 n + hess_len doubles per member) if the loop has not allocated it yet.
 * Errors: INVALID_ARG for x or out null, sx < n, smu neither 0 nor >= n, unknown flag bits, mubar and Qbar both null, every output
 * null, bit 0 without a batch constraint, no batch likelihood (a plain handle that has none among them), no prior or a map that is not
 * the likelihood's, a sharded handle, a plain constraint set or a plain design likelihood held -- all before GMRFX_ERR_NO_DEVICE on
 * symbolic_only handles where they need no device state; GMRFX_ERR_NOT_FACTORIZED without bit 1 before the first factorisation;
 * GMRFX_ERR_NOT_POSDEF as above. gmrfx_ga_pullback keeps refusing batched handles.
 * LIMITS: nbatch <= 65535 (the member is the second dimension of the launch grid); otherwise those of gmrfx_ga_pullback. */
int32_t gmrfx_batch_ga_pullback(gmrfx_handle *h, const double *x, int64_t sx, const double *mu /* nullable */, int64_t smu /* 0: one mean for all */,
                                const double *mubar /* n x nbatch, nullable */, const double *Qbar /* nnz x nbatch, nullable */, int32_t flags,
                                double *Qbar_prior /* nnz x nbatch, nullable */, double *mubar_prior /* n x nbatch, nullable */,
                                double *lambda /* n x nbatch, nullable */, double *out /* host, 2 x nbatch */, int64_t *info /* host, nbatch, nullable */);
int32_t gmrfx_batch_ga_pullback_dev(gmrfx_handle *h, const double *d_x, int64_t sx, const double *d_mu, int64_t smu, const double *d_mubar,
                                    const double *d_Qbar, int32_t flags, double *d_Qbar_prior, double *d_mubar_prior, double *d_lambda,
                                    double *out /* host, 2 x nbatch */, int64_t *info /* host, nbatch, nullable */);

/* ---- The same pullback for a composite likelihood ---------------------------------------------------------------------------------------
 * The last link of logpdf_grad_dev -> ga_pullback -> pattern_dot for the joint models of gmrfx_obs_set_composite: the formulas of
 * gmrfx_ga_pullback with d3, gp and dp of every row taken under the family and parameter of the row's component, and the parameter
 * cotangent split by component,
 *   param_bar[c] = sum_{i in rows of c} (A lam)_i gp_i - sum_{i in rows of c} c_i dp_i          ncomp values, on the host
 *   *check       = lam' xbar                                                                    nullable
 * param_bar[c] is exactly 0.0 for a Poisson, Bernoulli or Binomial component. x, mu, mubar, Qbar, flags, Qbar_prior, mubar_prior and
 * lambda are those of gmrfx_ga_pullback; bit 1 factorises Q_prior - H(x) through the composite evaluation. No atomics: a workgroup's
 * partial sum never mixes components (the observations are tiled per component, csrc/kernels.h: GapTiles), a component's partials
 * are added in the order gmrfx_ga_pullback adds all of them; results are bit-reproducible, the host and the _dev forms agree bit for
 * bit, and ONE component gives every array, param_bar[0] and *check of gmrfx_ga_pullback after gmrfx_obs_set_design on the same A
 * bit for bit. Work memory: that of gmrfx_ga_pullback, at most nobs / 16 + ncomp partial sums twice, ncomp results and 12 (ncomp + 1)
 * bytes of tiling offsets, uploaded on the first call and dropped when the likelihood is replaced; gmrfx_obs_composite_set_param
 * leaves it.
 * Errors, in this order: INVALID_ARG for a sharded or batched handle or a handle without a composite (gmrfx_ga_pullback serves the
 * single-family likelihoods); INVALID_ARG for x or param_bar null, unknown flag bits, mubar and Qbar both null, every array output
 * null, bit 0 without a constraint; then GMRFX_ERR_NO_DEVICE, GMRFX_ERR_NOT_FACTORIZED and GMRFX_ERR_NOT_POSDEF as
 * gmrfx_ga_pullback. A refused call leaves the handle as it was.
 * LIMITS: plain handles (no batched composite); otherwise those of gmrfx_ga_pullback. */
int32_t gmrfx_ga_pullback_composite(gmrfx_handle *h, const double *x, const double *mu /* nullable */, const double *mubar /* n, nullable */,
                                    const double *Qbar /* nnz, nullable */, int32_t flags, double *Qbar_prior /* nnz, nullable */,
                                    double *mubar_prior /* n, nullable */, double *lambda /* n, nullable */,
                                    double *param_bar /* host, ncomp */, double *check /* host, 1, nullable */);
int32_t gmrfx_ga_pullback_composite_dev(gmrfx_handle *h, const double *d_x, const double *d_mu, const double *d_mubar, const double *d_Qbar,
                                        int32_t flags, double *d_Qbar_prior, double *d_mubar_prior, double *d_lambda,
                                        double *param_bar /* host, ncomp */, double *check /* host, 1, nullable */);

/* ---- Linear-predictor marginals and predictive scores ----------------------------------------------------------------------------------
 * What follows a fit: linear_predictor_marginals(ga, obs_lik) of the reference (src/linear_predictor_marginals.jl:58-195, with the
 * constraint correction and clamp of _subtract_constraint_correction!, :189-195) and pointwise_loglik (src/observation_models/
 * exponential_family/pointwise_implementations.jl), the inputs of posterior predictive checks and WAIC / CPO accumulators. Plain
 * handles with a likelihood set (gmrfx_obs_set or gmrfx_obs_set_design; the six families), observations in the caller's order: the
 * order of `indices` in node form, the rows of A in design form. With Sigma the selected inverse of the factorisation the handle holds
 * (gmrfx_gaussian_approximation with its flag bit 3 leaves that of Q_post), a_i row i of A (node form: a unit vector):
 *   mu_eta_i = (A x)_i + b_i            node form: x[idx_i]. Design form: the eta gmrfx_fisher_eval forms, bit for bit
 *   v_eta_i  = a_i' Sigma a_i           node form: Sigma[idx_i, idx_i]; design form: the sum over the pairs (j <= k) of row i of
 *                                       (j == k ? 1 : 2) A_ij A_ik Sigma[position of (j, k)] (the table of gmrfx_obs_design_rows); an
 *                                       empty row gives +0.0
 *   flags bit 0, with a constraint set:  v_eta_i <- max(v_eta_i - sum_{l < m} ((a_i B)_l)^2, 0), B = Q^-1 A_c' L_c^-T read where the
 *                                       constraint keeps it (n x m, column-major; no transposed copy is built); a NaN stays a NaN.
 *                                       Without the bit there is no clamp
 *   pll_i    = l_i(mu_eta_i) + c_i      the full log density of observation i at the mean; c_i: gmrfx_obs_pointwise_const
 * x: n values (the mode, already projected under a constraint); mu_eta, v_eta, pll: nobs each, each nullable, not all three. v_eta
 * needs a factorisation and computes the selected inverse if this factorisation has none yet; mu_eta and pll need neither.
 * gmrfx_obs_pointwise_const: c_i, the terms of the log density that do not depend on x, each computed in long double and rounded
 * (Normal -1/2 log 2 pi - log sigma; Poisson -lgamma(y + 1); Bernoulli 0; Binomial the log binomial coefficient; NegBin lgamma(y + r) -
 * lgamma(r) - lgamma(y + 1) + r log r; Gamma phi log phi - lgamma(phi) + (phi - 1) log y). Works on symbolic_only handles; their sum is
 * the loglik_const of gmrfx_obs_info.
 *
 * gmrfx_predictive_scores: with s_i = sqrt(v_eta_i) and l_k = l_i(mu_eta_i + s_i z_k) + c_i over the caller's K nodes z and weights w
 * of the standard normal (host arrays in both forms; 1 <= K <= 64, all finite, weights positive; the library holds no rule and does
 * not normalise):
 *   elp_i  = sum_k w_k l_k                                      vlp_i = sum_k w_k (l_k - elp_i)^2
 *   lpd_i  = M + log sum_k w_k exp(l_k - M),  M = max_k l_k     (-inf when every l_k is)
 *   lcpo_i = -(M' + log sum_k w_k exp(-l_k - M')),  M' = max_k -l_k      (-inf when some l_k is -inf)
 * A NaN or negative v_eta_i gives NaN in all four; where elp_i is -inf, vlp_i is NaN. mu_eta, v_eta: nobs values each (normally the
 * outputs above, left on the device); lpd, lcpo, elp, vlp: nobs each, each nullable; out[4] (host): the totals sum_i lpd_i, lcpo_i,
 * elp_i, vlp_i, computed whether or not the arrays are asked for (p_waic = out[3], WAIC = -2 (out[0] - out[3]): the caller's).
 * No atomics: every sum is formed in an order that depends on indices only; results are bit-reproducible, independent of the
 * alignment of the operands (8 bytes suffice), the host and the _dev forms agree bit for bit, and a selection matrix A without offset
 * gives mu_eta, v_eta and pll of the node form bit for bit. Device memory added on the first call after gmrfx_obs_set[_design]: 8 nobs
 * bytes (c), 4 nobs (the observation order, node form) or 8 cnt (the plan's map, design form), and in design form, for v_eta, the
 * plan's transposed term table (12 B per term, shared with gmrfx_ga_pullback; none of its work vectors); gmrfx_clone carries nothing new.
 * Errors: INVALID_ARG (with a message, nothing written) for x null, every output null, unknown flag bits, bit 0 without a constraint,
 * no likelihood, a batched or sharded handle; for the scores mu_eta / v_eta / out null and a refused quadrature rule. Then
 * GMRFX_ERR_NO_DEVICE for symbolic_only handles, GMRFX_ERR_NOT_FACTORIZED when v_eta is asked for before the first factorisation,
 * GMRFX_ERR_NOT_POSDEF when the constraint's W fails (outputs untouched).
 * LIMITS: plain handles; n, nobs < 2^31; K <= 64. A row's term list is summed by one lane group whatever its length (a row of k entries
 * has k (k + 1) / 2 terms), and with bit 0 a row costs m lane-group sums. */
int32_t gmrfx_obs_pointwise_const(const gmrfx_handle *h, double *out /* nobs */);
int32_t gmrfx_predictor_marginals(gmrfx_handle *h, const double *x /* n */, int32_t flags, double *mu_eta /* nobs, nullable */,
                                  double *v_eta /* nobs, nullable */, double *pll /* nobs, nullable */);
int32_t gmrfx_predictor_marginals_dev(gmrfx_handle *h, const double *d_x, int32_t flags, double *d_mu_eta, double *d_v_eta, double *d_pll);
int32_t gmrfx_predictive_scores(gmrfx_handle *h, const double *mu_eta /* nobs */, const double *v_eta /* nobs */, int64_t K,
                                const double *z /* host, K */, const double *w /* host, K */, double *lpd /* nobs, nullable */,
                                double *lcpo /* nobs, nullable */, double *elp /* nobs, nullable */, double *vlp /* nobs, nullable */,
                                double *out /* host, 4 */);
int32_t gmrfx_predictive_scores_dev(gmrfx_handle *h, const double *d_mu_eta, const double *d_v_eta, int64_t K, const double *z /* host, K */,
                                    const double *w /* host, K */, double *d_lpd, double *d_lcpo, double *d_elp, double *d_vlp,
                                    double *out /* host, 4 */);

/* ---- The same read-outs for every member of a batched handle, and the mixture over the sweep ----------------------------------------------
 * After gmrfx_batch_gaussian_approximation (flag bit 3: the forest holds the factor of every Q_post,k) the formulas above, member by
 * member, with the ONE likelihood of gmrfx_batch_obs_set / gmrfx_batch_obs_set_design and param[k]: one launch per step for all
 * members, the member in the launch grid. A plain handle that holds a batch likelihood is a batch of one.
 * LAYOUT. Member k's mean at x + k sx (sx >= n). Every per-observation array is nobs x nbatch, column k member k's (stride nobs):
 * mu_eta, v_eta, pll, the inputs and the four outputs of the scores, the inputs of the mixture. out of the scores: 4 per member.
 * gmrfx_batch_obs_pointwise_const: c_ik = the term of gmrfx_obs_pointwise_const at param[k], nobs x nbatch (the families without a
 * parameter repeat one column; the device keeps one column for them and nobs x nbatch for Normal, NegBin and Gamma). The device's
 * table is dropped by gmrfx_batch_obs_set_param and gmrfx_batch_obs_set*: the next call rebuilds it.
 * FLAGS (marginals). Bit 0: member k's v_eta gets the BATCH constraint's correction with its own B_k (read where
 * gmrfx_batch_constraints_set keeps it, no transposed copy) and the clamp. A held constraint without the bit is ignored.
 * INFO (host, nbatch, nullable), the convention of gmrfx_batch_ga_pullback: 0; -1 when member k's factorisation failed; 1 + the
 * failing pivot when its W_k did (bit 0). Such a member is masked out of every launch: NaN in its requested slices (and its four
 * totals), nothing else of it is touched, everybody else is complete; the call returns GMRFX_OK. The marginals look at the factor only
 * when v_eta is asked for: without it every member gets its mu_eta and pll. The scores read no factor; where the handle holds one, a
 * member whose factor failed is reported and masked all the same.
 * BITS. No atomics. Without bit 0 member k's results (and its four totals) have the bits of the plain calls on a plain handle
 * factorised at Q_post,k with param[k], whichever members share the batch, in host or _dev form, whatever the alignment (8 bytes
 * suffice) -- given that the member's selected inverse has the plain handle's bits. Under bit 0 the preparation of W_k is the batch
 * constraint's own: close to, not bitwise, the plain one.
 *
 * gmrfx_batch_predictive_mixture: the predictive distribution integrated over the members with weights omega_k proportional to
 * exp(logw_k) (logw: host, nbatch, unnormalised; -inf excludes a member). The library forms omega_k = exp(logw_k - max) / sum in long
 * double and rounds omega_k and log omega_k to double. Per observation, the members in ascending k:
 *   mix_mu_i  = sum_k omega_k mu_ik            mix_v_i = sum_k omega_k (v_ik + (mu_ik - mix_mu_i)^2)
 *   mix_lpd_i = M_i + log sum_k exp(log omega_k + lpd_ik - M_i),  M_i = max_k (log omega_k + lpd_ik)      (-inf when M_i is)
 * lpd nullable (then mix_lpd is not computed and out[0] is NaN); mix_mu, mix_v, mix_lpd: nobs each, each nullable. out[0] (host,
 * nullable): sum_i mix_lpd_i, through per-workgroup partials and one final workgroup in a fixed order. An excluded member is never
 * read (its NaN does no harm); an included member's NaN propagates. One member with logw = [0] returns its inputs bit for bit, with
 * one exception of sign: a v_eta or lpd entry of -0.0 comes back as +0.0 (0 + -0.0 in the sums); mu_eta keeps its sign of zero. No
 * atomics; bit-reproducible; shifting every logw by a constant that is exact in double changes nothing.
 * Device memory, on the first call after gmrfx_batch_obs_set*, on the handle's books: the tables of the plain calls once (c as above),
 * 32 bytes of partial sums per 16 observations and member, 4 n bytes (node form, for v_eta), 16 nbatch bytes of weights.
 * Errors: INVALID_ARG (with a message, nothing written) for x null, sx < n, every output null, unknown flag bits, bit 0 without a batch
 * constraint, no batch likelihood, a sharded handle, more than 65535 members, a plain constraint or a plain design likelihood held;
 * for the scores mu_eta / v_eta / out null and a refused quadrature rule; for the mixture logw / mu_eta / v_eta null, every output
 * null, mix_lpd without lpd, a NaN or +inf weight, every member excluded. Then GMRFX_ERR_NO_DEVICE, then GMRFX_ERR_NOT_FACTORIZED when
 * v_eta is asked for before the first factorisation. gmrfx_predictor_marginals and gmrfx_predictive_scores keep refusing batched handles.
 * LIMITS: nbatch <= 65535; n, nobs < 2^31; K <= 64; unsharded handles. */
int32_t gmrfx_batch_obs_pointwise_const(const gmrfx_handle *h, double *out /* nobs x nbatch */);
int32_t gmrfx_batch_predictor_marginals(gmrfx_handle *h, const double *x, int64_t sx, int32_t flags, double *mu_eta /* nobs x nbatch, nullable */,
                                        double *v_eta /* nobs x nbatch, nullable */, double *pll /* nobs x nbatch, nullable */,
                                        int64_t *info /* host, nbatch, nullable */);
int32_t gmrfx_batch_predictor_marginals_dev(gmrfx_handle *h, const double *d_x, int64_t sx, int32_t flags, double *d_mu_eta, double *d_v_eta,
                                            double *d_pll, int64_t *info /* host, nbatch, nullable */);
int32_t gmrfx_batch_predictive_scores(gmrfx_handle *h, const double *mu_eta /* nobs x nbatch */, const double *v_eta /* nobs x nbatch */, int64_t K,
                                      const double *z /* host, K */, const double *w /* host, K */, double *lpd /* nobs x nbatch, nullable */,
                                      double *lcpo /* nobs x nbatch, nullable */, double *elp /* nobs x nbatch, nullable */,
                                      double *vlp /* nobs x nbatch, nullable */, double *out /* host, 4 x nbatch */,
                                      int64_t *info /* host, nbatch, nullable */);
int32_t gmrfx_batch_predictive_scores_dev(gmrfx_handle *h, const double *d_mu_eta, const double *d_v_eta, int64_t K, const double *z /* host, K */,
                                          const double *w /* host, K */, double *d_lpd, double *d_lcpo, double *d_elp, double *d_vlp,
                                          double *out /* host, 4 x nbatch */, int64_t *info /* host, nbatch, nullable */);
int32_t gmrfx_batch_predictive_mixture(gmrfx_handle *h, const double *logw /* host, nbatch */, const double *mu_eta /* nobs x nbatch */,
                                       const double *v_eta /* nobs x nbatch */, const double *lpd /* nobs x nbatch, nullable */,
                                       double *mix_mu /* nobs, nullable */, double *mix_v /* nobs, nullable */, double *mix_lpd /* nobs, nullable */,
                                       double *out /* host, 1, nullable */);
int32_t gmrfx_batch_predictive_mixture_dev(gmrfx_handle *h, const double *logw /* host, nbatch */, const double *d_mu_eta, const double *d_v_eta,
                                           const double *d_lpd, double *d_mix_mu, double *d_mix_v, double *d_mix_lpd,
                                           double *out /* host, 1, nullable */);

#ifdef __cplusplus
}
#endif
#endif /* GMRFX_H */
