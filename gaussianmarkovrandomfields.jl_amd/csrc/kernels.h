// kernels.h -- records and launch wrappers of the HIP kernels. Which variant a wrapper launches, its geometry and the thresholds in
// between: the choose_* functions and constants of device_plan.h. The device-side helpers the kernels share: kernel_common.h.
#pragma once
#include <hip/hip_runtime.h>

#include "device.h"

namespace gmrfx {

// (FrontArg / FrontView -- the geometry of one front for the panel kernels -- live in device.h / device_plan.h. The panel chain at the top
// of the tree, potrf -> trsm -> gemm, ~120 dependent launches on a single front, gets it in the kernel arguments; everything
// else reads one record at its position in the level list.)

void launch_gather_values(hipStream_t st, const double *nzval, const int *qsrc, double *out, long long cnt);
void launch_assemble(hipStream_t st, const DevSym &S, const int *list, const AsmRec *arec, const double *nzp, int nfronts, int max_cols, int max_rows,
                     const double *nzval, double *L, double *CB);
// info[0] = INT_MAX (no pivot failed), stamps[2 k] = all ones, stamps[2 k + 1] = 0 for the nslots SYRK slots: one launch of one workgroup
void launch_factor_reset(hipStream_t st, int *info, unsigned long long *stamps, int nslots);
// The time of the SYRK launches (Device::syrk_ms) from the device's wall clock. stamp (k_syrk_cb, k_syrk_big): the launch's slot of
// two words -- earliest start, latest end over its workgroups (kernel_common.h, stamp_begin / stamp_end; one atomic each per
// workgroup); launches that share a slot span it together. times (k_syrk_cb_rec): two words per tile of the level, start and
// end, plain stores; launch_syrk_reduce takes them into the slots behind the last level.
void launch_syrk_cb(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_trail, const double *L, double *CB, unsigned long long *stamp);
// The same tiles from self-contained records, one contiguous run per XCD (workgroup id mod 8 = XCD): see k_syrk_cb_rec.
void launch_syrk_cb_recs(hipStream_t st, const DevSym &S, const SyrkTile *recs, const SyrkSplit &split, int per_xcd, const double *L, double *CB,
                         unsigned long long *times, int noprod = 0, bool piped = false);
// lev[0 .. nlev): per level the first tile (index into `times` / 2), the number of tiles and the slot (-1: none)
struct SyrkLevelTimes { long long off; int cnt, slot; };
void launch_syrk_reduce(hipStream_t st, const SyrkLevelTimes *lev, int nlev, const unsigned long long *times, unsigned long long *stamps);
// piped: the product loop in three stages of two k-steps, each requested two stages ahead (levels whose widest front has at least
// kSyrkPipedMinCols columns, device_plan.h; measured on cfg 2, round 6: k_syrk_cb_rec 3.60-3.69 -> 3.37-3.45 ms per step with 32 / 64 / 128 /
// 200 / 300 alike, 600: 3.56)
// CB -= L21 L21' on 128 x 128 LDS-staged tiles (behind a gather-only pass: noprod = 1), for levels of huge fronts
void launch_syrk_big(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_trail, const double *L, double *CB, unsigned long long *stamp);
// blocks at most 32 columns wide, factorisation only (k_trsm<0, 0>'s arithmetic on half the registers)
void launch_trsm_narrow(hipStream_t st, const FrontView *frec, int nactive, int kb, int max_rows_below, double *L);
void launch_trsm(hipStream_t st, const DevSym &S, const FrontView *frec, int nactive, int kb, int mode, int max_rows_below,
                 double *L, double *Yh, const long long *yoff, const FrontArg &fa);
void launch_gemm_nt(hipStream_t st, const DevSym &S, const FrontView *frec, int nactive, int k0, int K, int c0, int c1,
                    int maxM, int maxN, double *L, const FrontArg &fa);
// cmin: fronts of at most cmin columns are skipped (passes of <= 16 right-hand sides: launch_fwd_update_wave has them, cmax = cmin)
void launch_fwd_update_recs(hipStream_t st, const DevSym &S, const FwdTile *recs, const SyrkSplit &split, int per_xcd, const double *L,
                            double *X, double *W, int nr, int ldx, int cmin = 0);
void launch_fwd_update_wave(hipStream_t st, const DevSym &S, const FwdTile *recs, const SyrkSplit &split, int per_xcd, const double *L,
                            double *X, double *W, int nr, int ldx, int cmax, bool split_k);      // split_k: the level has fronts wider than kWaveSplitCols
void launch_fwd_assemble(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_cols, double *X,
                         const double *W, int nr, int ldx);
void launch_fwd_update(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_trail, const double *L,
                       double *X, double *W, int nr, int ldx, int cmin = 0);

// inverse.hip -- dense L11^-1 of big fronts (recursive doubling) and the sweeps that use it
void launch_inv_stage(hipStream_t st, const DevSym &S, const int *list, int nactive, int B, int max_c, int phase,
                      double *L, double *T, const long long *toff);
// out: nfronts x cdiv(max_c, 256) partial maxima (front-major)
void launch_pivot_growth(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_c, const double *L, double *out);
void launch_xmul(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_c, int trans, const double *L,
                 const double *Xin, double *Xout, int nr, int ldx, int blk = 0, int cap = 1 << 30);
void launch_copy_own(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_c, const double *Xsrc,
                     double *Xdst, int nr, int ldx, int blk = 0, int cap = 1 << 30);
// X: rows of the ancestors (already final x, read only); Xown: the fronts' own rows, updated in place
void launch_bwd_gemm(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_cols, const double *L,
                     const double *X, double *Xown, int nr, int ldx, int blk = -1, int cap = 1 << 30, int mmin = 0);
// passes of at most 16 right-hand sides: the fronts with at most mmax trailing rows, one wave per 16 own columns (launch_bwd_gemm with
// mmin = mmax has the others)
void launch_bwd_wave(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_cols, const double *L, const double *X, double *Xown,
                     int nr, int ldx, int mmax, bool split_k);       // split_k: the level has fronts with more than kWaveSplitRows trailing rows
// blocked substitution inside fronts wider than `cap` columns (forward): own rows below block blk -= L[.., block] y_blk
void launch_fwd_own_update(hipStream_t st, const DevSym &S, const int *list, int nfronts, int max_cols, const double *L,
                           const double *Y, double *X, int nr, int ldx, int blk, int cap);
// iperm: position of original row i in the elimination order (nullptr: identity)
void launch_assemble_cyclic(hipStream_t st, const DevSym &S, const int *list, int ncols, const double *nzval, double *L, double *CB,
                            int cyc_w, int cyc_r, bool compact = false);     // compact: block-cyclic STORAGE (own blocks one behind the other)
void launch_syrk_cb_cyclic(hipStream_t st, const DevSym &S, const int *list, int trail, const double *L, double *CB, int cyc_w, int cyc_r, int cyc_b0);
void launch_level_mark(hipStream_t st, int phase, int level);   // phase 1 = forward sweep, 2 = backward sweep, 3 = factorisation, 4 = selected inversion
void launch_permute(hipStream_t st, const int *iperm, int n, double *Bc, long long ldb, double *X, int nr, int ldx, int dir);
void launch_newton_update(hipStream_t st, const double *prior, double *nz, long long nnz, const long long *map, const double *h,
                          long long cnt);
int quadform_blocks(int n);
void launch_quadform(hipStream_t st, int n, const long long *colptr, const int *row, const double *val, int use_lower,
                     const double *X, long long ldx, int nvec, const double *mu, double *part, double *out);
void launch_seg_wsum(hipStream_t st, const double *src, const long long *segptr, long long nseg, const long long *off,
                     const double *w, double *out);
void launch_seg_wsum_pairs(hipStream_t st, const double *src, const long long *segptr, long long nseg, const long long *off,
                           const int *pi, const int *qi, const double *vals, double *out);
void launch_logdet(hipStream_t st, const double *L, const long long *diagoff, const unsigned char *own, int n, double *part,
                   int nparts, double *out);
void launch_gather(hipStream_t st, const double *src, const long long *off, long long cnt, double *out);
void launch_gather_diag(hipStream_t st, const double *src, const long long *diagoff, const int *perm, int n, double *out);


// batch.hip -- per-member kernels of a batched handle (B members of nm nodes each, forest of N = B nm nodes)
int batch_diag_parts(int nm);
// logdet[k] = 2 sum log L_jj and info[k] = 0 or 1 + first member-local column with !(L_jj > 0), over the columns [k nm, (k+1) nm);
// psum / pbad: nbatch x batch_diag_parts(nm) partials
void launch_batch_diag(hipStream_t st, const double *L, const long long *diagoff, int nm, int nbatch, double *psum, int *pbad,
                       double *logdet, long long *info);
// launch_permute with a member stride: member k's block of the caller's array at A + k s (leading dimension ld)
void launch_batch_permute(hipStream_t st, const int *iperm, int N, int nm, double *A, long long ld, long long s, double *X, int nr, int ldx,
                          int dir);
int batch_quadform_blocks(int nm);
// out[k nvec + v] = (x_vk - mu_k)' Q_k (x_vk - mu_k): x_vk = X + k sx + v ldx, Q_k's values val + k nnz, mu_k = mu + k nm (nullable);
// part: nvec nbatch batch_quadform_blocks(nm) doubles
void launch_batch_quadform(hipStream_t st, int nm, const long long *colptr, const int *row, const double *val, long long nnz, int use_lower,
                           const double *X, long long ldx, long long sx, int nvec, int nbatch, const double *mu, double *part, double *out);

// klchol.hip -- KL (Vecchia-type) sparse approximate Cholesky (gmrfx_kl_cholesky): one task = the rows of a local system (nrows
// entries of rows[] from rows_off) and the columns of L it yields (ncols entries of cols[] from cols_off). The host driver: all
// index arrays 0-based, theta n x n column-major (host or device); returns -1, or the first task whose local matrix is not positive definite.
struct KlTask { long long rows_off, cols_off; int nrows, ncols; };
long long kl_cholesky_run(int device, long long n, const double *theta, long long ldt, bool theta_on_device, const std::vector<KlTask> &tasks,
                          const std::vector<int> &rows, const std::vector<int> &cols, const long long *Lcolptr, long long nnzL, double reg,
                          double *nzval_out);

// dense.hip -- the dense-operator leg of the Kronecker path: R = D T (row-major, D n1 x n1, T / R n1 x n2) and a transpose
void launch_dense_apply(hipStream_t st, const double *D, const double *T, double *R, int n1, long long n2);
void launch_transpose(hipStream_t st, const double *src, double *dst, long long rows, long long cols);

// constraint.hip -- linear equality constraints A x = e (m <= 64 sparse rows; At, B: n x m column-major, ld n)
// nb members (batched handles; a plain handle is one): member k's At / B at + k n m, Linv at + k m m, R at + k m cols, part at
// + k choff[m] cols, X at + k sx, mu at + k smu, add at + k m
// active (launch_con_ax, launch_con_apply): nb bytes on the device, nullable = all; a member whose byte is 0 is skipped by every
// workgroup before its first load and nothing of it is written (X, R, part)
constexpr int kConChunk = 4096;        // entries of a row of A per partial sum of A X (fixed: the sums' order depends on it)
constexpr int kConColTile = 8;         // columns of X per workgroup of the reduction
constexpr int kConApplyGroups = 2048;  // row-tile workgroups of the correction kernel per column block (they walk the tiles)
void launch_con_scatter(hipStream_t st, const long long *rowptr, const int *col, const double *val, int n, int m, long long maxlen, double *out,
                        int nb = 1);
// R[r + j m] = (A X)[r, j] (- e[r]) (+ add[r]); part: choff[m] k doubles, choff = prefix sum of the rows' chunk counts
void launch_con_ax(hipStream_t st, const long long *rowptr, const int *col, const double *val, const int *choff, int maxchunks, int m,
                   const double *X, long long ldx, int k, double *part, const double *e, const double *add, double *R, int nb = 1,
                   long long sx = 0, const unsigned char *active = nullptr);
void launch_con_trsm(hipStream_t st, const double *At, const double *Linv, int n, int m, double *B, int nb = 1);
void launch_con_var(hipStream_t st, const double *B, int n, int m, double *sig, int nb = 1);
// X <- X (+ mu) - B (Linv R); m = 0 with a mean: X += mu
void launch_con_apply(hipStream_t st, const double *B, const double *Linv, const double *R, const double *mu, double *X, long long ldx, int n,
                      int m, int k, int nb = 1, long long sx = 0, long long smu = 0, const unsigned char *active = nullptr);
// per member k < nb, one workgroup each: L_c L_c' = W_k (column-major m x m at W + k m m) -> Linv (row-major, + k m m), logdet[k],
// cinfo[k] = 0, 1 + failing pivot, or -1 when finfo[k] != 0 (finfo nullable); a failed member gets NaN
void launch_batch_con_chol(hipStream_t st, const double *W, int m, int nb, const long long *finfo, double *Linv, double *logdet, long long *cinfo);
// members with cinfo[k] = -1: NaN into their nat doubles of At and nw doubles of W
void launch_batch_con_void(hipStream_t st, const long long *cinfo, double *At, long long nat, double *W, int nw, int nb);
// out[k] = max_r |R[k m + r]| for the members of active (nbatch bytes on the device, nullable = all)
void launch_batch_con_maxabs(hipStream_t st, const double *R, int m, int nb, const unsigned char *active, double *out);
// quad[k] = |Linv_k r_k|^2, r_k = m values at R + k sr
void launch_batch_con_quad(hipStream_t st, const double *Linv, const double *R, long long sr, int m, int nb, double *quad);

// small.hip -- fused kernels for fronts with r <= 96 / 128 rows and c <= 64 columns
void launch_factor_small(hipStream_t st, const DevSym &S, const int *list, int nfronts, int rmax,
                         const double *nzval, double *L, double *CB, int *info);
// phase 0: factor, 1: forward sweep, 2: backward sweep of whole small subtrees (one workgroup per subtree)
void launch_subtree(hipStream_t st, const DevSym &S, int phase, const int *sub_first, const int *sub_last, int ntasks,
                    int rmax, const double *nzval, double *L, double *CB, int *info, double *X, double *W, int nr, int ldx);
// wmax: the widest block of the launch (<= 64): picks the workgroup shape (potrf64.hip)
void launch_potrf64(hipStream_t st, const DevSym &S, const FrontView *frec, int nactive, int kb, double *L, int *info, const FrontArg &fa,
                    int wmax = 64);
void launch_fwd_small(hipStream_t st, const DevSym &S, const int *list, int nfronts, int rmax, const double *L,
                      double *X, double *W, int nr, int ldx);
void launch_bwd_small(hipStream_t st, const DevSym &S, const int *list, int nfronts, int rmax, const double *L,
                      double *X, int nr, int ldx);

// backward step of a front of at most kFrontMaxCols columns (device_plan.h) as one workgroup (sweep_front.hip): x[own] = L11^-T (Yin[own] - L21' Xt[trailing])
void launch_bwd_front(hipStream_t st, const DevSym &S, const int *list, int nfronts, const double *L, const double *Xt, const double *Yin,
                      double *Xout, int nr, int ldx);
// the forward twin: the whole forward step of such a front (own rows assembled, Y[own] = L11^-1 b, W = children - L21 y) as one workgroup
void launch_fwd_front(hipStream_t st, const DevSym &S, const int *list, int nfronts, const double *L, const double *X, double *Y, double *W,
                      int nr, int ldx);
// chunk form of the sweep tasks (sweep_chunk.hip)
void launch_pack_diag(hipStream_t st, const Symbolic::SwChunk *recs, int nchunks, const double *L, double *dtile);
void launch_sweep_chunks(hipStream_t st, const DevSym &S, int phase, const SweepTask *tasks, int ntasks, const Symbolic::SwChunk *recs_fwd,
                         const Symbolic::SwChunk *recs_bwd, const int *listf, const int *listb, const double *dtile, const double *L,
                         double *X, double *W, int nr, int ldx, size_t extra_lds);

// sweep_wave.hip -- the same tasks, one wave per (task, 16 right-hand sides); order = task ids of one LDS class
void launch_wave_tasks(hipStream_t st, const DevSym &S, int phase, const SweepTask *tasks, const int *order, int ntasks, int rows_cap,
                       const double *L, const double *rdiag, const double *zero, double *X, double *W, int nr, int ldx);
void launch_rdiag(hipStream_t st, const double *L, const long long *diagoff, int n, double *out);

// selinv.hip -- Takahashi recursion, top-down over the supernodal tree
void launch_sel_gather(hipStream_t st, const SelRec *recs, const DevSym &S, const int *list, int nfronts, int max_trail,
                       const double *Z, double *ZB);
void launch_sel_symm(hipStream_t st, const DevSym &S, const int *list, int nactive, int kb, int max_rows_below,
                     double *Z, const double *ZB, const double *Yh, const long long *yoff);
void launch_sel_diag(hipStream_t st, const DevSym &S, const int *list, int nactive, int kb, const double *L,
                     double *Z, const double *Yh, const long long *yoff);
// whole-front Takahashi step for big fronts through the dense inverse X = L11^-1:
// phase 0: Yt = (L21 X)', phase 1: Z21 = -Z22 Y, phase 2: Z11 = X'X - Y' Z21
void launch_sel_dense(hipStream_t st, const DevSym &S, const int *list, int nfronts, int phase, int max_c, int max_trail,
                      const double *L, double *Z, const double *ZB, double *Yt, double *Z21t, const long long *woff);

// rbmc.hip -- Rao-Blackwellised Monte Carlo marginal variances (gmrfx_rbmc_var). Samples go through in blocks of kRbmcW columns:
// ONE pass of the backward sweep (Device::pass_width), and one sample per lane of a wave in the estimator kernels.
constexpr int kRbmcW = 64;
// symmetric row structure of Q (RbmcSym) and, for the block estimator, the plan's tables (RbmcPlan) on the device
struct RbmcDev {
    const long long *rp; const int *col, *pos, *dpos;
    const long long *bptr; const int *rows, *ns; const unsigned char *owner; const long long *eptr; const int *loc;
};
// blocks per launch of a size class: the classes that keep Q_BB (<= 512 rows) or R (<= 128, <= 512) in global scratch index it by workgroup
inline int rbmc_class_chunk(int cls) { return cls == 3 ? 128 : (cls == 2 ? 1024 : 1 << 20); }
// Xc (column-major n x w, ld n) -> Xt (row-major n x kRbmcW, zeros from column w on)
void launch_rbmc_transpose(hipStream_t st, const double *Xc, long long n, int w, double *Xt);
// one block of w samples after na earlier ones: the rows' (mean, M2) merged in place; last: out = base + M2 / (k - 1)
void launch_rbmc_plain(hipStream_t st, const RbmcDev &P, long long n, const double *val, const double *Xt, long long na, int w, bool last,
                       long long k, double *mean, double *m2, double *out);
void launch_rbmc_blocks(hipStream_t st, const RbmcDev &P, int cls, const int *order, int cnt, const double *val, const double *Xt, long long na,
                        int w, bool first, bool last, long long k, double *mean, double *m2, double *base, double *out, double *scrM,
                        double *scrR);

// grad.hip -- log-density gradients on the pattern of Q (gmrfx_logpdf_grad, gmrfx_pattern_dot). nb members (a plain handle is one):
// member k's values / offsets / Qbar at + k nnz, vectors at + k n, Bt at + k n m, tw at + k 2m, ybar[k], bad[k] (nullable; nonzero: NaN)
struct GradPattern {
    int n, m;                    // m = 0: no constraint (Bt, u unused)
    long long nnz;
    const long long *colptr;     // the member's pattern
    const int *row;
    const long long *zoff;       // offset of every stored entry in the selected-inverse panels
    const double *Z, *r, *ybar, *Bt, *u;
    const long long *bad;
    double *Qbar;
};
struct GradMean {
    int n, m;
    long long nnz;
    const long long *rp;         // Symmetric(Q) by rows (RbmcSym): row pointers, columns, positions in the caller's values
    const int *col, *pos;
    const double *val, *r, *ybar;
    const long long *acolptr;    // A by columns (nullable: no constraint)
    const int *arow;
    const double *aval, *tw;
    const long long *bad;
    double *mubar;
};
void launch_grad_residual(hipStream_t st, int n, int nb, const double *z, long long sz, const double *mu, double *r);
void launch_grad_bt(hipStream_t st, int n, int m, int nb, const double *B, double *Bt);
// tw: per member t = L_c^-1 (e - A mu), then w = L_c^-T t, from R = A mu - e
void launch_grad_tw(hipStream_t st, int m, int nb, const double *Linv, const double *R, double *tw);
void launch_grad_u(hipStream_t st, int n, int m, int nb, const double *B, const double *tw, double *u);
void launch_grad_pattern(hipStream_t st, const GradPattern &a, int nb);
void launch_grad_mubar(hipStream_t st, const GradMean &a, int nb);
// out[k p + c] = sum_e wgt[e] G[k nnz + e] J[k sj + c ldj + e]; part: nb p choose_grad_dot(nnz, p, nb).gx doubles
void launch_grad_dot(hipStream_t st, long long nnz, const unsigned char *wgt, const double *G, const double *J, long long ldj, long long sj, int p,
                     int nb, double *part, double *out);

// fisher.hip -- one pass over Symmetric(Q_prior) for a Fisher-scoring iterate (gmrfx_fisher_eval, gmrfx_batch_fisher_eval): a lane group of
// kFisherLanes lanes per row, kFisherRows rows per workgroup of 256 threads; the final pass adds the workgroups' partial sums with
// kFisherFinal threads. nbatch members (a plain handle is one, with strides 0): the member in the grid's second dimension, ONE copy of
// the member's row structure and ONE data set, per-member values / points / parameters. A workgroup never spans two members; the partial
// sums are kept per member and reduced by one workgroup per member, so member k's results have the bits of a plain handle of Q_p,k,
// param[k] and x_k. active (nbatch bytes, nullable = all): a member whose byte is 0 is skipped by every workgroup before its first load,
// and nothing of it is written. A per-member scalar is the by-value argument unless its device array (nbatch) is non-null.
constexpr int kFisherLanes = 16, kFisherRows = 16, kFisherFinal = 256;
struct FisherEval {
    int n, family;
    const long long *rp;         // the MEMBER's Symmetric(Q) by rows (RbmcSym), as GradMean: n + 1
    const int *col, *pos;
    const double *val, *x, *mu;  // the priors' values; the points; the prior means (nullable: h = 0)
    const double *y, *aux;       // ONE likelihood by node (aux nullable)
    const unsigned char *mask;   // 1: the node has an observation
    double param, logparam;
    double *score, *hess;        // n each, either nullable
    double *part;                // 2 per workgroup: energy, loglik; member k's at + 2 k fisher_blocks(n)
    // the members, behind what one member needs (a plain handle leaves them zero and its workgroups never fetch them)
    long long nnz, sx, smu, ss;  // member k's val at + k nnz, x at + k sx, mu at + k smu (0: one mean for all), score / hess at + k ss
    const double *param_k, *logparam_k;  // nullable: one per member, in place of param / logparam
    const unsigned char *active; // nullable
};
inline int fisher_blocks(int n) { return (n + kFisherRows - 1) / kFisherRows; }
// out[2 k] = member k's sum of the energy partials, out[2 k + 1] = of the loglik partials (device); inactive members' pairs are left
void launch_fisher_eval(hipStream_t st, const FisherEval &a, int nbatch, double *out);
// the loop's vector work (gmrfx_gaussian_approximation, gmrfx_batch_gaussian_approximation) on vectors of n entries per member, member
// k's at + k stride (the loop's work vectors), for the members whose byte in active is set (nullable = all)
struct FisherMembers { int n, nbatch; long long stride; const unsigned char *active; };
// out_k = x_k - alpha s_k (alpha_k non-null: alpha_k[k] s_k); out may be x
void launch_fisher_candidate(hipStream_t st, const FisherMembers &m, const double *x, const double *s, double alpha, const double *alpha_k,
                             double *out);
// out4[4 k ..] = {sum a b, sum (c - d)^2, sum d^2, max |b|} over member k's entries (a pair with a null member is left at 0), in chunks
// of kFisherStatChunk entries; part: 4 per chunk, member k's at + 4 k fisher_stat_blocks(n)
constexpr int kFisherStatChunk = 4096;
inline int fisher_stat_blocks(int n) { return (n + kFisherStatChunk - 1) / kFisherStatChunk; }
void launch_fisher_stats(hipStream_t st, const FisherMembers &m, const double *a, const double *b, const double *c, const double *d, double *part,
                         double *out4);

// fisher_design.hip -- the same evaluation through a sparse design matrix, eta = A x + b (gmrfx_obs_set_design). A lane group of
// kDesignLanes lanes per row of A, per node and per Hessian position, kDesignRows of them per workgroup of 256 threads. A SEGMENT (a
// column of A for A' g, a position's term list for A' D A) of at most kDesignChunk entries is summed by its lane group; a longer one is
// cut into chunks of kDesignChunk entries, one workgroup each, whose sums the lane group then adds (design_chunks of them, in order).
constexpr int kDesignLanes = 16, kDesignRows = 16, kDesignChunk = 512;
static_assert(kDesignLanes == kFisherLanes && kDesignRows == kFisherRows, "the energy of the design form has the bits of the node form");
inline int design_chunks(long long len) { return len > kDesignChunk ? (int)((len + kDesignChunk - 1) / kDesignChunk) : 0; }
inline int design_blocks(long long rows) { return (int)((rows + kDesignRows - 1) / kDesignRows); }
struct FisherDesign {
    int n, nobs, cnt, family;
    const long long *rp;         // Symmetric(Q) by rows, as FisherEval
    const int *col, *pos;
    const double *val, *x, *mu;
    const long long *arp;        // A by rows: nobs + 1
    const int *acol;
    const double *aval, *offset; // offset nullable
    const long long *acp;        // A by columns: n + 1
    const int *arow;
    const double *acv;
    const long long *tptr;       // the term lists: cnt + 1
    const int *tobs;
    const double *tw;
    const int *cchoff, *tchoff;  // n + 1 / cnt + 1: prefix sums of design_chunks over the columns / term lists (the latter from ncc on)
    const long long *chs;        // ncc + nct: first entry of every chunk (columns' chunks first)
    const int *chl;              // and its length
    int ncc, nct;
    const double *y, *aux;       // by observation (aux nullable)
    double param, logparam;
    double *g, *d;               // nobs each: work
    double *cpart;               // ncc + nct chunk sums
    double *score, *hess;        // n / cnt, either nullable
    double *epart, *lpart;       // energy per workgroup of nodes, loglik per workgroup of observations
    // the members, behind what one member needs (a plain handle leaves them zero): member k's val at + k nnz, x at + k sx, mu at + k smu
    // (0: one mean for all), score at + k ss, hess at + k sh (>= cnt), g and d at + k nobs, cpart at + k (ncc + nct), epart at
    // + k design_blocks(n), lpart at + k design_blocks(nobs); the tables, y, aux and offset are one copy
    long long nnz, sx, smu, ss, sh;
    const double *param_k, *logparam_k;  // nullable: one per member, in place of param / logparam
    const unsigned char *active; // nullable = all; a member whose byte is 0 is skipped and nothing of it is written
};
// nbatch members (a plain handle: 1): out[2 k] = member k's energy, out[2 k + 1] = its sum of the x-dependent terms of loglik (device);
// inactive members' pairs are left
void launch_fisher_design(hipStream_t st, const FisherDesign &a, int nbatch, double *out);
// A composite likelihood (gmrfx_obs_set_composite): the rows of A belong to ncomp <= kObsMaxComponents components, each with a family
// and a parameter of its own. comp[i]: the component of observation i (one byte beside the >= 20 a row reads); family / param /
// logparam: ncomp each, in device memory (a lane-varying index into a by-value array would send the array to scratch). The kernels
// that take one read the row's (family, param, logparam) there and ignore those of their first argument; everything else is the
// single-family kernel's: same lane groups, same order of summation, same trees.
struct ObsComp {
    const unsigned char *comp;   // nobs
    const int *family;           // ncomp
    const double *param, *logparam;
};
// the same launch sequence with k_design_eta_comp in place of k_design_eta (the other four kernels never read the family)
void launch_fisher_design_comp(hipStream_t st, const FisherDesign &a, const ObsComp &t, int nbatch, double *out);

// ga_pullback.hip -- the array arithmetic of the implicit-function rule of the Gaussian approximation (gmrfx_ga_pullback,
// gmrfx_batch_ga_pullback). The solve in the middle is the handle's own; these are the kernels on either side of it. Node form: one
// thread per node, kGapNode nodes per workgroup. Design form: the lane-group layout of fisher_design.hip (kDesignLanes lanes per row of
// A / per node, kDesignRows per workgroup), the columns of A cut into chunks by the same design_chunks() rule. The pattern and mean
// kernels have the layout of k_grad_pattern / k_grad_mubar (device_plan.h: kGradLanes, kGradCols, kGradRows).
// nbatch members (a plain handle is one, strides 0, scalars by value, nobody masked): the member in the grid's second dimension
// (the first in k_gap_final), ONE copy of every table, the data set and the member's slice of the Hessian map; per-member cotangents,
// points, work vectors and partial sums. A workgroup never spans two members; active (nbatch bytes, nullable = all): a member whose
// byte is 0 is skipped by every workgroup before its first load, and nothing of it is written.
constexpr int kGapNode = 256;
inline int gap_node_blocks(int n) { return (n + kGapNode - 1) / kGapNode; }
// workgroups of the per-observation kernels (k_gap_point*, k_gap_param*), and so the partial sums each of them leaves per member
inline int gap_obs_blocks(bool design, long long n, long long nobs) { return design ? design_blocks(nobs) : gap_node_blocks((int)n); }
struct GapPoint {
    int n, nobs, family;
    const double *G;             // the precision cotangent on the pattern (nnz)
    const long long *hmap;       // the map of gmrfx_set_prior: the position of (i, i) in node form, of the plan's pairs in design form
    const double *x, *mubar;     // the mode; the mean cotangent (nullable: 0)
    const double *y, *aux;       // the likelihood, by node / by observation (aux nullable)
    const unsigned char *mask;   // node form: 1 = observed
    const long long *arp;        // design form: A by rows, the offset (nullable), the transposed term table of the plan
    const int *acol;
    const double *aval, *offset;
    const long long *optr;
    const int *oidx;
    const double *ow;
    double param, logparam;
    double *t;                   // design form, nobs: t_i = c_i d3_i
    double *xbar;                // node form: mubar_i - t_i, n
    double *ppart;               // sum of c_i dp_i per workgroup; member k's at + k gap_obs_blocks(...)
    // the members, behind what one member needs (a plain handle leaves them zero): member k's G at + k sg (hmap is the MEMBER's slice:
    // positions in one member's values), x at + k sx, mubar at + k sm, t at + k nobs, xbar at + k sw
    long long sg, sx, sm, sw;
    const double *param_k, *logparam_k;  // nullable: one per member, in place of param / logparam
    const unsigned char *active; // nullable = all
};
void launch_gap_point(hipStream_t st, const GapPoint &a, bool design, int nbatch);
struct GapGather {
    int n, ncc;
    const long long *acp;        // A by columns
    const int *arow;
    const double *acv;
    const int *cchoff;           // the chunk tables of the long columns (FisherDesign)
    const long long *chs;
    const int *chl;
    const double *t, *mubar;     // mubar nullable
    double *cpart, *xbar;
    // the members: member k's t at + k st, mubar at + k sm, cpart at + k sc, xbar at + k sw
    long long st, sm, sc, sw;
    const unsigned char *active;
};
void launch_gap_gather(hipStream_t st, const GapGather &a, int nbatch);
struct GapPattern {
    int n;
    const long long *colptr;     // the MEMBER's pattern of Q
    const int *row;
    const double *G;             // nullable: 0
    const double *lam, *x, *mu;  // mu nullable
    double *out;                 // nnz; may be G itself
    // the members: member k's G and out at + k sg, lam at + k sw, x at + k sx, mu at + k smu (0: one mean for all)
    long long sg, sw, sx, smu;
    const unsigned char *active;
};
void launch_gap_pattern(hipStream_t st, const GapPattern &a, int nbatch);
// out_i = sum_q val[pos[q]] lam[col[q]] over row i of the member's Symmetric(Q) (RbmcSym); member k's val at + k nnz, lam at + k sw,
// out at + k so
struct GapMean {
    int n;
    const long long *rp;
    const int *col, *pos;
    const double *val, *lam;
    double *out;
    long long nnz, sw, so;
    const unsigned char *active;
};
void launch_gap_mean(hipStream_t st, const GapMean &a, int nbatch);
struct GapParam {
    int n, nobs, family;
    const double *lam, *x;
    const double *y, *aux;
    const unsigned char *mask;
    const long long *arp;        // design form: eta is formed again beside A lam, in the same pass over the row
    const int *acol;
    const double *aval, *offset;
    double param, logparam;
    double *gpart;               // sum of (A lam)_i gp_i per workgroup; member k's at + k gap_obs_blocks(...)
    // the members: member k's lam at + k sw, x at + k sx
    long long sw, sx;
    const double *param_k, *logparam_k;
    const unsigned char *active;
};
void launch_gap_param(hipStream_t st, const GapParam &a, bool design, int nbatch);
// out[k] = sum of member k's gpart - sum of its ppart (np / ng = 0: that sum is 0); one workgroup per member, inactive members' left
void launch_gap_final(hipStream_t st, const double *gpart, int ng, const double *ppart, int np, const unsigned char *active, int nbatch, double *out);
// dst_k = src_k (n entries; member k's at + k sd / + k ss) for the active members; dst_k = NaN for the INACTIVE ones (gap_fill_failed:
// what a member whose factorisation or W_k failed gets in its output slices)
void launch_gap_copy(hipStream_t st, long long n, const double *src, long long ss, double *dst, long long sd, const unsigned char *active, int nbatch);
void launch_gap_fill_failed(hipStream_t st, long long n, double *dst, long long sd, const unsigned char *active, int nbatch);
// A composite likelihood (gmrfx_ga_pullback_composite): the parameter cotangent is one number per component, so no workgroup's
// partial sum may mix components. The observations are tiled PER COMPONENT: component c owns workgroups bptr[c] .. bptr[c + 1],
// bptr[c + 1] - bptr[c] = design_blocks(rows of c); workgroup b of c takes rows rowptr[c] + kDesignRows (b - bptr[c]) .., cut at
// rowptr[c + 1]. At most design_blocks(nobs) + ncomp - 1 workgroups; one component: the tiling of k_gap_point. bptr (ncomp + 1) and
// rowptr (ncomp + 1) lie in device memory; a workgroup finds its component by a uniform search over bptr.
struct GapTiles {
    int ncomp;
    const int *bptr;
    const long long *rowptr;
};
// bptr of the tiling above from the components' row offsets (ncomp + 1 entries each); returns the number of workgroups
inline int gap_comp_tiles(const long long *rowptr, int ncomp, int *bptr) {
    bptr[0] = 0;
    for (int c = 0; c < ncomp; c++) bptr[c + 1] = bptr[c] + design_blocks(rowptr[c + 1] - rowptr[c]);
    return bptr[ncomp];
}
// k_gap_point_comp / k_gap_param_comp: the design-form kernels on that tiling with the component's (family, param, logparam) from the
// table (a.family / a.param / a.logparam and the *_k arrays are ignored); nblk = bptr[ncomp] workgroups and partial sums per member.
// A component whose family has no parameter leaves 0 in its partials of (A lam) gp without walking its rows.
void launch_gap_point_comp(hipStream_t st, const GapPoint &a, const ObsComp &t, const GapTiles &w, int nblk, int nbatch);
void launch_gap_param_comp(hipStream_t st, const GapParam &a, const ObsComp &t, const GapTiles &w, int nblk, int nbatch);
// out[k ncomp + c] = sum of gpart over c's workgroups - sum of ppart over them (has_p false: that sum is 0), in the order of
// k_gap_final; one workgroup per component and member, member k's partials at + k nblk
void launch_gap_final_comp(hipStream_t st, const double *gpart, const double *ppart, bool has_p, const GapTiles &w, int nblk,
                           const unsigned char *active, int nbatch, double *out);

// predictive.hip -- the marginals of the linear predictor (gmrfx_predictor_marginals, gmrfx_batch_predictor_marginals), the quadrature
// scores over them (gmrfx_predictive_scores, gmrfx_batch_predictive_scores) and the mixture of the members' predictive distributions
// (gmrfx_batch_predictive_mixture). Node form: one thread per observation, kPredNode per workgroup. Design form and the scores: the
// lane-group layout of fisher_design.hip (kDesignLanes lanes per observation, kDesignRows observations per workgroup of 256 threads).
// nbatch members (a plain handle is one, strides 0, scalars by value, nobody masked): the member in the grid's second dimension (the
// first in k_pred_final), ONE copy of every table and of the data set; per-member points, selected inverse, B, constants, outputs and
// partial sums. A workgroup never spans two members; active (nbatch bytes, nullable = all): a member whose byte is 0 is skipped by
// every workgroup before its first load, and nothing of it is written.
constexpr int kPredNode = 256, kPredMaxNodes = 64, kPredNodesPerLane = kPredMaxNodes / kDesignLanes, kPredMix = 256;
struct PredMarg {
    int n, nobs, m, family;      // m: columns of B to subtract (0: no correction, no clamp)
    const double *x;             // the posterior mean, n
    const int *idx;              // node form: the observed node of every observation, in the caller's order
    const int *dpos;             // node form: position of (j, j) in the pattern, per node (RbmcSym::diag)
    const long long *arp;        // design form: A by rows, the offset (nullable), the transposed term table and the plan's map
    const int *acol;
    const double *aval, *offset;
    const long long *optr;
    const int *oidx;
    const double *ow;
    const long long *hmap;
    const long long *zoff;       // offset of every stored entry of Q in the selected-inverse panels (null: no variance wanted)
    const double *Z;
    const double *B;             // the constraint's B = Q^-1 A' L_c^-T, n x m column-major
    const double *y, *aux;       // by node (node form) / by observation (design form); aux nullable
    const double *c;             // the constant of every observation's log density, nobs
    double param, logparam;
    double *mu_eta, *v_eta, *pll;        // nobs each, each nullable
    // the members, behind what one member needs (a plain handle leaves them zero): member k's x at + k sx, its entries of zoff at
    // + k sz (dpos and hmap are the MEMBER's: positions in one member's values; the offsets themselves are absolute), B at + k sb,
    // c at + k sc (0: one column for all), mu_eta / v_eta / pll at + k so
    long long sx, sz, sb, sc, so;
    const double *param_k, *logparam_k;  // nullable: one per member, in place of param / logparam
    const unsigned char *active; // nullable = all
};
void launch_pred_marginals(hipStream_t st, const PredMarg &a, bool design, int nbatch);
// a composite likelihood (design form only): k_pred_design_comp; a.c holds every observation's constant under its own component
void launch_pred_marginals_comp(hipStream_t st, const PredMarg &a, const ObsComp &t, int nbatch);
struct PredScores {
    int nobs, K, family;
    const double *mu, *v;        // nobs each
    const int *idx;              // node form: y / aux are by node; null: by observation
    const double *y, *aux, *c;
    const double *z, *w;         // K quadrature nodes and weights of the standard normal
    double param, logparam;
    double *lpd, *lcpo, *elp, *vlp;      // nobs each, each nullable
    double *part;                // 4 per workgroup
    // the members: member k's mu and v at + k sm, c at + k sc (0: one column for all), lpd / lcpo / elp / vlp at + k so, part at
    // + 4 k design_blocks(nobs)
    long long sm, sc, so;
    const double *param_k, *logparam_k;
    const unsigned char *active;
};
// out4 (device) = member k's totals of lpd, lcpo, elp, vlp at + 4 k; inactive members' are left
void launch_pred_scores(hipStream_t st, const PredScores &a, int nbatch, double *out4);
void launch_pred_scores_comp(hipStream_t st, const PredScores &a, const ObsComp &t, int nbatch, double *out4);      // (a.idx null: by observation)
// The mixture over the members with weights omega_k (w: nbatch weights, then nbatch logs of them; a member whose log is -inf is never
// read): mix_mu = sum omega mu, mix_v = sum omega (v + (mu - mix_mu)^2), mix_lpd = log sum exp(log omega + lpd). mu, v, lpd (nullable):
// nobs x nbatch, member stride nobs; mix_* nobs each, nullable. One thread per observation, members in ascending order. With lpd:
// part gets 4 per workgroup (the sum of mix_lpd, then zeros) and out4[0] their total in the order of k_pred_final.
struct PredMix {
    int nobs, nbatch;
    const double *w;
    const double *mu, *v, *lpd;
    double *mix_mu, *mix_v, *mix_lpd;
    double *part;
};
inline int pred_mix_blocks(long long nobs) { return (int)((nobs + kPredMix - 1) / kPredMix); }
void launch_pred_mixture(hipStream_t st, const PredMix &a, double *out4);

}  // namespace gmrfx
