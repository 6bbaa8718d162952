// device.h -- device-resident symbolic structure + numeric drivers (HIP, gfx950).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "device_plan.h"
#include "fisher_design_plan.h"
#include "ga_rules.h"
#include "rbmc_plan.h"
#include "resource.h"

namespace gmrfx {

// Pointers to the symbolic structure in HBM; passed to kernels by value.
struct DevSym {
    int n, nsuper;
    const int *sfirst;          // nsuper+1
    const long long *rowptr;    // nsuper+1
    const int *rows;            // sum_rows (permuted indices; own columns first)
    const int *rel;             // sum_rows (index in parent's row list for trailing rows)
    const long long *panelptr;  // nsuper+1 (doubles)
    const int *ld;              // nsuper
    const long long *cbptr;     // nsuper (doubles, contribution-block arena)
    const long long *childptr;  // nsuper+1
    const int *children;
    const int *sparent;
    const long long *qptr;      // nsuper+1
    const int *qsrc;            // index into caller nzval
    const int *qdst;            // destination ROW inside the panel column qcol (entries sorted by column, then row)
    const int *qcol;            // front-local destination column (row / column kept apart: a panel may hold more
                                // than 2^31 entries -- the 47 000-column root of a 126^3-node 3-D mesh)
    const int *qcolptr;         // n+1: first entry (index into qsrc / qdst) of every column of L, in elimination order
    const int *erow;            // per child edge, per own column tc of the parent (EdgeRec::eoff + tc): the child's trailing
                                // row that maps to that column, or -1 -- the panel assembly looks up, it does not search
    const long long *wptr;      // nsuper+1: prefix sum of trailing rows (r-c)
    const long long *diagoff;   // n
    const int *perm;            // n
    const EdgeRec *edge;        // one per child edge (same index as `children`)
    // etile[tptr + T], T = 0 .. ceil((r_p - c_p) / 32): first trailing row a of the child whose
    // position in the parent is >= c_p + 32 T (the child's rows falling into the parent's 32-row
    // trailing tile T are [etile[T], etile[T+1]) -- no search at run time)
    const int *etile;
    const int *lrow;            // sum_rows: local row (sweep tasks) of every trailing row of a task front
    const unsigned char *foreign_parent;   // sharded handles: 1 = the parent of this front is owned by another rank
                                           // (its trailing inverse block arrives over the wire: no local gather); else null
};

// geometry of one front for the panel kernels in the kernel arguments (FrontView: the same as one record per level-list position)
// ppa (round 6): where the K operand columns of a panel update live when they are NOT in the panel itself -- the received block of a
// distributed front with block-cyclic storage sits in a window (Device::dist_front_phase); kNoPpa = in the panel, as everywhere else
// Linear equality constraints A x = e as the handle keeps them on the host (gmrfx_constraints_set): m sparse rows, 0-based 32-bit
// columns sorted and unique within a row, the right-hand side e and log det(A A').
struct ConHost {
    int m = 0;
    std::vector<long long> rowptr;
    std::vector<int> col;
    std::vector<double> val, e;
    double logdet_AAt = 0;
};

// The observation likelihood a plain handle keeps (gmrfx_obs_set), host copy, also on symbolic_only handles; nobs = 0: none.
// Families (canonical or log link, reference canonical_implementations.jl:146-327): 0 Normal / identity (param sigma), 1 Poisson / log
// (aux = log exposure), 2 Bernoulli / logit, 3 Binomial / logit (aux = trials), 4 NegativeBinomial / log (aux = log exposure, param r),
// 5 Gamma / log (param phi). idx: the observed nodes, 0-based, in the caller's order; y and aux (empty: none) go with them.
// design (gmrfx_obs_set_design): non-null when the likelihood is observed through eta = A x + b; idx is then empty and y / aux go
// with the rows of A.
// comp (gmrfx_obs_set_composite): non-empty when the rows of A belong to several components, each with a family and a parameter of its
// own; family is then kObsComposite, param unused, aux one value per row (0 on the rows of components without one; empty: none given)
// and loglik_const the sum of the components'.
constexpr int kObsFamilies = 6, kObsMaxComponents = 16, kObsComposite = -2;
struct ObsComponents {
    std::vector<int> family;                 // ncomp
    std::vector<double> param, loglik_const; // ncomp each: the component's parameter and its constant over its own rows
    std::vector<long long> rowptr;           // ncomp + 1: component c owns rows rowptr[c] .. rowptr[c + 1]
    bool empty() const { return family.empty(); }
    size_t size() const { return family.size(); }
};
struct ObsComp;
struct ObsHost {
    int family = 0;
    long long nobs = 0;
    std::vector<long long> idx;
    std::vector<double> y, aux;
    double param = 0, loglik_const = 0;      // the sum of the terms of loglik that do not depend on x (long double on the host)
    std::shared_ptr<const DesignPlan> design;
    ObsComponents comp;
};
// The likelihood of a batched handle (gmrfx_batch_obs_set): ONE data set (idx, y, aux as in ObsHost) and one parameter per member, with
// the member's loglik_const; nobs = 0: none. A plain handle keeps one too, as a batch of one, beside the ObsHost of gmrfx_obs_set.
constexpr int kBatchFisherMaxMembers = 65535;      // the member is the second dimension of the launch grid
struct BObsHost {
    int family = 0;
    long long nobs = 0;
    std::vector<long long> idx;
    std::vector<double> y, aux, param, loglik_const;      // param, loglik_const: one per member
    std::shared_ptr<const DesignPlan> design;             // gmrfx_batch_obs_set_design: the plan on the MEMBER's pattern (idx empty)
};
// what the node form of either likelihood puts on the device: (idx, y, aux) expanded to one value per node, mask = 1 where a node has
// an observation, 0 elsewhere (aux stays empty when there is none)
struct ObsByNode { std::vector<double> y, aux; std::vector<unsigned char> mask; };
ObsByNode obs_by_node(size_t n, long long nobs, const std::vector<long long> &idx, const std::vector<double> &y, const std::vector<double> &aux);
// the log r the negative binomial's stable forms take beside r (fisher_point.h); the other families do not read it
inline double fisher_logparam(int family, double param) { return family == 4 ? std::log(param) : 0.0; }

constexpr long long kNoPpa = (long long)0x8000000000000000ull;
struct FrontArg { int on, s, c, r, ld, first; long long pp; long long ppa = kNoPpa; };
// Where one sweep pass runs: a stream and the right-hand-side buffers it works in (X: the pass's columns in elimination order,
// X2: y of the big fronts, W: the update vectors). The sweep drivers take it as a parameter; nothing selects a lane by state.
struct SweepLane { hipStream_t st; double *X, *X2, *W; };
struct FisherMembers;      // (kernels.h)
struct SyrkLevelTimes;     // (kernels.h)
class Device {
public:
    Device() = default;
    ~Device();
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;

    // Uploads the symbolic structure; allocates factor / arena storage. Throws on HIP errors.
    void init(const Symbolic &S, int device);
    void clone_from(const Device &o, const Symbolic &S);

    void refactorize(const double *nzval, bool on_device);
    // numeric factorisation + solve as ONE pipelined call (gmrfx_refactorize_solve): the forward sweep follows the factorisation
    // up the tree, one level behind, on the side stream
    void refactorize_solve(const double *nzval, bool nz_on_device, const double *B, long long ldb, long long nrhs, double *X, long long ldx,
                           bool b_on_device);
    void refactorize_logpdf(const double *d_nz, const double *d_X, long long ldx, long long nvec, const double *d_mu, double *quad_out,
                            double *logdet_out);
    void refactorize_update_solve(const double *h, bool h_on_device, const double *B, long long ldb, long long nrhs, double *X, long long ldx,
                                  bool b_on_device);
    // Newton loop with Q resident on the device: set_prior uploads the prior's values (and the
    // Hessian -> Q index map) once; refactorize_update forms nz = prior, nz[map[k]] -= h[k] on the device from the
    // cnt Hessian values (host or device) and refactorises -- only h crosses PCIe per iterate.
    void set_prior(const double *prior_nzval, const long long *map, long long cnt);
    void refactorize_update(const double *h, bool on_device);
    // sharded handles: phase 0 = the subtrees this rank owns, phase 1 = the top fronts (rank 0; after the
    // contribution blocks of the other ranks' subtree roots have been written into cb_arena())
    void refactorize_phase(const double *d_nzval, int phase);
    // sharded solve (device buffers, nrhs <= 64): 0 = transpose in + forward over the own subtrees, 1 = the top
    // (forward, then backward; rank 0), 2 = backward over the own subtrees, 3 = transpose out (rank 0, after
    // the owned rows have been gathered). Between the phases the host moves W / X rows (gmrfx/shard.py).
    void solve_phase(const double *d_B, long long ldb, long long nrhs, double *d_X, long long ldx, int phase);
    double *rhs_x() { return d_X_; }
    double *rhs_w() { return d_W_; }
    void ensure_rhs(long long nrhs) { ensure_rhs_capacity(nrhs); }
    // columns per sweep pass for a solve of nrhs right-hand sides: ONE rule for solve() and the pipelined call, so that both give
    // the same bits for the same nrhs. 64 throughout. (Round 6, measured and dropped: 17 .. 32 right-hand sides as TWO 16-column
    // passes side by side on the two lanes -- 17 / 24 / 32 columns 3.01 / 3.35 / 3.71 ms against 3.40 / 3.4 / 3.44 as one pass: two
    // latency-bound passes do not overlap on this runtime (twice the launches through one command processor), the second lane only
    // pays from 65 columns on. What such passes get instead: the narrow level kernels on two right-hand-side tiles, kNarrowPassMax.)
    static int pass_width(long long) { return 64; }
    double *cb_arena() { return d_cb_; }
    double *factor_panels() { return d_L_; }
    bool sharded() const { return S_ && S_->shard_plan; }
    // B: column-major n x nrhs (original ordering); mode 0: full solve, 1: backward only (P' L^-T Z)
    // ml (batched handles, device arrays only): member k's n_member x nrhs block of B / X at + k sin / + k sout, leading dimension ldb / ldx
    struct MemberLayout { long long n_member, sin, sout; };
    void solve(const double *B, long long ldb, long long nrhs, double *X, long long ldx, bool on_device, int mode,
               const MemberLayout *ml = nullptr);
    // ---- batched handles (gmrfx_create_batched): nbatch members of n_member nodes, the forest diag(Q_1 .. Q_B) -------------------
    void set_batch(int nbatch, long long n_member, long long nnz_member);
    bool batched() const { return (bool)h_bdiag_; }
    // more than one member: what the plain-handle-only calls (obs_set, fisher_eval, ga_pullback, predictor_marginals, predictive_scores)
    // refuse. NOT batched(): a plain handle becomes a batch of one on its first gmrfx_batch_* call and stays a plain handle to them.
    bool many_members() const { return nbatch_ > 1; }
    // per-member log det / pivot status (1 + member-local column, 0 = fine) of the current factorisation, host arrays of nbatch
    void batch_diag(double *logdet_out, long long *info_out);
    // quad[k nvec + v] = (x_vk - mu_k)' Q_k (x_vk - mu_k), device operands: x_vk = d_X + k sx + v ldx, Q_k = d_nz + k nnz_member,
    // mu_k = d_mu + k n_member (nullable); quad is a host array of nvec nbatch
    void batch_quadform(const double *d_nz, const double *d_X, long long ldx, long long sx, long long nvec, const double *d_mu, double *quad_out);
    // refactorisation + batch_quadform beside it + batch_diag, one synchronisation: same bits as the three calls
    void batch_refactorize_logpdf(const double *d_nz, const double *d_X, long long ldx, long long sx, long long nvec, const double *d_mu,
                                  double *quad_out, double *logdet_out, long long *info_out);
    double logdet();
    // q[v] = (x_v - mu)' Q (x_v - mu), v < nvec, on the device: x_v = d_X + v * ldx, d_mu nullable (zero mean).
    // d_nz = Q's values in the pattern's CSC order (device); nullptr = the values of the last refactorisation
    // when the handle holds them itself (host-pointer refactorize / refactorize_update).
    void quadform(const double *d_nz, const double *d_X, long long ldx, long long nvec, const double *d_mu, double *out_host);
    void selinv_compute();
    // sharded selected inversion, top-down (include/gmrfx.h): 0 = begin, 1 = gather the trailing inverse blocks of the
    // OTHER ranks' fronts at level `hi` whose parents this rank owns (they are then sent to their owners),
    // 2 = this rank's fronts of levels hi-1 .. lo, 3 = end
    void selinv_phase(int what, int hi, int lo);
    void selinv_diag(double *out_host);
    void gather_z(const long long *offsets_host, long long cnt, double *out_host);  // offsets into panel storage, -1 -> 0.0
    // out[g] = sum_{t in segment g} w[t] * Z[off[t]] (off = -1 -> 0), all arrays on the host; Z = selected inverse panels
    void weighted_z_sums(const long long *segptr_host, long long nseg, const long long *off_host, const double *w_host, double *out_host);
    // diag(A Sigma A') with the pair plan of a design matrix kept on the device: only A's values go in and the m
    // results come out per call (the plan depends on the pattern of A and on the symbolic structure only)
    long long rowdiag_plan_create(const long long *segptr_host, long long nseg, const long long *off_host, const int *p_host,
                                  const int *q_host, long long nvals);
    void rowdiag_plan_apply(long long id, const double *values_host, double *out_host);
    void rowdiag_plan_free(long long id);
    void copy_factor(double *out_host);
    // dense-operator leg of the Kronecker path (dense.hip): R = D T, all row-major device arrays; dst = src' (rows x cols)
    void dense_apply(const double *d_D, const double *d_T, double *d_R, long long n1, long long n2);
    void transpose(const double *d_src, double *d_dst, long long rows, long long cols);
    long long fail_col();
    // ---- linear equality constraints (device_constraint.cpp, constraint.hip) ------------------------------------------------------
    // con_set uploads A / e (m = 0: none) and drops everything derived. con_prepare (lazy, once per factorisation) builds
    // At = Q^-1 A' (scatter + ONE blocked solve), W = A At, L_c, L_c^-1 (host, m <= 64) and B = At L_c^-T; false = W is not positive definite.
    void con_set(const ConHost &c);
    int con_m() const { return con_.m; }
    bool con_prepare();
    double con_logdet_w() const { return con_.logdet_w; }
    double con_ms() const { return con_.ms; }
    void con_get(double *At_host, long long ld, double *W_host);
    // X <- X (+ mu) - At W^-1 (A (X + mu) - e) on nvec columns of a device array (d_mu nullable); without constraints X += mu
    void con_correct(double *d_X, long long ldx, long long nvec, const double *d_mu, bool homogeneous = false);      // homogeneous: e = 0
    double ms_con_correct = 0;         // GPU time of the kernels of the most recent con_correct
    // A mu - e of the most recent con_correct (its first column), host copy of m values
    void con_residual(double *out_host);
    const std::vector<double> &con_linv() const { return con_.h_linv; }
    // max(diag Sigma - rowsum(B^2), 0) (selected inverse computed if absent); without constraints = selinv_diag
    void con_var(double *out_host);
    // ---- the same for every member of a batched handle (gmrfx_batch_constraints_*): ONE A and e, everything derived per member ----
    // Member k's At_k = Q_k^-1 A' and B_k = At_k L_ck^-T: n_member x m column-major blocks at + k n_member m; W_k (m x m, column-
    // major) and L_ck^-1 (row-major) at + k m m. bcon_set builds the new state aside and throws std::bad_alloc, with nothing
    // changed, when the two operand arrays do not fit. bcon_prepare (lazy, once per factorisation): memset + scatter of A' into all
    // blocks, ONE member-strided forest solve of m columns, W_k by the chunked reduction, k_batch_con_chol (no download of W, no
    // host loop), B_k; false = W_k is not positive definite for a member whose factorisation succeeded (bcon_cinfo: 0, 1 + the
    // failing pivot, or -1 for a member whose factorisation failed -- its operands are NaN, nobody else's are touched).
    void bcon_set(const ConHost &c);
    int bcon_m() const { return bcon_.m; }
    bool bcon_prepare();
    // the same refresh, handing back cinfo per member instead of folding it into one answer (the lockstep loop stops members alone)
    const std::vector<long long> &bcon_prepare_members() { bcon_prepare(); return bcon_.h_cinfo; }
    // S_k <- S_k - At_k W_k^-1 (A S_k) for the members whose byte in d_active (nbatch bytes on the device, nullable = all) is set:
    // the one-column, e = 0 case of bcon_correct on the operands bcon_prepare left, S_k = d_S + k stride. Enqueues only: the
    // caller's next synchronisation covers it. A member whose W_k failed must be masked out (its L_ck^-1 is NaN).
    void bcon_project(double *d_S, long long stride, const unsigned char *d_active);
    // out_host[k] = max_r |(A x_k - e)_r|, x_k = d_x + k sx, for the members whose byte in d_active is set (the others: left)
    void bcon_residual(const double *d_x, long long sx, const unsigned char *d_active, const unsigned char *active_host, double *out_host);
    const std::vector<double> &bcon_logdet_w() const { return bcon_.h_logdet; }
    const std::vector<long long> &bcon_cinfo() const { return bcon_.h_cinfo; }
    double bcon_ms() const { return bcon_.ms; }
    void bcon_get(int member, double *At_host, long long ld, double *W_host);
    // member k's n_member x nvec block at d_X + k sx (leading dimension ldx), d_mu: n_member x nbatch (nullable)
    void bcon_correct(double *d_X, long long ldx, long long sx, long long nvec, const double *d_mu);
    // quad[k] = r_k' W_k^-1 r_k = |L_ck^-1 r_k|^2, r_k = A x_k - e, x_k = d_x + k n_member (d_x null: zero); host array of nbatch
    void bcon_quad(const double *d_x, double *quad_host);
    void bcon_var(double *out_host);       // n_member x nbatch

    // ---- Rao-Blackwellised Monte Carlo marginal variances (device_rbmc.cpp, rbmc.hip; gmrfx_rbmc_var) --------------------------------
    // plan = nullptr: RBMCStrategy, else BlockRBMCStrategy on that plan. Z: n x k column-major standard normals (host or device),
    // processed in blocks of kRbmcW columns: backward sweep -> transpose -> estimator kernels, per-row (mean, M2) merged block by
    // block; device memory O(n kRbmcW) for any k. d_nz = Q's values on the device (nullptr: the held values). out: n doubles.
    void rbmc_var(const RbmcSym &sym, const RbmcPlan *plan, const double *d_nz, const double *Z, long long ldz, bool z_on_device, long long k,
                  double *out, bool out_on_device);
    double ms_rbmc = 0, ms_rbmc_bsolve = 0;      // GPU time of the most recent rbmc_var, and the backward sweeps' part of it

    // ---- log-density gradients on Q's own pattern (device_grad.cpp, grad.hip; gmrfx_logpdf_grad, gmrfx_pattern_dot) -----------------
    // Members: the handle's batch (a handle without batch buffers is one member of S.n nodes). Device operands: nz = Q's values
    // (nnz per member; nullptr: the held values; only read for mubar), z at + k sz, mu n per member (nullable), Qbar nnz per member and
    // mubar n per member (either nullable: not computed); ybar: host, one per member. With a constraint set (con_* or bcon_*, A = its
    // host rows) the outputs are the gradient of logpdf + log_correction. Ensures the selected inverse (Qbar) and the constraint
    // preparation, enqueues the kernels on the main stream and synchronises once. info_host[k] (nullable): 0, -1 when member k's
    // factorisation failed, 1 + the failing pivot when its W did -- such a member's outputs are NaN, nobody else's are touched.
    struct GradIO { const double *d_nz, *d_z; long long sz; const double *d_mu; const double *ybar_host; double *d_Qbar, *d_mubar; };
    void logpdf_grad(const RbmcSym &sym, const ConHost *A, const GradIO &io, long long *info_host);
    // out[k p + c] = sum_e w_e G[k nnz + e] J[k sj + c ldj + e], w_e the weights of the quadratic form; out: host, p per member
    void pattern_dot(const double *d_G, const double *d_J, long long ldj, long long sj, long long p, double *out_host);

    // ---- Fisher scoring on the device (device_fisher.cpp, fisher.hip; gmrfx_obs_set, gmrfx_fisher_eval) ------------------------------
    // obs_set expands y, aux and the observed mask to length-n arrays on the device (nobs = 0: drops them), built aside: a failed
    // upload leaves the previous likelihood in place.
    void obs_set(const ObsHost &o);
    // the parameters of the composite in place replaced (gmrfx_obs_composite_set_param): C.param and the new total constant
    void obs_composite_set_param(const ObsComponents &C, double loglik_const);
    bool obs_held() const { return (bool)fisher_.y; }
    // entries of the Hessian vector of fisher_eval / gaussian_approximation: n in node form, the map's cnt in design form
    long long hess_len() const { return fisher_.design ? fisher_.design->cnt : S_->n; }
    // One pass over Symmetric(Q_prior) at the point d_x: score = (Q_p x - h) - g(x) and hess = d(x) (n each, device, either nullable),
    // out_host = {1/2 x' Q_p x - x' h, sum of the x-dependent terms of loglik}; h = Q_p mu (d_mu nullable: 0). Needs set_prior with the
    // diagonal map (position of (i, i) for every i) and a likelihood; no factorisation. Synchronises once.
    // Design form (device_fisher.cpp, fisher_design.hip): eta = A x + b, score = (Q_p x - h) - A' g(eta), d_hess = the hess_len() values
    // sum_t w_t d(eta_{i_t}) of A' D A in map order; needs set_prior with exactly the map of the plan.
    void fisher_eval(const RbmcSym &sym, const double *d_x, const double *d_mu, double *d_score, double *d_hess, double *out_host);
    // The Fisher-scoring loop of the reference (src/workspace/gaussian_approximation.jl:230-313), control flow on the host, every vector
    // in HBM; its decisions (_ga_line_search, _predict_converged, _frozen_finish) are the functions of ga_rules.h, GaOpts with its flags too.
    // d_x0 nullable (= mu, or 0); d_x: n out; d_hess: n out, nullable. result[8], dec_trace / alpha_trace (max_iter + 1, nullable): host.
    // Returns 0, 1 when a factorisation failed (*info = 1 + the failing step; d_x = the last accepted iterate), 2 when the
    // constraint's W = A Q^-1 A' did.
    using GaOpts = gmrfx::GaOpts;
    int gaussian_approximation(const RbmcSym &sym, const double *d_mu, const double *d_x0, const GaOpts &o, double *d_x, double *d_hess,
                               double *result, double *dec_trace, double *alpha_trace, long long *info);

    // ---- the same for every member of a batched handle (device_batch_fisher.cpp, fisher.hip; gmrfx_batch_obs_set,
    // gmrfx_batch_obs_set_design, gmrfx_batch_fisher_eval, gmrfx_batch_gaussian_approximation). Node or design form, no constraints. The
    // prior's values and the Hessian map are those of set_prior on the forest (gmrfx_batch_set_prior builds the map).
    void bobs_set(const RbmcSym &sym, const BObsHost &o);
    bool bobs_held() const { return (bool)bfisher_.y; }
    // entries of a member's Hessian vector: n_member in node form, the plan's cnt in design form
    long long bhess_len() const { return bfisher_.design ? bfisher_.design->cnt : nmember_; }
    // set_prior on the forest with the map of the batch likelihood in place: the forest's diagonal (no likelihood, node form), or the
    // member's plan map shifted by k nnz_member for k = 0 .. nbatch - 1 (design form); map: the forest's, as the caller built it
    void bset_prior(const double *prior_nzval, const std::vector<long long> &map, bool design);
    // Member k's evaluation at d_x + k sx with the mean d_mu + k smu (nullable; smu = 0: one mean): score at + k ss, hess (bhess_len()
    // entries) at + k sh (either nullable), out_host[2 k ..] = {energy, loglik}. active (host, nbatch bytes, nullable = all): a member
    // whose byte is 0 is skipped and nothing of it is written, on the device or in out_host. One synchronisation.
    struct BEvalIO { const double *d_x; long long sx; const double *d_mu; long long smu; const unsigned char *active; double *d_score, *d_hess; long long ss, sh; };
    void batch_fisher_eval(const BEvalIO &io, double *out_host);
    // The loop of gaussian_approximation for all members in lockstep: one forest-wide launch per step, member k seeing exactly the
    // sequence of operations its own plain loop would perform. d_x0 nullable (= mu, or 0). result: host, 10 per member (the plain
    // call's eight, then energy and loglik at the member's x); totals: host, 3 (forest factorisations, solves, evaluations launched);
    // dec_trace / alpha_trace: host, (max_iter + 1) per member, nullable; info: host, one per member. Returns 0, or 1 when a member's
    // factorisation failed (info[k] = 1 + its failing step, its x = its last accepted iterate, everybody else complete).
    struct BGaIO { const double *d_mu; long long smu; const double *d_x0; long long sx0; double *d_x; long long sx; double *d_hess; long long sh; };
    // With a batch constraint held (bcon_m() > 0) every step is projected as the plain loop projects it: bcon_prepare + bcon_project
    // after the refactorize_update_solve of every iterate (masked to the running members) and bcon_project after each chord solve of
    // the frozen finish (masked to the firing members, same factor, no re-preparation). cinfo (host, nbatch, nullable): 0, 1 + the
    // failing pivot of W_k (that member stops alone, its x its last accepted iterate), -1 beside a failed factorisation; residual
    // (host, nbatch, nullable): max_r |(A x_k - e)_r| of the members that did not fail (NaN for the others). Bit 1 of the return
    // value: some member's W_k failed.
    int batch_gaussian_approximation(const BGaIO &io, const GaOpts &o, double *result, double *totals, double *dec_trace, double *alpha_trace,
                                     long long *info, long long *cinfo = nullptr, double *residual = nullptr);
    // the members' likelihood parameters replaced in place (gmrfx_batch_obs_set_param): param and loglik_const, nbatch each
    void bobs_set_param(const std::vector<double> &param, const std::vector<double> &loglik_const);

    // The pullback of gaussian_approximation at its mode d_x (device_ga_pullback.cpp, ga_pullback.hip; gmrfx_ga_pullback): from the
    // cotangents of the mode (d_mubar, n) and of the posterior precision (d_Qbar, nnz on the pattern), either nullable, those of the
    // prior's precision (d_Qbar_prior, nnz; may be d_Qbar itself) and mean (d_mubar_prior, n), lam = Q_post^-1 xbar (d_lambda, n), each
    // nullable, and out_host = {parameter cotangent, lam' xbar}. flags: bit 0 projects lam with the constraint set (e = 0), bit 1
    // refactorises at Q_prior - H(d_x) first; without it the handle's factor is taken to be that one. Returns 0, 1 when that
    // factorisation failed (*info = 1 + the failing step), 2 when the constraint's W did.
    struct GapIO { const double *d_x, *d_mu, *d_mubar, *d_Qbar; int flags; double *d_Qbar_prior, *d_mubar_prior, *d_lambda; };
    int ga_pullback(const RbmcSym &sym, const GapIO &io, double *out_host, long long *info);
    // The same for a composite likelihood (gmrfx_ga_pullback_composite): param_bar_host gets one parameter cotangent per component
    // (0.0 for a component whose family has no parameter), *check_host (nullable) lam' xbar. The unchanged kernels, the solve and the
    // projection are launched as ga_pullback launches them; k_gap_point_comp, k_gap_param_comp and k_gap_final_comp take the place
    // of the three that read a family.
    int ga_pullback_composite(const RbmcSym &sym, const GapIO &io, double *param_bar_host, double *check_host, long long *info);
    // The same for every member of a batched handle (gmrfx_batch_ga_pullback), forest-wide, one launch per step: member k's mode at
    // d_x + k sx, prior mean at d_mu + k smu (nullable; smu = 0: one mean), cotangents and outputs dense per member (n / nnz_member
    // each). Needs the batch likelihood and the prior of gmrfx_batch_set_prior. Bit 0 projects with the BATCH constraint (a held
    // constraint without the bit: the plain solve); bit 1 evaluates every member's Hessian at its x and refactorises the forest first.
    // out_host: 2 per member; info_host (nbatch, nullable): 0, -1 when member k's factorisation failed, 1 + the failing pivot when its
    // W_k did -- such a member is masked out of every launch, its requested output slices and its two results are NaN, nobody
    // else's are touched. Returns 0, or 1 when some member failed. One synchronisation behind the last launch.
    struct BGapIO { const double *d_x; long long sx; const double *d_mu; long long smu; const double *d_mubar, *d_Qbar; int flags;
                    double *d_Qbar_prior, *d_mubar_prior, *d_lambda; };
    int batch_ga_pullback(const RbmcSym &sym, const BGapIO &io, double *out_host, long long *info_host);

    // ---- the linear predictor's marginals and the predictive scores (device_predictive.cpp, predictive.hip) -------------------------
    // Per observation, in the caller's order (the indices of gmrfx_obs_set / the rows of A): the mean of the linear predictor at d_x
    // (n), its variance under the handle's factorisation (the selected inverse is computed if absent) and the full log density at
    // the mean; device arrays of nobs, each nullable. flags bit 0: subtract the constraint's correction and clamp at 0. o: the
    // handle's host copy of the likelihood (the observation order and the constants go up on the first call after obs_set).
    // Returns 0, or 2 when the constraint's W is not positive definite (nothing written).
    struct PredIO { const double *d_x; int flags; double *d_mu_eta, *d_v_eta, *d_pll; };
    int predictor_marginals(const RbmcSym &sym, const ObsHost &o, const PredIO &io);
    // The quadrature scores over N(d_mu[i], d_v[i]) (device, nobs each) with K nodes z and weights w of the standard normal (host):
    // lpd, lcpo, elp, vlp per observation (device, each nullable) and their totals out4_host, computed either way.
    struct ScoreIO { const double *d_mu, *d_v; int K; const double *z, *w; double *d_lpd, *d_lcpo, *d_elp, *d_vlp; };
    void predictive_scores(const ObsHost &o, const ScoreIO &io, double *out4_host);
    // The same for every member of a batched handle (gmrfx_batch_predictor_marginals, gmrfx_batch_predictive_scores), forest-wide, one
    // launch per step: member k's mean at d_x + k sx, outputs dense per member (nobs each, member stride nobs). Needs the batch
    // likelihood; the variance needs the forest's factorisation (the selected inverse is computed if absent). Bit 0 subtracts the
    // BATCH constraint's correction per member and clamps (a held constraint without the bit is ignored). info_host (nbatch): 0, -1
    // when member k's factorisation failed, 1 + the failing pivot when its W_k did (bit 0) -- such a member is masked out of every
    // launch and gets NaN in its requested slices, nobody else's are touched; without d_v_eta no factor is looked at and nobody is
    // masked. Returns 0, or 1 when some member failed. One synchronisation behind the last launch.
    struct BPredIO { const double *d_x; long long sx; int flags; double *d_mu_eta, *d_v_eta, *d_pll; };
    int batch_predictor_marginals(const RbmcSym &sym, const BObsHost &o, const BPredIO &io, long long *info_host);
    // d_mu / d_v and the four outputs: nobs x nbatch; out_host: 4 per member. A member whose factorisation failed (when the handle
    // holds one) is masked as above: info_host[k] = -1, NaN in its slices and totals.
    int batch_predictive_scores(const BObsHost &o, const ScoreIO &io, double *out_host, long long *info_host);
    // The mixture of the members' predictive distributions (gmrfx_batch_predictive_mixture; k_pred_mixture): w = nbatch weights omega_k,
    // then nbatch logs of them (-inf: the member is never read), as the C ABI rounded them; d_mu, d_v, d_lpd (nullable): nobs x nbatch;
    // the three outputs nobs each, nullable; *out_host = the sum of mix_lpd (NaN without d_lpd).
    struct MixIO { const double *d_mu, *d_v, *d_lpd; double *d_mix_mu, *d_mix_v, *d_mix_lpd; };
    void batch_predictive_mixture(const BObsHost &o, const std::vector<double> &w, const MixIO &io, double *out_host);

    bool factorized = false, selinv_valid = false;
    bool inverse_pending = false;   // dense inverses of the big fronts are computed lazily, on a side stream
    double ms_factor = 0, ms_solve = 0, ms_fwd = 0, ms_bwd = 0, ms_perm = 0, ms_bsolve = 0, ms_logdet = 0, ms_selinv = 0;
    long long last_nrhs = 0;
    double ms_quadform = 0;
    double ms_inv_decide = 0;      // host wall time of the one-time inverse-cap decision (decide_inverse_cap), 0 before / without it
    int inv_cap() const { return inv_cap_; }
    bool syrk_times_pending_ = false;
    double syrk_ms();                 // summed device time of the SYRK launches of the last factorisation (read lazily)
    double ms_syrk = 0, syrk_flops = 0;   // dominant kernel (k_syrk_cb): device wall-clock stamps of its own workgroups per refactorisation, flops
    long long syrk_launches = 0;
    double bytes_total = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    Stream own_stream_;                  // the main stream this handle created (`stream` may be the caller's: set_external_stream)
    bool async_phases_ = false;          // sharded phase entry points return after enqueueing (no host synchronisation, no timings)
    Stream stream2;                 // side stream: dense-inverse stages overlap the leaf levels of the forward sweep
    Stream stream3;                 // second sweep lane (solves with more than 64 right-hand sides)

private:
    void upload(const Symbolic &S);
    void ensure_rhs_capacity(long long nrhs);
    // record_level_events: the pipelined call's "level is factored" events (ev_flevel_) behind every level
    void factor_levels(int lo, int hi, bool record_level_events);
    // the three parts of a level (device.cpp, above factor_levels); factor_small_fronts returns whether the third stream took part
    struct PanelChain;
    bool factor_small_fronts(const LevelInfo &L);
    bool factor_panel_chains(const LevelInfo &L);       // returns whether there were two chains (joined behind the last block)
    void panel_block(const PanelChain &ch, const LevelInfo &L, int b);
    void factor_contribution_blocks(const LevelInfo &L, int slot);
    SweepKnobs sweep_knobs() const;
    // follows_factor: the pipelined call's forward sweep, one level behind the factorisation (waits for the level events, builds the
    // dense inverses level by level)
    void forward(const SweepLane &ln, int nr, int ldx, int lo, int hi, bool follows_factor);
    void backward(const SweepLane &ln, int nr, int ldx, bool y_in_x2, int hi, int lo);
    // one pass of a solve on lane ln: transpose in, forward (mode 0), backward, transpose out; ev (nullable): the lane's five timing events
    void sweep_pass(const SweepLane &ln, const Event *ev, const double *dB, long long ldin, double *dXo, long long ldout, int nr, int mode,
                    const MemberLayout *ml);
    // lane 0: the main stream and d_X_ / d_X2_ / d_W_; lane 1: the third stream and their twins (solves of more than 64 right-hand sides)
    SweepLane lane(int k) const { return k == 0 ? SweepLane{stream, d_X_, d_X2_, d_W_} : SweepLane{stream3, d_Xb_, d_X2b_, d_Wb_}; }
    // the three parts every numeric factorisation shares (device.cpp, above refactorize)
    void begin_factor(const double *d_src);
    void enqueue_factor_tail();
    void finish_factor();
    void newton_values(const double *h, bool on_device);
    void ensure_io(long long need);
    void read_batch_diag(double *logdet_out, long long *info_out) const;
    // Members are destroyed in reverse order of declaration: the streams (own_stream_, stream2, stream3 above, stream_io_ here) are
    // declared before every buffer and event of the handle, so that those are released first and the streams last.
    Stream stream_io_;                // copy stream of the pipelined call's host I/O
    // The events by their uses (all in device.cpp):
    //   stream-to-stream hand-offs, only ever the argument of hipStreamWaitEvent on this device: ev_fact_, ev_inv_, ev_ready_,
    //                 ev_ready2_, ev_done1_, ev_nzp0_, ev_nzp_, ev_flevel_[*]
    //   host-waited:  ev_logdet_, ev_ring_[*], ev_bdiag_ (hipEventSynchronize); ev_up_, ev_x_, ev_qf_ (they order copies to / from
    //                 host memory that the host reads or reuses behind them)
    //   times read:   ev_[*], ev_lane_[*][*] (some of them are waited for by a stream as well), ev_level_[*] (GMRFX_LEVEL_MARK),
    //                 con_ev_, bcon_ev_, rb_ev_: default flags
    // The constraint, Fisher, RBMC and selected-inversion paths fork no stream of their own. MEASURED and not adopted (DESIGN.md
    // section 5, "SYRK times from device stamps"): the hand-offs created with hipEventDisableTiming | hipEventReleaseToDevice
    // (a device-scope release instead of the system-scope one) -- the step within its run-to-run spread either way; they stay
    // hipEventDisableTiming alone.
    Event ev_fact_, ev_inv_;
    // the arena of the tables that live as long as the handle (append-only, released by the destructor)
    template <class T> T *dalloc(size_t count);
    std::vector<void *> allocs_;

    const Symbolic *S_ = nullptr;
    const SelRec *d_selrec_ = nullptr;    // one per supernode
    DevSym ds_{};
    std::vector<LevelInfo> levels_;
    std::vector<LevelInfo> swlevels_;   // the sweeps' level schedule: levels_ without the fronts of the sweep tasks
    int *d_sw_levellist_ = nullptr;
    SweepTask *d_swt_ = nullptr;
    int nswt_ = 0;
    const unsigned char *d_owncol_ = nullptr;   // sharded handles: 1 for the columns of the fronts this rank factors
    const long long *d_zbptr_ = nullptr;   // arena offsets of the trailing inverse blocks (Symbolic::zbptr)
    const int *d_iperm_ = nullptr;   // inverse permutation (original row -> position), used by the RHS transposes
    int *d_levellist_ = nullptr;
    FwdTile *d_fwd_recs_ = nullptr;     // one record per 32-row tile of every big front's update vector (sweep levels)
    double *d_nzp_ = nullptr;           // Q's values in assembly order (nzp[q] = nzval[qsrc[q]]): gathered once per factorisation, one dependent load less per panel column
    long long nq_ = 0;
    Event ev_nzp_, ev_nzp0_;
    AsmRec *d_arec_ = nullptr;          // one per position of the level lists (Symbolic::levellist order)
    SyrkTile *d_syrk_recs_ = nullptr;   // one record per contribution-block tile, level by level, in hand-out order
    unsigned long long *d_syrk_times_ = nullptr;        // two device wall-clock words per record: the tile's start and end (k_syrk_cb_rec)
    SyrkLevelTimes *d_syrk_level_times_ = nullptr;      // one per level: its records and its SYRK slot (k_syrk_reduce)
    EnvKnobs env_;                  // the environment's knobs (device_plan.h), read by init
    FrontView *d_frec_ = nullptr, *d_frec2_ = nullptr, *d_sel_frec_ = nullptr;   // geometry records parallel to the level lists
    int *d_levellist2_ = nullptr;   // per level: the big fronts re-ordered [even positions..., odd positions...] (two-stream panel chains)
    // wave tasks (sweep_wave.hip): task ids by LDS class (kWaveRows, device_plan.h)
    const int *d_wave_order_ = nullptr;
    int wave_first_[kWaveClasses] = {0, 0}, wave_count_[kWaveClasses] = {0, 0};
    void sweep_tasks(const SweepLane &ln, int phase, int nr, int ldx, bool follows_factor);
public:
    void set_external_stream(hipStream_t s, bool use, bool async);
    int level_times(int phase, double *out, int cap);
    void dist_front_phase(const double *d_nzval, int front, int what, int block);
private:
    void ensure_rdiag(hipStream_t st);
    bool nzp_pending_ = false;                    // k_gather_values runs on the third stream and the main stream has not waited for it yet
    void ensure_dtile(hipStream_t st);
    Symbolic::SwChunk *d_swc_fwd_ = nullptr, *d_swc_bwd_ = nullptr;   // chunk records of the sweep tasks (forward order / backward slot programs)
    int *d_swc_listf_ = nullptr, *d_swc_listb_ = nullptr;               // their target rows as LDS byte offsets, in the lane order of the two kernels
    double *d_dtile_ = nullptr;                   // inverse diagonal blocks of the chunks, packed (k_pack_diag): 256 doubles per chunk
    int nswc_ = 0;
    unsigned long long dtile_for_ = 0;            // d_dtile_ belongs to factorisation number dtile_for_
    double *d_rdiag_ = nullptr;                   // n reciprocals of L's diagonal (+ a zero word): operands of the wave tasks
    unsigned long long factor_serial_ = 1, rdiag_for_ = 0;    // d_rdiag_ belongs to factorisation number rdiag_for_
    std::vector<int> sel_max_cols_, sel_max_trail_;   // per level, over the big fronts of the selected-inversion list
    int *d_dist_list_ = nullptr;  // the distributed fronts (Symbolic::dist_fronts) as a device list for the assembly / SYRK kernels
    bool selinv_begun_ = false;   // sharded selected inversion: phase 0 has run since the last refactorisation (gmrfx_selinv_phase)
    std::vector<Event> ev_level_[3];
    int level_slots_[3] = {0, 0, 0};
    void level_event(hipStream_t st, int phase, int slot);
    int *d_sub_first_ = nullptr, *d_sub_last_ = nullptr, *d_sel_levellist_ = nullptr;
    int nsub_cls_[3] = {0, 0, 0};
    double *d_L_ = nullptr, *d_Z_ = nullptr, *d_cb_ = nullptr, *d_nz_ = nullptr;
    const double *nz_src_ = nullptr;
    double *d_prior_ = nullptr;
    DevBuf<double> d_h_;
    DevBuf<long long> d_hmap_;
    long long hmap_cnt_ = 0, hmap_cap_ = 0;   // values of the refactorisation in flight (d_nz_ or the caller's device buffer)
    double *d_X_ = nullptr, *d_X2_ = nullptr, *d_W_ = nullptr, *d_part_ = nullptr;
    DevBuf<double> d_io_, d_tmp_;
    // dense-inverse stages (inverse.hip)
    int *d_invlist_ = nullptr;
    std::vector<int> inv_nact_;            // per stage: fronts with more than 64<<stage columns
    std::vector<long long *> d_inv_toff_;   // per stage: offsets of the T buffers
    double *d_invT_ = nullptr;
    int inv_maxc_ = 0;
    // Recursive doubling of the diagonal-block inverses stops at inv_cap_ columns (a full inverse of a c-column
    // front costs O(c^3): most of a 3-D solve); wider fronts substitute block by block in the sweeps. The selected
    // inversion needs the full inverses and runs the remaining stages on demand (B from inv_cap_ up).
    int inv_cap_ = EnvKnobs{}.inv_cap;     // 2048, measured: cfg 2 flat between 1024 and 4096 (6.18 vs 6.26 ms), 3-D 100^3 solve 44 vs 54 ms
    // An explicit inverse of an ill-conditioned L11 is not backward stable (inverse.hip, "Conditioning"): the handle's first
    // successful factorisation measures the pivot growth max_j sqrt(A11_jj) / L_jj of every front wider than NB, and above
    // kInvGrowthMax the cap drops to NB for the rest of the handle's life. One cap per handle, decided before any sweep runs
    // (refactorize_solve takes the plain sequence until then), keeps the pipelined and the separate calls bit-identical; the
    // measure is the same bits for D Q D (D of powers of two) as for Q, so both take the same path. Sharded handles never
    // decide (their fronts are spread over ranks): they keep the cap they were created with. Costs one pass over the
    // lower triangles of those fronts, O(c^2) each, and one synchronisation, once per handle (stats: ms_inv_decide; measured
    // 2.5 ms on the 1000 x 1000 2-D benchmark mesh, 14 ms on a 100^3 3-D grid whose top front has 30 000 columns).
    static constexpr double kInvGrowthMax = 1e4;
    bool inv_cap_decided_ = false;
    double *d_pivgrowth_ = nullptr;
    void decide_inverse_cap();
    bool inverse_full_ = false;
    // pipelined factor + solve: per-level "level is factored" events, the dense-inverse stages per level, the highest level a
    // sweep task / small subtree reaches
    std::vector<Event> ev_flevel_;
    int bottom_top_level_ = 0, fused_gate_level_ = 0;
    int *d_inv_lvl_list_ = nullptr;
    std::vector<int> inv_lvl_first_, inv_lvl_maxc_;
    std::vector<std::vector<int>> inv_lvl_nact_;              // [level][stage]
    std::vector<long long *> d_inv_lvl_toff_;                  // per stage: offsets into d_invT_, aligned with d_inv_lvl_list_
    void invert_level(hipStream_t st, int lev);
    bool fact_event_valid_ = false;   // ev_fact_ was recorded at the end of the last factorisation
    // the pivot report of the last factorisation, then its SYRK stamps: kInfoWords ints (the pivot word + padding to 8 bytes), then
    // per SYRK slot two 64-bit device wall-clock values (earliest start, latest end). d_info_ has the same layout; one copy brings both.
    static constexpr int kInfoWords = 2;
    PinnedBuf<int> h_info_;
    static unsigned long long *syrk_stamps(int *info) { return reinterpret_cast<unsigned long long *>(info + kInfoWords); }
    static size_t info_bytes(long long slots) { return kInfoWords * sizeof(int) + 2 * (size_t)slots * sizeof(unsigned long long); }
    double wall_clock_khz_ = 0;       // hipDeviceAttributeWallClockRate: ticks per millisecond of the stamps
    PinnedBuf<double> h_qf_;          // quadratic forms of refactorize_logpdf
    Event ev_qf_;
    void prepare_quadform(long long nvec);
    PinnedBuf<double> h_logdet_;      // log det of factorisation logdet_for_ (valid once ev_logdet_ has passed)
    unsigned long long logdet_for_ = 0;
    Event ev_logdet_;
    void enqueue_logdet(hipStream_t st, bool timed);
    bool info_cached_ = false;
    void invert_diag_blocks(hipStream_t st, int b_from, int b_to);
    void start_inverse_async();
    void wait_inverse(hipStream_t st);
    int first_multiblock_level_ = 0;
    long long rhs_cap_ = 0, io_cap_ = 0, tmp_cap_ = 0;
    long long *d_yoff_ = nullptr;                 // selected inversion: per-front offsets of the Yh / Yt workspaces
    int *d_fchild_ = nullptr;                     // sharded: other ranks' children of this rank's fronts, by level
    std::vector<int> fc_levelptr_, fc_maxtrail_;  // ranges of d_fchild_ per level, max trailing rows per level
    void selinv_begin();
    void selinv_levels(int hi, int lo);
    // Solves with more than 64 right-hand sides run their 64-column passes on TWO lanes (SweepLane: stream + buffers each):
    // one pass is launch-latency bound (4.6 ms for 1 column, 5.9 for 64), two interleave on the idle CUs.
    double *d_Xb_ = nullptr, *d_X2b_ = nullptr, *d_Wb_ = nullptr;   // lane 1 (lane 0 = d_X_ / d_X2_ / d_W_ on `stream`): lane()
    Event ev_lane_[2][5];
    Event ev_ready_, ev_ready2_, ev_done1_;
    int *d_info_ = nullptr;
    // host I/O of the pipelined factor + solve call (copy stream: stream_io_): page-locked staging buffers, events
    PinnedBuf<double> h_stage_, h_nzstage_;
    void host_upload_values(const double *nzval);
    Event ev_up_, ev_x_;
    std::vector<Event> ev_ring_;                  // one per slot of the page-locked staging ring (host_upload / host_download)
    void host_io_reserve(long long count);
    void host_upload(const double *B, long long ldb, long long nrhs, double *d_dst);
    void host_download(const double *d_src, long long nrhs, double *X, long long ldx, hipStream_t after);
    struct RowDiagPlan { long long nseg = 0, cnt = 0, nvals = 0; DevBuf<long long> seg, off; DevBuf<int> p, q; DevBuf<double> vals, out; };     // (not on the handle's books)
    std::vector<RowDiagPlan> rd_plans_;
    // caller's CSC pattern, uploaded on the first quadform call
    long long *d_in_colptr_ = nullptr;
    int *d_in_row_ = nullptr;
    DevBuf<double> d_qf_part_, d_qf_out_;
    long long qf_cap_ = 0;
    bool nz_held_ = false;    // d_nz_ holds the values of the factorisation
    Event ev_[8];
    long long l_size_ = 0, sum_trail_ = 0;
    // batched handles (set_batch): members, member size / values; device partials + results of batch_diag / batch_quadform, pinned copies
    int nbatch_ = 1;
    long long nmember_ = 0, nnz_member_ = 0;
    double *d_bpsum_ = nullptr, *d_bdiag_ = nullptr;
    PinnedBuf<double> h_bdiag_;                   // d_bdiag_ / h_bdiag_: nbatch log dets, then nbatch info words
    int *d_bpbad_ = nullptr;
    unsigned long long bdiag_for_ = 0;            // h_bdiag_ belongs to factorisation number bdiag_for_
    Event ev_bdiag_;
    long long *d_bin_colptr_ = nullptr;           // the MEMBER's pattern (the forest's first n_member columns)
    int *d_bin_row_ = nullptr;
    DevBuf<double> d_bqf_part_, d_bqf_out_;
    PinnedBuf<double> h_bqf_;
    long long bqf_cap_ = 0;
    void enqueue_batch_diag(hipStream_t st);
    // what con_set / bcon_set keep of A itself: the CSR rows and e on the device, the chunk offsets of the reduction and its buffers
    // (R: m x colcap, part: totchunks x colcap, per member)
    struct ConRows {
        int m = 0, maxchunks = 0;
        long long nnz = 0, maxlen = 0, totchunks = 0, colcap = 0;
        DevBuf<long long> rowptr;
        DevBuf<int> col, choff;
        DevBuf<double> val, e, R, part;
    };
    ConRows con_rows_upload(const ConHost &c);
    void con_reserve_cols(ConRows &a, long long cols, int members);
    // constraint state: A, the cached operands of factorisation serial. The events outlive the state: a new A replaces the state only.
    struct ConDev : ConRows {
        DevBuf<double> At, B, Linv, amu, sig;
        std::vector<double> h_w, h_linv;
        double logdet_w = 0, ms = 0;
        unsigned long long serial = 0;      // 0: nothing cached
    } con_;
    struct BConDev : ConRows {
        long long piece = 0;
        DevBuf<long long> cinfo;
        DevBuf<double> At, B, W, Linv, amu, sig, stat;      // stat: nbatch log det W, then nbatch |L_c^-1 r|^2
        std::vector<double> h_logdet;
        std::vector<long long> h_cinfo;
        double ms = 0;
        bool ok = false;
        unsigned long long serial = 0;      // 0: nothing cached
    } bcon_;
    Event con_ev_[2], bcon_ev_[2], rb_ev_[2];     // begin / end of the timed part of con_*, bcon_*, rbmc_var
    // the symmetric row structure of Q (RbmcSym) on the device, uploaded once per handle: shared by rbmc_var and logpdf_grad
    struct SymRowsDev {
        DevBuf<long long> rp;
        DevBuf<int> col, pos, dpos;
    } sym_rows_;
    void sym_rows_upload(const RbmcSym &sym);
    // RBMC state: the work arrays (allocated once), the tables of the current block plan
    struct RbmcSymDev {
        DevBuf<double> Xc, Xt, mean, m2, base, out;
    };
    struct RbmcPlanDev {
        DevBuf<long long> bptr, eptr;
        DevBuf<int> rows, ns, loc, order[kRbmcClasses];
        DevBuf<unsigned char> owner;
        int cnt[kRbmcClasses] = {};
        DevBuf<double> scrM, scrR;
        int enclosure = -2;
        unsigned long long serial = 0;
    };
    struct RbmcState { RbmcSymDev sym; RbmcPlanDev plan; } rb_;
    void rbmc_upload_sym(const RbmcSym &sym);
    void rbmc_upload_plan(const RbmcPlan &plan);
    // gradient state. Tables of the handle's life: zoff (offset of every stored entry of Q in the selected-inverse panels; all members),
    // wgt (the member's quadratic-form weights, one byte per entry). Bt = B' per member, of factorisation bt_serial and the constraint
    // set then, and acol* (A by columns): con_set / bcon_set drop both. Work arrays, allocated once: r, u (n per member), tw (2 x 64), R (64),
    // zero (a zero mean), ybar and the bad words, the contraction's partial sums and results.
    struct GradDev {
        DevBuf<long long> zoff, acolptr, bad;
        DevBuf<unsigned char> wgt;
        DevBuf<int> arow;
        DevBuf<double> aval, Bt, r, u, tw, R, ybar, zero, dpart, dout;
        long long dot_cap = 0, out_cap = 0;
        unsigned long long bt_serial = 0;       // 0: nothing cached
    } grad_;
    // design form, what a plain and a batched likelihood hold alike (design_upload): the plan, its tables as they are, and the chunk
    // tables of the long columns and term lists (choff: prefix sums of chunk counts; chs / chl: start and length of every chunk,
    // columns' first). One copy, whatever the number of members.
    struct DesignTables {
        std::shared_ptr<const DesignPlan> design;
        DevBuf<long long> arp, acp, tptr, chs;
        DevBuf<int> acol, arow, tobs, cchoff, tchoff, chl;
        DevBuf<double> aval, acv, tw, offset;
        int ncc = 0, nct = 0;
    };
    void design_upload(const std::shared_ptr<const DesignPlan> &plan, DesignTables &t);
    // Fisher-scoring state, ONE data set for `members` members (fisher_build). Node form: y, aux, mask by node (n each), part = one
    // (energy, loglik) pair per workgroup and member. Design form: y / aux by observation (mask unused), the tables above once, and per
    // member g, d (nobs each), the chunk sums cpart (ncc + nct), the energy partials (part: design_blocks(n)) and the loglik partials
    // (lpart: design_blocks(nobs)). Either form: spart = the loop's reductions (4 per chunk and member), out = 6 per member (2 of every
    // member's evaluation, then 4 of every member's reductions) with its pinned copy, work = the loop's five vectors and the Hessian
    // (5 n + hess_len per member, on first use).
    // The handle keeps two, independent of each other. fisher_ (gmrfx_obs_set): one member, its parameter and the log by value, the
    // rows of sym_rows_. bfisher_ (gmrfx_batch_obs_set; a plain handle's is a batch of one): the members' parameters and their logs on
    // the device, the member's own row structure (the forest's first n rows), nnz = the member's stride in the priors' values, and the
    // loop's control words (ctl: `members` step lengths, then `members` mask bytes) with their pinned copy.
    struct FisherDev : DesignTables {
        int family = 0, members = 1, n = 0;                  // n: a member's nodes
        double param = 0, logparam = 0;                    // by value (fisher_); 0 where param_k / logparam_k hold one per member
        long long nnz = 0;
        std::vector<double> loglik_const;                    // one per member
        DevBuf<double> y, aux, part, out, spart, work;
        DevBuf<unsigned char> mask;
        PinnedBuf<double> h_out;
        DevBuf<double> g, d, lpart, cpart;
        DevBuf<double> param_k, logparam_k, ctl;
        // a composite likelihood (fisher_ only; ncomp = 0: a single family): the component of every observation and the component
        // table, cpar = ncomp parameters, then their ncomp logs
        int ncomp = 0;
        DevBuf<unsigned char> comp;
        DevBuf<int> cfamily;
        DevBuf<double> cpar;
        std::vector<long long> crowptr;  // host: ncomp + 1 row offsets (the pullback's component tiling is built from them)
        std::vector<int> cfam;           // host: ncomp families
        ObsComp comp_table() const;      // (kernels.h; device_fisher.cpp)
        DevBuf<long long> rp;
        DevBuf<int> col, pos;
        PinnedBuf<double> h_ctl;
    } fisher_, bfisher_;
    // what a likelihood is built from: the data by node, or by observation with the plan (design non-null), and one parameter with its
    // loglik_const per member. rows non-null: the batch slot (parameters, rows and control words on the device), n its member's nodes.
    struct FisherSource {
        int family;
        const ObsByNode *by_node;
        const std::vector<double> *y, *aux;
        std::shared_ptr<const DesignPlan> design;
        const std::vector<double> &param, &loglik_const;
        const ObsComponents *comp = nullptr;      // a composite likelihood (design form, one member)
    };
    FisherDev fisher_build(const FisherSource &src, size_t n, const RbmcSym *rows);
    // An evaluation of every member of a slot on the row structure `rows`: member k's point at d_x + k sx, mean at d_mu + k smu
    // (nullable), score at + k ss, hess at + k sh (either nullable), d_active (device, nullable = all) its mask and active (host,
    // nullable) the same bytes: out_host[2 k ..] = {energy, loglik with the member's loglik_const} of the members it names. The one
    // place FisherEval and FisherDesign are filled. Synchronises.
    struct FisherRows { const long long *rp; const int *col, *pos; };
    struct FisherIO { const double *d_x; long long sx; const double *d_mu; long long smu; double *d_score, *d_hess; long long ss, sh; const unsigned char *d_active; };
    void fisher_launch(FisherDev &f, const FisherRows &rows, const FisherIO &io, const unsigned char *active, double *out_host);
    // the loop's four reductions {sum a b, sum (c - d)^2, sum d^2, max |b|} of the members of m, to the host: out4[4 k ..] for the
    // members `active` names (host, nullable = all). Synchronises.
    void fisher_stats(FisherDev &f, const FisherMembers &m, const double *a, const double *b, const double *c, const double *d,
                      const unsigned char *active, double *out4);
    // the map gmrfx_batch_set_prior installed: false: the forest's diagonal (node form), true: the replicated map of a design plan;
    // bprior_map_ok_: -1 not compared with the plan in place since then, 0 / 1 (also reset by bobs_set)
    bool bprior_design_ = false;
    int bprior_map_ok_ = -1;
    void bfisher_ctl(const std::vector<double> *alpha, const std::vector<unsigned char> &mask);
    void bfisher_check_prior();
    // pullback state, built on the first gmrfx_ga_pullback for the likelihood in place (obs_set drops it): the transposed term table
    // of the plan (ONE copy), and per member the work vectors xbar, lam (n each) and t (nobs, design form), the partial sums of the two
    // parameter sums, the result
    // A composite (gap_ only): the component tiling of kernels.h: GapTiles -- bptr and the row offsets on the device, nblk workgroups;
    // part holds 2 nblk partial sums and out / h_out ncomp results. Uploaded with the first composite pullback, dropped by obs_set
    // with the rest; gmrfx_obs_composite_set_param leaves them (only the parameter table changes).
    struct GapDev {
        DevBuf<long long> optr;
        DevBuf<int> oidx;
        DevBuf<double> ow, work, part, out;
        PinnedBuf<double> h_out;
        DevBuf<int> bptr;
        DevBuf<long long> crow;
        int nblk = 0;
    } gap_, bgap_;               // of fisher_ (obs_set drops it) and of bfisher_ (bobs_set does): sized for the slot's members
    void gap_tables(const FisherDev &f, GapDev &g);
    void gap_term_table();       // the plan's transposed term table alone (also what gmrfx_predictor_marginals needs of the pullback's state)
    void gap_term_table(const FisherDev &f, GapDev &g);
    // The launch sequence of the pullback for the members of a likelihood slot (f with its state g), the ONE place the kernels'
    // arguments are filled: xbar, the forest solve, the projection (project: 0 none, 1 the plain constraint, 2 the batch constraint;
    // its operands prepared by the caller), the outputs, the two results per member. The factor in hand is the one to solve with.
    // hmap / colptr / row / rows: the MEMBER's slice of the Hessian map, its pattern and its symmetric rows; d_active (device, nullable
    // = all) and active (host) name the members that take part: the others get NaN in their output slices and results.
    struct GapRun {
        const long long *hmap, *colptr;
        const int *row;
        FisherRows rows;
        long long sx, smu;
        int project;
        const unsigned char *d_active, *active;
    };
    void gap_launch(FisherDev &f, GapDev &g, const GapRun &r, const GapIO &io, double *out_host);
    // what ga_pullback and ga_pullback_composite do ahead of their launches: the argument checks (messages prefixed "who: "), the
    // factorisation of Q_prior - H(x) under bit 1, the constraint's operands under bit 0, the pattern and the symmetric rows.
    // Returns 0, 1 (factorisation failed, *info = 1 + the step) or 2 (the constraint's W failed).
    int gap_prepare(const RbmcSym &sym, const GapIO &io, long long *info, const char *who);
    // predictive state, built on the first gmrfx_predictor_marginals / gmrfx_predictive_scores for the likelihood in place (obs_set
    // drops it): the observed nodes in the caller's order (node form, 4 nobs bytes), the constants c (8 nobs), the plan's map (design
    // form, 8 cnt), the scores' partial sums (4 per workgroup), totals and quadrature rule. The batch slot (bpred_, of bfisher_;
    // bobs_set and bobs_set_param drop it): the same tables once, c as ONE column (sc = 0; families 1, 2, 3) or one per member (sc =
    // nobs; the families with a parameter), partial sums and totals per member, the member's diagonal positions (node form, 4 n bytes,
    // on the first variance) and the mixture's weights with their pinned copy.
    struct PredDev {
        long long nobs = 0, sc = 0;
        int members = 1;
        DevBuf<int> idx, dpos;
        DevBuf<long long> hmap;
        DevBuf<double> c, part, out, quad, mixw;
        PinnedBuf<double> h_out, h_quad, h_mixw;
    } pred_, bpred_;
    void pred_tables(const ObsHost &o);
    void bpred_tables(const BObsHost &o);
    // what pred_tables and bpred_tables build alike, aside: the observation order or the plan's map, c (cols columns), the work of
    // `members` members
    PredDev pred_build(long long nobs, const std::vector<long long> &idx, const DesignPlan *plan, const std::vector<double> &c, int members);
    // The launches of the marginals and of the scores for the members of a likelihood slot (f with its pullback state g, whose term
    // table the design form reads, and its predictive state p), the ONE place the kernels' arguments are filled. Both only enqueue.
    // dpos: the member's diagonal positions; B (m columns; m = 0: no correction): member k's at + k sb; sz: the member's stride in
    // the offset table of Z; d_active (device, nullable = all): the members that take part.
    struct PredRun { const int *dpos; const double *B; int m; long long sx, sz, sb, so; const unsigned char *d_active; };
    void pred_marg_launch(const FisherDev &f, const GapDev &g, const PredDev &p, const PredRun &r, const PredIO &io);
    void pred_score_launch(const FisherDev &f, PredDev &p, const ScoreIO &io, long long stride, const unsigned char *d_active);
    void fisher_check_map(const RbmcSym &sym, const char *who);
    std::vector<long long> h_hmap_;       // host copy of set_prior's map: fisher_eval checks that it is the diagonal's
    int prior_diag_ = -1;                 // -1: not looked at since set_prior, 0 / 1: the map is (not) "position of (i, i) for every i"
    int prior_design_ = -1;               // the same against the map of the design plan (also reset by obs_set)
    void grad_tables();
    void grad_drop_constraint() { grad_.acolptr.reset(); grad_.arow.reset(); grad_.aval.reset(); grad_.Bt.reset(); grad_.bt_serial = 0; }   // (behind a synchronisation)
    void grad_constraint_tables(const ConHost &A, int m, const double *d_B, int nb, long long n);
    void con_drop();
    void prepare_batch_quadform(long long npairs);
    void enqueue_batch_quadform(hipStream_t st, const double *d_nz, const double *d_X, long long ldx, long long sx, long long nvec,
                                const double *d_mu);
};

void hip_check(hipError_t e, const char *what);

// out[k] = the term of observation k's log density that does not depend on x (obs_const.h), rounded to double; no device
void obs_pointwise_const(const ObsHost &o, double *out);
// the same at param[k] of every member, out: nobs x members (the families without a parameter repeat one column)
void bobs_pointwise_const(const BObsHost &o, double *out);

// slicing of a column-major n x nrhs host array for the page-locked staging ring (device.cpp: host_upload / host_download)
struct HostIoPlan { long long cols_per = 1, ppc = 1, rows_per = 0, slot_doubles = 0, nsl = 0, reserve = 0; };
HostIoPlan host_io_plan(long long n, long long nrhs, long long slice_bytes);
HostIoPlan host_io_plan_dir(long long n, long long nrhs, int download);

}  // namespace gmrfx
