"""MI355XBatchLaplace -- a batched handle with the non-Gaussian path: one observation data set, one prior precision and one
likelihood parameter per member, Fisher scoring and the Gaussian approximation for all members in one pass over the forest
(include/gmrfx.h: gmrfx_batch_set_prior, gmrfx_batch_obs_set, gmrfx_batch_obs_set_design, gmrfx_batch_fisher_eval,
gmrfx_batch_gaussian_approximation, gmrfx_batch_constrained_gaussian_approximation while set_constraints holds a constraint). The hyper-parameter sweep of a model with Poisson, binomial or similar observations: one Laplace
approximation per theta_k. The observations sit on nodes (set_observations) or are seen through a sparse design matrix, eta = A x + b
(set_design_observations: points inside mesh triangles, intercepts, group effects)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from ._lib import ERR_NOT_POSDEF, check, lib, ptr
from .backend import MI355XBackend, MI355XBatchBackend


class MI355XBatchLaplace(MI355XBatchBackend):
    """Everything MI355XBatchBackend does, plus the likelihood. Shapes: NZ (nnz, B); points, means and scores (n, B); Hessians (n, B) in
    node form and (cnt, B) in design form, in the order of observations_hess_map()."""

    OBS_FAMILIES = MI355XBackend.OBS_FAMILIES

    def clone(self) -> "MI355XBatchLaplace":
        other = super().clone()
        other.__class__ = MI355XBatchLaplace
        return other

    def _points(self, X, what: str, shared_ok: bool = False):
        """(n, B) -> (Fortran array, member stride); (n,) with shared_ok -> (array, 0)"""
        if X is None:
            return None, 0
        X = np.asarray(X, dtype=np.float64)
        if shared_ok and X.shape == (self.n,):
            return np.ascontiguousarray(X), 0
        if X.shape != (self.n, self.nbatch):
            raise ValueError(f"{what} must have shape (n, nbatch) = ({self.n}, {self.nbatch})" + (" or (n,)" if shared_ok else "") + f", got {X.shape}")
        return np.asfortranarray(X), self.n

    def _active(self, active):
        if active is None:
            return None
        a = np.ascontiguousarray(np.asarray(active).astype(bool), dtype=np.uint8).reshape(-1)
        if a.size != self.nbatch:
            raise ValueError("active must have one entry per member")
        return a

    def set_prior(self, NZ) -> None:
        """The members' prior precisions, (nnz, B); the Hessian map of every member is installed by the library, for the likelihood in
        place: the diagonal (none yet, or set_observations) or the map of the design form. Call it again after changing the
        likelihood's form."""
        nz = self._values(NZ)
        check(lib().gmrfx_batch_set_prior(self._h, ptr(nz)), self._h)

    def set_observations(self, family, y, indices=None, aux=None, param=0.0, index_base: int = 0) -> None:
        """ONE data set for all members (as MI355XBackend.set_observations) and one param per member: a scalar, or an array of length B.
        An empty y removes the likelihood."""
        fam = self.OBS_FAMILIES[family] if isinstance(family, str) else int(family)
        yy = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        ax = None if aux is None else np.ascontiguousarray(aux, dtype=np.float64).reshape(-1)
        if (idx is not None and idx.size != yy.size) or (ax is not None and ax.size != yy.size):
            raise ValueError("indices / aux do not have one entry per observation")
        pp = np.asarray(param, dtype=np.float64)
        pp = np.full(self.nbatch, float(pp)) if pp.ndim == 0 else np.ascontiguousarray(pp).reshape(-1)
        if pp.size != self.nbatch:
            raise ValueError("param must be a scalar or have one entry per member")
        check(lib().gmrfx_batch_obs_set(self._h, fam, yy.size, ptr(idx), int(index_base), ptr(yy), ptr(ax), ptr(pp)), self._h)

    def set_design_observations(self, family, y, A, b=None, aux=None, param=0.0) -> None:
        """ONE data set for all members observed through eta = A x + b (gmrfx_batch_obs_set_design; as
        MI355XBackend.set_design_observations: A any scipy sparse matrix, nobs x n) and one param per member: a scalar, or an array of
        length B. Replaces a node-form likelihood; an empty y removes the likelihood. set_prior (again) installs the members' maps."""
        fam = self.OBS_FAMILIES[family] if isinstance(family, str) else int(family)
        yy = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        Ac = sp.csc_matrix(A, dtype=np.float64)
        if Ac.shape != (yy.size, self.n):
            raise ValueError(f"A must be nobs x n = {yy.size} x {self.n}, got {Ac.shape}")
        if not Ac.has_canonical_format:
            Ac = Ac.copy()
            Ac.sum_duplicates()
        off = None if b is None else np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
        ax = None if aux is None else np.ascontiguousarray(aux, dtype=np.float64).reshape(-1)
        if (off is not None and off.size != yy.size) or (ax is not None and ax.size != yy.size):
            raise ValueError("b / aux do not have one entry per observation")
        pp = np.asarray(param, dtype=np.float64)
        pp = np.full(self.nbatch, float(pp)) if pp.ndim == 0 else np.ascontiguousarray(pp).reshape(-1)
        if pp.size != self.nbatch:
            raise ValueError("param must be a scalar or have one entry per member")
        cp = np.ascontiguousarray(Ac.indptr, dtype=np.int64)
        rv = np.ascontiguousarray(Ac.indices, dtype=np.int64)
        nz = np.ascontiguousarray(Ac.data, dtype=np.float64)
        check(lib().gmrfx_batch_obs_set_design(self._h, fam, yy.size, ptr(cp), ptr(rv), ptr(nz), 0, ptr(off), ptr(yy), ptr(ax), ptr(pp)), self._h)

    def set_param(self, param) -> None:
        """The members' likelihood parameters (sigma, r, phi) replaced in place (gmrfx_batch_obs_set_param): a scalar, or an array of
        length B. The data set and, in design form, the plan stay as they are; works while a constraint is held, where
        set_observations is refused."""
        pp = np.asarray(param, dtype=np.float64)
        pp = np.full(self.nbatch, float(pp)) if pp.ndim == 0 else np.ascontiguousarray(pp).reshape(-1)
        if pp.size != self.nbatch:
            raise ValueError("param must be a scalar or have one entry per member")
        check(lib().gmrfx_batch_obs_set_param(self._h, ptr(pp)), self._h)

    def observations_hess_map(self) -> np.ndarray:
        """0-based positions into ONE member's values of the entries of A' D A, ascending (gmrfx_batch_obs_hess_map): the order of the
        Hessian values fisher_eval and gaussian_approximation return per member in design form."""
        cnt = C.c_int64(0)
        check(lib().gmrfx_batch_obs_hess_map(self._h, None, 0, C.byref(cnt)), self._h)
        m = np.empty(cnt.value, np.int64)
        check(lib().gmrfx_batch_obs_hess_map(self._h, ptr(m), m.size, C.byref(cnt)), self._h)
        return m

    def observations_design_info(self) -> dict:
        """nnz(A), cnt and the term count of the design plan (-1 each in node form)"""
        a, c, t = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().gmrfx_batch_obs_design_info(self._h, C.byref(a), C.byref(c), C.byref(t)), self._h)
        return {"nnz": a.value, "cnt": c.value, "terms": t.value}

    def _hess_len(self) -> int:
        """entries of a member's Hessian vector: n in node form, the map's cnt in design form"""
        cnt = self.observations_design_info()["cnt"]
        return self.n if cnt < 0 else cnt

    def observations_info(self) -> dict:
        fam, nobs, c = C.c_int32(0), C.c_int64(0), np.zeros(self.nbatch)
        check(lib().gmrfx_batch_obs_info(self._h, C.byref(fam), C.byref(nobs), ptr(c)), self._h)
        return {"family": fam.value, "nobs": nobs.value, "loglik_const": c}

    def fisher_eval(self, X, mean=None, active=None, want_score: bool = True, want_hess: bool = True, score=None, hess=None):
        """(score (n, B), hess (n, B), energy (B,), loglik (B,)) at the members' points X (n, B); mean: (n,) for every member or (n, B).
        Design form: hess is (cnt, B). Both outputs are views of arrays of max(n, cnt) rows (one member stride serves both); arrays
        passed in must have that many rows. active: B flags; a member whose flag is 0 is skipped and its columns of score / hess (pass
        arrays to see that; fresh ones are NaN there) and its energy / loglik (NaN) are left untouched."""
        Xf, sx = self._points(X, "X")
        mu, smu = self._points(mean, "mean", shared_ok=True)
        act = self._active(active)
        hl = self._hess_len()
        ld = max(self.n, hl)

        def _out(given, want):
            if not want and given is None:
                return None
            if given is None:
                return np.full((ld, self.nbatch), np.nan, order="F")
            if given.shape != (ld, self.nbatch) or not given.flags.f_contiguous or given.dtype != np.float64:
                raise ValueError("score / hess must be Fortran float64 arrays of shape (max(n, cnt), nbatch)")
            return given
        sc, hs = _out(score, want_score), _out(hess, want_hess)
        out = np.full((2, self.nbatch), np.nan, order="F")
        check(lib().gmrfx_batch_fisher_eval(self._h, ptr(Xf), sx, ptr(mu), smu, ptr(act), ptr(sc), ptr(hs), ld, ptr(out)), self._h)
        if ld != self.n and sc is not None:
            sc = sc[:self.n]
        if ld != hl and hs is not None:
            hs = hs[:hl]
        return sc, hs, out[0].copy(), out[1].copy()

    def fisher_eval_dev(self, d_x: int, sx: int, d_mu: int = 0, smu: int = 0, active=None, d_score: int = 0, d_hess: int = 0, ss: int = 0, out=None):
        """Device pointers with member strides (smu = 0: one mean; ss serves score and hess: at least n for score, at least cnt for a
        design-form hess; default max(n, cnt)); returns (energy (B,), loglik (B,)); `out` (2, B) Fortran is filled in place when given
        (inactive members' pairs stay as they are)."""
        if not d_x:
            raise ValueError("fisher_eval_dev: null pointer")
        act = self._active(active)
        if out is None:
            out = np.full((2, self.nbatch), np.nan, order="F")
        check(lib().gmrfx_batch_fisher_eval_dev(self._h, d_x, sx, d_mu or None, smu, ptr(act), d_score or None, d_hess or None, ss or max(self.n, self._hess_len()),
                                                ptr(out)), self._h)
        return out[0].copy(), out[1].copy()

    def _ga_call(self, dev: bool, head, tail):
        """the loop's entry point for the handle's state: the constrained one while set_constraints holds a constraint. Returns
        (rc, cinfo, residual), the last two None without a constraint."""
        L = lib()
        if self._con_m() > 0:
            ci, rs = np.zeros(self.nbatch, np.int64), np.full(self.nbatch, np.nan)
            fn = L.gmrfx_batch_constrained_gaussian_approximation_dev if dev else L.gmrfx_batch_constrained_gaussian_approximation
            return fn(*head, *tail, ptr(ci), ptr(rs)), ci, rs
        fn = L.gmrfx_batch_gaussian_approximation_dev if dev else L.gmrfx_batch_gaussian_approximation
        return fn(*head, *tail), None, None

    @staticmethod
    def _laplace_state(res, cinfo, refactorize_final):
        """what laplace_terms() keeps of the last loop: energy and loglik at the modes; at_modes: a constraint was held and the handle
        was left factorised at the modes (logdet_W is then that of the modes); failed: the members whose constraint status is not 0"""
        return {"energy": res[8].copy(), "loglik": res[9].copy(), "at_modes": cinfo is not None and bool(refactorize_final),
                "failed": None if cinfo is None else cinfo != 0}

    def _ga_info(self, res, totals, dec, alp, info, rc, cinfo=None, residual=None):
        con = {} if cinfo is None else {"cinfo": cinfo, "residual": residual}
        return {**con, "iterations": res[0].astype(np.int64), "converged": res[1] != 0, "alpha": res[2].copy(), "decrement": res[3].copy(),
                "factorizations": res[4].astype(np.int64), "solves": res[5].astype(np.int64), "merit_evaluations": res[6].astype(np.int64),
                "frozen_finish": res[7] != 0, "energy": res[8].copy(), "loglik": res[9].copy(), "info": info.copy(),
                "dec_trace": [dec[~np.isnan(dec[:, k]), k].copy() for k in range(self.nbatch)],
                "alpha_trace": [alp[~np.isnan(alp[:, k]), k].copy() for k in range(self.nbatch)],
                "totals": {"factorizations": int(totals[0]), "solves": int(totals[1]), "evaluations": int(totals[2])},
                "posdef": rc != ERR_NOT_POSDEF}

    def gaussian_approximation(self, mean=None, x0=None, max_iter: int = 50, mean_change_tol: float = 1e-4, newton_dec_tol: float = 1e-5,
                               adaptive_stepsize: bool = True, max_linesearch_iter: int = 10, step_recovery: str = "retry_full",
                               predictive_convergence: bool = True, refactorize_final: bool = False):
        """The Gaussian approximation of every member (gmrfx_batch_gaussian_approximation): (X (n, B), H, info); H is (n, B) in node form
        and (cnt, B) in design form (the values of A' D_k A at the mode, in the order of observations_hess_map()). info holds
        per-member arrays (iterations, converged, alpha, decrement, factorizations, solves, merit_evaluations, frozen_finish, energy,
        loglik, info; dec_trace and alpha_trace as lists of arrays) and the forest-level `totals`. A member whose factorisation failed
        does not raise: info["info"][k] > 0, X[:, k] is its last accepted iterate and H[:, k] is NaN; the others are complete.
        While set_constraints holds a constraint every step is projected onto A s = 0 (gmrfx_batch_constrained_gaussian_approximation;
        x0 or the mean must satisfy A x = e) and info gains cinfo (0, 1 + the failing pivot of W_k, -1 beside a failed
        factorisation) and residual (max |A x_k - e|, NaN for a failed member)."""
        mu, smu = self._points(mean, "mean", shared_ok=True)
        xs, sx0 = self._points(x0, "x0")
        hl = self._hess_len()
        X = np.empty((self.n, self.nbatch), order="F")
        H = np.full((hl, self.nbatch), np.nan, order="F")
        res, totals = np.zeros((10, self.nbatch), order="F"), np.zeros(3)
        dec, alp = (np.full((max_iter + 1, self.nbatch), np.nan, order="F") for _ in range(2))
        info = np.zeros(self.nbatch, np.int64)
        flags = MI355XBackend._ga_flags(adaptive_stepsize, step_recovery, predictive_convergence, refactorize_final)
        rc, ci, rs = self._ga_call(False, (self._h, ptr(mu), smu, ptr(xs), sx0, max_iter, max_linesearch_iter, float(mean_change_tol),
                                           float(newton_dec_tol), flags),
                                   (ptr(X), self.n, ptr(H), hl, ptr(res), ptr(totals), ptr(dec), ptr(alp), ptr(info)))
        self._info = info.copy()
        if rc != ERR_NOT_POSDEF:
            check(rc, self._h)
        self._laplace = self._laplace_state(res, ci, refactorize_final)
        return X, H, self._ga_info(res, totals, dec, alp, info, rc, ci, rs)

    def gaussian_approximation_dev(self, d_x: int, sx: int, d_hess: int = 0, sh: int = 0, d_mu: int = 0, smu: int = 0, d_x0: int = 0, sx0: int = 0,
                                   max_iter: int = 50, mean_change_tol: float = 1e-4, newton_dec_tol: float = 1e-5, adaptive_stepsize: bool = True,
                                   max_linesearch_iter: int = 10, step_recovery: str = "retry_full", predictive_convergence: bool = True,
                                   refactorize_final: bool = False) -> dict:
        """Device pointers with member strides: the modes x and hess (0 = not wanted; sh at least n, or cnt in design form, which is
        the default) outputs, mean (smu = 0: one mean) and x0. Returns the info dict."""
        if not d_x:
            raise ValueError("gaussian_approximation_dev: null pointer")
        res, totals = np.zeros((10, self.nbatch), order="F"), np.zeros(3)
        dec, alp = (np.full((max_iter + 1, self.nbatch), np.nan, order="F") for _ in range(2))
        info = np.zeros(self.nbatch, np.int64)
        flags = MI355XBackend._ga_flags(adaptive_stepsize, step_recovery, predictive_convergence, refactorize_final)
        rc, ci, rs = self._ga_call(True, (self._h, d_mu or None, smu, d_x0 or None, sx0 or self.n, max_iter, max_linesearch_iter,
                                          float(mean_change_tol), float(newton_dec_tol), flags),
                                   (d_x, sx, d_hess or None, sh or self._hess_len(), ptr(res), ptr(totals), ptr(dec), ptr(alp), ptr(info)))
        self._info = info.copy()
        if rc != ERR_NOT_POSDEF:
            check(rc, self._h)
        self._laplace = self._laplace_state(res, ci, refactorize_final)
        return self._ga_info(res, totals, dec, alp, info, rc, ci, rs)

    def laplace_terms(self) -> dict:
        """energy and loglik at the modes of the last gaussian_approximation and logdet of the factor in hand, per member. With
        log det Q_p,k the Laplace marginal likelihood of member k is loglik - energy' + (log det Q_p,k - logdet) / 2, where energy' is
        the energy plus mu' Q_p,k mu / 2 (zero for a zero prior mean). After refactorize_final=True the factor is that of the mode.
        With a constraint held and refactorize_final=True the dict gains logdet_W (B,): log det(A Q_post,k^-1 A') at the modes
        (constraint_info), NaN for the members that failed."""
        if getattr(self, "_laplace", None) is None:
            raise ValueError("laplace_terms: gaussian_approximation has not been called")
        st = self._laplace
        out = {"energy": st["energy"].copy(), "loglik": st["loglik"].copy(), "logdet": self.logdet()}
        if st["at_modes"] and self._con_m() > 0:
            ci = self.constraint_info(check_posdef=False)
            out["logdet_W"] = np.where(st["failed"] | (ci["cinfo"] != 0), np.nan, ci["logdet_W"])
        return out

    # -- the pullback of the Gaussian approximation, per member (include/gmrfx.h "The same pullback for every member of a batched handle")
    def ga_pullback(self, X, mean=None, mubar=None, Qbar=None, project: bool = False, refactorize: bool = False,
                    want_Qbar_prior: bool = True, want_mubar_prior: bool = True, want_lambda: bool = True):
        """The implicit-function rule at every member's mode (gmrfx_batch_ga_pullback), the link between logpdf_grad and pattern_dot.
        X (n, B); mean (n,) for every member or (n, B); mubar (n, B) / Qbar (nnz, B, on the pattern, as logpdf_grad returns it): the
        cotangents of the posterior means / precisions, either None (zero). Returns (Qbar_prior (nnz, B), mubar_prior (n, B), lam
        (n, B), param (B,), check (B,), info (B,)); the arrays not asked for are None. project: lam_k is projected with the batch
        constraint; refactorize: every member is factorised at Q_p,k - H(x_k) first (otherwise the handle holds those factors:
        gaussian_approximation with refactorize_final=True). A member whose factorisation (info[k] = -1) or W_k (1 + the failing
        pivot) failed does not raise: its columns, param[k] and check[k] are NaN, the others are complete."""
        Xf, sx = self._points(X, "X")
        mu, smu = self._points(mean, "mean", shared_ok=True)
        mb, _ = self._points(mubar, "mubar")
        qb = None if Qbar is None else self._values(Qbar)
        qp = np.empty((self._nnz, self.nbatch), order="F") if want_Qbar_prior else None
        mp = np.empty((self.n, self.nbatch), order="F") if want_mubar_prior else None
        lam = np.empty((self.n, self.nbatch), order="F") if want_lambda else None
        out = np.empty((2, self.nbatch), order="F")
        info = np.zeros(self.nbatch, np.int64)
        flags = int(bool(project)) | (int(bool(refactorize)) << 1)
        rc = lib().gmrfx_batch_ga_pullback(self._h, ptr(Xf), sx, ptr(mu), smu, ptr(mb), ptr(qb), flags, ptr(qp), ptr(mp), ptr(lam), ptr(out),
                                           ptr(info))
        check(rc, self._h)
        return qp, mp, lam, out[0].copy(), out[1].copy(), info

    def ga_pullback_dev(self, d_x: int, sx: int, d_mu: int = 0, smu: int = 0, d_mubar: int = 0, d_Qbar: int = 0, d_Qbar_prior: int = 0,
                        d_mubar_prior: int = 0, d_lambda: int = 0, project: bool = False, refactorize: bool = False):
        """Device pointers (0 = absent): member k's x at + k sx, mu at + k smu (0: one mean), mubar / mubar_prior / lambda at + k n,
        Qbar / Qbar_prior at + k nnz; d_Qbar_prior may be d_Qbar. Returns (param (B,), check (B,), info (B,))."""
        if not d_x:
            raise ValueError("ga_pullback_dev: null pointer")
        out = np.empty((2, self.nbatch), order="F")
        info = np.zeros(self.nbatch, np.int64)
        flags = int(bool(project)) | (int(bool(refactorize)) << 1)
        rc = lib().gmrfx_batch_ga_pullback_dev(self._h, d_x, sx, d_mu or None, smu, d_mubar or None, d_Qbar or None, flags, d_Qbar_prior or None,
                                               d_mubar_prior or None, d_lambda or None, ptr(out), ptr(info))
        check(rc, self._h)
        return out[0].copy(), out[1].copy(), info

    # -- what follows the fit, per member (include/gmrfx.h "The same read-outs for every member of a batched handle")
    def _nobs(self) -> int:
        nobs = self.observations_info()["nobs"]
        if nobs <= 0:
            raise ValueError("no observation likelihood is set (set_observations / set_design_observations)")
        return nobs

    def _per_obs(self, a, what: str):
        a = np.asarray(a, dtype=np.float64)
        if a.shape != (self._nobs(), self.nbatch):
            raise ValueError(f"{what} must have shape (nobs, nbatch) = ({self._nobs()}, {self.nbatch}), got {a.shape}")
        return np.asfortranarray(a)

    def observations_pointwise_const(self) -> np.ndarray:
        """c (nobs, B): the terms of every observation's log density that do not depend on x, at every member's param
        (gmrfx_batch_obs_pointwise_const); no device needed."""
        c = np.empty((self._nobs(), self.nbatch), order="F")
        check(lib().gmrfx_batch_obs_pointwise_const(self._h, ptr(c)), self._h)
        return c

    def predictor_marginals(self, X, constraint_correction: bool = False, want_mean: bool = True, want_var: bool = True, want_pll: bool = True):
        """(mu_eta, v_eta, pll, info): mean and variance of every member's linear predictor and the log density at the mean, (nobs, B)
        each in the caller's observation order (gmrfx_batch_predictor_marginals); X (n, B) the members' modes. The variance needs the
        factors of the modes (gaussian_approximation with refactorize_final=True). constraint_correction: every member's variance gets
        the correction and clamp of the batch constraint. A member whose factorisation (info[k] = -1) or W_k (1 + the failing pivot)
        failed does not raise: its columns are NaN, the others are complete. The arrays not asked for are None."""
        Xf, sx = self._points(X, "X")
        nobs = self._nobs()
        mu, v, pll = (np.empty((nobs, self.nbatch), order="F") if want else None for want in (want_mean, want_var, want_pll))
        info = np.zeros(self.nbatch, np.int64)
        check(lib().gmrfx_batch_predictor_marginals(self._h, ptr(Xf), sx, int(bool(constraint_correction)), ptr(mu), ptr(v), ptr(pll), ptr(info)),
              self._h)
        return mu, v, pll, info

    def predictor_marginals_dev(self, d_x: int, sx: int, d_mu_eta: int = 0, d_v_eta: int = 0, d_pll: int = 0, constraint_correction: bool = False):
        """Device pointers (0 = not wanted): member k's x at + k sx, outputs (nobs, B) with member stride nobs. Returns info (B,)."""
        info = np.zeros(self.nbatch, np.int64)
        check(lib().gmrfx_batch_predictor_marginals_dev(self._h, d_x or None, sx, int(bool(constraint_correction)), d_mu_eta or None, d_v_eta or None,
                                                        d_pll or None, ptr(info)), self._h)
        return info

    batch_predictor_marginals = predictor_marginals
    batch_predictor_marginals_dev = predictor_marginals_dev

    @staticmethod
    def _rule(nodes, weights, K: int):
        if nodes is None or weights is None:
            nodes, weights = MI355XBackend.gauss_hermite(K)
        z = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if z.size != w.size:
            raise ValueError("nodes and weights must have the same length")
        return z, w

    def predictive_scores(self, mu_eta, v_eta, K: int = 32, nodes=None, weights=None):
        """The quadrature scores of every member over eta_ik ~ N(mu_eta_ik, v_eta_ik) (gmrfx_batch_predictive_scores; the rule of
        MI355XBackend.gauss_hermite(K) unless nodes and weights are given): a dict of lpd, lcpo, elp, vlp (nobs, B), totals (4, B)
        in that order, and info (B,) (-1: the member's factorisation failed; its columns and totals are NaN)."""
        mu, v = self._per_obs(mu_eta, "mu_eta"), self._per_obs(v_eta, "v_eta")
        z, w = self._rule(nodes, weights, K)
        arrs = [np.empty(mu.shape, order="F") for _ in range(4)]
        out = np.empty((4, self.nbatch), order="F")
        info = np.zeros(self.nbatch, np.int64)
        check(lib().gmrfx_batch_predictive_scores(self._h, ptr(mu), ptr(v), z.size, ptr(z), ptr(w), *(ptr(a) for a in arrs), ptr(out), ptr(info)),
              self._h)
        return {"lpd": arrs[0], "lcpo": arrs[1], "elp": arrs[2], "vlp": arrs[3], "totals": out, "info": info}

    def predictive_scores_dev(self, d_mu_eta: int, d_v_eta: int, K: int = 32, nodes=None, weights=None, d_lpd: int = 0, d_lcpo: int = 0,
                              d_elp: int = 0, d_vlp: int = 0):
        """Device pointers, (nobs, B) with member stride nobs (outputs: 0 = not wanted). Returns (totals (4, B), info (B,))."""
        z, w = self._rule(nodes, weights, K)
        out = np.empty((4, self.nbatch), order="F")
        info = np.zeros(self.nbatch, np.int64)
        check(lib().gmrfx_batch_predictive_scores_dev(self._h, d_mu_eta or None, d_v_eta or None, z.size, ptr(z), ptr(w), d_lpd or None,
                                                      d_lcpo or None, d_elp or None, d_vlp or None, ptr(out), ptr(info)), self._h)
        return out, info

    def _logw(self, logw):
        lw = np.ascontiguousarray(logw, dtype=np.float64).reshape(-1)
        if lw.size != self.nbatch:
            raise ValueError("logw must have one entry per member")
        return lw

    def predictive_mixture(self, logw, mu_eta, v_eta, lpd=None):
        """The predictive distribution integrated over the members with weights proportional to exp(logw) (B unnormalised log weights,
        -inf excludes a member; gmrfx_batch_predictive_mixture): (mix_mu, mix_v, mix_lpd, total), (nobs,) each and the sum of mix_lpd;
        without lpd the last two are None."""
        lw = self._logw(logw)
        mu, v = self._per_obs(mu_eta, "mu_eta"), self._per_obs(v_eta, "v_eta")
        lp = None if lpd is None else self._per_obs(lpd, "lpd")
        nobs = mu.shape[0]
        mm, mv = np.empty(nobs), np.empty(nobs)
        ml = None if lp is None else np.empty(nobs)
        out = np.full(1, np.nan)
        check(lib().gmrfx_batch_predictive_mixture(self._h, ptr(lw), ptr(mu), ptr(v), ptr(lp), ptr(mm), ptr(mv), ptr(ml), ptr(out)), self._h)
        return mm, mv, ml, (None if lp is None else float(out[0]))

    def predictive_mixture_dev(self, logw, d_mu_eta: int, d_v_eta: int, d_lpd: int = 0, d_mix_mu: int = 0, d_mix_v: int = 0, d_mix_lpd: int = 0):
        """Device pointers: inputs (nobs, B) with member stride nobs, outputs (nobs,) (0 = not wanted). Returns the sum of mix_lpd
        (NaN without d_lpd)."""
        lw = self._logw(logw)
        out = np.full(1, np.nan)
        check(lib().gmrfx_batch_predictive_mixture_dev(self._h, ptr(lw), d_mu_eta or None, d_v_eta or None, d_lpd or None, d_mix_mu or None,
                                                       d_mix_v or None, d_mix_lpd or None, ptr(out)), self._h)
        return float(out[0])
