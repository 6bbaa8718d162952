"""Composite likelihoods: several observation families on one handle (gmrfx_obs_set_composite; the reference's
CompositeObservationModel / CompositeLikelihood, src/observation_models/composite/). A CompositeObservations collects the components
and stacks them into the one design matrix the C ABI takes; the free functions below call the C ABI on a backend's handle. Everything
after that is the backend's own: set_prior with observations_hess_map(), fisher_eval, gaussian_approximation, predictor_marginals,
predictive_scores and observations_pointwise_const run the composite unchanged. The pullback of gaussian_approximation needs one
parameter cotangent per component: ga_pullback / ga_pullback_dev below (gmrfx_ga_pullback_composite), free functions as the setters are."""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from ._lib import check, lib, ptr
from .backend import MI355XBackend

MAX_COMPONENTS = 16
COMPOSITE = -2      # the family gmrfx_obs_info reports for a composite


class CompositeObservations:
    """The components of a joint model on n latent nodes, in the order they are added. Each is (family, y, A or indices, offset, aux,
    param): `A` a sparse n_c x n design matrix (the reference's LinearlyTransformedLikelihood), or `indices` the observed nodes
    (0-based; rows of the identity, the reference's plain ExponentialFamily likelihood on x[indices]); None for both: every node in
    order. Two components may observe the same nodes."""

    def __init__(self, n: int):
        self.n = int(n)
        self.components = []

    def add(self, family, y, A=None, indices=None, offset=None, aux=None, param: float = 0.0) -> "CompositeObservations":
        fam = MI355XBackend.OBS_FAMILIES[family] if isinstance(family, str) else int(family)
        yy = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if A is not None and indices is not None:
            raise ValueError("a component is given by A or by indices, not both")
        if A is None:
            idx = np.arange(self.n, dtype=np.int64) if indices is None else np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
            if idx.size != yy.size or (idx.size and (idx.min() < 0 or idx.max() >= self.n)):
                raise ValueError("indices must name one node in [0, n) per observation")
            Ac = sp.csr_matrix((np.ones(idx.size), idx, np.arange(idx.size + 1)), shape=(idx.size, self.n))
        else:
            Ac = sp.csr_matrix(A, dtype=np.float64)
            if Ac.shape != (yy.size, self.n):
                raise ValueError(f"A must be nobs x n = {yy.size} x {self.n}, got {Ac.shape}")
        if yy.size == 0:
            raise ValueError("a component needs at least one observation")
        vec = [None if v is None else np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (offset, aux)]
        if any(v is not None and v.size != yy.size for v in vec):
            raise ValueError("offset / aux do not have one entry per observation")
        self.components.append((fam, yy, Ac, vec[0], vec[1], float(param)))
        return self

    def stacked(self) -> dict:
        """What gmrfx_obs_set_composite takes: family, param, rowptr (0-based) per component; y, the stacked A in sorted CSC, offset
        and aux per row (None when no component has one; a component without one gets 0 / NaN on its rows -- aux is never read there)."""
        if not 1 <= len(self.components) <= MAX_COMPONENTS:
            raise ValueError(f"a composite has 1 .. {MAX_COMPONENTS} components")
        fam, ys, As, offs, auxs, par = zip(*self.components)
        rows = [y.size for y in ys]
        A = sp.vstack(As, format="csc")
        if not A.has_canonical_format:
            A.sum_duplicates()
        offset = None if all(o is None for o in offs) else np.concatenate([np.zeros(r) if o is None else o for o, r in zip(offs, rows)])
        aux = None if all(a is None for a in auxs) else np.concatenate([np.full(r, np.nan) if a is None else a for a, r in zip(auxs, rows)])
        return {"family": np.asarray(fam, np.int32), "param": np.asarray(par, np.float64),
                "rowptr": np.concatenate([[0], np.cumsum(rows)]).astype(np.int64), "y": np.concatenate(ys), "A": A, "offset": offset, "aux": aux}


def set_composite_observations(backend, comp: CompositeObservations) -> None:
    """The composite as state of the backend's handle. set_prior then takes backend.observations_hess_map()."""
    if comp.n != backend.n:
        raise ValueError(f"the composite is on {comp.n} nodes, the backend on {backend.n}")
    s = comp.stacked()
    A = s["A"]
    cp, rv = np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int64)
    nz = np.ascontiguousarray(A.data, dtype=np.float64)
    check(lib().gmrfx_obs_set_composite(backend._h, len(s["family"]), ptr(s["family"]), ptr(s["param"]), ptr(s["rowptr"]), s["y"].size,
                                        ptr(cp), ptr(rv), ptr(nz), 0, ptr(s["offset"]), ptr(s["y"]), ptr(s["aux"])), backend._h)


def composite_info(backend) -> dict:
    """family, param, rowptr (0-based) and loglik_const per component (gmrfx_obs_composite_info); empty arrays when none is set"""
    nc = C.c_int32(0)
    check(lib().gmrfx_obs_composite_info(backend._h, C.byref(nc), None, None, None, None), backend._h)
    fam, par, rp, c = np.empty(nc.value, np.int32), np.empty(nc.value), np.empty(nc.value + 1, np.int64), np.empty(nc.value)
    if nc.value > 0:
        check(lib().gmrfx_obs_composite_info(backend._h, C.byref(nc), ptr(fam), ptr(par), ptr(rp), ptr(c)), backend._h)
    return {"family": fam, "param": par, "rowptr": rp if nc.value > 0 else rp[:0], "loglik_const": c}


def _flags(backend, project: bool, refactorize: bool) -> int:
    if refactorize:         # the factor changes: the backend's cached selected inverse no longer belongs to it
        backend._selinv_cache = None
        backend._selinv_diag_cache = None
    return int(bool(project)) | (int(bool(refactorize)) << 1)


def ga_pullback(backend, x, mean=None, mubar=None, Qbar=None, project: bool = False, refactorize: bool = False,
                want_Qbar_prior: bool = True, want_mubar_prior: bool = True, want_lambda: bool = True):
    """The implicit-function rule at the mode x for the composite on the backend's handle (gmrfx_ga_pullback_composite): the arguments
    of MI355XBackend.ga_pullback. Returns (Qbar_prior, mubar_prior, lambda, param_bar, lambda' xbar) with param_bar one cotangent per
    component (0.0 for a component without a parameter); the arrays not asked for are None."""
    n, nnz = backend.n, backend._nnz
    xx = np.ascontiguousarray(x, dtype=np.float64)
    mu, mb, qb = (None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (mean, mubar, Qbar))
    if xx.shape != (n,) or any(v is not None and v.shape != (n,) for v in (mu, mb)) or (qb is not None and qb.shape != (nnz,)):
        raise ValueError("dimension mismatch")
    qp = np.empty(nnz) if want_Qbar_prior else None
    mp = np.empty(n) if want_mubar_prior else None
    lam = np.empty(n) if want_lambda else None
    par, chk = np.zeros(max(composite_info(backend)["family"].size, 1)), C.c_double(0.0)
    rc = lib().gmrfx_ga_pullback_composite(backend._h, ptr(xx), ptr(mu), ptr(mb), ptr(qb), _flags(backend, project, refactorize), ptr(qp), ptr(mp),
                                           ptr(lam), ptr(par), C.byref(chk))
    check(rc, backend._h)
    return qp, mp, lam, par, chk.value


def ga_pullback_dev(backend, d_x: int, d_mu: int = 0, d_mubar: int = 0, d_Qbar: int = 0, d_Qbar_prior: int = 0, d_mubar_prior: int = 0,
                    d_lambda: int = 0, project: bool = False, refactorize: bool = False):
    """Device pointers (0 = absent); d_Qbar_prior may be d_Qbar. Returns (param_bar, lambda' xbar)."""
    if not d_x:
        raise ValueError("ga_pullback_dev: null pointer")
    par, chk = np.zeros(max(composite_info(backend)["family"].size, 1)), C.c_double(0.0)
    rc = lib().gmrfx_ga_pullback_composite_dev(backend._h, d_x, d_mu or None, d_mubar or None, d_Qbar or None, _flags(backend, project, refactorize),
                                               d_Qbar_prior or None, d_mubar_prior or None, d_lambda or None, ptr(par), C.byref(chk))
    check(rc, backend._h)
    return par, chk.value


def set_composite_param(backend, params) -> None:
    """The components' sigma / r / phi replaced in place (gmrfx_obs_composite_set_param): the plan and the map stay."""
    p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
    if p.size != composite_info(backend)["family"].size:
        raise ValueError("params must have one entry per component")
    check(lib().gmrfx_obs_composite_set_param(backend._h, ptr(p)), backend._h)
