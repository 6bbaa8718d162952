"""Composite likelihoods: several observation families on one handle (gmrfx_obs_set_composite; the reference's
CompositeObservationModel / CompositeLikelihood, src/observation_models/composite/). A CompositeObservations collects the components
and stacks them into the one design matrix the C ABI takes; the free functions below call the C ABI on a backend's handle. Everything
after that is the backend's own: set_prior with observations_hess_map(), fisher_eval, gaussian_approximation, predictor_marginals,
predictive_scores and observations_pointwise_const run the composite unchanged."""
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


def set_composite_param(backend, params) -> None:
    """The components' sigma / r / phi replaced in place (gmrfx_obs_composite_set_param): the plan and the map stay."""
    p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
    if p.size != composite_info(backend)["family"].size:
        raise ValueError("params must have one entry per component")
    check(lib().gmrfx_obs_composite_set_param(backend._h, ptr(p)), backend._h)
