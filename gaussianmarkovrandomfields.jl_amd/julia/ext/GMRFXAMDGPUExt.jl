# GMRFXAMDGPUExt.jl -- package extension of GMRFX (weak dependency AMDGPU.jl): the device-resident entry points of
# include/gmrfx.h (`*_dev`: operands already in HBM, no PCIe traffic inside the call) for ROCArray arguments.
#
# Project.toml of the plug-in package:
#     [weakdeps]
#     AMDGPU = "21141c5a-9bdb-4563-92ae-f87d6854732e"
#     [extensions]
#     GMRFXAMDGPUExt = "AMDGPU"
#
# Layout: a ROCMatrix{Float64} of size n x k is column-major with leading dimension stride(A, 2) -- exactly the `ldb` / `ldx`
# convention of the C ABI. The library runs on its own streams and returns when the result is complete; AMDGPU.jl's
# task-local stream is synchronised before the call so that the operands are.
# Reference calls replaced: src/workspace/backend.jl:165-189 (refactorize!), :191-209 (backend_solve), :281-284
# (backend_backward_solve), src/workspace/workspace_gmrf.jl:288-292 (logpdf).
# NOTE: like GMRFX.jl this file cannot be run in this image (no Julia); tests/test_julia_shim_signatures.py checks every
# ccall tuple below against include/gmrfx.h.
module GMRFXAMDGPUExt

using AMDGPU
using LinearAlgebra
import GMRFX
import GMRFX: MI355XBackend, LIB, check, refactorize_solve!, backend_solve!, backend_backward_solve!, logpdf_terms
import GMRFX: MI355XBatch, constrained_logpdf_terms, rbmc_var_dev!, logpdf_grad_dev!, pattern_dot_dev, fisher_eval_dev!, gaussian_approximation_dev!, ga_pullback_dev!, ga_pullback_composite_dev!, composite_info, _ga_flags, _ga_info
import GMRFX: ShardedMI355X, LIB_RCCL, check_rccl, solve!
import GaussianMarkovRandomFields: refactorize!

devptr(A::ROCArray{Float64}) = reinterpret(Ptr{Float64}, pointer(A))

function _invalidate!(b::MI355XBackend)
    b.selinv_cache = nothing
    b.selinv_diag_cache = nothing
    return nothing
end

# numeric refactorisation from values resident in HBM (pattern order of the Q the backend was built from)
function refactorize!(b::MI355XBackend, d_nz::ROCVector{Float64})
    AMDGPU.synchronize()
    info = Ref{Int64}(0)
    GC.@preserve d_nz check(ccall((:gmrfx_refactorize_dev, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ref{Int64}),
        b.h.ptr, devptr(d_nz), info), b.h)
    _invalidate!(b)
    return info[]                                   # 0, or the elimination step of the first non-positive pivot
end

# workspace_solve on a stale factorisation, everything in HBM: the call bench.py times (gmrfx_refactorize_solve_dev)
function refactorize_solve!(X::ROCMatrix{Float64}, b::MI355XBackend, d_nz::ROCVector{Float64}, B::ROCMatrix{Float64})
    size(B, 1) == b.n && size(X) == size(B) || throw(DimensionMismatch("B / X must be n x k"))
    AMDGPU.synchronize()
    info = Ref{Int64}(0)
    GC.@preserve d_nz B X check(ccall((:gmrfx_refactorize_solve_dev, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ref{Int64}),
        b.h.ptr, devptr(d_nz), devptr(B), stride(B, 2), size(B, 2), devptr(X), stride(X, 2), info), b.h)
    _invalidate!(b)
    info[] > 0 && throw(PosDefException(Int(info[])))      # (as `b.factor \ rhs` does on a failed CHOLMOD factor: backend.jl:178-193)
    return X
end

function backend_solve!(X::ROCMatrix{Float64}, b::MI355XBackend, B::ROCMatrix{Float64})
    size(B, 1) == b.n && size(X) == size(B) || throw(DimensionMismatch("B / X must be n x k"))
    AMDGPU.synchronize()
    GC.@preserve B X check(ccall((:gmrfx_solve_dev, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64),
        b.h.ptr, devptr(B), stride(B, 2), size(B, 2), devptr(X), stride(X, 2)), b.h)
    return X
end

# k samples x = P' L^-T z in one sweep (src/gmrf.jl:271-281 draws them one by one)
function backend_backward_solve!(X::ROCMatrix{Float64}, b::MI355XBackend, Z::ROCMatrix{Float64})
    size(Z, 1) == b.n && size(X) == size(Z) || throw(DimensionMismatch("Z / X must be n x k"))
    AMDGPU.synchronize()
    GC.@preserve Z X check(ccall((:gmrfx_backward_solve_dev, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64),
        b.h.ptr, devptr(Z), stride(Z, 2), size(Z, 2), devptr(X), stride(X, 2)), b.h)
    return X
end

# one evaluation of the hyper-parameter loop: new values -> factorisation, (x_k - mean)' Q (x_k - mean) for every column of X and
# log det Q in one call; logpdf_k = -q_k / 2 + logdet / 2 - n log(2 pi) / 2 (workspace_gmrf.jl:288-292)
function logpdf_terms(b::MI355XBackend, d_nz::ROCVector{Float64}, X::ROCMatrix{Float64}; mean::Union{Nothing, ROCVector{Float64}} = nothing)
    size(X, 1) == b.n || throw(DimensionMismatch("X must be n x k"))
    AMDGPU.synchronize()
    quad = Vector{Float64}(undef, size(X, 2))
    ld = Ref{Float64}(0.0)
    info = Ref{Int64}(0)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : devptr(mean)
    GC.@preserve d_nz X mean quad check(ccall((:gmrfx_refactorize_logpdf_dev, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Int64}),
        b.h.ptr, devptr(d_nz), devptr(X), stride(X, 2), size(X, 2), mu, quad, ld, info), b.h)
    _invalidate!(b)
    return quad, ld[]
end


# the batched, constrained evaluation with everything resident in HBM (gmrfx_batch_constrained_logpdf_dev): d_nz nnz x B, Z n x B,
# mean n x B -> (logdet, quad, log_correction, info, cinfo), each of length B
function constrained_logpdf_terms(bb::MI355XBatch, d_nz::ROCMatrix{Float64}, Z::ROCMatrix{Float64}; mean::Union{Nothing, ROCMatrix{Float64}} = nothing)
    size(d_nz) == (bb.nnz, bb.nbatch) || throw(DimensionMismatch("d_nz must be nnz x nbatch"))
    size(Z) == (bb.n, bb.nbatch) || throw(DimensionMismatch("Z must be n x nbatch"))
    mean === nothing || size(mean) == (bb.n, bb.nbatch) || throw(DimensionMismatch("mean must be n x nbatch"))
    AMDGPU.synchronize()
    quad = Vector{Float64}(undef, bb.nbatch); ld = similar(quad); lc = similar(quad)
    cinfo = zeros(Int64, bb.nbatch)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : devptr(mean)
    GC.@preserve d_nz Z mean quad ld lc cinfo check(ccall((:gmrfx_batch_constrained_logpdf_dev, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}),
        bb.h.ptr, devptr(d_nz), devptr(Z), bb.n, bb.n, 1, mu, quad, ld, lc, bb.info, cinfo), bb.h)
    return ld, quad, lc, copy(bb.info), cinfo
end

# ---- one factorisation over several GPUs: the native RCCL driver (libgmrfx_rccl.so) with operands resident in HBM ----
function refactorize!(sf::ShardedMI355X, d_nz::ROCVector{Float64})
    AMDGPU.synchronize()
    GC.@preserve d_nz check_rccl(ccall((:gmrfx_rccl_refactorize, LIB_RCCL), Int32, (Ptr{Cvoid}, Ptr{Float64}), sf.drv, devptr(d_nz)), sf)
    return sf
end

# Q X = B over all ranks; gather = true: all of X on rank 0, false: every rank keeps the rows it owns (+ every top front's)
function solve!(X::ROCMatrix{Float64}, sf::ShardedMI355X, B::ROCMatrix{Float64}; gather::Bool = true)
    size(B, 1) == sf.n && size(X) == size(B) || throw(DimensionMismatch("B / X must be n x k"))
    AMDGPU.synchronize()
    GC.@preserve B X check_rccl(ccall((:gmrfx_rccl_solve, LIB_RCCL), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int32),
        sf.drv, devptr(B), stride(B, 2), size(B, 2), devptr(X), stride(X, 2), gather ? 1 : 0), sf)
    return X
end

# RBMC marginal variances with Z (n x k standard normals) and the result in HBM (src/solvers/rbmc.jl:71-87, :124-158); Q's values are
# those of the last refactorisation
function rbmc_var_dev!(out::ROCVector{Float64}, b::MI355XBackend, Z::ROCMatrix{Float64}; enclosure_size::Integer = -1)
    size(Z, 1) == b.n && length(out) == b.n || throw(DimensionMismatch("Z must be n x k, out of length n"))
    AMDGPU.synchronize()
    GC.@preserve Z out check(ccall((:gmrfx_rbmc_var_dev, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int32, Ptr{Float64}),
        b.h.ptr, C_NULL, devptr(Z), stride(Z, 2), size(Z, 2), enclosure_size, devptr(out)), b.h)
    return out
end

# The gradient of logpdf (+ log_correction) with everything resident in HBM (gmrfx_logpdf_grad_dev): Qbar (nnz, in the pattern's order)
# and mubar (n) are written in place; Q's values are those of the last refactorisation unless d_nz is given
function logpdf_grad_dev!(Qbar::ROCVector{Float64}, mubar::ROCVector{Float64}, b::MI355XBackend, z::ROCVector{Float64};
                          mean::Union{Nothing, ROCVector{Float64}} = nothing, ybar::Real = 1.0, d_nz::Union{Nothing, ROCVector{Float64}} = nothing)
    length(z) == b.n && length(mubar) == b.n || throw(DimensionMismatch("z and mubar must have n entries"))
    AMDGPU.synchronize()
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : devptr(mean)
    nz = d_nz === nothing ? Ptr{Float64}(C_NULL) : devptr(d_nz)
    GC.@preserve Qbar mubar z mean d_nz check(ccall((:gmrfx_logpdf_grad_dev, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}),
        b.h.ptr, nz, devptr(z), mu, Float64(ybar), devptr(Qbar), devptr(mubar)), b.h)
    return Qbar, mubar
end
# one evaluation of a Fisher-scoring iterate with everything resident in HBM: score and hess are written, (energy, loglik) returned
function fisher_eval_dev!(score::ROCVector{Float64}, hess::ROCVector{Float64}, b::MI355XBackend, x::ROCVector{Float64};
                          mean::Union{Nothing, ROCVector{Float64}} = nothing)
    length(x) == b.n && length(score) == b.n && length(hess) == b.n || throw(DimensionMismatch("x, score and hess must have n entries"))
    AMDGPU.synchronize()
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : devptr(mean)
    out = zeros(2)
    GC.@preserve score hess x mean out check(ccall((:gmrfx_fisher_eval_dev, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        b.h.ptr, devptr(x), mu, devptr(score), devptr(hess), out), b.h)
    return out[1], out[2]
end
# the whole loop with the mode and the final Hessian written to ROCArrays; mean and x0 resident in HBM as well; returns the info tuple
function gaussian_approximation_dev!(x::ROCVector{Float64}, hess::ROCVector{Float64}, b::MI355XBackend;
                                     mean::Union{Nothing, ROCVector{Float64}} = nothing, x0::Union{Nothing, ROCVector{Float64}} = nothing,
                                     max_iter::Int = 50, mean_change_tol::Real = 1.0e-4, newton_dec_tol::Real = 1.0e-5,
                                     adaptive_stepsize::Bool = true, max_linesearch_iter::Int = 10, step_recovery::Symbol = :retry_full,
                                     predictive_convergence::Bool = true, refactorize_final::Bool = false)
    length(x) == b.n && length(hess) == b.n || throw(DimensionMismatch("x and hess must have n entries"))
    AMDGPU.synchronize()
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : devptr(mean)
    xs = x0 === nothing ? Ptr{Float64}(C_NULL) : devptr(x0)
    res = zeros(8); dec = fill(NaN, max_iter + 1); alp = fill(NaN, max_iter + 1); info = Ref{Int64}(0)
    flags = _ga_flags(adaptive_stepsize, step_recovery, predictive_convergence, refactorize_final)
    code = GC.@preserve x hess mean x0 res dec alp ccall((:gmrfx_gaussian_approximation_dev, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}),
        b.h.ptr, mu, xs, max_iter, max_linesearch_iter, Float64(mean_change_tol), Float64(newton_dec_tol), flags, devptr(x), devptr(hess), res, dec, alp, info)
    _invalidate!(b)
    info[] > 0 && throw(PosDefException(Int(info[])))
    check(code, b.h)
    return _ga_info(res, dec, alp)
end
# the pullback of gaussian_approximation with everything resident in HBM (gmrfx_ga_pullback_dev): Qbar_prior (nnz; may be Qbar itself),
# mubar_prior and lambda (n) are written, each optional; returns (param_bar, lambda' xbar)
function ga_pullback_dev!(b::MI355XBackend, x::ROCVector{Float64}; mean::Union{Nothing, ROCVector{Float64}} = nothing,
                          mubar::Union{Nothing, ROCVector{Float64}} = nothing, Qbar::Union{Nothing, ROCVector{Float64}} = nothing,
                          Qbar_prior::Union{Nothing, ROCVector{Float64}} = nothing, mubar_prior::Union{Nothing, ROCVector{Float64}} = nothing,
                          lambda::Union{Nothing, ROCVector{Float64}} = nothing, project::Bool = false, refactorize::Bool = false)
    length(x) == b.n || throw(DimensionMismatch("x must have n entries"))
    AMDGPU.synchronize()
    p(a) = a === nothing ? Ptr{Float64}(C_NULL) : devptr(a)
    out = zeros(2)
    flags = Int32(project) | (Int32(refactorize) << 1)
    code = GC.@preserve x mean mubar Qbar Qbar_prior mubar_prior lambda out ccall((:gmrfx_ga_pullback_dev, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        b.h.ptr, devptr(x), p(mean), p(mubar), p(Qbar), flags, p(Qbar_prior), p(mubar_prior), p(lambda), out)
    refactorize && _invalidate!(b)
    check(code, b.h)
    return out[1], out[2]
end
# the same for a composite likelihood (gmrfx_ga_pullback_composite_dev); returns (param_bar per component, lambda' xbar)
function ga_pullback_composite_dev!(b::MI355XBackend, x::ROCVector{Float64}; mean::Union{Nothing, ROCVector{Float64}} = nothing,
                                    mubar::Union{Nothing, ROCVector{Float64}} = nothing, Qbar::Union{Nothing, ROCVector{Float64}} = nothing,
                                    Qbar_prior::Union{Nothing, ROCVector{Float64}} = nothing, mubar_prior::Union{Nothing, ROCVector{Float64}} = nothing,
                                    lambda::Union{Nothing, ROCVector{Float64}} = nothing, project::Bool = false, refactorize::Bool = false)
    length(x) == b.n || throw(DimensionMismatch("x must have n entries"))
    AMDGPU.synchronize()
    p(a) = a === nothing ? Ptr{Float64}(C_NULL) : devptr(a)
    par = zeros(max(length(composite_info(b).family), 1)); chk = Ref{Float64}(0.0)
    flags = Int32(project) | (Int32(refactorize) << 1)
    code = GC.@preserve x mean mubar Qbar Qbar_prior mubar_prior lambda par ccall((:gmrfx_ga_pullback_composite_dev, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
        b.h.ptr, devptr(x), p(mean), p(mubar), p(Qbar), flags, p(Qbar_prior), p(mubar_prior), p(lambda), par, chk)
    refactorize && _invalidate!(b)
    check(code, b.h)
    return par, chk[]
end
# the same for the members of a batch (gmrfx_batch_ga_pullback_dev): X / mean / mubar / mubar_prior / lambda n x B, Qbar / Qbar_prior nnz x B
# (Qbar_prior may be Qbar itself: the Qbar of logpdf_grad_dev! goes in, pattern_dot_dev takes it on); returns (param_bar, lambda' xbar, info)
function ga_pullback_dev!(bb::MI355XBatch, X::ROCMatrix{Float64}; mean::Union{Nothing, ROCMatrix{Float64}} = nothing,
                          mubar::Union{Nothing, ROCMatrix{Float64}} = nothing, Qbar::Union{Nothing, ROCMatrix{Float64}} = nothing,
                          Qbar_prior::Union{Nothing, ROCMatrix{Float64}} = nothing, mubar_prior::Union{Nothing, ROCMatrix{Float64}} = nothing,
                          lambda::Union{Nothing, ROCMatrix{Float64}} = nothing, project::Bool = false, refactorize::Bool = false)
    size(X, 1) == bb.n && size(X, 2) == bb.nbatch || throw(DimensionMismatch("X must be n x nbatch"))
    for a in (mubar, mubar_prior, lambda)
        a === nothing || (size(a) == (bb.n, bb.nbatch) && stride(a, 2) == bb.n) || throw(DimensionMismatch("mubar / mubar_prior / lambda must be dense n x nbatch"))
    end
    for a in (Qbar, Qbar_prior)
        a === nothing || (size(a) == (bb.nnz, bb.nbatch) && stride(a, 2) == bb.nnz) || throw(DimensionMismatch("Qbar / Qbar_prior must be dense nnz x nbatch"))
    end
    AMDGPU.synchronize()
    p(a) = a === nothing ? Ptr{Float64}(C_NULL) : devptr(a)
    out = zeros(2, bb.nbatch); inf = zeros(Int64, bb.nbatch)
    flags = Int32(project) | (Int32(refactorize) << 1)
    smu = mean === nothing ? 0 : stride(mean, 2)
    GC.@preserve X mean mubar Qbar Qbar_prior mubar_prior lambda out inf check(ccall((:gmrfx_batch_ga_pullback_dev, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
        bb.h.ptr, devptr(X), stride(X, 2), p(mean), smu, p(mubar), p(Qbar), flags, p(Qbar_prior), p(mubar_prior), p(lambda), out, inf), bb.h)
    return out[1, :], out[2, :], inf
end
# the members of a batch: Qbar nnz x B, mubar / Z / mean n x B; returns info
function logpdf_grad_dev!(Qbar::ROCMatrix{Float64}, mubar::ROCMatrix{Float64}, bb::MI355XBatch, Z::ROCMatrix{Float64}, ybar::Vector{Float64};
                          mean::Union{Nothing, ROCMatrix{Float64}} = nothing, d_nz::Union{Nothing, ROCMatrix{Float64}} = nothing)
    size(Z) == (bb.n, bb.nbatch) && size(mubar) == (bb.n, bb.nbatch) && size(Qbar) == (bb.nnz, bb.nbatch) && length(ybar) == bb.nbatch ||
        throw(DimensionMismatch("Z / mubar n x nbatch, Qbar nnz x nbatch, ybar of length nbatch"))
    AMDGPU.synchronize()
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : devptr(mean)
    nz = d_nz === nothing ? Ptr{Float64}(C_NULL) : devptr(d_nz)
    inf = zeros(Int64, bb.nbatch)
    GC.@preserve Qbar mubar Z mean d_nz ybar inf check(ccall((:gmrfx_batch_logpdf_grad_dev, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
        bb.h.ptr, nz, devptr(Z), stride(Z, 2), mu, ybar, devptr(Qbar), devptr(mubar), inf), bb.h)
    return inf
end
# dlogpdf/dtheta from Qbar's values and the Jacobian of Q's values, both in HBM: p numbers come back
function pattern_dot_dev(b::MI355XBackend, G::ROCVector{Float64}, J::ROCMatrix{Float64})
    size(J, 1) == length(G) || throw(DimensionMismatch("J must have one row per stored entry"))
    AMDGPU.synchronize()
    out = Vector{Float64}(undef, size(J, 2))
    GC.@preserve G J out check(ccall((:gmrfx_pattern_dot_dev, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}),
        b.h.ptr, devptr(G), devptr(J), max(stride(J, 2), 1), size(J, 2), out), b.h)
    return out
end
function pattern_dot_dev(bb::MI355XBatch, G::ROCMatrix{Float64}, J::ROCArray{Float64, 3})
    size(G) == (bb.nnz, bb.nbatch) && size(J, 1) == bb.nnz && size(J, 3) == bb.nbatch || throw(DimensionMismatch("G nnz x nbatch, J nnz x p x nbatch"))
    AMDGPU.synchronize()
    p = size(J, 2)
    out = Matrix{Float64}(undef, p, bb.nbatch)
    GC.@preserve G J out check(ccall((:gmrfx_batch_pattern_dot_dev, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}),
        bb.h.ptr, devptr(G), devptr(J), max(bb.nnz, 1), bb.nnz * p, p, out), bb.h)
    return out
end

# X = P' L^-T Z over all ranks (samples: Z in elimination order, as CHOLMOD's F.UP \ z takes it)
function backend_backward_solve!(X::ROCMatrix{Float64}, sf::ShardedMI355X, Z::ROCMatrix{Float64}; gather::Bool = true)
    size(Z, 1) == sf.n && size(X) == size(Z) || throw(DimensionMismatch("Z / X must be n x k"))
    AMDGPU.synchronize()
    GC.@preserve Z X check_rccl(ccall((:gmrfx_rccl_backward_solve, LIB_RCCL), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int32),
        sf.drv, devptr(Z), stride(Z, 2), size(Z, 2), devptr(X), stride(X, 2), gather ? 1 : 0), sf)
    return X
end

end # module
