# GMRFX.jl -- thin ccall layer over libgmrfx.so (include/gmrfx.h), and the two plug-ins that attach
# it to GaussianMarkovRandomFields.jl:
#   * seam B: `MI355XBackend <: WorkspaceBackend`            (src/workspace/backend.jl:8-30)
#   * seam A: `MI355XCholesky` LinearSolve algorithm + hooks  (ext/GaussianMarkovRandomFieldsPardiso.jl:10-80)
# NOTE: this image has no Julia; the same call sequences are exercised by the Python ctypes binding
# (gmrfx/_lib.py, gmrfx/backend.py) and the test mirrors of the host code above the seams
# (tests/mirror/workspace.py = seam B state machine, tests/mirror/linsolve.py = seam A: `MI355XCacheval`,
# `solve!`, the hooks below, `deepcopy(cache)`). Keep them in sync.
module GMRFX

using LinearAlgebra, SparseArrays, Random
import LinearAlgebra: logdet      # extended for the owned MI355XBatch only (batched handles below)
import Distributions
import GaussianMarkovRandomFields as G
import GaussianMarkovRandomFields: WorkspaceBackend, refactorize!, backend_solve, compute_logdet,
    compute_selinv!, get_selinv, get_selinv_diag, backend_backward_solve, selinv_dot, selinv_extract_at,
    GMRFWorkspace

const LIB = get(ENV, "GMRFX_LIB", joinpath(@__DIR__, "..", "libgmrfx.so"))

Base.@kwdef struct Opts            # mirrors gmrfx_opts
    struct_size::Int32 = 0
    uplo::Int32 = 0
    ordering::Int32 = 0
    device::Int32 = -1
    symbolic_only::Int32 = 0
    check_posdef::Int32 = 0
    nd_leaf::Int32 = 0
    relax_cols::Int32 = 0
    relax_zeros::Float64 = 0.0
    coord_dim::Int32 = 0
    reserved0::Int32 = 0
    coords::Ptr{Float64} = C_NULL
    shard_rank::Int32 = 0          # one factorisation sharded over several GPUs (include/gmrfx.h); 0 / 1 = unsharded
    shard_world::Int32 = 1
    shard_min_top::Int32 = 0       # > 0: at least this many top fronts; with shard_world == 1 a sharded handle of one rank (testing)
    reserved1::Int32 = 0
end

mutable struct Handle
    ptr::Ptr{Cvoid}
    function Handle(p)
        h = new(p)
        finalizer(x -> (x.ptr == C_NULL || ccall((:gmrfx_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.ptr); x.ptr = C_NULL), h)
        return h
    end
end

function check(code::Int32, h::Union{Handle, Nothing} = nothing)
    code == 0 && return nothing
    msg = h === nothing ? unsafe_string(ccall((:gmrfx_last_create_error, LIB), Cstring, ())) :
        unsafe_string(ccall((:gmrfx_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr))
    code == 1 && throw(ArgumentError(msg))
    code == 5 && throw(PosDefException(1))
    error("gmrfx error $code: $msg")
end

# `ordering` (src/workspace/backend.jl:73-153): nothing -> libgmrfx's own nested dissection; :natural; a permutation
# vector; anything else CliqueTrees accepts (an EliminationAlgorithm such as CliqueTrees.MMD(), an (order, index)
# tuple) or a `PinDenseColumns` wrapper is resolved ONCE by the reference's own `ordering_permutation(A, ordering)`
# (backend.jl:86-133) and reaches the library as an explicit permutation. Nothing is dropped silently: whatever
# that resolver rejects throws there.
resolve_ordering(Q, ordering::Nothing) = nothing
resolve_ordering(Q, ordering::Symbol) = ordering === :natural ? nothing : throw(ArgumentError("unknown ordering $ordering"))
resolve_ordering(Q, ordering::AbstractVector{<:Integer}) = Vector{Int}(ordering)
resolve_ordering(Q, ordering) = Vector{Int}(G.ordering_permutation(Q, ordering))

function create(Q::SparseMatrixCSC{Float64, Int}; ordering = nothing, coords = nothing, device = -1,
        check_posdef = false, shard_rank = 0, shard_world = 1, shard_min_top = 0)
    n = size(Q, 1)
    perm = resolve_ordering(Q, ordering)
    perm === nothing || isperm(perm) && length(perm) == n || throw(ArgumentError("ordering is not a permutation of 1:$n"))
    C = coords === nothing ? nothing : Matrix{Float64}(transpose(coords))     # dim x n == n x dim row-major
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Q perm C begin
        o = Opts(struct_size = sizeof(Opts), device = device, check_posdef = check_posdef,
            shard_rank = shard_rank, shard_world = shard_world, shard_min_top = shard_min_top,
            ordering = ordering === :natural ? 1 : 0,
            coord_dim = C === nothing ? 0 : size(C, 1), coords = C === nothing ? C_NULL : pointer(C))
        check(ccall((:gmrfx_create, LIB), Int32,
            (Int64, Ptr{Int64}, Ptr{Int64}, Int32, Ptr{Int64}, Ref{Opts}, Ref{Ptr{Cvoid}}),
            n, SparseArrays.getcolptr(Q), rowvals(Q), 1, perm === nothing ? C_NULL : pointer(perm), Ref(o), out))
    end
    return Handle(out[])
end

# ---------------------------------------------------------------------------------- seam B
mutable struct MI355XBackend <: WorkspaceBackend
    h::Handle
    n::Int
    selinv_cache::Union{Nothing, SparseMatrixCSC{Float64, Int}}
    selinv_diag_cache::Union{Nothing, Vector{Float64}}
end

function MI355XBackend(Q::Symmetric{Float64, <:SparseMatrixCSC{Float64}}; ordering = nothing, coords = nothing, device = -1)
    A = parent(Q)                                   # both triangles stored; uplo=:U defines Q
    b = MI355XBackend(create(A; ordering, coords, device), size(A, 1), nothing, nothing)
    refactorize!(b, Q)
    return b
end

function refactorize!(b::MI355XBackend, Q::Symmetric)
    nz = nonzeros(parent(Q))
    info = Ref{Int64}(0)
    GC.@preserve nz check(ccall((:gmrfx_refactorize, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ref{Int64}), b.h.ptr, nz, info), b.h)
    b.selinv_cache = nothing
    b.selinv_diag_cache = nothing
    return nothing                                  # never throws on indefiniteness (backend.jl:184)
end

# workspace_solve(ws, B) on a workspace whose values were just updated (gmrf_workspace.jl:170-178, 207-215: ensure_numeric! then
# backend_solve) as ONE pipelined call: the forward sweep follows the factorisation up the tree on a side stream. The host
# transfers are SERIAL -- B goes up in front of the factorisation (staged through page-locked memory by host threads when
# pageable), X comes down in slices behind the backward sweep (csrc/device.cpp, host_upload / host_download: a transfer beside
# the factorisation slows its launch chain by more than it hides). Same bits as refactorize! + backend_solve.
# The reference's workspace_solve ends in `b.factor \ rhs`, which throws PosDefException on a failed factor (backend.jl:178-193):
# so does this call -- a non-positive pivot never comes back as a silent NaN solution.
function refactorize_solve!(b::MI355XBackend, Q::Symmetric, rhs::AbstractVecOrMat)
    nz = nonzeros(parent(Q))
    B = Matrix{Float64}(reshape(rhs, b.n, :)); X = similar(B)
    info = Ref{Int64}(0)
    GC.@preserve nz B X check(ccall((:gmrfx_refactorize_solve, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ref{Int64}),
        b.h.ptr, nz, B, b.n, size(B, 2), X, b.n, info), b.h)
    b.selinv_cache = nothing
    b.selinv_diag_cache = nothing
    info[] > 0 && throw(PosDefException(Int(info[])))
    return rhs isa AbstractVector ? vec(X) : X
end

# The reference's workspace_solve (gmrf_workspace.jl:207-215) for workspaces on this backend: a STALE factorisation and the solve
# behind it go down as the one pipelined call above (this is the call bench.py times, through the host entry point); a current
# factorisation is a plain backend_solve. Two methods, as in the reference (one AbstractVecOrMat method would be ambiguous with its).
function _workspace_solve(ws::GMRFWorkspace, B::AbstractVecOrMat)
    ws.numeric_valid && return backend_solve(ws.backend, B isa AbstractVector ? B : Matrix{Float64}(B))
    X = refactorize_solve!(ws.backend, Symmetric(ws.Q), B)          # = ensure_numeric!(ws) + backend_solve(ws.backend, B); throws on a failed factor
    ws.numeric_valid = true
    ws.selinv_valid = false
    ws.logdet_valid = false
    return X
end
G.workspace_solve(ws::GMRFWorkspace{<:Any, MI355XBackend}, b::AbstractVector) = _workspace_solve(ws, b)
G.workspace_solve(ws::GMRFWorkspace{<:Any, MI355XBackend}, B::AbstractMatrix) = _workspace_solve(ws, B)

# Device-resident operands (the *_dev entry points of include/gmrfx.h) are bound for AMDGPU.jl's ROCArray in the package
# extension ext/GMRFXAMDGPUExt.jl (weak dependency: loaded when AMDGPU is): refactorize!(b, d_nz), refactorize_solve!(X, b, d_nz, B),
# backend_solve!(X, b, B), backend_backward_solve!(X, b, Z), logpdf_terms(b, d_nz, X; mean).
function backend_solve! end
function backend_backward_solve! end
function logpdf_terms end

function backend_solve(b::MI355XBackend, rhs::AbstractVector)
    B = Vector{Float64}(rhs); X = similar(B)
    GC.@preserve B X check(ccall((:gmrfx_solve, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64),
        b.h.ptr, B, b.n, 1, X, b.n), b.h)
    return X
end
function backend_solve(b::MI355XBackend, RHS::Matrix{Float64})
    X = similar(RHS)
    GC.@preserve RHS X check(ccall((:gmrfx_solve, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64),
        b.h.ptr, RHS, stride(RHS, 2), size(RHS, 2), X, stride(X, 2)), b.h)
    return X
end

function compute_logdet(b::MI355XBackend)
    out = Ref{Float64}(0)
    check(ccall((:gmrfx_logdet, LIB), Int32, (Ptr{Cvoid}, Ref{Float64}), b.h.ptr, out), b.h)
    return out[]
end

compute_selinv!(b::MI355XBackend) = nothing         # lazy, like CHOLMODBackend (backend.jl:215-221)

function get_selinv(b::MI355XBackend)
    if b.selinv_cache === nothing
        nnzr = Ref{Int64}(0)
        check(ccall((:gmrfx_selinv_nnz, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), b.h.ptr, nnzr), b.h)
        colptr = Vector{Int}(undef, b.n + 1); rv = Vector{Int}(undef, nnzr[]); nz = Vector{Float64}(undef, nnzr[])
        GC.@preserve colptr rv nz check(ccall((:gmrfx_selinv_csc, LIB), Int32,
            (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}), b.h.ptr, 1, colptr, rv, nz), b.h)
        b.selinv_cache = SparseMatrixCSC(b.n, b.n, colptr, rv, nz)
    end
    return b.selinv_cache
end

function get_selinv_diag(b::MI355XBackend)
    if b.selinv_diag_cache === nothing
        d = Vector{Float64}(undef, b.n)
        GC.@preserve d check(ccall((:gmrfx_selinv_diag, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), b.h.ptr, d), b.h)
        b.selinv_diag_cache = d
    end
    return b.selinv_diag_cache
end

function selinv_extract_at(b::MI355XBackend, B::SparseMatrixCSC)
    out = Vector{Float64}(undef, nnz(B))
    cp = Vector{Int}(SparseArrays.getcolptr(B)); rv = Vector{Int}(rowvals(B))
    GC.@preserve cp rv out check(ccall((:gmrfx_selinv_extract, LIB), Int32,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Int32, Ptr{Float64}), b.h.ptr, b.n, cp, rv, 1, out), b.h)
    return SparseMatrixCSC(size(B)..., cp, rv, out)
end
# values of Sigma are gathered on the GPU; the contraction stays in Julia so B may carry Duals
selinv_dot(b::MI355XBackend, B::SparseMatrixCSC) = dot(nonzeros(selinv_extract_at(b, B)), nonzeros(B))

# Float64 B: contracted on the device. Anything else (ForwardDiff.Dual values): gather Sigma on B's pattern and
# contract in Julia, as the generic fallback does.
function selinv_dot(b::MI355XBackend, B::SparseMatrixCSC{Float64, Int})
    out = Ref{Float64}(0.0)
    cp, rv, nz = B.colptr, B.rowval, B.nzval
    GC.@preserve cp rv nz check(ccall((:gmrfx_selinv_dot, LIB), Int32,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int32, Ref{Float64}),
        b.h.ptr, size(B, 2), cp, rv, nz, 1, out), b.h)
    return out[]
end
selinv_dot(b::MI355XBackend, B::AbstractMatrix) = dot(selinv_extract_at(b, sparse(B)), B)

# diag(A * Sigma * A') for a sparse design matrix (rows of A = columns of At): src/linear_predictor_marginals.jl:125-165
function row_diag_AΣAt(b::MI355XBackend, A::SparseMatrixCSC{Float64, Int})
    At = sparse(transpose(A))
    out = Vector{Float64}(undef, size(A, 1))
    cp, rv, nz = At.colptr, At.rowval, At.nzval
    GC.@preserve cp rv nz out check(ccall((:gmrfx_selinv_row_diag, LIB), Int32,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Float64}),
        b.h.ptr, size(A, 1), cp, rv, nz, 1, out), b.h)
    return out
end

function backend_backward_solve(b::MI355XBackend, x::AbstractVector)
    Z = Vector{Float64}(x); X = similar(Z)          # copies views (backend.jl:282-283)
    GC.@preserve Z X check(ccall((:gmrfx_backward_solve, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64),
        b.h.ptr, Z, b.n, 1, X, b.n), b.h)
    return X
end
# batched sampling: k samples in one sweep instead of the reference's k single-RHS solves (src/gmrf.jl:271-281)
function backend_backward_solve(b::MI355XBackend, Zm::Matrix{Float64})
    X = similar(Zm)
    GC.@preserve Zm X check(ccall((:gmrfx_backward_solve, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64),
        b.h.ptr, Zm, stride(Zm, 2), size(Zm, 2), X, stride(X, 2)), b.h)
    return X
end

# ---- rand(d, k): k samples in ONE backward sweep ------------------------------------------------------------------------------
# The reference's `_rand!` takes one vector (src/gmrf.jl:271-281, src/workspace/workspace_gmrf.jl:275-286) and Distributions' matrix
# method `_rand!(rng, d, X::AbstractMatrix)` loops it over the columns: rand(d, 256) is 256 single-RHS sweeps with 256 host round
# trips. On this backend the matrix method is ONE `backend_backward_solve(b, Z::Matrix)`: randn! fills Z column by column in the
# order the column loop would draw it, so the same rng gives the same samples (to 1e-12: a wide pass and a one-column pass take kernels
# that add the same terms in different orders: tests/mirror/workspace_gmrf.py, tests/test_seam_a_and_constraints.py); the mean and the constraint correction
# (x -= A~' (L_c \ (A x - e)), workspace_gmrf.jl:280-284) are applied to all columns at once.
function Distributions._rand!(rng::AbstractRNG, d::G.WorkspaceGMRF{<:Any, MI355XBackend}, X::AbstractMatrix{<:Real})
    G.ensure_loaded!(d)
    Z = randn!(rng, Matrix{Float64}(undef, size(X, 1), size(X, 2)))
    G.ensure_numeric!(d.workspace)
    b = d.workspace.backend
    if d.constraints === nothing || size(d.constraints.matrix, 1) <= MAX_DEVICE_CONSTRAINTS
        # mean and constraint correction on the device, in the same call as the sweep (gmrfx_sample): nothing but Z and X crosses
        sync_constraints!(b, d.constraints)
        X .= sample(b, Z, Vector{Float64}(d.mean))
        return X
    end
    # more than 64 constraint rows: the generic host arithmetic (workspace_gmrf.jl:280-284 on all columns at once)
    sync_constraints!(b, nothing)
    Y = backend_backward_solve(d.workspace.backend, Z)
    Y .+= d.mean
    ci = d.constraints
    Y .-= ci.A_tilde_T * (ci.L_c \ (ci.matrix * Y .- ci.vector))
    X .= Y
    return X
end

# ---- linear equality constraints on the device (include/gmrfx.h "linear equality constraints") ----------------------------------
# The reference keeps A, e and what it derives from them in ConstraintInfo (src/workspace/workspace_gmrf.jl:22-56) and applies them on
# the host. Here A and e become state of the handle (gmrfx_constraints_set: m <= 64 rows); A~' = Q^-1 A', W = A A~', L_c and
# B = A~' L_c^-T are built on the device once per factorisation, and the corrections of `_rand!` (:280-284) and `var` (:260-273) run there.
const MAX_DEVICE_CONSTRAINTS = 64
const CONSTRAINT_KEYS = WeakKeyDict{Any, UInt}()      # backend -> objectid of the ConstraintInfo its handle holds (0: none)

function set_constraints!(b::MI355XBackend, A::AbstractMatrix, e::AbstractVector)
    At = sparse(transpose(sparse(A)))                 # CSC of A' = CSR of A
    cp = Vector{Int}(SparseArrays.getcolptr(At)); rv = Vector{Int}(rowvals(At)); nz = Vector{Float64}(nonzeros(At))
    ev = Vector{Float64}(e)
    size(A, 2) == b.n || throw(ArgumentError("Constraint matrix size $(size(A)) incompatible with workspace size $(b.n)"))
    size(A, 1) == length(ev) || throw(ArgumentError("Constraint matrix rows $(size(A, 1)) != constraint vector length $(length(ev))"))
    GC.@preserve cp rv nz ev check(ccall((:gmrfx_constraints_set, LIB), Int32,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Float64}), b.h.ptr, size(A, 1), cp, rv, nz, 1, ev), b.h)
    return nothing
end
function clear_constraints!(b::MI355XBackend)
    check(ccall((:gmrfx_constraints_set, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Float64}),
        b.h.ptr, 0, C_NULL, C_NULL, C_NULL, 1, C_NULL), b.h)
    return nothing
end
# the handle holds the constraint of `ci` (a ConstraintInfo, or nothing): set once per (backend, ConstraintInfo) pair
function sync_constraints!(b::MI355XBackend, ci)
    key = ci === nothing ? UInt(0) : objectid(ci)
    get(CONSTRAINT_KEYS, b, UInt(0)) == key && return nothing
    ci === nothing ? clear_constraints!(b) : set_constraints!(b, ci.matrix, ci.vector)
    CONSTRAINT_KEYS[b] = key
    return nothing
end
function constraint_info(b::MI355XBackend)
    m = Ref{Int64}(0); ldw = Ref{Float64}(0); lda = Ref{Float64}(0); ms = Ref{Float64}(0)
    check(ccall((:gmrfx_constraints_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Float64}, Ref{Float64}, Ref{Float64}),
        b.h.ptr, m, ldw, lda, ms), b.h)
    return (m = Int(m[]), logdet_W = ldw[], logdet_AAt = lda[], ms = ms[])
end
# (A_tilde_T, W): the fields of ConstraintInfo; L_c = cholesky(Symmetric(W))
function constraint_fields(b::MI355XBackend)
    m = constraint_info(b).m
    At = Matrix{Float64}(undef, b.n, m); W = Matrix{Float64}(undef, m, m)
    GC.@preserve At W check(ccall((:gmrfx_constraints_get, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}),
        b.h.ptr, At, b.n, W), b.h)
    return At, W
end
function constrained_mean(b::MI355XBackend, mu::Vector{Float64})
    out = Vector{Float64}(undef, b.n); lc = Ref{Float64}(0)
    GC.@preserve mu out check(ccall((:gmrfx_constraints_mean, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
        b.h.ptr, mu, out, lc), b.h)
    return out, lc[]
end
function constraint_correct!(b::MI355XBackend, X::StridedVecOrMat{Float64})
    GC.@preserve X check(ccall((:gmrfx_constraints_correct, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64),
        b.h.ptr, X, X isa AbstractVector ? b.n : stride(X, 2), size(X, 2)), b.h)
    return X
end
function constrained_var(b::MI355XBackend)
    out = Vector{Float64}(undef, b.n)
    GC.@preserve out check(ccall((:gmrfx_constraints_var, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), b.h.ptr, out), b.h)
    return out
end
# Rao-Blackwellised Monte Carlo marginal variances on given standard-normal draws Z (n x k): `var(d, RBMCStrategy(k))`
# (enclosure_size = -1) / `var(d, BlockRBMCStrategy(k; enclosure_size))`, src/solvers/rbmc.jl:71-87, :124-158 -- there k single-vector
# rand! calls, a host SpMM and one CHOLMOD factorisation per block; here one call on the values of the last refactorisation.
function rbmc_var(b::MI355XBackend, Z::Matrix{Float64}; enclosure_size::Integer = -1)
    size(Z, 1) == b.n || throw(DimensionMismatch("Z must be n x k"))
    out = Vector{Float64}(undef, b.n)
    GC.@preserve Z out check(ccall((:gmrfx_rbmc_var, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int32, Ptr{Float64}),
        b.h.ptr, C_NULL, Z, stride(Z, 2), size(Z, 2), enclosure_size, out), b.h)
    return out
end
function rbmc_var_dev! end      # ROCArray method: ext/GMRFXAMDGPUExt.jl

# The arithmetic of the logpdf / logdetcov pullbacks (src/autodiff/logpdf.jl:63-90, src/workspace/autodiff.jl:14-50) on the device and
# on Q's own pattern: (Qbar as a SparseMatrixCSC on the pattern of `Q`, mubar); zbar = -mubar. With a constraint set on the handle the
# two constraint terms of autodiff.jl:24-37 are included. `Q` only lends its pattern (the one the handle was created with); the values
# are those of the last refactorisation.
function logpdf_grad(b::MI355XBackend, Q::SparseMatrixCSC{Float64, Int}, z::Vector{Float64}; mean::Union{Nothing, Vector{Float64}} = nothing,
                     ybar::Real = 1.0)
    length(z) == b.n && size(Q) == (b.n, b.n) || throw(DimensionMismatch("z must have n entries, Q be n x n"))
    hn = Ref{Int64}(0)
    check(ccall((:gmrfx_pattern_nnz, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), b.h.ptr, hn), b.h)
    nnz(Q) == hn[] || throw(DimensionMismatch("Q has $(nnz(Q)) stored entries, the handle's pattern $(hn[]): Q must be the matrix the handle was created with"))
    mean === nothing || length(mean) == b.n || throw(DimensionMismatch("mean must have n entries"))
    qbar = Vector{Float64}(undef, nnz(Q)); mubar = Vector{Float64}(undef, b.n)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    GC.@preserve z mean qbar mubar check(ccall((:gmrfx_logpdf_grad, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}),
        b.h.ptr, C_NULL, z, mu, Float64(ybar), qbar, mubar), b.h)
    return SparseMatrixCSC(b.n, b.n, copy(Q.colptr), copy(Q.rowval), qbar), mubar
end
# out[k] = sum_e w_e G[e] J[e, k] over the stored entries (w_e: the Symmetric(Q) weights of the quadratic form): dlogpdf/dtheta_k from
# G = nonzeros(Qbar) and the Jacobian J (nnz x p) of Q's stored values
function pattern_dot(b::MI355XBackend, G::Vector{Float64}, J::Matrix{Float64})
    size(J, 1) == length(G) || throw(DimensionMismatch("J must have one row per stored entry"))
    out = Vector{Float64}(undef, size(J, 2))
    GC.@preserve G J out check(ccall((:gmrfx_pattern_dot, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}),
        b.h.ptr, G, J, max(stride(J, 2), 1), size(J, 2), out), b.h)
    return out
end
function logpdf_grad_dev! end   # ROCArray methods: ext/GMRFXAMDGPUExt.jl
function pattern_dot_dev end

# Fisher scoring on the device (include/gmrfx.h "Fisher scoring"): the observation likelihood as state of the handle. family: a key of
# OBS_FAMILIES or its id; indices: the observed nodes, 1-based as the reference's `lik.indices` (nothing: every node in order); aux: log
# exposure (Poisson, NegBin) or trials (Binomial); param: sigma / r / phi. An empty y removes the likelihood.
const OBS_FAMILIES = (normal = 0, poisson = 1, bernoulli = 2, binomial = 3, negbin = 4, gamma = 5)
function set_observations!(b::MI355XBackend, family::Union{Symbol, Integer}, y::Vector{Float64};
                           indices::Union{Nothing, Vector{Int64}} = nothing, aux::Union{Nothing, Vector{Float64}} = nothing, param::Real = 0.0)
    fam = family isa Symbol ? getfield(OBS_FAMILIES, family) : Int(family)
    (indices === nothing || length(indices) == length(y)) && (aux === nothing || length(aux) == length(y)) ||
        throw(DimensionMismatch("indices / aux must have one entry per observation"))
    pidx = indices === nothing ? Ptr{Int64}(C_NULL) : pointer(indices)
    paux = aux === nothing ? Ptr{Float64}(C_NULL) : pointer(aux)
    GC.@preserve y indices aux check(ccall((:gmrfx_obs_set, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Int32, Ptr{Float64}, Ptr{Float64}, Float64),
        b.h.ptr, Int32(fam), length(y), pidx, Int32(1), y, paux, Float64(param)), b.h)
    return b
end
function observations_info(b::MI355XBackend)
    fam = Ref{Int32}(0); nobs = Ref{Int64}(0); c = Ref{Float64}(0.0)
    check(ccall((:gmrfx_obs_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int64}, Ref{Float64}), b.h.ptr, fam, nobs, c), b.h)
    return (family = fam[], nobs = nobs[], loglik_const = c[])
end
# The likelihood observed through eta = A x + offset (gmrfx_obs_set_design; the reference's LinearlyTransformedLikelihood): A is handed
# over as Julia holds it (CSC, 1-based). set_prior! then takes observations_hess_map(b) (1-based positions into nzval, ascending),
# and fisher_eval / gaussian_approximation_device return the values of A' D A in that order.
function set_design_observations!(b::MI355XBackend, family::Union{Symbol, Integer}, y::Vector{Float64}, A::SparseMatrixCSC{Float64, Int64};
                                  offset::Union{Nothing, Vector{Float64}} = nothing, aux::Union{Nothing, Vector{Float64}} = nothing,
                                  param::Real = 0.0)
    fam = family isa Symbol ? getfield(OBS_FAMILIES, family) : Int(family)
    size(A) == (length(y), b.n) || throw(DimensionMismatch("A must be nobs x n"))
    (offset === nothing || length(offset) == length(y)) && (aux === nothing || length(aux) == length(y)) ||
        throw(DimensionMismatch("offset / aux must have one entry per observation"))
    poff = offset === nothing ? Ptr{Float64}(C_NULL) : pointer(offset)
    paux = aux === nothing ? Ptr{Float64}(C_NULL) : pointer(aux)
    GC.@preserve y A offset aux check(ccall((:gmrfx_obs_set_design, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64),
        b.h.ptr, Int32(fam), length(y), A.colptr, A.rowval, A.nzval, Int32(1), poff, y, paux, Float64(param)), b.h)
    return b
end
# A composite likelihood (gmrfx_obs_set_composite; the reference's CompositeObservationModel): `families` and `params` per component,
# A the stacked design matrix [A_1; ...; A_C] and `rows` the components' row counts in that order; y, offset and aux go with A's rows.
# The map, set_prior!, fisher_eval, gaussian_approximation_device and the predictive calls are those of the design form.
function set_composite_observations!(b::MI355XBackend, families::Vector{<:Union{Symbol, Integer}}, rows::Vector{<:Integer}, y::Vector{Float64},
                                     A::SparseMatrixCSC{Float64, Int64}; params::Vector{Float64} = zeros(length(families)),
                                     offset::Union{Nothing, Vector{Float64}} = nothing, aux::Union{Nothing, Vector{Float64}} = nothing)
    fam = Int32[f isa Symbol ? getfield(OBS_FAMILIES, f) : Int(f) for f in families]
    length(rows) == length(fam) == length(params) || throw(DimensionMismatch("families, rows and params must have one entry per component"))
    rowptr = Int64[0; cumsum(rows)]
    size(A) == (length(y), b.n) && rowptr[end] == length(y) || throw(DimensionMismatch("A must be nobs x n, with nobs = sum(rows)"))
    (offset === nothing || length(offset) == length(y)) && (aux === nothing || length(aux) == length(y)) ||
        throw(DimensionMismatch("offset / aux must have one entry per observation"))
    poff = offset === nothing ? Ptr{Float64}(C_NULL) : pointer(offset)
    paux = aux === nothing ? Ptr{Float64}(C_NULL) : pointer(aux)
    GC.@preserve fam params rowptr y A offset aux check(ccall((:gmrfx_obs_set_composite, LIB), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}),
        b.h.ptr, Int32(length(fam)), fam, params, rowptr, length(y), A.colptr, A.rowval, A.nzval, Int32(1), poff, y, paux), b.h)
    return b
end
function composite_info(b::MI355XBackend)
    nc = Ref{Int32}(0)
    check(ccall((:gmrfx_obs_composite_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}),
                b.h.ptr, nc, C_NULL, C_NULL, C_NULL, C_NULL), b.h)
    fam = Vector{Int32}(undef, nc[]); par = Vector{Float64}(undef, nc[]); rp = Vector{Int64}(undef, nc[] + 1); c = Vector{Float64}(undef, nc[])
    nc[] > 0 && check(ccall((:gmrfx_obs_composite_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}),
                            b.h.ptr, nc, fam, par, rp, c), b.h)
    return (family = fam, param = par, rowptr = nc[] > 0 ? rp : Int64[], loglik_const = c)
end
function set_composite_param!(b::MI355XBackend, params::Vector{Float64})
    length(params) == length(composite_info(b).family) || throw(DimensionMismatch("params must have one entry per component"))
    check(ccall((:gmrfx_obs_composite_set_param, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), b.h.ptr, params), b.h)
    return b
end
function observations_design_info(b::MI355XBackend)
    a = Ref{Int64}(0); c = Ref{Int64}(0); t = Ref{Int64}(0)
    check(ccall((:gmrfx_obs_design_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}), b.h.ptr, a, c, t), b.h)
    return (nnz = a[], cnt = c[], terms = t[])
end
function observations_hess_map(b::MI355XBackend)
    cnt = Ref{Int64}(0)
    check(ccall((:gmrfx_obs_hess_map, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}), b.h.ptr, cnt, C_NULL), b.h)
    m = Vector{Int64}(undef, cnt[])
    check(ccall((:gmrfx_obs_hess_map, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}), b.h.ptr, cnt, m), b.h)
    return m .+ 1
end
# entries of the Hessian vector: n in node form, the map's cnt in design form
_hess_len(b::MI355XBackend) = (c = observations_design_info(b).cnt; c < 0 ? b.n : Int(c))
# (score, hess, energy, loglik) at x, one pass over the prior gmrfx_set_prior keeps: score = Q_p x - Q_p mean - loggrad(x), hess = the
# diagonal of loghessian(x) -- the operands of one Newton step --, energy = x'Q_p x / 2 - x'Q_p mean, loglik(x)
function fisher_eval(b::MI355XBackend, x::Vector{Float64}; mean::Union{Nothing, Vector{Float64}} = nothing)
    length(x) == b.n && (mean === nothing || length(mean) == b.n) || throw(DimensionMismatch("x and mean must have n entries"))
    score = Vector{Float64}(undef, b.n); hess = Vector{Float64}(undef, _hess_len(b)); out = zeros(2)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    GC.@preserve x mean score hess out check(ccall((:gmrfx_fisher_eval, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        b.h.ptr, x, mu, score, hess, out), b.h)
    return score, hess, out[1], out[2]
end
function fisher_eval_dev! end   # ROCArray method: ext/GMRFXAMDGPUExt.jl

# The whole Fisher-scoring loop on the device (gmrfx_gaussian_approximation; include/gmrfx.h): prior = the values of set_prior! with
# mean `mean`, likelihood = set_observations!, constraint = set_constraints! (projected with e = 0). Returns (mode, hess = the diagonal
# of loghessian(mode), info) with info = (iterations, converged, alpha, newton_decrement, factorizations, solves, merit_evaluations,
# frozen_finish, dec_trace, alpha_trace). A failed factorisation throws PosDefException.
_ga_flags(adaptive_stepsize::Bool, step_recovery::Symbol, predictive_convergence::Bool, refactorize_final::Bool) =
    Int32(adaptive_stepsize) | (Int32(G._retry_full_step(step_recovery)) << 1) | (Int32(predictive_convergence) << 2) | (Int32(refactorize_final) << 3)
function _ga_info(res::Vector{Float64}, dec::Vector{Float64}, alp::Vector{Float64})
    used = .!isnan.(dec)
    return (iterations = Int(res[1]), converged = res[2] != 0, alpha = res[3], newton_decrement = res[4], factorizations = Int(res[5]),
            solves = Int(res[6]), merit_evaluations = Int(res[7]), frozen_finish = res[8] != 0, dec_trace = dec[used], alpha_trace = alp[used])
end
function gaussian_approximation_device(b::MI355XBackend; mean::Union{Nothing, Vector{Float64}} = nothing, x0::Union{Nothing, Vector{Float64}} = nothing,
                                       max_iter::Int = 50, mean_change_tol::Real = 1.0e-4, newton_dec_tol::Real = 1.0e-5,
                                       adaptive_stepsize::Bool = true, max_linesearch_iter::Int = 10, step_recovery::Symbol = :retry_full,
                                       predictive_convergence::Bool = true, refactorize_final::Bool = false)
    (mean === nothing || length(mean) == b.n) && (x0 === nothing || length(x0) == b.n) || throw(DimensionMismatch("mean and x0 must have n entries"))
    x = Vector{Float64}(undef, b.n); hess = Vector{Float64}(undef, _hess_len(b)); res = zeros(8)
    dec = fill(NaN, max_iter + 1); alp = fill(NaN, max_iter + 1); info = Ref{Int64}(0)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    xs = x0 === nothing ? Ptr{Float64}(C_NULL) : pointer(x0)
    flags = _ga_flags(adaptive_stepsize, step_recovery, predictive_convergence, refactorize_final)
    code = GC.@preserve mean x0 x hess res dec alp ccall((:gmrfx_gaussian_approximation, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}),
        b.h.ptr, mu, xs, max_iter, max_linesearch_iter, Float64(mean_change_tol), Float64(newton_dec_tol), flags, x, hess, res, dec, alp, info)
    b.selinv_cache = nothing
    b.selinv_diag_cache = nothing
    info[] > 0 && throw(PosDefException(Int(info[])))
    check(code, b.h)
    return x, hess, _ga_info(res, dec, alp)
end
function gaussian_approximation_dev! end   # ROCArray method: ext/GMRFXAMDGPUExt.jl

# The pullback of gaussian_approximation at its mode x (gmrfx_ga_pullback; include/gmrfx.h; the rule of src/workspace/autodiff.jl:140-202):
# from the cotangents of the posterior mean (mubar, n) and precision (Qbar, nnz values on the pattern, the convention of logpdf_grad),
# either `nothing`, returns (Qbar_prior, mubar_prior, lambda, param_bar, lambda' xbar). project: lambda <- lambda - A~' W^-1 (A lambda)
# with the constraint set; refactorize: factorise Q_prior - H(x) first (otherwise the handle holds it: refactorize_final = true above).
function pattern_nnz(b::MI355XBackend)
    r = Ref{Int64}(0)
    check(ccall((:gmrfx_pattern_nnz, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), b.h.ptr, r), b.h)
    return Int(r[])
end
function ga_pullback(b::MI355XBackend, x::Vector{Float64}; mean::Union{Nothing, Vector{Float64}} = nothing,
                     mubar::Union{Nothing, Vector{Float64}} = nothing, Qbar::Union{Nothing, Vector{Float64}} = nothing,
                     project::Bool = false, refactorize::Bool = false)
    nnz = pattern_nnz(b)
    length(x) == b.n && (mean === nothing || length(mean) == b.n) && (mubar === nothing || length(mubar) == b.n) &&
        (Qbar === nothing || length(Qbar) == nnz) || throw(DimensionMismatch("x, mean, mubar need n entries, Qbar nnz"))
    qp = Vector{Float64}(undef, nnz); mp = Vector{Float64}(undef, b.n); lam = Vector{Float64}(undef, b.n); out = zeros(2)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    mb = mubar === nothing ? Ptr{Float64}(C_NULL) : pointer(mubar)
    qb = Qbar === nothing ? Ptr{Float64}(C_NULL) : pointer(Qbar)
    flags = Int32(project) | (Int32(refactorize) << 1)
    code = GC.@preserve x mean mubar Qbar qp mp lam out ccall((:gmrfx_ga_pullback, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        b.h.ptr, x, mu, mb, qb, flags, qp, mp, lam, out)
    if refactorize
        b.selinv_cache = nothing
        b.selinv_diag_cache = nothing
    end
    check(code, b.h)
    return qp, mp, lam, out[1], out[2]
end
function ga_pullback_dev! end   # ROCArray method: ext/GMRFXAMDGPUExt.jl
# The same for a composite likelihood (gmrfx_ga_pullback_composite): param_bar is a vector, one cotangent per component (0.0 for a
# component without a parameter). Returns (Qbar_prior, mubar_prior, lambda, param_bar, lambda' xbar).
function ga_pullback_composite(b::MI355XBackend, x::Vector{Float64}; mean::Union{Nothing, Vector{Float64}} = nothing,
                               mubar::Union{Nothing, Vector{Float64}} = nothing, Qbar::Union{Nothing, Vector{Float64}} = nothing,
                               project::Bool = false, refactorize::Bool = false)
    nnz = pattern_nnz(b)
    length(x) == b.n && (mean === nothing || length(mean) == b.n) && (mubar === nothing || length(mubar) == b.n) &&
        (Qbar === nothing || length(Qbar) == nnz) || throw(DimensionMismatch("x, mean, mubar need n entries, Qbar nnz"))
    qp = Vector{Float64}(undef, nnz); mp = Vector{Float64}(undef, b.n); lam = Vector{Float64}(undef, b.n)
    par = zeros(max(length(composite_info(b).family), 1)); chk = Ref{Float64}(0.0)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    mb = mubar === nothing ? Ptr{Float64}(C_NULL) : pointer(mubar)
    qb = Qbar === nothing ? Ptr{Float64}(C_NULL) : pointer(Qbar)
    flags = Int32(project) | (Int32(refactorize) << 1)
    code = GC.@preserve x mean mubar Qbar qp mp lam par ccall((:gmrfx_ga_pullback_composite, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
        b.h.ptr, x, mu, mb, qb, flags, qp, mp, lam, par, chk)
    if refactorize
        b.selinv_cache = nothing
        b.selinv_diag_cache = nothing
    end
    check(code, b.h)
    return qp, mp, lam, par, chk[]
end
function ga_pullback_composite_dev! end   # ROCArray method: ext/GMRFXAMDGPUExt.jl

# linear_predictor_marginals(ga, obs_lik) of the reference (src/linear_predictor_marginals.jl:58-195) and pointwise_loglik at the mean,
# on the device (gmrfx_predictor_marginals; include/gmrfx.h): (mean, variance, pointwise log density) of every observation's linear
# predictor, in the caller's order, under the factorisation the handle holds (refactorize_final = true above leaves Q_post).
# constraint_correction: the correction and clamp of _subtract_constraint_correction!.
function observations_pointwise_const(b::MI355XBackend)
    fam = Ref{Int32}(0); nobs = Ref{Int64}(0); c0 = Ref{Float64}(0.0)
    check(ccall((:gmrfx_obs_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int64}, Ref{Float64}), b.h.ptr, fam, nobs, c0), b.h)
    c = Vector{Float64}(undef, nobs[])
    GC.@preserve c check(ccall((:gmrfx_obs_pointwise_const, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), b.h.ptr, c), b.h)
    return c
end
function predictor_marginals(b::MI355XBackend, x::Vector{Float64}; constraint_correction::Bool = false)
    length(x) == b.n || throw(DimensionMismatch("x must have n entries"))
    nobs = length(observations_pointwise_const(b))
    mu = Vector{Float64}(undef, nobs); v = Vector{Float64}(undef, nobs); pll = Vector{Float64}(undef, nobs)
    GC.@preserve x mu v pll check(ccall((:gmrfx_predictor_marginals, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        b.h.ptr, x, Int32(constraint_correction), mu, v, pll), b.h)
    return mu, v, pll
end
# The quadrature scores over eta_i ~ N(mu_eta_i, v_eta_i) (gmrfx_predictive_scores): nodes and weights of the standard normal from the
# caller. Returns (lpd, lcpo, elp, vlp) per observation and the totals (lpd, lcpo, elp, p_waic, waic = -2 (lpd - p_waic)).
function predictive_scores(b::MI355XBackend, mu_eta::Vector{Float64}, v_eta::Vector{Float64}, nodes::Vector{Float64}, weights::Vector{Float64})
    nobs = length(mu_eta)
    length(v_eta) == nobs && length(nodes) == length(weights) || throw(DimensionMismatch("mu_eta / v_eta and nodes / weights must pair up"))
    lpd = Vector{Float64}(undef, nobs); lcpo = Vector{Float64}(undef, nobs); elp = Vector{Float64}(undef, nobs); vlp = Vector{Float64}(undef, nobs)
    out = zeros(4)
    GC.@preserve mu_eta v_eta nodes weights lpd lcpo elp vlp out check(ccall((:gmrfx_predictive_scores, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        b.h.ptr, mu_eta, v_eta, length(nodes), nodes, weights, lpd, lcpo, elp, vlp, out), b.h)
    return (lpd = lpd, lcpo = lcpo, elp = elp, vlp = vlp), (lpd = out[1], lcpo = out[2], elp = out[3], p_waic = out[4], waic = -2 * (out[1] - out[4]))
end

# gaussian_approximation(prior::WorkspaceGMRF, obs_lik) of the reference (src/workspace/gaussian_approximation.jl:191-313) for workspaces on
# this backend and the pointwise exponential-family likelihoods the device evaluates: one method per likelihood type, each more
# specific than the reference's (WorkspaceGMRF, ObservationLikelihood) method. Everything else -- other links, Student-t, generic and
# AD likelihoods, LatentPrior -- keeps the reference's method by dispatch, and NormalLikelihood{IdentityLink} keeps the reference's
# own conjugate method (linear_condition), as in the reference itself.
_obs_indices(::Nothing) = nothing
_obs_indices(idx) = collect(Int64, idx)
_obs_offset(::Nothing, k::Int) = nothing
_obs_offset(o::Real, k::Int) = fill(Float64(o), k)
_obs_offset(o::AbstractVector, k::Int) = Vector{Float64}(o)
device_likelihood(l::G.PoissonLikelihood{G.LogLink}) = (1, Vector{Float64}(l.y), _obs_indices(l.indices), _obs_offset(l.logexposure, length(l.y)), 0.0)
device_likelihood(l::G.BernoulliLikelihood{G.LogitLink}) = (2, Vector{Float64}(l.y), _obs_indices(l.indices), nothing, 0.0)
device_likelihood(l::G.BinomialLikelihood{G.LogitLink}) = (3, Vector{Float64}(l.y), _obs_indices(l.indices), Vector{Float64}(l.n), 0.0)
device_likelihood(l::G.NegBinLikelihood{G.LogLink}) = (4, Vector{Float64}(l.y), _obs_indices(l.indices), _obs_offset(l.logexposure, length(l.y)), Float64(l.r))
device_likelihood(l::G.GammaLikelihood{G.LogLink}) = (5, Vector{Float64}(l.y), _obs_indices(l.indices), nothing, Float64(l.phi))

# ws.Q <- Q_p - A' D A from the device's cnt values: the map addresses the triangle the handle reads, the workspace's Q may hold both,
# so the mirrored entry (where it is stored) takes the same value. Then what _update_hessian! does after its own subtraction.
function _subtract_design_hessian!(ws, Qp::Vector{Float64}, hmap::Vector{Int}, hess::Vector{Float64})
    Q = ws.Q
    cp, rv, nz = Q.colptr, Q.rowval, Q.nzval
    copyto!(nz, Qp)
    for (p, hv) in zip(hmap, hess)
        c = searchsortedlast(cp, p)
        r = rv[p]
        nz[p] -= hv
        if r != c       # entry (c, r): row c in column r
            q = cp[r] - 1 + searchsortedfirst(view(rv, cp[r]:(cp[r + 1] - 1)), c)
            q < cp[r + 1] && rv[q] == c && (nz[q] -= hv)
        end
    end
    G._invalidate!(ws)
    ws.loaded_version = 0
    return nothing
end

function _device_gaussian_approximation(prior::G.WorkspaceGMRF, obs_lik; x0::Union{Nothing, AbstractVector} = nothing, max_iter::Int = 50,
                                        mean_change_tol::Real = 1.0e-4, newton_dec_tol::Real = 1.0e-5, adaptive_stepsize::Bool = true,
                                        max_linesearch_iter::Int = 10, step_recovery::Symbol = :retry_full,
                                        predictive_convergence::Bool = true, verbose::Bool = false)
    ws = prior.workspace
    b = ws.backend
    ci = prior.constraints
    if ci !== nothing && size(ci.matrix, 1) > MAX_DEVICE_CONSTRAINTS       # more rows than the device's constraint state takes: the reference's loop
        return invoke(G.gaussian_approximation, Tuple{G.WorkspaceGMRF, G.ObservationLikelihood}, prior, obs_lik; x0, max_iter, mean_change_tol,
                      newton_dec_tol, adaptive_stepsize, max_linesearch_iter, step_recovery, predictive_convergence, verbose)
    end
    design = obs_lik isa G.LinearlyTransformedLikelihood
    fam, y, idx, aux, param = device_likelihood(design ? obs_lik.base_likelihood : obs_lik)
    if design && idx !== nothing        # a base likelihood with its own indices: not a row-per-observation design, the reference's loop
        return invoke(G.gaussian_approximation, Tuple{G.WorkspaceGMRF, G.ObservationLikelihood}, prior, obs_lik; x0, max_iter, mean_change_tol,
                      newton_dec_tol, adaptive_stepsize, max_linesearch_iter, step_recovery, predictive_convergence, verbose)
    end
    G.ensure_loaded!(prior)
    Qp = copy(ws.Q.nzval)
    diag_idx = G._diagonal_indices(ws.Q)
    hmap = nothing
    if design       # eta = A x + b: the Hessian A' D A sits on the positions the handle computes once; pattern(A'A) outside Q throws, as _sparse_hessian_map does
        A = obs_lik.design_matrix
        off = obs_lik.offset === nothing ? nothing : Vector{Float64}(obs_lik.offset)
        set_design_observations!(b, fam, y, SparseMatrixCSC{Float64, Int64}(A); offset = off, aux = aux, param = param)
        hmap = Vector{Int}(observations_hess_map(b))
        set_prior!(b, Qp, hmap)
    else
        set_prior!(b, Qp, Vector{Int}(diag_idx))
        set_observations!(b, fam, y; indices = idx, aux = aux, param = param)
    end
    sync_constraints!(b, ci)
    x, hess, info = gaussian_approximation_device(b; mean = Vector{Float64}(prior.mean), x0 = x0 === nothing ? nothing : Vector{Float64}(x0),
                                                  max_iter, mean_change_tol, newton_dec_tol, adaptive_stepsize, max_linesearch_iter,
                                                  step_recovery, predictive_convergence)
    verbose && println(info.converged ? "  Converged after $(info.iterations) iterations" : "  Reached max_iter without convergence")
    # _workspace_build_result: ws.Q <- Q_p - H(x_final), not factorised eagerly; the constraints are re-applied by _build_result
    if design
        _subtract_design_hessian!(ws, Qp, hmap, hess)
    else
        G._update_hessian!(ws, Diagonal(hess), Qp, diag_idx, nothing)
    end
    return G._build_result(ws, x, ci)
end
G.gaussian_approximation(prior::G.WorkspaceGMRF{<:Any, MI355XBackend}, obs_lik::G.PoissonLikelihood{G.LogLink}; kw...) =
    _device_gaussian_approximation(prior, obs_lik; kw...)
G.gaussian_approximation(prior::G.WorkspaceGMRF{<:Any, MI355XBackend}, obs_lik::G.BernoulliLikelihood{G.LogitLink}; kw...) =
    _device_gaussian_approximation(prior, obs_lik; kw...)
G.gaussian_approximation(prior::G.WorkspaceGMRF{<:Any, MI355XBackend}, obs_lik::G.BinomialLikelihood{G.LogitLink}; kw...) =
    _device_gaussian_approximation(prior, obs_lik; kw...)
G.gaussian_approximation(prior::G.WorkspaceGMRF{<:Any, MI355XBackend}, obs_lik::G.NegBinLikelihood{G.LogLink}; kw...) =
    _device_gaussian_approximation(prior, obs_lik; kw...)
G.gaussian_approximation(prior::G.WorkspaceGMRF{<:Any, MI355XBackend}, obs_lik::G.GammaLikelihood{G.LogLink}; kw...) =
    _device_gaussian_approximation(prior, obs_lik; kw...)
# eta = A x + b with a sparse A over one of the likelihoods above; a dense A or another base keeps the reference's method
const DeviceBaseLikelihood = Union{G.PoissonLikelihood{G.LogLink}, G.BernoulliLikelihood{G.LogitLink}, G.BinomialLikelihood{G.LogitLink},
                                   G.NegBinLikelihood{G.LogLink}, G.GammaLikelihood{G.LogLink}}
G.gaussian_approximation(prior::G.WorkspaceGMRF{<:Any, MI355XBackend},
                         obs_lik::G.LinearlyTransformedLikelihood{<:DeviceBaseLikelihood, <:SparseMatrixCSC}; kw...) =
    _device_gaussian_approximation(prior, obs_lik; kw...)

# `_rand!` on given draws: X = P' L^-T Z + mean, then the constraint correction when the handle holds one
function sample(b::MI355XBackend, Z::Matrix{Float64}, mean::Union{Nothing, Vector{Float64}} = nothing)
    X = similar(Z)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    GC.@preserve Z X mean check(ccall((:gmrfx_sample, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64),
        b.h.ptr, Z, stride(Z, 2), size(Z, 2), mu, X, stride(X, 2)), b.h)
    return X
end
# var(d) (workspace_gmrf.jl:260-273) with the subtraction of rowsum(B^2) on the device; more than 64 rows: the reference's method
function G.var(d::G.WorkspaceGMRF{<:Any, MI355XBackend})
    G.ensure_loaded!(d)
    G.ensure_numeric!(d.workspace)
    b = d.workspace.backend
    if d.constraints !== nothing && size(d.constraints.matrix, 1) > MAX_DEVICE_CONSTRAINTS
        return invoke(G.var, Tuple{G.WorkspaceGMRF}, d)
    end
    sync_constraints!(b, d.constraints)
    return constrained_var(b)
end

ordering_permutation(b::MI355XBackend) = (p = Vector{Int}(undef, b.n);
    ccall((:gmrfx_get_perm, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Int64}), b.h.ptr, 1, p); p)

# selector, like GMRFWorkspace(Q, CliqueTreesBackend; alg) (src/workspace/cliquetrees_backend.jl:132-150)
function G.GMRFWorkspace(Q::SparseMatrixCSC{Float64}, ::Type{MI355XBackend}; kwargs...)
    n = size(Q, 1)
    n == size(Q, 2) || throw(ArgumentError("Q must be square"))
    backend = MI355XBackend(Symmetric(Q); kwargs...)
    return GMRFWorkspace{Float64, MI355XBackend}(copy(Q), backend, zeros(n), zeros(n), true, false, false, 0.0, 1, 0)
end

# Newton loop with Q resident on the device (include/gmrfx.h "Newton loop"): the workspace-side
# `_update_hessian!` (src/workspace/gaussian_approximation.jl:103-129) becomes one upload of the prior values
# and of the index map (`_diag_indices(ws.Q)` or `_sparse_hessian_map(ws.Q, H)`, 1-based positions into nzval)
# followed, per iterate, by the Hessian's values only.
function set_prior!(b::MI355XBackend, prior_nzval::Vector{Float64}, hess_map::Vector{Int})
    GC.@preserve prior_nzval hess_map check(ccall((:gmrfx_set_prior, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Int64, Int32), b.h.ptr, prior_nzval, hess_map, length(hess_map), 1), b.h)
    return nothing
end
function refactorize_update!(b::MI355XBackend, hvals::Vector{Float64})
    info = Ref{Int64}(0)
    GC.@preserve hvals check(ccall((:gmrfx_refactorize_update, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ref{Int64}),
        b.h.ptr, hvals, info), b.h)
    b.selinv_cache = nothing; b.selinv_diag_cache = nothing
    return nothing
end

# one Newton iterate (gaussian_approximation.jl:103-129) in one pipelined call: Hessian values in, solve for the new mean out
function refactorize_update_solve!(b::MI355XBackend, hvals::Vector{Float64}, rhs::AbstractVecOrMat)
    B = Matrix{Float64}(reshape(rhs, b.n, :)); X = similar(B)
    info = Ref{Int64}(0)
    GC.@preserve hvals B X check(ccall((:gmrfx_refactorize_update_solve, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ref{Int64}),
        b.h.ptr, hvals, B, b.n, size(B, 2), X, b.n, info), b.h)
    b.selinv_cache = nothing; b.selinv_diag_cache = nothing
    return rhs isa AbstractVector ? vec(X) : X
end

# dot(r, Q * r), r = x - mean, on the device with the values of the last refactorize! (the quadratic form of
# logpdf(::WorkspaceGMRF, z), src/workspace/workspace_gmrf.jl:288-292, and sqmahal, src/gmrf.jl:94-97).
# X: n vector or n x k matrix (one value per column).
function sqmahal(b::MI355XBackend, X::StridedVecOrMat{Float64}; mean::Union{Nothing, Vector{Float64}} = nothing)
    nvec = size(X, 2)
    out = Vector{Float64}(undef, nvec)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    GC.@preserve X mean out check(ccall((:gmrfx_quadform, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
        b.h.ptr, C_NULL, X, X isa AbstractVector ? length(X) : stride(X, 2), nvec, mu, out), b.h)
    return X isa AbstractVector ? out[1] : out
end

# KL (Vecchia) sparse approximate Cholesky on the GPU (src/kl_cholesky/kl_cholesky.jl:32-55): same contract as the
# reference method, for a dense Float64 covariance. One task per column: its row indices in descending order.
# Selected by a trailing `MI355XBackend` argument, like `GMRFWorkspace(Q, MI355XBackend)`: a method on (Matrix{Float64},
# SparseMatrixCSC{Float64, Int}) alone would REPLACE the reference's own for those types (piracy) and take its AD-transparent
# generic path away from every caller that merely loads the plug-in.
function G.sparse_approximate_cholesky!(Θ::Matrix{Float64}, L::SparseMatrixCSC{Float64, Int}, ::Type{MI355XBackend}; device::Integer = -1)
    n = size(L, 2)
    rows = similar(L.rowval)
    for k in 1:n
        r = nzrange(L, k)
        rows[r] .= @view L.rowval[reverse(r)]
    end
    cols = collect(1:n); colptr_t = collect(1:(n + 1)); info = Ref{Int64}(0)
    GC.@preserve Θ L rows cols colptr_t begin
        code = ccall((:gmrfx_kl_cholesky, LIB), Int32,
            (Int64, Ptr{Float64}, Int64, Int32, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
             Int32, Float64, Int32, Ptr{Float64}, Ref{Int64}),
            n, Θ, stride(Θ, 2), 0, L.colptr, n, L.colptr, rows, colptr_t, cols, 1, 1.0e-6, device, L.nzval, info)
    end
    code == 5 && throw(PosDefException(Int(info[])))
    check(code)
    return
end

function Base.deepcopy_internal(b::MI355XBackend, stackdict::IdDict)   # deepcopy(cache) in Newton loops
    haskey(stackdict, b) && return stackdict[b]::MI355XBackend
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:gmrfx_clone, LIB), Int32, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), b.h.ptr, out))
    c = MI355XBackend(Handle(out[]), b.n, nothing, nothing)
    stackdict[b] = c
    return c
end

# ---------------------------------------------------------------------------------- one factorisation over several GPUs
# The native driver of the sharded protocol (libgmrfx_rccl.so, include/gmrfx_rccl.h: RCCL point-to-point / broadcast / all-reduce
# between the phases of libgmrfx.so), one Julia process (Distributed.jl worker / MPI rank) per GPU:
#     id = rank == 0 ? rccl_unique_id() : <the 128 bytes from rank 0, by whatever the host uses: Distributed, MPI, a file>
#     sf = ShardedMI355X(Q, world, rank, id; coords)          # same Q on every rank
#     refactorize!(sf, d_nz); solve!(d_X, sf, d_B); logdet(sf) # ROCArray operands: julia/ext/GMRFXAMDGPUExt.jl
# The reference has nothing to replace here (CHOLMOD has one address space: src/workspace/backend.jl:165-209); this is what the
# exchange of Schur-complement blocks stands in for.
const LIB_RCCL = get(ENV, "GMRFX_RCCL_LIB", joinpath(@__DIR__, "..", "libgmrfx_rccl.so"))

function rccl_unique_id()
    id = Vector{UInt8}(undef, 128)
    code = ccall((:gmrfx_rccl_unique_id, LIB_RCCL), Int32, (Ptr{Cvoid},), id)
    code == 0 || error("gmrfx_rccl_unique_id failed ($code)")
    return id
end

mutable struct ShardedMI355X
    h::Handle
    drv::Ptr{Cvoid}
    n::Int
    world::Int
    rank::Int
end

function ShardedMI355X(Q::SparseMatrixCSC{Float64, Int}, world::Integer, rank::Integer, id::Vector{UInt8};
        ordering = nothing, coords = nothing, device = -1, shard_min_top = 0)
    length(id) == 128 || throw(ArgumentError("the communicator id has 128 bytes"))
    h = create(Q; ordering, coords, device, shard_rank = rank, shard_world = world, shard_min_top)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    code = GC.@preserve id ccall((:gmrfx_rccl_create, LIB_RCCL), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
        h.ptr, world, rank, id, C_NULL, out)
    code == 0 || error("gmrfx_rccl_create failed ($code)")
    sf = ShardedMI355X(h, out[], size(Q, 1), world, rank)
    finalizer(x -> (x.drv == C_NULL || ccall((:gmrfx_rccl_destroy, LIB_RCCL), Cvoid, (Ptr{Cvoid},), x.drv); x.drv = C_NULL), sf)
    return sf
end

function check_rccl(code::Int32, sf::ShardedMI355X)
    code == 0 && return nothing
    error("gmrfx_rccl ($code): " * unsafe_string(ccall((:gmrfx_rccl_last_error, LIB_RCCL), Cstring, (Ptr{Cvoid},), sf.drv)))
end

# log det Q over all ranks + the pivot report (PosDefException like refactorize! under check_posdef)
function LinearAlgebra.logdet(sf::ShardedMI355X)
    ld = Ref{Float64}(0.0); info = Ref{Int64}(0)
    check_rccl(ccall((:gmrfx_rccl_logdet, LIB_RCCL), Int32, (Ptr{Cvoid}, Ref{Float64}, Ref{Int64}), sf.drv, ld, info), sf)
    info[] > 0 && throw(PosDefException(Int(info[])))
    return ld[]
end

# diag(Q^-1) on every rank (the sharded Takahashi recursion + an all-reduce)
function selinv_diag(sf::ShardedMI355X)
    out = Vector{Float64}(undef, sf.n)
    check_rccl(ccall((:gmrfx_rccl_selinv_diag, LIB_RCCL), Int32, (Ptr{Cvoid}, Ptr{Float64}), sf.drv, out), sf)
    return out
end

# the rows of B this rank reads in solve! (the ranks' masks partition 1:n: B may be row-sharded)
function needed_rows(sf::ShardedMI355X)
    mask = Vector{UInt8}(undef, sf.n)
    check_rccl(ccall((:gmrfx_rccl_needed_rows, LIB_RCCL), Int32, (Ptr{Cvoid}, Ptr{UInt8}), sf.drv, mask), sf)
    return mask .!= 0
end

function solve! end       # ROCArray methods: julia/ext/GMRFXAMDGPUExt.jl

# ---------------------------------------------------------------------------------- batched handles
# B precisions with ONE pattern factored in one pass (include/gmrfx.h, gmrfx_create_batched): the hyper-parameter loop of
# docs/src/literate-tutorials/workspace_factorization_reuse.jl evaluates logpdf for many values of one pattern, and WorkspacePool
# (src/workspace/workspace_pool.jl:5-22) runs such evaluations side by side. Member k's values are column k of an nnz x B matrix
# (the pattern's CSC order), right-hand sides are n x B or n x r x B arrays.
mutable struct MI355XBatch
    h::Handle
    n::Int           # nodes per member
    nbatch::Int
    nnz::Int         # stored entries per member
    info::Vector{Int64}
end

function MI355XBatch(Q::SparseMatrixCSC{Float64, Int}, nbatch::Integer; ordering = nothing, coords = nothing, device = -1)
    n = size(Q, 1)
    perm = resolve_ordering(Q, ordering)
    perm === nothing || isperm(perm) && length(perm) == n || throw(ArgumentError("ordering is not a permutation of 1:$n"))
    C = coords === nothing ? nothing : Matrix{Float64}(transpose(coords))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Q perm C begin
        o = Opts(struct_size = sizeof(Opts), device = device, ordering = ordering === :natural ? 1 : 0,
            coord_dim = C === nothing ? 0 : size(C, 1), coords = C === nothing ? C_NULL : pointer(C))
        check(ccall((:gmrfx_create_batched, LIB), Int32,
            (Int64, Ptr{Int64}, Ptr{Int64}, Int32, Ptr{Int64}, Int64, Ref{Opts}, Ref{Ptr{Cvoid}}),
            n, SparseArrays.getcolptr(Q), rowvals(Q), 1, perm === nothing ? C_NULL : pointer(perm), nbatch, Ref(o), out))
    end
    return MI355XBatch(Handle(out[]), n, Int(nbatch), nnz(Q), zeros(Int64, nbatch))
end

function refactorize!(bb::MI355XBatch, NZ::Matrix{Float64})
    size(NZ) == (bb.nnz, bb.nbatch) || throw(DimensionMismatch("NZ must be nnz x nbatch"))
    GC.@preserve NZ check(ccall((:gmrfx_batch_refactorize, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}),
        bb.h.ptr, NZ, bb.info), bb.h)
    return bb
end

# per-member pivot status of the last refactorize!: 0, or 1 + the first failing column of that member (elimination order)
info(bb::MI355XBatch) = copy(bb.info)

function logdet(bb::MI355XBatch)
    out = Vector{Float64}(undef, bb.nbatch)
    GC.@preserve out check(ccall((:gmrfx_batch_logdet, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), bb.h.ptr, out), bb.h)
    return out
end

function _batch_solve(bb::MI355XBatch, R::Array{Float64}, name::Symbol)
    (ndims(R) == 2 && size(R) == (bb.n, bb.nbatch)) || (ndims(R) == 3 && size(R, 1) == bb.n && size(R, 3) == bb.nbatch) ||
        throw(DimensionMismatch("expected n x nbatch or n x r x nbatch"))
    r = ndims(R) == 3 ? size(R, 2) : 1
    X = similar(R)
    code = GC.@preserve R X if name === :solve
        ccall((:gmrfx_batch_solve, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64),
            bb.h.ptr, R, bb.n, bb.n * r, r, X, bb.n, bb.n * r)
    else
        ccall((:gmrfx_batch_backward_solve, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64),
            bb.h.ptr, R, bb.n, bb.n * r, r, X, bb.n, bb.n * r)
    end
    check(code, bb.h)
    return X
end
# X_k = Q_k \ R_k
solve(bb::MI355XBatch, R::Union{Matrix{Float64}, Array{Float64, 3}}) = _batch_solve(bb, R, :solve)
# X_k = P' L_k^-T Z_k (samples)
backward_solve(bb::MI355XBatch, Z::Union{Matrix{Float64}, Array{Float64, 3}}) = _batch_solve(bb, Z, :backward)

# diag(Q_k^-1) of every member: n x nbatch
function selinv_diag(bb::MI355XBatch)
    out = Matrix{Float64}(undef, bb.n, bb.nbatch)
    GC.@preserve out check(ccall((:gmrfx_selinv_diag, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), bb.h.ptr, out), bb.h)
    return out
end

# the terms of logpdf for every member (src/workspace/workspace_gmrf.jl:288-292): new values -> (log det Q_k, (z_k - mu_k)' Q_k (z_k - mu_k));
# Z: n x nbatch, mean: n x nbatch or nothing
function logpdf_terms(bb::MI355XBatch, NZ::Matrix{Float64}, Z::Matrix{Float64}; mean::Union{Nothing, Matrix{Float64}} = nothing)
    size(Z) == (bb.n, bb.nbatch) || throw(DimensionMismatch("Z must be n x nbatch"))
    mean === nothing || size(mean) == (bb.n, bb.nbatch) || throw(DimensionMismatch("mean must be n x nbatch"))
    refactorize!(bb, NZ)
    quad = Vector{Float64}(undef, bb.nbatch)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    GC.@preserve NZ Z mean quad check(ccall((:gmrfx_batch_quadform, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
        bb.h.ptr, NZ, Z, bb.n, bb.n, 1, mu, quad), bb.h)
    return logdet(bb), quad, info(bb)
end

# ONE constraint A x = e for every member (gmrfx_batch_constraints_set: m <= 64 rows over the member's n columns). What is derived
# from it -- A~'_k = Q_k^-1 A', W_k = A A~'_k, L_ck, B_k -- is built per member on the device, once per factorisation.
function set_constraints!(bb::MI355XBatch, A::AbstractMatrix, e::AbstractVector)
    At = sparse(transpose(sparse(A)))                 # CSC of A' = CSR of A
    cp = Vector{Int}(SparseArrays.getcolptr(At)); rv = Vector{Int}(rowvals(At)); nz = Vector{Float64}(nonzeros(At))
    ev = Vector{Float64}(e)
    size(A, 2) == bb.n || throw(ArgumentError("Constraint matrix size $(size(A)) incompatible with member size $(bb.n)"))
    size(A, 1) == length(ev) || throw(ArgumentError("Constraint matrix rows $(size(A, 1)) != constraint vector length $(length(ev))"))
    GC.@preserve cp rv nz ev check(ccall((:gmrfx_batch_constraints_set, LIB), Int32,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Float64}), bb.h.ptr, size(A, 1), cp, rv, nz, 1, ev), bb.h)
    return nothing
end
function clear_constraints!(bb::MI355XBatch)
    check(ccall((:gmrfx_batch_constraints_set, LIB), Int32, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Float64}),
        bb.h.ptr, 0, C_NULL, C_NULL, C_NULL, 1, C_NULL), bb.h)
    return nothing
end

# logpdf_terms plus the members' log_constraint_correction (workspace_gmrf.jl:46-51, 288-305):
# logpdf_k = -quad_k / 2 + logdet_k / 2 - n log(2 pi) / 2 + log_correction_k
function constrained_logpdf_terms(bb::MI355XBatch, NZ::Matrix{Float64}, Z::Matrix{Float64}; mean::Union{Nothing, Matrix{Float64}} = nothing)
    ld, quad, inf = logpdf_terms(bb, NZ, Z; mean = mean)
    lc = Vector{Float64}(undef, bb.nbatch)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    GC.@preserve mean lc check(ccall((:gmrfx_batch_constraints_mean, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        bb.h.ptr, mu, C_NULL, lc), bb.h)
    return ld, quad, lc, inf
end

# `_rand!` per member on given draws: X_k = P' L_k^-T Z_k + mean_k, then the constraint correction; Z: n x nbatch or n x r x nbatch
function sample(bb::MI355XBatch, Z::Union{Matrix{Float64}, Array{Float64, 3}}, mean::Union{Nothing, Matrix{Float64}} = nothing)
    (ndims(Z) == 2 && size(Z) == (bb.n, bb.nbatch)) || (ndims(Z) == 3 && size(Z, 1) == bb.n && size(Z, 3) == bb.nbatch) ||
        throw(DimensionMismatch("expected n x nbatch or n x r x nbatch"))
    mean === nothing || size(mean) == (bb.n, bb.nbatch) || throw(DimensionMismatch("mean must be n x nbatch"))
    r = ndims(Z) == 3 ? size(Z, 2) : 1
    X = similar(Z)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    GC.@preserve Z X mean check(ccall((:gmrfx_batch_sample, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64),
        bb.h.ptr, Z, bb.n, bb.n * r, r, mu, X, bb.n, bb.n * r), bb.h)
    return X
end

# The gradient of every member's logpdf (+ log_correction) on the members' pattern: Z, mean n x nbatch, ybar a number or one per member
# -> (Qbar nnz x nbatch, mubar n x nbatch, info); info[k] != 0 (-1: factorisation failed, > 0: W_k failed): member k's columns are NaN
function logpdf_grad(bb::MI355XBatch, Z::Matrix{Float64}; mean::Union{Nothing, Matrix{Float64}} = nothing, ybar = 1.0)
    size(Z) == (bb.n, bb.nbatch) || throw(DimensionMismatch("Z must be n x nbatch"))
    mean === nothing || size(mean) == (bb.n, bb.nbatch) || throw(DimensionMismatch("mean must be n x nbatch"))
    yb = ybar isa Real ? fill(Float64(ybar), bb.nbatch) : Vector{Float64}(ybar)
    length(yb) == bb.nbatch || throw(DimensionMismatch("ybar must have one entry per member"))
    qbar = Matrix{Float64}(undef, bb.nnz, bb.nbatch); mubar = Matrix{Float64}(undef, bb.n, bb.nbatch)
    inf = zeros(Int64, bb.nbatch)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    GC.@preserve Z mean yb qbar mubar inf check(ccall((:gmrfx_batch_logpdf_grad, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
        bb.h.ptr, C_NULL, Z, bb.n, mu, yb, qbar, mubar, inf), bb.h)
    return qbar, mubar, inf
end
# out[k, b] = sum_e w_e G[e, b] J[e, k, b]: G nnz x nbatch, J nnz x p x nbatch -> p x nbatch
function pattern_dot(bb::MI355XBatch, G::Matrix{Float64}, J::Array{Float64, 3})
    size(G) == (bb.nnz, bb.nbatch) && size(J, 1) == bb.nnz && size(J, 3) == bb.nbatch || throw(DimensionMismatch("G nnz x nbatch, J nnz x p x nbatch"))
    p = size(J, 2)
    out = Matrix{Float64}(undef, p, bb.nbatch)
    GC.@preserve G J out check(ccall((:gmrfx_batch_pattern_dot, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}),
        bb.h.ptr, G, J, max(bb.nnz, 1), bb.nnz * p, p, out), bb.h)
    return out
end

# The pullback of gaussian_approximation for every member (gmrfx_batch_ga_pullback): the link between logpdf_grad(bb, ...) and
# pattern_dot(bb, ...). X n x nbatch (the modes); mean n x nbatch; mubar n x nbatch and Qbar nnz x nbatch as logpdf_grad returns them,
# either `nothing`. Returns (Qbar_prior nnz x nbatch, mubar_prior, lambda n x nbatch, param_bar, lambda' xbar (nbatch each), info):
# info[k] = 0, -1 (member k's factorisation failed) or 1 + the failing pivot of W_k; such a member's columns and results are NaN.
function ga_pullback(bb::MI355XBatch, X::Matrix{Float64}; mean::Union{Nothing, Matrix{Float64}} = nothing,
                     mubar::Union{Nothing, Matrix{Float64}} = nothing, Qbar::Union{Nothing, Matrix{Float64}} = nothing,
                     project::Bool = false, refactorize::Bool = false)
    size(X) == (bb.n, bb.nbatch) && (mean === nothing || size(mean) == (bb.n, bb.nbatch)) && (mubar === nothing || size(mubar) == (bb.n, bb.nbatch)) &&
        (Qbar === nothing || size(Qbar) == (bb.nnz, bb.nbatch)) || throw(DimensionMismatch("X, mean, mubar must be n x nbatch, Qbar nnz x nbatch"))
    qp = Matrix{Float64}(undef, bb.nnz, bb.nbatch); mp = Matrix{Float64}(undef, bb.n, bb.nbatch); lam = Matrix{Float64}(undef, bb.n, bb.nbatch)
    out = zeros(2, bb.nbatch); inf = zeros(Int64, bb.nbatch)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    mb = mubar === nothing ? Ptr{Float64}(C_NULL) : pointer(mubar)
    qb = Qbar === nothing ? Ptr{Float64}(C_NULL) : pointer(Qbar)
    flags = Int32(project) | (Int32(refactorize) << 1)
    GC.@preserve X mean mubar Qbar qp mp lam out inf check(ccall((:gmrfx_batch_ga_pullback, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
        bb.h.ptr, X, bb.n, mu, bb.n, mb, qb, flags, qp, mp, lam, out, inf), bb.h)
    return qp, mp, lam, out[1, :], out[2, :], inf
end

# What follows the fit, for every member (gmrfx_batch_predictor_marginals, gmrfx_batch_predictive_scores, gmrfx_batch_predictive_mixture):
# X n x nbatch (the modes); every per-observation array nobs x nbatch. info[k] = 0, -1 (member k's factorisation failed) or 1 + the
# failing pivot of W_k; such a member's columns (and totals) are NaN.
function batch_nobs(bb::MI355XBatch)
    fam = Ref{Int32}(0); nobs = Ref{Int64}(0); c = zeros(bb.nbatch)
    GC.@preserve c check(ccall((:gmrfx_batch_obs_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int64}, Ptr{Float64}), bb.h.ptr, fam, nobs, c), bb.h)
    return Int(nobs[])
end
function observations_pointwise_const(bb::MI355XBatch)
    c = Matrix{Float64}(undef, batch_nobs(bb), bb.nbatch)
    GC.@preserve c check(ccall((:gmrfx_batch_obs_pointwise_const, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), bb.h.ptr, c), bb.h)
    return c
end
function predictor_marginals(bb::MI355XBatch, X::Matrix{Float64}; constraint_correction::Bool = false)
    size(X) == (bb.n, bb.nbatch) || throw(DimensionMismatch("X must be n x nbatch"))
    nobs = batch_nobs(bb)
    mu = Matrix{Float64}(undef, nobs, bb.nbatch); v = Matrix{Float64}(undef, nobs, bb.nbatch); pll = Matrix{Float64}(undef, nobs, bb.nbatch)
    inf = zeros(Int64, bb.nbatch)
    GC.@preserve X mu v pll inf check(ccall((:gmrfx_batch_predictor_marginals, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
        bb.h.ptr, X, bb.n, Int32(constraint_correction), mu, v, pll, inf), bb.h)
    return mu, v, pll, inf
end
function predictive_scores(bb::MI355XBatch, mu_eta::Matrix{Float64}, v_eta::Matrix{Float64}, nodes::Vector{Float64}, weights::Vector{Float64})
    nobs = batch_nobs(bb)
    size(mu_eta) == (nobs, bb.nbatch) && size(v_eta) == (nobs, bb.nbatch) && length(nodes) == length(weights) ||
        throw(DimensionMismatch("mu_eta / v_eta must be nobs x nbatch, nodes / weights must pair up"))
    lpd = Matrix{Float64}(undef, nobs, bb.nbatch); lcpo = Matrix{Float64}(undef, nobs, bb.nbatch)
    elp = Matrix{Float64}(undef, nobs, bb.nbatch); vlp = Matrix{Float64}(undef, nobs, bb.nbatch)
    out = zeros(4, bb.nbatch); inf = zeros(Int64, bb.nbatch)
    GC.@preserve mu_eta v_eta nodes weights lpd lcpo elp vlp out inf check(ccall((:gmrfx_batch_predictive_scores, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
        bb.h.ptr, mu_eta, v_eta, length(nodes), nodes, weights, lpd, lcpo, elp, vlp, out, inf), bb.h)
    return (lpd = lpd, lcpo = lcpo, elp = elp, vlp = vlp), out, inf
end
# the predictive distribution integrated over the members with weights proportional to exp(logw) (-Inf excludes a member):
# (mix_mu, mix_v, mix_lpd, sum of mix_lpd); without lpd the last two are `nothing`
function predictive_mixture(bb::MI355XBatch, logw::Vector{Float64}, mu_eta::Matrix{Float64}, v_eta::Matrix{Float64},
                            lpd::Union{Nothing, Matrix{Float64}} = nothing)
    nobs = batch_nobs(bb)
    length(logw) == bb.nbatch && size(mu_eta) == (nobs, bb.nbatch) && size(v_eta) == (nobs, bb.nbatch) &&
        (lpd === nothing || size(lpd) == (nobs, bb.nbatch)) || throw(DimensionMismatch("logw must have nbatch entries, the arrays nobs x nbatch"))
    mm = Vector{Float64}(undef, nobs); mv = Vector{Float64}(undef, nobs); ml = Vector{Float64}(undef, nobs)
    out = zeros(1)
    lp = lpd === nothing ? Ptr{Float64}(C_NULL) : pointer(lpd)
    mlp = lpd === nothing ? Ptr{Float64}(C_NULL) : pointer(ml)
    GC.@preserve logw mu_eta v_eta lpd mm mv ml out check(ccall((:gmrfx_batch_predictive_mixture, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        bb.h.ptr, logw, mu_eta, v_eta, lp, mm, mv, mlp, out), bb.h)
    return mm, mv, (lpd === nothing ? nothing : ml), (lpd === nothing ? nothing : out[1])
end

# max(diag Sigma_k - rowsum(B_k^2), 0) of every member: n x nbatch; without a constraint selinv_diag(bb)
function constrained_var(bb::MI355XBatch)
    out = Matrix{Float64}(undef, bb.n, bb.nbatch)
    GC.@preserve out check(ccall((:gmrfx_batch_constraints_var, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), bb.h.ptr, out), bb.h)
    return out
end

# ---- the non-Gaussian path for every member (include/gmrfx.h: gmrfx_batch_set_prior .. gmrfx_batch_gaussian_approximation) ----------------
# the members' prior precisions, nnz x nbatch; the library installs every member's Hessian map for the likelihood in place
# (the diagonal, or the design form's: call it again after changing the likelihood's form)
function set_prior!(bb::MI355XBatch, NZ::Matrix{Float64})
    size(NZ) == (bb.nnz, bb.nbatch) || throw(DimensionMismatch("NZ must be nnz x nbatch"))
    GC.@preserve NZ check(ccall((:gmrfx_batch_set_prior, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), bb.h.ptr, NZ), bb.h)
    return nothing
end
# ONE data set for all members (family id 0 .. 5, y, 1-based indices or nothing, aux or nothing) and one param per member
function set_observations!(bb::MI355XBatch, family::Integer, y::Vector{Float64}, param::Vector{Float64};
                           indices::Union{Nothing, Vector{Int64}} = nothing, aux::Union{Nothing, Vector{Float64}} = nothing)
    length(param) == bb.nbatch || throw(DimensionMismatch("param must have one entry per member"))
    idx = indices === nothing ? Ptr{Int64}(C_NULL) : pointer(indices)
    ax = aux === nothing ? Ptr{Float64}(C_NULL) : pointer(aux)
    GC.@preserve y param indices aux check(ccall((:gmrfx_batch_obs_set, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        bb.h.ptr, Int32(family), length(y), idx, Int32(1), y, ax, param), bb.h)
    return nothing
end
# the members' parameters (sigma, r, phi) replaced in place (gmrfx_batch_obs_set_param): no data goes up, no plan is rebuilt; works while
# a constraint is held, where set_observations! is refused
function set_param!(bb::MI355XBatch, param::Vector{Float64})
    length(param) == bb.nbatch || throw(DimensionMismatch("param must have one entry per member"))
    GC.@preserve param check(ccall((:gmrfx_batch_obs_set_param, LIB), Int32, (Ptr{Cvoid}, Ptr{Float64}), bb.h.ptr, param), bb.h)
    return nothing
end
# rows of the batch constraint held (0: none)
function _con_m(bb::MI355XBatch)
    m = Ref{Int64}(0)
    check(ccall((:gmrfx_batch_constraints_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}),
        bb.h.ptr, m, C_NULL, C_NULL, C_NULL, C_NULL), bb.h)
    return m[]
end
# The same data set observed through eta = A x + offset (gmrfx_batch_obs_set_design): A as Julia holds it (CSC, 1-based), nobs x n of the
# MEMBER. Replaces the node form; call set_prior! again afterwards, it installs the members' maps. fisher_eval and gaussian_approximation
# then return cnt Hessian values per member, in the order of observations_hess_map(bb).
function set_design_observations!(bb::MI355XBatch, family::Integer, y::Vector{Float64}, A::SparseMatrixCSC{Float64, Int64},
                                  param::Vector{Float64}; offset::Union{Nothing, Vector{Float64}} = nothing,
                                  aux::Union{Nothing, Vector{Float64}} = nothing)
    length(param) == bb.nbatch || throw(DimensionMismatch("param must have one entry per member"))
    size(A) == (length(y), bb.n) || throw(DimensionMismatch("A must be nobs x n"))
    (offset === nothing || length(offset) == length(y)) && (aux === nothing || length(aux) == length(y)) ||
        throw(DimensionMismatch("offset / aux must have one entry per observation"))
    poff = offset === nothing ? Ptr{Float64}(C_NULL) : pointer(offset)
    paux = aux === nothing ? Ptr{Float64}(C_NULL) : pointer(aux)
    GC.@preserve y A offset aux param check(ccall((:gmrfx_batch_obs_set_design, LIB), Int32,
        (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        bb.h.ptr, Int32(family), length(y), A.colptr, A.rowval, A.nzval, Int32(1), poff, y, paux, param), bb.h)
    return nothing
end
function observations_design_info(bb::MI355XBatch)
    a = Ref{Int64}(0); c = Ref{Int64}(0); t = Ref{Int64}(0)
    check(ccall((:gmrfx_batch_obs_design_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}), bb.h.ptr, a, c, t), bb.h)
    return (nnz = a[], cnt = c[], terms = t[])
end
# 1-based positions into ONE member's values of the entries of A' D A, ascending
function observations_hess_map(bb::MI355XBatch)
    cnt = Ref{Int64}(0)
    check(ccall((:gmrfx_batch_obs_hess_map, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}, Int64, Ref{Int64}), bb.h.ptr, C_NULL, Int64(0), cnt), bb.h)
    m = Vector{Int64}(undef, cnt[])
    check(ccall((:gmrfx_batch_obs_hess_map, LIB), Int32, (Ptr{Cvoid}, Ptr{Int64}, Int64, Ref{Int64}), bb.h.ptr, m, Int64(length(m)), cnt), bb.h)
    return m .+ 1
end
# entries of a member's Hessian vector: n in node form, the map's cnt in design form
_hess_len(bb::MI355XBatch) = (c = observations_design_info(bb).cnt; c < 0 ? bb.n : Int(c))
function observations_info(bb::MI355XBatch)
    fam = Ref{Int32}(0); nobs = Ref{Int64}(0); c = zeros(bb.nbatch)
    GC.@preserve c check(ccall((:gmrfx_batch_obs_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int64}, Ptr{Float64}), bb.h.ptr, fam, nobs, c), bb.h)
    return (family = fam[], nobs = nobs[], loglik_const = c)
end
# (score, hess, energy, loglik) at the members' points X (n x nbatch); mean n x nbatch or nothing; active: one byte per member or nothing;
# hess: n x nbatch in node form, cnt x nbatch in design form (both outputs go down at one member stride, max(n, cnt))
function fisher_eval(bb::MI355XBatch, X::Matrix{Float64}; mean::Union{Nothing, Matrix{Float64}} = nothing,
                     active::Union{Nothing, Vector{UInt8}} = nothing)
    size(X) == (bb.n, bb.nbatch) || throw(DimensionMismatch("X must be n x nbatch"))
    mean === nothing || size(mean) == (bb.n, bb.nbatch) || throw(DimensionMismatch("mean must be n x nbatch"))
    active === nothing || length(active) == bb.nbatch || throw(DimensionMismatch("active must have one entry per member"))
    hl = _hess_len(bb); ld = max(bb.n, hl)
    score = fill(NaN, ld, bb.nbatch); hess = fill(NaN, ld, bb.nbatch); out = fill(NaN, 2, bb.nbatch)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    act = active === nothing ? Ptr{UInt8}(C_NULL) : pointer(active)
    GC.@preserve X mean active score hess out check(ccall((:gmrfx_batch_fisher_eval, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}),
        bb.h.ptr, X, bb.n, mu, bb.n, act, score, hess, ld, out), bb.h)
    return score[1:bb.n, :], hess[1:hl, :], out[1, :], out[2, :]
end
# The Gaussian approximation of every member: (X, H, result 10 x nbatch, totals, dec_trace, alpha_trace, info). A member whose
# factorisation failed does not throw: info[k] > 0, X[:, k] its last accepted iterate, H[:, k] NaN. H: n x nbatch in node form, cnt x nbatch
# in design form. The tuple always has nine entries: the last two are cinfo and residual, `nothing` each without a constraint (callers that
# destructure the first seven are unaffected). While set_constraints! holds a constraint the loop is
# gmrfx_batch_constrained_gaussian_approximation (every step projected onto A s = 0): cinfo is 0, 1 + the failing pivot of W_k, or -1
# beside a failed factorisation; residual is max |A x_k - e| per member, NaN for a failed one.
function gaussian_approximation(bb::MI355XBatch; mean::Union{Nothing, Matrix{Float64}} = nothing, x0::Union{Nothing, Matrix{Float64}} = nothing,
                                max_iter::Integer = 50, max_linesearch_iter::Integer = 10, mean_change_tol::Real = 1e-4,
                                newton_dec_tol::Real = 1e-5, flags::Integer = 7)
    mean === nothing || size(mean) == (bb.n, bb.nbatch) || throw(DimensionMismatch("mean must be n x nbatch"))
    x0 === nothing || size(x0) == (bb.n, bb.nbatch) || throw(DimensionMismatch("x0 must be n x nbatch"))
    hl = _hess_len(bb)
    X = Matrix{Float64}(undef, bb.n, bb.nbatch); H = fill(NaN, hl, bb.nbatch)
    result = zeros(10, bb.nbatch); totals = zeros(3)
    dec = fill(NaN, max_iter + 1, bb.nbatch); alp = fill(NaN, max_iter + 1, bb.nbatch)
    inf = zeros(Int64, bb.nbatch)
    mu = mean === nothing ? Ptr{Float64}(C_NULL) : pointer(mean)
    xs = x0 === nothing ? Ptr{Float64}(C_NULL) : pointer(x0)
    if _con_m(bb) > 0
        cinf = zeros(Int64, bb.nbatch); res = fill(NaN, bb.nbatch)
        rc = GC.@preserve mean x0 X H result totals dec alp inf cinf res ccall((:gmrfx_batch_constrained_gaussian_approximation, LIB), Int32,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Int64, Float64, Float64, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
            bb.h.ptr, mu, bb.n, xs, bb.n, Int64(max_iter), Int64(max_linesearch_iter), Float64(mean_change_tol), Float64(newton_dec_tol),
            Int32(flags), X, bb.n, H, hl, result, totals, dec, alp, inf, cinf, res)
        bb.info .= inf
        rc == 5 || check(rc, bb.h)          # GMRFX_ERR_NOT_POSDEF: reported per member in info and cinfo
        return X, H, result, totals, dec, alp, inf, cinf, res
    end
    rc = GC.@preserve mean x0 X H result totals dec alp inf ccall((:gmrfx_batch_gaussian_approximation, LIB), Int32,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Int64, Float64, Float64, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
        bb.h.ptr, mu, bb.n, xs, bb.n, Int64(max_iter), Int64(max_linesearch_iter), Float64(mean_change_tol), Float64(newton_dec_tol),
        Int32(flags), X, bb.n, H, hl, result, totals, dec, alp, inf)
    bb.info .= inf
    rc == 5 || check(rc, bb.h)          # GMRFX_ERR_NOT_POSDEF: reported per member in info
    return X, H, result, totals, dec, alp, inf, nothing, nothing
end

# deepcopy(bb) (Newton loops copy their caches) reaches the owning Handle: a copy of a handle is a clone of the native one
# (gmrfx_clone), never a second owner of the same pointer
function Base.deepcopy_internal(h::Handle, stackdict::IdDict)
    haskey(stackdict, h) && return stackdict[h]::Handle
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:gmrfx_clone, LIB), Int32, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), h.ptr, out))
    c = Handle(out[])
    stackdict[h] = c
    return c
end

# ---------------------------------------------------------------------------------- seam A
# LinearSolve algorithm; GMRF-side hooks exactly as the Pardiso extension (ext/GaussianMarkovRandomFieldsPardiso.jl:10-80).
import LinearSolve, SciMLBase
struct MI355XCholesky <: LinearSolve.AbstractFactorization
    ordering::Any
end
MI355XCholesky() = MI355XCholesky(nothing)

# `LinearCache`'s `cacheval` field is parameterised on the type `init_cacheval` returns, so it must be a concrete
# MUTABLE holder from the start (returning `nothing` and assigning a backend later is a `convert` error). The
# backend handle is created by the first `solve!`; `colptr` / `rowval` remember the pattern it was analysed for.
mutable struct MI355XCacheval
    be::Union{Nothing, MI355XBackend}
    colptr::Vector{Int}
    rowval::Vector{Int}
end
LinearSolve.init_cacheval(::MI355XCholesky, A, b, u, Pl, Pr, maxiters, abstol, reltol, verbose, assumptions) =
    MI355XCacheval(nothing, Int[], Int[])
# deepcopy(cache) (gaussian_approximation.jl:103-109): the default field-wise deepcopy of the holder reaches
# `deepcopy_internal(::MI355XBackend)` above, i.e. gmrfx_clone -- the factor survives the fork.

function SciMLBase.solve!(cache::LinearSolve.LinearCache, alg::MI355XCholesky; kwargs...)
    A = cache.A isa Symmetric ? parent(cache.A) : cache.A
    cv = LinearSolve.@get_cacheval(cache, :MI355XCholesky)::MI355XCacheval
    if cache.isfresh
        cp, rv = SparseArrays.getcolptr(A), rowvals(A)
        if cv.be === nothing || cv.colptr != cp || cv.rowval != rv        # first solve!, or cache.A got a new pattern
            h = create(A; ordering = alg.ordering, check_posdef = true)     # seam A throws PosDefException
            cv.be = MI355XBackend(h, size(A, 1), nothing, nothing)
            cv.colptr, cv.rowval = copy(cp), copy(rv)
        end
        refactorize!(cv.be, Symmetric(A))
        cache.isfresh = false
    end
    cache.u .= backend_solve(cv.be::MI355XBackend, cache.b)
    return SciMLBase.build_linear_solution(alg, cache.u, nothing, cache)
end
_be(cache) = (LinearSolve.@get_cacheval(cache, :MI355XCholesky)::MI355XCacheval).be::MI355XBackend
G.supports_selinv(::MI355XCholesky) = Val{true}()
G.supports_backward_solve(::MI355XCholesky) = Val{true}()
G._selinv_diag_impl(cache, ::MI355XCholesky) = get_selinv_diag(_be(cache))
G._selinv_impl(cache, ::MI355XCholesky) = Symmetric(get_selinv(_be(cache)))
G._backward_solve_impl(cache, x, ::MI355XCholesky) = backend_backward_solve(_be(cache), x)
G._backward_solve_impl(cache, Z::Matrix{Float64}, ::MI355XCholesky) = backend_backward_solve(_be(cache), Z)
# seam-A twin of the batched sampler above (src/gmrf.jl:271-281 draws the columns one by one). Restricted BY DISPATCH to GMRFs whose
# LinearSolve cache carries this plug-in's algorithm: `GMRF` has its cache type as its sixth parameter (src/gmrf.jl:144-156) and
# `LinearSolve.LinearCache{TA, Tb, Tu, Tp, Talg, ...}` its algorithm type as its fifth (LinearSolve 2 and 3, the compat range of
# the reference's Project.toml; checked when the module loads). Every other GMRF keeps Distributions' own matrix method -- the
# plug-in owns a type in the signature (`MI355XCholesky`), so this is no piracy on Distributions / GaussianMarkovRandomFields.
let body = Base.unwrap_unionall(LinearSolve.LinearCache)
    body.parameters[5] === fieldtype(body, :alg) ||
        error("GMRFX: LinearSolve.LinearCache no longer has its algorithm as fifth type parameter; adjust MI355XLinearCache")
end
const MI355XLinearCache = LinearSolve.LinearCache{<:Any, <:Any, <:Any, <:Any, MI355XCholesky}
const MI355XGMRF = G.GMRF{<:Any, <:Any, <:Any, <:Any, <:Any, <:MI355XLinearCache}
function Distributions._rand!(rng::AbstractRNG, d::MI355XGMRF, X::AbstractMatrix{<:Real})
    Z = randn!(rng, Matrix{Float64}(undef, size(X, 1), size(X, 2)))
    X .= G.backward_solve(d.linsolve_cache, Z) .+ d.mean
    return X
end
# seam-A methods of the two RBMC strategies (src/gmrf.jl:318-332 -> src/solvers/rbmc.jl:71-87, :124-158). `MI355XGMRF` is the plug-in's own
# alias (its cache type carries `MI355XCholesky`), so, as for `_rand!` above, this is no piracy: every other GMRF keeps the reference's
# generic host methods. The draws come from the strategy's rng, column by column, as the reference's k `rand!` calls would take them.
function G.var(d::MI355XGMRF, s::G.RBMCStrategy)
    Z = randn!(s.rng, Matrix{Float64}(undef, length(d.mean), s.n_samples))
    return rbmc_var(_be(d.linsolve_cache), Z)
end
function G.var(d::MI355XGMRF, s::G.BlockRBMCStrategy)
    Z = randn!(s.rng, Matrix{Float64}(undef, length(d.mean), s.n_samples))
    return rbmc_var(_be(d.linsolve_cache), Z; enclosure_size = s.enclosure_size)
end
G._logdet_cov_impl(cache, ::MI355XCholesky) = -compute_logdet(_be(cache))       # note the sign (logdet.jl:30)
G.prepare_for_linsolve(A::SparseMatrixCSC, ::MI355XCholesky) = Symmetric(A)
G.configure_algorithm(alg::MI355XCholesky) = alg
# Val{true}() / Val{false}() like every method of this predicate (linsolve_utils.jl:49-56): `_resolve_linsolve`
# dispatches on the Val; dense or SymTridiagonal storage falls back to LinearSolve's default
G.algorithm_applicable(::MI355XCholesky, ::Union{SparseMatrixCSC, Symmetric{<:Any, <:SparseMatrixCSC}}) = Val{true}()
G.algorithm_applicable(::MI355XCholesky, ::AbstractMatrix) = Val{false}()

export MI355XBackend, MI355XCholesky, MI355XCacheval, ordering_permutation, ShardedMI355X, rccl_unique_id, MI355XBatch
end # module
