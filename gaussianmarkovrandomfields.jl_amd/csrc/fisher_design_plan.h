// fisher_design_plan.h -- host analysis of a likelihood observed through a sparse design matrix, eta = A x + b (fisher_design_plan.cpp,
// no HIP; gmrfx_obs_set_design). Built once per call and kept on the handle (shared with its clones: the plan is immutable);
// Device::obs_set uploads the tables as they are. Reference: LinearlyTransformedLikelihood (src/observation_models/
// linearly_transformed.jl:313-340: loggrad = A' g, loghessian = A' D A) and _sparse_hessian_map (src/workspace/gaussian_approximation.jl:73-129).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "rbmc_plan.h"

namespace gmrfx {

struct DesignPlan {
    i64 n = 0, nobs = 0, nnz = 0, cnt = 0, terms = 0;
    // A by rows (for eta; columns ascending within a row) and by columns (for A' g; rows ascending), 0-based, explicit zeros kept
    std::vector<i64> rptr, cptr;
    std::vector<i32> rcol, crow;
    std::vector<double> rval, cval;
    std::vector<double> offset;          // nobs, or empty: b = 0
    // The Hessian A' D A on Q's pattern: map[p] = position in the handle's nzval (the triangle in use) of the p-th unordered pair (j, k)
    // with a common row in A, ascending; the pair's terms (i_t, w_t = A[i_t, j] A[i_t, k]) in ascending i_t at tptr[p] .. tptr[p + 1].
    std::vector<i64> map, tptr;
    std::vector<i32> tobs;
    std::vector<double> tw;
    // The transpose of the term table (gmrfx_ga_pullback: c_i = a_i' G a_i): per observation i, at optr[i] .. optr[i + 1], the pairs of
    // row i as (oidx = the pair's index p in map, ow = w_t, doubled off the diagonal), ascending in p and so in position. An index into
    // map is below cnt <= terms < 2^31: 32 bits always do.
    std::vector<i64> optr;
    std::vector<i32> oidx;
    std::vector<double> ow;
};

// Throws std::invalid_argument when n, nobs or nnz(A) is 2^31 or above: before anything of that length is read.
void design_check_sizes(i64 n, i64 nobs, i64 nnz, const std::string &who = "obs_set_design: ");
// A: nobs x n in CSC with ptr[0] == index_base and a monotone colptr (the caller has checked both). Throws std::invalid_argument
// (P unchanged) for a row index outside [0, nobs), unsorted or repeated row indices within a column, a non-finite value of A or
// offset, a pair (j, k) of pattern(A'A) that Q does not store (the first one, named in the caller's index base), and for n, nobs,
// nnz(A) or the term count at 2^31 or above. nnzq: stored entries of Q. who: the prefix of the messages (the entry point's name).
void design_build_plan(const RbmcSym &R, i64 n, i64 nnzq, i64 nobs, const int64_t *colptr, const int64_t *rowval, const double *nzval,
                       int index_base, const double *offset, DesignPlan &P, const std::string &who = "obs_set_design: ");

}  // namespace gmrfx
