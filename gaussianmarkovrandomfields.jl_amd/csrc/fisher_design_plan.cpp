// fisher_design_plan.cpp -- host analysis of eta = A x + b (fisher_design_plan.h). No HIP.
//   (a) validation of A and b, A by columns (as given) and by rows (one counting pass: columns stay ascending within a row);
//   (b) the Hessian's positions: every pair (j <= k) of a row of A is looked up in row j of Symmetric(Q) (RbmcSym, binary search), a
//       counting sort by position keeps the observation indices ascending within a pair's term list. O(terms log(row of Q)).
#include "fisher_design_plan.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>

namespace gmrfx {

static constexpr i64 kDesignIndexLimit = (i64)1 << 31;

void design_check_sizes(i64 n, i64 nobs, i64 nnz, const std::string &who) {
    if (n >= kDesignIndexLimit || nobs >= kDesignIndexLimit || nnz >= kDesignIndexLimit)
        throw std::invalid_argument(who + "n, nobs or nnz(A) is 2^31 or above");
}

void design_build_plan(const RbmcSym &R, i64 n, i64 nnzq, i64 nobs, const int64_t *colptr, const int64_t *rowval, const double *nzval,
                       int index_base, const double *offset, DesignPlan &out, const std::string &who) {
    const i64 nnz = colptr[n] - index_base;
    design_check_sizes(n, nobs, nnz, who);
    DesignPlan P;
    P.n = n; P.nobs = nobs; P.nnz = nnz;
    P.cptr.resize((size_t)n + 1);
    P.crow.resize((size_t)nnz);
    P.cval.assign(nzval, nzval + nnz);
    P.rptr.assign((size_t)nobs + 1, 0);
    for (i64 j = 0; j <= n; j++) P.cptr[(size_t)j] = colptr[j] - index_base;
    for (i64 j = 0; j < n; j++)
        for (i64 q = P.cptr[(size_t)j]; q < P.cptr[(size_t)j + 1]; q++) {
            const i64 i = rowval[q] - index_base;
            const std::string at = " (column " + std::to_string(j + index_base) + ")";
            if (i < 0 || i >= nobs) throw std::invalid_argument(who + "a row index of A is outside [0, nobs)" + at);
            if (q > P.cptr[(size_t)j] && i <= rowval[q - 1] - index_base)
                throw std::invalid_argument(who + "row indices of A are unsorted or repeated within a column" + at);
            if (!std::isfinite(nzval[q])) throw std::invalid_argument(who + "a value of A is not finite" + at);
            P.crow[(size_t)q] = (i32)i;
            P.rptr[(size_t)i + 1]++;
        }
    if (offset) {
        for (i64 i = 0; i < nobs; i++)
            if (!std::isfinite(offset[i])) throw std::invalid_argument(who + "offset is not finite (observation " + std::to_string(i) + ")");
        P.offset.assign(offset, offset + nobs);
    }
    i64 terms = 0;
    for (i64 i = 0; i < nobs; i++) {
        const i64 r = P.rptr[(size_t)i + 1];
        terms += r * (r + 1) / 2;
        if (terms >= kDesignIndexLimit) throw std::invalid_argument(who + "A' D A has 2^31 terms or more");
        P.rptr[(size_t)i + 1] += P.rptr[(size_t)i];
    }
    P.terms = terms;
    P.rcol.resize((size_t)nnz);
    P.rval.resize((size_t)nnz);
    {
        std::vector<i64> fill(P.rptr.begin(), P.rptr.end() - 1);
        for (i64 j = 0; j < n; j++)
            for (i64 q = P.cptr[(size_t)j]; q < P.cptr[(size_t)j + 1]; q++) {
                const i64 d = fill[(size_t)P.crow[(size_t)q]]++;
                P.rcol[(size_t)d] = (i32)j;
                P.rval[(size_t)d] = P.cval[(size_t)q];
            }
    }
    // pass 1: the position of every term, in generation order (row by row, pairs a <= b of the row), and the terms per position
    std::vector<i64> tpos((size_t)terms);
    std::vector<i32> slot((size_t)nnzq, 0);
    i64 t = 0;
    for (i64 i = 0; i < nobs; i++)
        for (i64 a = P.rptr[(size_t)i]; a < P.rptr[(size_t)i + 1]; a++) {
            const i64 j = P.rcol[(size_t)a];
            const auto lo = R.col.begin() + R.rowptr[(size_t)j], hi = R.col.begin() + R.rowptr[(size_t)j + 1];
            auto it = lo;
            for (i64 b = a; b < P.rptr[(size_t)i + 1]; b++) {
                const i32 k = P.rcol[(size_t)b];
                it = std::lower_bound(it, hi, k);      // (the columns of a row of A ascend, so does the search)
                if (it == hi || *it != k)
                    throw std::invalid_argument(who + "pattern(A'A) is not contained in the pattern of Q: entry (" + std::to_string(j + index_base) +
                                                ", " + std::to_string(k + index_base) + ") is missing (row " + std::to_string(i + index_base) + " of A)");
                const i64 p = R.pos[(size_t)(it - R.col.begin())];
                tpos[(size_t)t++] = p;
                slot[(size_t)p]++;
            }
        }
    // positions in ascending order; slot[p] becomes the index of position p in the map
    P.tptr.push_back(0);
    for (i64 p = 0; p < nnzq; p++)
        if (slot[(size_t)p] > 0) {
            P.tptr.push_back(P.tptr.back() + slot[(size_t)p]);
            slot[(size_t)p] = (i32)P.map.size();
            P.map.push_back(p);
        }
    P.cnt = (i64)P.map.size();
    // pass 2: the same order again; rows ascend, so every term list does. The same terms by observation (the transposed table): a
    // row's pairs are one run of the generation order, sorted by map index afterwards
    P.tobs.resize((size_t)terms);
    P.tw.resize((size_t)terms);
    P.optr.assign((size_t)nobs + 1, 0);
    P.oidx.resize((size_t)terms);
    P.ow.resize((size_t)terms);
    std::vector<std::pair<i32, double>> rowlist;
    std::vector<i64> cur(P.tptr.begin(), P.tptr.end() - 1);
    t = 0;
    for (i64 i = 0; i < nobs; i++) {
        rowlist.clear();
        for (i64 a = P.rptr[(size_t)i]; a < P.rptr[(size_t)i + 1]; a++)
            for (i64 b = a; b < P.rptr[(size_t)i + 1]; b++) {
                const i32 s = slot[(size_t)tpos[(size_t)t++]];
                const i64 d = cur[(size_t)s]++;
                P.tobs[(size_t)d] = (i32)i;
                P.tw[(size_t)d] = P.rval[(size_t)a] * P.rval[(size_t)b];
                rowlist.emplace_back(s, a == b ? P.tw[(size_t)d] : 2.0 * P.tw[(size_t)d]);
            }
        std::sort(rowlist.begin(), rowlist.end(), [](const std::pair<i32, double> &u, const std::pair<i32, double> &v) { return u.first < v.first; });
        const i64 o0 = P.optr[(size_t)i];
        for (size_t q = 0; q < rowlist.size(); q++) {
            P.oidx[(size_t)o0 + q] = rowlist[q].first;
            P.ow[(size_t)o0 + q] = rowlist[q].second;
        }
        P.optr[(size_t)i + 1] = o0 + (i64)rowlist.size();
    }
    out = std::move(P);
}

}  // namespace gmrfx
