// fisher_gather.h -- the gather over one row of Symmetric(Q_p) that k_fisher_eval (fisher.hip) and k_design_score (fisher_design.hip)
// share, so that the energy and Q_p x - h of the design form have the bits of the node form. Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace gmrfx {

// Lane l's share of row i: s += v x[c] and, with a mean, t += v mu[c] over the entries rp[i] + l, rp[i] + l + kFisherLanes, ... in that
// order, each one fused multiply-add. The caller joins the kFisherLanes lane sums with its own group sum (k_design_score's lane
// groups have kDesignLanes lanes: kernels.h asserts kDesignLanes == kFisherLanes).
__device__ __forceinline__ void fisher_row_gather(long long i, int l, const long long *rp, const int *col, const int *pos, const double *val,
                                                  const double *x, const double *mu, double &s, double &t) {
    const long long q1 = rp[i + 1];
    for (long long q = rp[i] + l; q < q1; q += kFisherLanes) {
        const double v = val[pos[q]];
        const int c = col[q];
        s = __builtin_fma(v, x[c], s);
        if (mu) t = __builtin_fma(v, mu[c], t);
    }
}

}  // namespace gmrfx
