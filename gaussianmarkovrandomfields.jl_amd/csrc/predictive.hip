// predictive.hip -- what a user does with the posterior after the Gaussian approximation: the marginals of every observation's
// linear predictor (gmrfx_predictor_marginals; the reference forms them on the host, src/linear_predictor_marginals.jl:58-195, with
// the constraint correction and clamp of _subtract_constraint_correction!, :189-195) and the quadrature scores over them
// (gmrfx_predictive_scores; the pointwise log densities are the reference's pointwise_loglik,
// src/observation_models/exponential_family/pointwise_implementations.jl). With Sigma the selected inverse of the handle's factor:
//   mu_eta_i = x[idx_i]                                  design form: (A x)_i + b_i, the eta of k_design_eta / k_gap_point, bit for bit
//   v_eta_i  = Sigma[idx_i, idx_i]                       design form: sum_t ow_t Sigma[position of pair t], the c of k_gap_point
//   v_eta_i <- max(v_eta_i - sum_{l < m} ((a_i B)_l)^2, 0)      under the constraint flag only; a NaN stays one (k_con_var)
//   pll_i    = l_i(mu_eta_i) + c_i                       l of fisher_point.h, c_i the observation's constant (obs_const.h)
// and, with s_i = sqrt(v_i), l_k = l_i(mu_i + s_i z_k) + c_i over the caller's K <= 64 nodes and weights:
//   elp_i = sum_k w_k l_k      vlp_i = sum_k w_k (l_k - elp_i)^2
//   lpd_i = M + log sum_k w_k exp(l_k - M), M = max_k l_k            (-inf when M is)
//   lcpo_i = -(M' + log sum_k w_k exp(-l_k - M')), M' = max_k -l_k   (-inf when M' = +inf: a density of 0 at a node)
// A NaN or negative v_i gives NaN in all four.
//   k_pred_node      one thread per observation
//   k_pred_design    a lane group per row of A; (a_i B)_l: one lane-group sum per column l of B, squares added in the order of l
//   k_pred_scores    a lane group per observation, lane l owns the nodes l, l + 16, l + 32, l + 48; one partial of each total per workgroup
//   k_pred_design_comp, k_pred_scores_comp   the same two for a composite likelihood (gmrfx_obs_set_composite): l_i under the family and
//                    parameter of observation i's component (kernels.h: ObsComp), c_i from the per-component constants
//   k_pred_final     the four totals: a strided loop over the workgroups' partials and a tree, as k_fisher_final
// B is read where the constraint keeps it (n x m column-major, stride n between columns): a row of A touches a few nodes, so a
// transposed copy (8 n m bytes more, a launch per factorisation) would save nothing a lane group could use.
// DETERMINISM. No atomics. A lane adds entries q0 + l, q0 + l + 16, ... in that order, the 16 lane sums meet in a fixed xor butterfly
// (which leaves the sum in every lane); the squares of the correction are added for l = 0, 1, ... in that order; the 16 observations of
// a workgroup meet in a fixed LDS tree, the workgroups in a fixed strided loop and tree. Every operand is read and written one double
// at a time: nothing depends on alignment. Contraction is off in the whole file; every fused multiply-add is written as one.
// MEMBERS (batched handles, gmrfx_batch_predictor_marginals / gmrfx_batch_predictive_scores). Every kernel takes a member index from its
// grid (blockIdx.y; blockIdx.x in k_pred_final) and offsets what belongs to the member by the strides of its argument record: the point,
// its entries of the offset table of Z (the offsets are absolute: the forest's panels are one array), its block of B, its column of the
// constants, its outputs and partial sums. The tables, the data set and the quadrature rule are one copy. A plain handle launches one
// member with every stride zero and null param_k / active: the same loads, the same arithmetic, the same bits.
//   k_pred_mixture   one thread per observation, the members in ascending order: the weighted mixture of the members' predictive
//                    distributions (gmrfx_batch_predictive_mixture); its total through k_pred_final
// SELECTION MATRICES. With A = rows of the identity and no offset every sum has one term of weight 1: mu_eta, v_eta (corrected or
// not) and pll have the bits of the node form.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "fisher_point.h"

namespace gmrfx {

#pragma clang fp contract(off)

__device__ __forceinline__ double pred_group_sum(double s) {
#pragma unroll
    for (int sh = kDesignLanes / 2; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, kDesignLanes);
    return s;
}
__device__ __forceinline__ double pred_group_max(double s) {
#pragma unroll
    for (int sh = kDesignLanes / 2; sh > 0; sh >>= 1) s = fmax(s, __shfl_xor(s, sh, kDesignLanes));
    return s;
}
__device__ __forceinline__ double pred_clamp(double v, double s) {
    const double d = v - s;
    return d != d ? d : fmax(d, 0.0);           // (a NaN stays one: fmax would return the zero)
}
__device__ __forceinline__ double pred_loglik(int family, double eta, double y, double aux, double param, double logparam, double c) {
    double g, d, ll;
    fisher_point(family, eta, y, aux, param, logparam, g, d, ll);
    return ll + c;
}

__global__ __launch_bounds__(kPredNode) void k_pred_node(const PredMarg a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    const long long i = (long long)blockIdx.x * kPredNode + threadIdx.x;
    if (i >= a.nobs) return;
    const long long o = (long long)k * a.so + i;
    const int j = a.idx[i];
    const double mu = a.x[(long long)k * a.sx + j];
    if (a.mu_eta) a.mu_eta[o] = mu;
    if (a.v_eta) {
        double v = a.Z[a.zoff[(long long)k * a.sz + a.dpos[j]]];
        if (a.m > 0) {
            const double *__restrict__ B = a.B + (long long)k * a.sb;
            double s = 0.0;
            for (int l = 0; l < a.m; l++) { const double b = B[j + (long long)l * a.n]; s = __builtin_fma(b, b, s); }
            v = pred_clamp(v, s);
        }
        a.v_eta[o] = v;
    }
    if (a.pll)
        a.pll[o] = pred_loglik(a.family, mu, a.y[j], a.aux ? a.aux[j] : 0.0, a.param_k ? a.param_k[k] : a.param,
                               a.logparam_k ? a.logparam_k[k] : a.logparam, a.c[(long long)k * a.sc + i]);
}

__global__ __launch_bounds__(256) void k_pred_design(const PredMarg a) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;
    if (i >= a.nobs) return;         // (a whole lane group leaves together)
    const long long o = (long long)k * a.so + i;
    const double *__restrict__ x = a.x + (long long)k * a.sx;
    const long long q0 = a.arp[i], q1 = a.arp[i + 1];
    double s = 0.0;
    for (long long q = q0 + l; q < q1; q += kDesignLanes) s = __builtin_fma(a.aval[q], x[a.acol[q]], s);
    s = pred_group_sum(s);
    const double mu = a.offset ? s + a.offset[i] : s;
    if (l == 0 && a.mu_eta) a.mu_eta[o] = mu;
    if (a.v_eta) {
        const long long *__restrict__ zoff = a.zoff + (long long)k * a.sz;
        double v = 0.0;
        const long long o1 = a.optr[i + 1];
        for (long long q = a.optr[i] + l; q < o1; q += kDesignLanes) v = __builtin_fma(a.ow[q], a.Z[zoff[a.hmap[a.oidx[q]]]], v);
        v = pred_group_sum(v);
        if (a.m > 0) {
            const double *__restrict__ B = a.B + (long long)k * a.sb;
            double corr = 0.0;
            for (int c = 0; c < a.m; c++) {
                const double *__restrict__ Bc = B + (long long)c * a.n;
                double ab = 0.0;
                for (long long q = q0 + l; q < q1; q += kDesignLanes) ab = __builtin_fma(a.aval[q], Bc[a.acol[q]], ab);
                ab = pred_group_sum(ab);
                corr = __builtin_fma(ab, ab, corr);
            }
            v = pred_clamp(v, corr);
        }
        if (l == 0) a.v_eta[o] = v;
    }
    if (l == 0 && a.pll)
        a.pll[o] = pred_loglik(a.family, mu, a.y[i], a.aux ? a.aux[i] : 0.0, a.param_k ? a.param_k[k] : a.param,
                               a.logparam_k ? a.logparam_k[k] : a.logparam, a.c[(long long)k * a.sc + i]);
}

// k_pred_design for a composite likelihood (kernels.h: ObsComp): the same statements -- mean and variance do not depend on the family
// -- except that lane 0 takes the row's (family, param, logparam) from the component table. KEEP THE TWO IN STEP: the body is written
// twice because sharing it through an inlined function gives k_pred_design another instruction schedule; the
// one-component test of tests/test_gpu_composite.py compares their bits.
__global__ __launch_bounds__(256) void k_pred_design_comp(const PredMarg a, const ObsComp t) {
    const int k = blockIdx.y;
    if (a.active && !a.active[k]) return;
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;
    if (i >= a.nobs) return;         // (a whole lane group leaves together)
    const long long o = (long long)k * a.so + i;
    const double *__restrict__ x = a.x + (long long)k * a.sx;
    const long long q0 = a.arp[i], q1 = a.arp[i + 1];
    double s = 0.0;
    for (long long q = q0 + l; q < q1; q += kDesignLanes) s = __builtin_fma(a.aval[q], x[a.acol[q]], s);
    s = pred_group_sum(s);
    const double mu = a.offset ? s + a.offset[i] : s;
    if (l == 0 && a.mu_eta) a.mu_eta[o] = mu;
    if (a.v_eta) {
        const long long *__restrict__ zoff = a.zoff + (long long)k * a.sz;
        double v = 0.0;
        const long long o1 = a.optr[i + 1];
        for (long long q = a.optr[i] + l; q < o1; q += kDesignLanes) v = __builtin_fma(a.ow[q], a.Z[zoff[a.hmap[a.oidx[q]]]], v);
        v = pred_group_sum(v);
        if (a.m > 0) {
            const double *__restrict__ B = a.B + (long long)k * a.sb;
            double corr = 0.0;
            for (int c = 0; c < a.m; c++) {
                const double *__restrict__ Bc = B + (long long)c * a.n;
                double ab = 0.0;
                for (long long q = q0 + l; q < q1; q += kDesignLanes) ab = __builtin_fma(a.aval[q], Bc[a.acol[q]], ab);
                ab = pred_group_sum(ab);
                corr = __builtin_fma(ab, ab, corr);
            }
            v = pred_clamp(v, corr);
        }
        if (l == 0) a.v_eta[o] = v;
    }
    if (l == 0 && a.pll) {
        const int c = t.comp[i];
        a.pll[o] = pred_loglik(t.family[c], mu, a.y[i], a.aux ? a.aux[i] : 0.0, t.param[c], t.logparam[c], a.c[(long long)k * a.sc + i]);
    }
}

// k_pred_scores and k_pred_scores_comp (COMP: the observation's family and parameter from the component table; every lane of the group
// reads its observation's component, the same address). COMP = false reads no table.
template <bool COMP>
__device__ __forceinline__ void pred_scores_rows(const PredScores &a, const ObsComp &tab) {
    __shared__ double sp[4][kDesignRows];
    const int m = blockIdx.y;
    if (a.active && !a.active[m]) return;       // (the whole workgroup: nobody waits at the barriers below)
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;
    double lpd = 0.0, lcpo = 0.0, elp = 0.0, vlp = 0.0;
    if (i < a.nobs) {           // (a whole lane group takes the branch together)
        const long long o = (long long)m * a.so + i;
        const double mu = a.mu[(long long)m * a.sm + i], v = a.v[(long long)m * a.sm + i];
        const long long j = a.idx ? a.idx[i] : i;
        const double y = a.y[j], aux = a.aux ? a.aux[j] : 0.0, c = a.c[(long long)m * a.sc + i];
        int family;
        double param, logparam;
        if constexpr (COMP) {
            const int cm = tab.comp[i];
            family = tab.family[cm]; param = tab.param[cm]; logparam = tab.logparam[cm];
        } else {
            family = a.family;
            param = a.param_k ? a.param_k[m] : a.param; logparam = a.logparam_k ? a.logparam_k[m] : a.logparam;
        }
        const double s = sqrt(v);
        double lk[kPredNodesPerLane], wk[kPredNodesPerLane];
        double M = -INFINITY, Mn = -INFINITY, e = 0.0;
#pragma unroll
        for (int t = 0; t < kPredNodesPerLane; t++) {
            const int k = l + t * kDesignLanes;
            lk[t] = 0.0; wk[t] = 0.0;
            if (k < a.K) {
                wk[t] = a.w[k];
                lk[t] = pred_loglik(family, __builtin_fma(s, a.z[k], mu), y, aux, param, logparam, c);
                M = fmax(M, lk[t]);
                Mn = fmax(Mn, -lk[t]);
                e = __builtin_fma(wk[t], lk[t], e);
            }
        }
        M = pred_group_max(M);
        Mn = pred_group_max(Mn);
        elp = pred_group_sum(e);
        double sl = 0.0, sc = 0.0, q = 0.0;
#pragma unroll
        for (int t = 0; t < kPredNodesPerLane; t++) {
            const int k = l + t * kDesignLanes;
            if (k < a.K) {
                const double d = lk[t] - elp;
                sl = __builtin_fma(wk[t], exp(lk[t] - M), sl);
                sc = __builtin_fma(wk[t], exp(-lk[t] - Mn), sc);
                q = __builtin_fma(wk[t], d * d, q);
            }
        }
        sl = pred_group_sum(sl);
        sc = pred_group_sum(sc);
        vlp = pred_group_sum(q);
        lpd = M == -INFINITY ? M : M + log(sl);
        lcpo = Mn == INFINITY ? -INFINITY : -(Mn + log(sc));
        if (!(v >= 0.0)) lpd = lcpo = elp = vlp = NAN;          // (a NaN or negative variance)
        if (l == 0) {
            if (a.lpd) a.lpd[o] = lpd;
            if (a.lcpo) a.lcpo[o] = lcpo;
            if (a.elp) a.elp[o] = elp;
            if (a.vlp) a.vlp[o] = vlp;
        }
    }
    if (l == 0) { sp[0][g] = lpd; sp[1][g] = lcpo; sp[2][g] = elp; sp[3][g] = vlp; }
    __syncthreads();
    for (int st = kDesignRows / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
#pragma unroll
            for (int r = 0; r < 4; r++) sp[r][threadIdx.x] += sp[r][threadIdx.x + st];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) a.part[4 * ((long long)m * gridDim.x + blockIdx.x) + threadIdx.x] = sp[threadIdx.x][0];
}
__global__ __launch_bounds__(256) void k_pred_scores(const PredScores a) { pred_scores_rows<false>(a, ObsComp{}); }
__global__ __launch_bounds__(256) void k_pred_scores_comp(const PredScores a, const ObsComp t) { pred_scores_rows<true>(a, t); }

// one workgroup per member: member k's nb partial quadruples at part + 4 k nb, its totals at out + 4 k
__global__ __launch_bounds__(kFisherFinal) void k_pred_final(const double *__restrict__ part, int nb, const unsigned char *__restrict__ active,
                                                             double *__restrict__ out) {
    __shared__ double sh[4][kFisherFinal];
    const int k = blockIdx.x;
    if (active && !active[k]) return;
    part += 4 * (long long)k * nb;
    out += 4 * (long long)k;
    const int tid = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < nb; b += kFisherFinal) {
#pragma unroll
        for (int r = 0; r < 4; r++) s[r] += part[4 * (long long)b + r];
    }
#pragma unroll
    for (int r = 0; r < 4; r++) sh[r][tid] = s[r];
    __syncthreads();
    for (int st = kFisherFinal / 2; st > 0; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int r = 0; r < 4; r++) sh[r][tid] += sh[r][tid + st];
        }
        __syncthreads();
    }
    if (tid < 4) out[tid] = sh[tid][0];
}

// The mixture of the members' predictive distributions, one thread per observation, the members in ascending order. The first included
// member's term is a plain product and every later one a fused multiply-add onto it, so one member of weight 1 hands its inputs through
// bit for bit. An excluded member (log omega = -inf) is never read; an included member's NaN propagates (fmax alone would drop it from
// the maximum: it is carried beside it). The workgroup's sum of mix_lpd: a fixed LDS tree over its kPredMix threads.
__global__ __launch_bounds__(kPredMix) void k_pred_mixture(const PredMix a) {
    __shared__ double sh[kPredMix];
    const long long i = (long long)blockIdx.x * kPredMix + threadIdx.x;
    const double *__restrict__ om = a.w, *__restrict__ lw = a.w + a.nbatch;
    double total = 0.0;
    if (i < a.nobs) {
        if (a.mix_mu || a.mix_v) {
            double mm = 0.0;
            bool first = true;
            for (int k = 0; k < a.nbatch; k++) {
                if (lw[k] == -INFINITY) continue;
                const double mu = a.mu[(long long)k * a.nobs + i];
                mm = first ? om[k] * mu : __builtin_fma(om[k], mu, mm);
                first = false;
            }
            if (a.mix_mu) a.mix_mu[i] = mm;
            if (a.mix_v) {
                double mv = 0.0;
                first = true;
                for (int k = 0; k < a.nbatch; k++) {
                    if (lw[k] == -INFINITY) continue;
                    const double d = a.mu[(long long)k * a.nobs + i] - mm;
                    const double t = __builtin_fma(d, d, a.v[(long long)k * a.nobs + i]);
                    mv = first ? om[k] * t : __builtin_fma(om[k], t, mv);
                    first = false;
                }
                a.mix_v[i] = mv;
            }
        }
        if (a.lpd) {
            double M = -INFINITY, bad = 0.0;
            for (int k = 0; k < a.nbatch; k++) {
                if (lw[k] == -INFINITY) continue;
                const double t = lw[k] + a.lpd[(long long)k * a.nobs + i];
                if (t != t) bad = t;
                M = fmax(M, t);
            }
            double r = M;
            if (bad != bad) r = bad;
            else if (M != -INFINITY) {
                double s = 0.0;
                for (int k = 0; k < a.nbatch; k++) {
                    if (lw[k] == -INFINITY) continue;
                    s += exp(lw[k] + a.lpd[(long long)k * a.nobs + i] - M);
                }
                r = M + log(s);
            }
            if (a.mix_lpd) a.mix_lpd[i] = r;
            total = r;
        }
    }
    if (!a.lpd) return;
    sh[threadIdx.x] = total;
    __syncthreads();
    for (int st = kPredMix / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x < 4) a.part[4 * (long long)blockIdx.x + threadIdx.x] = threadIdx.x == 0 ? sh[0] : 0.0;
}

void launch_pred_marginals(hipStream_t st, const PredMarg &a, bool design, int nbatch) {
    if (a.nobs <= 0 || nbatch <= 0) return;
    if (design) hipLaunchKernelGGL(k_pred_design, dim3((unsigned)design_blocks(a.nobs), (unsigned)nbatch), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_pred_node, dim3((unsigned)((a.nobs + kPredNode - 1) / kPredNode), (unsigned)nbatch), dim3(kPredNode), 0, st, a);
}

void launch_pred_marginals_comp(hipStream_t st, const PredMarg &a, const ObsComp &t, int nbatch) {
    if (a.nobs <= 0 || nbatch <= 0) return;
    hipLaunchKernelGGL(k_pred_design_comp, dim3((unsigned)design_blocks(a.nobs), (unsigned)nbatch), dim3(256), 0, st, a, t);
}

void launch_pred_scores_comp(hipStream_t st, const PredScores &a, const ObsComp &t, int nbatch, double *out4) {
    if (a.nobs <= 0 || nbatch <= 0) return;
    const int nb = design_blocks(a.nobs);
    hipLaunchKernelGGL(k_pred_scores_comp, dim3((unsigned)nb, (unsigned)nbatch), dim3(256), 0, st, a, t);
    hipLaunchKernelGGL(k_pred_final, dim3((unsigned)nbatch), dim3(kFisherFinal), 0, st, a.part, nb, a.active, out4);
}

void launch_pred_scores(hipStream_t st, const PredScores &a, int nbatch, double *out4) {
    if (a.nobs <= 0 || nbatch <= 0) return;
    const int nb = design_blocks(a.nobs);
    hipLaunchKernelGGL(k_pred_scores, dim3((unsigned)nb, (unsigned)nbatch), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_pred_final, dim3((unsigned)nbatch), dim3(kFisherFinal), 0, st, a.part, nb, a.active, out4);
}

void launch_pred_mixture(hipStream_t st, const PredMix &a, double *out4) {
    if (a.nobs <= 0 || a.nbatch <= 0) return;
    const int nb = pred_mix_blocks(a.nobs);
    hipLaunchKernelGGL(k_pred_mixture, dim3((unsigned)nb), dim3(kPredMix), 0, st, a);
    if (a.lpd) hipLaunchKernelGGL(k_pred_final, dim3(1), dim3(kFisherFinal), 0, st, a.part, nb, (const unsigned char *)nullptr, out4);
}

}  // namespace gmrfx
