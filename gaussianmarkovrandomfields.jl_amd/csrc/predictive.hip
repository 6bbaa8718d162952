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
//   k_pred_final     the four totals: a strided loop over the workgroups' partials and a tree, as k_fisher_final
// B is read where the constraint keeps it (n x m column-major, stride n between columns): a row of A touches a few nodes, so a
// transposed copy (8 n m bytes more, a launch per factorisation) would save nothing a lane group could use.
// DETERMINISM. No atomics. A lane adds entries q0 + l, q0 + l + 16, ... in that order, the 16 lane sums meet in a fixed xor butterfly
// (which leaves the sum in every lane); the squares of the correction are added for l = 0, 1, ... in that order; the 16 observations of
// a workgroup meet in a fixed LDS tree, the workgroups in a fixed strided loop and tree. Every operand is read and written one double
// at a time: nothing depends on alignment. Contraction is off in the whole file; every fused multiply-add is written as one.
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
    const long long i = (long long)blockIdx.x * kPredNode + threadIdx.x;
    if (i >= a.nobs) return;
    const int j = a.idx[i];
    const double mu = a.x[j];
    if (a.mu_eta) a.mu_eta[i] = mu;
    if (a.v_eta) {
        double v = a.Z[a.zoff[a.dpos[j]]];
        if (a.m > 0) {
            double s = 0.0;
            for (int l = 0; l < a.m; l++) { const double b = a.B[j + (long long)l * a.n]; s = __builtin_fma(b, b, s); }
            v = pred_clamp(v, s);
        }
        a.v_eta[i] = v;
    }
    if (a.pll) a.pll[i] = pred_loglik(a.family, mu, a.y[j], a.aux ? a.aux[j] : 0.0, a.param, a.logparam, a.c[i]);
}

__global__ __launch_bounds__(256) void k_pred_design(const PredMarg a) {
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;
    if (i >= a.nobs) return;         // (a whole lane group leaves together)
    const long long q0 = a.arp[i], q1 = a.arp[i + 1];
    double s = 0.0;
    for (long long q = q0 + l; q < q1; q += kDesignLanes) s = __builtin_fma(a.aval[q], a.x[a.acol[q]], s);
    s = pred_group_sum(s);
    const double mu = a.offset ? s + a.offset[i] : s;
    if (l == 0 && a.mu_eta) a.mu_eta[i] = mu;
    if (a.v_eta) {
        double v = 0.0;
        const long long o1 = a.optr[i + 1];
        for (long long q = a.optr[i] + l; q < o1; q += kDesignLanes) v = __builtin_fma(a.ow[q], a.Z[a.zoff[a.hmap[a.oidx[q]]]], v);
        v = pred_group_sum(v);
        if (a.m > 0) {
            double corr = 0.0;
            for (int k = 0; k < a.m; k++) {
                const double *__restrict__ Bk = a.B + (long long)k * a.n;
                double ab = 0.0;
                for (long long q = q0 + l; q < q1; q += kDesignLanes) ab = __builtin_fma(a.aval[q], Bk[a.acol[q]], ab);
                ab = pred_group_sum(ab);
                corr = __builtin_fma(ab, ab, corr);
            }
            v = pred_clamp(v, corr);
        }
        if (l == 0) a.v_eta[i] = v;
    }
    if (l == 0 && a.pll) a.pll[i] = pred_loglik(a.family, mu, a.y[i], a.aux ? a.aux[i] : 0.0, a.param, a.logparam, a.c[i]);
}

__global__ __launch_bounds__(256) void k_pred_scores(const PredScores a) {
    __shared__ double sp[4][kDesignRows];
    const int g = threadIdx.x / kDesignLanes, l = threadIdx.x % kDesignLanes;
    const long long i = (long long)blockIdx.x * kDesignRows + g;
    double lpd = 0.0, lcpo = 0.0, elp = 0.0, vlp = 0.0;
    if (i < a.nobs) {           // (a whole lane group takes the branch together)
        const double mu = a.mu[i], v = a.v[i];
        const long long j = a.idx ? a.idx[i] : i;
        const double y = a.y[j], aux = a.aux ? a.aux[j] : 0.0, c = a.c[i];
        const double s = sqrt(v);
        double lk[kPredNodesPerLane], wk[kPredNodesPerLane];
        double M = -INFINITY, Mn = -INFINITY, e = 0.0;
#pragma unroll
        for (int t = 0; t < kPredNodesPerLane; t++) {
            const int k = l + t * kDesignLanes;
            lk[t] = 0.0; wk[t] = 0.0;
            if (k < a.K) {
                wk[t] = a.w[k];
                lk[t] = pred_loglik(a.family, __builtin_fma(s, a.z[k], mu), y, aux, a.param, a.logparam, c);
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
            if (a.lpd) a.lpd[i] = lpd;
            if (a.lcpo) a.lcpo[i] = lcpo;
            if (a.elp) a.elp[i] = elp;
            if (a.vlp) a.vlp[i] = vlp;
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
    if (threadIdx.x < 4) a.part[4 * (long long)blockIdx.x + threadIdx.x] = sp[threadIdx.x][0];
}

__global__ __launch_bounds__(kFisherFinal) void k_pred_final(const double *__restrict__ part, int nb, double *__restrict__ out) {
    __shared__ double sh[4][kFisherFinal];
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

void launch_pred_marginals(hipStream_t st, const PredMarg &a, bool design) {
    if (a.nobs <= 0) return;
    if (design) hipLaunchKernelGGL(k_pred_design, dim3((unsigned)design_blocks(a.nobs)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_pred_node, dim3((unsigned)((a.nobs + kPredNode - 1) / kPredNode)), dim3(kPredNode), 0, st, a);
}

void launch_pred_scores(hipStream_t st, const PredScores &a, double *out4) {
    if (a.nobs <= 0) return;
    const int nb = design_blocks(a.nobs);
    hipLaunchKernelGGL(k_pred_scores, dim3((unsigned)nb), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_pred_final, dim3(1), dim3(kFisherFinal), 0, st, a.part, nb, out4);
}

}  // namespace gmrfx
