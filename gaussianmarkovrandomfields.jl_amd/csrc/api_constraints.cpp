// api_constraints.cpp -- the C ABI of include/gmrfx.h: linear equality constraints A x = e of a plain handle and of the members of a batch.
#include <cmath>

#include "api_common.h"

// ---- linear equality constraints A x = e (include/gmrfx.h; Device::con_*, csrc/constraint.hip) --------------------------------------
// log det(A A') on the host: the m x m Gram matrix of the sparse rows through one dense scratch row, then a plain Cholesky
// (-inf when A A' is not positive definite: a rank-deficient A is reported by the numeric entry points, as the reference does)
static double logdet_gram(const ConHost &c, int64_t n) {
    const int m = c.m;
    std::vector<double> G((size_t)m * m, 0.0), row((size_t)n, 0.0);
    for (int r = 0; r < m; r++) {
        for (long long p = c.rowptr[r]; p < c.rowptr[r + 1]; p++) row[c.col[p]] = c.val[p];
        for (int s = 0; s <= r; s++) {
            double acc = 0.0;
            for (long long p = c.rowptr[s]; p < c.rowptr[s + 1]; p++) acc += c.val[p] * row[c.col[p]];
            G[(size_t)r * m + s] = acc;
        }
        for (long long p = c.rowptr[r]; p < c.rowptr[r + 1]; p++) row[c.col[p]] = 0.0;
    }
    double ld = 0.0;
    for (int j = 0; j < m; j++) {
        double d = G[(size_t)j * m + j];
        for (int q = 0; q < j; q++) d -= G[(size_t)j * m + q] * G[(size_t)j * m + q];
        if (!(d > 0.0)) return -HUGE_VAL;
        const double dj = std::sqrt(d);
        G[(size_t)j * m + j] = dj;
        ld += 2.0 * std::log(dj);
        for (int i = j + 1; i < m; i++) {
            double t = G[(size_t)i * m + j];
            for (int q = 0; q < j; q++) t -= G[(size_t)i * m + q] * G[(size_t)j * m + q];
            G[(size_t)i * m + j] = t / dj;
        }
    }
    return ld;
}

// A (m sparse rows over n columns) and e as the handle keeps them: validated, columns sorted, duplicates summed, log det(A A')
static ConHost read_constraints(int64_t n, int64_t m, const int64_t *rowptr, const int64_t *colind, const double *values, int32_t base,
                                const double *e) {
    ConHost c;
    if (m <= 0) return c;
    if (!rowptr || !colind || !values || !e) throw std::invalid_argument("constraints: null argument");
    check_index_base(base);
    check_compressed_ptr(rowptr, m, base, "rowptr");
    c.m = (int)m;
    c.rowptr.assign((size_t)m + 1, 0);
    c.e.assign(e, e + m);
    std::vector<std::pair<int, double>> ent;
    for (int64_t r = 0; r < m; r++) {
        if (rowptr[r + 1] == rowptr[r]) throw std::invalid_argument("constraints: row " + std::to_string(r) + " of A is empty");
        ent.clear();
        for (int64_t p = rowptr[r] - base; p < rowptr[r + 1] - base; p++) {
            const int64_t j = colind[p] - base;
            if (j < 0 || j >= n) throw std::invalid_argument("constraints: column index out of range");
            ent.push_back({(int)j, values[p]});
        }
        std::stable_sort(ent.begin(), ent.end(), [](const std::pair<int, double> &a, const std::pair<int, double> &b) { return a.first < b.first; });
        for (size_t t = 0; t < ent.size(); t++) {
            if (t > 0 && ent[t].first == ent[t - 1].first) c.val.back() += ent[t].second;      // duplicates are summed
            else { c.col.push_back(ent[t].first); c.val.push_back(ent[t].second); }
        }
        c.rowptr[(size_t)r + 1] = (long long)c.col.size();
    }
    c.logdet_AAt = logdet_gram(c, n);
    return c;
}

extern "C" int32_t gmrfx_constraints_set(gmrfx_handle *h, int64_t m, const int64_t *rowptr, const int64_t *colind, const double *values,
                                         int32_t base, const double *e) {
    return guarded(h, [&]() -> int32_t {
        // everything is checked and built aside first: a refused call changes nothing
        if (m < 0) throw std::invalid_argument("constraints: m < 0");
        if (m > 64) throw std::invalid_argument("constraints: more than 64 rows (the limit of the device path: one sweep pass, m x m operands in LDS)");
        if (h->nbatch > 1) throw std::invalid_argument("constraints: batched handles are not supported (their members take gmrfx_batch_constraints_set)");
        check_unsharded(h, "constraints: sharded handles are not supported");
        if (m > 0 && h->bcon.m > 0) throw std::invalid_argument("constraints: the handle holds a batch constraint (gmrfx_batch_constraints_set); clear it first");
        ConHost c = read_constraints(h->S.n, m, rowptr, colind, values, base, e);
        if (h->D) h->D->con_set(c);
        h->con = std::move(c);
        return GMRFX_OK;
    });
}

// the cached operands of the current factorisation (built on first use)
static int32_t con_ready(gmrfx_handle *h) {
    if (int32_t e = need_device(h, true)) return e;
    if (h->con.m > 0 && !h->D->con_prepare()) {
        h->err = "constraints: A Q^-1 A' is not positive definite (rank-deficient constraint matrix)";
        return GMRFX_ERR_NOT_POSDEF;
    }
    return GMRFX_OK;
}

extern "C" int32_t gmrfx_constraints_info(gmrfx_handle *h, int64_t *m, double *logdet_W, double *logdet_AAt, double *ms) {
    return guarded(h, [&]() -> int32_t {
        if (m) *m = h->con.m;
        if (logdet_AAt) *logdet_AAt = h->con.m > 0 ? h->con.logdet_AAt : 0.0;
        if (logdet_W) *logdet_W = 0.0;
        if (ms) *ms = 0.0;
        if (h->con.m == 0 || (!logdet_W && !ms)) return GMRFX_OK;
        if (int32_t e = con_ready(h)) return e;
        if (logdet_W) *logdet_W = h->D->con_logdet_w();
        if (ms) *ms = h->D->con_ms();
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_constraints_get(gmrfx_handle *h, double *A_tilde_T, int64_t ld, double *W) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = con_ready(h)) return e;
        if (A_tilde_T && ld < h->S.n) throw std::invalid_argument("constraints: ld < n");
        h->D->con_get(A_tilde_T, ld, W);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_constraints_mean(gmrfx_handle *h, const double *mu, double *mean_c, double *log_correction) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = con_ready(h)) return e;
        const int64_t n = h->S.n;
        const int m = h->con.m;
        DevBlock x;
        if (mu) stage_up(h, x, mu, n, n, 1);
        else stage_zeros(h, x, n);
        h->D->con_correct(x, n, 1, nullptr);
        if (mean_c) stage_down(h, x, mean_c, n, n, 1);
        if (log_correction) {
            *log_correction = 0.0;
            if (m > 0) {
                // 0.5 (m log 2 pi + log det W + r' W^-1 r) - 0.5 log det(A A'), r = e - A mu: r' W^-1 r = |L_c^-1 r|^2
                std::vector<double> r((size_t)m);
                h->D->con_residual(r.data());
                const std::vector<double> &Li = h->D->con_linv();
                double quad = 0.0;
                for (int l = 0; l < m; l++) {
                    double t = 0.0;
                    for (int q = 0; q <= l; q++) t += Li[(size_t)l * m + q] * r[q];
                    quad += t * t;
                }
                *log_correction = 0.5 * (m * std::log(2.0 * 3.14159265358979323846) + h->D->con_logdet_w() + quad) - 0.5 * h->con.logdet_AAt;
            }
        }
        return GMRFX_OK;
    });
}

static int32_t constraints_correct_impl(gmrfx_handle *h, double *X, int64_t ldx, int64_t nvec, bool dev) {
    return guarded(h, [&]() -> int32_t {
        check_block(h, X, ldx, nvec, "nvec", "X");
        if (int32_t e = con_ready(h)) return e;
        if (nvec == 0 || h->con.m == 0) return GMRFX_OK;
        if (dev) { h->D->con_correct(X, ldx, nvec, nullptr); return GMRFX_OK; }
        const int64_t n = h->S.n;
        DevBlock x;
        stage_up(h, x, X, ldx, n, nvec);
        h->D->con_correct(x, n, nvec, nullptr);
        stage_down(h, x, X, ldx, n, nvec);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_constraints_correct(gmrfx_handle *h, double *X, int64_t ldx, int64_t nvec) { return constraints_correct_impl(h, X, ldx, nvec, false); }
extern "C" int32_t gmrfx_constraints_correct_dev(gmrfx_handle *h, double *d_X, int64_t ldx, int64_t nvec) { return constraints_correct_impl(h, d_X, ldx, nvec, true); }

extern "C" int32_t gmrfx_constraints_var(gmrfx_handle *h, double *out) {
    return guarded(h, [&]() -> int32_t {
        if (!out) throw std::invalid_argument("out is null");
        if (int32_t e = con_ready(h)) return e;
        h->D->con_var(out);
        return GMRFX_OK;
    });
}

static int32_t sample_impl(gmrfx_handle *h, const double *Z, int64_t ldz, int64_t nrhs, const double *mu, double *X, int64_t ldx, bool dev) {
    return guarded(h, [&]() -> int32_t {
        check_rhs(h, Z, ldz, X, ldx, nrhs, "Z/X");
        if (int32_t e = con_ready(h)) return e;
        if (nrhs == 0) return GMRFX_OK;
        if (dev) {
            h->D->solve(Z, ldz, nrhs, X, ldx, true, 1);
            h->D->con_correct(X, ldx, nrhs, mu);
            return GMRFX_OK;
        }
        if (h->con.m == 0 && !mu) { h->D->solve(Z, ldz, nrhs, X, ldx, false, 1); return GMRFX_OK; }     // = gmrfx_backward_solve
        const int64_t n = h->S.n;
        DevBlock x, dm;
        stage_up(h, x, Z, ldz, n, nrhs);
        if (mu) stage_up(h, dm, mu, n, n, 1);
        h->D->solve(x, n, nrhs, x, n, true, 1);
        h->D->con_correct(x, n, nrhs, dm);
        stage_down(h, x, X, ldx, n, nrhs);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_sample(gmrfx_handle *h, const double *Z, int64_t ldz, int64_t nrhs, const double *mu, double *X, int64_t ldx) {
    return sample_impl(h, Z, ldz, nrhs, mu, X, ldx, false);
}
extern "C" int32_t gmrfx_sample_dev(gmrfx_handle *h, const double *d_Z, int64_t ldz, int64_t nrhs, const double *d_mu, double *d_X, int64_t ldx) {
    return sample_impl(h, d_Z, ldz, nrhs, d_mu, d_X, ldx, true);
}

// ---- the constraint of every member of a batch (include/gmrfx.h; Device::bcon_*, csrc/constraint.hip) -------------------------------
extern "C" int32_t gmrfx_batch_constraints_set(gmrfx_handle *h, int64_t m, const int64_t *rowptr, const int64_t *colind, const double *values,
                                               int32_t base, const double *e) {
    return guarded(h, [&]() -> int32_t {
        if (m < 0) throw std::invalid_argument("batch constraints: m < 0");
        if (m > 64) throw std::invalid_argument("batch constraints: more than 64 rows (the limit of the device path: one sweep pass, m x m operands in LDS)");
        check_unsharded(h, "batch constraints: sharded handles are not supported");
        if (m > 0 && h->con.m > 0) throw std::invalid_argument("batch constraints: the handle holds a plain constraint (gmrfx_constraints_set); clear it first");
        ConHost c = read_constraints(h->n_member, m, rowptr, colind, values, base, e);
        if (h->D) {
            if (m > 0 && !h->D->batched()) h->D->set_batch(1, h->S.n, h->S.nnz_in);       // a plain handle: a batch of one
            try {
                h->D->bcon_set(c);
            } catch (const std::bad_alloc &) {
                h->err = "batch constraints: the two n x B x m operand arrays do not fit into device memory";
                return GMRFX_ERR_ALLOC;
            }
        }
        h->bcon = std::move(c);
        return GMRFX_OK;
    });
}

// the members' cached operands of the current factorisation (built on first use). NOT_POSDEF: W_k failed for a member whose
// factorisation succeeded; a member whose factorisation failed is reported through cinfo alone
static int32_t bcon_ready(gmrfx_handle *h) {
    if (int32_t e = need_batch(h, true)) return e;
    if (h->bcon.m > 0 && !h->D->bcon_prepare()) {
        const std::vector<long long> &ci = h->D->bcon_cinfo();
        int64_t k = 0;
        while (k < h->nbatch && ci[(size_t)k] <= 0) k++;
        h->err = "batch constraints: A Q^-1 A' of member " + std::to_string(k) + " is not positive definite (rank-deficient constraint matrix)";
        return GMRFX_ERR_NOT_POSDEF;
    }
    return GMRFX_OK;
}

extern "C" int32_t gmrfx_batch_constraints_info(gmrfx_handle *h, int64_t *m, double *logdet_W, double *logdet_AAt, int64_t *cinfo, double *ms) {
    return guarded(h, [&]() -> int32_t {
        const int64_t nb = h->nbatch;
        if (m) *m = h->bcon.m;
        if (logdet_AAt) *logdet_AAt = h->bcon.m > 0 ? h->bcon.logdet_AAt : 0.0;
        if (logdet_W) std::fill(logdet_W, logdet_W + nb, 0.0);
        if (cinfo) std::fill(cinfo, cinfo + nb, (int64_t)0);
        if (ms) *ms = 0.0;
        if (h->bcon.m == 0 || (!logdet_W && !cinfo && !ms)) return GMRFX_OK;
        const int32_t rc = bcon_ready(h);
        if (rc != GMRFX_OK && rc != GMRFX_ERR_NOT_POSDEF) return rc;
        if (logdet_W) std::copy(h->D->bcon_logdet_w().begin(), h->D->bcon_logdet_w().end(), logdet_W);
        if (cinfo) std::copy(h->D->bcon_cinfo().begin(), h->D->bcon_cinfo().end(), cinfo);
        if (ms) *ms = h->D->bcon_ms();
        return rc;
    });
}

extern "C" int32_t gmrfx_batch_constraints_get(gmrfx_handle *h, int64_t member, double *A_tilde_T, int64_t ld, double *W) {
    return guarded(h, [&]() -> int32_t {
        if (member < 0 || member >= h->nbatch) throw std::invalid_argument("batch constraints: member out of range");
        if (A_tilde_T && ld < h->n_member) throw std::invalid_argument("batch constraints: ld < n");
        if (int32_t e = bcon_ready(h)) return e;
        h->D->bcon_get((int)member, A_tilde_T, ld, W);
        return GMRFX_OK;
    });
}

// log_correction[k] from the members' log det W_k and r_k' W_k^-1 r_k (both formed on the device)
static void batch_log_correction(const gmrfx_handle *h, const std::vector<double> &quad, double *out) {
    const int m = h->bcon.m;
    const std::vector<double> &ldw = h->D->bcon_logdet_w();
    for (int64_t k = 0; k < h->nbatch; k++)
        out[k] = m > 0 ? 0.5 * (m * std::log(2.0 * 3.14159265358979323846) + ldw[(size_t)k] + quad[(size_t)k]) - 0.5 * h->bcon.logdet_AAt : 0.0;
}

extern "C" int32_t gmrfx_batch_constraints_mean(gmrfx_handle *h, const double *mu, double *mean_c, double *log_correction) {
    return guarded(h, [&]() -> int32_t {
        if (int32_t e = bcon_ready(h)) return e;
        const int64_t n = h->n_member, nb = h->nbatch;
        DevBlock x;
        if (mu) stage_up(h, x, mu, n * nb);
        else stage_zeros(h, x, n * nb);
        if (log_correction) {
            std::vector<double> quad((size_t)nb, 0.0);
            h->D->bcon_quad(x, quad.data());
            batch_log_correction(h, quad, log_correction);
        }
        if (mean_c) {
            h->D->bcon_correct(x, n, n, 1, nullptr);
            stage_down(h, x, mean_c, n, n, nb);
        }
        return GMRFX_OK;
    });
}

static int32_t batch_constraints_correct_impl(gmrfx_handle *h, double *X, int64_t ldx, int64_t sx, int64_t nvec, bool dev) {
    return guarded(h, [&]() -> int32_t {
        check_member_block(h, X, ldx, sx, nvec, "X");
        if (int32_t e = bcon_ready(h)) return e;
        if (nvec == 0 || h->bcon.m == 0) return GMRFX_OK;
        if (dev) { h->D->bcon_correct(X, ldx, sx, nvec, nullptr); return GMRFX_OK; }
        const int64_t n = h->n_member;
        DevBlock x;
        stage_up(h, x, X, ldx, n, nvec, sx, h->nbatch);
        h->D->bcon_correct(x, n, n * nvec, nvec, nullptr);
        stage_down(h, x, X, ldx, n, nvec, sx, h->nbatch);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_batch_constraints_correct(gmrfx_handle *h, double *X, int64_t ldx, int64_t sx, int64_t nvec) {
    return batch_constraints_correct_impl(h, X, ldx, sx, nvec, false);
}
extern "C" int32_t gmrfx_batch_constraints_correct_dev(gmrfx_handle *h, double *d_X, int64_t ldx, int64_t sx, int64_t nvec) {
    return batch_constraints_correct_impl(h, d_X, ldx, sx, nvec, true);
}

extern "C" int32_t gmrfx_batch_constraints_var(gmrfx_handle *h, double *out) {
    return guarded(h, [&]() -> int32_t {
        if (!out) throw std::invalid_argument("out is null");
        if (int32_t e = bcon_ready(h)) return e;
        h->D->bcon_var(out);
        return GMRFX_OK;
    });
}

static int32_t batch_sample_impl(gmrfx_handle *h, const double *Z, int64_t ldz, int64_t sz, int64_t nrhs, const double *mu, double *X, int64_t ldx,
                                 int64_t sx, bool dev) {
    if (h && h->bcon.m == 0 && !mu)
        return dev ? gmrfx_batch_backward_solve_dev(h, Z, ldz, sz, nrhs, X, ldx, sx) : gmrfx_batch_backward_solve(h, Z, ldz, sz, nrhs, X, ldx, sx);
    return guarded(h, [&]() -> int32_t {
        check_member_block(h, Z, ldz, sz, nrhs, "Z");
        check_member_block(h, X, ldx, sx, nrhs, "X");
        if (int32_t e = bcon_ready(h)) return e;
        if (nrhs == 0) return GMRFX_OK;
        const int64_t n = h->n_member;
        if (dev) {
            const Device::MemberLayout ml{n, sz, sx};
            h->D->solve(Z, ldz, nrhs, X, ldx, true, 1, &ml);
            h->D->bcon_correct(X, ldx, sx, nrhs, mu);
            return GMRFX_OK;
        }
        DevBlock x, dm;
        stage_up(h, x, Z, ldz, n, nrhs, sz, h->nbatch);
        if (mu) stage_up(h, dm, mu, n * h->nbatch);
        const Device::MemberLayout ml{n, n * nrhs, n * nrhs};
        h->D->solve(x, n, nrhs, x, n, true, 1, &ml);
        h->D->bcon_correct(x, n, n * nrhs, nrhs, dm);
        stage_down(h, x, X, ldx, n, nrhs, sx, h->nbatch);
        return GMRFX_OK;
    });
}
extern "C" int32_t gmrfx_batch_sample(gmrfx_handle *h, const double *Z, int64_t ldz, int64_t sz, int64_t nrhs, const double *mu, double *X,
                                      int64_t ldx, int64_t sx) {
    return batch_sample_impl(h, Z, ldz, sz, nrhs, mu, X, ldx, sx, false);
}
extern "C" int32_t gmrfx_batch_sample_dev(gmrfx_handle *h, const double *d_Z, int64_t ldz, int64_t sz, int64_t nrhs, const double *d_mu, double *d_X,
                                          int64_t ldx, int64_t sx) {
    return batch_sample_impl(h, d_Z, ldz, sz, nrhs, d_mu, d_X, ldx, sx, true);
}

extern "C" int32_t gmrfx_batch_constrained_logpdf_dev(gmrfx_handle *h, const double *d_nzval, const double *d_X, int64_t ldx, int64_t sx,
                                                      int64_t nvec, const double *d_mu, double *quad, double *logdet, double *log_correction,
                                                      int64_t *info, int64_t *cinfo) {
    return guarded(h, [&]() -> int32_t {
        if (!d_nzval) throw std::invalid_argument("nzval is null");
        check_batch_quadform(h, d_X, ldx, sx, nvec, quad);
        if (int32_t e = need_batch(h, false)) return e;
        const int64_t nb = h->nbatch;
        std::vector<int64_t> inf((size_t)nb);
        h->D->batch_refactorize_logpdf(d_nzval, d_X, ldx, sx, nvec, d_mu, quad, logdet, (long long *)inf.data());
        if (info) std::copy(inf.begin(), inf.end(), info);
        if (cinfo) std::fill(cinfo, cinfo + nb, (int64_t)0);
        if (log_correction) std::fill(log_correction, log_correction + nb, 0.0);
        int32_t rc = GMRFX_OK;
        if (h->bcon.m > 0) {
            rc = bcon_ready(h);
            if (rc != GMRFX_OK && rc != GMRFX_ERR_NOT_POSDEF) return rc;
            if (cinfo) std::copy(h->D->bcon_cinfo().begin(), h->D->bcon_cinfo().end(), cinfo);
            if (log_correction) {
                std::vector<double> q((size_t)nb, 0.0);
                h->D->bcon_quad(d_mu, q.data());
                batch_log_correction(h, q, log_correction);
            }
        }
        if (int32_t e = batch_status(h, inf)) return e;
        return rc;
    });
}
