// api_common.h -- what the files of the extern "C" boundary (api_*.cpp, one per subject of include/gmrfx.h) share: the handle, the
// guards that turn exceptions into return codes, one vocabulary of argument checks, and the stagers that carry host operands through
// plain device buffers. Nothing outside the stagers talks to the HIP runtime.
#pragma once
#include "../../include/gmrfx.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "device.h"
#include "symbolic.h"

using namespace gmrfx;       // (this header is for the api_*.cpp files only)

struct gmrfx_handle {
    Symbolic S;
    std::unique_ptr<Device> D;   // null for symbolic_only handles
    gmrfx_opts opts{};
    std::string err;
    // lazily built pattern of the de-permuted selected inverse
    bool zpat_built = false;
    std::vector<i64> zcolptr, zrow, zoff;
    // batched handles (gmrfx_create_batched): S is the forest of nbatch copies of the member's pattern; plain handles: 1, n, nnz
    int64_t nbatch = 1, n_member = 0, nnz_member = 0;
    // linear equality constraints A x = e (gmrfx_constraints_set): host copy, also on symbolic_only handles; con.m = 0: none
    ConHost con;
    // the same for every member of a batch (gmrfx_batch_constraints_set): one A (n_member columns) and e; at most one of the two is set
    ConHost bcon;
    // the observation likelihood of Fisher scoring (gmrfx_obs_set): host copy, also on symbolic_only handles; obs.nobs = 0: none
    ObsHost obs;
    // the likelihood of the batch calls (gmrfx_batch_obs_set): one data set, one parameter per member; bobs.nobs = 0: none
    BObsHost bobs;
    // host analysis of the RBMC variance estimators (gmrfx_rbmc_plan / gmrfx_rbmc_var), built lazily: the symmetric row structure
    // once, the block plan of the most recent enclosure_size
    RbmcSym rsym;
    RbmcPlan rplan;
};

extern thread_local std::string g_create_err;       // (api_core.cpp) create-time failures have no handle to carry the message
// gmrfx_opts -> the analysis options (api_core.cpp, beside gmrfx_create; gmrfx_create_batched reads them the same way)
void sym_options(const gmrfx_opts &o, SymOptions &so);

// ---- guards ----------------------------------------------------------------------------------------------------------------------
template <class F> int32_t guarded(gmrfx_handle *h, F &&f) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    try {
        return f();
    } catch (const std::invalid_argument &e) {
        h->err = e.what();
        return GMRFX_ERR_INVALID_ARG;
    } catch (const std::bad_alloc &) {
        h->err = "out of host memory";
        return GMRFX_ERR_ALLOC;
    } catch (const std::exception &e) {
        h->err = e.what();
        return GMRFX_ERR_HIP;
    }
}

inline int32_t device_failure(const std::exception &e) {
    g_create_err = e.what();
    return std::string(e.what()).find("no HIP device") != std::string::npos ? GMRFX_ERR_NO_DEVICE : GMRFX_ERR_HIP;
}
// analysis = true: anything but a refused argument / a failed host allocation is a refused argument too (the analysis never touches
// the device); false: it is a device failure
template <class F> int32_t create_guarded(bool analysis, F &&f) {
    try {
        return f();
    } catch (const std::invalid_argument &e) {
        g_create_err = e.what();
        return GMRFX_ERR_INVALID_ARG;
    } catch (const std::bad_alloc &) {
        g_create_err = "out of host memory";
        return GMRFX_ERR_ALLOC;
    } catch (const std::exception &e) {
        if (!analysis) return device_failure(e);
        g_create_err = e.what();
        return GMRFX_ERR_INVALID_ARG;
    }
}
// the caller's options over the defaults (struct_size bytes of them); false: refused
inline bool read_opts(const gmrfx_opts *opts, gmrfx_opts &o) {
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (int32_t)sizeof(gmrfx_opts);
    o.device = -1;
    if (!opts) return true;
    if (opts->struct_size <= 0) { g_create_err = "opts.struct_size not set"; return false; }
    std::memcpy(&o, opts, std::min<size_t>((size_t)opts->struct_size, sizeof(gmrfx_opts)));
    return true;
}
// the device state of an analysed handle (none for symbolic_only); every failure in here is a device failure
inline int32_t attach_device(gmrfx_handle *h, bool batched) {
    if (h->opts.symbolic_only) return GMRFX_OK;
    try {
        h->D.reset(new Device());
        h->D->init(h->S, h->opts.device);
        if (batched) h->D->set_batch((int)h->nbatch, h->n_member, h->nnz_member);
    } catch (const std::exception &e) {
        return device_failure(e);
    }
    return GMRFX_OK;
}

// ---- argument checks: each throws std::invalid_argument, which `guarded` turns into GMRFX_ERR_INVALID_ARG + the message --------------
inline void check_index_base(int32_t base, const char *prefix = "") {
    if (base != 0 && base != 1) throw std::invalid_argument(std::string(prefix) + "index_base must be 0 or 1");
}
inline void check_unsharded(const gmrfx_handle *h, const char *message) {
    if (h->S.shard_plan) throw std::invalid_argument(message);
}
// A block of cnt vectors at p with leading dimension ld; with a member stride (s non-null: the batch calls) member k's block sits at
// p + k s, its rows are the member's, and the blocks of two members must not overlap (s >= ld cnt). Refused, in this order: cnt < 0
// ("<count> < 0"), then for cnt > 0 a null p ("<null_what> is null"; callers with two pointers under one message pass null when
// either is), ld < n, a stride under ld cnt (the last two prefixed "<what>: " on member-strided blocks).
inline void check_block(const gmrfx_handle *h, const void *p, int64_t ld, int64_t cnt, const char *count, const char *null_what,
                        const int64_t *s = nullptr, const char *what = "") {
    if (cnt < 0) throw std::invalid_argument(std::string(count) + " < 0");
    if (cnt == 0) return;
    if (!p) throw std::invalid_argument(std::string(null_what) + " is null");
    const std::string pre = s ? std::string(what) + ": " : "";
    if (ld < (s ? h->n_member : h->S.n)) throw std::invalid_argument(pre + "leading dimension smaller than n");
    if (s && h->nbatch > 1 && (*s < 0 || *s / ld < cnt)) throw std::invalid_argument(pre + "member stride smaller than ld * columns");
}
// right-hand sides in, solutions out: column-major n x nrhs each (names: "B/X", "Z/X" -- how the message calls them)
inline void check_rhs(const gmrfx_handle *h, const void *B, int64_t ldb, const void *X, int64_t ldx, int64_t nrhs, const char *names) {
    check_block(h, B && X ? B : nullptr, ldb, nrhs, "nrhs", names);
    check_block(h, X, ldx, nrhs, "nrhs", names);
}
inline void check_member_block(const gmrfx_handle *h, const void *X, int64_t ldx, int64_t sx, int64_t nvec, const char *what) {
    check_block(h, X, ldx, nvec, "nvec", what, &sx, what);
}
inline void check_batch_quadform(const gmrfx_handle *h, const double *X, int64_t ldx, int64_t sx, int64_t nvec, const double *quad) {
    check_block(h, X && quad ? X : nullptr, ldx, nvec, "nvec", "X / quad", &sx, "X");
    if (nvec > INT32_MAX / h->nbatch) throw std::invalid_argument("nvec * nbatch exceeds INT32_MAX");
}
// A caller-supplied compressed pattern (ptr has ncol + 1 entries): ptr[0] == base, monotone. Everything that
// sizes a buffer from ptr[ncol] and then walks ptr[j] .. ptr[j + 1] checks this first (INVALID_ARG, not a heap overrun).
inline void check_compressed_ptr(const int64_t *ptr, int64_t ncol, int32_t base, const char *what) {
    if (ptr[0] != base) throw std::invalid_argument(std::string(what) + "[0] != index_base");
    for (int64_t j = 0; j < ncol; j++)
        if (ptr[j + 1] < ptr[j]) throw std::invalid_argument(std::string(what) + " not monotone");
}

// ---- the handle's state ------------------------------------------------------------------------------------------------------------
inline int32_t need_device(gmrfx_handle *h, bool need_factor) {
    if (!h->D) { h->err = "handle has no device state (symbolic_only or no HIP device): numeric entry points are GPU-only"; return GMRFX_ERR_NO_DEVICE; }
    if (need_factor && !h->D->factorized) { h->err = "gmrfx_refactorize has not been called"; return GMRFX_ERR_NOT_FACTORIZED; }
    return GMRFX_OK;
}
// batch entry points on a plain handle: a batch of one (the device-side buffers are set up on first use)
inline int32_t need_batch(gmrfx_handle *h, bool need_factor) {
    if (int32_t e = need_device(h, need_factor)) return e;
    if (!h->D->batched()) {
        check_unsharded(h, "sharded handle: the batch entry points need an unsharded handle");
        h->D->set_batch(1, h->S.n, h->S.nnz_in);
    }
    return GMRFX_OK;
}
// the pivot report of the factorisation just done: *info = 0, or 1 + the failing elimination step; an error when the handle checks
inline int32_t pivot_status(gmrfx_handle *h, int64_t *info) {
    const long long fc = h->D->fail_col();
    if (info) *info = fc < 0 ? 0 : fc + 1;
    if (fc >= 0 && h->opts.check_posdef) {
        h->err = "matrix is not positive definite (non-positive pivot at elimination step " + std::to_string(fc + 1) + ")";
        return GMRFX_ERR_NOT_POSDEF;
    }
    return GMRFX_OK;
}
inline int32_t batch_status(gmrfx_handle *h, const std::vector<int64_t> &info) {
    for (int64_t k = 0; k < h->nbatch; k++)
        if (info[k] != 0 && h->opts.check_posdef) {
            h->err = "member " + std::to_string(k) + " is not positive definite (non-positive pivot at elimination step " + std::to_string(info[k]) + ")";
            return GMRFX_ERR_NOT_POSDEF;
        }
    return GMRFX_OK;
}

// ---- stagers: host operands of an entry point as plain device buffers, freed when it returns. Each selects the handle's device
// itself; the copies are synchronous. -------------------------------------------------------------------------------------------------
using DevBlock = DevBuf<double>;
inline void stage_alloc(const gmrfx_handle *h, DevBlock &b, int64_t count) {
    hip_check(hipSetDevice(h->D->device), "hipSetDevice");
    b.alloc((size_t)count);
}
// count doubles
inline void stage_up(const gmrfx_handle *h, DevBlock &b, const double *src, int64_t count) {
    stage_alloc(h, b, count);
    hip_check(hipMemcpy(b, src, (size_t)count * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
}
// count zeros: the fill is enqueued on the handle's main stream, so it is ordered before the kernels that read it
inline void stage_zeros(const gmrfx_handle *h, DevBlock &b, int64_t count) {
    stage_alloc(h, b, count);
    hip_check(hipMemsetAsync(b, 0, (size_t)count * sizeof(double), h->D->stream), "hipMemsetAsync");
}
// nblk blocks of cnt vectors of n rows: block k at host + k s with leading dimension ld <-> packed on the device (ld = n, block
// stride n cnt). One block: a plain n x cnt array; the members of a batch: s = their stride, n = n_member, nblk = nbatch.
inline void stage_up(const gmrfx_handle *h, DevBlock &b, const double *src, int64_t ld, int64_t n, int64_t cnt, int64_t s = 0, int64_t nblk = 1) {
    stage_alloc(h, b, n * cnt * nblk);
    for (int64_t k = 0; k < nblk; k++)
        hip_check(hipMemcpy2D(b.get() + k * n * cnt, (size_t)n * sizeof(double), src + k * s, (size_t)ld * sizeof(double), (size_t)n * sizeof(double),
                              (size_t)cnt, hipMemcpyHostToDevice), "hipMemcpy2D");
}
inline void stage_down(const gmrfx_handle *h, const DevBlock &b, double *dst, int64_t ld, int64_t n, int64_t cnt, int64_t s = 0, int64_t nblk = 1) {
    hip_check(hipSetDevice(h->D->device), "hipSetDevice");
    for (int64_t k = 0; k < nblk; k++)
        hip_check(hipMemcpy2D(dst + k * s, (size_t)ld * sizeof(double), b.get() + k * n * cnt, (size_t)n * sizeof(double), (size_t)n * sizeof(double),
                              (size_t)cnt, hipMemcpyDeviceToHost), "hipMemcpy2D");
}
