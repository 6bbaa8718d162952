// api_composite.cpp -- the C ABI of include/gmrfx.h: a composite likelihood on a plain handle, several observation families through one
// stacked design matrix (the reference's CompositeObservationModel / CompositeLikelihood, src/observation_models/composite/: loglik,
// loggrad and loghessian are sums over the components, pointwise_loglik their concatenation). The state is the design form's
// (api_fisher.cpp: the same plan, the same map) with a component per row; the evaluation, the loop and the predictive calls find it
// on the handle (Device::obs_set; k_design_eta_comp, k_pred_design_comp, k_pred_scores_comp).
#include <cmath>

#include "api_obs.h"

static std::string comp_name(int64_t c) { return "component " + std::to_string(c); }

// the components' constants over their own rows (C.loglik_const) and their sum, in component order, in long double
static double composite_constants(ObsComponents &C, const std::vector<double> &y, const std::vector<double> &aux) {
    C.loglik_const.resize(C.size());
    long double total = 0.0L;
    for (size_t c = 0; c < C.size(); c++) {
        const long long r0 = C.rowptr[c], r1 = C.rowptr[c + 1];
        const long double cc = obs_loglik_const_ld(C.family[c], r1 - r0, y.data() + r0, aux.empty() ? nullptr : aux.data() + r0, C.param[c]);
        C.loglik_const[c] = (double)cc;
        total += cc;
    }
    return (double)total;
}

extern "C" int32_t gmrfx_obs_set_composite(gmrfx_handle *h, int32_t ncomp, const int32_t *family, const double *param, const int64_t *rowptr,
                                           int64_t nobs, const int64_t *colptr, const int64_t *rowval, const double *nzval, int32_t index_base,
                                           const double *offset, const double *y, const double *aux) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "obs_set_composite: ";
        obs_check_handle(h, who);
        const int64_t n = h->S.n;
        if (ncomp < 1 || ncomp > kObsMaxComponents) throw std::invalid_argument(who + "ncomp outside [1, " + std::to_string(kObsMaxComponents) + "]");
        if (!family || !param || !rowptr) throw std::invalid_argument(who + "family / param / rowptr is null");
        if (nobs <= 0) throw std::invalid_argument(who + "nobs must be positive (gmrfx_obs_set with nobs = 0 removes the likelihood)");
        if (rowptr[0] != 0) throw std::invalid_argument(who + "rowptr does not start at 0");
        for (int32_t c = 0; c < ncomp; c++)
            if (rowptr[c + 1] <= rowptr[c]) throw std::invalid_argument(who + "rowptr is not strictly increasing (" + comp_name(c) + " is empty)");
        if (rowptr[ncomp] != nobs) throw std::invalid_argument(who + "rowptr does not end at nobs");
        for (int32_t c = 0; c < ncomp; c++) obs_check_family(who + comp_name(c) + ": ", family[c]);
        check_index_base(index_base, who.c_str());
        if (!colptr) throw std::invalid_argument(who + "colptr is null");
        check_compressed_ptr(colptr, n, index_base, "obs_set_composite: colptr");
        design_check_sizes(n, nobs, colptr[n] - index_base, who);        // (before y, aux or A are read at those lengths)
        if (colptr[n] > index_base && (!rowval || !nzval)) throw std::invalid_argument(who + "rowval / nzval is null");
        bool any_aux = false;
        for (int32_t c = 0; c < ncomp; c++) {
            obs_check_operands(who + comp_name(c) + ": ", family[c], y, aux, param[c]);
            any_aux = any_aux || obs_family_reads_aux(family[c]);
        }
        ObsHost o;
        o.family = kObsComposite; o.nobs = nobs;
        o.y.assign(y, y + nobs);
        // aux is read on the rows of the components that have one; the others' rows hold 0 whatever the caller's array does
        if (aux && any_aux) o.aux.assign((size_t)nobs, 0.0);
        o.comp.family.assign(family, family + ncomp);
        o.comp.param.assign(param, param + ncomp);
        o.comp.rowptr.assign(rowptr, rowptr + ncomp + 1);
        for (int32_t c = 0; c < ncomp; c++) {
            const bool reads = !o.aux.empty() && obs_family_reads_aux(family[c]);
            for (int64_t k = rowptr[c]; k < rowptr[c + 1]; k++) {
                if (reads) o.aux[(size_t)k] = aux[k];
                if (offset && !std::isfinite(offset[k]))       // (ahead of the plan's own check, which cannot name the component)
                    throw std::invalid_argument(who + comp_name(c) + ": offset is not finite (observation " + std::to_string(k) + ")");
                obs_check_value(who + comp_name(c) + ": ", family[c], o.y[(size_t)k], reads ? &o.aux[(size_t)k] : nullptr,
                                " (observation " + std::to_string(k) + ")");
            }
        }
        o.loglik_const = composite_constants(o.comp, o.y, o.aux);
        if (!h->rsym.built) rbmc_build_sym(h->S, h->rsym);
        auto plan = std::make_shared<DesignPlan>();
        design_build_plan(h->rsym, n, h->S.nnz_in, nobs, colptr, rowval, nzval, index_base, offset, *plan, who);
        o.design = std::move(plan);
        if (h->D) h->D->obs_set(o);
        h->obs = std::move(o);
        return GMRFX_OK;
    });
}

extern "C" int32_t gmrfx_obs_composite_info(const gmrfx_handle *h, int32_t *ncomp, int32_t *family, double *param, int64_t *rowptr,
                                            double *loglik_const) {
    if (!h) return GMRFX_ERR_INVALID_ARG;
    const ObsComponents &C = h->obs.comp;
    if (ncomp) *ncomp = (int32_t)C.size();
    if (family) std::copy(C.family.begin(), C.family.end(), family);
    if (param) std::copy(C.param.begin(), C.param.end(), param);
    if (rowptr) std::copy(C.rowptr.begin(), C.rowptr.end(), rowptr);
    if (loglik_const) std::copy(C.loglik_const.begin(), C.loglik_const.end(), loglik_const);
    return GMRFX_OK;
}

// The components' parameters replaced in place: the positivity checks of gmrfx_obs_set_composite, the constants again; the plan, the
// map and the device tables stay (y and aux were validated when they were set).
extern "C" int32_t gmrfx_obs_composite_set_param(gmrfx_handle *h, const double *param) {
    return guarded(h, [&]() -> int32_t {
        const std::string who = "obs_composite_set_param: ";
        obs_check_handle(h, who);
        if (h->obs.comp.empty()) throw std::invalid_argument(who + "no composite likelihood is set (gmrfx_obs_set_composite)");
        if (!param) throw std::invalid_argument(who + "param is null");
        const size_t nc = h->obs.comp.size();
        for (size_t c = 0; c < nc; c++) obs_check_param(who + comp_name((int64_t)c) + ": ", h->obs.comp.family[c], param[c]);
        // aside: the device call may refuse, and then nothing has changed
        ObsComponents C = h->obs.comp;
        C.param.assign(param, param + nc);
        const double total = composite_constants(C, h->obs.y, h->obs.aux);
        if (h->D) h->D->obs_composite_set_param(C, total);
        h->obs.comp = std::move(C);
        h->obs.loglik_const = total;
        return GMRFX_OK;
    });
}
