/* lbfgs_search.h — the four line searches of the sequential reference (line_search.cpp:19-30
 * backtracking, 57-121 interpolation, 125-189 Wolfe, 33-55 backtracking-Wolfe), stated ONCE: the two
 * interpolants, the values a search already holds (lbk_search's caches), the bookkeeping of a trial
 * pass, and the four loops over a caller-supplied trial(alpha, need_g, f, dphi). The loops are
 * resumable: their variables live in lbk_search (lbfgs_device.h) at the top of an iteration.
 *
 * Instantiated three times from this one text:
 *   - on the device by k_coop_search (lbfgs_kernels_impl.h) and the two batched solvers
 *     (lbfgs_kernels_batch_solve.h, lbfgs_kernels_batch_solve_dense.h), trial = a grid-wide pass;
 *   - on the host by lbfgs_search_host.cpp, which exports the C entry below; the driver's host loop
 *     (lbfgs_driver.c run_search) and the sanitizer job's test double of the device layer
 *     (tests/sanitize/host_device_double.c) run it over their own trial functions.
 * Both sides compile with -ffp-contract=off, IEEE division and square root: the same decisions and
 * the same step bit for bit. */
#ifndef LBFGS_SEARCH_H
#define LBFGS_SEARCH_H

#include "lbfgs_device.h"

/* ---- the C entry (lbfgs_search_host.cpp); ls in LBFGS_LS_* numbering ---- */
#ifdef __cplusplus
extern "C" {
#endif
/* 1: a value in *f (and *dphi with need_g); 0: no value, the loop stops at the top of this iteration
 * with its variables in s; < 0: an error, which lbk_search_run returns */
typedef int (*lbk_trial_fn)(void* ctx, double alpha, int need_g, double* f, double* dphi);
/* runs (or resumes) the search from s until it is done (s->done, s->step) or the trial stops it */
int lbk_search_run(int ls, lbk_search* s, lbk_trial_fn trial, void* ctx);
/* the values s holds: the commit's first trial, backtracking's candidate step, the last trial pass */
int lbk_search_lookup(const lbk_search* s, double alpha, int need_g, double* f, double* dphi);
void lbk_search_chain(int ls, const lbk_search* s, double alpha, double* a /* [LBK_TRIALS_NC] */);
void lbk_search_note_f(lbk_search* s, const double* a, const double* t /* both [LBK_TRIALS_NC] */);
void lbk_search_note_fg(lbk_search* s, double alpha, const double* t /* [2]: f, g.d */);
double lbk_search_cubic(double a0, double a1, double p0, double dp0, double p1, double dp1);
double lbk_search_quad(double a0, double p0, double dp0, double p1);
#ifdef __cplusplus
}
#endif

#ifdef __cplusplus
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LBK_SEARCH_FN __host__ __device__ __forceinline__
#else
#include <math.h>
#define LBK_SEARCH_FN static inline
#endif

LBK_SEARCH_FN double wolfe_cubic(double a0, double a1, double p0, double dp0, double p1, double dp1) {
    const double d1 = dp0 + dp1 - 3 * (p1 - p0) / (a1 - a0);  // line_search.cpp:8-12
    const double d2 = copysign(sqrt(d1 * d1 - dp0 * dp1), a1 - a0);
    return a0 + (a1 - a0) * (dp0 + d2 - d1) / (dp0 - dp1 + 2 * d2);
}
LBK_SEARCH_FN double search_quad(double a0, double p0, double dp0, double p1) {  // :14-16
    return a0 - 0.5 * dp0 * a0 * a0 / (p1 - p0 - dp0 * a0);
}

// the values the search holds (the commit's first trial, the backtracking commit's f at the next
// step, the last trial pass): no pass for these
LBK_SEARCH_FN bool search_cached(const lbk_search& s, double alpha, bool need_g, double& f, double& dphi) {
    if (s.have_spec && alpha == s.spec_a) {
        f = s.spec_f;
        dphi = s.spec_dphi;
        return true;
    }
    if (!need_g && s.have_cand && alpha == s.cand_a) {
        f = s.cand_f;
        return true;
    }
    // (unrolled over the cache's capacity: a runtime-indexed tc_a[] would put the whole state in scratch)
#pragma unroll
    for (int j = 0; j < LBK_TRIALS_NC; ++j)
        if (j < s.tc_n && alpha == s.tc_a[j] && (!need_g || (j == 0 && s.tc_dphi_ok))) {
            f = s.tc_f[j];
            dphi = s.tc_dphi;
            return true;
        }
    return false;
}
// the steps of an f-only trial pass from alpha: the search's halving chain
template <int LS>
LBK_SEARCH_FN void search_chain(const lbk_search& s, double alpha, double (&a)[LBK_TRIALS_NC]) {
    const double ratio = LS == 0 ? s.beta : 0.5;
    a[0] = alpha;
#pragma unroll
    for (int j = 1; j < LBK_TRIALS_NC; ++j) a[j] = a[j - 1] * ratio;
}
// a trial pass's totals become the last-trial-pass cache
LBK_SEARCH_FN void search_note_fg(lbk_search& s, double alpha, const double (&t)[2]) {
    s.tc_n = 1;
    s.tc_a[0] = alpha;
    s.tc_f[0] = t[0];
    s.tc_dphi = t[1];
    s.tc_dphi_ok = 1;
    s.passes_fg++;
}
LBK_SEARCH_FN void search_note_f(lbk_search& s, const double (&a)[LBK_TRIALS_NC],
                                 const double (&t)[LBK_TRIALS_NC]) {
    s.tc_n = LBK_TRIALS_NC;
#pragma unroll
    for (int j = 0; j < LBK_TRIALS_NC; ++j) {
        s.tc_a[j] = a[j];
        s.tc_f[j] = t[j];
    }
    s.tc_dphi = 0.0;
    s.tc_dphi_ok = 0;
    s.passes_f++;
}

// the four loops (s.alpha and the search's own variables: at the top of an iteration, in and out)
// over trial(alpha, need_g, f, dphi) -> bool (false: no value, the loop stops at the top of its
// iteration with its variables in s)
template <int LS, class Trial>
LBK_SEARCH_FN void search_loop(lbk_search& s, Trial&& trial) {
    auto finish = [&](double step) {
        s.done = 1;
        s.step = step;
    };
    double alpha = s.alpha;
    if (LS == 0) {  // backtracking
        for (;;) {
            double ft, dd;
            if (!trial(alpha, false, ft, dd)) break;
            if (!(s.f_x - ft < s.c1 * alpha * s.gd)) {
                finish(alpha);
                break;
            }
            alpha *= s.beta;
            if (alpha < s.tol) {
                finish(alpha);
                break;
            }
        }
    } else if (LS == 1) {  // interpolation (iter: the loop counter before its `it++ < 20` test)
        double alpha_prev = s.alpha_prev, f_prev = s.f_prev;
        int it = s.iter;
        for (;;) {
            if (!(it++ < 20)) {
                finish(alpha);
                break;
            }
            double f_new, dd;
            if (!trial(alpha, false, f_new, dd)) {
                --it;
                break;
            }
            if (f_new <= s.f_x + s.c1 * alpha * s.gd) {
                finish(alpha);
                break;
            }
            if (alpha < s.amin) {
                finish(s.amin);
                break;
            }
            if (alpha_prev > 0) {
                const double delta = alpha - alpha_prev;
                if (fabs(delta) < 1e-10) {
                    alpha *= 0.5;
                } else {
                    const double ga = (f_new - s.f_x - s.gd * alpha) / (alpha * alpha);
                    alpha = wolfe_cubic(alpha_prev, alpha, f_prev, s.gd, f_new, ga);
                    if (alpha < 0.1 * alpha_prev || alpha > 0.9 * alpha_prev) alpha = alpha_prev * 0.5;
                }
            } else {
                alpha = search_quad(alpha, f_new, s.gd, s.f_x);
                if (alpha < 0.1 * s.init || alpha > 0.9 * s.init) alpha = s.init * 0.5;
            }
            alpha_prev = alpha;
            f_prev = f_new;
        }
        s.alpha_prev = alpha_prev;
        s.f_prev = f_prev;
        s.iter = it;
    } else if (LS == 2) {  // Wolfe
        double lo = s.alpha_lo, hi = s.alpha_hi, f_lo = s.f_lo, dphi_lo = s.dphi_lo;
        int iter = s.iter;
        for (;;) {
            if (iter >= 20) {
                finish(alpha);
                break;
            }
            double f_new, dphi_new;
            if (!trial(alpha, false, f_new, dphi_new)) break;
            if (f_new > s.f_x + s.c1 * alpha * s.gd || (f_new >= f_lo && iter > 0)) {
                hi = alpha;
                alpha = wolfe_cubic(lo, hi, f_lo, dphi_lo, f_new, (f_new - s.f_x - s.gd * alpha) / (alpha * alpha));
                ++iter;
                continue;
            }
            trial(alpha, true, f_new, dphi_new);  // the same pass's g.d (cached: want_dphi)
            if (fabs(dphi_new) <= -s.c2 * s.gd) {
                finish(alpha);
                break;
            }
            if (dphi_new >= 0) {
                hi = alpha;
                alpha = wolfe_cubic(lo, hi, f_lo, dphi_lo, f_new, dphi_new);
            } else {
                lo = alpha;
                f_lo = f_new;
                dphi_lo = dphi_new;
                if (hi == INFINITY)
                    alpha *= 2;
                else
                    alpha = wolfe_cubic(lo, hi, f_lo, dphi_lo, f_new, dphi_new);
            }
            if (alpha < s.amin) {
                finish(s.amin);
                break;
            }
            ++iter;
        }
        s.alpha_lo = lo;
        s.alpha_hi = hi;
        s.f_lo = f_lo;
        s.dphi_lo = dphi_lo;
        s.iter = iter;
    } else {  // backtracking-Wolfe
        for (;;) {
            double fn, dphi;
            if (!trial(alpha, true, fn, dphi)) break;
            if (fn > s.f_x + s.c1 * alpha * s.gd) {
                alpha *= s.beta;
            } else if (dphi < s.c2 * s.gd) {
                alpha *= 1.1;
            } else {
                finish(alpha);
                break;
            }
            if (alpha < s.tol) {
                finish(alpha);
                break;
            }
        }
    }
    s.alpha = alpha;
}
#endif /* __cplusplus */
#endif
