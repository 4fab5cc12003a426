// lbfgs_search_host.cpp — the host instantiation of lbfgs_search.h and its C entry, for the C
// driver's host loop (lbfgs_driver.c) and the sanitizer job's test double of the device layer
// (tests/sanitize/host_device_double.c). Built with -ffp-contract=off, like the driver.
#include "lbfgs_search.h"

namespace {
template <int LS>
int run(lbk_search* s, lbk_trial_fn trial, void* ctx) {
    int err = 0;
    // (after an error nothing more is evaluated: the Wolfe loop does not test its second call)
    search_loop<LS>(*s, [&](double alpha, bool need_g, double& f, double& dphi) -> bool {
        const int r = err ? err : trial(ctx, alpha, need_g, &f, &dphi);
        if (r < 0) {
            err = r;
            f = dphi = 0.0;
        }
        return r > 0;
    });
    return err;
}
}  // namespace

extern "C" {
int lbk_search_run(int ls, lbk_search* s, lbk_trial_fn trial, void* ctx) {
    switch (ls) {
        case 0: return run<0>(s, trial, ctx);
        case 1: return run<1>(s, trial, ctx);
        case 2: return run<2>(s, trial, ctx);
        default: return run<3>(s, trial, ctx);
    }
}
int lbk_search_lookup(const lbk_search* s, double alpha, int need_g, double* f, double* dphi) {
    return search_cached(*s, alpha, need_g != 0, *f, *dphi);
}
void lbk_search_chain(int ls, const lbk_search* s, double alpha, double* a) {
    double(&c)[LBK_TRIALS_NC] = *reinterpret_cast<double(*)[LBK_TRIALS_NC]>(a);
    if (ls == 0)
        search_chain<0>(*s, alpha, c);
    else
        search_chain<1>(*s, alpha, c);
}
void lbk_search_note_f(lbk_search* s, const double* a, const double* t) {
    search_note_f(*s, *reinterpret_cast<const double(*)[LBK_TRIALS_NC]>(a),
                  *reinterpret_cast<const double(*)[LBK_TRIALS_NC]>(t));
}
void lbk_search_note_fg(lbk_search* s, double alpha, const double* t) {
    search_note_fg(*s, alpha, *reinterpret_cast<const double(*)[2]>(t));
}
double lbk_search_cubic(double a0, double a1, double p0, double dp0, double p1, double dp1) {
    return wolfe_cubic(a0, a1, p0, dp0, p1, dp1);
}
double lbk_search_quad(double a0, double p0, double dp0, double p1) { return search_quad(a0, p0, dp0, p1); }
}
