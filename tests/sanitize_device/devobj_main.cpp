// devobj_main.cpp — sanitizer job for the device-callback objective (LBFGS_OBJ_DEVICE) and the
// device-buffer entry points (lbfgs_minimize_device, lbfgs_solver_init_device, lbfgs_get_x_device);
// tests/sanitize_device/Makefile, run by tests/test_sanitize_device.py.
//
// lbfgs_driver.c built with -fsanitize=address,undefined over the unmodified host test double of
// the device layer (tests/sanitize/host_device_double.c): under it "device" memory is host memory,
// so a callback is plain C++ on the pointers it is given and the caller's "device" buffers are heap
// blocks of exactly n doubles - one element read or written past either end is an ASan report.
// That this program links at all shows the driver kept to the lbk_* functions the double has.
// Every solve must reproduce the oracle's ORC_CANON trajectory bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "lbfgs_hip.h"
#include "lbfgs_oracle.h"

static int g_fail = 0;
#define EXPECT(cond, ...)                                             \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);                        \
            std::fprintf(stderr, "\n");                               \
            ++g_fail;                                                 \
        }                                                             \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (std::isnan(a) && std::isnan(b)); }

struct OracleRun {
    std::vector<double> x, f, gn, al;
    std::vector<uint64_t> c1, c2;
    std::string msg;
    orc_result res;
};

static OracleRun oracle(int obj, int ls, int64_t n, int m, int maxit, const double* x0,
                        double (*hf)(const double*, int64_t, void*) = nullptr,
                        void (*hg)(const double*, int64_t, double*, void*) = nullptr, void* user = nullptr) {
    orc_opts o;
    std::memset(&o, 0, sizeof o);
    o.obj = obj;
    o.ls = ls;
    o.mode = ORC_CANON;
    o.n = n;
    o.m = m;
    o.maxit = maxit;
    o.tol = 1e-5;
    o.c1 = 1e-4;
    o.c2 = 0.9;
    o.initial_step = 1.0;
    o.backtracking_alpha = 0.5;
    o.backtracking_tol = 1e-8;
    o.wolfe_interp_min = 1e-10;
    o.host_f = hf;
    o.host_g = hg;
    o.host_user = user;
    OracleRun r;
    const int cap = maxit + 2;
    r.x.resize(n);
    r.f.resize(cap);
    r.gn.resize(cap);
    r.al.resize(cap);
    r.c1.resize(cap);
    r.c2.resize(cap);
    std::vector<int64_t> nf(cap);
    std::vector<char> msg(1 << 20);
    int64_t fn = 0, gnn = 0;
    orc_lbfgs(&o, x0, r.x.data(), r.f.data(), r.gn.data(), r.al.data(), r.c1.data(), r.c2.data(), nf.data(), cap,
              nullptr, 0, &fn, nullptr, 0, &gnn, msg.data(), (int)msg.size(), &r.res);
    r.msg = msg.data();
    return r;
}

// trace, final x (n doubles at x), messages, status and iteration count against the oracle's run
static void compare(const char* tag, lbfgs_ctx* c, int status, const double* x, int64_t n, const lbfgs_result& res,
                    const OracleRun& o) {
    const int len = lbfgs_trace_len(c);
    EXPECT(len == o.res.ntrace, "%s: trace length %d vs %d", tag, len, o.res.ntrace);
    std::vector<double> f(len + 1), gn(len + 1), al(len + 1);
    std::vector<uint64_t> c1(len + 1), c2(len + 1);
    lbfgs_trace_get(c, f.data(), gn.data(), al.data(), c1.data(), c2.data(), len);
    for (int k = 0; k < len && k < o.res.ntrace; ++k) {
        EXPECT(same_bits(f[k], o.f[k]) && same_bits(gn[k], o.gn[k]), "%s: iteration %d f %.17g/%.17g", tag, k, f[k],
               o.f[k]);
        EXPECT(same_bits(al[k], o.al[k]), "%s: iteration %d alpha %.17g/%.17g", tag, k, al[k], o.al[k]);
        EXPECT(c1[k] == o.c1[k] && c2[k] == o.c2[k], "%s: iteration %d x checksum", tag, k);
    }
    for (int64_t i = 0; i < n; ++i)
        if (!same_bits(x[i], o.x[i])) {
            EXPECT(false, "%s: x[%lld] %.17g vs %.17g", tag, (long long)i, x[i], o.x[i]);
            break;
        }
    std::vector<char> msg(1 << 20);
    lbfgs_messages(c, msg.data(), (int)msg.size());
    EXPECT(o.msg == msg.data(), "%s: messages differ", tag);
    EXPECT(status == o.res.status && res.iterations == o.res.iters, "%s: status %d/%d iterations %d/%d", tag, status,
           o.res.status, res.iterations, o.res.iters);
}

// a caller's "device" buffer: exactly n doubles on the heap
static std::unique_ptr<double[]> exact(int64_t n) { return std::unique_ptr<double[]>(new double[(size_t)n]); }
static std::unique_ptr<double[]> x0_for(int64_t n, uint32_t seed) {
    auto x = exact(n);
    orc_x0_uniform(x.get(), n, seed, -2.0, 2.0);
    return x;
}

struct Counter {
    int obj;
    int64_t calls = 0, nf = 0, ng = 0, both = 0;
    int64_t fail_at = 0;  // > 0: the fail_at-th call returns nonzero
};
static double cb_f(const double* x, int64_t n, void* u) {
    Counter* k = static_cast<Counter*>(u);
    ++k->nf;
    return orc_f(k->obj, x, n, ORC_CANON);
}
static void cb_g(const double* x, int64_t n, double* g, void* u) {
    Counter* k = static_cast<Counter*>(u);
    ++k->ng;
    orc_grad(k->obj, x, n, g);
}
// the device callback: the same f and grad, on the "device" pointers; grad writes exactly [0, n)
static int cb_dev(const double* x, int64_t n, double* f_out, double* g_dev, void* u) {
    Counter* k = static_cast<Counter*>(u);
    ++k->calls;
    if (k->fail_at > 0 && k->calls == k->fail_at) return 7;
    if (!f_out && !g_dev) return 9;
    if (f_out) {
        ++k->nf;
        *f_out = orc_f(k->obj, x, n, ORC_CANON);
    }
    if (g_dev) {
        ++k->ng;
        orc_grad(k->obj, x, n, g_dev);
    }
    if (f_out && g_dev) ++k->both;
    return 0;
}

static const int64_t kSizes[] = {1, 3, 513};
static const unsigned kFlags = LBFGS_FLAG_QUIET | LBFGS_FLAG_TRACE;

// LBFGS_OBJ_DEVICE through lbfgs_minimize_device, the four searches, eager_grad off and on, against
// the oracle and against the host-callback path's call counts
static void device_callback() {
    for (int64_t n : kSizes)
        for (int ls = 0; ls < 4; ++ls) {
            const int m = n < 10 ? 2 : 5, maxit = 40, obj = LBFGS_OBJ_ROSENBROCK;
            const auto x0 = x0_for(n, 42 + (uint32_t)n);
            Counter ko{obj}, kh{obj};
            const OracleRun o = oracle(ORC_OBJ_HOST, ls, n, m, maxit, x0.get(), cb_f, cb_g, &ko);
            lbfgs_ctx* c = nullptr;
            EXPECT(lbfgs_ctx_create(&c, n, m, 0) == 0, "create n=%lld", (long long)n);
            if (!c) continue;
            lbfgs_result rh;
            {  // the host-callback path in its default order: the call counts to match
                lbfgs_host_fn cb{cb_f, cb_g, &kh};
                auto x = exact(n);
                const int st = lbfgs_minimize(c, LBFGS_OBJ_HOST, &cb, ls, nullptr, x0.get(), x.get(), maxit, 1e-5,
                                              kFlags, &rh);
                EXPECT(st >= 0, "host n=%lld ls=%d: %d", (long long)n, ls, st);
            }
            for (int eager = 0; eager < 2; ++eager) {
                char tag[96];
                std::snprintf(tag, sizeof tag, "device n=%lld ls=%d eager=%d", (long long)n, ls, eager);
                Counter kd{obj};
                lbfgs_device_fn fn{cb_dev, &kd, eager ? LBFGS_DEVICE_EAGER_GRAD : 0u};
                EXPECT(lbfgs_set_device_objective(c, &fn) == 0, "%s: set", tag);
                auto x = exact(n);
                lbfgs_result res;
                const int st = lbfgs_minimize_device(c, LBFGS_OBJ_DEVICE, nullptr, ls, nullptr, x0.get(), x.get(),
                                                     maxit, 1e-5, kFlags, &res);
                EXPECT(st >= 0, "%s: %d %s", tag, st, lbfgs_last_error(c));
                if (st < 0) continue;
                compare(tag, c, st, x.get(), n, res, o);
                EXPECT(res.f_calls == kd.nf && res.grad_calls == kd.ng, "%s: counters %lld/%lld f %lld/%lld g", tag,
                       (long long)res.f_calls, (long long)kd.nf, (long long)res.grad_calls, (long long)kd.ng);
                if (eager)
                    EXPECT(kd.both == kd.calls && kd.calls == rh.f_calls, "%s: %lld calls, %lld with both, host f %lld",
                           tag, (long long)kd.calls, (long long)kd.both, (long long)rh.f_calls);
                else
                    EXPECT(res.f_calls == rh.f_calls && res.grad_calls == rh.grad_calls,
                           "%s: calls %lld/%lld f %lld/%lld g", tag, (long long)res.f_calls, (long long)rh.f_calls,
                           (long long)res.grad_calls, (long long)rh.grad_calls);
                // the stepping form, host x0, device x out
                Counter ks{obj};
                lbfgs_device_fn fs{cb_dev, &ks, eager ? LBFGS_DEVICE_EAGER_GRAD : 0u};
                EXPECT(lbfgs_set_device_objective(c, &fs) == 0, "%s: set", tag);
                EXPECT(lbfgs_solver_init(c, LBFGS_OBJ_DEVICE, nullptr, ls, nullptr, x0.get(), 1e-5, kFlags) == 0,
                       "%s: init", tag);
                lbfgs_result rs;
                int ss = LBFGS_STATUS_RUNNING;
                for (int k = 0; k < maxit && ss == LBFGS_STATUS_RUNNING; k += 7) ss = lbfgs_solver_step(c, 7, &rs);
                EXPECT(ss >= 0, "%s: step %d", tag, ss);
                auto xs = exact(n);
                EXPECT(lbfgs_get_x_device(c, xs.get()) == 0, "%s: get_x_device", tag);
                if (ss != LBFGS_STATUS_RUNNING && st != LBFGS_STATUS_MAX_ITER)
                    for (int64_t i = 0; i < n; ++i)
                        if (!same_bits(xs[i], x[i])) {
                            EXPECT(false, "%s: stepped x[%lld]", tag, (long long)i);
                            break;
                        }
            }
            lbfgs_ctx_destroy(c);
        }
}

// a callback that fails at its k-th call: LBFGS_ERR_CALLBACK, and the context solves on afterwards
static void failing_callback() {
    const int64_t n = 513;
    const int m = 5, maxit = 20;
    const auto x0 = x0_for(n, 7);
    lbfgs_ctx* c = nullptr;
    lbfgs_ctx_create(&c, n, m, 0);
    if (!c) {
        EXPECT(false, "create");
        return;
    }
    for (int ls = 0; ls < 4; ++ls)
        for (int eager = 0; eager < 2; ++eager)
            for (int64_t k = 1; k <= 9; ++k) {
                Counter kd{LBFGS_OBJ_ROSENBROCK};
                kd.fail_at = k;
                lbfgs_device_fn fn{cb_dev, &kd, eager ? LBFGS_DEVICE_EAGER_GRAD : 0u};
                lbfgs_set_device_objective(c, &fn);
                auto x = exact(n);
                lbfgs_result res;
                const int st = lbfgs_minimize_device(c, LBFGS_OBJ_DEVICE, nullptr, ls, nullptr, x0.get(), x.get(), maxit,
                                                     1e-5, kFlags, &res);
                EXPECT(st == LBFGS_ERR_CALLBACK, "fail at call %lld (ls %d eager %d): %d", (long long)k, ls, eager, st);
                EXPECT(kd.calls == k, "fail at call %lld: %lld calls made", (long long)k, (long long)kd.calls);
                EXPECT(std::strstr(lbfgs_last_error(c), "callback") != nullptr, "fail at call %lld: message '%s'",
                       (long long)k, lbfgs_last_error(c));
                if (k == 1) EXPECT(lbfgs_solver_step(c, 1, &res) < 0, "a failed init left a solve to step");
            }
    // the same context, a built-in objective
    auto x = exact(n);
    lbfgs_result res;
    const int st = lbfgs_minimize_device(c, LBFGS_OBJ_ROSENBROCK, nullptr, LBFGS_LS_WOLFE, nullptr, x0.get(), x.get(),
                                         maxit, 1e-5, kFlags, &res);
    EXPECT(st >= 0, "built-in after failures: %d", st);
    if (st >= 0)
        compare("built-in after failures", c, st, x.get(), n, res,
                oracle(LBFGS_OBJ_ROSENBROCK, LBFGS_LS_WOLFE, n, m, maxit, x0.get()));
    lbfgs_ctx_destroy(c);
}

// every refusal is LBFGS_ERR_BAD_ARG, before any call of the objective
static void refusals() {
    const int64_t n = 513;
    const auto x0 = x0_for(n, 3);
    auto x = exact(n);
    lbfgs_ctx* c = nullptr;
    lbfgs_ctx_create(&c, n, 5, 0);
    if (!c) {
        EXPECT(false, "create");
        return;
    }
    lbfgs_result res;
    // no objective set
    EXPECT(lbfgs_minimize(c, LBFGS_OBJ_DEVICE, nullptr, 0, nullptr, x0.get(), x.get(), 5, 1e-5, kFlags, &res) ==
               LBFGS_ERR_BAD_ARG, "no objective set: minimize");
    EXPECT(lbfgs_minimize_device(c, LBFGS_OBJ_DEVICE, nullptr, 0, nullptr, x0.get(), x.get(), 5, 1e-5, kFlags, &res) ==
               LBFGS_ERR_BAD_ARG, "no objective set: minimize_device");
    EXPECT(lbfgs_solver_init(c, LBFGS_OBJ_DEVICE, nullptr, 0, nullptr, x0.get(), 1e-5, kFlags) == LBFGS_ERR_BAD_ARG,
           "no objective set: init");
    EXPECT(lbfgs_solver_init_device(c, LBFGS_OBJ_DEVICE, nullptr, 0, nullptr, x0.get(), 1e-5, kFlags) ==
               LBFGS_ERR_BAD_ARG, "no objective set: init_device");
    Counter kd{LBFGS_OBJ_ROSENBROCK};
    lbfgs_device_fn none{nullptr, &kd, 0u}, fn{cb_dev, &kd, 0u};
    EXPECT(lbfgs_set_device_objective(c, &none) == LBFGS_ERR_BAD_ARG, "set: eval == NULL");
    EXPECT(lbfgs_set_device_objective(nullptr, &fn) == LBFGS_ERR_BAD_ARG, "set: ctx == NULL");
    EXPECT(lbfgs_set_device_objective(c, &fn) == 0, "set");
    const unsigned bad[] = {LBFGS_FLAG_UNFUSED, LBFGS_FLAG_VECTOR_FREE, LBFGS_FLAG_REFERENCE_CALLS,
                            LBFGS_FLAG_CUDA_COMPAT, LBFGS_FLAG_CUDA_COMPAT | LBFGS_FLAG_CUDA_VARIANT};
    for (unsigned f : bad) {
        EXPECT(lbfgs_minimize(c, LBFGS_OBJ_DEVICE, nullptr, 0, nullptr, x0.get(), x.get(), 5, 1e-5, kFlags | f, &res) ==
                   LBFGS_ERR_BAD_ARG, "flag %u: minimize", f);
        EXPECT(lbfgs_solver_init_device(c, LBFGS_OBJ_DEVICE, nullptr, 0, nullptr, x0.get(), 1e-5, kFlags | f) ==
                   LBFGS_ERR_BAD_ARG, "flag %u: init_device", f);
    }
    double a = 0.0, f = 0.0, dphi = 0.0;
    auto g = exact(n);
    EXPECT(lbfgs_line_search(c, LBFGS_OBJ_DEVICE, nullptr, 0, nullptr, x0.get(), x0.get(), x0.get(), &a) ==
               LBFGS_ERR_BAD_ARG, "line_search");
    EXPECT(lbfgs_dev_objective(c, LBFGS_OBJ_DEVICE, x0.get(), &f, g.get()) == LBFGS_ERR_BAD_ARG, "dev_objective");
    EXPECT(lbfgs_dev_trial(c, LBFGS_OBJ_DEVICE, x0.get(), x0.get(), 0.5, &f, g.get(), &dphi) == LBFGS_ERR_BAD_ARG,
           "dev_trial");
    EXPECT(lbfgs_minimize(c, LBFGS_OBJ_DEVICE + 1, nullptr, 0, nullptr, x0.get(), x.get(), 5, 1e-5, kFlags, &res) ==
               LBFGS_ERR_BAD_ARG, "objective 6");
    EXPECT(lbfgs_minimize_device(c, LBFGS_OBJ_ROSENBROCK, nullptr, 0, nullptr, nullptr, x.get(), 5, 1e-5, kFlags, &res) ==
               LBFGS_ERR_BAD_ARG, "x0 == NULL");
    EXPECT(lbfgs_get_x_device(c, nullptr) == LBFGS_ERR_BAD_ARG, "get_x_device NULL");
    EXPECT(kd.calls == 0, "a refused call reached the objective (%lld calls)", (long long)kd.calls);
    // set, it solves; cleared, it is refused again
    EXPECT(lbfgs_minimize(c, LBFGS_OBJ_DEVICE, nullptr, 0, nullptr, x0.get(), x.get(), 5, 1e-5, kFlags, &res) >= 0,
           "set: solves");
    EXPECT(lbfgs_set_device_objective(c, nullptr) == 0, "clear");
    EXPECT(lbfgs_minimize(c, LBFGS_OBJ_DEVICE, nullptr, 0, nullptr, x0.get(), x.get(), 5, 1e-5, kFlags, &res) ==
               LBFGS_ERR_BAD_ARG, "cleared: minimize");
    lbfgs_ctx_destroy(c);
}

// the device-buffer forms with every other objective: the host-buffer forms' bits
static void device_buffers() {
    const int objs[] = {LBFGS_OBJ_ROSENBROCK, LBFGS_OBJ_QUAD_TRIDIAG, LBFGS_OBJ_QUAD_SEPARABLE, LBFGS_OBJ_HOST};
    for (int64_t n : kSizes)
        for (int obj : objs)
            for (int ls = 0; ls < 4; ++ls) {
                if (obj == LBFGS_OBJ_QUAD_SEPARABLE && ls == LBFGS_LS_WOLFE) continue;  // diverges to NaN
                const int m = n < 10 ? 2 : 5, maxit = 25;
                const auto x0 = x0_for(n, 11 + (uint32_t)n);
                char tag[96];
                std::snprintf(tag, sizeof tag, "buffers n=%lld obj=%d ls=%d", (long long)n, obj, ls);
                Counter ko{LBFGS_OBJ_ROSENBROCK}, kg{LBFGS_OBJ_ROSENBROCK};
                lbfgs_host_fn cb{cb_f, cb_g, &kg};
                const lbfgs_host_fn* cbp = obj == LBFGS_OBJ_HOST ? &cb : nullptr;
                const OracleRun o = obj == LBFGS_OBJ_HOST
                                        ? oracle(ORC_OBJ_HOST, ls, n, m, maxit, x0.get(), cb_f, cb_g, &ko)
                                        : oracle(obj, ls, n, m, maxit, x0.get());
                lbfgs_ctx* c = nullptr;
                lbfgs_ctx_create(&c, n, m, 0);
                if (!c) {
                    EXPECT(false, "%s: create", tag);
                    continue;
                }
                auto x = exact(n);
                lbfgs_result res;
                const int st = lbfgs_minimize_device(c, obj, cbp, ls, nullptr, x0.get(), x.get(), maxit, 1e-5, kFlags,
                                                     &res);
                EXPECT(st >= 0, "%s: %d %s", tag, st, lbfgs_last_error(c));
                if (st >= 0) compare(tag, c, st, x.get(), n, res, o);
                // init_device + step + get_x_device against init + step + get_x
                auto xa = exact(n), xb = exact(n);
                lbfgs_result ra, rb;
                EXPECT(lbfgs_solver_init_device(c, obj, cbp, ls, nullptr, x0.get(), 1e-5, kFlags) == 0, "%s: init_device",
                       tag);
                const int sa = lbfgs_solver_step(c, 6, &ra);
                EXPECT(lbfgs_get_x_device(c, xa.get()) == 0, "%s: get_x_device", tag);
                EXPECT(lbfgs_solver_init(c, obj, cbp, ls, nullptr, x0.get(), 1e-5, kFlags) == 0, "%s: init", tag);
                const int sb = lbfgs_solver_step(c, 6, &rb);
                EXPECT(lbfgs_get_x(c, xb.get()) == 0, "%s: get_x", tag);
                EXPECT(sa == sb && ra.iterations == rb.iterations && same_bits(ra.f, rb.f) && same_bits(ra.gnorm, rb.gnorm),
                       "%s: stepping forms differ", tag);
                for (int64_t i = 0; i < n; ++i)
                    if (!same_bits(xa[i], xb[i])) {
                        EXPECT(false, "%s: stepped x[%lld]", tag, (long long)i);
                        break;
                    }
                lbfgs_ctx_destroy(c);
            }
}

int main() {
    device_callback();
    failing_callback();
    refusals();
    device_buffers();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("device-objective sanitizer job: all checks passed\n");
    return 0;
}
