/* lbfgs_driver.c — C host driver of the MI355X L-BFGS solver (public ABI: include/lbfgs_hip.h).
 *
 * The control flow is the reference's LBFGS() (sequential-implementation/lbfgs.cpp:17-203) and
 * its line searches (line_search.cpp:8-189; their loops are lbfgs_search.h's, shared with the
 * device), restated over scalars only: every n-vector lives
 * on the GPU and every vector operation is a fused device pass (lbfgs_kernels.hip). The host
 * sees, per iteration, one 512-byte read-back of the commit's reductions (g.d, f, s.y, y.y,
 * |g|^2, s.g, g.d_phi), plus one per extra line-search trial.
 *
 * Per-iteration device schedule (h stored pairs, reference line numbers):
 *   [P0]  s_{h-1}.g         fused into the previous commit (SG), or lbk_dot if that pair
 *                           was not pushed                                     (:133)
 *   h-1 x k_axpy_dot        q -= alpha_{i+1} y_{i+1};  s_i.q                    (:124-138)
 *   k_mid                   r = (q - alpha_0 y_0) gamma;  y_0.r                 (:141-154,:160)
 *   h-1 x k_axpy2_dot       r += s_i (alpha_i - beta_i);  y_{i+1}.r             (:157-165)
 *   k_commit (TWOLOOP)      d = -(r + s(alpha-beta)), g.d, x+a0 d, f, grad, s, y, dots
 *                           — the last second-loop pass, the first line-search trial at
 *                           a0 = INITIAL_STEP_SIZE and the commit, in one pass  (:163-198)
 * If the line search accepts a0 (the common case) the iteration is complete; otherwise d is
 * materialised (k_last), the remaining trials run as k_trial passes and the commit is redone
 * at the accepted step. Results are bit-identical to running the reference's steps
 * separately in the canonical reduction order (oracle/lbfgs_oracle.c, ORC_CANON).
 *
 * The three iteration loops - iterate (the schedule above and its small-n, persistent and unfused
 * forms), iterate_vf (vector-free) and iterate_cuda (the CUDA path) - and the entry points beside
 * them state each step they share once:
 *   iterate_top                trace entry, verbose line, convergence test
 *   ring_view / ring_push      the history ring read in ring order / advanced by one pair (the
 *                              speculative launch predicts with the same push); swap_iterates
 *   twoloop_passes             the launch sequence above, also lbfgs_dev_twoloop's
 *   last_update                the record of the update the commit, a trial pass or k_last forms
 *   vf_combine                 the vector-free coefficient sums, in the oracle's order
 *   cache_f / cache_g          what an external objective has evaluated at the trial point
 *   cu_interpolation, cu_wolfe the CUDA path's searches, L-BFGS.cu's and the variant files'
 */
#define _POSIX_C_SOURCE 199309L
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "lbfgs_device.h"
#include "lbfgs_hip.h"
#include "lbfgs_search.h"

/* roctx ranges (SURVEY §5 tracing): "lbfgs iteration" around every iteration and "line search"
 * around its trials, visible under rocprofv3 --marker-trace; no-ops without a tool attached.
 * The product build defines LBFGS_ROCTX (cuda-lbfgs_amd/Makefile); other host builds of this
 * file (the sanitizer job) compile them out. */
#ifdef LBFGS_ROCTX
struct hsa_agent_s; /* named in roctx.h's prototypes (C: declare before use) */
struct ihipStream_t;
#include <rocprofiler-sdk-roctx/roctx.h>
#define TRACE_PUSH(name) roctxRangePushA(name)
#define TRACE_POP() roctxRangePop()
#else
#define TRACE_PUSH(name) ((void)0)
#define TRACE_POP() ((void)0)
#endif

#define MMAX 64

/* result slots */
#define SLOT_INIT 0
#define SLOT_COMMIT0 1 /* commits alternate 1 / 2 so SG survives into the next iteration */
#define SLOT_P0 3
#define SLOT_A0 4 /* + i  : s_i . q          */
#define SLOT_B0(m) (4 + (m)) /* + i : y_i . r   */
#define SLOT_LAST(m) (4 + 2 * (m))
#define SLOT_TRIAL(m) (5 + 2 * (m))
#define SLOT_MISC(m) (6 + 2 * (m))
#define REF(slot, comp) ((slot) * LBK_KMAX + (comp))
#define D_VF 3 /* direction as a combination of the basis (vector-free mode) */

struct lbfgs_ctx {
    lbk_ctx* dev;
    const lbk_geo* geo;
    int64_t n;
    int m;
    /* device vectors */
    double *x, *g, *xn, *gn, *d, *q, *r, *gt;
    const double* rc;   /* the r the last two-loop pass wrote */
    double* S[MMAX + 1];
    double* Y[MMAX + 1];
    /* history: ring[0] oldest .. ring[h-1] newest, indices into the m+1 pair pool */
    int h, ring[MMAX + 1], free_pair;
    double sy[MMAX + 1], yy[MMAX + 1];
    /* solver state */
    int inited, obj, ls, k, status, finished;
    lbfgs_constants K;
    double tol;
    unsigned flags;
    double f_cur, gg;
    int sg_valid, sg_ref;
    lbfgs_host_fn cb;
    /* host-callback objective (LBFGS_OBJ_HOST), pinned buffers: hx the trial point z, hxx the
     * iterate x (reference call order only), hg[2] the gradient double buffer (a callback fills
     * one while the other's upload may still be in flight) */
    double *hx, *hxx, *hg[2];
    int hg_cur;
    int hz_valid, hz_pending; /* hx holds (or is receiving) z = x + hz_alpha d of this iteration */
    double hz_alpha;
    int hxx_valid, hxx_pending;
    int hf_valid; /* f(z) at hf_alpha, this iteration */
    double hf_alpha, hf_val;
    int refcalls; /* LBFGS_FLAG_REFERENCE_CALLS */
    int dense_set; /* lbfgs_set_dense_quadratic called */
    /* device-callback objective (LBFGS_OBJ_DEVICE): the caller's eval on solver-owned device
     * memory; dcb.eval == NULL: none set */
    lbfgs_device_fn dcb;
    int64_t cb_f, cb_g;
    /* per-iteration working state */
    int dmode, d_ready;
    double rho_last, a0;
    int ref_b_last, ref_a_last, s_last_pair;
    double spec_tot[LBK_KMAX];
    /* this iteration's line search (lbfgs_search.h): its constants and loop variables, and the
     * values it holds - the fused commit's first trial at a0 (have_spec), the backtracking
     * commit's f at the next step (have_cand), the last trial pass (tc_*) */
    lbk_search sr;
    int gt_valid;
    double gt_alpha;
    int unfused; /* LBFGS_FLAG_UNFUSED */
    /* batched line-search trials (LBFGS_BATCH, default on): the first commit also reduces f at
     * the backtracking search's next step; a trial pass evaluates the next LBK_TRIALS_NC steps of
     * a halving chain, or f and g.d together for the Wolfe searches; d stays unmaterialised for
     * the first two trial passes and the commit */
    int batch;
    int trial_passes;
    /* the last two-loop iteration whose search ran trial passes here took three or more of them
     * (tl_search: this iteration's search is such a one): the next one materialises d first */
    int many_passes, tl_search;
    /* small n: the device-resident line search (lbk_search_dev) commits at the step it finds into
     * this slot (-1: no commit requested); committed: it did, this iteration; recommit_a0: a
     * launch that timed out may have left the first commit's outputs partly rewritten, so the
     * commit is repeated even at the first trial's step */
    int search_cslot, search_committed, recommit_a0;
    int64_t search_launches, search_commits; /* since solver init (lbfgs_search_stats) */
    /* vector-free mode (LBFGS_FLAG_VECTOR_FREE): Gram matrix over the pair pool, indexed by
     * pool slot (P = m + 1): Gss[p][q] = s_p.s_q, Gsy[p][q] = s_p.y_q, Gyy[p][q] = y_p.y_q,
     * Gsg[p] = s_p.g, Gyg[p] = y_p.g (g = current gradient; |g|^2 is gg) */
    int vf;
    double *Gss, *Gsy, *Gyy, *Gsg, *Gyg;
    int vf_h;                            /* basis size of this iteration's direction */
    const double* vf_S[MMAX];            /* basis, ring order */
    const double* vf_Y[MMAX];
    double vf_cs[MMAX], vf_cy[MMAX], vf_cg; /* d = sum cs s + sum cy y + cg g */
    double vf_tot[LBK_KW], vf_spec[LBK_KW];
    int vf_hb;
    /* f at the backtracking candidates a0 beta, a0 beta^2, reduced by the first commit pass */
    double vf_cand[LBK_VF_NA], vf_cand_f[LBK_VF_NA];
    int vf_cand_valid;
    /* speculative next iteration (small n, cooperative form): the launch of
     * iteration sp_k queued behind iteration sp_k - 1's before the host has read that one's
     * results, with the arguments the host will pass if the first trial is taken and the pair
     * stored (the kernel checks exactly that, see lbk_spec) */
    int spec_on;                  /* LBFGS_SPEC (default 1) */
    int steps_left;               /* iterations still to run in this lbfgs_solver_step call */
    unsigned long long cur_epoch; /* this iteration's cooperative launch (0: none) */
    int cur_spec;                 /* ... which was a speculative one, adopted */
    double cur_rho, cur_gamma;    /* the host's rho of the newest pair and gamma, this iteration */
    int cur_p0;
    int sp_pend, sp_k, sp_h, sp_free, sp_p0, sp_cslot, sp_hostgo;
    double sp_alpha; /* the step the queued launch assumes iteration sp_k - 1 commits */
    int sp_ring[MMAX + 1];
    double *sp_x, *sp_xn, *sp_g, *sp_gn;
    double sp_rho[MMAX];
    unsigned long long sp_epoch;
    int64_t sp_adopted, sp_dropped;
    /* counters */
    int64_t trials_f, trials_fg, commits, passes;
    int h_min, h_max; /* pairs stored at the top of the iterations of the current call */
    /* LBFGS_FLAG_CUDA_COMPAT: the CUDA path's per-ring-slot alpha and rho (kept across iterations
     * as L-BFGS.cu's vector<double> alpha(m), rho(m)), its stale line-search gradient g0 */
    int cuda;          /* 1: LBFGS_FLAG_CUDA_COMPAT (L-BFGS.cu), 2: with LBFGS_FLAG_CUDA_VARIANT */
    double cv_f0;      /* the variants' initial_f = f(x0) */
    double cv_fhost;   /* f at their host copy x_host: the last trial point a search transferred */
    double cu_alpha[MMAX], cu_rho[MMAX];
    double* g0c;
    /* messages / trace */
    char* msg;
    int msg_len, msg_cap;
    double *tr_f, *tr_gn, *tr_a;
    uint64_t *tr_c1, *tr_c2;
    int tr_len, tr_cap;
    char err[256];
};

/* ------------------------------------------------------------------------------------------ */
static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static void say(lbfgs_ctx* c, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    int k = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (k < 0) return;
    if (!(c->flags & LBFGS_FLAG_QUIET)) {
        fputs(buf, stdout);
        fflush(stdout);
    }
    if (c->msg_len + k + 1 > c->msg_cap) {
        int cap = c->msg_cap ? c->msg_cap * 2 : 4096;
        while (cap < c->msg_len + k + 1) cap *= 2;
        char* p = (char*)realloc(c->msg, (size_t)cap);
        if (!p) return;
        c->msg = p;
        c->msg_cap = cap;
    }
    memcpy(c->msg + c->msg_len, buf, (size_t)k);
    c->msg_len += k;
    c->msg[c->msg_len] = 0;
}

static int dev_err(lbfgs_ctx* c, int rc) {
    if (rc < 0) snprintf(c->err, sizeof c->err, "%s", lbk_last_error(c->dev));
    return rc < -6 ? LBFGS_ERR_HIP : rc;
}
#define DEV(call)                                 \
    do {                                          \
        int rc_ = (call);                         \
        if (rc_ != 0) return dev_err(c, rc_);     \
        c->passes++;                              \
    } while (0)
#define DEVNC(call)                               \
    do {                                          \
        int rc_ = (call);                         \
        if (rc_ != 0) return dev_err(c, rc_);     \
    } while (0)

static int trace_push(lbfgs_ctx* c, double f, double gn, int with_ck) {
    if (!(c->flags & LBFGS_FLAG_TRACE)) return 0;
    if (c->tr_len == c->tr_cap) {
        int cap = c->tr_cap ? 2 * c->tr_cap : 1024;
        double* a = (double*)realloc(c->tr_f, sizeof(double) * cap);
        if (a) c->tr_f = a;
        a = (double*)realloc(c->tr_gn, sizeof(double) * cap);
        if (a) c->tr_gn = a;
        a = (double*)realloc(c->tr_a, sizeof(double) * cap);
        if (a) c->tr_a = a;
        uint64_t* u = (uint64_t*)realloc(c->tr_c1, sizeof(uint64_t) * cap);
        if (u) c->tr_c1 = u;
        u = (uint64_t*)realloc(c->tr_c2, sizeof(uint64_t) * cap);
        if (u) c->tr_c2 = u;
        if (!c->tr_f || !c->tr_gn || !c->tr_a || !c->tr_c1 || !c->tr_c2) return LBFGS_ERR_NOMEM;
        c->tr_cap = cap;
    }
    int i = c->tr_len++;
    c->tr_f[i] = f;
    c->tr_gn[i] = gn;
    c->tr_a[i] = NAN;
    c->tr_c1[i] = c->tr_c2[i] = 0;
    if (with_ck) DEVNC(lbk_checksum(c->dev, c->x, &c->tr_c1[i], &c->tr_c2[i]));
    return 0;
}

/* ------------------------------------------------------------------------------------------ */
void lbfgs_constants_default(lbfgs_constants* k) { /* sequential-implementation/config.h:5-17 */
    k->c1 = 1e-4;
    k->c2 = 0.9;
    k->initial_step = 1.0;
    k->backtracking_alpha = 0.5;
    k->backtracking_tol = 1e-8;
    k->wolfe_interp_min = 1e-10;
    k->wolfe_interp_max = 10.0;
}

void lbfgs_constants_cuda(lbfgs_constants* k) { /* parallel-implementation/constants.h:5-17 */
    lbfgs_constants_default(k);
    k->c2 = 0.7;
}

#ifndef LBFGS_SRC_HASH
#define LBFGS_SRC_HASH "unknown"
#endif
int lbfgs_spec_stats(const lbfgs_ctx* c, int64_t* adopted, int64_t* dropped) {
    if (!c) return LBFGS_ERR_BAD_ARG;
    if (adopted) *adopted = c->sp_adopted;
    if (dropped) *dropped = c->sp_dropped;
    return 0;
}

int lbfgs_search_stats(const lbfgs_ctx* c, int64_t* launches, int64_t* commits) {
    if (!c) return LBFGS_ERR_BAD_ARG;
    if (launches) *launches = c->search_launches;
    if (commits) *commits = c->search_commits;
    return 0;
}

#ifndef LBFGS_ARCH
#define LBFGS_ARCH "unknown"
#endif
const char* lbfgs_build_info(void) {
    return "src=" LBFGS_SRC_HASH " built=" __DATE__ " " __TIME__ " arch=" LBFGS_ARCH;
}

int lbfgs_unique_id(void* out128) { return lbk_unique_id(out128) == 0 ? 0 : LBFGS_ERR_RCCL; }

int lbfgs_device_count(void) { return lbk_device_count(); }

static void free_vectors(lbfgs_ctx* c) {
    double** v[] = {&c->x, &c->g, &c->xn, &c->gn, &c->d, &c->q, &c->r, &c->gt, &c->g0c};
    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) {
        lbk_vec_free(c->dev, *v[i]);
        *v[i] = NULL;
    }
    for (int i = 0; i <= MMAX; ++i) {
        lbk_vec_free(c->dev, c->S[i]);
        lbk_vec_free(c->dev, c->Y[i]);
        c->S[i] = c->Y[i] = NULL;
    }
}

struct lbfgs_host_group {
    lbk_group* g;
    int world;
};

int lbfgs_host_group_create(lbfgs_host_group** out, int world) {
    if (!out || world < 1 || world > 8 || (8 % world) != 0) return LBFGS_ERR_BAD_ARG;
    lbfgs_host_group* h = (lbfgs_host_group*)calloc(1, sizeof *h);
    if (!h) return LBFGS_ERR_NOMEM;
    h->g = lbk_group_create(world);
    h->world = world;
    if (!h->g) {
        free(h);
        return LBFGS_ERR_NOMEM;
    }
    *out = h;
    return 0;
}

void lbfgs_host_group_destroy(lbfgs_host_group* h) {
    if (!h) return;
    lbk_group_destroy(h->g);
    free(h);
}

static int ctx_create(lbfgs_ctx** out, int64_t n, int m, int device, int rank, int world,
                      const void* unique_id, lbk_group* grp) {
    if (!out) return LBFGS_ERR_BAD_ARG;
    *out = NULL;
    if (n < 1 || m < 1 || m > MMAX || world < 1 || (8 % world) != 0 || rank < 0 || rank >= world)
        return LBFGS_ERR_BAD_ARG;
    lbfgs_ctx* c = (lbfgs_ctx*)calloc(1, sizeof(lbfgs_ctx));
    if (!c) return LBFGS_ERR_NOMEM;
    c->n = n;
    c->m = m;
    int rc = lbk_create(&c->dev, device, n, rank, world, unique_id, grp);
    if (rc != 0) {
        if (c->dev) {
            snprintf(c->err, sizeof c->err, "%s", lbk_last_error(c->dev));
            fprintf(stderr, "lbfgs_ctx_create: %s\n", c->err);
            lbk_destroy(c->dev);
        }
        free(c);
        return rc == -3 ? LBFGS_ERR_RCCL : rc == -1 ? LBFGS_ERR_BAD_ARG : LBFGS_ERR_HIP;
    }
    c->geo = lbk_geometry(c->dev);
    double** v[] = {&c->x, &c->g, &c->xn, &c->gn, &c->d, &c->q, &c->r, &c->gt};
    int ok = 1;
    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) ok &= (*v[i] = lbk_vec_alloc(c->dev)) != NULL;
    for (int i = 0; i <= m; ++i) {
        ok &= (c->S[i] = lbk_vec_alloc(c->dev)) != NULL;
        ok &= (c->Y[i] = lbk_vec_alloc(c->dev)) != NULL;
    }
    if (!ok) {
        fprintf(stderr, "lbfgs_ctx_create: %s\n", lbk_last_error(c->dev));
        free_vectors(c);
        lbk_destroy(c->dev);
        free(c);
        return LBFGS_ERR_NOMEM;
    }
    lbk_sync(c->dev);
    *out = c;
    return 0;
}

int lbfgs_ctx_create_sharded(lbfgs_ctx** out, int64_t n, int m, int device, int rank, int world,
                             const void* unique_id) {
    return ctx_create(out, n, m, device, rank, world, unique_id, NULL);
}

int lbfgs_ctx_create_emulated(lbfgs_ctx** out, int64_t n, int m, int device, int rank,
                              lbfgs_host_group* grp) {
    if (!grp) return LBFGS_ERR_BAD_ARG;
    return ctx_create(out, n, m, device, rank, grp->world, NULL, grp->g);
}

int lbfgs_ctx_create(lbfgs_ctx** out, int64_t n, int m, int device) {
    return ctx_create(out, n, m, device, 0, 1, NULL, NULL);
}

void lbfgs_ctx_destroy(lbfgs_ctx* c) {
    if (!c) return;
    free_vectors(c);
    lbk_destroy(c->dev);
    lbk_host_free(c->hx);
    lbk_host_free(c->hxx);
    lbk_host_free(c->hg[0]);
    lbk_host_free(c->hg[1]);
    free(c->msg);
    free(c->tr_f);
    free(c->tr_gn);
    free(c->tr_a);
    free(c->tr_c1);
    free(c->tr_c2);
    free(c->Gss);
    free(c->Gsy);
    free(c->Gyy);
    free(c->Gsg);
    free(c->Gyg);
    free(c);
}

const char* lbfgs_last_error(const lbfgs_ctx* c) { return c ? c->err : "null context"; }

int lbfgs_shard_range(int64_t n, int rank, int world, int64_t* elem_lo, int64_t* n_loc) {
    lbk_geo g;
    if (lbk_geometry_plan(n, rank, world, &g) != 0) return LBFGS_ERR_BAD_ARG;
    if (elem_lo) *elem_lo = g.elem_lo;
    if (n_loc) *n_loc = g.n_loc;
    return 0;
}

int lbfgs_local_range(const lbfgs_ctx* c, int64_t* elem_lo, int64_t* n_loc) {
    if (!c) return LBFGS_ERR_BAD_ARG;
    if (elem_lo) *elem_lo = c->geo->elem_lo;
    if (n_loc) *n_loc = c->geo->n_loc;
    return 0;
}

int lbfgs_sync(lbfgs_ctx* c) { return lbk_sync(c->dev) == 0 ? 0 : LBFGS_ERR_HIP; }

int lbfgs_peer_handle(lbfgs_ctx* c, void* out) {
    if (!c || !out || lbk_peer_handle(c->dev, out) != 0) return LBFGS_ERR_BAD_ARG;
    return 0;
}

int lbfgs_peer_connect(lbfgs_ctx* c, const void* handles) {
    if (!c || !handles || c->geo->world <= 1) return LBFGS_ERR_BAD_ARG;
    const int rc = lbk_peer_connect(c->dev, handles);
    if (rc != 0) {
        snprintf(c->err, sizeof c->err, "%s", lbk_last_error(c->dev));
        return rc == -1 ? LBFGS_ERR_BAD_ARG : rc == -3 ? LBFGS_ERR_RCCL : LBFGS_ERR_HIP;
    }
    return 0;
}

int lbfgs_peer_enable(lbfgs_ctx* c, int on) {
    if (!c || c->geo->world <= 1) return LBFGS_ERR_BAD_ARG;
    return lbk_peer_enable(c->dev, on) == 0 ? 0 : LBFGS_ERR_STATE;
}

int lbfgs_rccl_attach(lbfgs_ctx* c, const void* unique_id) {
    if (!c || !unique_id || c->geo->world <= 1) return LBFGS_ERR_BAD_ARG;
    const int rc = lbk_rccl_attach(c->dev, unique_id);
    if (rc != 0) {
        snprintf(c->err, sizeof c->err, "%s", lbk_last_error(c->dev));
        return rc == -1 ? LBFGS_ERR_BAD_ARG : rc == -3 ? LBFGS_ERR_RCCL : LBFGS_ERR_HIP;
    }
    return 0;
}

int lbfgs_set_dense_quadratic(lbfgs_ctx* c, const double* A, const double* b) {
    if (!c || !A || !b || c->geo->world != 1) return LBFGS_ERR_BAD_ARG;
    const int rc = lbk_dense_set(c->dev, A, b);
    if (rc != 0) {
        snprintf(c->err, sizeof c->err, "%s", lbk_last_error(c->dev));
        return rc == -1 ? LBFGS_ERR_BAD_ARG : LBFGS_ERR_HIP;
    }
    c->inited = 0;
    c->dense_set = 1;
    return 0;
}

int lbfgs_set_device_objective(lbfgs_ctx* c, const lbfgs_device_fn* fn) {
    if (!c || (fn && (!fn->eval || c->geo->world != 1))) return LBFGS_ERR_BAD_ARG;
    if (c->inited && c->obj == LBFGS_OBJ_DEVICE) c->inited = 0; /* a solve in progress loses its objective */
    if (fn)
        c->dcb = *fn;
    else
        memset(&c->dcb, 0, sizeof c->dcb);
    return 0;
}

int lbfgs_exchange_backend(const lbfgs_ctx* c) { return c ? lbk_exchange_backend(c->dev) : LBFGS_ERR_BAD_ARG; }
int lbfgs_exchange_fold(const lbfgs_ctx* c) { return c ? lbk_exchange_fold(c->dev) : LBFGS_ERR_BAD_ARG; }

int lbfgs_exchange_latency(lbfgs_ctx* c, int backend, int components, int iters, double* us) {
    if (!c || !us) return LBFGS_ERR_BAD_ARG;
    const int rc = lbk_exchange_bench(c->dev, backend, components, iters, us);
    if (rc == 0) return 0;
    snprintf(c->err, sizeof c->err, "%s", lbk_last_error(c->dev));
    return rc == -1 ? LBFGS_ERR_BAD_ARG : rc == -5 ? LBFGS_ERR_STATE : rc == -3 ? LBFGS_ERR_RCCL : LBFGS_ERR_HIP;
}

int lbfgs_cu_partition(const lbfgs_ctx* c) { return c ? lbk_cu_partition(c->dev) : LBFGS_ERR_BAD_ARG; }

int lbfgs_vector_fallbacks(const lbfgs_ctx* c) { return c ? lbk_vec_fallbacks(c->dev) : LBFGS_ERR_BAD_ARG; }

int lbfgs_vector_pool(const lbfgs_ctx* c, int* pooled, double* held_gb) {
    return c ? lbk_vec_pool_stats(c->dev, pooled, held_gb) : LBFGS_ERR_BAD_ARG;
}

int lbfgs_wait_stats(const lbfgs_ctx* c, double* slept_s, uint64_t* waits, int* adaptive) {
    if (!c) return LBFGS_ERR_BAD_ARG;
    unsigned long long w = 0;
    const int rc = lbk_wait_stats(c->dev, slept_s, &w, adaptive);
    if (waits) *waits = (uint64_t)w;
    return rc;
}

int lbfgs_coop_info(const lbfgs_ctx* c, int* coop_max, int* search_max, int* fallbacks) {
    return c ? lbk_coop_info(c->dev, coop_max, search_max, fallbacks) : LBFGS_ERR_BAD_ARG;
}

int lbfgs_stream_probe(lbfgs_ctx* c, int launches, double* us, double* bytes) {
    /* the work vector holds a copy of y_0 (random doubles, as the passes' q): a zero-filled one
     * streamed ~3 % faster in the same process (profiles/r06/gap/), which overstated the box */
    return lbfgs_stream_probe_variant(c, 16, launches, us, bytes);
}

int lbfgs_stream_probe_variant(lbfgs_ctx* c, int variant, int launches, double* us, double* bytes) {
    if (!c || !us || launches < 1 || variant < 0 || (variant & 7) > 6 || variant > 31) return LBFGS_ERR_BAD_ARG;
    if (!c->inited) return LBFGS_ERR_STATE;
    /* + 8: the work vector is the solver's own q (variants 0-5), which the next iteration's first
     * two-loop pass rewrites from g before anything reads it (gap analysis: the same buffer as the
     * in-solve passes) */
    const int own_q = (variant & 8) != 0 && (variant & 7) <= 5;
    const int fill = (variant & 16) != 0; /* + 16: the scratch vector starts as a copy of y_0, not zeros */
    variant &= 7;
    /* the written operand is a scratch vector, not the solver's q: nothing of the solve is touched
     * (q - 0 * y is q only while y is finite) */
    double* scratch = lbk_vec_alloc(c->dev);
    if (!scratch) return dev_err(c, -2);
    double* outs[4] = {NULL, NULL, NULL, NULL}; /* variant 6: the commit's four written vectors */
    int rc = 0;
    for (int k = 0; variant == 6 && k < 4 && rc == 0; ++k)
        if (!(outs[k] = lbk_vec_alloc(c->dev))) rc = -2;
    if (rc == 0 && fill && !own_q) rc = lbk_copy(c->dev, scratch, c->Y[0]);
    if (rc == 0)
        rc = lbk_stream_probe(c->dev, own_q ? c->q : scratch, (const double* const*)c->Y, (const double* const*)c->S,
                              c->m + 1, launches, us, variant, outs);
    for (int k = 0; k < 4; ++k) lbk_vec_free(c->dev, outs[k]);
    lbk_vec_free(c->dev, scratch);
    if (rc != 0) return dev_err(c, rc);
    if (bytes) *bytes = (variant == 6 ? 64.0 : 32.0) * (double)c->geo->n_loc;
    return 0;
}

/* the context's vectors in allocation order (lbfgs_ctx_create): x, g, xn, gn, d, q, r, gt, then
 * S_0, Y_0, S_1, Y_1, ...; index 8 + 2 (m + 1) = a scratch vector allocated for the call */
static double* vec_by_index(lbfgs_ctx* c, int k, double* scratch) {
    double* w[] = {c->x, c->g, c->xn, c->gn, c->d, c->q, c->r, c->gt};
    if (k >= 0 && k < 8) return w[k];
    k -= 8;
    if (k >= 0 && k < 2 * (c->m + 1)) return (k & 1) ? c->Y[k >> 1] : c->S[k >> 1];
    return k == 2 * (c->m + 1) ? scratch : NULL;
}

int lbfgs_vector_address(lbfgs_ctx* c, int k, uint64_t* addr) {
    if (!c || !addr) return LBFGS_ERR_BAD_ARG;
    double* v = vec_by_index(c, k, NULL);
    if (!v) return LBFGS_ERR_BAD_ARG;
    *addr = (uint64_t)(uintptr_t)v;
    return 0;
}

int lbfgs_stream_probe_vectors(lbfgs_ctx* c, int qk, int yk, int sk, int launches, double* us) {
    if (!c || !us || launches < 1) return LBFGS_ERR_BAD_ARG;
    if (!c->inited) return LBFGS_ERR_STATE;
    double* scratch = lbk_vec_alloc(c->dev);
    if (!scratch) return dev_err(c, -2);
    double* q = vec_by_index(c, qk, scratch);
    const double* y = vec_by_index(c, yk, scratch);
    const double* s = vec_by_index(c, sk, scratch);
    int rc = (q && y && s) ? 0 : -1;
    /* alpha = 0: q is written back unchanged (the vectors are finite at any step of a solve) */
    if (rc == 0) rc = lbk_stream_probe(c->dev, q, &y, &s, 1, launches, us, 0, NULL);
    lbk_vec_free(c->dev, scratch);
    return rc == 0 ? 0 : rc == -1 ? LBFGS_ERR_BAD_ARG : dev_err(c, rc);
}

/* ------------------------------------------------------------------------------------------
 * Host-callback objective (LBFGS_OBJ_HOST; single rank). The device forms every point the
 * objective is called at (z = x + alpha d, as the commit will form x_new) and the host calls
 * f / grad on a pinned copy of it.
 *   default: one f and at most one grad call per distinct point: z, f(z) and grad(z) are
 *            cached for the iteration, so a Wolfe trial's gradient (line_search.cpp:160) reuses
 *            its f call (:146), and the commit (lbfgs.cpp:160,171) reuses both;
 *   LBFGS_FLAG_REFERENCE_CALLS: the reference's own call sequence, call for call, including its
 *            re-evaluations of f(x) inside the line searches (line_search.cpp:24,42,65,133) and
 *            of f, grad at x_new after them (lbfgs.cpp:160,171); values returned by those calls
 *            are the ones used, as in the reference.
 * Transfers are asynchronous on the solver stream: the gradient upload runs from one of two
 * pinned buffers while the host goes on (e.g. into the f call that follows a grad call,
 * line_search.cpp:39-42), and in the reference order z's download overlaps the f(x) call.
 * ---------------------------------------------------------------------------------------- */
#define XF_Z 0
#define XF_X 1
#define XF_G0 2 /* + buffer */

/* objectives evaluated outside the fused stencil passes: host callbacks, the dense quadratic
 * (a matrix-vector product needs the whole trial point first) and device callbacks. All run the
 * same driver path: z = x + alpha d formed on the device, f / grad at z, the commit with the
 * gradient supplied. */
static int ext_obj(const lbfgs_ctx* c) {
    return c->obj == LBFGS_OBJ_HOST || c->obj == LBFGS_OBJ_DENSE_QUAD || c->obj == LBFGS_OBJ_DEVICE;
}
/* ... whose trial point and gradient never leave the device */
static int resident_obj(const lbfgs_ctx* c) { return c->obj == LBFGS_OBJ_DENSE_QUAD || c->obj == LBFGS_OBJ_DEVICE; }

/* One call of the device callback (LBFGS_OBJ_DEVICE) at the solver vector z: f into *f and / or the
 * gradient into the solver vector g. Every launch that produced z has completed when eval is
 * entered; eval returns with its own work on g complete (include/lbfgs_hip.h). */
static int device_eval(lbfgs_ctx* c, const double* z, double* f, double* g) {
    DEVNC(lbk_sync(c->dev));
    const int rc = c->dcb.eval(z, c->n, f, g, c->dcb.user);
    if (f) c->cb_f++;
    if (g) c->cb_g++;
    if (rc != 0) {
        snprintf(c->err, sizeof c->err, "device objective callback returned %d", rc);
        return LBFGS_ERR_CALLBACK;
    }
    return 0;
}

static int host_bufs(lbfgs_ctx* c) {
    const size_t b = sizeof(double) * (size_t)c->n;
    if (!c->hx) c->hx = (double*)lbk_host_alloc(b);
    if (!c->hg[0]) c->hg[0] = (double*)lbk_host_alloc(b);
    if (!c->hg[1]) c->hg[1] = (double*)lbk_host_alloc(b);
    if (c->refcalls && !c->hxx) c->hxx = (double*)lbk_host_alloc(b);
    return (c->hx && c->hg[0] && c->hg[1] && (!c->refcalls || c->hxx)) ? 0 : LBFGS_ERR_NOMEM;
}

/* x or d changed: nothing cached refers to the current iteration */
static void host_invalidate(lbfgs_ctx* c) {
    c->hz_valid = 0;
    c->hf_valid = 0;
    c->gt_valid = 0;
}

/* issue z = x + alpha d and its download (no wait) */
static int host_point_issue(lbfgs_ctx* c, double alpha) {
    if (c->hz_valid && c->hz_alpha == alpha) return 0;
    if (c->hz_pending) DEVNC(lbk_xfer_wait(c->dev, XF_Z)); /* hx is still being written */
    DEV(lbk_point(c->dev, c->xn, c->x, c->d, alpha));
    if (resident_obj(c)) { /* z stays on the device (xn) */
        c->hz_valid = 1;
        c->hz_pending = 0;
        c->hz_alpha = alpha;
        c->hf_valid = 0;
        return 0;
    }
    DEVNC(lbk_download_local_async(c->dev, c->hx, c->xn, XF_Z));
    c->hz_valid = c->hz_pending = 1;
    c->hz_alpha = alpha;
    c->hf_valid = 0;
    return 0;
}

static int host_point(lbfgs_ctx* c, double alpha) {
    int rc = host_point_issue(c, alpha);
    if (rc) return rc;
    if (c->hz_pending) {
        DEVNC(lbk_xfer_wait(c->dev, XF_Z));
        c->hz_pending = 0;
    }
    return 0;
}

/* f(z(alpha)) is now known */
static void cache_f(lbfgs_ctx* c, double alpha, double f) {
    c->hf_valid = 1;
    c->hf_alpha = alpha;
    c->hf_val = f;
}

/* grad(z(alpha)) is now in dst: cached if dst is gt, else a gt cached at this alpha is dropped
 * (the values of the latest call are the ones used) */
static void cache_g(lbfgs_ctx* c, double alpha, const double* dst) {
    if (dst == c->gt) {
        c->gt_valid = 1;
        c->gt_alpha = alpha;
    } else if (c->gt_valid && c->gt_alpha == alpha) {
        c->gt_valid = 0;
    }
}

/* f(z(alpha)); fresh = 1 calls f even if it was evaluated at this point before */
static int host_f_at(lbfgs_ctx* c, double alpha, int fresh, double* f) {
    if (!fresh && c->hf_valid && c->hf_alpha == alpha && c->hz_valid && c->hz_alpha == alpha) {
        *f = c->hf_val;
        return 0;
    }
    int rc = host_point(c, alpha);
    if (rc) return rc;
    if (c->obj == LBFGS_OBJ_DENSE_QUAD) { /* f and, for free, grad into gt */
        DEV(lbk_dense_eval(c->dev, c->xn, c->gt, SLOT_TRIAL(c->m)));
        DEVNC(lbk_fetch(c->dev, SLOT_TRIAL(c->m), 1, f));
        cache_g(c, alpha, c->gt);
    } else if (c->obj == LBFGS_OBJ_DEVICE) {
        /* LBFGS_DEVICE_EAGER_GRAD: the gradient with every f, into gt as the dense objective's */
        const int eager = (c->dcb.flags & LBFGS_DEVICE_EAGER_GRAD) != 0;
        rc = device_eval(c, c->xn, f, eager ? c->gt : NULL);
        if (rc) return rc;
        if (eager) cache_g(c, alpha, c->gt);
    } else {
        *f = c->cb.f(c->hx, c->n, c->cb.user);
        c->cb_f++;
    }
    cache_f(c, alpha, *f);
    return 0;
}

/* grad(z(alpha)) into the device vector dst (the upload is left in flight) */
static int host_g_at(lbfgs_ctx* c, double alpha, int fresh, double* dst) {
    if (!fresh && c->gt_valid && c->gt_alpha == alpha) {
        if (dst != c->gt) DEVNC(lbk_copy(c->dev, dst, c->gt));
        return 0;
    }
    int rc = host_point(c, alpha);
    if (rc) return rc;
    if (c->obj == LBFGS_OBJ_DENSE_QUAD) {
        double f;
        DEV(lbk_dense_eval(c->dev, c->xn, dst, SLOT_TRIAL(c->m)));
        DEVNC(lbk_fetch(c->dev, SLOT_TRIAL(c->m), 1, &f));
        cache_f(c, alpha, f);
    } else if (c->obj == LBFGS_OBJ_DEVICE) { /* f with it where this point's is not cached yet */
        const int need_f = !(c->hf_valid && c->hf_alpha == alpha);
        double f = 0.0;
        rc = device_eval(c, c->xn, need_f ? &f : NULL, dst);
        if (rc) return rc;
        if (need_f) cache_f(c, alpha, f);
    } else {
        const int b = c->hg_cur;
        c->hg_cur ^= 1;
        DEVNC(lbk_xfer_wait(c->dev, XF_G0 + b)); /* the upload that last read this buffer */
        c->cb.grad(c->hx, c->n, c->hg[b], c->cb.user);
        c->cb_g++;
        DEVNC(lbk_upload_local_async(c->dev, dst, c->hg[b], XF_G0 + b));
    }
    cache_g(c, alpha, dst);
    return 0;
}

/* reference call order: f at the iterate x itself (line_search.cpp:24,42,65,133) */
static int host_fx_issue(lbfgs_ctx* c) {
    if (c->hxx_valid) return 0;
    DEVNC(lbk_download_local_async(c->dev, c->hxx, c->x, XF_X));
    c->hxx_valid = c->hxx_pending = 1;
    return 0;
}

static int host_fx(lbfgs_ctx* c, double* f) {
    int rc = host_fx_issue(c);
    if (rc) return rc;
    if (c->hxx_pending) {
        DEVNC(lbk_xfer_wait(c->dev, XF_X));
        c->hxx_pending = 0;
    }
    *f = c->cb.f(c->hxx, c->n, c->cb.user);
    c->cb_f++;
    return 0;
}

/* f(x) as a line search sees it: the reference's fresh call in its order (the next trial
 * point's download issued first, so it overlaps the call), else the iteration's f_current */
static int ls_fx(lbfgs_ctx* c, double next_alpha, double* fx) {
    if (!(c->obj == LBFGS_OBJ_HOST && c->refcalls)) {
        *fx = c->f_cur;
        return 0;
    }
    int rc = host_fx_issue(c);
    if (!rc && next_alpha > 0) rc = host_point_issue(c, next_alpha);
    if (!rc) rc = host_fx(c, fx);
    return rc;
}

/* ------------------------------------------------------------------------------------------
 * Line-search trial evaluation. The fused speculative commit already evaluated f and
 * g_new.d at a0; every other step runs one k_trial pass over materialised x, d.
 * ---------------------------------------------------------------------------------------- */
static int materialize_d(lbfgs_ctx* c) {
    if (c->d_ready) return 0;
    const int m = c->m;
    if (c->dmode == LBK_D_TWOLOOP) {
        DEV(lbk_last(c->dev, c->d, c->rc, c->S[c->s_last_pair], c->g, c->rho_last, c->ref_b_last,
                     c->ref_a_last, SLOT_LAST(m)));
    } else if (c->dmode == D_VF) {
        DEV(lbk_vf_dir(c->dev, c->vf_h, c->d, c->g, c->vf_S, c->vf_Y, c->vf_cs, c->vf_cy, c->vf_cg));
    } else if (c->dmode == LBK_D_NEG_G && c->unfused) {
        DEV(lbk_update(c->dev, LBK_U_NEG, c->d, c->g, NULL, 0.0, -1, -1, 0.0));
        DEV(lbk_dot(c->dev, c->g, c->d, SLOT_LAST(m)));
    } else if (c->dmode == LBK_D_NEG_G) {
        DEV(lbk_negdot(c->dev, c->d, c->g, SLOT_LAST(m)));
    }
    /* sharded: neighbours' edge d rides this slot (vector-free: d's ghost cells hold it) */
    lbk_set_ghost_slot(c->dev, c->dmode == D_VF ? -1 : SLOT_LAST(m));
    c->dmode = LBK_D_BUF;
    c->d_ready = 1;
    return 0;
}

/* Device objectives, batched (c->batch). The steps a search tries after a rejection are known in
 * advance on its halving chains - backtracking alpha * beta (line_search.cpp:26), interpolation
 * alpha * 0.5 once alpha_prev == alpha (:92-97, the reference's alpha_prev quirk) - so one pass
 * evaluates LBK_TRIALS_NC of them, formed by the same repeated multiplication as the search. The
 * Wolfe searches' next step depends on the f just computed, so their pass takes one step, with
 * g.d (:160) in the same read (the gradient is recomputed by the commit, never stored). Results
 * are those of separate single-step passes, bit for bit. */
static int trial_batched(lbfgs_ctx* c, double alpha, int need_g, double* f, double* dphi) {
    const int want_dphi = need_g || c->ls == LBFGS_LS_WOLFE || c->ls == LBFGS_LS_BACKTRACKING_WOLFE;
    double a[LBK_TRIALS_NC];
    int nc = 1;
    a[0] = alpha;
    if (!want_dphi) {
        nc = LBK_TRIALS_NC;
        lbk_search_chain(c->ls, &c->sr, alpha, a);
    }
    /* d: the buffer once materialised; -g formed on the fly (one rank); the last second-loop
     * update formed on the fly for this iteration's first two trial passes, then materialised
     * (3 vector reads per pass against 4 once for k_last + 2 per pass: 2 P + 6 for P >= 3 passes
     * against 2 P + 4 with d materialised first). A search that took three or more passes in the
     * last iteration that had any (a Wolfe search far from its first step takes a pass per step)
     * is taken to do so again: d is materialised first, as without batching. The same bits. */
    int dm = LBK_D_BUF;
    if (!c->d_ready) {
        if (c->dmode == LBK_D_TWOLOOP) c->tl_search = 1;
        if (c->dmode == LBK_D_NEG_G && c->geo->world == 1) {
            dm = LBK_D_NEG_G;
        } else if (c->dmode == LBK_D_TWOLOOP && c->trial_passes < 2 && !c->many_passes) {
            dm = LBK_D_TWOLOOP;
        } else {
            int rc = materialize_d(c);
            if (rc) return rc;
        }
    }
    const double* dsrc = dm == LBK_D_BUF ? c->d : dm == LBK_D_TWOLOOP ? c->rc : NULL;
    const double* s_last = dm == LBK_D_TWOLOOP ? c->S[c->s_last_pair] : NULL;
    DEV(lbk_trials(c->dev, c->obj, dm, c->x, dsrc, s_last, c->g, c->rho_last, c->ref_b_last, c->ref_a_last, a, nc,
                   want_dphi, SLOT_TRIAL(c->m)));
    double t[LBK_TRIALS_NC + 1];
    DEVNC(lbk_fetch(c->dev, SLOT_TRIAL(c->m), nc + (want_dphi ? 1 : 0), t));
    c->trial_passes++;
    *f = t[0];
    if (want_dphi) {
        lbk_search_note_fg(&c->sr, alpha, t);
        *dphi = t[1];
        c->trials_fg++;
    } else {
        lbk_search_note_f(&c->sr, a, t);
        c->trials_f++;
    }
    return 0;
}

static int trial(lbfgs_ctx* c, double alpha, int need_g, double* f, double* dphi) {
    if (c->vf && c->vf_cand_valid && !need_g) { /* f already reduced by the first commit pass */
        for (int j = 0; j < LBK_VF_NA; ++j)
            if (alpha == c->vf_cand[j]) {
                *f = c->vf_cand_f[j];
                return 0;
            }
    }
    if (lbk_search_lookup(&c->sr, alpha, need_g, f, dphi)) return 0;
    if (c->batch && !c->unfused && !ext_obj(c)) return trial_batched(c, alpha, need_g, f, dphi);
    int rc = materialize_d(c);
    if (rc) return rc;
    if (c->unfused) {
        /* x_new = x + alpha d materialised, then f (and grad, g_new . d) on it */
        double t[2];
        DEV(lbk_update(c->dev, LBK_U_POINT, c->xn, c->x, c->d, 0.0, -1, -1, alpha));
        DEV(lbk_eval(c->dev, c->obj, c->xn, need_g ? c->gt : NULL, SLOT_TRIAL(c->m)));
        DEVNC(lbk_fetch(c->dev, SLOT_TRIAL(c->m), 1, t));
        *f = t[0];
        if (need_g) {
            DEV(lbk_dot(c->dev, c->gt, c->d, SLOT_MISC(c->m) + 3));
            DEVNC(lbk_fetch(c->dev, SLOT_MISC(c->m) + 3, 1, &t[1]));
            *dphi = t[1];
        }
    } else if (ext_obj(c)) {
        /* reference order: the backtracking-Wolfe search takes grad(x_new) before f(x_new)
         * (line_search.cpp:39-42); the Wolfe search's gradient follows its own f call at the
         * same point (:146,160), never a second f */
        const int rf = c->refcalls && !(need_g && c->ls == LBFGS_LS_WOLFE);
        if (need_g && c->ls == LBFGS_LS_BACKTRACKING_WOLFE) {
            rc = host_g_at(c, alpha, c->refcalls, c->gt);
            if (!rc) rc = host_f_at(c, alpha, rf, f);
        } else {
            rc = host_f_at(c, alpha, rf, f);
            if (!rc && need_g) rc = host_g_at(c, alpha, c->refcalls, c->gt);
        }
        if (rc) return rc;
        if (need_g) {
            double t;
            DEV(lbk_dot(c->dev, c->gt, c->d, SLOT_TRIAL(c->m)));
            DEVNC(lbk_fetch(c->dev, SLOT_TRIAL(c->m), 1, &t));
            *dphi = t;
        }
    } else {
        double t[2];
        DEV(lbk_trial(c->dev, c->obj, c->x, c->d, alpha, need_g ? c->gt : NULL, SLOT_TRIAL(c->m)));
        DEVNC(lbk_fetch(c->dev, SLOT_TRIAL(c->m), 2, t));
        *f = t[0];
        if (need_g) *dphi = t[1];
    }
    if (need_g)
        c->trials_fg++;
    else
        c->trials_f++;
    return 0;
}

/* Small n (single rank, a cooperative size, device objective): once a line search needs a trial
 * pass, the rest of the search runs on the device in one launch (lbk_search_dev: the same loop
 * from the same text, lbfgs_search.h, so the same passes and caches) instead of a
 * launch and a host round trip per trial pass, and the commit at the step it finds follows in the
 * same launch. search_here: trial(alpha, need_g) would launch a pass, and the device form applies. */
static int search_here(const lbfgs_ctx* c, double alpha, int need_g) {
    double f, dphi;
    if (ext_obj(c) || c->unfused || !c->batch || c->vf || !lbk_search_dev_ok(c->dev, c->obj)) return 0;
    return !lbk_search_lookup(&c->sr, alpha, need_g, &f, &dphi);
}

/* c->sr at the top of an iteration of its loop goes to the device and comes back as the host loop
 * would have left it. Returns 0 (sr.done: the step; else its pass budget is spent and the loop
 * variables are those to go on from), 1 when the launch's grid barrier timed out (nothing came
 * back: the host loop goes on from the same state, and the device form is off for the context),
 * or < 0. */
static int search_device(lbfgs_ctx* c) {
    lbk_search* st = &c->sr;
    int rc = materialize_d(c);
    if (rc) return rc;
    lbk_search_commit cm = {c->g, c->xn, c->gn, c->S[c->free_pair], c->Y[c->free_pair], c->search_cslot};
    rc = lbk_search_dev(c->dev, c->obj, c->ls, c->x, c->d, st, &cm);
    if (rc == -6) { /* barrier time-out: the host loop takes over */
        if (cm.slot >= 0) c->recommit_a0 = 1;
        return 1;
    }
    if (rc) return dev_err(c, rc);
    const int passes = st->passes_f + st->passes_fg;
    c->trials_f += st->passes_f;
    c->trials_fg += st->passes_fg;
    c->trial_passes += passes;
    c->passes += passes;
    c->search_launches++;
    if (st->committed) {
        c->search_committed = 1;
        c->search_commits++;
        c->passes++;
    }
    return 0;
}

/* the host's trial for the shared loops: stops the loop where the device form applies (not for
 * the one trial after a launch that came back unfinished: that iteration runs here, as it would
 * have without the device form). With LBFGS_FLAG_REFERENCE_CALLS it makes the reference's fresh
 * f(x) calls in its order: before every backtracking trial (line_search.cpp:24, left operand
 * first), after every backtracking-Wolfe trial (:42). */
typedef struct {
    lbfgs_ctx* c;
    int on_host;
} ls_host;

static int host_trial(void* ctx, double alpha, int need_g, double* f, double* dphi) {
    ls_host* h = (ls_host*)ctx;
    lbfgs_ctx* c = h->c;
    if (!h->on_host && search_here(c, alpha, need_g)) return 0;
    h->on_host = 0;
    int rc = 0;
    if (c->ls == LBFGS_LS_BACKTRACKING) rc = ls_fx(c, alpha, &c->sr.f_x);
    if (!rc) rc = trial(c, alpha, need_g, f, dphi);
    if (!rc && c->ls == LBFGS_LS_BACKTRACKING_WOLFE) rc = ls_fx(c, 0.0, &c->sr.f_x);
    return rc ? rc : 1; /* (errors are negative) */
}

/* line_search.cpp:19-189: the loops of lbfgs_search.h from their start values (f(x) == f_current,
 * g.d == gd: identical values, evaluated once), over host_trial, continued on the device where
 * that applies. After a launch that came back unfinished (its pass budget spent, or its grid
 * barrier timed out) the loop resumes from c->sr with that iteration's trial on the host; only
 * the next iteration may launch again. */
static int search_run(lbfgs_ctx* c, double gd, double* out) {
    const lbfgs_constants* K = &c->K;
    lbk_search* s = &c->sr;
    s->gd = gd;
    s->c1 = K->c1;
    s->c2 = K->c2;
    s->amin = K->wolfe_interp_min;
    s->init = K->initial_step;
    s->beta = K->backtracking_alpha;
    s->tol = K->backtracking_tol;
    s->f_x = c->f_cur;
    if (c->ls == LBFGS_LS_INTERPOLATION || c->ls == LBFGS_LS_WOLFE) { /* :65,133 */
        const int rc = ls_fx(c, K->initial_step, &s->f_x);
        if (rc) return rc;
    }
    s->alpha = K->initial_step;
    s->alpha_prev = s->alpha_lo = 0.0;
    s->alpha_hi = INFINITY;
    s->f_prev = s->f_lo = s->f_x;
    s->dphi_lo = gd;
    s->iter = 0;
    s->done = s->committed = 0;
    ls_host h = {c, 0};
    while (!s->done) {
        int rc = lbk_search_run(c->ls, s, host_trial, &h);
        if (rc) return rc;
        if (s->done) break;
        rc = search_device(c); /* host_trial stopped the loop */
        if (rc < 0) return rc;
        h.on_host = 1;
    }
    *out = s->step;
    return 0;
}

static int run_line_search(lbfgs_ctx* c, double gd, double* alpha) {
    TRACE_PUSH("line search");
    const int rc = search_run(c, gd, alpha);
    TRACE_POP();
    return rc;
}

/* ------------------------------------------------------------------------------------------
 * Commit at step alpha: x_new, g_new, s, y and their reductions into tot[].
 * ---------------------------------------------------------------------------------------- */
/* unfused commit (LBFGS_FLAG_UNFUSED): lbfgs.cpp:159-181 one operation per launch */
static int commit_unfused(lbfgs_ctx* c, double alpha, double* tot) {
    const int pair = c->free_pair, sm = SLOT_MISC(c->m);
    double t[2];
    DEV(lbk_update(c->dev, LBK_U_POINT, c->xn, c->x, c->d, 0.0, -1, -1, alpha));
    DEV(lbk_eval(c->dev, c->obj, c->xn, c->gn, sm)); /* f(x_new), g_new, g_new . g_new */
    DEV(lbk_update(c->dev, LBK_U_SUB, c->S[pair], c->xn, c->x, 0.0, -1, -1, 0.0));
    DEV(lbk_update(c->dev, LBK_U_SUB, c->Y[pair], c->gn, c->g, 0.0, -1, -1, 0.0));
    DEV(lbk_dot(c->dev, c->S[pair], c->Y[pair], sm + 1));
    DEV(lbk_dot(c->dev, c->Y[pair], c->Y[pair], sm + 2));
    DEVNC(lbk_fetch(c->dev, sm, 2, t));
    tot[LBK_C_F] = t[0];
    tot[LBK_C_GG] = t[1];
    DEVNC(lbk_fetch(c->dev, sm + 1, 1, &tot[LBK_C_SY]));
    DEVNC(lbk_fetch(c->dev, sm + 2, 1, &tot[LBK_C_YY]));
    c->commits++;
    return 0;
}

/* unfused two-loop (lbfgs.cpp:127-171): a dot launch and an update launch per pair and
 * loop, gamma scaling and d = -r as launches of their own; leaves d and g.d (SLOT_LAST) */
static int twoloop_unfused(lbfgs_ctx* c, const double* rho, double gamma) {
    const int h = c->h, m = c->m;
    const double* qsrc = c->g;
    for (int i = h - 1; i >= 0; --i) {
        const int sa = i == h - 1 ? SLOT_P0 : SLOT_A0 + i;
        DEV(lbk_dot(c->dev, c->S[c->ring[i]], qsrc, sa));
        DEV(lbk_update(c->dev, LBK_U_AXPY_Q, c->q, qsrc, c->Y[c->ring[i]], rho[i], sa, -1, 0.0));
        qsrc = c->q;
    }
    DEV(lbk_update(c->dev, LBK_U_SCALE, c->r, c->q, NULL, 0.0, -1, -1, gamma));
    for (int i = 0; i < h; ++i) {
        const int sa = i == h - 1 ? SLOT_P0 : SLOT_A0 + i, sb = SLOT_B0(m) + i;
        DEV(lbk_dot(c->dev, c->Y[c->ring[i]], c->r, sb));
        DEV(lbk_update(c->dev, LBK_U_AXPY_R, c->r, c->r, c->S[c->ring[i]], rho[i], sa, sb, 0.0));
    }
    DEV(lbk_update(c->dev, LBK_U_NEG, c->d, c->r, NULL, 0.0, -1, -1, 0.0));
    DEV(lbk_dot(c->dev, c->g, c->d, SLOT_LAST(m)));
    c->dmode = LBK_D_BUF;
    c->d_ready = 1;
    return 0;
}

static int commit(lbfgs_ctx* c, int dmode, double alpha, int cslot, double* tot, double cand) {
    if (c->unfused) return commit_unfused(c, alpha, tot);
    const int pair = c->free_pair;
    const double* dsrc = dmode == LBK_D_BUF ? c->d : c->rc;
    const double* s_last = dmode == LBK_D_TWOLOOP ? c->S[c->s_last_pair] : NULL;
    int obj = c->obj;
    if (ext_obj(c)) {
        /* f(x_new) (lbfgs.cpp:160), then - unless the step failed (:164-168) - grad(x_new)
         * (:171) onto the device for the commit kernel; both from the line search's cache
         * unless the reference call order asks for the reference's fresh calls */
        double f;
        int rc = host_f_at(c, alpha, c->refcalls, &f);
        if (rc) return rc;
        if (alpha < 1e-10) { /* the caller stops here; nothing else of tot is read */
            tot[LBK_C_F] = f;
            return 0;
        }
        rc = host_g_at(c, alpha, c->refcalls, c->gn);
        if (rc) return rc;
        obj = LBK_OBJ_NONE;
        DEV(lbk_commit(c->dev, obj, dmode, c->x, dsrc, s_last, c->g, c->rho_last, c->ref_b_last,
                       c->ref_a_last, alpha, c->xn, c->gn, c->S[pair], c->Y[pair], cslot, 0.0));
        DEVNC(lbk_fetch(c->dev, cslot, 7, tot));
        tot[LBK_C_F] = f;
    } else {
        const int with_cand = cand > 0.0 && dmode != LBK_D_BUF;
        DEV(lbk_commit(c->dev, obj, dmode, c->x, dsrc, s_last, c->g, c->rho_last, c->ref_b_last,
                       c->ref_a_last, alpha, c->xn, c->gn, c->S[pair], c->Y[pair], cslot, with_cand ? cand : 0.0));
        DEVNC(lbk_fetch(c->dev, cslot, with_cand ? 8 : 7, tot));
        if (with_cand) {
            c->sr.have_cand = 1;
            c->sr.cand_a = cand;
            c->sr.cand_f = tot[LBK_C_FC];
        }
    }
    c->commits++;
    return 0;
}

/* ------------------------------------------------------------------------------------------
 * One iteration of lbfgs.cpp:72-199. Returns 0 to continue, 1 when finished, < 0 on error.
 * ---------------------------------------------------------------------------------------- */
static void note_h(lbfgs_ctx* c, int h) {
    if (c->h_min < 0 || h < c->h_min) c->h_min = h;
    if (h > c->h_max) c->h_max = h;
}

/* the top of an iteration (:72-84): the trace entry, the verbose line, the convergence test.
 * Returns 1 when converged. */
static int iterate_top(lbfgs_ctx* c) {
    const double gnorm = sqrt(c->gg);
    const int rc = trace_push(c, c->f_cur, gnorm, 1);
    if (rc) return rc;
    if (c->flags & LBFGS_FLAG_VERBOSE) { /* :76-78 */
        printf("Iteration %d, f = %g, |grad| = %g\n", c->k, c->f_cur, gnorm);
        fflush(stdout);
    }
    if (gnorm < c->tol) { /* :80-84 */
        say(c, "Converged!\n");
        c->status = LBFGS_STATUS_CONVERGED;
        return 1;
    }
    note_h(c, c->h);
    return 0;
}

/* The history ring, shared by every path that reads or advances it.
 * ring_view: the h pairs of a ring in ring order (oldest first) - rho_i = 1 / s_i.y_i and / or
 * the pairs' vectors, whichever is asked for. */
static void ring_view(const lbfgs_ctx* c, const int* ring, int h, double* rho, const double** Sr,
                      const double** Yr) {
    for (int i = 0; i < h; ++i) {
        if (rho) rho[i] = 1.0 / c->sy[ring[i]];
        if (Sr) {
            Sr[i] = c->S[ring[i]];
            Yr[i] = c->Y[ring[i]];
        }
    }
}

/* ring_push (:182-191): the pair in pool slot *free_pair becomes the newest. A full ring drops its
 * oldest pair, whose slot is the next free one; otherwise pool slots 0..h-1 are used and h is free. */
static void ring_push(int m, int* ring, int* h, int* free_pair) {
    const int pair = *free_pair;
    if (*h >= m) {
        const int oldest = ring[0];
        for (int i = 0; i + 1 < m; ++i) ring[i] = ring[i + 1];
        ring[m - 1] = pair;
        *free_pair = oldest;
    } else {
        ring[(*h)++] = pair;
        *free_pair = *h;
    }
}

/* x = x_new, g = g_new (:197-198): the buffers trade places */
static void swap_iterates(lbfgs_ctx* c) {
    double* t = c->x;
    c->x = c->xn;
    c->xn = t;
    t = c->g;
    c->g = c->gn;
    c->gn = t;
}

/* the backtracking search's second step, f reduced by the commit pass (line_search.cpp:26) */
static double first_cand(const lbfgs_ctx* c) {
    return (c->batch && c->ls == LBFGS_LS_BACKTRACKING) ? c->K.initial_step * c->K.backtracking_alpha : 0.0;
}

/* a queued speculative launch the host does not take: wait for its record. It either did not go
 * (nothing written, reservations released) or ran on buffers the host no longer reads - which
 * holds only if the host also took the first trial and stored the pair in the iteration before
 * (the kernel's other tests - convergence, rho, gamma - can only differ by a rounding the
 * host then handles itself). */
static int spec_drop(lbfgs_ctx* c) {
    if (!c->sp_pend) return 0;
    c->sp_pend = 0;
    c->sp_dropped++;
    double t[1];
    int went = 0;
    DEVNC(lbk_small_fetch(c->dev, c->sp_epoch, c->sp_cslot, 1, t, &went, NULL, NULL));
    if (!went) c->passes--; /* a launch that did nothing is no pass */
    if (went && !c->sp_hostgo) {
        snprintf(c->err, sizeof c->err, "speculative iteration %d ran where the host stopped", c->sp_k);
        return LBFGS_ERR_STATE;
    }
    return 0;
}

/* queue iteration k + 1 behind iteration k's latest commit, assuming the pair is stored: the ring
 * then drops its oldest pair (h = m) or grows, the new pair is the current free one, x/xn and g/gn
 * swap, and alpha_{h-1} of the first loop is the commit's s.g (component SG). decided = 0: behind
 * the cooperative launch, whose commit at a0 the line search has yet to judge (the kernel
 * re-checks its first-trial test); decided > 0: behind a recommit at that step */
static int spec_next(lbfgs_ctx* c, double decided) {
    const int m = c->m, h = c->h, k = c->k;
    if (!c->spec_on || c->steps_left <= 0 || c->cur_epoch == 0 || c->K.initial_step < 1e-10) return 0;
    int ring1[MMAX + 1], h1 = h, free1 = c->free_pair; /* the ring after the push */
    memcpy(ring1, c->ring, sizeof(int) * (size_t)h);
    ring_push(m, ring1, &h1, &free1);
    if (!lbk_small_spec_ok(c->dev, h1)) return 0;
    const double* Sr[MMAX];
    const double* Yr[MMAX];
    double rho1[MMAX];
    ring_view(c, ring1, h1, rho1, Sr, Yr);
    rho1[h1 - 1] = 0.0; /* the new pair's: the kernel's */
    const int cslot = SLOT_COMMIT0 + (k & 1), cslot1 = SLOT_COMMIT0 + ((k + 1) & 1);
    const int p01 = REF(cslot, LBK_C_SG);
    lbk_spec sp;
    sp.prev_slot = cslot;
    sp.ls = decided > 0.0 ? -1 : c->ls; /* a recommit's step is the host's already */
    sp.fx = c->f_cur;
    sp.c1 = c->K.c1;
    sp.c2 = c->K.c2;
    sp.tol = c->tol;
    sp.chain_epoch = c->cur_spec && decided <= 0.0 ? c->cur_epoch : 0;
    DEV(lbk_small_iter(c->dev, c->obj, h1, c->gn, c->q, c->r, Sr, Yr, rho1, 0.0, p01, c->K.initial_step, c->xn,
                       c->x, c->g, c->S[free1], c->Y[free1], SLOT_P0, SLOT_A0, SLOT_B0(m), cslot1, first_cand(c),
                       &sp, &c->sp_epoch));
    c->sp_alpha = decided > 0.0 ? decided : c->K.initial_step;
    c->sp_pend = 1;
    c->sp_k = k + 1;
    c->sp_h = h1;
    memcpy(c->sp_ring, ring1, sizeof(int) * (size_t)h1);
    c->sp_free = free1;
    c->sp_p0 = p01;
    c->sp_cslot = cslot1;
    c->sp_x = c->xn;
    c->sp_xn = c->x;
    c->sp_g = c->gn;
    c->sp_gn = c->g;
    memcpy(c->sp_rho, rho1, sizeof(double) * (size_t)h1);
    c->sp_hostgo = 0;
    return 0;
}

/* this iteration's cooperative (or single-workgroup) launch: the two-loop passes and the commit at a0 */
static int small_launch(lbfgs_ctx* c, const double* rho, const double* const* Sr, const double* const* Yr,
                        double gamma, int p0_ref) {
    DEV(lbk_small_iter(c->dev, c->obj, c->h, c->g, c->q, c->r, Sr, Yr, rho, gamma, p0_ref, c->K.initial_step,
                       c->x, c->xn, c->gn, c->S[c->free_pair], c->Y[c->free_pair], SLOT_P0, SLOT_A0,
                       SLOT_B0(c->m), SLOT_COMMIT0 + (c->k & 1), first_cand(c), NULL, &c->cur_epoch));
    c->cur_spec = 0;
    return 0;
}

/* the commit totals of this iteration's small launch. An adopted speculative launch that did not
 * go (its tests disagreed with the host's, possible only through a rounding difference: never
 * seen) is replaced by an ordinary launch; the one queued behind it was chained to it and did not
 * go either. One that went with another rho or gamma than the host's cannot be replaced (the
 * launch behind it has overwritten this iteration's x) and fails the solve. */
static int small_fetch(lbfgs_ctx* c, int cslot, double* tot) {
    int went = 1;
    double vr = 0.0, vg = 0.0;
    DEVNC(lbk_small_fetch(c->dev, c->cur_epoch, cslot, 8, tot, &went, &vr, &vg));
    if (!c->cur_spec) return 0;
    if (!went) {
        c->passes -= c->sp_pend ? 2 : 1; /* this launch and the one chained behind it did nothing */
        c->sp_pend = 0;
        c->sp_dropped++;
        double rho[MMAX];
        const double* Sr[MMAX];
        const double* Yr[MMAX];
        ring_view(c, c->ring, c->h, rho, Sr, Yr);
        int rc = small_launch(c, rho, Sr, Yr, c->cur_gamma, c->cur_p0);
        if (rc) return rc;
        DEVNC(lbk_small_fetch(c->dev, c->cur_epoch, cslot, 8, tot, NULL, NULL, NULL));
        return 0;
    }
    if (memcmp(&vr, &c->cur_rho, sizeof vr) != 0 || memcmp(&vg, &c->cur_gamma, sizeof vg) != 0) {
        snprintf(c->err, sizeof c->err, "speculative iteration %d: device rho/gamma %.17g/%.17g, host %.17g/%.17g",
                 c->k, vr, vg, c->cur_rho, c->cur_gamma);
        return LBFGS_ERR_STATE;
    }
    c->sp_adopted++;
    return 0;
}

/* small n, the line search took another step than a0: the recommit, then iteration k + 1 queued
 * behind it (no line-search test: the step is decided), then the commit's totals once the stream
 * has passed the recommit */
static int commit_queued(lbfgs_ctx* c, int dmode, double alpha, int cslot, double* tot) {
    const int pair = c->free_pair;
    const double* dsrc = dmode == LBK_D_BUF ? c->d : c->rc;
    const double* s_last = dmode == LBK_D_TWOLOOP ? c->S[c->s_last_pair] : NULL;
    DEV(lbk_commit(c->dev, c->obj, dmode, c->x, dsrc, s_last, c->g, c->rho_last, c->ref_b_last, c->ref_a_last, alpha,
                   c->xn, c->gn, c->S[pair], c->Y[pair], cslot, 0.0));
    DEVNC(lbk_mark(c->dev)); /* an event, not a pass */
    int rc = alpha >= 1e-10 ? spec_next(c, alpha) : 0;
    if (rc) return rc;
    DEVNC(lbk_fetch_marked(c->dev, cslot, 7, tot));
    c->commits++;
    return 0;
}

/* the queued launch is this iteration's exactly (same history, buffers, slots and the host's
 * rho of the older pairs; rho and gamma of the newest pair are compared when its record is read) */
static int spec_matches(const lbfgs_ctx* c, int h, const double* rho, int p0_ref) {
    if (!c->sp_pend || c->sp_k != c->k || c->sp_h != h || c->sp_free != c->free_pair || c->sp_p0 != p0_ref ||
        c->sp_cslot != SLOT_COMMIT0 + (c->k & 1) || c->sp_x != c->x || c->sp_xn != c->xn || c->sp_g != c->g ||
        c->sp_gn != c->gn)
        return 0;
    for (int i = 0; i < h; ++i)
        if (c->sp_ring[i] != c->ring[i]) return 0;
    for (int i = 0; i + 1 < h; ++i)
        if (memcmp(&c->sp_rho[i], &rho[i], sizeof(double)) != 0) return 0;
    return 1;
}

/* The two-loop passes as separate launches, over h pairs in ring order: s_{h-1}.g unless sg_ref
 * (>= 0) names it among the previous commit's reductions, the first loop down to k_mid, the second
 * loop up to its last update, which is left to the commit (or k_last; last_update).
 * q and r are updated in place as far as the driver is concerned. The device layer keeps the two
 * ends of each vector in place - the tail the alternating walk re-reads from the Infinity Cache -
 * and ping-pongs the segments between them through an alternate buffer of its own
 * (LBFGS_WORK_SPLIT, DESIGN.md §4 "Split work vector"). A ping-pong of the whole vectors measured
 * neutral at 1e8 and -8 % at 1e7: it gives up the cached ends. */
static int twoloop_passes(lbfgs_ctx* c, int h, const double* rho, const double* const* Sr,
                          const double* const* Yr, double gamma, int sg_ref) {
    const int m = c->m;
    int refA[MMAX], refB[MMAX];
    if (sg_ref >= 0) {
        refA[h - 1] = sg_ref; /* s_{h-1}.g from the previous commit */
    } else {
        DEV(lbk_dot(c->dev, Sr[h - 1], c->g, SLOT_P0));
        refA[h - 1] = REF(SLOT_P0, 0);
    }
    const double* qsrc = c->g;
    for (int i = h - 2; i >= 0; --i) {
        DEV(lbk_axpy_dot(c->dev, c->q, qsrc, Yr[i + 1], Sr[i], rho[i + 1], refA[i + 1], SLOT_A0 + i));
        refA[i] = REF(SLOT_A0 + i, 0);
        qsrc = c->q;
    }
    DEV(lbk_mid(c->dev, c->r, qsrc, Yr[0], rho[0], gamma, refA[0], SLOT_B0(m)));
    refB[0] = REF(SLOT_B0(m), 0);
    for (int i = 0; i + 1 < h; ++i) {
        DEV(lbk_axpy2_dot(c->dev, c->r, c->r, Sr[i], Yr[i + 1], rho[i], refB[i], refA[i], SLOT_B0(m) + i + 1));
        refB[i + 1] = REF(SLOT_B0(m) + i + 1, 0);
    }
    return 0;
}

/* the record of the second loop's last update, d = -(r + s_{h-1} (alpha_{h-1} - beta_{h-1})), which
 * the commit, a trial pass or k_last forms: the same slots whichever form ran the passes before it
 * (alpha_{h-1} = s_{h-1}.g: sg_ref, or SLOT_P0 where the passes reduced it themselves) */
static void last_update(lbfgs_ctx* c, int h, double rho, int sg_ref) {
    c->rc = c->r;
    c->rho_last = rho;
    c->ref_b_last = REF(SLOT_B0(c->m) + h - 1, 0);
    c->ref_a_last = sg_ref >= 0 ? sg_ref : REF(SLOT_P0, 0);
    c->s_last_pair = c->ring[h - 1];
}

static int iterate(lbfgs_ctx* c) {
    const int k = c->k, m = c->m, h = c->h;
    int rc = iterate_top(c);
    if (rc == 1) {
        rc = spec_drop(c);
        return rc ? rc : 1;
    }
    if (rc) return rc;

    /* ---- search direction (:87-143) ---- */
    int dmode = LBK_D_NEG_G;
    int small_done = 0;
    const int small = !ext_obj(c) && !c->unfused && c->geo->world == 1 && lbk_small_ok(c->dev, h);
    c->cur_epoch = 0;
    c->cur_spec = 0;
    c->d_ready = 0;
    c->sr.have_spec = 0;
    c->sr.have_cand = 0;
    c->sr.tc_n = 0;
    if (c->tl_search && c->trial_passes > 0) c->many_passes = c->trial_passes >= 3;
    c->tl_search = 0;
    c->trial_passes = 0;
    host_invalidate(c);
    c->hxx_valid = 0;
    if (!(k == 0 || h == 0)) {
        int bad_rho = 0;
        for (int i = h - 1; i >= 0; --i)
            if (!isfinite(1.0 / c->sy[c->ring[i]])) bad_rho = 1; /* :102-108 */
        double gamma = 0.0;
        if (bad_rho) {
            say(c, "Warning: Invalid rho at iteration %d\n", k);
        } else {
            const int top = c->ring[h - 1];
            gamma = c->sy[top] / c->yy[top]; /* :117-118 */
            if (gamma <= 0 || !isfinite(gamma)) {
                say(c, "Warning: Invalid gamma at iteration %d\n", k);
            } else {
                dmode = LBK_D_TWOLOOP;
            }
        }
        if (dmode == LBK_D_TWOLOOP) {
            double rho[MMAX];
            const double* Sr[MMAX];
            const double* Yr[MMAX];
            const int p0_ref = c->sg_valid ? c->sg_ref : -1; /* s_{h-1}.g from the previous commit */
            ring_view(c, c->ring, h, rho, Sr, Yr);
            if (c->unfused) {
                rc = twoloop_unfused(c, rho, gamma);
                if (rc) return rc;
                dmode = LBK_D_BUF;
            } else {
                if (small) {
                    /* one single-workgroup launch: the passes of twoloop_passes and the commit at a0 */
                    c->cur_rho = rho[h - 1];
                    c->cur_gamma = gamma;
                    c->cur_p0 = p0_ref;
                    if (spec_matches(c, h, rho, p0_ref)) { /* already queued behind the last iteration */
                        c->sp_pend = 0;
                        c->cur_epoch = c->sp_epoch;
                        c->cur_spec = 1;
                    } else {
                        rc = spec_drop(c);
                        if (rc) return rc;
                        rc = small_launch(c, rho, Sr, Yr, gamma, p0_ref);
                        if (rc) return rc;
                    }
                    /* the next iteration, queued before this one's results are read */
                    rc = spec_next(c, 0.0);
                    if (rc) return rc;
                    small_done = 1;
                } else if (!ext_obj(c) && c->geo->world == 1 && lbk_twoloop_ok(c->dev, h)) {
                    /* LBFGS_PERSIST=2: the passes of twoloop_passes in one persistent launch, same slots */
                    DEV(lbk_twoloop_persist(c->dev, h, c->g, c->q, c->r, Sr, Yr, rho, gamma, p0_ref, SLOT_P0, SLOT_A0,
                                            SLOT_B0(m)));
                } else {
                    rc = twoloop_passes(c, h, rho, Sr, Yr, gamma, p0_ref);
                    if (rc) return rc;
                }
                last_update(c, h, rho[h - 1], p0_ref);
            }
        }
    }
    if (c->sp_pend && c->sp_k == k) { /* queued for this iteration, which took another path */
        rc = spec_drop(c);
        if (rc) return rc;
    }
    c->dmode = dmode;
    if (c->unfused && dmode == LBK_D_BUF) c->d_ready = 1;

    /* ---- descent check (:146-153) and the line search (:156) ---- */
    const int cslot = SLOT_COMMIT0 + (k & 1);
    double tot[LBK_KMAX];
    double gd;
    c->a0 = c->K.initial_step;
    const int sharded = c->geo->world > 1;
    if (!ext_obj(c) && !c->unfused) {
        /* last two-loop pass + first trial at a0 + commit fused in one pass. Sharded, the
         * stencil's halo of d at the rank edges comes from the neighbours' edge r (published
         * with the last second-loop pass's reduction) and s_{h-1}'s ghost cells; d = -g is
         * materialised first so that its edge values reach the neighbours through its slot. */
        if (sharded && c->dmode == LBK_D_TWOLOOP) {
            lbk_set_ghost_slot(c->dev, SLOT_B0(m) + h - 1);
        } else if (sharded) {
            rc = materialize_d(c);
            if (rc) return rc;
        }
        const double cand = first_cand(c); /* a0 is the initial step */
        if (small_done) { /* the commit at a0 ran inside lbk_small_iter */
            rc = small_fetch(c, cslot, tot);
            if (rc) return rc;
            c->commits++;
            if (cand > 0.0) {
                c->sr.have_cand = 1;
                c->sr.cand_a = cand;
                c->sr.cand_f = tot[LBK_C_FC];
            }
        } else {
            rc = commit(c, c->dmode, c->a0, cslot, tot, cand);
            if (rc) return rc;
        }
        gd = tot[LBK_C_GD];
        if (gd >= 0) {
            say(c, "Warning: Not a descent direction, using gradient\n");
            c->dmode = dmode = LBK_D_NEG_G;
            c->d_ready = 0;
            if (sharded) {
                rc = materialize_d(c);
                if (rc) return rc;
            }
            rc = commit(c, c->dmode, c->a0, cslot, tot, cand);
            if (rc) return rc;
            gd = tot[LBK_C_GD];
        }
        c->sr.have_spec = 1;
        c->sr.spec_a = c->a0;
        c->sr.spec_f = tot[LBK_C_F];
        c->sr.spec_dphi = tot[LBK_C_DPHI];
        memcpy(c->spec_tot, tot, sizeof tot);
    } else {
        rc = materialize_d(c);
        if (rc) return rc;
        DEVNC(lbk_fetch(c->dev, SLOT_LAST(m), 1, &gd));
        if (gd >= 0) {
            say(c, "Warning: Not a descent direction, using gradient\n");
            c->dmode = LBK_D_NEG_G;
            c->d_ready = 0;
            host_invalidate(c);
            rc = materialize_d(c);
            if (rc) return rc;
            DEVNC(lbk_fetch(c->dev, SLOT_LAST(m), 1, &gd));
        }
    }

    double alpha = 0.0;
    c->search_cslot = (!ext_obj(c) && !c->unfused) ? cslot : -1; /* a device search may commit */
    c->search_committed = 0;
    c->recommit_a0 = 0;
    rc = run_line_search(c, gd, &alpha);
    c->search_cslot = -1;
    if (rc) return rc;
    if (c->flags & LBFGS_FLAG_TRACE) c->tr_a[c->tr_len - 1] = alpha;

    /* ---- commit (:159-198) ---- */
    if (c->search_committed) {
        /* the device search's launch committed at its step already (the commit below, D_BUF):
         * its totals, then iteration k + 1 queued behind it as commit_queued would */
        if (small_done && c->spec_on) {
            rc = spec_drop(c);
            if (rc) return rc;
        }
        DEVNC(lbk_fetch(c->dev, cslot, 7, tot));
        c->commits++;
        if (small_done && c->spec_on && alpha >= 1e-10) {
            rc = spec_next(c, alpha);
            if (rc) return rc;
        }
    } else if (!(c->sr.have_spec && alpha == c->a0) || c->recommit_a0) {
        /* batched: d may still be unmaterialised (formed on the fly again, same bits) */
        if (!(c->batch && !c->unfused && !ext_obj(c) && !c->d_ready &&
              (c->dmode == LBK_D_TWOLOOP || (c->dmode == LBK_D_NEG_G && c->geo->world == 1)))) {
            rc = materialize_d(c);
            if (rc) return rc;
        }
        if (small_done && c->spec_on) { /* the next iteration queued behind the recommit */
            rc = spec_drop(c);
            if (!rc) rc = commit_queued(c, c->d_ready ? LBK_D_BUF : c->dmode, alpha, cslot, tot);
        } else {
            rc = commit(c, c->d_ready ? LBK_D_BUF : c->dmode, alpha, cslot, tot, 0.0);
        }
        if (rc) return rc;
    }
    c->f_cur = tot[LBK_C_F];
    c->sp_hostgo = alpha == c->sp_alpha && tot[LBK_C_SY] > 0; /* what a queued launch of k + 1 assumed */
    if (alpha < 1e-10) { /* :164-168 */
        say(c, "Warning: Line search failed at iteration %d\n", k);
        c->status = LBFGS_STATUS_LS_FAILED;
        return 1;
    }
    const double sy = tot[LBK_C_SY];
    if (sy > 0) { /* :182-191 */
        c->sy[c->free_pair] = sy;
        c->yy[c->free_pair] = tot[LBK_C_YY];
        ring_push(m, c->ring, &c->h, &c->free_pair);
        c->sg_valid = !c->unfused;
        c->sg_ref = REF(cslot, LBK_C_SG);
    } else {
        say(c, "Warning: Skipping update, sy = %g\n", sy); /* :192-195 */
        c->sg_valid = 0;
    }
    swap_iterates(c);
    c->gg = tot[LBK_C_GG];
    c->k++;
    return 0;
}


/* ------------------------------------------------------------------------------------------
 * Vector-free mode (LBFGS_FLAG_VECTOR_FREE; outside the bit-parity contract with the
 * reference's operation order). lbfgs.cpp:87-143's two-loop recursion runs
 * on the host over the Gram matrix of the basis [s_0..s_{h-1}, y_0..y_{h-1}, g] (q and r are
 * coefficient vectors); one device pass forms d from the basis, takes the first trial and the
 * commit, and reduces g_new and y_new against the basis. The s_new row is derived,
 * s_new . v = alpha (d . v). Every sum below runs over s terms (ring order), then y terms, then
 * the g term, starting from 0.0 (oracle/lbfgs_oracle.c restates it in the same order).
 * ---------------------------------------------------------------------------------------- */
#define GI(c, p, q) ((p) * ((c)->m + 1) + (q))

/* coefficient vector (ds, dy, dg) dotted with basis vector s_{ring i} or y_{ring i} */
static double vf_dot_s(const lbfgs_ctx* c, int i, const double* ds, const double* dy, double dg) {
    const int ri = c->ring[i];
    double a = 0.0;
    for (int j = 0; j < c->h; ++j) a = a + ds[j] * c->Gss[GI(c, ri, c->ring[j])];
    for (int j = 0; j < c->h; ++j) a = a + dy[j] * c->Gsy[GI(c, ri, c->ring[j])];
    return a + dg * c->Gsg[ri];
}
static double vf_dot_y(const lbfgs_ctx* c, int i, const double* ds, const double* dy, double dg) {
    const int ri = c->ring[i];
    double a = 0.0;
    for (int j = 0; j < c->h; ++j) a = a + ds[j] * c->Gsy[GI(c, c->ring[j], ri)];
    for (int j = 0; j < c->h; ++j) a = a + dy[j] * c->Gyy[GI(c, ri, c->ring[j])];
    return a + dg * c->Gyg[ri];
}

static int vf_commit(lbfgs_ctx* c, double alpha, double* tot) {
    int hb = 0;
    DEV(lbk_vf_commit(c->dev, c->obj, c->vf_h, c->x, c->g, c->vf_S, c->vf_Y, c->vf_cs, c->vf_cy, c->vf_cg, alpha,
                      c->vf_cand, c->xn, c->gn, c->S[c->free_pair], c->Y[c->free_pair], LBK_WSLOT0, &hb));
    DEVNC(lbk_fetch(c->dev, LBK_WSLOT0, LBK_VF_YB + 4 * hb + LBK_VF_NA, tot));
    c->vf_hb = hb;
    c->commits++;
    return 0;
}

/* the direction's coefficients (vf_cs, vf_cy, vf_cg) against a row of the basis' products with some
 * vector v: sum_j cs_j (s_j.v), then sum_j cy_j (y_j.v), then cg (g.v), in that order from 0.0 */
static double vf_combine(const lbfgs_ctx* c, const double* rowS, const double* rowY, double gval) {
    double a = 0.0;
    for (int j = 0; j < c->vf_h; ++j) a = a + c->vf_cs[j] * rowS[j];
    for (int j = 0; j < c->vf_h; ++j) a = a + c->vf_cy[j] * rowY[j];
    return a + c->vf_cg * gval;
}

static int iterate_vf(lbfgs_ctx* c) {
    const int k = c->k, m = c->m, h = c->h;
    int rc = iterate_top(c);
    if (rc) return rc;

    /* ---- direction in coefficient space (:87-143): d = -(r) with r over the basis ---- */
    c->vf_h = h;
    ring_view(c, c->ring, h, NULL, c->vf_S, c->vf_Y);
    for (int j = 0; j < h; ++j) c->vf_cs[j] = c->vf_cy[j] = 0.0;
    c->vf_cg = -1.0;
    if (!(k == 0 || h == 0)) {
        int bad_rho = 0;
        for (int i = h - 1; i >= 0; --i)
            if (!isfinite(1.0 / c->Gsy[GI(c, c->ring[i], c->ring[i])])) bad_rho = 1;
        const int top = c->ring[h - 1];
        if (bad_rho) {
            say(c, "Warning: Invalid rho at iteration %d\n", k);
        } else {
            const double gamma = c->Gsy[GI(c, top, top)] / c->Gyy[GI(c, top, top)];
            if (gamma <= 0 || !isfinite(gamma)) {
                say(c, "Warning: Invalid gamma at iteration %d\n", k);
            } else {
                double ds[MMAX], dy[MMAX], a[MMAX], dg = 1.0;
                for (int j = 0; j < h; ++j) ds[j] = dy[j] = 0.0;
                for (int i = h - 1; i >= 0; --i) {
                    const double rho = 1.0 / c->Gsy[GI(c, c->ring[i], c->ring[i])];
                    a[i] = rho * vf_dot_s(c, i, ds, dy, dg);
                    dy[i] = dy[i] - a[i];
                }
                for (int j = 0; j < h; ++j) {
                    ds[j] = ds[j] * gamma;
                    dy[j] = dy[j] * gamma;
                }
                dg = dg * gamma;
                for (int i = 0; i < h; ++i) {
                    const double rho = 1.0 / c->Gsy[GI(c, c->ring[i], c->ring[i])];
                    const double beta = rho * vf_dot_y(c, i, ds, dy, dg);
                    ds[i] = ds[i] + (a[i] - beta);
                }
                for (int j = 0; j < h; ++j) {
                    c->vf_cs[j] = -ds[j];
                    c->vf_cy[j] = -dy[j];
                }
                c->vf_cg = -dg;
            }
        }
    }
    /* g . d from the Gram row of g, in ring order */
    double sg[MMAX], yg[MMAX];
    for (int j = 0; j < h; ++j) {
        sg[j] = c->Gsg[c->ring[j]];
        yg[j] = c->Gyg[c->ring[j]];
    }
    double gd = vf_combine(c, sg, yg, c->gg);
    if (gd >= 0) { /* :146-153 */
        say(c, "Warning: Not a descent direction, using gradient\n");
        for (int j = 0; j < h; ++j) c->vf_cs[j] = c->vf_cy[j] = 0.0;
        c->vf_cg = -1.0;
        gd = vf_combine(c, sg, yg, c->gg);
    }
    c->dmode = D_VF;
    c->d_ready = 0;
    c->sr.have_cand = 0;
    c->sr.tc_n = 0;
    c->trial_passes = 0;
    c->gt_valid = 0;

    /* ---- fused first trial + commit at a0, then the line search (:156) ---- */
    c->a0 = c->K.initial_step;
    c->vf_cand[0] = c->a0 * c->K.backtracking_alpha; /* the steps line_search.cpp:27 would try next */
    for (int j = 1; j < LBK_VF_NA; ++j) c->vf_cand[j] = c->vf_cand[j - 1] * c->K.backtracking_alpha;
    c->vf_cand_valid = 0;
    rc = vf_commit(c, c->a0, c->vf_spec);
    if (rc) return rc;
    const double* T = c->vf_spec;
    const int gb = LBK_VF_YB + 2 * c->vf_hb; /* g_new . b_l components */
    for (int j = 0; j < LBK_VF_NA; ++j) c->vf_cand_f[j] = T[LBK_VF_YB + 4 * c->vf_hb + j];
    c->vf_cand_valid = 1;
    double dgn = vf_combine(c, &T[gb], &T[gb + h], T[LBK_VF_GGO]); /* g_new . d */
    c->sr.have_spec = 1;
    c->sr.spec_a = c->a0;
    c->sr.spec_f = T[LBK_VF_F];
    c->sr.spec_dphi = dgn;

    double alpha = 0.0;
    rc = run_line_search(c, gd, &alpha);
    if (rc) return rc;
    if (c->flags & LBFGS_FLAG_TRACE) c->tr_a[c->tr_len - 1] = alpha;

    /* ---- commit (:159-198) ---- */
    if (alpha == c->a0) {
        memcpy(c->vf_tot, c->vf_spec, sizeof c->vf_tot);
    } else {
        rc = vf_commit(c, alpha, c->vf_tot);
        if (rc) return rc;
        T = c->vf_tot;
        dgn = vf_combine(c, &T[gb], &T[gb + h], T[LBK_VF_GGO]);
    }
    T = c->vf_tot;
    c->f_cur = T[LBK_VF_F];
    if (alpha < 1e-10) { /* :164-168 */
        say(c, "Warning: Line search failed at iteration %d\n", k);
        c->status = LBFGS_STATUS_LS_FAILED;
        return 1;
    }
    const double sy = T[LBK_VF_SY];
    const int yb = LBK_VF_YB;
    if (sy > 0) { /* :182-191 */
        const int p = c->free_pair;
        /* derived row of s_new = alpha d against the old basis (old g row) */
        double dS[MMAX], dY[MMAX];
        for (int q = 0; q < h; ++q) {
            const int rq = c->ring[q];
            double a = 0.0, b = 0.0;
            for (int j = 0; j < h; ++j) a = a + c->vf_cs[j] * c->Gss[GI(c, c->ring[j], rq)];
            for (int j = 0; j < h; ++j) a = a + c->vf_cy[j] * c->Gsy[GI(c, rq, c->ring[j])];
            dS[q] = a + c->vf_cg * c->Gsg[rq];
            for (int j = 0; j < h; ++j) b = b + c->vf_cs[j] * c->Gsy[GI(c, c->ring[j], rq)];
            for (int j = 0; j < h; ++j) b = b + c->vf_cy[j] * c->Gyy[GI(c, c->ring[j], rq)];
            dY[q] = b + c->vf_cg * c->Gyg[rq];
        }
        const double dd = vf_combine(c, dS, dY, gd);
        for (int q = 0; q < h; ++q) {
            const int rq = c->ring[q];
            c->Gss[GI(c, p, rq)] = c->Gss[GI(c, rq, p)] = alpha * dS[q];
            c->Gsy[GI(c, p, rq)] = alpha * dY[q];
            c->Gsy[GI(c, rq, p)] = T[yb + q];
            c->Gyy[GI(c, p, rq)] = c->Gyy[GI(c, rq, p)] = T[yb + h + q];
            c->Gsg[rq] = T[gb + q];
            c->Gyg[rq] = T[gb + h + q];
        }
        c->Gss[GI(c, p, p)] = (alpha * alpha) * dd;
        c->Gsy[GI(c, p, p)] = sy;
        c->Gyy[GI(c, p, p)] = T[LBK_VF_YY];
        c->Gsg[p] = alpha * dgn;
        c->Gyg[p] = T[LBK_VF_YG];
        ring_push(m, c->ring, &c->h, &c->free_pair);
    } else {
        say(c, "Warning: Skipping update, sy = %g\n", sy); /* :192-195 */
        for (int q = 0; q < h; ++q) {
            c->Gsg[c->ring[q]] = T[gb + q];
            c->Gyg[c->ring[q]] = T[gb + h + q];
        }
    }
    swap_iterates(c);
    c->gg = T[LBK_VF_GG];
    c->k++;
    return 0;
}

/* ------------------------------------------------------------------------------------------ */
/* ------------------------------------------------------------------------------------------
 * LBFGS_FLAG_CUDA_COMPAT: LBFGS_CUDA of parallel-implementation/L-BFGS.cu:195-358 with the
 * line searches of parallel-implementation/line_search.cpp, on device vectors. The reference
 * reads every cuBLAS dot back to the host (host-pointer mode); so does this path (one fetch per
 * dot), and its line searches run on the host over device evaluations: f(x + a d) and
 * g(x + a d) . d by the trial kernel, f(x) by the objective kernel, g0 . d as a canonical dot.
 * ---------------------------------------------------------------------------------------- */
static int cu_dot(lbfgs_ctx* c, const double* a, const double* b, double* out) {
    DEV(lbk_dot(c->dev, a, b, SLOT_MISC(c->m)));
    DEVNC(lbk_fetch(c->dev, SLOT_MISC(c->m), 1, out));
    return 0;
}

static int cu_fx(lbfgs_ctx* c, double* f) { /* f(x): the objective kernel, its gradient into scratch */
    double t[2];
    DEV(lbk_eval(c->dev, c->obj, c->x, c->gt, SLOT_TRIAL(c->m)));
    DEVNC(lbk_fetch(c->dev, SLOT_TRIAL(c->m), 2, t));
    *f = t[0];
    c->trials_f++;
    return 0;
}

static int cu_ft(lbfgs_ctx* c, double a, double* f, double* gnd) { /* f(x + a d) [, g(x + a d) . d] */
    double t[2];
    DEV(lbk_trial(c->dev, c->obj, c->x, c->d, a, gnd ? c->gt : NULL, SLOT_TRIAL(c->m)));
    DEVNC(lbk_fetch(c->dev, SLOT_TRIAL(c->m), gnd ? 2 : 1, t));
    *f = t[0];
    if (gnd) {
        *gnd = t[1];
        c->trials_fg++;
    } else {
        c->trials_f++;
    }
    return 0;
}

#define CU(call)                    \
    do {                            \
        const int rc_ = (call);     \
        if (rc_) return rc_;        \
    } while (0)

static int cu_backtracking(lbfgs_ctx* c, double gd, double* out) { /* line_search.cpp:21-40 */
    const lbfgs_constants* K = &c->K;
    double fx, ft, alpha = K->initial_step;
    CU(cu_fx(c, &fx)); /* the reference re-evaluates f(x) per trial: the same value */
    for (;;) {
        CU(cu_ft(c, alpha, &ft, NULL));
        if (!(fx - ft < K->c1 * alpha * gd)) break;
        alpha *= K->backtracking_alpha;
        if (alpha < K->backtracking_tol) break;
    }
    *out = alpha < 1e-4 ? 0.5 : alpha;
    return 0;
}

static int cu_backtracking_wolfe(lbfgs_ctx* c, double gd, double* out) { /* :42-147, its own constants */
    const double C1 = 1e-4, C2 = 0.9, TOL = 1e-10;
    double alpha = 1.0, f_current, alpha_lo = 0.0, alpha_hi = DBL_MAX;
    double ca[24], cf[24]; /* the search's cache of f by alpha */
    int nc = 0, iter = 0;
    CU(cu_fx(c, &f_current));
    while (iter++ < 20) {
        int hit = -1;
        for (int j = 0; j < nc; ++j)
            if (ca[j] == alpha) hit = j;
        double f_new;
        if (hit >= 0) {
            f_new = cf[hit];
        } else {
            CU(cu_ft(c, alpha, &f_new, NULL));
            if (nc < 24) {
                ca[nc] = alpha;
                cf[nc++] = f_new;
            }
        }
        if (f_new <= f_current + C1 * alpha * gd) {
            double fg, gnd;
            CU(cu_ft(c, alpha, &fg, &gnd)); /* grad(x_new) . d */
            if (gnd >= C2 * gd) break;
            alpha_lo = alpha;
        } else {
            alpha_hi = alpha;
        }
        if (alpha_hi < DBL_MAX)
            alpha = (alpha_lo + alpha_hi) / 2.0;
        else
            alpha = 2.0 * alpha_lo;
        if (alpha < TOL) break;
    }
    *out = alpha;
    return 0;
}

/* The interpolation and Wolfe searches of L-BFGS.cu (line_search.cpp:149-213, :277-368) and of the
 * variant files (L-BFGS-Interpolation.cu:259-342, L-BFGS-Wolfe.cu:259-349) are one loop each. What
 * differs comes in and goes out: f_x, the f the tests compare against (a fresh f(x) pass in
 * L-BFGS.cu, cv_fhost in the variants); f0, the start of f_prev / f_lo (the same f_x, or the
 * variants' cv_f0); *f_last, the f of the last trial point (the variants' next cv_fhost); *ok, the
 * variants' line_search_success. */
static int cu_interpolation(lbfgs_ctx* c, double gd, double f_x, double f0, int floor_every_exit, double* out,
                            double* f_last, int* ok) {
    const lbfgs_constants* K = &c->K;
    double alpha = K->initial_step, alpha_prev = 0.0, f_prev = f0;
    int iter;
    *ok = 0;
    for (iter = 0; iter < 20; ++iter) {
        double f_new;
        CU(cu_ft(c, alpha, &f_new, NULL));
        *f_last = f_new;
        if (f_new <= f_x + K->c1 * alpha * gd) {
            *ok = 1;
            break;
        }
        if (alpha < K->wolfe_interp_min) {
            alpha = K->wolfe_interp_min;
            break;
        }
        if (alpha_prev > 0) {
            const double delta = alpha - alpha_prev;
            if (fabs(delta) < 1e-10) {
                alpha *= 0.5;
            } else {
                const double ga = (f_new - f_x - gd * alpha) / (alpha * alpha);
                alpha = lbk_search_cubic(alpha_prev, alpha, f_prev, gd, f_new, ga);
                if (alpha < 0.1 * alpha_prev || alpha > 0.9 * alpha_prev) alpha = alpha_prev * 0.5;
            }
        } else {
            alpha = lbk_search_quad(alpha, f_new, gd, f_x);
            if (alpha < 0.1 * K->initial_step || alpha > 0.9 * K->initial_step) alpha = K->initial_step * 0.5;
        }
        alpha_prev = alpha; /* after the update (L-BFGS-Interpolation.cu:335) */
        f_prev = f_new;
    }
    /* the floor: only after 20 trials in L-BFGS.cu's search, on every exit in the variant's (:339-342) */
    if ((iter == 20 || floor_every_exit) && alpha < 1e-4) alpha = 0.5;
    *out = alpha;
    return 0;
}

/* :216-275: endpoints sorted, the midpoint whenever a step is not finite or the cubic has no
 * real minimiser, the result kept 10 % inside the bracket */
static double cu_safe_cubic(double a0, double a1, double p0, double dp0, double p1, double dp1) {
    if (a0 > a1) {
        double t = a0;
        a0 = a1;
        a1 = t;
        t = p0;
        p0 = p1;
        p1 = t;
        t = dp0;
        dp0 = dp1;
        dp1 = t;
    }
    const double d1 = dp0 + dp1 - 3 * (p1 - p0) / (a1 - a0);
    if (isnan(d1) || isinf(d1)) return 0.5 * (a0 + a1);
    const double disc = d1 * d1 - dp0 * dp1;
    if (disc < 0) return 0.5 * (a0 + a1);
    const double d2 = copysign(sqrt(disc), a1 - a0);
    const double den = dp0 - dp1 + 2 * d2;
    if (fabs(den) < 1e-10) return 0.5 * (a0 + a1);
    const double r = a0 + (a1 - a0) * (dp0 + d2 - d1) / den;
    if (isnan(r) || isinf(r)) return 0.5 * (a0 + a1);
    const double lo = a0 + 0.1 * (a1 - a0), hi = a1 - 0.1 * (a1 - a0);
    const double mn = (r < hi) ? r : hi; /* std::min(hi, r) */
    return (lo < mn) ? mn : lo;          /* std::max(lo, .) */
}

static int cu_wolfe(lbfgs_ctx* c, double gd, double f_x, double f0, double* out, double* f_last, int* ok) {
    const lbfgs_constants* K = &c->K;
    double alpha = K->initial_step, alpha_lo = 0.0, alpha_hi = INFINITY, f_lo = f0, dphi_lo = gd;
    *ok = 0;
    for (int iter = 0; iter < 20; ++iter) {
        double f_new;
        CU(cu_ft(c, alpha, &f_new, NULL));
        *f_last = f_new;
        if (f_new > f_x + K->c1 * alpha * gd || (f_new >= f_lo && iter > 0)) {
            alpha_hi = alpha;
            alpha = cu_safe_cubic(alpha_lo, alpha_hi, f_lo, dphi_lo, f_new, (f_new - f_x - gd * alpha) / (alpha * alpha));
            continue; /* past the WOLFE_INTERP_MIN floor */
        }
        double fg, dphi_new;
        CU(cu_ft(c, alpha, &fg, &dphi_new)); /* grad(x_new) . d */
        if (fabs(dphi_new) <= -K->c2 * gd) {
            *ok = 1;
            break;
        }
        if (dphi_new >= 0) {
            alpha_hi = alpha;
            alpha = cu_safe_cubic(alpha_lo, alpha_hi, f_lo, dphi_lo, f_new, dphi_new);
        } else {
            alpha_lo = alpha;
            f_lo = f_new;
            dphi_lo = dphi_new;
            if (alpha_hi == INFINITY)
                alpha *= 2;
            else
                alpha = cu_safe_cubic(alpha_lo, alpha_hi, f_lo, dphi_lo, f_new, dphi_new);
        }
        if (alpha < K->wolfe_interp_min) {
            alpha = K->wolfe_interp_min;
            break;
        }
    }
    *out = alpha;
    return 0;
}

/* ------------------------------------------------------------------------------------------
 * LBFGS_FLAG_CUDA_VARIANT: the inline searches of the four variant files. Each trial transfers
 * x + a d to the host copy x_host, so f(x_host) at the next iteration is the f of the last trial
 * point transferred (cv_fhost), not f(x). ok = the search's line_search_success. Interpolation
 * and Wolfe are the loops above; the two backtracking searches are the files' own.
 * ---------------------------------------------------------------------------------------- */
static int cv_backtracking(lbfgs_ctx* c, double gd, double* out) { /* L-BFGS-Backtracking.cu:293-341 */
    const double C1 = 1e-4, TOL = 1e-10; /* :153-156, the file's own constants */
    double fx, ft, step = 1.0;
    CU(cu_fx(c, &fx)); /* f(x_host), x_host freshly copied from d_x */
    for (;;) {
        CU(cu_ft(c, step, &ft, NULL));
        if (ft <= fx + C1 * step * gd) break;
        step *= 0.5;
        if (step < TOL) {
            step = 0.5;
            break;
        }
    }
    *out = step;
    return 0;
}

static int cv_backtracking_wolfe(lbfgs_ctx* c, double gd, double* out, int* ok) { /* L-BFGS-Backtracking_Wolfe.cu:256-397 */
    const double C1 = 1e-4, C2 = 0.9, TOL = 1e-10; /* :261-264, the file's own constants */
    const double f_x = c->cv_fhost;
    double alpha = 1.0, alpha_lo = 0.0, alpha_hi = DBL_MAX;
    double ca[24], cf[24], cgd[24]; /* cache: f by alpha, and g(x + alpha d) . d once evaluated */
    int cg[24], nc = 0;
    *ok = 0;
    for (int iter = 0; iter < 20; ++iter) {
        int hit = -1;
        for (int j = 0; j < nc; ++j)
            if (ca[j] == alpha) hit = j;
        if (hit < 0) {
            double f_new;
            CU(cu_ft(c, alpha, &f_new, NULL));
            c->cv_fhost = f_new;
            hit = nc++;
            ca[hit] = alpha;
            cf[hit] = f_new;
            cg[hit] = 0;
        }
        if (cf[hit] <= f_x + C1 * alpha * gd) {
            if (!cg[hit]) { /* x + alpha d transferred again, its gradient evaluated */
                double fg;
                c->cv_fhost = cf[hit];
                CU(cu_ft(c, alpha, &fg, &cgd[hit]));
                cg[hit] = 1;
            }
            if (cgd[hit] >= C2 * gd) {
                *ok = 1;
                break;
            }
            alpha_lo = alpha;
        } else {
            alpha_hi = alpha;
        }
        if (alpha_hi < DBL_MAX)
            alpha = (alpha_lo + alpha_hi) / 2.0;
        else
            alpha = 2.0 * alpha_lo;
        if (alpha < TOL) {
            double f_t;
            alpha = TOL;
            CU(cu_ft(c, alpha, &f_t, NULL));
            c->cv_fhost = f_t;
            break;
        }
    }
    *out = alpha;
    return 0;
}

/* one iteration k of L-BFGS.cu:195-358; returns 1 when the solve ended */
static int iterate_cuda(lbfgs_ctx* c) {
    const int k = c->k, m = c->m;
    if (k == 0) {
        DEV(lbk_elementwise(c->dev, 2, c->d, c->g, NULL, 0.0)); /* negateVector :208 */
    } else {
        DEVNC(lbk_copy(c->dev, c->q, c->g)); /* :212 */
        const int lo = k - m > 0 ? k - m : 0;
        for (int i = k - 1; i >= lo; --i) { /* :216-235 */
            const int sl = i % m;
            if (c->sy[sl] <= 1e-10) continue; /* alpha[sl], rho[sl] keep their last values */
            c->cu_rho[sl] = 1.0 / c->sy[sl];
            double sq;
            CU(cu_dot(c, c->S[sl], c->q, &sq));
            c->cu_alpha[sl] = c->cu_rho[sl] * sq;
            DEV(lbk_elementwise(c->dev, 3, c->q, c->q, c->Y[sl], -c->cu_alpha[sl])); /* daxpy */
        }
        const int last = (k - 1) % m; /* :237-262 */
        const double ys = c->sy[last], yy = c->yy[last];
        const double gamma = (yy > 0 && ys > 1e-10) ? ys / yy : 1.0;
        DEV(lbk_elementwise(c->dev, 0, c->r, c->q, NULL, gamma)); /* scaleByRho */
        for (int i = lo; i < k; ++i) { /* :264-274 */
            const int sl = i % m;
            double yr;
            CU(cu_dot(c, c->Y[sl], c->r, &yr));
            const double beta = c->cu_rho[sl] * yr;
            const double diff = c->cu_alpha[sl] - beta;
            DEV(lbk_elementwise(c->dev, 3, c->r, c->r, c->S[sl], diff));
        }
        DEV(lbk_elementwise(c->dev, 2, c->d, c->r, NULL, 0.0)); /* :276 */
    }
    double gd, step;
    if (c->cuda == 2) { /* the variants: the current gradient (d_g), their own searches */
        int ok = 1;
        CU(cu_dot(c, c->g, c->d, &gd));
        switch (c->ls) {
            case LBFGS_LS_BACKTRACKING: CU(cv_backtracking(c, gd, &step)); break;
            case LBFGS_LS_INTERPOLATION:
                CU(cu_interpolation(c, gd, c->cv_fhost, c->cv_f0, 1, &step, &c->cv_fhost, &ok));
                break;
            case LBFGS_LS_WOLFE: CU(cu_wolfe(c, gd, c->cv_fhost, c->cv_f0, &step, &c->cv_fhost, &ok)); break;
            default: CU(cv_backtracking_wolfe(c, gd, &step, &ok)); break;
        }
        say(c, "alpha: %g\n", step);
        if (c->ls == LBFGS_LS_BACKTRACKING) {
            if (step < 1e-4) /* L-BFGS-Backtracking.cu:345-348 */
                say(c, "Warning: Line search resulted in very small step size at iteration %d\n", k);
        } else if (!ok && step < 1e-10) { /* e.g. L-BFGS-Wolfe.cu:353-366 */
            say(c, "Warning: Line search failed at iteration %d\n", k);
            c->status = LBFGS_STATUS_LS_FAILED;
            return 1;
        }
    } else { /* the line search with the iteration-0 gradient (:199, :293) */
        double fx, f_last; /* f(x): a pass of its own; the last trial's f and ok are the variants' */
        int ok;
        CU(cu_dot(c, c->g0c, c->d, &gd));
        switch (c->ls) {
            case LBFGS_LS_BACKTRACKING: CU(cu_backtracking(c, gd, &step)); break;
            case LBFGS_LS_INTERPOLATION:
                CU(cu_fx(c, &fx));
                CU(cu_interpolation(c, gd, fx, fx, 0, &step, &f_last, &ok));
                break;
            case LBFGS_LS_WOLFE:
                CU(cu_fx(c, &fx));
                CU(cu_wolfe(c, gd, fx, fx, &step, &f_last, &ok));
                break;
            default: CU(cu_backtracking_wolfe(c, gd, &step)); break;
        }
        if (step < 1e-10) { /* :295-306 */
            say(c, "Warning: Line search failed at iteration %d\n", k);
            c->status = LBFGS_STATUS_LS_FAILED;
            return 1;
        }
        say(c, "alpha: %g\n", step); /* :308 */
    }
    DEV(lbk_point(c->dev, c->xn, c->x, c->d, step)); /* updateSolution :310 */
    double t[2];
    DEV(lbk_eval(c->dev, c->obj, c->xn, c->gn, SLOT_COMMIT0)); /* grad(x_new) :323, f(x_new) :348 */
    DEVNC(lbk_fetch(c->dev, SLOT_COMMIT0, 2, t));
    const int sl = k % m; /* updateVectors :332, whatever s.y */
    DEV(lbk_elementwise(c->dev, 3, c->S[sl], c->xn, c->x, -1.0));
    DEV(lbk_elementwise(c->dev, 3, c->Y[sl], c->gn, c->g, -1.0));
    CU(cu_dot(c, c->S[sl], c->Y[sl], &c->sy[sl])); /* the next iteration's ddot(s, y) and ddot(y, y) */
    CU(cu_dot(c, c->Y[sl], c->Y[sl], &c->yy[sl]));
    swap_iterates(c); /* :335-340 */
    c->commits++;
    c->f_cur = t[0];
    c->gg = t[1];
    const double norm_g = sqrt(t[1]); /* :342-345 */
    say(c, "Iteration %d: norm_g = %g\n", k, norm_g);
    say(c, "Optimum value: %g\n", t[0]);
    if (c->flags & LBFGS_FLAG_TRACE) {
        CU(trace_push(c, t[0], norm_g, 1));
        c->tr_a[c->tr_len - 1] = step;
    }
    note_h(c, k + 1 < m ? k + 1 : m); /* ring slots written */
    c->k++;
    if (norm_g <= c->tol) { /* :353-357 */
        say(c, "Convergence achieved at iteration %d\n", k);
        c->status = LBFGS_STATUS_CONVERGED;
        return 1;
    }
    return 0;
}
#undef CU

/* Caller-owned device buffers (the _device entry points): n doubles, unpadded, 8-byte aligned. The
 * streaming passes assume lbk_vec_alloc's layout (ghost cells, zeroed padding, 16-byte rows) and are
 * never launched on one; a buffer is copied to or from a solver vector by one pass of the
 * elementwise kernel on the solver stream, which reads and writes exactly [0, n) (op 0 with
 * alpha = 1.0 keeps every double value). */
static int import_device(lbfgs_ctx* c, double* dst, const double* src_dev) {
    DEV(lbk_elementwise(c->dev, 0, dst, src_dev, NULL, 1.0));
    return 0;
}

static int export_device(lbfgs_ctx* c, double* dst_dev, const double* src) {
    DEV(lbk_elementwise(c->dev, 0, dst_dev, src, NULL, 1.0));
    DEVNC(lbk_sync(c->dev)); /* complete on return */
    return 0;
}

/* an on/off environment switch: unset = dflt, else its integer value != 0 */
static int env_switch(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) != 0 : dflt;
}

/* the line-search constants of a solve or a standalone search: the caller's, or the defaults */
static void set_constants(lbfgs_ctx* c, const lbfgs_constants* k) {
    if (k)
        c->K = *k;
    else
        lbfgs_constants_default(&c->K);
}

/* x0_dev != 0: x0 is a caller-owned device buffer (lbfgs_solver_init_device) */
static int solver_init_at(lbfgs_ctx* c, int objective, const lbfgs_host_fn* cb, int line_search,
                          const lbfgs_constants* k, const double* x0, int x0_dev, double tolerance,
                          unsigned flags) {
    if (!c || !x0) return LBFGS_ERR_BAD_ARG;
    if (objective < 0 || objective > LBFGS_OBJ_DEVICE) return LBFGS_ERR_BAD_ARG;
    if (line_search < 0 || line_search > LBFGS_LS_BACKTRACKING_WOLFE) return LBFGS_ERR_BAD_ARG;
    if (x0_dev && c->geo->world != 1) return LBFGS_ERR_BAD_ARG;
    if (objective == LBFGS_OBJ_DENSE_QUAD && !c->dense_set) return LBFGS_ERR_STATE;
    if (objective == LBFGS_OBJ_DEVICE) { /* one rank, the default driver path only */
        if (!c->dcb.eval || c->geo->world != 1) return LBFGS_ERR_BAD_ARG;
        if (flags & (LBFGS_FLAG_UNFUSED | LBFGS_FLAG_VECTOR_FREE | LBFGS_FLAG_REFERENCE_CALLS | LBFGS_FLAG_CUDA_COMPAT))
            return LBFGS_ERR_BAD_ARG;
    }
    c->refcalls = (flags & LBFGS_FLAG_REFERENCE_CALLS) != 0;
    if (objective == LBFGS_OBJ_HOST) {
        if (!cb || !cb->f || !cb->grad || c->geo->world != 1) return LBFGS_ERR_BAD_ARG;
        c->cb = *cb;
        if (host_bufs(c)) return LBFGS_ERR_NOMEM;
    }
    host_invalidate(c);
    c->hxx_valid = 0;
    c->cb_f = c->cb_g = 0;
    {
        const int rc = spec_drop(c);
        if (rc) return rc;
    }
    /* speculative next iteration at small n (LBFGS_SPEC=0: off; the same iterates either way) */
    c->spec_on = env_switch("LBFGS_SPEC", 1);
    c->cur_epoch = 0;
    c->cur_spec = 0;
    c->sp_adopted = c->sp_dropped = 0;
    c->search_launches = c->search_commits = 0;
    c->unfused = (flags & LBFGS_FLAG_UNFUSED) != 0;
    c->many_passes = c->tl_search = 0;
    c->batch = env_switch("LBFGS_BATCH", 1);
    if (c->unfused && (objective >= LBFGS_OBJ_HOST || c->geo->world != 1)) return LBFGS_ERR_BAD_ARG;
    c->vf = (flags & LBFGS_FLAG_VECTOR_FREE) != 0;
    if (c->vf) {
        if (c->unfused || objective >= LBFGS_OBJ_HOST || c->m > LBK_VF_HMAX) return LBFGS_ERR_BAD_ARG;
        const size_t P = (size_t)c->m + 1;
        if (!c->Gss) {
            c->Gss = (double*)calloc(P * P, sizeof(double));
            c->Gsy = (double*)calloc(P * P, sizeof(double));
            c->Gyy = (double*)calloc(P * P, sizeof(double));
            c->Gsg = (double*)calloc(P, sizeof(double));
            c->Gyg = (double*)calloc(P, sizeof(double));
            if (!c->Gss || !c->Gsy || !c->Gyy || !c->Gsg || !c->Gyg) return LBFGS_ERR_NOMEM;
        }
    }
    c->cuda = (flags & LBFGS_FLAG_CUDA_COMPAT) != 0;
    if ((flags & LBFGS_FLAG_CUDA_VARIANT) && !c->cuda) return LBFGS_ERR_BAD_ARG;
    if (c->cuda && (flags & LBFGS_FLAG_CUDA_VARIANT)) c->cuda = 2;
    if (c->cuda) {
        if (c->unfused || c->vf || objective >= LBFGS_OBJ_HOST || c->geo->world != 1) return LBFGS_ERR_BAD_ARG;
        if (!c->g0c && !(c->g0c = lbk_vec_alloc(c->dev))) return LBFGS_ERR_NOMEM;
        memset(c->cu_alpha, 0, sizeof c->cu_alpha); /* L-BFGS.cu:191-192: vector<double> alpha(m), rho(m) */
        memset(c->cu_rho, 0, sizeof c->cu_rho);
    }
    c->obj = objective;
    c->ls = line_search;
    set_constants(c, k);
    c->tol = tolerance;
    c->flags = flags;
    c->k = 0;
    c->h = 0;
    c->free_pair = 0;
    c->sg_valid = 0;
    c->status = LBFGS_STATUS_RUNNING;
    c->finished = 0;
    c->msg_len = 0;
    if (c->msg) c->msg[0] = 0;
    c->tr_len = 0;
    c->trials_f = c->trials_fg = c->commits = c->passes = 0;

    const double* x0_host = x0;
    if (x0_dev) { /* x = x0 */
        const int rc = import_device(c, c->x, x0);
        if (rc) return rc;
        if (objective == LBFGS_OBJ_HOST) { /* the callbacks read x0 from the pinned point buffer */
            DEVNC(lbk_download_local(c->dev, c->hx, c->x));
            x0_host = c->hx;
        }
    } else {
        DEVNC(lbk_upload(c->dev, c->x, x0));
    }
    if (objective == LBFGS_OBJ_DEVICE) {
        const int rc = device_eval(c, c->x, &c->f_cur, c->g);
        if (rc) return rc;
        DEV(lbk_dot(c->dev, c->g, c->g, SLOT_INIT));
        DEVNC(lbk_fetch(c->dev, SLOT_INIT, 1, &c->gg));
    } else if (objective == LBFGS_OBJ_HOST) {  /* :29-30 */
        c->f_cur = c->cb.f(x0_host, c->n, c->cb.user);
        const int b = c->hg_cur;
        c->hg_cur ^= 1;
        DEVNC(lbk_xfer_wait(c->dev, XF_G0 + b));
        c->cb.grad(x0_host, c->n, c->hg[b], c->cb.user);
        c->cb_f++;
        c->cb_g++;
        DEVNC(lbk_upload_local(c->dev, c->g, c->hg[b]));
        DEV(lbk_dot(c->dev, c->g, c->g, SLOT_INIT));
        DEVNC(lbk_fetch(c->dev, SLOT_INIT, 1, &c->gg));
    } else {
        double t[2];
        if (objective == LBFGS_OBJ_DENSE_QUAD)
            DEV(lbk_dense_eval(c->dev, c->x, c->g, SLOT_INIT));
        else
            DEV(lbk_eval(c->dev, objective, c->x, c->g, SLOT_INIT));
        DEVNC(lbk_fetch(c->dev, SLOT_INIT, 2, t));
        c->f_cur = t[0];
        c->gg = t[1];
        if (c->vf) DEVNC(lbk_vf_ghost_init(c->dev, c->x, c->g, LBK_WSLOT0));
    }
    if (c->cuda) { /* L-BFGS.cu:115, :199 - the host gradient every line search will be given */
        DEVNC(lbk_copy(c->dev, c->g0c, c->g));
        c->cv_f0 = c->cv_fhost = c->f_cur; /* the variants' initial_f = f(x_host), x_host = x0 */
        say(c, "Starting\n");
    }
    c->inited = 1;
    return 0;
}

int lbfgs_solver_init(lbfgs_ctx* c, int objective, const lbfgs_host_fn* cb, int line_search,
                      const lbfgs_constants* k, const double* x0_host, double tolerance,
                      unsigned flags) {
    return solver_init_at(c, objective, cb, line_search, k, x0_host, 0, tolerance, flags);
}

int lbfgs_solver_init_device(lbfgs_ctx* c, int objective, const lbfgs_host_fn* cb, int line_search,
                             const lbfgs_constants* k, const double* x0_dev, double tolerance,
                             unsigned flags) {
    return solver_init_at(c, objective, cb, line_search, k, x0_dev, 1, tolerance, flags);
}

static void fill_result(lbfgs_ctx* c, lbfgs_result* out, double t0, double b0) {
    if (!out) return;
    out->iterations = c->k;
    out->status = c->status;
    out->f = c->f_cur;
    out->gnorm = sqrt(c->gg);
    out->trials_f = c->trials_f;
    out->trials_fg = c->trials_fg;
    out->commits = c->commits;
    out->passes = c->passes;
    out->bytes = lbk_bytes_moved(c->dev) - b0;
    out->seconds = now_s() - t0;
    out->h_min = c->h_min;
    out->h_max = c->h_min < 0 ? -1 : c->h_max;
    out->f_calls = c->cb_f;
    out->grad_calls = c->cb_g;
}

int lbfgs_solver_step(lbfgs_ctx* c, int max_steps, lbfgs_result* out) {
    if (!c || !c->inited) return LBFGS_ERR_STATE;
    const double t0 = now_s(), b0 = lbk_bytes_moved(c->dev);
    c->h_min = -1;
    c->h_max = -1;
    if (!c->finished) {
        for (int s = 0; s < max_steps; ++s) {
            c->steps_left = max_steps - s - 1;
            TRACE_PUSH("lbfgs iteration");
            int rc = c->cuda ? iterate_cuda(c) : c->vf ? iterate_vf(c) : iterate(c);
            TRACE_POP();
            if (rc < 0) {
                (void)spec_drop(c);
                return rc;
            }
            if (rc == 1) {
                c->finished = 1;
                break;
            }
        }
        int rc = spec_drop(c);
        if (rc) return rc;
    }
    fill_result(c, out, t0, b0);
    return c->finished ? c->status : LBFGS_STATUS_RUNNING;
}

int lbfgs_get_x(lbfgs_ctx* c, double* x_out_host) {
    if (!c || !x_out_host) return LBFGS_ERR_BAD_ARG;
    DEVNC(lbk_download(c->dev, x_out_host, c->x));
    return 0;
}

int lbfgs_get_x_device(lbfgs_ctx* c, double* x_out_dev) {
    if (!c || !x_out_dev || c->geo->world != 1) return LBFGS_ERR_BAD_ARG;
    return export_device(c, x_out_dev, c->x);
}

/* dev != 0: x0 and x_out are caller-owned device buffers (lbfgs_minimize_device) */
static int minimize_at(lbfgs_ctx* c, int objective, const lbfgs_host_fn* cb, int line_search,
                       const lbfgs_constants* k, const double* x0, double* x_out, int dev,
                       int max_iterations, double tolerance, unsigned flags, lbfgs_result* out) {
    const double t0 = now_s();
    if (!c) return LBFGS_ERR_BAD_ARG;
    const double b0 = lbk_bytes_moved(c->dev);
    int rc = solver_init_at(c, objective, cb, line_search, k, x0, dev, tolerance, flags);
    if (rc) return rc;
    rc = lbfgs_solver_step(c, max_iterations, NULL); /* sets h_min / h_max for the whole solve */
    if (rc < 0) return rc;
    if (!c->finished) { /* :201-202 (the CUDA path's loop just ends, L-BFGS.cu:358-365) */
        if (!c->cuda) {
            rc = trace_push(c, c->f_cur, sqrt(c->gg), 1);
            if (rc) return rc;
            say(c, "Maximum iterations reached\n");
        }
        c->status = LBFGS_STATUS_MAX_ITER;
        c->finished = 1;
    }
    if (x_out) {
        rc = dev ? lbfgs_get_x_device(c, x_out) : lbfgs_get_x(c, x_out);
        if (rc) return rc;
    }
    fill_result(c, out, t0, b0);
    return c->status;
}

int lbfgs_minimize(lbfgs_ctx* c, int objective, const lbfgs_host_fn* cb, int line_search,
                   const lbfgs_constants* k, const double* x0_host, double* x_out_host,
                   int max_iterations, double tolerance, unsigned flags, lbfgs_result* out) {
    return minimize_at(c, objective, cb, line_search, k, x0_host, x_out_host, 0, max_iterations, tolerance, flags,
                       out);
}

int lbfgs_minimize_device(lbfgs_ctx* c, int objective, const lbfgs_host_fn* cb, int line_search,
                          const lbfgs_constants* k, const double* x0_dev, double* x_out_dev,
                          int max_iterations, double tolerance, unsigned flags, lbfgs_result* out) {
    return minimize_at(c, objective, cb, line_search, k, x0_dev, x_out_dev, 1, max_iterations, tolerance, flags,
                       out);
}

int lbfgs_messages(const lbfgs_ctx* c, char* buf, int cap) {
    if (!c || !buf || cap <= 0) return LBFGS_ERR_BAD_ARG;
    int k = c->msg_len < cap - 1 ? c->msg_len : cap - 1;
    if (k > 0) memcpy(buf, c->msg, (size_t)k);
    buf[k] = 0;
    return c->msg_len;
}

int lbfgs_trace_len(const lbfgs_ctx* c) { return c ? c->tr_len : 0; }

int lbfgs_trace_enable(lbfgs_ctx* c, int on) {
    if (!c || !c->inited) return LBFGS_ERR_STATE;
    if (on)
        c->flags |= LBFGS_FLAG_TRACE;
    else
        c->flags &= ~LBFGS_FLAG_TRACE;
    return 0;
}

int lbfgs_trace_get(const lbfgs_ctx* c, double* f, double* gnorm, double* alpha, uint64_t* c1,
                    uint64_t* c2, int cap) {
    if (!c) return LBFGS_ERR_BAD_ARG;
    int k = c->tr_len < cap ? c->tr_len : cap;
    for (int i = 0; i < k; ++i) {
        if (f) f[i] = c->tr_f[i];
        if (gnorm) gnorm[i] = c->tr_gn[i];
        if (alpha) alpha[i] = c->tr_a[i];
        if (c1) c1[i] = c->tr_c1[i];
        if (c2) c2[i] = c->tr_c2[i];
    }
    return k;
}

/* ------------------------------------------------------------------------------------------
 * Device primitives over host buffers (tests, drop-in vector_utils). They use the context's
 * work vectors and therefore end any solve in progress.
 * ---------------------------------------------------------------------------------------- */
int lbfgs_dev_dot(lbfgs_ctx* c, const double* a, const double* b, double* out) {
    if (!c || !a || !b || !out) return LBFGS_ERR_BAD_ARG;
    c->inited = 0;
    DEVNC(lbk_upload(c->dev, c->q, a));
    DEVNC(lbk_upload(c->dev, c->r, b));
    DEV(lbk_dot(c->dev, c->q, c->r, SLOT_MISC(c->m)));
    DEVNC(lbk_fetch(c->dev, SLOT_MISC(c->m), 1, out));
    return 0;
}

int lbfgs_dev_norm(lbfgs_ctx* c, const double* v, double* out) {
    if (!c || !v || !out) return LBFGS_ERR_BAD_ARG;
    double t;
    int rc = lbfgs_dev_dot(c, v, v, &t);
    if (rc) return rc;
    *out = sqrt(t);
    return 0;
}

int lbfgs_dev_objective(lbfgs_ctx* c, int obj, const double* x, double* f_out, double* g_out) {
    if (!c || !x || obj < 0 || obj == LBFGS_OBJ_HOST || obj > LBFGS_OBJ_DENSE_QUAD) return LBFGS_ERR_BAD_ARG;
    if (obj == LBFGS_OBJ_DENSE_QUAD && !c->dense_set) return LBFGS_ERR_STATE;
    c->inited = 0;
    double t[2];
    DEVNC(lbk_upload(c->dev, c->q, x));
    if (obj == LBFGS_OBJ_DENSE_QUAD)
        DEV(lbk_dense_eval(c->dev, c->q, c->gt, SLOT_MISC(c->m)));
    else
        DEV(lbk_eval(c->dev, obj, c->q, c->gt, SLOT_MISC(c->m)));
    DEVNC(lbk_fetch(c->dev, SLOT_MISC(c->m), 2, t));
    if (f_out) *f_out = t[0];
    if (g_out) DEVNC(lbk_download(c->dev, g_out, c->gt));
    return 0;
}

int lbfgs_dev_trial(lbfgs_ctx* c, int obj, const double* x, const double* d, double alpha,
                    double* f_out, double* g_out, double* dphi_out) {
    if (!c || !x || !d || obj < 0 || obj >= LBFGS_OBJ_HOST) return LBFGS_ERR_BAD_ARG;
    c->inited = 0;
    double t[2];
    DEVNC(lbk_upload(c->dev, c->q, x));
    DEVNC(lbk_upload(c->dev, c->d, d));
    DEV(lbk_trial(c->dev, obj, c->q, c->d, alpha, g_out ? c->gt : NULL, SLOT_MISC(c->m)));
    DEVNC(lbk_fetch(c->dev, SLOT_MISC(c->m), 2, t));
    if (f_out) *f_out = t[0];
    if (dphi_out) *dphi_out = t[1];
    if (g_out) DEVNC(lbk_download(c->dev, g_out, c->gt));
    return 0;
}

int lbfgs_dev_twoloop(lbfgs_ctx* c, const double* g, const double* const* S, const double* const* Y,
                      int h, double* d_out, double* gd_out) {
    if (!c || !g || h < 1 || h > c->m || !S || !Y) return LBFGS_ERR_BAD_ARG;
    c->inited = 0;
    const int m = c->m;
    DEVNC(lbk_upload(c->dev, c->g, g));
    for (int i = 0; i < h; ++i) {
        DEVNC(lbk_upload(c->dev, c->S[i], S[i]));
        DEVNC(lbk_upload(c->dev, c->Y[i], Y[i]));
        c->ring[i] = i;
        DEV(lbk_dot(c->dev, c->S[i], c->Y[i], SLOT_MISC(m)));
        DEVNC(lbk_fetch(c->dev, SLOT_MISC(m), 1, &c->sy[i]));
        DEV(lbk_dot(c->dev, c->Y[i], c->Y[i], SLOT_MISC(m)));
        DEVNC(lbk_fetch(c->dev, SLOT_MISC(m), 1, &c->yy[i]));
    }
    /* the solver's own passes over the identity ring, no s_{h-1}.g carried over, then k_last */
    double rho[MMAX];
    const double* Sr[MMAX];
    const double* Yr[MMAX];
    ring_view(c, c->ring, h, rho, Sr, Yr);
    const int rc = twoloop_passes(c, h, rho, Sr, Yr, c->sy[h - 1] / c->yy[h - 1], -1);
    if (rc) return rc;
    last_update(c, h, rho[h - 1], -1);
    DEV(lbk_last(c->dev, c->d, c->rc, c->S[c->s_last_pair], c->g, c->rho_last, c->ref_b_last, c->ref_a_last,
                 SLOT_LAST(m)));
    double gd;
    DEVNC(lbk_fetch(c->dev, SLOT_LAST(m), 1, &gd));
    if (gd_out) *gd_out = gd;
    if (d_out) DEVNC(lbk_download(c->dev, d_out, c->d));
    return 0;
}

/* Line search alone (line_search.cpp:19-189) at x along d with gradient g: the same driver code
 * as inside lbfgs_minimize, with every trial evaluated on the device (or through the host
 * callbacks for LBFGS_OBJ_HOST). f(x) and g.d are evaluated once (the reference re-evaluates
 * them with identical values). Single rank. */
int lbfgs_line_search(lbfgs_ctx* c, int objective, const lbfgs_host_fn* cb, int line_search,
                      const lbfgs_constants* k, const double* x, const double* d, const double* g,
                      double* alpha_out) {
    if (!c || !x || !d || !g || !alpha_out || c->geo->world != 1) return LBFGS_ERR_BAD_ARG;
    if (objective < 0 || objective > LBFGS_OBJ_DENSE_QUAD) return LBFGS_ERR_BAD_ARG;
    if (line_search < 0 || line_search > LBFGS_LS_BACKTRACKING_WOLFE) return LBFGS_ERR_BAD_ARG;
    if (objective == LBFGS_OBJ_DENSE_QUAD && !c->dense_set) return LBFGS_ERR_STATE;
    c->refcalls = 0; /* the standalone search evaluates f(x) once (see above) */
    if (objective == LBFGS_OBJ_HOST) {
        if (!cb || !cb->f || (!cb->grad && (line_search == LBFGS_LS_WOLFE || line_search == LBFGS_LS_BACKTRACKING_WOLFE)))
            return LBFGS_ERR_BAD_ARG;
        c->cb = *cb;
        if (host_bufs(c)) return LBFGS_ERR_NOMEM;
    }
    c->cb_f = c->cb_g = 0;
    c->inited = 0;
    c->unfused = 0;
    c->batch = env_switch("LBFGS_BATCH", 1);
    c->sr.have_cand = 0;
    c->sr.tc_n = 0;
    c->trial_passes = 0;
    c->many_passes = c->tl_search = 0;
    c->cuda = 0;
    c->obj = objective;
    c->ls = line_search;
    set_constants(c, k);
    const int m = c->m;
    DEVNC(lbk_upload(c->dev, c->x, x));
    DEVNC(lbk_upload(c->dev, c->d, d));
    DEVNC(lbk_upload(c->dev, c->g, g));
    if (objective == LBFGS_OBJ_HOST) {
        c->f_cur = c->cb.f(x, c->n, c->cb.user);
        c->cb_f++;
    } else if (objective == LBFGS_OBJ_DENSE_QUAD) {
        DEV(lbk_dense_eval(c->dev, c->x, c->gt, SLOT_MISC(m)));
        DEVNC(lbk_fetch(c->dev, SLOT_MISC(m), 1, &c->f_cur));
    } else {
        double t[2];
        DEV(lbk_eval(c->dev, objective, c->x, NULL, SLOT_MISC(m)));
        DEVNC(lbk_fetch(c->dev, SLOT_MISC(m), 1, t));
        c->f_cur = t[0];
    }
    double gd;
    DEV(lbk_dot(c->dev, c->g, c->d, SLOT_LAST(m)));
    DEVNC(lbk_fetch(c->dev, SLOT_LAST(m), 1, &gd));
    c->dmode = LBK_D_BUF;
    c->d_ready = 1;
    c->sr.have_spec = 0;
    c->search_cslot = -1;
    host_invalidate(c);
    c->hxx_valid = 0;
    double alpha = 0.0;
    const int rc = search_run(c, gd, &alpha);
    if (rc) return rc;
    *alpha_out = alpha;
    return 0;
}

/* vector_utils.cpp:43-73 on the device: op 0 out = alpha*a, 1 out = a+b, 2 out = -a */
int lbfgs_dev_elementwise(lbfgs_ctx* c, int op, const double* a, const double* b, double alpha,
                          double* out) {
    if (!c || !a || !out || op < 0 || op > 2 || (op == 1 && !b)) return LBFGS_ERR_BAD_ARG;
    c->inited = 0;
    DEVNC(lbk_upload(c->dev, c->q, a));
    if (op == 1) DEVNC(lbk_upload(c->dev, c->r, b));
    DEV(lbk_elementwise(c->dev, op, c->d, c->q, c->r, alpha));
    DEVNC(lbk_download(c->dev, out, c->d));
    return 0;
}

/* ---- profiling ---- */
void lbfgs_prof_enable(lbfgs_ctx* c, int on) { lbk_prof_enable(c->dev, on); }
void lbfgs_prof_reset(lbfgs_ctx* c) { lbk_prof_reset(c->dev); }
int lbfgs_prof_get(lbfgs_ctx* c, int kind, double* ms, int64_t* launches, double* bytes) {
    return lbk_prof_get(c->dev, kind, ms, launches, bytes) == 0 ? 0 : LBFGS_ERR_BAD_ARG;
}
