// lbfgs_kernels_batch.hip — the batched small-n solver (lbfgs_batch_*, include/lbfgs_hip.h): B
// independent problems that share n (or not: ragged batches, below), m, objective, line search,
// constants, tolerance and iteration limit and differ in x0, each solved by ONE workgroup that runs
// the whole loop of iterate() (lbfgs_driver.c) on the device. A translation unit of its own: twelve
// large kernels for the stencil objectives (k_batch_solve), and four for dense quadratics with each
// problem's own A and b (k_batch_solve_dense, further down: the driver's external-objective path),
// and four for a caller's objective evaluated by the host between launches (k_batch_solve_ext, behind
// the dense ones: the dense kernel with the evaluation taken out).
//
// The two kernel templates follow different branches of iterate() and stay two kernels. What the
// branches have in common is written once, as force-inlined stages that both call (batch_enter,
// batch_iter_top, batch_direction, batch_materialise_d, batch_search_begin, batch_accept,
// batch_leave, with BatchView / BatchIter for the vectors), so the host's expressions in the host's
// operand order are kept in one place; a kernel body is the sequence of its stages with only its
// own evaluation, trial and commit inline.
//
// Every pass walks the problem's canonical segments one after another with the per-segment code of
// the launch sequence (seg_at, stream, the Op* operators, wave_sum, ((w0 + w1) + (w2 + w3))), so
// each segment partial is the launch sequence's; the <= 64 partials meet in LDS and one wave forms
// the group-0 tree and the seven empty groups as coop_pass does. The decisions between the passes
// are the host's expressions on the same totals, which every thread holds (uniform branches). The
// result of every problem is therefore bit for bit lbfgs_minimize's for that problem alone.
// Nothing here waits on another workgroup, a flag or the host: no grid barrier, no time-out.
//
// x0 and x are rows at a stride (BatchArgs xin / xout), A's rows and b likewise (BatchDenseArgs lda /
// ldb): the batch's own buffers for the host forms, a caller's device buffers as they are for
// lbfgs_batch_minimize_device and lbfgs_batch_set_dense_quadratics_device.
//
// A ragged batch (lbfgs_batch_create_ragged) gives every problem its own n: the
// problems' vectors lie packed one behind another, a table in device memory has a row per problem
// (BatchRow), and the workgroup forms its problem's geometry, vectors and rows from that row inside
// the problem loop; passes, stages and searches are the same code. Its kernels are a second
// compilation of the two kernel bodies (sixteen more), so a uniform batch runs what it always ran.
#include "lbfgs_hip.h"
#include "lbfgs_kernels_impl.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>

#define LBK_BATCH_NMAX 32768       // L = 512 and at most 64 segments: stage 2 is one wave
#define LBK_BATCH_SEGMAX 64
#define LBK_BATCH_ITERS 64         // iterations per launch (default)
#define LBK_BATCH_BTW_CAP 4096     // trial passes of one backtracking_wolfe search (see the header)
#define LBK_BATCH_NVEC(m) (7 + 2 * ((m) + 1))  // x g xn gn d q r, then the m + 1 pairs (s, y)
#define LBK_BATCH_DENSE_NMAX 4096  // dense quadratics: 128 MiB of A per problem at the limit

namespace {

// one problem's state between launches (device memory; the host reads it after the last launch)
struct BatchState {
    int k, h, status, free_pair, sg_valid, flip;  // flip: x/xn and g/gn have changed places
    int h_min, h_max, tr_len;
    int ev[4];                                    // not_descent, skipped_updates, invalid_rho, invalid_gamma
    int ring[LBK_SMALL_HMAX];
    long long trials_f, trials_fg, commits;
    double f_cur, gg, sg, vecs;                   // sg: the last commit's s . g_new; vecs: n-vectors streamed
    double sy[LBK_SMALL_HMAX + 1], yy[LBK_SMALL_HMAX + 1];
};

struct BatchArgs {
    int B, m, iters, max_iterations, trace, init, tr_cap;
    int64_t vstride, pstride;  // doubles per vector / per problem
    double* base;              // element 0 of vector 0 of problem 0
    const double* xin;         // x0 in: problem p's n doubles at xin + p * ldxin (ldxin 0: one x0 for all)
    double* xout;              // x out: problem p's at xout + p * ldxout. The batch's own [B][n] for both
    int64_t ldxin, ldxout;     // (lbfgs_batch_minimize), or the caller's rows (lbfgs_batch_minimize_device)
    BatchState* st;
    double* tr;                // [B][3][tr_cap]: f, |g|, alpha
    int* running;              // set when a problem is unfinished at the end of the launch
    double tol;
    lbfgs_constants K;
};

// A ragged batch (lbfgs_batch_create_ragged): problem p has its own size n_p and
// its vectors lie packed behind those of the problems before it. One row per problem, written once
// at creation; every offset is in doubles.
struct BatchRow {
    int64_t n;        // n_p
    int64_t vbase;    // element 0 of vector 0 of problem p, from BatchArgs::base
    int64_t vstride;  // doubles per vector: lbk_vec_alloc's layout for n_p
    int64_t off;      // packed offset of x0 / x / b: the sum of n_q over q < p
    int64_t off2;     // packed offset of A: the sum of n_q * n_q over q < p
    int64_t xbase;    // dense: problem p's terms vector t, from BatchDenseArgs::xbase
};

// The last argument of a ragged batch's kernels; a uniform batch's do not have it.
struct BatchRagged {
    const BatchRow* tab;  // [B]
    const int* order;     // [B]: the i-th problem taken is order[i] (largest first); null: i itself
};

// The problem a workgroup is on: its index, and on a ragged batch its row of the table.
struct BatchProb {
    int p;
    const BatchRow* row;
};

// A table value: the same in every thread of the workgroup, so it belongs in SGPRs. The load is
// through the constant address space (a scalar load; the table is written before the first launch
// and never by a kernel), and the halves pass through readfirstlane so that the compiler knows the
// uniformity wherever it has lost sight of it.
__device__ __forceinline__ int64_t batch_row_ld(const int64_t* q) {
    const int64_t v = *(const __attribute__((address_space(4))) int64_t*)q;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}

template <bool RAGGED>
__device__ __forceinline__ BatchProb batch_prob(const BatchRagged& rg, int i) {
    if (!RAGGED) return {i, nullptr};
    const int p =
        rg.order ? __builtin_amdgcn_readfirstlane(*(const __attribute__((address_space(4))) int*)(rg.order + i)) : i;
    return {p, rg.tab + p};
}

// The geometry of the problem: the batch's, with n, n_loc and nseg the problem's own on a ragged batch.
template <bool RAGGED>
__device__ __forceinline__ Geo batch_geo(const Geo& geo, const BatchProb& P) {
    Geo g = geo;
    if (RAGGED) {
        const int64_t n = batch_row_ld(&P.row->n);
        g.n = g.n_loc = n;
        g.nseg = (n + 511) / 512;
    }
    return g;
}

// A problem's scalars are the same in every thread of its workgroup. Held in registers they (the
// state, the search's variables and caches, the commit's totals: some 250 values) are live across
// every inlined pass and left the streaming loops no registers; each wave keeps its own copy in LDS
// instead, every lane storing the same value to the same address, and nothing is read across waves.
struct BatchWave {
    BatchState st;
    lbk_search s;
    double tot[LBK_KMAX];      // the latest commit's totals
    double TA[LBK_SMALL_HMAX]; // s_i . q of the first loop
    double coef, rho_top;      // TWOLOOP: alpha - beta and rho of the last second-loop update
    int dmode, top, d_ready, capped, passes;
};

struct BatchLds {
    double ws[4][LBK_KMAX][LBK_BATCH_SEGMAX];  // wave partials of every segment of the pass
    double tl[LBK_KMAX];
    BatchWave wv[4];
};

__device__ __forceinline__ void batch_stage_sync() {  // stores of one stage before loads of the next
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One pass of one problem: the segments in order, each exactly as its workgroup of the launch
// sequence streams it; then the fixed-order total (coop_pass's nseg <= 64 form). The barrier with
// its workgroup-scope fences also orders this pass's vector stores before the next pass's loads
// (other waves' rows, and the stencil halo across a segment seam).
template <int K, class Op>
__device__ __forceinline__ void batch_pass(const Op& op, const Geo& geo, BatchLds& L, double* tot) {
    // the thread index through an empty asm: without it every inlined pass's per-lane addresses
    // (loop invariants of the iteration loop) are formed at kernel entry and held in registers
    // throughout - some 250 VGPRs, with spills into the streaming loops
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    const int lane = t & 63, w = t >> 6;
    const int nseg = (int)geo.nseg;
    for (int sg = 0; sg < nseg; ++sg) {
        const Seg s = seg_at(geo, sg, t);
        double acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0.0;
        stream(op, s, geo, acc);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double v = wave_sum(acc[k]);
            if (lane == 0) L.ws[w][k][sg] = v;
        }
    }
    batch_stage_sync();
#pragma unroll
    for (int k = w; k < K; k += 4) {  // wave w: components w, w + 4; lane j: segment j
        const double p = lane < nseg ? (L.ws[0][k][lane] + L.ws[1][k][lane]) + (L.ws[2][k][lane] + L.ws[3][k][lane]) : 0.0;
        const double q0 = wave_sum(p) + 0.0;  // group 0: the tree's levels above 64 add 0.0
        if (lane == 0) {
            double tt = q0;
#pragma unroll
            for (int g = 1; g < LBK_GROUPS; ++g) tt = tt + 0.0;
            L.tl[k] = tt;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) tot[k] = L.tl[k];
    __syncthreads();  // ws / tl reuse by the next pass
}

template <int OBJ, int DMODE, bool CAND>
__device__ __forceinline__ void batch_commit(const Geo& geo, BatchLds& L, const double* x, const DirArgs& da,
                                             double alpha, double* xn, double* gn, double* so, double* yo,
                                             double cand, double* tot) {
    batch_pass<CAND ? 8 : 7>(OpCommit<OBJ, DMODE, false, CAND>{x, da, alpha, xn, gn, so, yo, geo.n, geo.n_loc, cand},
                             geo, L, tot);
}

// ---------------------------------------------------------------------------------------
// The stages of iterate() that k_batch_solve and k_batch_solve_dense share, each written once.
// They take the wave's records by reference and keep nothing of them in locals across a pass.
// ---------------------------------------------------------------------------------------

// one problem's vectors (x g xn gn d q r, then the m + 1 pairs) and its trace rows
struct BatchView {
    double* vb;       // element 0 of vector 0
    int64_t vstride;
    double* trf;      // [3][tr_cap]: f, |g|, alpha; null without a trace
    __device__ __forceinline__ double* vec(int i) const { return vb + (int64_t)i * vstride; }
    __device__ __forceinline__ double* d() const { return vec(4); }
    __device__ __forceinline__ double* q() const { return vec(5); }
    __device__ __forceinline__ double* r() const { return vec(6); }
    __device__ __forceinline__ double* s(int pair) const { return vec(7 + 2 * pair); }
    __device__ __forceinline__ double* y(int pair) const { return vec(8 + 2 * pair); }
};

template <bool RAGGED>
__device__ __forceinline__ BatchView batch_view(const BatchArgs& a, const BatchProb& P) {
    const int p = P.p;
    if (RAGGED)
        return {a.base + batch_row_ld(&P.row->vbase), batch_row_ld(&P.row->vstride),
                a.trace ? a.tr + (int64_t)p * 3 * a.tr_cap : nullptr};
    return {a.base + (int64_t)p * a.pstride, a.vstride, a.trace ? a.tr + (int64_t)p * 3 * a.tr_cap : nullptr};
}

// Problem p's row of a batch of rows: at p * ld, or on a ragged batch with ld == LBFGS_BATCH_PACKED at
// the problem's packed offset.
template <bool RAGGED>
__device__ __forceinline__ int64_t batch_row_at(const BatchProb& P, int64_t ld) {
    if (RAGGED && ld < 0) return batch_row_ld(&P.row->off);
    return (int64_t)P.p * ld;
}

// one iteration's vectors: which of x/xn and g/gn is current, and the spare pair the commit fills
struct BatchIter {
    double *x, *xn, *g, *gn, *so, *yo;
};

// Entering a problem. A new solve starts a fresh record and moves x0 into the vector layout (the
// kernel then evaluates there); a later launch loads the record. True when the problem finished in
// an earlier launch (uniform).
template <bool RAGGED>
__device__ __forceinline__ bool batch_enter(const BatchArgs& a, const BatchView& V, const BatchProb& P, int64_t n,
                                            BatchState& S) {
    const int p = P.p;
    if (!a.init) {
        const BatchState* G = a.st + p;
        if (G->status != LBFGS_STATUS_RUNNING) return true;
        S = *G;
        return false;
    }
    S = BatchState();
    S.status = LBFGS_STATUS_RUNNING;
    S.h_min = S.h_max = -1;
    double* x0 = V.vec(0);
    const double* xin = a.xin + batch_row_at<RAGGED>(P, a.ldxin);
    for (int64_t i = threadIdx.x; i < n; i += LB_BLOCK) x0[i] = xin[i];
    batch_stage_sync();
    return false;
}

__device__ __forceinline__ void batch_trace_push(const BatchArgs& a, const BatchView& V, BatchState& S, double f,
                                                 double gn) {
    if (!V.trf) return;
    if (threadIdx.x == 0 && S.tr_len < a.tr_cap) {
        V.trf[S.tr_len] = f;
        V.trf[a.tr_cap + S.tr_len] = gn;
        V.trf[2 * a.tr_cap + S.tr_len] = __builtin_nan("");
    }
    S.tr_len++;
}

// the accepted step into the entry that the iteration's top pushed
__device__ __forceinline__ void batch_trace_step(const BatchArgs& a, const BatchView& V, const BatchState& S,
                                                 double alpha) {
    if (V.trf && threadIdx.x == 0 && S.tr_len - 1 < a.tr_cap) V.trf[2 * a.tr_cap + S.tr_len - 1] = alpha;
}

// Top of an iteration; true when it ends the problem (status set).
__device__ __forceinline__ bool batch_iter_top(const BatchArgs& a, const BatchView& V, BatchState& S, BatchIter& I) {
    if (S.k >= a.max_iterations) {  // lbfgs.cpp:201-202
        batch_trace_push(a, V, S, S.f_cur, sqrt(S.gg));
        S.status = LBFGS_STATUS_MAX_ITER;
        return true;
    }
    const int h = S.h;
    I.x = V.vec(S.flip ? 2 : 0);
    I.xn = V.vec(S.flip ? 0 : 2);
    I.g = V.vec(S.flip ? 3 : 1);
    I.gn = V.vec(S.flip ? 1 : 3);
    I.so = V.s(S.free_pair);
    I.yo = V.y(S.free_pair);
    const double gnorm = sqrt(S.gg);
    batch_trace_push(a, V, S, S.f_cur, gnorm);
    if (gnorm < a.tol) {  // :80-84
        S.status = LBFGS_STATUS_CONVERGED;
        return true;
    }
    if (S.h_min < 0 || h < S.h_min) S.h_min = h;
    if (h > S.h_max) S.h_max = h;
    return false;
}

// Search direction (:87-143): the validity tests and the two-loop's passes but the last update.
// Leaves W.dmode, and for TWOLOOP W.coef, W.rho_top, W.top with r holding all but that update.
__device__ __forceinline__ void batch_direction(const BatchView& V, const BatchIter& I, const Geo& geo, BatchLds& L,
                                                BatchState& S, BatchWave& W) {
    const int h = S.h;
    double* const q = V.q();
    double* const r = V.r();
    W.dmode = LBK_D_NEG_G;
    double gamma = 0.0;
    if (!(S.k == 0 || h == 0)) {
        int bad_rho = 0;
        for (int i = h - 1; i >= 0; --i)
            if (!isfinite(1.0 / S.sy[S.ring[i]])) bad_rho = 1;  // :102-108
        if (bad_rho) {
            S.ev[2]++;
        } else {
            const int top = S.ring[h - 1];
            gamma = S.sy[top] / S.yy[top];  // :117-118
            if (gamma <= 0 || !isfinite(gamma))
                S.ev[3]++;
            else
                W.dmode = LBK_D_TWOLOOP;
        }
    }
    if (W.dmode != LBK_D_TWOLOOP) return;
    const int top = S.ring[h - 1];
    const double rho_top = 1.0 / S.sy[top];
    double t1[1];
    // alpha_{h-1} = rho_{h-1} (s_{h-1} . g): the previous commit's s . g_new, or a dot pass
    if (S.sg_valid) {
        t1[0] = S.sg;
    } else {
        batch_pass<1>(OpDot<false>{V.s(top), I.g}, geo, L, t1);
        S.vecs += 2.0;
    }
    W.TA[h - 1] = t1[0];
    double alpha = rho_top * t1[0];
    const double* qsrc = I.g;
    for (int i = h - 2; i >= 0; --i) {  // q = q - alpha_{i+1} y_{i+1};  s_i . q
        batch_pass<1>(OpAxpyDot<false>{q, qsrc, V.y(S.ring[i + 1]), V.s(S.ring[i]), alpha}, geo, L, t1);
        S.vecs += 4.0;
        W.TA[i] = t1[0];
        alpha = (1.0 / S.sy[S.ring[i]]) * t1[0];
        qsrc = q;
    }
    batch_pass<1>(OpMid<false>{r, qsrc, V.y(S.ring[0]), alpha, gamma}, geo, L, t1);
    S.vecs += 3.0;
    for (int i = 0; i + 1 < h; ++i) {  // r += s_i (alpha_i - beta_i);  y_{i+1} . r
        const double rho = 1.0 / S.sy[S.ring[i]];
        const double beta = rho * t1[0];
        const double alph = rho * W.TA[i];
        batch_pass<1>(OpAxpy2Dot<false>{r, r, V.s(S.ring[i]), V.y(S.ring[i + 1]), alph - beta}, geo, L, t1);
        S.vecs += 4.0;
    }
    // the last second-loop update rides the commit (k_commit TWOLOOP) or the pass that materialises d
    const double beta = rho_top * t1[0];
    const double alph = rho_top * W.TA[h - 1];
    W.coef = alph - beta;
    W.rho_top = rho_top;
    W.top = top;
}

// d into its buffer (materialize_d: k_last / k_negdot); the pass total is g . d
__device__ __forceinline__ double batch_materialise_d(const BatchView& V, const BatchIter& I, const Geo& geo,
                                                      BatchLds& L, BatchState& S, BatchWave& W) {
    double t1[1];
    if (W.dmode == LBK_D_TWOLOOP) {
        batch_pass<1>(OpLast<false>{V.d(), V.r(), V.s(W.top), I.g, W.coef}, geo, L, t1);
        S.vecs += 4.0;
    } else {
        batch_pass<1>(OpNegDot<false>{V.d(), I.g}, geo, L, t1);
        S.vecs += 2.0;
    }
    return t1[0];
}

// the direction read from d's buffer (k_commit's / k_trials' BUF)
__device__ __forceinline__ DirArgs batch_buf_args(const BatchView& V, const BatchIter& I) {
    DirArgs db = {};
    db.dsrc = V.d();
    db.g = I.g;
    db.g_hi = LBK_GROUPS;
    return db;
}

// The line search (:156) from the top: everything but the fused path's caches.
__device__ __forceinline__ void batch_search_begin(const BatchArgs& a, const BatchState& S, lbk_search& s, double gd) {
    __builtin_memset(&s, 0, sizeof s);
    s.f_x = S.f_cur;
    s.gd = gd;
    s.c1 = a.K.c1;
    s.c2 = a.K.c2;
    s.amin = a.K.wolfe_interp_min;
    s.init = a.K.initial_step;
    s.beta = a.K.backtracking_alpha;
    s.tol = a.K.backtracking_tol;
    s.alpha = a.K.initial_step;
    s.alpha_hi = INFINITY;
    s.f_lo = s.f_prev = S.f_cur;
    s.dphi_lo = gd;
}

// Accepting the step (:182-198) from the commit's totals: the pair stored when s . y > 0, the ring
// rotated with the spare pair once it is full; x = x_new, g = g_new.
__device__ __forceinline__ void batch_accept(int m, BatchState& S, const BatchWave& W) {
    const int h = S.h;
    const double sy = W.tot[LBK_C_SY];
    if (sy > 0) {  // :182-191
        const int pair = S.free_pair;
        if (h >= m) {
            const int oldest = S.ring[0];
            for (int i = 0; i + 1 < m; ++i) S.ring[i] = S.ring[i + 1];
            S.ring[m - 1] = pair;
            S.free_pair = oldest;
        } else {
            S.ring[h] = pair;
            S.h = h + 1;
            S.free_pair = h + 1;  // pool slots 0..h used, h + 1 is free
        }
        S.sy[pair] = sy;
        S.yy[pair] = W.tot[LBK_C_YY];
        S.sg_valid = 1;
        S.sg = W.tot[LBK_C_SG];
    } else {  // :192-195
        S.ev[1]++;
        S.sg_valid = 0;
    }
    S.flip ^= 1;  // :197-198
    S.gg = W.tot[LBK_C_GG];
    S.k++;
}

// Leaving a problem: x out when it finished in this launch, the record stored, the running flag.
template <bool RAGGED>
__device__ __forceinline__ void batch_leave(const BatchArgs& a, const BatchView& V, const BatchProb& P, int64_t n,
                                            const BatchState& S) {
    const int p = P.p;
    if (S.status != LBFGS_STATUS_RUNNING) {
        const double* xc = V.vec(S.flip ? 2 : 0);
        double* xout = a.xout + batch_row_at<RAGGED>(P, a.ldxout);
        for (int64_t i = threadIdx.x; i < n; i += LB_BLOCK) xout[i] = xc[i];
    }
    if (threadIdx.x == 0) {
        a.st[p] = S;
        if (S.status == LBFGS_STATUS_RUNNING) atomicOr(a.running, 1);
    }
}

// The fused stencil branch of iterate(): the first trial at initial_step rides the commit, the
// search starts from that pass's totals, and the commit is repeated only at another step.
// One body, two argument lists (lbfgs_kernels_batch_solve.h says why).
template <int OBJ, int LS>
__global__ __launch_bounds__(LB_BLOCK) void k_batch_solve(BatchArgs a, Geo geo_b) {
    constexpr bool RAGGED = false;
    const BatchRagged rg = {nullptr, nullptr};
#include "lbfgs_kernels_batch_solve.h"
}

template <int OBJ, int LS>
__global__ __launch_bounds__(LB_BLOCK) void k_batch_solve_ragged(BatchArgs a, Geo geo_b, BatchRagged rg) {
    constexpr bool RAGGED = true;
#include "lbfgs_kernels_batch_solve.h"
}

// ---------------------------------------------------------------------------------------
// Dense quadratics, every problem with its own A and b (lbfgs_batch_set_dense_quadratics):
// k_batch_solve_dense follows the external-objective branch of iterate() (lbfgs_driver.c,
// ext_obj()), not the fused stencil branch above, over the same stages. d is materialised before
// the search (k_last / k_negdot, whose total is g . d), the search starts with nothing cached, a
// trial is z = x + alpha d (k_point), the rows of A z (k_dense_rows) and the terms pass
// (k_terms_dot), the commit reads the gradient it is given (OpCommit<LBK_OBJ_NONE>) and takes f
// from the evaluation.
// ---------------------------------------------------------------------------------------
struct BatchDenseArgs {
    const double* A;   // problem p's row i at A + p * astride + i * lda; astride 0: one matrix for all
    const double* b;   // problem p's at b + p * ldb; ldb 0: one b for all
    double* xbase;     // element 0 of problem 0's terms vector t; its trial gradient gt one vector behind
    int64_t astride;   // the batch's own copies: n * n (or 0), lda = ldb = n; a caller's buffers
    int64_t lda, ldb;  // (lbfgs_batch_set_dense_quadratics_device): the caller's strides
};

// the host's caches of an external objective (host_point_issue / host_f_at / host_g_at with
// refcalls = 0): the point in xn, f at the last point, the gradient in gt at the last point
struct DenseWave {
    int hz_valid, hf_valid, gt_valid;
    double hz_alpha, hf_alpha, hf_val, gt_alpha;
};

struct BatchDenseLds {
    BatchLds L;
    DenseWave dw[4];
};

// z = x + alpha d, k_point's arithmetic. k_point also forms the two ghost cells, 0 + alpha * 0; no
// stage of the dense path reads them, and a step that is not finite would leave NaN there for a
// later stencil solve on the same batch object, whose halo loads rely on zero ghosts: [0, n) only.
__device__ __forceinline__ void dense_point(double* z, const double* x, const double* d, double alpha, int64_t n) {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    for (int64_t i = t; i < n; i += LB_BLOCK) z[i] = x[i] + alpha * d[i];
    batch_stage_sync();
}

// k_dense_rows inside one workgroup: row i is one wave (wave w: rows w, w + 4, ...; which wave takes
// which row does not reach the bits), lane l accumulates fma(A_ij, z_j) over j = l, l + 64, ...
// ascending, then the wave butterfly. The row index is wave-uniform and the loop holds no barrier,
// so with fewer rows than waves the idle waves fall through to the barrier behind it.
__device__ __forceinline__ void dense_rows(const double* __restrict__ A, const double* __restrict__ b, const double* z,
                                           double* g, double* tv, int64_t n, int64_t lda) {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    const int lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    for (int64_t i = w; i < n; i += 4) {
        const double* __restrict__ a = A + i * lda;
        double v = 0.0;
        for (int64_t j = lane; j < n; j += 64) v = fma(a[j], z[j], v);
        v = wave_sum(v);
        if (lane == 0) {
            const double zi = z[i];
            g[i] = 2.0 * v + b[i];
            tv[i] = zi * v + b[i] * zi;
        }
    }
    batch_stage_sync();
}

template <int LS>
__global__ __launch_bounds__(LB_BLOCK) void k_batch_solve_dense(BatchArgs a, BatchDenseArgs dq, Geo geo_b) {
    constexpr bool RAGGED = false;
    const BatchRagged rg = {nullptr, nullptr};
#include "lbfgs_kernels_batch_solve_dense.h"
}

template <int LS>
__global__ __launch_bounds__(LB_BLOCK) void k_batch_solve_dense_ragged(BatchArgs a, BatchDenseArgs dq, Geo geo_b,
                                                                       BatchRagged rg) {
    constexpr bool RAGGED = true;
#include "lbfgs_kernels_batch_solve_dense.h"
}

// ---------------------------------------------------------------------------------------
// A caller's objective (lbfgs_batch_set_device_objective): k_batch_solve_ext is
// the dense kernel with the evaluation taken out. A problem that needs f and the gradient at a point
// writes the point into its Z row, stores where it stands (BatchExtRec, beside its BatchState) and is
// left; the host calls the caller's function once for all waiting problems and launches again. The
// kernel holds no wait, no flag and no time-out, as the other batch kernels.
// ---------------------------------------------------------------------------------------
enum { LBK_EXT_TOP = 0, LBK_EXT_AT_X0 = 1, LBK_EXT_SEARCH = 2, LBK_EXT_COMMIT_F = 3, LBK_EXT_COMMIT_G = 4 };

// where a problem stands between two launches: its phase, the step it waits for, the search's
// variables, the driver's three caches, the search's pass count and cap flag. d is in its buffer,
// g . d in s.gd and the commit reads LBK_D_BUF, so nothing else has to survive.
struct BatchExtRec {
    int phase, wait, capped, passes;
    long long evals;  // rounds the problem was active in
    double pend;
    DenseWave D;
    lbk_search s;
};

struct BatchExtArgs {
    double* zbase;     // element 0 of problem 0's point row Z; its gradient row GT one vector behind
    const double* F;   // [B]: f at the pending point, from the round
    int* active;       // [B]: set for a problem that waits (cleared by the host before the launch)
    int* nactive;      // how many were set
    BatchExtRec* rec;  // [B]
    long long* evals;  // [B]: rec[p].evals as the problem was last left, for the host's read-back
};

struct BatchExtLds {
    BatchLds L;
    BatchExtRec xr[4];
};

template <int LS>
__global__ __launch_bounds__(LB_BLOCK) void k_batch_solve_ext(BatchArgs a, BatchExtArgs xa, Geo geo_b) {
#include "lbfgs_kernels_batch_solve_ext.h"
}

const void* batch_ext_kernel(int ls) {
    switch (ls) {
        case 0: return (const void*)k_batch_solve_ext<0>;
        case 1: return (const void*)k_batch_solve_ext<1>;
        case 2: return (const void*)k_batch_solve_ext<2>;
        default: return (const void*)k_batch_solve_ext<3>;
    }
}

// A ragged batch has its own kernels, with the BatchRagged as their last argument; a uniform batch
// runs the kernels it always ran.
const void* batch_dense_kernel(int ls, bool ragged) {
    switch (ls) {
        case 0: return ragged ? (const void*)k_batch_solve_dense_ragged<0> : (const void*)k_batch_solve_dense<0>;
        case 1: return ragged ? (const void*)k_batch_solve_dense_ragged<1> : (const void*)k_batch_solve_dense<1>;
        case 2: return ragged ? (const void*)k_batch_solve_dense_ragged<2> : (const void*)k_batch_solve_dense<2>;
        default: return ragged ? (const void*)k_batch_solve_dense_ragged<3> : (const void*)k_batch_solve_dense<3>;
    }
}

template <int OBJ>
const void* batch_kernel_ls(int ls, bool ragged) {
    switch (ls) {
        case 0: return ragged ? (const void*)k_batch_solve_ragged<OBJ, 0> : (const void*)k_batch_solve<OBJ, 0>;
        case 1: return ragged ? (const void*)k_batch_solve_ragged<OBJ, 1> : (const void*)k_batch_solve<OBJ, 1>;
        case 2: return ragged ? (const void*)k_batch_solve_ragged<OBJ, 2> : (const void*)k_batch_solve<OBJ, 2>;
        default: return ragged ? (const void*)k_batch_solve_ragged<OBJ, 3> : (const void*)k_batch_solve<OBJ, 3>;
    }
}
const void* batch_kernel(int obj, int ls, bool ragged) {
    switch (obj) {
        case LBK_OBJ_ROSENBROCK: return batch_kernel_ls<LBK_OBJ_ROSENBROCK>(ls, ragged);
        case LBK_OBJ_QUAD_TRIDIAG: return batch_kernel_ls<LBK_OBJ_QUAD_TRIDIAG>(ls, ragged);
        default: return batch_kernel_ls<LBK_OBJ_QUAD_SEPARABLE>(ls, ragged);
    }
}

int64_t batch_vstride(int64_t n) { return LBK_FRONT + ((n + 511) / 512) * 512 + 512; }  // lbk_create's vec_doubles

}  // namespace

struct lbfgs_batch {
    int64_t n, vstride, pstride;  // a ragged batch: n = the largest n_p, vstride and pstride unused
    // a ragged batch (lbfgs_batch_create_ragged): the sizes, and the B + 1 running sums of n_p, of
    // n_p * n_p and of the vector strides; the table and the order of work in device memory
    bool ragged;
    std::vector<int64_t> np, off, off2, vsum;
    BatchRow* tab;
    int* order;
    int m, B, device, cus;
    int max_wg, iters;
    double* vecs;     // B problems x NVEC vectors, each laid out as lbk_vec_alloc's
    double* xio;      // [B][n]; a ragged batch: packed, problem p at off[p]
    BatchState* st;
    int* running;
    double* tr;       // device trace, [B][3][tr_cap]
    int tr_cap;
    // dense quadratics (lbfgs_batch_set_dense_quadratics): the matrices, the linear terms, and per
    // problem the terms vector t and the trial gradient gt in the vectors' own layout
    double* dq_A;
    double* dq_b;
    double* dq_x;
    size_t dq_A_doubles;  // capacity of dq_A
    bool dq_set, dq_shared;
    // ... or, by reference, a caller's device buffers (lbfgs_batch_set_dense_quadratics_device):
    // nothing of them is copied, dq_A and dq_b are released, t and gt stay the batch's own
    bool dq_ref;
    const double* ref_A;
    const double* ref_b;
    int64_t ref_astride, ref_lda, ref_ldb;
    // a caller's objective (lbfgs_batch_set_device_objective): per problem the point row Z and the
    // gradient row GT in the vectors' own layout, f per problem, the flags (running, the count of
    // waiting problems, then active[B]) and the resumable records; allocated by the first setter call
    lbfgs_batch_device_fn cb;
    bool cb_set;
    double* cb_x;
    double* cb_F;
    int* cb_flags;
    BatchExtRec* cb_rec;
    long long* cb_evals;
    std::vector<long long> hevals;  // the rounds each problem was active in, after the last such solve
    hipStream_t stream;
    std::vector<BatchState> hst;  // the states after the last solve
    std::vector<double> htr;      // its traces (LBFGS_FLAG_TRACE)
    int htr_cap;
    bool solved;
    Geo geo;
    char err[256];
};

#define BHIP(b, expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            snprintf((b)->err, sizeof (b)->err, "%s: %s", #expr, hipGetErrorString(e_));        \
            return LBFGS_ERR_HIP;                                                               \
        }                                                                                       \
    } while (0)

static int64_t batch_sum_v(const lbfgs_batch* b);

// The per-problem terms vector t and trial gradient gt of the dense objective, allocated once.
static int batch_dense_scratch(lbfgs_batch* b, const char* who) {
    if (b->dq_x) return 0;
    const size_t xbytes = sizeof(double) * 2 * (size_t)batch_sum_v(b);
    if (hipMalloc((void**)&b->dq_x, xbytes) != hipSuccess) {  // the batch stays usable for the stencil objectives
        (void)hipGetLastError();
        b->dq_x = nullptr;
        snprintf(b->err, sizeof b->err, "%s: out of device memory", who);
        return LBFGS_ERR_NOMEM;
    }
    // ghost cells and padding are zero and stay zero, as the batch's other vectors'
    if (hipMemsetAsync(b->dq_x, 0, xbytes, b->stream) != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(b->dq_x);
        b->dq_x = nullptr;
        snprintf(b->err, sizeof b->err, "%s: hipMemsetAsync failed", who);
        return LBFGS_ERR_HIP;
    }
    return 0;
}

// A caller's buffer of `doubles` doubles at p: 8-byte aligned, plain device memory of the batch's
// device (pinned host, managed and other devices' memory are refused), and, where the runtime
// knows the allocation, inside it from the first byte to the last. A wrong pointer ends here as a
// status, not as a fault in a kernel.
static bool batch_caller_range(const lbfgs_batch* b, const double* p, int64_t doubles) {
    if (!p || ((uintptr_t)p & 7) != 0 || doubles < 1) return false;
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (at.type != hipMemoryTypeDevice || at.isManaged || at.device != b->device) return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return true;  // an allocation the runtime gives no extent for: the attributes are the check
    }
    return (const char*)p >= (const char*)base &&
           (const char*)p + sizeof(double) * (size_t)doubles <= (const char*)base + size;
}

// the doubles from the first element of row 0 to the last of row rows - 1 (ld 0: one row)
static int64_t batch_span(int64_t rows, int64_t ld, int64_t n) { return (ld ? (rows - 1) * ld : 0) + n; }

static bool batch_overlap(const double* p, int64_t np, const double* q, int64_t nq) {
    return (uintptr_t)p < (uintptr_t)(q + nq) && (uintptr_t)q < (uintptr_t)(p + np);
}

// ---- the sizes a ragged batch's checks and copies need; a uniform batch answers with n ----
static int64_t batch_np(const lbfgs_batch* b, int64_t p) { return b->ragged ? b->np[(size_t)p] : b->n; }
static int64_t batch_sum_n(const lbfgs_batch* b) { return b->ragged ? b->off[(size_t)b->B] : b->n * b->B; }
static int64_t batch_sum_v(const lbfgs_batch* b) { return b->ragged ? b->vsum[(size_t)b->B] : b->vstride * b->B; }
// the doubles a batch of rows spans: (B - 1) * ld + n_{B-1} (ld 0: one row), or packed the sum of n_p
static int64_t batch_xspan(const lbfgs_batch* b, int64_t ld) {
    if (ld == LBFGS_BATCH_PACKED) return batch_sum_n(b);
    return batch_span(b->B, ld, batch_np(b, b->B - 1));
}
// ... and the matrices: (B - 1) * astride + (n_{B-1} - 1) * lda + n_{B-1}, or packed the sum of n_p * n_p
static int64_t batch_aspan(const lbfgs_batch* b, int64_t astride, int64_t lda) {
    if (astride == LBFGS_BATCH_PACKED) return b->off2[(size_t)b->B];
    const int64_t nl = batch_np(b, b->B - 1);
    return batch_span(b->B, astride, (nl - 1) * lda + nl);
}
static bool batch_any_over(const lbfgs_batch* b, int64_t limit) {
    if (!b->ragged) return b->n > limit;
    for (int64_t v : b->np)
        if (v > limit) return true;
    return false;
}

// The order of work of a ragged batch: the largest problems first (ties by index), so that with
// fewer workgroups than problems no workgroup is left with a large problem at the end. A launch
// with a workgroup for every problem does not use it (batch_solve). Results do not depend on it;
// LBFGS_BATCH_ORDER=identity gives 0, 1, 2, ... (tests and measurements).
static void batch_order(const std::vector<int64_t>& np, std::vector<int>& order) {
    order.resize(np.size());
    for (size_t i = 0; i < np.size(); ++i) order[i] = (int)i;
    const char* e = getenv("LBFGS_BATCH_ORDER");
    if (e && strcmp(e, "identity") == 0) return;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return np[(size_t)x] > np[(size_t)y]; });
}

extern "C" {

int lbfgs_batch_ragged_plan(const int64_t* n, int batch, int m, int dense, double* bytes) {
    if (!n || batch < 1 || m < 1 || m > LBK_SMALL_HMAX) return LBFGS_ERR_BAD_ARG;
    double total = 0.0;
    for (int p = 0; p < batch; ++p) {
        if (n[p] < 1 || n[p] > (dense ? LBK_BATCH_DENSE_NMAX : LBK_BATCH_NMAX)) return LBFGS_ERR_BAD_ARG;
        const double np = (double)n[p], vs = (double)batch_vstride(n[p]);
        // the problem as a batch of one (lbfgs_batch_plan), its row of the table and its entry of the order
        total += 8.0 * ((double)LBK_BATCH_NVEC(m) * vs + np) + (double)sizeof(BatchState) +
                 (double)(sizeof(BatchRow) + sizeof(int));
        if (dense) total += 8.0 * (2.0 * vs + np) + 8.0 * np * np;  // t and gt, b, the matrix
    }
    if (bytes) *bytes = total;
    return 0;
}

int lbfgs_batch_plan(int64_t n, int m, int batch, double* bytes) {
    if (n < 1 || n > LBK_BATCH_NMAX || m < 1 || m > LBK_SMALL_HMAX || batch < 1) return LBFGS_ERR_BAD_ARG;
    if (bytes)
        *bytes = (double)batch * (8.0 * ((double)LBK_BATCH_NVEC(m) * (double)batch_vstride(n) + (double)n) +
                                  (double)sizeof(BatchState));
    return 0;
}

int lbfgs_batch_dense_plan(int64_t n, int m, int batch, int shared_A, double* bytes) {
    double base = 0.0;
    if (n > LBK_BATCH_DENSE_NMAX || lbfgs_batch_plan(n, m, batch, &base) != 0) return LBFGS_ERR_BAD_ARG;
    if (bytes)  // the batch, then t and gt and b per problem, then the matrices
        *bytes = base + (double)batch * 8.0 * (2.0 * (double)batch_vstride(n) + (double)n) +
                 (shared_A ? 1.0 : (double)batch) * 8.0 * (double)n * (double)n;
    return 0;
}

void lbfgs_batch_destroy(lbfgs_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->vecs) (void)hipFree(b->vecs);
    if (b->xio) (void)hipFree(b->xio);
    if (b->st) (void)hipFree(b->st);
    if (b->running) (void)hipFree(b->running);
    if (b->tr) (void)hipFree(b->tr);
    if (b->dq_A) (void)hipFree(b->dq_A);
    if (b->dq_b) (void)hipFree(b->dq_b);
    if (b->dq_x) (void)hipFree(b->dq_x);
    if (b->cb_x) (void)hipFree(b->cb_x);
    if (b->cb_F) (void)hipFree(b->cb_F);
    if (b->cb_flags) (void)hipFree(b->cb_flags);
    if (b->cb_rec) (void)hipFree(b->cb_rec);
    if (b->cb_evals) (void)hipFree(b->cb_evals);
    if (b->tab) (void)hipFree(b->tab);
    if (b->order) (void)hipFree(b->order);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

}  // extern "C"

// both creators: n the size (a ragged batch: the largest), sizes the n_p of a ragged batch or null
static int batch_create(lbfgs_batch** out, int64_t n, const int64_t* sizes, int m, int batch, int device) {
    lbk_geo G;
    if (lbk_geometry_plan(n, 0, 1, &G) != 0 || G.L != 512 || G.nseg > LBK_BATCH_SEGMAX) return LBFGS_ERR_BAD_ARG;
    lbfgs_batch* b = new (std::nothrow) lbfgs_batch();
    if (!b) return LBFGS_ERR_NOMEM;
    b->n = n;
    b->m = m;
    b->B = batch;
    b->device = device;
    b->vstride = batch_vstride(n);
    b->pstride = b->vstride * LBK_BATCH_NVEC(m);
    std::vector<BatchRow> rows;
    std::vector<int> order;
    if (sizes) {
        b->ragged = true;
        b->np.assign(sizes, sizes + batch);
        b->off.assign((size_t)batch + 1, 0);
        b->off2.assign((size_t)batch + 1, 0);
        b->vsum.assign((size_t)batch + 1, 0);
        rows.resize((size_t)batch);
        for (int p = 0; p < batch; ++p) {
            const int64_t np = sizes[p], vs = batch_vstride(np);
            rows[(size_t)p] = {np, b->vsum[(size_t)p] * LBK_BATCH_NVEC(m), vs, b->off[(size_t)p], b->off2[(size_t)p],
                               b->vsum[(size_t)p] * 2};
            b->off[(size_t)p + 1] = b->off[(size_t)p] + np;
            b->off2[(size_t)p + 1] = b->off2[(size_t)p] + np * np;
            b->vsum[(size_t)p + 1] = b->vsum[(size_t)p] + vs;
        }
        batch_order(b->np, order);
    }
    b->geo.n = n;
    b->geo.L = G.L;
    b->geo.nseg = G.nseg;
    b->geo.seg_lo = 0;
    b->geo.elem_lo = 0;
    b->geo.n_loc = n;
    b->geo.g_lo = 0;
    b->geo.g_hi = LBK_GROUPS;
    b->geo.spg = LBK_SEG_PER_GROUP;
    b->geo.rev = 0;
    b->geo.ppart = nullptr;
    b->geo.edge_slot = nullptr;
    hipDeviceProp_t prop;
    const size_t vbytes = sizeof(double) * (size_t)LBK_BATCH_NVEC(m) * (size_t)batch_sum_v(b);
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess ||
        hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void**)&b->vecs, vbytes) != hipSuccess ||
        hipMalloc((void**)&b->xio, sizeof(double) * (size_t)batch_sum_n(b)) != hipSuccess ||
        hipMalloc((void**)&b->st, sizeof(BatchState) * (size_t)batch) != hipSuccess ||
        hipMalloc((void**)&b->running, sizeof(int)) != hipSuccess ||
        // ghost cells and padding are zero and stay zero: no pass stores outside [0, n)
        hipMemsetAsync(b->vecs, 0, vbytes, b->stream) != hipSuccess ||
        hipMemsetAsync(b->st, 0, sizeof(BatchState) * (size_t)batch, b->stream) != hipSuccess ||
        // the table and the order of work, written once
        (sizes && (hipMalloc((void**)&b->tab, sizeof(BatchRow) * (size_t)batch) != hipSuccess ||
                   hipMalloc((void**)&b->order, sizeof(int) * (size_t)batch) != hipSuccess ||
                   hipMemcpyAsync(b->tab, rows.data(), sizeof(BatchRow) * (size_t)batch, hipMemcpyHostToDevice,
                                  b->stream) != hipSuccess ||
                   hipMemcpyAsync(b->order, order.data(), sizeof(int) * (size_t)batch, hipMemcpyHostToDevice,
                                  b->stream) != hipSuccess)) ||
        hipStreamSynchronize(b->stream) != hipSuccess) {
        (void)hipGetLastError();
        lbfgs_batch_destroy(b);
        return LBFGS_ERR_HIP;
    }
    b->cus = prop.multiProcessorCount;
    *out = b;
    return 0;
}

extern "C" {

int lbfgs_batch_create(lbfgs_batch** out, int64_t n, int m, int batch, int device) {
    if (!out) return LBFGS_ERR_BAD_ARG;
    *out = nullptr;
    if (lbfgs_batch_plan(n, m, batch, nullptr) != 0) return LBFGS_ERR_BAD_ARG;
    return batch_create(out, n, nullptr, m, batch, device);
}

int lbfgs_batch_create_ragged(lbfgs_batch** out, const int64_t* n, int m, int batch, int device) {
    if (!out) return LBFGS_ERR_BAD_ARG;
    *out = nullptr;
    if (lbfgs_batch_ragged_plan(n, batch, m, 0, nullptr) != 0) return LBFGS_ERR_BAD_ARG;
    return batch_create(out, *std::max_element(n, n + batch), n, m, batch, device);
}

int lbfgs_batch_sizes(const lbfgs_batch* b, int64_t* n_out, int64_t* offset_out) {
    if (!b) return LBFGS_ERR_BAD_ARG;
    for (int64_t p = 0; p < b->B; ++p) {
        if (n_out) n_out[p] = batch_np(b, p);
        if (offset_out) offset_out[p] = b->ragged ? b->off[(size_t)p] : p * b->n;
    }
    if (offset_out) offset_out[b->B] = batch_sum_n(b);
    return 0;
}

const char* lbfgs_batch_last_error(const lbfgs_batch* b) { return b ? b->err : "null batch"; }

int lbfgs_batch_set_launch(lbfgs_batch* b, int max_workgroups, int iters_per_launch) {
    if (!b || max_workgroups < 0 || iters_per_launch < 0) return LBFGS_ERR_BAD_ARG;
    b->max_wg = max_workgroups;
    b->iters = iters_per_launch;
    return 0;
}

int lbfgs_batch_set_dense_quadratics(lbfgs_batch* b, const double* A, int shared_A, const double* bvec) {
    if (!b) return LBFGS_ERR_BAD_ARG;
    b->err[0] = 0;
    if (!A || !bvec || batch_any_over(b, LBK_BATCH_DENSE_NMAX)) {
        snprintf(b->err, sizeof b->err, "lbfgs_batch_set_dense_quadratics: A and b, and a batch of n <= %d",
                 LBK_BATCH_DENSE_NMAX);
        return LBFGS_ERR_BAD_ARG;
    }
    if (b->ragged && shared_A) {
        snprintf(b->err, sizeof b->err, "lbfgs_batch_set_dense_quadratics: one shared A needs problems of one size, "
                 "not a ragged batch");
        return LBFGS_ERR_BAD_ARG;
    }
    BHIP(b, hipSetDevice(b->device));
    const size_t nn = (size_t)b->n * (size_t)b->n, B = (size_t)b->B;
    const size_t a_doubles = b->ragged ? (size_t)b->off2[B] : shared_A ? nn : nn * B;
    const size_t b_doubles = (size_t)batch_sum_n(b);
    b->dq_set = false;
    b->dq_ref = false;  // a caller's buffers are referenced no longer
    b->ref_A = b->ref_b = nullptr;
    bool ok = true;
    if (!b->dq_b) ok = hipMalloc((void**)&b->dq_b, sizeof(double) * b_doubles) == hipSuccess;
    if (ok) {
        const int rc = batch_dense_scratch(b, "lbfgs_batch_set_dense_quadratics");
        if (rc != 0) return rc;
    }
    if (ok && b->dq_A_doubles < a_doubles) {
        if (b->dq_A) (void)hipFree(b->dq_A);
        b->dq_A = nullptr;
        b->dq_A_doubles = 0;
        ok = hipMalloc((void**)&b->dq_A, sizeof(double) * a_doubles) == hipSuccess;
        if (ok) b->dq_A_doubles = a_doubles;
    }
    if (!ok) {  // the batch stays usable for the stencil objectives
        (void)hipGetLastError();
        snprintf(b->err, sizeof b->err, "lbfgs_batch_set_dense_quadratics: out of device memory");
        return LBFGS_ERR_NOMEM;
    }
    BHIP(b, hipMemcpyAsync(b->dq_A, A, sizeof(double) * a_doubles, hipMemcpyHostToDevice, b->stream));
    BHIP(b, hipMemcpyAsync(b->dq_b, bvec, sizeof(double) * b_doubles, hipMemcpyHostToDevice, b->stream));
    BHIP(b, hipStreamSynchronize(b->stream));
    b->dq_shared = shared_A != 0;
    b->dq_set = true;
    return 0;
}

int lbfgs_batch_set_dense_quadratics_device(lbfgs_batch* b, const double* A_dev, int64_t a_batch_stride, int64_t lda,
                                            const double* b_dev, int64_t ldb) {
    if (!b) return LBFGS_ERR_BAD_ARG;
    b->err[0] = 0;
    const int64_t n = b->n;  // a ragged batch: the largest n_p
    const char* bad = nullptr;
    const bool a_packed = a_batch_stride == LBFGS_BATCH_PACKED || lda == LBFGS_BATCH_PACKED;
    if (batch_any_over(b, LBK_BATCH_DENSE_NMAX))
        bad = "a batch of n <= 4096";
    else if (!A_dev || !b_dev)
        bad = "A_dev and b_dev";
    else if (!b->ragged && (a_packed || ldb == LBFGS_BATCH_PACKED))
        bad = "LBFGS_BATCH_PACKED is a stride of ragged batches only";
    else if (a_packed && !(a_batch_stride == LBFGS_BATCH_PACKED && lda == LBFGS_BATCH_PACKED))
        bad = "a_batch_stride and lda both strides or both LBFGS_BATCH_PACKED";
    else if (b->ragged && ((!a_packed && a_batch_stride == 0) || ldb == 0))
        bad = "a ragged batch has no shared A or b: a_batch_stride and ldb not 0";
    else if (!a_packed && lda < n)
        bad = "lda >= n";
    else if (!a_packed && a_batch_stride != 0 && a_batch_stride < (n - 1) * lda + n)
        bad = "a_batch_stride >= (n - 1) * lda + n, or 0 for one shared matrix";
    if (!bad && ldb != LBFGS_BATCH_PACKED && ldb != 0 && ldb < n) bad = "ldb >= n, or 0 for one shared b";
    if (!bad) {
        BHIP(b, hipSetDevice(b->device));
        if (!batch_caller_range(b, A_dev, batch_aspan(b, a_batch_stride, lda)) ||
            !batch_caller_range(b, b_dev, batch_xspan(b, ldb)))
            bad = "A_dev and b_dev 8-byte aligned in device memory of the batch's device (not pinned host, not managed)";
    }
    if (bad) {  // the data set before, if any, stay as they are
        snprintf(b->err, sizeof b->err, "lbfgs_batch_set_dense_quadratics_device: %s", bad);
        return LBFGS_ERR_BAD_ARG;
    }
    b->dq_set = false;
    const int rc = batch_dense_scratch(b, "lbfgs_batch_set_dense_quadratics_device");
    if (rc != 0) return rc;
    // the batch's own copies of an earlier host-form call are released: nothing holds a second A
    BHIP(b, hipStreamSynchronize(b->stream));
    if (b->dq_A) (void)hipFree(b->dq_A);
    if (b->dq_b) (void)hipFree(b->dq_b);
    b->dq_A = b->dq_b = nullptr;
    b->dq_A_doubles = 0;
    b->ref_A = A_dev;
    b->ref_b = b_dev;
    b->ref_astride = a_batch_stride;
    b->ref_lda = lda;
    b->ref_ldb = ldb;
    b->dq_ref = true;
    b->dq_set = true;
    return 0;
}

int lbfgs_batch_set_device_objective(lbfgs_batch* b, const lbfgs_batch_device_fn* fn) {
    if (!b) return LBFGS_ERR_BAD_ARG;
    b->err[0] = 0;
    if (!fn) {  // cleared; the buffers stay for a later call
        b->cb_set = false;
        b->cb.eval = nullptr;
        return 0;
    }
    const char* bad = nullptr;
    if (b->ragged)
        bad = "a uniform batch (problems of one size), not a ragged one";
    else if (!fn->eval)
        bad = "eval";
    else if (fn->flags != 0)
        bad = "flags 0";
    if (bad) {  // the objective set before, if any, stays as it is
        snprintf(b->err, sizeof b->err, "lbfgs_batch_set_device_objective: %s", bad);
        return LBFGS_ERR_BAD_ARG;
    }
    if (!b->cb_rec) {
        BHIP(b, hipSetDevice(b->device));
        const size_t B = (size_t)b->B, xbytes = sizeof(double) * 2 * (size_t)batch_sum_v(b);
        double *x = nullptr, *F = nullptr;
        int* fl = nullptr;
        BatchExtRec* rec = nullptr;
        long long* ev = nullptr;
        // ghost cells and padding of Z and GT are zero and stay zero, as the batch's other vectors'
        if (hipMalloc((void**)&x, xbytes) != hipSuccess || hipMalloc((void**)&F, sizeof(double) * B) != hipSuccess ||
            hipMalloc((void**)&fl, sizeof(int) * (B + 2)) != hipSuccess ||
            hipMalloc((void**)&rec, sizeof(BatchExtRec) * B) != hipSuccess ||
            hipMalloc((void**)&ev, sizeof(long long) * B) != hipSuccess ||
            hipMemsetAsync(x, 0, xbytes, b->stream) != hipSuccess ||
            hipMemsetAsync(F, 0, sizeof(double) * B, b->stream) != hipSuccess ||
            hipMemsetAsync(rec, 0, sizeof(BatchExtRec) * B, b->stream) != hipSuccess ||
            hipMemsetAsync(ev, 0, sizeof(long long) * B, b->stream) != hipSuccess ||
            hipStreamSynchronize(b->stream) != hipSuccess) {  // the batch stays usable for its other objectives
            (void)hipGetLastError();
            if (x) (void)hipFree(x);
            if (F) (void)hipFree(F);
            if (fl) (void)hipFree(fl);
            if (rec) (void)hipFree(rec);
            if (ev) (void)hipFree(ev);
            snprintf(b->err, sizeof b->err, "lbfgs_batch_set_device_objective: out of device memory");
            return LBFGS_ERR_NOMEM;
        }
        b->cb_x = x;
        b->cb_F = F;
        b->cb_flags = fl;
        b->cb_rec = rec;
        b->cb_evals = ev;
    }
    b->cb = *fn;
    b->cb_set = true;
    return 0;
}

}  // extern "C"

// The rounds of a solve with the caller's objective: launch, synchronise, one call of eval for all
// waiting problems, launch again, until no problem waits (then none is running: a launch leaves a
// problem waiting or finished). The rounds are bounded by what the searches can ask for.
static int batch_ext_rounds(lbfgs_batch* b, const char* who, BatchArgs& a, const BatchExtArgs& xa, const void* kern,
                            int grid, void** kargs, int max_iterations, long long* launches) {
    // an iteration's evaluations: its search's trials (20 of interpolation and Wolfe, 4096 of
    // backtracking-Wolfe here, backtracking's own count of steps down to its tolerance where that
    // is more) and the commit's two; the solve's: those of max_iterations iterations, and x0's
    double per_iter = (double)LBK_BATCH_BTW_CAP;
    if (a.K.backtracking_alpha > 0 && a.K.backtracking_alpha < 1 && a.K.backtracking_tol > 0 && a.K.initial_step > 0)
        per_iter = std::max(per_iter, std::ceil(std::log(a.K.backtracking_tol / a.K.initial_step) /
                                                std::log(a.K.backtracking_alpha)) + 1.0);
    const double bound = 1.0 + ((double)max_iterations + 1.0) * (per_iter + 2.0);
    const long long max_rounds = bound < 9e18 ? (long long)bound : LLONG_MAX;
    const int64_t ld = 2 * b->vstride;
    for (;;) {
        int flags[2] = {0, 0};  // running, waiting
        BHIP(b, hipMemsetAsync(b->cb_flags, 0, sizeof(int) * ((size_t)b->B + 2), b->stream));
        BHIP(b, hipLaunchKernel(kern, dim3(grid), dim3(LB_BLOCK), kargs, 0, b->stream));
        BHIP(b, hipMemcpyAsync(flags, b->cb_flags, sizeof flags, hipMemcpyDeviceToHost, b->stream));
        BHIP(b, hipStreamSynchronize(b->stream));  // eval's ordering: everything that formed Z is complete
        a.init = 0;
        ++*launches;
        if (flags[1] == 0) {
            if (flags[0]) {  // cannot happen: a running problem waits
                snprintf(b->err, sizeof b->err, "%s: problems running but none waiting", who);
                return LBFGS_ERR_STATE;
            }
            return 0;
        }
        if (*launches > max_rounds) {
            snprintf(b->err, sizeof b->err, "%s: problems unfinished after %lld rounds", who, *launches);
            return LBFGS_ERR_STATE;
        }
        const int rc = b->cb.eval(xa.zbase, ld, b->cb_F, xa.zbase + b->vstride, ld, xa.active, flags[1], b->B, b->n,
                                  b->cb.user);
        BHIP(b, hipSetDevice(b->device));  // the callback may have left another device current
        if (rc != 0) {
            snprintf(b->err, sizeof b->err, "%s: device objective callback returned %d", who, rc);
            return LBFGS_ERR_CALLBACK;
        }
    }
}

// Both forms of lbfgs_batch_minimize: x0 is read at xin + p * ldxin and x written at xout + p * ldxout,
// device memory both. x0_host / x_out_host (the host form only) are copied to and from the batch's
// own xio around the launches; no hipMemcpy ever touches a caller's device buffer.
static int batch_solve(lbfgs_batch* b, const char* who, int objective, int line_search, const lbfgs_constants* k,
                       const double* xin, int64_t ldxin, double* xout, int64_t ldxout, const double* x0_host,
                       double* x_out_host, int max_iterations, double tolerance, unsigned flags, lbfgs_result* out) {
    const bool dense = objective == LBFGS_OBJ_DENSE_QUAD && b->dq_set;
    const bool ext = objective == LBFGS_OBJ_DEVICE && b->cb_set && b->cb.eval && !b->ragged;
    if ((!dense && !ext && (objective < LBFGS_OBJ_ROSENBROCK || objective > LBFGS_OBJ_QUAD_SEPARABLE)) ||
        line_search < LBFGS_LS_BACKTRACKING || line_search > LBFGS_LS_BACKTRACKING_WOLFE || max_iterations < 0 ||
        (flags & ~(LBFGS_FLAG_TRACE | LBFGS_FLAG_QUIET)) != 0) {
        snprintf(b->err, sizeof b->err, "%s: device stencil objectives (the dense quadratic once "
                 "its data is set, LBFGS_OBJ_DEVICE once lbfgs_batch_set_device_objective has set one), the four "
                 "line searches, LBFGS_FLAG_TRACE / LBFGS_FLAG_QUIET only", who);
        return LBFGS_ERR_BAD_ARG;
    }
    const auto t0 = std::chrono::steady_clock::now();
    BHIP(b, hipSetDevice(b->device));
    b->solved = false;
    const bool trace = (flags & LBFGS_FLAG_TRACE) != 0;
    const int tr_cap = max_iterations + 1;  // one entry per iteration's top, one at the exit
    if (trace && (!b->tr || b->tr_cap < tr_cap)) {
        if (b->tr) BHIP(b, hipFree(b->tr));
        b->tr = nullptr;
        BHIP(b, hipMalloc((void**)&b->tr, sizeof(double) * 3 * (size_t)tr_cap * (size_t)b->B));
        b->tr_cap = tr_cap;
    }
    BatchArgs a;
    memset(&a, 0, sizeof a);
    a.B = b->B;
    a.m = b->m;
    a.iters = b->iters > 0 ? b->iters : LBK_BATCH_ITERS;
    a.max_iterations = max_iterations;
    a.trace = trace;
    a.init = 1;
    a.tr_cap = trace ? b->tr_cap : 0;
    a.vstride = b->vstride;
    a.pstride = b->pstride;
    a.base = b->vecs + LBK_FRONT;
    a.xin = xin;
    a.ldxin = ldxin;
    a.xout = xout;
    a.ldxout = ldxout;
    a.st = b->st;
    a.tr = trace ? b->tr : nullptr;
    a.running = b->running;
    a.tol = tolerance;
    if (k)
        a.K = *k;
    else
        lbfgs_constants_default(&a.K);
    BatchDenseArgs dq;
    memset(&dq, 0, sizeof dq);
    if (dense) {
        dq.A = b->dq_ref ? b->ref_A : b->dq_A;
        dq.b = b->dq_ref ? b->ref_b : b->dq_b;
        dq.xbase = b->dq_x + LBK_FRONT;
        dq.astride = b->dq_ref ? b->ref_astride : b->dq_shared ? 0 : b->n * b->n;
        dq.lda = b->dq_ref ? b->ref_lda : b->n;
        dq.ldb = b->dq_ref ? b->ref_ldb : b->n;
        if (b->ragged && !b->dq_ref) dq.astride = dq.lda = dq.ldb = LBFGS_BATCH_PACKED;  // the batch's own copies
    }
    BatchExtArgs xa;
    memset(&xa, 0, sizeof xa);
    if (ext) {
        xa.zbase = b->cb_x + LBK_FRONT;
        xa.F = b->cb_F;
        xa.nactive = b->cb_flags + 1;
        xa.active = b->cb_flags + 2;
        xa.rec = b->cb_rec;
        xa.evals = b->cb_evals;
        a.running = b->cb_flags;  // running and the count of waiting problems come back in one copy
    }
    BatchRagged rg = {b->tab, nullptr};
    // the one kernel of this solve and its arguments
    const void* const kern = ext     ? batch_ext_kernel(line_search)
                             : dense ? batch_dense_kernel(line_search, b->ragged)
                                     : batch_kernel(objective, line_search, b->ragged);
    void* args_stencil[] = {&a, &b->geo, &rg};     // rg: the ragged kernels' last argument; a uniform batch's
    void* args_dense[] = {&a, &dq, &b->geo, &rg};  // kernels have none, and the entry is not read
    void* args_ext[] = {&a, &xa, &b->geo};
    void** const kargs = ext ? args_ext : dense ? args_dense : args_stencil;
    int grid = b->max_wg;
    if (grid <= 0) {  // every workgroup resident: occupancy x CUs
        int per_cu = 0;
        BHIP(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, LB_BLOCK, 0));
        grid = std::max(1, per_cu) * std::max(1, b->cus);
    }
    grid = std::min(grid, b->B);
    // the order of work balances workgroups that take several problems each; with one problem each
    // there is nothing to balance, and the problems stay where their index puts them
    // (the table's order, of ragged batches: the kernels of a uniform batch, k_batch_solve_ext among
    // them, have no such argument and take their problems by index)
    if (grid < b->B) rg.order = b->order;
    auto launch = [&] { return hipLaunchKernel(kern, dim3(grid), dim3(LB_BLOCK), kargs, 0, b->stream); };
    // x0 up (one contiguous copy; each workgroup moves its problem's x0 into the vector layout)
    if (x0_host)
        BHIP(b, hipMemcpyAsync(b->xio, x0_host, sizeof(double) * (size_t)batch_sum_n(b), hipMemcpyHostToDevice,
                               b->stream));
    long long launches = 0;
    if (ext) {
        const int rc = batch_ext_rounds(b, who, a, xa, kern, grid, kargs, max_iterations, &launches);
        if (rc != 0) return rc;
    } else {
        // every launch takes each unfinished problem at least one iteration further, or ends it
        const long long max_launches = (long long)max_iterations / a.iters + 2;
        for (;;) {
            int running = 0;
            BHIP(b, hipMemsetAsync(b->running, 0, sizeof(int), b->stream));
            BHIP(b, launch());
            BHIP(b, hipMemcpyAsync(&running, b->running, sizeof(int), hipMemcpyDeviceToHost, b->stream));
            BHIP(b, hipStreamSynchronize(b->stream));
            a.init = 0;
            ++launches;
            if (!running) break;
            if (launches >= max_launches) {
                snprintf(b->err, sizeof b->err, "%s: problems unfinished after %lld launches", who, launches);
                return LBFGS_ERR_STATE;
            }
        }
    }
    b->hst.resize((size_t)b->B);
    BHIP(b, hipMemcpyAsync(b->hst.data(), b->st, sizeof(BatchState) * (size_t)b->B, hipMemcpyDeviceToHost, b->stream));
    if (ext) {  // the rounds each problem was active in
        b->hevals.resize((size_t)b->B);
        BHIP(b, hipMemcpyAsync(b->hevals.data(), b->cb_evals, sizeof(long long) * (size_t)b->B, hipMemcpyDeviceToHost,
                               b->stream));
    }
    if (x_out_host)
        BHIP(b, hipMemcpyAsync(x_out_host, b->xio, sizeof(double) * (size_t)batch_sum_n(b), hipMemcpyDeviceToHost,
                               b->stream));
    b->htr_cap = 0;
    if (trace) {
        b->htr.resize(3 * (size_t)b->tr_cap * (size_t)b->B);
        BHIP(b, hipMemcpyAsync(b->htr.data(), b->tr, sizeof(double) * b->htr.size(), hipMemcpyDeviceToHost, b->stream));
        b->htr_cap = b->tr_cap;
    }
    BHIP(b, hipStreamSynchronize(b->stream));
    b->solved = true;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (out)
        for (int p = 0; p < b->B; ++p) {
            const BatchState& s = b->hst[(size_t)p];
            lbfgs_result& r = out[p];
            memset(&r, 0, sizeof r);
            r.iterations = s.k;
            r.status = s.status;
            r.f = s.f_cur;
            r.gnorm = sqrt(s.gg);
            r.trials_f = s.trials_f;
            r.trials_fg = s.trials_fg;
            r.commits = s.commits;
            r.passes = launches;
            r.bytes = s.vecs * 8.0 * (double)batch_np(b, p);
            r.seconds = secs;
            r.h_min = s.h_min;
            r.h_max = s.h_min < 0 ? -1 : s.h_max;
            if (ext) r.f_calls = r.grad_calls = b->hevals[(size_t)p];
        }
    return 0;
}

extern "C" {

int lbfgs_batch_minimize(lbfgs_batch* b, int objective, int line_search, const lbfgs_constants* k,
                         const double* x0_host, double* x_out_host, int max_iterations, double tolerance,
                         unsigned flags, lbfgs_result* out) {
    if (!b) return LBFGS_ERR_BAD_ARG;
    b->err[0] = 0;
    if (!x0_host) {
        snprintf(b->err, sizeof b->err, "lbfgs_batch_minimize: x0_host");
        return LBFGS_ERR_BAD_ARG;
    }
    const int64_t ld = b->ragged ? LBFGS_BATCH_PACKED : b->n;  // the batch's own rows
    return batch_solve(b, "lbfgs_batch_minimize", objective, line_search, k, b->xio, ld, b->xio, ld, x0_host,
                       x_out_host, max_iterations, tolerance, flags, out);
}

int lbfgs_batch_minimize_device(lbfgs_batch* b, int objective, int line_search, const lbfgs_constants* k,
                                const double* x0_dev, int64_t ldx0, double* x_out_dev, int64_t ldx, int max_iterations,
                                double tolerance, unsigned flags, lbfgs_result* out) {
    if (!b) return LBFGS_ERR_BAD_ARG;
    b->err[0] = 0;
    const int64_t n = b->n;  // a ragged batch: the largest n_p
    const char* bad = nullptr;
    const bool packed0 = ldx0 == LBFGS_BATCH_PACKED, packed = x_out_dev && ldx == LBFGS_BATCH_PACKED;
    if (!x0_dev)
        bad = "x0_dev";
    else if (!b->ragged && (packed0 || packed))
        bad = "LBFGS_BATCH_PACKED is a stride of ragged batches only";
    else if (b->ragged && ldx0 == 0)
        bad = "a ragged batch has no x0 shared by every problem: ldx0 >= the largest n, or LBFGS_BATCH_PACKED";
    else if (!packed0 && ldx0 != 0 && ldx0 < n)
        bad = "ldx0 >= n, or 0 for one x0 shared by every problem";
    else if (x_out_dev && !packed && ldx < n)
        bad = "ldx >= n";
    const int64_t span0 = bad ? 0 : batch_xspan(b, ldx0), span = bad || !x_out_dev ? 0 : batch_xspan(b, ldx);
    if (!bad) {
        BHIP(b, hipSetDevice(b->device));
        if (!batch_caller_range(b, x0_dev, span0) || (x_out_dev && !batch_caller_range(b, x_out_dev, span)))
            bad = "x0_dev and x_out_dev 8-byte aligned in device memory of the batch's device (not pinned host, not "
                  "managed)";
    }
    if (!bad && x_out_dev) {
        // in place (the same rows: a problem's row is read at its entry and written at its exit by
        // the same workgroup) or disjoint from x0; disjoint from the A and b the batch refers to
        const bool in_place = x_out_dev == x0_dev && ldx == ldx0;
        if (!in_place && batch_overlap(x_out_dev, span, x0_dev, span0))
            bad = "x_out_dev either x0_dev itself with ldx == ldx0 >= n or not overlapping it";
        else if (b->dq_set && b->dq_ref &&
                 (batch_overlap(x_out_dev, span, b->ref_A, batch_aspan(b, b->ref_astride, b->ref_lda)) ||
                  batch_overlap(x_out_dev, span, b->ref_b, batch_xspan(b, b->ref_ldb))))
            bad = "x_out_dev not overlapping the A and b set by lbfgs_batch_set_dense_quadratics_device";
    }
    if (bad) {
        snprintf(b->err, sizeof b->err, "lbfgs_batch_minimize_device: %s", bad);
        return LBFGS_ERR_BAD_ARG;
    }
    // without x_out_dev the kernel's x goes to the batch's own rows
    return batch_solve(b, "lbfgs_batch_minimize_device", objective, line_search, k, x0_dev, ldx0,
                       x_out_dev ? x_out_dev : b->xio, x_out_dev ? ldx : b->ragged ? LBFGS_BATCH_PACKED : n, nullptr,
                       nullptr, max_iterations, tolerance,
                       flags, out);
}

int lbfgs_batch_trace_len(const lbfgs_batch* b, int problem) {
    if (!b || problem < 0 || problem >= b->B) return LBFGS_ERR_BAD_ARG;
    if (!b->solved || !b->htr_cap) return 0;
    return std::min(b->hst[(size_t)problem].tr_len, b->htr_cap);
}

int lbfgs_batch_trace_get(const lbfgs_batch* b, int problem, double* f, double* gnorm, double* alpha, int cap) {
    const int len = lbfgs_batch_trace_len(b, problem);
    if (len < 0) return len;
    const int kk = len < cap ? len : cap;
    const double* base = len ? b->htr.data() + 3 * (size_t)b->htr_cap * (size_t)problem : nullptr;
    for (int i = 0; i < kk; ++i) {
        if (f) f[i] = base[i];
        if (gnorm) gnorm[i] = base[b->htr_cap + i];
        if (alpha) alpha[i] = base[2 * (size_t)b->htr_cap + i];
    }
    return kk < 0 ? 0 : kk;
}

int lbfgs_batch_events_get(const lbfgs_batch* b, int problem, lbfgs_batch_events* out) {
    if (!b || !out || problem < 0 || problem >= b->B || !b->solved) return LBFGS_ERR_BAD_ARG;
    const BatchState& s = b->hst[(size_t)problem];
    out->not_descent = s.ev[0];
    out->skipped_updates = s.ev[1];
    out->invalid_rho = s.ev[2];
    out->invalid_gamma = s.ev[3];
    return 0;
}

}  // extern "C"
