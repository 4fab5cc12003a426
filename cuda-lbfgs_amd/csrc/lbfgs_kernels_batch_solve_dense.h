// lbfgs_kernels_batch_solve_dense.h - the body of k_batch_solve_dense and k_batch_solve_dense_ragged
// (lbfgs_kernels_batch.hip), included once in each. The two kernels are one text and differ in their
// argument lists alone: a uniform batch's kernel keeps the arguments it always had, and with them its
// code; a ragged batch's takes the table as well. In scope where this is included: a, dq, geo_b,
// constexpr bool RAGGED, and rg (the BatchRagged; nulls, never read, in the uniform kernel).
// NOT a stand-alone header: no include guard, no declarations of its own; it is the statements of a
// __global__ function and is included inside one, nowhere else.
    __shared__ BatchDenseLds LD;
    BatchLds& L = LD.L;
    const int t = threadIdx.x;
    BatchWave& W = L.wv[t >> 6];
    DenseWave& D = LD.dw[t >> 6];
    BatchState& S = W.st;
    lbk_search& s = W.s;
    for (int i = blockIdx.x; i < a.B; i += gridDim.x) {
        const BatchProb P = batch_prob<RAGGED>(rg, i);
        const int p = P.p;
        const Geo geo = batch_geo<RAGGED>(geo_b, P);
        const int64_t n = geo.n;
        const BatchView V = batch_view<RAGGED>(a, P);
        double* const d = V.d();
        // a ragged batch's packed A (astride == LBFGS_BATCH_PACKED): problem p's at its packed offset, rows n apart
        const bool a_packed = RAGGED && dq.astride < 0;
        const double* const Ap = dq.A + (a_packed ? batch_row_ld(&P.row->off2) : (int64_t)p * dq.astride);
        const int64_t lda_p = a_packed ? n : dq.lda;
        // The uniform kernel spells the addresses of b, t and gt and the row stride as it always did (the
        // RAGGED ? ... : ... below; batch_row_at, lda_p and V.vstride are the same values there): with
        // the shorter spelling the compiler allocates the uniform dense kernels' registers differently,
        // and their code has to stay instruction for instruction what it was.
        const double* const bp = dq.b + (RAGGED ? batch_row_at<RAGGED>(P, dq.ldb) : (int64_t)p * dq.ldb);
        double* const tv = dq.xbase + (RAGGED ? batch_row_ld(&P.row->xbase) : (int64_t)p * 2 * a.vstride);
        double* const gt = tv + (RAGGED ? V.vstride : a.vstride);
        // lbk_dense_eval: the rows at z with the gradient into gout, then f (and gout . gout) from the terms
        auto eval = [&](const double* z, double* gout, double (&t2)[2]) {
            dense_rows(Ap, bp, z, gout, tv, n, RAGGED ? lda_p : dq.lda);
            batch_pass<2>(OpTermsDot<false>{tv, gout}, geo, L, t2);
            S.vecs += (double)n + 5.0;
        };
        if (batch_enter<RAGGED>(a, V, P, n, S)) continue;
        if (a.init) {  // f, g and g.g at x0
            double t2[2];
            eval(V.vec(0), V.vec(1), t2);
            S.f_cur = t2[0];
            S.gg = t2[1];
        }

        for (int it = 0; it < a.iters; ++it) {
            BatchIter I;
            if (batch_iter_top(a, V, S, I)) break;
            batch_direction(V, I, geo, L, S, W);

            // ---- d into its buffer, g . d that pass's total; a direction that is no descent
            // direction gives way to -g, materialised again (once) ----
            double gd;
            for (bool fell_back = false;;) {
                gd = batch_materialise_d(V, I, geo, L, S, W);
                if (!(gd >= 0) || fell_back) break;
                S.ev[0]++;
                W.dmode = LBK_D_NEG_G;
                fell_back = true;
            }
            D.hz_valid = D.hf_valid = D.gt_valid = 0;  // host_invalidate: nothing cached refers to this x, d

            auto point = [&](double alpha) {  // host_point_issue
                if (D.hz_valid && D.hz_alpha == alpha) return;
                dense_point(I.xn, I.x, d, alpha, n);
                S.vecs += 3.0;
                D.hz_valid = 1;
                D.hz_alpha = alpha;
                D.hf_valid = 0;
            };
            // one evaluation at z(alpha) with the gradient into dst: f is cached with it, and the
            // gradient when dst is gt (host_g_at's dense branch; host_f_at's is this with dst = gt)
            auto eval_at = [&](double alpha, double* dst) {
                point(alpha);
                double t2[2];
                eval(I.xn, dst, t2);
                D.hf_valid = 1;
                D.hf_alpha = alpha;
                D.hf_val = t2[0];
                if (dst == gt) {
                    D.gt_valid = 1;
                    D.gt_alpha = alpha;
                } else if (D.gt_valid && D.gt_alpha == alpha) {
                    D.gt_valid = 0;
                }
            };
            auto f_at = [&](double alpha) -> double {  // host_f_at
                if (!(D.hf_valid && D.hf_alpha == alpha && D.hz_valid && D.hz_alpha == alpha)) eval_at(alpha, gt);
                return D.hf_val;
            };
            auto g_at = [&](double alpha, double* dst) {  // host_g_at
                if (D.gt_valid && D.gt_alpha == alpha) {
                    if (dst != gt) {
                        for (int64_t i = t; i < n; i += LB_BLOCK) dst[i] = gt[i];
                        batch_stage_sync();
                        S.vecs += 2.0;
                    }
                    return;
                }
                eval_at(alpha, dst);
            };

            // ---- the line search, from the top, nothing cached (no first trial rode a commit) ----
            batch_search_begin(a, S, s, gd);
            W.capped = W.passes = 0;
            // lbfgs_driver.c trial() for an external objective: one step per call, f from its cache or
            // an evaluation, with need_g the gradient in gt and gt . d; the backtracking-Wolfe search
            // asks for the gradient before f (line_search.cpp:39-42)
            auto trial = [&](double alpha, bool need_g, double& f, double& dphi) -> bool {
                if (LS == 3 && W.passes >= LBK_BATCH_BTW_CAP) {  // the reference's loop has no bound of its own
                    W.capped = 1;
                    return false;
                }
                W.passes++;
                const bool g_first = need_g && LS == 3;
                // (a loop of two steps, not unrolled, so that f_at and g_at are inlined once each)
#pragma unroll 1
                for (int step = 0; step < 2; ++step) {
                    if ((step == 0) == g_first) {
                        if (need_g) g_at(alpha, gt);
                    } else {
                        f = f_at(alpha);
                    }
                }
                if (need_g) {
                    double t1[1];
                    batch_pass<1>(OpDot<false>{gt, d}, geo, L, t1);
                    S.vecs += 2.0;
                    dphi = t1[0];
                    S.trials_fg++;
                } else {
                    S.trials_f++;
                }
                return true;
            };
            search_loop<LS>(s, trial);
            if (W.capped || !s.done) {
                S.status = LBFGS_ERR_STATE;
                break;
            }
            const double alpha = s.step;
            batch_trace_step(a, V, S, alpha);

            // ---- commit (lbfgs_driver.c commit(), ext_obj): f at the step, then - unless the step
            // failed - the gradient at the step into gn, and the commit pass that reads it ----
            const double f_new = f_at(alpha);
            S.f_cur = f_new;
            if (alpha < 1e-10) {
                S.status = LBFGS_STATUS_LS_FAILED;
                break;
            }
            g_at(alpha, I.gn);
            batch_pass<7>(OpCommit<LBK_OBJ_NONE, LBK_D_BUF, false, false>{I.x, batch_buf_args(V, I), alpha, I.xn, I.gn,
                                                                          I.so, I.yo, n, n, 0.0},
                          geo, L, W.tot);
            W.tot[LBK_C_F] = f_new;
            S.vecs += 7.0;
            S.commits++;
            batch_accept(a.m, S, W);
        }
        batch_leave<RAGGED>(a, V, P, n, S);
    }
