// lbfgs_kernels_batch_solve_ext.h - the body of k_batch_solve_ext (lbfgs_kernels_batch.hip): the
// dense kernel (lbfgs_kernels_batch_solve_dense.h) with the evaluation taken out. Where that kernel
// evaluates, this one writes the point into the problem's Z row, records what it waits for, stores
// its state and goes to its next problem; the host evaluates every waiting problem with one call of
// the caller's function (f into F[p], the gradient into the GT row) and launches again. Nothing here
// waits: a launch takes every unfinished problem to its next evaluation or to its end.
// In scope where this is included: a, xa (the BatchExtArgs), geo_b. Uniform batches only.
// NOT a stand-alone header: the statements of a __global__ function, included inside one.
    __shared__ BatchExtLds LE;
    BatchLds& L = LE.L;
    const int t = threadIdx.x;
    BatchWave& W = L.wv[t >> 6];
    BatchExtRec& X = LE.xr[t >> 6];
    BatchState& S = W.st;
    lbk_search& s = X.s;
    const BatchRagged rg = {nullptr, nullptr};
    for (int i = blockIdx.x; i < a.B; i += gridDim.x) {
        const BatchProb P = batch_prob<false>(rg, i);
        const int p = P.p;
        const Geo geo = batch_geo<false>(geo_b, P);
        const int64_t n = geo.n;
        const BatchView V = batch_view<false>(a, P);
        double* const d = V.d();
        double* const z = xa.zbase + (int64_t)p * 2 * a.vstride;  // the point row; [0, n) only is ever written
        double* const gt = z + a.vstride;                         // the gradient row, the caller's to write
        if (batch_enter<false>(a, V, P, n, S)) continue;

        auto copy = [&](double* dst, const double* src) {  // lbk_copy, [0, n) only
            int tt = threadIdx.x;
            asm volatile("" : "+v"(tt));
            for (int64_t j = tt; j < n; j += LB_BLOCK) dst[j] = src[j];
            batch_stage_sync();
            S.vecs += 2.0;
        };
        // The driver's three caches hold one evaluation, the latest (LBFGS_DEVICE_EAGER_GRAD: f and the
        // gradient come together, the gradient into gt). alpha is compared with == as there; a step
        // that is not a number is also equal to itself here, bit for bit, so that the value a round
        // delivered for it is taken: the driver evaluates at such a step again, and gets the same.
        auto same = [](double u, double v) { return u == v || __double_as_longlong(u) == __double_as_longlong(v); };
        auto have_f = [&](double alpha) {  // host_f_at's test
            return X.D.hf_valid && same(X.D.hf_alpha, alpha) && X.D.hz_valid && same(X.D.hz_alpha, alpha);
        };
        auto have_g = [&](double alpha) { return X.D.gt_valid && same(X.D.gt_alpha, alpha); };  // host_g_at's
        // a miss: the point (host_point_issue) into Z, and the problem waits for the round
        auto request = [&](double alpha, const double* x) {
            dense_point(z, x, d, alpha, n);
            S.vecs += 3.0;
            X.D.hz_valid = 1;
            X.D.hz_alpha = alpha;
            X.D.hf_valid = 0;
            X.pend = alpha;
            X.wait = 1;
            X.evals++;
        };

        if (a.init) {  // x0 into Z (lbfgs_solver_init for LBFGS_OBJ_DEVICE evaluates at x)
            X = BatchExtRec();
            copy(z, V.vec(0));
            X.phase = LBK_EXT_AT_X0;
            X.wait = 1;
            X.evals = 1;
        } else {
            X = xa.rec[p];
            X.wait = 0;
            if (X.phase == LBK_EXT_AT_X0) {  // g into the gradient vector, g . g by a canonical dot pass
                double t1[1];
                copy(V.vec(1), gt);
                batch_pass<1>(OpDot<false>{V.vec(1), V.vec(1)}, geo, L, t1);
                S.vecs += 2.0;
                S.f_cur = xa.F[p];
                S.gg = t1[0];
                X.phase = LBK_EXT_TOP;
            } else {  // f and the gradient at the pending step
                X.D.hf_valid = 1;
                X.D.hf_alpha = X.pend;
                X.D.hf_val = xa.F[p];
                X.D.gt_valid = 1;
                X.D.gt_alpha = X.pend;
            }
        }

        while (!X.wait) {
            BatchIter I;
            if (X.phase == LBK_EXT_TOP) {
                if (batch_iter_top(a, V, S, I)) break;
                batch_direction(V, I, geo, L, S, W);
                double gd;
                for (bool fell_back = false;;) {  // as the dense kernel: -g, once, for a direction of no descent
                    gd = batch_materialise_d(V, I, geo, L, S, W);
                    if (!(gd >= 0) || fell_back) break;
                    S.ev[0]++;
                    W.dmode = LBK_D_NEG_G;
                    fell_back = true;
                }
                X.D.hz_valid = X.D.hf_valid = X.D.gt_valid = 0;  // host_invalidate
                batch_search_begin(a, S, s, gd);
                X.capped = X.passes = 0;
                X.phase = LBK_EXT_SEARCH;
            } else {  // the iteration's vectors again, as its top chose them (S is as the top left it)
                I.x = V.vec(S.flip ? 2 : 0);
                I.xn = V.vec(S.flip ? 0 : 2);
                I.g = V.vec(S.flip ? 3 : 1);
                I.gn = V.vec(S.flip ? 1 : 3);
                I.so = V.s(S.free_pair);
                I.yo = V.y(S.free_pair);
            }

            if (X.phase == LBK_EXT_SEARCH) {
                // lbfgs_driver.c trial() for an external objective; every order of f and the gradient
                // is one evaluation here, since they arrive together
                auto trial = [&](double alpha, bool need_g, double& f, double& dphi) -> bool {
                    if (LS == 3 && X.passes >= LBK_BATCH_BTW_CAP) {
                        X.capped = 1;
                        return false;
                    }
                    if (!(have_f(alpha) && (!need_g || have_g(alpha)))) {
                        request(alpha, I.x);
                        return false;
                    }
                    X.passes++;
                    f = X.D.hf_val;
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
                if (X.wait) break;
                if (X.capped || !s.done) {
                    S.status = LBFGS_ERR_STATE;
                    break;
                }
                batch_trace_step(a, V, S, s.step);
                X.phase = LBK_EXT_COMMIT_F;
            }

            // ---- commit (lbfgs_driver.c commit(), ext_obj): f at the step, then - unless the step
            // failed - the gradient at the step into gn, and the commit pass that reads it ----
            const double alpha = s.step;
            if (X.phase == LBK_EXT_COMMIT_F) {
                if (!have_f(alpha)) {
                    request(alpha, I.x);
                    break;
                }
                S.f_cur = X.D.hf_val;
                if (alpha < 1e-10) {
                    S.status = LBFGS_STATUS_LS_FAILED;
                    break;
                }
                X.phase = LBK_EXT_COMMIT_G;
            }
            // (the gradient arrives with f here, so this never waits; it would with a call order that
            // asks for f alone where the search does not need the gradient)
            if (!have_g(alpha)) {
                request(alpha, I.x);
                break;
            }
            copy(I.gn, gt);
            batch_pass<7>(OpCommit<LBK_OBJ_NONE, LBK_D_BUF, false, false>{I.x, batch_buf_args(V, I), alpha, I.xn, I.gn,
                                                                          I.so, I.yo, n, n, 0.0},
                          geo, L, W.tot);
            W.tot[LBK_C_F] = S.f_cur;
            S.vecs += 7.0;
            S.commits++;
            batch_accept(a.m, S, W);
            X.phase = LBK_EXT_TOP;
        }
        batch_leave<false>(a, V, P, n, S);
        if (threadIdx.x == 0) {
            xa.rec[p] = X;
            xa.evals[p] = X.evals;
            if (X.wait) {
                xa.active[p] = 1;
                atomicAdd(xa.nactive, 1);
            }
        }
    }
