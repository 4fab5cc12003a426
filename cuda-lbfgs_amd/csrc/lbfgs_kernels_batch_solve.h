// lbfgs_kernels_batch_solve.h - the body of k_batch_solve and k_batch_solve_ragged
// (lbfgs_kernels_batch.hip), included once in each. The two kernels are one text and differ in their
// argument lists alone: a uniform batch's kernel keeps the arguments it always had, and with them its
// code; a ragged batch's takes the table as well. In scope where this is included: a, geo_b,
// constexpr bool RAGGED, and rg (the BatchRagged; nulls, never read, in the uniform kernel).
// NOT a stand-alone header: no include guard, no declarations of its own; it is the statements of a
// __global__ function and is included inside one, nowhere else.
    __shared__ BatchLds L;
    constexpr bool FG = LS == 2 || LS == 3;
    constexpr bool CAND = LS == 0;  // the backtracking search's second step rides the first commit
    constexpr int NC = LBK_TRIALS_NC;
    BatchWave& W = L.wv[threadIdx.x >> 6];
    BatchState& S = W.st;
    lbk_search& s = W.s;
    for (int i = blockIdx.x; i < a.B; i += gridDim.x) {
        const BatchProb P = batch_prob<RAGGED>(rg, i);
        const Geo geo = batch_geo<RAGGED>(geo_b, P);
        const int64_t n = geo.n;
        const BatchView V = batch_view<RAGGED>(a, P);
        if (batch_enter<RAGGED>(a, V, P, n, S)) continue;
        if (a.init) {  // f and g.g at x0 (lbfgs.cpp:29-30)
            DirArgs da0 = {};
            double t2[2];
            batch_pass<2>(OpObjective<OBJ, true, true, false>{V.vec(0), da0, 0.0, V.vec(1), n, n}, geo, L, t2);
            S.f_cur = t2[0];
            S.gg = t2[1];
            S.vecs = 2.0;
        }

        for (int it = 0; it < a.iters; ++it) {
            BatchIter I;
            if (batch_iter_top(a, V, S, I)) break;
            batch_direction(V, I, geo, L, S, W);

            // ---- the fused first trial at a0 with the commit ----
            const double a0 = a.K.initial_step;
            const double cand = CAND ? a0 * a.K.backtracking_alpha : 0.0;
            // how the direction is formed until d is materialised (k_commit's TWOLOOP / NEG_G)
            auto dir_args = [&]() {
                DirArgs dd = {};
                dd.g = I.g;
                dd.g_hi = LBK_GROUPS;
                if (W.dmode == LBK_D_TWOLOOP) {
                    dd.dsrc = V.r();
                    dd.s = V.s(W.top);
                    dd.coef = W.coef;
                    dd.rho = W.rho_top;
                }
                return dd;
            };
            double gd;
            for (bool fell_back = false;;) {  // the first trial at a0 and the commit, in one pass
                const DirArgs dd = dir_args();
                if (W.dmode == LBK_D_TWOLOOP) {
                    batch_commit<OBJ, LBK_D_TWOLOOP, CAND>(geo, L, I.x, dd, a0, I.xn, I.gn, I.so, I.yo, cand, W.tot);
                    S.vecs += 8.0;
                } else {
                    batch_commit<OBJ, LBK_D_NEG_G, CAND>(geo, L, I.x, dd, a0, I.xn, I.gn, I.so, I.yo, cand, W.tot);
                    S.vecs += 6.0;
                }
                S.commits++;
                gd = W.tot[LBK_C_GD];
                if (!(gd >= 0) || fell_back) break;
                S.ev[0]++;  // :146-153: not a descent direction, the gradient instead (once, as the host)
                W.dmode = LBK_D_NEG_G;
                fell_back = true;
            }

            // ---- the line search, with the host's caches of that pass ----
            batch_search_begin(a, S, s, gd);
            s.have_spec = 1;
            s.spec_a = a0;
            s.spec_f = W.tot[LBK_C_F];
            s.spec_dphi = W.tot[LBK_C_DPHI];
            if (CAND && cand > 0.0) {
                s.have_cand = 1;
                s.cand_a = cand;
                s.cand_f = W.tot[LBK_C_FC];
            }
            W.d_ready = W.capped = W.passes = 0;
            // d into its buffer before the first pass that reads it. Always inlined: left to the cost
            // model it is a call in some of the twelve kernels, and what it captures (geo, the view,
            // the iteration's vectors) then lives in scratch
            auto need_d = [&]() __attribute__((always_inline)) {
                if (W.d_ready) return;
                batch_materialise_d(V, I, geo, L, S, W);
                W.d_ready = 1;
            };
            auto trial = [&](double alpha, bool need_g, double& f, double& dphi) -> bool {
                if (search_cached(s, alpha, need_g, f, dphi)) return true;
                if (LS == 3 && W.passes >= LBK_BATCH_BTW_CAP) {  // the reference's loop has no bound of its own
                    W.capped = 1;
                    return false;
                }
                need_d();
                W.passes++;
                S.vecs += 2.0;
                if (FG) {
                    OpTrials<OBJ, LBK_D_BUF, 1, true, false> op{I.x, batch_buf_args(V, I), {alpha}, n, n};
                    double tt[2];
                    batch_pass<2>(op, geo, L, tt);
                    search_note_fg(s, alpha, tt);
                    f = tt[0];
                    dphi = tt[1];
                } else {
                    OpTrials<OBJ, LBK_D_BUF, NC, false, false> op{I.x, batch_buf_args(V, I), {}, n, n};
                    search_chain<LS>(s, alpha, op.a);
                    double tt[NC];
                    batch_pass<NC>(op, geo, L, tt);
                    search_note_f(s, op.a, tt);
                    f = tt[0];
                }
                return true;
            };
            search_loop<LS>(s, trial);
            S.trials_f += s.passes_f;
            S.trials_fg += s.passes_fg;
            if (W.capped || !s.done) {
                S.status = LBFGS_ERR_STATE;
                break;
            }
            const double alpha = s.step;
            batch_trace_step(a, V, S, alpha);

            // ---- commit (:159-198): again at the search's step when that is not the first trial's ----
            if (!(alpha == a0)) {
                need_d();
                batch_commit<OBJ, LBK_D_BUF, false>(geo, L, I.x, batch_buf_args(V, I), alpha, I.xn, I.gn, I.so, I.yo, 0.0,
                                                    W.tot);
                S.vecs += 7.0;
                S.commits++;
            }
            S.f_cur = W.tot[LBK_C_F];
            if (alpha < 1e-10) {  // :164-168
                S.status = LBFGS_STATUS_LS_FAILED;
                break;
            }
            batch_accept(a.m, S, W);
        }
        batch_leave<RAGGED>(a, V, P, n, S);
    }
