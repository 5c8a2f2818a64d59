// relax_solve.hip -- the relaxation pressure solves of the device context
// (Jacobi, Red-Black SOR): the two-pass form, the fused device loop and the
// two-iterations-per-sweep form (kernels: relax_kernels.hpp, rb2.hpp). Declared in ctx.hpp.
#include "poll.hpp"
#include "rb2.hpp"

// Z-slab ranks of a relaxation solver load this unit's code object at context
// creation (a kernel attribute query does), not in the first solve on a rank
// thread.
bool relax_preload() {
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, (const void*)k_rx_init) == hipSuccess;
}

static double optimal_omega(size_t nx, size_t ny, size_t nz, double dx, double dy, double dz) {
    // linear_solver_internal.h:184-220
    double inv_dx2 = 1.0 / (dx * dx), inv_dy2 = 1.0 / (dy * dy);
    double inv_dz2 = (dz > 0.0) ? (1.0 / (dz * dz)) : 0.0;
    double num = cos(M_PI / (double)(nx - 1)) * inv_dx2 + cos(M_PI / (double)(ny - 1)) * inv_dy2;
    double den = inv_dx2 + inv_dy2;
    if (nz > 1 && inv_dz2 > 0.0) {
        num += cos(M_PI / (double)(nz - 1)) * inv_dz2;
        den += inv_dz2;
    }
    double rj = num / den;
    return 2.0 / (1.0 + sqrt(1.0 - (rj * rj)));
}

static cfd_status_t residual_linf(hip_proj_ctx* c, const double* x, const ResCoef& rc, double* out) {
    const int G = tile_grid(c);
    launch_init_red(c);
    timed(c, HIP_KT_RESIDUAL, [&] {
        klaunch(c, k_residual_linf, dim3(G), dim3(NT), c->geo, rc, x, c->rhs, c->red + 4);
    });
    cfd_status_t st;
    const unsigned long long* red = reduce_red(c, &st);
    if (st != CFD_SUCCESS) return st;
    HIP_TRY(hipMemcpyAsync(c->h_red, red, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = ord_dec(c->h_red[4]);
    return CFD_SUCCESS;
}

cfd_status_t relax_residual_linf(hip_proj_ctx* c, const double* x, double dx, double dy,
                                 double dz, double* out) {
    // relax_solve's coefficients
    const ResCoef rc{dx * dx, dy * dy, (dz > 0.0) ? (1.0 / (dz * dz)) : 0.0};
    return residual_linf(c, x, rc, out);
}

// One k_rb1 sweep on one device (3-D): xi -> xo (one RB-SOR iteration with
// its Neumann shell when neu_fold), the L-inf residual of xi decided on `st`
// as sweep `it` of the fused loop.
static void rb1_sweep_single(hip_proj_ctx* c, const RelaxCoef& rc, const double* xi, double* xo,
                             int it, RxState* st, bool neu_fold) {
    constexpr int FLR = SW_NT_STORE | SW_PREFETCH | SW_EDGE1;
    const unsigned nb1 = (unsigned)(c->rgeo.tiles_x * c->rgeo.tiles_y * c->rgeo.tiles_z);
    // register-ring prefetch (default); CFD_HIP_RB1_PF=0 selects the
    // end-of-step loads (experiments)
    const bool rb1_pf = c->env.rb1_pf;
    // memory hints of k_rb1 / k_rb1m (SW_* bits): FLR = 13, NT stores
    // of Y and plain rhs loads (r03: the NT rhs loads of 15 made the
    // neighbouring tiles re-fetch the rhs halo rows; 512^3 0.744 ->
    // 0.726 ms, 1024^2 x 512 2.925 -> 2.85 ms, fetch 19.6 -> 18.7
    // B/cell, profiles/r03_rbfl.jsonl)
    // odd iterations march z downwards (REV), so each sweep starts on
    // the planes the previous one wrote last, in the Infinity Cache;
    // bitwise either way (relax_kernels.hpp rb1_body). CFD_HIP_RB1_ALT=0:
    // every iteration upwards
    const bool rev = c->env.rb1_alt && rb1_pf && (it & 1);
    if (c->rb_strip_tc && rb1_pf) {
        // full-width tiles and the narrow strip in one grid
        const SGeo& gm = c->rg_main;
        const SGeo& gs = c->rg_strip;
        const int nbm = gm.tiles_x * gm.tiles_y * gm.tiles_z;
        const unsigned nbt = (unsigned)(nbm + gs.tiles_x * gs.tiles_y * gs.tiles_z);
        timed(c, HIP_KT_RELAX, [&] {
            klaunch(c, rev ? k_rb1m<FLR, 16, true> : k_rb1m<FLR, 16>, dim3(nbt), dim3(1024), gm,
                    gs, nbm, rc, xi, xo, c->rhs, st, c->partials, c->counter, it,
                    neu_fold ? 1 : 0);
        }, it);
        return;
    }
    timed(c, HIP_KT_RELAX, [&] {
        // k_rb1<FLR, TC, PF, DIST, REV>: the tile widths other than 64 only
        // with the prefetch, REV only at 64
        const auto kern = [&] {
            if (!rb1_pf) return k_rb1<FLR, 64, false>;
            if (c->rb1_tc == 32) return k_rb1<FLR, 32, true>;
            if (c->rb1_tc == 16) return k_rb1<FLR, 16, true>;
            if (rev) return k_rb1<FLR, 64, true, false, true>;
            return k_rb1<FLR, 64, true>;
        }();
        klaunch(c, kern, dim3(nb1), dim3(1024), c->rgeo, rc, xi, xo, c->rhs, st, c->partials,
                c->counter, it, nullptr, 0, 0, nullptr, nullptr, neu_fold ? 1 : 0);
    });
}


// Two RB-SOR iterations per sweep (k_rb2, rb2.hpp) on one device in 3-D with
// the Neumann shell, check_interval 1 (the reference default): the fused
// loop of relax_solve_fused with sweep 0 a k_rb1 sweep (the exact initial
// residual), then k_rb2 sweeps s = 1, 3, 5, ... (iterate s -> s + 2, the
// decisions on iterates s and s + 1). The host logs every launch (iterate,
// kind, buffers), so after the loop stops it finds the decided iterate: the
// input of a launch (intact) or the middle iterate of a k_rb2 sweep, which it
// recomputes with one k_rb1 sweep from that sweep's input. With apx (the
// product form) the device may also stop on
//  - ST_RB2_AMBIG (an approximate residual within its bound of the
//    threshold): the host computes that iterate's exact residual and resumes
//    the loop from the iterate with it as an override;
//  - ST_RB2_UNCERT (a value outside the certified range): the host resumes
//    from that sweep's input with k_rb1 sweeps for the rest of the solve;
// and the final residual is recomputed exactly. Iterates, iteration counts,
// statuses and residuals are those of relax_solve_fused.
static cfd_status_t relax_solve_rb2(hip_proj_ctx* c, const RelaxCoef& rc, double rel_tol,
                                    double abs_tol, int max_iter, bool apx) {
    ST_TRY(ensure_aux(c, true, true));
    if (!c->rxst) HIP_TRY(hipMalloc((void**)&c->rxst, sizeof(RxState)));
    if (!c->rxst2) HIP_TRY(hipMalloc((void**)&c->rxst2, sizeof(RxState)));
    if (!c->rb2dec) HIP_TRY(hipMalloc((void**)&c->rb2dec, sizeof(Rb2Dec)));
    Rb2Coef cf;
    cf.rc = rc;
    cf.k2 = 2.0 * (rc.rdx2 + rc.rdy2 + rc.inv_dz2);
    cf.slow = 0x1p-900;
    cf.nif = -rc.inv_factor;
    double escale = 1.0, mlim = 0x1p800;
    if (c->env.rb2_test) {  // tests: force the host paths
        const int v = c->env.rb2_test;
        if (v == 1) escale = 1e300;  // every approximate decision ambiguous
        if (v == 2) mlim = 0.0;      // every sweep uncertified
        if (v == 3) cf.slow = 1e300; // every SOR update in the reference's arithmetic
    }
    klaunch(c, k_rb2_dec_init, dim3(1), dim3(64), c->rb2dec, rc.rdx2 + rc.rdy2 + rc.inv_dz2, escale,
            mlim);
    // the fast division's range argument (rb2.hpp rb2_sorc) needs 1 <= 1/d^2 <= 2^60
    if (!(rc.rdx2 >= 1.0 && rc.rdy2 >= 1.0 && rc.rdx2 <= 0x1p60 && rc.rdy2 <= 0x1p60))
        apx = false;
    constexpr int FLR = SW_NT_STORE | SW_PREFETCH | SW_EDGE1;
    const SGeo& g2 = c->r2geo;
    const int xmap = c->env.rb2_xmap;
    const unsigned nb2 = (unsigned)(g2.tiles_x * g2.tiles_y * g2.tiles_z);
    klaunch(c, k_rx_init, dim3(1), dim3(64), c->rxst, rel_tol, abs_tol, max_iter, 1);
    if (apx) {
        const int nbm = (int)std::min<long long>(4LL * c->grid_cap,
                                                 ((long long)c->nx * c->ny * c->nz + 255) / 256);
        klaunch(c, k_rb2_bmax, dim3(std::max(1, nbm)), dim3(256), c->geo, c->rhs, c->rxst);
    }
    struct Launch {
        int s, kind;  // kind 1: k_rb1 (iterate s -> s + 1), 2: k_rb2 (s -> s + 2)
        double *x, *y;
    };
    std::vector<Launch> log;
    double* bx = c->pn;
    double* by = c->xt;
    int cur = 0;
    bool exact_mode = false, force_certx = false;
    int n_ambig = 0, n_uncert = 0;
    auto launch = [&]() {
        if (cur == 0 || exact_mode) {
            rb1_sweep_single(c, rc, bx, by, cur, c->rxst, true);
            log.push_back({cur, 1, bx, by});
            cur += 1;
        } else {
            const int certx = (force_certx || log.empty() || log.back().kind == 1) ? 1 : 0;
            force_certx = false;
            if (apx && certx) {  // X's own values: max |X| for the sweep's range test
                // (an error here is sticky: the loop's next HIP_TRY reports it)
                (void)hipMemsetAsync(&c->rxst->xmax, 0, sizeof(double), c->stream);
                const int nbm = (int)std::min<long long>(
                    4LL * c->grid_cap, ((long long)c->nx * c->ny * c->nz + 255) / 256);
                klaunch(c, k_rb2_xmax, dim3(std::max(1, nbm)), dim3(256), c->geo, bx, c->rxst);
            }
            timed(c, HIP_KT_RELAX2, [&] {
                with_bool(apx, [&](auto APX) {
                    klaunch(c, k_rb2<APX, FLR>, dim3(nb2), dim3(1024), g2, cf, bx, by, c->rhs,
                            c->rxst, c->partials, c->counter, cur, certx, xmap, c->rb2dec);
                });
            }, cur);
            log.push_back({cur, 2, bx, by});
            cur += 2;
        }
        std::swap(bx, by);
    };
    // the middle iterate of k_rb2 launch L, recomputed into L.y (one k_rb1
    // sweep on a scratch state that never decides)
    auto recompute_mid = [&](const Launch& L) {
        klaunch(c, k_rx_init, dim3(1), dim3(64), c->rxst2, 0.0, 0.0, 0x7fffffff, 1);
        rb1_sweep_single(c, rc, L.x, L.y, 1, c->rxst2, true);
    };
    auto find = [&](int t, int* kind_mid) -> int {  // log index holding iterate t
        for (int q = (int)log.size() - 1; q >= 0; --q) {
            if (log[q].s == t) {
                *kind_mid = 0;
                return q;
            }
            if (log[q].kind == 2 && log[q].s + 1 == t) {
                *kind_mid = 1;
                return q;
            }
        }
        return -1;
    };
    const ResCoef resc{rc.dx2, rc.dy2, rc.inv_dz2};
    for (;;) {
        // iterates 0 .. max_iter; every (re-)entry starts with a chunk of 8
        ST_TRY(poll_loop(c, c->rxst, cur, max_iter + 1, [&](int&) {
            launch();  // advances cur
            return CFD_SUCCESS;
        }));
        RxState r;
        ST_TRY(poll_final(c, c->rxst, &r));
        if (!r.done) {
            set_err(CFD_ERROR, "relaxation (k_rb2): device loop ended without a decision");
            return CFD_ERROR;
        }
        int mid = 0;
        const int li = find(r.res_it, &mid);
        if (li < 0) {
            set_err(CFD_ERROR, "relaxation (k_rb2): decided iterate not in the launch log");
            return CFD_ERROR;
        }
        const Launch L = log[li];
        if (r.status == ST_RB2_UNCERT) {
            ++n_uncert;
            // rerun from this sweep's input with k_rb1 sweeps
            log.resize(li);
            exact_mode = true;
            bx = L.x;
            by = L.y;
            cur = L.s;
            klaunch(c, k_rb2_resume, dim3(1), dim3(64), c->rxst, -1, 0.0);
            continue;
        }
        double* xt = mid ? L.y : L.x;
        if (mid) recompute_mid(L);
        if (r.status == ST_RB2_AMBIG) {
            ++n_ambig;
            double m = 0.0;
            ST_TRY(residual_linf(c, xt, resc, &m));
            log.resize(li);
            force_certx = true;  // the next sweep's input came from a recompute
            bx = xt;
            by = mid ? L.x : L.y;
            cur = r.res_it;
            klaunch(c, k_rb2_resume, dim3(1), dim3(64), c->rxst, r.res_it, m);
            continue;
        }
        flush_timing(c);
        double res = r.res;
        if (!r.res_exact) ST_TRY(residual_linf(c, xt, resc, &res));
        if (c->env.rb2_log) {  // diagnostics: the loop's launches and stops
            int n1 = 0, n2 = 0;
            for (const Launch& q : log) (q.kind == 1 ? n1 : n2)++;
            int n_int = 0;  // interior tiles, by k_rb2's own predicate
            for (int ty = 0; ty < g2.tiles_y; ++ty)
                for (int tx = 0; tx < g2.tiles_x; ++tx)
                    n_int += rb2_tile_interior(tx, ty, g2.nx, g2.ny) ? 1 : 0;
            fprintf(stderr, "rb2: iterations %d status %d, k_rb1 %d k_rb2 %d launches, "
                    "%d ambiguous, %d uncertified, res_it %d, kc %d tiles %d x %d x %d "
                    "interior %d\n", r.iterations, r.status, n1, n2, n_ambig, n_uncert,
                    r.res_it, g2.kc, g2.tiles_x, g2.tiles_y, g2.tiles_z, n_int);
        }
        if (xt != c->pn) std::swap(c->pn, c->xt);
        return finish_stats(c, r, res);
    }
}

// Fused relaxation loop (single device, 16-row sweep tiles): the iteration's
// sweeps, boundary shell and convergence test all run on the device (k_rx,
// relax_kernels.hpp); the host polls the state one chunk behind, like cg_solve.
// Same iterates, residuals, iteration counts and statuses as relax_solve's
// two-pass form below.
static cfd_status_t relax_solve_fused(hip_proj_ctx* c, int method, const RelaxCoef& rc,
                                      double rel_tol, double abs_tol, int max_iter,
                                      int check_interval) {
    ST_TRY(ensure_aux(c, true, true));
    if (!c->rxst) HIP_TRY(hipMalloc((void**)&c->rxst, sizeof(RxState)));
    double* X[2] = {c->pn, c->xt};
    const bool D = dist(c);
    Mbox* mb = mbox(c);
    // Z-slabs without a device mailbox: residual max through RCCL (red[6] -> redg[6])
    unsigned long long* dred = c->red + 6;
    unsigned long long* gred = D ? c->redg + 6 : nullptr;
    const unsigned nb = (unsigned)sweep_grid(c);
    const unsigned TH = 64u * (unsigned)c->sweep_ty;
    constexpr int FL = SW_NT_STORE | SW_NT_LOAD | SW_PREFETCH | SW_EDGE1;
    // k_rb1: plain rhs loads (its tiles' rhs halo rows are re-read by the
    // neighbouring tile; see the one-device launch below)
    constexpr int FLR = SW_NT_STORE | SW_PREFETCH | SW_EDGE1;
    auto sweep = [&](int mode, const double* xi, double* xo, int it) {
        timed(c, HIP_KT_RELAX, [&] {
            with_int<8, 16>(c->sweep_ty, [&](auto TY) {
                with_bool(D, [&](auto DIST) {
                    with_int<RX_JACOBI, RX_RED, RX_BLACK>(mode, [&](auto MODE) {
                        klaunch(c, k_rx<TY, MODE, FL, DIST>, dim3(nb), dim3(TH), c->sgeo, rc, xi,
                                xo, c->rhs, c->rxst, c->partials, c->counter, it, mb, dred);
                    });
                });
            });
        });
    };
    // the residual sweep's all-ranks max when there is no device mailbox
    auto finish = [&](int it) -> cfd_status_t {
        if (!D || mb) return CFD_SUCCESS;
        ST_TRY(c->comm->allreduce_max_u64(c->stream, dred, gred, 1));
        klaunch(c, k_rx_finish, dim3(1), dim3(64), c->rxst, gred, it);
        return CFD_SUCCESS;
    };
    // one-pass RB-SOR (k_rb1) on a single device in 3-D; relax_two_pass = 2
    // forces the two colour sweeps of k_rx
    // one-pass RB-SOR (k_rb1) in 3-D, on one device or on Z-slabs (there with
    // the edge planes' R exchanged first); relax_two_pass = 2 forces the two
    // colour sweeps of k_rx
    const bool single = method == HIP_POISSON_REDBLACK && c->nz > 1 &&
                        c->cfg.relax_two_pass == 0;
    // k_rb1 writes the iteration's Neumann shell itself (no k_rx_shell);
    // CFD_HIP_RB1_FOLD=0 keeps the separate shell launch (A/B)
    const bool neu_fold = single && c->env.rb1_fold && c->poisson_bc == HIP_POISSON_BC_NEUMANN;
    // two iterations per sweep on one device (rb2.hpp): CFD_HIP_RB2 = 1 (the
    // default: certified fast arithmetic), 2 (the reference's arithmetic
    // throughout), 0 (one iteration per sweep, k_rb1)
    const int rb2_env = c->env.rb2;
    if (neu_fold && !D && check_interval == 1 && rb2_env != 0 && c->r2geo.tiles_x > 0)
        return relax_solve_rb2(c, rc, rel_tol, abs_tol, max_iter, rb2_env != 2);
    ST_TRY(halo(c, {c->pn}));
    klaunch(c, k_rx_init, dim3(1), dim3(64), c->rxst, rel_tol, abs_tol, max_iter, check_interval);
    // Halo exchanges are host-launched and run even after the device decided
    // to stop; they then copy the neighbours' final owned planes into the
    // result's halo planes, which is what they hold anyway.
    auto iterate = [&](int it) -> cfd_status_t {
        double* xi = X[it & 1];
        double* xo = X[(it + 1) & 1];
        if (single && D) {
            // R of the own edge planes -> the neighbours' halo planes of RH
            // (the CG residual array, free during a relaxation solve), then
            // the one-pass sweep with R on the halo planes taken from RH
            double* RH = c->r;
            c->cg_scratch_dirty = 1;
            const long long plane = (long long)c->nx * (long long)c->ny;
            const unsigned ne = (unsigned)std::min<long long>((2 * plane + 255) / 256,
                                                              (long long)c->grid_cap * 4);
            timed(c, HIP_KT_RELAX, [&] {
                klaunch(c, k_rb_edge_r, dim3(ne), dim3(256), c->rgeo, rc, xi, c->rhs, RH);
            }, it);
            auto rb1 = [&](const SGeo& sg) {
                const unsigned nbx = (unsigned)(sg.tiles_x * sg.tiles_y * sg.tiles_z);
                timed(c, HIP_KT_RELAX, [&] {
                    klaunch(c, k_rb1<FLR, 64, true, true>, dim3(nbx), dim3(1024), sg, rc, xi, xo,
                            c->rhs, c->rxst, c->partials, c->counter, it, RH,
                            c->geo.lo_face ? 0 : 1, c->geo.hi_face ? 0 : 1, mb, dred,
                            neu_fold ? 1 : 0);
                }, it);
            };
            // exchange of `f`'s edge planes on the side stream (halo
            // communicator), ordered after the main stream's work so far
            auto side_halo = [&](double* f) -> cfd_status_t {
                HIP_TRY(hipEventRecord(c->ev_b, c->stream));
                HIP_TRY(hipStreamWaitEvent(c->hstream, c->ev_b, 0));
                double* ff[1] = {f};
                ST_TRY(timed_span(c, c->hstream, HIP_KT_HALO, [&] {
                    return c->comm->halo(c->hstream, ff, 1, c->ps, (int)c->nz, false);
                }, it));
                HIP_TRY(hipEventRecord(c->ev_h, c->hstream));
                return CFD_SUCCESS;
            };
            if (c->split_rb) {
                // R's edge planes travel while interior part 1 (which needs no
                // halo R) runs; the edge planes of Y follow, and their exchange
                // overlaps interior part 2 and the residual's all-reduce. The
                // three launches write disjoint planes of Y and share one
                // L-inf reduction, so Y and the decision are the one-launch ones.
                ST_TRY(side_halo(RH));
                rb1(c->rg_in1);
                HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_h, 0));
                rb1(c->rg_edge);
                ST_TRY(side_halo(xo));
                rb1(c->rg_in2);
                if (!mb)
                    ST_TRY(timed_span(c, c->stream, HIP_KT_ALLREDUCE, [&] { return finish(it); },
                                      it));
                HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_h, 0));
            } else {
                // same collective order as the split form (R halo, Y halo,
                // residual max): the in-process group pairs its ranks' calls
                // by order, and a slab of < 4 planes runs this form beside
                // split neighbours
                ST_TRY(timed_span(c, c->stream, HIP_KT_HALO, [&] { return halo(c, {RH}); }, it));
                rb1(c->rgeo);
                ST_TRY(timed_span(c, c->stream, HIP_KT_HALO, [&] { return halo(c, {xo}); }, it));
                if (!mb)
                    ST_TRY(timed_span(c, c->stream, HIP_KT_ALLREDUCE, [&] { return finish(it); },
                                      it));
            }
        } else if (single) {
            rb1_sweep_single(c, rc, xi, xo, it, c->rxst, neu_fold);
        } else if (method == HIP_POISSON_REDBLACK) {
            sweep(RX_RED, xi, xo, it);
            ST_TRY(finish(it));
            klaunch(c, k_rx_shell, dim3(shell_blocks(c)), dim3(256), c->geo, c->rxst, xi, xo, 0);
            ST_TRY(halo(c, {xo}));  // the black pass reads the neighbours' red cells
            sweep(RX_BLACK, nullptr, xo, it);
        } else {
            sweep(RX_JACOBI, xi, xo, it);
            ST_TRY(finish(it));
        }
        if (D && !single)
            ST_TRY(timed_span(c, c->stream, HIP_KT_HALO, [&] { return halo(c, {xo}); }, it));
        // the iteration's apply_bc: Neumann (linear_solver_redblack.c:139,
        // linear_solver_jacobi.c:118), or the caller's fixed boundary values,
        // or x's own boundary kept
        if (!neu_fold) {
            const double* shell_src = (c->poisson_bc == HIP_POISSON_BC_FIXED) ? c->bcfix : xi;
            const int shell_mode = (c->poisson_bc == HIP_POISSON_BC_NEUMANN) ? 1 : 0;
            klaunch(c, k_rx_shell, dim3(shell_blocks(c)), dim3(256), c->geo, c->rxst, shell_src, xo,
                    shell_mode);
        }
        return CFD_SUCCESS;
    };
    // iterations 0..max_iter: sweep it also yields the residual after it - 1
    // iterations, so the last launch only completes the final test
    int it = 0;
    ST_TRY(poll_loop(c, c->rxst, it, max_iter + 1, [&](int& i) -> cfd_status_t {
        ST_TRY(iterate(i));
        ++i;
        return CFD_SUCCESS;
    }));
    RxState r;
    ST_TRY(poll_final(c, c->rxst, &r));
    flush_timing(c);
    if (r.status == ST_COMM_TIMEOUT) {
        set_err(CFD_ERROR, "relaxation: slab all-reduce timed out (a rank stopped)");
        return CFD_ERROR;
    }
    if (!r.done) {
        set_err(CFD_ERROR, "relaxation: device loop ended without a decision");
        return CFD_ERROR;
    }
    if (r.result == 1) std::swap(c->pn, c->xt);
    return finish_stats(c, r, r.res);
}

// Relaxation methods driven by the common loop (linear_solver.c:397-485):
// L-infinity residual before the loop and every check_interval iterations.
cfd_status_t relax_solve(hip_proj_ctx* c, int method, double dx, double dy, double dz,
                         double rel_tol, double abs_tol, int max_iter, int check_interval,
                         double omega_in) {
    const int G = tile_grid(c);
    RelaxCoef rc;
    rc.dx2 = dx * dx;
    rc.dy2 = dy * dy;
    rc.inv_dz2 = (dz > 0.0) ? (1.0 / (dz * dz)) : 0.0;
    rc.inv_factor = 1.0 / (2.0 * (1.0 / rc.dx2 + 1.0 / rc.dy2 + rc.inv_dz2));
    rc.omega = (omega_in <= 0.0) ? optimal_omega(c->nx, c->ny, c->nzg, dx, dy, dz) : omega_in;
    rc.rdx2 = 1.0 / rc.dx2;
    rc.rdy2 = 1.0 / rc.dy2;
    if ((c->sweep_ty == 16 || c->sweep_ty == 8) && max_iter > 0 &&
        (c->cfg.relax_two_pass != 1 || c->poisson_bc != HIP_POISSON_BC_NEUMANN))
        return relax_solve_fused(c, method, rc, rel_tol, abs_tol, max_iter, check_interval);
    ResCoef res_c{rc.dx2, rc.dy2, rc.inv_dz2};
    const DirVals dv{};
    // caller boundary modes (hip_proj_poisson_solve_ex): the iteration's
    // apply_bc copies the shell from bcfix (FIXED) or keeps x's own (NONE);
    // k_rx_shell does the copy, gated on an RxState that k_rx_init leaves
    // undecided
    const bool neumann_bc = c->poisson_bc == HIP_POISSON_BC_NEUMANN;
    if (!neumann_bc) {
        if (!c->rxst) HIP_TRY(hipMalloc((void**)&c->rxst, sizeof(RxState)));
        klaunch(c, k_rx_init, dim3(1), dim3(64), c->rxst, rel_tol, abs_tol, max_iter,
                check_interval);
    }
    ST_TRY(halo(c, {c->pn}));
    double res0 = 0.0;
    cfd_status_t s = residual_linf(c, c->pn, res_c, &res0);
    if (s != CFD_SUCCESS) return s;
    double tol = rel_tol * res0;
    if (tol < abs_tol) tol = abs_tol;
    c->pstats.initial_residual = res0;
    if (res0 < abs_tol) {
        c->pstats.status = POISSON_CONVERGED;
        c->pstats.iterations = 0;
        c->pstats.final_residual = res0;
        return CFD_SUCCESS;
    }
    int iter;
    bool conv = false;
    double res = res0;
    for (iter = 0; iter < max_iter; ++iter) {
        if (method == HIP_POISSON_REDBLACK) {
            timed(c, HIP_KT_RELAX, [&] {
                klaunch(c, k_rb_pass, dim3(G), dim3(NT), c->geo, rc, c->pn, c->rhs, 1);
            });
            ST_TRY(halo(c, {c->pn}));  // the black pass reads the neighbours' red cells
            timed(c, HIP_KT_RELAX, [&] {
                klaunch(c, k_rb_pass, dim3(G), dim3(NT), c->geo, rc, c->pn, c->rhs, 0);
            });
        } else {
            timed(c, HIP_KT_RELAX, [&] {
                klaunch(c, k_jacobi, dim3(G), dim3(NT), c->geo, rc, c->pn, c->xt, c->rhs);
            });
            // memcpy(x, x_temp) + BC == swap buffers then BC (all boundary
            // cells are rewritten by the Neumann gather; with a caller mode
            // the shell is copied below)
            std::swap(c->pn, c->xt);
        }
        ST_TRY(halo(c, {c->pn}));
        if (neumann_bc) {
            launch_bc(c, c->pn, 0, dv);
        } else if (c->poisson_bc == HIP_POISSON_BC_FIXED || method != HIP_POISSON_REDBLACK) {
            // FIXED: the caller's values; NONE + Jacobi: the iterate's previous
            // boundary (now in xt), as the fused loop keeps it. NONE + RB-SOR
            // updates in place and never writes the shell.
            const double* src = (c->poisson_bc == HIP_POISSON_BC_FIXED) ? c->bcfix : c->xt;
            klaunch(c, k_rx_shell, dim3(shell_blocks(c)), dim3(256), c->geo, c->rxst, src, c->pn,
                    0);
        }
        if (iter % check_interval == 0) {
            s = residual_linf(c, c->pn, res_c, &res);
            if (s != CFD_SUCCESS) return s;
            if (res < tol || res < abs_tol) {
                conv = true;
                break;
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    flush_timing(c);
    c->pstats.iterations = iter + 1;
    c->pstats.final_residual = res;
    c->pstats.status = conv ? POISSON_CONVERGED : POISSON_MAX_ITER;
    return conv ? CFD_SUCCESS : CFD_ERROR_MAX_ITER;
}
