// poisson_solve.hpp -- the pressure solvers of the device context that are
// compiled with projection_hip.hip (CG in its textbook and single-reduction
// forms, BiCGSTAB, and through transform_solve.hpp the direct sine- and
// cosine-transform solves) with their launch wrappers. The relaxation methods
// are a unit of their own, relax_solve.hip; the polled device loop all share
// is poll.hpp. Host code only; private to projection_hip.hip.
#pragma once

#include "poll.hpp"
#include "kernels.hpp"
#include "ccf.hpp"
#include "bicgstab.hpp"

// f(IntC<TY>, IntC<FL>) for the context's sweep tile rows and memory hints:
// sweep_ty 8 or 16 with any planned sweep_variant (23 and 31: 16 rows only),
// sweep_ty 4 with variant 0 only
template <class F>
static void with_sweep(const hip_proj_ctx* c, F&& f) {
    if (c->sweep_ty == 4)
        f(IntC<4>{}, IntC<0>{});
    else if (c->sweep_ty == 16)
        with_int<0, 1, 2, 3, 4, 7, 15, 23, 31>(c->sweep_variant,
                                               [&](auto FL) { f(IntC<16>{}, FL); });
    else
        with_int<0, 1, 2, 3, 4, 7, 15>(c->sweep_variant, [&](auto FL) { f(IntC<8>{}, FL); });
}

// fd.x == nullptr: no fold this iteration
static void launch_cgA(hip_proj_ctx* c, bool first, const Lap& L, const double* r,
                       const double* po, double* pn, int it, const PFold& fd) {
    with_sweep(c, [&](auto TY, auto FL) {
        auto sweep = [&](auto FIRST, auto FLV, auto FOLD) {
            with_bool(dist(c), [&](auto DIST) {
                klaunch(c, k_cgA<TY, FIRST, DIST, FLV, FOLD>, dim3(sweep_grid(c)), dim3(64 * TY),
                        c->sgeo, L, r, po, pn, c->st, c->partials, c->counter, it, c->dsum,
                        mbox(c), fd);
            });
        };
        if (first) sweep(BoolC<true>{}, FL, BoolC<false>{});
        // the fold sweep streams 4 more fields: without the plane prefetch's
        // second register bundle it fits without spilling
        else if (fd.x) sweep(BoolC<false>{}, IntC<(FL & ~SW_PREFETCH)>{}, BoolC<true>{});
        else sweep(BoolC<false>{}, FL, BoolC<false>{});
    });
}

// Sweep B operands: p = p_it (stencil) and r.
struct BArgs {
    const double* p;
    double* r;
};

static void launch_cgB(hip_proj_ctx* c, const SGeo& sg, const Lap& L, const BArgs& a, int it) {
    const unsigned nb = (unsigned)(sg.tiles_x * sg.tiles_y * sg.tiles_z);
    with_sweep(c, [&](auto TY, auto FL) {
        with_bool(dist(c), [&](auto DIST) {
            // sweep B marches z downwards on one device in 3-D (r03: it starts on the
            // planes sweep A touched last, in the Infinity Cache; 512^3 sweep B
            // 0.551 -> 0.539 ms, CG iteration 1.355 -> 1.335 ms, profiles/r03_rev.jsonl);
            // CFD_HIP_CGB_REV=0 restores the upward march
            const bool rev = !DIST && c->env.cgb_rev && c->geo.sz && sg.kmode == 0;
            klaunch(c, rev ? k_cgB<TY, DIST, FL, true> : k_cgB<TY, DIST, FL>, dim3(nb),
                    dim3(64 * TY), sg, L, a.p, a.r, c->st, c->partials, c->counter, it, c->dsum,
                    mbox(c));
        });
    });
}

// Chronopoulos-Gear CG launches (cg_variant 1)
static void launch_cc1(hip_proj_ctx* c, double* pn, const double* po, const PPrev& pv, double* x,
                       int it) {
    const unsigned n = (unsigned)(c->px / 2) * (unsigned)(c->ny - 2) *
                       (unsigned)(c->sgeo.k1 - c->sgeo.k0);
    const unsigned nb = std::max(1u, std::min((n + 255) / 256, (unsigned)c->grid_cap * 4));
    const bool fold = (it % CG_XFOLD) == CG_XFOLD - 1;
    auto kern = k_cc1<true, false>;  // <FIRST, FOLD>
    if (it > 0) kern = fold ? k_cc1<false, true> : k_cc1<false, false>;
    klaunch(c, kern, dim3(nb), dim3(256), c->sgeo, c->r, c->cw, c->cs, po, pn, pv, x, c->st, it);
}

// w = A r (stored for k_cc1 when wst) and the iteration's one reduction, over
// the planes of g (c->sgeo: all of them; c->cc2_edge: a slab's edge planes)
static void launch_cc2(hip_proj_ctx* c, const Lap& L, int it, bool init, const double* r,
                       bool wst, const SGeo* gp = nullptr) {
    const SGeo& g = gp ? *gp : c->sgeo;
    const unsigned nb = (unsigned)(g.tiles_x * g.tiles_y * g.tiles_z);
    with_int<8, 16, 4>(c->sweep_ty, [&](auto TY) {
        with_bool(wst, [&](auto WST) {
            with_bool(dist(c), [&](auto DIST) {
                with_bool(init, [&](auto INIT) {
                    klaunch(c, k_cc2<TY, DIST, INIT, WST>, dim3(nb), dim3(64 * TY), g, L, r,
                            c->cw, c->st, c->partials, c->counter, it, c->dsum, mbox(c));
                });
            });
        });
    });
}

// k_ccf (ccf.hpp): cg_variant 1's whole iteration in one z-march; r_it is in
// c->r for even it and in c->r2 for odd it
// Z-slabs (NOC): the march stops after r_{it+1} (and p_it, also on the halo
// planes); the r halo and k_cc2 (w = A r in registers, the one reduction)
// follow
static const double* ccf_r0(const hip_proj_ctx* c, int it) { return (it & 1) ? c->r2 : c->r; }
static double* ccf_r1(hip_proj_ctx* c, int it) { return (it & 1) ? c->r : c->r2; }

// g: c->ccgeo (the whole march), or on Z-slabs c->cc_edge / c->cc_int. noc:
// the march stops after r_{it+1} (Z-slab edge planes, or a whole slab of < 3
// planes), else it also forms w and the dot products (one device; a slab's
// interior planes in the fused form)
static void launch_ccf(hip_proj_ctx* c, const SGeo& g, const Lap& L, double* pn,
                       const double* po, const PPrev& pv, double* x, int it, bool noc,
                       hipStream_t s = nullptr) {
    // clock sample on one launch in eight while timing (iterations 5 and 7
    // mod 8: a plain and a fold launch)
    unsigned long long* clk = (c->timing && c->clk && (it & 5) == 5) ? c->clk : nullptr;
    // k_ccf<.., false> is the edge-sum form, whose 60 x 29 tiling only
    // c->ccgeo of an edge-sum context has; every other march with stage c (a
    // Z-slab's interior planes, CFD_HIP_CCF_EDGE_DOT=0) is k_ccf_cell
    const bool cell = !noc && !(c->ccf_edge_dot && g.kmode == 0);
    const bool fold = (it % CG_XFOLD) == CG_XFOLD - 1;
    auto launch = [&](auto kern) {
        klaunch_on(c, s ? s : c->stream, kern, dim3(g.tiles_x * g.tiles_y * g.tiles_z),
                   dim3(1024), g, L, ccf_r0(c, it), ccf_r1(c, it), po, pn, pv, x, c->st,
                   c->partials, c->counter, it, c->env.ccf_xmap, dist(c) ? 1 : 0, c->dsum, mbox(c),
                   clk);
    };
    with_bool(noc, [&](auto NOC) {
        auto march = [&](auto FIRST, auto FOLD) {
            if constexpr (!NOC) {
                if (cell) return launch(k_ccf_cell<FIRST, FOLD>);
            }
            launch(k_ccf<FIRST, FOLD, NOC>);
        };
        if (it == 0) march(BoolC<true>{}, BoolC<false>{});
        else if (fold) march(BoolC<false>{}, BoolC<true>{});
        else march(BoolC<false>{}, BoolC<false>{});
    });
}

// RK4 stages (rk4_hip.hip) and the Z-slab one-pass relaxation borrow r and
// the p ring and leave wall values there; the Krylov solvers need zero wall
// cells in them
static cfd_status_t clear_cg_scratch(hip_proj_ctx* c) {
    if (!c->cg_scratch_dirty) return CFD_SUCCESS;
    for (double* f : {c->r, c->pa, c->pb, c->pc4, c->pd4, c->r2})
        if (f) HIP_TRY(hipMemsetAsync(f, 0, field_elems(c) * sizeof(double), c->stream));
    c->cg_scratch_dirty = 0;
    return CFD_SUCCESS;
}

// ---------------------------------------------------------------------------
// pressure solvers on ctx->pn
// ---------------------------------------------------------------------------
enum RhsSource { RHS_FROM_VELOCITY, RHS_FROM_ARRAY };

static cfd_status_t cg_solve(hip_proj_ctx* c, double dx, double dy, double dz,
                             const DivCoef& dc, RhsSource src, double rel_tol, double abs_tol,
                             int max_iter, int check_interval, bool final_bc) {
    const Lap L = make_lap(dx, dy, dz);
    const int G = tile_grid(c);
    const DirVals dv{};
    const bool D = dist(c);
    double* x = c->pn;
    ST_TRY(clear_cg_scratch(c));
    ST_TRY(halo(c, {x}));
    // poisson_solver_apply_bc(x) at solve start (linear_solver_cg.c:320); a
    // caller override runs on the host around the device solve instead
    const bool neumann = (c->poisson_bc == HIP_POISSON_BC_NEUMANN);
    if (neumann) launch_bc(c, x, 0, dv);
    timed(c, HIP_KT_CG_SETUP, [&] {
        // the right-hand side: the divergence of (us, vs, ws), or c->rhs
        const bool vel = (src == RHS_FROM_VELOCITY);
        with_bool(vel, [&](auto VEL) {
            with_bool(D, [&](auto DIST) {
                klaunch(c, k_cg_setup<VEL, false, true, DIST>, dim3(G), dim3(NT), c->geo, L, dc,
                        vel ? c->us : nullptr, vel ? c->vs : nullptr, vel ? c->ws : nullptr,
                        vel ? nullptr : c->rhs, x, c->r, c->st, c->partials, c->counter, rel_tol,
                        abs_tol, max_iter, check_interval, c->dsum, mbox(c));
            });
        });
    });
    if (D && !mbox(c)) {
        ST_TRY(reduce_dot(c));
        klaunch(c, k_finish_setup, dim3(1), dim3(64), c->st, c->dsum + 1, rel_tol, abs_tol,
                max_iter, check_interval);
    }
    if (D) ST_TRY(halo(c, {c->r}));
    double* P[CG_XFOLD] = {c->pa, c->pb, c->pc4, c->pd4};
    // one CG iteration: sweep A (+ all-reduce of (p,Ap); on slabs A also
    // forms p on the halo planes), sweep B (+ all-reduce of (r,r), halo of r)
    auto iterate = [&](int it) -> cfd_status_t {
        double* pnew = P[it % CG_XFOLD];
        double* pold = P[(it + CG_XFOLD - 1) % CG_XFOLD];
        // x += alpha_j p_j of iterations it-4 .. it-1, folded by sweep A
        const bool fold = it > 0 && (it % CG_XFOLD) == 0;
        const PFold fd{P[(it + 1) % CG_XFOLD], P[(it + 2) % CG_XFOLD], fold ? x : nullptr};
        const BArgs ba{pnew, c->r};
        const int kb = HIP_KT_CG_SWEEP_B;
        const int ka = fold ? HIP_KT_CG_SWEEP_BX : HIP_KT_CG_SWEEP_A;
        timed(c, ka, [&] { launch_cgA(c, it == 0, L, c->r, pold, pnew, it, fd); }, it);
        if (D && !mbox(c)) {
            ST_TRY(timed_span(c, c->stream, HIP_KT_ALLREDUCE, [&] {
                ST_TRY(reduce_dot(c));
                hipLaunchKernelGGL(k_finish_A, dim3(1), dim3(64), 0, c->stream, c->st,
                                   c->dsum + 1, it, fold ? 1 : 0);
                return CFD_SUCCESS;
            }, it));
        }
        if (!D) timed(c, kb, [&] { launch_cgB(c, c->sgeo, L, ba, it); }, it);
        if (D) {
            // r's halo goes out on the side stream (halo communicator) as soon
            // as the two slab-edge planes of the new r exist: sweep B runs them
            // first, then the interior planes overlap the exchange; the (r,r)
            // all-reduce follows on the main stream; the next sweep A waits
            // for both
            if (c->split_b) launch_cgB(c, c->sg_edge, L, ba, it);
            else timed(c, kb, [&] { launch_cgB(c, c->sgeo, L, ba, it); }, it);
            HIP_TRY(hipEventRecord(c->ev_b, c->stream));
            HIP_TRY(hipStreamWaitEvent(c->hstream, c->ev_b, 0));
            double* rr[1] = {c->r};
            ST_TRY(timed_span(c, c->hstream, HIP_KT_HALO, [&] {
                return c->comm->halo(c->hstream, rr, 1, c->ps, (int)c->nz, false);
            }, it));
            HIP_TRY(hipEventRecord(c->ev_h, c->hstream));
            if (c->split_b) timed(c, kb, [&] { launch_cgB(c, c->sg_int, L, ba, it); }, it);
            if (!mbox(c)) {
                ST_TRY(timed_span(c, c->stream, HIP_KT_ALLREDUCE, [&] {
                    ST_TRY(reduce_dot(c));
                    hipLaunchKernelGGL(k_finish_B, dim3(1), dim3(64), 0, c->stream, c->st,
                                       c->dsum + 1, it);
                    return CFD_SUCCESS;
                }, it));
            }
            HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_h, 0));
        }
        return CFD_SUCCESS;
    };
    // Chronopoulos-Gear (cg_variant 1): k_cc1 (pointwise) -> halo of r ->
    // k_cc2 (w = A r and both dots, ONE reduction / all-reduce)
    const bool cc = (c->cfg.cg_variant == 1);
    // 3-D: the fused iteration (k_ccf; on Z-slabs + the r halo + k_cc2);
    // CFD_HIP_CCF = 0 keeps k_cc1 + k_cc2 (c->env: read at context creation)
    const bool ccf = cc && c->ccgeo.tiles_x > 0 && !c->env.ccf_off;
    auto reduce_cc = [&](int it, bool init) -> cfd_status_t {
        if (!D || mbox(c)) return CFD_SUCCESS;
        return timed_span(c, c->stream, HIP_KT_ALLREDUCE, [&] {
            ST_TRY(c->comm->allreduce_sum(c->stream, c->dsum, c->dsum + 2, 2));
            hipLaunchKernelGGL(k_finish_cc, dim3(1), dim3(64), 0, c->stream, c->st, c->dsum + 2,
                               it, (it % CG_XFOLD) == CG_XFOLD - 1 ? 1 : 0, init ? 1 : 0);
            return CFD_SUCCESS;
        }, it);
    };
    auto iterate_cc = [&](int it) -> cfd_status_t {
        double* pnew = P[it % CG_XFOLD];
        double* pold = P[(it + CG_XFOLD - 1) % CG_XFOLD];
        PPrev pv;
        for (int q = 0; q < CG_XFOLD - 1; ++q) pv.q[q] = P[(it + 1 + q) % CG_XFOLD];
        // the fold launches (x += the four pending alpha p, every 4th) time
        // apart from the plain ones
        const int kcf = (it > 0 && (it % CG_XFOLD) == CG_XFOLD - 1) ? HIP_KT_CC_FOLD
                                                                     : HIP_KT_CC_FUSED;
        if (ccf && !D) {
            timed(c, kcf,
                  [&] { launch_ccf(c, c->ccgeo, L, pnew, pold, pv, x, it, false); }, it);
            return CFD_SUCCESS;
        }
        if (ccf) {
            // Z-slabs: r_{it+1} on the two edge planes first; its halo then
            // travels on the side stream (halo communicator) while the march
            // covers the interior planes; the SpMV + reduction wait for it.
            // Fused form (default): the interior march also forms w and the
            // dot products of planes k0 + 1 .. k1 - 2, so k_cc2 covers only the
            // two edge planes (whose w needs the neighbours' r) and completes
            // the shared reduction; CFD_HIP_CCF_SLAB_FUSED=0: k_cc2 over every
            // plane (r04)
            double* r1 = ccf_r1(c, it);
            if (c->cc_edge.tiles_x > 0) {
                const bool fused = c->cc2_edge.tiles_x > 0;
                if (c->env.ccf_edge_side) {
                    // r06: the edge planes' march runs on the side stream,
                    // beside the interior march instead of before it: the
                    // two read only r_it and p_{it-1} and write disjoint
                    // planes of p_it, r_{it+1} and x (the interior march
                    // forms the edge planes' r_{it+1} it needs itself), so
                    // only the halo waits for the edge launch. The side
                    // stream first waits for the main stream (the previous
                    // iteration's reduction: alpha, beta)
                    HIP_TRY(hipEventRecord(c->ev_b, c->stream));
                    HIP_TRY(hipStreamWaitEvent(c->hstream, c->ev_b, 0));
                    launch_ccf(c, c->cc_edge, L, pnew, pold, pv, x, it, true, c->hstream);
                } else {
                    launch_ccf(c, c->cc_edge, L, pnew, pold, pv, x, it, true);
                    HIP_TRY(hipEventRecord(c->ev_b, c->stream));
                    HIP_TRY(hipStreamWaitEvent(c->hstream, c->ev_b, 0));
                }
                double* rr[1] = {r1};
                ST_TRY(timed_span(c, c->hstream, HIP_KT_HALO, [&] {
                    return c->comm->halo(c->hstream, rr, 1, c->ps, (int)c->nz, false);
                }, it));
                HIP_TRY(hipEventRecord(c->ev_h, c->hstream));
                timed(c, kcf,
                      [&] { launch_ccf(c, fused ? c->cc_int_red : c->cc_int, L, pnew, pold, pv,
                                       x, it, !fused); }, it);
                HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_h, 0));
                timed(c, HIP_KT_CC_SPMV, [&] {
                    launch_cc2(c, L, it, false, r1, false, fused ? &c->cc2_edge : nullptr);
                }, it);
            } else {
                timed(c, kcf,
                      [&] { launch_ccf(c, c->ccgeo, L, pnew, pold, pv, x, it, true); }, it);
                ST_TRY(timed_span(c, c->stream, HIP_KT_HALO, [&] { return halo(c, {r1}); }, it));
                timed(c, HIP_KT_CC_SPMV, [&] { launch_cc2(c, L, it, false, r1, false); }, it);
            }
            return reduce_cc(it, false);
        }
        timed(c, HIP_KT_CC_UPDATE, [&] { launch_cc1(c, pnew, pold, pv, x, it); }, it);
        if (D)
            ST_TRY(timed_span(c, c->stream, HIP_KT_HALO,
                              [&] { return halo(c, {c->r}); }, it));
        timed(c, HIP_KT_CC_SPMV, [&] { launch_cc2(c, L, it, false, c->r, true); }, it);
        return reduce_cc(it, false);
    };
    if (cc) {
        const size_t n = field_elems(c);
        if (!ccf && !c->cw) ST_TRY(dalloc(c, &c->cw, n));
        if (!ccf && !c->cs) ST_TRY(dalloc(c, &c->cs, n));
        if (ccf && !c->r2) ST_TRY(dalloc(c, &c->r2, n));
        // w_0 = A r_0 and alpha_0 (the textbook's first (p, Ap) with p_0 =
        // r_0); the fused iteration needs no stored w
        timed(c, HIP_KT_CC_SPMV, [&] { launch_cc2(c, L, -1, true, c->r, !ccf); });
        ST_TRY(reduce_cc(-1, true));
    }
    auto step_it = [&](int it) { return cc ? iterate_cc(it) : iterate(it); };
    // small grids: the whole solve in one cooperative launch (k_cg_small);
    // CFD_HIP_CG_SMALL = 0 never, 1 up to 64 x 256 x 16 interior cells,
    // default up to CG_SMALL_CELLS
    bool small_done = false;
    const long long ncell = (long long)(c->nx - 2) * (long long)(c->ny - 2) *
                            (long long)(c->geo.k1 - c->geo.k0);
    {
        const int mode = c->env.cg_small;
        const long long cap = (mode == 1) ? (long long)CGS_MAX_WG * CGS_THREADS * 16
                                          : (mode == 0 ? 0 : CG_SMALL_CELLS);
        if (!D && !cc && max_iter > 0 && ncell > 0 && ncell <= cap) {
            int rate_khz = 0;
            hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, c->device);
            long long ticks = (long long)std::max(rate_khz, 1000) * 1000LL * 20;  // 20 s
            unsigned nbw = (unsigned)std::min<long long>(
                CGS_MAX_WG, (ncell + CGS_THREADS - 1) / CGS_THREADS);
            Geo geo = c->geo;
            Lap lap = L;
            double* xx = x;
            unsigned* barp = c->counter + 8;
            void* args[] = {&geo, &lap, &xx, &c->r, &c->pa, &c->pb, &c->st, &c->partials,
                            &barp, &ticks};
            ST_TRY(timed_span(c, c->stream, HIP_KT_CG_SMALL, [&]() -> cfd_status_t {
                HIP_TRY(hipMemsetAsync(barp, 0, sizeof(unsigned), c->stream));
                if (hipLaunchCooperativeKernel((const void*)k_cg_small, dim3(nbw),
                                               dim3(CGS_THREADS), args, 0,
                                               c->stream) == hipSuccess)
                    small_done = true;
                else
                    (void)hipGetLastError();  // not co-resident here: the sweep loop
                return CFD_SUCCESS;
            }));
        }
    }
    int it = 0;
    if (max_iter > 0 && !small_done) {
        ST_TRY(step_it(0));
        it = 1;
    }
    if (!small_done)
        ST_TRY(poll_loop(c, c->st, it, max_iter, [&](int& i) -> cfd_status_t {
            ST_TRY(step_it(i));
            ++i;
            return CFD_SUCCESS;
        }));
    PRing pr;
    for (int q = 0; q < CG_XFOLD; ++q) pr.p[q] = P[q];
    klaunch(c, k_cg_finalize, dim3(G), dim3(NT), c->geo, pr, x, c->st);
    CgState s;
    ST_TRY(poll_final(c, c->st, &s));
    flush_timing(c, s.iterations);
    if (s.status == ST_COMM_TIMEOUT) {
        set_err(CFD_ERROR, small_done
                               ? "projection_hip: small-grid CG grid barrier timed out"
                               : "projection_hip: slab all-reduce timed out (a rank stopped)");
        return CFD_ERROR;
    }
    const bool stagnated = (s.status == ST_STAGNATED);
    // final poisson_solver_apply_bc (cg.c:447); the breakdown exit skips it.
    if (final_bc && neumann && !stagnated && !(s.iterations == 0 && s.status == ST_CONVERGED))
        launch_bc(c, x, 0, dv);
    ST_TRY(halo(c, {x}));
    return finish_stats(c, s, s.res);
}

// ---------------------------------------------------------------------------
// BiCGSTAB (bicgstab.hpp): one device, rhs from c->rhs, x in c->pn. p_it and
// v_it live in the p ring: p in pa / pb and v in pc4 / pd4, by the parity of it.
// ---------------------------------------------------------------------------
// one iteration: its three launches
static void launch_bcg(hip_proj_ctx* c, const Lap& L, int it) {
    BcgState* st = c->bcgst;
    double* pn = (it & 1) ? c->pb : c->pa;
    double* po = (it & 1) ? c->pa : c->pb;
    double* vn = (it & 1) ? c->pd4 : c->pc4;
    double* vo = (it & 1) ? c->pc4 : c->pd4;
    with_int<8, 4, 16>(c->sweep_ty, [&](auto TY) {
        const dim3 grid(sweep_grid(c)), blk(64 * TY);
        timed(c, HIP_KT_BCG_V, [&] {
            klaunch(c, it == 0 ? k_bcg_sweep<TY, 0, true> : k_bcg_sweep<TY, 0, false>, grid, blk,
                    c->sgeo, L, c->r, po, vo, c->rhat, pn, vn, st, c->bcg_part, c->counter, it);
        }, it);
        timed(c, HIP_KT_BCG_T, [&] {
            klaunch(c, k_bcg_sweep<TY, 1, false>, grid, blk, c->sgeo, L, c->r, vn, nullptr,
                    nullptr, c->bs, c->bt, st, c->bcg_part, c->counter, it);
        }, it);
        timed(c, HIP_KT_BCG_X, [&] {
            klaunch(c, k_bcg_x<TY>, grid, blk, c->sgeo, c->pn, pn, c->bs, c->bt, c->rhat, c->r,
                    st, c->bcg_part, c->counter, it);
        }, it);
    });
}

static cfd_status_t bicgstab_solve(hip_proj_ctx* c, double dx, double dy, double dz,
                                   double rel_tol, double abs_tol, int max_iter,
                                   int check_interval) {
    const Lap L = make_lap(dx, dy, dz);
    const int G = tile_grid(c);
    const DirVals dv{};
    double* x = c->pn;
    const size_t n = field_elems(c);
    if (!c->rhat) ST_TRY(dalloc(c, &c->rhat, n));
    if (!c->bs) ST_TRY(dalloc(c, &c->bs, n));
    if (!c->bt) ST_TRY(dalloc(c, &c->bt, n));
    if (!c->bcgst) HIP_TRY(hipMalloc((void**)&c->bcgst, sizeof(BcgState)));
    if (!c->bcg_part)
        HIP_TRY(hipMalloc((void**)&c->bcg_part,
                          sizeof(double) * (size_t)std::max(3 * sweep_grid(c), G)));
    ST_TRY(clear_cg_scratch(c));  // as cg_solve: zero walls of r and of the ring (p, v)
    // poisson_solver_apply_bc(x) at solve start (linear_solver_bicgstab.c:295)
    const bool neumann = (c->poisson_bc == HIP_POISSON_BC_NEUMANN);
    if (neumann) launch_bc(c, x, 0, dv);
    timed(c, HIP_KT_CG_SETUP, [&] {
        klaunch(c, k_bcg_setup, dim3(G), dim3(NT), c->geo, L, c->rhs, x, c->r, c->rhat, c->bcgst,
                c->bcg_part, c->counter, rel_tol, abs_tol, max_iter, check_interval);
    });
    int it = 0;
    ST_TRY(poll_loop(c, c->bcgst, it, max_iter, [&](int& i) {
        launch_bcg(c, L, i++);
        return CFD_SUCCESS;
    }));
    klaunch(c, k_bcg_finalize, dim3(G), dim3(NT), c->geo, c->pa, c->pb, x, c->bcgst);
    BcgState s;
    ST_TRY(poll_final(c, c->bcgst, &s));
    flush_timing(c, s.iterations);
    if (!s.done) {
        set_err(CFD_ERROR, "projection_hip: BiCGSTAB device loop ended without a decision");
        return CFD_ERROR;
    }
    // the closing poisson_solver_apply_bc (:483): every breakdown exit and the
    // converged-at-start return leave before it
    if (neumann && s.status != ST_STAGNATED &&
        !(s.iterations == 0 && s.status == ST_CONVERGED && s.res0 < s.abs_tol))
        launch_bc(c, x, 0, dv);
    return finish_stats(c, s, s.res);
}

// the direct sine- and cosine-transform solvers: use ensure_aux and the poll
// helpers
#include "transform_solve.hpp"
