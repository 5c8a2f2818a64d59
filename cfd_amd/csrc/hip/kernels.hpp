// kernels.hpp -- the gfx950 kernels of the projection step and of its CG
// pressure solve: the CG sweeps and the small-grid CG, the energy and thermal
// kernels, the predictor and corrector. Included by one translation unit
// only, projection_hip.hip (through poisson_solve.hpp), so that its
// non-template kernels are emitted once. What other units share with it is in
// device_util.hpp; the relaxation kernels are in relax_kernels.hpp
// (relax_solve.hip), the integrators' in rk_kernels.hpp (rk4_hip.hip) and
// k_bc_shell in bc_gpu.hip.
#pragma once

#include "device_util.hpp"

namespace cfdhip {

// Laplacian exactly as linear_solver_cg.c:113-116 groups it.
__device__ __forceinline__ double lap7(const Lap& L, double c, double xm, double xp, double ym,
                                       double yp, double zm, double zp) {
    return ((xp - (2.0 * c) + xm) * L.dx2_inv) + ((yp - (2.0 * c) + ym) * L.dy2_inv) +
           ((zp + zm - (2.0 * c)) * L.inv_dz2);
}

// ---------------------------------------------------------------------------
// CG state transitions, run by one thread once a dot product's global total is
// known: inline in the last workgroup on one device, or in a 1-thread k_finish_*
// kernel after the cross-rank all-reduce of the per-rank totals (Z-slabs).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void fin_setup(CgState* st, double tot, double rel_tol, double abs_tol,
                                          int max_iter, int check_interval) {
    double res0 = sqrt(tot);                   // linear_solver_cg.c:345
    double tol = rel_tol * res0;               // :352-355
    if (tol < abs_tol) tol = abs_tol;
    st->rho = tot;
    st->res0 = res0;
    st->res = res0;
    st->tol = tol;
    st->abs_tol = abs_tol;
    for (int q = 0; q < CG_XFOLD; ++q) st->alpha[q] = 0.0;
    st->beta = 0.0;
    st->pAp = 0.0;
    st->iterations = 0;
    st->nalpha = 0;
    st->xdone = 0;
    st->max_iter = max_iter;
    st->check_interval = check_interval;
    if (res0 < abs_tol || max_iter <= 0) {     // :357-365
        st->done = 1;
        st->status = (res0 < abs_tol) ? ST_CONVERGED : ST_MAX_ITER;
    } else {
        st->done = 0;
        st->status = ST_MAX_ITER;
    }
}

// after (p, Ap): alpha or pAp breakdown (linear_solver_cg.c:395-407)
__device__ __forceinline__ void fin_A(CgState* st, double tot, int it, bool fold = false) {
    if (fold) st->xdone = it;  // this sweep A folded alpha_j p_j, j < it, into x
    st->pAp = tot;
    if (fabs(tot) < 1e-30) {
        st->done = 1;
        st->status = ST_STAGNATED;
        st->iterations = it + 1;
    } else {
        st->alpha[it % CG_XFOLD] = st->rho / tot;
        st->nalpha = it + 1;
    }
}

// after (r, r): convergence test, rho breakdown, beta (linear_solver_cg.c:416-445)
__device__ __forceinline__ void fin_B(CgState* st, double tot, int it) {
    double res = sqrt(tot);
    st->res = res;
    st->iterations = it + 1;
    const bool check = (it % st->check_interval) == 0;
    const bool conv = (res < st->tol) || (res < st->abs_tol);
    if (check && conv) {
        st->done = 1;
        st->status = ST_CONVERGED;
    } else if (fabs(st->rho) < 1e-30) {
        st->done = 1;
        st->status = ST_STAGNATED;
    } else {
        st->beta = tot / st->rho;
        st->rho = tot;
        if (it + 1 >= st->max_iter) {
            st->done = 1;
            st->status = conv ? ST_CONVERGED : ST_MAX_ITER;
        }
    }
}

__device__ __forceinline__ void comm_fail(CgState* st) {
    st->done = 1;
    st->status = ST_COMM_TIMEOUT;
}

static __global__ void k_finish_setup(CgState* st, const double* tot, double rel_tol, double abs_tol,
                               int max_iter, int check_interval) {
    if (threadIdx.x == 0) fin_setup(st, tot[0], rel_tol, abs_tol, max_iter, check_interval);
}
static __global__ void k_finish_A(CgState* st, const double* tot, int it, int fold) {
    if (threadIdx.x == 0 && !st->done) fin_A(st, tot[0], it, fold != 0);
}
static __global__ void k_finish_B(CgState* st, const double* tot, int it) {
    if (threadIdx.x == 0 && !st->done) fin_B(st, tot[0], it);
}

// ---------------------------------------------------------------------------
// CG setup: r = -rhs + lap(x) (linear_solver_cg.c:134-158) and rho = (r, r).
// FROM_VEL: rhs = (rho/dt) * div(u*) computed on the fly exactly as
// solver_projection.c:195-214 (the rhs array is never materialised for CG);
// otherwise rhs is read from memory. WRITE_RHS stores the rhs for the
// relaxation solvers, which re-read it every sweep.
// ---------------------------------------------------------------------------
struct DivCoef {
    double two_dx, two_dy;   // 2.0*dx, 2.0*dy (divided by, as the reference does)
    double inv_2dz;          // 1/(2dz), 0 in 2-D
    double rho_over_dt;
};

template <bool FROM_VEL, bool WRITE_RHS, bool WITH_RR, bool DIST = false>
static __global__ __launch_bounds__(NT) void k_cg_setup(Geo g, Lap L, DivCoef dc,
                                                 const double* __restrict__ us,
                                                 const double* __restrict__ vs,
                                                 const double* __restrict__ ws,
                                                 double* __restrict__ rhs,
                                                 const double* __restrict__ x,
                                                 double* __restrict__ r, CgState* st,
                                                 double* partials, unsigned* counter,
                                                 double rel_tol, double abs_tol, int max_iter,
                                                 int check_interval, double* dsum,
                                                 Mbox* mb) {
    __shared__ double sh[NWAVE];
    __shared__ int flag;
    double acc = 0.0;
    const int ntiles = g.tiles_x * g.tiles_y * g.tiles_z;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        TileCoord c = tile_coord(g, t);
        if (!c.active) continue;
        long long idx = cidx(g, c.i, c.j, c.kb);
        double xm = x[idx - g.sz], xc = x[idx];
        for (int k = c.kb; k < c.ke; ++k, idx += g.ps) {
            double xp = x[idx + g.sz];
            double b;
            if (FROM_VEL) {
                double dus = (us[idx + 1] - us[idx - 1]) / dc.two_dx;
                double dvs = (vs[idx + g.px] - vs[idx - g.px]) / dc.two_dy;
                double dws = (ws[idx + g.sz] - ws[idx - g.sz]) * dc.inv_2dz;
                double div = dus + dvs + dws;
                b = dc.rho_over_dt * div;
                if (WRITE_RHS) rhs[idx] = b;
            } else {
                b = rhs[idx];
            }
            double lap = lap7(L, xc, x[idx - 1], x[idx + 1], x[idx - g.px], x[idx + g.px], xm, xp);
            double rv = -b + lap;
            if (WITH_RR) {
                r[idx] = rv;
                acc += rv * rv;
            }
            xm = xc;
            xc = xp;
        }
    }
    if (!WITH_RR) return;
    double bt = block_sum(acc, sh);
    double tot;
    if (grid_sum_last(bt, partials, counter, sh, &flag, tot) && threadIdx.x == 0) {
        if (DIST && mb) {
            double g;
            if (mbox_allreduce(mb, tot, &g)) fin_setup(st, g, rel_tol, abs_tol, max_iter, check_interval);
            else comm_fail(st);
        } else if (DIST) {
            dsum[0] = tot;
        } else {
            fin_setup(st, tot, rel_tol, abs_tol, max_iter, check_interval);
        }
    }
}

// ===========================================================================
// Production CG sweeps ("row-pair" kernels).
//
// Tile = 128 (x) x TY (y) x kc (z); one wavefront per y row, each lane owns
// the x pair (i0, i0+1) and moves it with 16-B loads/stores (the streaming
// width MI355X's memory path prefers). x neighbours come from the adjacent
// lanes (__shfl), y neighbours from the TY+2 rows the workgroup's waves
// publish in LDS each plane (double-buffered, one barrier per plane), z
// neighbours from registers. Workgroups are mapped to tiles XCD-aware: the 8
// XCDs each get a contiguous band of tiles, so the y halo rows a workgroup
// reads were just streamed into the same XCD's L2 by its neighbour.
// Measured at 512^3 (tools/mb/stencil_mb6.hip): 5.2 TB/s for sweep A versus
// 4.3-4.5 TB/s for one-cell-per-lane designs.
// ===========================================================================
// SGeo, the tiling of one launch: tile_plan.hpp

template <bool NT>
__device__ __forceinline__ double2 ld2n(const double* p, long long i) {
    if (NT) {
        d2x w = __builtin_nontemporal_load(reinterpret_cast<const d2x*>(p + i));
        return make_double2(w.x, w.y);
    }
    return *reinterpret_cast<const double2*>(p + i);
}

__device__ __forceinline__ double2 fma2p(double2 a, double beta, double2 b) {
    return make_double2(a.x + beta * b.x, a.y + beta * b.y);
}

// Sweep A (iteration it):  p_it = r + beta p_{it-1} (FIRST: p = r), written
// to pnew; (p, A p) with A p in registers.
// FOLD (it % CG_XFOLD == 0, it > 0): x = (((x + a_{it-4} p_{it-4}) +
// a_{it-3} p_{it-3}) + a_{it-2} p_{it-2}) + a_{it-1} p_{it-1}, the
// reference's per-iteration updates x += alpha p (linear_solver_cg.c:379-380,
// axpy :85-96) in their order with the partial sums in registers, so x is
// bitwise the reference's while it is read and written every fourth
// iteration only. p_{it-1} = p_old is already streamed by this sweep and
// p_{it-4} is the ring slot p_it is written to (read before the write, same
// lane), so the fold costs x, p_{it-3}, p_{it-2} and the x store.
struct PFold {
    const double* q3;  // p_{it-3}
    const double* q2;  // p_{it-2}
    double* x;
};

template <int TY, bool FIRST, bool DIST, int FL = 0, bool FOLD = false>
static __global__ __launch_bounds__(64 * TY, sweep_min_waves<FL>()) void k_cgA(
    SGeo g, Lap L, const double* __restrict__ r, const double* __restrict__ po,
    double* __restrict__ pn, CgState* st, double* partials, unsigned* counter, int it,
    double* dsum, Mbox* mb, PFold fd) {
    constexpr bool PF = (FL & SW_PREFETCH) != 0;
    __shared__ double2 rows[2][TY + 2][64];
    __shared__ double sh[TY];
    __shared__ int flag;
    if (st->done) return;
    const double beta = FIRST ? 0.0 : st->beta;
    double fa[CG_XFOLD];  // alpha_{it-4} .. alpha_{it-1}
#pragma unroll
    for (int q = 0; q < CG_XFOLD; ++q) fa[q] = FOLD ? st->alpha[(it + q) % CG_XFOLD] : 0.0;
    const double* __restrict__ fq3 = fd.q3;
    const double* __restrict__ fq2 = fd.q2;
    double* __restrict__ fx = fd.x;
    RowPair c = row_pair<TY>(g);
    const bool halo = (c.w == 0) || (c.w == TY - 1);
    const int jh = (c.w == 0) ? max(c.j - 1, 0) : min(c.j + 1, g.ny - 1);
    const int hslot = (c.w == 0) ? 0 : TY + 1;
    const long long hoff = (long long)(jh - min(c.j, g.ny - 1)) * g.px;
    const bool xok = c.i0 < g.nx;
    const bool eok_l = c.lane == 0 && c.i0 >= 1 && xok;
    const bool eok_r = c.lane == 63 && c.i0 + 2 < g.nx;
    constexpr bool E1 = (FL & SW_EDGE1) != 0;
    const bool eok = eok_l || eok_r;
    const long long eoff = (c.lane == 0) ? -1 : 2;
    const bool inner = (FL & SW_NT_INNER) && !halo;
    const double2 zero = make_double2(0.0, 0.0);
    // raw r / p_old of: the centre of plane k+1, the y-halo row of plane k+1,
    // the x-edge cells of plane k (p is formed from them when used; with
    // SW_EDGE1 lane 0's left and lane 63's right cell share lr / lo)
    struct Bundle {
        double2 cr, co, hr, ho;
        double lr, lo, rr, ro;
        double2 fxo, f4, f3, f2;  // FOLD: x, p_{it-4}, p_{it-3}, p_{it-2} of plane k
    };
    auto issue = [&](int k, long long ix) __attribute__((always_inline)) {
        const double2 zero = make_double2(0.0, 0.0);  // a value, not the captured object
        Bundle b;
        const long long ip = ix + g.sz;
        if (inner) {
            b.cr = xok ? ld2n<true>(r, ip) : zero;
            b.co = (xok && !FIRST) ? ld2n<true>(po, ip) : zero;
        } else {
            b.cr = xok ? ld2(r, ip) : zero;
            b.co = (xok && !FIRST) ? ld2(po, ip) : zero;
        }
        const bool h = xok && halo && k + 1 < c.ke;
        b.hr = h ? ld2(r, ip + hoff) : zero;
        b.ho = (h && !FIRST) ? ld2(po, ip + hoff) : zero;
        if (E1) {
            b.lr = eok ? r[ix + eoff] : 0.0;
            b.lo = (eok && !FIRST) ? po[ix + eoff] : 0.0;
            b.rr = b.ro = 0.0;
        } else {
            b.lr = eok_l ? r[ix - 1] : 0.0;
            b.lo = (eok_l && !FIRST) ? po[ix - 1] : 0.0;
            b.rr = eok_r ? r[ix + 2] : 0.0;
            b.ro = (eok_r && !FIRST) ? po[ix + 2] : 0.0;
        }
        const bool fl = FOLD && xok && c.act;
        b.fxo = fl ? ld2v<FL>(fx, ix) : zero;
        b.f4 = fl ? ld2v<FL>(pn, ix) : zero;
        b.f3 = fl ? ld2v<FL>(fq3, ix) : zero;
        b.f2 = fl ? ld2v<FL>(fq2, ix) : zero;
        return b;
    };
    auto form2 = [&](double2 a, double2 b) { return FIRST ? a : fma2p(a, beta, b); };
    auto form1 = [&](double a, double b) { return FIRST ? a : a + beta * b; };
    double acc = 0.0;
    long long idx = c.idx;
    double2 pm = xok ? form2(ld2(r, idx - g.sz), FIRST ? zero : ld2(po, idx - g.sz)) : zero;
    // raw p_{it-1} of the current plane (the fold's last term)
    double2 praw = (FOLD && xok) ? ld2(po, idx) : zero;
    double2 pc = xok ? form2(ld2(r, idx), FIRST ? zero : (FOLD ? praw : ld2(po, idx))) : zero;
    double2 hc = (xok && halo) ? form2(ld2(r, idx + hoff), FIRST ? zero : ld2(po, idx + hoff))
                               : zero;
    // Z-slabs: p is pointwise in r and p_old, so the tiles at the slab ends
    // also write the new p on the halo planes (r's halo is exchanged after
    // sweep B); sweep B then needs no halo exchange of p.
    if (DIST && c.act && c.kb == g.k0) {
        double2 pw;
        pw.x = c.in0 ? pm.x : 0.0;
        pw.y = c.in1 ? pm.y : 0.0;
        st2(pn, idx - g.sz, pw);
    }
    Bundle cur;
    if (PF) cur = issue(c.kb, idx);
    int buf = 0;
    for (int k = c.kb; k < c.ke; ++k, idx += g.ps) {
        Bundle nxt;
        if (PF) {
            if (k + 1 < c.ke) nxt = issue(k + 1, idx + g.ps);
        } else {
            cur = issue(k, idx);
        }
        rows[buf][c.w + 1][c.lane] = pc;
        if (halo) rows[buf][hslot][c.lane] = hc;
        __syncthreads();
        const double2 ys = rows[buf][c.w][c.lane];
        const double2 yn = rows[buf][c.w + 2][c.lane];
        const double2 pp = form2(cur.cr, cur.co);
        double left = __shfl_up(pc.y, 1, 64);
        double right = __shfl_down(pc.x, 1, 64);
        if (c.lane == 0) left = form1(cur.lr, cur.lo);
        if (c.lane == 63) right = E1 ? form1(cur.lr, cur.lo) : form1(cur.rr, cur.ro);
        const double Ap0 = -lap7(L, pc.x, left, pc.y, ys.x, yn.x, pm.x, pp.x);
        const double Ap1 = -lap7(L, pc.y, pc.x, right, ys.y, yn.y, pm.y, pp.y);
        if (FOLD && c.act) {
            double2 xw;
            xw.x = c.in0 ? (((cur.fxo.x + fa[0] * cur.f4.x) + fa[1] * cur.f3.x) + fa[2] * cur.f2.x) +
                               fa[3] * praw.x
                         : cur.fxo.x;
            xw.y = c.in1 ? (((cur.fxo.y + fa[0] * cur.f4.y) + fa[1] * cur.f3.y) + fa[2] * cur.f2.y) +
                               fa[3] * praw.y
                         : cur.fxo.y;
            st2v<FL>(fx, idx, xw);
        }
        if (c.act) {
            double2 pw;
            pw.x = c.in0 ? pc.x : 0.0;
            pw.y = c.in1 ? pc.y : 0.0;
            st2v<FL>(pn, idx, pw);
        }
        if (c.in0) acc += pc.x * Ap0;
        if (c.in1) acc += pc.y * Ap1;
        pm = pc;
        pc = pp;
        if (FOLD) praw = cur.co;
        hc = form2(cur.hr, cur.ho);
        if (PF) cur = nxt;
        buf ^= 1;
    }
    if (DIST && c.act && c.ke == g.k1) {  // pc = p on plane k1 (upper halo)
        double2 pw;
        pw.x = c.in0 ? pc.x : 0.0;
        pw.y = c.in1 ? pc.y : 0.0;
        st2(pn, idx, pw);
    }
    // deterministic workgroup sum: wave tree, then waves in order
    acc = wave_sum(acc);
    if (c.lane == 0) sh[c.w] = acc;
    __syncthreads();
    double bt = 0.0;
    if (threadIdx.x == 0)
        for (int q = 0; q < TY; ++q) bt += sh[q];
    double tot;
    double* shs = (double*)&rows[0][0][0];
    if (grid_sum_last_n<64 * TY>(bt, partials, counter, shs, &flag, tot) && threadIdx.x == 0) {
        if (DIST && mb) {
            double g;
            if (mbox_allreduce(mb, tot, &g)) fin_A(st, g, it, FOLD);
            else comm_fail(st);
        } else if (DIST) {
            dsum[0] = tot;
        } else {
            fin_A(st, tot, it, FOLD);
        }
    }
}

// Sweep B (iteration it): r -= alpha A p (A p recomputed from p, bitwise equal
// to sweep A's), rho_new = (r, r), convergence test and beta. (x is folded by
// sweep A every CG_XFOLD iterations, k_cgA<FOLD>.)
struct PRing {
    const double* p[CG_XFOLD];  // p_j at [j % CG_XFOLD]
};
struct PPrev {
    const double* q[CG_XFOLD - 1];  // p_{it-3}, p_{it-2}, p_{it-1}
};

// REV (r03, one device, 3-D): the tile marches z downwards. Sweep A marches
// upwards, so each sweep starts on the planes the previous one touched last,
// which the 256 MB Infinity Cache still holds (p just written by sweep A,
// r just read by it; then r just written by sweep B for the next sweep A).
// The z neighbours keep their roles in lap7, so A p is bitwise sweep A's; only
// the order of the (r, r) partial sums within a tile changes.
template <int TY, bool DIST, int FL = 0, bool REV = false>
static __global__ __launch_bounds__(64 * TY, sweep_min_waves<FL>()) void k_cgB(
    SGeo g, Lap L, const double* __restrict__ p, double* __restrict__ r, CgState* st,
    double* partials, unsigned* counter, int it, double* dsum, Mbox* mb) {
    constexpr bool PF = (FL & SW_PREFETCH) != 0;
    __shared__ double2 rows[2][TY + 2][64];
    __shared__ double sh[TY];
    __shared__ int flag;
    if (st->done) return;
    const double malpha = -st->alpha[it % CG_XFOLD];
    RowPair c = row_pair<TY>(g);
    const bool halo = (c.w == 0) || (c.w == TY - 1);
    const int jh = (c.w == 0) ? max(c.j - 1, 0) : min(c.j + 1, g.ny - 1);
    const int hslot = (c.w == 0) ? 0 : TY + 1;
    const long long hoff = (long long)(jh - min(c.j, g.ny - 1)) * g.px;
    const bool xok = c.i0 < g.nx;
    const bool eok_l = c.lane == 0 && c.i0 >= 1 && xok;
    const bool eok_r = c.lane == 63 && c.i0 + 2 < g.nx;
    constexpr bool E1 = (FL & SW_EDGE1) != 0;
    const bool eok = eok_l || eok_r;
    const long long eoff = (c.lane == 0) ? -1 : 2;
    const bool inner = (FL & SW_NT_INNER) && !halo;
    const double2 zero = make_double2(0.0, 0.0);
    // p of the centre and y-halo row of plane k+1; r and the x-edge p of
    // plane k (SW_EDGE1: both edge cells in el)
    struct Bundle {
        double2 pp, hp, rr;
        double el, er;
    };
    // sd: the z stride towards the next plane of the march
    const long long sd = REV ? -g.sz : g.sz;
    const long long pstep = REV ? -g.ps : g.ps;
    auto issue = [&](int k, long long ix) __attribute__((always_inline)) {
        const double2 zero = make_double2(0.0, 0.0);  // a value, not the captured object
        Bundle b;
        const long long ip = ix + sd;
        const bool more = REV ? (k - 1 >= c.kb) : (k + 1 < c.ke);
        if (inner) b.pp = xok ? ld2n<true>(p, ip) : zero;
        else b.pp = xok ? ld2(p, ip) : zero;
        b.hp = (xok && halo && more) ? ld2(p, ip + hoff) : zero;
        b.rr = xok ? ld2v<FL>(r, ix) : zero;
        if (E1) {
            b.el = eok ? p[ix + eoff] : 0.0;
            b.er = 0.0;
        } else {
            b.el = eok_l ? p[ix - 1] : 0.0;
            b.er = eok_r ? p[ix + 2] : 0.0;
        }
        return b;
    };
    double acc = 0.0;
    const int k_first = REV ? c.ke - 1 : c.kb;
    long long idx = c.idx + (REV ? (long long)(c.ke - 1 - c.kb) * g.ps : 0LL);
    // pm: the plane the march left (z- forwards, z+ in REV), pp: the next one
    double2 pm = xok ? ld2(p, idx - sd) : zero;
    double2 pc = xok ? ld2(p, idx) : zero;
    double2 hc = (xok && halo) ? ld2(p, idx + hoff) : zero;
    Bundle cur;
    if (PF) cur = issue(k_first, idx);
    int buf = 0;
    for (int n = 0, k = k_first; n < c.ke - c.kb; ++n, k += REV ? -1 : 1, idx += pstep) {
        Bundle nxt;
        if (PF) {
            if (n + 1 < c.ke - c.kb) nxt = issue(REV ? k - 1 : k + 1, idx + pstep);
        } else {
            cur = issue(k, idx);
        }
        rows[buf][c.w + 1][c.lane] = pc;
        if (halo) rows[buf][hslot][c.lane] = hc;
        __syncthreads();
        const double2 ys = rows[buf][c.w][c.lane];
        const double2 yn = rows[buf][c.w + 2][c.lane];
        const double2 pp = cur.pp;
        double left = __shfl_up(pc.y, 1, 64);
        double right = __shfl_down(pc.x, 1, 64);
        if (c.lane == 0) left = cur.el;
        if (c.lane == 63) right = E1 ? cur.el : cur.er;
        const double2 zm = REV ? pp : pm, zp = REV ? pm : pp;
        const double Ap0 = -lap7(L, pc.x, left, pc.y, ys.x, yn.x, zm.x, zp.x);
        const double Ap1 = -lap7(L, pc.y, pc.x, right, ys.y, yn.y, zm.y, zp.y);
        double2 rn;
        rn.x = c.in0 ? cur.rr.x + malpha * Ap0 : cur.rr.x;
        rn.y = c.in1 ? cur.rr.y + malpha * Ap1 : cur.rr.y;
        if (c.act) st2v<FL>(r, idx, rn);
        if (c.in0) acc += rn.x * rn.x;
        if (c.in1) acc += rn.y * rn.y;
        pm = pc;
        pc = pp;
        hc = cur.hp;
        if (PF) cur = nxt;
        buf ^= 1;
    }
    acc = wave_sum(acc);
    if (c.lane == 0) sh[c.w] = acc;
    __syncthreads();
    double bt = 0.0;
    if (threadIdx.x == 0)
        for (int q = 0; q < TY; ++q) bt += sh[q];
    double tot;
    double* shs = (double*)&rows[0][0][0];
    if (grid_sum_last_n<64 * TY>(bt, partials, counter, shs, &flag, tot, g.part_ofs,
                                 g.part_total) &&
        threadIdx.x == 0) {
        if (DIST && mb) {
            double g2;
            if (mbox_allreduce(mb, tot, &g2)) fin_B(st, g2, it);
            else comm_fail(st);
        } else if (DIST) {
            dsum[0] = tot;
        } else {
            fin_B(st, tot, it);
        }
    }
}

// ---------------------------------------------------------------------------
// Whole CG solve in ONE persistent launch for small grids (r02b). On a
// 128 x 128 grid a CG iteration's two sweeps cost ~15 us, nearly all kernel
// dispatch and completion. Here one cooperative launch runs
// every iteration: phase A (p = r + beta p_old, A p, (p, Ap)), a grid barrier,
// phase B (x += alpha p, r -= alpha A p, (r, r)), a grid barrier (up to 256
// workgroups, one per 256 interior cells). Every
// workgroup sums the per-workgroup partials in the same order and applies
// the state transition (fin_A / fin_B) to its own LDS copy of the CG state,
// so all leave the loop at the same iteration with no extra barrier. r and
// the two p buffers are shared between workgroups inside the launch, so they
// move through agent-scope atomic loads / stores (coherent across the XCDs'
// L2s); x is only touched by its own cell. Per-cell arithmetic is the
// sweeps' (same lap7 operands, p = r + beta p_old, r + (-alpha) A p,
// x + alpha p per iteration, which is bitwise the sweeps' x fold); only the
// dot-product summation order differs, as between the sweep kernels and the
// reference. The barrier wait is bounded (a timeout ends the solve with
// ST_COMM_TIMEOUT instead of hanging the GPU).
// ---------------------------------------------------------------------------
constexpr int CGS_THREADS = 256;
constexpr long long CG_SMALL_CELLS = 300000;  // default ceiling (interior cells): 64^3 yes, 96^3 no

static __global__ __launch_bounds__(CGS_THREADS) void k_cg_small(Geo g, Lap L,
                                                                 double* __restrict__ x, double* r,
                                                                 double* pa, double* pb,
                                                                 CgState* st, double* partials,
                                                                 unsigned* bar,
                                                                 long long timeout_ticks) {
    __shared__ CgState ls;
    __shared__ double sh[CGS_THREADS / 64];
    __shared__ int bad;
    const unsigned nb = gridDim.x;
    const long long nxi = g.nx - 2, nyi = g.ny - 2;
    const long long ncell = nxi * nyi * (long long)(g.k1 - g.k0);
    if (threadIdx.x == 0) {
        ls = *st;
        bad = 0;
    }
    __syncthreads();
    unsigned target = 0;
    auto barrier = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores landed
        __syncthreads();
        target += nb;
        if (threadIdx.x == 0) {
            __hip_atomic_fetch_add((gu32*)bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const long long t0 = wall_clock64();
            while (__hip_atomic_load((gu32*)bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <
                   target) {
                __builtin_amdgcn_s_sleep(1);
                if (wall_clock64() - t0 > timeout_ticks) {
                    bad = 1;
                    break;
                }
            }
        }
        __syncthreads();
    };
    // block partial -> partials[slot][block] -> barrier (gsum_begin); every
    // workgroup then sums the partials in the same fixed tree (gsum_end,
    // total in thread 0). The next phase's loads of each thread's first cell
    // are issued between the two, so they overlap the partials' round trip.
    auto gsum_begin = [&](int slot, double v) __attribute__((always_inline)) {
        v = wave_sum(v);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double b = 0.0;
#pragma unroll
            for (int w = 0; w < CGS_THREADS / 64; ++w) b += sh[w];
            store_sc1(&partials[slot * CGS_MAX_WG + blockIdx.x], b);
        }
        barrier();
    };
    auto gsum_end = [&](int slot) __attribute__((always_inline)) {
        double t = (threadIdx.x < nb) ? load_sc1(&partials[slot * CGS_MAX_WG + threadIdx.x]) : 0.0;
        t = wave_sum(t);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = t;
        __syncthreads();
        double tot = 0.0;
        if (threadIdx.x == 0) {
#pragma unroll
            for (int w = 0; w < CGS_THREADS / 64; ++w) tot += sh[w];
        }
        __syncthreads();  // sh is reused by the next reduction
        return tot;
    };
    auto cell = [&](long long e) __attribute__((always_inline)) {
        const long long i = 1 + e % nxi;
        const long long q = e / nxi;
        const long long j = 1 + q % nyi;
        const long long k = g.k0 + q / nyi;
        return k * g.ps + j * g.px + i;
    };
    const long long stride = (long long)nb * CGS_THREADS;
    const long long e0 = (long long)blockIdx.x * CGS_THREADS + threadIdx.x;
    const bool has0 = e0 < ncell;
    const long long c0 = cell(has0 ? e0 : 0);  // a valid address either way
    // the 7 stencil points of a cell: centre, x-, x+, y-, y+, z-, z+
    auto pts = [&](long long c, long long (&q)[7]) __attribute__((always_inline)) {
        q[0] = c; q[1] = c - 1; q[2] = c + 1; q[3] = c - g.px; q[4] = c + g.px;
        q[5] = c - g.sz; q[6] = c + g.sz;
    };
    long long q0s[7];
    pts(c0, q0s);
    // phase A operands of cell c0: r and p_old at its stencil points
    double ar[7], ap[7];
    auto loadA = [&](const double* po_, bool first_) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            ar[t] = load_sc1(&r[q0s[t]]);
            ap[t] = first_ ? 0.0 : load_sc1(&po_[q0s[t]]);
        }
    };
    // phase A of one cell from its operands: p = r + beta p_old, A p
    auto cellA = [&](long long c, const double (&rv)[7], const double (&pv)[7], bool first_,
                     double beta, double* pn_, double& acc) __attribute__((always_inline)) {
        double pp[7];
#pragma unroll
        for (int t = 0; t < 7; ++t) pp[t] = first_ ? rv[t] : rv[t] + beta * pv[t];
        const double Ap = -lap7(L, pp[0], pp[1], pp[2], pp[3], pp[4], pp[5], pp[6]);
        store_sc1(&pn_[c], pp[0]);
        acc += pp[0] * Ap;
    };
    // phase B operands of cell c0: p_it at its stencil points, r, x
    double bp[7], brr, bx;
    auto loadB = [&](const double* pn_) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 7; ++t) bp[t] = load_sc1(&pn_[q0s[t]]);
        brr = load_sc1(&r[c0]);
        bx = x[c0];
    };
    auto cellB = [&](long long c, const double (&pv)[7], double rv, double xv, double al,
                     double ma, double& acc) __attribute__((always_inline)) {
        const double Ap = -lap7(L, pv[0], pv[1], pv[2], pv[3], pv[4], pv[5], pv[6]);
        x[c] = xv + al * pv[0];
        const double rn = rv + ma * Ap;
        store_sc1(&r[c], rn);
        acc += rn * rn;
    };
    loadA(pb, true);  // iteration 0: p = r
    for (int it = 0;; ++it) {
        if (ls.done) break;
        double* pn = (it & 1) ? pb : pa;
        const double* po = (it & 1) ? pa : pb;
        const bool first = (it == 0);
        const double beta = first ? 0.0 : ls.beta;
        // phase A: p_it = r + beta p_{it-1} (formed at the neighbours too), (p, A p)
        double acc = 0.0;
        if (has0) cellA(c0, ar, ap, first, beta, pn, acc);
        for (long long e = e0 + stride; e < ncell; e += stride) {
            const long long c = cell(e);
            long long q[7];
            pts(c, q);
            double rv[7], pv[7];
#pragma unroll
            for (int t = 0; t < 7; ++t) {
                rv[t] = load_sc1(&r[q[t]]);
                pv[t] = first ? 0.0 : load_sc1(&po[q[t]]);
            }
            cellA(c, rv, pv, first, beta, pn, acc);
        }
        gsum_begin(0, acc);
        if (bad) break;
        loadB(pn);
        const double tA = gsum_end(0);
        if (threadIdx.x == 0) fin_A(&ls, tA, it);
        __syncthreads();
        if (ls.done) break;
        // phase B: x += alpha p, r -= alpha A p (A p recomputed), (r, r)
        const double al = ls.alpha[it % CG_XFOLD];
        const double ma = -al;
        acc = 0.0;
        if (has0) cellB(c0, bp, brr, bx, al, ma, acc);
        for (long long e = e0 + stride; e < ncell; e += stride) {
            const long long c = cell(e);
            long long q[7];
            pts(c, q);
            double pv[7];
#pragma unroll
            for (int t = 0; t < 7; ++t) pv[t] = load_sc1(&pn[q[t]]);
            cellB(c, pv, load_sc1(&r[c]), x[c], al, ma, acc);
        }
        gsum_begin(1, acc);
        if (bad) break;
        loadA(pn, false);  // iteration it + 1: p_old = p_it
        const double tB = gsum_end(1);
        if (threadIdx.x == 0) fin_B(&ls, tB, it);
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (bad) {
            ls.done = 1;
            ls.status = ST_COMM_TIMEOUT;
        }
        ls.xdone = ls.nalpha;  // x holds every alpha_j p_j: nothing for k_cg_finalize
        *st = ls;
    }
}

// Apply the x += alpha_j p_j the sweeps have not folded yet (j in [xdone,
// nalpha), at most CG_XFOLD of them: a stop after iteration it = 4m + 3
// leaves alpha_{4m} .. alpha_{4m+3}, whose p_j still sit in the four ring
// slots), in order, partial sums in a register (bitwise the reference's
// sequential updates).
static __global__ __launch_bounds__(NT) void k_cg_finalize(Geo g, PRing pr,
                                                    double* __restrict__ x, const CgState* st) {
    const int j0 = st->xdone, j1 = st->nalpha;  // at most CG_XFOLD pending
    if (j0 >= j1) return;
    const int ntiles = g.tiles_x * g.tiles_y * g.tiles_z;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        TileCoord c = tile_coord(g, t);
        if (!c.active) continue;
        long long idx = cidx(g, c.i, c.j, c.kb);
        for (int k = c.kb; k < c.ke; ++k, idx += g.ps) {
            double v = x[idx];
            for (int jj = j0; jj < j1; ++jj)
                v += st->alpha[jj % CG_XFOLD] * pr.p[jj % CG_XFOLD][idx];
            x[idx] = v;
        }
    }
}

// ===========================================================================
// Chronopoulos-Gear CG (opt-in, hip_proj_config_t.cg_variant = 1): the two
// dot products of an iteration come out of ONE reduction, so a Z-slab run
// needs one all-reduce per iteration instead of two. With
// w = A r and s = A p kept as vectors (Chronopoulos & Gear 1989):
//   p_i = r_i + beta_i p_{i-1},  s_i = w_i + beta_i s_{i-1}      (k_cc1)
//   x_{i+1} = x_i + alpha_i p_i, r_{i+1} = r_i - alpha_i s_i      (k_cc1)
//   w_{i+1} = A r_{i+1}; gamma = (r, r), delta = (w, r)          (k_cc2)
//   beta_{i+1} = gamma_{i+1} / gamma_i,
//   alpha_{i+1} = gamma_{i+1} / (delta_{i+1} - beta_{i+1} gamma_{i+1} / alpha_i)
// Same operator, boundary semantics (zero walls in r, lagged Neumann x),
// stopping rule and statistics as the textbook loop; the iterates differ by
// rounding, so it is gated against textbook CG (iterations +-2, residual),
// not bitwise. x += alpha p is folded every CG_XFOLD iterations as in k_cgB.
// ===========================================================================
// after the first w = A r_0: alpha_0 = (r,r) / (w,r) (the textbook's first
// (p, Ap) with p_0 = r_0), breakdown as fin_A
__device__ __forceinline__ void fin_cc0(CgState* st, double delta) {
    st->pAp = delta;
    if (fabs(delta) < 1e-30) {
        st->done = 1;
        st->status = ST_STAGNATED;
        st->iterations = 1;
    } else {
        st->alpha[0] = st->rho / delta;
        st->beta = 0.0;
    }
}

// after iteration it's reduction: convergence test as fin_B, then beta and
// the next alpha (its denominator standing in for the textbook's (p, Ap))
__device__ __forceinline__ void fin_cc(CgState* st, double gamma, double delta, int it,
                                       bool fold) {
    if (fold) st->xdone = it + 1;
    st->nalpha = it + 1;
    const double res = sqrt(gamma);
    st->res = res;
    st->iterations = it + 1;
    const bool check = (it % st->check_interval) == 0;
    const bool conv = (res < st->tol) || (res < st->abs_tol);
    if (check && conv) {
        st->done = 1;
        st->status = ST_CONVERGED;
    } else if (fabs(st->rho) < 1e-30) {
        st->done = 1;
        st->status = ST_STAGNATED;
    } else {
        const double beta = gamma / st->rho;
        const double den = delta - beta * gamma / st->alpha[it % CG_XFOLD];
        st->beta = beta;
        st->rho = gamma;
        st->pAp = den;
        if (it + 1 >= st->max_iter) {
            st->done = 1;
            st->status = conv ? ST_CONVERGED : ST_MAX_ITER;
        } else if (fabs(den) < 1e-30) {
            st->done = 1;
            st->status = ST_STAGNATED;
            st->iterations = it + 2;
        } else {
            st->alpha[(it + 1) % CG_XFOLD] = gamma / den;
        }
    }
}

static __global__ void k_finish_cc(CgState* st, const double* tot, int it, int fold, int init) {
    if (threadIdx.x != 0 || st->done) return;
    if (init) fin_cc0(st, tot[1]);
    else fin_cc(st, tot[0], tot[1], it, fold != 0);
}

// Pointwise part of iteration it over the interior cells, 16-B pairs:
// p_it into the ring slot pn, s in place, r in place; FOLD (it % 4 == 3)
// also x += the four pending alpha_j p_j in the reference's order.
template <bool FIRST, bool FOLD>
static __global__ __launch_bounds__(256) void k_cc1(SGeo g, double* __restrict__ r,
                                                    const double* __restrict__ w,
                                                    double* __restrict__ s,
                                                    const double* __restrict__ po,
                                                    double* __restrict__ pn, PPrev pv,
                                                    double* __restrict__ x, const CgState* st,
                                                    int it) {
    if (st->done) return;
    const double a = st->alpha[it % CG_XFOLD];
    const double ma = -a;
    const double beta = FIRST ? 0.0 : st->beta;
    double aq[CG_XFOLD - 1];
#pragma unroll
    for (int q = 0; q < CG_XFOLD - 1; ++q)
        aq[q] = FOLD ? st->alpha[(it + 1 + q) % CG_XFOLD] : 0.0;  // alpha_{it-3+q}
    const unsigned pairs = (unsigned)(g.px / 2);
    const unsigned nyi = (unsigned)(g.ny - 2);
    const unsigned n = pairs * nyi * (unsigned)(g.k1 - g.k0);
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const unsigned row = e / pairs;
        const int i0 = 2 * (int)(e - row * pairs);
        if (i0 >= g.nx) continue;
        const int j = 1 + (int)(row % nyi);
        const int k = g.k0 + (int)(row / nyi);
        const bool in0 = i0 >= 1 && i0 <= g.nx - 2;
        const bool in1 = i0 + 1 <= g.nx - 2;
        const long long idx = (long long)k * g.ps + (long long)j * g.px + i0;
        const double2 rv = ld2(r, idx);
        const double2 wv = ld2(w, idx);
        const double2 pf = FIRST ? rv : fma2p(rv, beta, ld2(po, idx));
        const double2 sf = FIRST ? wv : fma2p(wv, beta, ld2(s, idx));
        const double2 pw = make_double2(in0 ? pf.x : 0.0, in1 ? pf.y : 0.0);
        const double2 sw = make_double2(in0 ? sf.x : 0.0, in1 ? sf.y : 0.0);
        st2(pn, idx, pw);
        st2(s, idx, sw);
        st2(r, idx, make_double2(in0 ? rv.x + ma * sf.x : rv.x, in1 ? rv.y + ma * sf.y : rv.y));
        if (FOLD) {
            const double2 xo = ld2(x, idx);
            const double2 qa = ld2(pv.q[0], idx), qb = ld2(pv.q[1], idx), qc = ld2(pv.q[2], idx);
            double2 xw;
            xw.x = in0 ? (((xo.x + aq[0] * qa.x) + aq[1] * qb.x) + aq[2] * qc.x) + a * pf.x : xo.x;
            xw.y = in1 ? (((xo.y + aq[0] * qa.y) + aq[1] * qb.y) + aq[2] * qc.y) + a * pf.y : xo.y;
            st2(x, idx, xw);
        }
    }
}

// Two-value form of grid_sum_last_n (partials[pofs + b] and partials[nb +
// pofs + b], nb = ptot, or gridDim.x when ptot is 0). With ptot > 0 several
// launches on one stream share the reduction: this launch owns slots [pofs,
// pofs + gridDim.x) of ptot, and the last of all ptot workgroups finishes.
template <int NTH>
__device__ __forceinline__ bool grid_sum2_last(double b0, double b1, double* partials,
                                               unsigned* counter, double* sh, int* flag,
                                               double& t0, double& t1, unsigned pofs = 0,
                                               unsigned ptot = 0) {
    const unsigned nb = ptot ? ptot : gridDim.x;
    if (threadIdx.x == 0) {
        store_sc1(&partials[pofs + blockIdx.x], b0);
        store_sc1(&partials[nb + pofs + blockIdx.x], b1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned t = __hip_atomic_fetch_add((gu32*)counter, 1u, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        *flag = (t == nb - 1) ? 1 : 0;
    }
    __syncthreads();
    if (*flag == 0) return false;
    double s0 = 0.0, s1 = 0.0;
    for (unsigned b = threadIdx.x; b < nb; b += NTH) {
        s0 += load_sc1(&partials[b]);
        s1 += load_sc1(&partials[nb + b]);
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6] = s0;
        sh[NTH / 64 + (threadIdx.x >> 6)] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int q = 0; q < NTH / 64; ++q) {
            a0 += sh[q];
            a1 += sh[NTH / 64 + q];
        }
        t0 = a0;
        t1 = a1;
        __hip_atomic_store((gu32*)counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return true;
}

// The end of the single-reduction iteration's one reduction (the finishing
// workgroup, thread 0): on Z-slabs the all-ranks sum through the device
// mailbox, or left in dsum for an RCCL all-reduce + k_finish_cc; on one
// device fin_cc0 / fin_cc directly.
__device__ __forceinline__ void cc_reduce_finish(CgState* st, double tg, double td, int it,
                                                 bool init, bool dist, Mbox* mb, double* dsum) {
    if (dist && mb) {
        double gg, gd;
        if (mbox_allreduce2(mb, tg, td, &gg, &gd)) {
            if (init) fin_cc0(st, gd);
            else fin_cc(st, gg, gd, it, (it % CG_XFOLD) == CG_XFOLD - 1);
        } else {
            comm_fail(st);
        }
    } else if (dist) {
        dsum[0] = tg;
        dsum[1] = td;
    } else if (init) {
        fin_cc0(st, td);
    } else {
        fin_cc(st, tg, td, it, (it % CG_XFOLD) == CG_XFOLD - 1);
    }
}

// w = A r on the row-pair tiling (k_cgA's stencil with p = r), written to w,
// and the one reduction of iteration it: gamma = (r, r), delta = (w, r).
// g.part_total > 0 (Z-slabs, the fused iteration): the launch covers the two
// edge planes (kmode 1) and shares the reduction with the k_ccf launch of the
// interior planes before it (its partials first).
// INIT: the w = A r_0 before iteration 0 (fin_cc0; gamma_0 comes from setup).
// WST = false (the fused iteration on Z-slabs, ccf.hpp): w stays in registers
template <int TY, bool DIST, bool INIT, bool WST = true>
static __global__ __launch_bounds__(64 * TY) void k_cc2(SGeo g, Lap L,
                                                        const double* __restrict__ r,
                                                        double* __restrict__ w, CgState* st,
                                                        double* partials, unsigned* counter,
                                                        int it, double* dsum, Mbox* mb) {
    __shared__ double2 rows[2][TY + 2][64];
    __shared__ double sh[2 * TY];
    __shared__ int flag;
    if (st->done) return;
    RowPair c = row_pair<TY>(g);
    const bool halo = (c.w == 0) || (c.w == TY - 1);
    const int jh = (c.w == 0) ? max(c.j - 1, 0) : min(c.j + 1, g.ny - 1);
    const int hslot = (c.w == 0) ? 0 : TY + 1;
    const long long hoff = (long long)(jh - min(c.j, g.ny - 1)) * g.px;
    const bool xok = c.i0 < g.nx;
    const bool eok_l = c.lane == 0 && c.i0 >= 1 && xok;
    const bool eok_r = c.lane == 63 && c.i0 + 2 < g.nx;
    const double2 zero = make_double2(0.0, 0.0);
    double accg = 0.0, accd = 0.0;
    long long idx = c.idx;
    double2 pm = xok ? ld2(r, idx - g.sz) : zero;
    double2 pc = xok ? ld2(r, idx) : zero;
    double2 hc = (xok && halo) ? ld2(r, idx + hoff) : zero;
    int buf = 0;
    for (int k = c.kb; k < c.ke; ++k, idx += g.ps) {
        const long long ip = idx + g.sz;
        const double2 pp = xok ? ld2(r, ip) : zero;
        const double2 hn = (xok && halo && k + 1 < c.ke) ? ld2(r, ip + hoff) : zero;
        const double el = eok_l ? r[idx - 1] : 0.0;
        const double er = eok_r ? r[idx + 2] : 0.0;
        rows[buf][c.w + 1][c.lane] = pc;
        if (halo) rows[buf][hslot][c.lane] = hc;
        __syncthreads();
        const double2 ys = rows[buf][c.w][c.lane];
        const double2 yn = rows[buf][c.w + 2][c.lane];
        double left = __shfl_up(pc.y, 1, 64);
        double right = __shfl_down(pc.x, 1, 64);
        if (c.lane == 0) left = el;
        if (c.lane == 63) right = er;
        const double w0 = -lap7(L, pc.x, left, pc.y, ys.x, yn.x, pm.x, pp.x);
        const double w1 = -lap7(L, pc.y, pc.x, right, ys.y, yn.y, pm.y, pp.y);
        if (WST && c.act) st2(w, idx, make_double2(c.in0 ? w0 : 0.0, c.in1 ? w1 : 0.0));
        if (c.in0) {
            accg += pc.x * pc.x;
            accd += w0 * pc.x;
        }
        if (c.in1) {
            accg += pc.y * pc.y;
            accd += w1 * pc.y;
        }
        pm = pc;
        pc = pp;
        hc = hn;
        buf ^= 1;
    }
    accg = wave_sum(accg);
    accd = wave_sum(accd);
    if (c.lane == 0) {
        sh[c.w] = accg;
        sh[TY + c.w] = accd;
    }
    __syncthreads();
    double bg = 0.0, bd = 0.0;
    if (threadIdx.x == 0)
        for (int q = 0; q < TY; ++q) {
            bg += sh[q];
            bd += sh[TY + q];
        }
    double tg, td;
    double* shs = (double*)&rows[0][0][0];
    if (grid_sum2_last<64 * TY>(bg, bd, partials, counter, shs, &flag, tg, td,
                                (unsigned)g.part_ofs, (unsigned)g.part_total) &&
        threadIdx.x == 0)
        cc_reduce_finish(st, tg, td, it, INIT, DIST, mb, dsum);
}


// Max over a full field (stats: max temperature, solver_registry.c:52-62),
// planes [k_first, k_first + gridDim.z).
static __global__ __launch_bounds__(256) void k_field_max(Geo g, const double* __restrict__ f,
                                                   unsigned long long* out, int k_first) {
    __shared__ double sh[4];
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int k = k_first + (int)blockIdx.z;
    double m = -INFINITY;
    if (i < g.nx && j < g.ny) {
        double v = f[cidx(g, i, j, k)];
        if (!isnan(v)) m = v;
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
        atomicMax(out, ord_enc(a));
    }
}

// ---------------------------------------------------------------------------
// Energy equation (energy_solver.c:21-176): explicit Euler on the corrected
// velocity, T_new = T + dt(-(u.grad)T + alpha lap T), boundary cells copied;
// any non-finite T_new sets red[5] (the reference's CFD_ERROR_DIVERGED scan).
// 40 B/cell: read T (stencil), u, v, w; write T_new.
// ---------------------------------------------------------------------------
struct EnergyCoef {
    double inv_2dx, inv_2dy, inv_2dz, inv_dx2, inv_dy2, inv_dz2, alpha, dt;
};

static __global__ __launch_bounds__(256) void k_energy(Geo g, EnergyCoef ec, const double* __restrict__ T,
                                                const double* __restrict__ U,
                                                const double* __restrict__ V,
                                                const double* __restrict__ W,
                                                double* __restrict__ Tn,
                                                unsigned long long* red) {
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int k = blockIdx.z;
    if (i >= g.nx || j >= g.ny) return;
    const long long idx = cidx(g, i, j, k);
    const bool interior = (i >= 1 && i <= g.nx - 2 && j >= 1 && j <= g.ny - 2 &&
                           k >= g.k0 && k < g.k1);
    double tn;
    if (interior) {
        const long long px = g.px, sz = g.sz;
        const double Tc = T[idx];
        double dT_dx = (T[idx + 1] - T[idx - 1]) * ec.inv_2dx;
        double dT_dy = (T[idx + px] - T[idx - px]) * ec.inv_2dy;
        double dT_dz = (T[idx + sz] - T[idx - sz]) * ec.inv_2dz;
        double adv = U[idx] * dT_dx + V[idx] * dT_dy + W[idx] * dT_dz;
        double d2x = (T[idx + 1] - 2.0 * Tc + T[idx - 1]) * ec.inv_dx2;
        double d2y = (T[idx + px] - 2.0 * Tc + T[idx - px]) * ec.inv_dy2;
        double d2z = (T[idx + sz] - 2.0 * Tc + T[idx - sz]) * ec.inv_dz2;
        double diff = ec.alpha * (d2x + d2y + d2z);
        double dT = ec.dt * (-adv + diff + 0.0);
        tn = Tc + dT;
    } else {
        tn = T[idx];
    }
    Tn[idx] = tn;
    if (!isfinite(tn)) atomicOr(&red[5], 1ull);
}

// Thermal boundary conditions (energy_solver.c:204-334), in the reference's
// face order as three gather passes: pass 0 = left/right (x faces, every
// local plane), pass 1 = bottom/top (reads the x-face values pass 0 wrote),
// pass 2 = back/front (whole planes, edge ranks only). Types per face:
// 0 periodic, 1 Neumann, 2 Dirichlet (bc_type_t); -1 = leave the face.
struct ThermalFaces {
    int type[6];   // left, right, bottom, top, back, front
    double val[6];
};

static __global__ __launch_bounds__(256) void k_thermal_bc(Geo g, double* __restrict__ T, ThermalFaces tf,
                                                    int pass) {
    const long long plane = (long long)g.nx * g.ny;
    long long total;
    if (pass == 0) total = 2LL * g.ny * g.nz;
    else if (pass == 1) total = 2LL * g.nx * g.nz;
    else total = 2LL * plane;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        int i, j, k, face;
        if (pass == 0) {
            face = (int)(e % 2);           // 0 left, 1 right
            long long q = e / 2;
            j = (int)(q % g.ny);
            k = (int)(q / g.ny);
            i = face == 0 ? 0 : g.nx - 1;
        } else if (pass == 1) {
            face = 2 + (int)(e % 2);       // 2 bottom, 3 top
            long long q = e / 2;
            i = (int)(q % g.nx);
            k = (int)(q / g.nx);
            j = face == 2 ? 0 : g.ny - 1;
        } else {
            face = 4 + (int)(e / plane);   // 4 back, 5 front
            if ((face == 4 && !g.lo_face) || (face == 5 && !g.hi_face)) continue;
            long long q = e % plane;
            j = (int)(q / g.nx);
            i = (int)(q % g.nx);
            k = face == 4 ? 0 : g.nz - 1;
        }
        const int t = tf.type[face];
        if (t < 0) continue;
        const long long dst = cidx(g, i, j, k);
        if (t == 2) {
            T[dst] = tf.val[face];
            continue;
        }
        int si = i, sj = j, sk = k;
        const bool per = (t == 0);
        switch (face) {
            case 0: si = per ? g.nx - 2 : 1; break;
            case 1: si = per ? 1 : g.nx - 2; break;
            case 2: sj = per ? g.ny - 2 : 1; break;
            case 3: sj = per ? 1 : g.ny - 2; break;
            case 4: sk = per ? g.nz - 2 : 1; break;
            default: sk = per ? 1 : g.nz - 2; break;
        }
        T[dst] = T[cidx(g, si, sj, sk)];
    }
}

// ===========================================================================
// Predictor (solver_projection.c:116-185, with compute_source_terms
// solver_explicit_euler.c:317-333 at iter = 0 as per-row / per-column tables
// and energy_compute_buoyancy energy_solver.c:185-196) and corrector
// (solver_projection.c:230-250 + the boundary restore :277-278, the NaN scan
// :281-289 and the stats of solver_registry.c:31-49), on a row-pair z-march.
//
// Tile = 128 (x) x 4 rows (one per wave) x kc planes, 256 threads. Each lane
// owns an x pair and moves it with 16-B loads/stores; x neighbours come from
// the adjacent lanes (the tile's two outer cells from one per-lane load by
// lanes 0 and 63), z neighbours from registers (each field read once per
// plane from HBM), y neighbours from the rows the neighbouring waves load in
// the same step (L1/L2 hits). No LDS and no barrier: the waves of a CU run
// independently, so memory latency hides behind the other resident waves.
// Divisions by the constant spacings use divz (correctly rounded, bitwise
// the reference's `/`), the reference's operation order is kept, and the
// file is compiled with -ffp-contract=off, so u*, v*, w*, u, v, w are
// bitwise the per-cell kernels'. Boundary cells of the tile's rows (i = 0,
// nx - 1) are copies; the rest of the boundary shell (rows j = 0, ny - 1, the
// z faces) is done by k_shell_copy / k_shell_stats.
// ===========================================================================
#ifndef CFD_PR_SYNC
#define CFD_PR_SYNC 1
#endif
// PR_TY rows (waves) per workgroup (tile_plan.hpp, -DCFD_PR_TY)

struct ZTile {
    int i0, j, kb, ke, lane;
    bool xok, in0, in1;
    long long col;   // j * px + x offset of the pair (clamped in-row when i0 >= nx)
    long long eoff;  // lanes 0 / 63: offset of the tile's outer x neighbour
    bool eok;
};

__device__ __forceinline__ ZTile ztile(const SGeo& g) {
    ZTile z;
    const int nt = g.tiles_x * g.tiles_y * g.tiles_z;
    const int t = xcd_tile(blockIdx.x, nt);
    const int tx = t % g.tiles_x;
    const int rest = t / g.tiles_x;
    const int ty = rest % g.tiles_y;
    const int tz = rest / g.tiles_y;
    z.lane = threadIdx.x & 63;
    z.i0 = tx * 128 + 2 * z.lane;
    z.j = ty * PR_TY + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    z.kb = g.k0 + tz * g.kc;
    z.ke = min(z.kb + g.kc, g.k1);
    z.xok = z.i0 < g.nx;
    z.in0 = z.xok && z.i0 >= 1 && z.i0 <= g.nx - 2;
    z.in1 = z.xok && z.i0 + 1 <= g.nx - 2;
    const int ic = z.xok ? z.i0 : g.nx - 2 - ((g.nx - 2) & 1);  // even, 16-B aligned
    z.col = (long long)z.j * g.px + ic;
    z.eok = (z.lane == 0 && z.i0 >= 1 && z.xok) || (z.lane == 63 && z.i0 + 2 < g.nx);
    z.eoff = (z.lane == 0) ? -1 : 2;
    return z;
}

// x neighbours of a lane's pair: .x = left of cell i0, .y = right of i0 + 1
__device__ __forceinline__ double2 xnbr(const ZTile& z, double2 c, double edge) {
    const double l = __shfl_up(c.y, 1, 64);
    const double r = __shfl_down(c.x, 1, 64);
    return make_double2(z.lane == 0 ? edge : l, z.lane == 63 ? edge : r);
}

struct PredCoef2 {
    double two_dx, two_dy, inv_2dz;  // first derivatives
    double dx_sq, dy_sq, inv_dz2;    // second derivatives
    double r_two_dx, r_two_dy, r_dx_sq, r_dy_sq;  // RN(1 / divisor) for divz
    double dt, nu;
    double beta, T_ref, g0, g1, g2;
};

// solver_projection.c:121-182 for one cell: c = centre (u, v, w), f = the
// field the output belongs to (0, 1, 2) with its 6 neighbours
template <class Dv>
__device__ __forceinline__ double pred_cell(const PredCoef2& pc, Dv dv, double u, double v,
                                            double w, double fc, double xm, double xp, double ym,
                                            double yp, double zm, double zp, double src) {
    const double d_dx = dv(xp - xm, pc.two_dx, pc.r_two_dx);
    const double d_dy = dv(yp - ym, pc.two_dy, pc.r_two_dy);
    const double d_dz = (zp - zm) * pc.inv_2dz;
    const double conv = u * d_dx + v * d_dy + w * d_dz;
    const double d2x = dv(xp - 2.0 * fc + xm, pc.dx_sq, pc.r_dx_sq);
    const double d2y = dv(yp - 2.0 * fc + ym, pc.dy_sq, pc.r_dy_sq);
    const double d2z = (zp - 2.0 * fc + zm) * pc.inv_dz2;
    const double visc = pc.nu * (d2x + d2y + d2z);
    const double a = fc + pc.dt * (-conv + visc + src);
    return fmax(-100.0, fmin(100.0, a));
}

// The loads of plane k + 1 (the z+ centre row, the two y rows, the x-edge
// cells, T) are issued while plane k is computed: two register slots
// alternate over an unrolled pair of planes, so a slot is first read one
// step after its loads were issued.
struct PredBundle {
    double2 pp[3], ym[3], yp[3], tc;
    double e[3];
};

// PF: 0 = each plane's loads issued in its own step, 1 = one plane ahead in
// two alternating register slots (more VGPRs, two waves per SIMD).
template <int PF>
constexpr int pred_min_waves() { return PF ? 2 : 4; }

template <bool BUOY, int PF>
static __global__ __launch_bounds__(64 * PR_TY, pred_min_waves<PF>()) void k_pred2(
    SGeo g, PredCoef2 pc, const double* __restrict__ U, const double* __restrict__ V,
    const double* __restrict__ W, const double* __restrict__ T,
    const double* __restrict__ src_u_row, const double* __restrict__ src_v_col,
    double* __restrict__ us, double* __restrict__ vs, double* __restrict__ ws) {
    const ZTile z = ztile(g);
    if (z.j < 1 || z.j > g.ny - 2) {  // boundary rows: k_shell_copy
        if (CFD_PR_SYNC)
            for (int k = z.kb; k < z.ke; ++k) __syncthreads();
        return;
    }
    const double su = src_u_row[z.j];
    const double sv0 = z.xok ? src_v_col[z.i0] : 0.0;
    const double sv1 = z.in1 ? src_v_col[z.i0 + 1] : 0.0;
    const double* F[3] = {U, V, W};
    double* O[3] = {us, vs, ws};
    const long long idx0 = (long long)z.kb * g.ps + z.col;
    auto issue = [&](PredBundle& b, long long idx) __attribute__((always_inline)) {
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            b.pp[f] = ld2(F[f], idx + g.sz);
            b.ym[f] = ld2(F[f], idx - g.px);
            b.yp[f] = ld2(F[f], idx + g.px);
            b.e[f] = z.eok ? F[f][idx + z.eoff] : 0.0;
        }
        b.tc = BUOY ? ld2(T, idx) : make_double2(0.0, 0.0);
    };
    double2 pm[3], pc3[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        pm[f] = ld2(F[f], idx0 - g.sz);
        pc3[f] = ld2(F[f], idx0);
    }
    // plane k from bundle b; the loads of plane k + 1 go to nb first
    auto step = [&](const PredBundle& b0, PredBundle& nb, int k) __attribute__((always_inline)) {
        if (CFD_PR_SYNC) __syncthreads();  // keep the tile's waves on one plane
        const long long idx = idx0 + (long long)(k - z.kb) * g.ps;
        PredBundle cur;
        if (PF) {
            if (k + 1 < z.ke) issue(nb, idx + g.ps);
        } else {
            issue(cur, idx);
        }
        const PredBundle& b = PF ? b0 : cur;
        const double u0 = pc3[0].x, u1 = pc3[0].y;
        const double v0 = pc3[1].x, v1 = pc3[1].y;
        const double w0 = pc3[2].x, w1 = pc3[2].y;
        // sources: compute_source_terms + energy_compute_buoyancy
        // (solver_explicit_euler.c:317-333, energy_solver.c:185-196)
        double s0[3] = {su, sv0, 0.0}, s1[3] = {su, sv1, 0.0};
        if (BUOY) {
            const double dT0 = b.tc.x - pc.T_ref, dT1 = b.tc.y - pc.T_ref;
            s0[0] += -pc.beta * dT0 * pc.g0;
            s0[1] += -pc.beta * dT0 * pc.g1;
            s0[2] += -pc.beta * dT0 * pc.g2;
            s1[0] += -pc.beta * dT1 * pc.g0;
            s1[1] += -pc.beta * dT1 * pc.g1;
            s1[2] += -pc.beta * dT1 * pc.g2;
        }
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            const double2 lr = xnbr(z, pc3[f], b.e[f]);
            // fast divisions, then one wave-uniform check per field: lanes
            // with a quotient outside divz's range redo the pair with the
            // generic division (bitwise the same where both apply)
            double r0, r1;
            auto compute = [&](auto dv) __attribute__((always_inline)) {
                r0 = pred_cell(pc, dv, u0, v0, w0, pc3[f].x, lr.x, pc3[f].y, b.ym[f].x,
                               b.yp[f].x, pm[f].x, b.pp[f].x, s0[f]);
                r1 = pred_cell(pc, dv, u1, v1, w1, pc3[f].y, pc3[f].x, lr.y, b.ym[f].y,
                               b.yp[f].y, pm[f].y, b.pp[f].y, s1[f]);
            };
            bool ok = true;
            compute(DivFastZ{ok});
            if (__builtin_expect(wave_any_bad(ok), 0)) {
                if (!ok) compute(DivExact{});
            }
            double2 o = pc3[f];  // boundary cells: u* = u
            if (z.in0) o.x = r0;
            if (z.in1) o.y = r1;
            if (z.xok) st2(O[f], idx, o);
        }
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            pm[f] = pc3[f];
            pc3[f] = b.pp[f];
        }
    };
    PredBundle A, B;
    if constexpr (PF != 0) {
        issue(A, idx0);
        int k = z.kb;
        for (; k + 1 < z.ke; k += 2) {
            step(A, B, k);
            step(B, A, k + 1);
        }
        if (k < z.ke) step(A, B, k);
    } else {
        for (int k = z.kb; k < z.ke; ++k) step(A, B, k);
    }
}

// Boundary shell of the predictor: u* = u on every cell the z-march does not
// write (rows j = 0, ny - 1 of every plane, the x edges, the z faces).
static __global__ __launch_bounds__(256) void k_shell_copy(Geo g, const double* __restrict__ U,
                                                           const double* __restrict__ V,
                                                           const double* __restrict__ W,
                                                           double* __restrict__ us,
                                                           double* __restrict__ vs,
                                                           double* __restrict__ ws) {
    const long long total = shell_total(g);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        int i, j, k;
        bool zlo, zhi;
        shell_cell(g, e, i, j, k, zlo, zhi);
        const long long d = cidx(g, i, j, k);
        us[d] = U[d];
        vs[d] = V[d];
        ws[d] = W[d];
    }
}

// Corrector (solver_projection.c:230-250) on the interior rows and planes +
// NaN/Inf scan and max |u|, max |p| of those cells; boundary cells of the
// tile's rows keep u (== u*) and join the scan. The rest of the shell is
// scanned by k_shell_stats. red[0] = max |u|^2 (encoded), [1] = max |p|,
// [2] = non-finite flag.
struct CorrCoef2 {
    double two_dx, two_dy, inv_2dz;
    double r_two_dx, r_two_dy;
    double dt_over_rho;
};

__device__ __forceinline__ void corr_reduce(double mv, double mp, bool bad,
                                            unsigned long long* red) {
    __shared__ double shv[PR_TY], shp[PR_TY];
    __shared__ int shbad;
    if (threadIdx.x == 0) shbad = 0;
    __syncthreads();
    mv = wave_max(mv);
    mp = wave_max(mp);
    if (bad) shbad = 1;
    if ((threadIdx.x & 63) == 0) {
        shv[threadIdx.x >> 6] = mv;
        shp[threadIdx.x >> 6] = mp;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = shv[0], b = shp[0];
        for (int q = 1; q < PR_TY; ++q) {
            a = fmax(a, shv[q]);
            b = fmax(b, shp[q]);
        }
        atomicMax(&red[0], ord_enc(a));
        atomicMax(&red[1], ord_enc(b));
        if (shbad) atomicOr(&red[2], 1ull);
    }
}

__device__ __forceinline__ void cell_stats(double u, double v, double w, double p, double& mv,
                                           double& mp, bool& bad) {
    if (!isfinite(u) || !isfinite(v) || !isfinite(w) || !isfinite(p)) bad = true;
    // solver_registry.c:31-49 takes max sqrt(u^2 + v^2 + w^2); sqrt is
    // correctly rounded, hence monotone, so the maximum of the squared speeds
    // is reduced (red[0]) and the host takes one sqrt of it: bitwise the same
    // value, and no fp64 sqrt sequence per cell
    const double vel2 = (u * u) + (v * v) + (w * w);
    if (vel2 > mv) mv = vel2;
    const double ap = fabs(p);
    if (ap > mp) mp = ap;
}

struct CorrBundle {
    double2 pp, ym, yp, a, b, c;
    double e;
};

// PF as in k_pred2: 1 = the loads of plane k + 1 are issued during plane k
template <int PF>
static __global__ __launch_bounds__(64 * PR_TY, PF ? 3 : 4) void k_corr2(
    SGeo g, CorrCoef2 cc, const double* __restrict__ us, const double* __restrict__ vs,
    const double* __restrict__ ws, const double* __restrict__ P, double* __restrict__ U,
    double* __restrict__ V, double* __restrict__ W, unsigned long long* red) {
    const ZTile z = ztile(g);
    double mv = 0.0, mp = 0.0;
    bool bad = false;
    if (z.j >= 1 && z.j <= g.ny - 2) {  // wave-uniform
        const long long idx0 = (long long)z.kb * g.ps + z.col;
        double2 pm = ld2(P, idx0 - g.sz), pc = ld2(P, idx0);
        auto issue = [&](CorrBundle& q, long long idx) __attribute__((always_inline)) {
            q.pp = ld2(P, idx + g.sz);
            q.ym = ld2(P, idx - g.px);
            q.yp = ld2(P, idx + g.px);
            q.e = z.eok ? P[idx + z.eoff] : 0.0;
            q.a = ld2(us, idx);
            q.b = ld2(vs, idx);
            q.c = ld2(ws, idx);
        };
        auto step = [&](const CorrBundle& q0, CorrBundle& nq, int k) __attribute__((always_inline)) {
            if (CFD_PR_SYNC) __syncthreads();  // keep the tile's waves on one plane
            const long long idx = idx0 + (long long)(k - z.kb) * g.ps;
            CorrBundle cur;
            if (PF) {
                if (k + 1 < z.ke) issue(nq, idx + g.ps);
            } else {
                issue(cur, idx);
            }
            const CorrBundle& q = PF ? q0 : cur;
            const double2 lr = xnbr(z, pc, q.e);
            const double left = lr.x, right = lr.y;
            double2 nu = q.a, nv = q.b, nw = q.c;  // boundary cells: u = u* (== u)
            // fast divisions, one wave-uniform check, generic division for
            // lanes whose quotients left divz's range (as in k_pred2)
            double dx0, dy0, dx1, dy1;
            auto compute = [&](auto dv) __attribute__((always_inline)) {
                dx0 = dv(pc.y - left, cc.two_dx, cc.r_two_dx);
                dy0 = dv(q.yp.x - q.ym.x, cc.two_dy, cc.r_two_dy);
                dx1 = dv(right - pc.x, cc.two_dx, cc.r_two_dx);
                dy1 = dv(q.yp.y - q.ym.y, cc.two_dy, cc.r_two_dy);
            };
            bool ok = true;
            compute(DivFastZ{ok});
            if (__builtin_expect(wave_any_bad(ok), 0)) {
                if (!ok) compute(DivExact{});
            }
            {
                const double dp_dz = (q.pp.x - pm.x) * cc.inv_2dz;
                const double x0 = fmax(-100.0, fmin(100.0, q.a.x - cc.dt_over_rho * dx0));
                const double y0 = fmax(-100.0, fmin(100.0, q.b.x - cc.dt_over_rho * dy0));
                const double w0 = fmax(-100.0, fmin(100.0, q.c.x - cc.dt_over_rho * dp_dz));
                if (z.in0) {
                    nu.x = x0;
                    nv.x = y0;
                    nw.x = w0;
                }
            }
            {
                const double dp_dz = (q.pp.y - pm.y) * cc.inv_2dz;
                const double x1 = fmax(-100.0, fmin(100.0, q.a.y - cc.dt_over_rho * dx1));
                const double y1 = fmax(-100.0, fmin(100.0, q.b.y - cc.dt_over_rho * dy1));
                const double w1 = fmax(-100.0, fmin(100.0, q.c.y - cc.dt_over_rho * dp_dz));
                if (z.in1) {
                    nu.y = x1;
                    nv.y = y1;
                    nw.y = w1;
                }
            }
            if (z.xok) {
                st2(U, idx, nu);
                st2(V, idx, nv);
                st2(W, idx, nw);
                cell_stats(nu.x, nv.x, nw.x, pc.x, mv, mp, bad);
                if (z.i0 + 1 < g.nx) cell_stats(nu.y, nv.y, nw.y, pc.y, mv, mp, bad);
            }
            pm = pc;
            pc = q.pp;
        };
        CorrBundle A, B;
        if constexpr (PF != 0) {
            issue(A, idx0);
            int k = z.kb;
            for (; k + 1 < z.ke; k += 2) {
                step(A, B, k);
                step(B, A, k + 1);
            }
            if (k < z.ke) step(A, B, k);
        } else {
            for (int k = z.kb; k < z.ke; ++k) step(A, B, k);
        }
    } else if (CFD_PR_SYNC) {
        for (int k = z.kb; k < z.ke; ++k) __syncthreads();
    }
    corr_reduce(mv, mp, bad, red);
}

// ---------------------------------------------------------------------------
// r03: the predictor and corrector on the CG sweeps' 128 x 16 tiles with the
// y neighbours from LDS (k_pred3, k_corr3). Each wave owns one row of the
// tile, the two edge waves also load the row beyond it (the y halo), and
// every wave publishes its centre row once per plane: a stencil field's rows
// are read from HBM 18 times per 16 rows written, where the 4-row tiles of
// k_pred2 / k_corr2 need L2 hits for 6 reads per 4 rows (k_pred2 fetched
// 45.8 B/cell for 24 B of reads, profiles/r02e_rocprof_summary.txt). One
// barrier per plane, rows double-buffered by plane parity. Operands and
// operation order are k_pred2's / k_corr2's, so the results are bitwise
// theirs. FL: SW_NT_STORE = non-temporal stores of the outputs, SW_NT_LOAD =
// non-temporal loads of the pointwise inputs (the corrector's u*, v*, w*).
// ---------------------------------------------------------------------------
// PC_TY = 16 rows per workgroup (tile_plan.hpp)

template <bool BUOY, int FL>
static __global__ __launch_bounds__(64 * PC_TY, 1) void k_pred3(
    SGeo g, PredCoef2 pc, const double* __restrict__ U, const double* __restrict__ V,
    const double* __restrict__ W, const double* __restrict__ T,
    const double* __restrict__ src_u_row, const double* __restrict__ src_v_col,
    double* __restrict__ us, double* __restrict__ vs, double* __restrict__ ws) {
    constexpr int TY = PC_TY;
    __shared__ double2 rows[2][3][TY + 2][64];
    const RowPair c = row_pair<TY>(g);
    const bool halo = (c.w == 0) || (c.w == TY - 1);
    const int jc = min(c.j, g.ny - 1);
    const int jh = (c.w == 0) ? max(c.j - 1, 0) : min(c.j + 1, g.ny - 1);
    const int hslot = (c.w == 0) ? 0 : TY + 1;
    const long long hoff = (long long)(jh - jc) * g.px;
    const bool xok = c.i0 < g.nx;
    const bool eok = (c.lane == 0 && c.i0 >= 1 && xok) || (c.lane == 63 && c.i0 + 2 < g.nx);
    const long long eoff = (c.lane == 0) ? -1 : 2;
    const double su = src_u_row[jc];
    const double sv0 = xok ? src_v_col[c.i0] : 0.0;
    const double sv1 = c.in1 ? src_v_col[c.i0 + 1] : 0.0;
    const double* F[3] = {U, V, W};
    double* O[3] = {us, vs, ws};
    const double2 zero = make_double2(0.0, 0.0);
    long long idx = c.idx;
    // rows of plane k are published into rows[k & 1] at the end of step
    // k - 1 (that buffer was last read in step k - 2, before the barrier of
    // step k - 1), so no row value is held in registers across a barrier
    double2 pm[3], pcv[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        pm[f] = ld2(F[f], idx - g.sz);
        pcv[f] = ld2(F[f], idx);
        rows[0][f][c.w + 1][c.lane] = pcv[f];
        if (halo) rows[0][f][hslot][c.lane] = ld2(F[f], idx + hoff);
    }
    int buf = 0;
    for (int k = c.kb; k < c.ke; ++k, idx += g.ps) {
        // this plane's loads: the z+ centre row, the halo row of plane k + 1,
        // the x-edge cells, T
        double2 pp[3], hn[3];
        double e[3];
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            pp[f] = ld2(F[f], idx + g.sz);
            hn[f] = halo ? ld2(F[f], idx + g.sz + hoff) : zero;
            e[f] = eok ? F[f][idx + eoff] : 0.0;
        }
        const double2 tc = BUOY ? ld2(T, idx) : zero;
        __syncthreads();
        const double u0 = pcv[0].x, u1 = pcv[0].y;
        const double v0 = pcv[1].x, v1 = pcv[1].y;
        const double w0 = pcv[2].x, w1 = pcv[2].y;
        double s0[3] = {su, sv0, 0.0}, s1[3] = {su, sv1, 0.0};
        if (BUOY) {
            const double dT0 = tc.x - pc.T_ref, dT1 = tc.y - pc.T_ref;
            s0[0] += -pc.beta * dT0 * pc.g0;
            s0[1] += -pc.beta * dT0 * pc.g1;
            s0[2] += -pc.beta * dT0 * pc.g2;
            s1[0] += -pc.beta * dT1 * pc.g0;
            s1[1] += -pc.beta * dT1 * pc.g1;
            s1[2] += -pc.beta * dT1 * pc.g2;
        }
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            const double2 ys = rows[buf][f][c.w][c.lane];
            const double2 yn = rows[buf][f][c.w + 2][c.lane];
            const double l = __shfl_up(pcv[f].y, 1, 64);
            const double rr = __shfl_down(pcv[f].x, 1, 64);
            const double left = c.lane == 0 ? e[f] : l;
            const double right = c.lane == 63 ? e[f] : rr;
            double r0, r1;
            auto compute = [&](auto dv) __attribute__((always_inline)) {
                r0 = pred_cell(pc, dv, u0, v0, w0, pcv[f].x, left, pcv[f].y, ys.x, yn.x, pm[f].x,
                               pp[f].x, s0[f]);
                r1 = pred_cell(pc, dv, u1, v1, w1, pcv[f].y, pcv[f].x, right, ys.y, yn.y, pm[f].y,
                               pp[f].y, s1[f]);
            };
            bool ok = true;
            compute(DivFastZ{ok});
            if (__builtin_expect(wave_any_bad(ok), 0)) {
                if (!ok) compute(DivExact{});
            }
            double2 o = pcv[f];  // boundary cells: u* = u
            if (c.in0) o.x = r0;
            if (c.in1) o.y = r1;
            if (c.act) st2v<FL>(O[f], idx, o);
        }
        buf ^= 1;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            pm[f] = pcv[f];
            pcv[f] = pp[f];
            rows[buf][f][c.w + 1][c.lane] = pp[f];
            if (halo) rows[buf][f][hslot][c.lane] = hn[f];
        }
    }
}

template <int NW>
__device__ __forceinline__ void corr_reduce_n(double mv, double mp, bool bad,
                                              unsigned long long* red) {
    __shared__ double shv[NW], shp[NW];
    __shared__ int shbad;
    if (threadIdx.x == 0) shbad = 0;
    __syncthreads();
    mv = wave_max(mv);
    mp = wave_max(mp);
    if (bad) shbad = 1;
    if ((threadIdx.x & 63) == 0) {
        shv[threadIdx.x >> 6] = mv;
        shp[threadIdx.x >> 6] = mp;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = shv[0], b = shp[0];
        for (int q = 1; q < NW; ++q) {
            a = fmax(a, shv[q]);
            b = fmax(b, shp[q]);
        }
        atomicMax(&red[0], ord_enc(a));
        atomicMax(&red[1], ord_enc(b));
        if (shbad) atomicOr(&red[2], 1ull);
    }
}

template <int FL>
static __global__ __launch_bounds__(64 * PC_TY, 1) void k_corr3(
    SGeo g, CorrCoef2 cc, const double* __restrict__ us, const double* __restrict__ vs,
    const double* __restrict__ ws, const double* __restrict__ P, double* __restrict__ U,
    double* __restrict__ V, double* __restrict__ W, unsigned long long* red) {
    constexpr int TY = PC_TY;
    __shared__ double2 rows[2][TY + 2][64];
    const RowPair c = row_pair<TY>(g);
    const bool halo = (c.w == 0) || (c.w == TY - 1);
    const int jc = min(c.j, g.ny - 1);
    const int jh = (c.w == 0) ? max(c.j - 1, 0) : min(c.j + 1, g.ny - 1);
    const int hslot = (c.w == 0) ? 0 : TY + 1;
    const long long hoff = (long long)(jh - jc) * g.px;
    const bool xok = c.i0 < g.nx;
    const bool eok = (c.lane == 0 && c.i0 >= 1 && xok) || (c.lane == 63 && c.i0 + 2 < g.nx);
    const long long eoff = (c.lane == 0) ? -1 : 2;
    const double2 zero = make_double2(0.0, 0.0);
    double mv = 0.0, mp = 0.0;
    bool bad = false;
    long long idx = c.idx;
    double2 pm = ld2(P, idx - g.sz), pcv = ld2(P, idx);
    rows[0][c.w + 1][c.lane] = pcv;  // publishing as in k_pred3
    if (halo) rows[0][hslot][c.lane] = ld2(P, idx + hoff);
    int buf = 0;
    for (int k = c.kb; k < c.ke; ++k, idx += g.ps) {
        const double2 pp = ld2(P, idx + g.sz);
        const double2 hn = halo ? ld2(P, idx + g.sz + hoff) : zero;
        const double e = eok ? P[idx + eoff] : 0.0;
        const double2 qa = ld2v<FL>(us, idx), qb = ld2v<FL>(vs, idx), qc = ld2v<FL>(ws, idx);
        __syncthreads();
        const double2 ys = rows[buf][c.w][c.lane];
        const double2 yn = rows[buf][c.w + 2][c.lane];
        const double l = __shfl_up(pcv.y, 1, 64);
        const double rr = __shfl_down(pcv.x, 1, 64);
        const double left = c.lane == 0 ? e : l;
        const double right = c.lane == 63 ? e : rr;
        double2 nu = qa, nv = qb, nw = qc;  // boundary cells: u = u* (== u)
        double dx0, dy0, dx1, dy1;
        auto compute = [&](auto dv) __attribute__((always_inline)) {
            dx0 = dv(pcv.y - left, cc.two_dx, cc.r_two_dx);
            dy0 = dv(yn.x - ys.x, cc.two_dy, cc.r_two_dy);
            dx1 = dv(right - pcv.x, cc.two_dx, cc.r_two_dx);
            dy1 = dv(yn.y - ys.y, cc.two_dy, cc.r_two_dy);
        };
        bool ok = true;
        compute(DivFastZ{ok});
        if (__builtin_expect(wave_any_bad(ok), 0)) {
            if (!ok) compute(DivExact{});
        }
        {
            const double dp_dz = (pp.x - pm.x) * cc.inv_2dz;
            const double x0 = fmax(-100.0, fmin(100.0, qa.x - cc.dt_over_rho * dx0));
            const double y0 = fmax(-100.0, fmin(100.0, qb.x - cc.dt_over_rho * dy0));
            const double w0 = fmax(-100.0, fmin(100.0, qc.x - cc.dt_over_rho * dp_dz));
            if (c.in0) {
                nu.x = x0;
                nv.x = y0;
                nw.x = w0;
            }
        }
        {
            const double dp_dz = (pp.y - pm.y) * cc.inv_2dz;
            const double x1 = fmax(-100.0, fmin(100.0, qa.y - cc.dt_over_rho * dx1));
            const double y1 = fmax(-100.0, fmin(100.0, qb.y - cc.dt_over_rho * dy1));
            const double w1 = fmax(-100.0, fmin(100.0, qc.y - cc.dt_over_rho * dp_dz));
            if (c.in1) {
                nu.y = x1;
                nv.y = y1;
                nw.y = w1;
            }
        }
        if (c.act) {
            st2v<FL>(U, idx, nu);
            st2v<FL>(V, idx, nv);
            st2v<FL>(W, idx, nw);
            cell_stats(nu.x, nv.x, nw.x, pcv.x, mv, mp, bad);
            if (c.i0 + 1 < g.nx) cell_stats(nu.y, nv.y, nw.y, pcv.y, mv, mp, bad);
        }
        pm = pcv;
        pcv = pp;
        buf ^= 1;
        rows[buf][c.w + 1][c.lane] = pp;
        if (halo) rows[buf][hslot][c.lane] = hn;
    }
    corr_reduce_n<TY>(mv, mp, bad, red);
}

// Stats over the boundary shell cells the corrector's z-march does not visit
// (rows j = 0, ny - 1 of the owned planes, the global z faces): u, v, w are
// the caller's boundary values there. Planes [ks, ke) as in the corrector.
static __global__ __launch_bounds__(256) void k_shell_stats(Geo g, const double* __restrict__ U,
                                                            const double* __restrict__ V,
                                                            const double* __restrict__ W,
                                                            const double* __restrict__ P,
                                                            unsigned long long* red) {
    __shared__ double shv[4], shp[4];
    __shared__ int shbad;
    if (threadIdx.x == 0) shbad = 0;
    __syncthreads();
    const int ks = (g.nz > 1 && !g.lo_face) ? 1 : 0;
    const int ke = (g.nz > 1 && !g.hi_face) ? g.nz - 1 : g.nz;
    const long long total = shell_total(g);
    double mv = 0.0, mp = 0.0;
    bool bad = false;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        int i, j, k;
        bool zlo, zhi;
        shell_cell(g, e, i, j, k, zlo, zhi);
        // the z-march covers i = 0 / nx - 1 of its rows on interior planes
        const bool marched = (j >= 1 && j <= g.ny - 2 && k >= g.k0 && k < g.k1);
        if (k < ks || k >= ke || marched) continue;
        const long long d = cidx(g, i, j, k);
        cell_stats(U[d], V[d], W[d], P[d], mv, mp, bad);
    }
    mv = wave_max(mv);
    mp = wave_max(mp);
    if (bad) shbad = 1;
    if ((threadIdx.x & 63) == 0) {
        shv[threadIdx.x >> 6] = mv;
        shp[threadIdx.x >> 6] = mp;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(&red[0], ord_enc(fmax(fmax(shv[0], shv[1]), fmax(shv[2], shv[3]))));
        atomicMax(&red[1], ord_enc(fmax(fmax(shp[0], shp[1]), fmax(shp[2], shp[3]))));
        if (shbad) atomicOr(&red[2], 1ull);
    }
}

}  // namespace cfdhip
