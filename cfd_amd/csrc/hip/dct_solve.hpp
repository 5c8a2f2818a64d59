// dct_solve.hpp -- the direct cosine-transform pressure solver (HIP_POISSON_DCT).
//
// Red-Black SOR and Jacobi apply the Neumann boundary condition after every
// sweep, so at their fixed point every shell cell equals its interior
// neighbour and the interior operator is the cell-centred Neumann Laplacian:
// the 7-point stencil whose end cells lose the missing neighbour's term. On
// the uniform box the orthonormal type-II cosine transform along each axis
// diagonalises it,
//   Q_n[a][b] = w_a cos(pi a (2 b + 1) / (2 n)),  lambda_n[a] = 4 sin^2(pi a / (2 n)) / h^2,
//   x = Qx^T Qy^T Qz^T [ (Qz Qy Qx (-rhs)) / (lx[i] + ly[j] + lz[k]) ]   (interior),
// followed by the Neumann shell (the sign is the relaxation solvers': they
// solve lap(x) = rhs, and the operator above is -lap). The transforms are the
// sine solver's passes (dst_solve.hpp: k_dst_x, k_dst_strided) with cosine
// tables. A pass computes out[a] = sum_b T[b][a] in[b]; the sine table is
// symmetric, Q is not: the forward pass is given Q^T, the inverse pass Q.
//
// The zero mode. lambda(0, 0, 0) = 0: the operator is singular, its null
// space the constants. The coefficient of that mode is set to exactly 0.0 and
// never divided, so the interior mean of the result is zero to rounding. A
// right-hand side whose interior mean m is not zero has no solution; the
// result is then the least-squares one, whose residual is m in every cell
// (L-inf residual |m|), which is also where the iterations' residual ends up:
// the status is the one they would reach. The pressure constant differs from
// RB-SOR's or Jacobi's in every case (they keep what their start and their
// splitting leave); only grad p enters the projection step.
//
// The initial and final residuals are the relaxation solvers' L-inf residual
// (k_residual_linf through relax_residual_linf), the status their rule.
// Host code only; private to projection_hip.hip (through poisson_solve.hpp).
#pragma once

#include "dst_solve.hpp"

// The cached tables of one axis length (device copies)
static cfd_status_t dct_table(hip_proj_ctx* c, int n, const DctTable** out) {
    for (const DctTable& t : c->dct_tabs)
        if (t.n == n) {
            *out = &t;
            return CFD_SUCCESS;
        }
    const size_t np = dst_table_pitch((size_t)n);
    std::vector<double> hq(np * np), hqt(np * np), he((size_t)n);
    dct_fill_cos_tables((size_t)n, hq.data(), hqt.data());
    dct_fill_eigenvalues((size_t)n, he.data());
    // owned by the context from here (free_ctx); n is set once it is complete
    c->dct_tabs.push_back(DctTable{-1, (int)np, nullptr, nullptr, nullptr});
    DctTable& t = c->dct_tabs.back();
    HIP_TRY(hipMalloc((void**)&t.Q, hq.size() * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&t.Qt, hqt.size() * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&t.e, he.size() * sizeof(double)));
    // pageable sources: synchronous copies (ordered before later stream work)
    HIP_TRY(hipMemcpy(t.Q, hq.data(), hq.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.Qt, hqt.data(), hqt.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.e, he.data(), he.size() * sizeof(double), hipMemcpyHostToDevice));
    t.n = n;
    *out = &t;
    return CFD_SUCCESS;
}

// the tables of the context's axes (tz == nullptr in 2-D); the vector may
// grow while they are looked up, so the pointers are taken afterwards
struct DctTabs {
    const DctTable *tx, *ty, *tz;
};

static cfd_status_t dct_tables_of(hip_proj_ctx* c, DctTabs* T) {
    const DctTable* t = nullptr;
    const int n[3] = {(int)c->nx - 2, (int)c->ny - 2, c->nz > 1 ? (int)c->nz - 2 : 0};
    for (int a = 0; a < 3; ++a)
        if (n[a] > 0) ST_TRY(dct_table(c, n[a], &t));
    ST_TRY(dct_table(c, n[0], &T->tx));
    ST_TRY(dct_table(c, n[1], &T->ty));
    T->tz = nullptr;
    if (n[2] > 0) ST_TRY(dct_table(c, n[2], &T->tz));
    return CFD_SUCCESS;
}

// One orthonormal DCT-II pass (inverse: its transpose, DCT-III) of the
// interior along `axis` (0 x, 1 y, 2 z): in -> out (distinct fields). neg
// (axis 0): the input is -in. sc (axes 1, 2): the eigenvalue division on the
// store.
static void dct_pass(hip_proj_ctx* c, const DctTabs& T, int axis, bool inverse, const double* in,
                     double* out, bool neg = false, const DstScale* sc = nullptr) {
    const DctTable* t = (axis == 0) ? T.tx : (axis == 1) ? T.ty : T.tz;
    const double* tab = inverse ? t->Q : t->Qt;
    if (axis == 0) {
        const DstRows g = dst_rows_geo(c, t->np);
        const dim3 grid((unsigned)(g.tiles_a * g.tiles_j * g.nk));
        if (neg)
            klaunch(c, k_dst_x<false, true>, grid, dim3(256), g, tab, in, nullptr, out, Lap{}, 0);
        else
            klaunch(c, k_dst_x<false>, grid, dim3(256), g, tab, in, nullptr, out, Lap{}, 0);
        return;
    }
    const DstAxis g = dst_axis_geo(c, axis, t->n, t->np);
    const dim3 grid((unsigned)(g.tiles_c * g.tiles_a * g.nb));
    if (sc) klaunch(c, k_dst_strided<true, true>, grid, dim3(256), g, tab, in, out, *sc);
    else klaunch(c, k_dst_strided<false>, grid, dim3(256), g, tab, in, out, DstScale{});
}

// ---------------------------------------------------------------------------
// The solve: x in c->pn, rhs in c->rhs. As in dst_solve the transforms
// ping-pong between c->xt and the interior of c->pn, whose shell the end BC
// writes; rhs stays intact for the final residual. max_iterations,
// check_interval and omega play no part.
// ---------------------------------------------------------------------------
static cfd_status_t dct_solve(hip_proj_ctx* c, double dx, double dy, double dz, double rel_tol,
                              double abs_tol) {
    const bool is3d = c->nz > 1;
    const Lap L = make_lap(dx, dy, is3d ? dz : 0.0);
    const DirVals dv{};
    double* x = c->pn;
    ST_TRY(ensure_aux(c, true, true));
    DctTabs T;
    ST_TRY(dct_tables_of(c, &T));
    for (hipEvent_t& e : c->dst_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(c->dst_ev[0], c->stream));
    // linear_solver.c:397-485: the residual of x as it stands, no start BC
    double res0 = 0.0;
    ST_TRY(relax_residual_linf(c, x, dx, dy, is3d ? dz : 0.0, &res0));
    double tol = rel_tol * res0;
    if (tol < abs_tol) tol = abs_tol;
    c->pstats.initial_residual = res0;
    if (res0 < abs_tol) {
        flush_timing(c);
        c->pstats.status = POISSON_CONVERGED;
        c->pstats.iterations = 0;
        c->pstats.final_residual = res0;
        c->pstats.elapsed_time_ms = 0.0;
        return CFD_SUCCESS;
    }
    DstScale sc{};
    sc.norm = 1.0;  // Q is orthonormal
    sc.ec = T.tx->e;
    sc.hc = L.dx2_inv;
    dct_pass(c, T, 0, false, c->rhs, c->xt, true);
    if (is3d) {
        sc.ea = T.tz->e, sc.ha = L.inv_dz2;
        sc.eb = T.ty->e, sc.hb = L.dy2_inv;
        dct_pass(c, T, 1, false, c->xt, x);
        dct_pass(c, T, 2, false, x, c->xt, false, &sc);
        dct_pass(c, T, 2, true, c->xt, x);
        dct_pass(c, T, 1, true, x, c->xt);
    } else {
        sc.ea = T.ty->e, sc.ha = L.dy2_inv;
        sc.eb = nullptr, sc.hb = 0.0;
        dct_pass(c, T, 1, false, c->xt, x, false, &sc);
        dct_pass(c, T, 1, true, x, c->xt);
    }
    dct_pass(c, T, 0, true, c->xt, x);
    launch_bc(c, x, 0, dv);  // the iterations' apply_bc
    double res = 0.0;
    ST_TRY(relax_residual_linf(c, x, dx, dy, is3d ? dz : 0.0, &res));
    HIP_TRY(hipEventRecord(c->dst_ev[1], c->stream));
    HIP_TRY(hipEventSynchronize(c->dst_ev[1]));
    flush_timing(c);
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->dst_ev[0], c->dst_ev[1]));
    const bool conv = (res < tol) || (res < abs_tol);
    c->pstats.status = conv ? POISSON_CONVERGED : POISSON_MAX_ITER;
    c->pstats.iterations = 1;
    c->pstats.final_residual = res;
    c->pstats.elapsed_time_ms = (double)ms;
    return conv ? CFD_SUCCESS : CFD_ERROR_MAX_ITER;
}
