// rk_kernels.hpp -- the explicit integrators' kernels: the RK4 / RK2 stages
// (k_rk_stage, k_rk_stage2), k_euler_step and k_vel_stats. Included by
// rk4_hip.hip only.
#pragma once

#include "device_util.hpp"

namespace cfdhip {

// ---------------------------------------------------------------------------
// RK4 (solver_rk4.c:69-259) with the shared momentum RHS
// (ns_momentum_rhs_scalar.h:49-190). One fused kernel per stage s:
//   k      = RHS(cur)                      (interior; 0 on boundary cells)
//   acc    = k | acc + 2k | acc + 2k       (s = 0, 1, 2: the reference's
//                                           k1 + 2 k2 + 2 k3 + k4, left to right)
//   out    = clamp(Q0 + fac_s k)           (s < 3; fac = dt/2, dt/2, dt)
//   out    = clamp(Q0 + dt/6 (acc + k))    (s = 3, written in place over Q0)
// so the stage derivatives never touch HBM. The stencil uses the
// reference's periodic neighbour indices (i = 1 reads nx-2, not the ghost).
// ---------------------------------------------------------------------------
struct RkCoef {
    double inv_2dz, inv_dz2;
    double mu, beta, T_ref, g0, g1, g2;
    double fac;   // dt/2, dt/2, dt, dt/6
};

struct Fld4 {
    double* f[4];  // u, v, w, p
};

__device__ __forceinline__ double clampl(double x, double lim) { return fmax(-lim, fmin(lim, x)); }

// One cell's RHS (ns_momentum_rhs_scalar.h:49-190 operation order): the 7
// values of u, v, w, p around the cell (periodic neighbour indices already
// resolved), rho, dx[i], dy[j], the source-table entries and T; kr = 0 where
// the reference skips the cell (rho or a spacing below 1e-10).
struct RkNbr {
    double c[4], l[4], r[4], d[4], u[4], m[4], p[4];  // centre, x-, x+, y-, y+, z-, z+
};

template <bool BUOY>
__device__ __forceinline__ void rk_rhs(const RkCoef& rc, const RkNbr& n, double r, double dxi,
                                       double dyj, double su, double sv, double Tc,
                                       double (&kr)[4]) {
    if (!(r <= 1e-10) && !(fabs(dxi) < 1e-10) && !(fabs(dyj) < 1e-10)) {
        const double tdx = 2.0 * dxi, tdy = 2.0 * dyj;
        const double dxx = dxi * dxi, dyy = dyj * dyj;
        const double uc = n.c[0], vc = n.c[1], wc = n.c[2];
        double du_dx = (n.r[0] - n.l[0]) / tdx, du_dy = (n.u[0] - n.d[0]) / tdy;
        double du_dz = (n.p[0] - n.m[0]) * rc.inv_2dz;
        double dv_dx = (n.r[1] - n.l[1]) / tdx, dv_dy = (n.u[1] - n.d[1]) / tdy;
        double dv_dz = (n.p[1] - n.m[1]) * rc.inv_2dz;
        double dw_dx = (n.r[2] - n.l[2]) / tdx, dw_dy = (n.u[2] - n.d[2]) / tdy;
        double dw_dz = (n.p[2] - n.m[2]) * rc.inv_2dz;
        double dp_dx = (n.r[3] - n.l[3]) / tdx, dp_dy = (n.u[3] - n.d[3]) / tdy;
        double dp_dz = (n.p[3] - n.m[3]) * rc.inv_2dz;
        double d2u_dx2 = (n.r[0] - 2.0 * uc + n.l[0]) / dxx;
        double d2u_dy2 = (n.u[0] - 2.0 * uc + n.d[0]) / dyy;
        double d2u_dz2 = (n.p[0] - 2.0 * uc + n.m[0]) * rc.inv_dz2;
        double d2v_dx2 = (n.r[1] - 2.0 * vc + n.l[1]) / dxx;
        double d2v_dy2 = (n.u[1] - 2.0 * vc + n.d[1]) / dyy;
        double d2v_dz2 = (n.p[1] - 2.0 * vc + n.m[1]) * rc.inv_dz2;
        double d2w_dx2 = (n.r[2] - 2.0 * wc + n.l[2]) / dxx;
        double d2w_dy2 = (n.u[2] - 2.0 * wc + n.d[2]) / dyy;
        double d2w_dz2 = (n.p[2] - 2.0 * wc + n.m[2]) * rc.inv_dz2;
        double nu = rc.mu / fmax(r, 1e-10);
        nu = fmin(nu, 1.0);
        du_dx = clampl(du_dx, 100.0); du_dy = clampl(du_dy, 100.0); du_dz = clampl(du_dz, 100.0);
        dv_dx = clampl(dv_dx, 100.0); dv_dy = clampl(dv_dy, 100.0); dv_dz = clampl(dv_dz, 100.0);
        dw_dx = clampl(dw_dx, 100.0); dw_dy = clampl(dw_dy, 100.0); dw_dz = clampl(dw_dz, 100.0);
        dp_dx = clampl(dp_dx, 100.0); dp_dy = clampl(dp_dy, 100.0); dp_dz = clampl(dp_dz, 100.0);
        d2u_dx2 = clampl(d2u_dx2, 1000.0); d2u_dy2 = clampl(d2u_dy2, 1000.0);
        d2u_dz2 = clampl(d2u_dz2, 1000.0); d2v_dx2 = clampl(d2v_dx2, 1000.0);
        d2v_dy2 = clampl(d2v_dy2, 1000.0); d2v_dz2 = clampl(d2v_dz2, 1000.0);
        d2w_dx2 = clampl(d2w_dx2, 1000.0); d2w_dy2 = clampl(d2w_dy2, 1000.0);
        d2w_dz2 = clampl(d2w_dz2, 1000.0);
        double sw = 0.0;
        if (BUOY) {
            const double dT = Tc - rc.T_ref;
            su += -rc.beta * dT * rc.g0;
            sv += -rc.beta * dT * rc.g1;
            sw += -rc.beta * dT * rc.g2;
        }
        kr[0] = -uc * du_dx - vc * du_dy - wc * du_dz - dp_dx / r +
                nu * (d2u_dx2 + d2u_dy2 + d2u_dz2) + su;
        kr[1] = -uc * dv_dx - vc * dv_dy - wc * dv_dz - dp_dy / r +
                nu * (d2v_dx2 + d2v_dy2 + d2v_dz2) + sv;
        kr[2] = -uc * dw_dx - vc * dw_dy - wc * dw_dz - dp_dz / r +
                nu * (d2w_dx2 + d2w_dy2 + d2w_dz2) + sw;
        double div = du_dx + dv_dy + dw_dz;
        div = fmax(-10.0, fmin(10.0, div));
        kr[3] = -0.1 * r * div;
    }
}

template <int STAGE, bool BUOY>
__global__ __launch_bounds__(256) void k_rk_stage(Geo g, RkCoef rc, Fld4 cur, Fld4 q0, Fld4 acc,
                                                  Fld4 out, const double* __restrict__ rho,
                                                  const double* __restrict__ T,
                                                  const double* __restrict__ dxa,
                                                  const double* __restrict__ dya,
                                                  const double* __restrict__ su_row,
                                                  const double* __restrict__ sv_col) {
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int k = blockIdx.z;
    if (i >= g.nx || j >= g.ny) return;
    const long long idx = cidx(g, i, j, k);
    const bool interior = (i >= 1 && i <= g.nx - 2 && j >= 1 && j <= g.ny - 2 &&
                           k >= g.k0 && k < g.k1);
    double kr[4] = {0.0, 0.0, 0.0, 0.0};
    if (interior) {
        const long long il = (i > 1) ? idx - 1 : cidx(g, g.nx - 2, j, k);
        const long long ir = (i < g.nx - 2) ? idx + 1 : cidx(g, 1, j, k);
        const long long jd = (j > 1) ? idx - g.px : cidx(g, i, g.ny - 2, k);
        const long long ju = (j < g.ny - 2) ? idx + g.px : cidx(g, i, 1, k);
        long long kd = idx, ku = idx;   // 2-D: z terms vanish (stride 0)
        if (g.sz) {
            kd = (k > 1) ? idx - g.sz : cidx(g, i, j, g.nz - 2);
            ku = (k < g.nz - 2) ? idx + g.sz : cidx(g, i, j, 1);
        }
        RkNbr n;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            n.c[f] = cur.f[f][idx];
            n.l[f] = cur.f[f][il];
            n.r[f] = cur.f[f][ir];
            n.d[f] = cur.f[f][jd];
            n.u[f] = cur.f[f][ju];
            n.m[f] = cur.f[f][kd];
            n.p[f] = cur.f[f][ku];
        }
        rk_rhs<BUOY>(rc, n, rho[idx], dxa[i], dya[j], su_row[j], sv_col[i],
                     BUOY ? T[idx] : 0.0, kr);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double o;
        if (STAGE == 0) {
            acc.f[q][idx] = kr[q];
            o = q0.f[q][idx] + rc.fac * kr[q];
        } else if (STAGE < 3) {
            acc.f[q][idx] = acc.f[q][idx] + 2.0 * kr[q];
            o = q0.f[q][idx] + rc.fac * kr[q];
        } else {
            o = q0.f[q][idx] + rc.fac * (acc.f[q][idx] + kr[q]);
        }
        if (q < 3) o = fmax(-100.0, fmin(100.0, o));
        out.f[q][idx] = o;
    }
}

// First and second differences of one field at the cells (i0, i0 + 1) of a
// pair (r02b): c2 the pair, d2 / u2 the
// (periodically resolved) y- / y+ rows, m2 / p2 the z- / z+ planes, xl the
// left of i0, ar the right of i0, bl the left of i0 + 1, xr the right of
// i0 + 1. Same expressions and order as rk_rhs, so the values are bitwise.
struct RkD1 {
    double dx, dy, dz, xx, yy, zz;
};

__device__ __forceinline__ void rk_pair_diffs(const RkCoef& rc, double2 c2, double2 d2, double2 u2,
                                              double2 m2, double2 p2, double xl, double ar,
                                              double bl, double xr, double dxa0, double dxa1,
                                              double dyj, RkD1& da, RkD1& db) {
    const double tdxa = 2.0 * dxa0, tdxb = 2.0 * dxa1, tdy = 2.0 * dyj;
    const double dxxa = dxa0 * dxa0, dxxb = dxa1 * dxa1, dyy = dyj * dyj;
    da.dx = (ar - xl) / tdxa;
    da.dy = (u2.x - d2.x) / tdy;
    da.dz = (p2.x - m2.x) * rc.inv_2dz;
    da.xx = (ar - 2.0 * c2.x + xl) / dxxa;
    da.yy = (u2.x - 2.0 * c2.x + d2.x) / dyy;
    da.zz = (p2.x - 2.0 * c2.x + m2.x) * rc.inv_dz2;
    db.dx = (xr - bl) / tdxb;
    db.dy = (u2.y - d2.y) / tdy;
    db.dz = (p2.y - m2.y) * rc.inv_2dz;
    db.xx = (xr - 2.0 * c2.y + bl) / dxxb;
    db.yy = (u2.y - 2.0 * c2.y + d2.y) / dyy;
    db.zz = (p2.y - 2.0 * c2.y + m2.y) * rc.inv_dz2;
}

// The stage derivatives of a pair (rk_rhs's expressions): diffs(f, da, db)
// yields field f's differences; p first (its gradient enters u, v, w), then
// u, v, w, so only one field's neighbourhood is live at a time.
template <bool BUOY, class Diffs>
__device__ __forceinline__ void rk_pair_kr(const RkCoef& rc, Diffs diffs, double2 uc, double2 vc,
                                           double2 wc, double2 r2, double2 t2, double su,
                                           double sv0, double sv1, bool oka, bool okb,
                                           double (&kra)[4], double (&krb)[4],
                                           double* div2 = nullptr) {
    RkD1 pa_, pb_;
    diffs(3, pa_, pb_);
    const double dpxa = clampl(pa_.dx, 100.0), dpya = clampl(pa_.dy, 100.0),
                 dpza = clampl(pa_.dz, 100.0);
    const double dpxb = clampl(pb_.dx, 100.0), dpyb = clampl(pb_.dy, 100.0),
                 dpzb = clampl(pb_.dz, 100.0);
    const double nua = fmin(rc.mu / fmax(r2.x, 1e-10), 1.0);
    const double nub = fmin(rc.mu / fmax(r2.y, 1e-10), 1.0);
    double sa[3] = {su, sv0, 0.0};
    double sb[3] = {su, sv1, 0.0};
    if (BUOY) {
        const double dTa = t2.x - rc.T_ref, dTb = t2.y - rc.T_ref;
        sa[0] += -rc.beta * dTa * rc.g0;
        sa[1] += -rc.beta * dTa * rc.g1;
        sa[2] += -rc.beta * dTa * rc.g2;
        sb[0] += -rc.beta * dTb * rc.g0;
        sb[1] += -rc.beta * dTb * rc.g1;
        sb[2] += -rc.beta * dTb * rc.g2;
    }
    const double gpa[3] = {dpxa, dpya, dpza}, gpb[3] = {dpxb, dpyb, dpzb};
    double diva = 0.0, divb = 0.0;  // du_dx + dv_dy + dw_dz (clamped terms)
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        RkD1 da, db;
        diffs(f, da, db);
        da.dx = clampl(da.dx, 100.0); da.dy = clampl(da.dy, 100.0); da.dz = clampl(da.dz, 100.0);
        db.dx = clampl(db.dx, 100.0); db.dy = clampl(db.dy, 100.0); db.dz = clampl(db.dz, 100.0);
        da.xx = clampl(da.xx, 1000.0); da.yy = clampl(da.yy, 1000.0); da.zz = clampl(da.zz, 1000.0);
        db.xx = clampl(db.xx, 1000.0); db.yy = clampl(db.yy, 1000.0); db.zz = clampl(db.zz, 1000.0);
        if (oka)
            kra[f] = -uc.x * da.dx - vc.x * da.dy - wc.x * da.dz - gpa[f] / r2.x +
                     nua * (da.xx + da.yy + da.zz) + sa[f];
        if (okb)
            krb[f] = -uc.y * db.dx - vc.y * db.dy - wc.y * db.dz - gpb[f] / r2.y +
                     nub * (db.xx + db.yy + db.zz) + sb[f];
        const double ta = (f == 0) ? da.dx : (f == 1 ? da.dy : da.dz);
        const double tb = (f == 0) ? db.dx : (f == 1 ? db.dy : db.dz);
        diva = (f == 0) ? ta : diva + ta;
        divb = (f == 0) ? tb : divb + tb;
    }
    if (oka) kra[3] = -0.1 * r2.x * fmax(-10.0, fmin(10.0, diva));
    if (okb) krb[3] = -0.1 * r2.y * fmax(-10.0, fmin(10.0, divb));
    if (div2) {  // the clamped divergence itself (k_euler_step scales it by dt)
        div2[0] = fmax(-10.0, fmin(10.0, diva));
        div2[1] = fmax(-10.0, fmin(10.0, divb));
    }
}

// The stage update of one pair of field q (solver_rk4.c stage sums): stage
// 0 stores k into the running sum, 1-2 add 2k, 3 forms the final state.
template <int STAGE, int FL = 0>
__device__ __forceinline__ void rk_pair_update(const RkCoef& rc, const Fld4& q0, const Fld4& acc,
                                               const Fld4& out, int q, long long idx, double ka,
                                               double kb) {
    const double2 q02 = ld2v<FL>(q0.f[q], idx);
    double2 o;
    if (STAGE == 0) {
        st2v<FL>(acc.f[q], idx, make_double2(ka, kb));
        o = make_double2(q02.x + rc.fac * ka, q02.y + rc.fac * kb);
    } else if (STAGE < 3) {
        const double2 a2 = ld2v<FL>(acc.f[q], idx);
        st2v<FL>(acc.f[q], idx, make_double2(a2.x + 2.0 * ka, a2.y + 2.0 * kb));
        o = make_double2(q02.x + rc.fac * ka, q02.y + rc.fac * kb);
    } else {
        const double2 a2 = ld2v<FL>(acc.f[q], idx);
        o = make_double2(q02.x + rc.fac * (a2.x + ka), q02.y + rc.fac * (a2.y + kb));
    }
    if (q < 3) {
        o.x = fmax(-100.0, fmin(100.0, o.x));
        o.y = fmax(-100.0, fmin(100.0, o.y));
    }
    st2v<FL>(out.f[q], idx, o);
}

// The same stage on x pairs (r02b): each lane owns cells (i0, i0 + 1) and
// moves every field with 16-B loads / stores; the cell's x neighbours are the
// pair's other cell or one scalar load (the periodic indices of i = 1 and
// nx - 2 by address), y / z neighbours are pair loads of the (periodically
// resolved) neighbour row / plane. Half the load instructions of k_rk_stage;
// rk_rhs's expressions, so the values are bitwise the per-cell kernel's.
template <int STAGE, bool BUOY>
__global__ __launch_bounds__(256) void k_rk_stage2(Geo g, RkCoef rc, Fld4 cur, Fld4 q0, Fld4 acc,
                                                   Fld4 out, const double* __restrict__ rho,
                                                   const double* __restrict__ T,
                                                   const double* __restrict__ dxa,
                                                   const double* __restrict__ dya,
                                                   const double* __restrict__ su_row,
                                                   const double* __restrict__ sv_col) {
    const int i0 = blockIdx.x * 128 + 2 * (threadIdx.x & 63);
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int k = blockIdx.z;
    if (i0 >= g.nx || j >= g.ny) return;
    const long long idx = cidx(g, i0, j, k);
    const bool rowin = (j >= 1 && j <= g.ny - 2 && k >= g.k0 && k < g.k1);
    const bool ina = rowin && i0 >= 1 && i0 <= g.nx - 2;
    const bool inb = rowin && i0 + 1 <= g.nx - 2;
    double kra[4] = {0.0, 0.0, 0.0, 0.0}, krb[4] = {0.0, 0.0, 0.0, 0.0};
    if (ina || inb) {
        const long long row = idx - i0;
        const long long jd = (j > 1) ? idx - g.px : cidx(g, i0, g.ny - 2, k);
        const long long ju = (j < g.ny - 2) ? idx + g.px : cidx(g, i0, 1, k);
        long long kd = idx, ku = idx;  // 2-D: z terms vanish (stride 0)
        if (g.sz) {
            kd = (k > 1) ? idx - g.sz : cidx(g, i0, j, g.nz - 2);
            ku = (k < g.nz - 2) ? idx + g.sz : cidx(g, i0, j, 1);
        }
        // x neighbours outside the pair: left of i0, right of i0 + 1
        const long long la = (i0 > 1) ? idx - 1 : row + (g.nx - 2);
        const long long rb = (i0 + 1 < g.nx - 2) ? idx + 2 : row + 1;
        const double2 r2 = ld2(rho, idx);
        const double2 t2 = BUOY ? ld2(T, idx) : make_double2(0.0, 0.0);
        const double dyj = dya[j], su = su_row[j];
        const double dxa0 = dxa[i0], dxa1 = dxa[min(i0 + 1, g.nx - 1)];
        const bool oka = ina && !(r2.x <= 1e-10) && !(fabs(dxa0) < 1e-10) && !(fabs(dyj) < 1e-10);
        const bool okb = inb && !(r2.y <= 1e-10) && !(fabs(dxa1) < 1e-10) && !(fabs(dyj) < 1e-10);
        const double2 uc = ld2(cur.f[0], idx), vc = ld2(cur.f[1], idx), wc = ld2(cur.f[2], idx);
        auto diffs = [&](int f, RkD1& da, RkD1& db) __attribute__((always_inline)) {
            const double* F = cur.f[f];
            const double2 c2 = ld2(F, idx), d2 = ld2(F, jd), u2 = ld2(F, ju);
            const double2 m2 = ld2(F, kd), p2 = ld2(F, ku);
            const double xl = F[la], xr = F[rb];
            const double ar = (i0 < g.nx - 2) ? c2.y : F[row + 1];
            const double bl = (i0 + 1 > 1) ? c2.x : F[row + (g.nx - 2)];
            rk_pair_diffs(rc, c2, d2, u2, m2, p2, xl, ar, bl, xr, dxa0, dxa1, dyj, da, db);
        };
        rk_pair_kr<BUOY>(rc, diffs, uc, vc, wc, r2, t2, su, sv_col[i0],
                         sv_col[min(i0 + 1, g.nx - 1)], oka, okb, kra, krb);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) rk_pair_update<STAGE>(rc, q0, acc, out, q, idx, kra[q], krb[q]);
}

// ---------------------------------------------------------------------------
// Explicit Euler (solver_explicit_euler.c:391-525): the whole update of u, v,
// w, p in one pass on k_rk_stage2's x pairs (128 columns x 4 rows per
// workgroup, 16-B loads and stores). The momentum expressions are the RK
// RHS's (rk_pair_kr); what differs from an RK stage:
//   - the stencil reads the ghost cells: neighbours are idx +- 1, +- px,
//     +- sz by address, no periodic index resolution (2-D: sz = 0);
//   - the increments rc.fac * k (rc.fac = min(dt, 1e-4)) are clamped to +-1
//     before they are added, u, v, w then to +-100;
//   - dp = -0.1 * fac * rho * clamp(div, +-10), clamped to +-1;
//   - boundary cells and the cells the reference skips (rho <= 1e-10 or a
//     spacing below 1e-10) keep their values: every cell of `out` is written,
//     so the caller swaps cur and out.
// Per cell: reads u, v, w, p, rho (and T with buoyancy), writes u, v, w, p:
// 72 / 80 B of algorithmic traffic.
// ---------------------------------------------------------------------------
template <bool BUOY>
__global__ __launch_bounds__(256) void k_euler_step(Geo g, RkCoef rc, Fld4 cur, Fld4 out,
                                                    const double* __restrict__ rho,
                                                    const double* __restrict__ T,
                                                    const double* __restrict__ dxa,
                                                    const double* __restrict__ dya,
                                                    const double* __restrict__ su_row,
                                                    const double* __restrict__ sv_col) {
    const int i0 = blockIdx.x * 128 + 2 * (threadIdx.x & 63);
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int k = blockIdx.z;
    if (i0 >= g.nx || j >= g.ny) return;
    const long long idx = cidx(g, i0, j, k);
    const bool rowin = (j >= 1 && j <= g.ny - 2 && k >= g.k0 && k < g.k1);
    const bool ina = rowin && i0 >= 1 && i0 <= g.nx - 2;
    const bool inb = rowin && i0 + 1 <= g.nx - 2;
    double2 o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = ld2(cur.f[q], idx);
    if (ina || inb) {
        const long long jd = idx - g.px, ju = idx + g.px;
        const long long kd = idx - g.sz, ku = idx + g.sz;  // 2-D: sz = 0, z terms vanish
        const double2 r2 = ld2(rho, idx);
        const double2 t2 = BUOY ? ld2(T, idx) : make_double2(0.0, 0.0);
        const double dyj = dya[j], su = su_row[j];
        const double dxa0 = dxa[i0], dxa1 = dxa[min(i0 + 1, g.nx - 1)];
        const bool oka = ina && !(r2.x <= 1e-10) && !(fabs(dxa0) < 1e-10) && !(fabs(dyj) < 1e-10);
        const bool okb = inb && !(r2.y <= 1e-10) && !(fabs(dxa1) < 1e-10) && !(fabs(dyj) < 1e-10);
        auto diffs = [&](int f, RkD1& da, RkD1& db) __attribute__((always_inline)) {
            const double* F = cur.f[f];
            const double2 c2 = ld2(F, idx), d2 = ld2(F, jd), u2 = ld2(F, ju);
            const double2 m2 = ld2(F, kd), p2 = ld2(F, ku);
            // x neighbours outside the pair; a cell that needs one is interior,
            // so i0 - 1 >= 0 and i0 + 2 <= nx - 1 where the value is used
            const double xl = ina ? F[idx - 1] : 0.0;
            const double xr = inb ? F[idx + 2] : 0.0;
            rk_pair_diffs(rc, c2, d2, u2, m2, p2, xl, c2.y, c2.x, xr, dxa0, dxa1, dyj, da, db);
        };
        double kra[4] = {0.0, 0.0, 0.0, 0.0}, krb[4] = {0.0, 0.0, 0.0, 0.0};
        double div2[2] = {0.0, 0.0};
        rk_pair_kr<BUOY>(rc, diffs, o[0], o[1], o[2], r2, t2, su, sv_col[i0],
                         sv_col[min(i0 + 1, g.nx - 1)], oka, okb, kra, krb, div2);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (oka) o[q].x = clampl(o[q].x + clampl(rc.fac * kra[q], 1.0), 100.0);
            if (okb) o[q].y = clampl(o[q].y + clampl(rc.fac * krb[q], 1.0), 100.0);
        }
        if (oka) o[3].x = o[3].x + clampl(-0.1 * rc.fac * r2.x * div2[0], 1.0);
        if (okb) o[3].y = o[3].y + clampl(-0.1 * rc.fac * r2.y * div2[1], 1.0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) st2(out.f[q], idx, o[q]);
}

// max |u|, max |p| and the non-finite flag over the owned planes (the
// stats / NaN scan of the RK wrappers, solver_registry.c:31-49,760-768)
static __global__ __launch_bounds__(256) void k_vel_stats(Geo g, const double* __restrict__ U,
                                                          const double* __restrict__ V,
                                                          const double* __restrict__ W,
                                                          const double* __restrict__ P,
                                                          unsigned long long* red) {
    __shared__ double shv[4], shp[4];
    __shared__ int shbad;
    if (threadIdx.x == 0) shbad = 0;
    __syncthreads();
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int k = blockIdx.z;
    double mv = 0.0, mp = 0.0;
    if (i < g.nx && j < g.ny) {
        const long long idx = cidx(g, i, j, k);
        const double u = U[idx], v = V[idx], w = W[idx], p = P[idx];
        if (!isfinite(u) || !isfinite(v) || !isfinite(w) || !isfinite(p)) shbad = 1;
        const double vel2 = (u * u) + (v * v) + (w * w);  // sqrt on the host (cell_stats)
        if (vel2 > mv) mv = vel2;
        const double ap = fabs(p);
        if (ap > mp) mp = ap;
    }
    mv = wave_max(mv);
    mp = wave_max(mp);
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
