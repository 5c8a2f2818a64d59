// bicgstab.hpp -- BiCGSTAB on the device (HIP_POISSON_BICGSTAB, the backend of
// create_bicgstab_gpu_solver).
//
// Numerics follow the CPU reference, linear_solver_bicgstab.c:265-495, as the
// other three backends follow their CPU files, and not the reference's CUDA
// file (poisson_solver_bicgstab_gpu.cu), which counts the half-step exits
// differently, ignores check_interval and always applies the closing BC:
//   A = -(7-point Laplacian) (5-point when nz = 1), zero walls for r, r^, p,
//   v, s, t, the Neumann shell copy on x at solve start, r_0 = -rhs + lap(x),
//   r^ = r_0, rho = alpha = omega = 1, p = v = 0, then per iteration
//     rho' = (r^, r);  beta = (rho' / rho) (alpha / omega)
//     p = r + beta (p - omega v);  v = A p;  alpha = rho' / (r^, v)
//     s = r - alpha v;  [||s|| test, every iteration]
//     t = A s;  omega = (t, s) / (t, t)
//     x += alpha p + omega s;  r = s - omega t;  [||r|| test, check_interval]
// with the exits and statistics of the reference (bcg_fin_* below).
//
// One iteration is three launches on the row-pair sweep tiling of k_cgA /
// k_cgB (sgeo: 128 columns x sweep_rows, z runs of kchunk, double2 lanes, the
// same edge loads), B/cell of fp64 traffic:
//   k_bcg_v  reads r, p_old, v_old (stencil halo), r^; writes p_new, v_new;
//            (r^, v)                                                     48
//   k_bcg_t  reads r, v (stencil halo); writes s, t; (s,s), (t,s), (t,t) 32
//   k_bcg_x  reads x, p, s, t, r^; writes x, r; (r,r), (r^,r)            56
// p_new = r + beta (p_old - omega v_old) and s = r - alpha v are formed on the
// fly at the cell and its six neighbours, as k_cgA forms r + beta p_old, so
// neither needs a pass of its own. p and v are double-buffered (other tiles
// still read the old ones): the context's four-slot p ring gives the two pairs.
//
// rho, alpha, beta, omega, the tolerances, the residual, iterations, status,
// done and the half-step flag live in a BcgState on the device. Each launch
// writes per-workgroup partials of its dot products; the last workgroup to
// arrive sums them in index order and takes the iteration's decision, so two
// solves of one input give the same bits. Launches after `done` return at
// once; k_bcg_finalize applies the x += alpha p the half-step exits leave.
// Stores are plain vector stores.
#pragma once

#include "kernels.hpp"

namespace cfdhip {

struct BcgState {
    double rho;    // (r^, r) of the iteration in progress
    double alpha, omega;
    double beta;   // for the next k_bcg_v
    double res;    // res_norm of the reference (||r||, or ||s|| after a half-step exit)
    double res0;
    double tol;    // max(rel_tol * res0, abs_tol)
    double abs_tol;
    int iterations;
    int done;
    int status;
    int half;      // a half-step exit left x += alpha p pending (k_bcg_finalize)
    int max_iter;
    int check_interval;
};

constexpr double BCG_BREAKDOWN = 1e-30;  // BICGSTAB_BREAKDOWN_THRESHOLD

// rho' of the next iteration is known: its breakdown test and beta
// (linear_solver_bicgstab.c:340-354); `it` is the iteration about to start
__device__ __forceinline__ void bcg_next_rho(BcgState* st, double rho_new, int it) {
    if (fabs(rho_new) < BCG_BREAKDOWN) {
        st->done = 1;
        st->status = ST_STAGNATED;
        st->iterations = it + 1;  // res stays the previous res_norm
        return;
    }
    st->beta = (rho_new / st->rho) * (st->alpha / st->omega);
    st->rho = rho_new;
}

// after r_0 and (r_0, r_0) (:311-332); (r^, r_0) is the same sum
__device__ __forceinline__ void bcg_fin_setup(BcgState* st, double tot, double rel_tol,
                                              double abs_tol, int max_iter, int check_interval) {
    const double res0 = sqrt(tot);
    double tol = rel_tol * res0;
    if (tol < abs_tol) tol = abs_tol;
    st->rho = 1.0;
    st->alpha = 1.0;
    st->omega = 1.0;
    st->beta = 0.0;
    st->res = res0;
    st->res0 = res0;
    st->tol = tol;
    st->abs_tol = abs_tol;
    st->iterations = 0;
    st->done = 0;
    st->status = ST_MAX_ITER;
    st->half = 0;
    st->max_iter = max_iter;
    st->check_interval = check_interval;
    if (res0 < abs_tol) {  // converged at start: returns before the closing BC
        st->done = 1;
        st->status = ST_CONVERGED;
    } else if (max_iter <= 0) {  // the loop never runs: the final test (:478)
        st->done = 1;
        st->status = (res0 < tol) ? ST_CONVERGED : ST_MAX_ITER;
    } else {
        bcg_next_rho(st, tot, 0);
    }
}

// after (r^, v) (:370-383)
__device__ __forceinline__ void bcg_fin_v(BcgState* st, double rhv, int it) {
    if (fabs(rhv) < BCG_BREAKDOWN) {
        st->done = 1;
        st->status = ST_STAGNATED;
        st->iterations = it + 1;
        return;
    }
    st->alpha = st->rho / rhv;
}

// after (s, s), (t, s), (t, t) (:396-425)
__device__ __forceinline__ void bcg_fin_t(BcgState* st, double ss, double ts, double tt, int it) {
    const double s_norm = sqrt(ss);
    if (s_norm < st->tol || s_norm < st->abs_tol) {
        st->done = 1;
        st->status = ST_CONVERGED;
        st->iterations = it + 1;
        st->res = s_norm;
        st->half = 1;
    } else if (fabs(tt) < BCG_BREAKDOWN) {
        st->done = 1;
        st->status = ST_STAGNATED;
        st->iterations = it + 1;
        st->res = s_norm;
        st->half = 1;
    } else {
        st->omega = ts / tt;
    }
}

// after (r, r) and (r^, r) of the new r (:451-478, then :340-354 of it + 1)
__device__ __forceinline__ void bcg_fin_x(BcgState* st, double rr, double rhr, int it) {
    const double res = sqrt(rr);
    st->res = res;
    st->iterations = it + 1;
    const bool conv = (res < st->tol) || (res < st->abs_tol);
    if ((it % st->check_interval) == 0 && conv) {
        st->done = 1;
        st->status = ST_CONVERGED;
    } else if (fabs(st->omega) < BCG_BREAKDOWN) {
        st->done = 1;
        st->status = ST_STAGNATED;
    } else if (it + 1 >= st->max_iter) {  // loop exhausted: one last test
        st->done = 1;
        st->status = conv ? ST_CONVERGED : ST_MAX_ITER;
    } else {
        bcg_next_rho(st, rhr, it + 1);
    }
}

// ND grid totals in one ticket: partial d of workgroup b at partials[d * nb +
// b]; the last workgroup sums each in index order (grid_sum_last_n's protocol).
// `sh` needs ND * NTH / 64 doubles of LDS no wave still reads.
template <int NTH, int ND>
__device__ __forceinline__ bool bcg_grid_sum(const double (&bt)[ND], double* partials,
                                             unsigned* counter, double* sh, int* flag,
                                             double (&tot)[ND]) {
    const unsigned nb = gridDim.x;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int d = 0; d < ND; ++d) store_sc1(&partials[(size_t)d * nb + blockIdx.x], bt[d]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned t = __hip_atomic_fetch_add((gu32*)counter, 1u, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        *flag = (t == nb - 1) ? 1 : 0;
    }
    __syncthreads();
    if (*flag == 0) return false;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        double s = 0.0;
        for (unsigned b = threadIdx.x; b < nb; b += NTH) s += load_sc1(&partials[(size_t)d * nb + b]);
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) sh[d * (NTH / 64) + (threadIdx.x >> 6)] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            double a = 0.0;
#pragma unroll
            for (int w = 0; w < NTH / 64; ++w) a += sh[d * (NTH / 64) + w];
            tot[d] = a;
        }
        __hip_atomic_store((gu32*)counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return true;
}

// r_0 = -rhs + lap(x) (compute_residual, :140-163), r^ = r_0, (r_0, r_0)
static __global__ __launch_bounds__(NT) void k_bcg_setup(Geo g, Lap L,
                                                         const double* __restrict__ rhs,
                                                         const double* __restrict__ x,
                                                         double* __restrict__ r,
                                                         double* __restrict__ rh, BcgState* st,
                                                         double* partials, unsigned* counter,
                                                         double rel_tol, double abs_tol,
                                                         int max_iter, int check_interval) {
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
            double lap = lap7(L, xc, x[idx - 1], x[idx + 1], x[idx - g.px], x[idx + g.px], xm, xp);
            double rv = -rhs[idx] + lap;
            r[idx] = rv;
            rh[idx] = rv;
            acc += rv * rv;
            xm = xc;
            xc = xp;
        }
    }
    double bt = block_sum(acc, sh);
    double tot;
    if (grid_sum_last(bt, partials, counter, sh, &flag, tot) && threadIdx.x == 0)
        bcg_fin_setup(st, tot, rel_tol, abs_tol, max_iter, check_interval);
}

// The two stencil launches of an iteration, one march:
//   MODE 0 (k_bcg_v): f = fa + beta (fb - omega fc) = p_new (FIRST: p_old =
//     v_old = 0, not read), o1 = f, o2 = A f = v_new, dot (r^, v_new)
//   MODE 1 (k_bcg_t): f = fa - alpha fb = s, o1 = f, o2 = A f = t,
//     dots (s, s), (t, s), (t, t)
// f is formed at the centre, the y-halo rows and the x-edge cells from the
// raw operands, whose walls are zero, so f's walls are zero too.
template <int TY, int MODE, bool FIRST>
static __global__ __launch_bounds__(64 * TY) void k_bcg_sweep(
    SGeo g, Lap L, const double* __restrict__ fa, const double* __restrict__ fb,
    const double* __restrict__ fc, const double* __restrict__ rh, double* __restrict__ o1,
    double* __restrict__ o2, BcgState* st, double* partials, unsigned* counter, int it) {
    constexpr int ND = (MODE == 0) ? 1 : 3;
    constexpr bool B = !(MODE == 0 && FIRST);  // fb is read
    constexpr bool C = (MODE == 0) && !FIRST;  // fc is read
    __shared__ double2 rows[2][TY + 2][64];
    __shared__ double sh[3][TY];
    __shared__ int flag;
    if (st->done) return;
    const double c1 = (MODE == 0) ? st->beta : st->alpha;
    const double c2 = (MODE == 0) ? st->omega : 0.0;
    RowPair c = row_pair<TY>(g);
    const bool halo = (c.w == 0) || (c.w == TY - 1);
    const int jh = (c.w == 0) ? max(c.j - 1, 0) : min(c.j + 1, g.ny - 1);
    const int hslot = (c.w == 0) ? 0 : TY + 1;
    const long long hoff = (long long)(jh - min(c.j, g.ny - 1)) * g.px;
    const bool xok = c.i0 < g.nx;
    const bool eok_l = c.lane == 0 && c.i0 >= 1 && xok;
    const bool eok_r = c.lane == 63 && c.i0 + 2 < g.nx;
    const double2 zero = make_double2(0.0, 0.0);
    auto form1 = [&](double a, double b, double cc) {
        if (MODE == 0) return a + c1 * (b - c2 * cc);  // :361
        return a - c1 * b;                             // :390
    };
    auto form2 = [&](double2 a, double2 b, double2 cc) {
        return make_double2(form1(a.x, b.x, cc.x), form1(a.y, b.y, cc.y));
    };
    auto ldc = [&](const double* f, bool on, long long i) { return on ? ld2(f, i) : zero; };
    auto at2 = [&](bool ok, long long i) {  // f at the pair starting at i
        return form2(ldc(fa, ok, i), ldc(fb, ok && B, i), ldc(fc, ok && C, i));
    };
    auto at1 = [&](bool ok, long long i) {  // f at the single cell i
        return form1(ok ? fa[i] : 0.0, (ok && B) ? fb[i] : 0.0, (ok && C) ? fc[i] : 0.0);
    };
    double acc[3] = {0.0, 0.0, 0.0};
    long long idx = c.idx;
    double2 pm = at2(xok, idx - g.sz);
    double2 pc = at2(xok, idx);
    double2 hc = at2(xok && halo, idx + hoff);
    int buf = 0;
    for (int k = c.kb; k < c.ke; ++k, idx += g.ps) {
        const long long ip = idx + g.sz;
        const double2 pp = at2(xok, ip);
        const double2 hn = at2(xok && halo && k + 1 < c.ke, ip + hoff);
        const double el = at1(eok_l, idx - 1);
        const double er = at1(eok_r, idx + 2);
        const double2 rv = (MODE == 0 && xok && c.act) ? ld2(rh, idx) : zero;
        rows[buf][c.w + 1][c.lane] = pc;
        if (halo) rows[buf][hslot][c.lane] = hc;
        __syncthreads();
        const double2 ys = rows[buf][c.w][c.lane];
        const double2 yn = rows[buf][c.w + 2][c.lane];
        double left = __shfl_up(pc.y, 1, 64);
        double right = __shfl_down(pc.x, 1, 64);
        if (c.lane == 0) left = el;
        if (c.lane == 63) right = er;
        const double A0 = -lap7(L, pc.x, left, pc.y, ys.x, yn.x, pm.x, pp.x);
        const double A1 = -lap7(L, pc.y, pc.x, right, ys.y, yn.y, pm.y, pp.y);
        if (c.act) {
            double2 w1, w2;
            w1.x = c.in0 ? pc.x : 0.0;
            w1.y = c.in1 ? pc.y : 0.0;
            w2.x = c.in0 ? A0 : 0.0;
            w2.y = c.in1 ? A1 : 0.0;
            st2(o1, idx, w1);
            st2(o2, idx, w2);
        }
        if (MODE == 0) {
            if (c.in0) acc[0] += rv.x * A0;
            if (c.in1) acc[0] += rv.y * A1;
        } else {
            if (c.in0) {
                acc[0] += pc.x * pc.x;
                acc[1] += A0 * pc.x;
                acc[2] += A0 * A0;
            }
            if (c.in1) {
                acc[0] += pc.y * pc.y;
                acc[1] += A1 * pc.y;
                acc[2] += A1 * A1;
            }
        }
        pm = pc;
        pc = pp;
        hc = hn;
        buf ^= 1;
    }
    // deterministic workgroup sums: wave tree, then waves in order
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const double a = wave_sum(acc[d]);
        if (c.lane == 0) sh[d][c.w] = a;
    }
    __syncthreads();
    double bt[ND], tot[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        bt[d] = 0.0;
        if (threadIdx.x == 0)
            for (int q = 0; q < TY; ++q) bt[d] += sh[d][q];
    }
    double* shs = (double*)&rows[0][0][0];
    if (bcg_grid_sum<64 * TY, ND>(bt, partials, counter, shs, &flag, tot) && threadIdx.x == 0) {
        if constexpr (MODE == 0) bcg_fin_v(st, tot[0], it);
        else bcg_fin_t(st, tot[0], tot[1], tot[2], it);
    }
}

// x += alpha p + omega s (:432), r = s - omega t (:442); (r, r), (r^, r).
// Pointwise on the same tiling (no halo, no LDS rows).
template <int TY>
static __global__ __launch_bounds__(64 * TY) void k_bcg_x(
    SGeo g, double* __restrict__ x, const double* __restrict__ p, const double* __restrict__ s,
    const double* __restrict__ t, const double* __restrict__ rh, double* __restrict__ r,
    BcgState* st, double* partials, unsigned* counter, int it) {
    __shared__ double sh[2][TY];
    __shared__ double shs[2 * TY];
    __shared__ int flag;
    if (st->done) return;
    const double alpha = st->alpha, omega = st->omega;
    RowPair c = row_pair<TY>(g);
    double acc[2] = {0.0, 0.0};
    if (c.act) {
        long long idx = c.idx;
        for (int k = c.kb; k < c.ke; ++k, idx += g.ps) {
            const double2 xv = ld2(x, idx), pv = ld2(p, idx), sv = ld2(s, idx), tv = ld2(t, idx);
            const double2 hv = ld2(rh, idx);
            double2 xw, rw;
            xw.x = c.in0 ? xv.x + (alpha * pv.x + omega * sv.x) : xv.x;
            xw.y = c.in1 ? xv.y + (alpha * pv.y + omega * sv.y) : xv.y;
            rw.x = c.in0 ? sv.x - omega * tv.x : 0.0;
            rw.y = c.in1 ? sv.y - omega * tv.y : 0.0;
            st2(x, idx, xw);
            st2(r, idx, rw);
            if (c.in0) {
                acc[0] += rw.x * rw.x;
                acc[1] += hv.x * rw.x;
            }
            if (c.in1) {
                acc[0] += rw.y * rw.y;
                acc[1] += hv.y * rw.y;
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const double a = wave_sum(acc[d]);
        if (c.lane == 0) sh[d][c.w] = a;
    }
    __syncthreads();
    double bt[2] = {0.0, 0.0}, tot[2];
    if (threadIdx.x == 0)
        for (int q = 0; q < TY; ++q) {
            bt[0] += sh[0][q];
            bt[1] += sh[1][q];
        }
    if (bcg_grid_sum<64 * TY, 2>(bt, partials, counter, shs, &flag, tot) && threadIdx.x == 0)
        bcg_fin_x(st, tot[0], tot[1], it);
}

// The x += alpha p a half-step exit leaves (:399, :415); p0 / p1: p_it by the
// parity of it = iterations - 1.
static __global__ __launch_bounds__(NT) void k_bcg_finalize(Geo g, const double* __restrict__ p0,
                                                            const double* __restrict__ p1,
                                                            double* __restrict__ x,
                                                            const BcgState* st) {
    if (!st->half) return;
    const double alpha = st->alpha;
    const double* __restrict__ p = ((st->iterations - 1) & 1) ? p1 : p0;
    const int ntiles = g.tiles_x * g.tiles_y * g.tiles_z;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        TileCoord c = tile_coord(g, t);
        if (!c.active) continue;
        long long idx = cidx(g, c.i, c.j, c.kb);
        for (int k = c.kb; k < c.ke; ++k, idx += g.ps) x[idx] += alpha * p[idx];
    }
}

}  // namespace cfdhip
