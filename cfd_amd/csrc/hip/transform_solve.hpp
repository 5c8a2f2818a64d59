// transform_solve.hpp -- the direct transform pressure solvers: sine
// (HIP_POISSON_DST) and cosine (HIP_POISSON_DCT). One table cache, one pass
// function and one solve serve both; what differs by kind is the table, the
// residual that decides the status, the boundary write and the scaling.
//
// The sine solve. Inside a solve the boundary cells of x are frozen (the
// reference's CG applies its BC to x only before and after the loop), so the
// interior system is the constant-coefficient 7-point Laplacian with Dirichlet data. On the
// uniform box the type-I sine transform along each axis diagonalises it:
//   x = S_x S_y S_z [ norm / (lx[i] + ly[j] + lz[k]) * S_z S_y S_x b ],
//   b = -rhs + (frozen boundary neighbours) / h^2,  norm = prod 2 / (n + 1).
// Every transform is a dense product with the symmetric sine matrix S_n
// (host/dst_tables.h) on the fp64 matrix cores (v_mfma_f64_16x16x4_f64):
//   k_dst_strided  Y = S X along y or z: the 16 columns of a tile are 16
//                  consecutive x cells, so the B operand is one 128-B load
//                  per k row; A comes from the table (S is symmetric, so the
//                  16 rows of a fragment are read as 16 consecutive entries
//                  of table row k);
//   k_dst_x        Y = X S along x: 32 rows of X are staged through LDS in
//                  64-column chunks (coalesced loads), the A fragments are
//                  read from there, B from the table; the first pass forms b
//                  while it loads.
// Both read and write interior cells only (never a pad column or a boundary
// cell): out-of-range rows, columns and k steps are masked to zero on the
// load and skipped on the store; the table is zero-padded to its 64-row tile.
// The summation order is fixed, so a solve is bitwise reproducible.
//
// The cosine solve. Red-Black SOR and Jacobi apply the Neumann boundary
// condition after every sweep, so at their fixed point every shell cell equals
// its interior neighbour and the interior operator is the cell-centred Neumann
// Laplacian: the 7-point stencil whose end cells lose the missing neighbour's
// term. On the uniform box the orthonormal type-II cosine transform along each
// axis diagonalises it,
//   Q_n[a][b] = w_a cos(pi a (2 b + 1) / (2 n)),  lambda_n[a] = 4 sin^2(pi a / (2 n)) / h^2,
//   x = Qx^T Qy^T Qz^T [ (Qz Qy Qx (-rhs)) / (lx[i] + ly[j] + lz[k]) ]   (interior),
// followed by the Neumann shell (the sign is the relaxation solvers': they
// solve lap(x) = rhs, and the operator above is -lap). The transforms are the
// sine solver's passes with cosine tables. A pass computes out[a] = sum_b
// T[b][a] in[b]; the sine table is symmetric, Q is not: the forward pass is
// given Q^T, the inverse pass Q.
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
// Host code + kernels; private to projection_hip.hip (through
// poisson_solve.hpp).
#pragma once

#include "ctx.hpp"
#include "../host/dst_tables.h"

namespace cfdhip {

typedef double dst_d4 __attribute__((ext_vector_type(4)));

// one strided pass: the transformed axis (n points, stride sa), 16-column
// tiles along x (nc columns), nb batch lines of stride sb
struct DstAxis {
    int n, nc, nb;
    long long sa, sb;
    long long off0;  // the first interior cell of batch line 0
    int np;          // table pitch
    int tiles_a, tiles_c;
};

// the eigenvalue scaling of the last forward pass: norm / (la + lc + lb) with
// l = e[index] * 1/h^2 along the pass's axis, its columns and its batch lines
// (eb == nullptr: no third axis)
struct DstScale {
    const double* ea;
    const double* ec;
    const double* eb;
    double ha, hc, hb, norm;
};

// the x pass: lines (j, k) of n = nx - 2 cells
struct DstRows {
    int n, nj, nk, k0;
    long long px, ps;
    int np;
    int tiles_j, tiles_a;
};

constexpr int DST_TA = 64;   // k_dst_strided: output rows per wave (4 MFMA tiles)
constexpr int DST_XR = 32;   // k_dst_x: lines per workgroup (2 MFMA tiles)
constexpr int DST_XK = 64;   // k_dst_x: columns of X staged per chunk
constexpr int DST_XP = 66;   // LDS row pitch: conflict-free fragment reads

// Workgroup = 4 waves on one 64-row tile of the output and 4 adjacent
// 16-column tiles (the waves share the table loads through the L1). COS (with
// SCALE): the cosine solve's scaling, a plain division by the
// eigenvalue sum with the zero mode written as 0.0 and never divided.
template <bool SCALE, bool COS = false>
static __global__ __launch_bounds__(256) void k_dst_strided(DstAxis g,
                                                            const double* __restrict__ S,
                                                            const double* __restrict__ in,
                                                            double* __restrict__ out,
                                                            DstScale sc) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int t = blockIdx.x;
    const int tc = t % g.tiles_c;
    t /= g.tiles_c;
    const int ta = t % g.tiles_a;
    const int q = t / g.tiles_a;
    if (q >= g.nb || tc * 64 + w * 16 >= g.nc) return;  // wave-uniform
    const int a0 = ta * DST_TA;
    const int col = tc * 64 + w * 16 + (lane & 15);
    const int kq = lane >> 4;
    const bool cin = col < g.nc;
    const long long base = g.off0 + (long long)q * g.sb + col;
    dst_d4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = dst_d4{0.0, 0.0, 0.0, 0.0};
    const int kend = (g.n + 3) & ~3;
    for (int b0 = 0; b0 < kend; b0 += 4) {
        const int kk = b0 + kq;
        double xv = 0.0;
        if (cin && kk < g.n) xv = in[base + (long long)kk * g.sa];
        const double* srow = S + (size_t)kk * g.np + a0 + (lane & 15);
#pragma unroll
        for (int m = 0; m < 4; ++m)
            acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(srow[16 * m], xv, acc[m], 0, 0, 0);
    }
    if (!cin) return;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + 16 * m + kq + 4 * r;
            if (a >= g.n) continue;
            double v = acc[m][r];
            if (SCALE && COS) {
                double lam = (sc.ea[a] * sc.ha) + (sc.ec[col] * sc.hc);
                if (sc.eb) lam += sc.eb[q] * sc.hb;
                const bool zero_mode = (a == 0) && (col == 0) && (!sc.eb || q == 0);
                v = zero_mode ? 0.0 : v / lam;
            } else if (SCALE) {
                double lam = (sc.ea[a] * sc.ha) + (sc.ec[col] * sc.hc);
                if (sc.eb) lam += sc.eb[q] * sc.hb;
                v *= sc.norm / lam;
            }
            out[base + (long long)a * g.sa] = v;
        }
    }
}

// Workgroup = 4 waves on 32 lines (consecutive j of one plane) x 256 output
// columns, 64 per wave. FORM_B: the input is b = -rhs + (frozen boundary
// neighbours of xb) / h^2, formed on the load (in = rhs). NEG (without
// FORM_B): the input is -in, with no boundary terms (the cosine solve).
template <bool FORM_B, bool NEG = false>
static __global__ __launch_bounds__(256) void k_dst_x(DstRows g, const double* __restrict__ S,
                                                      const double* __restrict__ in,
                                                      const double* __restrict__ xb,
                                                      double* __restrict__ out, Lap L, int is3d) {
    __shared__ double xs[DST_XR][DST_XP];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int t = blockIdx.x;
    const int ta = t % g.tiles_a;
    t /= g.tiles_a;
    const int tj = t % g.tiles_j;
    const int kq = t / g.tiles_j;  // 0 .. nk - 1
    const int j0 = tj * DST_XR;    // interior line index
    const long long plane = (long long)(g.k0 + kq) * g.ps;
    const int a0w = ta * 256 + w * 64;
    const bool wact = a0w < g.np;  // wave-uniform: this wave has output columns
    dst_d4 acc[2][4];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = dst_d4{0.0, 0.0, 0.0, 0.0};
    for (int b0 = 0; b0 < g.n; b0 += DST_XK) {
        __syncthreads();  // the previous chunk's fragments are read
#pragma unroll
        for (int u = 0; u < DST_XR * DST_XK / 256; ++u) {
            const int e = (int)threadIdx.x + 256 * u;
            const int row = e >> 6, bl = e & 63;
            const int b = b0 + bl, jj = j0 + row;
            double v = 0.0;
            if (jj < g.nj && b < g.n) {
                const long long idx = plane + (long long)(jj + 1) * g.px + (b + 1);
                if (FORM_B) {
                    v = -in[idx];
                    if (b == 0) v += xb[idx - 1] * L.dx2_inv;
                    if (b == g.n - 1) v += xb[idx + 1] * L.dx2_inv;
                    if (jj == 0) v += xb[idx - g.px] * L.dy2_inv;
                    if (jj == g.nj - 1) v += xb[idx + g.px] * L.dy2_inv;
                    if (is3d) {
                        if (kq == 0) v += xb[idx - g.ps] * L.inv_dz2;
                        if (kq == g.nk - 1) v += xb[idx + g.ps] * L.inv_dz2;
                    }
                } else if (NEG) {
                    v = -in[idx];
                } else {
                    v = in[idx];
                }
            }
            xs[row][bl] = v;
        }
        __syncthreads();
        if (!wact) continue;
        const int kc = min(DST_XK, (g.n - b0 + 3) & ~3);
        for (int s = 0; s < kc; s += 4) {
            const int kk = s + (lane >> 4);
            const double a_lo = xs[lane & 15][kk];
            const double a_hi = xs[16 + (lane & 15)][kk];
            const double* srow = S + (size_t)(b0 + kk) * g.np + a0w + (lane & 15);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const double bv = srow[16 * ni];
                acc[0][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_lo, bv, acc[0][ni], 0, 0, 0);
                acc[1][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_hi, bv, acc[1][ni], 0, 0, 0);
            }
        }
    }
    if (!wact) return;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jj = j0 + mi * 16 + (lane >> 4) + 4 * r;
            if (jj >= g.nj) continue;
            const long long rowi = plane + (long long)(jj + 1) * g.px + 1;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int a = a0w + 16 * ni + (lane & 15);
                if (a < g.n) out[rowi + a] = acc[mi][ni][r];
            }
        }
    }
}

}  // namespace cfdhip

// the kind of a direct transform method (hip_poisson_method_t), -1 for any other
static int transform_kind(int method) {
    return method == HIP_POISSON_DST ? TR_SINE : method == HIP_POISSON_DCT ? TR_COSINE : -1;
}

// The cached device tables of one kind and axis length. The entry is pushed
// with n = -1, which no lookup matches, so the context owns its allocations
// from the start (free_ctx) and a failed allocation or copy leaves nothing
// that a later solve could find; n is set once the entry is complete.
static cfd_status_t transform_table(hip_proj_ctx* c, int kind, int n,
                                    const TransformTable** out) {
    for (const TransformTable& t : c->tr_tabs)
        if (t.kind == kind && t.n == n) {
            *out = &t;
            return CFD_SUCCESS;
        }
    const bool cosine = (kind == TR_COSINE);
    const size_t np = dst_table_pitch((size_t)n), bytes = np * np * sizeof(double);
    std::vector<double> hf(np * np), hi(cosine ? np * np : 0), he((size_t)n);
    if (cosine) {
        dct_fill_cos_tables((size_t)n, hi.data(), hf.data());
        dct_fill_eigenvalues((size_t)n, he.data());
    } else {
        dst_fill_sine_table((size_t)n, hf.data());
        dst_fill_eigenvalues((size_t)n, he.data());
    }
    c->tr_tabs.push_back(TransformTable{kind, -1, (int)np, nullptr, nullptr, nullptr});
    TransformTable& t = c->tr_tabs.back();
    HIP_TRY(hipMalloc((void**)&t.fwd, bytes));
    if (cosine) HIP_TRY(hipMalloc((void**)&t.inv, bytes));
    else t.inv = t.fwd;  // S is symmetric: one allocation
    HIP_TRY(hipMalloc((void**)&t.e, he.size() * sizeof(double)));
    // pageable sources: synchronous copies (ordered before later stream work)
    HIP_TRY(hipMemcpy(t.fwd, hf.data(), bytes, hipMemcpyHostToDevice));
    if (cosine) HIP_TRY(hipMemcpy(t.inv, hi.data(), bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.e, he.data(), he.size() * sizeof(double), hipMemcpyHostToDevice));
    t.n = n;
    *out = &t;
    return CFD_SUCCESS;
}

// the tables of the context's axes x, y, z (z: nullptr in 2-D)
struct TransformTabs {
    const TransformTable* t[3];
};

// two rounds: the vector may grow while the tables are built in the first,
// so the pointers are those of the second
static cfd_status_t tables_of(hip_proj_ctx* c, int kind, TransformTabs* T) {
    const int n[3] = {(int)c->nx - 2, (int)c->ny - 2, c->nz > 1 ? (int)c->nz - 2 : 0};
    for (int round = 0; round < 2; ++round)
        for (int a = 0; a < 3; ++a) {
            T->t[a] = nullptr;
            if (n[a] > 0) ST_TRY(transform_table(c, kind, n[a], &T->t[a]));
        }
    return CFD_SUCCESS;
}

// The launch geometry of the x pass (table pitch np) and of a strided pass
// along axis 1 (y) or 2 (z) with n points
static DstRows dst_rows_geo(const hip_proj_ctx* c, int np) {
    const bool is3d = c->nz > 1;
    DstRows g;
    g.n = (int)c->nx - 2;
    g.nj = (int)c->ny - 2;
    g.nk = is3d ? (int)c->nz - 2 : 1;
    g.k0 = is3d ? 1 : 0;
    g.px = c->px;
    g.ps = c->ps;
    g.np = np;
    g.tiles_j = (g.nj + DST_XR - 1) / DST_XR;
    g.tiles_a = (g.n + 255) / 256;
    return g;
}

static DstAxis dst_axis_geo(const hip_proj_ctx* c, int axis, int n, int np) {
    const bool is3d = c->nz > 1;
    DstAxis g;
    g.n = n;
    g.nc = (int)c->nx - 2;
    g.np = np;
    if (axis == 1) {
        g.nb = is3d ? (int)c->nz - 2 : 1;
        g.sa = c->px;
        g.sb = c->ps;
        g.off0 = (long long)(is3d ? 1 : 0) * c->ps + c->px + 1;
    } else {
        g.nb = (int)c->ny - 2;
        g.sa = c->ps;
        g.sb = c->px;
        g.off0 = c->ps + c->px + 1;
    }
    g.tiles_a = g.np / DST_TA;
    g.tiles_c = (g.nc + 63) / 64;
    return g;
}

// One pass of the interior along `axis` (0 x, 1 y, 2 z): in -> out (distinct
// fields). Sine: the unnormalised DST-I, its own inverse up to norm. Cosine:
// the orthonormal DCT-II, or with `inverse` its transpose, the DCT-III. sc
// (axes 1, 2): the eigenvalue scaling on the store, the kind's own. load (axis
// 0): the input as PassLoad says; LOAD_FORM_B takes the shell from xb and L.
enum PassLoad {
    LOAD_PLAIN,   // in
    LOAD_NEG,     // -in
    LOAD_FORM_B,  // b formed from in = rhs and the frozen shell of xb
};

static void transform_pass(hip_proj_ctx* c, const TransformTabs& T, int axis, bool inverse,
                           const double* in, double* out, const DstScale* sc = nullptr,
                           PassLoad load = LOAD_PLAIN, const double* xb = nullptr,
                           const Lap* L = nullptr) {
    const TransformTable* t = T.t[axis];
    const double* tab = inverse ? t->inv : t->fwd;
    if (axis == 0) {
        const DstRows g = dst_rows_geo(c, t->np);
        const dim3 grid((unsigned)(g.tiles_a * g.tiles_j * g.nk));
        if (load == LOAD_FORM_B)
            klaunch(c, k_dst_x<true>, grid, dim3(256), g, tab, in, xb, out, *L,
                    c->nz > 1 ? 1 : 0);
        else if (load == LOAD_NEG)
            klaunch(c, k_dst_x<false, true>, grid, dim3(256), g, tab, in, nullptr, out, Lap{}, 0);
        else
            klaunch(c, k_dst_x<false>, grid, dim3(256), g, tab, in, nullptr, out, Lap{}, 0);
        return;
    }
    const DstAxis g = dst_axis_geo(c, axis, t->n, t->np);
    const dim3 grid((unsigned)(g.tiles_c * g.tiles_a * g.nb));
    if (!sc)
        klaunch(c, k_dst_strided<false>, grid, dim3(256), g, tab, in, out, DstScale{});
    else if (t->kind == TR_COSINE)
        klaunch(c, k_dst_strided<true, true>, grid, dim3(256), g, tab, in, out, *sc);
    else
        klaunch(c, k_dst_strided<true>, grid, dim3(256), g, tab, in, out, *sc);
}

// ---------------------------------------------------------------------------
// The solve: x in c->pn, rhs in c->rhs. The transforms ping-pong between
// c->xt and the interior of c->pn (whose values are not needed once the first
// pass has read its input; its shell is written by the boundary condition
// only), so rhs stays intact for the final residual. max_iterations,
// check_interval and omega play no part.
// ---------------------------------------------------------------------------
static cfd_status_t transform_solve(hip_proj_ctx* c, int kind, double dx, double dy, double dz,
                                    double rel_tol, double abs_tol) {
    const bool is3d = c->nz > 1, sine = (kind == TR_SINE);
    const Lap L = make_lap(dx, dy, is3d ? dz : 0.0);
    const DirVals dv{};
    double* x = c->pn;
    ST_TRY(ensure_aux(c, true, true));
    TransformTabs T;
    ST_TRY(tables_of(c, kind, &T));
    for (hipEvent_t& e : c->tr_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(c->tr_ev[0], c->stream));
    // sine: poisson_solver_apply_bc(x) at solve start, as cg_solve: the
    // default Neumann shell, or the caller's boundary left as it is. cosine
    // (linear_solver.c:397-485): the residual of x as it stands
    const bool neumann = (c->poisson_bc == HIP_POISSON_BC_NEUMANN);
    if (sine && neumann) launch_bc(c, x, 0, dv);
    // the residual of x: sine, CG's || -rhs + lap(x) || from k_cg_setup with
    // x's boundary as it stands; cosine, the relaxation solvers' L-inf
    // residual (k_residual_linf). tol: the tolerance the residual sets
    auto residual = [&](double* res, double* tol = nullptr) -> cfd_status_t {
        if (!sine) {
            ST_TRY(relax_residual_linf(c, x, dx, dy, is3d ? dz : 0.0, res));
            if (tol) *tol = std::max(rel_tol * *res, abs_tol);
            return CFD_SUCCESS;
        }
        timed(c, HIP_KT_CG_SETUP, [&] {
            klaunch(c, k_cg_setup<false, false, true, false>, dim3(tile_grid(c)), dim3(NT),
                    c->geo, L, DivCoef{}, nullptr, nullptr, nullptr, c->rhs, x, c->r, c->st,
                    c->partials, c->counter, rel_tol, abs_tol, 1, 1, c->dsum, nullptr);
        });
        CgState s;
        ST_TRY(poll_final(c, c->st, &s));
        *res = s.res0;
        if (tol) *tol = s.tol;
        return CFD_SUCCESS;
    };
    double res0 = 0.0, tol = 0.0;
    ST_TRY(residual(&res0, &tol));
    c->pstats.initial_residual = res0;
    if (res0 < abs_tol) {  // linear_solver_cg.c:353-361: no end BC
        flush_timing(c);
        c->pstats.status = POISSON_CONVERGED;
        c->pstats.iterations = 0;
        c->pstats.final_residual = res0;
        c->pstats.elapsed_time_ms = 0.0;
        return CFD_SUCCESS;
    }
    DstScale sc{};
    sc.norm = 1.0;  // Q is orthonormal
    if (sine) {
        sc.norm = (2.0 / (double)(c->nx - 1)) * (2.0 / (double)(c->ny - 1));
        if (is3d) sc.norm *= 2.0 / (double)(c->nz - 1);
    }
    sc.ec = T.t[0]->e;
    sc.hc = L.dx2_inv;
    // the first pass forms b from rhs and the frozen shell of x (sine), or
    // takes -rhs (cosine)
    transform_pass(c, T, 0, false, c->rhs, c->xt, nullptr, sine ? LOAD_FORM_B : LOAD_NEG, x, &L);
    if (is3d) {
        sc.ea = T.t[2]->e, sc.ha = L.inv_dz2;
        sc.eb = T.t[1]->e, sc.hb = L.dy2_inv;
        transform_pass(c, T, 1, false, c->xt, x);
        transform_pass(c, T, 2, false, x, c->xt, &sc);
        transform_pass(c, T, 2, true, c->xt, x);
        transform_pass(c, T, 1, true, x, c->xt);
    } else {
        sc.ea = T.t[1]->e, sc.ha = L.dy2_inv;
        sc.eb = nullptr, sc.hb = 0.0;
        transform_pass(c, T, 1, false, c->xt, x, &sc);
        transform_pass(c, T, 1, true, x, c->xt);
    }
    transform_pass(c, T, 0, true, c->xt, x);
    double res = 0.0;
    if (sine) {
        // || b - A x || with the boundary still frozen, then CG's end BC
        ST_TRY(residual(&res));
        if (neumann) launch_bc(c, x, 0, dv);  // linear_solver_cg.c:447
    } else {
        launch_bc(c, x, 0, dv);  // the iterations' apply_bc
        ST_TRY(residual(&res));
    }
    HIP_TRY(hipEventRecord(c->tr_ev[1], c->stream));
    HIP_TRY(hipEventSynchronize(c->tr_ev[1]));
    flush_timing(c);
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->tr_ev[0], c->tr_ev[1]));
    const bool conv = (res < tol) || (res < abs_tol);
    c->pstats.status = conv ? POISSON_CONVERGED : POISSON_MAX_ITER;
    c->pstats.iterations = 1;
    c->pstats.final_residual = res;
    c->pstats.elapsed_time_ms = (double)ms;
    return conv ? CFD_SUCCESS : CFD_ERROR_MAX_ITER;
}
