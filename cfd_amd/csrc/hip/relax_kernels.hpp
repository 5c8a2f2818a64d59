// relax_kernels.hpp -- the relaxation kernels: the two-pass k_rb_pass /
// k_jacobi with k_residual_linf, the fused loop's k_rx* and the one-pass
// Red-Black SOR sweeps k_rb1 / k_rb1m with k_rb_edge_r. Included by
// relax_solve.hip only (through rb2.hpp, whose k_rb2 builds on k_rb1's
// helpers), so that its non-template kernels are emitted once.
#pragma once

#include "device_util.hpp"

namespace cfdhip {

// ---------------------------------------------------------------------------
// Relaxation solvers.
// Red-Black SOR colour pass (linear_solver_redblack.c:97-133). `parity` is the
// (i+j+k) parity updated in this pass: the reference's first ("red") pass
// updates odd cells, the second even cells. Each cell reads only the other
// colour, so the in-place update is race-free and bitwise the reference's.
// Jacobi (linear_solver_jacobi.c:92-109) reads xin, writes xout.
// ---------------------------------------------------------------------------
struct RelaxCoef {
    double dx2, dy2, inv_dz2, inv_factor, omega;
    double rdx2, rdy2;  // RN(1 / dx2), RN(1 / dy2) for divc
};

static __global__ __launch_bounds__(NT) void k_rb_pass(Geo g, RelaxCoef rc, double* __restrict__ x,
                                                const double* __restrict__ rhs, int parity) {
    const int ntiles = g.tiles_x * g.tiles_y * g.tiles_z;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        TileCoord c = tile_coord(g, t);
        if (!c.active) continue;
        long long idx = cidx(g, c.i, c.j, c.kb);
        for (int k = c.kb; k < c.ke; ++k, idx += g.ps) {
            if (((c.i + c.j + k + g.kofs) & 1) != parity) continue;  // global parity
            double pn = -(rhs[idx] - (x[idx + 1] + x[idx - 1]) / rc.dx2 -
                          (x[idx + g.px] + x[idx - g.px]) / rc.dy2 -
                          (x[idx + g.sz] + x[idx - g.sz]) * rc.inv_dz2) *
                        rc.inv_factor;
            double xo = x[idx];
            x[idx] = xo + rc.omega * (pn - xo);
        }
    }
}

static __global__ __launch_bounds__(NT) void k_jacobi(Geo g, RelaxCoef rc, const double* __restrict__ xin,
                                               double* __restrict__ xout,
                                               const double* __restrict__ rhs) {
    const int ntiles = g.tiles_x * g.tiles_y * g.tiles_z;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        TileCoord c = tile_coord(g, t);
        if (!c.active) continue;
        long long idx = cidx(g, c.i, c.j, c.kb);
        for (int k = c.kb; k < c.ke; ++k, idx += g.ps) {
            xout[idx] = -(rhs[idx] - (xin[idx + 1] + xin[idx - 1]) / rc.dx2 -
                          (xin[idx + g.px] + xin[idx - g.px]) / rc.dy2 -
                          (xin[idx + g.sz] + xin[idx - g.sz]) * rc.inv_dz2) *
                         rc.inv_factor;
        }
    }
}

// L-infinity residual |lap(x) - rhs| (linear_solver.c:304-346, division form).
struct ResCoef {
    double dx2, dy2, inv_dz2;
};

static __global__ __launch_bounds__(NT) void k_residual_linf(Geo g, ResCoef rc,
                                                      const double* __restrict__ x,
                                                      const double* __restrict__ rhs,
                                                      unsigned long long* out) {
    __shared__ double sh[NWAVE];
    double m = 0.0;
    const int ntiles = g.tiles_x * g.tiles_y * g.tiles_z;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        TileCoord c = tile_coord(g, t);
        if (!c.active) continue;
        long long idx = cidx(g, c.i, c.j, c.kb);
        for (int k = c.kb; k < c.ke; ++k, idx += g.ps) {
            double lap = (x[idx + 1] - 2.0 * x[idx] + x[idx - 1]) / rc.dx2 +
                         (x[idx + g.px] - 2.0 * x[idx] + x[idx - g.px]) / rc.dy2 +
                         (x[idx + g.sz] + x[idx - g.sz] - 2.0 * x[idx]) * rc.inv_dz2;
            double res = fabs(lap - rhs[idx]);
            if (res > m) m = res;
        }
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = sh[0];
        for (int w = 1; w < NWAVE; ++w) a = fmax(a, sh[w]);
        atomicMax(out, ord_enc(a));
    }
}

// ---------------------------------------------------------------------------
// Relaxation iterations on the row-pair sweep tiling (single device), with
// the common loop's convergence test (linear_solver.c:397-485) on the device.
// Ping-pong buffers: iteration it reads X = buf[it & 1] (the iterate after
// it - 1 iterations, BCs applied) and leaves buf[(it + 1) & 1].
//   RB-SOR:  k_rx<RX_RED>   X -> Y: first-colour ((i+j+k) odd, the CPU
//                           reference's "red", linear_solver_redblack.c:97-114)
//                           cells SOR-updated, the other cells copied; and the
//                           L-inf residual of X;
//            k_rx_shell     boundary shell X -> Y (the sweeps read it);
//            k_rx<RX_BLACK> Y in place: second-colour cells (:116-133);
//            k_rx_shell     Neumann BC on Y (poisson_solver_apply_bc).
//   Jacobi:  k_rx<RX_JACOBI> X -> Y (linear_solver_jacobi.c:92-109) + the
//            residual of X; k_rx_shell Neumann on Y.
// The residual of the iterate after iteration it - 1 is thus computed by the
// first sweep of iteration it, which has to read X anyway (16 B/cell of the
// reference's separate residual pass saved); when it shows convergence the
// result is X, still intact in its buffer, and everything launched after it
// returns at once (RxState.done). Per-cell arithmetic is the reference's, and
// L-inf (a max) is order-independent, so iterates, residuals and iteration
// counts are bitwise the reference's.
// ---------------------------------------------------------------------------
constexpr int RX_RED = 0;
constexpr int RX_BLACK = 1;
constexpr int RX_JACOBI = 2;

// m = L-inf residual of the iterate after it - 1 iterations (it = 0: x0)
__device__ __forceinline__ void rx_finish(RxState* st, double m, int it) {
    if (it == 0) {  // linear_solver.c:415-437
        st->res0 = m;
        st->res = m;
        double tol = st->rel_tol * m;
        if (tol < st->abs_tol) tol = st->abs_tol;
        st->tol = tol;
        if (m < st->abs_tol) {
            st->done = 1;
            st->status = ST_CONVERGED;
            st->iterations = 0;
            st->result = 0;
            st->res_it = 0;
        }
        return;
    }
    const int prev = it - 1;  // :443-468, iteration prev just completed
    if (prev % st->check_interval == 0) {
        st->res = m;
        if (m < st->tol || m < st->abs_tol) {
            st->done = 1;
            st->status = ST_CONVERGED;
            st->iterations = it;  // iter + 1 at the break
            st->result = it & 1;
            st->res_it = it;
            return;
        }
    }
    if (it >= st->max_iter) {  // loop ran out: iterations = iter + 1 = max_iter + 1 (:472)
        st->done = 1;
        st->status = ST_MAX_ITER;
        st->iterations = st->max_iter + 1;
        st->result = it & 1;
        st->res_it = it;
    }
}

static __global__ void k_rx_init(RxState* st, double rel_tol, double abs_tol, int max_iter,
                                 int check_interval) {
    if (threadIdx.x == 0) {
        st->tol = 0.0;
        st->abs_tol = abs_tol;
        st->rel_tol = rel_tol;
        st->res0 = st->res = 0.0;
        st->iterations = 0;
        st->done = 0;
        st->status = ST_MAX_ITER;
        st->max_iter = max_iter;
        st->check_interval = check_interval;
        st->result = 0;
        st->res_it = 0;
        st->res_exact = 1;
        st->ovr_it = -1;
        st->pad0 = 0;
        st->ovr_m = 0.0;
        st->bmax = 0.0;
    }
}

// Boundary shell of an iteration: mode 0 copies src -> dst, mode 1 applies
// the Neumann gathers to dst.
static __global__ __launch_bounds__(256) void k_rx_shell(Geo g, const RxState* st,
                                                  const double* __restrict__ src,
                                                  double* __restrict__ dst, int mode) {
    if (st->done) return;
    const long long total = shell_total(g);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        int i, j, k;
        bool zlo, zhi;
        shell_cell(g, e, i, j, k, zlo, zhi);
        const long long d = cidx(g, i, j, k);
        if (mode == 0) {
            dst[d] = src[d];
        } else {
            const int sk = (zlo || zhi) ? bc_map(k, g.nz, 0) : k;
            dst[d] = dst[cidx(g, bc_map(i, g.nx, 0), bc_map(j, g.ny, 0), sk)];
        }
    }
}

// Z-slabs (DIST): the residual is an all-ranks max, through the device
// mailbox (mb) or, without one, left encoded in dred[0] for an RCCL max
// all-reduce + k_rx_finish.
template <int TY, int MODE, int FL, bool DIST = false>
static __global__ __launch_bounds__(64 * TY, sweep_min_waves<FL>()) void k_rx(
    SGeo g, RelaxCoef rc, const double* __restrict__ xin, double* __restrict__ xout,
    const double* __restrict__ rhs, RxState* st, double* partials, unsigned* counter, int it,
    Mbox* mb, unsigned long long* dred) {
    constexpr bool PF = (FL & SW_PREFETCH) != 0;
    constexpr bool RES = MODE != RX_BLACK;
    __shared__ double2 rows[2][TY + 2][64];
    __shared__ double sh[TY];
    __shared__ int flag;
    if (st->done) return;
    // stencil field: X (red / Jacobi) or Y in place (black)
    const double* xs = (MODE == RX_BLACK) ? xout : xin;
    RowPair c = row_pair<TY>(g);
    const bool halo = (c.w == 0) || (c.w == TY - 1);
    const int jh = (c.w == 0) ? max(c.j - 1, 0) : min(c.j + 1, g.ny - 1);
    const int hslot = (c.w == 0) ? 0 : TY + 1;
    const long long hoff = (long long)(jh - min(c.j, g.ny - 1)) * g.px;
    const bool xok = c.i0 < g.nx;
    const bool eok = (c.lane == 0 && c.i0 >= 1 && xok) || (c.lane == 63 && c.i0 + 2 < g.nx);
    const long long eoff = (c.lane == 0) ? -1 : 2;
    // parity (i+j+k) of the pair's first cell at local plane k is
    // (j + k + kofs) & 1 (i0 even); the first colour pass updates odd cells
    const int upd = (MODE == RX_RED) ? 1 : 0;
    const double2 zero = make_double2(0.0, 0.0);
    struct Bundle {
        double2 pp, hp, rr;  // X centre / y-halo of plane k+1; rhs of plane k
        double el;           // x-edge cell of plane k
    };
    auto issue = [&](int k, long long ix) __attribute__((always_inline)) {
        const double2 zero = make_double2(0.0, 0.0);
        Bundle b;
        const long long ip = ix + g.sz;
        b.pp = xok ? ld2(xs, ip) : zero;
        b.hp = (xok && halo && k + 1 < c.ke) ? ld2(xs, ip + hoff) : zero;
        b.rr = xok ? ld2v<FL>(rhs, ix) : zero;
        b.el = eok ? xs[ix + eoff] : 0.0;
        return b;
    };
    double m = 0.0;
    long long idx = c.idx;
    double2 pm = xok ? ld2(xs, idx - g.sz) : zero;
    double2 pc = xok ? ld2(xs, idx) : zero;
    double2 hc = (xok && halo) ? ld2(xs, idx + hoff) : zero;
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
        const double2 pp = cur.pp;
        double left = __shfl_up(pc.y, 1, 64);
        double right = __shfl_down(pc.x, 1, 64);
        if (c.lane == 0) left = cur.el;
        if (c.lane == 63) right = cur.el;
        // cell 0: (xm, xp) = (left, pc.y); cell 1: (pc.x, right)
        if (RES) {  // linear_solver.c:304-346 (k_residual_linf's expression)
            const double l0 = divc(pc.y - 2.0 * pc.x + left, rc.dx2, rc.rdx2) +
                              divc(yn.x - 2.0 * pc.x + ys.x, rc.dy2, rc.rdy2) +
                              (pp.x + pm.x - 2.0 * pc.x) * rc.inv_dz2;
            const double l1 = divc(right - 2.0 * pc.y + pc.x, rc.dx2, rc.rdx2) +
                              divc(yn.y - 2.0 * pc.y + ys.y, rc.dy2, rc.rdy2) +
                              (pp.y + pm.y - 2.0 * pc.y) * rc.inv_dz2;
            const double r0 = fabs(l0 - cur.rr.x), r1 = fabs(l1 - cur.rr.y);
            if (c.in0 && r0 > m) m = r0;
            if (c.in1 && r1 > m) m = r1;
        }
        double2 out = pc;
        if (MODE == RX_JACOBI) {
            const double pn0 = -(cur.rr.x - divc(pc.y + left, rc.dx2, rc.rdx2) -
                                 divc(yn.x + ys.x, rc.dy2, rc.rdy2) -
                                 (pp.x + pm.x) * rc.inv_dz2) *
                               rc.inv_factor;
            const double pn1 = -(cur.rr.y - divc(right + pc.x, rc.dx2, rc.rdx2) -
                                 divc(yn.y + ys.y, rc.dy2, rc.rdy2) -
                                 (pp.y + pm.y) * rc.inv_dz2) *
                               rc.inv_factor;
            if (c.in0) out.x = pn0;
            if (c.in1) out.y = pn1;
        } else {
            // one cell of the pair has this pass's colour: gather its stencil
            // (wave-uniform choice: the parity depends on j and k only)
            const bool first = ((c.j + k + g.kofs) & 1) == upd;  // global parity
            const double xc = first ? pc.x : pc.y;
            const double xl = first ? left : pc.x, xr = first ? pc.y : right;
            const double yl = first ? ys.x : ys.y, yr = first ? yn.x : yn.y;
            const double zl = first ? pm.x : pm.y, zr = first ? pp.x : pp.y;
            const double rh = first ? cur.rr.x : cur.rr.y;
            const double pn = -(rh - divc(xr + xl, rc.dx2, rc.rdx2) -
                                divc(yr + yl, rc.dy2, rc.rdy2) - (zr + zl) * rc.inv_dz2) *
                              rc.inv_factor;
            const double xn = xc + rc.omega * (pn - xc);
            if (first) {
                if (c.in0) out.x = xn;
            } else if (c.in1) {
                out.y = xn;
            }
        }
        if (c.act) st2v<FL>(xout, idx, out);
        pm = pc;
        pc = pp;
        hc = cur.hp;
        if (PF) cur = nxt;
        buf ^= 1;
    }
    if (!RES) return;
    m = wave_max(m);
    if (c.lane == 0) sh[c.w] = m;
    __syncthreads();
    double* shs = (double*)&rows[0][0][0];
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int q = 0; q < TY; ++q) a = fmax(a, sh[q]);
        store_sc1(&partials[blockIdx.x], a);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned t = __hip_atomic_fetch_add((gu32*)counter, 1u, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        flag = (t == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (flag == 0) return;
    double a = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += 64 * TY) a = fmax(a, load_sc1(&partials[b]));
    a = wave_max(a);
    if (c.lane == 0) shs[c.w] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int q = 0; q < TY; ++q) tot = fmax(tot, shs[q]);
        __hip_atomic_store((gu32*)counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!DIST) {
            rx_finish(st, tot, it);
        } else if (mb) {
            double gm;
            if (mbox_allreduce(mb, tot, &gm, true)) {
                rx_finish(st, gm, it);
            } else {
                st->done = 1;
                st->status = ST_COMM_TIMEOUT;
            }
        } else {
            dred[0] = ord_enc(tot);
        }
    }
}

__device__ __forceinline__ double ord_dec_dev(unsigned long long e) {
    const unsigned long long b =
        (e & 0x8000000000000000ull) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e;
    return __longlong_as_double((long long)b);
}

// after the RCCL max all-reduce of dred (Z-slabs without a device mailbox)
static __global__ void k_rx_finish(RxState* st, const unsigned long long* gred, int it) {
    if (threadIdx.x == 0 && !st->done) rx_finish(st, ord_dec_dev(gred[0]), it);
}

// ---------------------------------------------------------------------------
// Single-pass Red-Black SOR iteration (3-D, single device): X -> Y in one
// z-march. For plane q the tile forms R_q = X_q with its first-colour ("red",
// (i+j+k) odd) interior cells SOR-updated (linear_solver_redblack.c:97-114);
// then the second colour of plane q-1 is updated from R (:116-133), and the
// L-inf residual of X at plane q (linear_solver.c:304-346) rides along. R at
// a tile's y/x halo is recomputed locally (overlapped tiles: 128 x 16 cells
// loaded per plane, 124 x 12 written), so each cell of X and rhs is read
// once from HBM and Y written once: 24 B/cell per iteration instead of the
// two colour passes' 48. R values are computed from the same X values by the
// same expression as the first pass would, so Y is bitwise the two-pass
// result.
// ---------------------------------------------------------------------------

// One SOR update of a cell (linear_solver_redblack.c:103-112 operation order).
template <class Dv>
__device__ __forceinline__ double sor1(const RelaxCoef& rc, Dv dv, double vc, double vl, double vr,
                                       double vs, double vn, double vm, double vp, double vb) {
    const double pn = -(vb - dv(vr + vl, rc.dx2, rc.rdx2) - dv(vn + vs, rc.dy2, rc.rdy2) -
                        (vp + vm) * rc.inv_dz2) *
                      rc.inv_factor;
    return vc + rc.omega * (pn - vc);
}

// |lap(x) - rhs| of one cell (linear_solver.c:304-346, the division form).
template <class Dv>
__device__ __forceinline__ double res1(const RelaxCoef& rc, Dv dv, double c, double xl, double xr,
                                       double ys, double yn, double zm, double zp, double b) {
    const double l = dv(xr - 2.0 * c + xl, rc.dx2, rc.rdx2) +
                     dv(yn - 2.0 * c + ys, rc.dy2, rc.rdy2) + (zp + zm - 2.0 * c) * rc.inv_dz2;
    return fabs(l - b);
}

// Tile shapes (r02b). A workgroup is 16 waves; lane l of wave w owns the x
// pair c = l % TC of tile row r = w + 16 (l / TC), so a tile is TC pairs (2 TC
// columns) by TR = 1024 / TC rows. Rows w and w + 16 h have the same parity,
// so the colour pattern of a step stays wave-uniform for every TC. R is
// recomputed on the tile's one-cell halo: 2 TC - 4 columns and TR - 4 rows are
// written per tile. TC = 64 (16 rows) loads 1.38x the cells it writes, TC = 32
// (32 rows) 1.22x, and the narrower tiles also waste less on the last x tile
// (512: 5 x 124 columns for 510 vs 9 x 60).
template <int TC>
constexpr int rb1_rows() { return 1024 / TC; }
template <int TC>
constexpr int rb1_ox() { return 2 * TC - 4; }  // output columns per tile
template <int TC>
constexpr int rb1_oy() { return 1024 / TC - 4; }  // output rows per tile

// Issue-model details (r02; profiles/r02_rb_variants.jsonl, r02_pmc_rb.jsonl):
//  - the colour pattern of a step is wave-uniform ((j + q) parity): the z
//    loop is unrolled by two planes and each step is compiled for its
//    pattern, so no per-lane selects pick the updated cell of a pair
//    (VALU instructions per launch 321 M -> 196 M at 512^3);
//  - x neighbours come from the row the wave already published in LDS (one
//    ds_read_b64 each side) instead of two ds_bpermute per double, and every
//    LDS operand of a step is read right after its barrier (one LDS round
//    trip per step);
//  - rhs is not loaded on the two halo rows, which never use it.
// PF = the register-ring prefetch below (r02: 0.90 -> 0.76 ms per iteration at
// 512^3 on one box, 128 VGPRs); the product instantiates PF = true.
// DIST (Z-slabs): R on a halo plane that has a neighbour (rh_lo: plane k0 - 1,
// rh_hi: plane k1) is the neighbour's R of its edge plane, exchanged into RH
// beforehand (k_rb_edge_r + halo); it cannot be formed here, since that needs
// X two planes beyond the halo. The L-inf residual leaves as in k_rx: the
// device mailbox's max, or dred for an RCCL max all-reduce + k_rx_finish.
// LDS of one k_rb1 workgroup: X and R rows of two plane parities (the same
// 64 KB for every tile width), the waves' residual maxima and the
// last-workgroup flag.
struct Rb1Lds {
    double xb[2 * 1024 * 2];
    double rb[2 * 1024 * 2];
    double sh[16];
    int flag;
};

// The body of k_rb1 for the tile width TC; bid = this workgroup's tile-block
// index within its geometry g (k_rb1m runs two geometries in one grid).
template <int FL, int TC, bool PF, bool DIST, bool REV = false>
__device__ __forceinline__ void rb1_body(
    Rb1Lds& L, int bid, SGeo g, RelaxCoef rc, const double* __restrict__ X,
    double* __restrict__ Y, const double* __restrict__ rhs, RxState* st, double* partials,
    unsigned* counter, int it, const double* __restrict__ RH, int rh_lo, int rh_hi, Mbox* mb,
    unsigned long long* dred, int neu) {
    constexpr int NW = 16;  // waves
    constexpr int TR = rb1_rows<TC>();
    constexpr int OX = rb1_ox<TC>(), OY = rb1_oy<TC>();
    // X and R rows by plane parity; a row is stored as its TC .x cells, then
    // its TC .y cells, so a pair is one ds_read2/ds_write2_b64 and an x
    // neighbour (one double of the adjacent lane) a conflict-free ds_read_b64
    // (with double2 rows those 8-B reads at a 16-B lane stride conflicted)
    auto& xb = *reinterpret_cast<double(*)[2][TR][2][TC]>(L.xb);
    auto& rb = *reinterpret_cast<double(*)[2][TR][2][TC]>(L.rb);
    auto& sh = L.sh;
    auto& flag = L.flag;
    // every LDS read stays a ds_read_b64 (2 LDS cycles per wave; a pair
    // merged into ds_read2_b64 takes 8): a scheduling barrier that lets every
    // instruction class cross it ends the pairing pass's search window
    auto lrd = [&](const double& v) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0x7ff);
        return v;
    };
    auto lget = [&](double (&a)[2][TR][2][TC], int p, int r, int l) __attribute__((always_inline)) {
        const double x = lrd(a[p][r][0][l]);
        return make_double2(x, lrd(a[p][r][1][l]));
    };
    auto lput = [&](double (&a)[2][TR][2][TC], int p, int r, int l, double2 v)
                    __attribute__((always_inline)) {
        a[p][r][0][l] = v.x;
        a[p][r][1][l] = v.y;
    };
    if (st->done) return;
    // tile = block index: round-robin dispatch spreads consecutive tiles over
    // the eight XCDs (r03: faster here than xcd_tile's contiguous ranges,
    // 2.86-2.87 -> 2.82-2.83 ms per iteration at 1024^2 x 512, equal at 512^3,
    // profiles/r03_tile_order.jsonl)
    const int t = bid;
    const int tx = t % g.tiles_x;
    const int rest = t / g.tiles_x;
    const int ty = rest % g.tiles_y;
    const int tz = rest / g.tiles_y;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane % TC;                     // pair within the row
    const int r = w + NW * (lane / TC);          // tile row
    const int cm = max(c - 1, 0), cp = min(c + 1, TC - 1);  // x neighbours' pairs
    const int rlo = max(r - 1, 0), rhi = min(r + 1, TR - 1);  // y neighbours' rows
    const int i0 = g.xofs + tx * OX - 2 + 2 * c;  // even; the pair is (i0, i0 + 1)
    const int j = ty * OY - 2 + r;       // grid row
    // kmode 1: the slab's two edge planes (tz 0 -> k0, tz 1 -> k1 - 1);
    // kmode 2: the planes [kt0, kt1); else [k0, k1). A march over a plane
    // range still forms R on its two lower neighbour planes (prologue), so
    // the ranges of one iteration's launches give the one-launch Y.
    int kb, ke;
    if (g.kmode == 1) {
        kb = (tz == 0) ? g.k0 : g.k1 - 1;
        ke = kb + 1;
    } else {
        const int kt0 = (g.kmode == 2) ? g.kt0 : g.k0;
        const int kt1 = (g.kmode == 2) ? g.kt1 : g.k1;
        kb = kt0 + tz * g.kc;
        ke = min(kb + g.kc, kt1);
    }
    const bool xin = (i0 >= 0 && i0 < g.nx);
    const bool ld = xin && j >= 0 && j < g.ny;
    const bool jin = (j >= 1 && j <= g.ny - 2);
    const bool in0 = jin && i0 >= 1 && i0 <= g.nx - 2;
    const bool in1 = jin && i0 + 1 <= g.nx - 2;
    const bool orow = (r >= 2 && r < 2 + OY);
    const bool own = orow && c >= 1 && c <= TC - 2;
    // wave-uniform skips: with TC = 64 a wave is one row, so its halo rows
    // (no R work: rows 0, 15; no output: rows 0, 1, 14, 15) skip whole
    // phases; narrower tiles mix rows in a wave and mask per lane instead
    const bool wr = (TC == 64) ? (r >= 1 && r <= TR - 2) : true;
    const bool wo = (TC == 64) ? orow : true;
    const long long col = (long long)max(min(j, g.ny - 1), 0) * g.px + max(i0, 0);
    // the folded Neumann shell (neu): this lane's x-face roles and whether it
    // stores (pairs (nx-1, pad) of odd nx leave cell nx-1 to role 4)
    const int nrole = (i0 == 0 ? 1 : 0) | (i0 + 1 == g.nx - 1 ? 2 : 0) |
                      (i0 + 1 == g.nx - 2 ? 4 : 0) |
                      ((own && jin && i0 <= g.nx - 2) ? 8 : 0);
    // Loads are issued unconditionally from clamped (always valid) addresses
    // and never masked: with the same loads on every control path and no
    // select right behind them, the compiler's vmcnt counting waits for a
    // plane only where a step consumes it (a load some path skips, or a
    // select on the loaded value, forces vmcnt(0) right after the prefetch of
    // the next plane, i.e. a full memory latency per step). Positions outside
    // the grid (ld false, k out of range) then hold other cells' values; they
    // only ever feed boundary cells, which are not updated, and halo lanes,
    // which are not stored or reduced. The halo rows 0 and TR - 1 (no R work)
    // load the adjacent row's rhs, which that row's lanes load too (an L2 hit).
    const int ic = (i0 < g.nx) ? max(i0, 0) : g.nx - 2 - ((g.nx - 2) & 1);
    const int jr = j + (r == 0 ? 1 : (r == TR - 1 ? -1 : 0));
    const long long colx = (long long)max(min(j, g.ny - 1), 0) * g.px + ic;
    const long long colr = (long long)max(min(jr, g.ny - 1), 0) * g.px + ic;
    auto ldx = [&](int k) -> double2 {
        return ld2(X, (long long)min(max(k, 0), g.nz - 1) * g.ps + colx);
    };
    auto ldr = [&](int k) -> double2 {
        return ld2v<FL>(rhs, (long long)min(max(k, 0), g.nz - 1) * g.ps + colr);
    };
    const double2 zero = make_double2(0.0, 0.0);
    // Step q forms R_{q+1} and updates the second colour of plane q.
    // Per lane: X_q, X_{q+1}, X_{q+2} (xm, xc, xp); R_{q-1}, R_q (rmm, rm);
    // rhs_{q+1} (bq). Of rhs_q and R_{q-1} only the component of the cell
    // this step's second-colour update touches is kept (bmh, rmmh): the
    // pattern alternates per plane, so the end of step q keeps the component
    // step q + 1 will use. LDS at the top of step q: X_{q+1} rows in
    // xb[(q+1)&1], R_q rows in rb[q&1].
    // PF (register ring): the X planes sit in a ring of four register slots
    // and rhs in a ring of two, indexed by the step's phase P = (q - q0) mod 4
    // at compile time (the z loop is unrolled by four), and step q issues the
    // loads of X_{q+3} and rhs_{q+2} into the free slots before its barrier:
    // a full step of latency hiding, and no register copy of a loaded value
    // (a copy would wait for the load). Without PF the loads are issued at
    // the end of step q and the three X planes shift through xm, xc, xp.
    // REV (r03, one device): the march runs z downwards, D = -1: step q forms
    // R_{q-1} and updates plane q, "ahead" is q - 1. Every cell's operands
    // keep their z roles (z- / z+ are picked by direction), R depends on X
    // only and the second colour on R only, and the residual is a max, so Y
    // and the iteration's decision are bitwise the upward march's. The host
    // alternates the direction per iteration, so each sweep starts on the
    // planes the previous one wrote last (in the Infinity Cache).
    constexpr int D = REV ? -1 : 1;
    const int q0 = REV ? ke + 1 : kb - 2;  // the first step
    double2 xr[4], br[2], rm;
    double bmh, rmmh;
    xr[0] = ldx(q0);
    xr[1] = ldx(q0 + D);
    xr[2] = ldx(q0 + 2 * D);
    xr[3] = zero;
    br[0] = ldr(q0 + D);
    br[1] = zero;
    rm = zero;
    bmh = rmmh = 0.0;
    lput(xb, (q0 + D) & 1, r, c, xr[1]);
    double m = 0.0;
    // E: cell i0 of the pair is the cell both updates of this step touch (the
    // first colour, (i+j+k) odd, of plane q+1 and the second of plane q)
    auto step = [&](auto Ec, auto Pc, int q) __attribute__((always_inline)) {
        constexpr bool E = decltype(Ec)::value;
        constexpr int P = PF ? decltype(Pc)::value : 0;  // ring phase
        constexpr int IM = P & 3, IC = (P + 1) & 3, IP = (P + 2) & 3, IN = (P + 3) & 3;
        constexpr int BQ = P & 1, BN = (P + 1) & 1;
        if constexpr (PF) {
            xr[IN] = ldx(q + 3 * D);
            br[BN] = ldr(q + 2 * D);
        }
        // behind / centre / ahead of plane qa, then its z- / z+ neighbours
        const double2 xbh = xr[IM], xc = xr[IC], xah = xr[IP], bq = br[BQ];
        const double2 xm = REV ? xah : xbh, xp = REV ? xbh : xah;
        __syncthreads();
        const int qa = q + D;
        const bool qin = (qa >= g.k0 && qa < g.k1);
        const bool rin = qin && qa >= kb && qa < ke;
        // the output's LDS operands (R_q rows) are read up front, so one LDS
        // round trip after the barrier serves both halves of the step
        const double2 rys = lget(rb, q & 1, rlo, c);
        const double2 ryn = lget(rb, q & 1, rhi, c);
        const double rlr = lrd(E ? rb[q & 1][r][1][cm] : rb[q & 1][r][0][cp]);
        double2 R = xc;
        if constexpr (DIST) {
            if ((qa == g.k0 - 1 && rh_lo) || (qa == g.k1 && rh_hi))
                R = ld2(RH, (long long)qa * g.ps + colx);
        }
        const double2 ys = lget(xb, qa & 1, rlo, c);
        const double2 yn = lget(xb, qa & 1, rhi, c);
        const double left = lrd(xb[qa & 1][r][1][cm]);
        const double right = lrd(xb[qa & 1][r][0][cp]);
        if (wr && qin) {
            if (E) {
                const double v = sor1(rc, DivC{}, xc.x, left, xc.y, ys.x, yn.x, xm.x, xp.x, bq.x);
                if (in0) R.x = v;
            } else {
                const double v = sor1(rc, DivC{}, xc.y, xc.x, right, ys.y, yn.y, xm.y, xp.y, bq.y);
                if (in1) R.y = v;
            }
            if (wo && rin) {
                const double a0 = res1(rc, DivC{}, xc.x, left, xc.y, ys.x, yn.x, xm.x, xp.x, bq.x);
                const double a1 = res1(rc, DivC{}, xc.y, xc.x, right, ys.y, yn.y, xm.y, xp.y, bq.y);
                if (own && in0 && a0 > m) m = a0;
                if (own && in1 && a1 > m) m = a1;
            }
        }
        // ---- second colour of plane q from R_{q-1}, R_q, R_{q+1} ----
        // (rmmh: R behind, R: R ahead; REV swaps their z roles)
        if ((REV ? q < ke : q >= kb) && wo) {
            double2 out = rm;
            if (E) {
                const double rzm = REV ? R.x : rmmh, rzp = REV ? rmmh : R.x;
                const double v = sor1(rc, DivC{}, rm.x, rlr, rm.y, rys.x, ryn.x, rzm, rzp, bmh);
                if (own && in0) out.x = v;
            } else {
                const double rzm = REV ? R.y : rmmh, rzp = REV ? rmmh : R.y;
                const double v = sor1(rc, DivC{}, rm.y, rm.x, rlr, rys.y, ryn.y, rzm, rzp, bmh);
                if (own && in1) out.y = v;
            }
            if (neu) {
                // the iteration's Neumann BC (linear_solver_redblack.c:139) folded
                // into the stores: every boundary cell of Y is the gather
                // k_bc_shell / k_rx_shell mode 1 makes, Y at the clamped-inward
                // position (bc_map), so the writer of that source cell stores
                // it to its mirror positions too: x faces within the pair (or
                // one 8-B store when nx is odd), y faces as a copy of rows 1 /
                // ny-2, z faces (global, not a slab's halo) as copies of
                // planes k0 / k1-1
                // nrole (lane constant): 1 = pair (0, 1), 2 = pair (nx-2, nx-1),
                // 4 = nx odd and .y is cell nx-2 (cell nx-1 <- .y), 8 = store
                if (nrole & 1) out.x = out.y;
                if (nrole & 2) out.y = out.x;
                if (nrole & 8) {
                    // j is wave-uniform with TC = 64 (one row per wave), so
                    // are q and the z-face tests: scalar branches
                    auto put = [&](long long base) __attribute__((always_inline)) {
                        st2v<FL>(Y, base, out);
                        if (nrole & 4) Y[base + 2] = out.y;
                        if (j == 1 || j == g.ny - 2) {
                            const long long b2 = base + (j == 1 ? -g.px : g.px);
                            st2v<FL>(Y, b2, out);
                            if (nrole & 4) Y[b2 + 2] = out.y;
                        }
                    };
                    const long long base = (long long)q * g.ps + col;
                    put(base);
                    if (q == g.k0 && !rh_lo) put(base - g.ps);
                    if (q == g.k1 - 1 && !rh_hi) put(base + g.ps);
                }
            } else if (own && ld && jin) {
                st2v<FL>(Y, (long long)q * g.ps + col, out);
            }
        }
        // step q + D updates the .x cell iff this step did not
        rmmh = E ? rm.y : rm.x;
        rm = R;
        bmh = E ? bq.y : bq.x;
        if constexpr (!PF) {
            xr[0] = xc;
            xr[1] = xah;
            xr[2] = ldx(q + 3 * D);
            br[0] = ldr(q + 2 * D);
        }
        // publish X_{q+2} and R_{q+1} for step q + 1 (their buffers were last
        // read in step q - 1, before this step's barrier)
        lput(xb, (q + 2 * D) & 1, r, c, xah);
        lput(rb, (q + D) & 1, r, c, rm);
    };
    // E(q) for the lane's row: ((j + q + kofs) & 1) == 0; E(kb - 2) == E(kb);
    // rows r and r + 16 h share the parity, so E is wave-uniform
    const bool E0 = __builtin_amdgcn_readfirstlane(((j + q0 + g.kofs) & 1) == 0 ? 1 : 0) != 0;
    // steps q0, q0 + D, ...: ke - kb + 2 of them (R is formed one plane ahead)
    const int nsteps = ke - kb + 2;
    int n = 0;
    auto march = [&](auto E0c) __attribute__((always_inline)) {
        constexpr bool A = decltype(E0c)::value;
        using TA = BoolC<A>;
        using TB = BoolC<!A>;
        if constexpr (PF) {
            for (; n + 3 < nsteps; n += 4) {
                step(TA{}, IntC<0>{}, q0 + D * n);
                step(TB{}, IntC<1>{}, q0 + D * (n + 1));
                step(TA{}, IntC<2>{}, q0 + D * (n + 2));
                step(TB{}, IntC<3>{}, q0 + D * (n + 3));
            }
            if (n < nsteps) step(TA{}, IntC<0>{}, q0 + D * n);
            if (n + 1 < nsteps) step(TB{}, IntC<1>{}, q0 + D * (n + 1));
            if (n + 2 < nsteps) step(TA{}, IntC<2>{}, q0 + D * (n + 2));
        } else {
            for (; n + 1 < nsteps; n += 2) {
                step(TA{}, IntC<0>{}, q0 + D * n);
                step(TB{}, IntC<0>{}, q0 + D * (n + 1));
            }
            if (n < nsteps) step(TA{}, IntC<0>{}, q0 + D * n);
        }
    };
    if (E0) march(BoolC<true>{});
    else march(BoolC<false>{});
    m = wave_max(m);
    if (lane == 0) sh[w] = m;
    __syncthreads();
    double* shs = &xb[0][0][0][0];
    // an iteration split over several launches (slabs: kmode 1 / 2) shares
    // one partials array: this launch owns [part_ofs, part_ofs + gridDim.x)
    // of part_total, and the last of all part_total workgroups (the last
    // launch on the stream) finishes the max
    const unsigned ptot = g.part_total ? (unsigned)g.part_total : gridDim.x;
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int v = 0; v < NW; ++v) a = fmax(a, sh[v]);
        store_sc1(&partials[g.part_ofs + blockIdx.x], a);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned tk = __hip_atomic_fetch_add((gu32*)counter, 1u, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        flag = (tk == ptot - 1) ? 1 : 0;
    }
    __syncthreads();
    if (flag == 0) return;
    double a = 0.0;
    for (unsigned b = threadIdx.x; b < ptot; b += 1024) a = fmax(a, load_sc1(&partials[b]));
    a = wave_max(a);
    if (lane == 0) shs[w] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int v = 0; v < NW; ++v) tot = fmax(tot, shs[v]);
        __hip_atomic_store((gu32*)counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!DIST) {
            rx_finish(st, tot, it);
        } else if (mb) {
            double gm;
            if (mbox_allreduce(mb, tot, &gm, true)) {
                rx_finish(st, gm, it);
            } else {
                st->done = 1;
                st->status = ST_COMM_TIMEOUT;
            }
        } else {
            dred[0] = ord_enc(tot);
        }
    }
}

template <int FL, int TC, bool PF, bool DIST = false, bool REV = false>
static __global__ __launch_bounds__(1024, 4) void k_rb1(
    SGeo g, RelaxCoef rc, const double* __restrict__ X, double* __restrict__ Y,
    const double* __restrict__ rhs, RxState* st, double* partials, unsigned* counter, int it,
    const double* __restrict__ RH, int rh_lo, int rh_hi, Mbox* mb, unsigned long long* dred,
    int neu) {
    __shared__ Rb1Lds L;
    rb1_body<FL, TC, PF, DIST, REV>(L, blockIdx.x, g, rc, X, Y, rhs, st, partials, counter, it, RH,
                               rh_lo, rh_hi, mb, dred, neu);
}

// One device, one launch: the full-width (TC 64) tiles of g64 in blocks
// [0, nb64) and the narrow strip of the columns past them (g2, tile width
// TC2) in the rest. A row's last TC-64 tile would be partial unless 124
// divides it, and costs a full tile's steps for its few columns (512^3: 14
// of 124); the strip's TC-16 / TC-32 tiles are 60 / 28 rows tall, so the
// column strip needs 4.8x / 2.2x fewer workgroups. Both geometries share the
// grid-wide residual reduction (part_total 0: gridDim.x workgroups).
template <int FL, int TC2, bool REV = false>
static __global__ __launch_bounds__(1024, 4) void k_rb1m(
    SGeo g64, SGeo g2, int nb64, RelaxCoef rc, const double* __restrict__ X,
    double* __restrict__ Y, const double* __restrict__ rhs, RxState* st, double* partials,
    unsigned* counter, int it, int neu) {
    __shared__ Rb1Lds L;
    if ((int)blockIdx.x < nb64)
        rb1_body<FL, 64, true, false, REV>(L, blockIdx.x, g64, rc, X, Y, rhs, st, partials,
                                           counter, it, nullptr, 0, 0, nullptr, nullptr, neu);
    else
        rb1_body<FL, TC2, true, false, REV>(L, blockIdx.x - nb64, g2, rc, X, Y, rhs, st,
                                            partials, counter, it, nullptr, 0, 0, nullptr,
                                            nullptr, neu);
}

// R (the first colour SOR-updated, linear_solver_redblack.c:97-114) of a
// slab's two edge planes k0 and k1 - 1 into RH, for the neighbours' k_rb1
// (DIST); same operands and order as k_rb1's R, so bitwise equal to it.
static __global__ __launch_bounds__(256) void k_rb_edge_r(SGeo g, RelaxCoef rc,
                                                         const double* __restrict__ X,
                                                         const double* __restrict__ rhs,
                                                         double* __restrict__ RH) {
    const long long plane = (long long)g.nx * g.ny;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < 2 * plane;
         e += (long long)gridDim.x * blockDim.x) {
        const int k = (e < plane) ? g.k0 : g.k1 - 1;
        const long long q = e % plane;
        const int j = (int)(q / g.nx), i = (int)(q % g.nx);
        if (i < 1 || i > g.nx - 2 || j < 1 || j > g.ny - 2) continue;
        const long long c = (long long)k * g.ps + (long long)j * g.px + i;
        double v = X[c];
        if (((i + j + k + g.kofs) & 1) == 1)
            v = sor1(rc, DivC{}, X[c], X[c - 1], X[c + 1], X[c - g.px], X[c + g.px], X[c - g.ps],
                     X[c + g.ps], rhs[c]);
        RH[c] = v;
    }
}


}  // namespace cfdhip
