// flow_diag.hip -- hip_proj_flow_diagnostics: the divergence norms and the
// kinetic energies the reference's validation drivers watch a run with
// (include/cfd_hip/flow_diagnostics.h; test_solver_helpers.h:176-309,
// taylor_green_3d_reference.h:125-171, lid_driven_cavity_common.h:194-201),
// reduced from the padded device fields in one launch, without a field
// download. The first stencil reduction of the library.
//
// k_flow_diag walks rows as k_derived_stats does: a wavefront owns row
// r = k * ny + j (rows r = 4 b + wave, then + 4 * gridDim.x), its lanes walk
// the row in 16-B pairs (i = 2 q, 2 q + 1; q = lane, lane + 64, ...), one 16-B
// load of u, v, w (and the resident rho) per pair: each field comes from HBM
// once. Every row is walked, boundary rows included (ke_rho_cells sums every
// cell). <false> is the pointwise energy pass. <true> adds, on interior rows
// (wave-uniform), the stencil: the pairs of v at j -+ 1 and of w at k -+ 1
// (16-B loads of rows the neighbouring waves and workgroups stream at about
// the same time: L1 / L2 hits) and u at i0 - 1 and i0 + 2 (8-B loads of lines
// this wave has just loaded). Rows start on 64-B boundaries (px is a multiple
// of 8), so the pair that straddles nx is loaded whole and its pad half is
// never folded into a result; pairs past nx are not loaded, and a stencil
// load is issued only on rows and for cells whose neighbour is a real cell.
//
// Per cell the reference's expressions in its operation order (the file is
// compiled with -ffp-contract=off); the two divisions by 2 dx and 2 dy are
// divz (device_util.hpp), the correctly rounded quotient, with its own
// fallback to `/` outside [2^-900, 2^900] and `/` throughout when the divisor
// is outside [2^-30, 2^30] (the range in which divz's residual is exact).
//
// Reduction (device_util.hpp's scheme, 6 scalars: four sums, the maximum, the
// NaN count): the per-thread walk order, a fixed 64-lane shuffle tree, the four
// waves in order, one record per workgroup stored by one lane with agent-scope
// relaxed (write-through) stores, s_waitcnt vmcnt(0), a ticket; the last
// workgroup reads every record with agent-scope loads and combines record b of
// each scalar in index order (thread t takes b = t, t + 256, ...; then the same
// tree and wave order). No floating-point atomics. The result depends on the
// grid size alone, never on which workgroup arrives last.
#include "ctx.hpp"

namespace {

constexpr int FD_NT = 256;  // threads per workgroup
constexpr int FD_WAVES = FD_NT / 64;
// scalars of a record
enum { FD_SUMSQ = 0, FD_KE, FD_KE_RHO, FD_KE_CELLS, FD_LINF, FD_NAN, FD_NS };
constexpr int FD_MAX_WG = 1024;  // 4 per CU: the last workgroup reads 6 x 1024 values
constexpr size_t FD_TOT = (size_t)FD_NS * FD_MAX_WG;  // totals after the records
constexpr size_t FD_TICKET = FD_TOT + 8;              // the ticket word
constexpr size_t FD_ELEMS = FD_TICKET + 8;

struct FdArgs {
    const double *u, *v, *w;
    const double* rho;  // nullptr: rho0 everywhere
    int nx, ny, nz;
    int k0, k1;             // interior planes [k0, k1)
    long long px, ps, sz;   // sz: the z stride of the stencil, ps in 3-D, 0 in 2-D
    double rho0;
    double two_dx, r_two_dx, two_dy, r_two_dy;  // 2.0 * d and RN(1 / (2.0 * d))
    double inv_2dz;         // 1.0 / (2.0 * dz) in 3-D, 0.0 in 2-D
    double dx, dy, dz;      // dz: 1.0 in 2-D (test_compute_kinetic_energy_3d's rule)
    int fast_div;           // both divisors inside divz's exact-residual range
};

// scalar S of a record: sums, the maximum of non-NaN values >= 0, and the NaN
// count, which travels as the 64 bits of a double (moves only)
template <int S>
__device__ __forceinline__ double fd_comb(double a, double b) {
    if constexpr (S == FD_NAN) {
        return __longlong_as_double(__double_as_longlong(a) + __double_as_longlong(b));
    } else {
        return S == FD_LINF ? fmax(a, b) : a + b;
    }
}
template <int S>
__device__ __forceinline__ double fd_wave(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fd_comb<S>(v, __shfl_down(v, off, 64));
    return v;
}

// wave totals of scalar S .. FD_NS - 1 into sh[s][wave]
template <int S>
__device__ __forceinline__ void fd_wave_all(const double (&x)[FD_NS], double (*sh)[FD_WAVES]) {
    if constexpr (S < FD_NS) {
        const double v = fd_wave<S>(x[S]);
        if ((threadIdx.x & 63) == 0) sh[S][threadIdx.x >> 6] = v;
        fd_wave_all<S + 1>(x, sh);
    }
}
// thread 0: the waves of scalar S in order
template <int S>
__device__ __forceinline__ void fd_block_all(double (*sh)[FD_WAVES], double (&out)[FD_NS]) {
    if constexpr (S < FD_NS) {
        double v = sh[S][0];
#pragma unroll
        for (int w = 1; w < FD_WAVES; ++w) v = fd_comb<S>(v, sh[S][w]);
        out[S] = v;
        fd_block_all<S + 1>(sh, out);
    }
}
// last workgroup: records 0 .. nb - 1 of scalar S, thread-strided in index
// order from the identity (0.0, all bits zero, for every scalar)
template <int S>
__device__ __forceinline__ void fd_grid_all(const double* rec, unsigned nb, double (&x)[FD_NS]) {
    if constexpr (S < FD_NS) {
        double v = 0.0;
        for (unsigned b = threadIdx.x; b < nb; b += FD_NT)
            v = fd_comb<S>(v, load_sc1(&rec[(size_t)S * nb + b]));
        x[S] = v;
        fd_grid_all<S + 1>(rec, nb, x);
    }
}

__device__ __forceinline__ double fd_div(const FdArgs& a, double num, double d, double r) {
    return a.fast_div ? divz(num, d, r) : num / d;
}

struct FdAcc {
    double sumsq, ke, ke_rho, ke_cells, linf;
    unsigned long long nan;
    // test_compute_divergence_linf_3d / _l2_3d: NaN never compares greater
    __device__ __forceinline__ void div(double d) {
        const double ad = fabs(d);
        if (ad > linf) linf = ad;
        sumsq += d * d;
        nan += d != d ? 1ULL : 0ULL;
    }
};

template <bool DIV>
__global__ __launch_bounds__(FD_NT) void k_flow_diag(FdArgs a, double* rec, double* tot,
                                                     unsigned* ticket) {
    __shared__ double sh[FD_NS][FD_WAVES];
    __shared__ int last;
    FdAcc acc = {0.0, 0.0, 0.0, 0.0, 0.0, 0ULL};
    const int lane = threadIdx.x & 63;
    const long long nrows = (long long)a.ny * a.nz;
    const int npair = (a.nx + 1) >> 1;
    for (long long r = (long long)blockIdx.x * FD_WAVES + (threadIdx.x >> 6); r < nrows;
         r += (long long)gridDim.x * FD_WAVES) {
        const long long k = r / a.ny, j = r - k * a.ny;
        const long long row = k * a.ps + j * a.px;
        // an interior row: its j -+ 1 and k -+ 1 neighbours are rows of the field
        const bool rin = j >= 1 && j <= a.ny - 2 && k >= a.k0 && k < a.k1;
        for (int q = lane; q < npair; q += 64) {
            const int i0 = 2 * q;
            const long long idx = row + i0;
            const bool two = i0 + 1 < a.nx;  // the pair's second cell is a cell, not pad
            const bool in0 = rin && i0 >= 1 && i0 <= a.nx - 2;
            const bool in1 = rin && i0 + 1 <= a.nx - 2;
            const double2 u = ld2(a.u, idx), v = ld2(a.v, idx), w = ld2(a.w, idx);
            const double2 rho = a.rho ? ld2(a.rho, idx) : make_double2(a.rho0, a.rho0);
            if (DIV && rin) {
                const double2 vn = ld2(a.v, idx + a.px), vs = ld2(a.v, idx - a.px);
                const double2 wn = ld2(a.w, idx + a.sz), ws = ld2(a.w, idx - a.sz);
                const double ul = in0 ? a.u[idx - 1] : 0.0;  // u(i0 - 1)
                const double ur = in1 ? a.u[idx + 2] : 0.0;  // u(i0 + 2)
                if (in0) {
                    const double du_dx = fd_div(a, u.y - ul, a.two_dx, a.r_two_dx);
                    const double dv_dy = fd_div(a, vn.x - vs.x, a.two_dy, a.r_two_dy);
                    const double dw_dz = (wn.x - ws.x) * a.inv_2dz;
                    acc.div(du_dx + dv_dy + dw_dz);
                }
                if (in1) {
                    const double du_dx = fd_div(a, ur - u.x, a.two_dx, a.r_two_dx);
                    const double dv_dy = fd_div(a, vn.y - vs.y, a.two_dy, a.r_two_dy);
                    const double dw_dz = (wn.y - ws.y) * a.inv_2dz;
                    acc.div(du_dx + dv_dy + dw_dz);
                }
            }
            const double sx = u.x * u.x + v.x * v.x + w.x * w.x;
            const double sy = u.y * u.y + v.y * v.y + w.y * w.y;
            acc.ke_cells += 0.5 * rho.x * sx;
            if (two) acc.ke_cells += 0.5 * rho.y * sy;
            if (in0) {
                acc.ke += 0.5 * sx * a.dx * a.dy * a.dz;
                acc.ke_rho += 0.5 * rho.x * sx * a.dx * a.dy * a.dz;
            }
            if (in1) {
                acc.ke += 0.5 * sy * a.dx * a.dy * a.dz;
                acc.ke_rho += 0.5 * rho.y * sy * a.dx * a.dy * a.dz;
            }
        }
    }
    double x[FD_NS];
    x[FD_SUMSQ] = acc.sumsq;
    x[FD_KE] = acc.ke;
    x[FD_KE_RHO] = acc.ke_rho;
    x[FD_KE_CELLS] = acc.ke_cells;
    x[FD_LINF] = acc.linf;
    x[FD_NAN] = __longlong_as_double((long long)acc.nan);
    fd_wave_all<0>(x, sh);
    __syncthreads();
    const unsigned nb = gridDim.x;
    if (threadIdx.x == 0) {
        double bt[FD_NS];
        fd_block_all<0>(sh, bt);
#pragma unroll
        for (int s = 0; s < FD_NS; ++s) store_sc1(&rec[(size_t)s * nb + blockIdx.x], bt[s]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned t = __hip_atomic_fetch_add((gu32*)ticket, 1u, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        last = (t == nb - 1) ? 1 : 0;
    }
    __syncthreads();
    if (last == 0) return;
    fd_grid_all<0>(rec, nb, x);
    fd_wave_all<0>(x, sh);
    __syncthreads();
    if (threadIdx.x == 0) {
        double gt[FD_NS];
        fd_block_all<0>(sh, gt);
#pragma unroll
        for (int s = 0; s < FD_NS; ++s) tot[s] = gt[s];
        __hip_atomic_store((gu32*)ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

unsigned fd_grid(const hip_proj_ctx* c) {
    const long long nrows = (long long)c->ny * (long long)c->nz;
    return (unsigned)std::max(1LL, std::min<long long>((nrows + FD_WAVES - 1) / FD_WAVES,
                                                       FD_MAX_WG));
}

cfd_status_t fd_refuse(cfd_status_t st, const char* msg) {
    set_err(st, msg);
    return st;
}

bool fd_divisor_ok(double d) { return d >= 0x1p-30 && d <= 0x1p+30; }

}  // namespace

extern "C" cfd_status_t hip_proj_flow_diagnostics(hip_proj_ctx_t* c, const grid* g, double rho0,
                                                  int what, cfd_flow_diag_t* out) {
    GroupHostLock hl_(c);
    if (!c || !g || !out || !g->dx || !g->dy)
        return fd_refuse(CFD_ERROR_INVALID, "hip_proj_flow_diagnostics: NULL argument");
    if (what < 1 || what > (HIP_DIAG_DIVERGENCE | HIP_DIAG_ENERGY))
        return fd_refuse(CFD_ERROR_INVALID,
                         "hip_proj_flow_diagnostics: `what` is HIP_DIAG_DIVERGENCE, "
                         "HIP_DIAG_ENERGY or both");
    if (dist(c))
        return fd_refuse(CFD_ERROR_UNSUPPORTED,
                         "hip_proj_flow_diagnostics: Z-slab contexts are not supported");
    const bool is3d = c->nz > 1;
    if (g->nx != c->nx || g->ny != c->ny || g->nz != c->nz || (is3d && !g->dz) ||
        g->k_start != (is3d ? 1u : 0u) || g->k_end != (is3d ? c->nz - 1 : 1u) ||
        g->stride_z != (is3d ? c->nx * c->ny : 0u))
        return fd_refuse(CFD_ERROR_INVALID,
                         "hip_proj_flow_diagnostics: grid/context dimension mismatch");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->fdiag && dalloc(c, &c->fdiag, FD_ELEMS) != CFD_SUCCESS) return CFD_ERROR_NOMEM;

    FdArgs a{};
    a.u = c->u;
    a.v = c->v;
    a.w = c->w;
    a.rho = c->rho;
    a.nx = (int)c->nx;
    a.ny = (int)c->ny;
    a.nz = (int)c->nz;
    a.k0 = (int)g->k_start;
    a.k1 = (int)g->k_end;
    a.px = c->px;
    a.ps = c->ps;
    a.sz = is3d ? c->ps : 0;
    a.rho0 = rho0;
    a.dx = g->dx[0];
    a.dy = g->dy[0];
    a.dz = is3d ? g->dz[0] : 1.0;
    a.two_dx = 2.0 * a.dx;
    a.two_dy = 2.0 * a.dy;
    a.r_two_dx = 1.0 / a.two_dx;
    a.r_two_dy = 1.0 / a.two_dy;
    a.inv_2dz = is3d ? 1.0 / (2.0 * g->dz[0]) : 0.0;
    a.fast_div = fd_divisor_ok(a.two_dx) && fd_divisor_ok(a.two_dy);

    double* tot = c->fdiag + FD_TOT;
    unsigned* ticket = reinterpret_cast<unsigned*>(c->fdiag + FD_TICKET);
    const dim3 grid(fd_grid(c)), block(FD_NT);
    if (what & HIP_DIAG_DIVERGENCE) klaunch(c, k_flow_diag<true>, grid, block, a, c->fdiag, tot, ticket);
    else klaunch(c, k_flow_diag<false>, grid, block, a, c->fdiag, tot, ticket);
    HIP_TRY(hipGetLastError());
    double h[FD_NS];
    HIP_TRY(hipMemcpyAsync(h, tot, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));

    memset(out, 0, sizeof(*out));
    if (what & HIP_DIAG_DIVERGENCE) {
        out->div_linf = h[FD_LINF];
        out->div_sumsq = h[FD_SUMSQ];
        const unsigned long long ni = c->nx > 2 ? c->nx - 2 : 0, nj = c->ny > 2 ? c->ny - 2 : 0;
        out->div_cells = ni * nj * (unsigned long long)(g->k_end - g->k_start);
        out->div_l2 = out->div_cells ? sqrt(out->div_sumsq / (double)out->div_cells) : 0.0;
        memcpy(&out->div_nan_cells, &h[FD_NAN], sizeof(out->div_nan_cells));
    }
    if (what & HIP_DIAG_ENERGY) {
        out->ke = h[FD_KE];
        out->ke_rho = h[FD_KE_RHO];
        out->ke_rho_cells = h[FD_KE_CELLS];
    }
    return CFD_SUCCESS;
}
