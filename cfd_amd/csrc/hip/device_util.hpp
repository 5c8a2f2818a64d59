// device_util.hpp -- what more than one translation unit's gfx950 kernels
// use: the layout and reduction conventions below, the state structs the
// context holds, the grid-wide sums and maxima, the row-pair tile helpers and
// the fast divisions. It defines no kernel, so any unit may include it
// (ctx.hpp does). The kernels are in kernels.hpp (projection_hip.hip),
// rk_kernels.hpp (rk4_hip.hip) and the .hip files that alone launch them.
//
// Layout in HBM: every field is an SoA fp64 array with a padded row pitch
// `px` (multiple of 8 doubles = 64 B) and plane pitch `ps` = px*ny, x fastest.
// The reference layout idx = k*nx*ny + j*nx + i (lib/include/cfd/core/indexing.h)
// is recovered with px = nx; uploads/downloads convert with 2-D copies.
//
// Stencil sweeps use 2.5-D tiles: a 256-thread workgroup owns a 64 (x) by 4 (y)
// column tile and marches a chunk of `kc` planes in z, keeping the k-1/k/k+1
// values of its own column in registers so each plane is read once from HBM;
// x/y neighbours come from the L1/L2 lines the neighbouring lanes and waves
// of the same tile just loaded. One wavefront = one 64-wide x row, so every
// load is a fully coalesced 512-B row segment.
//
// Reductions are deterministic: per-thread sums in a fixed k order, a fixed
// 64-lane shuffle tree, a fixed cross-wave order, one partial per workgroup,
// and the last-arriving workgroup (agent-scope ticket) sums the partials in
// index order. The partial hand-off follows the sc1 write-through protocol
// (MI355X_MICROARCH.md "Valid forms", first table row): one lane stores the
// partial with an agent-scope relaxed store, waits vmcnt(0), then takes the
// ticket; the last workgroup reads every partial with agent-scope loads.
//
// All arithmetic is written in the reference's operation order and the file
// is compiled with -ffp-contract=off, so every per-cell value is bitwise the
// reference's; only the summation order of the CG dot products differs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mbox.hpp"
#include "tile_plan.hpp"

namespace cfdhip {

// TX x TY: the tile of the grid-stride kernels (tile_plan.hpp)
constexpr int NT = TX * TY;  // threads per workgroup
constexpr int NWAVE = NT / 64;

// Poisson status codes (poisson_solver.h:83-89)
constexpr int ST_CONVERGED = 0;
constexpr int ST_MAX_ITER = 1;
constexpr int ST_STAGNATED = 3;

struct Lap {
    double dx2_inv, dy2_inv, inv_dz2;  // linear_solver_cg.c:103-110
};

// x is updated every CG_XFOLD iterations: sweep A of iteration it with
// it % CG_XFOLD == 0, it > 0, folds the CG_XFOLD pending alpha_j p_j
// (j = it - 4 .. it - 1) into x before p_it overwrites slot it % CG_XFOLD;
// the search directions live in a ring of CG_XFOLD buffers (p_j in [j % CG_XFOLD]).
// A solve that stops after iteration it therefore leaves it % CG_XFOLD + 1
// (1 .. CG_XFOLD) updates pending, in distinct ring slots, for k_cg_finalize.
constexpr int CG_XFOLD = 4;

// Device-resident CG state; written only by the finishing (last) workgroup.
struct CgState {
    double rho;     // (r, r) of the current residual
    double alpha[CG_XFOLD];  // alpha_j of iteration j at [j % CG_XFOLD]
    double beta;    // beta for the next sweep A
    double pAp;
    double res;     // current residual 2-norm
    double res0;    // initial residual
    double tol;     // max(rel_tol * res0, abs_tol)
    double abs_tol;
    int iterations; // completed iterations (reference stats->iterations)
    int done;       // no further iteration may run
    int status;     // poisson_solver_status_t
    int nalpha;     // iterations whose alpha is valid (x must hold alpha_j p_j, j < nalpha)
    int xdone;      // x holds alpha_j p_j for j < xdone (folded by sweep B)
    int max_iter;
    int check_interval;
    int pad0;
};

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;

__device__ __forceinline__ void store_sc1(double* p, double v) {
    __hip_atomic_store((gu64*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double load_sc1(const double* p) {
    unsigned long long b =
        __hip_atomic_load((gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __longlong_as_double((long long)b);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    return v;
}

// Sum over the workgroup; result valid in thread 0. `sh` holds NWAVE doubles.
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < NWAVE; ++w) s += sh[w];
    }
    __syncthreads();
    return s;
}

// Grid-wide deterministic sum. Returns true (in every thread) for the
// last-arriving workgroup; its thread 0 then holds the grid total.
__device__ __forceinline__ bool grid_sum_last(double block_total, double* partials,
                                              unsigned* counter, double* sh, int* flag,
                                              double& total) {
    if (threadIdx.x == 0) {
        store_sc1(&partials[blockIdx.x], block_total);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned t = __hip_atomic_fetch_add((gu32*)counter, 1u, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        *flag = (t == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (*flag == 0) return false;
    double s = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += NT) s += load_sc1(&partials[b]);
    total = block_sum(s, sh);
    if (threadIdx.x == 0)
        __hip_atomic_store((gu32*)counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// Same protocol for NTH-thread workgroups; `sh` needs NTH/64 doubles of LDS
// that no wave still reads (callers pass their stencil row buffer after the
// workgroup barrier that ends the sweep).
template <int NTH>
__device__ __forceinline__ bool grid_sum_last_n(double block_total, double* partials,
                                                unsigned* counter, double* sh, int* flag,
                                                double& total, unsigned pofs = 0,
                                                unsigned ptot = 0) {
    if (ptot == 0) ptot = gridDim.x;
    if (threadIdx.x == 0) {
        store_sc1(&partials[pofs + blockIdx.x], block_total);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned t = __hip_atomic_fetch_add((gu32*)counter, 1u, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        *flag = (t == ptot - 1) ? 1 : 0;
    }
    __syncthreads();
    if (*flag == 0) return false;
    double s = 0.0;
    for (unsigned b = threadIdx.x; b < ptot; b += NTH) s += load_sc1(&partials[b]);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < NTH / 64; ++w) a += sh[w];
        total = a;
        __hip_atomic_store((gu32*)counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return true;
}

// Order-preserving encoding of doubles into uint64 for atomicMax.
__device__ __forceinline__ unsigned long long ord_enc(double d) {
    unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}

struct TileCoord {
    int i, j, kb, ke;
    bool active;
};

__device__ __forceinline__ TileCoord tile_coord(const Geo& g, int t) {
    TileCoord c;
    const int tx = t % g.tiles_x;
    const int rest = t / g.tiles_x;
    const int ty = rest % g.tiles_y;
    const int tz = rest / g.tiles_y;
    c.i = tx * TX + (threadIdx.x & 63);
    c.j = ty * TY + (threadIdx.x >> 6);
    c.kb = g.k0 + tz * g.kc;
    c.ke = min(c.kb + g.kc, g.k1);
    c.active = (c.i >= 1) && (c.i <= g.nx - 2) && (c.j >= 1) && (c.j <= g.ny - 2);
    return c;
}

__device__ __forceinline__ long long cidx(const Geo& g, int i, int j, int k) {
    return (long long)k * g.ps + (long long)j * g.px + i;
}

constexpr int ST_COMM_TIMEOUT = 9;

__device__ __forceinline__ int xcd_tile(int b, int nt) {
    // bijective remap: block b runs on XCD b % 8 (round-robin dispatch);
    // give each XCD a contiguous range of tiles (speed only, never correctness)
    const int q = nt / 8, rem = nt % 8;
    const int x = b % 8, l = b / 8;
    const int start = x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q;
    return start + l;
}

__device__ __forceinline__ double2 ld2(const double* p, long long i) {
    return *reinterpret_cast<const double2*>(p + i);
}
__device__ __forceinline__ void st2(double* p, long long i, double2 v) {
    *reinterpret_cast<double2*>(p + i) = v;
}

// Sweep variants (template FL): the SW_* flags of tile_plan.hpp.
typedef double d2x __attribute__((ext_vector_type(2)));
template <int FL>
__device__ __forceinline__ void st2v(double* p, long long i, double2 v) {
    if (FL & SW_NT_STORE) {
        d2x w = {v.x, v.y};
        __builtin_nontemporal_store(w, reinterpret_cast<d2x*>(p + i));
    } else {
        *reinterpret_cast<double2*>(p + i) = v;
    }
}
// A 16-B store into one plane through a buffer resource: an offset past the
// plane's bytes is dropped by the hardware, so a lane (or a step) that must
// not store passes ST_NOSTORE instead of branching around the store. Every
// step of a march then issues the same stores, and the compiler's vmcnt
// counting stays exact (a store under a branch counts as possibly absent, so
// the wait for a later plane's loads would also wait for that store).
constexpr int ST_NOSTORE = 0x7ffffff0;
// AUX: the store's cache-policy bits (2: nt, 16: sc1 write-through)
template <int AUX>
__device__ __forceinline__ void st2ba(double* plane_base, long long plane_elems, int boff,
                                      double2 v) {
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(plane_base, 0, (int)(plane_elems * 8), 0x00020000);
    const unsigned long long bx = (unsigned long long)__double_as_longlong(v.x);
    const unsigned long long by = (unsigned long long)__double_as_longlong(v.y);
    const u4 d = {(unsigned)bx, (unsigned)(bx >> 32), (unsigned)by, (unsigned)(by >> 32)};
    __builtin_amdgcn_raw_buffer_store_b128(d, rs, boff, 0, AUX);
}
template <bool NT>
__device__ __forceinline__ void st2b(double* plane_base, long long plane_elems, int boff,
                                     double2 v) {
    st2ba<NT ? 2 : 0>(plane_base, plane_elems, boff, v);  // aux 2: nt
}

// The load counterpart of st2b: a 16-B load from one plane through a buffer
// resource; an offset past the plane (ST_NOSTORE) returns zeros without a
// memory access, so a lane or step that needs no data issues the same load
// instead of branching around it (no branch: exact vmcnt counting).
// AUX: the load's cache-policy bits (2: nt, 16: sc1, which bypasses the L1)
template <int AUX>
__device__ __forceinline__ double2 ld2ba(const double* plane_base, long long plane_elems,
                                         int boff) {
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double*>(plane_base), 0, (int)(plane_elems * 8), 0x00020000);
    const u4 d = __builtin_amdgcn_raw_buffer_load_b128(rs, boff, 0, AUX);
    const unsigned long long bx = (unsigned long long)d.x | ((unsigned long long)d.y << 32);
    const unsigned long long by = (unsigned long long)d.z | ((unsigned long long)d.w << 32);
    return make_double2(__longlong_as_double((long long)bx), __longlong_as_double((long long)by));
}
template <bool NT = false>
__device__ __forceinline__ double2 ld2b(const double* plane_base, long long plane_elems, int boff) {
    return ld2ba<NT ? 2 : 0>(plane_base, plane_elems, boff);  // aux 2: nt
}

template <int FL>
__device__ __forceinline__ double2 ld2v(const double* p, long long i) {
    if (FL & SW_NT_LOAD) {
        d2x w = __builtin_nontemporal_load(reinterpret_cast<const d2x*>(p + i));
        return make_double2(w.x, w.y);
    }
    return *reinterpret_cast<const double2*>(p + i);
}

struct RowPair {
    int i0, j, kb, ke, lane, w;
    bool act, in0, in1;
    long long idx;   // cell (i0, clamp(j), kb)
};

template <int TY>
__device__ __forceinline__ RowPair row_pair(const SGeo& g) {
    RowPair c;
    const int nt = g.tiles_x * g.tiles_y * g.tiles_z;
    const int t = xcd_tile(blockIdx.x, nt);
    const int tx = t % g.tiles_x;
    const int rest = t / g.tiles_x;
    const int ty = rest % g.tiles_y;
    const int tz = rest / g.tiles_y;
    c.lane = threadIdx.x & 63;
    c.w = threadIdx.x >> 6;
    c.i0 = tx * 128 + 2 * c.lane;
    c.j = ty * TY + c.w;
    if (g.kmode == 1) {
        c.kb = (tz == 0) ? g.k0 : g.k1 - 1;
        c.ke = c.kb + 1;
    } else {
        c.kb = g.k0 + tz * g.kc;
        c.ke = min(c.kb + g.kc, g.k1);
    }
    c.act = (c.j >= 1) && (c.j <= g.ny - 2) && (c.i0 < g.nx);
    c.in0 = c.act && (c.i0 >= 1) && (c.i0 <= g.nx - 2);
    c.in1 = c.act && (c.i0 + 1 <= g.nx - 2);
    const int ic = min(c.i0, g.nx - 2 - ((g.nx - 2) & 1));  // even, in-row, 16-B aligned
    const int jc = min(c.j, g.ny - 1);
    c.idx = (long long)c.kb * g.ps + (long long)jc * g.px + (c.i0 < g.nx ? c.i0 : ic);
    return c;
}

// (r01e: asking for 8 waves per SIMD, i.e. <= 64 VGPRs and two 1024-thread
// workgroups per CU, spills and is slower; profiles/r01e_sweep_variants.jsonl)
template <int FL>
constexpr int sweep_min_waves() {
    return (FL & SW_PREFETCH) ? 4 : 1;
}

struct DirVals {
    double left, right, top, bottom, front, back;
};

__device__ __forceinline__ int bc_map(int c, int n, int mode) {
    if (mode == 0) return c == 0 ? 1 : (c == n - 1 ? n - 2 : c);
    return c == 0 ? n - 2 : (c == n - 1 ? 1 : c);
}

// In a Z-slab the z faces exist only on the edge ranks (lo_face / hi_face);
// the x/y ring is applied on every local plane, halo planes included (their
// owner applies the identical gather to the same values).
// Boundary-shell cell e of the enumeration k_bc_shell / k_rx_shell share:
// the x/y ring of every local plane, then the z faces the rank owns.
__device__ __forceinline__ long long shell_total(const Geo& g) {
    const bool is3d = g.nz > 1;
    const long long ring = 2LL * g.nx + 2LL * (g.ny - 2);
    const long long plane = (long long)g.nx * g.ny;
    return ring * g.nz + ((is3d && g.lo_face) ? plane : 0) + ((is3d && g.hi_face) ? plane : 0);
}
__device__ __forceinline__ void shell_cell(const Geo& g, long long e, int& i, int& j, int& k,
                                           bool& zlo, bool& zhi) {
    const bool is3d = g.nz > 1;
    const bool lo = is3d && g.lo_face, hi = is3d && g.hi_face;
    const long long ring = 2LL * g.nx + 2LL * (g.ny - 2);  // x/y boundary ring of one plane
    const long long nring = ring * g.nz;
    const long long plane = (long long)g.nx * g.ny;
    if (e < nring) {
        k = (int)(e / ring);
        long long q = e % ring;
        if (q < g.nx) { i = (int)q; j = 0; }
        else if (q < 2LL * g.nx) { i = (int)(q - g.nx); j = g.ny - 1; }
        else if (q < 2LL * g.nx + (g.ny - 2)) { i = 0; j = (int)(q - 2LL * g.nx) + 1; }
        else { i = g.nx - 1; j = (int)(q - 2LL * g.nx - (g.ny - 2)) + 1; }
    } else {
        long long q = e - nring;
        k = (lo && q < plane) ? 0 : g.nz - 1;
        q = q % plane;
        j = (int)(q / g.nx);
        i = (int)(q % g.nx);
    }
    zlo = lo && k == 0;
    zhi = hi && k == g.nz - 1;
}

// a / d, correctly rounded, for the constant divisors dx2 / dy2 of the
// relaxation sweeps, from the correctly rounded reciprocal r = RN(1/d):
// q = RN(a r) is within 1 ulp of a/d, a - q d is exact in one FMA, and the
// corrected q + (a - q d) r rounds to RN(a/d) (Markstein's correction, the
// IA-64 division scheme) -- 3 VALU ops instead of the ~14-op generic fp64
// division, bitwise the reference's `/` (checked on 9.6e8 random quotients,
// tools/divc_check.c, and by the bitwise relaxation tests). Quotients near the
// underflow/overflow range, zeros (sign of zero) and non-finite values take
// the generic division.
__device__ __forceinline__ double divc(double a, double d, double r) {
    const double q = a * r;
    const double aq = fabs(q);
    if (!(aq >= 0x1p-900 && aq <= 0x1p+900)) return a / d;  // residual stays normal
    return fma(fma(-q, d, a), r, q);
}

// Division functors for the stencil helpers. DivC: divc, its range test a
// branch per division. DivFastZ (below, with divz) defers the test: the fast
// quotient's range check goes into a lane flag (compare masks, no branch) and
// the caller recomputes the lanes whose flag dropped with DivExact behind ONE
// wave-uniform branch; where the flag held the value is divz's, so results
// are bitwise either way. That form helps the predictor (fewer, longer basic
// blocks) but spilled in k_rb1 and made it slower (0.845 vs 0.751 ms at
// 512^3, profiles/r02_deferred_div.jsonl), which keeps DivC.
struct DivC {  // divc, its range test branching per division
    __device__ __forceinline__ double operator()(double a, double d, double r) const {
        return divc(a, d, r);
    }
};
struct DivExact {  // the reference's division (the recompute path)
    __device__ __forceinline__ double operator()(double a, double d, double) const { return a / d; }
};
// true when some lane of the wave dropped its flag (wave-uniform)
__device__ __forceinline__ bool wave_any_bad(bool ok) {
    return __builtin_amdgcn_ballot_w64(!ok) != 0;
}

struct RxState {
    double tol, abs_tol, rel_tol, res0, res;
    int iterations, done, status, max_iter, check_interval, result;  // result: buffer index
    // two iterations per sweep (k_rb2, rb2.hpp): the iterate index the loop
    // stopped on, whether `res` is that iterate's exact residual, the
    // host-resolved exact residual of iterate ovr_it (-1: none), and max |rhs|
    int res_it, res_exact, ovr_it, pad0;
    double ovr_m, bmax;
    double xmax;  // max |X| of a k_rb2 sweep's input when it certifies X (k_rb2_xmax)
};

template <bool V>
using BoolC = std::integral_constant<bool, V>;
template <int V>
using IntC = std::integral_constant<int, V>;

// a / d correctly rounded, like divc, for operands that are often exactly
// zero (derivatives of a field at rest): e = q d - a and q - e r give the
// signed zero of a / d for a = +-0, so zeros stay on the fast path.
__device__ __forceinline__ double divz(double a, double d, double r) {
    const double q = a * r;
    const double aq = fabs(q);
    if (!(aq <= 0x1p+900 && (aq >= 0x1p-900 || aq == 0.0))) return a / d;
    return fma(-fma(q, d, -a), r, q);
}
// divz with the range test deferred into a lane flag (see DivC)
struct DivFastZ {
    bool& ok;
    __device__ __forceinline__ double operator()(double a, double d, double r) const {
        const double q = a * r;
        const double aq = fabs(q);
        ok &= (aq <= 0x1p+900) & ((aq >= 0x1p-900) | (aq == 0.0));
        return fma(-fma(q, d, -a), r, q);
    }
};

}  // namespace cfdhip
