// derived_stats.hip -- monitoring of the device-resident state: the
// reference's field statistics and velocity magnitude
// (lib/src/core/derived_fields.c:65-224) and its three CSV outputs
// (lib/src/io/csv_output.c:121-285, text in ../host/csv_format.h) computed
// from the padded device fields, without a field download.
//
// k_derived_stats is one streaming pass. Rows are walked by (j, k): a
// wavefront owns row r = k * ny + j (rows r = 4 b + wave, then + 4 * gridDim.x),
// its lanes walk the row in 16-B pairs (i = 2 q, 2 q + 1; q = lane, lane + 64,
// ...), one 16-B load per resident field and pair. Rows start on 64-B
// boundaries (px is a multiple of 8), so the pair that straddles nx is loaded
// whole and its pad half is never folded into a result; pairs past nx are not
// loaded at all. Per thread: min, max (fmin / fmax over the non-NaN values),
// sum and the first-zero key (ds_comb), in that walk order, of each resident
// field among u, v, w, p, rho, T and, on request, of
// sqrt((u*u) + (v*v) + (w*w)) (the reference's expression; the file is
// compiled with -ffp-contract=off), which an optional output array receives
// with non-temporal 16-B stores in the padded layout. The lane that holds
// cell 0 also stores each quantity's cell-0 value beside the totals. From
// these the host states the reference's sequential `<` / `>` loop (ds_stats):
// a NaN in cell 0 is min and max, bit for bit; a zero extreme has the sign of
// the zero with the lowest packed index.
//
// Reduction (device_util.hpp's scheme, 28 scalars): the per-thread order above, a
// fixed 64-lane shuffle tree, the four waves in order, one record of 28
// values per workgroup stored by one lane with agent-scope relaxed
// (write-through) stores, s_waitcnt vmcnt(0), a ticket; the last workgroup
// reads every record with agent-scope loads and combines record b of each
// scalar in index order (thread t takes b = t, t + 256, ...; then the same
// tree and wave order). The grid is capped at DS_MAX_WG workgroups so that
// pass stays short. The result depends on the grid size alone, never on which
// workgroup arrives last.
//
// k_line_gather copies row j = ny/2 or column i = nx/2 of the k = 0 plane of
// the six fields and the magnitude into one packed buffer for the centerline
// CSV (IDX_2D(i, j, nx) of the reference is the k = 0 plane on a 3-D grid too).
#include "ctx.hpp"

#include "../host/csv_format.h"

#include <limits>
#include <memory>

namespace {

constexpr int DS_NT = 256;       // threads per workgroup
constexpr int DS_WAVES = DS_NT / 64;
constexpr int DS_NF = 7;         // u v w p rho T |vel|
constexpr int DS_NK = 4;         // min, max, sum, first-zero key of each
constexpr int DS_NS = DS_NK * DS_NF;
constexpr int DS_MAX_WG = 1024;  // 4 per CU: the last workgroup reads 28 x 1024 values
constexpr size_t DS_TOT = (size_t)DS_NS * DS_MAX_WG;  // totals after the records
constexpr size_t DS_CELL0 = DS_TOT + DS_NS;           // cell 0 of each quantity after the totals
constexpr size_t DS_TICKET = DS_TOT + 40;             // the ticket word
constexpr size_t DS_ELEMS = DS_TICKET + 8;
constexpr int DS_NOUT = DS_NS + DS_NF;                // what the host reads back
static_assert(DS_CELL0 + DS_NF <= DS_TICKET, "the cell-0 values end before the ticket");
constexpr unsigned long long DS_NO_ZERO = ~0ULL;      // key of a field without a zero

struct DsArgs {
    const double* f[6];  // u v w p rho T; nullptr: not part of this pass
    double* mag;         // padded-layout output of the magnitude, or nullptr
    int nx, ny, nz;
    long long px, ps;
};

// scalar s of a record: field s / 4, kind s % 4 (0 min, 1 max, 2 sum, 3 the
// first-zero key). The key is 2 * (k nx ny + j nx + i) + sign bit of the zero
// with the lowest packed index, DS_NO_ZERO without one; it travels through the
// record as the 64 bits of a double (moves only) and combines as an unsigned min.
template <int KIND>
__device__ __forceinline__ double ds_comb(double a, double b) {
    if constexpr (KIND == 3) {
        const unsigned long long x = (unsigned long long)__double_as_longlong(a);
        const unsigned long long y = (unsigned long long)__double_as_longlong(b);
        return __longlong_as_double((long long)(x < y ? x : y));
    } else {
        return KIND == 0 ? fmin(a, b) : (KIND == 1 ? fmax(a, b) : a + b);
    }
}
template <int KIND>
__device__ __forceinline__ double ds_wave(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = ds_comb<KIND>(v, __shfl_down(v, off, 64));
    return v;
}
template <int KIND>
__device__ __forceinline__ double ds_ident() {
    return KIND == 0 ? __longlong_as_double(0x7FF0000000000000LL)
           : KIND == 1 ? __longlong_as_double((long long)0xFFF0000000000000ULL)
           : KIND == 2 ? 0.0 : __longlong_as_double((long long)DS_NO_ZERO);
}

struct DsAcc {
    double mn, mx, sm;
    unsigned long long zk;
    __device__ __forceinline__ void fold(double v) {
        mn = fmin(mn, v);
        mx = fmax(mx, v);
        sm += v;
    }
    __device__ __forceinline__ void zero(double v, unsigned long long cell) {
        const unsigned long long key =
            (cell << 1) | ((unsigned long long)__double_as_longlong(v) >> 63);
        zk = key < zk ? key : zk;
    }
    // One 16-B pair; cell: the packed index k nx ny + j nx + i of v.x; two: v.y
    // is a cell, not pad. The key work sits behind a branch the whole wave
    // takes together, so a pair without a zero pays two compares for it.
    __device__ __forceinline__ void add(double2 v, bool two, unsigned long long cell) {
        fold(v.x);
        if (two) fold(v.y);
        const bool zx = v.x == 0.0, zy = two && v.y == 0.0;
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(zx || zy) != 0, 0)) {
            if (zx) zero(v.x, cell);
            if (zy) zero(v.y, cell + 1);
        }
    }
};

template <int S>
__device__ __forceinline__ double ds_get(const DsAcc (&a)[DS_NF]) {
    constexpr int K = S % DS_NK, F = S / DS_NK;
    return K == 0 ? a[F].mn : K == 1 ? a[F].mx : K == 2 ? a[F].sm
                                                       : __longlong_as_double((long long)a[F].zk);
}

// wave totals of scalar S .. DS_NS - 1 into sh[s][wave]
template <int S>
__device__ __forceinline__ void ds_wave_all(const DsAcc (&a)[DS_NF], double (*sh)[DS_WAVES]) {
    if constexpr (S < DS_NS) {
        const double v = ds_wave<S % DS_NK>(ds_get<S>(a));
        if ((threadIdx.x & 63) == 0) sh[S][threadIdx.x >> 6] = v;
        ds_wave_all<S + 1>(a, sh);
    }
}

// thread 0: the waves of scalar S in order
template <int S>
__device__ __forceinline__ void ds_block_all(double (*sh)[DS_WAVES], double (&out)[DS_NS]) {
    if constexpr (S < DS_NS) {
        double v = sh[S][0];
#pragma unroll
        for (int w = 1; w < DS_WAVES; ++w) v = ds_comb<S % DS_NK>(v, sh[S][w]);
        out[S] = v;
        ds_block_all<S + 1>(sh, out);
    }
}

// last workgroup: records 0 .. nb - 1 of scalar S, thread-strided in index
// order (thread t folds b = t, t + 256, ... from the identity). The thread's
// records of one field's DS_NK scalars are loaded together (one memory latency
// per field, not one per record), then folded in that order.
constexpr int DS_NB = DS_MAX_WG / DS_NT;  // records of a scalar per thread, at most
template <int S>
__device__ __forceinline__ void ds_grid_fold(const double (&x)[DS_NB], unsigned nb,
                                             double (*sh)[DS_WAVES]) {
    double v = ds_ident<S % DS_NK>();
#pragma unroll
    for (int i = 0; i < DS_NB; ++i)
        if (threadIdx.x + i * DS_NT < nb) v = ds_comb<S % DS_NK>(v, x[i]);
    v = ds_wave<S % DS_NK>(v);
    if ((threadIdx.x & 63) == 0) sh[S][threadIdx.x >> 6] = v;
}
template <int F>
__device__ __forceinline__ void ds_grid_all(const double* rec, unsigned nb,
                                            double (*sh)[DS_WAVES]) {
    if constexpr (F < DS_NF) {
        double x[DS_NK][DS_NB];
#pragma unroll
        for (int k = 0; k < DS_NK; ++k) {
#pragma unroll
            for (int i = 0; i < DS_NB; ++i) {
                const unsigned b = threadIdx.x + i * DS_NT;  // past nb: record 0, not folded
                x[k][i] = load_sc1(&rec[(size_t)(F * DS_NK + k) * nb + (b < nb ? b : 0u)]);
            }
        }
        ds_grid_fold<F * DS_NK + 0>(x[0], nb, sh);
        ds_grid_fold<F * DS_NK + 1>(x[1], nb, sh);
        ds_grid_fold<F * DS_NK + 2>(x[2], nb, sh);
        ds_grid_fold<F * DS_NK + 3>(x[3], nb, sh);
        ds_grid_all<F + 1>(rec, nb, sh);
    }
}
static_assert(DS_NK == 4, "ds_grid_all folds four scalars per field");

template <bool MAG>
__global__ __launch_bounds__(DS_NT) void k_derived_stats(DsArgs a, double* rec, double* tot,
                                                         unsigned* ticket) {
    __shared__ double sh[DS_NS][DS_WAVES];
    __shared__ int last;
    DsAcc acc[DS_NF];
#pragma unroll
    for (int q = 0; q < DS_NF; ++q) {
        acc[q].mn = ds_ident<0>();
        acc[q].mx = ds_ident<1>();
        acc[q].sm = 0.0;
        acc[q].zk = DS_NO_ZERO;
    }
    const int lane = threadIdx.x & 63;
    const long long nrows = (long long)a.ny * a.nz;
    const int npair = (a.nx + 1) >> 1;
    for (long long r = (long long)blockIdx.x * DS_WAVES + (threadIdx.x >> 6); r < nrows;
         r += (long long)gridDim.x * DS_WAVES) {
        const long long k = r / a.ny, j = r - k * a.ny;
        const long long row = k * a.ps + j * a.px;
        const unsigned long long cell0 = (unsigned long long)r * (unsigned long long)a.nx;
        for (int q = lane; q < npair; q += 64) {
            const long long idx = row + 2 * q;
            const unsigned long long cell = cell0 + 2 * (unsigned)q;
            const bool first = r == 0 && q == 0;  // this lane holds cell 0
            const bool two = 2 * q + 1 < a.nx;  // the pair's second cell is a cell, not pad
            double2 val[6];
#pragma unroll
            for (int f = 0; f < 6; ++f)
                val[f] = a.f[f] ? ld2(a.f[f], idx) : make_double2(0.0, 0.0);
#pragma unroll
            for (int f = 0; f < 6; ++f) {
                if (a.f[f]) {
                    acc[f].add(val[f], two, cell);
                    if (first) tot[DS_NS + f] = val[f].x;
                }
            }
            if (MAG) {
                // derived_fields.c:175; an absent w is w_i = 0.0
                const double mx = sqrt((val[0].x * val[0].x) + (val[1].x * val[1].x) +
                                       (val[2].x * val[2].x));
                const double my = sqrt((val[0].y * val[0].y) + (val[1].y * val[1].y) +
                                       (val[2].y * val[2].y));
                acc[6].add(make_double2(mx, my), two, cell);
                if (first) tot[DS_NS + 6] = mx;
                if (a.mag) {
                    d2x w = {mx, two ? my : 0.0};
                    __builtin_nontemporal_store(w, reinterpret_cast<d2x*>(a.mag + idx));
                }
            }
        }
    }
    ds_wave_all<0>(acc, sh);
    __syncthreads();
    const unsigned nb = gridDim.x;
    if (threadIdx.x == 0) {
        double bt[DS_NS];
        ds_block_all<0>(sh, bt);
#pragma unroll
        for (int s = 0; s < DS_NS; ++s) store_sc1(&rec[(size_t)s * nb + blockIdx.x], bt[s]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned t = __hip_atomic_fetch_add((gu32*)ticket, 1u, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        last = (t == nb - 1) ? 1 : 0;
    }
    __syncthreads();
    if (last == 0) return;
    ds_grid_all<0>(rec, nb, sh);
    __syncthreads();
    if (threadIdx.x == 0) {
        double gt[DS_NS];
        ds_block_all<0>(sh, gt);
#pragma unroll
        for (int s = 0; s < DS_NS; ++s) tot[s] = gt[s];
        __hip_atomic_store((gu32*)ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// out[q * n + e], q = u v w p rho T |vel|: point e of row j = ny/2 (vertical
// == 0, n = nx) or column i = nx/2 (n = ny) of the k = 0 plane
__global__ void k_line_gather(DsArgs a, int vertical, int n, double rho0, double* out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const long long idx = vertical ? (long long)e * a.px + a.nx / 2
                                   : (long long)(a.ny / 2) * a.px + e;
    const double u = a.f[0][idx], v = a.f[1][idx];
    const double w = a.f[2] ? a.f[2][idx] : 0.0;
    out[e] = u;
    out[(size_t)n + e] = v;
    out[2 * (size_t)n + e] = w;
    out[3 * (size_t)n + e] = a.f[3][idx];
    out[4 * (size_t)n + e] = a.f[4] ? a.f[4][idx] : rho0;
    out[5 * (size_t)n + e] = a.f[5] ? a.f[5][idx] : 0.0;
    out[6 * (size_t)n + e] = sqrt((u * u) + (v * v) + (w * w));
}

DsArgs ds_args(const hip_proj_ctx* c) {
    DsArgs a{};
    a.nx = (int)c->nx;
    a.ny = (int)c->ny;
    a.nz = (int)c->nz;
    a.px = c->px;
    a.ps = c->ps;
    return a;
}

unsigned ds_grid(const hip_proj_ctx* c) {
    const long long nrows = (long long)c->ny * (long long)c->nz;
    return (unsigned)std::max(1LL, std::min<long long>((nrows + DS_WAVES - 1) / DS_WAVES,
                                                       DS_MAX_WG));
}

// One pass over the fields of `a`; tot[4 q .. 4 q + 3] = min, max, sum and
// first-zero key of field q, tot[DS_NS + q] its cell 0 (valid for the fields
// in the pass, and for q = 6 with `mag`).
cfd_status_t ds_run(hip_proj_ctx* c, const DsArgs& a, bool mag, double (&tot)[DS_NOUT]) {
    if (!c->dstat) {
        if (dalloc(c, &c->dstat, DS_ELEMS) != CFD_SUCCESS) return CFD_ERROR_NOMEM;
    }
    unsigned* ticket = reinterpret_cast<unsigned*>(c->dstat + DS_TICKET);
    const dim3 grid(ds_grid(c)), block(DS_NT);
    if (mag) klaunch(c, k_derived_stats<true>, grid, block, a, c->dstat, c->dstat + DS_TOT, ticket);
    else klaunch(c, k_derived_stats<false>, grid, block, a, c->dstat, c->dstat + DS_TOT, ticket);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tot, c->dstat + DS_TOT, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CFD_SUCCESS;
}

// The reference's sequential loop (derived_fields.c:107-120): min and max
// start at data[0] and move on strict `<` / `>`. A NaN in cell 0 therefore
// stays in both; any other NaN is ignored; a zero extreme keeps the sign of
// the first zero in index order (no later zero compares below or above it).
field_stats ds_stats(const double (&tot)[DS_NOUT], int q, double count) {
    field_stats s;
    const double first = tot[DS_NS + q];
    if (first != first) {
        s.min_val = s.max_val = first;
    } else {
        unsigned long long key;
        memcpy(&key, &tot[DS_NK * q + 3], sizeof(key));
        const double zero = (key & 1ULL) ? -0.0 : 0.0;
        s.min_val = tot[DS_NK * q] == 0.0 ? zero : tot[DS_NK * q];
        s.max_val = tot[DS_NK * q + 1] == 0.0 ? zero : tot[DS_NK * q + 1];
    }
    s.sum_val = tot[DS_NK * q + 2];
    s.avg_val = s.sum_val / count;
    return s;
}

field_stats ds_const(double v, double count) {
    field_stats s;
    s.min_val = s.max_val = v;
    s.sum_val = v * count;
    s.avg_val = s.sum_val / count;
    return s;
}

cfd_status_t ds_check(const hip_proj_ctx* c, const char* who) {
    if (dist(c)) {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: Z-slab contexts are not supported", who);
        set_err(CFD_ERROR_UNSUPPORTED, msg);
        return CFD_ERROR_UNSUPPORTED;
    }
    return CFD_SUCCESS;
}

cfd_status_t ds_derived(hip_proj_ctx* c, int with_vel_mag, double rho0, derived_fields* out) {
    HIP_TRY(hipSetDevice(c->device));
    DsArgs a = ds_args(c);
    const double* fs[6] = {c->u, c->v, c->w, c->p, c->rho, c->T};
    for (int q = 0; q < 6; ++q) a.f[q] = fs[q];
    double tot[DS_NOUT];
    ST_TRY(ds_run(c, a, with_vel_mag != 0, tot));
    const double count = (double)(c->nx * c->ny * c->nz);
    field_stats* dst[6] = {&out->u_stats, &out->v_stats, &out->w_stats,
                           &out->p_stats, &out->rho_stats, &out->T_stats};
    const double absent[6] = {0.0, 0.0, 0.0, 0.0, rho0, 0.0};
    for (int q = 0; q < 6; ++q) *dst[q] = fs[q] ? ds_stats(tot, q, count) : ds_const(absent[q], count);
    if (with_vel_mag) out->vel_mag_stats = ds_stats(tot, 6, count);
    out->stats_computed = 1;
    return CFD_SUCCESS;
}

}  // namespace

extern "C" {

cfd_status_t hip_proj_field_statistics(hip_proj_ctx_t* c, int field_id, field_stats* out) {
    GroupHostLock hl_(c);
    if (!c || !out) return CFD_ERROR_INVALID;
    ST_TRY(ds_check(c, "hip_proj_field_statistics"));
    const double* f = field_ptr(c, field_id);
    if (!f) {
        set_err(CFD_ERROR_INVALID, "hip_proj_field_statistics: the context holds no such field");
        return CFD_ERROR_INVALID;
    }
    HIP_TRY(hipSetDevice(c->device));
    DsArgs a = ds_args(c);
    a.f[0] = f;
    double tot[DS_NOUT];
    ST_TRY(ds_run(c, a, false, tot));
    *out = ds_stats(tot, 0, (double)(c->nx * c->ny * c->nz));
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_derived_statistics(hip_proj_ctx_t* c, int with_vel_mag, double rho0,
                                         derived_fields* out) {
    GroupHostLock hl_(c);
    if (!c || !out) return CFD_ERROR_INVALID;
    ST_TRY(ds_check(c, "hip_proj_derived_statistics"));
    return ds_derived(c, with_vel_mag, rho0, out);
}

cfd_status_t hip_proj_velocity_magnitude(hip_proj_ctx_t* c, double* host) {
    GroupHostLock hl_(c);
    if (!c || !host) return CFD_ERROR_INVALID;
    ST_TRY(ds_check(c, "hip_proj_velocity_magnitude"));
    HIP_TRY(hipSetDevice(c->device));
    if (!c->vmag && dalloc(c, &c->vmag, field_elems(c)) != CFD_SUCCESS) return CFD_ERROR_NOMEM;
    DsArgs a = ds_args(c);
    a.f[0] = c->u;
    a.f[1] = c->v;
    a.f[2] = c->w;
    a.mag = c->vmag;
    double tot[DS_NOUT];
    ST_TRY(ds_run(c, a, true, tot));
    HIP_TRY(copy_out(c, host, c->vmag));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_write_csv_timeseries(hip_proj_ctx_t* c, const char* filename, int step,
                                           double time, const ns_solver_params_t* params,
                                           const ns_solver_stats_t* stats, int with_vel_mag,
                                           int create_new) {
    GroupHostLock hl_(c);
    if (!c || !filename || !params || !stats) return CFD_ERROR_INVALID;
    ST_TRY(ds_check(c, "hip_proj_write_csv_timeseries"));
    derived_fields d{};
    ST_TRY(ds_derived(c, with_vel_mag, c->rho0, &d));
    if (csv_timeseries_row(filename, step, time, params->dt, &d, with_vel_mag != 0,
                           stats->iterations, stats->residual, stats->elapsed_time_ms,
                           create_new) != 0) {
        set_err(CFD_ERROR_IO, "Failed to open CSV timeseries file for writing");
        return CFD_ERROR_IO;
    }
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_write_csv_statistics(hip_proj_ctx_t* c, const char* filename, int step,
                                           double time, double rho0, int with_vel_mag,
                                           int create_new) {
    GroupHostLock hl_(c);
    if (!c || !filename) return CFD_ERROR_INVALID;
    ST_TRY(ds_check(c, "hip_proj_write_csv_statistics"));
    derived_fields d{};
    ST_TRY(ds_derived(c, with_vel_mag, rho0, &d));
    if (csv_statistics_row(filename, step, time, &d, with_vel_mag != 0, create_new) != 0) {
        set_err(CFD_ERROR_IO, "Failed to open CSV statistics file for writing");
        return CFD_ERROR_IO;
    }
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_write_csv_centerline(hip_proj_ctx_t* c, const char* filename, const grid* g,
                                           profile_direction direction, double rho0,
                                           int with_vel_mag) {
    GroupHostLock hl_(c);
    if (!c || !filename || !g || !g->x || !g->y) return CFD_ERROR_INVALID;
    ST_TRY(ds_check(c, "hip_proj_write_csv_centerline"));
    if (g->nx != c->nx || g->ny != c->ny || g->nz != c->nz) {
        set_err(CFD_ERROR_INVALID, "hip_proj_write_csv_centerline: grid/context dimension mismatch");
        return CFD_ERROR_INVALID;
    }
    HIP_TRY(hipSetDevice(c->device));
    const int vertical = direction == PROFILE_HORIZONTAL ? 0 : 1;
    const int n = (int)(vertical ? c->ny : c->nx);
    DsArgs a = ds_args(c);
    const double* fs[6] = {c->u, c->v, c->w, c->p, c->rho, c->T};
    for (int q = 0; q < 6; ++q) a.f[q] = fs[q];
    double* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, (size_t)DS_NF * n * sizeof(double)));
    std::unique_ptr<double[]> line(new double[(size_t)DS_NF * n]);
    klaunch(c, k_line_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), a, vertical, n, rho0,
            dev);
    cfd_status_t st = CFD_SUCCESS;
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(line.get(), dev, (size_t)DS_NF * n * sizeof(double), hipMemcpyDeviceToHost,
                       c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        st = CFD_ERROR;
    hipFree(dev);
    if (st != CFD_SUCCESS) {
        set_err(st, "hip_proj_write_csv_centerline: line gather failed");
        return st;
    }
    const double* l = line.get();
    if (csv_centerline_file(filename, vertical ? 'y' : 'x', vertical ? g->y : g->x, (size_t)n, 0, 1,
                            l, l + n, l + 2 * (size_t)n, l + 3 * (size_t)n, l + 4 * (size_t)n,
                            l + 5 * (size_t)n, with_vel_mag ? l + 6 * (size_t)n : nullptr) != 0) {
        set_err(CFD_ERROR_IO, "Failed to open CSV centerline file for writing");
        return CFD_ERROR_IO;
    }
    return CFD_SUCCESS;
}

}  // extern "C"
