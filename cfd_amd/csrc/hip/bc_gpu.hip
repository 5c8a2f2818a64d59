// bc_gpu.hip -- the reference's device-pointer BC entry points
// (boundary_conditions_gpu.cuh:32-151, impl boundary/gpu/boundary_conditions_gpu.cu)
// on caller-owned packed arrays: one k_bc_shell launch (pure gathers from
// interior cells) per field on the caller's stream; and the library's own
// launches of k_bc_shell on a context's field (launch_bc), so that the kernel
// is emitted by this unit only. The shell enumeration it shares with
// k_rx_shell and the step's shell passes is in device_util.hpp.
#include "ctx.hpp"

#include "cfd_hip/boundary_conditions_gpu.h"

namespace cfdhip {

// ---------------------------------------------------------------------------
// Boundary conditions as pure gathers from interior cells (race-free):
//   Neumann  (boundary_conditions_core_impl.h:41-85): c -> clamp(c, 1, n-2)
//   Periodic (:90-134):                               0 -> n-2, n-1 -> 1
// The reference applies x faces, then y faces, then z faces in place; the
// composition of those copies is exactly this per-coordinate map, edges and
// corners included. Dirichlet (:139-186) keeps the z > y > x face precedence.
// Threads cover the boundary shell: z faces (3-D) plus the x/y ring of every
// plane. mode: 0 Neumann, 1 periodic, 2 Dirichlet.
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_bc_shell(Geo g, double* __restrict__ f, int mode,
                                                  DirVals dv) {
    const long long total = shell_total(g);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        int i, j, k;
        bool zlo, zhi;
        shell_cell(g, e, i, j, k, zlo, zhi);
        const long long dst = cidx(g, i, j, k);
        if (mode == 2) {
            double v;
            if (zlo) v = dv.back;
            else if (zhi) v = dv.front;
            else if (j == 0) v = dv.bottom;
            else if (j == g.ny - 1) v = dv.top;
            else if (i == 0) v = dv.left;
            else v = dv.right;
            f[dst] = v;
        } else {
            int si = bc_map(i, g.nx, mode), sj = bc_map(j, g.ny, mode);
            int sk = (zlo || zhi) ? bc_map(k, g.nz, mode) : k;
            f[dst] = f[cidx(g, si, sj, sk)];
        }
    }
}

}  // namespace cfdhip

void launch_bc_geo(hip_proj_ctx* c, const Geo& g, double* f, int mode, const DirVals& dv) {
    klaunch(c, k_bc_shell, dim3(shell_blocks(c)), dim3(256), g, f, mode, dv);
}

void launch_bc(hip_proj_ctx* c, double* f, int mode, const DirVals& dv) {
    launch_bc_geo(c, c->geo, f, mode, dv);
}

namespace {

Geo packed_geo(size_t nx, size_t ny, size_t nz) {
    Geo g{};
    g.nx = (int)nx;
    g.ny = (int)ny;
    g.nz = (int)nz;
    g.px = (long long)nx;
    g.ps = (long long)nx * (long long)ny;
    g.sz = nz > 1 ? g.ps : 0;
    g.k0 = nz > 1 ? 1 : 0;
    g.k1 = nz > 1 ? (int)nz - 1 : 1;
    g.lo_face = g.hi_face = 1;
    return g;
}

void shell(double* f, const Geo& g, int mode, const DirVals& dv, void* stream) {
    const long long ring = 2LL * g.nx + 2LL * (g.ny - 2);
    const long long total = ring * g.nz + (g.nz > 1 ? 2LL * g.nx * g.ny : 0);
    const unsigned blocks = (unsigned)std::max(1LL, std::min((total + 255) / 256, 65535LL));
    hipLaunchKernelGGL(k_bc_shell, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, f, mode,
                       dv);
}

// bc_type_t -> k_bc_shell mode; the reference's device switch treats every
// type other than PERIODIC as NEUMANN (boundary_conditions_gpu.cu:477-526)
int mode_of(bc_type_t t) { return t == BC_TYPE_PERIODIC ? 1 : 0; }

DirVals dirvals(const bc_dirichlet_values_t* v) {
    DirVals d{};
    d.left = v->left;
    d.right = v->right;
    d.top = v->top;
    d.bottom = v->bottom;
    d.front = v->front;
    d.back = v->back;
    return d;
}

}  // namespace

extern "C" {

void bc_apply_scalar_gpu(double* d_field, size_t nx, size_t ny, bc_type_t type, void* stream) {
    if (!d_field || nx < 3 || ny < 3) return;
    shell(d_field, packed_geo(nx, ny, 1), mode_of(type), DirVals{}, stream);
}

void bc_apply_neumann_gpu(double* d_field, size_t nx, size_t ny, void* stream) {
    bc_apply_scalar_gpu(d_field, nx, ny, BC_TYPE_NEUMANN, stream);
}

void bc_apply_velocity_gpu(double* d_u, double* d_v, size_t nx, size_t ny, bc_type_t type,
                           void* stream) {
    if (!d_u || !d_v || nx < 3 || ny < 3) return;
    const Geo g = packed_geo(nx, ny, 1);
    shell(d_u, g, mode_of(type), DirVals{}, stream);
    shell(d_v, g, mode_of(type), DirVals{}, stream);
}

void bc_apply_dirichlet_scalar_gpu(double* d_field, size_t nx, size_t ny,
                                   const bc_dirichlet_values_t* values, void* stream) {
    if (!d_field || !values || nx < 3 || ny < 3) return;
    shell(d_field, packed_geo(nx, ny, 1), 2, dirvals(values), stream);
}

void bc_apply_dirichlet_velocity_gpu(double* d_u, double* d_v, size_t nx, size_t ny,
                                     const bc_dirichlet_values_t* u_values,
                                     const bc_dirichlet_values_t* v_values, void* stream) {
    if (!d_u || !d_v || !u_values || !v_values || nx < 3 || ny < 3) return;
    const Geo g = packed_geo(nx, ny, 1);
    shell(d_u, g, 2, dirvals(u_values), stream);
    shell(d_v, g, 2, dirvals(v_values), stream);
}

void bc_apply_scalar_3d_gpu(double* d_field, size_t nx, size_t ny, size_t nz, bc_type_t type,
                            void* stream) {
    if (!d_field || nx < 3 || ny < 3) return;
    if (nz == 1) return bc_apply_scalar_gpu(d_field, nx, ny, type, stream);
    if (nz < 3) return;
    shell(d_field, packed_geo(nx, ny, nz), mode_of(type), DirVals{}, stream);
}

void bc_apply_velocity_3d_gpu(double* d_u, double* d_v, double* d_w, size_t nx, size_t ny,
                              size_t nz, bc_type_t type, void* stream) {
    if (!d_u || !d_v || nx < 3 || ny < 3) return;
    if (nz == 1) return bc_apply_velocity_gpu(d_u, d_v, nx, ny, type, stream);
    if (nz < 3) return;
    const Geo g = packed_geo(nx, ny, nz);
    shell(d_u, g, mode_of(type), DirVals{}, stream);
    shell(d_v, g, mode_of(type), DirVals{}, stream);
    if (d_w) shell(d_w, g, mode_of(type), DirVals{}, stream);
}

}  // extern "C"
