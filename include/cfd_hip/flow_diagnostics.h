/*
 * flow_diagnostics.h -- the numbers the reference's validation drivers watch
 * a run with, from the device-resident state (hip_proj_flow_diagnostics,
 * libcfd_hip.so, one kernel launch, no field download) or from host arrays
 * (cfd_flow_diagnostics, libcfd_host.so, the reference's sequential loops):
 *
 *   divergence norms   test_compute_divergence_linf_3d / _l2_3d
 *                      (tests/solvers/navier_stokes/test_solver_helpers.h:176-234),
 *                      tg3_compute_max_divergence (taylor_green_3d_reference.h:149-171)
 *   kinetic energy     test_compute_kinetic_energy_3d / test_compute_kinetic_energy
 *                      (test_solver_helpers.h:244-309), tg3_compute_kinetic_energy
 *                      (taylor_green_3d_reference.h:125-147), the cavity drivers'
 *                      compute_kinetic_energy (lid_driven_cavity_common.h:194-201)
 *
 * Interior: 1 <= i <= nx-2, 1 <= j <= ny-2, k in [g->k_start, g->k_end)
 * (1 .. nz-2 in 3-D, the single plane in 2-D). Spacings: dx[0], dy[0], dz[0].
 * Per interior cell, in the helpers' operation order (no contraction):
 *   du_dx = (u[+1] - u[-1]) / (2.0*dx)
 *   dv_dy = (v[+nx] - v[-nx]) / (2.0*dy)
 *   dw_dz = (w[+sz] - w[-sz]) * inv_2dz,  inv_2dz = 1.0/(2.0*dz) in 3-D;
 *           in 2-D sz = 0 and inv_2dz = 0.0: dw_dz = (w - w) * 0.0, so a
 *           non-finite w makes that cell's divergence NaN, as in the reference
 *   div   = (du_dx + dv_dy) + dw_dz
 * Not part of cfd_abi.h, which mirrors reference types only. Additive: no ABI
 * version change, no kernel timer.
 */
#ifndef CFD_HIP_FLOW_DIAGNOSTICS_H
#define CFD_HIP_FLOW_DIAGNOSTICS_H

#include "cfd_hip/cfd_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { HIP_DIAG_DIVERGENCE = 1, HIP_DIAG_ENERGY = 2 };

typedef struct {
    /* max |div| over the interior, the helper's loop: starts at 0.0 and moves
     * only on fabs(div) > max, so a NaN divergence is skipped and a field of
     * NaNs reports 0.0 -- read div_nan_cells beside it */
    double div_linf;                  /* test_compute_divergence_linf_3d */
    double div_sumsq;                 /* the sum inside test_compute_divergence_l2_3d */
    double div_l2;                    /* sqrt(div_sumsq / (double)div_cells), formed on the host */
    unsigned long long div_cells;     /* interior cells (the helper's `count`, 64-bit here) */
    unsigned long long div_nan_cells; /* interior cells whose divergence is NaN */
    /* sum over the interior of 0.5 * (u*u + v*v + w*w) * dx * dy * dz, with
     * dz -> 1.0 in 2-D (the helper's rule) */
    double ke;                        /* test_compute_kinetic_energy_3d / tg3_compute_kinetic_energy */
    /* sum over the interior of 0.5 * rho * (u*u + v*v + w*w) * dx * dy * dz,
     * same rule; in 2-D with w = 0 every term has the bits of
     * test_compute_kinetic_energy's */
    double ke_rho;
    /* sum over EVERY cell, boundary included, of 0.5 * rho * (u*u + v*v + w*w),
     * no volume factor: on a 2-D field with w = 0 the cavity drivers'
     * compute_kinetic_energy; on 3-D grids it is this library's extension
     * (the reference defines none) */
    double ke_rho_cells;
} cfd_flow_diag_t;

typedef struct hip_proj_ctx hip_proj_ctx_t;

/* The diagnostics of the device-resident u, v, w in one kernel launch: `what`
 * is HIP_DIAG_DIVERGENCE, HIP_DIAG_ENERGY or both (3); the outputs of a bit
 * that is not set are 0. rho is the resident HIP_FIELD_RHO where the context
 * holds it, else the constant rho0 (the convention of hip_proj_write_vtk and
 * hip_proj_derived_statistics). Every per-cell term has the reference's bits;
 * the sums run in the device's fixed order (per thread, 64-lane tree, waves,
 * workgroups in index order), a function of the grid size alone: bit-identical
 * from run to run, equal to the sequential sum up to rounding. Any NaN term
 * makes a sum NaN (sign and payload unspecified); +inf terms only, +inf.
 * Changes no device state, ends no resident (dirty_faces) run.
 * CFD_ERROR_INVALID: a NULL argument (g->dx / dy / dz included), `what`
 * outside 1..3, a grid whose extents differ from the context's;
 * CFD_ERROR_UNSUPPORTED: a Z-slab context. Nothing is launched on a refusal. */
CFD_HIP_EXPORT cfd_status_t hip_proj_flow_diagnostics(hip_proj_ctx_t* ctx, const grid* g,
                                                      double rho0, int what,
                                                      cfd_flow_diag_t* out);

/* The same numbers from host arrays with the reference's sequential loops
 * (libcfd_host.so): every number, sums included, is bitwise the helper's.
 * field->w == NULL reads as w = 0.0 in the energies (the helpers' rule); the
 * divergence needs w (CFD_ERROR_INVALID without it, as the helpers would
 * fault). field->rho == NULL uses rho0. */
CFD_HIP_EXPORT cfd_status_t cfd_flow_diagnostics(const flow_field* field, const grid* g,
                                                 double rho0, int what, cfd_flow_diag_t* out);

#ifdef __cplusplus
}
#endif

#endif /* CFD_HIP_FLOW_DIAGNOSTICS_H */
