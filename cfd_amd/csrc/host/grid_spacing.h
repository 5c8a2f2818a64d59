/*
 * grid_spacing.h -- what the explicit integrators and the energy equation
 * read of a grid's per-index spacing, shared by the device library (rk4_hip.hip
 * stages dx[], dy[] for the upload; ctx_validate_params refuses non-uniform
 * spacing with the energy equation on) and a host-only driver that runs the
 * same code under AddressSanitizer (tests/test_host_sanitizers.py).
 *
 * grid_create (grid.c:42-43; cfd_host.c, chk_format.h chk_read_grid) allocates
 * nx - 1 entries of dx and ny - 1 of dy: cell i spans x[i] .. x[i + 1]. The
 * device arrays have nx and ny slots, so that a kernel may index them with any
 * cell index; no interior cell reads the last slot.
 */
#ifndef CFD_HIP_GRID_SPACING_H
#define CFD_HIP_GRID_SPACING_H

#include "cfd_hip/cfd_abi.h"

#include <math.h>
#include <stddef.h>

/* n - 1 spacings into n slots; slot n - 1 repeats the last valid entry */
static inline void grid_stage_axis(const double* d, size_t n, double* out) {
    if (n == 0) return;
    for (size_t i = 0; i + 1 < n; i++) out[i] = d[i];
    out[n - 1] = (n > 1) ? d[n - 2] : 0.0;
}

/* out_dx[nx], out_dy[ny] from g->dx[nx - 1], g->dy[ny - 1] */
static inline void grid_stage_spacing(const grid* g, double* out_dx, double* out_dy) {
    grid_stage_axis(g->dx, g->nx, out_dx);
    grid_stage_axis(g->dy, g->ny, out_dy);
}

/* energy_step_explicit_with_workspace's uniformity check of one axis
 * (energy_solver.c:55-91): entries 1 .. n - 2 against entry 0 */
static inline int grid_axis_is_uniform(const double* d, size_t n) {
    if (n < 3) return 1;
    const double d0 = d[0];
    const double tol = 1e-12 * fmax(1.0, fabs(d0));
    for (size_t i = 1; i < n - 1; i++)
        if (fabs(d[i] - d0) > tol) return 0;
    return 1;
}

#endif
