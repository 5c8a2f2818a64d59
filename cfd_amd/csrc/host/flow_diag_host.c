/*
 * flow_diag_host.c -- libcfd_host.so: cfd_flow_diagnostics, the host twin of
 * hip_proj_flow_diagnostics (include/cfd_hip/flow_diagnostics.h). Plain
 * sequential loops in the order of the reference's validation helpers, so
 * every number, sums included, is bitwise theirs:
 *   test_compute_divergence_linf_3d / _l2_3d, test_compute_kinetic_energy_3d,
 *   test_compute_kinetic_energy   tests/solvers/navier_stokes/test_solver_helpers.h:176-309
 *   tg3_compute_kinetic_energy    tests/validation/taylor_green_3d_reference.h:125-147
 *   compute_kinetic_energy        tests/validation/lid_driven_cavity_common.h:194-201
 */
#include "cfd_hip/flow_diagnostics.h"

#include <math.h>
#include <string.h>

cfd_status_t cfd_flow_diagnostics(const flow_field* field, const grid* g, double rho0, int what,
                                  cfd_flow_diag_t* out) {
    if (!field || !g || !out || !field->u || !field->v || !g->dx || !g->dy)
        return CFD_ERROR_INVALID;
    if (what < 1 || what > (HIP_DIAG_DIVERGENCE | HIP_DIAG_ENERGY)) return CFD_ERROR_INVALID;
    if (g->nx != field->nx || g->ny != field->ny || g->nz != field->nz) return CFD_ERROR_INVALID;
    if (field->nz > 1 && !g->dz) return CFD_ERROR_INVALID;
    if ((what & HIP_DIAG_DIVERGENCE) && !field->w) return CFD_ERROR_INVALID;
    const size_t nx = field->nx, ny = field->ny, nz = field->nz;
    const size_t stride_z = g->stride_z;
    const double dx = g->dx[0], dy = g->dy[0];
    const double* u = field->u;
    const double* v = field->v;
    const double* w = field->w;
    const double* rho = field->rho;
    memset(out, 0, sizeof(*out));

    if (what & HIP_DIAG_DIVERGENCE) {
        const double inv_2dz = (nz > 1) ? 1.0 / (2.0 * g->dz[0]) : 0.0;
        double max_div = 0.0, sum = 0.0;
        unsigned long long count = 0, nans = 0;
        for (size_t k = g->k_start; k < g->k_end; k++) {
            for (size_t j = 1; j + 1 < ny; j++) {
                for (size_t i = 1; i + 1 < nx; i++) {
                    size_t idx = (k * stride_z) + j * nx + i;
                    double du_dx = (u[idx + 1] - u[idx - 1]) / (2.0 * dx);
                    double dv_dy = (v[idx + nx] - v[idx - nx]) / (2.0 * dy);
                    double dw_dz = (w[idx + stride_z] - w[idx - stride_z]) * inv_2dz;
                    double div = du_dx + dv_dy + dw_dz;
                    if (fabs(div) > max_div) max_div = fabs(div);
                    sum += div * div;
                    count++;
                    if (div != div) nans++;
                }
            }
        }
        out->div_linf = max_div;
        out->div_sumsq = sum;
        out->div_cells = count;
        out->div_nan_cells = nans;
        out->div_l2 = (count > 0) ? sqrt(sum / (double)count) : 0.0;
    }

    if (what & HIP_DIAG_ENERGY) {
        const double dz = (nz > 1) ? g->dz[0] : 1.0;
        double ke = 0.0, ke_rho = 0.0, ke_cells = 0.0;
        for (size_t k = g->k_start; k < g->k_end; k++) {
            for (size_t j = 1; j + 1 < ny; j++) {
                for (size_t i = 1; i + 1 < nx; i++) {
                    size_t idx = (k * stride_z) + j * nx + i;
                    double r = rho ? rho[idx] : rho0;
                    double ui = u[idx], vi = v[idx];
                    double wi = w ? w[idx] : 0.0;
                    ke += 0.5 * (ui * ui + vi * vi + wi * wi) * dx * dy * dz;
                    ke_rho += 0.5 * r * (ui * ui + vi * vi + wi * wi) * dx * dy * dz;
                }
            }
        }
        const size_t total = nx * ny * nz;
        for (size_t i = 0; i < total; i++) {
            double r = rho ? rho[i] : rho0;
            double wi = w ? w[i] : 0.0;
            ke_cells += 0.5 * r * (u[i] * u[i] + v[i] * v[i] + wi * wi);
        }
        out->ke = ke;
        out->ke_rho = ke_rho;
        out->ke_rho_cells = ke_cells;
    }
    return CFD_SUCCESS;
}
