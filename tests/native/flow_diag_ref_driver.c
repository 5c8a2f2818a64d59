/*
 * flow_diag_ref_driver.c -- calls the reference's own validation helpers on a
 * seeded input and prints their results as hex floats. Compiled by
 * tests/golden/make_flow_diag_golden.py against the reference's include
 * directories (lib/include, tests/solvers/navier_stokes, tests/validation)
 * with -ffp-contract=off; an empty unity.h stand-in in the work directory
 * satisfies the two validation headers, which use none of its macros outside
 * functions this driver never calls. Never built by the product.
 *
 * usage: flow_diag_ref_driver INPUT
 * INPUT: uint64 nx, ny, nz; double dx, dy, dz; then u, v, w, rho as
 * nx*ny*nz packed doubles each (idx = k*nx*ny + j*nx + i).
 * Output: one "name hexfloat" line per helper. The 2-D helpers run on
 * nz == 1 inputs only, the tg3 helpers (they read g->dz[0]) on nz > 1 only.
 */
#include "test_solver_helpers.h"
#include "taylor_green_3d_reference.h"
#include "lid_driven_cavity_common.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static double* read_array(FILE* fp, size_t n) {
    double* a = (double*)malloc(n * sizeof(double));
    if (!a || fread(a, sizeof(double), n, fp) != n) {
        fprintf(stderr, "flow_diag_ref_driver: short input\n");
        exit(2);
    }
    return a;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    uint64_t dims[3];
    double h[3];
    if (fread(dims, sizeof(uint64_t), 3, fp) != 3 || fread(h, sizeof(double), 3, fp) != 3) return 2;
    const size_t nx = dims[0], ny = dims[1], nz = dims[2], n = nx * ny * nz;

    flow_field f;
    memset(&f, 0, sizeof(f));
    f.nx = nx;
    f.ny = ny;
    f.nz = nz;
    f.u = read_array(fp, n);
    f.v = read_array(fp, n);
    f.w = read_array(fp, n);
    f.rho = read_array(fp, n);
    fclose(fp);

    /* a hand-filled uniform grid: the helpers read dx[0], dy[0], dz[0],
     * stride_z, k_start and k_end only (grid.c's values for these) */
    grid g;
    memset(&g, 0, sizeof(g));
    g.nx = nx;
    g.ny = ny;
    g.nz = nz;
    g.dx = &h[0];
    g.dy = &h[1];
    if (nz > 1) {
        g.dz = &h[2];
        g.stride_z = nx * ny;
        g.k_start = 1;
        g.k_end = nz - 1;
    } else {
        g.dz = NULL;
        g.stride_z = 0;
        g.k_start = 0;
        g.k_end = 1;
    }

    printf("test_compute_divergence_linf_3d %a\n", test_compute_divergence_linf_3d(&f, &g));
    printf("test_compute_divergence_l2_3d %a\n", test_compute_divergence_l2_3d(&f, &g));
    printf("test_compute_kinetic_energy_3d %a\n", test_compute_kinetic_energy_3d(&f, &g));
    if (nz > 1) {
        printf("tg3_compute_kinetic_energy %a\n", tg3_compute_kinetic_energy(&f, &g));
        printf("tg3_compute_max_divergence %a\n", tg3_compute_max_divergence(&f, &g));
    } else {
        printf("test_compute_kinetic_energy %a\n", test_compute_kinetic_energy(&f, &g));
        printf("test_compute_kinetic_energy_simple %a\n",
               test_compute_kinetic_energy_simple(&f, &g));
        printf("compute_kinetic_energy %a\n", compute_kinetic_energy(&f));
    }
    return 0;
}
