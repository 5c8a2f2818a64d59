/*
 * derived_host.c -- libcfd_host.so: host mirror of the reference's monitoring
 * layer, sequential code with the reference's signatures:
 *   field statistics and derived fields  lib/src/core/derived_fields.c:27-224
 *   CSV writers                          lib/src/io/csv_output.c:121-285
 * The CSV text lives in csv_format.h, which the device-state writers of
 * libcfd_hip.so (hip_proj_write_csv_*) format with as well.
 */
#define _GNU_SOURCE
#include "cfd_hip/cfd_host.h"
#include "csv_format.h"

#include <math.h>
#include <stdlib.h>

derived_fields* derived_fields_create(size_t nx, size_t ny, size_t nz) {
    derived_fields* derived = (derived_fields*)calloc(1, sizeof(derived_fields));
    if (derived) {
        derived->nx = nx;
        derived->ny = ny;
        derived->nz = nz;
        derived->velocity_magnitude = NULL;
    }
    return derived;
}

void derived_fields_clear(derived_fields* derived) {
    if (!derived) return;
    if (derived->velocity_magnitude) {
        free(derived->velocity_magnitude);
        derived->velocity_magnitude = NULL;
    }
    derived->stats_computed = 0;
}

void derived_fields_destroy(derived_fields* derived) {
    if (!derived) return;
    derived_fields_clear(derived);
    free(derived);
}

/* derived_fields.c:65-140, the sequential loop: min and max start at data[0]
 * and move on `<` / `>` (a NaN anywhere but data[0] is ignored), the sum runs
 * in index order. */
field_stats calculate_field_statistics(const double* data, size_t count) {
    field_stats stats = {0};
    if (!data || count == 0) return stats;
    stats.min_val = data[0];
    stats.max_val = data[0];
    stats.sum_val = 0.0;
    for (size_t i = 0; i < count; i++) {
        double val = data[i];
        if (val < stats.min_val) stats.min_val = val;
        if (val > stats.max_val) stats.max_val = val;
        stats.sum_val += val;
    }
    stats.avg_val = stats.sum_val / (double)count;
    return stats;
}

/* derived_fields.c:146-189 */
void derived_fields_compute_velocity_magnitude(derived_fields* derived, const flow_field* field) {
    if (!derived || !field || !field->u || !field->v) return;
    size_t n = derived->nx * derived->ny * derived->nz;
    if (!derived->velocity_magnitude) {
        derived->velocity_magnitude = (double*)malloc(n * sizeof(double));
        if (!derived->velocity_magnitude) return;
    }
    const double* u = field->u;
    const double* v = field->v;
    const double* w = field->w;
    double* vel_mag = derived->velocity_magnitude;
    for (size_t i = 0; i < n; i++) {
        double w_i = w ? w[i] : 0.0;
        vel_mag[i] = sqrt((u[i] * u[i]) + (v[i] * v[i]) + (w_i * w_i));
    }
}

/* derived_fields.c:191-224 */
void derived_fields_compute_statistics(derived_fields* derived, const flow_field* field) {
    if (!derived || !field) return;
    size_t count = derived->nx * derived->ny * derived->nz;
    if (field->u) derived->u_stats = calculate_field_statistics(field->u, count);
    if (field->v) derived->v_stats = calculate_field_statistics(field->v, count);
    if (field->w) derived->w_stats = calculate_field_statistics(field->w, count);
    if (field->p) derived->p_stats = calculate_field_statistics(field->p, count);
    if (field->rho) derived->rho_stats = calculate_field_statistics(field->rho, count);
    if (field->T) derived->T_stats = calculate_field_statistics(field->T, count);
    if (derived->velocity_magnitude)
        derived->vel_mag_stats = calculate_field_statistics(derived->velocity_magnitude, count);
    derived->stats_computed = 1;
}

void write_csv_timeseries(const char* filename, int step, double time, const flow_field* field,
                          const derived_fields* derived, const ns_solver_params_t* params,
                          const ns_solver_stats_t* stats, size_t nx, size_t ny, int create_new) {
    (void)field;
    (void)nx;
    (void)ny;
    if (!filename || !derived || !derived->stats_computed || !params || !stats) return;
    csv_timeseries_row(filename, step, time, params->dt, derived,
                       derived->velocity_magnitude != NULL, stats->iterations, stats->residual,
                       stats->elapsed_time_ms, create_new);
}

void write_csv_centerline(const char* filename, const flow_field* field,
                          const derived_fields* derived, const double* x_coords,
                          const double* y_coords, size_t nx, size_t ny,
                          profile_direction direction) {
    if (!filename || !field || !x_coords || !y_coords) return;
    const double* vel_mag = derived ? derived->velocity_magnitude : NULL;
    if (direction == PROFILE_HORIZONTAL)
        csv_centerline_file(filename, 'x', x_coords, nx, (ny / 2) * nx, 1, field->u, field->v,
                            field->w, field->p, field->rho, field->T, vel_mag);
    else
        csv_centerline_file(filename, 'y', y_coords, ny, nx / 2, nx, field->u, field->v,
                            field->w, field->p, field->rho, field->T, vel_mag);
}

void write_csv_statistics(const char* filename, int step, double time, const flow_field* field,
                          const derived_fields* derived, size_t nx, size_t ny, int create_new) {
    (void)field;
    (void)nx;
    (void)ny;
    if (!filename || !derived || !derived->stats_computed) return;
    csv_statistics_row(filename, step, time, derived, derived->velocity_magnitude != NULL,
                       create_new);
}
