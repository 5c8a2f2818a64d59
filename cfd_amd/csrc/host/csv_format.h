/*
 * csv_format.h -- CSV text of the reference's monitoring outputs
 * (lib/src/io/csv_output.c:121-285: write_csv_timeseries, write_csv_centerline,
 * write_csv_statistics), shared by the host mirror (libcfd_host.so) and the
 * device-state writers of libcfd_hip.so (hip_proj_write_csv_*). Same header
 * rows, the same "%.6e" / "%.2f" values, the same header rule
 * (create_new || the file does not exist: truncate and write the header, else
 * append one row) and the same column sets with and without the velocity
 * magnitude. Each function returns 0, or -1 when the file cannot be opened.
 */
#ifndef CFD_HIP_CSV_FORMAT_H
#define CFD_HIP_CSV_FORMAT_H

#include "cfd_hip/cfd_abi.h"

#include <stddef.h>
#include <stdio.h>
#include <sys/stat.h>

static inline int csv_file_exists(const char* filename) {
    struct stat buffer;
    return (stat(filename, &buffer) == 0);
}

/* csv_output.c:121-164 */
static inline int csv_timeseries_row(const char* filename, int step, double time, double dt,
                                     const derived_fields* d, int has_vel_mag, int iterations,
                                     double residual, double elapsed_time_ms, int create_new) {
    int write_header = create_new || !csv_file_exists(filename);
    FILE* fp = fopen(filename, write_header ? "w" : "a");
    if (!fp) return -1;
    if (write_header) {
        fprintf(fp, "step,time,dt,max_u,max_v,max_w,max_p,avg_u,avg_v,avg_w,avg_p");
        if (has_vel_mag) fprintf(fp, ",max_vel_mag,avg_vel_mag");
        fprintf(fp, ",iterations,residual,elapsed_ms\n");
    }
    fprintf(fp, "%d,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e", step, time, dt,
            d->u_stats.max_val, d->v_stats.max_val, d->w_stats.max_val, d->p_stats.max_val,
            d->u_stats.avg_val, d->v_stats.avg_val, d->w_stats.avg_val, d->p_stats.avg_val);
    if (has_vel_mag) fprintf(fp, ",%.6e,%.6e", d->vel_mag_stats.max_val, d->vel_mag_stats.avg_val);
    fprintf(fp, ",%d,%.6e,%.2f\n", iterations, residual, elapsed_time_ms);
    fclose(fp);
    return 0;
}

/* csv_output.c:235-285 */
static inline int csv_statistics_row(const char* filename, int step, double time,
                                     const derived_fields* d, int has_vel_mag, int create_new) {
    int write_header = create_new || !csv_file_exists(filename);
    FILE* fp = fopen(filename, write_header ? "w" : "a");
    if (!fp) return -1;
    if (write_header) {
        fprintf(fp, "step,time,min_u,max_u,avg_u,min_v,max_v,avg_v,min_w,max_w,avg_w,"
                    "min_p,max_p,avg_p,min_rho,max_rho,avg_rho,min_T,max_T,avg_T");
        if (has_vel_mag) fprintf(fp, ",min_vel_mag,max_vel_mag,avg_vel_mag");
        fprintf(fp, "\n");
    }
    fprintf(fp,
            "%d,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,"
            "%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e",
            step, time, d->u_stats.min_val, d->u_stats.max_val, d->u_stats.avg_val,
            d->v_stats.min_val, d->v_stats.max_val, d->v_stats.avg_val, d->w_stats.min_val,
            d->w_stats.max_val, d->w_stats.avg_val, d->p_stats.min_val, d->p_stats.max_val,
            d->p_stats.avg_val, d->rho_stats.min_val, d->rho_stats.max_val, d->rho_stats.avg_val,
            d->T_stats.min_val, d->T_stats.max_val, d->T_stats.avg_val);
    if (has_vel_mag)
        fprintf(fp, ",%.6e,%.6e,%.6e", d->vel_mag_stats.min_val, d->vel_mag_stats.max_val,
                d->vel_mag_stats.avg_val);
    fprintf(fp, "\n");
    fclose(fp);
    return 0;
}

/* csv_output.c:170-229. One profile of `n` points: point e reads element
 * first + e * stride of every array (the host mirror passes the packed fields
 * with IDX_2D(i, j_mid, nx) / IDX_2D(i_mid, j, nx), the device writer its
 * gathered lines with first 0, stride 1). axis is 'x' or 'y'; w and vel_mag
 * may be NULL (0.0 written / no column). */
static inline int csv_centerline_file(const char* filename, char axis, const double* coords,
                                      size_t n, size_t first, size_t stride, const double* u,
                                      const double* v, const double* w, const double* p,
                                      const double* rho, const double* T,
                                      const double* vel_mag) {
    FILE* fp = fopen(filename, "w");
    if (!fp) return -1;
    fprintf(fp, "%c,u,v,w,p,rho,T", axis);
    if (vel_mag) fprintf(fp, ",vel_mag");
    fprintf(fp, "\n");
    for (size_t e = 0; e < n; e++) {
        size_t idx = first + e * stride;
        double w_val = w ? w[idx] : 0.0;
        fprintf(fp, "%.6e,%.6e,%.6e,%.6e,%.6e,%.6e,%.6e", coords[e], u[idx], v[idx], w_val,
                p[idx], rho[idx], T[idx]);
        if (vel_mag) fprintf(fp, ",%.6e", vel_mag[idx]);
        fprintf(fp, "\n");
    }
    fclose(fp);
    return 0;
}

#endif /* CFD_HIP_CSV_FORMAT_H */
