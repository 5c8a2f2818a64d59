/*
 * derived_host_main.c -- stand-alone driver of the host monitoring code
 * (cfd_amd/csrc/host/derived_host.c + csv_format.h) for the sanitizer build of
 * tests/test_derived_fixtures.py: heap blocks of exactly nx*ny*nz doubles, the
 * statistics, the magnitude with and without w, and every CSV writer with
 * and without the magnitude, header and append paths, both directions.
 * usage: derived_host_main <scratch directory>
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cfd_hip/cfd_host.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static long file_lines(const char* path) {
    FILE* fp = fopen(path, "r");
    if (!fp) return -1;
    long n = 0;
    for (int ch; (ch = fgetc(fp)) != EOF;) n += ch == '\n';
    fclose(fp);
    return n;
}

static int run(const char* dir, size_t nx, size_t ny, size_t nz, int with_w) {
    const size_t n = nx * ny * nz;
    char path[1024];
    double* arr[6];
    for (int q = 0; q < 6; q++) {
        arr[q] = (double*)malloc(n * sizeof(double));
        CHECK(arr[q]);
        for (size_t e = 0; e < n; e++) arr[q][e] = (double)((e * 7 + (size_t)q * 3) % 11) - 5.0;
    }
    arr[0][n - 1] = 40.0; /* max in the last cell */
    arr[0][0] = -40.0;    /* min at index 0 */
    arr[3][n / 2] = NAN;  /* ignored by min / max, propagates into the sum */
    flow_field f = {arr[0], arr[1], with_w ? arr[2] : NULL, arr[3], arr[4], arr[5], nx, ny, nz};
    double* x = (double*)malloc(nx * sizeof(double));
    double* y = (double*)malloc(ny * sizeof(double));
    CHECK(x && y);
    for (size_t i = 0; i < nx; i++) x[i] = (double)i / (double)nx;
    for (size_t j = 0; j < ny; j++) y[j] = (double)j / (double)ny;

    field_stats s = calculate_field_statistics(arr[0], n);
    CHECK(s.min_val == -40.0 && s.max_val == 40.0 && s.avg_val == s.sum_val / (double)n);
    s = calculate_field_statistics(NULL, n);
    CHECK(s.min_val == 0.0 && s.sum_val == 0.0);
    s = calculate_field_statistics(arr[0], 0);
    CHECK(s.max_val == 0.0);

    derived_fields* d = derived_fields_create(nx, ny, nz);
    CHECK(d && !d->velocity_magnitude && !d->stats_computed);
    ns_solver_params_t prm;
    memset(&prm, 0, sizeof prm);
    prm.dt = 1e-3;
    ns_solver_stats_t st;
    memset(&st, 0, sizeof st);
    st.iterations = 5;
    st.residual = 1e-7;
    st.elapsed_time_ms = 1.5;
    snprintf(path, sizeof path, "%s/ts.csv", dir);
    remove(path);
    write_csv_timeseries(path, 0, 0.0, &f, d, &prm, &st, nx, ny, 0); /* stats not computed */
    CHECK(file_lines(path) == -1);
    for (int mag = 0; mag < 2; mag++) {
        if (mag) {
            derived_fields_compute_velocity_magnitude(d, &f);
            CHECK(d->velocity_magnitude);
            double w0 = with_w ? arr[2][n - 1] : 0.0;
            CHECK(d->velocity_magnitude[n - 1] ==
                  sqrt((arr[0][n - 1] * arr[0][n - 1]) + (arr[1][n - 1] * arr[1][n - 1]) +
                       (w0 * w0)));
        }
        derived_fields_compute_statistics(d, &f);
        CHECK(d->stats_computed == 1 && d->u_stats.max_val == 40.0);
        CHECK(isnan(d->p_stats.sum_val) && !isnan(d->p_stats.min_val) &&
              !isnan(d->p_stats.max_val));
        snprintf(path, sizeof path, "%s/ts%d.csv", dir, mag);
        remove(path);
        for (int step = 0; step < 3; step++)
            write_csv_timeseries(path, step, 0.1 * step, &f, d, &prm, &st, nx, ny, 0);
        CHECK(file_lines(path) == 4); /* header by absence, then appended rows */
        write_csv_timeseries(path, 3, 0.3, &f, d, &prm, &st, nx, ny, 1);
        CHECK(file_lines(path) == 2); /* create_new truncates */
        snprintf(path, sizeof path, "%s/st%d.csv", dir, mag);
        remove(path);
        for (int step = 0; step < 3; step++)
            write_csv_statistics(path, step, 0.1 * step, &f, d, nx, ny, step == 0);
        CHECK(file_lines(path) == 4);
        snprintf(path, sizeof path, "%s/clh%d.csv", dir, mag);
        write_csv_centerline(path, &f, d, x, y, nx, ny, PROFILE_HORIZONTAL);
        CHECK(file_lines(path) == (long)nx + 1);
        snprintf(path, sizeof path, "%s/clv%d.csv", dir, mag);
        write_csv_centerline(path, &f, mag ? d : NULL, x, y, nx, ny, PROFILE_VERTICAL);
        CHECK(file_lines(path) == (long)ny + 1);
    }
    write_csv_centerline(NULL, &f, d, x, y, nx, ny, PROFILE_VERTICAL);
    write_csv_statistics(path, 0, 0.0, &f, NULL, nx, ny, 1);
    derived_fields_clear(d);
    CHECK(!d->velocity_magnitude && !d->stats_computed);
    derived_fields_destroy(d);
    derived_fields_destroy(NULL);
    derived_fields_clear(NULL);
    for (int q = 0; q < 6; q++) free(arr[q]);
    free(x);
    free(y);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    CHECK(run(argv[1], 17, 13, 11, 1) == 0);
    CHECK(run(argv[1], 9, 6, 1, 0) == 0);
    CHECK(run(argv[1], 2, 2, 1, 1) == 0);
    printf("ok\n");
    return 0;
}
