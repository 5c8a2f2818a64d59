/*
 * dst_tables.h -- the host tables of the direct transform pressure solvers
 * (hip/transform_solve.hpp). Sine: the type-I sine matrix S_n and the
 * eigenvalues of the 1-D second difference with zero Dirichlet ends, for n
 * interior points; further down, the cosine tables.
 * Shared by the device library and by host-only drivers that run the builders
 * under AddressSanitizer (tests/test_dst_cases.py, tests/test_dct_cases.py).
 *
 *   S_n[a][b] = sin(pi (a + 1)(b + 1) / (n + 1)),  a, b = 0 .. n - 1
 *   e_n[a]    = 4 sin^2(pi (a + 1) / (2 (n + 1)))   (lambda_n[a] = e_n[a] / h^2)
 *
 * Both are evaluated in long double and rounded once to double. The sine's
 * argument is reduced as an integer, (a + 1)(b + 1) mod 2 (n + 1), and folded
 * into the first quadrant, so an entry's error does not grow with a b.
 */
#ifndef CFD_HIP_DST_TABLES_H
#define CFD_HIP_DST_TABLES_H

#include <math.h>
#include <stddef.h>

#define DST_PI_L 3.14159265358979323846264338327950288L

/* rows and columns of the table the kernels read: n rounded up to their
 * 64-row tile, the rest zero, so that a tile's table loads need no mask */
static inline size_t dst_table_pitch(size_t n) { return (n + 63) / 64 * 64; }

/* sin(pi m / N) for integers 0 <= m < 2 N */
static inline long double dst_sin_ratio(unsigned long long m, unsigned long long N) {
    int neg = 0;
    if (m >= N) {
        m -= N;
        neg = 1;
    }
    if (2 * m > N) m = N - m; /* sin(pi - t) = sin(t) */
    const long double s = sinl(DST_PI_L * (long double)m / (long double)N);
    return neg ? -s : s;
}

/* table[pitch * pitch], pitch = dst_table_pitch(n): S_n in the leading n x n
 * block, zero elsewhere */
static inline void dst_fill_sine_table(size_t n, double* table) {
    const size_t np = dst_table_pitch(n);
    const unsigned long long N = (unsigned long long)n + 1;
    for (size_t a = 0; a < np; a++)
        for (size_t b = 0; b < np; b++) {
            double v = 0.0;
            if (a < n && b < n) {
                const unsigned long long m =
                    ((unsigned long long)(a + 1) * (unsigned long long)(b + 1)) % (2 * N);
                v = (double)dst_sin_ratio(m, N);
            }
            table[a * np + b] = v;
        }
}

/* eig[n]: e_n */
static inline void dst_fill_eigenvalues(size_t n, double* eig) {
    const unsigned long long N2 = 2 * ((unsigned long long)n + 1);
    for (size_t a = 0; a < n; a++) {
        const long double s = dst_sin_ratio((unsigned long long)a + 1, N2);
        eig[a] = (double)(4.0L * s * s);
    }
}

/*
 * The tables of the direct cosine-transform solve (hip/transform_solve.hpp): the
 * orthonormal type-II cosine matrix Q_n and the eigenvalues of the 1-D second
 * difference with Neumann (mirror) ends on n cell centres.
 *
 *   Q_n[a][b] = w_a cos(pi a (2 b + 1) / (2 n)),  w_0 = sqrt(1 / n), w_a = sqrt(2 / n)
 *   e_n[a]    = 4 sin^2(pi a / (2 n))             (lambda_n[a] = e_n[a] / h^2, e_n[0] = 0)
 *
 * The cosine's argument is reduced as an integer, a (2 b + 1) mod 4 n, and
 * folded into the first quadrant. Q_n is not symmetric. The transform passes
 * compute out[a] = sum_b T[b][a] in[b], so the forward transform Q takes the
 * table Q^T and the inverse Q^T takes Q: both are filled, from one rounding.
 */

/* cos(pi m / (2 n)) for integers 0 <= m < 4 n */
static inline long double dct_cos_ratio(unsigned long long m, unsigned long long n) {
    int neg = 0;
    if (m > 2 * n) m = 4 * n - m; /* cos(2 pi - t) = cos(t) */
    if (m > n) {                  /* cos(pi - t) = -cos(t) */
        m = 2 * n - m;
        neg = 1;
    }
    long double c;
    if (m == n) c = 0.0L;
    else if (2 * m > n) c = sinl(DST_PI_L * (long double)(n - m) / (long double)(2 * n));
    else c = cosl(DST_PI_L * (long double)m / (long double)(2 * n));
    return neg ? -c : c;
}

/* q and qt [pitch * pitch], pitch = dst_table_pitch(n): Q_n and its transpose
 * in the leading n x n block, zero elsewhere */
static inline void dct_fill_cos_tables(size_t n, double* q, double* qt) {
    const size_t np = dst_table_pitch(n);
    const long double w0 = sqrtl(1.0L / (long double)n), w1 = sqrtl(2.0L / (long double)n);
    for (size_t a = 0; a < np; a++)
        for (size_t b = 0; b < np; b++) {
            double v = 0.0;
            if (a < n && b < n) {
                const unsigned long long m =
                    ((unsigned long long)a * (2 * (unsigned long long)b + 1)) %
                    (4 * (unsigned long long)n);
                v = (double)((a == 0 ? w0 : w1) * dct_cos_ratio(m, (unsigned long long)n));
            }
            q[a * np + b] = v;
            qt[b * np + a] = v;
        }
}

/* eig[n]: e_n of the cosine transform (eig[0] is exactly 0) */
static inline void dct_fill_eigenvalues(size_t n, double* eig) {
    const unsigned long long N2 = 2 * (unsigned long long)n;
    for (size_t a = 0; a < n; a++) {
        const long double s = dst_sin_ratio((unsigned long long)a, N2);
        eig[a] = (double)(4.0L * s * s);
    }
}

#endif
