/* CPU check of the divc() correction in cfd_amd/csrc/hip/device_util.hpp:
 * q = RN(a * RN(1/d)), q' = RN(q + RN(a - q d) * RN(1/d)) (two FMAs) against
 * the correctly rounded a / d, bit for bit, for the divisors dx^2 of grids of
 * n = 17 .. 1025 points on domains of length 1, 2*pi and 0.5, over random a
 * of either sign with exponents in [-60, 60] (2e7 quotients per divisor).
 *   gcc -O2 -ffp-contract=off -o /tmp/divc_check tools/divc_check.c -lm && /tmp/divc_check
 * Optional argv[1]: quotients per divisor. Prints the number of mismatches
 * (0 expected) and exits 1 on any.
 *
 * Second mode, `divc_check divz [quotients per divisor and operand family]`:
 * restates divz and the deferred form (DivFastZ's lane flag, then DivExact on
 * the lanes whose flag dropped) next to divc and checks all three bit for bit
 * against `/` (every NaN one class), for the divisors 2 h and h^2 of the
 * spacings h = L / (n - 1), L = 1 and 0.7, of every extent n that
 * tests/cg_seam_shapes.py, tests/rb2_shapes.py, tests/special_values.py and
 * tests/test_gpu_rb_variants.py use in x or y, of the 512^3 unit cube and of
 * 1024 x 1024 x 512. Operands: random bit patterns (the whole exponent range,
 * NaNs and infinities included), random values within +-4 binades of the
 * operand that puts the quotient on either threshold (2^-900, 2^900),
 * subnormals, and +-0, +-inf, NaN, +-DBL_MIN, +-DBL_MAX, +-2^-1074. It also
 * checks the two claims the thresholds rest on: where the range test passes
 * the inner residual fma(q, d, -a) is zero or normal, so it did not underflow
 * (compared with the 113-bit product), and wherever the fast value is not
 * `/`'s the flag has dropped (and it drops only for quotients outside
 * [2^-899, 2^899]).
 * Prints its own summary line and exits 1 on any mismatch. */
#include <stdlib.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static uint64_t s = 88172645463325252ull;
static inline uint64_t xorshift(void) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

/* ---- the second mode ---- */
static double bits2d(uint64_t b) { double a; memcpy(&a, &b, 8); return a; }
static int same(double x, double y) {  /* bitwise, every NaN one class */
    if (isnan(x) || isnan(y)) return isnan(x) && isnan(y);
    return memcmp(&x, &y, 8) == 0;
}
static double divc_(double a, double d, double r) {
    const double q = a * r;
    const double aq = fabs(q);
    if (!(aq >= 0x1p-900 && aq <= 0x1p+900)) return a / d;
    return fma(fma(-q, d, a), r, q);
}
static double divz_(double a, double d, double r) {
    const double q = a * r;
    const double aq = fabs(q);
    if (!(aq <= 0x1p+900 && (aq >= 0x1p-900 || aq == 0.0))) return a / d;
    return fma(-fma(q, d, -a), r, q);
}
static double divfastz_(double a, double d, double r, int* ok) {
    const double q = a * r;
    const double aq = fabs(q);
    *ok &= (aq <= 0x1p+900) & ((aq >= 0x1p-900) | (aq == 0.0));
    return fma(-fma(q, d, -a), r, q);
}

static long z_tot, z_rounded, z_bad[5];  /* divc, divz, deferred, residual, flag */
static const char* z_name[5] = {"divc", "divz", "deferred", "residual", "flag"};
static void z_fail(int what, double a, double d, double got, double want) {
    if (z_bad[what]++ < 3) printf("mismatch %s a=%a d=%a got=%a want=%a\n", z_name[what], a, d, got, want);
}
static void z_one(double a, double d, double r) {
    const double ex = a / d;
    z_tot++;
    const double c = divc_(a, d, r);
    if (!same(c, ex)) z_fail(0, a, d, c, ex);
    const double z = divz_(a, d, r);
    if (!same(z, ex)) z_fail(1, a, d, z, ex);
    int ok = 1;
    const double f = divfastz_(a, d, r, &ok);
    const double sel = ok ? f : a / d;  /* the caller's recompute with DivExact */
    if (!same(sel, ex)) z_fail(2, a, d, sel, ex);
    if (ok) {  /* the residual is zero or normal: it cannot have underflowed */
        const double q = a * r;
        const double e = fma(q, d, -a);
        const __float128 e128 = (__float128)q * (__float128)d - (__float128)a;
        const __float128 ae = e128 < 0 ? -e128 : e128;
        if (e != (double)e128 || (ae != 0 && ae < (__float128)0x1p-1022)) z_fail(3, a, d, e, (double)e128);
        /* q = RN(a RN(1/d)) can be 1.5 ulp from a / d, so the residual can
         * need a 54th bit; counted, the corrected quotient is `/`'s all the same */
        if ((__float128)e != e128) z_rounded++;
    } else if (isfinite(a) && a != 0.0) {
        /* the flag dropped for its reason: the quotient is outside the range */
        const double aq = fabs(ex);
        if (aq >= 0x1p-899 && aq <= 0x1p+899) z_fail(4, a, d, f, ex);
    }
}

static int divz_mode(long per) {
    const int ns[] = {4, 5, 14, 15, 16, 17, 18, 20, 21, 27, 28, 29, 30, 31, 33, 37, 41, 50, 53,
                      54, 57, 58, 59, 60, 61, 62, 63, 70, 82, 101, 102, 117, 118, 121, 122, 123,
                      126, 127, 128, 129, 130, 131, 178, 249, 250, 255, 512, 1024};
    const double lens[] = {1.0, 0.7};
    const double special[] = {0.0, -0.0, INFINITY, -INFINITY, NAN, 0x1p-1022, -0x1p-1022,
                              0x1.fffffffffffffp+1023, -0x1.fffffffffffffp+1023, 0x1p-1074,
                              -0x1p-1074, 0x1p-900, 0x1p+900, -0x1p-900, -0x1p+900};
    int ndiv = 0;
    for (size_t t = 0; t < sizeof ns / sizeof ns[0]; t++)
        for (int dom = 0; dom < 2; dom++) {
            const double h = lens[dom] / (ns[t] - 1);
            const double ds[2] = {2.0 * h, h * h};
            for (int w = 0; w < 2; w++, ndiv++) {
                const double d = ds[w], r = 1.0 / d;
                for (size_t n = 0; n < sizeof special / sizeof special[0]; n++) {
                    z_one(special[n], d, r);
                    z_one(special[n] * d, d, r);  /* quotients on the thresholds themselves */
                }
                for (long n = 0; n < per; n++) {
                    z_one(bits2d(xorshift()), d, r);  /* any bit pattern */
                    for (int th = 0; th < 2; th++) {  /* +-4 binades of either threshold */
                        const uint64_t b = xorshift();
                        const double m = bits2d((b & 0x000FFFFFFFFFFFFFull) | (1023ull << 52) |
                                                (b & 0x8000000000000000ull));
                        const int e = (th ? 900 : -900) - 4 + (int)((b >> 52) % 9);
                        z_one(ldexp(m, e) * d, d, r);
                    }
                    if (n % 4 == 0)  /* subnormal operands */
                        z_one(bits2d(xorshift() & 0x800FFFFFFFFFFFFFull), d, r);
                }
            }
        }
    long bad = 0;
    for (int w = 0; w < 5; w++) bad += z_bad[w];
    printf("divz_check: %ld quotients, %d divisors, %ld mismatches (divc %ld, divz %ld, "
           "deferred %ld, residual %ld, flag %ld); %ld residuals rounded\n", z_tot, ndiv, bad,
           z_bad[0], z_bad[1], z_bad[2], z_bad[3], z_bad[4], z_rounded);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "divz") == 0)
        return divz_mode(argc > 2 ? atol(argv[2]) : 1000000);
    const long per = argc > 1 ? atol(argv[1]) : 20000000;
    const int ns[] = {17, 24, 32, 33, 41, 64, 65, 100, 128, 129, 256, 257, 512, 1000, 1024, 1025};
    const double lens[] = {1.0, 2.0 * M_PI, 0.5};
    long bad = 0, tot = 0;
    for (size_t t = 0; t < sizeof ns / sizeof ns[0]; t++) {
        for (int dom = 0; dom < 3; dom++) {
            const double dx = lens[dom] / (ns[t] - 1);
            const double d = dx * dx, r = 1.0 / d;
            for (long n = 0; n < per; n++) {
                const uint64_t b = xorshift();
                const uint64_t e = 1023 - 60 + (b >> 52) % 121;
                const uint64_t bits = (b & 0x000FFFFFFFFFFFFFull) | (e << 52) | ((xorshift() & 1) << 63);
                double a;
                memcpy(&a, &bits, 8);
                const double q = a * r;
                const double q1 = fma(fma(-q, d, a), r, q);
                const double ex = a / d;
                if (memcmp(&q1, &ex, 8) != 0) {
                    if (bad < 5) printf("mismatch n=%d L=%g a=%a got=%a want=%a\n", ns[t], lens[dom], a, q1, ex);
                    bad++;
                }
                tot++;
            }
        }
    }
    printf("divc_check: %ld quotients, %ld mismatches\n", tot, bad);
    return bad ? 1 : 0;
}
