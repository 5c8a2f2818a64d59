// shell_map_check -- the resident mode's packed shell layout and its host code
// (cfd_amd/csrc/hip/shell_map.hpp) on their own. No GPU, no HIP:
// tests/test_shell_cases.py builds it with g++ once under ASan + UBSan and once
// under TSan, runs it directly and compares what it writes with a numpy model.
//
// usage: shell_map_check OUTDIR SMALL_CELLS NXxNYxNZ...
//
// For every shape and depth D = 1, 2 it writes OUTDIR/order_NXxNYxNZ_D.bin:
// int64[total()], the linear index (k ny + j) nx + i of the cell that
// host_rows gathers to each packed offset (-1: no cell), taken from a
// one-thread, one-field gather of an array that holds its own indices. The
// buffer has exactly total() cells, so a write past it is the sanitizer's.
// Against that order it checks itself, for 1, 2, 3, 7 and 16 threads and 1, 4
// and 5 fields: gather puts field f's cell at f total + offset; scatter into
// arrays of sentinels writes exactly those cells and leaves every other
// cell's bits alone.
// For shapes of at most SMALL_CELLS cells it writes OUTDIR/cover_NXxNYxNZ.bin:
// uint8 per cell, bit 0 / bit 1 set when flipping one bit of that cell alone
// changes host_hash's deep / layer-1 part; and checks that swapping
// neighbouring covered cells changes the part. For every shape: the hashes
// do not depend on the thread count.
// host_max against the sequential loop, and one `threads CELLS ENV HW N` line
// per shell_thread_count probe, follow. The last line is SHELL_MAP_OK; a
// failed check prints to stderr and exits 1.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>

#include "shell_map.hpp"

static const int THREADS[] = {1, 2, 3, 7, 16};
static const int FIELD_COUNTS[] = {1, 4, 5};

[[noreturn]] static void fail(const std::string& what) {
    fprintf(stderr, "shell_map_check: %s\n", what.c_str());
    exit(1);
}

static uint64_t bits(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof(b));
    return b;
}

static void write_file(const std::string& path, const void* data, size_t bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(data, 1, bytes, f) != bytes || fclose(f) != 0) fail("cannot write " + path);
}

static double field_value(int f, long long cell) { return (double)(((long long)f << 40) + cell); }
static double sentinel(int f, long long cell) { return -field_value(f, cell) - 0.5; }

// gather and scatter of nf fields on nt threads against the packed order
static void check_rows(const std::string& tag, const ShellMap& m, const std::vector<long long>& order,
                       int nf, int nt) {
    const long long cells = m.nx * m.ny * m.nz, total = m.total();
    const std::string id = tag + " nf " + std::to_string(nf) + " nt " + std::to_string(nt);
    std::vector<std::vector<double>> arr(nf, std::vector<double>((size_t)cells));
    std::vector<double*> ptr(nf);
    for (int f = 0; f < nf; ++f) {
        for (long long c = 0; c < cells; ++c) arr[f][c] = field_value(f, c);
        ptr[f] = arr[f].data();
    }
    std::vector<double> buf((size_t)(total * nf), -1.0);
    host_rows(m, nf, ptr.data(), buf.data(), true, nt);
    for (int f = 0; f < nf; ++f)
        for (long long o = 0; o < total; ++o)
            if (bits(buf[f * total + o]) != bits(field_value(f, order[o])))
                fail(id + ": gather, field " + std::to_string(f) + " offset " + std::to_string(o));
    // scatter: the staged values are the cells' own, negated; the rest sentinels
    std::vector<char> staged((size_t)cells, 0);
    for (long long o = 0; o < total; ++o) staged[order[o]] = 1;
    for (int f = 0; f < nf; ++f) {
        for (long long c = 0; c < cells; ++c) arr[f][c] = sentinel(f, c);
        for (long long o = 0; o < total; ++o) buf[f * total + o] = -field_value(f, order[o]);
    }
    buf[0] = -0.0;  // field 0, first cell: a signed zero travels as bits
    host_rows(m, nf, ptr.data(), buf.data(), false, nt);
    for (int f = 0; f < nf; ++f)
        for (long long c = 0; c < cells; ++c) {
            double want = staged[c] ? -field_value(f, c) : sentinel(f, c);
            if (f == 0 && c == order[0]) want = -0.0;
            if (bits(arr[f][c]) != bits(want))
                fail(id + ": scatter, field " + std::to_string(f) + " cell " + std::to_string(c));
        }
}

static void check_shape(const std::string& outdir, long long small, long long nx, long long ny,
                        long long nz) {
    const std::string sid =
        std::to_string(nx) + "x" + std::to_string(ny) + "x" + std::to_string(nz);
    const long long cells = nx * ny * nz;
    for (int D = 1; D <= 2; ++D) {
        const ShellMap m = make_map(nx, ny, nz, D);
        const long long total = m.total();
        if (total <= 0 || total > cells) fail(sid + ": total() out of range");
        std::vector<double> self((size_t)cells);
        for (long long c = 0; c < cells; ++c) self[c] = (double)c;
        double* one[1] = {self.data()};
        std::vector<double> buf((size_t)total, -1.0);
        host_rows(m, 1, one, buf.data(), true, 1);
        std::vector<long long> order((size_t)total);
        for (long long o = 0; o < total; ++o) {
            order[o] = (long long)buf[o];
            if (order[o] < 0 || order[o] >= cells)
                fail(sid + " D " + std::to_string(D) + ": offset " + std::to_string(o) + " not written");
        }
        write_file(outdir + "/order_" + sid + "_" + std::to_string(D) + ".bin", order.data(),
                   order.size() * sizeof(long long));
        for (int nf : FIELD_COUNTS)
            for (int nt : THREADS) check_rows(sid + " D " + std::to_string(D), m, order, nf, nt);
    }

    // the guard's hashes: five fields of random bits' worth of values
    const int nf = 5;
    std::mt19937_64 rng(12345 + (uint64_t)cells);
    std::uniform_real_distribution<double> uni(-1.0, 1.0);
    std::vector<std::vector<double>> arr(nf, std::vector<double>((size_t)cells));
    std::vector<const double*> ptr(nf);
    for (int f = 0; f < nf; ++f) {
        for (double& v : arr[f]) v = uni(rng);
        ptr[f] = arr[f].data();
    }
    unsigned long long base[2][5], h[5];
    for (int part = 0; part < 2; ++part) {
        host_hash(nx, ny, nz, ptr.data(), nf, part == 1, 1, base[part]);
        for (int nt : THREADS) {
            host_hash(nx, ny, nz, ptr.data(), nf, part == 1, nt, h);
            for (int f = 0; f < nf; ++f)
                if (h[f] != base[part][f])
                    fail(sid + ": hash part " + std::to_string(part) + " depends on the thread count " +
                         std::to_string(nt));
        }
    }
    if (cells > small) return;
    // coverage, on field 2 with three threads: flip one bit of one cell
    const int f = 2;
    const double* onef[1] = {arr[f].data()};
    std::vector<uint8_t> cover((size_t)cells, 0);
    for (long long c = 0; c < cells; ++c) {
        const double keep = arr[f][c];
        for (uint64_t flip : {1ull, 1ull << 63}) {
            const uint64_t b = bits(keep) ^ flip;
            memcpy(&arr[f][c], &b, sizeof(b));
            uint8_t got = 0;
            for (int part = 0; part < 2; ++part) {
                host_hash(nx, ny, nz, onef, 1, part == 1, 3, h);
                if (h[0] != base[part][f]) got |= (uint8_t)(1 << part);
            }
            if (flip == 1ull) cover[c] = got;
            else if (got != cover[c]) fail(sid + ": sign flip and low-bit flip disagree");
        }
        arr[f][c] = keep;
    }
    write_file(outdir + "/cover_" + sid + ".bin", cover.data(), cover.size());
    // swapping two unequal cells of a part changes it: each covered cell with
    // the next one of its part
    for (int part = 0; part < 2; ++part) {
        long long prev = -1;
        for (long long c = 0; c < cells; ++c) {
            if (!(cover[c] & (1 << part))) continue;
            if (prev >= 0 && bits(arr[f][prev]) != bits(arr[f][c])) {
                std::swap(arr[f][prev], arr[f][c]);
                host_hash(nx, ny, nz, onef, 1, part == 1, 2, h);
                if (h[0] == base[part][f])
                    fail(sid + ": swapping cells " + std::to_string(prev) + " and " +
                         std::to_string(c) + " keeps the hash of part " + std::to_string(part));
                std::swap(arr[f][prev], arr[f][c]);
            }
            prev = c;
        }
    }
}

static double seq_max(const double* T, size_t n) {
    double m = T[0];
    for (size_t i = 1; i < n; ++i)
        if (T[i] > m) m = T[i];
    return m;
}

static void expect_max(const std::string& what, const std::vector<double>& T) {
    const double want = seq_max(T.data(), T.size());
    for (int nt : THREADS) {
        const double got = host_max(T.data(), T.size(), nt);
        if (bits(got) != bits(want)) fail("host_max " + what + ", " + std::to_string(nt) + " threads");
    }
    const double got =
        host_max(T.data(), T.size(), host_max_thread_count(T.size(), 16));
    if (bits(got) != bits(want)) fail("host_max " + what + ", its own thread count");
}

static void check_max() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> uni(250.0, 350.0);
    const size_t big = (1u << 20) + 4321;  // above the threshold: 16 chunks
    if (host_max_thread_count(big, 64) != 16 || host_max_thread_count(big, 0) != 1 ||
        host_max_thread_count(big, 5) != 5 || host_max_thread_count((1u << 20) - 1, 64) != 1 ||
        host_max_thread_count(1u << 20, 64) != 16)
        fail("host_max_thread_count");
    std::vector<double> T(big);
    for (double& v : T) v = uni(rng);
    expect_max("random", T);
    {
        std::vector<double> A = T;
        A[0] = nan;
        expect_max("NaN first", A);
        A[0] = 400.0;  // T[0] itself the maximum
        expect_max("maximum at index 0", A);
    }
    {
        std::vector<double> A = T;
        for (size_t i = 1; i < A.size(); i += 1009) A[i] = nan;
        A[A.size() - 1] = nan;
        expect_max("NaNs elsewhere", A);
    }
    // the maximum in the first and in the last cell of every chunk of 7 and of
    // 16 (chunk t is [1 + (n-1) t / nt, 1 + (n-1) (t+1) / nt)), on a short and
    // on the long array
    for (size_t n : {(size_t)1000, big})
        for (size_t nt : {(size_t)7, (size_t)16})
            for (size_t t = 0; t < nt; ++t)
                for (int last = 0; last < 2; ++last) {
                    if (n == big && t % 5 != 0 && t + 1 != nt) continue;  // a few chunks of the long one
                    std::vector<double> A(T.begin(), T.begin() + n);
                    const size_t a = 1 + (n - 1) * t / nt, b = 1 + (n - 1) * (t + 1) / nt;
                    A[last ? b - 1 : a] = 500.0;
                    expect_max("chunk edge", A);
                }
    // ties of -0.0 and +0.0: the earlier one stays, at index 0, inside a
    // chunk and across chunks
    for (size_t n : {(size_t)2, (size_t)64, (size_t)1000})
        for (int first_negative = 0; first_negative < 2; ++first_negative)
            for (size_t at : {(size_t)0, n / 3}) {
                std::vector<double> A(n, -1.0);
                const double z0 = first_negative ? -0.0 : 0.0;
                A[at] = z0;
                for (size_t i = at + 1; i < n; i += 2) A[i] = -z0;
                for (size_t i = at + 2; i < n; i += 2) A[i] = z0;
                expect_max("signed zeros", A);
                if (bits(seq_max(A.data(), n)) != bits(z0)) fail("the sequential loop's own tie");
            }
    expect_max("n = 1", std::vector<double>(1, -3.5));
    expect_max("n = 1, NaN", std::vector<double>(1, nan));
    expect_max("all NaN", std::vector<double>(50, nan));
    expect_max("-inf", std::vector<double>(50, -INFINITY));
    if (host_max(nullptr, 0, 4) != 0.0) fail("host_max n = 0");
}

int main(int argc, char** argv) {
    if (argc < 3) fail("usage: shell_map_check OUTDIR SMALL_CELLS NXxNYxNZ...");
    const std::string outdir = argv[1];
    const long long small = atoll(argv[2]);
    for (int a = 3; a < argc; ++a) {
        long long nx, ny, nz;
        if (sscanf(argv[a], "%lldx%lldx%lld", &nx, &ny, &nz) != 3) fail(std::string("shape ") + argv[a]);
        check_shape(outdir, small, nx, ny, nz);
    }
    check_max();
    const long long edge = 1LL << 18;
    for (long long cells : {1LL, edge - 1, edge, edge + 1})
        for (int env : {0, 1, 3, 40})
            for (unsigned hw : {0u, 1u, 8u, 16u, 17u, 256u})
                printf("threads %lld %d %u %d\n", cells, env, hw, shell_thread_count(cells, env, hw));
    printf("SHELL_MAP_OK\n");
    return 0;
}
