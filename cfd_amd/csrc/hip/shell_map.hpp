// shell_map.hpp -- the packed layout of the resident mode's boundary-shell
// transfers (shell_io.hip) and the host code that walks it: the map both
// sides index with, the threaded gather / scatter over caller arrays, the
// threaded maximum and the guard's hashes. C++17 standard library only, no
// HIP header: shell_io.hip includes it for the kernel and the ctx_* entry
// points, and a host compiler builds it alone (tests/native/shell_map_check.cpp,
// driven by tests/test_shell_cases.py under ASan + UBSan and under TSan).
//
// Shell of depth D, in the packed order both sides use: for each z plane k,
// for each row j, the row's shell cells in x order. A row is whole (nx cells)
// when k < D or k >= nz-D (3-D) or j < D or j >= ny-D; otherwise it holds its
// first D and last D cells. Fields follow each other in the staging buffer.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <thread>
#include <vector>

#ifdef __HIPCC__
#define CFD_SHELL_HD __host__ __device__
#else
#define CFD_SHELL_HD
#endif

// An unnamed namespace, as the kernel's unit had it: ShellMap is a kernel
// parameter, so its name is part of k_shell_io's symbols, and every function
// here is local to the unit that includes the header.
namespace {

struct ShellMap {
    long long nx, ny, nz;
    int D;
    long long fp, pp;  // cells of a whole plane / of a plane with only x,y shell rows

    CFD_SHELL_HD bool whole_plane(long long k) const {
        return nz > 1 && (k < D || k >= nz - D);
    }
    CFD_SHELL_HD static long long clampll(long long v, long long lo, long long hi) {
        return v < lo ? lo : (v > hi ? hi : v);
    }
    CFD_SHELL_HD long long plane_off(long long k) const {
        if (nz == 1) return 0;
        const long long whole = (k < D ? k : D) + (k > nz - D ? k - (nz - D) : 0);
        return whole * fp + clampll(k - D, 0, nz - 2 * D) * pp;
    }
    CFD_SHELL_HD long long total() const {
        return nz == 1 ? pp : 2LL * D * fp + (nz - 2LL * D) * pp;
    }
    // packed offset of row (j, k) within one field; *whole = row stored whole
    CFD_SHELL_HD long long row_off(long long j, long long k, bool* whole) const {
        const long long o = plane_off(k);
        if (whole_plane(k)) {
            *whole = true;
            return o + j * nx;
        }
        *whole = (j < D || j >= ny - D);
        const long long wr = (j < D ? j : D) + (j > ny - D ? j - (ny - D) : 0);
        return o + wr * nx + clampll(j - D, 0, ny - 2 * D) * (2LL * D);
    }
};

// every extent > 2 D (ctx_shell_fits); nz = 1: a 2-D field
inline ShellMap make_map(long long nx, long long ny, long long nz, int D) {
    ShellMap m;
    m.nx = nx;
    m.ny = ny;
    m.nz = nz;
    m.D = D;
    m.fp = m.nx * m.ny;
    m.pp = 2LL * D * m.nx + (m.ny - 2LL * D) * (2LL * D);
    return m;
}

// Threads of the host walks before their own limits: at most 16 of the
// machine's, or the override (CFD_HIP_SHELL_THREADS, 0: unset) in their place.
inline int shell_base_threads(int env_override, unsigned hardware_threads) {
    int nt = (int)std::min<unsigned>(hardware_threads ? hardware_threads : 1, 16);
    if (env_override > 0) nt = env_override;
    return nt;
}

// Threads host_rows splits `cells` staged cells over: one below 2^18 cells,
// whatever the override says.
inline int shell_thread_count(long long cells, int env_override, unsigned hardware_threads) {
    if (cells < (1LL << 18)) return 1;
    return shell_base_threads(env_override, hardware_threads);
}

// Host side of the layout over caller arrays (nx*ny*nz, packed), split over
// nt threads by rows: the partial rows touch two cache lines each, 4 KB or
// more apart, which one core walks at a fraction of the copy rate.
inline void host_rows(const ShellMap& m, int nf, double* const* host, double* buf, bool gather,
                      int nt) {
    const long long nrows = m.ny * m.nz * nf;
    const long long total = m.total();
    auto work = [&](long long r0, long long r1) {
        for (long long row = r0; row < r1; ++row) {
            const int fi = (int)(row / (m.ny * m.nz));
            const long long r = row - fi * m.ny * m.nz;
            const long long k = r / m.ny, j = r - k * m.ny;
            bool whole;
            double* b = buf + fi * total + m.row_off(j, k, &whole);
            double* h = host[fi] + (k * m.ny + j) * m.nx;
            if (whole) {
                if (gather) memcpy(b, h, m.nx * sizeof(double));
                else memcpy(h, b, m.nx * sizeof(double));
            } else {
                const long long tail = m.nx - m.D;
                if (gather) {
                    memcpy(b, h, m.D * sizeof(double));
                    memcpy(b + m.D, h + tail, m.D * sizeof(double));
                } else {
                    memcpy(h, b, m.D * sizeof(double));
                    memcpy(h + tail, b + m.D, m.D * sizeof(double));
                }
            }
        }
    };
    if (nt <= 1) {
        work(0, nrows);
        return;
    }
    std::vector<std::thread> th;
    th.reserve(nt);
    for (int t = 0; t < nt; ++t) {
        const long long r0 = nrows * t / nt, r1 = nrows * (t + 1) / nt;
        try {
            th.emplace_back(work, r0, r1);
        } catch (...) {  // no thread: this share on the caller's (C ABI)
            work(r0, r1);
        }
    }
    for (auto& t : th) t.join();
}

// Threads host_max splits n cells over: up to 16, one below 2^20 cells.
inline int host_max_thread_count(size_t n, unsigned hardware_threads) {
    if (n < (1u << 20)) return 1;
    return (int)std::min<unsigned>(hardware_threads ? hardware_threads : 1, 16);
}

// compute_max_temperature (solver_registry.c:52-62) over a host array with
// the reference's sequential semantics, m = T[0]; m = T[i] if T[i] > m, split
// over nt chunks (one thread each): each chunk's maximum from -inf with the
// same strict comparison (its first occurrence; NaNs never compare greater),
// combined in chunk order with that comparison, so the result is the
// sequential loop's bit for bit (a NaN T[0] stays; -0.0 / +0.0 keep the
// earlier one).
inline double host_max(const double* T, size_t n, int nt) {
    if (n == 0) return 0.0;
    if (nt < 1) nt = 1;
    std::vector<double> part(nt, -INFINITY);
    auto work = [&](int t) {
        const size_t a = 1 + (n - 1) * (size_t)t / (size_t)nt;
        const size_t b = 1 + (n - 1) * (size_t)(t + 1) / (size_t)nt;
        double m = -INFINITY;
        for (size_t i = a; i < b; ++i)
            if (T[i] > m) m = T[i];
        part[t] = m;
    };
    if (nt == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        th.reserve(nt);
        for (int t = 0; t < nt; ++t) {
            try {
                th.emplace_back(work, t);
            } catch (...) {  // no thread: this share on the caller's (C ABI)
                work(t);
            }
        }
        for (auto& t : th) t.join();
    }
    double m = T[0];
    for (double v : part)
        if (v > m) m = v;
    return m;
}

// Resident-mode guard (hip_proj_config_t.dirty_verify_interval): hashes of
// the host arrays' cells inside the outer layer (the layer a caller's BC
// routine writes), in two parts: the deep interior (every index in
// [2, n-3]; the resident steps never write it on the host, so its hash holds
// until a full download) and layer 1 (the cells next to the boundary, which
// every step's depth-2 shell download rewrites, so its hash is retaken after
// each step; shell-sized). Each cell contributes mix(bits) * (2 idx + 1), so
// a sum is order-independent (summed per plane range over threads) and
// changes when any value changes or two values swap. nt: shell_base_threads;
// layer 1 takes at most 4 of them, and no part more than it has planes.
inline void host_hash(long long nx, long long ny, long long nz, const double* const* host, int nf,
                      bool layer1, int nt, unsigned long long* out) {
    const bool is3d = nz > 1;
    const long long k0 = is3d ? 1 : 0, k1 = is3d ? nz - 1 : 1;
    const long long planes = k1 - k0;
    if (layer1) nt = std::min(nt, 4);
    nt = (int)std::max(1LL, std::min<long long>(nt, planes));
    auto mix = [](const double* p, long long idx) {
        unsigned long long b;
        memcpy(&b, p, sizeof(b));
        b ^= b >> 31;
        b *= 0x9E3779B97F4A7C15ull;
        return b * (unsigned long long)(2 * idx + 1);
    };
    for (int f = 0; f < nf; ++f) {
        std::vector<unsigned long long> part(nt, 0ull);
        auto work = [&](int t) {
            unsigned long long h = 0;
            for (long long k = k0 + planes * t / nt; k < k0 + planes * (t + 1) / nt; ++k) {
                const bool kedge = is3d && (k == 1 || k == nz - 2);
                for (long long j = 1; j < ny - 1; ++j) {
                    const long long row = (k * ny + j) * nx;
                    const bool edge_row = kedge || j == 1 || j == ny - 2;
                    if (!layer1) {
                        if (edge_row) continue;
                        for (long long i = 2; i < nx - 2; ++i) h += mix(host[f] + row + i, row + i);
                    } else if (edge_row) {
                        for (long long i = 1; i < nx - 1; ++i) h += mix(host[f] + row + i, row + i);
                    } else {
                        h += mix(host[f] + row + 1, row + 1);
                        h += mix(host[f] + row + nx - 2, row + nx - 2);
                    }
                }
            }
            part[t] = h;
        };
        if (nt == 1) {
            work(0);
        } else {
            // reached from extern "C" entry points: a thread that cannot be
            // created (std::system_error) must not cross the C ABI, so its
            // share runs on this thread instead (the sum is order-free)
            std::vector<std::thread> th;
            th.reserve(nt);
            for (int t = 0; t < nt; ++t) {
                try {
                    th.emplace_back(work, t);
                } catch (...) {
                    work(t);
                }
            }
            for (auto& t : th) t.join();
        }
        unsigned long long h = 0;
        for (auto v : part) h += v;
        out[f] = h;
    }
}

}  // namespace
