// shell_io.hip -- boundary-shell transfers of the host-buffer step's resident
// mode (hip_proj_config_t.dirty_faces, SURVEY.md:449-455).
//
// Between two `step` calls a reference driver changes only boundary cells of
// its host flow_field (lid / periodic / Neumann BCs, lid_driven_cavity_common.h:306-308,
// taylor_green_3d_reference.h:297-313), and reads only the boundary layer and
// the layer next to it (what those BC routines read). In the resident mode the
// interior stays in HBM: a step uploads the depth-1 shell of u, v, w, p (T)
// and downloads the depth-2 shell, instead of whole fields.
//
// The packed layout (ShellMap), the threaded host gather / scatter over it,
// the host maximum and the guard's hashes are shell_map.hpp, which a host
// compiler builds alone; here are the device kernel that walks the same map,
// the staging buffers and the ctx_* entry points.
#include "ctx.hpp"
#include "shell_map.hpp"

namespace {

struct FieldSet {
    double* f[5];
};

// One wavefront per row; PACK: device fields -> staging, else staging -> fields.
template <bool PACK>
__global__ __launch_bounds__(256) void k_shell_io(FieldSet fs, int nf, ShellMap m, long long px,
                                                  long long ps, double* buf) {
    const int lane = threadIdx.x & 63;
    const long long nrows = m.ny * m.nz;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const long long total = m.total();
    for (long long row = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
         row < nrows * nf; row += waves) {
        const int fi = (int)(row / nrows);
        const long long r = row - fi * nrows;
        const long long k = r / m.ny, j = r - k * m.ny;
        bool whole;
        double* b = buf + fi * total + m.row_off(j, k, &whole);
        double* d = fs.f[fi] + k * ps + j * px;
        if (whole) {
            for (long long i = lane; i < m.nx; i += 64) {
                if (PACK) b[i] = d[i];
                else d[i] = b[i];
            }
        } else if (lane < 2 * m.D) {
            const long long i = (lane < m.D) ? lane : m.nx - 2 * m.D + lane;
            if (PACK) b[lane] = d[i];
            else d[i] = b[lane];
        }
    }
}

// CFD_HIP_SHELL_THREADS (experiments), read once per process
static int shell_threads_env() {
    static const int n = [] {
        const char* e = getenv("CFD_HIP_SHELL_THREADS");
        return e ? std::max(1, atoi(e)) : 0;
    }();
    return n;
}

// host_rows (shell_map.hpp) over this map's staged cells of nf fields
void ctx_host_rows(const ShellMap& m, int nf, double* const* host, double* buf, bool gather) {
    const int nt = shell_thread_count(m.total() * nf, shell_threads_env(),
                                      std::thread::hardware_concurrency());
    host_rows(m, nf, host, buf, gather, nt);
}

cfd_status_t ensure_staging(hip_proj_ctx* c, size_t n) {
    if (c->shell_cap >= n) return CFD_SUCCESS;
    if (c->shell_host) hipHostFree(c->shell_host);
    c->shell_host = nullptr;
    c->shell_cap = 0;
    if (c->shell_dev) hipFree(c->shell_dev);
    c->shell_dev = nullptr;
    HIP_TRY(hipMalloc((void**)&c->shell_dev, n * sizeof(double)));
    HIP_TRY(hipHostMalloc((void**)&c->shell_host, n * sizeof(double), hipHostMallocDefault));
    c->shell_cap = n;
    return CFD_SUCCESS;
}

unsigned io_blocks(const ShellMap& m, int nf) {
    const long long waves = m.ny * m.nz * nf;
    return (unsigned)std::max(1LL, std::min((waves + 3) / 4, 8192LL));
}

}  // namespace

bool ctx_shell_fits(const hip_proj_ctx* c, int depth) {
    return c->nranks == 1 && (long long)c->nx > 2 * depth && (long long)c->ny > 2 * depth &&
           (c->nz == 1 || (long long)c->nz > 2 * depth);
}

cfd_status_t ctx_shell_put(hip_proj_ctx* c, const double* const* host, double* const* dev, int nf,
                           int depth) {
    const ShellMap m = make_map((long long)c->nx, (long long)c->ny, (long long)c->nz, depth);
    const size_t n = (size_t)(m.total() * nf);
    ST_TRY(ensure_staging(c, n));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the staging buffer may still be in flight
    ctx_host_rows(m, nf, const_cast<double* const*>(host), c->shell_host, true);
    HIP_TRY(hipMemcpyAsync(c->shell_dev, c->shell_host, n * sizeof(double), hipMemcpyHostToDevice,
                           c->stream));
    FieldSet fs{};
    for (int i = 0; i < nf; ++i) fs.f[i] = dev[i];
    hipLaunchKernelGGL(k_shell_io<false>, dim3(io_blocks(m, nf)), dim3(256), 0, c->stream, fs, nf,
                       m, c->px, c->ps, c->shell_dev);
    HIP_TRY(hipGetLastError());
    return CFD_SUCCESS;
}

cfd_status_t ctx_shell_get(hip_proj_ctx* c, double* const* host, double* const* dev, int nf,
                           int depth) {
    const ShellMap m = make_map((long long)c->nx, (long long)c->ny, (long long)c->nz, depth);
    const size_t n = (size_t)(m.total() * nf);
    ST_TRY(ensure_staging(c, n));
    FieldSet fs{};
    for (int i = 0; i < nf; ++i) fs.f[i] = dev[i];
    hipLaunchKernelGGL(k_shell_io<true>, dim3(io_blocks(m, nf)), dim3(256), 0, c->stream, fs, nf, m,
                       c->px, c->ps, c->shell_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->shell_host, c->shell_dev, n * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ctx_host_rows(m, nf, host, c->shell_host, false);
    return CFD_SUCCESS;
}

// compute_max_temperature over a host array, the sequential loop's result
// bit for bit on up to 16 threads (shell_map.hpp, host_max)
double ctx_host_max(const double* T, size_t n) {
    return host_max(T, n, host_max_thread_count(n, std::thread::hardware_concurrency()));
}

// The resident-mode guard's hashes of the host arrays (shell_map.hpp, host_hash)
void ctx_host_hash(const hip_proj_ctx* c, const double* const* host, int nf, bool layer1,
                   unsigned long long* out) {
    const int nt = shell_base_threads(shell_threads_env(), std::thread::hardware_concurrency());
    host_hash((long long)c->nx, (long long)c->ny, (long long)c->nz, host, nf, layer1, nt, out);
}
