// pcl_spectrum.hip -- binned plane-crossing energy spectra (ScatterMeasureStep(measure_E=True, E_bins=...)).
//
// A translation unit of its own, linked into libphysicl_hip.so: it does not see struct pcl_ctx and works through the
// public C ABI (include/physicl_hip.h) like any other host of the library.  The tuned kernels, their register budgets and
// the source hash the counter records are tied to (physicl_amd/build.py: csrc_sha) are not touched by anything here.
//
//   k_plane_spectra<T>   one grid-stride sweep of the tiled slab for ALL planes of a call: per slot r[ax] and dr[ax] of
//                        every axis some plane uses, E only where a plane was crossed; crossing lanes look their bin up
//                        in the edges (LDS, binary search) and add to a workgroup-private histogram in LDS; a workgroup
//                        flushes its non-zero bins with 64-bit atomics at the end.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/physicl_hip.h"

namespace {

constexpr int kBlock = 256;                 // 4 wave64 per workgroup, as the library's sweeps
constexpr int kWorkgroupsPerCU = 8;         // grid cap of the sweep: resident workgroups, each takes the same number of trips
// A workgroup-private bin is a uint32: a workgroup adds at most one per slot and plane bin, and the entry point bounds a
// workgroup to fewer than 2^32 slots (kMaxSlotsPerWorkgroup), so it cannot overflow.
constexpr int64_t kMaxSlotsPerWorkgroup = ((int64_t)1 << 32) - kBlock;

template <typename T>
struct spectrum_args {
    const T *E;
    const T *r[3], *dr[3];       // rows of the axes in use (NULL otherwise)
    const unsigned char *kind;   // NULL: every particle is a photon
    const double *edges;         // n_bins + 1, device
    unsigned long long *hist;    // [n_planes][n_bins], device, zeroed by the entry point
    unsigned long long *counts;  // [n_planes]
    int64_t N, ts;               // particles, tile stride of the slab (elements)
    int tile_log;                // log2 of the tile length (pcl_store_layout: 2048 particles)
    T L[PCL_MAX_PLANES];
    int ax[PCL_MAX_PLANES];
    int n_planes, n_bins, ax_used; // bit k of ax_used: some plane is defined on axis k
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_plane_spectra(spectrum_args<T> a) {
    extern __shared__ double s_mem[];                                  // edges | histogram | counts
    double *s_edges = s_mem;
    uint32_t *s_hist = reinterpret_cast<uint32_t *>(s_mem + a.n_bins + 1);
    uint32_t *s_cnt = s_hist + a.n_planes * a.n_bins;
    const int n_cells = a.n_planes * a.n_bins;
    for (int k = threadIdx.x; k <= a.n_bins; k += kBlock) s_edges[k] = a.edges[k];
    for (int k = threadIdx.x; k < n_cells + a.n_planes; k += kBlock) s_hist[k] = 0; // (the counts follow the histogram)
    __syncthreads();
    const double e_lo = s_edges[0], e_hi = s_edges[a.n_bins];
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // whole waves run the same number of trips (the ballots below need every lane of the wave inside the loop)
    const int64_t n_round = (a.N + 63) / 64 * 64;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = (i >> a.tile_log) * a.ts + (i & (((int64_t)1 << a.tile_log) - 1));
        T x[3] = {(T)0, (T)0, (T)0}, prev[3] = {(T)0, (T)0, (T)0};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (in && ((a.ax_used >> k) & 1)) {
                x[k] = a.r[k][ti];
                prev[k] = x[k] - a.dr[k][ti];
            }
        uint32_t crossed = 0; // bit p: this slot crossed plane p in its last move
        for (int p = 0; p < a.n_planes; ++p) {
            const int ax = a.ax[p];
            const T L = a.L[p], xx = ax == 0 ? x[0] : (ax == 1 ? x[1] : x[2]), pp = ax == 0 ? prev[0] : (ax == 1 ? prev[1] : prev[2]);
            const bool c = in && ((pp <= L && L <= xx) || (pp >= L && L >= xx)); // physicl/light.py:386
            const uint32_t nc = (uint32_t)__popcll(__ballot(c));
            if (lane == 0 && nc) atomicAdd(&s_cnt[p], nc);
            crossed |= c ? (1u << p) : 0u;
        }
        if (crossed && (a.kind ? a.kind[i] != 0 : true)) {
            const double e = (double)a.E[ti]; // fp32 widens exactly
            if (e >= e_lo && e <= e_hi) {     // NaN and under/overflow are counted in no bin
                int lo = 0, hi = a.n_bins;    // invariant: edges[lo] <= e, and e < edges[hi] or hi == n_bins
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_edges[mid] <= e) lo = mid; else hi = mid;
                }
                // lo = the last edge <= e among edges[0 .. n_bins - 1]: bins [e_b, e_b+1), the last one closed (numpy.histogram)
                for (uint32_t m = crossed; m; m &= m - 1) atomicAdd(&s_hist[(__ffs(m) - 1) * a.n_bins + lo], 1u);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_cells; k += kBlock)
        if (s_hist[k]) atomicAdd(&a.hist[k], (unsigned long long)s_hist[k]);
    if ((int)threadIdx.x < a.n_planes && s_cnt[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// The calling thread's message (pcl_last_error) lives in the core unit and has no setter in the ABI.  A refused call
// leaves the core's own generic "bad argument" there (pcl_dev_alloc refuses a negative size) rather than the text of some
// earlier failure; the text does not say which edge or plane, and a failed launch of this unit leaves whatever was there
// (include/physicl_hip.h says so).
int bad_argument(pcl_ctx *ctx) {
    void *none = nullptr;
    (void)pcl_dev_alloc(ctx, -1, &none);
    return PCL_ERR_ARG;
}

#define SPC_TRY(expr)                    \
    do {                                 \
        int rc__ = (expr);               \
        if (rc__ != PCL_OK) return rc__; \
    } while (0)

struct dev_block { // one device allocation per call, handed back on every way out
    pcl_ctx *ctx;
    void *p = nullptr;
    explicit dev_block(pcl_ctx *c) : ctx(c) {}
    ~dev_block() { if (p) pcl_dev_free(ctx, p); }
};

template <typename T>
int launch_spectra(pcl_ctx *ctx, hipStream_t stream, spectrum_args<T> &a, const double *planes_host, int n_cu) {
    for (int p = 0; p < a.n_planes; ++p) a.L[p] = (T)planes_host[3 * p + a.ax[p]];
    for (int k = 0; k < 3; ++k) {
        if (!((a.ax_used >> k) & 1)) continue;
        void *r = nullptr, *dr = nullptr;
        SPC_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        SPC_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));
        a.r[k] = static_cast<const T *>(r);
        a.dr[k] = static_cast<const T *>(dr);
    }
    const int64_t blocks = (a.N + kBlock - 1) / kBlock;
    int64_t grid = blocks, cap = (int64_t)(n_cu > 0 ? n_cu : 256) * kWorkgroupsPerCU;
    if (grid > cap) {
        int64_t trips = (blocks + cap - 1) / cap;
        while (trips * kBlock > kMaxSlotsPerWorkgroup) { cap *= 2; trips = (blocks + cap - 1) / cap; } // (never, below 2^43 slots)
        grid = (blocks + trips - 1) / trips; // every workgroup takes the same number of trips
    }
    const size_t lds = (size_t)(a.n_bins + 1) * sizeof(double) + ((size_t)a.n_planes * a.n_bins + a.n_planes) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_plane_spectra<T>, dim3((unsigned)grid), dim3(kBlock), lds, stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int plane_spectra(pcl_ctx *ctx, const double *planes_host, int n_planes, const double *edges_host, int n_bins,
                  int64_t *counts_out_host, int64_t *hist_out_host) {
    if (!ctx || !planes_host || !edges_host || !counts_out_host || !hist_out_host) return bad_argument(ctx);
    if (n_planes < 1 || n_planes > PCL_MAX_PLANES || n_bins < 1 || n_bins > PCL_SPECTRUM_MAX_BINS) return bad_argument(ctx);
    for (int b = 0; b <= n_bins; ++b)
        if (!std::isfinite(edges_host[b]) || (b > 0 && !(edges_host[b] > edges_host[b - 1]))) return bad_argument(ctx);
    int ax[PCL_MAX_PLANES], ax_used = 0;
    for (int p = 0; p < n_planes; ++p) {
        const double *loc = planes_host + 3 * p;
        ax[p] = !std::isnan(loc[0]) ? 0 : (!std::isnan(loc[1]) ? 1 : 2); // first defining coordinate, light.py:385-396
        if (std::isnan(loc[ax[p]])) return bad_argument(ctx);
        ax_used |= 1 << ax[p];
    }
    // the first look at the store: a store behind an alive mask becomes dense, an implicit dr real (PCL_ERR_STATE without a store)
    void *E = nullptr;
    SPC_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    for (int p = 0; p < n_planes; ++p) counts_out_host[p] = 0;
    memset(hist_out_host, 0, (size_t)n_planes * n_bins * sizeof(int64_t));
    int64_t N = 0, tile = 0, ts = 0;
    SPC_TRY(pcl_store_count(ctx, &N));
    if (N <= 0) return PCL_OK;
    int dtype = PCL_DTYPE_F64, uniform = 0, n_cu = 0;
    SPC_TRY(pcl_store_dtype(ctx, &dtype));
    SPC_TRY(pcl_store_layout(ctx, &tile, &ts));
    int tile_log = 0;
    while (((int64_t)1 << tile_log) < tile) ++tile_log;
    if (((int64_t)1 << tile_log) != tile) return PCL_ERR_STATE; // the slab's tiles are a power of two long
    SPC_TRY(pcl_store_is_uniform(ctx, &uniform));
    SPC_TRY(pcl_ctx_device_info(ctx, nullptr, 0, nullptr, &n_cu, nullptr));
    void *stream_v = nullptr;
    SPC_TRY(pcl_ctx_stream(ctx, &stream_v));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);

    // plain Objects carry no energy: their kind bytes go along when the store holds any (the ABI hands them out on the host only)
    std::vector<uint8_t> kind_host;
    bool mixed = false;
    if (!uniform) {
        kind_host.resize((size_t)N);
        SPC_TRY(pcl_store_download_kind(ctx, kind_host.data(), 0, N));
        mixed = memchr(kind_host.data(), PCL_KIND_OBJECT, (size_t)N) != nullptr;
    }
    const size_t cells = (size_t)n_planes * n_bins;
    const size_t out_bytes = (cells + n_planes) * sizeof(uint64_t), edge_bytes = (size_t)(n_bins + 1) * sizeof(double);
    dev_block blk(ctx);
    SPC_TRY(pcl_dev_alloc(ctx, (int64_t)(out_bytes + edge_bytes + (mixed ? (size_t)N : 0)), &blk.p));
    char *base = static_cast<char *>(blk.p);
    if (hipMemsetAsync(base, 0, out_bytes, stream) != hipSuccess) return PCL_ERR_HIP;
    if (hipMemcpyAsync(base + out_bytes, edges_host, edge_bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return PCL_ERR_HIP;
    if (mixed && hipMemcpyAsync(base + out_bytes + edge_bytes, kind_host.data(), (size_t)N, hipMemcpyHostToDevice, stream) != hipSuccess)
        return PCL_ERR_HIP;
    const unsigned char *kind = mixed ? reinterpret_cast<const unsigned char *>(base + out_bytes + edge_bytes) : nullptr;

    int rc;
    if (dtype == PCL_DTYPE_F64) {
        spectrum_args<double> a{};
        a.E = static_cast<const double *>(E);
        a.kind = kind; a.edges = reinterpret_cast<const double *>(base + out_bytes);
        a.hist = reinterpret_cast<unsigned long long *>(base); a.counts = a.hist + cells;
        a.N = N; a.ts = ts; a.tile_log = tile_log; a.n_planes = n_planes; a.n_bins = n_bins; a.ax_used = ax_used;
        for (int p = 0; p < n_planes; ++p) a.ax[p] = ax[p];
        rc = launch_spectra<double>(ctx, stream, a, planes_host, n_cu);
    } else {
        spectrum_args<float> a{};
        a.E = static_cast<const float *>(E);
        a.kind = kind; a.edges = reinterpret_cast<const double *>(base + out_bytes);
        a.hist = reinterpret_cast<unsigned long long *>(base); a.counts = a.hist + cells;
        a.N = N; a.ts = ts; a.tile_log = tile_log; a.n_planes = n_planes; a.n_bins = n_bins; a.ax_used = ax_used;
        for (int p = 0; p < n_planes; ++p) a.ax[p] = ax[p];
        rc = launch_spectra<float>(ctx, stream, a, planes_host, n_cu);
    }
    SPC_TRY(rc);
    std::vector<uint64_t> out(cells + n_planes);
    SPC_TRY(pcl_d2h(ctx, out.data(), base, (int64_t)out_bytes)); // the call's one synchronisation
    for (size_t k = 0; k < cells; ++k) hist_out_host[k] = (int64_t)out[k];
    for (int p = 0; p < n_planes; ++p) counts_out_host[p] = (int64_t)out[cells + p];
    return PCL_OK;
}

int group_plane_spectra(pcl_group *group, const double *planes_host, int n_planes, const double *edges_host, int n_bins,
                        int64_t *counts_out_host, int64_t *hist_out_host) {
    int n = 0;
    SPC_TRY(pcl_group_size(group, &n));
    if (!counts_out_host || !hist_out_host || n_planes < 1 || n_planes > PCL_MAX_PLANES || n_bins < 1 || n_bins > PCL_SPECTRUM_MAX_BINS) {
        pcl_ctx *first = nullptr;
        SPC_TRY(pcl_group_ctx(group, 0, &first));
        return bad_argument(first);
    }
    const size_t cells = (size_t)n_planes * n_bins;
    std::vector<pcl_ctx *> ctx((size_t)n);
    for (int g = 0; g < n; ++g) SPC_TRY(pcl_group_ctx(group, g, &ctx[(size_t)g]));
    std::vector<std::vector<int64_t>> part((size_t)n, std::vector<int64_t>(cells + n_planes, 0));
    std::vector<int> rcs((size_t)n, PCL_OK);
    auto one = [&](int g) {
        rcs[(size_t)g] = pcl_step_plane_spectra(ctx[(size_t)g], planes_host, n_planes, edges_host, n_bins, part[(size_t)g].data() + cells,
                                                part[(size_t)g].data());
    };
    // the shards' sweeps run side by side: a thread each per call (the group's own workers cannot be reached through the
    // ABI), the calling thread takes shard 0.  A shard whose thread cannot be started is served by the calling thread.
    std::vector<std::thread> th;
    th.reserve((size_t)n);
    for (int g = 1; g < n; ++g) {
        try {
            th.emplace_back(one, g);
        } catch (const std::system_error &) {
            one(g);
        }
    }
    one(0);
    for (auto &t : th) t.join();
    for (int g = 0; g < n; ++g) SPC_TRY(rcs[(size_t)g]);
    for (int p = 0; p < n_planes; ++p) counts_out_host[p] = 0;
    memset(hist_out_host, 0, cells * sizeof(int64_t));
    for (int g = 0; g < n; ++g) {
        for (size_t k = 0; k < cells; ++k) hist_out_host[k] += part[(size_t)g][k];
        for (int p = 0; p < n_planes; ++p) counts_out_host[p] += part[(size_t)g][cells + p];
    }
    return PCL_OK;
}

} // namespace

extern "C" {

// Nothing may be thrown through the C boundary: host allocations of the bodies above (the kind bytes of a big store, the
// per-shard rows) can fail.
int pcl_step_plane_spectra(pcl_ctx *ctx, const double *planes_host, int n_planes, const double *edges_host, int n_bins,
                           int64_t *counts_out_host, int64_t *hist_out_host) {
    try {
        return plane_spectra(ctx, planes_host, n_planes, edges_host, n_bins, counts_out_host, hist_out_host);
    } catch (const std::bad_alloc &) {
        return PCL_ERR_NOMEM;
    } catch (...) {
        return PCL_ERR_HIP;
    }
}

int pcl_group_step_plane_spectra(pcl_group *group, const double *planes_host, int n_planes, const double *edges_host, int n_bins,
                                 int64_t *counts_out_host, int64_t *hist_out_host) {
    try {
        return group_plane_spectra(group, planes_host, n_planes, edges_host, n_bins, counts_out_host, hist_out_host);
    } catch (const std::bad_alloc &) {
        return PCL_ERR_NOMEM;
    } catch (...) {
        return PCL_ERR_HIP;
    }
}

} // extern "C"
