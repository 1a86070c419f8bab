// pcl_spectrum.hip -- binned plane-crossing energy spectra (ScatterMeasureStep(measure_E=True, E_bins=...)).
//
// A translation unit of its own, linked into libphysicl_hip.so: it does not see struct pcl_ctx and works through the
// public C ABI (include/physicl_hip.h) like any other host of the library.  The tuned kernels, their register budgets and
// the source hash the counter records are tied to (physicl_amd/build.py: csrc_sha) are not touched by anything here.  What
// it shares with the other units of its kind -- opening the store, the balanced grid, the group fan-out, the device
// helpers -- is pcl_sweep.h.
//
//   k_plane_spectra<T>   one grid-stride sweep of the tiled slab for ALL planes of a call: per slot r[ax] and dr[ax] of
//                        every axis some plane uses, E only where a plane was crossed; crossing lanes look their bin up
//                        in the edges (LDS, binary search) and add to a workgroup-private histogram in LDS; a workgroup
//                        flushes its non-zero bins with 64-bit atomics at the end.
#include "pcl_sweep.h"

namespace {

using namespace pcl_sweep;

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
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
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
                const int lo = bin_of(s_edges, a.n_bins, e);
                for (uint32_t m = crossed; m; m &= m - 1) atomicAdd(&s_hist[(__ffs(m) - 1) * a.n_bins + lo], 1u);
            }
        }
    }
    __syncthreads();
    flush_cells(s_hist, a.hist, n_cells);
    if ((int)threadIdx.x < a.n_planes && s_cnt[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

template <typename T>
int launch_spectra(pcl_ctx *ctx, const store_view &v, const void *E, const staged &st, const double *planes_host, const int *ax,
                   int ax_used, int n_planes, int n_bins) {
    spectrum_args<T> a{};
    a.E = static_cast<const T *>(E); a.kind = st.kind; a.edges = st.tables;
    a.hist = st.out; a.counts = st.out + (size_t)n_planes * n_bins;
    a.N = v.N; a.ts = v.ts; a.tile_log = v.tile_log; a.n_planes = n_planes; a.n_bins = n_bins; a.ax_used = ax_used;
    for (int p = 0; p < n_planes; ++p) {
        a.ax[p] = ax[p];
        a.L[p] = (T)planes_host[3 * p + ax[p]];
    }
    for (int k = 0; k < 3; ++k) {
        if (!((ax_used >> k) & 1)) continue;
        void *r = nullptr, *dr = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));
        a.r[k] = static_cast<const T *>(r);
        a.dr[k] = static_cast<const T *>(dr);
    }
    const size_t lds = (size_t)(n_bins + 1) * sizeof(double) + ((size_t)n_planes * n_bins + n_planes) * sizeof(uint32_t);
    const int64_t grid = balanced_grid(v.N, v.n_cu, kWorkgroupsPerCU);
    hipLaunchKernelGGL(k_plane_spectra<T>, dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int plane_spectra(pcl_ctx *ctx, const double *planes_host, int n_planes, const double *edges_host, int n_bins,
                  int64_t *counts_out_host, int64_t *hist_out_host) {
    if (!ctx || !planes_host || !edges_host || !counts_out_host || !hist_out_host) return bad_argument(ctx);
    if (n_planes < 1 || n_planes > PCL_MAX_PLANES || n_bins < 1 || n_bins > PCL_SPECTRUM_MAX_BINS) return bad_argument(ctx);
    if (!check_edges(edges_host, n_bins, kEdgePlain)) return bad_argument(ctx);
    int ax[PCL_MAX_PLANES], ax_used = 0;
    for (int p = 0; p < n_planes; ++p) {
        const double *loc = planes_host + 3 * p;
        ax[p] = !std::isnan(loc[0]) ? 0 : (!std::isnan(loc[1]) ? 1 : 2); // first defining coordinate, light.py:385-396
        if (std::isnan(loc[ax[p]])) return bad_argument(ctx);
        ax_used |= 1 << ax[p];
    }
    const spans out = {{hist_out_host, (size_t)n_planes * n_bins}, {counts_out_host, (size_t)n_planes}};
    void *E = nullptr;
    store_view v;
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_E, &v, &E));
    zero_spans(out);
    if (v.N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(stage(st, v, cells_of(out), edges_host, (size_t)n_bins + 1, false));   // nothing is drawn: no ids
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_spectra, ctx, v, E, st, planes_host, ax, ax_used, n_planes, n_bins));
    return fetch(st, out);
}

int group_plane_spectra(pcl_group *group, const double *planes_host, int n_planes, const double *edges_host, int n_bins,
                        int64_t *counts_out_host, int64_t *hist_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    if (n < 1 || !counts_out_host || !hist_out_host || n_planes < 1 || n_planes > PCL_MAX_PLANES || n_bins < 1 || n_bins > PCL_SPECTRUM_MAX_BINS)
        return bad_argument(n > 0 ? ctx[0] : nullptr);
    const size_t cells = (size_t)n_planes * n_bins;
    return sum_shards(ctx, {{hist_out_host, cells}, {counts_out_host, (size_t)n_planes}}, [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_plane_spectra(one, planes_host, n_planes, edges_host, n_bins, p + cells, p);
    });
}

} // namespace

extern "C" {

int pcl_step_plane_spectra(pcl_ctx *ctx, const double *planes_host, int n_planes, const double *edges_host, int n_bins,
                           int64_t *counts_out_host, int64_t *hist_out_host) {
    return guarded([&] { return plane_spectra(ctx, planes_host, n_planes, edges_host, n_bins, counts_out_host, hist_out_host); });
}

int pcl_group_step_plane_spectra(pcl_group *group, const double *planes_host, int n_planes, const double *edges_host, int n_bins,
                                 int64_t *counts_out_host, int64_t *hist_out_host) {
    return guarded([&] { return group_plane_spectra(group, planes_host, n_planes, edges_host, n_bins, counts_out_host, hist_out_host); });
}

} // extern "C"
