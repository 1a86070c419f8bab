// pcl_shell.hip -- spherical-shell crossing tallies (ShellCrossingMeasureStep): what passed through the spheres of a radial
// problem in the last move -- per shell the particles that went out and the ones that came in, the crossing photons'
// energies and the cosine of the move against the local vertical as integer histograms --, made in one read-only sweep of
// the resident store.
//
// A translation unit of its own, linked into libphysicl_hip.so between pcl_source.hip and pcl_grid.hip: it does not see
// struct pcl_ctx and works through the public C ABI (include/physicl_hip.h) like any other host of the library.  The tuned
// kernels, their register budgets and the source hash the counter records are tied to (physicl_amd/build.py: csrc_sha) are
// not touched by anything here.
//
//   k_shell_crossings<T>   one grid-stride sweep of the tiled slab for ALL shells of a call: per slot r and dr of the three
//                          axes (48 B in fp64), widened to double; q_now and q_prev against R*R of every shell (LDS), one
//                          ballot + popcount per shell and direction for the counts; lanes that crossed look E up in the
//                          energy edges and W = s*|s| against w_b*D in the direction edges (LDS, binary searches, no square
//                          root and no division) and add to workgroup-private uint32 histograms in LDS; a workgroup
//                          flushes its non-zero cells with 64-bit atomics at the end.
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
constexpr int kLdsPerCU = 160 * 1024;       // gfx950
// A workgroup-private cell is a uint32: a workgroup adds at most one per slot to a cell, and the entry point bounds a
// workgroup to fewer than 2^32 slots (kMaxSlotsPerWorkgroup), so it cannot overflow.
constexpr int64_t kMaxSlotsPerWorkgroup = ((int64_t)1 << 32) - kBlock;

template <typename T>
struct shell_args {
    const T *r[3], *dr[3];
    const T *E;                  // NULL without energy bins
    const unsigned char *kind;   // NULL: every particle is a photon
    const double *tables;        // E edges (n_E + 1, if any) | w_b = e_b*|e_b| (n_mu + 1, if any) | R*R (n_shells), device
    unsigned long long *out;     // counts [2][S] | E_hist [2][S][n_E] | mu_hist [2][S][n_mu], device, zeroed by the entry point
    int64_t N, ts;               // particles, tile stride of the slab (elements)
    int tile_log;                // log2 of the tile length (pcl_store_layout: 2048 particles)
    int n_shells, n_E, n_mu;
    double c[3];
};

// The bin of v in e[0 .. nb]: [e_b, e_b+1), the last one closed (numpy.histogram); the caller has checked e[0] <= v <= e[nb].
__device__ __forceinline__ int bin_of(const double *e, int nb, double v) {
    int lo = 0, hi = nb;        // invariant: e[lo] <= v, and v < e[hi] or hi == nb
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename T>
__global__ void __launch_bounds__(kBlock) k_shell_crossings(shell_args<T> a) {
    extern __shared__ double s_mem[];                                  // tables | counts | E histogram | mu histogram
    const int S = a.n_shells, nE = a.n_E, nmu = a.n_mu;
    const int n_tab = (nE ? nE + 1 : 0) + (nmu ? nmu + 1 : 0) + S;
    const int n_cells = 2 * S * (1 + nE + nmu);
    double *s_E = s_mem;
    double *s_w = s_E + (nE ? nE + 1 : 0);
    double *s_R2 = s_w + (nmu ? nmu + 1 : 0);
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_mem + n_tab);
    uint32_t *s_Eh = s_cnt + 2 * S;
    uint32_t *s_muh = s_Eh + 2 * S * nE;
    for (int k = threadIdx.x; k < n_tab; k += kBlock) s_mem[k] = a.tables[k];
    for (int k = threadIdx.x; k < n_cells; k += kBlock) s_cnt[k] = 0;  // (the histograms follow the counts)
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // whole waves run the same number of trips (the ballots below need every lane of the wave inside the loop)
    const int64_t n_round = (a.N + 63) / 64 * 64;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = (i >> a.tile_log) * a.ts + (i & (((int64_t)1 << a.tile_log) - 1));
        double d[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (in) {
                d[k] = (double)a.r[k][ti] - a.c[k];                    // fp32 widens exactly
                m[k] = (double)a.dr[k][ti];
            }
        // unfused, in this order (the library is built with -ffp-contract=off)
        const double p0 = d[0] - m[0], p1 = d[1] - m[1], p2 = d[2] - m[2];
        const double q_now = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        const double q_prev = (p0 * p0 + p1 * p1) + p2 * p2;
        uint32_t crossed = 0;   // bit s: outward through shell s in the last move, bit 16 + s: inward (NaN: neither)
        for (int s = 0; s < S; ++s) {
            const double R2 = s_R2[s];
            const bool o = in && q_prev < R2 && q_now >= R2, b = in && q_prev >= R2 && q_now < R2;
            const uint32_t no = (uint32_t)__popcll(__ballot(o)), nb = (uint32_t)__popcll(__ballot(b));
            if (lane == 0 && no) atomicAdd(&s_cnt[s], no);
            if (lane == 0 && nb) atomicAdd(&s_cnt[S + s], nb);
            crossed |= (o ? 1u << s : 0u) | (b ? 0x10000u << s : 0u);
        }
        if (!crossed) continue; // lanes that crossed nothing wait at the loop's head: no ballot below this line
        if (nE && (a.kind ? a.kind[i] != 0 : true)) {                  // plain Objects carry no energy
            const double e = (double)a.E[ti];
            if (e >= s_E[0] && e <= s_E[nE]) {                         // NaN and under/overflow are counted in no bin
                const int lo = bin_of(s_E, nE, e);
                for (uint32_t x = crossed; x; x &= x - 1) {
                    const int bit = __ffs(x) - 1;                      // cell row: direction * S + shell
                    atomicAdd(&s_Eh[((bit >> 4) * S + (bit & 15)) * nE + lo], 1u);
                }
            }
        }
        if (nmu) {
            const double sp = (d[0] * m[0] + d[1] * m[1]) + d[2] * m[2];
            const double dd = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
            const double W = sp * fabs(sp), D = q_now * dd;
            // mu = sp / sqrt(D) in bin b iff w_b*D <= W < w_(b+1)*D: one multiply per probe, rounded products are monotone in b.
            // D == 0 (no move, or on the centre) and anything not finite: counted above, in no bin
            if (D > 0.0 && D < INFINITY && fabs(W) < INFINITY && W >= s_w[0] * D && W <= s_w[nmu] * D) {
                int lo = 0, hi = nmu;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_w[mid] * D <= W) lo = mid; else hi = mid;
                }
                for (uint32_t x = crossed; x; x &= x - 1) {
                    const int bit = __ffs(x) - 1;
                    atomicAdd(&s_muh[((bit >> 4) * S + (bit & 15)) * nmu + lo], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_cells; k += kBlock)
        if (s_cnt[k]) atomicAdd(&a.out[k], (unsigned long long)s_cnt[k]);
}

// The calling thread's message (pcl_last_error) lives in the core unit and has no setter in the ABI: a refused call leaves
// the core's own generic "bad argument" there, as pcl_spectrum.hip does (include/physicl_hip.h says so).
int bad_argument(pcl_ctx *ctx) {
    void *none = nullptr;
    if (ctx) (void)pcl_dev_alloc(ctx, -1, &none);
    return PCL_ERR_ARG;
}

#define SHL_TRY(expr)                    \
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

struct shell_spec { // a call's arguments, checked; what the kernel compares against
    int n_shells = 0, n_E = 0, n_mu = 0;
    double c[3] = {0.0, 0.0, 0.0};
    std::vector<double> tables; // E edges | w_b | R*R
    size_t cells() const { return (size_t)2 * n_shells * (1 + n_E + n_mu); }
};

// n + 1 finite, strictly increasing edges, 1 <= n <= PCL_SHELL_MAX_BINS -- or none at all (NULL or not, 0 bins)
bool check_edges(const double *edges, int n, const int64_t *out, bool signed_square, std::vector<double> &to) {
    if (n == 0) return true;
    if (n < 0 || n > PCL_SHELL_MAX_BINS || !edges || !out) return false;
    for (int b = 0; b <= n; ++b) {
        if (!std::isfinite(edges[b]) || (b > 0 && !(edges[b] > edges[b - 1]))) return false;
        const double v = signed_square ? edges[b] * std::fabs(edges[b]) : edges[b];
        if (!std::isfinite(v) || (b > 0 && !(v > to.back()))) return false;
        to.push_back(v);
    }
    return true;
}

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_spec(int n_shells, const double *radii, const double *center, const double *E_edges, int n_E, const double *mu_edges,
                int n_mu, const int64_t *counts_out, const int64_t *E_out, const int64_t *mu_out, shell_spec &s) {
    if (!radii || !counts_out || n_shells < 1 || n_shells > PCL_SHELL_MAX_SHELLS) return false;
    if (!check_edges(E_edges, n_E, E_out, false, s.tables)) return false;
    if (!check_edges(mu_edges, n_mu, mu_out, true, s.tables)) return false;
    if ((int64_t)2 * n_shells * ((int64_t)n_E + n_mu) > PCL_SHELL_MAX_CELLS) return false;
    for (int k = 0; k < n_shells; ++k) {
        const double R2 = radii[k] * radii[k];
        if (!std::isfinite(radii[k]) || !(radii[k] > 0) || !std::isfinite(R2)) return false;
        s.tables.push_back(R2);
    }
    if (center)
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(center[k])) return false;
            s.c[k] = center[k];
        }
    s.n_shells = n_shells; s.n_E = n_E; s.n_mu = n_mu;
    return true;
}

void zero_outputs(const shell_spec &s, int64_t *counts, int64_t *E_hist, int64_t *mu_hist) {
    memset(counts, 0, (size_t)2 * s.n_shells * sizeof(int64_t));
    if (s.n_E) memset(E_hist, 0, (size_t)2 * s.n_shells * s.n_E * sizeof(int64_t));
    if (s.n_mu) memset(mu_hist, 0, (size_t)2 * s.n_shells * s.n_mu * sizeof(int64_t));
}

template <typename T>
int launch_shell(pcl_ctx *ctx, hipStream_t stream, const shell_spec &s, const void *E, const unsigned char *kind, const double *tables_dev,
                 unsigned long long *out_dev, int64_t N, int64_t ts, int tile_log, int n_cu) {
    shell_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *dr = nullptr;
        SHL_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        SHL_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));
        a.r[k] = static_cast<const T *>(r);
        a.dr[k] = static_cast<const T *>(dr);
        a.c[k] = s.c[k];
    }
    a.E = static_cast<const T *>(E); a.kind = kind; a.tables = tables_dev; a.out = out_dev;
    a.N = N; a.ts = ts; a.tile_log = tile_log;
    a.n_shells = s.n_shells; a.n_E = s.n_E; a.n_mu = s.n_mu;
    const size_t lds = s.tables.size() * sizeof(double) + s.cells() * sizeof(uint32_t);
    // resident workgroups only: every workgroup flushes its own histograms
    int per_cu = (int)(kLdsPerCU / lds);
    per_cu = per_cu < 1 ? 1 : (per_cu > kWorkgroupsPerCU ? kWorkgroupsPerCU : per_cu);
    const int64_t blocks = (N + kBlock - 1) / kBlock;
    int64_t grid = blocks, cap = (int64_t)(n_cu > 0 ? n_cu : 256) * per_cu;
    if (grid > cap) {
        int64_t trips = (blocks + cap - 1) / cap;
        while (trips * kBlock > kMaxSlotsPerWorkgroup) { cap *= 2; trips = (blocks + cap - 1) / cap; } // (never, below 2^43 slots)
        grid = (blocks + trips - 1) / trips; // every workgroup takes the same number of trips
    }
    hipLaunchKernelGGL(k_shell_crossings<T>, dim3((unsigned)grid), dim3(kBlock), lds, stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int shell_crossings(pcl_ctx *ctx, int n_shells, const double *radii_host, const double *center_host, const double *E_edges_host,
                    int n_E_bins, const double *mu_edges_host, int n_mu_bins, int64_t *counts_out_host, int64_t *E_hist_out_host,
                    int64_t *mu_hist_out_host) {
    shell_spec s;
    if (!ctx || !check_spec(n_shells, radii_host, center_host, E_edges_host, n_E_bins, mu_edges_host, n_mu_bins, counts_out_host,
                            E_hist_out_host, mu_hist_out_host, s))
        return bad_argument(ctx);
    // the first look at the store: a store behind an alive mask becomes dense, an implicit dr real (PCL_ERR_STATE without a
    // store).  E is asked for only with energy bins: the pointer costs a wavelength-dependent scatter step its term cache.
    void *first = nullptr, *E = nullptr;
    SHL_TRY(pcl_store_field_ptr(ctx, PCL_R0, &first));
    if (s.n_E) SHL_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    int64_t N = 0, tile = 0, ts = 0;
    SHL_TRY(pcl_store_count(ctx, &N));
    if (N <= 0) {
        zero_outputs(s, counts_out_host, E_hist_out_host, mu_hist_out_host);
        return PCL_OK;
    }
    int dtype = PCL_DTYPE_F64, uniform = 1, n_cu = 0;
    SHL_TRY(pcl_store_dtype(ctx, &dtype));
    SHL_TRY(pcl_store_layout(ctx, &tile, &ts));
    int tile_log = 0;
    while (((int64_t)1 << tile_log) < tile) ++tile_log;
    if (((int64_t)1 << tile_log) != tile) return PCL_ERR_STATE; // the slab's tiles are a power of two long
    SHL_TRY(pcl_ctx_device_info(ctx, nullptr, 0, nullptr, &n_cu, nullptr));
    void *stream_v = nullptr;
    SHL_TRY(pcl_ctx_stream(ctx, &stream_v));
    hipStream_t stream = static_cast<hipStream_t>(stream_v);

    // plain Objects carry no energy: their kind bytes go along when energies are binned and the store holds any (the ABI
    // hands them out on the host only)
    std::vector<uint8_t> kind_host;
    bool mixed = false;
    if (s.n_E) {
        SHL_TRY(pcl_store_is_uniform(ctx, &uniform));
        if (!uniform) {
            kind_host.resize((size_t)N);
            SHL_TRY(pcl_store_download_kind(ctx, kind_host.data(), 0, N));
            mixed = memchr(kind_host.data(), PCL_KIND_OBJECT, (size_t)N) != nullptr;
        }
    }
    const size_t cells = s.cells();
    const size_t out_bytes = cells * sizeof(uint64_t), tab_bytes = s.tables.size() * sizeof(double);
    dev_block blk(ctx);
    SHL_TRY(pcl_dev_alloc(ctx, (int64_t)(out_bytes + tab_bytes + (mixed ? (size_t)N : 0)), &blk.p));
    char *base = static_cast<char *>(blk.p);
    if (hipMemsetAsync(base, 0, out_bytes, stream) != hipSuccess) return PCL_ERR_HIP;
    if (hipMemcpyAsync(base + out_bytes, s.tables.data(), tab_bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return PCL_ERR_HIP;
    if (mixed && hipMemcpyAsync(base + out_bytes + tab_bytes, kind_host.data(), (size_t)N, hipMemcpyHostToDevice, stream) != hipSuccess)
        return PCL_ERR_HIP;
    const unsigned char *kind = mixed ? reinterpret_cast<const unsigned char *>(base + out_bytes + tab_bytes) : nullptr;
    const double *tables_dev = reinterpret_cast<const double *>(base + out_bytes);
    unsigned long long *out_dev = reinterpret_cast<unsigned long long *>(base);
    SHL_TRY(dtype == PCL_DTYPE_F64 ? launch_shell<double>(ctx, stream, s, E, kind, tables_dev, out_dev, N, ts, tile_log, n_cu)
                                   : launch_shell<float>(ctx, stream, s, E, kind, tables_dev, out_dev, N, ts, tile_log, n_cu));
    std::vector<int64_t> out(cells);
    SHL_TRY(pcl_d2h(ctx, out.data(), base, (int64_t)out_bytes)); // the call's one synchronisation (a count is below 2^63)
    const size_t n_cnt = (size_t)2 * s.n_shells;
    memcpy(counts_out_host, out.data(), n_cnt * sizeof(int64_t));
    if (s.n_E) memcpy(E_hist_out_host, out.data() + n_cnt, n_cnt * s.n_E * sizeof(int64_t));
    if (s.n_mu) memcpy(mu_hist_out_host, out.data() + n_cnt * (1 + s.n_E), n_cnt * s.n_mu * sizeof(int64_t));
    return PCL_OK;
}

int group_shell_crossings(pcl_group *group, int n_shells, const double *radii_host, const double *center_host,
                          const double *E_edges_host, int n_E_bins, const double *mu_edges_host, int n_mu_bins, int64_t *counts_out_host,
                          int64_t *E_hist_out_host, int64_t *mu_hist_out_host) {
    int n = 0;
    SHL_TRY(pcl_group_size(group, &n));
    std::vector<pcl_ctx *> ctx((size_t)n);
    for (int g = 0; g < n; ++g) SHL_TRY(pcl_group_ctx(group, g, &ctx[(size_t)g]));
    shell_spec s;
    if (n < 1 || !check_spec(n_shells, radii_host, center_host, E_edges_host, n_E_bins, mu_edges_host, n_mu_bins, counts_out_host,
                             E_hist_out_host, mu_hist_out_host, s))
        return bad_argument(n > 0 ? ctx[0] : nullptr);
    const size_t n_cnt = (size_t)2 * n_shells, at_E = n_cnt, at_mu = n_cnt * (1 + (size_t)n_E_bins);
    std::vector<std::vector<int64_t>> part((size_t)n, std::vector<int64_t>(s.cells(), 0));
    std::vector<int> rcs((size_t)n, PCL_OK);
    auto one = [&](int g) {
        int64_t *p = part[(size_t)g].data();
        rcs[(size_t)g] = pcl_step_shell_crossings(ctx[(size_t)g], n_shells, radii_host, center_host, E_edges_host, n_E_bins, mu_edges_host,
                                                  n_mu_bins, p, p + at_E, p + at_mu);
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
    for (int g = 0; g < n; ++g) SHL_TRY(rcs[(size_t)g]);
    zero_outputs(s, counts_out_host, E_hist_out_host, mu_hist_out_host);
    for (int g = 0; g < n; ++g) {
        const int64_t *p = part[(size_t)g].data();
        for (size_t k = 0; k < n_cnt; ++k) counts_out_host[k] += p[k];
        for (size_t k = 0; k < n_cnt * (size_t)n_E_bins; ++k) E_hist_out_host[k] += p[at_E + k];
        for (size_t k = 0; k < n_cnt * (size_t)n_mu_bins; ++k) mu_hist_out_host[k] += p[at_mu + k];
    }
    return PCL_OK;
}

} // namespace

extern "C" {

// Nothing may be thrown through the C boundary: host allocations of the bodies above (the tables, the kind bytes of a big
// store, the per-shard rows) can fail.
int pcl_step_shell_crossings(pcl_ctx *ctx, int n_shells, const double *radii_host, const double *center_host, const double *E_edges_host,
                             int n_E_bins, const double *mu_edges_host, int n_mu_bins, int64_t *counts_out_host, int64_t *E_hist_out_host,
                             int64_t *mu_hist_out_host) {
    try {
        return shell_crossings(ctx, n_shells, radii_host, center_host, E_edges_host, n_E_bins, mu_edges_host, n_mu_bins, counts_out_host,
                               E_hist_out_host, mu_hist_out_host);
    } catch (const std::bad_alloc &) {
        return PCL_ERR_NOMEM;
    } catch (...) {
        return PCL_ERR_HIP;
    }
}

int pcl_group_step_shell_crossings(pcl_group *group, int n_shells, const double *radii_host, const double *center_host,
                                   const double *E_edges_host, int n_E_bins, const double *mu_edges_host, int n_mu_bins,
                                   int64_t *counts_out_host, int64_t *E_hist_out_host, int64_t *mu_hist_out_host) {
    try {
        return group_shell_crossings(group, n_shells, radii_host, center_host, E_edges_host, n_E_bins, mu_edges_host, n_mu_bins,
                                     counts_out_host, E_hist_out_host, mu_hist_out_host);
    } catch (const std::bad_alloc &) {
        return PCL_ERR_NOMEM;
    } catch (...) {
        return PCL_ERR_HIP;
    }
}

} // extern "C"
