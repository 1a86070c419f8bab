// pcl_source.hip -- photon sources for bulk generation (PhotonSource / generate_photons_bulk(..., source=)).
//
// pcl_store_fill_photons[_table] creates every photon at r = 0 with v = (c, 0, 0).  pcl_store_apply_source gives that fresh
// population its positions and velocities: a point, a disc or a gaussian spot around ``origin``; a beam along ``d``, an
// isotropic point source, a cone or a lambertian (cosine-weighted) emitter about ``d``.
//
// A translation unit of its own, linked into libphysicl_hip.so behind pcl_spectrum.hip: it does not see struct pcl_ctx and
// works through the public C ABI (include/physicl_hip.h) like any other host of the library; pcl_device.h is included for
// the Philox block, the 53-bit uniform and the project's sincos only.  The tuned kernels, their register budgets and the
// source hash the counter records are tied to (physicl_amd/build.py: csrc_sha) are not touched by anything here.
//
//   k_apply_source<T>   one grid-stride sweep of photons [0, n): Philox block 4 of the photon's id for the direction, block 5
//                       for the position (blocks 2 and 3 are the energy draws of k_fill_photons / k_fill_table), so a photon
//                       is the same photon however the run is sharded.  Everything is computed in fp64, unfused, and rounded
//                       once to the store's precision.  Rows that would not change are not written.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/physicl_hip.h"
#include "pcl_device.h"

namespace {

constexpr int kBlock = 256;         // 4 wave64 per workgroup, as the library's sweeps
constexpr int kWorkgroupsPerCU = 8; // grid cap of the sweep

template <typename T>
struct source_args {
    T *r[3], *v[3];              // rows to write (NULL: the row keeps what the fill wrote)
    int64_t n, id_base, ts;      // photons, id of photon 0, tile stride of the slab (elements)
    int tile_log;                // log2 of the tile length (pcl_store_layout: 2048 particles)
    int angular, spatial;
    double origin[3], e1[3], e2[3], d[3];
    double c, cos_half_angle, radius;
    uint64_t seed;
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_apply_source(source_args<T> a) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const pcl_u32 k0 = (pcl_u32)a.seed, k1 = (pcl_u32)(a.seed >> 32);
    const bool write_v = a.v[0] != nullptr, write_r = a.r[0] != nullptr;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
        const int64_t ti = (i >> a.tile_log) * a.ts + (i & (((int64_t)1 << a.tile_log) - 1));
        const uint64_t id = (uint64_t)(a.id_base + i);
        if (write_v) {
            if (a.angular == PCL_SRC_BEAM) { // a constant: no draw
#pragma unroll
                for (int k = 0; k < 3; ++k) a.v[k][ti] = (T)__dmul_rn(a.c, a.d[k]);
            } else {
                const pcl_u32x4 w = pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), 0xFFFFFFFFu, 4u, k0, k1);
                const double u_a = pcl_u53(w.x, w.y), u_b = pcl_u53(w.z, w.w);
                double mu; // cosine of the polar angle about d
                if (a.angular == PCL_SRC_ISOTROPIC)
                    mu = __dsub_rn(1.0, __dmul_rn(2.0, u_a));                                         // uniform on the sphere
                else if (a.angular == PCL_SRC_CONE)
                    mu = __dsub_rn(1.0, __dmul_rn(u_a, __dsub_rn(1.0, a.cos_half_angle)));            // uniform in solid angle
                else
                    mu = __dsqrt_rn(__dsub_rn(1.0, u_a));                                             // cosine-weighted hemisphere
                const double s = __dsqrt_rn(__dmul_rn(__dsub_rn(1.0, mu), __dadd_rn(1.0, mu)));
                double sn, cs;
                pcl_sincos_2pi(__dmul_rn(__dmul_rn(u_b, 2.0), PCL_PI), &sn, &cs);                     // the scatter step's angle
                const double sc = __dmul_rn(s, cs), ss = __dmul_rn(s, sn);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double dir = __dadd_rn(__dadd_rn(__dmul_rn(sc, a.e1[k]), __dmul_rn(ss, a.e2[k])), __dmul_rn(mu, a.d[k]));
                    a.v[k][ti] = (T)__dmul_rn(a.c, dir);
                }
            }
        }
        if (write_r) {
            if (a.spatial == PCL_SRC_POINT) {
#pragma unroll
                for (int k = 0; k < 3; ++k) a.r[k][ti] = (T)a.origin[k];
            } else {
                const pcl_u32x4 w = pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), 0xFFFFFFFFu, 5u, k0, k1);
                const double u_c = pcl_u53(w.x, w.y), u_d = pcl_u53(w.z, w.w);
                double rho;
                if (a.spatial == PCL_SRC_DISC)
                    rho = __dmul_rn(a.radius, __dsqrt_rn(u_c));                                       // uniform over the disc
                else                                                                                  // 1 - u_c is in (0, 1]
                    rho = __dmul_rn(a.radius, __dsqrt_rn(__dmul_rn(-2.0, log(__dsub_rn(1.0, u_c)))));
                double sn, cs;
                pcl_sincos_2pi(__dmul_rn(__dmul_rn(u_d, 2.0), PCL_PI), &sn, &cs);
                const double rc = __dmul_rn(rho, cs), rs = __dmul_rn(rho, sn);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    a.r[k][ti] = (T)__dadd_rn(a.origin[k], __dadd_rn(__dmul_rn(rc, a.e1[k]), __dmul_rn(rs, a.e2[k])));
            }
        }
    }
}

// The calling thread's message (pcl_last_error) lives in the core unit and has no setter in the ABI: a refused call leaves
// the core's own generic "bad argument" there (pcl_dev_alloc refuses a negative size), as pcl_spectrum.hip does.
int bad_argument(pcl_ctx *ctx) {
    void *none = nullptr;
    (void)pcl_dev_alloc(ctx, -1, &none);
    return PCL_ERR_ARG;
}

#define SRC_TRY(expr)                    \
    do {                                 \
        int rc__ = (expr);               \
        if (rc__ != PCL_OK) return rc__; \
    } while (0)

bool finite3(const double *x) { return std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]); }

bool source_ok(const pcl_source *s, double c) {
    if (s->angular < PCL_SRC_BEAM || s->angular > PCL_SRC_LAMBERTIAN || s->spatial < PCL_SRC_POINT || s->spatial > PCL_SRC_GAUSSIAN)
        return false;
    if (!finite3(s->origin) || !finite3(s->e1) || !finite3(s->e2) || !finite3(s->d) || !std::isfinite(c)) return false;
    if (s->angular == PCL_SRC_CONE && !(s->cos_half_angle >= -1.0 && s->cos_half_angle <= 1.0)) return false;
    if (s->spatial != PCL_SRC_POINT && !(std::isfinite(s->radius) && s->radius >= 0.0)) return false;
    return true;
}

template <typename T>
int launch_source(pcl_ctx *ctx, const pcl_source *s, bool write_r, bool write_v, source_args<T> &a, int n_cu) {
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *v = nullptr;
        if (write_r) SRC_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        if (write_v) SRC_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &v));
        a.r[k] = static_cast<T *>(r);
        a.v[k] = static_cast<T *>(v);
        a.origin[k] = s->origin[k]; a.e1[k] = s->e1[k]; a.e2[k] = s->e2[k]; a.d[k] = s->d[k];
    }
    void *stream_v = nullptr;
    SRC_TRY(pcl_ctx_stream(ctx, &stream_v));
    const int64_t blocks = (a.n + kBlock - 1) / kBlock, cap = (int64_t)(n_cu > 0 ? n_cu : 256) * kWorkgroupsPerCU;
    hipLaunchKernelGGL(k_apply_source<T>, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(kBlock), 0, static_cast<hipStream_t>(stream_v), a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int apply_source(pcl_ctx *ctx, const pcl_source *s, double c, uint64_t seed) {
    if (!ctx || !s || !source_ok(s, c)) return bad_argument(ctx);
    int uniform = 0;
    SRC_TRY(pcl_store_is_uniform(ctx, &uniform)); // (PCL_ERR_STATE without a store)
    if (!uniform) return PCL_ERR_STATE;           // ids must be id_base + index: a freshly filled population
    int64_t n = 0, id_base = 0, tile = 0, ts = 0;
    SRC_TRY(pcl_store_count(ctx, &n));
    if (n <= 0) return PCL_OK;
    // rows that would not change are not written: the fill left r = 0 and v = (c, 0, 0)
    const bool write_r = s->spatial != PCL_SRC_POINT || s->origin[0] != 0.0 || s->origin[1] != 0.0 || s->origin[2] != 0.0;
    const bool write_v = s->angular != PCL_SRC_BEAM || !(s->d[0] == 1.0 && s->d[1] == 0.0 && s->d[2] == 0.0);
    if (!write_r && !write_v) return PCL_OK;
    SRC_TRY(pcl_store_download_ids(ctx, &id_base, 0, 1)); // (a uniform store keeps no id array: answered on the host)
    int dtype = PCL_DTYPE_F64, n_cu = 0, tile_log = 0;
    SRC_TRY(pcl_store_dtype(ctx, &dtype));
    SRC_TRY(pcl_store_layout(ctx, &tile, &ts));
    while (((int64_t)1 << tile_log) < tile) ++tile_log;
    if (((int64_t)1 << tile_log) != tile) return PCL_ERR_STATE; // the slab's tiles are a power of two long
    SRC_TRY(pcl_ctx_device_info(ctx, nullptr, 0, nullptr, &n_cu, nullptr));
    if (dtype == PCL_DTYPE_F64) {
        source_args<double> a{};
        a.n = n; a.id_base = id_base; a.ts = ts; a.tile_log = tile_log; a.angular = s->angular; a.spatial = s->spatial;
        a.c = c; a.cos_half_angle = s->cos_half_angle; a.radius = s->radius; a.seed = seed;
        return launch_source<double>(ctx, s, write_r, write_v, a, n_cu);
    }
    source_args<float> a{};
    a.n = n; a.id_base = id_base; a.ts = ts; a.tile_log = tile_log; a.angular = s->angular; a.spatial = s->spatial;
    a.c = c; a.cos_half_angle = s->cos_half_angle; a.radius = s->radius; a.seed = seed;
    return launch_source<float>(ctx, s, write_r, write_v, a, n_cu);
}

int group_apply_source(pcl_group *group, const pcl_source *s, double c, uint64_t seed) {
    int n = 0;
    SRC_TRY(pcl_group_size(group, &n));
    std::vector<pcl_ctx *> ctx((size_t)n);
    for (int g = 0; g < n; ++g) SRC_TRY(pcl_group_ctx(group, g, &ctx[(size_t)g]));
    if (!s || !source_ok(s, c)) return bad_argument(n > 0 ? ctx[0] : nullptr); // before any shard is written
    for (int g = 0; g < n; ++g) {
        int uniform = 0;
        SRC_TRY(pcl_store_is_uniform(ctx[(size_t)g], &uniform));
        if (!uniform) return PCL_ERR_STATE;
    }
    std::vector<int> rcs((size_t)n, PCL_OK);
    auto one = [&](int g) { rcs[(size_t)g] = pcl_store_apply_source(ctx[(size_t)g], s, c, seed); };
    // the shards side by side: a thread each per call (the group's own workers cannot be reached through the ABI), the
    // calling thread takes shard 0.  A shard whose thread cannot be started is served by the calling thread.
    std::vector<std::thread> th;
    th.reserve((size_t)n);
    for (int g = 1; g < n; ++g) {
        try {
            th.emplace_back(one, g);
        } catch (const std::system_error &) {
            one(g);
        }
    }
    if (n > 0) one(0);
    for (auto &t : th) t.join();
    for (int g = 0; g < n; ++g) SRC_TRY(rcs[(size_t)g]);
    return PCL_OK;
}

} // namespace

extern "C" {

// Nothing may be thrown through the C boundary (the group form allocates on the host).
int pcl_store_apply_source(pcl_ctx *ctx, const pcl_source *src, double c, uint64_t seed) {
    try {
        return apply_source(ctx, src, c, seed);
    } catch (const std::bad_alloc &) {
        return PCL_ERR_NOMEM;
    } catch (...) {
        return PCL_ERR_HIP;
    }
}

int pcl_group_apply_source(pcl_group *group, const pcl_source *src, double c, uint64_t seed) {
    try {
        return group_apply_source(group, src, c, seed);
    } catch (const std::bad_alloc &) {
        return PCL_ERR_NOMEM;
    } catch (...) {
        return PCL_ERR_HIP;
    }
}

} // extern "C"
