// pcl_source.hip -- photon sources for bulk generation (PhotonSource / generate_photons_bulk(..., source=)).
//
// pcl_store_fill_photons[_table] creates every photon at r = 0 with v = (c, 0, 0).  pcl_store_apply_source gives that fresh
// population its positions and velocities: a point, a disc or a gaussian spot around ``origin``; a beam along ``d``, an
// isotropic point source, a cone or a lambertian (cosine-weighted) emitter about ``d``.
//
// A translation unit of its own, linked into libphysicl_hip.so behind pcl_spectrum.hip: it does not see struct pcl_ctx and
// works through the public C ABI (include/physicl_hip.h) like any other host of the library; pcl_device.h is included for
// the Philox block, the 53-bit uniform and the project's sincos only.  The tuned kernels, their register budgets and the
// source hash the counter records are tied to (physicl_amd/build.py: csrc_sha) are not touched by anything here.  The
// scaffold it shares with the other units of its kind is pcl_sweep.h; the launch geometry is its own (there is nothing
// to flush, so every block's workgroup may as well exist: min(blocks, cap)).
//
//   k_apply_source<T>   one grid-stride sweep of photons [0, n): Philox block 4 of the photon's id for the direction, block 5
//                       for the position (blocks 2 and 3 are the energy draws of k_fill_photons / k_fill_table), so a photon
//                       is the same photon however the run is sharded.  Everything is computed in fp64, unfused, and rounded
//                       once to the store's precision.  Rows that would not change are not written.
#include "pcl_sweep.h"

#include "pcl_device.h" // (after the HIP runtime and the ABI's header, which pcl_sweep.h brings)
#include "pcl_rules.h"  // (after both)

namespace {

using namespace pcl_sweep;
using namespace pcl_rules;

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
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        const uint64_t id = (uint64_t)(a.id_base + i);
        if (write_v) {
            if (a.angular == PCL_SRC_BEAM) { // a constant: no draw
#pragma unroll
                for (int k = 0; k < 3; ++k) a.v[k][ti] = (T)__dmul_rn(a.c, a.d[k]);
            } else {
                const pcl_u32x4 w = pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), 0xFFFFFFFFu, 4u, k0, k1);
                const double u_a = pcl_u53(w.x, w.y), u_b = pcl_u53(w.z, w.w);
                double mu;      // source_mu, in place in both emitters (a helper changes the kernels): the cosine of the polar angle about d
                if (a.angular == PCL_SRC_ISOTROPIC)
                    mu = __dsub_rn(1.0, __dmul_rn(2.0, u_a));                                         // uniform on the sphere
                else if (a.angular == PCL_SRC_CONE)
                    mu = __dsub_rn(1.0, __dmul_rn(u_a, __dsub_rn(1.0, a.cos_half_angle)));            // uniform in solid angle
                else
                    mu = __dsqrt_rn(__dsub_rn(1.0, u_a));                                             // cosine-weighted hemisphere
                double sc, ss; polar(mu, u_b, &sc, &ss);
#pragma unroll
                for (int k = 0; k < 3; ++k) a.v[k][ti] = (T)__dmul_rn(a.c, turned(sc, ss, mu, a.e1[k], a.e2[k], a.d[k]));
            }
        }
        if (write_r) {
            if (a.spatial == PCL_SRC_POINT) {
#pragma unroll
                for (int k = 0; k < 3; ++k) a.r[k][ti] = (T)a.origin[k];
            } else {
                const pcl_u32x4 w = pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), 0xFFFFFFFFu, 5u, k0, k1);
                const double u_c = pcl_u53(w.x, w.y), u_d = pcl_u53(w.z, w.w);
                double rho;     // source_rho, in place in both emitters (a helper changes the kernels): the distance from the origin
                if (a.spatial == PCL_SRC_DISC)
                    rho = __dmul_rn(a.radius, __dsqrt_rn(u_c));                                       // uniform over the disc
                else                                                                                  // 1 - u_c is in (0, 1]
                    rho = __dmul_rn(a.radius, __dsqrt_rn(__dmul_rn(-2.0, log(__dsub_rn(1.0, u_c)))));
                double rc, rs; azimuth(rho, u_d, &rc, &rs);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    a.r[k][ti] = (T)__dadd_rn(a.origin[k], __dadd_rn(__dmul_rn(rc, a.e1[k]), __dmul_rn(rs, a.e2[k])));
            }
        }
    }
}

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
int launch_source(pcl_ctx *ctx, const store_view &v, const pcl_source *s, double c, uint64_t seed, int64_t id_base, bool write_r,
                  bool write_v) {
    source_args<T> a{};
    a.n = v.N; a.id_base = id_base; a.ts = v.ts; a.tile_log = v.tile_log; a.angular = s->angular; a.spatial = s->spatial;
    a.c = c; a.cos_half_angle = s->cos_half_angle; a.radius = s->radius; a.seed = seed;
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr;
        if (write_r) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        if (write_v) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        a.r[k] = static_cast<T *>(r);
        a.v[k] = static_cast<T *>(vel);
        a.origin[k] = s->origin[k]; a.e1[k] = s->e1[k]; a.e2[k] = s->e2[k]; a.d[k] = s->d[k];
    }
    const int64_t blocks = (a.n + kBlock - 1) / kBlock, cap = (int64_t)(v.n_cu > 0 ? v.n_cu : 256) * kWorkgroupsPerCU;
    hipLaunchKernelGGL(k_apply_source<T>, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(kBlock), 0, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int apply_source(pcl_ctx *ctx, const pcl_source *s, double c, uint64_t seed) {
    if (!ctx || !s || !source_ok(s, c)) return bad_argument(ctx);
    int uniform = 0;
    PCL_SWEEP_TRY(pcl_store_is_uniform(ctx, &uniform)); // (PCL_ERR_STATE without a store)
    if (!uniform) return PCL_ERR_STATE;                 // ids must be id_base + index: a freshly filled population
    // rows that would not change are not written: the fill left r = 0 and v = (c, 0, 0)
    const bool write_r = s->spatial != PCL_SRC_POINT || s->origin[0] != 0.0 || s->origin[1] != 0.0 || s->origin[2] != 0.0;
    const bool write_v = s->angular != PCL_SRC_BEAM || !(s->d[0] == 1.0 && s->d[1] == 0.0 && s->d[2] == 0.0);
    if (!write_r && !write_v) return PCL_OK;
    store_view v;
    PCL_SWEEP_TRY(read_store(ctx, &v)); // (no field is looked at first: a uniform store is dense)
    if (v.N <= 0) return PCL_OK;
    int64_t id_base = 0;
    PCL_SWEEP_TRY(pcl_store_download_ids(ctx, &id_base, 0, 1)); // (a uniform store keeps no id array: answered on the host)
    return v.dtype == PCL_DTYPE_F64 ? launch_source<double>(ctx, v, s, c, seed, id_base, write_r, write_v)
                                    : launch_source<float>(ctx, v, s, c, seed, id_base, write_r, write_v);
}

int group_apply_source(pcl_group *group, const pcl_source *s, double c, uint64_t seed) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    if (!s || !source_ok(s, c)) return bad_argument(ctx.empty() ? nullptr : ctx[0]); // before any shard is written
    for (pcl_ctx *one : ctx) {
        int uniform = 0;
        PCL_SWEEP_TRY(pcl_store_is_uniform(one, &uniform));
        if (!uniform) return PCL_ERR_STATE;
    }
    return for_each_shard(ctx, [&](int, pcl_ctx *one) { return pcl_store_apply_source(one, s, c, seed); });
}

} // namespace

extern "C" {

int pcl_store_apply_source(pcl_ctx *ctx, const pcl_source *src, double c, uint64_t seed) {
    return guarded([&] { return apply_source(ctx, src, c, seed); });
}

int pcl_group_apply_source(pcl_group *group, const pcl_source *src, double c, uint64_t seed) {
    return guarded([&] { return group_apply_source(group, src, c, seed); });
}

} // extern "C"
