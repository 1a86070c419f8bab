// pcl_surface.hip -- a reflecting sphere (SurfaceReflectStep): the ground of a radial problem.  Photons whose last move took
// them into the sphere are put back: reflected at the point where the move met the sphere (specular, or cosine-weighted about
// the outward normal), or -- with an albedo below 1 -- absorbed there and left in the store at rest.  Nothing is removed.
//
// A translation unit of its own, linked into libphysicl_hip.so behind the other units on the public ABI: it does not see
// struct pcl_ctx and works through the public C ABI (include/physicl_hip.h) like any other host of the library; pcl_device.h is
// included for the Philox block, the 53-bit uniform and the project's sincos only.  The tuned kernels, their register budgets
// and the source hash the counter records are tied to (physicl_amd/build.py: csrc_sha) are not touched by anything here.  The
// scaffold it shares with the other units of its kind is pcl_sweep.h.
//
//   k_surface_reflect<T>   one grid-stride sweep of the tiled slab: per slot r and dr of the three axes (48 B in fp64), widened
//                          to double; the shell sweep's q_now and q_prev against R*R decide who is hit; one ballot + popcount
//                          per wave for the two counters (LDS cells, flushed with 64-bit atomics).  Only lanes that are hit go
//                          on: they load v (and their id, if the store keeps an array of them), work the hit point and the new
//                          direction out in fp64 -- every operation rounded once, in the order written in
//                          include/physicl_hip.h -- and write r, v, dr, dv rounded once to the store's precision.
//
// Operation order (what light._surface_bounce restates with numpy; x.y of two vectors is always (x0*y0 + x1*y1) + x2*y2):
//   d = r - center, m = dr, p = d - m;  q_now = d.d, q_prev = p.p;  hit iff q_now < R2 <= q_prev < inf, a photon
//   a = m.m;  b = p.m;  cq = q_prev - R2;  disc = max(b*b - a*cq, 0);  t = cq / (sqrt(disc) - b)
//   x_k = p_k + t*m_k;  nrm_k = x_k / sqrt(x.x);  sa = sqrt(a);  w = (1 - t)*sa
//   absorbed (u_0 >= albedo):  r_k = center_k + x_k;  v_k = 0;  dr_k = x_k - p_k;  dv_k = 0 - v_old_k
//   specular:    mh_k = m_k / sa;  dn = mh.nrm;  dir_k = mh_k - (2*dn)*nrm_k
//   lambertian:  mu = sqrt(1 - u_a);  s = sqrt((1 - mu)*(1 + mu));  psi = (u_b*2)*pi;  sc = s*cos psi;  ss = s*sin psi
//                sg = copysign(1, n2);  aa = -1/(sg + n2);  bb = (n0*n1)*aa;  sn0 = sg*n0
//                e1 = (1 + (sn0*n0)*aa, sg*bb, -sn0);  e2 = (bb, sg + (n1*n1)*aa, -n1)        (Duff et al. 2017, branch-free)
//                dir_k = (sc*e1_k + ss*e2_k) + mu*nrm_k
//   reflected:   v_k = c*dir_k;  dv_k = v_k - v_old_k;  dr_k = w*dir_k;  r_k = center_k + (x_k + dr_k)
#include "pcl_sweep.h"

#include "pcl_device.h" // (after the HIP runtime and the ABI's header, which pcl_sweep.h brings)

namespace {

using namespace pcl_sweep;

template <typename T>
struct surface_args {
    T *r[3], *v[3], *dr[3], *dv[3];
    const unsigned char *kind;   // NULL: every particle is a photon
    const int64_t *ids;          // NULL: the id of slot i is id_base + i
    unsigned long long *out;     // [2]: reflected, absorbed; device, zeroed by the entry point
    int64_t N, ts, id_base;      // particles, tile stride of the slab (elements), id of slot 0
    int tile_log;                // log2 of the tile length (pcl_store_layout: 2048 particles)
    int mode;
    double c[3], R2, albedo, speed;
    uint32_t k0, k1, pass;       // Philox key (seed_lo, seed_hi), the step's own pass counter
};

__device__ __forceinline__ double dot3(const double *x, const double *y) {
    return __dadd_rn(__dadd_rn(__dmul_rn(x[0], y[0]), __dmul_rn(x[1], y[1])), __dmul_rn(x[2], y[2]));
}

template <typename T>
__global__ void __launch_bounds__(kBlock) k_surface_reflect(surface_args<T> a) {
    __shared__ uint32_t s_cnt[2];                                       // reflected, absorbed
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // whole waves run the same number of trips (the ballots below need every lane of the wave inside the loop)
    const int64_t n_round = (a.N + 63) / 64 * 64;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        double d[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0}, p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (in) {
                d[k] = __dsub_rn((double)a.r[k][ti], a.c[k]);           // fp32 widens exactly
                m[k] = (double)a.dr[k][ti];
            }
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = __dsub_rn(d[k], m[k]);
        const double q_now = dot3(d, d), q_prev = dot3(p, p);
        // the shell sweep's inward crossing, of photons, with a previous position that can be worked with (NaN: false)
        bool hit = in && q_now < a.R2 && q_prev >= a.R2 && q_prev < INFINITY;
        if (hit && a.kind) hit = a.kind[i] != 0;
        uint64_t id = 0;
        bool refl = hit;
        if (hit) {
            id = (uint64_t)(a.ids ? a.ids[i] : a.id_base + i);
            if (a.albedo < 1.0) {
                const pcl_u32x4 w0 = pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 9u, a.k0, a.k1);
                refl = pcl_u53(w0.x, w0.y) < a.albedo;
            }
        }
        const uint32_t n_hit = (uint32_t)__popcll(__ballot(hit)), n_refl = (uint32_t)__popcll(__ballot(refl));
        if (lane == 0 && n_refl) atomicAdd(&s_cnt[0], n_refl);
        if (lane == 0 && n_hit - n_refl) atomicAdd(&s_cnt[1], n_hit - n_refl);
        if (!hit) continue;     // lanes that are not hit wait at the loop's head: no ballot below this line
        const double aq = dot3(m, m), b = dot3(p, m), cq = __dsub_rn(q_prev, a.R2);
        const double disc = fmax(__dsub_rn(__dmul_rn(b, b), __dmul_rn(aq, cq)), 0.0);
        const double t = __ddiv_rn(cq, __dsub_rn(__dsqrt_rn(disc), b));
        double x[3], nrm[3], vo[3], dir[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] = __dadd_rn(p[k], __dmul_rn(t, m[k]));
            vo[k] = (double)a.v[k][ti];
        }
        if (!refl) {            // absorbed: parked on the sphere, at rest
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a.r[k][ti] = (T)__dadd_rn(a.c[k], x[k]);
                a.v[k][ti] = (T)0.0;
                a.dr[k][ti] = (T)__dsub_rn(x[k], p[k]);
                a.dv[k][ti] = (T)__dsub_rn(0.0, vo[k]);
            }
            continue;
        }
        const double xn = __dsqrt_rn(dot3(x, x)), sa = __dsqrt_rn(aq);
#pragma unroll
        for (int k = 0; k < 3; ++k) nrm[k] = __ddiv_rn(x[k], xn);
        if (a.mode == PCL_SURFACE_SPECULAR) {
            double mh[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) mh[k] = __ddiv_rn(m[k], sa);
            const double dn2 = __dmul_rn(2.0, dot3(mh, nrm));
#pragma unroll
            for (int k = 0; k < 3; ++k) dir[k] = __dsub_rn(mh[k], __dmul_rn(dn2, nrm[k]));
        } else {
            const pcl_u32x4 w = pcl_philox4x32_10((pcl_u32)id, (pcl_u32)(id >> 32), a.pass, 8u, a.k0, a.k1);
            const double u_a = pcl_u53(w.x, w.y), u_b = pcl_u53(w.z, w.w);
            const double mu = __dsqrt_rn(__dsub_rn(1.0, u_a));                                       // cosine-weighted hemisphere
            const double s = __dsqrt_rn(__dmul_rn(__dsub_rn(1.0, mu), __dadd_rn(1.0, mu)));
            double sn, cs;
            pcl_sincos_2pi(__dmul_rn(__dmul_rn(u_b, 2.0), PCL_PI), &sn, &cs);                        // the scatter step's angle
            const double sc = __dmul_rn(s, cs), ss = __dmul_rn(s, sn);
            const double sg = copysign(1.0, nrm[2]);
            const double aa = __ddiv_rn(-1.0, __dadd_rn(sg, nrm[2]));
            const double bb = __dmul_rn(__dmul_rn(nrm[0], nrm[1]), aa), sn0 = __dmul_rn(sg, nrm[0]);
            const double e1[3] = {__dadd_rn(1.0, __dmul_rn(__dmul_rn(sn0, nrm[0]), aa)), __dmul_rn(sg, bb), -sn0};
            const double e2[3] = {bb, __dadd_rn(sg, __dmul_rn(__dmul_rn(nrm[1], nrm[1]), aa)), -nrm[1]};
#pragma unroll
            for (int k = 0; k < 3; ++k)
                dir[k] = __dadd_rn(__dadd_rn(__dmul_rn(sc, e1[k]), __dmul_rn(ss, e2[k])), __dmul_rn(mu, nrm[k]));
        }
        const double w = __dmul_rn(__dsub_rn(1.0, t), sa);              // the rest of the move, flown along the new direction
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double vk = __dmul_rn(a.speed, dir[k]), drk = __dmul_rn(w, dir[k]);
            a.r[k][ti] = (T)__dadd_rn(a.c[k], __dadd_rn(x[k], drk));
            a.v[k][ti] = (T)vk;
            a.dr[k][ti] = (T)drk;
            a.dv[k][ti] = (T)__dsub_rn(vk, vo[k]);
        }
    }
    __syncthreads();
    flush_cells(s_cnt, a.out, 2);
}

struct surface_spec { // a call's arguments, checked
    double c[3] = {0.0, 0.0, 0.0};
    double R2 = 0.0, albedo = 1.0, speed = 0.0;
    int mode = PCL_SURFACE_LAMBERTIAN;
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_spec(double radius, const double *center, double albedo, int mode, double c, const int64_t *counts_out, surface_spec &s) {
    if (!counts_out || (mode != PCL_SURFACE_LAMBERTIAN && mode != PCL_SURFACE_SPECULAR)) return false;
    s.R2 = radius * radius;
    if (!std::isfinite(radius) || !(radius > 0) || !std::isfinite(s.R2)) return false;
    if (!(albedo >= 0.0 && albedo <= 1.0) || !std::isfinite(c)) return false;
    if (center)
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(center[k])) return false;
            s.c[k] = center[k];
        }
    s.albedo = albedo; s.mode = mode; s.speed = c;
    return true;
}

template <typename T>
int launch_surface(pcl_ctx *ctx, const store_view &v, const surface_spec &s, uint64_t seed, uint32_t pass, int64_t id_base,
                   const int64_t *ids, const unsigned char *kind, unsigned long long *out_dev) {
    surface_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *vel = nullptr, *dr = nullptr, *dv = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_V0 + k, &vel));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DV0 + k, &dv));
        a.r[k] = static_cast<T *>(r); a.v[k] = static_cast<T *>(vel);
        a.dr[k] = static_cast<T *>(dr); a.dv[k] = static_cast<T *>(dv);
        a.c[k] = s.c[k];
    }
    a.kind = kind; a.ids = ids; a.out = out_dev;
    a.N = v.N; a.ts = v.ts; a.id_base = id_base; a.tile_log = v.tile_log; a.mode = s.mode;
    a.R2 = s.R2; a.albedo = s.albedo; a.speed = s.speed;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.pass = pass;
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(2 * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_surface_reflect<T>, dim3((unsigned)grid), dim3(kBlock), 0, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int surface_reflect(pcl_ctx *ctx, double radius, const double *center_host, double albedo, int mode, double c, uint64_t seed,
                    uint32_t pass, int64_t *counts_out_host) {
    surface_spec s;
    if (!ctx || !check_spec(radius, center_host, albedo, mode, c, counts_out_host, s)) return bad_argument(ctx);
    // E is never asked for: the pointer costs a wavelength-dependent scatter step its term cache (pcl_shell.hip).
    store_view v;
    PCL_SWEEP_TRY(open_store(ctx, PCL_R0, &v));
    counts_out_host[0] = counts_out_host[1] = 0;
    if (v.N <= 0) return PCL_OK;
    // a store that is not uniform: the kinds go along if it holds a plain Object, the ids if they are not id[0] + index --
    // both come over the host link and go back up, every call (pcl_sweep::id_words / kind_bytes say what that costs)
    std::vector<uint8_t> kind_host;
    std::vector<int64_t> ids_host;
    bool mixed = false;
    int64_t id_base = 0;
    PCL_SWEEP_TRY(kind_bytes(ctx, v.N, kind_host, &mixed));
    PCL_SWEEP_TRY(id_words(ctx, v.N, ids_host, &id_base));
    const size_t out_bytes = 2 * sizeof(uint64_t), id_bytes = ids_host.size() * sizeof(int64_t);
    dev_block blk(ctx);
    PCL_SWEEP_TRY(stage(blk, v.stream, out_bytes, nullptr, 0, kind_host, ids_host));
    char *base = static_cast<char *>(blk.p);
    const int64_t *ids = id_bytes ? reinterpret_cast<const int64_t *>(base + out_bytes) : nullptr;
    const unsigned char *kind = mixed ? reinterpret_cast<const unsigned char *>(base + out_bytes + id_bytes) : nullptr;
    unsigned long long *out_dev = reinterpret_cast<unsigned long long *>(base);
    PCL_SWEEP_TRY(v.dtype == PCL_DTYPE_F64 ? launch_surface<double>(ctx, v, s, seed, pass, id_base, ids, kind, out_dev)
                                           : launch_surface<float>(ctx, v, s, seed, pass, id_base, ids, kind, out_dev));
    return pcl_d2h(ctx, counts_out_host, base, (int64_t)out_bytes); // the call's one synchronisation (a count is below 2^63)
}

int group_surface_reflect(pcl_group *group, double radius, const double *center_host, double albedo, int mode, double c,
                          uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    surface_spec s;
    if (n < 1 || !check_spec(radius, center_host, albedo, mode, c, counts_out_host, s)) return bad_argument(n > 0 ? ctx[0] : nullptr);
    std::vector<int64_t> part((size_t)2 * n, 0);
    PCL_SWEEP_TRY(for_each_shard(ctx, [&](int g, pcl_ctx *one) {
        return pcl_step_surface_reflect(one, radius, center_host, albedo, mode, c, seed, pass, &part[(size_t)2 * g]);
    }));
    counts_out_host[0] = counts_out_host[1] = 0;
    for (int g = 0; g < n; ++g) {
        counts_out_host[0] += part[(size_t)2 * g];
        counts_out_host[1] += part[(size_t)2 * g + 1];
    }
    return PCL_OK;
}

} // namespace

extern "C" {

int pcl_step_surface_reflect(pcl_ctx *ctx, double radius, const double *center_host, double albedo, int mode, double c, uint64_t seed,
                             uint32_t pass, int64_t *counts_out_host) {
    return guarded([&] { return surface_reflect(ctx, radius, center_host, albedo, mode, c, seed, pass, counts_out_host); });
}

int pcl_group_step_surface_reflect(pcl_group *group, double radius, const double *center_host, double albedo, int mode, double c,
                                   uint64_t seed, uint32_t pass, int64_t *counts_out_host) {
    return guarded([&] { return group_surface_reflect(group, radius, center_host, albedo, mode, c, seed, pass, counts_out_host); });
}

} // extern "C"
