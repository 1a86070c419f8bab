// pcl_shell.hip -- spherical-shell crossing tallies (ShellCrossingMeasureStep): what passed through the spheres of a radial
// problem in the last move -- per shell the particles that went out and the ones that came in, the crossing photons'
// energies and the cosine of the move against the local vertical as integer histograms --, made in one read-only sweep of
// the resident store.
//
// A translation unit of its own, linked into libphysicl_hip.so between pcl_source.hip and pcl_grid.hip: it does not see
// struct pcl_ctx and works through the public C ABI (include/physicl_hip.h) like any other host of the library.  The tuned
// kernels, their register budgets and the source hash the counter records are tied to (physicl_amd/build.py: csrc_sha) are
// not touched by anything here.  The scaffold it shares with the other units of its kind is pcl_sweep.h.
//
//   k_shell_crossings<T>   one grid-stride sweep of the tiled slab for ALL shells of a call: per slot r and dr of the three
//                          axes (48 B in fp64), widened to double; q_now and q_prev against R*R of every shell (LDS), one
//                          ballot + popcount per shell and direction for the counts; lanes that crossed look E up in the
//                          energy edges and W = s*|s| against w_b*D in the direction edges (LDS, binary searches, no square
//                          root and no division) and add to workgroup-private uint32 histograms in LDS; a workgroup
//                          flushes its non-zero cells with 64-bit atomics at the end.
//
// Beside it, the crossing tally of a finite instrument (DetectorMeasureStep): what went through a small oriented aperture in
// the last move, sorted by the direction it came from into the pixels of a pinhole camera and -- when asked for -- by energy
// into bands.
//
//   k_detector_image<T>    one grid-stride sweep of the tiled slab, the same 48 B per slot: a = r - p and b = a - dr against the
//                          aperture's plane (front to back: s_prev > 0 >= s_now), the hit point times D against R*R*(D*D), the
//                          direction the photon came from against the pixel edges times wn (LDS, binary searches; no division,
//                          no square root); one ballot + popcount each for the two counts; the few lanes that are seen add to
//                          their image cell with a 64-bit atomic straight on the device block -- an aperture is small, so there
//                          is no histogram in LDS and no flush, and the image may be large.
//
// And at the end of the unit the crossing tally of horizontal levels by column (PlaneFluxMapStep), k_plane_flux<T, lds>, described
// where it stands.
#include "pcl_sweep.h"

namespace {

using namespace pcl_sweep;

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
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
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
                const int lo = bin_of(s_w, nmu, W, D);
                for (uint32_t x = crossed; x; x &= x - 1) {
                    const int bit = __ffs(x) - 1;
                    atomicAdd(&s_muh[((bit >> 4) * S + (bit & 15)) * nmu + lo], 1u);
                }
            }
        }
    }
    __syncthreads();
    flush_cells(s_cnt, a.out, n_cells);
}

struct shell_spec { // a call's arguments, checked; what the kernel compares against
    int n_shells = 0, n_E = 0, n_mu = 0;
    double c[3] = {0.0, 0.0, 0.0};
    std::vector<double> tables; // E edges | w_b | R*R
    size_t cells() const { return (size_t)2 * n_shells * (1 + n_E + n_mu); }
    spans out(int64_t *counts, int64_t *E_hist, int64_t *mu_hist) const {
        const size_t n_cnt = (size_t)2 * n_shells;
        return {{counts, n_cnt}, {E_hist, n_cnt * n_E}, {mu_hist, n_cnt * n_mu}};
    }
};

// n + 1 finite, strictly increasing edges, 1 <= n <= PCL_SHELL_MAX_BINS -- or none at all (NULL or not, 0 bins)
bool check_bins(const double *edges, int n, const int64_t *out, edge_transform t, std::vector<double> &to) {
    if (n == 0) return true;
    return n > 0 && n <= PCL_SHELL_MAX_BINS && edges && out && check_edges(edges, n, t, &to);
}

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_spec(int n_shells, const double *radii, const double *center, const double *E_edges, int n_E, const double *mu_edges,
                int n_mu, const int64_t *counts_out, const int64_t *E_out, const int64_t *mu_out, shell_spec &s) {
    if (!radii || !counts_out || n_shells < 1 || n_shells > PCL_SHELL_MAX_SHELLS) return false;
    if (!check_bins(E_edges, n_E, E_out, kEdgePlain, s.tables)) return false;
    if (!check_bins(mu_edges, n_mu, mu_out, kEdgeSignedSquare, s.tables)) return false;
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

template <typename T>
int launch_shell(pcl_ctx *ctx, const store_view &v, const shell_spec &s, const void *E, const staged &st) {
    shell_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *dr = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));
        a.r[k] = static_cast<const T *>(r);
        a.dr[k] = static_cast<const T *>(dr);
        a.c[k] = s.c[k];
    }
    a.E = static_cast<const T *>(E); a.kind = st.kind; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.tile_log = v.tile_log;
    a.n_shells = s.n_shells; a.n_E = s.n_E; a.n_mu = s.n_mu;
    const size_t lds = s.tables.size() * sizeof(double) + s.cells() * sizeof(uint32_t);
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    hipLaunchKernelGGL(k_shell_crossings<T>, dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int shell_crossings(pcl_ctx *ctx, int n_shells, const double *radii_host, const double *center_host, const double *E_edges_host,
                    int n_E_bins, const double *mu_edges_host, int n_mu_bins, int64_t *counts_out_host, int64_t *E_hist_out_host,
                    int64_t *mu_hist_out_host) {
    shell_spec s;
    if (!ctx || !check_spec(n_shells, radii_host, center_host, E_edges_host, n_E_bins, mu_edges_host, n_mu_bins, counts_out_host,
                            E_hist_out_host, mu_hist_out_host, s))
        return bad_argument(ctx);
    // E is asked for only with energy bins: the pointer costs a wavelength-dependent scatter step its term cache.
    const spans out = s.out(counts_out_host, E_hist_out_host, mu_hist_out_host);
    store_view v;
    staged st(ctx);
    void *E = nullptr;
    PCL_SWEEP_TRY(open_store(ctx, PCL_R0, &v));
    if (s.n_E) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    if (v.N <= 0) {
        zero_spans(out);
        return PCL_OK;
    }
    // the kinds go along when energies are binned and the store holds a plain Object; nothing is drawn: no ids
    PCL_SWEEP_TRY(stage(st, v, s.cells(), s.tables.data(), s.tables.size(), false, s.n_E > 0));
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_shell, ctx, v, s, E, st));
    return fetch(st, out);
}

int group_shell_crossings(pcl_group *group, int n_shells, const double *radii_host, const double *center_host,
                          const double *E_edges_host, int n_E_bins, const double *mu_edges_host, int n_mu_bins, int64_t *counts_out_host,
                          int64_t *E_hist_out_host, int64_t *mu_hist_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    shell_spec s;
    if (n < 1 || !check_spec(n_shells, radii_host, center_host, E_edges_host, n_E_bins, mu_edges_host, n_mu_bins, counts_out_host,
                             E_hist_out_host, mu_hist_out_host, s))
        return bad_argument(n > 0 ? ctx[0] : nullptr);
    const size_t n_cnt = (size_t)2 * n_shells;
    return sum_shards(ctx, s.out(counts_out_host, E_hist_out_host, mu_hist_out_host), [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_shell_crossings(one, n_shells, radii_host, center_host, E_edges_host, n_E_bins, mu_edges_host, n_mu_bins, p,
                                        p + n_cnt, p + n_cnt * (1 + (size_t)n_E_bins));
    });
}

// ---------------------------------------------------------------------------------------------- the aperture's image
template <typename T>
struct detector_args {
    const T *r[3], *dr[3];
    const T *E;                  // NULL without bands
    const unsigned char *kind;   // NULL: every particle is a photon
    const double *tables;        // x edges (nx + 1) | y edges (ny + 1) | E edges (n_E + 1, if any), device
    unsigned long long *out;     // through, seen | image [max(n_E, 1)][ny][nx], device, zeroed by the entry point
    int64_t N, ts;               // particles, tile stride of the slab (elements)
    int tile_log;                // log2 of the tile length
    int nx, ny, n_E;
    double p[3], e1[3], e2[3], n[3], R2;
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_detector_image(detector_args<T> a) {
    extern __shared__ double s_det[];                                  // the three edge tables, nothing else
    const int nx = a.nx, ny = a.ny, nE = a.n_E;
    const int n_tab = (nx + 1) + (ny + 1) + (nE ? nE + 1 : 0);
    const double *s_x = s_det, *s_y = s_x + (nx + 1), *s_E = s_y + (ny + 1);
    for (int k = threadIdx.x; k < n_tab; k += kBlock) s_det[k] = a.tables[k];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // whole waves run the same number of trips (the ballots below need every lane of the wave inside the loop)
    const int64_t n_round = (a.N + 63) / 64 * 64;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        double d[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (in) {
                d[k] = (double)a.r[k][ti] - a.p[k];                    // fp32 widens exactly
                m[k] = (double)a.dr[k][ti];
            }
        // unfused, in this order (the library is built with -ffp-contract=off)
        const double b0 = d[0] - m[0], b1 = d[1] - m[1], b2 = d[2] - m[2];            // where the move began
        const double s_now = (d[0] * a.n[0] + d[1] * a.n[1]) + d[2] * a.n[2];
        const double s_prev = (b0 * a.n[0] + b1 * a.n[1]) + b2 * a.n[2];
        const bool crossed = in && s_prev > 0.0 && s_now <= 0.0;       // front to back; ending on the plane: arrived (NaN: neither)
        const double D = s_prev - s_now;
        const double H0 = b0 * D + m[0] * s_prev, H1 = b1 * D + m[1] * s_prev, H2 = b2 * D + m[2] * s_prev;   // the hit point times D
        const double hh = (H0 * H0 + H1 * H1) + H2 * H2, lim = a.R2 * (D * D);
        const bool through = crossed && hh <= lim && lim < INFINITY;   // the rim is inside
        const double wn = -((m[0] * a.n[0] + m[1] * a.n[1]) + m[2] * a.n[2]);
        const double ax = -((m[0] * a.e1[0] + m[1] * a.e1[1]) + m[2] * a.e1[2]);
        const double ay = -((m[0] * a.e2[0] + m[1] * a.e2[1]) + m[2] * a.e2[2]);
        // the direction it came from, gnomonic: ax / wn, ay / wn inside the edges -- compared as ax against e * wn, wn > 0
        const bool seen = through && wn > 0.0 && wn < INFINITY && s_x[0] * wn <= ax && ax <= s_x[nx] * wn && s_y[0] * wn <= ay &&
                          ay <= s_y[ny] * wn;
        const unsigned long long n_through = (unsigned long long)__popcll(__ballot(through));
        const unsigned long long n_seen = (unsigned long long)__popcll(__ballot(seen));
        if (lane == 0 && n_through) atomicAdd(&a.out[0], n_through);
        if (lane == 0 && n_seen) atomicAdd(&a.out[1], n_seen);
        if (!seen) continue;    // lanes that saw nothing wait at the loop's head: no ballot below this line
        int band = 0;
        if (nE) {
            if (a.kind ? a.kind[i] == 0 : false) continue;             // plain Objects carry no energy: seen, in no cell
            const double e = (double)a.E[ti];
            if (!(e >= s_E[0] && e <= s_E[nE])) continue;              // NaN and under/overflow: seen, in no cell
            band = bin_of(s_E, nE, e);
        }
        const int col = bin_of(s_x, nx, ax, wn), row = bin_of(s_y, ny, ay, wn);
        // band, row and col come from bin_of alone, which answers [0, n - 1] for n bins (lo starts at 0 and only ever becomes a
        // mid < n): the cell lies in [0, max(n_E, 1) * ny * nx), the block the entry point allocated behind the two counts
        atomicAdd(&a.out[2 + ((size_t)band * ny + row) * nx + col], 1ull);
    }
}

struct detector_spec { // a call's arguments, checked; what the kernel compares against
    int nx = 0, ny = 0, n_E = 0;
    double p[3], frame[9], R2 = 0.0;
    std::vector<double> tables; // x edges | y edges | E edges
    size_t image_cells() const { return (size_t)(n_E > 0 ? n_E : 1) * ny * nx; }
    size_t cells() const { return 2 + image_cells(); }
    spans out(int64_t *counts, int64_t *image) const { return {{counts, 2}, {image, image_cells()}}; }
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_detector(const double *position, const double *frame, double radius, const double *x_edges, int nx, const double *y_edges,
                    int ny, const double *E_edges, int n_E, const int64_t *counts_out, const int64_t *image_out, detector_spec &s) {
    if (!position || !frame || !x_edges || !y_edges || !counts_out || !image_out) return false;
    if (nx < 1 || nx > PCL_DETECTOR_MAX_PIXELS || ny < 1 || ny > PCL_DETECTOR_MAX_PIXELS) return false;
    if (n_E < 0 || n_E > PCL_DETECTOR_MAX_BANDS || (n_E > 0 && !E_edges)) return false;
    if ((int64_t)(n_E > 0 ? n_E : 1) * ny * nx > PCL_DETECTOR_MAX_CELLS) return false;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(position[k])) return false;
        s.p[k] = position[k];
    }
    for (int k = 0; k < 9; ++k) {
        if (!std::isfinite(frame[k])) return false;
        s.frame[k] = frame[k];
    }
    if (frame[6] == 0.0 && frame[7] == 0.0 && frame[8] == 0.0) return false;      // a plane needs a normal
    s.R2 = radius * radius;
    if (!std::isfinite(radius) || !(radius > 0) || !std::isfinite(s.R2)) return false;
    if (!check_edges(x_edges, nx, kEdgePlain, &s.tables) || !check_edges(y_edges, ny, kEdgePlain, &s.tables)) return false;
    if (n_E > 0 && !check_edges(E_edges, n_E, kEdgePlain, &s.tables)) return false;
    s.nx = nx; s.ny = ny; s.n_E = n_E;
    return true;
}

template <typename T>
int launch_detector(pcl_ctx *ctx, const store_view &v, const detector_spec &s, const void *E, const staged &st) {
    detector_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *dr = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + k, &dr));
        a.r[k] = static_cast<const T *>(r);
        a.dr[k] = static_cast<const T *>(dr);
        a.p[k] = s.p[k]; a.e1[k] = s.frame[k]; a.e2[k] = s.frame[3 + k]; a.n[k] = s.frame[6 + k];
    }
    a.E = static_cast<const T *>(E); a.kind = st.kind; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.tile_log = v.tile_log;
    a.nx = s.nx; a.ny = s.ny; a.n_E = s.n_E; a.R2 = s.R2;
    const size_t lds = s.tables.size() * sizeof(double);               // at most 3 x 1025 doubles
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    hipLaunchKernelGGL(k_detector_image<T>, dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int detector_image(pcl_ctx *ctx, const double *position_host, const double *frame_host, double radius, const double *x_edges_host, int nx,
                   const double *y_edges_host, int ny, const double *E_edges_host, int n_E_bins, int64_t *counts_out_host,
                   int64_t *image_out_host) {
    detector_spec s;
    if (!ctx || !check_detector(position_host, frame_host, radius, x_edges_host, nx, y_edges_host, ny, E_edges_host, n_E_bins,
                                counts_out_host, image_out_host, s))
        return bad_argument(ctx);
    // E is asked for only with bands: the pointer costs a wavelength-dependent scatter step its term cache.
    const spans out = s.out(counts_out_host, image_out_host);
    store_view v;
    staged st(ctx);
    void *E = nullptr;
    PCL_SWEEP_TRY(open_store(ctx, PCL_R0, &v));
    if (s.n_E) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    if (v.N <= 0) {
        zero_spans(out);
        return PCL_OK;
    }
    // the kinds go along when energies are binned and the store holds a plain Object; nothing is drawn: no ids
    PCL_SWEEP_TRY(stage(st, v, s.cells(), s.tables.data(), s.tables.size(), false, s.n_E > 0));
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_detector, ctx, v, s, E, st));
    return fetch(st, out);
}

int group_detector_image(pcl_group *group, const double *position_host, const double *frame_host, double radius,
                         const double *x_edges_host, int nx, const double *y_edges_host, int ny, const double *E_edges_host, int n_E_bins,
                         int64_t *counts_out_host, int64_t *image_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    detector_spec s;
    if (n < 1 || !check_detector(position_host, frame_host, radius, x_edges_host, nx, y_edges_host, ny, E_edges_host, n_E_bins,
                                 counts_out_host, image_out_host, s))
        return bad_argument(n > 0 ? ctx[0] : nullptr);
    return sum_shards(ctx, s.out(counts_out_host, image_out_host), [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_detector_image(one, position_host, frame_host, radius, x_edges_host, nx, y_edges_host, ny, E_edges_host, n_E_bins,
                                       p, p + 2);
    });
}

// ---------------------------------------------------------------------------------------------- the flux maps of planes
// Up and down fluxes through the planes normal to one axis, resolved by column (PlaneFluxMapStep): the shells' change of side,
// counted exactly once, and the detector's hit point without a division, sorted into the cells of a map.
//
//   k_plane_flux<T, lds>   one grid-stride sweep of the tiled slab for ALL levels of a call: per slot r and dr of the normal axis
//                          (16 B in fp64) against every level (LDS), one ballot + popcount per level and direction for the counts;
//                          only the lanes that crossed load r and dr of the two transverse axes (and E with bands), make the hit
//                          point times D per level and look it up in the edges times D (LDS, binary searches, no division);
//                          lds: the maps are workgroup-private uint32 cells in LDS, flushed at the end; otherwise the lanes add to
//                          the device block with 64-bit atomics and only the 2S counts stay in LDS.
// The LDS form's switch-over is the siblings' (k_scatter_grid, k_absorb_grid): it was not tuned for this kernel.
constexpr int kPlaneFluxLdsCells = PCL_PLANE_FLUX_LDS_CELLS;
constexpr size_t kPlaneFluxLdsBytes = PCL_PLANE_FLUX_LDS_BYTES;

template <typename T>
struct pflux_args {
    const T *ra, *dra;           // r and dr along the normal
    const T *rt[2], *drt[2];     // r and dr along u and v
    const T *E;                  // NULL without bands
    const unsigned char *kind;   // NULL: every particle is a photon
    const double *tables;        // levels (S) | u edges (n_u + 1) | v edges (n_v + 1) | E edges (n_E + 1, if any), device
    unsigned long long *out;     // counts [2][S] | maps [2][S][max(n_E, 1)][n_u][n_v], device, zeroed by the entry point
    int64_t N, ts;               // particles, tile stride of the slab (elements)
    int tile_log;                // log2 of the tile length
    int S, n_u, n_v, n_E;
};

template <typename T, bool kLds>
__global__ void __launch_bounds__(kBlock) k_plane_flux(pflux_args<T> a) {
    extern __shared__ double s_flux[];                                 // tables | counts | maps (LDS form)
    const int S = a.S, nu = a.n_u, nv = a.n_v, nE = a.n_E, nB = nE ? nE : 1;
    const int n_tab = S + (nu + 1) + (nv + 1) + (nE ? nE + 1 : 0);
    const int n_map = 2 * S * nB * nu * nv;                            // at most PCL_PLANE_FLUX_MAX_CELLS
    const int n_cnt = 2 * S + (kLds ? n_map : 0);
    const double *s_lev = s_flux, *s_u = s_lev + S, *s_v = s_u + (nu + 1), *s_E = s_v + (nv + 1);
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_flux + n_tab);
    uint32_t *s_map = s_cnt + 2 * S;
    for (int k = threadIdx.x; k < n_tab; k += kBlock) s_flux[k] = a.tables[k];
    for (int k = threadIdx.x; k < n_cnt; k += kBlock) s_cnt[k] = 0;    // (the maps follow the counts)
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // whole waves run the same number of trips (the ballots below need every lane of the wave inside the loop)
    const int64_t n_round = (a.N + 63) / 64 * 64;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_round; i += stride) {
        const bool in = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        double now = 0.0, m = 0.0;
        if (in) {
            now = (double)a.ra[ti];                                    // fp32 widens exactly
            m = (double)a.dra[ti];
        }
        const double prev = now - m;
        uint32_t crossed = 0;   // bit s: up through level s in the last move, bit 16 + s: down (NaN: neither)
        for (int s = 0; s < S; ++s) {
            const double X = s_lev[s];
            const bool up = in && prev < X && now >= X, dn = in && prev >= X && now < X;      // on the plane is above
            const uint32_t n_up = (uint32_t)__popcll(__ballot(up)), n_dn = (uint32_t)__popcll(__ballot(dn));
            if (lane == 0 && n_up) atomicAdd(&s_cnt[s], n_up);
            if (lane == 0 && n_dn) atomicAdd(&s_cnt[S + s], n_dn);
            crossed |= (up ? 1u << s : 0u) | (dn ? 0x10000u << s : 0u);
        }
        if (!crossed) continue; // lanes that crossed nothing wait at the loop's head: no ballot below this line
        int band = 0;
        if (nE) {
            if (a.kind ? a.kind[i] == 0 : false) continue;             // plain Objects carry no energy: counted, in no cell
            const double e = (double)a.E[ti];
            if (!(e >= s_E[0] && e <= s_E[nE])) continue;              // NaN and under/overflow: counted, in no cell
            band = bin_of(s_E, nE, e);
        }
        const double D = fabs(m);
        if (!(D < INFINITY)) continue;                                 // an infinite move: counted, in no cell
        const double du = (double)a.drt[0][ti], dv = (double)a.drt[1][ti];
        const double pu = (double)a.rt[0][ti] - du, pv = (double)a.rt[1][ti] - dv;            // where the move began
        // unfused, in this order (the library is built with -ffp-contract=off)
        for (uint32_t x = crossed; x; x &= x - 1) {
            const int bit = __ffs(x) - 1, s = bit & 15;
            const double G = fabs(s_lev[s] - prev);
            const double Hu = pu * D + du * G, Hv = pv * D + dv * G;   // the crossing point times D
            // p_t + dr_t*G/D in bin b iff e_b*D <= H_t < e_(b+1)*D: one multiply per probe, rounded products are monotone in b
            if (!(fabs(Hu) < INFINITY && fabs(Hv) < INFINITY)) continue;
            if (!(Hu >= s_u[0] * D && Hu <= s_u[nu] * D && Hv >= s_v[0] * D && Hv <= s_v[nv] * D)) continue;
            const int iu = bin_of(s_u, nu, Hu, D), iv = bin_of(s_v, nv, Hv, D);
            // band, iu and iv come from bin_of alone, which answers [0, n - 1] for n bins; s < S and bit >> 4 is 0 or 1: the cell
            // lies in [0, n_map), the block behind the 2S counts -- in LDS (the launch asked for it) or on the device
            const int cell = ((((bit >> 4) * S + s) * nB + band) * nu + iu) * nv + iv;
            if (kLds) atomicAdd(&s_map[cell], 1u);
            else atomicAdd(&a.out[2 * S + cell], 1ull);
        }
    }
    __syncthreads();
    flush_cells(s_cnt, a.out, n_cnt);
}

struct pflux_spec { // a call's arguments, checked; what the kernel compares against
    int axis = 0, S = 0, n_u = 0, n_v = 0, n_E = 0;
    std::vector<double> tables; // levels | u edges | v edges | E edges
    size_t n_cnt() const { return (size_t)2 * S; }
    size_t n_map() const { return (size_t)2 * S * (n_E > 0 ? n_E : 1) * n_u * n_v; }
    size_t cells() const { return n_cnt() + n_map(); }
    size_t lds_small() const { return tables.size() * sizeof(double) + n_cnt() * sizeof(uint32_t); }          // the global form's
    size_t lds_whole() const { return lds_small() + n_map() * sizeof(uint32_t); }                               // the LDS form's
    bool lds_form() const { return n_map() <= (size_t)kPlaneFluxLdsCells && lds_whole() <= kPlaneFluxLdsBytes; }
    spans out(int64_t *counts, int64_t *maps) const { return {{counts, n_cnt()}, {maps, n_map()}}; }
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_pflux(int axis, int n_levels, const double *levels, const double *u_edges, int n_u, const double *v_edges, int n_v,
                 const double *E_edges, int n_E, const int64_t *counts_out, const int64_t *maps_out, pflux_spec &s) {
    if (!levels || !u_edges || !v_edges || !counts_out || !maps_out) return false;
    if (axis < 0 || axis > 2 || n_levels < 1 || n_levels > PCL_PLANE_FLUX_MAX_LEVELS) return false;
    if (n_u < 1 || n_u > PCL_PLANE_FLUX_MAX_BINS || n_v < 1 || n_v > PCL_PLANE_FLUX_MAX_BINS) return false;
    if (n_E < 0 || n_E > PCL_PLANE_FLUX_MAX_BANDS || (n_E > 0 && !E_edges)) return false;
    if ((int64_t)2 * n_levels * (n_E > 0 ? n_E : 1) * n_u * n_v > PCL_PLANE_FLUX_MAX_CELLS) return false;
    for (int k = 0; k < n_levels; ++k) {
        if (!std::isfinite(levels[k]) || (k > 0 && !(levels[k] > levels[k - 1]))) return false;
        s.tables.push_back(levels[k]);
    }
    if (!check_edges(u_edges, n_u, kEdgePlain, &s.tables) || !check_edges(v_edges, n_v, kEdgePlain, &s.tables)) return false;
    if (n_E > 0 && !check_edges(E_edges, n_E, kEdgePlain, &s.tables)) return false;
    s.axis = axis; s.S = n_levels; s.n_u = n_u; s.n_v = n_v; s.n_E = n_E;
    return true;
}

template <typename T>
int launch_pflux(pcl_ctx *ctx, const store_view &v, const pflux_spec &s, const void *E, const staged &st) {
    pflux_args<T> a{};
    const int tu = s.axis == 0 ? 1 : 0, tv = s.axis == 2 ? 1 : 2;      // the remaining two axes, in x, y, z order
    const int axes[3] = {s.axis, tu, tv};
    for (int k = 0; k < 3; ++k) {
        void *r = nullptr, *dr = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + axes[k], &r));
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_DR0 + axes[k], &dr));
        if (k == 0) {
            a.ra = static_cast<const T *>(r); a.dra = static_cast<const T *>(dr);
        } else {
            a.rt[k - 1] = static_cast<const T *>(r); a.drt[k - 1] = static_cast<const T *>(dr);
        }
    }
    a.E = static_cast<const T *>(E); a.kind = st.kind; a.tables = st.tables; a.out = st.out;
    a.N = v.N; a.ts = v.ts; a.tile_log = v.tile_log;
    a.S = s.S; a.n_u = s.n_u; a.n_v = s.n_v; a.n_E = s.n_E;
    const bool lds_form = s.lds_form();
    const size_t lds = lds_form ? s.lds_whole() : s.lds_small();       // at most 64 KiB either way
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    if (lds_form) hipLaunchKernelGGL((k_plane_flux<T, true>), dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    else hipLaunchKernelGGL((k_plane_flux<T, false>), dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int plane_flux(pcl_ctx *ctx, int axis, int n_levels, const double *levels_host, const double *u_edges_host, int n_u,
               const double *v_edges_host, int n_v, const double *E_edges_host, int n_E_bins, int64_t *counts_out_host,
               int64_t *maps_out_host) {
    pflux_spec s;
    if (!ctx || !check_pflux(axis, n_levels, levels_host, u_edges_host, n_u, v_edges_host, n_v, E_edges_host, n_E_bins, counts_out_host,
                             maps_out_host, s))
        return bad_argument(ctx);
    // E is asked for only with bands: the pointer costs a wavelength-dependent scatter step its term cache.
    const spans out = s.out(counts_out_host, maps_out_host);
    store_view v;
    staged st(ctx);
    void *E = nullptr;
    PCL_SWEEP_TRY(open_store(ctx, PCL_R0, &v));
    if (s.n_E) PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_E, &E));
    if (v.N <= 0) {
        zero_spans(out);
        return PCL_OK;
    }
    // the kinds go along when energies are binned and the store holds a plain Object; nothing is drawn: no ids
    PCL_SWEEP_TRY(stage(st, v, s.cells(), s.tables.data(), s.tables.size(), false, s.n_E > 0));
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_pflux, ctx, v, s, E, st));
    return fetch(st, out);
}

int group_plane_flux(pcl_group *group, int axis, int n_levels, const double *levels_host, const double *u_edges_host, int n_u,
                     const double *v_edges_host, int n_v, const double *E_edges_host, int n_E_bins, int64_t *counts_out_host,
                     int64_t *maps_out_host) {
    pflux_spec s;                                                       // the arguments first: a refused call looks at no group
    if (!check_pflux(axis, n_levels, levels_host, u_edges_host, n_u, v_edges_host, n_v, E_edges_host, n_E_bins, counts_out_host,
                     maps_out_host, s))
        return bad_argument(nullptr);
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    if (ctx.empty()) return bad_argument(nullptr);
    return sum_shards(ctx, s.out(counts_out_host, maps_out_host), [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_plane_flux(one, axis, n_levels, levels_host, u_edges_host, n_u, v_edges_host, n_v, E_edges_host, n_E_bins, p,
                                   p + s.n_cnt());
    });
}

} // namespace

extern "C" {

int pcl_step_shell_crossings(pcl_ctx *ctx, int n_shells, const double *radii_host, const double *center_host, const double *E_edges_host,
                             int n_E_bins, const double *mu_edges_host, int n_mu_bins, int64_t *counts_out_host, int64_t *E_hist_out_host,
                             int64_t *mu_hist_out_host) {
    return guarded([&] {
        return shell_crossings(ctx, n_shells, radii_host, center_host, E_edges_host, n_E_bins, mu_edges_host, n_mu_bins, counts_out_host,
                               E_hist_out_host, mu_hist_out_host);
    });
}

int pcl_group_step_shell_crossings(pcl_group *group, int n_shells, const double *radii_host, const double *center_host,
                                   const double *E_edges_host, int n_E_bins, const double *mu_edges_host, int n_mu_bins,
                                   int64_t *counts_out_host, int64_t *E_hist_out_host, int64_t *mu_hist_out_host) {
    return guarded([&] {
        return group_shell_crossings(group, n_shells, radii_host, center_host, E_edges_host, n_E_bins, mu_edges_host, n_mu_bins,
                                     counts_out_host, E_hist_out_host, mu_hist_out_host);
    });
}

int pcl_step_detector_image(pcl_ctx *ctx, const double *position_host, const double *frame_host, double radius,
                            const double *x_edges_host, int nx, const double *y_edges_host, int ny, const double *E_edges_host,
                            int n_E_bins, int64_t *counts_out_host, int64_t *image_out_host) {
    return guarded([&] {
        return detector_image(ctx, position_host, frame_host, radius, x_edges_host, nx, y_edges_host, ny, E_edges_host, n_E_bins,
                              counts_out_host, image_out_host);
    });
}

int pcl_group_step_detector_image(pcl_group *group, const double *position_host, const double *frame_host, double radius,
                                  const double *x_edges_host, int nx, const double *y_edges_host, int ny, const double *E_edges_host,
                                  int n_E_bins, int64_t *counts_out_host, int64_t *image_out_host) {
    return guarded([&] {
        return group_detector_image(group, position_host, frame_host, radius, x_edges_host, nx, y_edges_host, ny, E_edges_host, n_E_bins,
                                    counts_out_host, image_out_host);
    });
}

int pcl_step_plane_flux(pcl_ctx *ctx, int axis, int n_levels, const double *levels_host, const double *u_edges_host, int n_u,
                        const double *v_edges_host, int n_v, const double *E_edges_host, int n_E_bins, int64_t *counts_out_host,
                        int64_t *maps_out_host) {
    return guarded([&] {
        return plane_flux(ctx, axis, n_levels, levels_host, u_edges_host, n_u, v_edges_host, n_v, E_edges_host, n_E_bins, counts_out_host,
                          maps_out_host);
    });
}

int pcl_group_step_plane_flux(pcl_group *group, int axis, int n_levels, const double *levels_host, const double *u_edges_host, int n_u,
                              const double *v_edges_host, int n_v, const double *E_edges_host, int n_E_bins, int64_t *counts_out_host,
                              int64_t *maps_out_host) {
    return guarded([&] {
        return group_plane_flux(group, axis, n_levels, levels_host, u_edges_host, n_u, v_edges_host, n_v, E_edges_host, n_E_bins,
                                counts_out_host, maps_out_host);
    });
}

} // extern "C"
