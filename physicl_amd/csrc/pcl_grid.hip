// pcl_grid.hip -- binned position grids (PositionGridMeasureStep): where the particles of the store are, as an integer
// histogram over one to three axes (x, y, z, or the distance from a centre), made in one sweep of the resident store.
//
// A translation unit of its own, linked into libphysicl_hip.so behind pcl_spectrum.hip and pcl_source.hip: it does not see
// struct pcl_ctx and works through the public C ABI (include/physicl_hip.h) like any other host of the library.  The tuned
// kernels, their register budgets and the source hash the counter records are tied to (physicl_amd/build.py: csrc_sha) are
// not touched by anything here.  The scaffold it shares with the other units of its kind is pcl_sweep.h.
//
//   k_position_grid<T, lds>   one grid-stride sweep of the tiled slab: per slot the r rows some axis needs (all three for a
//                             radius axis), a binary search per axis in the edges (LDS), then one add to the slot's cell --
//                             lds = true:  into a workgroup-private uint32 histogram in LDS, flushed at the end with 64-bit
//                                          atomics on the non-zero cells (grids of up to PCL_GRID_LDS_CELLS cells);
//                             lds = false: 64-bit atomics straight onto the device grid (up to PCL_GRID_MAX_CELLS cells).
//                             A wave whose in-range lanes all hold the same cell -- the population every bulk run starts
//                             from -- issues ONE add of their count instead of up to 64 adds to one address, and one add
//                             for a whole run of such trips in the same cell.
#include <cstdlib>

#include "pcl_sweep.h"

namespace {

using namespace pcl_sweep;

// The LDS form's switch-over: grids of up to this many cells are accumulated per workgroup in LDS.  4096 cells are 16 KiB;
// with the largest edge table (3 x 1025 doubles, 24 KiB) a workgroup then holds 40 KiB and three of them (12 waves) share
// a CU, a 64 x 64 image with its 130 edges holds 17 KiB and all eight do ("Position grids").  PCL_GRID_LDS_CELLS
// (environment, read per call) moves it, up to kLdsCellsMax: edges + histogram stay below the 64 KiB a launch may ask for.
constexpr int kLdsCellsDefault = 4096;
constexpr int kLdsCellsMax = 8192;

template <typename T>
struct grid_args {
    const T *r[3];               // rows some axis needs (NULL otherwise)
    const double *edges;         // the axes' edges one after another (a radius axis: squared), device
    unsigned long long *grid;    // [n_cells], device, zeroed by the entry point
    int64_t N, ts;               // particles, tile stride of the slab (elements)
    int tile_log;                // log2 of the tile length (pcl_store_layout: 2048 particles)
    int n_axes, n_edges, n_cells;
    int coord[PCL_GRID_MAX_AXES], n_bins[PCL_GRID_MAX_AXES], edge_at[PCL_GRID_MAX_AXES];
    int rows;                    // bit k: row k is read
    double c[3];                 // centre of a radius axis
};

template <typename T, bool kLds>
__global__ void __launch_bounds__(kBlock) k_position_grid(grid_args<T> a) {
    extern __shared__ double s_mem[];                                  // edges | histogram (LDS form)
    double *s_edges = s_mem;
    uint32_t *s_hist = reinterpret_cast<uint32_t *>(s_mem + a.n_edges);
    for (int k = threadIdx.x; k < a.n_edges; k += kBlock) s_edges[k] = a.edges[k];
    if (kLds)
        for (int k = threadIdx.x; k < a.n_cells; k += kBlock) s_hist[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // whole waves run the same number of trips (the ballots below need every lane of the wave inside the loop)
    const int64_t n_round = (a.N + 63) / 64 * 64;
    // wave-uniform: the cell and the count of consecutive trips whose in-range lanes all sat in that one cell, not added yet
    // (fewer than 2^32: kMaxSlotsPerWorkgroup).  Adds to ONE address serialise where they are carried out -- the untouched
    // fill through the global form was 19 ms at 1e8 photons with an add per trip (CHANGELOG.md) --, so a run is added once.
    int run_cell = 0;
    uint32_t run_n = 0;
    auto flush_run = [&]() {
        if (lane == 0 && run_n) {
            if (kLds) atomicAdd(&s_hist[run_cell], run_n);
            else atomicAdd(&a.grid[run_cell], (unsigned long long)run_n);
        }
        run_n = 0;
    };
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_round; i += stride) {
        bool ok = i < a.N;
        const int64_t ti = tile_index(i, a.tile_log, a.ts);
        double x[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (ok && ((a.rows >> k) & 1)) x[k] = (double)a.r[k][ti]; // fp32 widens exactly
        int cell = 0;
        for (int ax = 0; ax < a.n_axes; ++ax) {
            const int co = a.coord[ax], nb = a.n_bins[ax];
            const double *e = s_edges + a.edge_at[ax];
            double v;
            if (co == PCL_GRID_RADIUS) {       // q, unfused, in this order (the library is built with -ffp-contract=off)
                const double dx = x[0] - a.c[0], dy = x[1] - a.c[1], dz = x[2] - a.c[2];
                v = (dx * dx + dy * dy) + dz * dz;
            } else {
                v = co == 0 ? x[0] : (co == 1 ? x[1] : x[2]);
            }
            ok = ok && v >= e[0] && v <= e[nb];  // NaN and anything outside the axis's range are in no cell
            cell = cell * nb + bin_of(e, nb, v); // (numpy.histogramdd)
        }
        const unsigned long long m = __ballot(ok);
        if (m) {
            const int first = __ffsll((long long)m) - 1;
            const int c0 = __shfl(cell, first);
            if (__ballot(ok && cell == c0) == m) { // every in-range lane of the wave in one cell: one add of their count,
                if (c0 != run_cell) {              // put off while the next trips land in the same cell
                    flush_run();
                    run_cell = c0;
                }
                run_n += (uint32_t)__popcll(m);
            } else if (ok) {
                if (kLds) atomicAdd(&s_hist[cell], 1u);
                else atomicAdd(&a.grid[cell], 1ull);
            }
        }
    }
    flush_run();
    if (kLds) {
        __syncthreads();
        flush_cells(s_hist, a.grid, a.n_cells);
    }
}

struct grid_spec { // a call's arguments, checked; what the kernel compares against
    int n_axes = 0, n_edges = 0, rows = 0;
    int64_t cells = 1;
    int coord[PCL_GRID_MAX_AXES], n_bins[PCL_GRID_MAX_AXES], edge_at[PCL_GRID_MAX_AXES];
    double c[3] = {0.0, 0.0, 0.0};
    std::vector<double> edges; // a radius axis: squared
};

// Everything PCL_ERR_ARG stands for except the NULL context; nothing is launched or written before this has passed.
bool check_spec(int n_axes, const int *coords, const int *n_bins, const double *edges, const double *center, int64_t *grid_out,
                grid_spec &s) {
    if (!coords || !n_bins || !edges || !grid_out) return false;
    if (n_axes < 1 || n_axes > PCL_GRID_MAX_AXES) return false;
    int seen = 0;
    for (int a = 0; a < n_axes; ++a) {
        if (coords[a] < PCL_GRID_X || coords[a] > PCL_GRID_RADIUS || ((seen >> coords[a]) & 1)) return false;
        seen |= 1 << coords[a];
        if (n_bins[a] < 1 || n_bins[a] > PCL_GRID_MAX_BINS) return false;
        s.cells *= n_bins[a];
    }
    if (s.cells > PCL_GRID_MAX_CELLS) return false;
    if (center)
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(center[k])) return false;
            s.c[k] = center[k];
        }
    s.n_axes = n_axes;
    for (int a = 0; a < n_axes; ++a) {
        s.coord[a] = coords[a];
        s.n_bins[a] = n_bins[a];
        s.edge_at[a] = s.n_edges;
        s.rows |= coords[a] == PCL_GRID_RADIUS ? 7 : 1 << coords[a];
        // q of a radius axis is compared against e*e: no square root anywhere
        if (!check_edges(edges + s.n_edges, n_bins[a], coords[a] == PCL_GRID_RADIUS ? kEdgeSquare : kEdgePlain, &s.edges)) return false;
        s.n_edges += n_bins[a] + 1;
    }
    return true;
}

int lds_cells_now() { // the switch-over of this call
    const char *t = getenv("PCL_GRID_LDS_CELLS");
    if (!t || !*t) return kLdsCellsDefault;
    char *end = nullptr;
    const long v = strtol(t, &end, 10);
    if (end == t) return kLdsCellsDefault;
    return v < 0 ? 0 : (v > kLdsCellsMax ? kLdsCellsMax : (int)v);
}

template <typename T>
int launch_grid(pcl_ctx *ctx, const store_view &v, const grid_spec &s, const staged &st) {
    grid_args<T> a{};
    for (int k = 0; k < 3; ++k) {
        if (!((s.rows >> k) & 1)) continue;
        void *r = nullptr;
        PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, PCL_R0 + k, &r));
        a.r[k] = static_cast<const T *>(r);
    }
    a.edges = st.tables; a.grid = st.out;
    a.N = v.N; a.ts = v.ts; a.tile_log = v.tile_log;
    a.n_axes = s.n_axes; a.n_edges = s.n_edges; a.n_cells = (int)s.cells; a.rows = s.rows;
    for (int k = 0; k < s.n_axes; ++k) { a.coord[k] = s.coord[k]; a.n_bins[k] = s.n_bins[k]; a.edge_at[k] = s.edge_at[k]; }
    for (int k = 0; k < 3; ++k) a.c[k] = s.c[k];
    const bool lds_form = s.cells <= lds_cells_now();
    const size_t lds = (size_t)s.n_edges * sizeof(double) + (lds_form ? (size_t)s.cells * sizeof(uint32_t) : 0);
    const int64_t grid = balanced_grid(v.N, v.n_cu, resident_per_cu(lds));
    if (lds_form) hipLaunchKernelGGL((k_position_grid<T, true>), dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    else hipLaunchKernelGGL((k_position_grid<T, false>), dim3((unsigned)grid), dim3(kBlock), lds, v.stream, a);
    return hipGetLastError() == hipSuccess ? PCL_OK : PCL_ERR_HIP;
}

int position_grid(pcl_ctx *ctx, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                  const double *center_host, int64_t *grid_out_host) {
    grid_spec s;
    if (!ctx || !check_spec(n_axes, coords_host, n_bins_host, edges_host, center_host, grid_out_host, s)) return bad_argument(ctx);
    const spans out = {{grid_out_host, (size_t)s.cells}};
    store_view v;
    staged st(ctx);
    PCL_SWEEP_TRY(open_store(ctx, PCL_R0 + (s.rows & 1 ? 0 : (s.rows & 2 ? 1 : 2)), &v)); // the first row some axis needs
    if (v.N <= 0) {
        zero_spans(out);
        return PCL_OK;
    }
    PCL_SWEEP_TRY(stage(st, v, (size_t)s.cells, s.edges.data(), (size_t)s.n_edges, false, false)); // positions only: no ids, no kinds
    PCL_SWEEP_TRY(PCL_SWEEP_LAUNCH(v, launch_grid, ctx, v, s, st));
    return fetch(st, out);
}

int group_position_grid(pcl_group *group, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                        const double *center_host, int64_t *grid_out_host) {
    std::vector<pcl_ctx *> ctx;
    PCL_SWEEP_TRY(shards_of(group, ctx));
    const int n = (int)ctx.size();
    grid_spec s;
    if (n < 1 || !check_spec(n_axes, coords_host, n_bins_host, edges_host, center_host, grid_out_host, s))
        return bad_argument(n > 0 ? ctx[0] : nullptr);
    return sum_shards(ctx, {{grid_out_host, (size_t)s.cells}}, [&](pcl_ctx *one, int64_t *p) {
        return pcl_step_position_grid(one, n_axes, coords_host, n_bins_host, edges_host, center_host, p);
    });
}

} // namespace

extern "C" {

int pcl_step_position_grid(pcl_ctx *ctx, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                           const double *center_host, int64_t *grid_out_host) {
    return guarded([&] { return position_grid(ctx, n_axes, coords_host, n_bins_host, edges_host, center_host, grid_out_host); });
}

int pcl_group_step_position_grid(pcl_group *group, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                                 const double *center_host, int64_t *grid_out_host) {
    return guarded([&] { return group_position_grid(group, n_axes, coords_host, n_bins_host, edges_host, center_host, grid_out_host); });
}

} // extern "C"
