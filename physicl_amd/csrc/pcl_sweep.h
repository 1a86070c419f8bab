// pcl_sweep.h -- what the units built on the public C ABI beside the tuned core (pcl_spectrum / pcl_source / pcl_shell /
// pcl_grid / pcl_surface .hip) share: one sweep of the resident store per call, tallied into workgroup-private cells.  Only those units
// include it; it knows nothing of physicl_hip.hip, pcl_device.h or pcl_sincos.h, and they nothing of it (build.py: csrc_sha).
//
// Two layers: plain host arithmetic that any C++ program can include (tests/native/sweep_host.cpp does), and under
// __HIPCC__ the glue around the ABI and the device helpers of the kernels ("Adding a unit on the public ABI").
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pcl_sweep {

constexpr int kBlock = 256;                 // 4 wave64 per workgroup, as the library's sweeps
constexpr int kWorkgroupsPerCU = 8;         // grid cap of a sweep: resident workgroups, each takes the same number of trips
constexpr int kLdsPerCU = 160 * 1024;       // gfx950
// A workgroup-private cell is a uint32: a workgroup adds at most one per slot to a cell, and balanced_grid bounds a
// workgroup to fewer than 2^32 slots, so it cannot overflow.
constexpr int64_t kMaxSlotsPerWorkgroup = ((int64_t)1 << 32) - kBlock;

// Workgroups of lds_bytes each that share a CU, 1 .. kWorkgroupsPerCU: every workgroup flushes its own cells, so a sweep
// launches resident workgroups only.
inline int resident_per_cu(size_t lds_bytes) {
    const size_t per_cu = (size_t)kLdsPerCU / (lds_bytes > 0 ? lds_bytes : 1);
    return per_cu < 1 ? 1 : (per_cu > (size_t)kWorkgroupsPerCU ? kWorkgroupsPerCU : (int)per_cu);
}

// Workgroups for n_slots slots on n_cu CUs (<= 0: 256) with per_cu of them resident on each: all of the blocks if they
// fit, otherwise as few as take the same number of trips (+-1) through the store.
inline int64_t balanced_grid(int64_t n_slots, int n_cu, int per_cu) {
    const int64_t blocks = (n_slots + kBlock - 1) / kBlock;
    int64_t grid = blocks, cap = (int64_t)(n_cu > 0 ? n_cu : 256) * per_cu;
    if (grid > cap) {
        int64_t trips = (blocks + cap - 1) / cap;
        while (trips * kBlock > kMaxSlotsPerWorkgroup) { cap *= 2; trips = (blocks + cap - 1) / cap; } // (never, below 2^43 slots)
        grid = (blocks + trips - 1) / trips;
    }
    return grid;
}

// log2 of the slab's tile length, -1 if that is not a power of two
inline int tile_log_of(int64_t tile) {
    int tile_log = 0;
    while (tile_log < 62 && ((int64_t)1 << tile_log) < tile) ++tile_log;
    return ((int64_t)1 << tile_log) == tile ? tile_log : -1;
}

// What the kernel compares against: the edge itself, e*|e| (a cosine against a signed square), e*e (a radius, not negative)
enum edge_transform { kEdgePlain, kEdgeSignedSquare, kEdgeSquare };

// n_bins + 1 finite, strictly increasing edges, as given and as transformed; the transformed ones are appended to ``to``
inline bool check_edges(const double *e, int n_bins, edge_transform t, std::vector<double> *to = nullptr) {
    double prev = 0.0;
    for (int b = 0; b <= n_bins; ++b) {
        if (!std::isfinite(e[b]) || (b > 0 && !(e[b] > e[b - 1])) || (t == kEdgeSquare && e[b] < 0)) return false;
        const double v = t == kEdgePlain ? e[b] : e[b] * (t == kEdgeSquare ? e[b] : std::fabs(e[b]));
        if (!std::isfinite(v) || (b > 0 && !(v > prev))) return false;
        if (to) to->push_back(v);
        prev = v;
    }
    return true;
}

// A call's one device block: out_bytes of zeroed tallies at 0 | the tables (if any) | the ids (if any; out_bytes and tab_bytes
// are multiples of 8) | the kind bytes (if any).  Where each part starts, and the size of the whole.
struct block_layout { size_t tables, ids, kind, total; };

inline block_layout layout_of(size_t out_bytes, size_t tab_bytes, size_t n_ids, size_t n_kind) {
    block_layout at;
    at.tables = out_bytes;
    at.ids = at.tables + tab_bytes;
    at.kind = at.ids + n_ids * sizeof(int64_t);
    at.total = at.kind + n_kind;
    return at;
}

// A call's outputs: the caller's arrays, in the order of the tallies' cells.  An array nobody asked for is a span of length 0
// and may be NULL: it is never handed to memset / memcpy.
struct span { int64_t *p; size_t n; };
typedef std::vector<span> spans;

inline size_t cells_of(const spans &out) {
    size_t n = 0;
    for (const span &s : out) n += s.n;
    return n;
}

inline void zero_spans(const spans &out) {
    for (const span &s : out)
        if (s.n) memset(s.p, 0, s.n * sizeof(int64_t));
}

// flat[0 .. cells_of(out)) written over the spans / added onto them
inline void copy_to_spans(const spans &out, const int64_t *flat) {
    for (const span &s : out) {
        if (s.n) memcpy(s.p, flat, s.n * sizeof(int64_t));
        flat += s.n;
    }
}

inline void add_to_spans(const spans &out, const int64_t *flat) {
    for (const span &s : out)
        for (size_t k = 0; k < s.n; ++k) s.p[k] += *flat++;
}

} // namespace pcl_sweep

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <new>
#include <system_error>
#include <thread>

#include "../../include/physicl_hip.h"

#define PCL_SWEEP_TRY(expr)              \
    do {                                 \
        int rc__ = (expr);               \
        if (rc__ != PCL_OK) return rc__; \
    } while (0)

namespace pcl_sweep {

// The calling thread's message (pcl_last_error) lives in the core unit and has no setter in the ABI.  A refused call
// leaves the core's own text there -- "bad argument" (pcl_dev_alloc refuses a negative size), "ctx is NULL" without a
// context -- rather than that of some earlier failure; it does not say which argument, and a failed launch of a unit
// leaves whatever was there (include/physicl_hip.h says so).
inline int bad_argument(pcl_ctx *ctx) {
    void *none = nullptr;
    (void)pcl_dev_alloc(ctx, -1, &none);
    return PCL_ERR_ARG;
}

struct dev_block { // one device allocation per call, handed back on every way out
    pcl_ctx *ctx;
    void *p = nullptr;
    explicit dev_block(pcl_ctx *c) : ctx(c) {}
    ~dev_block() { if (p) pcl_dev_free(ctx, p); }
};

struct store_view { // what a sweep needs to know of the store; all but N unset for an empty one
    int64_t N = 0, ts = 0;       // particles, tile stride of the slab (elements)
    int tile_log = 0, dtype = PCL_DTYPE_F64, n_cu = 0;
    hipStream_t stream = nullptr;
};

inline int read_store(pcl_ctx *ctx, store_view *v) {
    PCL_SWEEP_TRY(pcl_store_count(ctx, &v->N));
    if (v->N <= 0) return PCL_OK; // (the caller zeroes its outputs)
    int64_t tile = 0;
    PCL_SWEEP_TRY(pcl_store_dtype(ctx, &v->dtype));
    PCL_SWEEP_TRY(pcl_store_layout(ctx, &tile, &v->ts));
    if ((v->tile_log = tile_log_of(tile)) < 0) return PCL_ERR_STATE; // the slab's tiles are a power of two long
    PCL_SWEEP_TRY(pcl_ctx_device_info(ctx, nullptr, 0, nullptr, &v->n_cu, nullptr));
    void *stream = nullptr;
    PCL_SWEEP_TRY(pcl_ctx_stream(ctx, &stream));
    v->stream = static_cast<hipStream_t>(stream);
    return PCL_OK;
}

// The first look at the store is at a field: a store behind an alive mask becomes dense, an implicit dr real, and there
// is PCL_ERR_STATE without a store before anything else.  *first_out: that field's row, if the caller wants it.
inline int open_store(pcl_ctx *ctx, int first_field, store_view *v, void **first_out = nullptr) {
    void *first = nullptr;
    PCL_SWEEP_TRY(pcl_store_field_ptr(ctx, first_field, first_out ? first_out : &first));
    return read_store(ctx, v);
}

// Plain Objects carry no energy.  *mixed: the store holds some, and ``kind`` then its N kind bytes (the ABI hands them out
// on the host only) for stage() to put behind the ids; empty otherwise.
inline int kind_bytes(pcl_ctx *ctx, int64_t N, std::vector<uint8_t> &kind, bool *mixed) {
    int uniform = 0;
    *mixed = false;
    PCL_SWEEP_TRY(pcl_store_is_uniform(ctx, &uniform));
    if (uniform) return PCL_OK;
    kind.resize((size_t)N);
    PCL_SWEEP_TRY(pcl_store_download_kind(ctx, kind.data(), 0, N));
    *mixed = memchr(kind.data(), PCL_KIND_OBJECT, (size_t)N) != nullptr;
    if (!*mixed) kind.clear();
    return PCL_OK;
}

// Ids for a unit whose draws are keyed by the particle's id.  A uniform store keeps no id array: its one id is answered on
// the host, *id_base = the id of slot 0 and ``ids`` stays empty.  Any other store's N ids are downloaded (the ABI hands them out
// on the host only: 8 B per particle over the host link, every call); if they turn out to be id[0] + index they are dropped
// again, otherwise they stay in ``ids`` for stage() to put behind the tables (another 8 B per particle).
inline int id_words(pcl_ctx *ctx, int64_t N, std::vector<int64_t> &ids, int64_t *id_base) {
    int uniform = 0;
    *id_base = 0;
    ids.clear();
    if (N <= 0) return PCL_OK;
    PCL_SWEEP_TRY(pcl_store_is_uniform(ctx, &uniform));
    if (uniform) return pcl_store_download_ids(ctx, id_base, 0, 1);
    ids.resize((size_t)N);
    PCL_SWEEP_TRY(pcl_store_download_ids(ctx, ids.data(), 0, N));
    *id_base = ids[0];
    for (int64_t i = 0; i < N; ++i)
        if (ids[(size_t)i] != *id_base + i) return PCL_OK;
    ids.clear();
    return PCL_OK;
}

// A call's device block (layout_of) as the kernels see it: typed pointers into it -- ids and kind NULL where the part is not there --,
// the id of slot 0, and the host copies of ids and kinds, which the copies on the stream read until the call's synchronisation.
struct staged {
    dev_block blk;
    unsigned long long *out = nullptr;
    const double *tables = nullptr;
    const int64_t *ids = nullptr;
    const unsigned char *kind = nullptr;
    int64_t id_base = 0;
    size_t out_bytes = 0;
    std::vector<int64_t> ids_host;
    std::vector<uint8_t> kind_host;
    explicit staged(pcl_ctx *c) : blk(c) {}
};

// Fills it on the store's stream: ``cells`` zeroed tallies, the n_tables doubles of ``tables``, and what a store that is not
// uniform makes necessary -- the kinds if it holds a plain Object (want_kinds), the ids if they are not id[0] + index (want_ids:
// a unit that draws).  Both come over the host link and go back up, every call (kind_bytes / id_words say what that costs).
inline int stage(staged &st, const store_view &v, size_t cells, const double *tables, size_t n_tables, bool want_ids,
                 bool want_kinds = true) {
    pcl_ctx *ctx = st.blk.ctx;
    bool mixed = false;
    if (want_kinds) PCL_SWEEP_TRY(kind_bytes(ctx, v.N, st.kind_host, &mixed));
    if (want_ids) PCL_SWEEP_TRY(id_words(ctx, v.N, st.ids_host, &st.id_base));
    const size_t tab_bytes = n_tables * sizeof(double), id_bytes = st.ids_host.size() * sizeof(int64_t);
    st.out_bytes = cells * sizeof(uint64_t);
    const block_layout at = layout_of(st.out_bytes, tab_bytes, st.ids_host.size(), st.kind_host.size());
    PCL_SWEEP_TRY(pcl_dev_alloc(ctx, (int64_t)at.total, &st.blk.p));
    char *base = static_cast<char *>(st.blk.p);
    if (hipMemsetAsync(base, 0, st.out_bytes, v.stream) != hipSuccess) return PCL_ERR_HIP;
    if (tab_bytes && hipMemcpyAsync(base + at.tables, tables, tab_bytes, hipMemcpyHostToDevice, v.stream) != hipSuccess) return PCL_ERR_HIP;
    if (id_bytes && hipMemcpyAsync(base + at.ids, st.ids_host.data(), id_bytes, hipMemcpyHostToDevice, v.stream) != hipSuccess)
        return PCL_ERR_HIP;
    if (mixed && hipMemcpyAsync(base + at.kind, st.kind_host.data(), st.kind_host.size(), hipMemcpyHostToDevice, v.stream) != hipSuccess)
        return PCL_ERR_HIP;
    st.out = reinterpret_cast<unsigned long long *>(base);
    st.tables = reinterpret_cast<const double *>(base + at.tables);
    st.ids = id_bytes ? reinterpret_cast<const int64_t *>(base + at.ids) : nullptr;
    st.kind = mixed ? reinterpret_cast<const unsigned char *>(base + at.kind) : nullptr;
    return PCL_OK;
}

// The call's one synchronisation: the tallies come back onto the caller's arrays (a count is below 2^63)
inline int fetch(const staged &st, const spans &out) {
    if (out.size() == 1) return pcl_d2h(st.blk.ctx, out[0].p, st.out, (int64_t)st.out_bytes);
    std::vector<int64_t> flat(st.out_bytes / sizeof(int64_t));
    PCL_SWEEP_TRY(pcl_d2h(st.blk.ctx, flat.data(), st.out, (int64_t)st.out_bytes));
    copy_to_spans(out, flat.data());
    return PCL_OK;
}

// launch<double> or launch<float>, as the store's elements are
#define PCL_SWEEP_LAUNCH(v, launch, ...) ((v).dtype == PCL_DTYPE_F64 ? launch<double>(__VA_ARGS__) : launch<float>(__VA_ARGS__))

inline int shards_of(pcl_group *group, std::vector<pcl_ctx *> &ctx) {
    int n = 0;
    PCL_SWEEP_TRY(pcl_group_size(group, &n));
    ctx.resize((size_t)n);
    for (int g = 0; g < n; ++g) PCL_SWEEP_TRY(pcl_group_ctx(group, g, &ctx[(size_t)g]));
    return PCL_OK;
}

// fn(g, ctx[g]) for the shards side by side: a thread each per call (the group's own workers cannot be reached through
// the ABI), the calling thread takes shard 0.  A shard whose thread cannot be started is served by the calling thread.
// The first failing shard's code, in shard order.
template <typename F>
int for_each_shard(const std::vector<pcl_ctx *> &ctx, F fn) {
    const int n = (int)ctx.size();
    std::vector<int> rcs((size_t)n, PCL_OK);
    auto one = [&](int g) { rcs[(size_t)g] = fn(g, ctx[(size_t)g]); };
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
    for (int g = 0; g < n; ++g) PCL_SWEEP_TRY(rcs[(size_t)g]);
    return PCL_OK;
}

// The group form of a sweep: fn(ctx, flat) -- the unit's own pcl_step_* entry on one shard, its outputs laid out in ``flat`` in
// the order of the cells -- for the shards side by side.  Only when every shard has succeeded are the caller's arrays zeroed
// and the shards' tallies added up: a failing shard leaves them as they were.
template <typename F>
int sum_shards(const std::vector<pcl_ctx *> &ctx, const spans &out, F fn) {
    std::vector<std::vector<int64_t>> part(ctx.size(), std::vector<int64_t>(cells_of(out), 0));
    PCL_SWEEP_TRY(for_each_shard(ctx, [&](int g, pcl_ctx *one) { return fn(one, part[(size_t)g].data()); }));
    zero_spans(out);
    for (const std::vector<int64_t> &p : part) add_to_spans(out, p.data());
    return PCL_OK;
}

// Nothing may be thrown through the C boundary: host allocations of an entry point's body can fail.
template <typename F>
int guarded(F fn) {
    try {
        return fn();
    } catch (const std::bad_alloc &) {
        return PCL_ERR_NOMEM;
    } catch (...) {
        return PCL_ERR_HIP;
    }
}

// Slot i of the tiled slab: tiles of 1 << tile_log particles, ts elements apart
__device__ __forceinline__ int64_t tile_index(int64_t i, int tile_log, int64_t ts) {
    return (i >> tile_log) * ts + (i & (((int64_t)1 << tile_log) - 1));
}

// The bin of v in scale * e[0 .. nb]: [e_b, e_b+1), the last one closed (numpy.histogram); the caller has checked that v is
// inside.  (scale is a literal 1 or the caller's own multiply per probe: the same instructions as written out in place.)
__device__ __forceinline__ int bin_of(const double *e, int nb, double v, double scale = 1.0) {
    int lo = 0, hi = nb;        // invariant: scale * e[lo] <= v, and v < scale * e[hi] or hi == nb
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] * scale <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// A workgroup's non-zero cells (LDS, after a __syncthreads) onto the device tallies, with 64-bit atomics
__device__ __forceinline__ void flush_cells(const uint32_t *cells, unsigned long long *out, int n) {
    for (int k = threadIdx.x; k < n; k += kBlock)
        if (cells[k]) atomicAdd(&out[k], (unsigned long long)cells[k]);
}

} // namespace pcl_sweep
#endif // __HIPCC__
