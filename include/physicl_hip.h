/*
 * physicl_hip.h -- C ABI of libphysicl_hip.so: the MI355X (gfx950) implementation of PhysiCL's
 * per-particle time-step hot path.
 *
 * This is the drop-in boundary.  The reference crosses it in ONE place: ``CLProgram.run``
 * (physicl/__init__.py:602-664) and the hand-rolled launch in
 * ``ScatterDeleteStepReference.__run_cl`` (physicl/light.py:164-205) gather per-object Python
 * attributes into numpy arrays, copy them to an OpenCL device, launch one kernel and copy the
 * result back.  A PhysiCL maintainer binds the functions below with ctypes instead of PyOpenCL
 * (see INTEGRATION.md).  Two levels are offered:
 *
 *   Level 1  "reference-ABI kernels"  (pcl_k_*): same argument lists as the three OpenCL kernels
 *            the reference builds at run time, on raw device pointers.  One call == one
 *            ``prog.<kernel>(queue, (N,), None, *args)``.
 *   Level 2  "particle store" (pcl_store_*, pcl_step_*): particles stay resident in HBM (one tiled
 *            slab, see pcl_store_alloc) for the whole simulation; a Step, a whole loop body
 *            (pcl_step_fused, pcl_step_fused_delete) or K loop bodies (pcl_step_fused_multi,
 *            pcl_step_fused_delete_multi) are one pass over it; replaces gather + H2D + launch + D2H +
 *            Python write-back.
 *
 * Conventions: plain C types only; every function returns 0 (PCL_OK) or a negative PCL_ERR_* code
 * and never throws; pcl_last_error() gives the calling thread's last message.  Unless a parameter
 * says "host", pointers are DEVICE pointers.  Every entry point binds its context's device to the
 * calling thread first (the reference creates its context on one thread and launches from the
 * Simulation thread, physicl/__init__.py:427-429, 501), so calls may come from any thread; at most
 * one call per context may be in flight at a time.  All work is enqueued on the context's stream;
 * functions that return values to the host synchronise that stream, the others do not.
 */
#ifndef PHYSICL_HIP_H
#define PHYSICL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCL_ABI_VERSION 1

#define PCL_OK          0
#define PCL_ERR_HIP    (-1) /* a HIP runtime call or kernel launch failed */
#define PCL_ERR_ARG    (-2) /* bad argument (null pointer, negative size, unknown enum) */
#define PCL_ERR_STATE  (-3) /* call not valid in the context's current state */
#define PCL_ERR_RTC    (-4) /* hipRTC compile/load failure; log is in pcl_last_error() */
#define PCL_ERR_EXPR   (-5) /* variable_n_fn expression rejected by the validator */
#define PCL_ERR_NOMEM  (-6) /* device or host allocation failed */

/* Per-particle state = the fields of physicl.Object / PhotonObject that a Step reads or writes
 * (physicl/__init__.py:390-394, physicl/light.py:26-35), one row per component, of the store's dtype. */
enum pcl_field {
    PCL_R0 = 0, PCL_R1, PCL_R2,      /* Object.r   position                    */
    PCL_V0, PCL_V1, PCL_V2,          /* Object.v   velocity                    */
    PCL_DR0, PCL_DR1, PCL_DR2,       /* Object.dr  last displacement           */
    PCL_DV0, PCL_DV1, PCL_DV2,       /* Object.dv  last velocity change        */
    PCL_E,                           /* PhotonObject.E                         */
    PCL_NFIELDS
};

/* element type of a particle store.  The reference is fp64-only (every input is marshalled as
 * np.double, physicl/__init__.py:613): PCL_DTYPE_F64 is the parity path; PCL_DTYPE_F32 exists for the
 * precision sweep of BASELINE.json configs[4]. */
#define PCL_DTYPE_F64 0
#define PCL_DTYPE_F32 1

/* pcl_step_scatter_isotropic / pcl_k_light_scatter_step_sphere ``flags`` */
#define PCL_SCATTER_WAVELENGTH 1 /* wavelength_dep_scattering=True  (light.py:275, 300-301) */
#define PCL_SCATTER_VARIABLE_N 2 /* variable_n=True                  (light.py:276, 299)     */
#define PCL_FUSED_LAZY         4 /* pcl_step_fused only: leave dr and dv implicit (see there)  */
#define PCL_SCATTER_PY_DV      8 /* pcl_step_scatter_isotropic only: a hit leaves dv = v_old, the write-back of the
                                    reference's CPU path ScatterIsotropicStep.__run_py (light.py:346-348)       */

/* where a step's three random numbers per photon come from */
#define PCL_RNG_INPUT  0 /* arrays uploaded with pcl_store_upload_rand: the reference's contract
                            ("randoms are kernel inputs", light.py:285, __init__.py:606-619)       */
#define PCL_RNG_PHILOX 1 /* generated in-kernel: Philox4x32-10 keyed by (seed, step, particle id):
                            decision block (id, step >> 1, 0) shared by two steps, direction block
                            (id, step, 1) on a hit (DESIGN.md "Device RNG")                         */

/* kind[] values (pcl_store_upload_kind) */
#define PCL_KIND_OBJECT 0 /* plain physicl.Object: moved by Newton, skipped by the light steps
                             (``if type(obj) != PhotonObject: continue``, light.py:233, 283)      */
#define PCL_KIND_PHOTON 1

/* index layout of pcl_step_counters() output */
#define PCL_CNT_N      0 /* particles in the store                                  */
#define PCL_CNT_XP     1 /* v_x > 0   (ScatterSignMeasureStep, light.py:424)         */
#define PCL_CNT_YP     2
#define PCL_CNT_ZP     3
#define PCL_CNT_PLANE0 4 /* first plane-crossing count (ScatterMeasureStep, light.py:385-399) */
#define PCL_MAX_PLANES 12

typedef struct pcl_ctx pcl_ctx; /* opaque */

/* ---------------------------------------------------------------- library / context ---------- */
int         pcl_abi_version(void);
const char *pcl_last_error(void);                 /* thread-local, never NULL */
int         pcl_device_count(int *n_out);         /* host pointer */
/* A/B switches ("knobs").  Every PCL_* environment variable the library reads at call time (the delete path's: PCL_ALIVE,
 * PCL_ALIVE_RATIO, PCL_ALIVE_MIN_SLOTS, PCL_ALIVE_POLL, PCL_ALIVE_FLUSH_KERNEL, PCL_COMPACT_SPARSE, PCL_AHEAD, PCL_AHEAD_K,
 * PCL_AHEAD_MAX_SLOTS, PCL_AHEAD_K_BIG, PCL_AHEAD_LIVE, PCL_MULTI_AHEAD; the K-step passes': PCL_MULTI_NQ2, PCL_MULTI_NQ3, PCL_MULTI_SAT,
 * PCL_MIXED_NE3, PCL_MIXED_INPLACE, PCL_MIXED_COMPACT_BELOW) can also be set from the program:
 * value = its text, NULL = back to the environment.  Process-wide, takes effect at the next call; results never depend
 * on a knob (that is what the tests that flip them check), only which formulation runs.                            */
int         pcl_set_knob(const char *name, const char *value);
/* Device blocks of >= 64 MB (stores, scratch, pcl_dev_alloc buffers) are not handed back to the driver when freed: the
 * process keeps up to PCL_POOL_GB (environment; default a third of the device's memory, 0 = off; without PCL_POOL_GB a freed
 * block is only kept while at least a quarter of the device stays free) of them for its next store of about that size --
 * a hipMalloc of tens of GB right after a hipFree of that size was measured to stall for seconds on this runtime.
 * pcl_pool_trim() releases everything the pool holds (bytes released in *released_out, may be NULL);
 * pcl_pool_bytes() tells how much it holds.                                                                          */
int         pcl_pool_trim(int64_t *released_out);
int         pcl_pool_bytes(int64_t *idle_out);
/* The same in detail (host pointers, any may be NULL): bytes of idle blocks; bytes of physical handles kept of ranges that were
 * unmapped (both count against PCL_POOL_GB); bytes of ADDRESS SPACE parked behind freed ranges -- on this runtime a new mapping at
 * addresses that were mapped before loses writes, so a freed range's addresses are reserved again at once and never mapped
 * (bounded at 32 TB of the 128 TB address space, then big blocks come from hipMalloc) --; how many times a fresh reservation was
 * found to overlap a formerly mapped range and was set aside; 1 while big blocks are still built with the virtual-memory API. */
int         pcl_pool_info(int64_t *idle_blocks_out, int64_t *idle_handles_out, int64_t *parked_va_out, int64_t *remaps_avoided_out,
                          int *vmm_on_out);

/* ``stream``: a hipStream_t to adopt (e.g. torch.cuda.current_stream().cuda_stream) or NULL to let
 * the context create its own non-blocking stream.  Replaces cl.create_some_context() +
 * cl.CommandQueue() (physicl/__init__.py:428-429). */
int pcl_ctx_create(int device, void *stream, pcl_ctx **ctx_out);
int pcl_ctx_destroy(pcl_ctx *ctx);
int pcl_ctx_sync(pcl_ctx *ctx);
int pcl_ctx_stream(pcl_ctx *ctx, void **stream_out);
/* name: host buffer of name_len bytes.  Replaces Simulation.get_device_info (__init__.py:470-499). */
int pcl_ctx_device_info(pcl_ctx *ctx, char *name, int name_len, int64_t *hbm_bytes, int *n_cu,
                        int *wavefront);
/* Free and total bytes of the context's device as the driver reports them (hipMemGetInfo; blocks idle in the library's
 * pool count as used -- add pcl_pool_bytes() for what the process could still get).  Either pointer may be NULL.        */
int pcl_ctx_mem_info(pcl_ctx *ctx, int64_t *free_out, int64_t *total_out);
/* PCI bus id of the context's device ("0000:05:00.0"; host buffer of >= 16 bytes): lets N ranks show that they
 * drive N different GPUs (bench.py "collective"). */
int pcl_ctx_device_pci(pcl_ctx *ctx, char *pci, int pci_len);
/* variable_n_fn texts of the three built-in shapes (the reference's examples) can start on the
 * ahead-of-time kernels at once while hipRTC compiles their specialisation on another thread (~2 s), which is taken over
 * at the first step call after it is ready -- same bits either way, and about the same speed (the ahead-of-time kernels
 * of the hot passes are compiled per shape and axis).
 * Off by default for a bare context (a measurement must not time the stand-in); physicl_amd.Simulation switches it on.
 * pcl_ctx_rtc_wait blocks until every pending specialisation of the context is in place (*pending_out: how many were).   */
int pcl_ctx_set_rtc_background(pcl_ctx *ctx, int on);
int pcl_ctx_rtc_wait(pcl_ctx *ctx, int *pending_out /* may be NULL */);

/* raw device memory for Level 1 callers: replaces cl_array.to_device / cl_array.empty / .get()
 * (physicl/__init__.py:614, 653, 662).  Copies are ordered on the context stream and return when
 * the host buffer may be reused (pcl_h2d) or holds the data (pcl_d2h). */
int pcl_dev_alloc(pcl_ctx *ctx, int64_t bytes, void **dev_out);
int pcl_dev_free(pcl_ctx *ctx, void *dev);
int pcl_h2d(pcl_ctx *ctx, void *dev, const void *host, int64_t bytes);
int pcl_d2h(pcl_ctx *ctx, void *host, const void *dev, int64_t bytes);
int pcl_dev_memset(pcl_ctx *ctx, void *dev, int value, int64_t bytes);

/* stream timing with HIP events (bench.py): *ms_out = device time between the two records. */
int pcl_timer_start(pcl_ctx *ctx);
int pcl_timer_stop(pcl_ctx *ctx, double *ms_out); /* synchronises */

/* Per-kernel device timing for bench.py: while enabled, every Level-2 step records a HIP event pair
 * on the context stream immediately around its kernel launch (no host synchronisation).
 * pcl_prof_enable(ctx, 1) clears earlier samples; pcl_prof_read synchronises and sums the samples of
 * one kernel.  Host pointers, any may be NULL. */
#define PCL_PROF_NEWTON      0 /* k_newton                         */
#define PCL_PROF_SCATTER     1 /* k_scatter / hipRTC specialisation */
#define PCL_PROF_DELETE_MASK 2 /* k_delete_mask                    */
#define PCL_PROF_COMPACT     3 /* k_compact                        */
#define PCL_PROF_COUNTERS    4 /* k_counters                       */
#define PCL_PROF_FUSED       5 /* k_fused / hipRTC specialisation  */
#define PCL_PROF_MULTI       6 /* k_multi / k_mixed / hipRTC specialisations */
#define PCL_PROF_ONEPASS     7 /* k_delete_onepass                 */
#define PCL_PROF_DELETE_AHEAD 8 /* k_delete_ahead / k_delete_ahead_live: delete loop bodies worked out a launch at a time */
int pcl_prof_enable(pcl_ctx *ctx, int on);
int pcl_prof_read(pcl_ctx *ctx, int kernel_id, int64_t *launches_out, double *total_ms_out,
                  double *min_ms_out, double *max_ms_out);

/* ---------------------------------------------------------------- Level 1: reference-ABI kernels
 * Argument ORDER and meaning follow the OpenCL kernels exactly; N is the global work size.        */

/* kernel light_scatter_step_del(dx, dy, dz, rand, n, A, result)          physicl/light.py:146-158 */
int pcl_k_light_scatter_step_del(pcl_ctx *ctx, const double *dx, const double *dy, const double *dz,
                                 const double *rand, double n, double A, int32_t *result, int64_t N);

/* kernel test(d0, d1, d2, rand, A, n, res) -- ScatterDeleteStep's CLProgram
 * body physicl/light.py:239-249, signature generated by physicl/__init__.py:583-597             */
int pcl_k_scatter_delete_test(pcl_ctx *ctx, const double *d0, const double *d1, const double *d2,
                              const double *rand, double A, double n, int32_t *res, int64_t N);

/* kernel light_scatter_step_sphere(d0,d1,d2, rtheta,rphi,rand, A,n, [E], [r0,r1,r2], res0,res1,res2)
 * physicl/light.py:299-315.  ``E`` is read iff flags & PCL_SCATTER_WAVELENGTH; ``r0..r2`` iff
 * flags & PCL_SCATTER_VARIABLE_N, in which case ``n_expr`` is the OpenCL-C expression the reference
 * splices into the source (light.py:299) and kernel argument ``n`` is unused, as in the reference.
 * ``c`` and ``h`` are the values of the literals str(c), str(h).upper() pasted into the source
 * (light.py:301, 309-311).  Miss: res0[i] = NaN, res1[i]/res2[i] NOT written (light.py:313).      */
int pcl_k_light_scatter_step_sphere(pcl_ctx *ctx, const double *d0, const double *d1, const double *d2,
                                    const double *rtheta, const double *rphi, const double *rand,
                                    double A, double n, const double *E, const double *r0,
                                    const double *r1, const double *r2, double *res0, double *res1,
                                    double *res2, int64_t N, int flags, double c, double h,
                                    const char *n_expr /* host string, may be NULL */);

/* Stable compaction indices of a flag array: idx_out[0..*n_keep) = ascending i with flags[i] == 0
 * -- the survivors of ``for idx, x in enumerate(out["res"]): if x == 1: sim.remove_obj(...)``
 * (physicl/light.py:258-260).  idx_out needs room for N entries; n_keep_out is a host pointer.    */
int pcl_k_compact_indices(pcl_ctx *ctx, const int32_t *flags, int64_t N, int64_t *idx_out,
                          int64_t *n_keep_out);

/* Validate a variable_n_fn expression without compiling it (host strings).  Accepted grammar:
 * numbers, + - * / ( ) , the functions exp sqrt pow log log2 log10 exp2 sin cos tanh fabs fmin fmax,
 * and the array reads r0[gid] r1[gid] r2[gid] d0[gid] d1[gid] d2[gid] E[gid].                     */
int pcl_expr_validate(const char *n_expr);
/* (The hipRTC code objects of an expression are cached in $PCL_RTC_CACHE -- a directory, "off" disables -- default
 * ~/.cache/physicl_amd/rtc, checksummed; a second process loads them instead of compiling.) */

/* User kernels -- the role of CLProgram.build_kernel()/run() (physicl/__init__.py:583-597, 648-656): the
 * caller supplies the parameter list it generated from its CLInput/CLOutput metadata (e.g.
 * "double *d0, double A, int *res") and the kernel BODY in the OpenCL-C dialect the reference's kernels use
 * (get_global_id(0), __global, NAN, pow/sqrt/sin/cos/exp ...).  The body is compiled with hipRTC (unfused
 * arithmetic) into a kernel that runs once per work-item 0..n-1.  argbuf = the arguments packed as a C struct
 * in declaration order (pointers and doubles 8-byte aligned, ints 4).  Unlike variable_n_fn expressions a body
 * is arbitrary code and is NOT validated: like any OpenCL kernel it can read out of bounds. */
int pcl_user_kernel_build(pcl_ctx *ctx, const char *name, const char *params, const char *body, void **kernel_out);
int pcl_user_kernel_launch(pcl_ctx *ctx, void *kernel, int64_t n, const void *argbuf, int64_t argbuf_bytes);
int pcl_user_kernel_free(pcl_ctx *ctx, void *kernel);

/* ---------------------------------------------------------------- Level 2: resident particle store */

/* Allocate storage for up to ``capacity`` particles; count is set to 0.  pcl_store_alloc = fp64.
 * The 13 fields (plus 4 internal rows: the velocity double buffer and the wavelength-term cache) live in ONE
 * allocation, tiled:  element i of a field is at  row0 + (i / T) * tile_stride + (i % T)  elements, T =
 * tile_len = 2048 particles, tile_stride = 17 * T -- so the ~13 streams a step reads are interleaved at 16 KiB
 * (fp64) granularity inside one slab and every HBM channel sees the same mix, wherever the driver placed the
 * slab.  upload/download translate to and from dense host arrays; pcl_store_layout reports T and the stride
 * for callers that read the rows directly.  ids, kinds, the compaction double buffer and the random-input
 * arrays are dense and allocated on first use.  Host buffers passed to upload/download/upload_rand hold
 * elements of the store's dtype (double or float). */
int pcl_store_alloc(pcl_ctx *ctx, int64_t capacity);
int pcl_store_alloc_dtype(pcl_ctx *ctx, int64_t capacity, int dtype);
int pcl_store_dtype(pcl_ctx *ctx, int *dtype_out);
int pcl_store_free(pcl_ctx *ctx);
int pcl_store_capacity(pcl_ctx *ctx, int64_t *capacity_out);
int pcl_store_count(pcl_ctx *ctx, int64_t *count_out);         /* host mirror, no sync */
/* The one-launch-per-body delete path (pcl_step_fused_delete with PCL_FUSED_LAZY, all photons, PCL_RNG_PHILOX) keeps
 * removed photons' slots until fewer than half of the slots are alive: a bit per slot says who is there, a loop body is
 * one kernel that moves nothing, and the stable compaction the reference's removal loop amounts to
 * (physicl/light.py:258-260) is run for several bodies at once.  *slots_out = slots the store currently spans (== the
 * count when it is dense); *pending_moves_out (may be NULL) = Newton moves r has not been given yet.  Every other entry
 * point sees the dense store: it is compacted first, survivors in order, r up to date.                               */
int pcl_store_slots(pcl_ctx *ctx, int64_t *slots_out, int *pending_moves_out);
/* Delete loop bodies ahead of their calls.  When a pcl_step_fused_delete call repeats the previous one with ``step``
 * advanced by one -- a run's loop, physicl/__init__.py:512-516 --, or is the first delete body of a population (taken for
 * the start of such a loop), the library works out that body AND the next ones in one
 * launch that leaves the store untouched (PCL_AHEAD_K = 24 bodies for stores of up to PCL_AHEAD_MAX_SLOTS = 2^22 slots,
 * PCL_AHEAD_K_BIG = 16, 12 beyond 2^25 slots, above: one sweep of the extent serves them all), and answers the following calls, if they are the
 * predicted ones, from those rows without a launch (a loop body of a small store is a 20 us round trip to the host, not
 * bytes; a big store's body is a sweep of its extent).  Any other call first makes the state after the bodies handed out so
 * far real (one kernel; a big store whose alive photons have fallen below the compaction threshold is compacted from those
 * masks), so nothing but timing ever shows; a caller whose loop keeps looking at the store between bodies makes the library
 * pause (exponentially) before it tries again.  Statistics since the context was created (host pointers, any may be NULL):
 * launches of the K-body kernel, bodies answered (the launching one included), launches whose rows were not all used.  */
int pcl_store_ahead_stats(pcl_ctx *ctx, int64_t *launches_out, int64_t *served_out, int64_t *missed_out);
/* What k_delete_ahead_live did in its launches since the context was created, as the kernel itself tallied it (host
 * pointers, any may be NULL): groups of 128 slots loaded (groups without an alive photon are skipped; the photons' first
 * Philox block is decided where they are loaded) whose first pass decided two bodies / one body, rounds of 64 listed
 * photons that decided two bodies, rounds that decided one.  bench.py prices them with the kernel's instruction counts
 * (profiles/isa_counts.json, "k_delete_ahead_live<double>") for the VALU roofline of the delete legs. */
int pcl_store_ahead_work(pcl_ctx *ctx, int64_t *groups_two_out, int64_t *groups_one_out, int64_t *rounds_two_out, int64_t *rounds_one_out);
/* The clock (GHz) the chip held under the k_delete_ahead_live launches of this context (as pcl_store_last_multi_clock,
 * over all of them); 0 before any launch. */
int pcl_store_ahead_clock(pcl_ctx *ctx, double *ghz_out);
/* Allocate now what the first compaction of the store would allocate on demand (the second slab -- chosen among a few
 * candidates like the first, tens of ms for a big store --, the id arrays, the mask scratch), so that a run whose step
 * list holds a delete step pays for it at set-up and not inside its third loop body.  Optional.                        */
int pcl_store_reserve_compaction(pcl_ctx *ctx);

/* Set the particle count (<= capacity) and declare a new population: ids = id_base + index (no id array is read) and
 * every particle a photon (a kind array of an earlier upload is dropped) until pcl_store_upload_ids / _kind. */
int pcl_store_set_count(pcl_ctx *ctx, int64_t count, int64_t id_base);

int pcl_store_upload(pcl_ctx *ctx, int field, const void *host, int64_t offset, int64_t n);
int pcl_store_download(pcl_ctx *ctx, int field, void *host, int64_t offset, int64_t n);
int pcl_store_upload_ids(pcl_ctx *ctx, const int64_t *host, int64_t offset, int64_t n);
int pcl_store_download_ids(pcl_ctx *ctx, int64_t *host, int64_t offset, int64_t n);
int pcl_store_upload_kind(pcl_ctx *ctx, const uint8_t *host, int64_t offset, int64_t n);
int pcl_store_download_kind(pcl_ctx *ctx, uint8_t *host, int64_t offset, int64_t n);
/* device pointer of element 0 of a field's CURRENT row (changes after a compaction and after a lazy fused
 * step); element i is at row0[(i / tile_len) * tile_stride + i % tile_len], see pcl_store_layout */
int pcl_store_field_ptr(pcl_ctx *ctx, int field, void **dev_out);
int pcl_store_layout(pcl_ctx *ctx, int64_t *tile_len_out, int64_t *tile_stride_out);
/* How the store's slab was chosen (stores of >= 512 MB; INTEGRATION.md, "Device memory"): the sweep rates in GB/s of the
 * candidate blocks in the order they were tried (up to ``cap`` <= 8 values), their number (0: no selection took place) and
 * the rate of the block that was kept.  Any pointer may be NULL.                                                        */
int pcl_store_alloc_info(pcl_ctx *ctx, int *n_candidates_out, double *rates_gbps_out, int cap, double *chosen_gbps_out);

/* Random inputs for PCL_RNG_INPUT: which = 0 rtheta, 1 rphi, 2 rand; n values for particles
 * [0, n) in store order (entries of non-photon particles are ignored). */
int pcl_store_upload_rand(pcl_ctx *ctx, int which, const void *host, int64_t n);
/* The three inputs of an isotropic scatter step at once, from the uniforms as the reference draws them: per photon three
 * np.random.random() in the order rtheta, rphi, rand (physicl/__init__.py:606-619), i.e. the (n, 3) row-major array of
 * np.random.random((n, 3)).  u3_host holds the rows of particles [offset, offset + n), n <= 2**20 per call; calls follow
 * one another in particle order starting at offset 0 (the same stream as one big draw).  The scaling of light.py:285,
 * rtheta = (u * 2) * pi and rphi = u * pi, is done on the device with those very operations.  The call returns when the
 * chunk has been staged (two pinned slots): the caller draws the next chunk while this one is copied.               */
int pcl_store_upload_rand3(pcl_ctx *ctx, const double *u3_host, int64_t offset, int64_t n);

/* Bulk creation on the device of ``n`` photons at r = 0 with v = (c, 0, 0), dr = dv = 0 and
 * E = e_min + (e_max - e_min) * U^(1/3) -- the SoA equivalent of light.generate_photons with its
 * default sampler np.random.power(3) (physicl/light.py:112-128).  U is Philox-keyed by
 * (seed, id_base + index).  Sets count = n, ids = id_base + index, every kind = photon. */
int pcl_store_fill_photons(pcl_ctx *ctx, int64_t n, int64_t id_base, double c, double e_min,
                           double e_max, uint64_t seed);

/* The same for a tabulated energy distribution: cdf_host[nbins] (non-decreasing, last = 1) and grid_host[nbins];
 * photon energy = grid[x] for the first x with cdf[x] >= U -- the binned Planck sampler
 * planck_phot_distribution (physicl/light.py:73-104) for all n photons at once (host pointers). */
int pcl_store_fill_photons_table(pcl_ctx *ctx, int64_t n, int64_t id_base, double c, const double *cdf_host,
                                 const double *grid_host, int nbins, uint64_t seed);

/* Photon sources: where the photons of a bulk fill start and where they go.  angular = the distribution of the direction
 * about the axis d, spatial = the distribution of the position in the plane through origin perpendicular to d. */
#define PCL_SRC_BEAM 0        /* angular: v = c * d */
#define PCL_SRC_ISOTROPIC 1   /*          uniform on the sphere */
#define PCL_SRC_CONE 2        /*          uniform in solid angle inside the half angle about d */
#define PCL_SRC_LAMBERTIAN 3  /*          cosine-weighted hemisphere about d (emission from a surface) */
#define PCL_SRC_POINT 0       /* spatial: r = origin */
#define PCL_SRC_DISC 1        /*          uniform over a disc of the given radius */
#define PCL_SRC_GAUSSIAN 2    /*          two-dimensional normal spot, radius = sigma */
typedef struct pcl_source {
    double origin[3];         /* code units */
    double e1[3], e2[3], d[3];/* right-handed orthonormal frame, d = the source's axis; made by the host */
    int angular, spatial;
    double cos_half_angle;    /* PCL_SRC_CONE */
    double radius;            /* PCL_SRC_DISC: radius; PCL_SRC_GAUSSIAN: sigma */
} pcl_source;
/* Gives the population that pcl_store_fill_photons[_table] has just created its positions and velocities.  The store must
 * be uniform (pcl_store_is_uniform: ids = id_base + index, every particle a photon; PCL_ERR_STATE otherwise, also without a
 * store); the rows R0..R2 and V0..V2 of photons [0, count) are overwritten in the store's dtype -- computed in fp64, unfused,
 * rounded once --, E, dr, dv, ids and kinds are not touched, and rows that would not change are not written (point source at
 * the origin: no r rows; beam along +x: nothing at all).  ``c`` = the speed of light in code units, ``seed`` = the fill's.
 * The draws are Philox4x32-10 blocks keyed like the fill's energy draw -- key (seed_lo, seed_hi), counter (id_lo, id_hi,
 * 0xFFFFFFFF, block), u53 = ((w_a >> 5) * 2^26 + (w_b >> 6)) / 2^53 -- so a photon is the same photon however the run is sharded:
 *   block 4, direction: u_a = u53(w0, w1), u_b = u53(w2, w3); mu = cosine of the polar angle about d: beam: no draw;
 *     isotropic mu = 1 - 2*u_a; cone mu = 1 - u_a*(1 - cos_half_angle); lambertian mu = sqrt(1 - u_a);
 *     s = sqrt((1 - mu)*(1 + mu)), psi = (u_b*2)*pi, v_k = c * ((s*cos psi)*e1_k + (s*sin psi)*e2_k + mu*d_k);
 *   block 5, position: u_c = u53(w0, w1), u_d = u53(w2, w3); disc rho = radius*sqrt(u_c); gaussian
 *     rho = radius*sqrt(-2*log(1 - u_c)); phi = (u_d*2)*pi, r_k = origin_k + ((rho*cos phi)*e1_k + (rho*sin phi)*e2_k).
 * PCL_ERR_ARG (NULL, unknown mode, non-finite origin / frame / c, cos_half_angle outside [-1, 1] for a cone, radius negative
 * or not finite for a disc / gaussian) is returned before anything is written; an empty store is PCL_OK.  Asynchronous on the
 * context's stream.  The group form checks every shard first and runs the shards side by side.  pcl_last_error() is generic
 * for these two entry points, as for pcl_step_plane_spectra: they are compiled from a source file of their own
 * (physicl_amd/csrc/pcl_source.hip) on top of the functions above. */
int pcl_store_apply_source(pcl_ctx *ctx, const pcl_source *src, double c, uint64_t seed);

/* NewtonianKinematicsStep.run (physicl/newton.py:10-16): dr = v*dt (rounded, stored); r = r + dr.
 * Applies to every particle of every kind. */
int pcl_step_newton(pcl_ctx *ctx, double dt);

/* ScatterIsotropicStep.__run_cl (physicl/light.py:281-331) fused: hit test, new direction AND the
 * host write-back (hit: v = v', dv = v' - v_old; miss: dv = 0).  ``A``/``n`` are the KERNEL
 * constants, i.e. after the reference's swap (light.py:287); the Python layer applies the swap.
 * hits_out (host, may be NULL): number of photons scattered in this call; when non-NULL the call
 * synchronises. */
int pcl_step_scatter_isotropic(pcl_ctx *ctx, double A, double n, int flags, double c, double h,
                               const char *n_expr, int rng_mode, uint64_t seed, uint32_t step,
                               int64_t *hits_out);

/* The reference's CPU paths of the light steps (``cl_on=False``: ScatterIsotropicStep.__run_py light.py:335-350,
 * ScatterDeleteStepReference.__run_py light.py:216-223) consume np.random in a DATA-DEPENDENT order -- a photon that is
 * hit draws two more numbers, a removal makes the list iteration skip the next object -- so the host has to see every
 * photon's collision probability before it can hand the device its randoms / removal flags.  pcl_step_scatter_pcoll
 * writes pcoll = A * n * |dr| [* pow((h*c)/E, -4)] of every particle (store dtype, constant n only: the CPU path has
 * no variable_n) to a host array; pcl_step_scatter_isotropic(PCL_RNG_INPUT, flags | PCL_SCATTER_PY_DV) then applies
 * the scatter with the host's draws, and pcl_step_delete_flags removes the particles whose flag is 1 (stable). */
int pcl_step_scatter_pcoll(pcl_ctx *ctx, double A, double n, int flags, double c, double h, void *pcoll_out_host);
int pcl_step_delete_flags(pcl_ctx *ctx, const int32_t *flags_host, int64_t *n_alive_out, int64_t *n_removed_out);

/* The whole Simulation loop body in ONE kernel: NewtonianKinematicsStep, then (do_scatter != 0)
 * ScatterIsotropicStep, then (n_planes >= 0) the counters of ScatterSignMeasureStep /
 * ScatterMeasureStep on the post-step state -- the step order every example and test uses
 * (test/test_light.py:32-36, physicl/__init__.py:512-516).  Per-particle arithmetic and order are
 * those of pcl_step_newton + pcl_step_scatter_isotropic + pcl_step_counters, so results are
 * bit-identical to calling the three; r, v, E are read once and dr is consumed from registers.
 * Scatter parameters as pcl_step_scatter_isotropic.  n_planes = -1 switches the counters off.
 * flags | PCL_FUSED_LAZY: dr and dv are NOT written by the step.  Both are pure functions of data the
 * store keeps anyway -- dr = v_before * dt (newton.py:15) and dv = v_after - v_before, which is the
 * reference's v' - v_old on a hit and exactly +0 on a miss (light.py:329-331) -- so the step writes
 * the new velocities into the other half of a v double buffer (whole lines, no read-modify-write)
 * and every later call that touches the store (download, field_ptr, any other step) first runs one
 * materialise pass that produces bit-identical dr/dv arrays.  A chain of lazy steps never pays for
 * the intermediate dr/dv that nothing reads: 104 B per particle-step instead of 128 + 24h.
 * out_host (may be NULL = no synchronisation): int64[5 + n_planes] =
 *   { N, xp, yp, zp, plane counts..., hits }. */
int pcl_step_fused(pcl_ctx *ctx, double dt, int do_scatter, double A, double n, int flags, double c,
                   double h, const char *n_expr, int rng_mode, uint64_t seed, uint32_t step,
                   const double *planes_host, int n_planes, int64_t *out_host);

/* 1 if every particle is a photon and ids are implicit (id_base + index: nothing has been compacted or uploaded
 * with explicit ids/kinds) -- the precondition of pcl_step_fused_multi.  (Any other store takes pcl_step_mixed_multi;
 * the fast single-step kernel has a variant that reads the explicit ids and the kind bytes.) */
int pcl_store_is_uniform(pcl_ctx *ctx, int *uniform_out);

/* k_steps consecutive fused steps (Newton + ScatterIsotropic + sign counters) in ONE pass over the store.  Photons
 * do not interact, so each one is loaded once, advanced k_steps times in registers -- the very operations of
 * k_steps calls of pcl_step_fused(dt, 1, ..., PCL_FUSED_LAZY, PCL_RNG_PHILOX, seed, step0 + k) in the same order --
 * and stored once: results and per-step counters are bit-identical to the step-by-step sequence while the HBM
 * traffic per particle-step falls from 104 B to 128 / k_steps B (fp64).  It is the device side of a run whose
 * passes are [UpdateTimeStep][NewtonStep][ScatterIsotropicStep][counting measures] with nothing on the host
 * looking at the photons in between (physicl/__init__.py:441-448 runs the same steps every pass).
 * Requirements: all-photon store with implicit ids (no compaction yet), device RNG; dr/dv are left implicit
 * exactly as after the last single lazy step.  flags: PCL_SCATTER_WAVELENGTH | PCL_SCATTER_VARIABLE_N.
 * planes_host / n_planes (0..12) as in pcl_step_fused.  out_host (may be NULL): int64[k_steps][5 + n_planes] =
 * { N, xp, yp, zp, plane counts..., hits } per step; 1 <= k_steps <= 64. */
int pcl_step_fused_multi(pcl_ctx *ctx, double dt, int k_steps, double A, double n, int flags, double c, double h,
                         const char *n_expr, uint64_t seed, uint32_t step0, const double *planes_host, int n_planes,
                         int64_t *out_host);
/* The work the last pcl_step_fused_multi launch did, as its kernel tallied it (host pointers, any may be NULL): the
 * K-step pass is bound by VALU issue, not by HBM, and its instruction count per wave is
 *   (instructions of a step's decision part) x wave-steps + (instructions of a dense pass) x dense passes,
 * the two static counts being properties of the code object (profiles/isa_counts.json).  *dense_passes_out = passes of
 * the waves' hit queues (ceil(hits of the wave in that step / 64) summed over waves and steps), *wave_steps_out = waves x
 * K, *photons_per_wave_out = 128 or 256 (fp64; the form the launch took), *saturated_wave_steps_out = wave-steps whose
 * variable_n_fn values came from exp's saturation shortcut instead of its polynomial (-1: the launch ran the variant
 * without the probe; the library picks per launch, PCL_MULTI_SAT = 1 / 0 forces).                                    */
int pcl_store_last_multi_work(pcl_ctx *ctx, int64_t *dense_passes_out, int64_t *wave_steps_out, int *photons_per_wave_out,
                              int64_t *saturated_wave_steps_out);
/* The clock (GHz) the chip held under the last pcl_step_fused_multi launch: shader cycles (s_memtime) over 100 MHz ticks
 * (s_memrealtime) between the start and the end of every workgroup, summed over the launch.  The ceiling of a kernel bound
 * by VALU issue is 1024 SIMDs x THIS clock, in SIMD-cycles per second (bench.py's roofline record); 0 before any launch.
 * No counterpart in the reference (instrumentation of this library).                                                    */
int pcl_store_last_multi_clock(pcl_ctx *ctx, double *ghz_out);
/* Rows of 64 particles a wave kept per trip in the last pcl_step_mixed_multi launch: 2 (pcl_mixed_body, every variable-n
 * form) or 3 (pcl_mixed_body_lds: constant n while a photon's hit probability A n c dt is below 0.33; PCL_MIXED_NE3 = 1 / 0
 * forces); 0 before any.  No counterpart in the reference (instrumentation of this library).                            */
int pcl_store_last_mixed_rows(pcl_ctx *ctx, int *rows_out);
/* Debug builds of the K-step kernels only (environment PCL_RTC_EXTRA=PCL_HIT_HIST, knob PCL_MULTI_HIST=1): the last
 * launch's histogram of hits queued per wave and step (per round in the 256-photon form), bins 0 .. 127 and ">= 128"
 * (host pointer, 129 elements).  tools/hit_hist.py; PCL_ERR_STATE otherwise.                                          */
int pcl_store_last_multi_hist(pcl_ctx *ctx, int64_t *hist129_out);

/* Counters of the OLDEST not-yet-read pcl_step_fused that was called with out_host == NULL and counters on
 * (same layout, same n_planes).  Up to two such steps may be outstanding: enqueue step k+1, then read step k --
 * the call waits for step k only (an event, not the stream), so the GPU runs step k+1 while the host handles
 * step k's counters (exit condition, all-reduce, measure rows). */
int pcl_step_fused_read(pcl_ctx *ctx, int n_planes, int64_t *out_host);

/* Hit count of the most recent pcl_step_scatter_isotropic / pcl_step_fused (host pointer).  Free of extra
 * synchronisation when a pcl_step_counters call has completed since that step. */
int pcl_store_last_scatter_hits(pcl_ctx *ctx, int64_t *hits_out);

/* ScatterDeleteStep.run (physicl/light.py:231-260) fused: flag kernel + stable compaction of every
 * state array.  Non-photon particles are never removed.  Outputs are host pointers (may be NULL);
 * the call synchronises (the new count is needed by exit conditions such as
 * ``len(sim.objects) == 0``, physicl/__init__.py:414). */
int pcl_step_scatter_delete(pcl_ctx *ctx, double A, double n, int rng_mode, uint64_t seed,
                            uint32_t step, int64_t *n_alive_out, int64_t *n_removed_out);
/* The loop body of a delete simulation as one pipeline: NewtonianKinematicsStep, then ScatterDeleteStep,
 * then (n_planes >= 0) the measure counters on the survivors -- the step order of test/test_light.py:52-59.
 * Pass 1 moves the particles and computes the delete flags in one sweep over r and v; pass 3 (the stable
 * compaction) counts while the survivors go through its registers.  Bit-identical to pcl_step_newton +
 * pcl_step_scatter_delete + pcl_step_counters.  flags: 0 or PCL_FUSED_LAZY (dr is neither written nor moved:
 * it stays v*dt until something reads it).  out_host (may be NULL): int64[5 + n_planes] =
 * { N alive, xp, yp, zp, plane counts..., removed }.  Synchronises (the new count is needed on the host). */
int pcl_step_fused_delete(pcl_ctx *ctx, double dt, double A, double n, int flags, int rng_mode, uint64_t seed,
                          uint32_t step, const double *planes_host, int n_planes, int64_t *out_host);

/* k_steps consecutive delete loop bodies (Newton + ScatterDelete + the counters of the measure steps) in one pass
 * and ONE compaction: a photon of a delete run never changes its velocity, so per step only r += v*dt, the
 * decision draw and the compare remain until it is removed.  State and per-step rows are identical to k_steps
 * calls of pcl_step_fused_delete(dt, A, n, PCL_FUSED_LAZY, PCL_RNG_PHILOX, seed, step0 + k, ...); dr is left
 * implicit.  Device RNG only.  out_host (may be NULL): int64[k_steps][5 + n_planes] =
 * { N alive after the step, xp, yp, zp, plane counts..., removed in the step }; n_planes = -1: alive/removed only. */
int pcl_step_fused_delete_multi(pcl_ctx *ctx, double dt, int k_steps, double A, double n, uint64_t seed, uint32_t step0,
                                const double *planes_host, int n_planes, int64_t *out_host);

/* k_passes whole passes of a loop whose body holds one isotropic-scatter phase and/or one delete phase, each phase =
 * NewtonianKinematicsStep + the light step + the counters of the measure steps that follow it:
 *   {ISOTROPIC}          [Newton, ScatterIsotropic]                      on ANY store (explicit ids, plain Objects)
 *   {DELETE}             [Newton, ScatterDelete]
 *   {ISOTROPIC, DELETE}  [Newton, ScatterIsotropic, Newton, ScatterDelete]   (BASELINE.json configs[4]; or the reverse)
 * in ONE pass over the store and, with a delete phase, ONE stable compaction afterwards.  Phase j of pass p uses launch
 * index step0 + p * n_phases + j, so state, survivor order and rows are identical to the same passes run one launch at
 * a time (pcl_step_fused / pcl_step_fused_delete with PCL_FUSED_LAZY, PCL_RNG_PHILOX).  A photon removed by a delete
 * phase takes no further part (physicl/__init__.py:455-459).  dr and dv are left implicit.  A, n, flags, c, h, n_expr:
 * the isotropic phase, as pcl_step_fused_multi; A_del, n_del: the delete phase.  Device RNG only.
 * out_host (may be NULL): int64[k_passes * n_phases][5 + n_planes] = { N alive after the phase, xp, yp, zp, plane
 * counts..., hits (isotropic phase) | removed (delete phase) }; k_passes * n_phases <= 64. */
#define PCL_PHASE_ISOTROPIC 0
#define PCL_PHASE_DELETE    1
int pcl_step_mixed_multi(pcl_ctx *ctx, double dt, int k_passes, int n_phases, const int *phase_kinds_host, double A, double n,
                         int flags, double c, double h, const char *n_expr, double A_del, double n_del, uint64_t seed,
                         uint32_t step0, const double *planes_host, int n_planes, int64_t *out_host);

/* TracePathMeasureStep.run for a tracked subset (physicl/light.py:447-458), worked out AHEAD of the K-pass launch that
 * will move the store: the positions the particles with the ids ``ids_host`` (strictly ascending, n_ids <= PCL_TRACE_MAX)
 * will have when the trace step runs in each of the next k_passes passes of a loop whose body holds the phases
 * ``phase_kinds_host`` -- the same description of the loop, with the same constants, seed and step0, that is about to be
 * handed to pcl_step_fused_multi (n_phases = 1, ISOTROPIC), pcl_step_fused_delete_multi (n_phases = 1, DELETE) or
 * pcl_step_mixed_multi.  ``record_phase``: the trace step sits behind that phase's light step (and its counting measures)
 * in the pass.  A photon's history is a pure function of its own state and of (seed, launch index, id) -- photons do not
 * interact, the device random stream is keyed by the id -- so one thread per TRACKED photon runs the per-photon
 * operations of the K-step kernels on the store as it stands and writes one row per pass; the store is NOT changed, and the
 * K-step kernels (bound by VALU issue) carry nothing for the trace.  Bit-identical to downloading r after every pass.
 * Works on any store (explicit ids after compactions, plain Objects, behind an alive mask, either dtype).
 * out_host: double[k_passes][n_ids][4] = { r0, r1, r2, moved } -- moved = 1 if the particle's dv is not the zero vector
 * at that point (trace_dv, light.py:456) else 0; four NaNs where the particle is not in the store at that point (removed
 * by a delete phase, or never there: the reference traces 'nan;nan;nan', light.py:435).  Device RNG only.  Synchronises --
 * unless out_host is NULL: the kernel is then only enqueued (it writes its rows into pinned host memory of the context) and the
 * K-pass launch can follow at once on the same in-order stream; pcl_store_trace_read(ctx, out_host, k_passes * n_ids * 4) hands
 * the rows out afterwards -- behind a launch that has returned its counter rows it does not wait at all.  The context holds
 * ONE set of rows: a second pcl_store_trace_ahead before the read waits for nothing and replaces them (several tracked sets
 * per launch: pass out_host, as physicl_amd/core.py does for more than one TracePathMeasureStep).                            */
#define PCL_TRACE_MAX 65536
int pcl_store_trace_ahead(pcl_ctx *ctx, const int64_t *ids_host, int n_ids, double dt, int k_passes, int n_phases,
                          const int *phase_kinds_host, int record_phase, double A, double n, int flags, double c, double h,
                          const char *n_expr, double A_del, double n_del, uint64_t seed, uint32_t step0, double *out_host);
int pcl_store_trace_read(pcl_ctx *ctx, double *out_host, int64_t n_doubles);

/* The int32 flag array of the most recent pcl_step_scatter_delete / pcl_step_fused_delete, in PRE-compaction order
 * (what the reference's kernel returns in ``res``).  flags_host needs room for the pre-delete count. */
int pcl_store_last_delete_flags(pcl_ctx *ctx, int32_t *flags_host, int64_t n);

/* ScatterMeasureStep(measure_E=True) (physicl/light.py:383-399): the energies of the photons whose last move
 * crossed the plane (one 3-vector, NaN in the coordinates that do not define it), in particle order.  *n_out =
 * number of crossing photons; the first min(n, cap) energies (store dtype) are copied to E_out_host (host pointers). */
int pcl_step_plane_energies(pcl_ctx *ctx, const double *plane_host, void *E_out_host, int64_t cap, int64_t *n_out);

/* ScatterSignMeasureStep.run + the counting part of ScatterMeasureStep.run
 * (physicl/light.py:414-431, 374-400).  planes_host: n_planes x 3 doubles, NaN = coordinate not
 * defining the plane.  out_host: int64[PCL_CNT_PLANE0 + n_planes].  Synchronises. */
int pcl_step_counters(pcl_ctx *ctx, const double *planes_host, int n_planes, int64_t *out_host);

/* ScatterMeasureStep(measure_E=True) with bin edges: what the reference's scripts do with the energy lists of
 * pcl_step_plane_energies is a histogram (examples/planck_distribution.ipynb: plt.hist(sim.steps[4].data[49][3], 50)), so
 * this returns the histogram -- per plane the count of crossing photons per energy bin, for ALL planes of the call in one
 * sweep of the store, as int64 rows that add across devices and ranks like every other counter.  planes_host: n_planes x 3
 * doubles, NaN = coordinate not defining the plane (1 <= n_planes <= PCL_MAX_PLANES, each with a defining coordinate);
 * edges_host: n_bins + 1 finite, strictly increasing doubles (1 <= n_bins <= PCL_SPECTRUM_MAX_BINS) in the unit E is
 * stored in.  counts_out_host[p] = the plane counter of pcl_step_counters (every particle of the store);
 * hist_out_host[p * n_bins + b] = crossing photons (plain Objects carry no energy) whose E lies in bin b as
 * numpy.histogram(E, bins=edges) counts it: [e_b, e_b+1), the last bin closed, E outside [e_0, e_nbins] or NaN in no bin
 * -- an fp32 store's E is widened to double (exact) for the comparison.  Crossing predicate and the store as
 * pcl_step_plane_energies sees it (dense, dr real).  Host pointers; synchronises once.  An empty store answers zeros without
 * a launch.  PCL_ERR_ARG / PCL_ERR_STATE (no store) are returned before anything is launched.
 * pcl_last_error() is GENERIC for these two entry points: the thread's text belongs to the core source file and has no setter,
 * so a refused argument leaves the core's "bad argument" (not which edge or plane; "ctx is NULL" after a NULL context), a
 * failed launch of this unit leaves the text of the last call that set one, and a shard's text in the group form stays on that
 * shard's thread.  Go by the code.  The same holds for every entry point compiled from a unit of its own on top of the
 * functions above (pcl_store_apply_source, pcl_step_position_grid, pcl_step_shell_crossings and their group forms): they
 * share that behaviour through physicl_amd/csrc/pcl_sweep.h.
 * Compiled from a source file of its own (physicl_amd/csrc/pcl_spectrum.hip) on top of the functions above; it reads E through
 * pcl_store_field_ptr, so a wavelength-dependent scatter step that follows rebuilds its wavelength-term cache. */
#define PCL_SPECTRUM_MAX_BINS 1024
int pcl_step_plane_spectra(pcl_ctx *ctx, const double *planes_host, int n_planes, const double *edges_host, int n_bins,
                           int64_t *counts_out_host, int64_t *hist_out_host);

/* Where the particles are: an integer histogram of the store's positions over one to three axes, made in one sweep of the
 * resident store -- an altitude profile (one PCL_GRID_RADIUS axis about the planet's centre), an image (two Cartesian axes), a
 * coarse volume density (three) -- as int64 cells that add across devices and ranks like every other counter row.  The other
 * way to it is a download of r (24 B per particle over the host link) and numpy.histogramdd.
 * coords_host[a]: the coordinate axis a bins (each at most once); n_bins_host[a]: its bins, 1..PCL_GRID_MAX_BINS, the product
 * at most PCL_GRID_MAX_CELLS; edges_host: the axes' n_bins[a] + 1 edges one after another, finite and strictly increasing, in
 * code units; center_host: 3 finite doubles, NULL = the origin.  grid_out_host: prod(n_bins) cells in C order, first axis slowest.
 * EVERY particle of the store counts, plain Objects included (as N and the plane counters; no kind bytes are read).
 * A Cartesian axis: the particle is in bin b iff e_b <= x < e_(b+1), the last bin closed -- exactly
 * numpy.histogramdd(sample, bins=[edges...]); only comparisons are made, an fp32 store's value is widened to double first
 * (exact).  A particle with any coordinate outside its axis's range, or NaN, is in no cell.
 * PCL_GRID_RADIUS bins q = ((x-cx)*(x-cx) + (y-cy)*(y-cy)) + (z-cz)*(z-cz), evaluated in fp64, unfused, in that order, against
 * the SQUARED edges e*e, which the entry point makes on the host: there is no square root anywhere, so numpy restates the
 * result exactly -- and it is NOT histogram(sqrt(q)) for a particle within an ulp of an edge.  Radius edges must be >= 0,
 * their squares finite and strictly increasing.
 * PCL_ERR_ARG (a NULL pointer, n_axes outside 1..3, an unknown or repeated coordinate, a bin count outside 1..1024, too many
 * cells, edges not finite or not strictly increasing, a non-finite centre) is returned before anything is launched or written;
 * PCL_ERR_STATE without a store; an empty store answers zeros without a launch.  Host pointers; synchronises once, with the
 * one copy of the grid.  The store is seen dense with r current (pcl_store_field_ptr(PCL_R0..R2): nothing is invalidated).
 * Grids of up to 4096 cells are accumulated per workgroup in LDS, larger ones with 64-bit atomics on the device grid; the
 * environment variable PCL_GRID_LDS_CELLS (read per call, 0..8192) moves that switch-over -- same cells either way.
 * pcl_last_error() is generic for these two entry points, as for pcl_step_plane_spectra: they are compiled from a source file
 * of their own (physicl_amd/csrc/pcl_grid.hip) on top of the functions above. */
#define PCL_GRID_X 0
#define PCL_GRID_Y 1
#define PCL_GRID_Z 2
#define PCL_GRID_RADIUS 3          /* distance from center_host */
#define PCL_GRID_MAX_AXES 3
#define PCL_GRID_MAX_BINS 1024     /* per axis */
#define PCL_GRID_MAX_CELLS (1 << 20)
int pcl_step_position_grid(pcl_ctx *ctx, int n_axes, const int *coords_host, const int *n_bins_host,
                           const double *edges_host,   /* the axes' edges one after another: sum(n_bins[a] + 1) */
                           const double *center_host,  /* 3 doubles, NULL = origin; used by PCL_GRID_RADIUS only */
                           int64_t *grid_out_host);    /* prod(n_bins) cells, C order, first axis slowest */

/* What passed through a sphere in the last move: the crossing measure of a radial problem (pcl_step_counters and
 * pcl_step_plane_spectra know axis-aligned planes only).  For up to PCL_SHELL_MAX_SHELLS spheres of radii radii_host[s] > 0
 * (finite, R*R finite, any order) about center_host (3 finite doubles, NULL = the origin), in ONE read-only sweep of the
 * resident store: per shell the particles that went out and the ones that came in, and -- when asked for -- histograms of
 * the crossing photons' energies and of the direction cosine of the move against the outward normal, as int64 cells that
 * add across devices and ranks like every other counter row.  The other way to it is a download of r and dr (48 B per
 * particle over the host link) and numpy, every pass.
 * All arithmetic is fp64, unfused, in the order written; an fp32 store's values are widened first (exact).  Per particle,
 * plain Objects included:  d = (x-cx, y-cy, z-cz);  p = d - dr, component by component (the position before the last move);
 * q_now = (d0*d0 + d1*d1) + d2*d2, q_prev the same over p;  R2 = R*R, made once per shell on the host.
 *   outward crossing of shell s  iff  q_prev <  R2_s and q_now >= R2_s
 *   inward  crossing             iff  q_prev >= R2_s and q_now <  R2_s
 * Half-open: a particle exactly on the sphere belongs to the outside, and every transition between q < R2 and q >= R2 is
 * counted exactly once -- unlike the plane rule, which counts a stop exactly on a plane twice.  End points are tested, as
 * the plane measure tests them: a chord that enters and leaves the sphere within one move is not counted.  NaN anywhere: no
 * crossing.
 * counts_out_host[dir * n_shells + s] (dir 0 = outward, 1 = inward): all particles.
 * E_hist_out_host[(dir * n_shells + s) * n_E_bins + b]: crossing PHOTONS (plain Objects carry no energy) whose E lies in bin
 * b as numpy.histogram(E, bins=E_edges) counts it: [e_b, e_b+1), the last bin closed, E outside the edges or NaN in no bin --
 * what pcl_step_plane_spectra does.
 * mu_hist_out_host[(dir * n_shells + s) * n_mu_bins + b]: all crossing particles by mu, the cosine between dr and the outward
 * normal at the new position, binned without a square root or a division so that numpy restates it bit for bit:
 *   s = (d0*dr0 + d1*dr1) + d2*dr2;  dd = (dr0*dr0 + dr1*dr1) + dr2*dr2;  W = s*|s|;  D = q_now*dd;  w_b = e_b*|e_b| (host);
 *   bin b  iff  w_b*D <= W < w_(b+1)*D, the last bin closed (W <= w_B*D): mu = s / sqrt(D), both sides signed-squared.
 * Rounded products are monotone in b: a binary search with one multiply per probe.  D == 0 (no move, or on the centre), or
 * D or W not finite: counted as a crossing, in no mu bin.
 * E_edges_host / mu_edges_host: n + 1 finite, strictly increasing doubles (1 <= n <= PCL_SHELL_MAX_BINS; the w_b finite and
 * strictly increasing too), or 0 bins (the pointers are not looked at): no such histogram.  2 * n_shells * (n_E_bins +
 * n_mu_bins) may not exceed PCL_SHELL_MAX_CELLS: a workgroup's uint32 histograms (32 KiB) and both edge tables stay below
 * the 64 KiB of LDS a launch may ask for.
 * PCL_ERR_ARG is returned before anything is launched or written; PCL_ERR_STATE without a store; an empty store answers zeros
 * without a launch.  Host pointers; one device allocation per call, handed back on every way out; synchronises once, with
 * the one copy of the results.  The store is seen dense with dr real (pcl_store_field_ptr); E is looked at only with energy
 * bins (a wavelength-dependent scatter step that follows then rebuilds its wavelength-term cache, as after
 * pcl_step_plane_spectra).  pcl_last_error() is generic for these two entry points, as for pcl_step_plane_spectra: they are
 * compiled from a source file of their own (physicl_amd/csrc/pcl_shell.hip) on top of the functions above. */
#define PCL_SHELL_MAX_SHELLS 16
#define PCL_SHELL_MAX_BINS 1024    /* per histogram */
#define PCL_SHELL_MAX_CELLS 8192   /* 2 * n_shells * (n_E_bins + n_mu_bins) */
int pcl_step_shell_crossings(pcl_ctx *ctx, int n_shells, const double *radii_host, const double *center_host,
                             const double *E_edges_host, int n_E_bins,      /* NULL, 0: no energy histograms */
                             const double *mu_edges_host, int n_mu_bins,    /* NULL, 0: no direction histograms */
                             int64_t *counts_out_host,                      /* [2][n_shells]: outward, inward */
                             int64_t *E_hist_out_host, int64_t *mu_hist_out_host);   /* may be NULL with 0 bins */

/* What a radiometer sees: a pinhole camera's image of the last move (DetectorMeasureStep).  The instrument is a disc of
 * ``radius`` > 0 (finite, R2 = radius*radius finite, made on the host) about position_host (3 finite doubles) in the plane whose
 * normal n points from the detector into the scene; frame_host holds the orthonormal frame e1, e2, n as nine finite doubles
 * (e1 | e2 | n; the caller makes it, nothing is normalised here, n may not be zero).  In ONE read-only sweep of the resident
 * store the particles that went through the disc from the front in their last move are counted, sorted by the direction they
 * came from into nx x ny pixels and -- with bands -- by energy, as int64 cells that add across devices and ranks like every
 * other counter row.  The other way to it is a download of r and dr (48 B per particle over the host link) and numpy, every pass.
 * All arithmetic is fp64, unfused, in the order written; an fp32 store's values are widened first (exact).  There is no division,
 * no square root and no transcendental function, so numpy restates every cell exactly.  Per slot, plain Objects included, m = dr:
 *   a_k = r_k - p_k;  b_k = a_k - m_k (where the move began);
 *   s_now = (a0*n0 + a1*n1) + a2*n2;  s_prev the same over b;
 *   crossed  iff  s_prev > 0 and s_now <= 0      -- front to back; a particle that ends exactly on the plane has arrived, one
 *                                                   that starts on it has not; NaN: neither.  As for the shells, only the end
 *                                                   points of the move are looked at.
 *   D = s_prev - s_now;  H_k = b_k*D + m_k*s_prev (the hit point times D);  hh = (H0*H0 + H1*H1) + H2*H2;  lim = R2*(D*D);
 *   through  iff  crossed and hh <= lim and lim < inf                        -- the rim is inside.
 *   wn = -((m0*n0 + m1*n1) + m2*n2);  ax = -((m0*e1_0 + m1*e1_1) + m2*e1_2);  ay the same with e2
 *                                                -- the direction the photon came from, in gnomonic coordinates ax/wn, ay/wn;
 *   seen  iff  through and wn > 0 and wn < inf and x_0*wn <= ax <= x_nx*wn and y_0*wn <= ay <= y_ny*wn.
 *   column c  iff  x_c*wn <= ax < x_(c+1)*wn, the last one closed; the row the same from the y edges.  Rounded products are
 *   monotone in the edge because wn > 0: a binary search with one multiply per probe.
 * Without bands (n_E_bins == 0, E_edges_host is not looked at) every seen particle adds 1 to image[0][row][col].  With bands only
 * a PHOTON (plain Objects carry no energy) with E_0 <= E <= E_nE adds, to image[band][row][col], the band as
 * numpy.histogram(E, bins=E_edges) finds it; a plain Object, an energy outside the bands or NaN is seen and lands in no cell.
 * counts_out_host = [through, seen]; image_out_host: max(n_E_bins, 1) * ny * nx cells, C order, the band slowest:
 * sum(image) <= seen <= through.
 * x_edges_host / y_edges_host / E_edges_host: n + 1 finite, strictly increasing doubles; nx, ny in 1..PCL_DETECTOR_MAX_PIXELS,
 * n_E_bins in 0..PCL_DETECTOR_MAX_BANDS, max(n_E_bins, 1) * ny * nx at most PCL_DETECTOR_MAX_CELLS.  Only the three edge tables
 * sit in LDS (at most 3 x 1025 doubles); the seen particles add to their cells with 64-bit atomics on the device -- an aperture is
 * small, so they are few.
 * PCL_ERR_ARG (a NULL pointer, a position, frame or radius that is not finite, a zero n, radius <= 0 or its square not finite,
 * edges not finite or not strictly increasing, a pixel, band or cell count outside its limits) is returned before the store is
 * looked at and before anything is written; PCL_ERR_STATE without a store; an empty store answers zeros without a launch.  Host
 * pointers; one device allocation per call, handed back on every way out; synchronises once, with the one copy of the results.
 * The store is seen dense with dr real (pcl_store_field_ptr); E is looked at only with bands: a wavelength-dependent scatter
 * step that follows then rebuilds its wavelength-term cache -- one more sweep of E per pass, as after pcl_step_plane_spectra --,
 * and a camera without bands costs that step nothing.  pcl_last_error() is generic for these two entry points, as for
 * pcl_step_plane_spectra: they are compiled from physicl_amd/csrc/pcl_shell.hip on top of the functions above. */
#define PCL_DETECTOR_MAX_PIXELS 1024      /* per image axis */
#define PCL_DETECTOR_MAX_BANDS 1024
#define PCL_DETECTOR_MAX_CELLS (1 << 20)  /* max(n_E_bins, 1) * ny * nx */
int pcl_step_detector_image(pcl_ctx *ctx, const double *position_host,      /* 3 doubles: the aperture's centre */
                            const double *frame_host,                       /* 9 doubles: e1 | e2 | n */
                            double radius, const double *x_edges_host, int nx, const double *y_edges_host, int ny,
                            const double *E_edges_host, int n_E_bins,       /* NULL, 0: no bands */
                            int64_t *counts_out_host,                       /* [2]: through, seen */
                            int64_t *image_out_host);                       /* [max(n_E_bins, 1)][ny][nx] */

/* A reflecting sphere: the ground of a radial problem (SurfaceReflectStep).  Photons whose last move took them into the sphere
 * of ``radius`` > 0 (finite, R2 = radius*radius finite, made on the host) about center_host (3 finite doubles, NULL = the
 * origin) are put back in ONE sweep of the resident store: reflected where the move met the sphere, or -- with albedo < 1 --
 * absorbed there and left in the store at rest.  Nothing is removed, the count does not change, E, ids and kinds are not touched
 * and E is not even asked for (a wavelength-dependent scatter step keeps its term cache).  Meant to be the last call of a pass.
 * All arithmetic is fp64, every operation rounded once, in the order written (x.y of two vectors is (x0*y0 + x1*y1) + x2*y2
 * everywhere); an fp32 store's values are widened first (exact) and what is written is rounded once to the store's dtype.
 *   d = r - center;  m = dr;  p = d - m (the position before the last move);  q_now = d.d;  q_prev = p.p
 *   hit  iff  q_now < R2 and R2 <= q_prev and q_prev < inf, and the particle is a photon
 * -- the inward crossing of pcl_step_shell_crossings for one shell, so that tally (made BEFORE this call) counts exactly the
 * photons hit, except for a move whose q_prev is not finite (it has no hit point: counted there, left alone here).  NaN
 * anywhere: not hit.  Plain Objects (kind 0) are never hit.  A particle that is not hit is not written at all.
 *   a = m.m;  b = p.m;  cq = q_prev - R2;  disc = max(b*b - a*cq, 0);  t = cq / (sqrt(disc) - b)        (0 <= t <= 1; b < 0 on a hit)
 *   x = p + t*m (the hit point, about the centre);  nrm = x / sqrt(x.x) (the outward normal);  sa = sqrt(a);  w = (1 - t)*sa
 * Outcome: reflected iff albedo == 1 or u_0 < albedo (albedo 0: every hit is absorbed, no matter what is drawn).
 *   absorbed:    r = center + x;  v = 0;  dr = x - p;  dv = 0 - v_old
 *   PCL_SURFACE_SPECULAR:    mh = m / sa;  dn = mh.nrm;  dir = mh - (2*dn)*nrm                               (no draw)
 *   PCL_SURFACE_LAMBERTIAN:  mu = sqrt(1 - u_a);  s = sqrt((1 - mu)*(1 + mu));  psi = (u_b*2)*pi;  sc = s*cos psi;  ss = s*sin psi;
 *     the frame of Duff et al. (2017), branch-free:  sg = copysign(1, nrm2);  aa = -1/(sg + nrm2);  bb = (nrm0*nrm1)*aa;
 *     sn0 = sg*nrm0;  e1 = (1 + (sn0*nrm0)*aa, sg*bb, -sn0);  e2 = (bb, sg + (nrm1*nrm1)*aa, -nrm1);
 *     dir = (sc*e1 + ss*e2) + mu*nrm   -- cosine-weighted about nrm, mu > 0 always; sin / cos are the scatter step's own
 *   reflected:   v = c*dir;  dv = v - v_old;  dr = w*dir;  r = center + (x + dr)    (the rest of the move, flown along dir)
 * ``c`` = the speed of light in code units (what the scatter step is handed).  The draws are Philox4x32-10 blocks with the key
 * (seed_lo, seed_hi) and u53 of pcl_store_apply_source: counter (id_lo, id_hi, pass, 8): u_a = u53(w0, w1), u_b = u53(w2, w3);
 * counter (id_lo, id_hi, pass, 9): u_0 = u53(w0, w1), drawn only with albedo < 1.  ``pass`` is the caller's own counter, here and in
 * every entry point below that takes one: calls that share a counter word within one pass of the caller's loop (two calls of one
 * entry point -- two gases, two clouds --, or of two that share words: the two grounds, the two phase functions) must be given
 * distinct ``pass`` values, or a photon draws the same number in both (physicl_amd.tally.WriterStep interleaves them).  The
 * scatter kernels use the counter words (step >> 1, 0) and (step, 1), fill and source (0xFFFFFFFF, 2..5): no block is shared,
 * and a photon draws the same numbers however the run is sharded.
 * counts_out_host[0] = photons reflected, [1] = absorbed, by this call.
 * A uniform store (pcl_store_is_uniform) runs from the device alone.  Any other store costs host traffic, every call: its ids
 * are downloaded (8 B per particle) and, unless they turn out to be id[0] + index, uploaded again behind the counters (8 B);
 * its kinds are downloaded (1 B) and uploaded (1 B) if a plain Object is among them.
 * PCL_ERR_ARG (NULL counts, unknown mode, radius not positive / not finite / its square not finite, centre or c not finite,
 * albedo outside [0, 1]) is returned before anything is launched or written; PCL_ERR_STATE without a store; an empty store
 * answers zeros without a launch.  Host pointers; one device allocation per call, handed back on every way out; synchronises
 * once, with the copy of the two counts.  pcl_last_error() is generic for these two entry points, as for
 * pcl_step_plane_spectra: they are compiled from a source file of their own (physicl_amd/csrc/pcl_surface.hip). */
#define PCL_SURFACE_LAMBERTIAN 0
#define PCL_SURFACE_SPECULAR 1
int pcl_step_surface_reflect(pcl_ctx *ctx, double radius, const double *center_host, double albedo, int mode, double c,
                             uint64_t seed, uint32_t pass, int64_t *counts_out_host /* [2]: reflected, absorbed */);

/* A phase function for the scatter step (PhaseFunctionStep).  Called directly behind the scatter step of a pass, it REPLACES the
 * direction that step gave a scattered photon by one drawn from a phase function about the photon's direction BEFORE the
 * scatter, in ONE sweep of the resident store.  pcl_step_scatter_isotropic keeps deciding who scatters; its own new direction
 * (polar angle uniform about the x axis: not isotropic, and independent of where the photon came from) is overwritten.
 * "Scattered in this pass" is read off the store: the scatter step leaves dv = v' - v_old on a hit and dv = 0 on a miss (not with
 * PCL_SCATTER_PY_DV, where a hit leaves dv = v_old: do not call this behind such a step).  Nothing is removed; r, dr, E, ids and
 * kinds are not touched and E is not even asked for.  All arithmetic is fp64, every operation rounded once, in the order written
 * (x.y is (x0*y0 + x1*y1) + x2*y2); an fp32 store's values are widened first and what is written is rounded once to its dtype.
 *   scattered  iff  the particle is a photon and (dv0 != 0 or dv1 != 0 or dv2 != 0)                     (NaN != 0 is true)
 *   o = v - dv (the velocity before the scatter);  oo = o.o;  re-directed iff scattered and 0 < oo < inf  (else: not written,
 *   not counted);  on = sqrt(oo);  w = o / on
 *   block A: u_a = u53(w0, w1), u_b = u53(w2, w3);  mu, the cosine of the scattering angle:
 *   PCL_PHASE_ISOTROPIC:  mu = 1 - 2*u_a                        (uniform on the sphere: the law of PCL_SRC_ISOTROPIC)
 *   PCL_PHASE_HG:         Henyey-Greenstein, |g| < 1 its mean cosine;  g == 0: the isotropic line, bit for bit;  otherwise
 *                         |g| >= 1/2, the closed inverse of the cumulative distribution:
 *                           q = (1 - g*g) / ((1 - g) + (2*g)*u_a);  m = ((1 + g*g) - q*q) / (2*g)
 *                         |g| < 1/2, the same inverse as a polynomial in g (the closed form subtracts two numbers near 1 and
 *                         divides by 2g: it loses ulp(1)/|g|, and below |g| = 1e-16 every digit):
 *                           s = 1 - 2*u_a;  gs = g*s;  d = 1 - gs;  s2 = s*s
 *                           p = (0.5*(s2 + 3) - gs) + (g*g)*(0.5*(s2 - 1));  m = (g*p - s) / (d*d)
 *                         mu = min(max(m, -1), 1).  Against exact arithmetic mu is good to 8 ulp(1) for |g| < 1/2, down to the
 *                         smallest g, and to 32 ulp(1)/(1 - |g|) above (q's denominator).  As g -> 0 the law tends to
 *                         mu = -(1 - 2*u_a), while g == 0 gives +(1 - 2*u_a): both are uniform on the sphere.
 *   PCL_PHASE_RAYLEIGH:   3/8 (1 + mu*mu) as the mixture of 3/4 uniform and 1/4 of the density 3/2 mu*mu:
 *                         s4 = u_a*4;  j = floor(s4);  f = s4 - j (both exact);  gq = 2*f - 1;   j < 3: mu = gq;
 *                         j == 3: block B: u_c = u53(w0, w1), u_d = u53(w2, w3);  mu = copysign(max(max(|gq|, u_c), u_d), gq)
 *                         (the largest of three uniforms has the density 3 x*x; the sign of gq is independent of its size)
 *   s = sqrt((1 - mu)*(1 + mu));  psi = (u_b*2)*pi;  sc = s*cos psi;  ss = s*sin psi;  the frame e1, e2 about w exactly as
 *   pcl_step_surface_reflect builds it about nrm;  dir = (sc*e1 + ss*e2) + mu*w;  v = c*dir;  dv = v - o
 * Add, subtract, multiply, divide, square root, min / max, copysign and floor only: everything but sin / cos (the scatter step's
 * own) can be restated bit for bit.  Philox4x32-10 blocks, key (seed_lo, seed_hi), u53 of pcl_store_apply_source: block A has the
 * counter (id_lo, id_hi, pass, 10), block B (id_lo, id_hi, pass, 11), drawn only by the lanes that need it; ``pass`` is the
 * caller's own counter.  The words 10 and 11 are used by nothing else (pcl_step_surface_reflect: 8 and 9), so every other step
 * draws what it drew, and a photon draws the same numbers however the run is sharded.  ``c`` = the speed of light in code units.
 * count_out_host[0] = photons re-directed by this call.  A store that is not uniform costs the host traffic it costs
 * pcl_step_surface_reflect.  PCL_ERR_ARG (NULL count, unknown phase, g not finite or |g| >= 1 with PCL_PHASE_HG -- g is ignored
 * otherwise --, c not finite) is returned before anything is launched or written; PCL_ERR_STATE without a store; an empty store
 * answers zero without a launch.  Host pointer; one device allocation per call, handed back on every way out; synchronises once,
 * with the copy of the count.  pcl_last_error() is generic, as for pcl_step_surface_reflect, whose source file these two entry
 * points share (physicl_amd/csrc/pcl_surface.hip).  PCL_PHASE_ISOTROPIC (0) is the define above pcl_step_mixed_multi: a loop's
 * phase kind and a phase function share that name and value, and nothing else. */
#define PCL_PHASE_HG 1
#define PCL_PHASE_RAYLEIGH 2
int pcl_step_phase_redirect(pcl_ctx *ctx, int phase, double g, double c, uint64_t seed, uint32_t pass,
                            int64_t *count_out_host /* [1]: re-directed */);

/* An absorbing medium (AbsorptionStep): the single-scattering albedo, by layer.  Called anywhere behind the scatter step of a pass
 * and before the next Newton step (before or behind pcl_step_phase_redirect), it lets each photon that step made interact be
 * ABSORBED instead, with probability 1 - omega0 of the layer it stands in, in ONE sweep of the resident store.  Analog: an absorbed
 * photon is left in the store at rest where it is; E is no statistical weight and is never scaled (the wavelength-dependent scatter
 * step reads it as the photon's colour).  Nothing is removed; r, dr, E, ids and kinds are not written, and E is asked for only
 * with energy bins.  "Interacted in this pass" is read off the store by pcl_step_phase_redirect's rule (not behind a
 * PCL_SCATTER_PY_DV step).  All arithmetic is fp64, every operation rounded once, in the order written; an fp32 store's values are
 * widened first (exact); what is written is zero.
 *   interacted  iff  the particle is a photon and (dv0 != 0 or dv1 != 0 or dv2 != 0)                    (NaN != 0 is true)
 *   n_layers == 0:  b = 0 for everybody: omega0_host[0] holds everywhere; edges_host and center_host are ignored
 *   n_layers = L >= 1:  d = r - center;  q = (d0*d0 + d1*d1) + d2*d2;  e2_k = e_k*e_k (made on the host);
 *                   inside iff e2_0 <= q and q <= e2_L (NaN: not inside);  b = the layer with e2_b <= q < e2_(b+1), the last one
 *                   closed (numpy.histogram); no square root is taken.  A photon that is not inside is counted as interacting and
 *                   left alone.
 *   inside and omega0_host[b] < 1:  u = u53(w0, w1) of the block below;  absorbed iff not (u < omega0_host[b])
 *                   (omega0 0: every interacting photon inside is absorbed; omega0 1: nothing is drawn)
 *   absorbed:       v = 0;  dv = 0
 * dv = 0 and not pcl_step_surface_reflect's dv = 0 - v_old: that call ends a pass, this one stands in the middle of one, and a
 * pcl_step_phase_redirect or a second call of this entry point later in the pass must see a photon that did not scatter and leave
 * it at rest (with dv = -v_old the phase function would give it the speed c again).  From then on the photon is what the ground
 * leaves behind: pcl_step_newton does not move it, the scatter steps hit it on a draw of exactly 0 only.
 * Compare, subtract, multiply and add only: everything can be restated bit for bit.  The draw is the Philox4x32-10 block with the
 * key (seed_lo, seed_hi) and the counter (id_lo, id_hi, pass, 12), u53 of pcl_store_apply_source; ``pass`` is the caller's own
 * counter.  The word 12 is used by nothing else (scatter kernels 0 and 1, fill and source 2..5, pcl_step_surface_reflect 8 and 9,
 * pcl_step_phase_redirect 10 and 11), so every other step draws what it drew, and a photon draws the same number however the run is
 * sharded.
 * omega0_host: L' = max(L, 1) doubles in [0, 1].  edges_host: L + 1 finite, non-negative, strictly increasing radii about
 * center_host (3 finite doubles, NULL = the origin) whose squares are finite and strictly increasing, 1 <= L <=
 * PCL_ABSORB_MAX_LAYERS.  E_edges_host: n_E_bins + 1 finite, strictly increasing doubles, 1 <= n_E_bins <= PCL_ABSORB_MAX_BINS, or
 * n_E_bins == 0 and no histogram.  2 + L' + L' * n_E_bins may not exceed PCL_ABSORB_MAX_CELLS: a workgroup's uint32 cells (48 KiB)
 * and the three tables stay below 64 KiB of LDS.
 * counts_out_host[0] = photons that interacted, [1] = absorbed, [2 + b] = absorbed in layer b, by this call;
 * E_hist_out_host[b * n_E_bins + k] = absorbed in layer b with E in bin k ([e_k, e_(k+1)), the last bin closed; NaN and energies
 * outside the edges in no bin).
 * A store that is not uniform costs the host traffic it costs pcl_step_surface_reflect; the ids go along only if some omega0 < 1.
 * PCL_ERR_ARG (NULL omega0 or counts, L outside 0 .. PCL_ABSORB_MAX_LAYERS, an omega0 outside [0, 1] or NaN, bad edges or centre,
 * bad n_E_bins or E edges, NULL histogram with bins, too many cells) is returned before anything is launched or written;
 * PCL_ERR_STATE without a store; an empty store answers zeros without a launch.  Host pointers; one device allocation per call,
 * handed back on every way out; synchronises once, with the copy of the tallies.  pcl_last_error() is generic, as for
 * pcl_step_surface_reflect, whose source file these two entry points share (physicl_amd/csrc/pcl_surface.hip). */
#define PCL_ABSORB_MAX_LAYERS 64
#define PCL_ABSORB_MAX_BINS 1024   /* per layer */
#define PCL_ABSORB_MAX_CELLS 12288 /* 2 + L' + L' * n_E_bins */
int pcl_step_absorb_scattered(pcl_ctx *ctx, int n_layers, const double *omega0_host, const double *edges_host,
                              const double *center_host, int n_E_bins, const double *E_edges_host, uint64_t seed, uint32_t pass,
                              int64_t *counts_out_host /* [2 + L'] */, int64_t *E_hist_out_host /* [L' * n_E_bins] or NULL */);

/* Phase functions by layer (LayeredPhaseStep): pcl_step_phase_redirect with a law that depends on where the photon stands, and with
 * tabulated laws.  Called where pcl_step_phase_redirect would be called (directly behind the scatter step of a pass, before or behind
 * pcl_step_absorb_scattered), it re-directs the photons that step scattered in ONE sweep of the resident store.  Each of the L' =
 * max(n_layers, 1) radial layers mixes the n_laws = M laws with its own weights.  A pass holds ONE phase step: this entry point
 * shares the blocks 10 and 11 with pcl_step_phase_redirect and must not be called in a pass in which that one, or this one, has
 * already been called with the same ``pass``.  Nothing is removed; r, dr, E, ids and kinds are not written, E is not asked for and r
 * only with layers.  All arithmetic is fp64, every operation rounded once, in the order written.
 *   scattered  iff  the particle is a photon, (dv0 != 0 or dv1 != 0 or dv2 != 0), and o = v - dv has 0 < o.o < inf
 *                   (pcl_step_phase_redirect's "re-directed")
 *   n_layers == 0:  b = 0 for everybody.   n_layers = L >= 1:  the layer b of q = (d0*d0 + d1*d1) + d2*d2, d = r - center, in
 *                   e2_k = e_k*e_k exactly as pcl_step_absorb_scattered finds it (last layer closed, NaN: in no layer, no square root)
 *   outside every layer:  counted as scattered, not written: the photon keeps the direction the scatter step gave it
 *   inside:         re-directed.  The law: M == 1: j = 0;  otherwise j = the first law with u_s < cum_host[b*M + j], u_s = u53(w0, w1)
 *                   of the block (id_lo, id_hi, pass, 13).  (Whether that block is computed for a row that is one-hot is the
 *                   kernel's business: the first positive entry of such a row is 1 and 0 <= u_s < 1.)
 *   block A (id_lo, id_hi, pass, 10): u_a = u53(w0, w1), u_b = u53(w2, w3);  mu by the law's kind:
 *     PCL_PHASE_ISOTROPIC, PCL_PHASE_HG with g_host[j], PCL_PHASE_RAYLEIGH (block B (id_lo, id_hi, pass, 11)): the lines of
 *     pcl_step_phase_redirect, bit for bit
 *     PCL_PHASE_TABLE: a piecewise-constant density on K bins with the nodes mu_0 = -1 < ... < mu_K = 1 and the cumulative values
 *     F_0 = 0 < ... < F_K = 1 (made by the caller: F = cumsum(p_k*(mu_(k+1) - mu_k)) / sum);  k = the bin of u_a in F ([F_k, F_(k+1)),
 *     always inside);  s_k = (mu_(k+1) - mu_k) / (F_(k+1) - F_k), made by the library on the host: two subtractions and one division,
 *     each rounded once;  mu = min(max(mu_k + (u_a - F_k)*s_k, mu_k), mu_(k+1))
 *   then s, psi, the frame about w = o / sqrt(o.o), dir, v = c*dir and dv = v - o exactly as pcl_step_phase_redirect.
 * So a call with one law and no layers leaves the store bit for bit as pcl_step_phase_redirect with that law, seed and pass leaves
 * it.  The word 13 is used by nothing else (scatter kernels 0 and 1, fill and source 2..5, pcl_step_surface_reflect 8 and 9,
 * pcl_step_phase_redirect 10 and 11, pcl_step_absorb_scattered 12).
 * kinds_host: M ints, 1 <= M <= PCL_LPHASE_MAX_LAWS.  g_host: M doubles, read for PCL_PHASE_HG laws only (finite, |g| < 1; may be
 * NULL without such a law).  n_bins_host: M ints, read for PCL_PHASE_TABLE laws only: K, 1 <= K <= PCL_LPHASE_MAX_NODES, the sum
 * over the tables at most PCL_LPHASE_MAX_TOTAL_NODES.  mu_host, F_host: the K + 1 nodes and cumulative values of the tables one behind
 * the other, in the order of the laws (all three may be NULL without a table).  cum_host: L' rows of M cumulative weights, each row
 * not decreasing from a value >= 0 and ending in exactly 1.  edges_host, center_host: as pcl_step_absorb_scattered, 1 <= L <=
 * PCL_LPHASE_MAX_LAYERS, ignored with n_layers == 0.  ``c``: the speed of light in code units.  The tables (at the limits about 54
 * KiB) and the cells stay below 64 KiB of LDS; a call is sized by what it uses.
 * counts_out_host[0] = photons scattered, [1] = re-directed, [2 + b] = re-directed in layer b, [2 + L' + j] = re-directed by law j.
 * A store that is not uniform costs the host traffic it costs pcl_step_surface_reflect.  PCL_ERR_ARG (NULL kinds, weights or counts,
 * M or L outside their limits, an unknown kind, a bad g, a table with bad counts, nodes that do not rise from -1 to 1, cumulative
 * values that do not rise strictly from 0 to 1, a row of weights that decreases or does not end in 1, bad edges or centre, c not
 * finite) is returned before anything is launched or written; PCL_ERR_STATE without a store; an empty store answers zeros without a
 * launch.  Host pointers; one device allocation per call, handed back on every way out; synchronises once, with the copy of the
 * tallies.  pcl_last_error() is generic, as for pcl_step_surface_reflect, whose source file these two entry points share. */
#define PCL_PHASE_TABLE 3
#define PCL_LPHASE_MAX_LAWS 8
#define PCL_LPHASE_MAX_LAYERS 64
#define PCL_LPHASE_MAX_NODES 1024       /* bins of one table */
#define PCL_LPHASE_MAX_TOTAL_NODES 2048 /* bins of all tables of a call */
int pcl_step_phase_layered(pcl_ctx *ctx, int n_laws, const int *kinds_host, const double *g_host, const int *n_bins_host,
                           const double *mu_host, const double *F_host, int n_layers, const double *cum_host,
                           const double *edges_host, const double *center_host, double c, uint64_t seed, uint32_t pass,
                           int64_t *counts_out_host /* [2 + L' + M] */);

/* A continuous source (RecycleStep): the last call of a pass, behind pcl_step_surface_reflect if there is one.  A photon the ground
 * or the medium has absorbed stays in the store at rest, one that has left through the top of the atmosphere flies on for ever:
 * this call gives the slots of both back to a photon source, in ONE sweep of the resident store.  The population stays constant and
 * the store dense; ids and kinds are never written, nothing is removed.  All arithmetic is fp64, unfused, every operation rounded
 * once, in the order written; an fp32 store's values are widened first (exact) and what is written is rounded once to the store's
 * dtype.
 *   rest   =  at_rest and v0 == 0 and v1 == 0 and v2 == 0                            (-0.0 counts as 0; a NaN in v: not at rest)
 *   d = r - center;  q = (d0*d0 + d1*d1) + d2*d2;  top2 = top*top (made on the host)
 *   gone   =  top > 0 (a top is given) and not rest and q > top2         (exactly on the sphere: not gone; NaN: not gone; inf: gone)
 *   spent  =  the particle is a photon and (rest or gone)
 * Plain Objects (kind 0) are never spent.  A particle that is not spent is not written at all.  The v rows are read only with
 * at_rest, the r rows only with a top.  A spent photon is re-emitted by ``src`` with exactly the arithmetic written out above for
 * pcl_store_apply_source -- mu per angular mode, s, psi, the frame e1, e2, d, rho and phi per spatial mode, the same sin / cos --
 * from blocks of its own: key (seed_lo, seed_hi), u53 as there,
 *   direction:  counter (id_lo, id_hi, pass, 14): u_a = u53(w0, w1), u_b = u53(w2, w3)      (a beam draws nothing: v = c*d)
 *   position:   counter (id_lo, id_hi, pass, 15): u_c = u53(w0, w1), u_d = u53(w2, w3)      (a point draws nothing: r = origin)
 *   dr = 0;  dv = 0                                                          (a newborn has not moved and has not scattered)
 * and, unlike the fill, EVERY row r, v, dr, dv of a spent photon is written, for a beam and a point source too.
 *   n_E > 0:    u = u53(w0, w1) of the counter (id_lo, id_hi, pass, 16);  E = grid_host[x] for the first x with cdf_host[x] >= u
 *               -- the table form of pcl_store_fill_photons_table, found by a binary search: compares only, bit for bit restatable.
 *   n_E == 0:   E is neither written nor asked for: a recycled photon keeps its energy.  Exact for a monochromatic source, or
 *               wherever no sink depends on E.
 * ``pass`` is the caller's own counter: a slot keeps its id, and every re-emission draws new numbers because ``pass`` moves.  The
 * words 14, 15 and 16 are used by nothing else (scatter kernels 0 and 1, fill and source 2..5, pcl_step_surface_reflect 8 and 9,
 * pcl_step_phase_redirect 10 and 11, pcl_step_absorb_scattered 12, pcl_step_phase_layered 13), so every other step draws what it drew,
 * and a photon is re-emitted the same way however the run is sharded.
 * ``c`` = the speed of light in code units.  ``top`` <= 0: no top.  center_host: 3 finite doubles, NULL = the origin.  cdf_host,
 * grid_host: n_E doubles each, 0 <= n_E <= PCL_RECYCLE_MAX_BINS (the table sits in 16 KiB of LDS at the most); cdf non-decreasing,
 * its last value exactly 1; grid finite.
 * counts_out_host[0] = photons recycled because they were at rest, [1] = because they were beyond the top, by this call.
 * A store that is not uniform costs the host traffic it costs pcl_step_surface_reflect.  PCL_ERR_ARG (NULL src or counts, unknown
 * mode, non-finite frame / origin / c / centre, cos_half_angle outside [-1, 1] for a cone, radius negative or not finite for a disc /
 * gaussian, top not finite or its square not finite, neither at_rest nor a top, n_E outside 0 .. PCL_RECYCLE_MAX_BINS, a NULL table
 * with n_E > 0, a cdf that decreases or does not end in 1, a grid that is not finite) is returned before anything is launched or
 * written; PCL_ERR_STATE without a store; an empty store answers zeros without a launch.  Host pointers; one device allocation per
 * call, handed back on every way out; synchronises once, with the copy of the two counts.  pcl_last_error() is generic, as for
 * pcl_step_surface_reflect, whose source file these two entry points share (physicl_amd/csrc/pcl_surface.hip). */
#define PCL_RECYCLE_MAX_BINS 1024
int pcl_step_recycle_spent(pcl_ctx *ctx, const pcl_source *src, double c, int at_rest, double top /* <= 0: none */,
                           const double *center_host, int n_E, const double *cdf_host, const double *grid_host, uint64_t seed,
                           uint32_t pass, int64_t *counts_out_host /* [2]: at rest, escaped */);

/* Absorption along the path (PathAbsorptionStep): a gas that absorbs without scattering -- Beer-Lambert over the move a photon has
 * just made, with a coefficient that depends on the radial layer it stands in and on the band its energy falls in.  Called anywhere
 * behind pcl_step_newton in a pass (before or behind the scatter, phase, absorption and ground calls, before
 * pcl_step_recycle_spent), it absorbs in ONE sweep of the resident store.  A photon moves c*dt in every pass, across a bounce off the
 * ground too, so the path length is not read from the store: the host makes the probability of absorption per pass,
 * p = -expm1(-k * (c*dt)), and the device only ever sees p.  Nothing is removed; r, dr, E, ids and kinds are never written.  All
 * arithmetic is fp64, unfused, every operation rounded once, in the order written; an fp32 store's values are widened first (exact);
 * what is written is zero.  L' = max(n_layers, 1), B' = max(n_E_bins, 1).
 *   at rest   iff  v0 == 0 and v1 == 0 and v2 == 0            (-0.0 counts as 0; a NaN in v: moving).  A slot at rest is skipped,
 *                  and nothing more is loaded for it; a slot with v0 != 0 is decided by v0 alone and loads neither v1 nor v2.
 *   a moving particle that is not a photon (kind 0) is skipped.
 *   n_layers == 0:  b = 0;  edges_host and center_host are ignored, r is not read
 *   n_layers = L >= 1:  d = r - center;  q = (d0*d0 + d1*d1) + d2*d2;  e2_k = e_k*e_k (made on the host);  inside iff e2_0 <= q and
 *                  q <= e2_L (NaN: not inside);  b = the layer with e2_b <= q < e2_(b+1), the last one closed (numpy.histogram);
 *                  no square root is taken -- the layer pcl_step_absorb_scattered finds.  A photon in no layer is skipped.
 *   n_E_bins == 0:  e = 0;  E is neither read nor asked for (pcl_store_field_ptr): a wavelength-dependent scatter step keeps its
 *                  lambda^-4 cache
 *   n_E_bins = B >= 1:  e = the bin of E (widened to double) in E_edges_host: [E_e, E_(e+1)), the last one closed; NaN and
 *                  energies outside the edges are in no band: the photon is skipped.  (Asking for E drops that cache, every pass: the
 *                  ABI has no read-only accessor.)
 *   exposed   =    a moving photon with a layer and a band;  p = p_host[b * B' + e]
 *   p == 0:        nothing is drawn.   p > 0:  u = u53(w0, w1) of the block below;  absorbed iff u < p       (p == 1: every one)
 *   absorbed:      v = 0;  dv = 0          (pcl_step_absorb_scattered's convention, for its reason: a later phase or absorption
 *                  call of the pass leaves the photon alone, and pcl_step_recycle_spent with at_rest picks it up)
 * A photon that is not absorbed is not written at all.  Compare, subtract, multiply and add only -- no transcendental function, no
 * division, no square root: everything can be restated bit for bit.  The draw is the Philox4x32-10 block with the key (seed_lo,
 * seed_hi) and the counter (id_lo, id_hi, pass, 17), u53 of pcl_store_apply_source; ``pass`` is the caller's own counter.  The word
 * 17 is used by nothing else (scatter kernels 0 and 1, fill and source 2..5, pcl_step_surface_reflect 8 and 9,
 * pcl_step_phase_redirect 10 and 11, pcl_step_absorb_scattered 12, pcl_step_phase_layered 13, pcl_step_recycle_spent 14, 15 and 16),
 * so every other step draws what it drew, and a photon draws the same number however the run is sharded.
 * p_host: L' * B' doubles in [0, 1], row b the layer, column e the band.  edges_host: L + 1 radii as for
 * pcl_step_absorb_scattered, 1 <= L <= PCL_PATH_ABSORB_MAX_LAYERS.  E_edges_host: B + 1 finite, strictly increasing doubles, 1 <= B
 * <= PCL_PATH_ABSORB_MAX_BANDS.  L' * B' may not exceed PCL_PATH_ABSORB_MAX_CELLS: a workgroup's uint32 cells (16 KiB), the
 * probabilities (32 KiB) and the two edge tables stay below 64 KiB of LDS.  center_host: 3 finite doubles, NULL = the origin.
 * counts_out_host[0] = photons exposed, [1] = absorbed, by this call;  cells_out_host[b * B' + e] = absorbed in layer b and band e.
 * A store that is not uniform costs the host traffic it costs pcl_step_surface_reflect; the ids go along only if some p > 0.
 * PCL_ERR_ARG (NULL p, counts or cells, L outside 0 .. PCL_PATH_ABSORB_MAX_LAYERS, B outside 0 .. PCL_PATH_ABSORB_MAX_BANDS, too
 * many cells, a p outside [0, 1] or NaN, NULL or bad edges with L > 0, NULL or bad E edges with B > 0, a centre that is not finite)
 * is returned before the store is looked at, and nothing is launched or written; PCL_ERR_STATE without a store; an empty store
 * answers zeros without a launch.  Host pointers; one device allocation per call, handed back on every way out; synchronises once,
 * with the copy of the tallies.  pcl_last_error() is generic, as for pcl_step_surface_reflect, whose source file these two entry
 * points share (physicl_amd/csrc/pcl_surface.hip). */
#define PCL_PATH_ABSORB_MAX_LAYERS 64
#define PCL_PATH_ABSORB_MAX_BANDS 1024
#define PCL_PATH_ABSORB_MAX_CELLS 4096 /* L' * B' */
int pcl_step_absorb_path(pcl_ctx *ctx, int n_layers, int n_E_bins, const double *p_host, const double *edges_host,
                         const double *center_host, const double *E_edges_host, uint64_t seed, uint32_t pass,
                         int64_t *counts_out_host /* [2]: exposed, absorbed */, int64_t *cells_out_host /* [L' * B'] */);

/* Re-emission in place (ReemissionStep): what the ground or the medium has absorbed is radiated again from where it was absorbed.
 * Every sink of a pass (pcl_step_surface_reflect with an albedo, pcl_step_absorb_scattered, pcl_step_absorb_path) parks a photon
 * at rest; called behind them and before pcl_step_recycle_spent (which then takes what this call left at rest), this call gives the
 * parked photons a new direction -- and, with a table, a new energy -- from their own position, by a law, a spectrum and a yield
 * that belong to the radial layer they are parked in, in ONE sweep of the resident store.  Nothing is removed; r, ids and kinds are
 * never written.  All arithmetic is fp64, unfused, every operation rounded once, in the order written; an fp32 store's values are
 * widened first (exact) and what is written is rounded once to the store's dtype.  L' = max(n_layers, 1).
 *   rest    =  v0 == 0 and v1 == 0 and v2 == 0                  (-0.0 counts as 0; a NaN in v: moving).  A slot with v0 != 0 is
 *              decided by v0 alone: it loads neither v1 nor v2, nor anything else.
 *   n_layers == 0:  b = 0;  edges_host is ignored, and r is read only if that one layer is lambertian
 *   n_layers = L >= 1:  d = r - center;  q = (d0*d0 + d1*d1) + d2*d2;  e2_k = e_k*e_k (made on the host);  inside iff e2_0 <= q and
 *              q <= e2_L (NaN: not inside);  b = the layer with e2_b <= q < e2_(b+1), the last one closed (numpy.histogram);
 *              no square root is taken -- the layer pcl_step_absorb_scattered finds
 *   parked  =  rest and the particle is a photon (kind != 0) and it has a layer b
 *   eta_b == 0:  nothing is drawn.
 *   eta_b > 0:   u = u53(w0, w1) of the counter (id_lo, id_hi, pass, 18);  re-emitted iff u < eta_b           (eta_b == 1: every one)
 *   direction:   (u_a, u_b) = (u53(w0, w1), u53(w2, w3)) of the counter (id_lo, id_hi, pass, 19)
 *     isotropic:   w = (1, 0, 0);  mu = 1 - 2*u_a
 *     lambertian:  d = r - center;  q as above;  s = sqrt(q);  w_k = d_k / s;  mu = sqrt(1 - u_a)       (about the local vertical)
 *                  q == 0 or q not finite: the photon has no vertical; it is not re-emitted and is counted in parked only
 *     e1, e2 = the frame about w, sc, ss of (mu, u_b) and the direction (sc*e1_k + ss*e2_k) + mu*w_k as written out for
 *     pcl_step_surface_reflect (frame, polar, turned), the same sin / cos;  v_k = c * direction_k
 *   energy (only if layer b has a table):  u = u53(w0, w1) of the counter (id_lo, id_hi, pass, 20);  E = grid_b[x] for the first x
 *              with cdf_b[x] >= u -- pcl_step_recycle_spent's look-up, a binary search: compares only.  The new E does not look at
 *              the old one.  Without a table a re-emitted photon keeps its E; if no layer has a table E is neither written nor
 *              asked for (pcl_store_field_ptr): a wavelength-dependent scatter step keeps its lambda^-4 cache.
 *   dr = 0;  dv = 0                    (later calls of the pass see a photon that has neither moved nor scattered)
 * A particle that is not re-emitted is not written at all.  The Philox4x32-10 blocks have the key (seed_lo, seed_hi), u53 of
 * pcl_store_apply_source; ``pass`` is the caller's own counter, so a photon that stays parked (eta_b < 1) draws again in the next
 * call: a lifetime of dt / eta_b.  The words 18, 19 and 20 are used by nothing else (scatter kernels 0 and 1, fill and source 2..5,
 * pcl_step_surface_reflect 8 and 9, pcl_step_phase_redirect 10 and 11, pcl_step_absorb_scattered 12, pcl_step_phase_layered 13,
 * pcl_step_recycle_spent 14, 15 and 16, pcl_step_absorb_path 17: 0-5 and 8-17 are taken), so every other step draws what it drew, and
 * a photon is re-emitted the same way however the run is sharded.
 * edges_host: L + 1 radii as for pcl_step_absorb_scattered, 1 <= L <= PCL_REEMIT_MAX_LAYERS.  center_host: 3 finite doubles, NULL =
 * the origin.  eta_host: L' doubles in [0, 1].  lambertian_host: L' ints, 0 (isotropic) or 1.  table_offsets_host: L' + 1 ints, the
 * first 0, not decreasing: layer b's table is [offsets[b], offsets[b + 1]) of cdf_host and grid_host, equal neighbours: no table; a
 * table has at most PCL_REEMIT_MAX_BINS entries, all together at most PCL_REEMIT_MAX_TOTAL_BINS (32 KiB of LDS); each table's cdf
 * does not decrease and ends in exactly 1, the grid is finite.  ``c`` = the speed of light in code units.
 * counts_out_host[0] = photons parked (at rest, with a layer), [1] = re-emitted, [2 + b] = re-emitted from layer b, by this call.
 * A store that is not uniform costs the host traffic it costs pcl_step_surface_reflect; the ids go along only if some eta > 0.
 * PCL_ERR_ARG (NULL eta, flags, offsets or counts, L outside 0 .. PCL_REEMIT_MAX_LAYERS, an eta outside [0, 1] or NaN, a flag that
 * is neither 0 nor 1, offsets that do not start at 0, decrease or exceed a limit, NULL tables with entries, a cdf that decreases or
 * does not end in 1, a grid that is not finite, NULL or bad edges with L > 0, a centre or c that is not finite) is returned before
 * the store is looked at, and nothing is launched or written; PCL_ERR_STATE without a store; an empty store answers zeros without a
 * launch.  Host pointers; one device allocation per call, handed back on every way out; synchronises once, with the copy of the
 * counts.  pcl_last_error() is generic, as for pcl_step_surface_reflect, whose source file these two entry points share
 * (physicl_amd/csrc/pcl_surface.hip). */
#define PCL_REEMIT_MAX_LAYERS 64
#define PCL_REEMIT_MAX_BINS 1024
#define PCL_REEMIT_MAX_TOTAL_BINS 2048
int pcl_step_reemit_parked(pcl_ctx *ctx, int n_layers, const double *edges_host, const double *center_host,
                           const double *eta_host /* [L'] */, const int *lambertian_host /* [L'] */,
                           const int *table_offsets_host /* [L' + 1], equal neighbours: no table */, const double *cdf_host,
                           const double *grid_host, double c, uint64_t seed, uint32_t pass,
                           int64_t *counts_out_host /* [2 + L']: parked, re-emitted, by layer */);

/* A refracting sphere (RefractiveSurfaceStep): a dielectric interface between a medium of refractive index n_inside within the
 * sphere of ``radius`` about center_host and one of n_outside around it -- an ocean under an atmosphere, a drop, the top of an
 * atmosphere.  Photons whose last move crossed the sphere, in either direction, are refracted by Snell's law or reflected -- with
 * Fresnel's probability for unpolarised light, and always beyond the critical angle -- in ONE sweep of the resident store.  It
 * stands where a ground would: the last call of a pass (before pcl_step_recycle_spent).  Nothing is removed; E, ids and kinds are
 * not touched and E is not asked for.  The model's photons move c*dt per pass everywhere (pcl_step_absorb_path relies on it), so
 * this call changes DIRECTIONS, NOT SPEEDS: |v| = c on both sides.  All arithmetic is fp64, unfused, every operation rounded
 * once, in the order written (x.y of two vectors is (x0*y0 + x1*y1) + x2*y2); an fp32 store's values are widened first (exact) and
 * what is written is rounded once to the store's dtype.
 *   d = r - center;  m = dr;  p = d - m;  q_now = d.d;  q_prev = p.p;  R2 = radius*radius (made on the host)
 *   inward   iff  q_now < R2 and R2 <= q_prev and q_prev < inf       (pcl_step_surface_reflect's test, character for character)
 *   outward  iff  q_prev < R2 and R2 <= q_now and q_now < inf
 * -- the two crossings of pcl_step_shell_crossings for one shell (a particle exactly on the sphere is outside), so that tally,
 * made BEFORE this call, counts exactly the photons that cross here if every q_prev is finite.  Only photons (kind != 0) cross; a
 * NaN anywhere in r or dr: no crossing.  A particle that does not cross is not written at all.
 *   a = m.m;  b = p.m;  cq = q_prev - R2;  disc = max(b*b - a*cq, 0);  sq = sqrt(disc)
 *   inward:   t = cq / (sq - b)                                                           (pcl_step_surface_reflect's lines)
 *   outward:  the other root, in the form that does not cancel:  b > 0:  t = (0 - cq) / (sq + b);  otherwise  t = (sq - b) / a;
 *             then t = min(max(t, 0), 1)  (min and max ignore a NaN: fmin, fmax)
 *   x = p + t*m;  nrm = x / sqrt(x.x);  sa = sqrt(a);  w = (1 - t)*sa;  mh = m / sa       (as pcl_step_surface_reflect goes on)
 *   inward:   N = nrm;   eta = n_outside / n_inside           (the two ratios are made on the host, one rounding each)
 *   outward:  N = -nrm;  eta = n_inside / n_outside
 *   ci = max(0 - mh.N, 0);  k = 1 - (eta*eta)*(1 - ci*ci)
 *   k < 0:    total internal reflection:  dir = mh + (2*ci)*N;  nothing is drawn
 *   k >= 0:   ct = sqrt(k) -- but eta == 1 (no interface): ct = ci, whatever 1 - (1 - ci*ci) rounds to, so that F = 0 and dir = mh --;
 *             ec = eta*ci;  rs = (ec - ct) / (ec + ct);  ect = eta*ct;  rp = (ci - ect) / (ci + ect);  F = (rs*rs + rp*rp)*0.5
 *             fresnel != 0 and F > 0 (a NaN is not):  u = u53(w0, w1) of the counter (id_lo, id_hi, pass, 21);  reflected iff u < F:
 *             dir = mh + (2*ci)*N
 *             otherwise refracted:  dir = eta*mh + (ec - ct)*N
 *   fresnel == 0:  nothing is ever drawn; every crossing that is not total refracts.
 *   v = c*dir;  dv = v - v_old;  dr = w*dir;  y = x + dr;  r = center + y         (the rest of the move, flown along dir)
 * One interaction per photon per call.  overshot: after the write, y.y >= R2 for an outcome that ends inside (inward refracted,
 * outward reflected or total), y.y < R2 for one that ends outside (inward reflected, outward refracted) -- the rest of the move has
 * carried the photon through the sphere again (a NaN: not counted).  A counter only, it changes nothing: c*dt is too large for
 * the radius.
 * The Philox4x32-10 block has the key (seed_lo, seed_hi), u53 of pcl_store_apply_source; ``pass`` is the caller's own counter.
 * The word 21 is used by nothing else (scatter kernels 0 and 1, fill and source 2..5, pcl_step_surface_reflect 8 and 9,
 * pcl_step_phase_redirect 10 and 11, pcl_step_absorb_scattered 12, pcl_step_phase_layered 13, pcl_step_recycle_spent 14, 15 and 16,
 * pcl_step_absorb_path 17, pcl_step_reemit_parked 18, 19 and 20: 0-5 and 8-20 are taken), so every other step draws what it drew,
 * and a photon meets the same fate however the run is sharded.
 * counts_out_host[0] = inward refracted, [1] = inward reflected (a total reflection on the way in, n_outside > n_inside, among
 * them), [2] = outward refracted, [3] = outward reflected (drawn), [4] = outward total, [5] = overshot, by this call.
 * A store that is not uniform costs the host traffic it costs pcl_step_surface_reflect; the ids go along only with fresnel != 0.
 * PCL_ERR_ARG (NULL counts, radius not positive / not finite / its square not finite, n_inside or n_outside not positive or not
 * finite, a centre or c that is not finite) is returned before the store is looked at -- by the group's entry point before the group
 * is --, and nothing is launched or written; PCL_ERR_STATE without a store; an empty store answers zeros without a launch.  Host
 * pointers; one device allocation per call, handed back on every way out; synchronises once, with the copy of the six counts.
 * pcl_last_error() is generic, as for pcl_step_surface_reflect, whose source file these two entry points share
 * (physicl_amd/csrc/pcl_surface.hip). */
int pcl_step_refract_surface(pcl_ctx *ctx, double radius, const double *center_host, double n_inside, double n_outside, int fresnel,
                             double c, uint64_t seed, uint32_t pass,
                             int64_t *counts_out_host /* [6]: in refracted, in reflected, out refracted, out reflected, out total, overshot */);

/* A spectral ground (SpectralSurfaceStep): pcl_step_surface_reflect's sphere with an albedo and a mirrored share that depend on the
 * band the photon's energy falls in -- vegetation, snow, water, a ground that is black in the infrared -- in ONE sweep of the resident
 * store.  It stands where the ground stands: the last call of a pass (before pcl_step_reemit_parked and pcl_step_recycle_spent), and a
 * pass has ONE ground: this call shares the ground's counter words 8 and 9.  Nothing is removed; the ground stays opaque.  E is read
 * and never written; ids and kinds are not touched.  All arithmetic is fp64, unfused, every operation rounded once, in the order
 * written; an fp32 store's values are widened first (exact) and what is written is rounded once to the store's dtype.
 *   E_edges_host: B + 1 finite, strictly increasing doubles in the unit E is stored in, 1 <= B <= PCL_SPECTRAL_MAX_BANDS;
 *   albedo_host, specular_host: B doubles in [0, 1] each.  center_host: 3 finite doubles, NULL = the origin.
 *   hit  iff  q_now < R2 and R2 <= q_prev and q_prev < inf, a photon             (pcl_step_surface_reflect's test, its d, m, p, q)
 *   e = (double)E;  band b: pcl_step_absorb_path's rule for E_edges -- numpy.histogram's bins [E_b, E_(b+1)), the last one closed;
 *   e < E_0, e > E_B or a NaN: NO BAND -- the photon is absorbed and counted in out_of_band, nothing is drawn
 *   albedo_b < 1:  u = u53(w0, w1) of the counter (id_lo, id_hi, pass, 9);  reflected iff u < albedo_b   (albedo_b == 1: reflected, no draw)
 *   reflected and 0 < specular_b < 1:  u = u53(w0, w1) of the counter (id_lo, id_hi, pass, 22);  mirrored iff u < specular_b
 *   reflected and specular_b == 1: mirrored, no draw;  specular_b == 0: not mirrored, no draw
 *   t, x, nrm, sa, w: pcl_step_surface_reflect's lines, operation for operation
 *   absorbed:      r = center + x;  v = 0;  dr = x - p;  dv = 0 - v_old                                    (the ground's park)
 *   mirrored:      mh = m / sa;  dn = mh.nrm;  dir = mh - (2*dn)*nrm                                       (the ground's specular line)
 *   not mirrored:  (u_a, u_b) of the counter (id_lo, id_hi, pass, 8);  mu = sqrt(1 - u_a);  dir as the ground's lambertian lines
 *   reflected:     v = c*dir;  dv = v - v_old;  dr = w*dir;  r = center + (x + dr)
 * So with one band that holds every energy of the store and specular = 0 (1) the store is left bit for bit as
 * pcl_step_surface_reflect leaves it in PCL_SURFACE_LAMBERTIAN (PCL_SURFACE_SPECULAR) with that albedo, seed and pass.
 * The Philox4x32-10 block has the key (seed_lo, seed_hi), u53 of pcl_store_apply_source; ``pass`` is the caller's own counter.
 * The word 22 is used by nothing else (scatter kernels 0 and 1, fill and source 2..5, pcl_step_surface_reflect and this call 8 and 9,
 * pcl_step_phase_redirect 10 and 11, pcl_step_absorb_scattered 12, pcl_step_phase_layered 13, pcl_step_recycle_spent 14, 15 and 16,
 * pcl_step_absorb_path 17, pcl_step_reemit_parked 18, 19 and 20, pcl_step_refract_surface 21: 0-5 and 8-21 are taken), so every
 * other step draws what it drew, and a photon meets the same fate however the run is sharded.
 * counts_out_host[0] = reflected, [1] = absorbed (those in no band among them), [2] = mirrored (of the reflected), [3] = out_of_band;
 * bands_out_host[0 .. B) = reflected by band, [B .. 2B) = absorbed by band (a photon in no band is in neither), by this call.
 * A store that is not uniform costs the host traffic it costs pcl_step_surface_reflect; the ids go along unless every albedo and
 * every specular is 1.  Asking for E costs a wavelength-dependent scatter step its term cache, every pass (the library has no
 * read-only access to E), as pcl_step_absorb_path's bands do.
 * PCL_ERR_ARG (NULL edges, albedo, specular, counts or bands, B outside 1 .. PCL_SPECTRAL_MAX_BANDS, edges that are not finite and
 * strictly increasing, an albedo or a specular outside [0, 1] or NaN, radius not positive / not finite / its square not finite, a
 * centre or c that is not finite) is returned before the store is looked at -- by the group's entry point before the group is --,
 * and nothing is launched or written; PCL_ERR_STATE without a store; an empty store answers zeros without a launch.  Host pointers;
 * one device allocation per call, handed back on every way out; synchronises once, with the copy of the tallies.
 * pcl_last_error() is generic, as for pcl_step_surface_reflect, whose source file these two entry points share
 * (physicl_amd/csrc/pcl_surface.hip). */
#define PCL_SPECTRAL_MAX_BANDS 1024
int pcl_step_ground_spectral(pcl_ctx *ctx, double radius, const double *center_host, int n_bands, const double *E_edges_host,
                             const double *albedo_host, const double *specular_host, double c, uint64_t seed, uint32_t pass,
                             int64_t *counts_out_host /* [4]: reflected, absorbed, mirrored, out_of_band */,
                             int64_t *bands_out_host /* [2][B]: reflected by band, absorbed by band */);

/* Scattering by layer and band (LayeredScatterStep): who scatters, with a scattering coefficient that depends on the radial layer a
 * photon stands in and on the band its energy falls in -- a cloud's optical depth, an aerosol spectrum beside the Rayleigh one, a
 * drop in vacuum.  The scattering twin of pcl_step_absorb_path: called behind pcl_step_newton (alone, or behind the scatter kernels
 * with first = 0) and before the phase, absorption and ground calls of the pass, it scatters in ONE sweep of the resident store.  A
 * photon moves c*dt in every pass, so the path length is not read from the store: the host makes the probability of scattering per
 * pass, p = -expm1(-k * (c*dt)), and the device only ever sees p.  Nothing is removed; r, dr, E, ids and kinds are never written.
 * All arithmetic is fp64, unfused, every operation rounded once, in the order written; an fp32 store's values are widened first
 * (exact) and what is written is rounded once to the store's dtype.  L' = max(n_layers, 1), B' = max(n_E_bins, 1).
 *   a particle that is not a photon (kind 0) is skipped and never written.
 *   at rest   iff  v0 == 0 and v1 == 0 and v2 == 0            (-0.0 counts as 0; a NaN in v: moving).  A slot with v0 != 0 is decided
 *                  by v0 alone and loads neither v1 nor v2; a slot at rest loads nothing more.
 *   layer b, band e:  pcl_step_absorb_path's lines, character for character -- n_layers == 0: b = 0, r is not read;  otherwise
 *                  d = r - center;  q = (d0*d0 + d1*d1) + d2*d2;  b = the layer with e2_b <= q < e2_(b+1), the last one closed, no
 *                  square root is taken;  n_E_bins == 0: e = 0, E is neither read nor asked for;  otherwise e = the bin of E (widened
 *                  to double) in E_edges_host: [E_e, E_(e+1)), the last one closed;  a NaN, a photon outside the edges: skipped
 *   exposed   =    a moving photon with a layer and a band;  p = p_host[b * B' + e]
 *   p == 0:        nothing is drawn.   p > 0:  u = u53(w0, w1) of the counter (id_lo, id_hi, pass, 23);  scattered iff u < p
 *   scattered:     (u_a, u_b) = (u53(w0, w1), u53(w2, w3)) of the counter (id_lo, id_hi, pass, 24);  w = (1, 0, 0);  mu = 1 - 2*u_a;
 *                  e1, e2 = the frame about w, sc, ss of (mu, u_b) and the direction (sc*e1_k + ss*e2_k) + mu*w_k as written out for
 *                  pcl_step_surface_reflect (frame, polar, turned), the same sin / cos -- pcl_step_reemit_parked's isotropic lines,
 *                  operation for operation: uniform on the sphere
 *                  v_k = c * direction_k;  dv_k = v_k - v_old_k         (both from the widened old velocity, rounded once: the
 *                  scatter kernels' mark, as pcl_step_phase_redirect writes it)
 *   not scattered: first == 0:  the particle is not written at all -- a mark an earlier scatterer of the pass left in dv survives
 *                  first == 1:  dv = 0 for every photon that is not scattered, exposed or not, at rest or not -- the scatter
 *                  kernels' contract for the first scatterer of a pass: dv != 0 then reads "scattered in this pass"
 * So a pcl_step_phase_redirect or pcl_step_phase_layered call behind this one turns its hits about v - dv, the direction before the
 * scatter, and pcl_step_absorb_scattered gives them a single-scattering albedo; a photon two scatterers of a pass both hit has
 * scattered twice, and a phase call turns it about the direction after the first.  A hit whose new velocity equals the old one bit
 * for bit reads as a miss, as with the scatter kernels.  The Philox4x32-10 blocks have the key (seed_lo, seed_hi), u53 of
 * pcl_store_apply_source; ``pass`` is the caller's own counter.  The words 23 and 24 are used by nothing else (scatter kernels 0 and
 * 1, fill and source 2..5, pcl_step_surface_reflect and pcl_step_ground_spectral 8 and 9, pcl_step_phase_redirect 10 and 11,
 * pcl_step_absorb_scattered 12, pcl_step_phase_layered 13, pcl_step_recycle_spent 14, 15 and 16, pcl_step_absorb_path 17,
 * pcl_step_reemit_parked 18, 19 and 20, pcl_step_refract_surface 21, pcl_step_ground_spectral 22: 0-5 and 8-22 are taken), so every
 * other step draws what it drew, and a photon scatters the same way however the run is sharded.
 * p_host, edges_host, E_edges_host, center_host: as for pcl_step_absorb_path, with PCL_SCATTER_LAYERED_MAX_LAYERS, _BANDS and _CELLS
 * equal to its limits for the same budget: a workgroup's uint32 cells (16 KiB), the probabilities (32 KiB) and the two edge tables
 * stay below 64 KiB of LDS.  first: 0 or 1.  ``c`` = the speed of light in code units.
 * counts_out_host[0] = photons exposed, [1] = scattered, by this call;  cells_out_host[b * B' + e] = scattered in layer b and band e.
 * A store that is not uniform costs the host traffic it costs pcl_step_surface_reflect; the ids go along only if some p > 0.
 * PCL_ERR_ARG (everything pcl_step_absorb_path refuses, a first that is neither 0 nor 1, a c that is not finite) is returned before
 * the store is looked at -- by the group's entry point before the group is --, and nothing is launched or written; PCL_ERR_STATE
 * without a store; an empty store answers zeros without a launch.  Host pointers; one device allocation per call, handed back on
 * every way out; synchronises once, with the copy of the tallies.  pcl_last_error() is generic, as for pcl_step_surface_reflect,
 * whose source file these two entry points share (physicl_amd/csrc/pcl_surface.hip). */
#define PCL_SCATTER_LAYERED_MAX_LAYERS 64
#define PCL_SCATTER_LAYERED_MAX_BANDS 1024
#define PCL_SCATTER_LAYERED_MAX_CELLS 4096 /* L' * B' */
int pcl_step_scatter_layered(pcl_ctx *ctx, int n_layers, int n_E_bins, const double *p_host, const double *edges_host,
                             const double *center_host, const double *E_edges_host, int first, double c, uint64_t seed, uint32_t pass,
                             int64_t *counts_out_host /* [2]: exposed, scattered */, int64_t *cells_out_host /* [L' * B'] */);

/* Scattering on a grid of cells (GridScatterStep): who scatters, with a scattering coefficient given per cell of a grid over one to
 * three of x, y, z and the distance from a centre, and per band of the photon's energy -- a cloud of finite width, a broken cloud
 * field, a plume or a fog bank over half of the scene.  pcl_step_scatter_layered with pcl_step_position_grid's cells in place of the
 * radial layers: called where that sweep is called, it scatters in ONE sweep of the resident store, the host makes
 * p = -expm1(-k * (c*dt)) and the device only ever sees p.  Nothing is removed; r, dr, E, ids and kinds are never written.  All
 * arithmetic is fp64, unfused, every operation rounded once, in the order written; an fp32 store's values are widened first (exact)
 * and what is written is rounded once to the store's dtype.  B' = max(n_E_bins, 1), G = the product of n_bins_host.
 *   a particle that is not a photon (kind 0) is skipped and never written.
 *   at rest   iff  v0 == 0 and v1 == 0 and v2 == 0            (-0.0 counts as 0; a NaN in v: moving), as pcl_step_scatter_layered
 *   cell g:        pcl_step_position_grid's lines, character for character -- per axis the bin with e_b <= x < e_(b+1), the last one
 *                  closed;  a PCL_GRID_RADIUS axis bins q = ((x-cx)*(x-cx) + (y-cy)*(y-cy)) + (z-cz)*(z-cz) against the squared
 *                  edges, no square root is taken;  a NaN, a position outside any axis's range: in no cell, skipped;  cells are
 *                  row-major in the order of the axes.  Only the rows of r some axis needs are read.
 *   band e:        n_E_bins == 0: e = 0, E is neither read nor asked for;  otherwise e = the bin of E (widened to double) in
 *                  E_edges_host: [E_e, E_(e+1)), the last one closed;  a NaN, a photon outside the edges: skipped
 *   exposed   =    a moving photon with a cell and a band;  p = p_host[g * B' + e]
 *   p == 0:        nothing is drawn.   p > 0:  u = u53(w0, w1) of the counter (id_lo, id_hi, pass, 25);  scattered iff u < p
 *   scattered:     (u_a, u_b) = (u53(w0, w1), u53(w2, w3)) of the counter (id_lo, id_hi, pass, 26);  w = (1, 0, 0);  mu = 1 - 2*u_a;
 *                  the direction, v_k = c * direction_k and dv_k = v_k - v_old_k: pcl_step_scatter_layered's lines, operation for
 *                  operation (frame, polar, turned; the same sin / cos): uniform on the sphere, the scatter kernels' mark
 *   not scattered: first == 0:  the particle is not written at all -- a mark an earlier scatterer of the pass left in dv survives
 *                  first == 1:  dv = 0 for every photon that is not scattered, exposed or not, at rest or not
 * What follows from the mark is what follows from pcl_step_scatter_layered's.  The Philox4x32-10 blocks have the key (seed_lo,
 * seed_hi), u53 of pcl_store_apply_source; ``pass`` is the caller's own counter.  The words 25 and 26 are used by nothing else (scatter
 * kernels 0 and 1, fill and source 2..5, pcl_step_surface_reflect and pcl_step_ground_spectral 8 and 9, pcl_step_phase_redirect 10 and
 * 11, pcl_step_absorb_scattered 12, pcl_step_phase_layered 13, pcl_step_recycle_spent 14, 15 and 16, pcl_step_absorb_path 17,
 * pcl_step_reemit_parked 18, 19 and 20, pcl_step_refract_surface 21, pcl_step_ground_spectral 22, pcl_step_scatter_layered 23 and 24,
 * this call 25 and 26: 0-5 and 8-26 are taken), so every other step draws what it drew, and a photon scatters the same way however
 * the run is sharded.
 * n_axes, coords_host, n_bins_host, edges_host, center_host: as for pcl_step_position_grid (1..PCL_GRID_MAX_AXES distinct axes,
 * 1..PCL_GRID_MAX_BINS bins each).  n_E_bins: 0..PCL_SCATTER_GRID_MAX_BANDS; E_edges_host: n_E_bins + 1 finite, strictly increasing
 * edges (NULL with 0).  p_host: G * B' values, every one finite and in [0, 1]; G * B' <= PCL_SCATTER_GRID_MAX_CELLS.  first: 0 or 1.
 * ``c`` = the speed of light in code units.
 * counts_out_host[0] = photons exposed, [1] = scattered, by this call;  cells_out_host[g * B' + e] = scattered in cell g and band e.
 * The edges are always staged in LDS (at most 4 x 1025 doubles).  Up to 4096 cells, and while edges, probabilities (8 B a cell) and a
 * workgroup's uint32 tallies (4 B a cell) stay within 64 KiB, the probabilities and tallies are in LDS too; above that the kernel
 * reads p from device memory and adds its hits to the device tallies with 64-bit atomics, one add per wave and cell where the hit
 * lanes of a wave share a cell.  Cost: the table goes up over the host link once per call and the tallies come back -- at 2^20 cells
 * 8 MB up and 8 MB down per call, whatever the store holds; nothing is cached between calls.  A store that is not uniform costs the
 * host traffic it costs pcl_step_surface_reflect; the ids go along only if some p > 0.
 * PCL_ERR_ARG (everything pcl_step_position_grid refuses of the geometry, everything pcl_step_scatter_layered refuses of p, E_edges,
 * first and c, too many cells, a NULL output) is returned before the store is looked at -- by the group's entry point before the
 * group is --, and nothing is launched or written; PCL_ERR_STATE without a store; an empty store answers zeros without a launch.
 * Host pointers; one device allocation per call, handed back on every way out; synchronises once, with the copy of the tallies.
 * pcl_last_error() is generic, as for pcl_step_surface_reflect, whose source file these two entry points share. */
#define PCL_SCATTER_GRID_MAX_BANDS 1024
#define PCL_SCATTER_GRID_MAX_CELLS (1 << 20) /* G * B': PCL_GRID_MAX_CELLS */
int pcl_step_scatter_grid(pcl_ctx *ctx, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                          const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host, int first, double c,
                          uint64_t seed, uint32_t pass, int64_t *counts_out_host /* [2]: exposed, scattered */,
                          int64_t *cells_out_host /* [G * B'] */);

/* Box walls (BoxBoundaryStep): the sides of the scene.  Per axis x, y, z the box [lo, hi] has a wall of one kind or none: a
 * PERIODIC wall hands a photon that has left through one side back in through the other (the horizontal boundary condition of a
 * cloud field), a MIRROR wall folds its whole move back at the wall, an OPEN wall ends its life: it is parked at rest as
 * pcl_step_absorb_path parks, for pcl_step_recycle_spent (at_rest) to hand its slot back to a source.  Called last in a pass, behind a
 * ground or an interface.  ONE deterministic sweep of the resident store: nothing is drawn, no id is read, nothing is removed; E, ids
 * and kinds are never written and E and ids never read.  All arithmetic is fp64, unfused, every operation rounded once, in the order
 * written; an fp32 store's values are widened first (exact) and what is written is rounded once to the store's dtype (a negation is
 * exact).  The operations are add, subtract, multiply, divide, floor, min, max and compares, so numpy restates every bit; min and max
 * are C's fmin and fmax (of a NaN and a number: the number).  L_a = hi_a - lo_a, made once on the host.
 *   a particle that is not a photon (kind 0) is skipped and never written.
 *   moving    iff  not (v0 == 0 and v1 == 0 and v2 == 0)         (-0.0 counts as 0; a NaN in v: moving), the siblings' test;
 *                  a photon at rest is not read further and not written.  moving is counted in counts_out_host[0].
 *   per axis a with a wall, x = r_a:   x not finite (NaN, +-inf): the axis is skipped.   below = x < lo.
 *                  above = x >= hi (PCL_WALL_PERIODIC: the box is [lo, hi)),  above = x > hi (PCL_WALL_MIRROR, PCL_WALL_OPEN: on the
 *                  wall is inside).   outside on a = below or above;  side = 0 if below, 1 if above.
 *   open first:    outside on some PCL_WALL_OPEN axis:  v_k = 0 and dv_k = 0 for k = 0, 1, 2;  r and dr are left alone;
 *                  crossed[a][side] += 1 for the FIRST such axis a in the order x, y, z, and for no other axis, whatever its kind;
 *                  nothing else is done to the photon and it is not counted in multi.  It is at rest: no later call counts it.
 *   otherwise, per PCL_WALL_PERIODIC or PCL_WALL_MIRROR axis a the photon is outside on, each by itself:
 *                  s = x - lo;   n = floor(s / L);   f = min(max(s - n*L, 0), L);   crossed[a][side] += 1, whatever n is
 *     periodic:    y = lo + f;   if not (y < hi): y = lo;   r_a = y.   dr, v and dv are not touched: r - dr is the image of where
 *                  the photon came from.  y is in [lo, hi).
 *     mirror:      h = n * 0.5;   odd = floor(h) != h;   y = odd ? hi - f : lo + f;   y = min(max(y, lo), hi);   r_a = y;
 *                  if odd:  v_a = -v_a,  dv_a = -dv_a,  dr_a = -dr_a.   The image of the whole move under the reflections, exact for
 *                  any number of bounces; |v| does not change.  y is in [lo, hi].
 *   multi:         a photon that is not parked with n < -1 or n > 1 on some axis it is outside on is counted once in
 *                  counts_out_host[1]: c*dt is too large for the box (pcl_step_refract_surface's overshot).  It changes nothing.
 *   a photon that is outside on no axis is not written at all.
 * modes_host: three of PCL_WALL_NONE, PCL_WALL_PERIODIC, PCL_WALL_MIRROR, PCL_WALL_OPEN, for x, y, z; lo_host, hi_host: three
 * doubles each, read for the axes with a wall only.  counts_out_host: moving, multi, crossed[3][2] (axis-major: [2 + 2*a + side]), by
 * this call.  Rows the call asks the store for (pcl_store_field_ptr, which is the whole store protocol): the three v rows; the r row
 * of every axis with a wall; dr of a mirror axis; dv of a mirror axis, and all three dv rows if some axis is open.  With three
 * periodic walls and nobody outside the sweep reads 48 B a slot in fp64.  A store that is not uniform costs the kinds' host traffic,
 * as for pcl_step_surface_reflect; ids never travel.
 * The call takes no seed, no pass and no c: it draws nothing, so the Philox counter words stay as they are (0-5 and 8-26 are taken,
 * see pcl_step_scatter_grid).
 * PCL_ERR_ARG (a NULL pointer, an unknown mode, all three modes PCL_WALL_NONE, and on an axis with a wall: lo, hi or hi - lo not
 * finite, or hi - lo <= 0) is returned before the store is looked at -- by the group's entry point before the group is --, and nothing
 * is launched or written; PCL_ERR_STATE without a store; an empty store answers zeros without a launch.  Host pointers; one device
 * allocation per call, handed back on every way out; synchronises once, with the copy of the counts.  pcl_last_error() is generic,
 * as for pcl_step_surface_reflect, whose source file these two entry points share. */
#define PCL_WALL_NONE 0
#define PCL_WALL_PERIODIC 1
#define PCL_WALL_MIRROR 2
#define PCL_WALL_OPEN 3
int pcl_step_box_walls(pcl_ctx *ctx, const int *modes_host /* [3] */, const double *lo_host /* [3] */, const double *hi_host /* [3] */,
                       int64_t *counts_out_host /* [8]: moving, multi, crossed[3][2] */);

/* Phase functions by grid cell (GridPhaseStep): pcl_step_phase_layered with pcl_step_position_grid's cells in place of the radial
 * layers -- droplets' forward peak in the cloudy cells of a broken cloud field, Rayleigh in the clear air between and around them.
 * Called where pcl_step_phase_layered would be called (directly behind the scatter step of a pass, before or behind
 * pcl_step_absorb_scattered), it re-directs the photons that step scattered in ONE sweep of the resident store.  The n_laws = M laws
 * are mixed in n_mixtures = K rows of cumulative weights, the MIXTURES; every cell of the grid names one of them, or none.  A pass
 * holds ONE phase step: this entry point shares the blocks 10, 11 and 13 with pcl_step_phase_redirect and pcl_step_phase_layered and
 * must not be called in a pass in which one of the three has already been called with the same ``pass``.  Nothing is removed; r, dr,
 * E, ids and kinds are not written, E is not asked for and of r only the rows some axis needs.  All arithmetic is fp64, unfused, every
 * operation rounded once, in the order written; an fp32 store's values are widened first (exact) and what is written is rounded once
 * to the store's dtype.  G = the product of n_bins_host.
 *   scattered  iff  the particle is a photon, (dv0 != 0 or dv1 != 0 or dv2 != 0), and o = v - dv has 0 < o.o < inf, o.o = (o0*o0 +
 *                   o1*o1) + o2*o2                                                    (pcl_step_phase_layered's "scattered")
 *   cell g:         pcl_step_position_grid's lines, character for character -- per axis the bin with e_b <= x < e_(b+1), the last one
 *                   closed;  a PCL_GRID_RADIUS axis bins q = ((x-cx)*(x-cx) + (y-cy)*(y-cy)) + (z-cz)*(z-cz) against the squared
 *                   edges, no square root is taken;  a NaN, a position outside any axis's range: in no cell;  cells are row-major in
 *                   the order of the axes.  Only the rows of r some axis needs are read, and only of scattered photons.
 *   mixture m:      in a cell:  mixture_host[g], a row of cum_host, or PCL_PHASE_GRID_ALONE: none.   in no cell:  ``outside``, a row of
 *                   cum_host, or -1: none.
 *   m = none:       counted as scattered, not written: the photon keeps the direction the scatter step gave it
 *   otherwise:      re-directed.  The law: M == 1: j = 0;  otherwise j = the first law with u_s < cum_host[m*M + j], u_s = u53(w0, w1)
 *                   of the block (id_lo, id_hi, pass, 13).  (Whether that block is computed for a row that is one-hot is the
 *                   kernel's business: the first positive entry of such a row is 1 and 0 <= u_s < 1.)
 *   block A (id_lo, id_hi, pass, 10): u_a = u53(w0, w1), u_b = u53(w2, w3);  mu by the law's kind:
 *     PCL_PHASE_ISOTROPIC:  mu = 1 - 2*u_a
 *     PCL_PHASE_HG with g = g_host[j]:  g == 0: the isotropic line.   |g| >= 1/2:  gg = g*g;  g2 = 2*g;
 *       q = (1 - gg) / ((1 - g) + g2*u_a);  mu = ((1 + gg) - q*q) / g2.   0 < |g| < 1/2:  s = 1 - 2*u_a;  gs = g*s;  d = 1 - gs;
 *       s2 = s*s;  p = (0.5*(s2 + 3) - gs) + gg*(0.5*(s2 - 1));  mu = (g*p - s) / (d*d).   Both:  mu = min(max(mu, -1), 1)
 *     PCL_PHASE_RAYLEIGH:  s4 = u_a*4;  jq = floor(s4);  gq = 2*(s4 - jq) - 1;  jq != 3: mu = gq;  jq == 3: block B (id_lo, id_hi,
 *       pass, 11): mu = copysign(max(max(|gq|, u53(w0, w1)), u53(w2, w3)), gq)
 *     PCL_PHASE_TABLE:  k = the bin of u_a in F ([F_k, F_(k+1)), always inside);  s_k = (mu_(k+1) - mu_k) / (F_(k+1) - F_k), made by the
 *       library on the host;  mu = min(max(mu_k + (u_a - F_k)*s_k, mu_k), mu_(k+1))
 *     -- pcl_step_phase_redirect's and pcl_step_phase_layered's lines, bit for bit
 *   then  on = sqrt(o.o);  w = o / on;  s = sqrt((1 - mu)*(1 + mu));  psi = (u_b*2)*pi;  sc = s*cos psi;  ss = s*sin psi;  e1, e2 = the
 *   frame of Duff et al. about w (pcl_step_surface_reflect writes it out);  dir = (sc*e1 + ss*e2) + mu*w;  v = c*dir;  dv = v - o.
 * So two calls are bit for bit, store and tallies, what an older entry point leaves:  one PCL_GRID_RADIUS axis with the edges e,
 * mixture_host[b] = b and outside = -1 is pcl_step_phase_layered with n_layers = L, cum_host and edges_host = e;  one cell, one law and
 * outside = 0 is pcl_step_phase_redirect with that law.  No new counter word is taken: the words in use are the scatter kernels' 0 and
 * 1, fill and source 2..5, pcl_step_surface_reflect and pcl_step_ground_spectral 8 and 9, pcl_step_phase_redirect 10 and 11,
 * pcl_step_absorb_scattered 12, pcl_step_phase_layered 10, 11 and 13, pcl_step_phase_grid (this call) 10, 11 and 13,
 * pcl_step_recycle_spent 14, 15 and 16, pcl_step_absorb_path 17, pcl_step_reemit_parked 18, 19 and 20, pcl_step_refract_surface 21,
 * pcl_step_ground_spectral 22, pcl_step_scatter_layered 23 and 24, pcl_step_scatter_grid 25 and 26: 0-5 and 8-26 are taken.
 * n_laws, kinds_host, g_host, law_bins_host (pcl_step_phase_layered's n_bins_host), mu_host, F_host: as for pcl_step_phase_layered.
 * cum_host: K rows of M cumulative weights, 1 <= K <= PCL_PHASE_GRID_MAX_MIXTURES, each row as pcl_step_phase_layered's.  n_axes,
 * coords_host, n_bins_host, edges_host, center_host: as for pcl_step_position_grid, G <= PCL_PHASE_GRID_MAX_CELLS.  mixture_host: G
 * bytes, row-major in the order of the axes, each below K or PCL_PHASE_GRID_ALONE.  outside: -1 .. K - 1.  ``c``: the speed of light
 * in code units.
 * The mixture map goes up with every call (G bytes, at most 1 MiB) and stays in device memory: a scattered photon reads one byte of
 * it.  Everything else sits in LDS, and with E = the sum of n_bins_host[a] + 1 over the axes and T = the nodes of all tables (the sum
 * of law_bins_host[j] + 1 over the PCL_PHASE_TABLE laws) a call is accepted only if
 *     8 * (K*M + E + M + 3*T + (3*M + 1)/2)  +  4 * (2 + K + M)  <=  PCL_PHASE_GRID_LDS_BYTES           ((3*M + 1)/2 rounded down)
 * -- the 64 KiB a launch may ask for.  The largest law tables (T = 2056: 49 344 B) and the largest edge tables (E = 2052: 16 416 B)
 * together do not fit; either fits with a small other.  A call is sized by what it uses.
 * counts_out_host[0] = photons scattered, [1] = re-directed, [2 + m] = re-directed by mixture m, [2 + K + j] = re-directed by law j.
 * A store that is not uniform costs the host traffic it costs pcl_step_surface_reflect.
 * PCL_ERR_ARG (everything pcl_step_phase_layered refuses of the laws, the rows of weights, the centre and c, everything
 * pcl_step_position_grid refuses of the geometry, K or outside beyond their limits, a byte of the map that is neither a row nor
 * PCL_PHASE_GRID_ALONE, tables beyond the LDS bound, a NULL kinds, cum, coords, n_bins, edges, mixture or counts pointer) is
 * returned before the store is looked at -- by the group's entry point before the group is --, and nothing is launched or written;
 * PCL_ERR_STATE without a store; an empty store answers zeros without a launch.  Host pointers; one device allocation per call,
 * handed back on every way out; synchronises once, with the copy of the tallies.  pcl_last_error() is generic, as for
 * pcl_step_surface_reflect, whose source file these two entry points share. */
#define PCL_PHASE_GRID_MAX_MIXTURES 64
#define PCL_PHASE_GRID_MAX_CELLS (1 << 20) /* G: PCL_GRID_MAX_CELLS */
#define PCL_PHASE_GRID_ALONE 255           /* a byte of mixture_host: a scattered photon in this cell is left alone */
#define PCL_PHASE_GRID_LDS_BYTES 65536
int pcl_step_phase_grid(pcl_ctx *ctx, int n_laws, const int *kinds_host, const double *g_host, const int *law_bins_host,
                        const double *mu_host, const double *F_host, int n_mixtures, const double *cum_host, int n_axes,
                        const int *coords_host, const int *n_bins_host, const double *edges_host, const double *center_host,
                        const unsigned char *mixture_host /* [G] */, int outside, double c, uint64_t seed, uint32_t pass,
                        int64_t *counts_out_host /* [2 + K + M] */);

/* Absorption on a grid of cells (GridAbsorptionStep): both kinds of absorption -- along the path (pcl_step_absorb_path's) and at an
 * interaction (pcl_step_absorb_scattered's) -- per cell of pcl_step_position_grid's grid and per band of the photon's energy, in ONE
 * sweep of the resident store, and the tally of what was absorbed per cell: the heating field of a smoke plume, a water-vapour column
 * of finite width, the droplets of a broken cloud field.  Called where those two sweeps are called: behind the scatter and phase steps
 * of a pass, in front of the ground.  Either table may be left out (NULL), not both.  The host makes p = -expm1(-k * (c*dt)) and the
 * device only ever sees p.  Nothing is removed; r, dr, E, ids and kinds are never written.  The rule holds compares and stores only --
 * no transcendental function, no division, no square root; q of a radius axis is fp64, unfused, every operation rounded once, in the
 * order written, an fp32 store's values widened first (exact) -- so numpy restates every bit.  B' = max(n_E_bins, 1), G = the
 * product of n_bins_host.
 *   a particle that is not a photon (kind 0) is skipped and never written.
 *   at rest    iff  v0 == 0 and v1 == 0 and v2 == 0           (-0.0 counts as 0; a NaN in v: moving), as pcl_step_scatter_grid;
 *                   a photon at rest is skipped.
 *   cell g, band e: pcl_step_scatter_grid's lines exactly -- per axis the bin with e_b <= x < e_(b+1), the last one closed;  a
 *                   PCL_GRID_RADIUS axis bins q = ((x-cx)*(x-cx) + (y-cy)*(y-cy)) + (z-cz)*(z-cz) against the squared edges;  cells are
 *                   row-major in the order of the axes;  n_E_bins == 0: e = 0, E is neither read nor asked for;  otherwise e = the bin
 *                   of E in E_edges_host;  a NaN, a position outside any axis's range and an energy outside the bands are in no cell.
 *                   Only the rows of r some axis needs are read.
 *   exposed    =    a moving photon with a cell and a band;  c = g * B' + e
 *   interacted =    exposed and (dv0 != 0 or dv1 != 0 or dv2 != 0), the scatter kernels' mark (a NaN in dv: interacted).  Evaluated
 *                   only with omega0_host: without it dv is not read and the count is 0.
 *   along the path  (p_host given and p_host[c] > 0; p == 0 draws nothing):  u = u53(w0, w1) of the counter (id_lo, id_hi, pass, 27);
 *                   absorbed iff u < p_host[c]
 *   at the interaction  (not absorbed along the path, omega0_host given, interacted, and omega0_host[c] < 1; a conservative cell
 *                   draws nothing):  u = u53(w0, w1) of the counter (id_lo, id_hi, pass, 28);  absorbed iff not (u < omega0_host[c]),
 *                   pcl_step_absorb_scattered's sense of the draw
 *   absorbed:       parked as those two sweeps park:  v_k = 0 and dv_k = 0 for k = 0, 1, 2;  cells_out_host[c] += 1, whichever kind
 *   not absorbed:   the particle is not written at all.
 * The Philox4x32-10 blocks have the key (seed_lo, seed_hi), u53 of pcl_store_apply_source; ``pass`` is the caller's own counter.  The
 * words 27 and 28 are used by nothing else: with this call's 27 and 28 the taken words are 0-5 and 8-28 (pcl_step_phase_grid lists the
 * users of the others), so every other step draws what it drew, and a photon meets the same fate however the run is sharded.
 * n_axes, coords_host, n_bins_host, edges_host, center_host, n_E_bins, E_edges_host: as for pcl_step_scatter_grid, n_E_bins at most
 * PCL_ABSORB_GRID_MAX_BANDS.  p_host, omega0_host: NULL, or G * B' values, every one in [0, 1] (not NaN);
 * G * B' <= PCL_ABSORB_GRID_MAX_CELLS.
 * counts_out_host[0] = photons exposed, [1] = interacted, [2] = absorbed along the path, [3] = absorbed at the interaction, by this
 * call;  cells_out_host[g * B' + e] = absorbed in cell g and band e, both kinds together.
 * The edges are always staged in LDS.  With E = every edge of the axes and of E_edges_host, C = G * B' and t = the tables given (1 or
 * 2), the tables and a workgroup's uint32 tallies are in LDS too while
 *     C <= PCL_ABSORB_GRID_LDS_CELLS   and   8 * E  +  8 * t * C  +  4 * (4 + C)  <=  PCL_ABSORB_GRID_LDS_BYTES
 * -- a 16 x 16 x 16 grid with one table, not with two; above that the kernel reads the tables from device memory and adds what it
 * absorbed to the device tallies with 64-bit atomics, one add per wave and cell where the absorbed lanes of a wave share a cell.
 * Cost: the tables go up over the host link once per call and the tallies come back, as for pcl_step_scatter_grid; nothing is cached
 * between calls.  A store that is not uniform costs the host traffic it costs pcl_step_surface_reflect; the ids go along only if some
 * p > 0 or some omega0 < 1.
 * PCL_ERR_ARG (everything pcl_step_scatter_grid refuses of the geometry and of E_edges, both tables NULL, a table value outside
 * [0, 1] or NaN, too many cells, a NULL output) is returned before the store is looked at -- by the group's entry point before the
 * group is --, and nothing is launched or written; PCL_ERR_STATE without a store; an empty store answers zeros without a launch.
 * Host pointers; one device allocation per call, handed back on every way out; synchronises once, with the copy of the tallies.
 * pcl_last_error() is generic, as for pcl_step_surface_reflect, whose source file these two entry points share. */
#define PCL_ABSORB_GRID_MAX_BANDS 1024
#define PCL_ABSORB_GRID_MAX_CELLS (1 << 20) /* G * B': PCL_GRID_MAX_CELLS */
#define PCL_ABSORB_GRID_LDS_CELLS 4096
#define PCL_ABSORB_GRID_LDS_BYTES 65536
int pcl_step_absorb_grid(pcl_ctx *ctx, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                         const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host /* or NULL */,
                         const double *omega0_host /* or NULL */, uint64_t seed, uint32_t pass,
                         int64_t *counts_out_host /* [4]: exposed, interacted, absorbed along the path, at the interaction */,
                         int64_t *cells_out_host /* [G * B'] */);

/* The irradiance field: up and down fluxes through the planes normal to one axis, as maps (PlaneFluxMapStep).  ``axis`` a = 0, 1, 2
 * (x, y, z) is the normal; the transverse axes (u, v) are the remaining two in x, y, z order: 0 gives (y, z), 1 gives (x, z), 2 gives
 * (x, y).  In ONE read-only sweep of the resident store every particle whose last move changed its side of a level is counted, by
 * level and direction, and sorted by where its straight move met the plane into n_u x n_v columns and -- with bands -- by energy, as
 * int64 cells that add across devices and ranks like every other counter row.  Called where pcl_step_shell_crossings of the ground's
 * radius is called: in front of the sweeps that rewrite r and dr of the move (the ground, the refracting interface, the walls).
 * All arithmetic is fp64, every operation rounded once, unfused, in the order written; an fp32 store's values are widened first
 * (exact).  No division and no square root is taken anywhere, so numpy restates every cell exactly.  Per slot, plain Objects included,
 * S = n_levels, B' = max(n_E_bins, 1):
 *   now = r_a;  m = dr_a;  prev = now - m;
 *   for each level X:   up  iff  prev < X and now >= X;   down  iff  prev >= X and now < X
 *                       -- on the plane is above; a NaN crosses nothing.  Every change of side is counted exactly once, so
 *                       cumsum(up - down) per level is the change of the population at or above it.  As for the shells, only the end
 *                       points of the move are looked at.
 *   counts_out_host[0][s] += 1 for up, counts_out_host[1][s] += 1 for down: every particle that crossed, photon or not.
 *   for each level the particle crossed (a move may cross several: it is tallied at each of them, with that level's G):
 *     G = |X - prev|;  D = |m|;
 *     for t in (u, v):  p_t = r_t - dr_t;  H_t = p_t*D + dr_t*G     (the crossing point times D)
 *     bin b of t  iff  e_b*D <= H_t < e_(b+1)*D, the last bin closed.  Rounded products are monotone in b: a binary search with one
 *     multiply per probe.
 *     in no cell  iff  D or an H_t is not finite, or H_t lies outside [e_0*D, e_n*D] on either axis.
 *   Without bands (n_E_bins == 0, E_edges_host is not looked at, E is neither read nor asked for) the band is 0.  With bands only a
 *   PHOTON (plain Objects carry no energy) with E_0 <= E <= E_nE has a band, as numpy.histogram(E, bins=E_edges) finds it; a plain
 *   Object, an energy outside the bands or NaN is counted and lands in no cell.
 *   maps_out_host[dir][s][band][iu][iv] += 1, dir 0 = up, 1 = down; C order.
 * levels_host: n_levels in 1..PCL_PLANE_FLUX_MAX_LEVELS finite, strictly increasing doubles.  u_edges_host / v_edges_host /
 * E_edges_host: n + 1 finite, strictly increasing doubles; n_u, n_v in 1..PCL_PLANE_FLUX_MAX_BINS, n_E_bins in
 * 0..PCL_PLANE_FLUX_MAX_BANDS, C = 2 * S * B' * n_u * n_v at most PCL_PLANE_FLUX_MAX_CELLS.
 * The levels and the three edge tables are always staged in LDS, and so are a workgroup's 2 S uint32 counts.  A workgroup's maps are
 * uint32 cells in LDS too, flushed once at the end, while
 *     C <= PCL_PLANE_FLUX_LDS_CELLS   and   8 * (S + n_u + 1 + n_v + 1 + (B ? B + 1 : 0))  +  4 * (2 S + C)  <=  PCL_PLANE_FLUX_LDS_BYTES
 * (B = n_E_bins); above that the crossing lanes add to the device block with 64-bit atomics.  PCL_PLANE_FLUX_LDS_CELLS is the
 * switch-over of pcl_step_scatter_grid and pcl_step_absorb_grid; it was not tuned for this sweep.  Per slot r_a and dr_a are read
 * first; only a lane that crossed reads r and dr of the transverse axes, and E with bands.
 * PCL_ERR_ARG (a NULL pointer, an axis outside 0..2, levels or edges that are not finite or not strictly increasing, a level, bin,
 * band or cell count outside its limits) is returned before the store is looked at -- by the group's entry point before the group is
 * --, with the outputs untouched; PCL_ERR_STATE without a store; an empty store answers zeros without a launch.  Host pointers; one
 * device allocation per call, handed back on every way out; synchronises once, with the one copy of the results.  The store is seen
 * dense with dr real (pcl_store_field_ptr); E is looked at only with bands, at pcl_step_detector_image's price.  pcl_last_error() is
 * generic, as for pcl_step_shell_crossings, whose source file these two entry points share. */
#define PCL_PLANE_FLUX_MAX_LEVELS 16
#define PCL_PLANE_FLUX_MAX_BINS 1024       /* per transverse axis */
#define PCL_PLANE_FLUX_MAX_BANDS 1024
#define PCL_PLANE_FLUX_MAX_CELLS (1 << 20) /* 2 * S * B' * n_u * n_v */
#define PCL_PLANE_FLUX_LDS_CELLS 4096
#define PCL_PLANE_FLUX_LDS_BYTES 65536
int pcl_step_plane_flux(pcl_ctx *ctx, int axis, int n_levels, const double *levels_host, const double *u_edges_host, int n_u,
                        const double *v_edges_host, int n_v, const double *E_edges_host, int n_E_bins /* NULL, 0: no bands */,
                        int64_t *counts_out_host /* [2][S]: up, down */,
                        int64_t *maps_out_host /* [2][S][B'][n_u][n_v] */);

/* ---- Device groups: several GPUs from ONE process ---------------------------------------------------------------
 * The reference is a single process with one simulation thread (physicl/__init__.py:400-432, 501-524); this is how
 * a host written against this ABI uses a node's GPUs the same way, without one process per GPU.  A group owns one
 * context (device, stream, store) and one worker thread per entry of device_ids (an id may repeat: two contexts on one
 * GPU).  Particles are sharded by GLOBAL index in contiguous blocks -- shard g of G owns [g*N/G, (g+1)*N/G) -- and ids
 * are global, so the id-keyed device RNG gives exactly the rows and the per-photon histories of a one-device run.  A
 * group step hands the call to every shard's worker, waits for all of them, and returns the SUM of the int64 counter
 * rows (same layout as the per-context call): the rows are in host memory when a launch returns, so this sum is the
 * group's collective (the counters are the only global quantities of the path).  Windows of the
 * particle order are read shard after shard (contiguous blocks + stable compaction = global particle order).
 * pcl_group_ctx gives the i-th context for anything per shard (uploads, pcl_store_*).  One group call at a time.
 * A tracked subset (pcl_store_trace_ahead) over a group: hand every shard's context the whole id list before the group's
 * K-pass launch -- a shard answers NaN rows for the ids it does not hold, a particle lives in exactly one shard, so the row
 * that is not NaN is the particle's (what physicl_amd.multidev.MultiDevice.trace_ahead does).
 * Errors: the first failing shard's code; pcl_last_error() names the shard.                                      */
typedef struct pcl_group pcl_group;
int pcl_group_create(int n_dev, const int *device_ids, pcl_group **group_out);
int pcl_group_destroy(pcl_group *group);
int pcl_group_size(pcl_group *group, int *n_out);
int pcl_group_ctx(pcl_group *group, int i, pcl_ctx **ctx_out);
int pcl_group_shard(pcl_group *group, int64_t n_global, int i, int64_t *lo_out, int64_t *hi_out);
int pcl_group_store_alloc(pcl_group *group, int64_t capacity_global, int dtype);
int pcl_group_store_dtype(pcl_group *group, int *dtype_out);      /* PCL_DTYPE_F64 / PCL_DTYPE_F32 of the shards' stores */
int pcl_group_fill_photons(pcl_group *group, int64_t n_global, int64_t id_base, double c, double e_min, double e_max,
                           uint64_t seed);
int pcl_group_count(pcl_group *group, int64_t *count_out);
int pcl_group_sync(pcl_group *group);
int pcl_group_reserve_compaction(pcl_group *group);
/* the steps: arguments and out_host layout of pcl_step_fused (synchronous form: out_host and n_planes >= 0 required),
 * pcl_step_fused_delete, pcl_step_fused_multi, pcl_step_fused_delete_multi, pcl_step_mixed_multi; counters summed     */
int pcl_group_step_fused(pcl_group *group, double dt, int do_scatter, double A, double n, int flags, double c, double h,
                         const char *n_expr, int rng_mode, uint64_t seed, uint32_t step, const double *planes_host,
                         int n_planes, int64_t *out_host);
int pcl_group_step_fused_delete(pcl_group *group, double dt, double A, double n, int flags, int rng_mode, uint64_t seed,
                                uint32_t step, const double *planes_host, int n_planes, int64_t *out_host);
int pcl_group_step_fused_multi(pcl_group *group, double dt, int k_steps, double A, double n, int flags, double c, double h,
                               const char *n_expr, uint64_t seed, uint32_t step0, const double *planes_host, int n_planes,
                               int64_t *out_host);
int pcl_group_step_fused_delete_multi(pcl_group *group, double dt, int k_steps, double A, double n, uint64_t seed,
                                      uint32_t step0, const double *planes_host, int n_planes, int64_t *out_host);
int pcl_group_step_mixed_multi(pcl_group *group, double dt, int k_passes, int n_phases, const int *phase_kinds_host, double A,
                               double n, int flags, double c, double h, const char *n_expr, double A_del, double n_del,
                               uint64_t seed, uint32_t step0, const double *planes_host, int n_planes, int64_t *out_host);
/* elements [offset, offset + n) of a field / of the ids in GLOBAL particle order (host pointers, store dtype / int64) */
int pcl_group_download(pcl_group *group, int field, void *host, int64_t offset, int64_t n);
int pcl_group_download_ids(pcl_group *group, int64_t *host, int64_t offset, int64_t n);
/* pcl_step_plane_spectra on every shard (side by side), counts and histograms summed over the group's devices */
int pcl_group_step_plane_spectra(pcl_group *group, const double *planes_host, int n_planes, const double *edges_host, int n_bins,
                                 int64_t *counts_out_host, int64_t *hist_out_host);
/* pcl_store_apply_source on every shard of a group filled with pcl_group_fill_photons (ids are global: the same photons) */
int pcl_group_apply_source(pcl_group *group, const pcl_source *src, double c, uint64_t seed);
/* pcl_step_position_grid on every shard (side by side), the grids summed over the group's devices; the arguments are checked
 * once for the group, before any shard is asked */
int pcl_group_step_position_grid(pcl_group *group, int n_axes, const int *coords_host, const int *n_bins_host,
                                 const double *edges_host, const double *center_host, int64_t *grid_out_host);
/* pcl_step_shell_crossings on every shard (side by side), counts and histograms summed over the group's devices; the
 * arguments are checked once for the group, before any shard is asked */
int pcl_group_step_shell_crossings(pcl_group *group, int n_shells, const double *radii_host, const double *center_host,
                                   const double *E_edges_host, int n_E_bins, const double *mu_edges_host, int n_mu_bins,
                                   int64_t *counts_out_host, int64_t *E_hist_out_host, int64_t *mu_hist_out_host);
/* pcl_step_detector_image on every shard (side by side), the two counts and the image summed over the group's devices; the
 * arguments are checked once for the group, before any shard is asked */
int pcl_group_step_detector_image(pcl_group *group, const double *position_host, const double *frame_host, double radius,
                                  const double *x_edges_host, int nx, const double *y_edges_host, int ny, const double *E_edges_host,
                                  int n_E_bins, int64_t *counts_out_host, int64_t *image_out_host);
/* pcl_step_surface_reflect on every shard (side by side), the two counts summed over the group's devices; the arguments
 * are checked once for the group, before any shard is written */
int pcl_group_step_surface_reflect(pcl_group *group, double radius, const double *center_host, double albedo, int mode, double c,
                                   uint64_t seed, uint32_t pass, int64_t *counts_out_host);
/* pcl_step_phase_redirect on every shard (side by side), the count summed over the group's devices; the arguments are checked
 * once for the group, before any shard is written */
int pcl_group_step_phase_redirect(pcl_group *group, int phase, double g, double c, uint64_t seed, uint32_t pass,
                                  int64_t *count_out_host);
/* pcl_step_absorb_scattered on every shard (side by side), the tallies summed over the group's devices; the arguments are checked
 * once for the group, before any shard is written */
int pcl_group_step_absorb_scattered(pcl_group *group, int n_layers, const double *omega0_host, const double *edges_host,
                                    const double *center_host, int n_E_bins, const double *E_edges_host, uint64_t seed, uint32_t pass,
                                    int64_t *counts_out_host, int64_t *E_hist_out_host);
/* pcl_step_phase_layered on every shard (side by side), the tallies summed over the group's devices; the arguments are checked
 * once for the group, before any shard is written */
int pcl_group_step_phase_layered(pcl_group *group, int n_laws, const int *kinds_host, const double *g_host, const int *n_bins_host,
                                 const double *mu_host, const double *F_host, int n_layers, const double *cum_host,
                                 const double *edges_host, const double *center_host, double c, uint64_t seed, uint32_t pass,
                                 int64_t *counts_out_host);
/* pcl_step_recycle_spent on every shard (side by side), the two counts summed over the group's devices; the arguments are checked
 * once for the group, before any shard is written (ids are global: the same photons are re-emitted the same way) */
int pcl_group_step_recycle_spent(pcl_group *group, const pcl_source *src, double c, int at_rest, double top,
                                 const double *center_host, int n_E, const double *cdf_host, const double *grid_host, uint64_t seed,
                                 uint32_t pass, int64_t *counts_out_host);
/* pcl_step_absorb_path on every shard (side by side), the counts and the cells summed over the group's devices; the arguments are
 * checked once for the group, before any shard is written (ids are global: the same photons are absorbed) */
int pcl_group_step_absorb_path(pcl_group *group, int n_layers, int n_E_bins, const double *p_host, const double *edges_host,
                               const double *center_host, const double *E_edges_host, uint64_t seed, uint32_t pass,
                               int64_t *counts_out_host, int64_t *cells_out_host);
/* pcl_step_reemit_parked on every shard (side by side), the 2 + L' counts summed over the group's devices; the arguments are
 * checked once for the group, before any shard is written (ids are global: the same photons are re-emitted the same way) */
int pcl_group_step_reemit_parked(pcl_group *group, int n_layers, const double *edges_host, const double *center_host,
                                 const double *eta_host, const int *lambertian_host, const int *table_offsets_host,
                                 const double *cdf_host, const double *grid_host, double c, uint64_t seed, uint32_t pass,
                                 int64_t *counts_out_host);
/* pcl_step_refract_surface on every shard (side by side), the six counts summed over the group's devices; the arguments are
 * checked once for the group, before the group is looked at (ids are global: the same photons meet the same fate) */
int pcl_group_step_refract_surface(pcl_group *group, double radius, const double *center_host, double n_inside, double n_outside,
                                   int fresnel, double c, uint64_t seed, uint32_t pass, int64_t *counts_out_host);
/* pcl_step_ground_spectral on every shard (side by side), the four counts and the two rows by band summed over the group's devices;
 * the arguments are checked once for the group, before the group is looked at (ids are global: the same photons meet the same fate) */
int pcl_group_step_ground_spectral(pcl_group *group, double radius, const double *center_host, int n_bands, const double *E_edges_host,
                                   const double *albedo_host, const double *specular_host, double c, uint64_t seed, uint32_t pass,
                                   int64_t *counts_out_host, int64_t *bands_out_host);
/* pcl_step_scatter_layered on every shard (side by side), the counts and the cells summed over the group's devices; the arguments
 * are checked once for the group, before the group is looked at (ids are global: the same photons scatter the same way) */
int pcl_group_step_scatter_layered(pcl_group *group, int n_layers, int n_E_bins, const double *p_host, const double *edges_host,
                                   const double *center_host, const double *E_edges_host, int first, double c, uint64_t seed,
                                   uint32_t pass, int64_t *counts_out_host, int64_t *cells_out_host);
/* pcl_step_scatter_grid on every shard (side by side), the counts and the cells summed over the group's devices; the arguments are
 * checked once for the group, before the group is looked at (ids are global: the same photons scatter the same way).  Every shard
 * stages the table and brings its tallies back: at 2^20 cells 8 MB up and 8 MB down per device */
int pcl_group_step_scatter_grid(pcl_group *group, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                                const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host, int first,
                                double c, uint64_t seed, uint32_t pass, int64_t *counts_out_host, int64_t *cells_out_host);
/* pcl_step_box_walls on every shard (side by side), the eight counts summed over the group's devices; the arguments are checked once
 * for the group, before the group is looked at (the rule reads no id: a photon meets the same wall however the run is sharded) */
int pcl_group_step_box_walls(pcl_group *group, const int *modes_host, const double *lo_host, const double *hi_host,
                             int64_t *counts_out_host);
/* pcl_step_phase_grid on every shard (side by side), the tallies summed over the group's devices; the arguments are checked once for
 * the group, before the group is looked at (ids are global: the same photons are turned the same way).  Every shard stages the map */
int pcl_group_step_phase_grid(pcl_group *group, int n_laws, const int *kinds_host, const double *g_host, const int *law_bins_host,
                              const double *mu_host, const double *F_host, int n_mixtures, const double *cum_host, int n_axes,
                              const int *coords_host, const int *n_bins_host, const double *edges_host, const double *center_host,
                              const unsigned char *mixture_host, int outside, double c, uint64_t seed, uint32_t pass,
                              int64_t *counts_out_host);
/* pcl_step_absorb_grid on every shard (side by side), the four counts and the cells summed over the group's devices; the arguments
 * are checked once for the group, before the group is looked at (ids are global: the same photons meet the same fate).  Every shard
 * stages the tables and brings its tallies back */
int pcl_group_step_absorb_grid(pcl_group *group, int n_axes, const int *coords_host, const int *n_bins_host, const double *edges_host,
                               const double *center_host, int n_E_bins, const double *E_edges_host, const double *p_host,
                               const double *omega0_host, uint64_t seed, uint32_t pass, int64_t *counts_out_host,
                               int64_t *cells_out_host);
/* pcl_step_plane_flux on every shard (side by side), the counts and the maps summed over the group's devices; the arguments are
 * checked once for the group, before the group is looked at.  Every shard brings its maps back: 8 B a cell per shard and call */
int pcl_group_step_plane_flux(pcl_group *group, int axis, int n_levels, const double *levels_host, const double *u_edges_host, int n_u,
                              const double *v_edges_host, int n_v, const double *E_edges_host, int n_E_bins, int64_t *counts_out_host,
                              int64_t *maps_out_host);

/* ---------------------------------------------------------------- the counters' collective (one process per GPU)
 * The path shards by global index with no data-path exchange; the only global quantities are the int64
 * counter rows a step returns (alive, hits / removed, sign counts, plane crossings) -- they are in host memory when the
 * call returns.  A host that runs ONE PROCESS PER GPU sums them over its ranks with RCCL (over xGMI inside a node):
 *   rank 0:      pcl_comm_unique_id(id)      and ships the PCL_COMM_ID_BYTES bytes to the other ranks by whatever it has
 *   every rank:  pcl_comm_create(ctx, id, rank, world, &comm)   -- collective: returns when all ranks have arrived and a
 *                                                                   one-element all-reduce has seen every one of them
 *   per launch:  pcl_comm_allreduce_sum_i64(comm, rows, n)       -- in place, host pointer, on the context's stream
 * librccl is loaded at run time (PCL_RCCL_LIB overrides the search).  There is no fallback: a missing library or a
 * failed bring-up is PCL_ERR_STATE / PCL_ERR_HIP, and the caller must treat it as fatal (physicl_amd/dist.py does).
 * One process on several GPUs needs none of this: pcl_group_* sums on the host.                                       */
#define PCL_COMM_ID_BYTES 128
typedef struct pcl_comm pcl_comm;
int pcl_comm_unique_id(void *id_out_host);                                                      /* PCL_COMM_ID_BYTES bytes */
int pcl_comm_create(pcl_ctx *ctx, const void *id_host, int rank, int world, pcl_comm **comm_out);
int pcl_comm_allreduce_sum_i64(pcl_comm *comm, int64_t *inout_host, int n);                     /* n <= 2048 */
int pcl_comm_info(pcl_comm *comm, int *rank_out, int *world_out, int *rccl_version_out, int64_t *reduces_out);
int pcl_comm_destroy(pcl_comm *comm);

#ifdef __cplusplus
}
#endif
#endif /* PHYSICL_HIP_H */
