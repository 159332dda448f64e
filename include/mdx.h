/*
 * mdx.h — C-ABI of libmdx.so, the MI355X-native trajectory-analysis core.
 *
 * The reference (bbye98/mdhelper) has no FFI on this path: its hot loops sit
 * behind Python functions.  Each entry point below therefore cites the Python
 * function (reference file:line) whose work it carries; INTEGRATION.md shows
 * the ctypes stub a maintainer adds at that call site.
 *
 * Conventions
 *   - every function returns MDX_OK (0) or a negative error class;
 *     mdx_last_error() returns the thread-local message of the last failure;
 *   - plain pointers and sizes only; the caller owns every host buffer and the
 *     library never keeps a host pointer past return;
 *   - "_device" variants take pointers obtained from mdx_malloc() (HBM-resident
 *     input, no PCIe traffic inside the call);
 *   - a handle owns its device memory and stream, is bound to one device and
 *     is not thread-safe (one handle per device per host thread);
 *   - positions are float32[n_frames][n][3] (MDAnalysis' native layout),
 *     boxes float32[n_frames][6] = (lx, ly, lz, alpha, beta, gamma), or NULL
 *     for no periodic boundaries.  Orthorhombic and triclinic cells are both
 *     handled by the RDF (a batch may mix them); the Fourier-space engines take
 *     positions only.
 */
#ifndef MDX_H
#define MDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDX_VERSION 100 /* 0.1.0 */

#define MDX_OK 0
#define MDX_ERR_INVALID_VALUE (-1) /* -> ValueError          */
#define MDX_ERR_UNSUPPORTED (-2)   /* -> NotImplementedError */
#define MDX_ERR_NO_DEVICE (-3)     /* -> RuntimeError        */
#define MDX_ERR_HIP (-4)           /* -> RuntimeError        */
#define MDX_ERR_ROCFFT (-5)        /* -> RuntimeError        */
#define MDX_ERR_RCCL (-6)          /* -> RuntimeError        */
#define MDX_ERR_OUT_OF_MEMORY (-7) /* -> MemoryError         */
#define MDX_ERR_STATE (-8)         /* -> RuntimeError        */
#define MDX_ERR_IO (-9)            /* -> OSError             */
#define MDX_ERR_INTERNAL (-10)     /* -> RuntimeError        */

/* ------------------------------------------------------------------ runtime
 * Loading the library sets GPU_PINNED_MIN_XFER_SIZE=1048576 (MiB) in the process unless the variable is set already:
 * the HIP runtime then stages pageable copies through its own buffers instead of page-locking caller memory and
 * KEEPING the registration (a kept registration of memory that is freed and handed out again, or of a file mapping
 * that is truncated, aborts or blocks the process: NOTES.md round 5).  Copies of >= 1 MiB through mdx_memcpy_* /
 * mdx_upload* use the library's pinned ring or pages it locks and unlocks itself.  MDX_ABORT_TRACE=<fd>: native
 * call stack on SIGABRT. */

const char *mdx_last_error(void);
int mdx_version(void);
int mdx_device_count(int *count);
/* name: caller buffer of name_len bytes; any out pointer may be NULL. */
int mdx_device_info(int dev, char *name, size_t name_len, int *compute_units,
                    size_t *hbm_bytes, size_t *hbm_free_bytes);
int mdx_malloc(int dev, size_t bytes, void **dptr);
int mdx_free(int dev, void *dptr);
int mdx_memcpy_h2d(int dev, void *dst, const void *src, size_t bytes);
int mdx_memcpy_d2h(int dev, void *dst, const void *src, size_t bytes);
int mdx_memset(int dev, void *dst, int value, size_t bytes);
/* Host memory -> HBM at the rate of the host-buffer entry points: page-locked / registered memory by one DMA
 * where it lies, pageable memory through the library's pinned ring with its copy threads (so does mdx_memcpy_h2d
 * from 1 MiB on; below that it is the runtime's staging).  Returns when the data is in HBM. */
int mdx_upload(int dev, void *d_dst, const void *src, size_t bytes);
/* ... for n_rows rows of row_bytes that lie src_stride bytes apart on the host and end up contiguous in HBM: a
 * range of particles out of every frame of float32[T][N][3] (row_bytes = 12 n_range, src_stride = 12 N) — what
 * Onsager streams per group while the group before is being transformed (transport.py:976-992).  Pageable rows of
 * >= 4 KB that lie >= 2 pages apart in anonymous memory are read by the DMA engine where they lie: slices of ~128 MB
 * are page-locked, copied by one 2-D DMA and unlocked again, several side by side; every slice is unlocked before
 * the call returns.  Short or nearly contiguous rows and rows of a file mapping are gathered into the pinned ring. */
int mdx_upload_rows(int dev, void *d_dst, const void *src, size_t row_bytes, size_t src_stride, size_t n_rows);
/* Destroyed handles and mdx_free leave their device blocks (of any size) in a per-device, per-process cache so
 * that an analysis object per call does not pay hipMalloc / hipFree each time (at C4 size: seconds inside
 * hipMalloc every other analysis).  The cache holds at most MDX_CACHE_GB GiB when that variable is set, else a
 * quarter of the memory that was FREE on the device when the cache was first used (at least 4 GiB).  It is given
 * back automatically when an allocation of this library fails, and here on request: call mdx_trim_cache before
 * handing the device to another library or process (rocFFT, another rank sharing the GPU) — nobody else can
 * reclaim it.  mdx_device_info reports free memory WITHOUT the cached bytes (they are reported separately by
 * mdx_cached_bytes).  freed_bytes may be NULL. */
int mdx_trim_cache(int dev, size_t *freed_bytes);
int mdx_cached_bytes(int dev, size_t *bytes);
/* Which user-mode ROCm libraries this library's calls are bound to in THIS process — the files the dynamic
 * linker resolved hipGetDeviceCount, rocfft_setup and ncclGetVersion to — with their versions and the ROCm root
 * the library was built for, as "key=value\n" text (keys: rocm_root, libamdhip64, librocfft, librccl, libmdx,
 * hip_runtime_version, hip_driver_version, rccl_version, rocfft_version).  Works without a device.  A process
 * that loaded another copy of these libraries first (e.g. `import torch`, whose wheel bundles its own ROCm)
 * binds libmdx.so to THAT copy; mdhelper_amd._lib refuses to run so (one process, one runtime). */
int mdx_runtime_info(char *buf, size_t bytes);
int mdx_device_synchronize(int dev);
/* Page-lock a caller buffer (e.g. the float32[n_frames][n][3] array an MDAnalysis memory reader
 * holds — what `universe.trajectory[frame].positions` views, reference structure.py:753,796) so
 * that the host-buffer entry points below hand it to the DMA engine where it lies, without the
 * staging copy through the library's own pinned ring.  Optional: unregistered memory works, one
 * host copy slower.  The caller unregisters before freeing the buffer. */
/* Whole pages are locked (the range is widened to page boundaries); a range that shares a page with one still
 * registered is refused (MDX_ERR_STATE); mdx_host_unregister takes the pointer that was registered, waits for
 * the device, and fails for a pointer it does not know.  A buffer only partly covered by a registration is
 * treated as pageable by every entry point. */
int mdx_host_register(int dev, void *ptr, size_t bytes);
int mdx_host_unregister(int dev, void *ptr);

/* Synthetic wrapped Gaussian random walk, generated in HBM (bench / tests):
 * frame 0 uniform in [0, L)^3, then x += sigma * N(0,1) wrapped into the box;
 * counter-based Philox-4x32-10 keyed by (seed, atom, frame) so any frame can
 * be regenerated anywhere.  out: float32[n_frames][n_atoms][3] on the device. */
int mdx_synth_random_walk(int dev, float *d_out, int64_t n_frames, int64_t n_atoms,
                          const float box_lengths[3], float sigma, uint64_t seed,
                          int wrap);
/* Unwrapped walk in float64[n_frames][n_atoms][3] (the Onsager position store,
 * transport.py:932), same generator. */
int mdx_synth_random_walk_f64(int dev, double *d_out, int64_t n_frames, int64_t n_atoms,
                              const float box_lengths[3], float sigma, uint64_t seed);

/* ---------------------------------------------------------------- collectives
 * One process per GPU; the communicator is RCCL over xGMI.  Rank 0 calls
 * mdx_comm_unique_id() and ships the 128-byte id to the other ranks through
 * whatever rendezvous the launcher offers (mdhelper_amd/launch.py: a node-local
 * unix socket); then every rank calls mdx_comm_init_rank(). */
typedef struct mdx_comm *mdx_comm_t;
#define MDX_COMM_ID_BYTES 128
int mdx_comm_unique_id(unsigned char id[MDX_COMM_ID_BYTES]);
int mdx_comm_init_rank(mdx_comm_t *comm, int dev, const unsigned char id[MDX_COMM_ID_BYTES],
                       int rank, int world_size);
int mdx_comm_destroy(mdx_comm_t comm);
/* what RCCL itself reports for this communicator (ncclCommCount / UserRank / CuDevice);
 * any out pointer may be NULL */
int mdx_comm_count(mdx_comm_t comm, int *count, int *rank, int *device);
int mdx_comm_barrier(mdx_comm_t comm);
/* in-place sum / max all-reduce of small host vectors (staged through HBM) */
int mdx_comm_allreduce_f64(mdx_comm_t comm, double *host_inout, int64_t n, int op_max);
int mdx_comm_allreduce_i64(mdx_comm_t comm, int64_t *host_inout, int64_t n);

/* ------------------------------------------------------------------------ RDF
 * Replaces the per-frame body of RadialDistributionFunction._single_frame
 * (reference src/mdhelper/analysis/structure.py:750-791), i.e. the call
 *     counts += radial_histogram(pos1, pos2, n_bins, range, dims, exclusion)
 * (structure.py:32-104, :788-791) for a batch of frames at once. */
typedef struct mdx_rdf *mdx_rdf_t;

#define MDX_RDF_ALGO_AUTO 0
#define MDX_RDF_ALGO_EXACT_F64 1 /* contract arithmetic on every pair            */
#define MDX_RDF_ALGO_FILTER_F32 2 /* f32 filter + exact f64 re-evaluation near edges */
#define MDX_RDF_ALGO_CELL 3      /* cell-sorted tiles, culled tile pairs, f32 filter */

/* edges: the n_bins+1 float64 bin edges exactly as numpy.linspace(r_min, r_max,
 * n_bins+1) yields them (structure.py:737; numpy.histogram builds the same
 * array).  Enforced, for every algo and before the device is touched: an array that is not
 * strictly increasing, or in which some edges[k] lies more than 4 ulp(edges[n_bins]) from
 * edges[0] + k (edges[n_bins] - edges[0]) / n_bins (numpy.linspace stays within 2), is refused
 * with MDX_ERR_INVALID_VALUE and a message that names the first such edge — the float32 filter
 * and the cell-sorted kernel take bins from the uniform grid and would count other arrays
 * wrongly.  excl1/excl2: the reference's `exclusion` tuple, 0/0 for None. */
int mdx_rdf_create(mdx_rdf_t *out, int dev, int n_bins, const double *edges,
                   int64_t excl1, int64_t excl2, int algo);
/* The launch plan of an engine created with these arguments (checked as mdx_rdf_create checks them) for ONE run of
 * n_frames frames of one cell kind, as every accumulate entry point hands it to the pair kernels: sets of n1 and n2
 * points (same != 0: one set against itself, n2 ignored; no grouping, no dropped axis), boxes float32[n_frames][6] on
 * the host or NULL for no periodic cell.  A batch that mixes orthorhombic and triclinic frames is cut into such runs
 * by the engine and refused here (MDX_ERR_INVALID_VALUE).  Slots 17 and 18 describe a run handed over whole, that is
 * one call of mdx_rdf_accumulate_device: the host-buffer and trajectory entry points stage a call in pieces of their
 * own first (MDX_RDF_PIPE_MB, 256 MiB of source frames by default, the first two pieces of a call a quarter and a
 * half of that or of the call), and every piece is a run of its own with slabs of its own.
 * Touches no device; honours MDX_RDF_SLAB_BYTES, MDX_RDF_TRI_BRUTE and MDX_RDF_CHUNK_TILES as the engine does.  out:
 *    0 kernel family: 0 rdf_tile_kernel, exact arithmetic; 1 rdf_tile_kernel, float32 filter; 2 rdf_cell_pair_kernel
 *      on orthorhombic frames; 3 rdf_tri_tile_kernel (brute-force triclinic); 4 rdf_cell_pair_kernel on triclinic
 *      frames (culled)
 *    1 IPT: i particles per thread (tile rows T = 256 IPT; 1 outside family 0 / 1)
 *    2 self: one set with one exclusion tag per row, mirror tile pairs counted twice
 *    3 EXCL, 4 PBC (frames have a cell), 5 LOWER (range starts above 0; families 2 / 4, else 0)
 *    6 SKIP (the step that leaves empty: families 2 / 4, always 1 in family 4; unused by the global form)
 *    7 GH: thresholds and histogram in global memory
 *    8 LDS histogram replicas n_hist (0 with GH)
 *    9 dynamic LDS bytes of the pair launch, 10 whether hipFuncAttributeMaxDynamicSharedMemorySize is set for it
 *      (above 48 KiB; the cell-sorted launches never set it)
 *   11, 12 padded rows of set 1 and set 2 (multiples of T; of 128 in families 2 / 4)
 *   13, 14 tiles of set 1 and set 2 (T rows; families 2 / 4: 128-row i tiles, 64-row j tiles)
 *   15 chunk: j tiles one block (families 2 / 4: one item) walks
 *   16 grid x of the pair launch (families 2 / 4: items per i tile; their grid is sized from the device's occupancy)
 *   17 frames per slab, 18 slabs of the run: at most 32 768 frames each.  Families 2 / 4: as on the serial route
 *      (MDX_RDF_SORT_BESIDE=0, or where the sort cannot run beside the pair kernel); with the sort beside, a run of
 *      more than one slab starts with a quarter and a half slab and so takes more slabs than slot 18 says
 *   19 lazy_orig: no sorted copy of the original coordinates (family 2 with exclusion 0 or 1)
 *   20 .. 23 reserved, 0. */
#define MDX_RDF_PLAN_SLOTS 24
int mdx_rdf_plan(int n_bins, const double *edges, int64_t excl1, int64_t excl2, int algo, int64_t n1, int64_t n2,
                 int same, const float *boxes, int64_t n_frames, int64_t out[MDX_RDF_PLAN_SLOTS]);
/* The same slots for the handle's most recent run, from the plan that run was launched from (the engine builds it
 * with the function mdx_rdf_plan calls).  A run is what one piece of a call hands over in frames of one cell kind, so
 * slots 17 and 18 follow the cuts of the entry point that fed it.  MDX_ERR_STATE before any run and after
 * mdx_rdf_reset. */
int mdx_rdf_last_plan(mdx_rdf_t h, int64_t out[MDX_RDF_PLAN_SLOTS]);
/* The constants of the float32 filter of rdf_cell_pair_kernel for one orthorhombic frame: cell lengths box[3], the
 * batch's largest |coordinate| max_abs, range [r0, r1] in n_bins bins.  Touches no device; the values are those the
 * frame-constant kernel computes (same functions, same arithmetic).  out:
 *    0 eta: distance from a bin edge, in bins, within which a pair goes to the exact arithmetic
 *    1 sure_w = 1 - 2 eta, 2 TQ = floor(2^16 sure_w) clamped to [0, 65 535]: a pair is sure when the low half of its
 *      16.16 fixed-point bin position is below TQ (LDS histogram) or fract(pos) < sure_w (global histogram)
 *    3 inv_w = fl32(1 / width), 4 pos0 = -r0 inv_w - eta: pos = fl32(sqrt(r2) inv_w + pos0)
 *    5 IWQ = 2^16 inv_w, 6 P0Q = 2^16 pos0 (exact scalings): q = floor(fl32(sqrt(r2) IWQ + P0Q))
 *    7, 8 the candidate window on the float32 squared distance (8: -1 when the range starts at 0)
 *    9 reserved, 0. */
#define MDX_RDF_FILTER_SLOTS 10
int mdx_rdf_filter_constants(int n_bins, double r0, double r1, const float box[3], float max_abs,
                             double out[MDX_RDF_FILTER_SLOTS]);
int mdx_rdf_destroy(mdx_rdf_t h);
int mdx_rdf_reset(mdx_rdf_t h);
/* Host buffers.  pos2 == NULL (or == pos1 with n2 == n1) means ag2 is ag1: the
 * kernel then evaluates each unordered pair once and counts it twice, which is
 * bit-identical because the contract arithmetic is exactly antisymmetric. */
int mdx_rdf_accumulate(mdx_rdf_t h, const float *pos1, int64_t n1, const float *pos2,
                       int64_t n2, const float *boxes, int64_t n_frames);
/* 2-D mode, RadialDistributionFunction(drop_axis=...) (structure.py:761-770): coordinate `axis`
 * (0, 1, 2; -1 switches the mode off) of both sets is set to zero after the centre-of-mass stage
 * and the cell length along it becomes max(lx, ly, lz), on the device, for every entry point. */
int mdx_rdf_set_drop_axis(mdx_rdf_t h, int axis);
/* Centres of mass on the device for groupings="residues"/"segments" (structure.py:753-759 via
 * algorithm/molecule.py:300-306): the rows of set `which` (1 or 2) handed to any accumulate
 * call are then PARTICLES, molecule g owning rows [offsets[g], offsets[g+1]); the histogram is
 * taken over the float32 centres sum_a m_a x_a / M_g.  offsets: int64[n_groups+1], masses:
 * float64[offsets[n_groups]], both on the host; n_groups <= 0 removes the grouping. */
int mdx_rdf_set_grouping(mdx_rdf_t h, int which, int64_t n_groups, const int64_t *offsets,
                         const double *masses);
/* Same, all pointers in HBM (from mdx_malloc); asynchronous on the handle's stream. */
int mdx_rdf_accumulate_device(mdx_rdf_t h, const float *d_pos1, int64_t n1,
                              const float *d_pos2, int64_t n2, const float *d_boxes,
                              int64_t n_frames);
/* Waits for the stream, then copies int64[n_bins] counts (np.intp, structure.py:740). */
int mdx_rdf_counts(mdx_rdf_t h, int64_t *counts);
int mdx_rdf_synchronize(mdx_rdf_t h);
/* Sum the counts of every rank's handle (one RCCL all-reduce, uint64 sum). */
int mdx_rdf_allreduce(mdx_rdf_t h, mdx_comm_t comm);
/* Timing / statistics of the pair kernel, measured with HIP events on the
 * handle's stream: launches since reset, total milliseconds, ordered pairs
 * covered (frames * n1 * n2), pairs re-evaluated by the exact path, and distance
 * evaluations actually executed (after symmetry and tile culling, padding
 * included).  Any pointer may be NULL. */
int mdx_rdf_stats(mdx_rdf_t h, int64_t *launches, double *kernel_ms,
                  int64_t *pairs_evaluated, int64_t *pairs_exact, int64_t *pairs_computed);
int mdx_rdf_enable_timing(mdx_rdf_t h, int on);
/* Raw device counters since reset: [0] exact re-evaluations, [1] (64 x 16)-pair units run by
 * the cell kernel, [2] units on its per-pair image-search path, [3] brute-force evaluations. */
int mdx_rdf_debug_counters(mdx_rdf_t h, int64_t out[4]);
/* Timing runs (mdx_rdf_enable_timing): the engine clock the cell-sorted pair kernel actually ran
 * at since reset, in Hz — every block adds its span in s_memtime and in 100 MHz s_memrealtime
 * ticks; 0 when no such kernel has run. */
int mdx_rdf_kernel_clock(mdx_rdf_t h, double *hz);
/* Cell path: slabs since reset whose sort ran beside the pair kernel of the slab before (two sets of
 * sorted copies, a second stream); 0 while every call took the serial route — single-slab calls,
 * triclinic frames, more than 65 535 particles in a set, MDX_RDF_SORT_BESIDE=0. */
int mdx_rdf_slabs_sorted_beside(mdx_rdf_t h, int64_t *out);
/* Cell path: the sorted copies (wrapped and original float4 rows, n_pad rows) of one frame of
 * the most recent slab — for debugging the tile logic on the host.  With exclusion 0 or 1 the
 * sorted originals are not materialised: pw is filled and MDX_ERR_STATE returned. */
int mdx_rdf_debug_sorted(mdx_rdf_t h, int64_t frame, int64_t n_pad, float *pw, float *po);

/* Function-level drop-in for structure.radial_histogram (structure.py:32-104):
 * one frame, host buffers, counts overwritten. */
int mdx_radial_histogram(int dev, const float *pos1, int64_t n1, const float *pos2,
                         int64_t n2, int n_bins, const double *edges, const float dims[6],
                         int64_t excl1, int64_t excl2, int64_t *counts);

/* --------------------------------------------------------------- structure factor
 * Replaces StructureFactor._single_frame (structure.py:1481-1527) with its
 * Numba kernels delta_fourier_transform_sum_2d_2d / inner_2d_2d /
 * pythagorean_trigonometric_identity_* (src/mdhelper/algorithm/accelerated.py:81-321):
 *   rho_g(q) = sum_{j in group g} exp(i q.r_j)  (fp64), then per pair (j,k)
 *   ssf += |rho_j|^2  (j == k)   or   2 Re(rho_j rho_k*)  (j != k).
 * Both `form`s of the reference map onto this one fused kernel. */
typedef struct mdx_sq *mdx_sq_t;

/* wavevectors: float64[n_q][3].  group_offsets: int64[n_groups+1] into the
 * concatenated position array (structure.py:1427-1431).  pairs: int32[n_pairs][2]
 * group indices; (-1,-1) = all particles as one group (mode=None). */
int mdx_sq_create(mdx_sq_t *out, int dev, const double *wavevectors, int64_t n_q,
                  const int64_t *group_offsets, int n_groups, const int32_t *pairs,
                  int n_pairs);
int mdx_sq_destroy(mdx_sq_t h);
int mdx_sq_reset(mdx_sq_t h);
/* groupings="residues" / "segments" (structure.py:1484-1486 with center_of_mass): the rows handed to
 * every accumulate entry point are then particles sorted molecule by molecule — molecule g = rows
 * [offsets[g], offsets[g+1]), masses float64[offsets[n_molecules]] — and the Fourier sums run over
 * the float32 centres of mass formed on the device; group_offsets of mdx_sq_create index the
 * molecules.  Groups with groupings="atoms" enter as molecules of one particle and mass 1.
 * n_molecules <= 0 removes the grouping. */
int mdx_sq_set_grouping(mdx_sq_t h, int64_t n_molecules, const int64_t *offsets, const double *masses);
/* Single-chain structure factor (SingleChainStructureFactor._single_frame, polymer.py:1095-1099): the points —
 * counted after mdx_sq_set_grouping — form chains of chain_length consecutive points, and mdx_sq_result returns
 * float64[1][n_q] un-normalised sums over frames of sum_c |sum_{j in chain c} exp(i q.r_j)|^2.  Needs a handle
 * created with one group over all points and pairs = {(-1,-1)}, and a point count divisible by chain_length;
 * only before the first frame (after mdx_sq_create or mdx_sq_reset).  chain_length <= 0 restores the normal
 * mode.  Every accumulate entry point, mdx_sq_allreduce and the statistics work as in the normal mode. */
int mdx_sq_set_chains(mdx_sq_t h, int64_t chain_length);
int mdx_sq_accumulate(mdx_sq_t h, const float *pos, int64_t n, int64_t n_frames);
/* Positions already in HBM.  ASYNCHRONOUS on the handle's stream: the call may return while kernels still read
 * d_pos; a producer that rewrites the buffer (an MD engine feeding batches) calls mdx_sq_synchronize first.
 * mdx_sq_result and mdx_sq_destroy wait by themselves. */
int mdx_sq_accumulate_device(mdx_sq_t h, const float *d_pos, int64_t n, int64_t n_frames);
int mdx_sq_synchronize(mdx_sq_t h);
/* float64[n_pairs][n_q] un-normalised sums over frames (structure.py:1494-1508). */
int mdx_sq_result(mdx_sq_t h, double *ssf);
int mdx_sq_allreduce(mdx_sq_t h, mdx_comm_t comm);
int mdx_sq_stats(mdx_sq_t h, int64_t *launches, double *kernel_ms);
int mdx_sq_enable_timing(mdx_sq_t h, int on);
/* The launch plan of an engine created with these wavevectors and n_groups groups (the largest of max_group points,
 * together spanning n_total points) for ONE accumulate call of n_frames frames; chain_length > 0: in the single-chain
 * mode of mdx_sq_set_chains (n_groups = 1, n_total a multiple of chain_length), else the normal mode.  Touches no
 * device; honours MDX_SQ_NO_LATTICE, MDX_SQ_NO_COLUMNS and MDX_SQ_NO_QUADS as mdx_sq_create and mdx_sq_set_chains
 * do.  out: 0 route (0 general sincos, 1 per-wavevector lattice tables, 2 column items, 3 register-blocked quads;
 * chain mode: 0 sincos or 3 quads), 1 row stride of the regular quad form (0: general items, or no quads),
 * 2 particles per LDS stage (the table tile of the lattice routes), 3 copies per quad item (1 without quads),
 * 4 items per block (quad or column items; general and tables: wavevectors), 5 blocks along the wavevectors,
 * 6 threads per block, 7 particle parts per group (chain mode: parts of whole chains, none empty), 8 frames per slab
 * (the call is cut at 32 768 frames or 512 MiB of partial sums), 9 chain mode: chains per part, else 0. */
int mdx_sq_plan(const double *wavevectors, int64_t n_q, int n_groups, int64_t max_group, int64_t n_total,
                int64_t chain_length, int64_t n_frames, int32_t out[10]);
/* Function-level drop-in for accelerated.delta_fourier_transform_sum_2d_2d
 * (accelerated.py:81-122): out = complex128[n_q] as (re, im) pairs; float64 positions. */
int mdx_fourier_sum(int dev, const double *wavevectors, int64_t n_q, const double *positions,
                    int64_t n, double *out_re_im);
/* Function-level drop-ins for the trigonometric forms (accelerated.py:167-247, :249-321, :323-627; the public
 * static methods StructureFactor.ssf_trigonometric_2d / psf_trigonometric_2d_2d, structure.py:1238-1317):
 *   mdx_inner         out[i][j] = q_i . r_j, float64[n_q][n]                      (inner_2d_2d)
 *   mdx_trig_rowsums  cos_out[i] = sum_j cos(x[i][j]), sin_out[i] = sum_j sin(x[i][j]) for a caller-supplied
 *                     float64[n_rows][n_cols] (either output may be NULL)         (cosine_sum_*, sine_sum_*,
 *                     and, squared and added on the host, pythagorean_trigonometric_identity_*)
 * x streams from host memory in row slabs (pinned ring / DMA) beside the kernels; the _device variant takes
 * x and the outputs in HBM and returns when they are written. */
int mdx_inner(int dev, const double *wavevectors, int64_t n_q, const double *positions, int64_t n, double *out);
int mdx_trig_rowsums(int dev, const double *x, int64_t n_rows, int64_t n_cols, double *cos_out, double *sin_out);
int mdx_trig_rowsums_device(int dev, const double *d_x, int64_t n_rows, int64_t n_cols, double *d_cos,
                            double *d_sin);

/* ------------------------------------------------- intermediate scattering function
 * Replaces IntermediateScatteringFunction._single_frame (structure.py:1956-2083): the
 * coherent part from lagged products of rho_g(q, f) and, optionally, the incoherent
 * part sum_j cos(q . (r_j(f) - r_j(f - lag))) for lags 0 .. n_lags-1.  Arguments as for
 * mdx_sq_create; frames must be fed in analysis order (consecutive calls continue). */
typedef struct mdx_isf *mdx_isf_t;
int mdx_isf_create(mdx_isf_t *out, int dev, const double *wavevectors, int64_t n_q,
                   const int64_t *group_offsets, int n_groups, const int32_t *pairs, int n_pairs,
                   int n_lags, int incoherent);
int mdx_isf_destroy(mdx_isf_t h);
int mdx_isf_reset(mdx_isf_t h);
/* Every call of a series gives the same n (with a grouping: the grouping's particles): another n after the first
 * frame is MDX_ERR_INVALID_VALUE and leaves the sums as they were, with or without the incoherent part;
 * mdx_isf_reset starts a new series, which may have another n. */
int mdx_isf_accumulate(mdx_isf_t h, const float *pos, int64_t n, int64_t n_frames);
/* Same, positions already in HBM on the engine's device (float32[n_frames][n][3]).  ASYNCHRONOUS on the
 * handle's stream: the frames are copied into the engine's position ring by a device-to-device copy queued on
 * that stream, and the call may return before the copy has run; a producer that rewrites d_pos calls
 * mdx_isf_synchronize first (mdx_isf_result / mdx_isf_stats / mdx_isf_destroy wait by themselves). */
int mdx_isf_accumulate_device(mdx_isf_t h, const float *d_pos, int64_t n, int64_t n_frames);
int mdx_isf_synchronize(mdx_isf_t h);
/* As mdx_sq_set_grouping; only before the first frame of a series. */
int mdx_isf_set_grouping(mdx_isf_t h, int64_t n_molecules, const int64_t *offsets, const double *masses);
/* cisf: float64[n_lags][n_pairs][n_q]; iisf (may be NULL): float64[n_lags][n_slots][n_q] with
 * n_slots = 1 for mode=None (pairs = (-1,-1)) and n_groups otherwise; un-normalised sums. */
int mdx_isf_result(mdx_isf_t h, double *cisf, double *iisf);
int mdx_isf_stats(mdx_isf_t h, int64_t *launches, double *kernel_ms, int64_t *frames);
int mdx_isf_enable_timing(mdx_isf_t h, int on);
/* The launch plan of an engine created with these wavevectors, n_groups groups (the largest of max_group
 * particles), n_slots incoherent slots (the largest of max_range particles) and n_lags lags, for a chunk of n_new
 * new frames (an accumulate call is cut into chunks of at most n_lags frames).  Touches no device; honours
 * MDX_SQ_NO_LATTICE and MDX_ISF_NO_QUADS as mdx_isf_create does.  out: 0 route (0 general sincos, 1 per-wavevector
 * lattice tables, 2 register-blocked quads), 1 row stride of the regular quad form (0: general items, or no quads),
 * 2 particles per table tile of the incoherent kernel, 3 copies per quad item (1 without quads), 4 quad items
 * (without quads: wavevectors) per block, 5 blocks along the wavevectors, 6 particle parts of rho, 7 particle parts
 * of the incoherent sums. */
int mdx_isf_plan(const double *wavevectors, int64_t n_q, int n_groups, int n_slots, int n_lags, int64_t max_group,
                 int64_t max_range, int64_t n_new, int32_t out[8]);

/* ------------------------------------------------------------- time correlation
 * Replaces algorithm.correlation.correlation_fft / msd_fft
 * (src/mdhelper/algorithm/correlation.py:17-226, :461-668) as called from
 * Onsager._conclude (src/mdhelper/analysis/transport.py:1016-1059). */
typedef struct mdx_msd *mdx_msd_t;

/* One engine per (n_frames_block, n_blocks).  The transform length n_fft >= 2 n_frames_block - 1
 * (any such length gives the same linear correlation; the reference pads to
 * 2*next_fast_len(n_frames_block), correlation.py:176-178): the shortest length of the engine's own
 * two-pass kernels (400 x 2^k or a power of two) for blocks of 201 .. 524 288 frames, else the reference
 * length or the next power of two through rocFFT (mdx_msd_n_fft / mdx_msd_transform report it). */
int mdx_msd_create(mdx_msd_t *out, int dev, int64_t n_frames_block, int n_blocks,
                   int n_groups);
int mdx_msd_destroy(mdx_msd_t h);
int mdx_msd_reset(mdx_msd_t h);
int mdx_msd_n_fft(mdx_msd_t h, int64_t *n_fft);
/* Which forward transform the engine runs: *own = 1 and n_fft = r1 x r2 for the engine's own two-pass kernels
 * (csrc/mdx_msd_fft.hpp), *own = 0 (r1 = r2 = 0) for the rocFFT pipeline.  No reference counterpart: the
 * reference has one path (scipy.fft, correlation.py:176-197); benchmarks and tests name the path they measured. */
int mdx_msd_transform(mdx_msd_t h, int *own, int *r1, int *r2);
/* The launch plan of an engine created with (n_frames_block, n_blocks) for ONE push of particles [first, first+count)
 * of an array of n_total particles per frame, elem_bytes 8 (mdx_msd_push_device) or 4 (mdx_msd_push_device_f32:
 * MDX_ERR_UNSUPPORTED where the engine does not read float32 in place), base_aligned != 0: the array starts on a
 * 128-byte boundary (anything from hipMalloc).  Touches no device; honours MDX_MSD_ROCFFT and MDX_MSD_TWO_PASS as
 * mdx_msd_create does.  The push is described as ONE chunk: the engine cuts a push into equal chunks only when the
 * half-transformed block of the whole push does not fit ~40 % of the free HBM, which no host-only query can know.
 * mdx_msd_push stages the selection first, so its pushes are (n_total = count, first = 0, base_aligned = 1).
 * out: 0 n_fft, 1 own transform (else rocFFT), 2 r1, 3 r2 (0 without own transform), 4 single pass, 5 pass A forms
 * the per-frame sums, 6 float32 read in place,
 * 7 pass A: 0 msd_gather_kernel + rocFFT, 1 msd_fft_single400_kernel<r2>, 2 msd_fft_cols400_fused_kernel<r2>,
 *   3 msd_fft_cols_small_fused_kernel<64, r2>, 4 msd_fft_cols_kernel<r1, r2> (sums: msd_sums_kernel),
 * 8 pass B: 0 none (single pass, rocFFT), 1 msd_fft_rows_tiny_power_kernel, 2 msd_fft_rows_short_power_kernel,
 *   3 msd_fft_rows_mid_power_kernel, 4 msd_fft_rows512_power_kernel, 5 msd_fft_rows1024_power_kernel,
 *   6 msd_fft_rows_power_kernel (the general rows kernel: no length of the engine's takes it),
 * 9 head: coordinates by which pass A enters the chunk early to read whole 128-byte lines, 10 n_elem = 3 count + head,
 * 11 p_pad: coordinate pairs padded to whole pair groups, 12 super groups of the fused pass A (0: not fused),
 * 13 the split of pass A's grid: blockIdx.x of the single-pass kernel, blockIdx.y of the others (0: rocFFT),
 * 14 parts of pass B (blockIdx.z; 0: no pass B), 15 Y is laid out pair-group-major. */
int mdx_msd_plan(int64_t n_frames_block, int n_blocks, int64_t n_total, int64_t first, int64_t count, int elem_bytes,
                 int base_aligned, int64_t out[16]);
/* Feed particles of one group: pos float64[n_blocks*n_frames_block][n_total][3]
 * (transport.py:932 layout), of which particles [first, first+count) belong to
 * `group`.  Accumulates sum_particles of the per-particle self MSD numerators
 * and sum_particles r(t) for the collective terms.  zero_dims: bit k set ->
 * dimension k is zeroed (transport.py:1025,1033). */
int mdx_msd_push(mdx_msd_t h, int group, const double *pos, int64_t n_total, int64_t first,
                 int64_t count, int zero_dims);
int mdx_msd_push_device(mdx_msd_t h, int group, const double *d_pos, int64_t n_total,
                        int64_t first, int64_t count, int zero_dims);
/* The same for float32 positions resident in HBM — what a trajectory reader or a GPU MD engine holds —, a plain
 * particle range with nothing to prepare (no unwrapping, no molecule centres, no shift): pass A widens them as it
 * stages them, so no float64 copy is made (C4: 18 GB of traffic per group less).  Only the engine's transforms
 * with a 400- or 64-point first factor read float32 in place (mdx_msd_transform: r1 == 400 or 64 — the single-pass
 * kernel, the 400 x R2 family and 2^13 .. 2^16: every block length up to 204 800 frames); other engines (2^18 .. 2^20,
 * rocFFT) return MDX_ERR_UNSUPPORTED
 * and the caller goes through mdx_msd_push_frames_device.  Results equal those of the widened
 * frames bit for bit. */
int mdx_msd_push_device_f32(mdx_msd_t h, int group, const float *d_pos, int64_t n_total, int64_t first,
                            int64_t count, int zero_dims);
/* msd_self[g][b][t] = sum_particles MSD_particle / N_g  (transport.py:1036-1039, before /2D)
 * sum_traj[g][b][t][3] = sum_particles r(t)            (input of :1034 and :1044-1052) */
int mdx_msd_result(mdx_msd_t h, double *msd_self_sum, double *sum_traj);
/* acf_sum[g][b][m] = sum_particles sum_d sum_k x(k) x(k+m), m < n_frames_block, not normalised:
 * the vector ACF numerator of correlation_fft(..., average=True, vector=True) as called by
 * EndToEndVector._conclude (src/mdhelper/analysis/polymer.py:765-781) = acf_sum / (N (T - m)). */
int mdx_msd_result_acf(mdx_msd_t h, double *acf_sum);
int mdx_msd_allreduce(mdx_msd_t h, mdx_comm_t comm);
int mdx_msd_stats(mdx_msd_t h, int64_t *launches, double *kernel_ms, int64_t *bytes_moved);
int mdx_msd_enable_timing(mdx_msd_t h, int on);

/* Function-level drop-in for correlation.correlation_fft on real input
 * (correlation.py:17-226): n_series independent series of length n_t, laid out
 * [n_series][n_t] contiguous; b == NULL -> ACF.  out[n_series][n_t] =
 * sum_k a[k] b[k+m] (un-normalised, lags m = 0..n_t-1); with neg_out != NULL the
 * negative lags sum_k a[k+m] b[k] are written there too. */
int mdx_correlate(int dev, const double *a, const double *b, int64_t n_series, int64_t n_t,
                  double *out, double *neg_out);

/* ------------------------------------------------------- trajectory ingest */

/* Native readers for the files the reference's users analyse: AMBER NetCDF trajectories
 * (the container and variables its own writer produces,
 * src/mdhelper/openmm/file.py:49-52 `NETCDF3_64BIT_OFFSET`, :160-188 `coordinates`,
 * `cell_lengths`, `cell_angles`, `time`) and CHARMM/NAMD DCD.  They replace the per-frame
 * Python reader behind `universe.trajectory[frame]` (structure.py:796, transport.py:976-985)
 * on the way to the GPU: raw records go through pinned buffers to HBM and are byte-swapped /
 * transposed / gathered there.  format: 1 NetCDF, 2 DCD. */
typedef struct mdx_traj *mdx_traj_t;
int mdx_traj_open(mdx_traj_t *out, const char *path);
int mdx_traj_close(mdx_traj_t h);
int mdx_traj_info(mdx_traj_t h, int64_t *n_frames, int64_t *n_atoms, int *has_box, int *has_time,
                  int *format);
/* Host reads of the listed frames: float32[n][n_atoms][3] (ts.positions), float32[n][6]
 * (ts.dimensions: lx ly lz alpha beta gamma), float64[n] times in ps. */
int mdx_traj_read_positions(mdx_traj_t h, const int64_t *frames, int64_t n, float *out);
int mdx_traj_read_boxes(mdx_traj_t h, const int64_t *frames, int64_t n, float *boxes6);
int mdx_traj_read_times(mdx_traj_t h, const int64_t *frames, int64_t n, double *times);
/* The listed frames into HBM: d_out float32[n][n_sel][3].  d_index: device int32[n_sel]
 * particle indices, or NULL for the first n_sel particles (n_sel <= 0: all). */
int mdx_traj_load_device(mdx_traj_t h, int dev, const int64_t *frames, int64_t n,
                         const int32_t *d_index, int64_t n_sel, float *d_out);
/* RDF over frames of a trajectory file.  boxes: host float32[n_frames][6] of those frames
 * (mdx_traj_read_boxes) or NULL; index1/index2: host int32 particle selections (ag.indices),
 * NULL = all particles; index2 == NULL with n2 == 0 = the same group twice. */
int mdx_rdf_accumulate_traj(mdx_rdf_t h, mdx_traj_t traj, const int64_t *frames,
                            int64_t n_frames, const float *boxes, const int32_t *index1,
                            int64_t n1, const int32_t *index2, int64_t n2);
/* S(q) / ISF over frames of a trajectory file.  index: host int32[n_index] particle indices
 * in the order of the concatenated groups (the `self._positions[s] = g.positions` fill of
 * structure.py:1484-1486), or NULL for the file's first n_index particles (<= 0: all).
 * The ISF consumes the frames in the order listed. */
int mdx_sq_accumulate_traj(mdx_sq_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                           const int32_t *index, int64_t n_index);
int mdx_isf_accumulate_traj(mdx_isf_t h, mdx_traj_t traj, const int64_t *frames,
                            int64_t n_frames, const int32_t *index, int64_t n_index);

/* MSD / Onsager: the first n_blocks * n_frames_block listed frames of a trajectory file as
 * one group's positions (the `self._positions[frame, slice] = g.positions` fill of
 * transport.py:976-992 for groupings="atoms").  index: host int32[n_index] particle indices or
 * NULL.  unwrap != 0 applies the reference's global unwrap (algorithm/topology.py:366-376,
 * thresholds dims/2 as passed by transport.py:933-937) on the device, with dims = the three
 * box lengths; zero_dims as for mdx_msd_push. */
int mdx_msd_push_traj(mdx_msd_t h, int group, mdx_traj_t traj, const int64_t *frames,
                      int64_t n_frames, const int32_t *index, int64_t n_index, int unwrap,
                      const double *dims, int zero_dims, const double *shift);
/* groupings="residues" / "segments" for the trajectory-file path (transport.py:983-992 with
 * center_of_mass(g, gr, images=...)): the rows of the following mdx_msd_push_traj calls are particles
 * sorted molecule by molecule — molecule g = rows [offsets[g], offsets[g+1]), masses
 * float64[offsets[n_molecules]] — and the engine receives the float64 centres of mass of the
 * unwrapped particles, minus `shift`.  n_molecules <= 0 removes the grouping. */
int mdx_msd_set_grouping(mdx_msd_t h, int64_t n_molecules, const int64_t *offsets, const double *masses);
/* System centre of mass of every listed frame, out float64[n_frames][3] (host), over the
 * listed particles with the given masses (transport.py:993-1014: all atoms for center_atom,
 * else the groups' particles); unwrap as above; wrap != 0 brings coordinates outside [0, L]
 * back first (center_wrap).  Its output is the `shift` of mdx_msd_push_traj (NULL: none):
 * shift[t] is subtracted from every position of frame t. */
int mdx_msd_system_com_traj(mdx_msd_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index, const double *masses, int unwrap,
                            const double *dims, int wrap, double *out);
/* Molecules made whole in the first analysed frame (Onsager(unwrap=True), reference
 * transport.py:936-941: make_whole over universe.atoms.fragments before the starting positions are
 * stored): images int32[n_sel][3] = the periodic image each row starts in, i.e. the flags the
 * reference's first unwrap call derives from x - x_whole.  They apply to every following unwrapped
 * push / system-COM call, whose selection must have n_sel rows in this order; n_sel = 0 clears. */
int mdx_msd_set_initial_images(mdx_msd_t h, const int32_t *images, int64_t n_sel);
/* The same frame preparation for frames in host memory (an in-memory trajectory): pos
 * float32[n_frames][n_sel][3] holds the selection, already gathered, in analysis order (rows sorted
 * molecule by molecule when mdx_msd_set_grouping is active); arguments otherwise as for
 * mdx_msd_push_traj / mdx_msd_system_com_traj. */
int mdx_msd_push_f32(mdx_msd_t h, int group, const float *pos, int64_t n_frames, int64_t n_sel,
                     int unwrap, const double *dims, int zero_dims, const double *shift);
int mdx_msd_system_com_f32(mdx_msd_t h, const float *pos, int64_t n_frames, int64_t n_sel,
                           const double *masses, int unwrap, const double *dims, int wrap, double *out);
/* ... and for float64 frames (an in-memory float64 trajectory: the reference's positions are the
 * float64 copies of transport.py:978); same stages, the unwrap state kept in float64. */
int mdx_msd_push_f64(mdx_msd_t h, int group, const double *pos, int64_t n_frames, int64_t n_sel,
                     int unwrap, const double *dims, int zero_dims, const double *shift);
int mdx_msd_system_com_f64(mdx_msd_t h, const double *pos, int64_t n_frames, int64_t n_sel,
                           const double *masses, int unwrap, const double *dims, int wrap, double *out);
/* Cross displacements between the groups' summed trajectories, out float64[n_pairs][n_blocks][n_frames_block]:
 * msd_fft(sum_i r, sum_j r) of reference correlation.py:461-668 as Onsager._conclude calls it for every pair
 * (transport.py:1034, 1052; pairs int32[n_pairs][2], i == j gives the collective MSD of a group), computed
 * from the summed trajectories the pushes have left in HBM (after mdx_msd_allreduce: of all ranks). */
int mdx_msd_cross(mdx_msd_t h, const int32_t *pairs, int64_t n_pairs, double *out);
/* ... and for frames already resident in HBM (a GPU MD engine's output, or a host / file trajectory uploaded
 * once for several groups: mdx_upload, mdx_traj_load_device): d_pos float32 (elem_bytes 4) or float64 (8)
 * [n_frames][n_total][3]; index: host int32[n_index] rows of the selection in analysis order, or NULL for
 * the first n_index rows (<= 0: all).  Nothing is staged or copied: the frame-preparation kernels gather. */
int mdx_msd_push_frames_device(mdx_msd_t h, int group, const void *d_pos, int elem_bytes, int64_t n_frames,
                               int64_t n_total, const int32_t *index, int64_t n_index, int unwrap,
                               const double *dims, int zero_dims, const double *shift);
int mdx_msd_system_com_device(mdx_msd_t h, const void *d_pos, int elem_bytes, int64_t n_frames,
                              int64_t n_total, const int32_t *index, int64_t n_index, const double *masses,
                              int unwrap, const double *dims, int wrap, double *out);
/* With a grouping declared (mdx_msd_set_grouping) both mdx_msd_system_com_* variants return the
 * centre of mass of the molecules' CENTRES (wrapped into the box first when wrap != 0), each
 * weighted with its molecule's mass: Onsager(center=True, center_atom=False, center_wrap=True)
 * with residue / segment groupings (transport.py:1004-1014). */

/* ---- density profiles: per-axis histograms of positions (reference analysis/profile.py DensityProfile) -----------
 * Counts of points along the requested axes, per group, equal to numpy.histogram(x, n_bins, (0, L)) count for count
 * after the reference's `wrap` (x < 0 or x > L: x -= floor(x / L) * L), all in float64; coordinates that are not
 * finite are not counted.  Rows arrive in the order of the concatenated groups: group g holds points
 * [group_offsets[g], group_offsets[g+1]), group_offsets[0] == 0.  axes[n_axes] (distinct, 0..2) and n_bins[n_axes]
 * name the profiles; dims[3] are the fixed box lengths.  per_frame == 0: one total per (group, bin) over all
 * frames; else one row per frame.  Argument errors return MDX_ERR_INVALID_VALUE before any device is touched. */
typedef struct mdx_prof *mdx_prof_t;
int mdx_prof_create(mdx_prof_t *out, int dev, int n_groups, const int64_t *group_offsets, int n_axes,
                    const int32_t *axes, const int64_t *n_bins, const double *dims, int per_frame);
int mdx_prof_destroy(mdx_prof_t h);
/* Zeroes the counts, forgets the frames seen and the unwrap state of the recentring. */
int mdx_prof_reset(mdx_prof_t h);
/* Incoming rows become particles sorted molecule by molecule (CSR offsets[n_molecules + 1], masses per row) and
 * the points are the float64 mass-weighted centres, summed in row order and divided once; n_molecules must equal
 * the number of points of the groups (<= 0 removes the grouping).  Only before the first frame. */
int mdx_prof_set_grouping(mdx_prof_t h, int64_t n_molecules, const int64_t *offsets, const double *masses);
/* Recentring (profile.py:782-801): per frame, over all points, the reference's global unwrap (a displacement since
 * the previous frame of |d| >= dims / 2 changes the image count by -sign(d)), then every point is shifted by
 * scom - target, scom the centre of the unwrapped points of `group` weighted with masses[points of the group]; a
 * NaN component of target leaves that axis alone.  Frames must then be fed in analysis order; the result does not
 * depend on how they are split into calls.  group < 0 switches it off.  Only before the first frame. */
int mdx_prof_set_recenter(mdx_prof_t h, int group, const double *masses, const double *target);
/* Host float32 [n_frames][n][3] through the pinned ring. */
int mdx_prof_accumulate(mdx_prof_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3], read where they lie; index: host int32[n_index] rows of a
 * frame in incoming order, or NULL for all n_atoms rows.  Asynchronous (mdx_prof_synchronize). */
int mdx_prof_accumulate_device(mdx_prof_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                               const int32_t *index, int64_t n_index);
int mdx_prof_accumulate_traj(mdx_prof_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                             const int32_t *index, int64_t n_index);
int mdx_prof_synchronize(mdx_prof_t h);
/* out: int64 [n_groups][n_bins of the slot], or [n_groups][frames seen][n_bins] for per_frame engines. */
int mdx_prof_counts(mdx_prof_t h, int axis_slot, int64_t *out);
/* replicas: LDS copies of the counters the kernels use (8, 4, 2, 1), 0 = they bin straight into global memory. */
int mdx_prof_stats(mdx_prof_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int *replicas);
int mdx_prof_enable_timing(mdx_prof_t h, int on);
/* Caps the LDS copies of the counters at `replicas` (8, 4, 2, 1; fewer where they do not fit), 0 makes the kernels
 * bin straight into global memory, -1 restores the engine's own choice.  The counts do not depend on it; it exists
 * for measurements and tests.  Only before the first frame. */
int mdx_prof_set_replicas(mdx_prof_t h, int replicas);
/* Host-only plan queries (no device is touched), for tests and tools that must know where a call is cut.
 * mdx_feed_slab_frames: the frames a host-memory or trajectory-file call of n_frames frames stages at a time, for every
 * per-frame engine (rows: the caller's n on the host route, the file's n_atoms on the file route).
 * mdx_X_slab_frames: the frames an engine with n_points points, configured as the flags say, takes per kernel launch
 * inside one call; a call of more frames is cut into such slabs, whose results do not depend on the cut. */
int mdx_feed_slab_frames(int64_t n_frames, int64_t rows, int64_t *slab);
int mdx_prof_slab_frames(int64_t n_points, int grouped, int recenter, int64_t *slab);

/* ---- radii of gyration of polymer chains (reference analysis/polymer.py Gyradius, algorithm/molecule.py
 * radius_of_gyration) ------------------------------------------------------------------------------------------------
 * Rows arrive in the order of the concatenated groups: group g holds n_chains[g] * n_monomers[g] consecutive points,
 * a chain is n_monomers[g] consecutive points; masses float64, one per point in that order.  Per frame and chain, in
 * float64 with separate multiply and add (float32 coordinates are widened before any arithmetic):
 *     c = sum m r / sum m;   S_d = sum m (r_d - c_d)^2 over the centred coordinates (two passes; the one-pass form
 *     sum m r^2 - (sum m r)^2 / sum m is not used: it cancels for chains far from the origin);
 *     Rg = sqrt((S_x + S_y + S_z) / sum m);   Rg_x = sqrt((S_y + S_z) / sum m), Rg_y = sqrt((S_x + S_z) / sum m),
 *     Rg_z = sqrt((S_x + S_y) / sum m)   (the radii "around the axes" of molecule.py:529-544);
 * the value of a group is the mean over its chains.  Every sum, across lanes and across chains, has a fixed order and
 * no floating-point atomics are used, so the rows are bit-identical across the three input routes and across any
 * split of the frames into calls.  Argument errors return MDX_ERR_INVALID_VALUE before any device is touched. */
typedef struct mdx_gyr *mdx_gyr_t;
int mdx_gyr_create(mdx_gyr_t *out, int dev, int n_groups, const int64_t *n_chains, const int64_t *n_monomers,
                   const double *masses);
int mdx_gyr_destroy(mdx_gyr_t h);
/* Forgets the frames seen and the unwrap state (the next frame is again compared with `start`). */
int mdx_gyr_reset(mdx_gyr_t h);
/* Incoming rows become particles sorted monomer by monomer (CSR offsets[n_molecules + 1], masses per row) and the
 * points are the float64 mass-weighted centres, summed in row order and divided once; n_molecules must equal the
 * number of points of the groups (<= 0 removes the grouping).  Only before the first frame. */
int mdx_gyr_set_grouping(mdx_gyr_t h, int64_t n_molecules, const int64_t *offsets, const double *masses);
/* The reference's global unwrap (algorithm/topology.py `unwrap`) per frame and point coordinate: d = x - x_prev;
 * |d| >= dims / 2 moves the image count by -sign(d); x_prev becomes the raw x; the point used is x + image * dims, the
 * shift applied in float64.  Before the first frame x_prev = start (float64 [n_points][3]: the points of the first
 * analysed frame with every chain made whole) and the image counts are 0, so the first frame recovers the make-whole
 * images itself.  Frames must then be fed in analysis order; the result does not depend on how they are split into
 * calls.  dims == NULL switches it off.  Only before the first frame. */
int mdx_gyr_set_unwrap(mdx_gyr_t h, const double *dims, const double *start);
/* Host float32 [n_frames][n][3] through the pinned ring. */
int mdx_gyr_accumulate(mdx_gyr_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3], read where they lie; index: host int32[n_index] rows of a
 * frame in incoming order, or NULL for all n_atoms rows.  Asynchronous (mdx_gyr_synchronize). */
int mdx_gyr_accumulate_device(mdx_gyr_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                              const int32_t *index, int64_t n_index);
int mdx_gyr_accumulate_traj(mdx_gyr_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index);
int mdx_gyr_synchronize(mdx_gyr_t h);
/* out: float64 [n_groups][frames seen][4]: the mean over the group's chains of Rg, Rg_x, Rg_y, Rg_z. */
int mdx_gyr_result(mdx_gyr_t h, double *out);
int mdx_gyr_stats(mdx_gyr_t h, int64_t *launches, double *kernel_ms, int64_t *frames);
int mdx_gyr_enable_timing(mdx_gyr_t h, int on);
/* Host-only (mdx_prof_slab_frames): n_chains chains in all, of n_points points in all. */
int mdx_gyr_slab_frames(int64_t n_chains, int64_t n_points, int grouped, int unwrap, int64_t *slab);

/* ---- per-chain linear projections: Rouse mode amplitudes (analysis/polymer.py RouseModes; no counterpart in the
 * reference) ---------------------------------------------------------------------------------------------------------
 * Rows arrive as for the gyration engine: group g holds n_chains[g] * n_monomers[g] consecutive points, a chain is
 * n_monomers[g] consecutive points.  weights: float64 [sum_g n_rows * n_monomers[g]], group after group, row-major
 * (w[g][k][n]); they must be finite.  Per frame, chain c and weight row k, in float64 with separate multiply and add
 * (float32 coordinates are widened before any arithmetic):
 *     x_n = (double)r_n + image_n * L,    X[c][k] = sum_n w[g][k][n] * x_n,
 * the products added one after the other in the order n = 0, 1, ... starting from +0.0 — a plain host loop gives the
 * same bits.  No floating-point atomics: the amplitudes are bit-identical across the three input routes and across
 * any split of the frames into calls.  They stay in HBM as double [frames][S][3], S = sum_g n_rows * n_chains[g],
 * series series0[g] + k * n_chains[g] + c with series0[g] = sum_{g' < g} n_rows * n_chains[g']: the chains of one
 * (group, row) are a contiguous range of a frame, the shape mdx_msd_push_device(group, d_pos, n_total = S, first,
 * count) takes.  Argument errors return MDX_ERR_INVALID_VALUE before any device is touched. */
typedef struct mdx_rouse *mdx_rouse_t;
int mdx_rouse_create(mdx_rouse_t *out, int dev, int n_groups, const int64_t *n_chains, const int64_t *n_monomers,
                     int64_t n_rows, const double *weights);
int mdx_rouse_destroy(mdx_rouse_t h);
/* Forgets the frames seen and the unwrap state (the next frame is again compared with `start`). */
int mdx_rouse_reset(mdx_rouse_t h);
/* Room for n_frames frames in all, allocated once (without it the buffer doubles as frames arrive). */
int mdx_rouse_reserve(mdx_rouse_t h, int64_t n_frames);
/* As mdx_gyr_set_grouping / mdx_gyr_set_unwrap: float64 centres of mass of monomers formed on the device; the global
 * unwrap with the same rule, the same carried state and x_prev = start before the first frame. */
int mdx_rouse_set_grouping(mdx_rouse_t h, int64_t n_molecules, const int64_t *offsets, const double *masses);
int mdx_rouse_set_unwrap(mdx_rouse_t h, const double *dims, const double *start);
/* The three input routes of the gyration engine: host float32 [n_frames][n][3] through the pinned ring; frames in
 * HBM read where they lie (asynchronous: mdx_rouse_synchronize); frames of a trajectory file. */
int mdx_rouse_accumulate(mdx_rouse_t h, const float *pos, int64_t n, int64_t n_frames);
int mdx_rouse_accumulate_device(mdx_rouse_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                                const int32_t *index, int64_t n_index);
int mdx_rouse_accumulate_traj(mdx_rouse_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                              const int32_t *index, int64_t n_index);
int mdx_rouse_synchronize(mdx_rouse_t h);
/* out: float64 [frames seen][S][3]. */
int mdx_rouse_result(mdx_rouse_t h, double *out);
/* Waits for the engine's stream and returns the amplitudes where they lie; the pointer is valid until the next
 * accumulate, reset or destroy of the handle. */
int mdx_rouse_device_result(mdx_rouse_t h, const double **d_ptr, int64_t *n_frames, int64_t *n_series);
int mdx_rouse_stats(mdx_rouse_t h, int64_t *launches, double *kernel_ms, int64_t *frames);
int mdx_rouse_enable_timing(mdx_rouse_t h, int on);
/* Host-only (mdx_prof_slab_frames). */
int mdx_rouse_slab_frames(int64_t n_points, int grouped, int unwrap, int64_t *slab);

/* ---- chain internal distances and bond-orientation correlations (analysis/polymer.py InternalDistances; no
 * counterpart in the reference) --------------------------------------------------------------------------------------
 * Rows arrive as for the gyration engine: group g holds n_chains[g] * n_monomers[g] consecutive points, a chain is
 * n_monomers[g] >= 2 consecutive points.  Per frame and group of M chains of N points, in float64 with separate
 * multiply and add (float32 coordinates are widened before any arithmetic):
 *     R2(s) = sum_c sum_i |x_{c,i+s} - x_{c,i}|^2 / (M (N - s)),        s = 1 ... N-1,   |d|^2 = (dx dx + dy dy) + dz dz
 *     u_i   = (x_{i+1} - x_i) / sqrt(|x_{i+1} - x_i|^2)                 (0 for a bond of no length)
 *     C(s)  = sum_c sum_i u_{c,i} . u_{c,i+s} / (M (N - 1 - s)),        s = 0 ... N-2.
 * Every sum has a fixed order that depends on (M, N) alone (csrc/mdx_msid_device.hpp: i ascending per chain and
 * separation, chains ascending within a unit, units ascending, one division) and no floating-point atomics are used,
 * so the rows are bit-identical across the three input routes and across any split of the frames into calls or
 * slabs.  A frame's rows: for group g at offset 2 sum_{h<g} (N_h - 1), first the N_g - 1 values R2(1 ... N-1), then
 * the N_g - 1 values C(0 ... N-2).  Argument errors return MDX_ERR_INVALID_VALUE before any device is touched. */
typedef struct mdx_msid *mdx_msid_t;
int mdx_msid_create(mdx_msid_t *out, int dev, int n_groups, const int64_t *n_chains, const int64_t *n_monomers);
int mdx_msid_destroy(mdx_msid_t h);
/* Forgets the frames seen and the unwrap state (the next frame is again compared with `start`). */
int mdx_msid_reset(mdx_msid_t h);
/* Room for n_frames frames in all, allocated once (without it the buffer doubles as frames arrive). */
int mdx_msid_reserve(mdx_msid_t h, int64_t n_frames);
/* As mdx_gyr_set_grouping / mdx_gyr_set_unwrap.  mdx_msid_set_unwrap excludes mdx_msid_set_whole. */
int mdx_msid_set_grouping(mdx_msid_t h, int64_t n_molecules, const int64_t *offsets, const double *masses);
int mdx_msid_set_unwrap(mdx_msid_t h, const double *dims, const double *start);
/* Every chain made whole in every frame by itself, in float64 on the points (the monomer centres under a grouping):
 * x_0 = r_0;  d = r_{n+1} - r_n per component;  |d| >= dims / 2 moves d by -sign(d) * dims;  x_{n+1} = x_n + d.
 * Bonds must be shorter than half the shortest box length.  No state is carried between frames, so frames may be
 * fed in any order and shard across ranks.  dims == NULL switches it off.  Only before the first frame; excludes
 * mdx_msid_set_unwrap. */
int mdx_msid_set_whole(mdx_msid_t h, const double *dims);
/* The three input routes of the gyration engine. */
int mdx_msid_accumulate(mdx_msid_t h, const float *pos, int64_t n, int64_t n_frames);
int mdx_msid_accumulate_device(mdx_msid_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                               const int32_t *index, int64_t n_index);
int mdx_msid_accumulate_traj(mdx_msid_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                             const int32_t *index, int64_t n_index);
int mdx_msid_synchronize(mdx_msid_t h);
/* out: float64 [frames seen][2 sum_g (N_g - 1)]. */
int mdx_msid_result(mdx_msid_t h, double *out);
int mdx_msid_stats(mdx_msid_t h, int64_t *launches, double *kernel_ms, int64_t *frames);
int mdx_msid_enable_timing(mdx_msid_t h, int on);
/* Host-only (mdx_prof_slab_frames): the chain layout of mdx_msid_create, from which the per-unit partial sums of a
 * frame follow; whole and unwrap exclude each other. */
int mdx_msid_slab_frames(int n_groups, const int64_t *n_chains, const int64_t *n_monomers, int grouped, int whole,
                         int unwrap, int64_t *slab);

/* ---- instantaneous dipole moments (reference analysis/electrostatics.py DipoleMoment) ------------------------------
 * Rows arrive in the order of the concatenated groups: group g holds n_points[g] consecutive points; charges float64,
 * one per point in that order, finite.  Per frame, group and component, in float64 with separate multiply and add
 * (float32 coordinates are widened before any arithmetic):
 *     M_gd = sum over the group's points of q_i * (r_id + image_id * L_d)          (image = 0 without unwrap).
 * Every sum has a fixed order that depends on the group sizes alone (csrc/mdx_dipole_device.hpp: tiles of points that
 * never span two groups, added in tile order) and no floating-point atomics are used, so the rows are bit-identical
 * across the three input routes and across any split of the frames into calls or slabs.  The positions are read from
 * HBM once and nothing of size frames x points is written.  Argument errors return MDX_ERR_INVALID_VALUE before any
 * device is touched. */
typedef struct mdx_dip *mdx_dip_t;
int mdx_dip_create(mdx_dip_t *out, int dev, int n_groups, const int64_t *n_points, const double *charges);
int mdx_dip_destroy(mdx_dip_t h);
/* Forgets the frames seen and the unwrap state (the next frame is again compared with `start`). */
int mdx_dip_reset(mdx_dip_t h);
/* The reference's global unwrap (algorithm/topology.py `unwrap`) per frame and point coordinate: d = x - x_prev;
 * |d| >= dims / 2 moves the image count by -sign(d); x_prev becomes the raw x; the point used is x + image * dims, the
 * shift applied in float64.  Before the first frame x_prev = start (float64 [n_points][3]: the points of the first
 * analysed frame with every molecule made whole) and the image counts are 0.  The state carries from slab to slab and
 * from call to call; frames must be fed in analysis order.  dims == NULL switches it off.  Only before the first
 * frame. */
int mdx_dip_set_unwrap(mdx_dip_t h, const double *dims, const double *start);
/* Frames per kernel launch, at most (1 ... 32768; 0 restores the default, which bounds the scratch of a launch).
 * The rows do not depend on it; tests use it to make a few frames cross several slabs. */
int mdx_dip_set_slab_frames(mdx_dip_t h, int64_t frames);
/* The plan of the next call, as mdx_rdf_plan reports the launch: *slab_frames = the frames a kernel launch takes at
 * most (the slab asked for, or the default: 32768, or fewer where 256 MiB of history or scratch hold fewer frames;
 * a lag engine limits it by the ring once the ring is sized), *ring_frames = the frames the ring of a lag engine
 * holds (max(lags) + slab, decided before the first frame of a pass; 0 for an engine without a ring).  Computed by
 * the functions the accumulate path calls.  Needs no device and reads no frame. */
int mdx_dip_plan(mdx_dip_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Host float32 [n_frames][n][3] through the pinned ring. */
int mdx_dip_accumulate(mdx_dip_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3], read where they lie; index: host int32[n_index] rows of a
 * frame in incoming order, or NULL for all n_atoms rows.  Asynchronous (mdx_dip_synchronize). */
int mdx_dip_accumulate_device(mdx_dip_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                              const int32_t *index, int64_t n_index);
int mdx_dip_accumulate_traj(mdx_dip_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index);
int mdx_dip_synchronize(mdx_dip_t h);
/* out: float64 [n_groups][frames seen][3]: the dipole moment of every group in every frame. */
int mdx_dip_result(mdx_dip_t h, double *out);
int mdx_dip_stats(mdx_dip_t h, int64_t *launches, double *kernel_ms, int64_t *frames);
int mdx_dip_enable_timing(mdx_dip_t h, int on);

/* ---- self van Hove function and displacement moments -----------------------------------------------------------------
 * Rows arrive in the order of the concatenated groups: group g holds n_points[g] consecutive points (a group may be
 * empty, all of them together may not).  Analysed frames are numbered f = 0, 1, ... in the order fed; lags: strictly
 * increasing, non-negative frame offsets (0 allowed).  Per point, lag k and frame f >= lags[k], in float64 with
 * separate multiply and add (float32 coordinates are widened before any arithmetic):
 *     x(f) = r(f) + image(f) * L (image = 0 without unwrap);  d = x(f) - x(f - lag), +0.0 for a dropped component;
 *     r2 = (dx*dx + dy*dy) + dz*dz;  r = sqrt(r2);  counts[k][g][b] += 1 where edges[b] <= r < edges[b+1] (the last
 *     bin closed on the right; r outside the edges or not finite is not counted);  m2[k][p] += r2, m4[k][p] += r2*r2.
 * edges: float64 [n_bins + 1], the caller's numpy.linspace(r_min, r_max, n_bins + 1) as for mdx_rdf_create; the counts
 * then equal numpy.histogram(r, n_bins, (r_min, r_max)) count for count.  zero_dims: bit k drops component k, as for
 * mdx_msd_push.  The accumulator of a (lag, point) receives its terms in frame order and a group's moments add the
 * accumulators of its points in row order (csrc/mdx_vanhove_device.hpp); no floating-point atomics are used, so
 * counts and moments are bit-identical across the three input routes, across any split of the frames into calls or
 * slabs, and after a reset.  The engine keeps max(lags) + one slab of float64 frames in HBM (MDX_ERR_OUT_OF_MEMORY
 * when that does not fit).  A handle touches its device with the first frame: mdx_vh_create and every argument error
 * (MDX_ERR_INVALID_VALUE) need none. */
typedef struct mdx_vh *mdx_vh_t;
int mdx_vh_create(mdx_vh_t *out, int dev, int n_groups, const int64_t *n_points, int n_bins, const double *edges,
                  int n_lags, const int64_t *lags, int zero_dims);
int mdx_vh_destroy(mdx_vh_t h);
/* Forgets the frames seen, the history and the unwrap state and zeroes counts and moments. */
int mdx_vh_reset(mdx_vh_t h);
/* The reference's global unwrap per point coordinate, as mdx_dip_set_unwrap; the first analysed frame is its own
 * start with image 0 (a displacement does not depend on the starting image).  dims: float64 [3] box lengths, or NULL:
 * off.  Only before the first frame. */
int mdx_vh_set_unwrap(mdx_vh_t h, const double *dims);
/* Frames per kernel launch, at most (1 ... 32768; 0 restores the default, which bounds the history), as
 * mdx_dip_set_slab_frames.  The results do not depend on it.  Only before the first frame. */
int mdx_vh_set_slab_frames(mdx_vh_t h, int64_t frames);
/* As mdx_dip_plan. */
int mdx_vh_plan(mdx_vh_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Host float32 [n_frames][n][3] through the pinned ring. */
int mdx_vh_accumulate(mdx_vh_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in incoming
 * order, or NULL for all n_atoms rows.  Asynchronous (mdx_vh_synchronize). */
int mdx_vh_accumulate_device(mdx_vh_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                             const int32_t *index, int64_t n_index);
int mdx_vh_accumulate_traj(mdx_vh_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                           const int32_t *index, int64_t n_index);
int mdx_vh_synchronize(mdx_vh_t h);
/* counts: int64 [n_lags][n_groups][n_bins]; moments: float64 [n_lags][n_groups][2] = sum r2, sum r4 over the group's
 * points and every frame pair of the lag; may be NULL. */
int mdx_vh_result(mdx_vh_t h, int64_t *counts, double *moments);
/* out: float64 [n_lags][n_points][2]: the accumulators of every point. */
int mdx_vh_point_moments(mdx_vh_t h, double *out);
/* evaluations: displacements formed so far (frame pairs x points, summed over the lags). */
int mdx_vh_stats(mdx_vh_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations);
int mdx_vh_enable_timing(mdx_vh_t h, int on);

/* ---- distinct van Hove function G_d(r, t) ---------------------------------------------------------------------------
 * Set 1 holds n1 rows, set 2 holds n2; incoming rows are set 1 then set 2, or set 1 alone with `same` (both are one
 * set, n1 == n2, the pair i == j is left out).  dims: float64 [3] box lengths, the same for every frame.  Analysed
 * frames are numbered f = 0, 1, ... in the order fed; lags: strictly increasing, non-negative; the frame pairs of lag k
 * are (f0, f0 + lags[k]) with f0 % origin_step == 0.  Per frame pair and pair (i of set 1 at f0, j of set 2 at
 * f0 + lag), in float64 with separate multiply and add (float32 coordinates are widened before any arithmetic):
 *     d = x2_j - x1_i;  w = d - L * rint(d * (1.0 / L)), +0.0 for a dropped component;
 *     r2 = (wx*wx + wy*wy) + wz*wz;  r = sqrt(r2);  counts[k][b] += 1 where edges[b] <= r < edges[b+1] (the last bin
 *     closed on the right; r outside the edges or not finite is not counted).
 * edges: float64 [n_bins + 1], the caller's numpy.linspace(r_min, r_max, n_bins + 1); the counts then equal
 * numpy.histogram(r, n_bins, (r_min, r_max)) count for count.  edges[n_bins] may not exceed half the shortest kept box
 * length.  zero_dims: bit k drops component k.  There is no unwrap (the minimum image of a difference needs none) and
 * no floating-point atomic: the counts are integers and identical across the three input routes, across any split of
 * the frames into calls or slabs, and after a reset (csrc/mdx_vanhove_distinct_device.hpp).  The engine keeps
 * max(lags) + one slab of float32 frames in HBM.  A handle touches its device with the first frame: mdx_vhd_create and
 * every argument error (MDX_ERR_INVALID_VALUE) need none. */
typedef struct mdx_vhd *mdx_vhd_t;
int mdx_vhd_create(mdx_vhd_t *out, int dev, int64_t n1, int64_t n2, int same, int n_bins, const double *edges,
                   int n_lags, const int64_t *lags, int64_t origin_step, const double *dims, int zero_dims);
int mdx_vhd_destroy(mdx_vhd_t h);
/* Forgets the frames seen and the history and zeroes the counts. */
int mdx_vhd_reset(mdx_vhd_t h);
/* Frames per kernel launch, at most (1 ... 32768; 0 restores the default, which bounds the history).  The results do
 * not depend on it.  Only before the first frame. */
int mdx_vhd_set_slab_frames(mdx_vhd_t h, int64_t frames);
/* As mdx_dip_plan. */
int mdx_vhd_plan(mdx_vhd_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Host float32 [n_frames][n][3] through the pinned ring; n = n1 + n2, or n1 with same. */
int mdx_vhd_accumulate(mdx_vhd_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in incoming
 * order, or NULL for all n_atoms rows.  Asynchronous (mdx_vhd_synchronize). */
int mdx_vhd_accumulate_device(mdx_vhd_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                              const int32_t *index, int64_t n_index);
int mdx_vhd_accumulate_traj(mdx_vhd_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index);
int mdx_vhd_synchronize(mdx_vhd_t h);
/* counts: int64 [n_lags][n_bins]. */
int mdx_vhd_result(mdx_vhd_t h, int64_t *counts);
/* evaluations: the contract's pair count so far, sum over the lags of origins x (n1 * n2 - (same ? n1 : 0)). */
int mdx_vhd_stats(mdx_vhd_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations);
int mdx_vhd_enable_timing(mdx_vhd_t h, int on);

/* ---- pair residence: contact survival functions --------------------------------------------------------------------
 * Sets, rows, `same`, dims, frames, lags, origin_step and zero_dims as for mdx_vhd_*.  Per frame f and pair (i of set 1,
 * j of set 2, both at frame f; with `same` the ordered pairs (i, j) and (j, i) both count and i == j does not), in
 * float64 with separate multiply and add (float32 coordinates are widened before any arithmetic):
 *     d = x2_j - x1_i;  w = d - L * rint(d * (1.0 / L)), +0.0 for a dropped component;
 *     r2 = (wx*wx + wy*wy) + wz*wz;  the pair is a contact where r2 <= cutoff * cutoff (a NaN r2 is none).
 * With C(f) the set of contacts of frame f:  contacts[f] = |C(f)|, and per lag k, summed over the origins f0 of the
 * lag (f0 % origin_step == 0, f0 + lags[k] analysed):
 *     origin_counts[k] += |C(f0)|;  intermittent[k] += |C(f0) & C(f0 + lags[k])|;
 *     continuous[k] += |C(f0) & C(f0 + 1) & ... & C(f0 + lags[k])|  (every analysed frame in between).
 * cutoff: positive, finite, at most half the shortest kept box length.  max_neighbors (1 ... 64): the contacts a row i
 * may hold in one frame.  A row that would hold more is never truncated silently: mdx_prs_synchronize, mdx_prs_result
 * and mdx_prs_contacts fail with MDX_ERR_INVALID_VALUE (the message names max_neighbors and the largest row seen)
 * until mdx_prs_reset.  continuous == 0: only the frames a lag away from an origin are visited and continuous[] stays
 * zero.  All results are integers and identical across the three input routes, across any split of the frames into
 * calls or slabs, and after a reset (csrc/mdx_residence_device.hpp).  The engine keeps max(lags) + one slab of frames
 * of contact lists in HBM, (max_neighbors + 3) * n1 * 4 bytes each.  A handle touches its device with the first frame:
 * mdx_prs_create and every argument error (MDX_ERR_INVALID_VALUE) need none. */
typedef struct mdx_prs *mdx_prs_t;
int mdx_prs_create(mdx_prs_t *out, int dev, int64_t n1, int64_t n2, int same, double cutoff, int n_lags,
                   const int64_t *lags, int64_t origin_step, const double *dims, int zero_dims, int max_neighbors,
                   int continuous);
int mdx_prs_destroy(mdx_prs_t h);
/* Forgets the frames seen, the history and an overflowing row, and zeroes the results. */
int mdx_prs_reset(mdx_prs_t h);
/* Frames per kernel launch, at most (1 ... 32768; 0 restores the default, which bounds the history).  The results do
 * not depend on it.  Only before the first frame. */
int mdx_prs_set_slab_frames(mdx_prs_t h, int64_t frames);
/* As mdx_dip_plan. */
int mdx_prs_plan(mdx_prs_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Host float32 [n_frames][n][3] through the pinned ring; n = n1 + n2, or n1 with same. */
int mdx_prs_accumulate(mdx_prs_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in incoming
 * order, or NULL for all n_atoms rows.  Asynchronous (mdx_prs_synchronize). */
int mdx_prs_accumulate_device(mdx_prs_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                              const int32_t *index, int64_t n_index);
int mdx_prs_accumulate_traj(mdx_prs_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index);
int mdx_prs_synchronize(mdx_prs_t h);
/* intermittent, continuous, origin_counts: int64 [n_lags] each. */
int mdx_prs_result(mdx_prs_t h, int64_t *intermittent, int64_t *continuous, int64_t *origin_counts);
/* out: int64 [n], the contacts of the first n frames seen. */
int mdx_prs_contacts(mdx_prs_t h, int64_t *out, int64_t n);
/* evaluations: the contract's pair count so far, frames x (n1 * n2 - (same ? n1 : 0)); max_row: the most contacts a
 * row held in one frame (beyond max_neighbors: the results are refused). */
int mdx_prs_stats(mdx_prs_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *max_row);
int mdx_prs_enable_timing(mdx_prs_t h, int on);

/* ------------------------------------------------------------------ ion clusters
 * Per analysed frame the connected components of the bond graph of n rows: the atoms of group 0, then group 1, ...;
 * species[n] (int32, 0 ... n_species - 1, n_species <= 8) names the group of a row.  Box, minimum image and r2 are
 * those of mdx_prs_*: float32 rows, one constant orthorhombic box dims[3], zero_dims (bit c set: component c takes no
 * part), everything in float64, one operation at a time.  cutoff[n_species * n_species] is a symmetric table of
 * non-negative finite values with at least one positive entry, the largest at most half the shortest kept box length;
 * rows i != j are bonded iff r2 <= cutoff[a][b]^2 with a, b their species, and never where cutoff[a][b] == 0.
 * label[f][i] is the smallest row of the component of i.  Results, all integers:
 *     per frame: bonds (unordered pairs), n_clusters, largest (rows of the largest component), sum_squares
 *                (sum over the components of size^2);
 *     over the frames seen: size_counts[s], s = 0 ... n (components of s rows), species_counts[g][s] (rows of species
 *                g in a component of s rows; sum_g species_counts[g][s] == s * size_counts[s]).
 * max_neighbors (1 ... 64): the bonds a row may hold in one frame, both directions counted.  A row that would hold
 * more is never truncated silently: mdx_clu_synchronize and every result call fail with MDX_ERR_INVALID_VALUE (the
 * message names max_neighbors and the largest row seen) until mdx_clu_reset.  The components are found on the device
 * from the bond lists by sweeps of hooking and pointer jumping (csrc/mdx_cluster_device.hpp); a slab that has not
 * settled after n + 1 sweeps is MDX_ERR_INTERNAL.  All results are identical across the three input routes, across
 * any split of the frames into calls or slabs, and after a reset.  Frames are independent: nothing but the results
 * outlives a slab.  A handle touches its device with the first frame: mdx_clu_create and every argument error
 * (MDX_ERR_INVALID_VALUE) need none. */
typedef struct mdx_clu *mdx_clu_t;
int mdx_clu_create(mdx_clu_t *out, int dev, int64_t n, const int32_t *species, int n_species, const double *cutoff,
                   const double *dims, int zero_dims, int max_neighbors, int keep_labels);
int mdx_clu_destroy(mdx_clu_t h);
/* Forgets the frames seen and an overflowing row, and zeroes the results. */
int mdx_clu_reset(mdx_clu_t h);
/* Frames per kernel launch, at most (1 ... 32768; 0 restores the default, which bounds the lists in HBM).  The results
 * do not depend on it.  Only before the first frame. */
int mdx_clu_set_slab_frames(mdx_clu_t h, int64_t frames);
/* As mdx_dip_plan. */
int mdx_clu_plan(mdx_clu_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Host float32 [n_frames][n][3] through the pinned ring. */
int mdx_clu_accumulate(mdx_clu_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in incoming
 * order, or NULL for all n_atoms rows. */
int mdx_clu_accumulate_device(mdx_clu_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                              const int32_t *index, int64_t n_index);
int mdx_clu_accumulate_traj(mdx_clu_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index);
int mdx_clu_synchronize(mdx_clu_t h);
/* size_counts: int64 [n + 1]; species_counts: int64 [n_species][n + 1]. */
int mdx_clu_result(mdx_clu_t h, int64_t *size_counts, int64_t *species_counts);
/* bonds, n_clusters, largest, sum_squares: int64 [n] each, the first n frames seen. */
int mdx_clu_frames(mdx_clu_t h, int64_t *bonds, int64_t *n_clusters, int64_t *largest, int64_t *sum_squares,
                   int64_t n);
/* out: int32 [n][points], the labels of the first n frames seen; only with keep_labels. */
int mdx_clu_labels(mdx_clu_t h, int32_t *out, int64_t n);
/* evaluations: the contract's pair count so far, frames x n (n - 1) / 2; max_row: the most bonds a row held in one
 * frame (beyond max_neighbors: the results are refused); sweeps: the labelling sweeps so far. */
int mdx_clu_stats(mdx_clu_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *max_row, int64_t *sweeps);
int mdx_clu_enable_timing(mdx_clu_t h, int on);

/* ------------------------------------------------------------------ angular distributions
 * Per analysed frame the angles ligand-center-ligand in the first shell of every center.  The rows of a frame are the
 * n_centers centers, then the ligands group by group: n_species groups (1 ... 4) of ligand_sizes[g] rows; species(j)
 * of a ligand follows from the sizes.  With same, n_species == 1, ligand_sizes[0] == n_centers, the ligands are the
 * centers themselves, the rows arrive once and j == i never counts.  Box, minimum image and r2 are those of
 * mdx_prs_*: float32 rows, one constant orthorhombic box dims[3], zero_dims (bit c set: component c takes no part),
 * everything in float64, one operation at a time.  For center i and ligand j:
 *     d = x_j - x_i;  w = d - L * rint(d * (1.0 / L)), +0.0 for a dropped component;  r2 = (wx*wx + wy*wy) + wz*wz;
 *     j is a neighbour of i iff r2 <= cutoff[species(j)]^2 (a NaN r2 is none).
 * cutoff[n_species]: positive, finite, the largest at most half the shortest kept box length.  For every center and
 * every unordered pair {j, k}, j != k, of its neighbours:
 *     dot = (w_ijx*w_ikx + w_ijy*w_iky) + w_ijz*w_ikz;  c = dot / sqrt(r2_ij * r2_ik)
 * (one multiply, one correctly rounded sqrt, one correctly rounded divide; symmetric in j and k).  thresholds is
 * t[0 ... n_bins], strictly decreasing (anything else is MDX_ERR_INVALID_VALUE); the bin of a triplet is
 * b = #{m in 1 ... n_bins - 1 : c <= t[m]}, so bin b holds t[b + 1] < c <= t[b], the first bin also takes c > t[0] and
 * the last also c <= t[n_bins]; only the inner thresholds are compared.  A NaN c (a ligand on its center, r2 == 0)
 * goes into no bin and adds 1 to degenerate[p].  Results, all integers:
 *     counts[p][b] and degenerate[p], p = a*G - a*(a-1)/2 + (b-a) the unordered pair of ligand species a <= b of the
 *                two ligands, P = G (G + 1) / 2 of them (G = n_species);
 *     coordination[g][m], m = 0 ... max_neighbors: the (frame, center) cases with exactly m neighbours of species g.
 * max_neighbors (1 ... 64): the neighbours of all species a center may hold in one frame; exactly full is no error.
 * A center that would hold more is never truncated silently: mdx_ang_synchronize and mdx_ang_result fail with
 * MDX_ERR_INVALID_VALUE (the message names max_neighbors and the largest row seen) until mdx_ang_reset.  All results
 * are identical across the three input routes, across any split of the frames into calls or slabs, and after a reset
 * (csrc/mdx_angle_device.hpp).  Frames are independent: nothing but the results outlives a slab.  Every (center,
 * ligand) pair is evaluated, there is no cell list.  A handle touches its device with the first frame: mdx_ang_create
 * and every argument error (MDX_ERR_INVALID_VALUE) need none. */
typedef struct mdx_ang *mdx_ang_t;
int mdx_ang_create(mdx_ang_t *out, int dev, int64_t n_centers, int n_species, const int64_t *ligand_sizes, int same,
                   const double *cutoff, int64_t n_bins, const double *thresholds, const double *dims, int zero_dims,
                   int max_neighbors);
int mdx_ang_destroy(mdx_ang_t h);
/* Forgets the frames seen and an overflowing row, and zeroes the results. */
int mdx_ang_reset(mdx_ang_t h);
/* Frames per kernel launch, at most (1 ... 32768; 0 restores the default, which bounds the lists in HBM).  The results
 * do not depend on it.  Only before the first frame. */
int mdx_ang_set_slab_frames(mdx_ang_t h, int64_t frames);
/* As mdx_dip_plan. */
int mdx_ang_plan(mdx_ang_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Host float32 [n_frames][n][3] through the pinned ring; n = n_centers + the ligands, or n_centers with same. */
int mdx_ang_accumulate(mdx_ang_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in incoming
 * order, or NULL for all n_atoms rows. */
int mdx_ang_accumulate_device(mdx_ang_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                              const int32_t *index, int64_t n_index);
int mdx_ang_accumulate_traj(mdx_ang_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index);
int mdx_ang_synchronize(mdx_ang_t h);
/* counts: int64 [P][n_bins]; degenerate: int64 [P]; coordination: int64 [n_species][max_neighbors + 1]. */
int mdx_ang_result(mdx_ang_t h, int64_t *counts, int64_t *degenerate, int64_t *coordination);
/* evaluations: the contract's pair count so far, frames x (n_centers * ligands - (same ? n_centers : 0)); triplets:
 * sum counts + sum degenerate; max_row: the most neighbours a center held in one frame (beyond max_neighbors: the
 * results are refused). */
int mdx_ang_stats(mdx_ang_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *triplets, int64_t *max_row);
int mdx_ang_enable_timing(mdx_ang_t h, int on);

/* ---- orientational relaxation: P1 / P2 reorientation of unit vectors and their order tensor ----------------------------
 * A frame delivers n_rows points; pairs: int32 [V][2] row numbers (tail, head) of the V vectors, tail != head; group g
 * holds n_vectors[g] consecutive vectors (a group may be empty, all of them together may not).  Analysed frames are
 * numbered f = 0, 1, ... in the order fed; lags: strictly increasing, non-negative frame offsets (0 allowed).  In
 * float64 with separate multiply and add (float32 coordinates are widened before any arithmetic), per vector and frame:
 *     d = x_head - x_tail;  w = d - L * rint(d * (1.0 / L)) with a box (mdx_ori_set_box), else w = d; +0.0 for a
 *     dropped component;  n2 = (wx*wx + wy*wy) + wz*wz;  u = w / sqrt(n2)  (sqrt and divide correctly rounded);
 * per vector v, lag k and frame f >= lags[k]:
 *     c = (ux(f)*ux(f-lag) + uy(f)*uy(f-lag)) + uz(f)*uz(f-lag);  acc[k][v][0] += c;  acc[k][v][1] += 1.5*(c*c) - 0.5;
 * and per frame f, group g and product ab = xx, xy, xz, yy, yz, zz:  frame_sums[f][g][ab] = sum of ua*ub.
 * zero_dims: bit k drops component k.  The accumulator of a (lag, vector) receives its terms in frame order, a group's
 * sums add the accumulators of its vectors in row order, and the products are added per tile of 64 vectors in row
 * order and then per group in tile order (csrc/mdx_orient_device.hpp); no floating-point atomics are used, so every
 * result is bit-identical across the three input routes, across any split of the frames into calls or slabs, and
 * after a reset.  A vector with n2 == 0 or n2 not finite has no direction: it is never averaged silently, and
 * mdx_ori_synchronize, mdx_ori_result, mdx_ori_vector_sums and mdx_ori_frame_sums fail with MDX_ERR_INVALID_VALUE
 * (the message counts such vectors) until mdx_ori_reset.  The engine keeps max(lags) + one slab of float64 frames of
 * unit vectors in HBM (MDX_ERR_OUT_OF_MEMORY when that does not fit).  A handle touches its device with the first
 * frame: mdx_ori_create and every argument error (MDX_ERR_INVALID_VALUE) need none. */
typedef struct mdx_ori *mdx_ori_t;
int mdx_ori_create(mdx_ori_t *out, int dev, int n_groups, const int64_t *n_vectors, int64_t n_rows,
                   const int32_t *pairs, int n_lags, const int64_t *lags, int zero_dims);
int mdx_ori_destroy(mdx_ori_t h);
/* Forgets the frames seen, the history and the degenerate vectors and zeroes the sums. */
int mdx_ori_reset(mdx_ori_t h);
/* One constant orthorhombic box for the minimum image of head - tail.  dims: float64 [3] box lengths, or NULL: none
 * (molecules that are whole already).  Only before the first frame. */
int mdx_ori_set_box(mdx_ori_t h, const double *dims);
/* Frames per kernel launch, at most (1 ... 32768; 0 restores the default, which bounds the history), as
 * mdx_vh_set_slab_frames.  The results do not depend on it.  Only before the first frame. */
int mdx_ori_set_slab_frames(mdx_ori_t h, int64_t frames);
/* As mdx_dip_plan. */
int mdx_ori_plan(mdx_ori_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Host float32 [n_frames][n][3] through the pinned ring; n = n_rows. */
int mdx_ori_accumulate(mdx_ori_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in the order the
 * pairs name them, or NULL for all n_atoms rows.  Asynchronous (mdx_ori_synchronize). */
int mdx_ori_accumulate_device(mdx_ori_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                              const int32_t *index, int64_t n_index);
int mdx_ori_accumulate_traj(mdx_ori_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index);
int mdx_ori_synchronize(mdx_ori_t h);
/* sums: float64 [n_lags][n_groups][2] = sum c, sum 1.5*c*c - 0.5 over the group's vectors and every frame pair of the
 * lag. */
int mdx_ori_result(mdx_ori_t h, double *sums);
/* out: float64 [n_lags][V][2]: the accumulators of every vector. */
int mdx_ori_vector_sums(mdx_ori_t h, double *out);
/* out: float64 [n][n_groups][6], the product sums of the first n frames seen. */
int mdx_ori_frame_sums(mdx_ori_t h, double *out, int64_t n);
/* evaluations: dot products formed so far (frame pairs x vectors, summed over the lags); degenerate: vectors without
 * a direction seen since the last reset (not zero: the results are refused). */
int mdx_ori_stats(mdx_ori_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *degenerate);
int mdx_ori_enable_timing(mdx_ori_t h, int on);

/* ---- bond-orientational order: Steinhardt q_l and the neighbour-averaged qbar_l of every center -----------------
 * Incoming rows of a frame: the n_centers centers, then the n_neighbors neighbour candidates (two disjoint sets); with
 * same the candidates are the centers themselves, the rows arrive once (n_neighbors == n_centers) and j == i never
 * counts.  In float64 with separate multiply and add, per frame, center i and candidate j:
 *     d = x_j - x_i;  w = d - L * rint(d * (1.0 / L));  r2 = (wx*wx + wy*wy) + wz*wz;  neighbour iff r2 <= cutoff^2
 * and per bond and degree l = degrees[d] (1 ... 12, at most 4 distinct ones) Y_lm(w / sqrt(r2)), m = 0 ... l, by the
 * recurrences and host tables of csrc/mdx_bond_order_device.hpp (Condon-Shortley phase).  Per center with m_i >= 1
 * neighbours: q_lm = (sum of Y_lm over its neighbours in ascending j) / m_i and
 * q_l = sqrt(4 pi / (2l + 1) * sum_m |q_lm|^2);
 * with averaged (same only): qbar_lm = (q_lm(i) + sum of q_lm(j) over the neighbours in ascending j) / (m_i + 1) and
 * qbar_l from it alike.  K = 2 with averaged, else 1; k = 0 is q_l, k = 1 is qbar_l.  A center without a neighbour is
 * isolated: its values are NaN, it is not binned and adds nothing to the sums.  edges: float64 [n_bins + 1], strictly
 * increasing; a value q is counted in bin #{m in 1 ... n_bins - 1 : q >= edges[m]} iff edges[0] <= q <= edges[n_bins]
 * (numpy.histogram's counts), else in outside.  dims: float64 [3] lengths of one constant orthorhombic box; the
 * cutoff may not exceed half the shortest.  A center holds at most max_neighbors (1 ... 64) neighbours in one frame:
 * one that would hold more is never truncated silently, and a neighbour on top of its center (r2 == 0) has no
 * direction; after either, mdx_boo_synchronize, mdx_boo_result, mdx_boo_frames and mdx_boo_values fail with
 * MDX_ERR_INVALID_VALUE (the message names max_neighbors and the largest row, or counts the bonds that had no
 * direction) until mdx_boo_reset.  The rows are sorted before they are summed, the frame sums run per tile of 64
 * centers in row order and then in tile order, and no floating-point atomics are used, so every result is
 * bit-identical across the three input routes, across any split of the frames into calls or slabs, and after a
 * reset.  Every (center, candidate) pair is evaluated, there is no cell list.  A handle touches its device with the
 * first frame: mdx_boo_create and every argument error (MDX_ERR_INVALID_VALUE) need none. */
typedef struct mdx_boo *mdx_boo_t;
int mdx_boo_create(mdx_boo_t *out, int dev, int64_t n_centers, int64_t n_neighbors, int same, double cutoff,
                   int n_degrees, const int32_t *degrees, int averaged, int64_t n_bins, const double *edges,
                   const double *dims, int max_neighbors, int keep_values);
int mdx_boo_destroy(mdx_boo_t h);
/* Forgets the frames seen, the largest row, the bonds without a direction and the kept values, and zeroes the
 * results. */
int mdx_boo_reset(mdx_boo_t h);
/* Frames per kernel launch, at most (1 ... 32768; 0 restores the default, which bounds the slab's buffers in HBM), as
 * mdx_ang_set_slab_frames.  The results do not depend on it.  Only before the first frame. */
int mdx_boo_set_slab_frames(mdx_boo_t h, int64_t frames);
/* As mdx_dip_plan. */
int mdx_boo_plan(mdx_boo_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Host float32 [n_frames][n][3] through the pinned ring; n = the rows of a frame. */
int mdx_boo_accumulate(mdx_boo_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in incoming
 * order, or NULL for all n_atoms rows.  Asynchronous (mdx_boo_synchronize). */
int mdx_boo_accumulate_device(mdx_boo_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                              const int32_t *index, int64_t n_index);
int mdx_boo_accumulate_traj(mdx_boo_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index);
int mdx_boo_synchronize(mdx_boo_t h);
/* counts: int64 [D][K][n_bins]; outside: int64 [D][K]; coordination: int64 [max_neighbors + 1], the (frame, center)
 * cases with exactly m neighbours. */
int mdx_boo_result(mdx_boo_t h, int64_t *counts, int64_t *outside, int64_t *coordination);
/* Of the first n frames seen: sums float64 [n][D][K], the sum of the values of the frame's centers that are not
 * isolated; counted int64 [n], how many those are. */
int mdx_boo_frames(mdx_boo_t h, double *sums, int64_t *counted, int64_t n);
/* values: float64 [n][D][K][n_centers] of the first n frames seen, NaN for an isolated center; only with
 * keep_values. */
int mdx_boo_values(mdx_boo_t h, double *values, int64_t n);
/* evaluations: frames * (n_centers * n_neighbors - (same ? n_centers : 0)); bonds: the list entries; degenerate: the
 * bonds without a direction seen since the last reset (not zero: the results are refused); max_row: the most
 * neighbours a center held in one frame. */
int mdx_boo_stats(mdx_boo_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *bonds, int64_t *degenerate, int64_t *max_row);
int mdx_boo_enable_timing(mdx_boo_t h, int on);

/* ---- tetrahedral order: q and S_k over the four nearest of the n_nearest nearest neighbours of every center --------
 * Rows, box and pair arithmetic as for mdx_boo_*.  Candidate j is in range of center i iff r2 <= cutoff^2 (cutoff *
 * cutoff formed once; a NaN r2 never is).  The candidates of a center are ordered by ascending r2 as float64, ties by
 * ascending j; its neighbours are the first min(n_nearest, m_i) of the m_i in range, 4 <= n_nearest <= 8: a function
 * of the frame alone.  A center with m_i < 4 is short: its values are NaN, it is not binned and adds nothing to the
 * sums.  For the others, with a, b = 0 ... 3 numbering the four nearest, in float64 with separate multiply and add:
 *     cos_ab = ((w_ax*w_bx + w_ay*w_by) + w_az*w_bz) / sqrt(r2_a * r2_b)
 *     q   = 1 - 0.375 * sum over (0,1) (0,2) (1,2) (0,3) (1,3) (2,3) of (cos_ab + 1.0 / 3.0)^2
 *     S_k = 1 - (sum_a (r_a - rbar)^2) / (12 * rbar * rbar),  r_a = sqrt(r2_a),
 *     rbar = (((r_0 + r_1) + r_2) + r_3) * 0.25
 * (every operation and its order: csrc/mdx_tetrahedral_device.hpp).  q_edges [q_bins + 1] and s_edges [s_bins + 1]:
 * float64, strictly increasing, each counted by numpy.histogram's rule as the edges of mdx_boo_create.
 * distance_thresholds: float64 [distance_bins + 1], strictly increasing thresholds of r2; the r2 of the neighbour of
 * every rank a = 0 ... n_nearest - 1 is counted against them by the same rule, short centers included.  dims: float64
 * [3] lengths of one constant orthorhombic box; the cutoff may not exceed half the shortest.  One of the four nearest
 * of a center that is not short on top of it (r2 == 0) has no direction; after that mdx_tet_synchronize,
 * mdx_tet_result, mdx_tet_frames and mdx_tet_values fail with MDX_ERR_INVALID_VALUE until mdx_tet_reset.  A short
 * center has no q, so a candidate on top of it is not an error: it is counted in found and at distance 0.  No floating-point atomics are used: every
 * result is bit-identical across the three input routes, across any split of the frames into calls, slabs or
 * candidate chunks, and after a reset.  Every (center, candidate) pair is evaluated, there is no cell list.  A handle
 * touches its device with the first frame: mdx_tet_create and every argument error (MDX_ERR_INVALID_VALUE) need
 * none. */
typedef struct mdx_tet *mdx_tet_t;
int mdx_tet_create(mdx_tet_t *out, int dev, int64_t n_centers, int64_t n_neighbors, int same, int n_nearest,
                   double cutoff, int64_t q_bins, const double *q_edges, int64_t s_bins, const double *s_edges,
                   int64_t distance_bins, const double *distance_thresholds, const double *dims, int keep_values);
int mdx_tet_destroy(mdx_tet_t h);
/* Forgets the frames seen, the neighbours without a direction and the kept values, and zeroes the results. */
int mdx_tet_reset(mdx_tet_t h);
/* As mdx_boo_set_slab_frames. */
int mdx_tet_set_slab_frames(mdx_tet_t h, int64_t frames);
/* Candidates a block of the selection kernel walks: a multiple of 256; 0 restores the plan's choice.  The results do
 * not depend on it.  Only before the first frame. */
int mdx_tet_set_chunk(mdx_tet_t h, int64_t candidates);
/* Advisory, for planning and for tests of the rule without a device; no other entry point needs it.  The plan's
 * choice for a launch of `frames` frames on a device of compute_units compute units: every candidate in
 * one chunk where ceil(n_centers / 256) * frames >= compute_units, else the candidates in ceil(compute_units /
 * (ceil(n_centers / 256) * frames)) parts rounded up to multiples of 256.  Needs no handle and no device. */
int mdx_tet_chunk_for(int64_t n_centers, int64_t n_neighbors, int64_t frames, int64_t compute_units, int64_t *chunk);
/* As mdx_dip_plan, and chunk: the candidates per block of a launch of slab_frames frames.  Where no chunk is set it
 * reads the compute units of the handle's device. */
int mdx_tet_plan(mdx_tet_t h, int64_t *slab_frames, int64_t *ring_frames, int64_t *chunk);
/* Host float32 [n_frames][n][3] through the pinned ring; n = the rows of a frame. */
int mdx_tet_accumulate(mdx_tet_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in incoming
 * order, or NULL for all n_atoms rows.  Asynchronous (mdx_tet_synchronize), except with keep_values: every slab then
 * ends in a wait for the stream and two copies of its values and neighbours to the host. */
int mdx_tet_accumulate_device(mdx_tet_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                              const int32_t *index, int64_t n_index);
int mdx_tet_accumulate_traj(mdx_tet_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index);
int mdx_tet_synchronize(mdx_tet_t h);
/* q_counts: int64 [q_bins]; s_counts: int64 [s_bins]; outside: int64 [2] (q, S_k); distance_counts: int64
 * [n_nearest][distance_bins]; distance_outside: int64 [n_nearest]; found: int64 [n_nearest + 1], the (frame, center)
 * cases with min(m_i, n_nearest) = m. */
int mdx_tet_result(mdx_tet_t h, int64_t *q_counts, int64_t *s_counts, int64_t *outside, int64_t *distance_counts,
                   int64_t *distance_outside, int64_t *found);
/* Of the first n frames seen: sums float64 [n][2], the sums of q and of S_k over the frame's centers that are not
 * short; counted int64 [n], how many those are. */
int mdx_tet_frames(mdx_tet_t h, double *sums, int64_t *counted, int64_t n);
/* Of the first n frames seen: values float64 [n][2][n_centers], NaN for a short center; neighbors int32
 * [n][n_nearest][n_centers], candidate numbers in the contract's order, -1 beyond m_i; only with keep_values. */
int mdx_tet_values(mdx_tet_t h, double *values, int32_t *neighbors, int64_t n);
/* evaluations: frames * (n_centers * n_neighbors - (same ? n_centers : 0)); degenerate: the neighbours without a
 * direction seen since the last reset (not zero: the results are refused); chunks: the candidate chunks of the last
 * launch. */
int mdx_tet_stats(mdx_tet_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *degenerate, int64_t *chunks);
int mdx_tet_enable_timing(mdx_tet_t h, int on);

/* ---- self-overlap Q(t) and four-point susceptibility chi_4(t) ------------------------------------------------------
 * Groups, rows, frames, lags, zero_dims, x, image and the unwrap rule as for mdx_vh_*; origin_step >= 1.  cutoffs:
 * float64 [n_cutoffs], 1 ... 8 of them, finite, not negative, strictly increasing.  Per lag k, cutoff c and frame
 * f >= lags[k] whose origin f0 = f - lags[k] satisfies f0 % origin_step == 0, in float64 with separate multiply and
 * add (float32 coordinates are widened before any arithmetic):
 *     d = x(f) - x(f0), +0.0 for a dropped component;  r2 = (dx*dx + dy*dy) + dz*dz;
 *     w = r2 <= cutoffs[c] * cutoffs[c] (one float64 multiply on the host; no sqrt; a NaN r2 is not counted);
 *     Q[k][g][c](f0) = the number of points of group g with w;  S1[k][g][c] += Q;  S2[k][g][c] += Q*Q;
 *     n_origins[k] = the number of such f0.
 * Everything added is an integer, so S1, S2 and n_origins are identical across the three input routes, across any split
 * of the frames into calls, slabs or point segments, and after a reset (csrc/mdx_chi4_device.hpp).  The engine keeps
 * max(lags) + one slab of float64 frames in HBM (MDX_ERR_OUT_OF_MEMORY when that does not fit).  A handle touches its
 * device with the first frame: mdx_chi4_create and every argument error (MDX_ERR_INVALID_VALUE) need none. */
typedef struct mdx_chi4 *mdx_chi4_t;
int mdx_chi4_create(mdx_chi4_t *out, int dev, int n_groups, const int64_t *n_points, int n_cutoffs,
                    const double *cutoffs, int n_lags, const int64_t *lags, int64_t origin_step, int zero_dims);
int mdx_chi4_destroy(mdx_chi4_t h);
/* Forgets the frames seen, the history and the unwrap state and zeroes the sums. */
int mdx_chi4_reset(mdx_chi4_t h);
/* As mdx_vh_set_unwrap.  dims: float64 [3] box lengths, or NULL: off.  Only before the first frame. */
int mdx_chi4_set_unwrap(mdx_chi4_t h, const double *dims);
/* Frames per kernel launch, at most (1 ... 32768; 0 restores the default, which bounds the history and the scratch), as
 * mdx_vh_set_slab_frames.  The results do not depend on it.  Only before the first frame. */
int mdx_chi4_set_slab_frames(mdx_chi4_t h, int64_t frames);
/* As mdx_dip_plan. */
int mdx_chi4_plan(mdx_chi4_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Points of the concatenated groups that one block of the counting kernel walks: a multiple of 64; 0 restores the
 * default.  For tests and measurement: the results do not depend on it.  Only before the first frame. */
int mdx_chi4_set_segment_points(mdx_chi4_t h, int64_t points);
/* The accumulate calls refuse (MDX_ERR_INVALID_VALUE), before they touch a device or read a frame, a call after which
 * (frames seen) * max_g(n_points[g])^2 would reach 2^63: S2 could then leave an int64.  What was accumulated before
 * stays valid.  Host float32 [n_frames][n][3] through the pinned ring. */
int mdx_chi4_accumulate(mdx_chi4_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in incoming
 * order, or NULL for all n_atoms rows.  Asynchronous (mdx_chi4_synchronize). */
int mdx_chi4_accumulate_device(mdx_chi4_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                               const int32_t *index, int64_t n_index);
int mdx_chi4_accumulate_traj(mdx_chi4_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                             const int32_t *index, int64_t n_index);
int mdx_chi4_synchronize(mdx_chi4_t h);
/* sums, square_sums: int64 [n_lags][n_groups][n_cutoffs] = S1, S2; n_origins: int64 [n_lags]. */
int mdx_chi4_result(mdx_chi4_t h, int64_t *sums, int64_t *square_sums, int64_t *n_origins);
/* evaluations: the contract's count of displacements so far, sum over the lags of origins x points. */
int mdx_chi4_stats(mdx_chi4_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations);
int mdx_chi4_enable_timing(mdx_chi4_t h, int on);

/* ---- hydrogen bonds: donor-H...acceptor counts, geometry and lifetimes ----------------------------------------------
 * The incoming rows of a frame are n_rows distinct atoms; h_row[n_h] names the hydrogens, d_row[n_h] the donor each
 * hydrogen is bonded to (it may repeat), a_row[n_a] the acceptors (int32 rows in [0, n_rows); no hydrogen and no
 * acceptor twice, no row both, d_row[i] != h_row[i]; a donor may be an acceptor).  dims, frames, lags, origin_step and
 * zero_dims as for mdx_prs_*.  Per frame, hydrogen i and acceptor j, with H, D, A their positions, in float64 with
 * separate multiply and add and the minimum image w(x) = x - L * rint(x * (1.0 / L)) (+0.0 for a dropped component):
 *     w_DA = w(A - D);  r2_DA = (w_DAx^2 + w_DAy^2) + w_DAz^2;  w_HD = w(D - H);  w_HA = w(A - H);
 *     c = ((w_HDx*w_HAx + w_HDy*w_HAy) + w_HDz*w_HAz) / sqrt(r2_HD * r2_HA);
 *     the pair is inside where r2_DA <= distance * distance and a_row[j] != d_row[i], and a bond where it is inside
 *     and c <= cos_max (cos_max = cos(150 degrees): angles D-H...A of at least 150 degrees).
 * A NaN r2_DA is not inside; an inside pair with NaN c (a hydrogen on its donor or on the acceptor) is no bond and
 * counts in `degenerate`.  With B(f) the bonds of frame f:  bonds[f] = |B(f)|;  origin_counts, intermittent and
 * continuous are those of mdx_prs_* with B for C;  donated[m], m = 0 ... max_neighbors: the (frame, hydrogen) cases
 * with exactly m bonds;  distance_counts[b]: the bonds with b = #{m in 1 ... n_r - 1 : r2_DA >= r2_thresholds[m]};
 * cosine_counts[b]: the bonds with b = #{m in 1 ... n_c - 1 : c <= cos_thresholds[m]}.
 * distance: positive, finite, at most half the shortest kept box length.  cos_max in [-1, 1].  max_neighbors
 * (1 ... 64): the bonds a hydrogen may hold in one frame.  A hydrogen that would hold more is never truncated
 * silently: mdx_hb_synchronize, mdx_hb_result, mdx_hb_bonds and mdx_hb_geometry fail with MDX_ERR_INVALID_VALUE (the
 * message names max_neighbors and the largest row seen) until mdx_hb_reset.  continuous == 0: only the frames a lag
 * away from an origin are visited and continuous[] stays zero.  All results are integers and identical across the
 * three input routes, across any split of the frames into calls or slabs, and after a reset
 * (csrc/mdx_hbond_device.hpp).  The engine keeps max(lags) + one slab of frames of bond lists in HBM,
 * (max_neighbors + 3) * n_h * 4 bytes each.  A handle touches its device with the first frame: mdx_hb_create,
 * mdx_hb_set_bins and every argument error (MDX_ERR_INVALID_VALUE) need none. */
typedef struct mdx_hb *mdx_hb_t;
int mdx_hb_create(mdx_hb_t *out, int dev, int64_t n_rows, int64_t n_h, const int32_t *h_row, const int32_t *d_row,
                  int64_t n_a, const int32_t *a_row, double distance, double cos_max, int n_lags, const int64_t *lags,
                  int64_t origin_step, const double *dims, int zero_dims, int max_neighbors, int continuous);
/* r2_thresholds: float64 [n_r + 1], strictly increasing (thresholds of r2_DA, not of the distance); cos_thresholds:
 * float64 [n_c + 1], strictly decreasing.  Only the inner ones are compared: the first and the last bin are open.
 * Without this call both histograms have one bin.  Only before the first frame. */
int mdx_hb_set_bins(mdx_hb_t h, int64_t n_r, const double *r2_thresholds, int64_t n_c, const double *cos_thresholds);
int mdx_hb_destroy(mdx_hb_t h);
/* Forgets the frames seen, the history and an overflowing row, and zeroes the results. */
int mdx_hb_reset(mdx_hb_t h);
/* Frames per kernel launch, at most (1 ... 32768; 0 restores the default, which bounds the history).  The results do
 * not depend on it.  Only before the first frame. */
int mdx_hb_set_slab_frames(mdx_hb_t h, int64_t frames);
/* As mdx_dip_plan. */
int mdx_hb_plan(mdx_hb_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Host float32 [n_frames][n][3] through the pinned ring; n = n_rows. */
int mdx_hb_accumulate(mdx_hb_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in incoming
 * order, or NULL for all n_atoms rows.  Asynchronous (mdx_hb_synchronize). */
int mdx_hb_accumulate_device(mdx_hb_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames, const int32_t *index,
                             int64_t n_index);
int mdx_hb_accumulate_traj(mdx_hb_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames, const int32_t *index,
                           int64_t n_index);
int mdx_hb_synchronize(mdx_hb_t h);
/* intermittent, continuous, origin_counts: int64 [n_lags] each. */
int mdx_hb_result(mdx_hb_t h, int64_t *intermittent, int64_t *continuous, int64_t *origin_counts);
/* out: int64 [n], the bonds of the first n frames seen. */
int mdx_hb_bonds(mdx_hb_t h, int64_t *out, int64_t n);
/* distance_counts: int64 [n_r]; cosine_counts: int64 [n_c]; donated: int64 [max_neighbors + 1]. */
int mdx_hb_geometry(mdx_hb_t h, int64_t *distance_counts, int64_t *cosine_counts, int64_t *donated);
/* evaluations: the contract's pair count so far, frames x (n_h * n_a - the pairs with a_row[j] == d_row[i]); max_row:
 * the most bonds a hydrogen held in one frame (beyond max_neighbors: the results are refused); degenerate: the inside
 * pairs without an angle. */
int mdx_hb_stats(mdx_hb_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                 int64_t *max_row, int64_t *degenerate);
int mdx_hb_enable_timing(mdx_hb_t h, int on);

/* ---- dihedrals: torsion angles, their histogram, conformer states and the lifetimes of the states ------------------
 * A frame delivers n_rows points; quads: int32 [D][4] row numbers (a, b, c, d) of the D dihedrals, four distinct rows
 * each; group g holds n_dihedrals[g] consecutive dihedrals (a group may be empty, all of them together may not).
 * Analysed frames are numbered f = 0, 1, ... in the order fed; lags: strictly increasing, non-negative frame offsets
 * below 2^31; every frame is a time origin.  In float64 with separate multiply and add (float32 coordinates are
 * widened before any arithmetic), per dihedral and frame:
 *     b1 = x_b - x_a, b2 = x_c - x_b, b3 = x_d - x_c, each w = d - L * rint(d * (1.0 / L)) with a box (mdx_dih_set_box);
 *     m = b1 x b2, n = b2 x b3 (m_x = b1y*b2z - b1z*b2y, ...);  m2, n2, l2 = the squares of m, n, b2;
 *     p = m . n;  q = b1 . n;  den = sqrt(m2 * n2);  c = p / den (cos phi);  s = (sqrt(l2) * q) / den (sin phi, IUPAC sign)
 * A dihedral whose m2 * n2 is not > 0 or not finite has no angle: it is counted, never averaged silently, and
 * mdx_dih_synchronize and every read-out fail with MDX_ERR_INVALID_VALUE until mdx_dih_reset.
 *     n_bins even, n_half = n_bins / 2; thresholds: float64 [n_half + 1], strictly decreasing (cos(m pi / n_half) bins
 *     phi evenly over [-180, 180) degrees; only the inner ones are compared);
 *     h = #{ m in 1 ... n_half - 1 : c <= thresholds[m] };  bin = q < 0 ? n_half - 1 - h : n_half + h
 *     state(f) = state_of_bin[bin]   (int32 [n_bins], values 0 ... n_states - 1, 1 <= n_states <= 8)
 *     run(0) = 0;  run(f) = state(f) == state(f - 1) ? min(run(f - 1) + 1, 2^31 - 1) : 0
 * Integer results, added with integer atomics: counts[g][bin]; state_counts[f][g][s]; transitions[g][s0][s1] over the
 * (dihedral, f >= 1) cases with state(f - 1) = s0 and state(f) = s1; same[k][g] over f >= lag_k with
 * state(f) == state(f - lag_k); stay[k][g] over f >= lag_k with run(f) >= lag_k.  Float result:
 * acc[k][v] += c(f)*c(f - lag_k) + s(f)*s(f - lag_k) in frame order, and sums[k][g] adds the accumulators of the group's
 * dihedrals in row order (csrc/mdx_dihedral_device.hpp); no floating-point atomics are used, so every result is
 * bit-identical across the three input routes, across any split of the frames into calls or slabs, and after a reset.
 * The engine keeps max(max lag, 1) + one slab of frames of c, s, state and run in HBM (MDX_ERR_OUT_OF_MEMORY when that
 * does not fit).  A handle touches its device with the first frame: mdx_dih_create and every argument error
 * (MDX_ERR_INVALID_VALUE) need none. */
typedef struct mdx_dih *mdx_dih_t;
int mdx_dih_create(mdx_dih_t *out, int dev, int n_groups, const int64_t *n_dihedrals, int64_t n_rows,
                   const int32_t *quads, int n_bins, const double *thresholds, int n_states,
                   const int32_t *state_of_bin, int n_lags, const int64_t *lags);
int mdx_dih_destroy(mdx_dih_t h);
/* Forgets the frames seen, the history and the degenerate dihedrals and zeroes the results. */
int mdx_dih_reset(mdx_dih_t h);
/* One constant orthorhombic box for the minimum image of the three bond vectors.  dims: float64 [3] box lengths, or
 * NULL: none (molecules that are whole already).  Only before the first frame. */
int mdx_dih_set_box(mdx_dih_t h, const double *dims);
/* As mdx_ori_set_slab_frames. */
int mdx_dih_set_slab_frames(mdx_dih_t h, int64_t frames);
/* As mdx_dip_plan; the ring holds max(max lag, 1) + slab frames. */
int mdx_dih_plan(mdx_dih_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Host float32 [n_frames][n][3] through the pinned ring; n = n_rows. */
int mdx_dih_accumulate(mdx_dih_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in the order the
 * quads name them, or NULL for all n_atoms rows.  Asynchronous (mdx_dih_synchronize). */
int mdx_dih_accumulate_device(mdx_dih_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                              const int32_t *index, int64_t n_index);
int mdx_dih_accumulate_traj(mdx_dih_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index);
int mdx_dih_synchronize(mdx_dih_t h);
/* sums: float64 [n_lags][n_groups]; same, stay: int64 [n_lags][n_groups]. */
int mdx_dih_result(mdx_dih_t h, double *sums, int64_t *same, int64_t *stay);
/* out: float64 [n_lags][D]: the accumulators of every dihedral. */
int mdx_dih_dihedral_sums(mdx_dih_t h, double *out);
/* out: int64 [n_groups][n_bins]. */
int mdx_dih_counts(mdx_dih_t h, int64_t *out);
/* out: int64 [n][n_groups][n_states], the state populations of the first n frames seen. */
int mdx_dih_state_counts(mdx_dih_t h, int64_t *out, int64_t n);
/* out: int64 [n_groups][n_states][n_states]. */
int mdx_dih_transitions(mdx_dih_t h, int64_t *out);
/* evaluations: correlation terms formed so far (frame pairs x dihedrals, summed over the lags); degenerate: dihedrals
 * without an angle seen since the last reset (not zero: the results are refused). */
int mdx_dih_stats(mdx_dih_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *degenerate);
int mdx_dih_enable_timing(mdx_dih_t h, int on);

/* ---- spatial distribution: 3-D densities of partner atoms in the body-fixed frame of a reference molecule ----------
 * The incoming rows of a frame are n_rows distinct atoms; o_row, a_row, b_row [n_ref] name the origin, the axis atom
 * and the plane atom of every reference molecule (int32 rows in [0, n_rows); no origin twice, the three rows of a
 * molecule differ pairwise); p_row [n_p] the partner atoms, group after group (no row twice), group_start
 * [n_groups + 1] non-decreasing from 0 to n_p, 1 <= n_groups <= 8; owner [n_p]: the reference molecule a partner
 * belongs to, in [0, n_ref), or -1: the pair (i, j) with owner[j] == i is never evaluated.  dims: float64 [3] lengths
 * of one constant orthorhombic box; all three components take part.  In float64 with separate multiply and add and
 * the minimum image w(x) = x - L * rint(x * (1.0 / L)), with O, A, B, P the positions of a frame:
 *     a = w(A - O);  b = w(B - O);  p = a  (mode 0, axis)  or  a / sqrt(r2(a)) + b / sqrt(r2(b))  (mode 1, bisector);
 *     e1 = p / sqrt(r2(p));  c = p x b;  e3 = c / sqrt(r2(c));  e2 = e3 x e1  (c_x = p_y*b_z - p_z*b_y, ...);
 *     w = w(P - O);  near = r2(w) <= cutoff * cutoff and owner[j] != i and e1, e2, e3 all finite;
 *     u = (w_x*e1_x + w_y*e1_y) + w_z*e1_z, v with e2, t with e3;
 *     inside = near and ex[0] <= u <= ex[nx] and ey[0] <= v <= ey[ny] and ez[0] <= t <= ez[nz];
 *     bin_x = #{m in 1 ... nx - 1 : u >= ex[m]}, likewise y and z (numpy.histogramdd: the last bin is closed above).
 * A molecule with a non-finite e1, e2 or e3 (an atom on another, three collinear atoms) counts once per frame in
 * `degenerate` and has no pair.  counts[g][bin_x][bin_y][bin_z]: the inside pairs of group g; inside[f]: those of
 * frame f.  cutoff: positive, finite, at most half the shortest box length.  All results are integers and identical
 * across the three input routes, across any split of the frames into calls or slabs, and after a reset
 * (csrc/mdx_sdf_device.hpp).  A handle touches its device with the first frame: mdx_sdf_create, mdx_sdf_set_bins and
 * every argument error (MDX_ERR_INVALID_VALUE, the message names the argument) need none. */
typedef struct mdx_sdf *mdx_sdf_t;
int mdx_sdf_create(mdx_sdf_t *out, int dev, int64_t n_rows, int64_t n_ref, const int32_t *o_row, const int32_t *a_row,
                   const int32_t *b_row, int n_groups, const int64_t *group_start, const int32_t *p_row,
                   const int32_t *owner, int mode, double cutoff, const double *dims);
/* ex: float64 [nx + 1], ey: [ny + 1], ez: [nz + 1], strictly increasing and finite, 1 ... 512 bins per axis and
 * n_groups * nx * ny * nz <= 2^26.  Without this call every axis has the one bin [-cutoff, cutoff].  Only before the
 * first frame. */
int mdx_sdf_set_bins(mdx_sdf_t h, int64_t nx, const double *ex, int64_t ny, const double *ey, int64_t nz,
                     const double *ez);
int mdx_sdf_destroy(mdx_sdf_t h);
/* Forgets the frames seen and zeroes the results. */
int mdx_sdf_reset(mdx_sdf_t h);
/* Frames per kernel launch, at most (1 ... 32768; 0 restores the default).  The results do not depend on it.  Only
 * before the first frame. */
int mdx_sdf_set_slab_frames(mdx_sdf_t h, int64_t frames);
/* As mdx_dip_plan; ring_frames = 0: a frame needs no other frame. */
int mdx_sdf_plan(mdx_sdf_t h, int64_t *slab_frames, int64_t *ring_frames);
/* Host float32 [n_frames][n][3] through the pinned ring; n = n_rows. */
int mdx_sdf_accumulate(mdx_sdf_t h, const float *pos, int64_t n, int64_t n_frames);
/* Frames already in HBM, float32 [n_frames][n_atoms][3]; index: host int32[n_index] rows of a frame in incoming
 * order, or NULL for all n_atoms rows.  Asynchronous (mdx_sdf_synchronize). */
int mdx_sdf_accumulate_device(mdx_sdf_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames, const int32_t *index,
                              int64_t n_index);
int mdx_sdf_accumulate_traj(mdx_sdf_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const int32_t *index, int64_t n_index);
int mdx_sdf_synchronize(mdx_sdf_t h);
/* counts: int64 [n_groups][nx][ny][nz]. */
int mdx_sdf_result(mdx_sdf_t h, int64_t *counts);
/* out: int64 [n], the inside pairs of the first n frames seen. */
int mdx_sdf_inside(mdx_sdf_t h, int64_t *out, int64_t n);
/* evaluations: the contract's pair count so far, frames x (n_ref * n_p - the pairs with owner[j] == i); degenerate:
 * the (frame, molecule) cases without a frame of their own. */
int mdx_sdf_stats(mdx_sdf_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *degenerate);
int mdx_sdf_enable_timing(mdx_sdf_t h, int on);

#ifdef __cplusplus
}
#endif
#endif /* MDX_H */
