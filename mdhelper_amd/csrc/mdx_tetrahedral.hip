// mdx_tetrahedral.hip — tetrahedral order (the orientational q of Chau-Hardwick / Errington-Debenedetti and its
// translational counterpart S_k) over the k nearest neighbours of every centre, on gfx950 (MI355X).
//
// Per frame the k nearest candidates in range of every centre: a register-resident top-k selection on the shared pair
// walk, ordered by (r2, j) so that it is a function of the frame alone; from the four nearest q and S_k, their
// histograms and per-frame sums; per neighbour rank the histogram of its distance; and how many neighbours the centres
// found.  Contract, kernel shapes and the cost model of the candidate chunks: mdx_tetrahedral_device.hpp; this unit is
// compiled with contraction off and spells its float64 operations out.
//
// Every float64 comes from a fixed sequence of operations on the ordered list and every tally is an integer atomic, so
// the results are the same bits whatever route the frames take and however they are split into calls, slabs or chunks.
//
// A handle touches its device with the first frame (or result): creating one, and every argument error, needs none.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_pairs_host.hpp"
#include "mdx_tetrahedral_device.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace mdx;
using namespace mdx_tet_dev;

namespace {

constexpr int64_t TET_SLAB_BYTES = int64_t(256) << 20;  // what the frames of a default slab take in HBM
constexpr int64_t TET_MAX_BINS = int64_t(1) << 20;

using SelectKernel = void (*)(const float *, int, int, int, int, int, int, int, PairBox, double, int *);
using FinishKernel = void (*)(const float *, int, int, int, PairBox, int, const int *, const double *, int, int64_t,
                              double *, int *, unsigned long long *, unsigned long long *, unsigned long long *,
                              unsigned long long *, unsigned long long *);

template <int K>
void tet_kernels_from(int k, bool lds_hist, SelectKernel *select, FinishKernel *finish)
{
    if (k == K) {
        *select = tet_select_kernel<K>;
        *finish = lds_hist ? tet_finish_kernel<K, true> : tet_finish_kernel<K, false>;
        return;
    }
    if constexpr (K < TET_MAX_NEAREST)
        tet_kernels_from<K + 1>(k, lds_hist, select, finish);
}

int64_t tet_round_up(int64_t n) { return ceil_div(n, TET_STAGE) * TET_STAGE; }

// The candidates per block of a launch of `frames` frames on a device of `cus` compute units: all of them (one chunk:
// a lane's bound falls through its whole walk) wherever i tiles x frames fills the device, else as many parts as it
// takes to fill it, each a multiple of the stage (mdx_tetrahedral_device.hpp, "Candidate chunks").
int64_t tet_chunk_for(int64_t n0, int64_t n1, int64_t frames, int64_t cus)
{
    const int64_t whole = tet_round_up(n1);
    const int64_t units = ceil_div(n0, TET_TILE) * std::max<int64_t>(frames, 1);
    if (units >= cus)
        return whole;
    return std::min(whole, tet_round_up(ceil_div(n1, ceil_div(cus, units))));
}

}  // namespace

struct mdx_tet : LazyFrameEngine {
    bool same = false, keep_values = false;
    int K = TET_MIN_NEAREST, cus = 0;   // cus: the device's compute units, 0 until asked for
    SelectKernel select_kernel = nullptr;
    FinishKernel finish_kernel = nullptr;
    int64_t n0 = 0, n1 = 0, n_rows = 0, q_bins = 0, s_bins = 0, d_bins = 0;
    int64_t pinned_chunk = 0;           // mdx_tet_set_chunk; 0: the plan's choice
    int64_t last_chunks = 0;            // chunks of the last launch
    double rc2 = 0.0, bound0 = 0.0;
    int64_t degenerate = 0;             // neighbours on their centre, as of the last look
    PairBox box;
    std::vector<double> tables;         // q edges [q_bins + 1], S_k edges [s_bins + 1], thresholds of r2 [d_bins + 1]
    std::vector<double> values;         // keep_values: [frames seen][2][n0] on the host
    std::vector<int32_t> neighbors;     // keep_values: [frames seen][K][n0] on the host
    // d_counts: uint64 q counts [q_bins], S_k counts [s_bins], outside [2], distance counts [K][d_bins], distance
    // outside [K], found [K + 1], degenerate [1]
    // d_list: int32 [launch frames][chunks][K][n0]; d_values: double [slab][2][n0]; d_neighbors: int32 [slab][K][n0]
    // d_frame_sums: double [frames seen][2]; d_counted: uint64 [frames seen]
    DeviceBuffer d_tables, d_counts, d_slab, d_list, d_values, d_neighbors, d_frame_sums, d_counted;

    int64_t words() const { return q_bins + s_bins + 2 + K * d_bins + K + (K + 1) + 1; }
    unsigned long long *q_words() { return d_counts.as<unsigned long long>(); }
    unsigned long long *s_words() { return q_words() + q_bins; }
    unsigned long long *outside_words() { return s_words() + s_bins; }
    unsigned long long *distance_words() { return outside_words() + 2; }
    unsigned long long *distance_outside_words() { return distance_words() + K * d_bins; }
    unsigned long long *found_words() { return distance_outside_words() + K; }
    unsigned long long *degenerate_word() { return found_words() + (K + 1); }
    const double *q_edges() { return d_tables.as<double>(); }
    const double *s_edges() { return q_edges() + (q_bins + 1); }
    const double *d_table() { return s_edges() + (s_bins + 1); }

    int64_t rows_wanted() const { return n_rows; }
    const char *rows_noun() const { return "groups"; }
    void clear_counters() { degenerate = 0; values.clear(); neighbors.clear(); }
    void free_device()
    {
        release({&d_tables, &d_counts, &d_slab, &d_list, &d_values, &d_neighbors, &d_frame_sums, &d_counted});
    }
};

// the chunks a pinned chunk cuts the candidates into, 1 for the plan's choice at a full slab
static int64_t tet_pinned_chunks(const mdx_tet *h)
{
    return h->pinned_chunk ? ceil_div(h->n1, std::min(h->pinned_chunk, tet_round_up(h->n1))) : 1;
}

// bytes a frame of a slab takes: its gathered rows, its chunk lists, its values and, where kept, its neighbours
static int64_t tet_frame_bytes(const mdx_tet *h)
{
    return 12 * h->n_rows + 4 * h->K * h->n0 * tet_pinned_chunks(h) + 16 * h->n0 +
           (h->keep_values ? 4 * h->K * h->n0 : 0);
}

static int64_t tet_slab(const mdx_tet *h)
{
    return pair_slab_frames(h->slab_frames, TET_SLAB_BYTES, tet_frame_bytes(h));
}

// candidates per block of a launch of nf frames
static int64_t tet_launch_chunk(const mdx_tet *h, int64_t nf)
{
    if (h->pinned_chunk)
        return std::min(h->pinned_chunk, tet_round_up(h->n1));
    return tet_chunk_for(h->n0, h->n1, nf, h->cus);
}

static int tet_zero(mdx_tet *h)
{
    MDX_HIP(hipMemsetAsync(h->d_counts.ptr, 0, size_t(8) * h->words(), h->stream));
    if (h->d_frame_sums.ptr)
        MDX_HIP(hipMemsetAsync(h->d_frame_sums.ptr, 0, h->d_frame_sums.bytes, h->stream));
    if (h->d_counted.ptr)
        MDX_HIP(hipMemsetAsync(h->d_counted.ptr, 0, h->d_counted.bytes, h->stream));
    h->degenerate = 0;
    h->values.clear();
    h->neighbors.clear();
    return MDX_OK;
}

// the compute units of the handle's device (mdx_device_info's figure), asked for once
static int tet_compute_units(mdx_tet *h)
{
    if (h->cus > 0)
        return MDX_OK;
    int cus = 0;
    MDX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->dev));
    h->cus = std::max(cus, 1);
    return MDX_OK;
}

// the device side of the handle: tables and counters
static int tet_build(mdx_tet *h)
{
    MDX_TRY(tet_compute_units(h));
    MDX_TRY(h->d_tables.ensure(size_t(8) * h->tables.size()));
    MDX_TRY(h->d_counts.ensure(size_t(8) * h->words()));
    MDX_HIP(hipMemcpy(h->d_tables.ptr, h->tables.data(), size_t(8) * h->tables.size(), hipMemcpyHostToDevice));
    return tet_zero(h);
}

static int tet_ensure_device(mdx_tet *h) { return h->ensure_device(tet_build); }

// The buffers of a slab, sized before the first frame of a pass.  Nothing is in flight then (a reset waits for the
// stream), so growing them loses nothing.  The chunk lists are sized per launch (tet_accumulate_rows).
static int tet_ensure_slab(mdx_tet *h)
{
    if (h->frames_seen > 0)
        return MDX_OK;
    const int64_t slab = tet_slab(h);
    MDX_REQUIRE(slab < (int64_t(1) << 40) / tet_frame_bytes(h), "a slab of %lld frames of %lld rows is too large",
                (long long)slab, (long long)h->n_rows);
    MDX_TRY(h->d_slab.ensure(size_t(12) * h->n_rows * slab));
    MDX_TRY(h->d_values.ensure(size_t(16) * h->n0 * slab));
    if (h->keep_values)
        MDX_TRY(h->d_neighbors.ensure(size_t(4) * h->K * h->n0 * slab));
    return MDX_OK;
}

// with the stream idle: the neighbours on their centre seen, without judging them
static int tet_look(mdx_tet *h)
{
    unsigned long long seen = 0;
    MDX_HIP(hipMemcpy(&seen, h->degenerate_word(), 8, hipMemcpyDeviceToHost));
    h->degenerate = (int64_t)seen;
    return MDX_OK;
}

// With the stream idle: a neighbour on its centre refuses the results until a reset.
static int tet_check(mdx_tet *h)
{
    MDX_TRY(tet_look(h));
    MDX_REQUIRE(h->degenerate == 0,
                "%lld of the four nearest neighbors had no direction (a neighbor on its center): their angles are "
                "undefined (reset starts over)", (long long)h->degenerate);
    return MDX_OK;
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int tet_accumulate_rows(mdx_tet *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                               int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_rows, "%lld rows given, the groups hold %lld", (long long)n_rows,
                (long long)h->n_rows);
    MDX_TRY(grow_frames(h->d_frame_sums, h->stream, 16, h->frames_seen, h->frames_seen + n_frames));
    MDX_TRY(grow_frames(h->d_counted, h->stream, 8, h->frames_seen, h->frames_seen + n_frames));
    const int n = (int)h->n_rows, n0 = (int)h->n0, n1 = (int)h->n1, off = h->same ? 0 : n0, K = h->K;
    const int64_t slab = tet_slab(h);       // what tet_ensure_slab sized the buffers for
    const int64_t tiles = ceil_div(h->n0, TET_TILE);
    const unsigned lanes = (unsigned)ceil_div(h->n0, TET_THREADS);
    double *values = h->d_values.as<double>();
    int *neighbors = h->keep_values ? h->d_neighbors.as<int>() : nullptr;
    const auto q_bin = h->q_bins <= TET_LDS_BINS ? tet_bin_kernel<true> : tet_bin_kernel<false>;
    const auto s_bin = h->s_bins <= TET_LDS_BINS ? tet_bin_kernel<true> : tet_bin_kernel<false>;
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        const int64_t f0 = h->frames_seen;
        const int64_t chunk = tet_launch_chunk(h, nf), n_chunks = ceil_div(h->n1, chunk);
        MDX_REQUIRE(tiles * n_chunks < (int64_t(1) << 31) && n_chunks * K * h->n0 < (int64_t(1) << 40) / (4 * nf),
                    "%lld centers and %lld chunks of neighbors are too many for one launch", (long long)h->n0,
                    (long long)n_chunks);
        // the lists of this launch; growing the block waits for the kernels that read the old one
        MDX_TRY(h->d_list.ensure(size_t(4) * n_chunks * K * h->n0 * nf));
        hipEvent_t ev = h->timer.begin();
        launch_gather<false>(h->stream, pos, src_rows, d_index, n, nf, h->d_slab.as<float>());
        hipLaunchKernelGGL(h->select_kernel, dim3((unsigned)(tiles * n_chunks), 1, (unsigned)nf), dim3(TET_THREADS), 0,
                           h->stream, h->d_slab.as<float>(), n, n0, n1, off, int(h->same), (int)n_chunks, (int)chunk,
                           h->box, h->bound0, h->d_list.as<int>());
        hipLaunchKernelGGL(h->finish_kernel, dim3(lanes, (unsigned)nf), dim3(TET_THREADS), 0, h->stream,
                           h->d_slab.as<float>(), n, n0, off, h->box, (int)n_chunks, h->d_list.as<int>(), h->d_table(),
                           (int)h->d_bins, f0, values, neighbors, h->distance_words(), h->distance_outside_words(),
                           h->found_words(), h->degenerate_word(), h->d_counted.as<unsigned long long>());
        // one quantity per launch, each against its own table; a block takes TET_BIN_CHUNK values
        const unsigned bin_blocks = (unsigned)ceil_div(nf * h->n0, TET_BIN_CHUNK);
        hipLaunchKernelGGL(q_bin, dim3(bin_blocks), dim3(TET_THREADS), 0, h->stream, values, nf * h->n0, n0, 0,
                           h->q_edges(), (int)h->q_bins, h->q_words(), h->outside_words());
        hipLaunchKernelGGL(s_bin, dim3(bin_blocks), dim3(TET_THREADS), 0, h->stream, values, nf * h->n0, n0, 1,
                           h->s_edges(), (int)h->s_bins, h->s_words(), h->outside_words() + 1);
        hipLaunchKernelGGL(tet_sum_kernel, dim3((unsigned)(nf * 2)), dim3(TET_THREADS), 0, h->stream, values, n0, f0,
                           h->d_frame_sums.as<double>());
        h->frames_seen += nf;
        h->last_chunks = n_chunks;
        h->timer.end(ev);
        MDX_HIP(hipGetLastError());
        if (h->keep_values) {               // the slab's values leave before the next slab overwrites them
            const size_t n_values = size_t(nf * 2 * h->n0), n_neighbors = size_t(nf * K * h->n0);
            const size_t at_values = h->values.size(), at_neighbors = h->neighbors.size();
            h->values.resize(at_values + n_values);
            h->neighbors.resize(at_neighbors + n_neighbors);
            MDX_HIP(hipStreamSynchronize(h->stream));
            MDX_HIP(hipMemcpy(h->values.data() + at_values, values, size_t(8) * n_values, hipMemcpyDeviceToHost));
            MDX_HIP(hipMemcpy(h->neighbors.data() + at_neighbors, neighbors, size_t(4) * n_neighbors,
                              hipMemcpyDeviceToHost));
        }
    }
    return MDX_OK;
}

// an increasing finite table of n + 1 values
static int tet_check_table(const char *name, int64_t n, const double *table)
{
    MDX_REQUIRE(n >= 1 && n <= TET_MAX_BINS, "%s must hold between 1 and %lld bins", name, (long long)TET_MAX_BINS);
    MDX_REQUIRE(std::isfinite(table[0]) && std::isfinite(table[n]), "%s must be finite", name);
    for (int64_t m = 0; m < n; ++m)
        MDX_REQUIRE(table[m] < table[m + 1], "%s must be strictly increasing: [%lld] = %g, [%lld] = %g", name,
                    (long long)m, table[m], (long long)(m + 1), table[m + 1]);
    return MDX_OK;
}

extern "C" {

int mdx_tet_create(mdx_tet_t *out, int dev, int64_t n_centers, int64_t n_neighbors, int same, int n_nearest,
                   double cutoff, int64_t q_bins, const double *q_edges, int64_t s_bins, const double *s_edges,
                   int64_t distance_bins, const double *distance_thresholds, const double *dims, int keep_values)
{
    MDX_REQUIRE(out && q_edges && s_edges && distance_thresholds && dims, "NULL argument");
    MDX_REQUIRE(n_nearest >= TET_MIN_NEAREST && n_nearest <= TET_MAX_NEAREST, "n_nearest must lie in [%d, %d]",
                TET_MIN_NEAREST, TET_MAX_NEAREST);
    MDX_REQUIRE(n_centers >= 1, "the centers must hold at least one point");
    MDX_REQUIRE(n_neighbors >= 1, "the neighbors must hold at least one point");
    MDX_REQUIRE(!same || n_neighbors == n_centers, "with same the neighbors are the %lld centers themselves",
                (long long)n_centers);
    const int64_t n_rows = same ? n_centers : n_centers + n_neighbors;
    const int64_t limit = (int64_t(1) << 31) / 3;
    MDX_REQUIRE(n_centers < limit && n_neighbors < limit && n_rows < limit,
                "the groups must hold fewer than 2^31 / 3 points");
    MDX_REQUIRE(cutoff > 0.0 && std::isfinite(cutoff), "cutoff must be positive and finite");
    PairBox box;
    int keep = 7;
    MDX_TRY(check_box_cutoff(dims, 0, cutoff, &box, &keep));
    MDX_TRY(tet_check_table("q_edges", q_bins, q_edges));
    MDX_TRY(tet_check_table("s_edges", s_bins, s_edges));
    MDX_TRY(tet_check_table("distance_thresholds", distance_bins, distance_thresholds));
    mdx_tet *h = new mdx_tet();
    h->dev = dev;
    h->n0 = n_centers;
    h->n1 = n_neighbors;
    h->n_rows = n_rows;
    h->same = same != 0;
    h->keep_values = keep_values != 0;
    h->K = n_nearest;
    h->rc2 = cutoff * cutoff;
    h->bound0 = std::nextafter(h->rc2, HUGE_VAL);       // r2 < bound0 is r2 <= rc2
    h->box = box;
    h->q_bins = q_bins;
    h->s_bins = s_bins;
    h->d_bins = distance_bins;
    h->tables.assign(q_edges, q_edges + q_bins + 1);
    h->tables.insert(h->tables.end(), s_edges, s_edges + s_bins + 1);
    h->tables.insert(h->tables.end(), distance_thresholds, distance_thresholds + distance_bins + 1);
    tet_kernels_from<TET_MIN_NEAREST>(n_nearest, distance_bins <= TET_LDS_BINS, &h->select_kernel, &h->finish_kernel);
    *out = h;
    return MDX_OK;
}

int mdx_tet_set_chunk(mdx_tet_t h, int64_t candidates)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_REQUIRE(candidates >= 0 && candidates % TET_STAGE == 0 && candidates < (int64_t(1) << 31),
                "candidates must be 0 or a multiple of %d", TET_STAGE);
    MDX_REQUIRE(h->frames_seen == 0, "mdx_tet_set_chunk must be called before the first frame");
    h->pinned_chunk = candidates;
    return MDX_OK;
}

int mdx_tet_chunk_for(int64_t n_centers, int64_t n_neighbors, int64_t frames, int64_t compute_units, int64_t *chunk)
{
    MDX_REQUIRE(chunk, "NULL argument");
    MDX_REQUIRE(n_centers >= 1 && n_neighbors >= 1 && frames >= 1 && compute_units >= 1,
                "n_centers, n_neighbors, frames and compute_units must be at least 1");
    *chunk = tet_chunk_for(n_centers, n_neighbors, frames, compute_units);
    return MDX_OK;
}

// Written out, not MDX_FRAME_PLAN: the plan of this engine also holds the candidates per block of a full slab, and
// where no chunk is pinned that choice reads the compute units of the handle's device (no frame, and no device memory).
int mdx_tet_plan(mdx_tet_t h, int64_t *slab_frames, int64_t *ring_frames, int64_t *chunk)
{
    MDX_REQUIRE(h && slab_frames && ring_frames && chunk, "NULL argument");
    if (!h->pinned_chunk)
        MDX_TRY(tet_compute_units(h));
    *slab_frames = tet_slab(h);
    *ring_frames = 0;           // no frame outlives its slab
    *chunk = tet_launch_chunk(h, *slab_frames);
    return MDX_OK;
}

// what a route prepares before the first kernel
static int tet_prepare(mdx_tet *h, int64_t)
{
    MDX_TRY(tet_ensure_device(h));
    return tet_ensure_slab(h);
}

int mdx_tet_result(mdx_tet_t h, int64_t *q_counts, int64_t *s_counts, int64_t *outside, int64_t *distance_counts,
                   int64_t *distance_outside, int64_t *found)
{
    MDX_REQUIRE(h && q_counts && s_counts && outside && distance_counts && distance_outside && found, "NULL argument");
    MDX_TRY(tet_ensure_device(h));
    MDX_TRY(h->collect());
    MDX_TRY(tet_check(h));
    // uint64 counts of fewer than 2^63 values each: they fit an int64
    MDX_HIP(hipMemcpy(q_counts, h->q_words(), size_t(8) * h->q_bins, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(s_counts, h->s_words(), size_t(8) * h->s_bins, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(outside, h->outside_words(), 16, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(distance_counts, h->distance_words(), size_t(8) * h->K * h->d_bins, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(distance_outside, h->distance_outside_words(), size_t(8) * h->K, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(found, h->found_words(), size_t(8) * (h->K + 1), hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_tet_frames(mdx_tet_t h, double *sums, int64_t *counted, int64_t n)
{
    MDX_REQUIRE(h && ((sums && counted) || n == 0), "NULL argument");
    MDX_REQUIRE(n >= 0 && n <= h->frames_seen, "%lld frames asked for, %lld seen", (long long)n,
                (long long)h->frames_seen);
    if (n == 0)
        return MDX_OK;
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(tet_check(h));
    MDX_HIP(hipMemcpy(sums, h->d_frame_sums.ptr, size_t(16) * n, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(counted, h->d_counted.ptr, size_t(8) * n, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_tet_values(mdx_tet_t h, double *values, int32_t *neighbors, int64_t n)
{
    MDX_REQUIRE(h && ((values && neighbors) || n == 0), "NULL argument");
    MDX_REQUIRE(h->keep_values, "the values are kept only by an engine created with keep_values");
    MDX_REQUIRE(n >= 0 && n <= h->frames_seen, "%lld frames asked for, %lld seen", (long long)n,
                (long long)h->frames_seen);
    if (n == 0)
        return MDX_OK;
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(tet_check(h));
    std::memcpy(values, h->values.data(), size_t(16) * h->n0 * n);
    std::memcpy(neighbors, h->neighbors.data(), size_t(4) * h->K * h->n0 * n);
    return MDX_OK;
}

int mdx_tet_stats(mdx_tet_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *degenerate, int64_t *chunks)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    if (h->ready)
        MDX_TRY(tet_look(h));
    if (evaluations) *evaluations = h->frames_seen * (h->n0 * h->n1 - (h->same ? h->n0 : 0));
    if (degenerate) *degenerate = h->degenerate;
    if (chunks) *chunks = h->last_chunks;
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(tet, tet_prepare, tet_accumulate_rows)
MDX_LAZY_FRAME_LIFE_CYCLE(tet, tet_zero, tet_check)
MDX_FRAME_SET_SLAB_FRAMES(tet, TET_SLAB_MAX)
