// mdx_cluster.hip — ion clusters (connected components of a contact graph) on gfx950 (MI355X).
//
// Per frame the bonds between the rows of one or several species (minimum-image distance within the cutoff of the
// two species), kept as capped per-row lists in HBM; from the lists the connected components (label = the smallest
// row of the component) and from the labels the cluster-size distribution, the per-species membership by cluster
// size and per-frame cluster counts.  Contract, cap, kernel shapes and why the labelling ends with the minimum:
// mdx_cluster_device.hpp; this unit is compiled with contraction off and spells its float64 operations out.
//
// Every result is an integer added with integer atomics, so the results are the same whatever route the frames take
// and however they are split into calls or slabs.
//
// A handle touches its device with the first frame (or result): creating one, and every argument error, needs none.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_pairs_host.hpp"
#include "mdx_cluster_device.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_clu_dev;

namespace {

constexpr int64_t CLU_SLAB_BYTES = int64_t(256) << 20;  // what the frames of a default slab take in HBM
constexpr int CLU_SWEEP_BATCH = 4;                      // sweeps queued between two looks at their "lowered" words

}  // namespace

struct mdx_clu : LazyFrameEngine {
    int n_species = 1, keep = 7;
    bool uniform = true, keep_labels = false;
    int64_t n = 0;
    int64_t sweeps = 0;
    PairBox box;
    CappedLists lists;                  // d_ctl: int32 max_row, then the "lowered" words of a batch of sweeps
    double rc2 = 0.0;                   // the one squared cutoff of a uniform table
    double table[CLU_MAX_SPECIES * CLU_MAX_SPECIES];    // rc2 at [8 * b + a], -1.0 where the species never bond
    std::vector<int32_t> species;
    // d_counts: uint64 [1 + G][n + 1], size_counts then species_counts; d_frames: uint64 [frames][CLU_FRAME_WORDS];
    // d_labels: int32 [frames][n] (keep_labels)
    DeviceBuffer d_species, d_table, d_counts, d_frames, d_labels, d_slab, d_label, d_size;

    int64_t rows_wanted() const { return n; }
    const char *rows_noun() const { return "groups"; }
    void clear_counters() { sweeps = lists.max_row = 0; }
    void free_device()
    {
        release({&d_species, &d_table, &d_counts, &d_frames, &d_labels, &lists.d_ctl, &d_slab, &lists.d_len,
                 &lists.d_list, &d_label, &d_size});
    }
};

// bytes a frame of a slab takes: its gathered rows, its lists and lengths, its labels and sizes
static int64_t clu_frame_bytes(const mdx_clu *h)
{
    return 12 * h->n + (int64_t(h->lists.max_nb) + 1) * 4 * h->n + 8 * h->n;
}

static int64_t clu_slab(const mdx_clu *h)
{
    return pair_slab_frames(h->slab_frames, CLU_SLAB_BYTES, clu_frame_bytes(h));
}

static int clu_zero(mdx_clu *h)
{
    MDX_HIP(hipMemsetAsync(h->d_counts.ptr, 0, size_t(8) * (1 + h->n_species) * (h->n + 1), h->stream));
    if (h->d_frames.ptr)
        MDX_HIP(hipMemsetAsync(h->d_frames.ptr, 0, h->d_frames.bytes, h->stream));
    return h->lists.zero(h->stream);
}

// the device side of the handle: tables and counters
static int clu_build(mdx_clu *h)
{
    MDX_TRY(h->d_species.ensure(size_t(4) * h->n));
    MDX_TRY(h->d_table.ensure(sizeof(h->table)));
    MDX_TRY(h->d_counts.ensure(size_t(8) * (1 + h->n_species) * (h->n + 1)));
    MDX_TRY(h->lists.ensure_ctl());
    MDX_HIP(hipMemcpy(h->d_species.ptr, h->species.data(), size_t(4) * h->n, hipMemcpyHostToDevice));
    MDX_HIP(hipMemcpy(h->d_table.ptr, h->table, sizeof(h->table), hipMemcpyHostToDevice));
    return clu_zero(h);
}

static int clu_ensure_device(mdx_clu *h) { return h->ensure_device(clu_build); }

// The buffers of a slab, sized before the first frame of a pass.  Nothing is in flight then (a reset waits for the
// stream), so growing them loses nothing.
static int clu_ensure_slab(mdx_clu *h)
{
    if (h->frames_seen > 0)
        return MDX_OK;
    const int64_t slab = clu_slab(h);
    MDX_REQUIRE(slab < (int64_t(1) << 40) / clu_frame_bytes(h),
                "a slab of %lld frames of %lld points with %d neighbors each is too large", (long long)slab,
                (long long)h->n, h->lists.max_nb);
    MDX_TRY(h->d_slab.ensure(size_t(12) * h->n * slab));
    MDX_TRY(h->lists.ensure(h->n, slab));
    MDX_TRY(h->d_label.ensure(size_t(4) * h->n * slab));
    MDX_TRY(h->d_size.ensure(size_t(4) * h->n * slab));
    return MDX_OK;
}

// With the stream idle: the largest row seen; a row beyond the cap refuses the results until a reset.
static int clu_check_rows(mdx_clu *h)
{
    return h->lists.check("row", "bonds");
}

// Labels the nf frames of the slab whose lists are queued on the stream: sweeps in batches, until one lowered
// nothing.  *labelled = false where a row of the slab (or an earlier one) went beyond the cap: the lists are then
// truncated, the results refused, and nothing more is done with the slab.  Returns with the stream idle.
static int clu_label_slab(mdx_clu *h, int64_t nf, hipEvent_t *ev, bool *labelled)
{
    const int n = (int)h->n;
    const dim3 grid((unsigned)ceil_div(h->n, CLU_ROW_THREADS), (unsigned)nf);
    int *ctl = h->lists.d_ctl.as<int>();
    int32_t seen[1 + CLU_SWEEP_BATCH];
    *labelled = false;
    for (int64_t done = 0;;) {
        MDX_HIP(hipMemsetAsync(ctl + 1, 0, size_t(4) * CLU_SWEEP_BATCH, h->stream));
        for (int b = 0; b < CLU_SWEEP_BATCH; ++b)
            hipLaunchKernelGGL(clu_sweep_kernel, grid, dim3(CLU_ROW_THREADS), 0, h->stream, n, h->lists.max_nb,
                               h->lists.d_len.as<int>(), h->lists.d_list.as<int>(), h->d_label.as<int>(),
                               ctl + 1 + b);
        h->timer.end(*ev);
        MDX_HIP(hipGetLastError());
        MDX_HIP(hipStreamSynchronize(h->stream));
        MDX_HIP(hipMemcpy(seen, ctl, sizeof(seen), hipMemcpyDeviceToHost));
        *ev = h->timer.begin();
        h->lists.max_row = seen[0];
        if (seen[0] > h->lists.max_nb)
            return MDX_OK;
        for (int b = 0; b < CLU_SWEEP_BATCH; ++b) {
            ++done;
            ++h->sweeps;
            if (!seen[1 + b]) {
                *labelled = true;       // a whole sweep lowered nothing
                return MDX_OK;
            }
            if (done > h->n)
                return fail(MDX_ERR_INTERNAL, "the labelling of %lld points did not settle in %lld sweeps",
                            (long long)h->n, (long long)done);
        }
    }
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int clu_accumulate_rows(mdx_clu *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                               int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n, "%lld rows given, the groups hold %lld", (long long)n_rows, (long long)h->n);
    MDX_TRY(grow_frames(h->d_frames, h->stream, size_t(8) * CLU_FRAME_WORDS, h->frames_seen,
                        h->frames_seen + n_frames));
    if (h->keep_labels)
        MDX_TRY(grow_frames(h->d_labels, h->stream, size_t(4) * h->n, h->frames_seen, h->frames_seen + n_frames));
    const int n = (int)h->n;
    const int64_t slab = clu_slab(h);       // what clu_ensure_slab sized the buffers for
    const int64_t n_jchunks = ceil_div(h->n, CLU_JCHUNK);
    const int64_t blocks = ceil_div(h->n, CLU_TILE) * n_jchunks;
    const int64_t row_tiles = ceil_div(h->n, CLU_ROW_THREADS);
    unsigned long long *counts = h->d_counts.as<unsigned long long>();
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        const int64_t f_lo = h->frames_seen;
        hipEvent_t ev = h->timer.begin();
        launch_gather<false>(h->stream, pos, src_rows, d_index, n, nf, h->d_slab.as<float>(), 0, 1,
                             CluStart{h->d_label.as<int>(), h->d_size.as<int>()});
        MDX_HIP(hipMemsetAsync(h->lists.d_len.ptr, 0, size_t(4) * n * nf, h->stream));
        const auto contact = h->uniform
                                 ? (h->keep == 7 ? clu_contact_kernel<true, true> : clu_contact_kernel<false, true>)
                                 : (h->keep == 7 ? clu_contact_kernel<true, false> : clu_contact_kernel<false, false>);
        hipLaunchKernelGGL(contact, dim3((unsigned)blocks, 1, (unsigned)nf), dim3(CLU_THREADS), 0, h->stream,
                           h->d_slab.as<float>(), n, (int)n_jchunks, f_lo, h->box, h->keep, h->rc2,
                           h->d_table.as<double>(), h->d_species.as<int>(), h->lists.max_nb,
                           h->lists.d_len.as<int>(), h->lists.d_list.as<int>(),
                           h->d_frames.as<unsigned long long>(), h->lists.d_ctl.as<int>());
        h->frames_seen += nf;
        bool labelled = false;
        // a row beyond the cap: the results are refused until a reset; only max_row goes on
        if (h->lists.max_row <= h->lists.max_nb) {
            const int rc = clu_label_slab(h, nf, &ev, &labelled);
            if (rc != MDX_OK) {
                h->timer.end(ev);
                return rc;
            }
        }
        if (labelled) {
            const dim3 grid((unsigned)row_tiles, (unsigned)nf);
            hipLaunchKernelGGL(clu_size_kernel, grid, dim3(CLU_ROW_THREADS), 0, h->stream, n, h->d_label.as<int>(),
                               h->d_size.as<int>());
            hipLaunchKernelGGL(clu_tally_kernel, grid, dim3(CLU_ROW_THREADS), 0, h->stream, n, f_lo,
                               h->d_label.as<int>(), h->d_size.as<int>(), h->d_species.as<int>(), counts,
                               counts + (h->n + 1), h->d_frames.as<unsigned long long>());
            if (h->keep_labels)
                MDX_HIP(hipMemcpyAsync(h->d_labels.as<int>() + f_lo * h->n, h->d_label.ptr, size_t(4) * n * nf,
                                       hipMemcpyDeviceToDevice, h->stream));
        }
        h->timer.end(ev);
        MDX_HIP(hipGetLastError());
    }
    return MDX_OK;
}

extern "C" {

int mdx_clu_create(mdx_clu_t *out, int dev, int64_t n, const int32_t *species, int n_species, const double *cutoff,
                   const double *dims, int zero_dims, int max_neighbors, int keep_labels)
{
    MDX_REQUIRE(out && species && cutoff && dims, "NULL argument");
    MDX_REQUIRE(n_species >= 1 && n_species <= CLU_MAX_SPECIES, "n_species must lie in [1, %d]", CLU_MAX_SPECIES);
    MDX_REQUIRE(zero_dims >= 0 && zero_dims < 7, "zero_dims must leave at least one component");
    MDX_REQUIRE(max_neighbors >= 1 && max_neighbors <= CLU_MAX_NEIGHBORS, "max_neighbors must lie in [1, %d]",
                CLU_MAX_NEIGHBORS);
    MDX_REQUIRE(n >= 1, "the groups must hold at least one point");
    MDX_REQUIRE(n < (int64_t(1) << 31) / 3, "the groups must hold fewer than 2^31 / 3 points");
    MDX_REQUIRE(ceil_div(n, CLU_TILE) * ceil_div(n, CLU_JCHUNK) < (int64_t(1) << 31),
                "%lld points are too many pairs for one launch", (long long)n);
    for (int64_t i = 0; i < n; ++i)
        MDX_REQUIRE(species[i] >= 0 && species[i] < n_species, "species[%lld] = %d out of range [0, %d)",
                    (long long)i, species[i], n_species);
    const int G = n_species;
    double largest = 0.0;
    bool uniform = true;
    for (int a = 0; a < G; ++a)
        for (int b = 0; b < G; ++b) {
            const double c = cutoff[a * G + b];
            MDX_REQUIRE(c >= 0.0 && std::isfinite(c), "cutoff[%d][%d] must be finite and not negative", a, b);
            MDX_REQUIRE(c == cutoff[b * G + a], "the cutoff table must be symmetric: [%d][%d] = %g, [%d][%d] = %g", a,
                        b, c, b, a, cutoff[b * G + a]);
            largest = std::max(largest, c);
            uniform = uniform && c == cutoff[0];
        }
    MDX_REQUIRE(largest > 0.0, "the cutoff table must hold at least one positive entry");
    PairBox box;
    int keep = 7;
    MDX_TRY(check_box_cutoff(dims, zero_dims, largest, &box, &keep));
    mdx_clu *h = new mdx_clu();
    h->dev = dev;
    h->n = n;
    h->n_species = G;
    h->keep = keep;
    h->box = box;
    h->lists.max_nb = max_neighbors;
    h->lists.ctl_words = 1 + CLU_SWEEP_BATCH;
    h->keep_labels = keep_labels != 0;
    h->species.assign(species, species + n);
    h->uniform = uniform;               // every entry is the one positive value
    h->rc2 = cutoff[0] * cutoff[0];
    for (double &t : h->table)
        t = -1.0;
    for (int a = 0; a < G; ++a)
        for (int b = 0; b < G; ++b)
            if (cutoff[a * G + b] > 0.0)
                h->table[CLU_MAX_SPECIES * b + a] = cutoff[a * G + b] * cutoff[a * G + b];
    *out = h;
    return MDX_OK;
}

// what a route prepares before the first kernel
static int clu_prepare(mdx_clu *h, int64_t)
{
    MDX_TRY(clu_ensure_device(h));
    return clu_ensure_slab(h);
}

int mdx_clu_result(mdx_clu_t h, int64_t *size_counts, int64_t *species_counts)
{
    MDX_REQUIRE(h && size_counts && species_counts, "NULL argument");
    MDX_TRY(clu_ensure_device(h));
    MDX_TRY(h->collect());
    MDX_TRY(clu_check_rows(h));
    // uint64 counts of at most frames x n < 2^63 each: they fit an int64
    const size_t bytes = size_t(8) * (h->n + 1);
    MDX_HIP(hipMemcpy(size_counts, h->d_counts.ptr, bytes, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(species_counts, h->d_counts.as<char>() + bytes, bytes * h->n_species, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_clu_frames(mdx_clu_t h, int64_t *bonds, int64_t *n_clusters, int64_t *largest, int64_t *sum_squares,
                   int64_t n)
{
    MDX_REQUIRE(h && ((bonds && n_clusters && largest && sum_squares) || n == 0), "NULL argument");
    MDX_REQUIRE(n >= 0 && n <= h->frames_seen, "%lld frames asked for, %lld seen", (long long)n,
                (long long)h->frames_seen);
    if (n == 0)
        return MDX_OK;
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(clu_check_rows(h));
    std::vector<uint64_t> words(size_t(CLU_FRAME_WORDS) * n);
    MDX_HIP(hipMemcpy(words.data(), h->d_frames.ptr, size_t(8) * words.size(), hipMemcpyDeviceToHost));
    for (int64_t f = 0; f < n; ++f) {
        const uint64_t *w = words.data() + CLU_FRAME_WORDS * f;
        bonds[f] = int64_t(w[0] / 2);       // the kernel counts a bond from both ends
        n_clusters[f] = int64_t(w[1]);
        largest[f] = int64_t(w[2]);
        sum_squares[f] = int64_t(w[3]);
    }
    return MDX_OK;
}

int mdx_clu_labels(mdx_clu_t h, int32_t *out, int64_t n)
{
    MDX_REQUIRE(h && (out || n == 0), "NULL argument");
    MDX_REQUIRE(h->keep_labels, "the handle was created without keep_labels");
    MDX_REQUIRE(n >= 0 && n <= h->frames_seen, "%lld frames asked for, %lld seen", (long long)n,
                (long long)h->frames_seen);
    if (n == 0)
        return MDX_OK;
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(clu_check_rows(h));
    MDX_HIP(hipMemcpy(out, h->d_labels.ptr, size_t(4) * h->n * n, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_clu_stats(mdx_clu_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *max_row, int64_t *sweeps)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    if (h->ready)
        MDX_TRY(h->lists.look());
    if (evaluations) *evaluations = h->frames_seen * (h->n * (h->n - 1) / 2);
    if (max_row) *max_row = h->lists.max_row;
    if (sweeps) *sweeps = h->sweeps;
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(clu, clu_prepare, clu_accumulate_rows)
MDX_LAZY_FRAME_LIFE_CYCLE(clu, clu_zero, clu_check_rows)
MDX_FRAME_SET_SLAB_FRAMES(clu, CLU_SLAB_MAX)
MDX_FRAME_PLAN(clu, clu_slab)
