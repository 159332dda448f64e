// mdx_hbond.hip — hydrogen bonds (donor-H...acceptor counts, geometry and lifetimes) on gfx950 (MI355X).
//
// Per frame the pairs (hydrogen i, acceptor j, the acceptor not the hydrogen's own donor) whose donor-acceptor
// minimum-image distance lies within the cutoff and whose angle at the hydrogen is wide enough, kept as capped
// per-hydrogen lists of acceptor numbers in a ring of frames in HBM; from the lists of a slab the histograms of the
// bonds' donor-acceptor distances and cosines and the distribution of the bonds a hydrogen donates; per lag the sizes
// of the intersections of an origin's bond set with the set of the frame a lag later (intermittent) and with the sets
// of every frame up to there (continuous), by the walk of the residence engine.  Contract, cap, kernel shapes and the
// bound that keeps the LDS counters from wrapping: mdx_hbond_device.hpp; this unit is compiled with contraction off
// and spells its float64 operations out.
//
// Every result is an integer added with integer atomics, and set membership does not depend on the order in which a
// row was filled, so the results are the same whatever route the frames take and however they are split into calls or
// slabs.
//
// A handle touches its device with the first frame (or result): creating one, and every argument error, needs none.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_lag_history.hpp"
#include "mdx_hbond_device.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_hb_dev;
using mdx_prs_dev::prs_walk_kernel;

namespace {

constexpr int64_t HB_HISTORY_BYTES = int64_t(256) << 20;    // what the frames of a default slab take in HBM
constexpr int64_t HB_MAX_BINS = int64_t(1) << 20;

}  // namespace

struct mdx_hb : LazyFrameEngine {
    int keep = 7;
    bool lds_hist = true;
    int64_t n_rows = 0, n_h = 0, n_a = 0;
    int64_t excluded = 0;               // the (i, j) with a_row[j] == d_row[i]
    int64_t n_r = 1, n_c = 1;           // bins of the two histograms
    LagTable lags;
    LagRing ring;                       // frames the rings hold
    PairBox box;
    CappedLists lists;                  // the rings of bond lists
    SurvivalWalk walk;
    double rc2 = 0.0, cos_max = 0.0;
    std::vector<int32_t> tables;        // h_row [n_h], d_row [n_h], a_row [n_a]
    std::vector<double> inner;          // the inner thresholds of r2_DA [n_r - 1], then those of c [n_c - 1]
    // d_bonds: uint64, one per frame seen;
    // d_geometry: uint64 distance_counts [n_r], cosine_counts [n_c], donated [max_nb + 1], degenerate [1]
    DeviceBuffer d_bonds, d_slab, d_tables, d_inner, d_geometry;

    int64_t geometry_words() const { return n_r + n_c + lists.max_nb + 2; }

    int64_t rows_wanted() const { return n_rows; }
    const char *rows_noun() const { return "tables"; }
    int64_t ring_lag() const { return lags.max_lag; }
    void clear_counters() { lists.max_row = 0; }
    void free_device()
    {
        release({&lags.d_lags, &walk.d_sums, &d_bonds, &lists.d_ctl, &d_slab, &lists.d_len, &lists.d_list, &walk.d_mask,
                 &d_tables, &d_inner, &d_geometry});
    }
};

// bytes a frame takes: its gathered rows while it is in flight, its lists and masks while it is in the rings
static int64_t hb_frame_bytes(const mdx_hb *h)
{
    return 12 * h->n_rows + (int64_t(h->lists.max_nb) + 1) * 4 * h->n_h + 8 * h->n_h;
}

static int64_t hb_slab(const mdx_hb *h)
{
    return pair_slab_frames(h->slab_frames, HB_HISTORY_BYTES, hb_frame_bytes(h));
}

static int hb_zero(mdx_hb *h)
{
    MDX_TRY(h->walk.zero(h->lags.n(), h->stream));
    MDX_HIP(hipMemsetAsync(h->d_geometry.ptr, 0, size_t(8) * h->geometry_words(), h->stream));
    if (h->d_bonds.ptr)
        MDX_HIP(hipMemsetAsync(h->d_bonds.ptr, 0, h->d_bonds.bytes, h->stream));
    return h->lists.zero(h->stream);
}

// the thresholds and the counters that go with them, with the stream idle
static int hb_upload_bins(mdx_hb *h)
{
    MDX_TRY(h->d_inner.ensure(size_t(8) * std::max<size_t>(h->inner.size(), 1)));
    MDX_TRY(h->d_geometry.ensure(size_t(8) * h->geometry_words()));
    if (!h->inner.empty())
        MDX_HIP(hipMemcpy(h->d_inner.ptr, h->inner.data(), size_t(8) * h->inner.size(), hipMemcpyHostToDevice));
    return MDX_OK;
}

// the device side of the handle: tables and counters
static int hb_build(mdx_hb *h)
{
    MDX_TRY(h->walk.ensure(h->lags.n()));
    MDX_TRY(h->d_tables.ensure(size_t(4) * h->tables.size()));
    MDX_TRY(h->lists.ensure_ctl());
    MDX_TRY(hb_upload_bins(h));
    MDX_TRY(h->lags.upload());
    MDX_HIP(hipMemcpy(h->d_tables.ptr, h->tables.data(), size_t(4) * h->tables.size(), hipMemcpyHostToDevice));
    return hb_zero(h);
}

static int hb_ensure_device(mdx_hb *h) { return h->ensure_device(hb_build); }

// What a route prepares before the first kernel: the device side, and before the first frame of a pass the rings and
// the slab.
static int hb_prepare(mdx_hb *h, int64_t)
{
    MDX_TRY(hb_ensure_device(h));
    MDX_TRY(h->ring.ensure(h->frames_seen, h->lags.max_lag, hb_slab(h), hb_frame_bytes(h),
                           "a history of %lld frames of %lld hydrogens with %d neighbors each is too large",
                           (long long)h->n_h, h->lists.max_nb));
    MDX_TRY(h->d_slab.ensure(size_t(12) * h->n_rows * h->ring.slab(hb_slab(h))));
    MDX_TRY(h->lists.ensure(h->n_h, h->ring.cap));
    return h->walk.ensure_mask(h->n_h, h->ring.cap);
}

// With the stream idle: the largest row seen; a row beyond the cap refuses the results until a reset.
static int hb_check_rows(mdx_hb *h)
{
    return h->lists.check("hydrogen", "bonds");
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int hb_accumulate_rows(mdx_hb *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                              int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_rows, "%lld rows given, the tables name %lld", (long long)n_rows,
                (long long)h->n_rows);
    MDX_TRY(grow_frames(h->d_bonds, h->stream, 8, h->frames_seen, h->frames_seen + n_frames));
    const int n = (int)h->n_rows, n_h = (int)h->n_h, n_a = (int)h->n_a, max_nb = h->lists.max_nb;
    int *len = h->lists.d_len.as<int>(), *list = h->lists.d_list.as<int>();
    const int *h_row = h->d_tables.as<int>(), *d_row = h_row + h->n_h, *a_row = d_row + h->n_h;
    const double *inner_r = h->d_inner.as<double>(), *inner_c = inner_r + (h->n_r - 1);
    unsigned long long *distance_counts = h->d_geometry.as<unsigned long long>();
    unsigned long long *cosine_counts = distance_counts + h->n_r, *donated = cosine_counts + h->n_c;
    unsigned long long *degenerate = donated + max_nb + 1;
    const int64_t slab = h->ring.slab(hb_slab(h)), cap = h->ring.cap;
    const int64_t n_jchunks = ceil_div(h->n_a, HB_JCHUNK);
    const int64_t blocks = ceil_div(h->n_h, HB_TILE) * n_jchunks;
    const int64_t geo_tiles = ceil_div(h->n_h, HB_GEO_THREADS);
    hipEvent_t ev = h->timer.begin();
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        const int64_t f_lo = h->frames_seen;
        launch_gather<false>(h->stream, pos, src_rows, d_index, n, nf, h->d_slab.as<float>());
        // the rows of the new frames start empty
        MDX_TRY(h->ring.zero_slots(len, size_t(4) * n_h, f_lo, nf, h->stream));
        const auto contact = h->keep == 7 ? hb_contact_kernel<true> : hb_contact_kernel<false>;
        hipLaunchKernelGGL(contact, dim3((unsigned)blocks, 1, (unsigned)nf), dim3(HB_THREADS), 0, h->stream,
                           h->d_slab.as<float>(), cap, n, n_h, n_a, h_row, d_row, a_row, (int)n_jchunks, f_lo,
                           h->box, h->keep, h->rc2, h->cos_max, max_nb, len, list,
                           h->d_bonds.as<unsigned long long>(), h->lists.d_ctl.as<int>(), degenerate);
        const auto geometry = h->lds_hist ? hb_geometry_kernel<true> : hb_geometry_kernel<false>;
        hipLaunchKernelGGL(geometry, dim3((unsigned)geo_tiles, (unsigned)nf), dim3(HB_GEO_THREADS), 0, h->stream,
                           h->d_slab.as<float>(), cap, n, n_h, h_row, d_row, a_row, f_lo, h->box, h->keep, max_nb,
                           len, list, inner_r, (int)h->n_r, inner_c, (int)h->n_c, distance_counts, cosine_counts,
                           donated);
        h->walk.walk(prs_walk_kernel<true>, prs_walk_kernel<false>, h->stream, h->lags, h->ring, h->lists, n_h, f_lo,
                     nf);
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

extern "C" {

int mdx_hb_create(mdx_hb_t *out, int dev, int64_t n_rows, int64_t n_h, const int32_t *h_row, const int32_t *d_row,
                  int64_t n_a, const int32_t *a_row, double distance, double cos_max, int n_lags, const int64_t *lags,
                  int64_t origin_step, const double *dims, int zero_dims, int max_neighbors, int continuous)
{
    MDX_REQUIRE(out && h_row && d_row && a_row && lags && dims, "NULL argument");
    MDX_REQUIRE(n_lags >= 1, "lags must hold at least one lag");
    MDX_REQUIRE(n_lags < (1 << 24), "at most 2^24 lags");
    MDX_REQUIRE(origin_step >= 1, "origin_step must be at least 1");
    MDX_REQUIRE(zero_dims >= 0 && zero_dims < 7, "zero_dims must leave at least one component");
    MDX_REQUIRE(max_neighbors >= 1 && max_neighbors <= HB_MAX_NEIGHBORS, "max_neighbors must lie in [1, %d]",
                HB_MAX_NEIGHBORS);
    MDX_REQUIRE(n_h >= 1 && n_a >= 1, "there must be at least one hydrogen and one acceptor");
    const int64_t limit = (int64_t(1) << 31) / 3;
    MDX_REQUIRE(n_rows >= 1 && n_rows < limit && n_h < limit && n_a < limit,
                "the frames and the tables must hold fewer than 2^31 / 3 rows");
    MDX_REQUIRE(ceil_div(n_h, HB_TILE) * ceil_div(n_a, HB_JCHUNK) < (int64_t(1) << 31),
                "%lld hydrogens and %lld acceptors are too many pairs for one launch", (long long)n_h, (long long)n_a);
    MDX_TRY(LagTable::check(n_lags, lags));
    // what a row is: 1 a hydrogen, 2 an acceptor
    std::vector<char> role((size_t)n_rows, 0);
    for (int64_t i = 0; i < n_h; ++i) {
        MDX_REQUIRE(h_row[i] >= 0 && h_row[i] < n_rows, "h_row[%lld] = %d out of range [0, %lld)", (long long)i,
                    h_row[i], (long long)n_rows);
        MDX_REQUIRE(d_row[i] >= 0 && d_row[i] < n_rows, "d_row[%lld] = %d out of range [0, %lld)", (long long)i,
                    d_row[i], (long long)n_rows);
        MDX_REQUIRE(d_row[i] != h_row[i], "hydrogen %lld (row %d) is its own donor", (long long)i, h_row[i]);
        MDX_REQUIRE(!role[h_row[i]], "row %d is a hydrogen twice", h_row[i]);
        role[h_row[i]] = 1;
    }
    for (int64_t j = 0; j < n_a; ++j) {
        MDX_REQUIRE(a_row[j] >= 0 && a_row[j] < n_rows, "a_row[%lld] = %d out of range [0, %lld)", (long long)j,
                    a_row[j], (long long)n_rows);
        MDX_REQUIRE(role[a_row[j]] != 2, "row %d is an acceptor twice", a_row[j]);
        MDX_REQUIRE(role[a_row[j]] != 1, "row %d is both a hydrogen and an acceptor", a_row[j]);
        role[a_row[j]] = 2;
    }
    int64_t excluded = 0;               // a_row holds no row twice: at most one j per hydrogen
    for (int64_t i = 0; i < n_h; ++i)
        excluded += role[d_row[i]] == 2;
    MDX_REQUIRE(distance > 0.0 && std::isfinite(distance), "distance must be positive and finite");
    MDX_REQUIRE(cos_max >= -1.0 && cos_max <= 1.0, "cos_max must lie in [-1, 1]");
    PairBox box;
    int keep = 7;
    MDX_TRY(check_box_cutoff(dims, zero_dims, distance, &box, &keep,
                             "distance %g reaches beyond half the shortest box length %g"));
    mdx_hb *h = new mdx_hb();
    h->dev = dev;
    h->n_rows = n_rows;
    h->n_h = n_h;
    h->n_a = n_a;
    h->excluded = excluded;
    h->walk.continuous = continuous != 0;
    h->keep = keep;
    h->box = box;
    h->lists.max_nb = max_neighbors;
    h->lags.assign(n_lags, lags, origin_step);
    h->rc2 = distance * distance;
    h->cos_max = cos_max;
    h->tables.assign(h_row, h_row + n_h);
    h->tables.insert(h->tables.end(), d_row, d_row + n_h);
    h->tables.insert(h->tables.end(), a_row, a_row + n_a);
    *out = h;
    return MDX_OK;
}

int mdx_hb_set_bins(mdx_hb_t h, int64_t n_r, const double *r2_thresholds, int64_t n_c, const double *cos_thresholds)
{
    MDX_REQUIRE(h && r2_thresholds && cos_thresholds, "NULL argument");
    MDX_REQUIRE(h->frames_seen == 0, "mdx_hb_set_bins must be called before the first frame");
    MDX_REQUIRE(n_r >= 1 && n_r <= HB_MAX_BINS && n_c >= 1 && n_c <= HB_MAX_BINS, "n_r and n_c must lie in [1, %lld]",
                (long long)HB_MAX_BINS);
    for (int64_t m = 0; m < n_r; ++m)
        MDX_REQUIRE(r2_thresholds[m] < r2_thresholds[m + 1],
                    "r2_thresholds must be strictly increasing: [%lld] = %g, [%lld] = %g", (long long)m,
                    r2_thresholds[m], (long long)(m + 1), r2_thresholds[m + 1]);
    for (int64_t m = 0; m < n_c; ++m)
        MDX_REQUIRE(cos_thresholds[m] > cos_thresholds[m + 1],
                    "cos_thresholds must be strictly decreasing: [%lld] = %g, [%lld] = %g", (long long)m,
                    cos_thresholds[m], (long long)(m + 1), cos_thresholds[m + 1]);
    h->n_r = n_r;
    h->n_c = n_c;
    h->lds_hist = n_r <= HB_LDS_BINS && n_c <= HB_LDS_BINS;
    h->inner.assign(r2_thresholds + 1, r2_thresholds + n_r);
    h->inner.insert(h->inner.end(), cos_thresholds + 1, cos_thresholds + n_c);
    if (!h->ready)
        return MDX_OK;
    // a handle that has touched its device without a frame (a result, a reset): the counters take their new sizes
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(hb_upload_bins(h));
    MDX_TRY(hb_zero(h));
    MDX_HIP(hipStreamSynchronize(h->stream));
    return MDX_OK;
}

int mdx_hb_result(mdx_hb_t h, int64_t *intermittent, int64_t *continuous, int64_t *origin_counts)
{
    MDX_REQUIRE(h && intermittent && continuous && origin_counts, "NULL argument");
    MDX_TRY(hb_ensure_device(h));
    MDX_TRY(h->collect());
    MDX_TRY(hb_check_rows(h));
    // sums of at most frames x n_h x max_neighbors each
    return h->walk.result(h->lags.n(), intermittent, continuous, origin_counts);
}

int mdx_hb_bonds(mdx_hb_t h, int64_t *out, int64_t n)
{
    MDX_REQUIRE(h && (out || n == 0), "NULL argument");
    MDX_REQUIRE(n >= 0 && n <= h->frames_seen, "%lld frames asked for, %lld seen", (long long)n,
                (long long)h->frames_seen);
    if (n == 0)
        return MDX_OK;
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(hb_check_rows(h));
    MDX_HIP(hipMemcpy(out, h->d_bonds.ptr, size_t(8) * n, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_hb_geometry(mdx_hb_t h, int64_t *distance_counts, int64_t *cosine_counts, int64_t *donated)
{
    MDX_REQUIRE(h && distance_counts && cosine_counts && donated, "NULL argument");
    MDX_TRY(hb_ensure_device(h));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(hb_check_rows(h));
    // uint64 counts of fewer than 2^63 bonds each: they fit an int64
    const char *src = h->d_geometry.as<char>();
    MDX_HIP(hipMemcpy(distance_counts, src, size_t(8) * h->n_r, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(cosine_counts, src + 8 * h->n_r, size_t(8) * h->n_c, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(donated, src + 8 * (h->n_r + h->n_c), size_t(8) * (h->lists.max_nb + 1), hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_hb_stats(mdx_hb_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                 int64_t *max_row, int64_t *degenerate)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    uint64_t seen = 0;
    if (h->ready) {
        MDX_TRY(h->lists.look());
        if (degenerate)
            MDX_HIP(hipMemcpy(&seen, h->d_geometry.as<uint64_t>() + h->geometry_words() - 1, 8,
                              hipMemcpyDeviceToHost));
    }
    if (evaluations) *evaluations = h->frames_seen * (h->n_h * h->n_a - h->excluded);
    if (max_row) *max_row = h->lists.max_row;
    if (degenerate) *degenerate = int64_t(seen);
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(hb, hb_prepare, hb_accumulate_rows)
MDX_LAZY_FRAME_LIFE_CYCLE(hb, hb_zero, hb_check_rows)
MDX_FRAME_SET_SLAB_FRAMES(hb, HB_SLAB_MAX)
MDX_FRAME_RING_PLAN(hb, hb_slab)
