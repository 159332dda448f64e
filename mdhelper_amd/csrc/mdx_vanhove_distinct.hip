// mdx_vanhove_distinct.hip — distinct van Hove function G_d(r, t) on gfx950 (MI355X).
//
// Per lag the histogram of the minimum-image distances |x2_j(f0 + lag) - x1_i(f0)| over every pair (i of set 1,
// j of set 2, j != i when both are one set) and every frame pair (f0, f0 + lag) with f0 a multiple of origin_step.
// Contract, early rejection and kernel shape: mdx_vanhove_distinct_device.hpp; this unit is compiled with contraction
// off and spells its float64 operations out.
//
// The gathered float32 rows go into a ring of max(lags) + slab frames in HBM, so that a lag reaches back across
// slabs and calls.  Counts are integers added with integer atomics; nothing here adds floating-point numbers at all,
// so the counts are the same whatever route the frames take and however they are split into calls or slabs.
//
// A handle touches its device with the first frame (or result): creating one, and every argument error, needs none.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_lag_history.hpp"
#include "mdx_vanhove_distinct_device.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_vhd_dev;

namespace {

constexpr int64_t VHD_HISTORY_BYTES = int64_t(256) << 20;   // what the frames of a default slab take in the ring

}  // namespace

struct mdx_vhd : LazyFrameEngine {
    int n_bins = 0, keep = 7;
    bool same = false;
    int64_t n1 = 0, n2 = 0, n_rows = 0;         // n_rows: rows of an incoming frame (n1 with same, else n1 + n2)
    int64_t evaluations = 0;
    LagTable lags;
    LagRing ring;
    PairBox box;
    double inv_width = 0.0, r2_lo = 0.0, r2_hi = 0.0;
    std::vector<double> edges;
    DeviceBuffer d_edges, d_counts, d_ring;

    int64_t rows_wanted() const { return n_rows; }
    const char *rows_noun() const { return "sets"; }
    int64_t ring_lag() const { return lags.max_lag; }
    void clear_counters() { evaluations = 0; }
    void free_device() { release({&lags.d_lags, &d_edges, &d_counts, &d_ring}); }
};

static int64_t vhd_slab(const mdx_vhd *h)
{
    return pair_slab_frames(h->slab_frames, VHD_HISTORY_BYTES, 12 * h->n_rows);
}

static int vhd_zero(mdx_vhd *h)
{
    MDX_HIP(hipMemsetAsync(h->d_counts.ptr, 0, size_t(8) * h->lags.n() * h->n_bins, h->stream));
    return MDX_OK;
}

// the device side of the handle: tables and counters
static int vhd_build(mdx_vhd *h)
{
    MDX_TRY(h->d_edges.ensure(size_t(8) * (h->n_bins + 1)));
    MDX_TRY(h->d_counts.ensure(size_t(8) * h->lags.n() * h->n_bins));
    MDX_TRY(h->lags.upload());
    MDX_HIP(hipMemcpy(h->d_edges.ptr, h->edges.data(), size_t(8) * (h->n_bins + 1), hipMemcpyHostToDevice));
    return vhd_zero(h);
}

static int vhd_ensure_device(mdx_vhd *h) { return h->ensure_device(vhd_build); }

// what a route prepares before the first kernel: the device side, and before the first frame of a pass the ring
static int vhd_prepare(mdx_vhd *h, int64_t)
{
    MDX_TRY(vhd_ensure_device(h));
    MDX_TRY(h->ring.ensure(h->frames_seen, h->lags.max_lag, vhd_slab(h), 12 * h->n_rows,
                           "a history of %lld frames of %lld points is too large", (long long)h->n_rows));
    return h->d_ring.ensure(size_t(12) * h->n_rows * h->ring.cap);
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int vhd_accumulate_rows(mdx_vhd *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                               int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_rows, "%lld rows given, the sets hold %lld", (long long)n_rows, (long long)h->n_rows);
    const int n = (int)h->n_rows;
    const int64_t slab = h->ring.slab(vhd_slab(h)), cap = h->ring.cap;
    const bool lds = h->n_bins <= VHD_LDS_BINS;
    const size_t lds_bytes =
        size_t(32) * VHD_STAGE + (lds ? size_t(8) * (h->n_bins + 1) + size_t(4) * VHD_WAVES * h->n_bins : 0);
    const int64_t n_jchunks = ceil_div(h->n2, VHD_JCHUNK);
    const int64_t blocks = ceil_div(h->n1, VHD_TILE) * n_jchunks;
    const int64_t per_pair = h->n1 * h->n2 - (h->same ? h->n1 : 0);
    hipEvent_t ev = h->timer.begin();
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        const int64_t f0 = h->frames_seen;
        launch_gather<true>(h->stream, pos, src_rows, d_index, n, nf, h->d_ring.as<float>(), f0, cap);
        const dim3 grid((unsigned)blocks, (unsigned)h->lags.n(), (unsigned)nf);
        const auto kernel = lds ? (h->keep == 7 ? vhd_pair_kernel<true, true> : vhd_pair_kernel<true, false>)
                                : (h->keep == 7 ? vhd_pair_kernel<false, true> : vhd_pair_kernel<false, false>);
        hipLaunchKernelGGL(kernel, grid, dim3(VHD_THREADS), lds_bytes, h->stream, h->d_ring.as<float>(), cap, n,
                           (int)h->n1, (int)h->n2, h->same ? 0 : (int)h->n1, h->same ? 1 : 0, (int)n_jchunks,
                           h->lags.d_lags.as<int64_t>(), f0, h->lags.origin_step, h->box, h->keep,
                           h->d_edges.as<double>(), h->n_bins, h->inv_width, h->r2_lo, h->r2_hi,
                           h->d_counts.as<unsigned long long>());
        // the contract's pair count: origins f - lag that are multiples of origin_step, f among the new frames
        h->evaluations += per_pair * h->lags.origins_met(f0, nf);
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

extern "C" {

int mdx_vhd_create(mdx_vhd_t *out, int dev, int64_t n1, int64_t n2, int same, int n_bins, const double *edges,
                   int n_lags, const int64_t *lags, int64_t origin_step, const double *dims, int zero_dims)
{
    MDX_REQUIRE(out && edges && lags && dims, "NULL argument");
    MDX_REQUIRE(n_bins >= 1 && n_bins <= (1 << 24), "n_bins out of range");
    MDX_REQUIRE(n_lags >= 1, "lags must hold at least one lag");
    MDX_REQUIRE(n_lags <= VHD_LAGS_MAX, "at most %d lags", VHD_LAGS_MAX);
    MDX_REQUIRE(origin_step >= 1, "origin_step must be at least 1");
    MDX_REQUIRE(zero_dims >= 0 && zero_dims < 7, "zero_dims must leave at least one component");
    MDX_REQUIRE(n1 >= 1 && n2 >= 1, "both sets must hold at least one point");
    MDX_REQUIRE(!same || n1 == n2, "same: both sets are one set, but n1 = %lld and n2 = %lld", (long long)n1,
                (long long)n2);
    const int64_t limit = (int64_t(1) << 31) / 3;
    MDX_REQUIRE(n1 < limit && n2 < limit && (same ? n1 : n1 + n2) < limit,
                "the sets must hold fewer than 2^31 / 3 points");
    MDX_REQUIRE(ceil_div(n1, VHD_TILE) * ceil_div(n2, VHD_JCHUNK) < (int64_t(1) << 31),
                "%lld x %lld points are too many pairs for one launch", (long long)n1, (long long)n2);
    for (int b = 0; b <= n_bins; ++b) {
        MDX_REQUIRE(std::isfinite(edges[b]), "edges must be finite");
        MDX_REQUIRE(b == 0 || edges[b] > edges[b - 1], "edges must be strictly increasing");
    }
    MDX_TRY(LagTable::check(n_lags, lags));
    PairBox box;
    int keep = 7;
    MDX_TRY(check_box_cutoff(dims, zero_dims, edges[n_bins], &box, &keep,
                             "edges reach %g, beyond half the shortest box length %g"));
    MDX_REQUIRE(int64_t(n_lags) * n_bins < (int64_t(1) << 31), "too many counters");
    mdx_vhd *h = new mdx_vhd();
    h->dev = dev;
    h->n1 = n1;
    h->n2 = n2;
    h->same = same != 0;
    h->n_rows = same ? n1 : n1 + n2;
    h->n_bins = n_bins;
    h->keep = keep;
    h->box = box;
    h->lags.assign(n_lags, lags, origin_step);
    h->edges.assign(edges, edges + n_bins + 1);
    h->inv_width = double(n_bins) / (edges[n_bins] - edges[0]);
    // the margins of the early rejection (mdx_vanhove_distinct_device.hpp); an upper edge below 0 counts nothing
    const double lo = edges[0], hi = edges[n_bins], margin = std::ldexp(1.0, -40);
    h->r2_lo = lo > 0.0 ? (lo * lo) * (1.0 - margin) : 0.0;
    h->r2_hi = hi >= 0.0 ? (hi * hi) * (1.0 + margin) : -1.0;
    *out = h;
    return MDX_OK;
}

int mdx_vhd_result(mdx_vhd_t h, int64_t *counts)
{
    MDX_REQUIRE(h && counts, "NULL argument");
    MDX_TRY(vhd_ensure_device(h));
    MDX_TRY(h->collect());
    // uint64 counters of at most frame pairs x n1 x n2 < 2^63 each: they fit an int64
    MDX_HIP(hipMemcpy(counts, h->d_counts.ptr, size_t(8) * h->lags.n() * h->n_bins, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_vhd_stats(mdx_vhd_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    if (evaluations) *evaluations = h->evaluations;
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(vhd, vhd_prepare, vhd_accumulate_rows)
MDX_LAZY_FRAME_LIFE_CYCLE(vhd, vhd_zero, unchecked)
MDX_FRAME_SET_SLAB_FRAMES(vhd, VHD_SLAB_MAX)
MDX_FRAME_RING_PLAN(vhd, vhd_slab)
