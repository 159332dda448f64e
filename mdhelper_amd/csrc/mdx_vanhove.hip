// mdx_vanhove.hip — self van Hove function and displacement moments on gfx950 (MI355X).
//
// Per lag and group the histogram of the displacement magnitudes |x(f) - x(f - lag)| of every point and frame, and
// per lag and point the sums of their second and fourth powers, from which the class forms G_s(r, t), the mean
// squared displacement and the non-Gaussian parameter.  Contract, kernel shape and summation order:
// mdx_vanhove_device.hpp; this unit is compiled with contraction off and spells its float64 operations out.
//
// The widened (and unwrapped) points go into a ring of max(lags) + slab frames in HBM, so that a lag reaches back
// across slabs and calls; counts are integers, the moments have one accumulator per (lag, point) that receives its
// terms in frame order.  Nothing is added with floating-point atomics, so counts and moments repeat bit for bit
// whatever route the frames take and however they are split into calls or slabs.
//
// A handle touches its device with the first frame (or result): creating one, and every argument error, needs none.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_lag_history.hpp"
#include "mdx_vanhove_device.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_vh_dev;

namespace {

constexpr int64_t VH_HISTORY_BYTES = int64_t(256) << 20;    // what the frames of a default slab take in the ring

}  // namespace

struct mdx_vh : LazyFrameEngine {
    int n_groups = 0, n_bins = 0, keep = 7;
    int64_t n_points = 0;
    int64_t evaluations = 0;
    LagTable lags;
    LagRing ring;
    UnwrappedHistory hist;
    double inv_width = 0.0;
    std::vector<VhTile> tiles;
    std::vector<int64_t> offsets;
    std::vector<double> edges;
    DeviceBuffer d_tiles, d_offsets, d_edges, d_counts, d_acc, d_moments;

    int64_t rows_wanted() const { return n_points; }
    const char *rows_noun() const { return "groups"; }
    int64_t ring_lag() const { return lags.max_lag; }
    void clear_counters() { evaluations = 0; }
    void free_device()
    {
        release({&d_tiles, &d_offsets, &lags.d_lags, &d_edges, &d_counts, &d_acc, &d_moments, &hist.d_hist,
                 &hist.d_prev, &hist.d_image});
    }
};

static int64_t vh_slab(const mdx_vh *h)
{
    if (h->slab_frames > 0)
        return h->slab_frames;
    return std::min(VH_SLAB_MAX, std::max<int64_t>(1, VH_HISTORY_BYTES / (24 * h->n_points)));
}

static int vh_zero(mdx_vh *h)
{
    MDX_HIP(hipMemsetAsync(h->d_counts.ptr, 0, size_t(8) * h->lags.n() * h->n_groups * h->n_bins, h->stream));
    MDX_HIP(hipMemsetAsync(h->d_acc.ptr, 0, size_t(16) * h->lags.n() * h->n_points, h->stream));
    return MDX_OK;
}

// the device side of the handle: tables, counters and accumulators
static int vh_build(mdx_vh *h)
{
    MDX_TRY(h->d_tiles.ensure(sizeof(VhTile) * h->tiles.size()));
    MDX_TRY(h->d_offsets.ensure(size_t(8) * (h->n_groups + 1)));
    MDX_TRY(h->d_edges.ensure(size_t(8) * (h->n_bins + 1)));
    MDX_TRY(h->d_counts.ensure(size_t(8) * h->lags.n() * h->n_groups * h->n_bins));
    MDX_TRY(h->d_acc.ensure(size_t(16) * h->lags.n() * h->n_points));
    MDX_TRY(h->d_moments.ensure(size_t(16) * h->lags.n() * h->n_groups));
    MDX_TRY(h->hist.ensure_state(h->n_points));
    MDX_HIP(hipMemcpy(h->d_tiles.ptr, h->tiles.data(), sizeof(VhTile) * h->tiles.size(), hipMemcpyHostToDevice));
    MDX_HIP(hipMemcpy(h->d_offsets.ptr, h->offsets.data(), size_t(8) * (h->n_groups + 1), hipMemcpyHostToDevice));
    MDX_TRY(h->lags.upload());
    MDX_HIP(hipMemcpy(h->d_edges.ptr, h->edges.data(), size_t(8) * (h->n_bins + 1), hipMemcpyHostToDevice));
    return vh_zero(h);
}

static int vh_ensure_device(mdx_vh *h) { return h->ensure_device(vh_build); }

// what a route prepares before the first kernel: the device side, and before the first frame of a pass the ring
static int vh_prepare(mdx_vh *h, int64_t)
{
    MDX_TRY(vh_ensure_device(h));
    MDX_TRY(h->ring.ensure(h->frames_seen, h->lags.max_lag, vh_slab(h), 24 * h->n_points,
                           "a history of %lld frames of %lld points is too large", (long long)h->n_points));
    return h->hist.ensure_ring(h->n_points, h->ring.cap);
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int vh_accumulate_rows(mdx_vh *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                              int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_points, "%lld rows given, the groups hold %lld", (long long)n_rows,
                (long long)h->n_points);
    const int n = (int)h->n_points;
    const int64_t slab = h->ring.slab(vh_slab(h)), cap = h->ring.cap;
    const bool lds = h->n_bins <= VH_LDS_BINS;
    const size_t lds_bytes = lds ? size_t(4) * VH_BLOCK_LAGS * h->n_bins : 0;
    const dim3 bin_grid((unsigned)h->tiles.size(), (unsigned)ceil_div(h->lags.n(), VH_BLOCK_LAGS));
    hipEvent_t ev = h->timer.begin();
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        const int64_t f0 = h->frames_seen;
        h->hist.prepare(vh_prepare_kernel<true>, vh_prepare_kernel<false>, h->stream, pos, src_rows, d_index, n, nf, f0,
                        cap);
        if (lds)
            hipLaunchKernelGGL(vh_bin_kernel<true>, bin_grid, dim3(VH_THREADS), lds_bytes, h->stream,
                               h->hist.d_hist.as<double>(), cap, n, h->d_tiles.as<VhTile>(),
                               h->lags.d_lags.as<int64_t>(), h->lags.n(), f0, f0 + nf, h->keep,
                               h->d_edges.as<double>(), h->n_bins, h->inv_width, h->n_groups,
                               h->d_counts.as<unsigned long long>(), h->d_acc.as<double>());
        else
            hipLaunchKernelGGL(vh_bin_kernel<false>, bin_grid, dim3(VH_THREADS), 0, h->stream,
                               h->hist.d_hist.as<double>(), cap, n, h->d_tiles.as<VhTile>(),
                               h->lags.d_lags.as<int64_t>(), h->lags.n(), f0, f0 + nf, h->keep,
                               h->d_edges.as<double>(), h->n_bins, h->inv_width, h->n_groups,
                               h->d_counts.as<unsigned long long>(), h->d_acc.as<double>());
        h->evaluations += h->n_points * h->lags.origins_met(f0, nf);
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

extern "C" {

int mdx_vh_create(mdx_vh_t *out, int dev, int n_groups, const int64_t *n_points, int n_bins, const double *edges,
                  int n_lags, const int64_t *lags, int zero_dims)
{
    MDX_REQUIRE(out && n_points && edges && lags, "NULL argument");
    MDX_REQUIRE(n_groups >= 1 && n_groups <= 4096, "n_groups out of range");
    MDX_REQUIRE(n_bins >= 1 && n_bins <= (1 << 24), "n_bins out of range");
    MDX_REQUIRE(n_lags >= 1 && n_lags <= (1 << 24), "lags must hold at least one lag");
    MDX_REQUIRE(zero_dims >= 0 && zero_dims < 7, "zero_dims must leave at least one component");
    const int64_t limit = (int64_t(1) << 31) / 3;
    int64_t total = 0;
    for (int g = 0; g < n_groups; ++g) {
        MDX_REQUIRE(n_points[g] >= 0 && n_points[g] < limit - total,
                    "group %d: a group size is not negative and all groups hold fewer than 2^31 / 3 points", g);
        total += n_points[g];
    }
    MDX_REQUIRE(total >= 1, "the groups hold no point");
    for (int b = 0; b <= n_bins; ++b) {
        MDX_REQUIRE(std::isfinite(edges[b]), "edges must be finite");
        MDX_REQUIRE(b == 0 || edges[b] > edges[b - 1], "edges must be strictly increasing");
    }
    MDX_TRY(LagTable::check(n_lags, lags));
    MDX_REQUIRE(int64_t(n_lags) * n_groups * n_bins < (int64_t(1) << 31), "too many counters");
    mdx_vh *h = new mdx_vh();
    h->dev = dev;
    h->n_groups = n_groups;
    h->n_bins = n_bins;
    h->keep = 7 & ~zero_dims;
    h->n_points = total;
    h->lags.assign(n_lags, lags);
    h->edges.assign(edges, edges + n_bins + 1);
    h->inv_width = double(n_bins) / (edges[n_bins] - edges[0]);
    // the tiles of every group (a tile never spans two groups) and the groups' point ranges
    h->offsets.push_back(0);
    int64_t point = 0;
    for (int g = 0; g < n_groups; ++g) {
        for (int64_t j = 0; j < n_points[g]; j += VH_TILE)
            h->tiles.push_back(VhTile{int(point + j), int(std::min<int64_t>(VH_TILE, n_points[g] - j)), g});
        point += n_points[g];
        h->offsets.push_back(point);
    }
    *out = h;
    return MDX_OK;
}

int mdx_vh_set_unwrap(mdx_vh_t h, const double *dims)
{
    MDX_REQUIRE(h, "NULL handle");
    return h->hist.set_unwrap(dims, h->frames_seen, "mdx_vh_set_unwrap");
}

int mdx_vh_result(mdx_vh_t h, int64_t *counts, double *moments)
{
    MDX_REQUIRE(h && counts, "NULL argument");
    MDX_TRY(vh_ensure_device(h));
    if (moments)
        hipLaunchKernelGGL(vh_fold_kernel, dim3((unsigned)ceil_div(int64_t(2) * h->lags.n() * h->n_groups, 256)),
                           dim3(256), 0, h->stream, h->d_acc.as<double>(), (int)h->n_points,
                           h->d_offsets.as<int64_t>(), h->n_groups, h->lags.n(), h->d_moments.as<double>());
    MDX_TRY(h->collect());
    // uint64 counters of at most frames x points each: they fit an int64
    MDX_HIP(hipMemcpy(counts, h->d_counts.ptr, size_t(8) * h->lags.n() * h->n_groups * h->n_bins,
                      hipMemcpyDeviceToHost));
    if (moments)
        MDX_HIP(hipMemcpy(moments, h->d_moments.ptr, size_t(16) * h->lags.n() * h->n_groups, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_vh_point_moments(mdx_vh_t h, double *out)
{
    MDX_REQUIRE(h && out, "NULL argument");
    MDX_TRY(vh_ensure_device(h));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_HIP(hipMemcpy(out, h->d_acc.ptr, size_t(16) * h->lags.n() * h->n_points, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_vh_stats(mdx_vh_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    if (evaluations) *evaluations = h->evaluations;
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(vh, vh_prepare, vh_accumulate_rows)
MDX_LAZY_FRAME_LIFE_CYCLE(vh, vh_zero, unchecked)
MDX_FRAME_SET_SLAB_FRAMES(vh, VH_SLAB_MAX)
MDX_FRAME_RING_PLAN(vh, vh_slab)
