// mdx_orient.hip — orientational relaxation (P1 / P2 reorientation of unit vectors) on gfx950 (MI355X).
//
// Per frame the unit vectors between pairs of rows (tail -> head, with the minimum image where a box is set), per lag
// and vector the sums of the first and second Legendre polynomials of u(f) . u(f - lag) over the frames, and per frame
// and group the sums of the six products u_a u_b from which the class forms the order tensor.  Contract, kernel shape
// and summation order: mdx_orient_device.hpp; this unit is compiled with contraction off and spells its float64
// operations out.
//
// The unit vectors go into a ring of max(lags) + slab frames in HBM, so that a lag reaches back across slabs and
// calls; every (lag, vector) has one accumulator that receives its terms in frame order.  Nothing is added with
// floating-point atomics, so the sums repeat bit for bit whatever route the frames take and however they are split
// into calls or slabs.
//
// A handle touches its device with the first frame (or result): creating one, and every argument error, needs none.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_lag_history.hpp"
#include "mdx_orient_device.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_ori_dev;

namespace {

constexpr int64_t ORI_HISTORY_BYTES = int64_t(256) << 20;   // what the frames of a default slab take in the ring

}  // namespace

struct mdx_ori : LazyFrameEngine {
    int n_groups = 0, keep = 7;
    int64_t n_vectors = 0, n_rows = 0;
    int64_t evaluations = 0;
    int64_t degenerate = 0;             // degenerate vectors seen, as of the last look
    LagTable lags;
    LagRing ring;
    bool boxed = false;
    PairBox box = {{0, 0, 0}, {0, 0, 0}};
    std::vector<OriTile> tiles;
    std::vector<int> tile_offsets, pairs;
    std::vector<int64_t> offsets;
    // d_frame_sums: double [frames seen][n_groups][6]; d_part: double [slab][tiles][6]; d_ctl: uint64 degenerate
    DeviceBuffer d_tiles, d_tile_offsets, d_pairs, d_offsets, d_acc, d_sums, d_hist, d_part, d_frame_sums, d_ctl;

    int64_t rows_wanted() const { return n_rows; }
    const char *rows_noun() const { return "pairs"; }
    int64_t ring_lag() const { return lags.max_lag; }
    void clear_counters() { evaluations = degenerate = 0; }
    void free_device()
    {
        release({&d_tiles, &d_tile_offsets, &d_pairs, &d_offsets, &lags.d_lags, &d_acc, &d_sums, &d_hist, &d_part,
                 &d_frame_sums, &d_ctl});
    }
};

static int64_t ori_slab(const mdx_ori *h)
{
    if (h->slab_frames > 0)
        return h->slab_frames;
    return std::min(ORI_SLAB_MAX, std::max<int64_t>(1, ORI_HISTORY_BYTES / (24 * h->n_vectors)));
}

static int ori_zero(mdx_ori *h)
{
    MDX_HIP(hipMemsetAsync(h->d_acc.ptr, 0, size_t(16) * h->lags.n() * h->n_vectors, h->stream));
    MDX_HIP(hipMemsetAsync(h->d_ctl.ptr, 0, 8, h->stream));
    if (h->d_frame_sums.ptr)
        MDX_HIP(hipMemsetAsync(h->d_frame_sums.ptr, 0, h->d_frame_sums.bytes, h->stream));
    h->degenerate = 0;
    return MDX_OK;
}

// the device side of the handle: tables, counter and accumulators
static int ori_build(mdx_ori *h)
{
    MDX_TRY(h->d_tiles.ensure(sizeof(OriTile) * h->tiles.size()));
    MDX_TRY(h->d_tile_offsets.ensure(size_t(4) * (h->n_groups + 1)));
    MDX_TRY(h->d_pairs.ensure(size_t(8) * h->n_vectors));
    MDX_TRY(h->d_offsets.ensure(size_t(8) * (h->n_groups + 1)));
    MDX_TRY(h->d_acc.ensure(size_t(16) * h->lags.n() * h->n_vectors));
    MDX_TRY(h->d_sums.ensure(size_t(16) * h->lags.n() * h->n_groups));
    MDX_TRY(h->d_ctl.ensure(8));
    MDX_HIP(hipMemcpy(h->d_tiles.ptr, h->tiles.data(), sizeof(OriTile) * h->tiles.size(), hipMemcpyHostToDevice));
    MDX_HIP(hipMemcpy(h->d_tile_offsets.ptr, h->tile_offsets.data(), size_t(4) * (h->n_groups + 1),
                      hipMemcpyHostToDevice));
    MDX_HIP(hipMemcpy(h->d_pairs.ptr, h->pairs.data(), size_t(8) * h->n_vectors, hipMemcpyHostToDevice));
    MDX_HIP(hipMemcpy(h->d_offsets.ptr, h->offsets.data(), size_t(8) * (h->n_groups + 1), hipMemcpyHostToDevice));
    MDX_TRY(h->lags.upload());
    return ori_zero(h);
}

static int ori_ensure_device(mdx_ori *h) { return h->ensure_device(ori_build); }

// What a route prepares before the first kernel: the device side, and before the first frame of a pass the ring and
// the tile partials of a slab.
static int ori_prepare(mdx_ori *h, int64_t)
{
    MDX_TRY(ori_ensure_device(h));
    MDX_TRY(h->ring.ensure(h->frames_seen, h->lags.max_lag, ori_slab(h), 24 * h->n_vectors,
                           "a history of %lld frames of %lld vectors is too large", (long long)h->n_vectors));
    MDX_TRY(h->d_hist.ensure(size_t(24) * h->n_vectors * h->ring.cap));
    return h->d_part.ensure(size_t(48) * h->tiles.size() * h->ring.slab(ori_slab(h)));
}

// With the stream idle: the degenerate vectors seen; one of them refuses the results until a reset.
static int ori_look(mdx_ori *h)
{
    unsigned long long seen = 0;
    MDX_HIP(hipMemcpy(&seen, h->d_ctl.ptr, 8, hipMemcpyDeviceToHost));
    h->degenerate = (int64_t)seen;
    return MDX_OK;
}

static int ori_check(mdx_ori *h)
{
    MDX_TRY(ori_look(h));
    MDX_REQUIRE(h->degenerate == 0,
                "%lld vectors had no direction (head on its tail, or a length that is not finite): their averages "
                "are undefined (reset starts over)", (long long)h->degenerate);
    return MDX_OK;
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int ori_accumulate_rows(mdx_ori *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                               int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_rows, "%lld rows given, the pairs hold %lld", (long long)n_rows,
                (long long)h->n_rows);
    MDX_TRY(grow_frames(h->d_frame_sums, h->stream, size_t(48) * h->n_groups, h->frames_seen,
                        h->frames_seen + n_frames));
    const int n = (int)h->n_vectors, n_tiles = (int)h->tiles.size();
    const int64_t slab = h->ring.slab(ori_slab(h)), cap = h->ring.cap;
    const dim3 cor_grid((unsigned)n_tiles, (unsigned)ceil_div(h->lags.n(), ORI_BLOCK_LAGS));
    const auto prepare = h->boxed ? ori_prepare_kernel<true> : ori_prepare_kernel<false>;
    hipEvent_t ev = h->timer.begin();
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        const int64_t f0 = h->frames_seen;
        hipLaunchKernelGGL(prepare, dim3((unsigned)ceil_div(n_tiles, ORI_BLOCK_TILES), (unsigned)nf),
                           dim3(ORI_TILE * ORI_BLOCK_TILES), 0, h->stream, pos, src_rows, d_index,
                           h->d_pairs.as<int>(), h->d_tiles.as<OriTile>(), n_tiles, n, f0, cap, h->box, h->keep,
                           h->d_hist.as<double>(), h->d_part.as<double>(), h->d_ctl.as<unsigned long long>());
        hipLaunchKernelGGL(ori_group_kernel, dim3((unsigned)ceil_div(nf * h->n_groups * 6, 256)), dim3(256), 0,
                           h->stream, h->d_part.as<double>(), n_tiles, h->d_tile_offsets.as<int>(), h->n_groups,
                           (int)nf, f0, h->d_frame_sums.as<double>());
        hipLaunchKernelGGL(ori_correlate_kernel, cor_grid, dim3(ORI_THREADS), 0, h->stream, h->d_hist.as<double>(),
                           cap, n, h->d_tiles.as<OriTile>(), h->lags.d_lags.as<int64_t>(), h->lags.n(), f0, f0 + nf,
                           h->d_acc.as<double>());
        h->evaluations += h->n_vectors * h->lags.origins_met(f0, nf);
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

extern "C" {

int mdx_ori_create(mdx_ori_t *out, int dev, int n_groups, const int64_t *n_vectors, int64_t n_rows,
                   const int32_t *pairs, int n_lags, const int64_t *lags, int zero_dims)
{
    MDX_REQUIRE(out && n_vectors && pairs && lags, "NULL argument");
    MDX_REQUIRE(n_groups >= 1 && n_groups <= 4096, "n_groups out of range");
    MDX_REQUIRE(n_lags >= 1 && n_lags <= (1 << 24), "lags must hold at least one lag");
    MDX_REQUIRE(zero_dims >= 0 && zero_dims < 7, "zero_dims must leave at least one component");
    const int64_t limit = (int64_t(1) << 31) / 3;
    MDX_REQUIRE(n_rows >= 2 && n_rows < limit, "n_rows must lie in [2, 2^31 / 3)");
    int64_t total = 0;
    for (int g = 0; g < n_groups; ++g) {
        MDX_REQUIRE(n_vectors[g] >= 0 && n_vectors[g] < limit - total,
                    "group %d: a group size is not negative and all groups hold fewer than 2^31 / 3 vectors", g);
        total += n_vectors[g];
    }
    MDX_REQUIRE(total >= 1, "the groups hold no vector");
    for (int64_t v = 0; v < total; ++v) {
        const int32_t tail = pairs[2 * v], head = pairs[2 * v + 1];
        MDX_REQUIRE(tail >= 0 && tail < n_rows && head >= 0 && head < n_rows,
                    "vector %lld: pair (%d, %d) out of range [0, %lld)", (long long)v, tail, head, (long long)n_rows);
        MDX_REQUIRE(tail != head, "vector %lld: row %d is both tail and head", (long long)v, tail);
    }
    MDX_TRY(LagTable::check(n_lags, lags));
    MDX_REQUIRE(int64_t(n_lags) * n_groups < (int64_t(1) << 30), "too many sums");
    mdx_ori *h = new mdx_ori();
    h->dev = dev;
    h->n_groups = n_groups;
    h->keep = 7 & ~zero_dims;
    h->n_vectors = total;
    h->n_rows = n_rows;
    h->lags.assign(n_lags, lags);
    h->pairs.assign(pairs, pairs + 2 * total);
    // the tiles of every group (a tile never spans two groups) and the groups' vector and tile ranges
    h->offsets.push_back(0);
    h->tile_offsets.push_back(0);
    int64_t vector = 0;
    for (int g = 0; g < n_groups; ++g) {
        for (int64_t j = 0; j < n_vectors[g]; j += ORI_TILE)
            h->tiles.push_back(OriTile{int(vector + j), int(std::min<int64_t>(ORI_TILE, n_vectors[g] - j)), g});
        vector += n_vectors[g];
        h->offsets.push_back(vector);
        h->tile_offsets.push_back((int)h->tiles.size());
    }
    *out = h;
    return MDX_OK;
}

int mdx_ori_set_box(mdx_ori_t h, const double *dims)
{
    MDX_REQUIRE(h, "NULL handle");
    if (dims)
        for (int c = 0; c < 3; ++c)
            MDX_REQUIRE(dims[c] > 0.0 && std::isfinite(dims[c]), "dims[%d] must be positive and finite", c);
    MDX_REQUIRE(h->frames_seen == 0, "mdx_ori_set_box must be called before the first frame");
    h->boxed = dims != nullptr;
    for (int c = 0; c < 3; ++c) {
        h->box.L[c] = dims ? dims[c] : 0.0;
        h->box.inv[c] = dims ? 1.0 / dims[c] : 0.0;
    }
    return MDX_OK;
}

int mdx_ori_result(mdx_ori_t h, double *sums)
{
    MDX_REQUIRE(h && sums, "NULL argument");
    MDX_TRY(ori_ensure_device(h));
    hipLaunchKernelGGL(ori_fold_kernel, dim3((unsigned)ceil_div(int64_t(2) * h->lags.n() * h->n_groups, 256)),
                       dim3(256), 0, h->stream, h->d_acc.as<double>(), (int)h->n_vectors,
                       h->d_offsets.as<int64_t>(), h->n_groups, h->lags.n(), h->d_sums.as<double>());
    MDX_TRY(h->collect());
    MDX_TRY(ori_check(h));
    MDX_HIP(hipMemcpy(sums, h->d_sums.ptr, size_t(16) * h->lags.n() * h->n_groups, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_ori_vector_sums(mdx_ori_t h, double *out)
{
    MDX_REQUIRE(h && out, "NULL argument");
    MDX_TRY(ori_ensure_device(h));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(ori_check(h));
    MDX_HIP(hipMemcpy(out, h->d_acc.ptr, size_t(16) * h->lags.n() * h->n_vectors, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_ori_frame_sums(mdx_ori_t h, double *out, int64_t n)
{
    MDX_REQUIRE(h && (out || n == 0), "NULL argument");
    MDX_REQUIRE(n >= 0 && n <= h->frames_seen, "%lld frames asked for, %lld seen", (long long)n,
                (long long)h->frames_seen);
    if (n == 0)
        return MDX_OK;
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(ori_check(h));
    MDX_HIP(hipMemcpy(out, h->d_frame_sums.ptr, size_t(48) * h->n_groups * n, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_ori_stats(mdx_ori_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *degenerate)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    if (h->ready)
        MDX_TRY(ori_look(h));
    if (evaluations) *evaluations = h->evaluations;
    if (degenerate) *degenerate = h->degenerate;
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(ori, ori_prepare, ori_accumulate_rows)
MDX_LAZY_FRAME_LIFE_CYCLE(ori, ori_zero, ori_check)
MDX_FRAME_SET_SLAB_FRAMES(ori, ORI_SLAB_MAX)
MDX_FRAME_RING_PLAN(ori, ori_slab)
