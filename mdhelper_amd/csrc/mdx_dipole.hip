// mdx_dipole.hip — instantaneous dipole moments on gfx950 (MI355X).
//
// Carries DipoleMoment._single_frame (reference src/mdhelper/analysis/electrostatics.py:374-391): positions ->
// optional global unwrap (topology.py `unwrap`) -> per group the charge-weighted sum M = sum q x.  Contract and
// summation order: mdx_dipole_device.hpp; this unit is compiled with contraction off and spells its float64
// operations out.
//
// One pass over the positions at 12 B per atom-frame: a wave owns a tile of points for a slab of frames, carries the
// unwrap state in registers from frame to frame and writes one partial sum per (frame, tile); a second, small kernel
// adds a group's tiles in tile order.  Nothing of size frames x points goes to memory and nothing is added with
// atomics, so the rows repeat bit for bit whatever route the frames take and however they are split into calls or
// slabs.
#include "mdx_common.hpp"
#include "mdx_dipole_device.hpp"
#include "mdx_frame_entry.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_dip_dev;

namespace {

constexpr int64_t DIP_SLAB_FRAMES = 32768;                // frames per launch, at most
constexpr int64_t DIP_SCRATCH_BYTES = int64_t(256) << 20; // tile sums of one slab

}  // namespace

struct mdx_dip : FrameEngine {
    int n_groups = 0;
    int64_t n_points = 0, n_tiles = 0;
    int64_t row_capacity = 0;
    bool unwrap = false;
    double dims[3] = {0, 0, 0};
    std::vector<double> start;         // [n_points][3]: x_prev before the first frame
    DeviceBuffer d_tiles, d_tile_offsets, d_charges, d_rows, d_partial, d_prev, d_image;

    int64_t rows_wanted() const { return n_points; }
    const char *rows_noun() const { return "groups"; }
    void free_device() { release({&d_tiles, &d_tile_offsets, &d_charges, &d_rows, &d_partial, &d_prev, &d_image}); }
};

// frames per launch: the one asked for, or what the scratch holds of frames of 24 B per tile
static int64_t dip_slab(const mdx_dip *h)
{
    if (h->slab_frames > 0)
        return h->slab_frames;
    return std::min(DIP_SLAB_FRAMES, std::max<int64_t>(1, DIP_SCRATCH_BYTES / (24 * h->n_tiles)));
}

static int dip_grow_rows(mdx_dip *h, int64_t more)
{
    return grow_rows(h->d_rows, h->stream, int64_t(24) * h->n_groups, h->frames_seen, more, &h->row_capacity);
}

template <bool UNWRAP>
static void dip_launch(mdx_dip *h, const float *pos, int64_t src_rows, const int *index, int64_t nf)
{
    const int per_block = UNWRAP ? (int)nf : DIP_BLOCK_FRAMES;
    hipLaunchKernelGGL((dip_tile_kernel<UNWRAP>), dim3((unsigned)h->n_tiles, (unsigned)ceil_div(nf, per_block)),
                       dim3(UNWRAP ? 192 : 64), 0, h->stream, pos, src_rows, index, h->d_tiles.as<DipTile>(),
                       (int)h->n_tiles, h->d_charges.as<double>(), (int)nf, per_block, h->dims[0], h->dims[1],
                       h->dims[2], h->d_prev.as<double>(), h->d_image.as<int>(), h->d_partial.as<double>());
    hipLaunchKernelGGL(dip_fold_kernel, dim3((unsigned)ceil_div(nf * h->n_groups * 3, 256)), dim3(256), 0, h->stream,
                       h->d_partial.as<double>(), (int)h->n_tiles, h->d_tile_offsets.as<int>(), h->n_groups, nf,
                       h->d_rows.as<double>() + h->frames_seen * h->n_groups * 3);
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int dip_accumulate_rows(mdx_dip *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                               int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_points, "%lld rows given, the groups hold %lld", (long long)n_rows,
                (long long)h->n_points);
    MDX_TRY(dip_grow_rows(h, n_frames));
    const int64_t n = h->n_points;
    if (h->unwrap && h->frames_seen == 0) {
        // before the first frame x_prev is the starting configuration and the image counts are 0
        MDX_HIP(hipMemcpyAsync(h->d_prev.ptr, h->start.data(), size_t(24) * n, hipMemcpyHostToDevice, h->stream));
        MDX_HIP(hipMemsetAsync(h->d_image.ptr, 0, size_t(12) * n, h->stream));
    }
    const int64_t slab = dip_slab(h);
    hipEvent_t ev = h->timer.begin();
    for (int64_t f0 = 0; f0 < n_frames; f0 += slab) {
        const int64_t nf = std::min(slab, n_frames - f0);
        const float *pos = d_pos + f0 * src_rows * 3;
        MDX_TRY(h->d_partial.ensure(size_t(24) * h->n_tiles * nf));
        if (h->unwrap)
            dip_launch<true>(h, pos, src_rows, d_index, nf);
        else
            dip_launch<false>(h, pos, src_rows, d_index, nf);
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

extern "C" {

int mdx_dip_create(mdx_dip_t *out, int dev, int n_groups, const int64_t *n_points, const double *charges)
{
    MDX_REQUIRE(out && n_points && charges, "NULL argument");
    MDX_REQUIRE(n_groups >= 1 && n_groups <= 4096, "n_groups out of range");
    const int64_t limit = (int64_t(1) << 31) / 3;
    int64_t total = 0;
    for (int g = 0; g < n_groups; ++g) {
        MDX_REQUIRE(n_points[g] >= 1 && n_points[g] < limit - total,
                    "group %d: a group holds at least 1 point and all groups fewer than 2^31 / 3", g);
        total += n_points[g];
    }
    for (int64_t i = 0; i < total; ++i)
        MDX_REQUIRE(std::isfinite(charges[i]), "charges must be finite");
    // the tiles of every group and the groups' tile ranges
    std::vector<DipTile> tiles;
    std::vector<int32_t> tile_offsets{0};
    int64_t point = 0;
    for (int g = 0; g < n_groups; ++g) {
        for (int64_t j = 0; j < n_points[g]; j += DIP_TILE)
            tiles.push_back(DipTile{int(point + j), int(std::min<int64_t>(DIP_TILE, n_points[g] - j))});
        point += n_points[g];
        tile_offsets.push_back(int32_t(tiles.size()));
    }
    MDX_TRY(set_device(dev));
    mdx_dip *h = new mdx_dip();
    h->dev = dev;
    h->n_groups = n_groups;
    h->n_points = total;
    h->n_tiles = (int64_t)tiles.size();
    int rc = MDX_OK;
    do {
        if ((rc = stream_acquire(&h->stream)) != MDX_OK) break;
        h->timer.stream = h->stream;
        if ((rc = h->d_tiles.ensure(sizeof(DipTile) * tiles.size())) != MDX_OK) break;
        if ((rc = h->d_tile_offsets.ensure(size_t(4) * (n_groups + 1))) != MDX_OK) break;
        if ((rc = h->d_charges.ensure(size_t(8) * total)) != MDX_OK) break;
        if (hipMemcpy(h->d_tiles.ptr, tiles.data(), sizeof(DipTile) * tiles.size(), hipMemcpyHostToDevice) !=
                hipSuccess ||
            hipMemcpy(h->d_tile_offsets.ptr, tile_offsets.data(), size_t(4) * (n_groups + 1),
                      hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_charges.ptr, charges, size_t(8) * total, hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(MDX_ERR_HIP, "upload failed");
            break;
        }
    } while (0);
    if (rc != MDX_OK) {
        mdx_dip_destroy(h);
        return rc;
    }
    *out = h;
    return MDX_OK;
}

int mdx_dip_set_unwrap(mdx_dip_t h, const double *dims, const double *start)
{
    MDX_REQUIRE(h, "NULL handle");
    if (dims) {
        MDX_REQUIRE(start, "NULL argument");
        for (int k = 0; k < 3; ++k)
            MDX_REQUIRE(dims[k] > 0.0 && std::isfinite(dims[k]), "dims[%d] must be positive and finite", k);
    }
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_REQUIRE(h->frames_seen == 0, "mdx_dip_set_unwrap must be called before the first frame");
    if (!dims) {
        h->unwrap = false;
        return MDX_OK;
    }
    MDX_TRY(h->d_prev.ensure(size_t(24) * h->n_points));
    MDX_TRY(h->d_image.ensure(size_t(12) * h->n_points));
    h->start.assign(start, start + 3 * h->n_points);
    for (int k = 0; k < 3; ++k)
        h->dims[k] = dims[k];
    h->unwrap = true;
    return MDX_OK;
}

// its own rule: it may be called after the first frame, which the other engines' set_slab_frames refuses
int mdx_dip_set_slab_frames(mdx_dip_t h, int64_t frames)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_REQUIRE(frames >= 0 && frames <= DIP_SLAB_FRAMES, "frames must lie in [0, %lld]",
                (long long)DIP_SLAB_FRAMES);
    h->slab_frames = frames;
    return MDX_OK;
}

// what a route prepares before the first kernel
static int dip_prepare(mdx_dip *h, int64_t n_frames)
{
    MDX_TRY(set_device(h->dev));
    return dip_grow_rows(h, n_frames);
}

int mdx_dip_result(mdx_dip_t h, double *out)
{
    MDX_REQUIRE(h && out, "NULL argument");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    h->timer.collect();
    const int64_t F = h->frames_seen, G = h->n_groups;
    if (F == 0)
        return MDX_OK;
    std::vector<double> rows(size_t(F * G * 3));
    MDX_HIP(hipMemcpy(rows.data(), h->d_rows.ptr, size_t(24) * F * G, hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < G; ++g)
        for (int64_t f = 0; f < F; ++f)
            for (int k = 0; k < 3; ++k)
                out[(g * F + f) * 3 + k] = rows[size_t((f * G + g) * 3 + k)];
    return MDX_OK;
}

int mdx_dip_stats(mdx_dip_t h, int64_t *launches, double *kernel_ms, int64_t *frames)
{
    MDX_REQUIRE(h, "NULL handle");
    return h->stats(true, launches, kernel_ms, frames);
}

}  // extern "C"

MDX_FRAME_ROUTES(dip, dip_prepare, dip_accumulate_rows)
MDX_FRAME_LIFE_CYCLE(dip)
MDX_FRAME_RESET(dip)
MDX_FRAME_PLAN(dip, dip_slab)
