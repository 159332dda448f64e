// mdx_sdf.hip — spatial distribution functions (3-D densities in a molecule's own frame) on gfx950 (MI355X).
//
// Per frame every reference molecule forms a body-fixed frame from three of its atoms (origin, axis atom, plane
// atom); every partner atom within the cutoff of the origin, not of the molecule itself, is rotated into that frame
// and counted in a three-dimensional histogram per partner group, with numpy.histogramdd's counts.  Contract and
// kernel shape: mdx_sdf_device.hpp; this unit is compiled with contraction off and spells its float64 operations out.
//
// Every result is an integer added with integer atomics, so the results are the same whatever route the frames take
// and however they are split into calls or slabs.
//
// A handle touches its device with the first frame (or result): creating one, and every argument error, needs none.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_pairs_host.hpp"
#include "mdx_sdf_device.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

using namespace mdx;
using namespace mdx_sdf_dev;

namespace {

constexpr int64_t SDF_SLAB_BYTES = int64_t(256) << 20;  // what the frames of a default slab take in HBM

}  // namespace

struct mdx_sdf : LazyFrameEngine {
    int n_groups = 1, mode = SDF_AXIS;
    int64_t n_rows = 0, n_ref = 0, n_p = 0;
    int64_t excluded = 0;               // the (i, j) with owner[j] == i
    PairBox box;
    double rc2 = 0.0;
    SdfGroups groups;
    SdfAxes axes;
    std::vector<int32_t> tables;        // o_row, a_row, b_row [n_ref], p_row, owner [n_p]
    std::vector<double> edges;          // ex [nx + 1], ey [ny + 1], ez [nz + 1]
    // d_counts: uint64 counts [G][nx][ny][nz], degenerate [1]; d_inside: uint64, one per frame seen
    DeviceBuffer d_tables, d_edges, d_counts, d_inside, d_slab;

    int64_t cells() const { return int64_t(n_groups) * axes.n[0] * axes.n[1] * axes.n[2]; }
    int64_t rows_wanted() const { return n_rows; }
    const char *rows_noun() const { return "tables"; }
    void free_device() { release({&d_tables, &d_edges, &d_counts, &d_inside, &d_slab}); }
};

static int64_t sdf_slab(const mdx_sdf *h)
{
    return pair_slab_frames(h->slab_frames, SDF_SLAB_BYTES, 12 * h->n_rows);
}

static int sdf_zero(mdx_sdf *h)
{
    MDX_HIP(hipMemsetAsync(h->d_counts.ptr, 0, size_t(8) * (h->cells() + 1), h->stream));
    if (h->d_inside.ptr)
        MDX_HIP(hipMemsetAsync(h->d_inside.ptr, 0, h->d_inside.bytes, h->stream));
    return MDX_OK;
}

// the edges and the counters that go with them, with the stream idle
static int sdf_upload_bins(mdx_sdf *h)
{
    MDX_TRY(h->d_edges.ensure(size_t(8) * h->edges.size()));
    MDX_TRY(h->d_counts.ensure(size_t(8) * (h->cells() + 1)));
    MDX_HIP(hipMemcpy(h->d_edges.ptr, h->edges.data(), size_t(8) * h->edges.size(), hipMemcpyHostToDevice));
    return MDX_OK;
}

// the device side of the handle: tables, edges and counters
static int sdf_build(mdx_sdf *h)
{
    MDX_TRY(h->d_tables.ensure(size_t(4) * h->tables.size()));
    MDX_TRY(sdf_upload_bins(h));
    MDX_HIP(hipMemcpy(h->d_tables.ptr, h->tables.data(), size_t(4) * h->tables.size(), hipMemcpyHostToDevice));
    return sdf_zero(h);
}

static int sdf_ensure_device(mdx_sdf *h) { return h->ensure_device(sdf_build); }

// What a route prepares before the first kernel: the device side, and before the first frame of a pass the slab
// (nothing is in flight then: a reset waits for the stream).
static int sdf_prepare(mdx_sdf *h, int64_t)
{
    MDX_TRY(sdf_ensure_device(h));
    if (h->frames_seen > 0)
        return MDX_OK;
    return h->d_slab.ensure(size_t(12) * h->n_rows * sdf_slab(h));
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int sdf_accumulate_rows(mdx_sdf *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                               int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_rows, "%lld rows given, the tables name %lld", (long long)n_rows,
                (long long)h->n_rows);
    MDX_TRY(grow_frames(h->d_inside, h->stream, 8, h->frames_seen, h->frames_seen + n_frames));
    const int n = (int)h->n_rows, n_ref = (int)h->n_ref, n_p = (int)h->n_p;
    const int *o_row = h->d_tables.as<int>(), *a_row = o_row + h->n_ref, *b_row = a_row + h->n_ref;
    const int *p_row = b_row + h->n_ref, *owner = p_row + h->n_p;
    unsigned long long *counts = h->d_counts.as<unsigned long long>(), *degenerate = counts + h->cells();
    const int64_t slab = sdf_slab(h);       // what sdf_prepare sized the slab for
    const int64_t n_jchunks = ceil_div(h->n_p, SDF_JCHUNK);
    const int64_t blocks = ceil_div(h->n_ref, SDF_TILE) * n_jchunks;
    const auto pairs = h->mode == SDF_BISECTOR ? sdf_pair_kernel<true> : sdf_pair_kernel<false>;
    hipEvent_t ev = h->timer.begin();
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        launch_gather<false>(h->stream, pos, src_rows, d_index, n, nf, h->d_slab.as<float>());
        hipLaunchKernelGGL(pairs, dim3((unsigned)blocks, 1, (unsigned)nf), dim3(SDF_THREADS), 0, h->stream,
                           h->d_slab.as<float>(), n, n_ref, n_p, o_row, a_row, b_row, p_row, owner, (int)n_jchunks,
                           h->frames_seen, h->box, h->rc2, h->groups, h->d_edges.as<double>(), h->axes, counts,
                           h->d_inside.as<unsigned long long>(), degenerate);
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

// one axis of mdx_sdf_set_bins: n bins, n + 1 strictly increasing finite edges
static int sdf_check_edges(const char *name, int64_t n, const double *e)
{
    MDX_REQUIRE(n >= 1 && n <= SDF_MAX_AXIS_BINS, "n%c must lie in [1, %d]", name[1], SDF_MAX_AXIS_BINS);
    for (int64_t m = 0; m <= n; ++m)
        MDX_REQUIRE(std::isfinite(e[m]), "%s[%lld] must be finite", name, (long long)m);
    for (int64_t m = 0; m < n; ++m)
        MDX_REQUIRE(e[m] < e[m + 1], "%s must be strictly increasing: [%lld] = %g, [%lld] = %g", name, (long long)m,
                    e[m], (long long)(m + 1), e[m + 1]);
    return MDX_OK;
}

extern "C" {

int mdx_sdf_create(mdx_sdf_t *out, int dev, int64_t n_rows, int64_t n_ref, const int32_t *o_row, const int32_t *a_row,
                   const int32_t *b_row, int n_groups, const int64_t *group_start, const int32_t *p_row,
                   const int32_t *owner, int mode, double cutoff, const double *dims)
{
    MDX_REQUIRE(out && o_row && a_row && b_row && group_start && p_row && owner && dims, "NULL argument");
    MDX_REQUIRE(n_groups >= 1 && n_groups <= SDF_MAX_GROUPS, "n_groups must lie in [1, %d]", SDF_MAX_GROUPS);
    MDX_REQUIRE(mode == SDF_AXIS || mode == SDF_BISECTOR, "mode must be 0 (axis) or 1 (bisector)");
    MDX_REQUIRE(n_ref >= 1, "n_ref: there must be at least one reference molecule");
    MDX_REQUIRE(group_start[0] == 0, "group_start[0] must be 0");
    for (int g = 0; g < n_groups; ++g)
        MDX_REQUIRE(group_start[g] <= group_start[g + 1], "group_start must not decrease: [%d] = %lld, [%d] = %lld", g,
                    (long long)group_start[g], g + 1, (long long)group_start[g + 1]);
    const int64_t n_p = group_start[n_groups];
    MDX_REQUIRE(n_p >= 1, "group_start: there must be at least one partner");
    const int64_t limit = (int64_t(1) << 31) / 3;
    MDX_REQUIRE(n_rows >= 1 && n_rows < limit && n_ref < limit && n_p < limit,
                "n_rows and the tables must hold fewer than 2^31 / 3 rows");
    MDX_REQUIRE(ceil_div(n_ref, SDF_TILE) * ceil_div(n_p, SDF_JCHUNK) < (int64_t(1) << 31),
                "%lld molecules and %lld partners are too many pairs for one launch", (long long)n_ref,
                (long long)n_p);
    std::vector<char> seen((size_t)n_rows, 0);
    for (int64_t i = 0; i < n_ref; ++i) {
        MDX_REQUIRE(o_row[i] >= 0 && o_row[i] < n_rows, "o_row[%lld] = %d out of range [0, %lld)", (long long)i,
                    o_row[i], (long long)n_rows);
        MDX_REQUIRE(a_row[i] >= 0 && a_row[i] < n_rows, "a_row[%lld] = %d out of range [0, %lld)", (long long)i,
                    a_row[i], (long long)n_rows);
        MDX_REQUIRE(b_row[i] >= 0 && b_row[i] < n_rows, "b_row[%lld] = %d out of range [0, %lld)", (long long)i,
                    b_row[i], (long long)n_rows);
        MDX_REQUIRE(a_row[i] != o_row[i], "a_row[%lld] = %d is the molecule's origin", (long long)i, a_row[i]);
        MDX_REQUIRE(b_row[i] != o_row[i], "b_row[%lld] = %d is the molecule's origin", (long long)i, b_row[i]);
        MDX_REQUIRE(b_row[i] != a_row[i], "b_row[%lld] = %d is the molecule's axis atom", (long long)i, b_row[i]);
        MDX_REQUIRE(!seen[o_row[i]], "o_row holds row %d twice", o_row[i]);
        seen[o_row[i]] = 1;
    }
    std::fill(seen.begin(), seen.end(), 0);
    int64_t excluded = 0;               // owner[j] names one molecule: one excluded pair per owned partner
    for (int64_t j = 0; j < n_p; ++j) {
        MDX_REQUIRE(p_row[j] >= 0 && p_row[j] < n_rows, "p_row[%lld] = %d out of range [0, %lld)", (long long)j,
                    p_row[j], (long long)n_rows);
        MDX_REQUIRE(!seen[p_row[j]], "p_row holds row %d twice", p_row[j]);
        seen[p_row[j]] = 1;
        MDX_REQUIRE(owner[j] >= -1 && owner[j] < n_ref, "owner[%lld] = %d out of range [-1, %lld)", (long long)j,
                    owner[j], (long long)n_ref);
        excluded += owner[j] >= 0;
    }
    MDX_REQUIRE(cutoff > 0.0 && std::isfinite(cutoff), "cutoff must be positive and finite");
    PairBox box;
    int keep = 7;
    MDX_TRY(check_box_cutoff(dims, 0, cutoff, &box, &keep));
    mdx_sdf *h = new mdx_sdf();
    h->dev = dev;
    h->n_rows = n_rows;
    h->n_ref = n_ref;
    h->n_p = n_p;
    h->n_groups = n_groups;
    h->mode = mode;
    h->excluded = excluded;
    h->box = box;
    h->rc2 = cutoff * cutoff;
    for (int g = 0; g < SDF_MAX_GROUPS; ++g)
        h->groups.start[g] = g < n_groups ? (int)group_start[g] : INT_MAX;
    // until mdx_sdf_set_bins: one bin per axis, the cube around the cutoff's sphere
    for (int c = 0; c < 3; ++c) {
        h->axes.n[c] = 1;
        h->axes.lo[c] = -cutoff;
        h->axes.hi[c] = cutoff;
        h->axes.scale[c] = 1.0 / (2.0 * cutoff);
        h->edges.push_back(-cutoff);
        h->edges.push_back(cutoff);
    }
    h->tables.assign(o_row, o_row + n_ref);
    h->tables.insert(h->tables.end(), a_row, a_row + n_ref);
    h->tables.insert(h->tables.end(), b_row, b_row + n_ref);
    h->tables.insert(h->tables.end(), p_row, p_row + n_p);
    h->tables.insert(h->tables.end(), owner, owner + n_p);
    *out = h;
    return MDX_OK;
}

int mdx_sdf_set_bins(mdx_sdf_t h, int64_t nx, const double *ex, int64_t ny, const double *ey, int64_t nz,
                     const double *ez)
{
    MDX_REQUIRE(h && ex && ey && ez, "NULL argument");
    MDX_REQUIRE(h->frames_seen == 0, "mdx_sdf_set_bins must be called before the first frame");
    MDX_TRY(sdf_check_edges("ex", nx, ex));
    MDX_TRY(sdf_check_edges("ey", ny, ey));
    MDX_TRY(sdf_check_edges("ez", nz, ez));
    MDX_REQUIRE(h->n_groups * nx * ny * nz <= SDF_MAX_COUNTERS,
                "%d groups of nx * ny * nz = %lld x %lld x %lld bins are more than 2^26 counters", h->n_groups,
                (long long)nx, (long long)ny, (long long)nz);
    h->axes.n[0] = (int)nx;
    h->axes.n[1] = (int)ny;
    h->axes.n[2] = (int)nz;
    const double *axis_edges[3] = {ex, ey, ez};
    for (int c = 0; c < 3; ++c) {
        h->axes.lo[c] = axis_edges[c][0];
        h->axes.hi[c] = axis_edges[c][h->axes.n[c]];
        h->axes.scale[c] = h->axes.n[c] / (h->axes.hi[c] - h->axes.lo[c]);
    }
    h->edges.assign(ex, ex + nx + 1);
    h->edges.insert(h->edges.end(), ey, ey + ny + 1);
    h->edges.insert(h->edges.end(), ez, ez + nz + 1);
    if (!h->ready)
        return MDX_OK;
    // a handle that has touched its device without a frame (a result, a reset): the counters take their new sizes
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(sdf_upload_bins(h));
    MDX_TRY(sdf_zero(h));
    MDX_HIP(hipStreamSynchronize(h->stream));
    return MDX_OK;
}

int mdx_sdf_result(mdx_sdf_t h, int64_t *counts)
{
    MDX_REQUIRE(h && counts, "NULL argument");
    MDX_TRY(sdf_ensure_device(h));
    MDX_TRY(h->collect());
    // uint64 counts of fewer than 2^63 pairs each: they fit an int64
    MDX_HIP(hipMemcpy(counts, h->d_counts.ptr, size_t(8) * h->cells(), hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_sdf_inside(mdx_sdf_t h, int64_t *out, int64_t n)
{
    MDX_REQUIRE(h && (out || n == 0), "NULL argument");
    MDX_REQUIRE(n >= 0 && n <= h->frames_seen, "%lld frames asked for, %lld seen", (long long)n,
                (long long)h->frames_seen);
    if (n == 0)
        return MDX_OK;
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_HIP(hipMemcpy(out, h->d_inside.ptr, size_t(8) * n, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_sdf_stats(mdx_sdf_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *degenerate)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    uint64_t seen = 0;
    if (h->ready && degenerate)
        MDX_HIP(hipMemcpy(&seen, h->d_counts.as<uint64_t>() + h->cells(), 8, hipMemcpyDeviceToHost));
    if (evaluations) *evaluations = h->frames_seen * (h->n_ref * h->n_p - h->excluded);
    if (degenerate) *degenerate = int64_t(seen);
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(sdf, sdf_prepare, sdf_accumulate_rows)
MDX_LAZY_FRAME_LIFE_CYCLE(sdf, sdf_zero, unchecked)
MDX_FRAME_SET_SLAB_FRAMES(sdf, SDF_SLAB_MAX)
MDX_FRAME_PLAN(sdf, sdf_slab)
