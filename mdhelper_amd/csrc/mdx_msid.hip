// mdx_msid.hip — chain internal distances and bond-orientation correlations on gfx950 (MI355X).
//
// Carries the frame work of analysis.polymer.InternalDistances: positions (atoms, or the float64 centres of mass of
// monomers) -> optional global unwrap (topology.py `unwrap`) or per-frame `whole` -> per group the mean-square
// distance R2(s) between monomers s bonds apart and the correlation C(s) of unit bond vectors s bonds apart.
// Contract, summation order and work layout: mdx_msid_device.hpp; this unit is compiled with contraction off and
// spells its float64 operations out.
//
// O(N^2) pair terms per chain out of LDS, against the 12 B per atom-frame the points cost once.  The unit kernel
// leaves per-unit sums in a slab scratch; a second, small kernel adds the units of each group in order, divides and
// writes rows[frame][2 sum_g (N_g - 1)] in HBM.  Nothing is added with atomics, so the rows repeat bit for bit
// whatever route the frames take and however they are split into calls or slabs.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_molecules.hpp"
#include "mdx_msid_device.hpp"
#include "mdx_points_device.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_msid_dev;
using mdx_prof_dev::prof_com_f64_kernel;
using mdx_prof_dev::prof_unwrap_scan_kernel;

namespace {

constexpr int64_t MSID_SLAB_FRAMES = 32768;                // frames per launch (grid y)
constexpr int64_t MSID_SCRATCH_BYTES = int64_t(256) << 20; // partial sums / centres or whole points / image counts

// frames per slab of msid_accumulate_rows: what its scratch of one frame allows; also what mdx_msid_slab_frames
// reports
int64_t msid_slab_frames(int64_t n_partial, int64_t n_points, bool grouped, bool whole, bool unwrap)
{
    const int64_t scratch = 8 * n_partial + (grouped || whole ? 24 * n_points : 0) + (unwrap ? 12 * n_points : 0);
    return std::min(MSID_SLAB_FRAMES, std::max<int64_t>(1, MSID_SCRATCH_BYTES / scratch));
}

// the checks of mdx_msid_create on the chain layout; *n_points: the points of all groups, *n_partial: the partial
// sums the units of a frame leave (2 (N - 1) per unit of msid_chains_per_unit(N) chains)
int msid_layout(int n_groups, const int64_t *n_chains, const int64_t *n_monomers, int64_t *n_points,
                int64_t *n_partial)
{
    MDX_REQUIRE(n_groups >= 1 && n_groups <= 4096, "n_groups out of range");
    const int64_t limit = (int64_t(1) << 31) / 3;
    *n_points = *n_partial = 0;
    for (int g = 0; g < n_groups; ++g) {
        MDX_REQUIRE(n_chains[g] >= 1 && n_chains[g] < limit, "group %d: n_chains must be at least 1", g);
        MDX_REQUIRE(n_monomers[g] >= 2 && n_monomers[g] < limit, "group %d: n_monomers must be at least 2", g);
        MDX_REQUIRE(n_chains[g] * n_monomers[g] < limit - *n_points,
                    "the groups must hold fewer than 2^31 / 3 points");
        *n_points += n_chains[g] * n_monomers[g];
        *n_partial += ceil_div(n_chains[g], msid_chains_per_unit(n_monomers[g])) * 2 * (n_monomers[g] - 1);
    }
    return MDX_OK;
}

}  // namespace

struct mdx_msid : FrameEngine {
    int n_groups = 0;
    int64_t n_points = 0, n_units = 0, n_rows = 0, n_partial = 0;
    int64_t row_capacity = 0;
    bool unwrap = false, whole = false;
    double dims[3] = {0, 0, 0};
    std::vector<double> start;         // [n_points][3]: x_prev before the first frame
    std::vector<MsidGroup> groups;     // (the chains of group g start at point sum_{h<g} M_h N_h)
    DeviceBuffer d_units, d_groups, d_rows, d_partials, d_points, d_images, d_prev, d_image;
    MoleculeStage mol;                 // offsets / masses of the grouping; the centres are formed in float64 here

    int64_t rows_wanted() const { return mol.rows_wanted(n_points); }
    const char *rows_noun() const { return mol.rows_noun(); }
    void free_device()
    {
        release({&d_units, &d_groups, &d_rows, &d_partials, &d_points, &d_images, &d_prev, &d_image});
        mol.recycle();
    }
};

static int msid_grow_rows(mdx_msid *h, int64_t more, bool exact = false)
{
    return grow_rows(h->d_rows, h->stream, int64_t(8) * h->n_rows, h->frames_seen, more, &h->row_capacity, exact);
}

template <typename SRC>
static void msid_launch(mdx_msid *h, const SRC *pos, int64_t src_rows, const int *index, int64_t nf,
                        const int *images)
{
    hipLaunchKernelGGL((msid_unit_kernel<SRC>), dim3((unsigned)h->n_units, (unsigned)nf), dim3(MSID_THREADS), 0,
                       h->stream, pos, src_rows, index, (int)h->n_points, h->d_units.as<MsidUnit>(), images,
                       h->dims[0], h->dims[1], h->dims[2], h->n_partial, h->d_partials.as<double>());
    hipLaunchKernelGGL(msid_rows_kernel, dim3((unsigned)h->n_groups, (unsigned)nf), dim3(MSID_THREADS), 0, h->stream,
                       h->d_partials.as<double>(), h->n_partial, h->d_groups.as<MsidGroup>(), h->n_rows,
                       h->d_rows.as<double>() + h->frames_seen * h->n_rows);
}

// every chain of nf frames made whole: pos -> out (double [nf][n_points][3]; may be pos itself)
template <typename SRC>
static void msid_make_whole(mdx_msid *h, const SRC *pos, int64_t src_rows, const int *index, int64_t nf, double *out)
{
    int64_t point = 0;
    for (const MsidGroup &g : h->groups) {
        hipLaunchKernelGGL((msid_whole_kernel<SRC>), dim3((unsigned)ceil_div(3 * g.n_chains, 256), (unsigned)nf),
                           dim3(256), 0, h->stream, pos, src_rows, index, (int)h->n_points, (int)point,
                           (int)g.n_chains, g.n_monomers, h->dims[0], h->dims[1], h->dims[2], out);
        point += g.n_chains * g.n_monomers;
    }
}

// image counts of nf frames of points (state carried in d_prev / d_image from call to call)
template <typename SRC>
static int msid_scan(mdx_msid *h, const SRC *pos, int64_t src_rows, const int *index, int64_t nf)
{
    const int n = (int)h->n_points;
    MDX_TRY(h->d_images.ensure(size_t(12) * n * nf));
    hipLaunchKernelGGL((prof_unwrap_scan_kernel<SRC>), dim3((unsigned)ceil_div(3 * int64_t(n), 256)), dim3(256), 0,
                       h->stream, pos, src_rows, index, n, (int)nf, h->dims[0] / 2, h->dims[1] / 2, h->dims[2] / 2, 0,
                       h->d_prev.as<double>(), h->d_image.as<int>(), h->d_images.as<int>());
    return MDX_OK;
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int msid_accumulate_rows(mdx_msid *h, const float *d_pos, int64_t src_rows, const int *d_index,
                                int64_t n_rows, int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    const bool grouped = h->mol.active();
    const int64_t want = grouped ? h->mol.n_atoms : h->n_points;
    MDX_REQUIRE(n_rows == want, "%lld rows given, the groups%s hold %lld", (long long)n_rows,
                grouped ? " (rows of the grouping)" : "", (long long)want);
    MDX_TRY(msid_grow_rows(h, n_frames));
    const int64_t n = h->n_points;
    if (h->unwrap && h->frames_seen == 0) {
        // before the first frame x_prev is the starting configuration and the image counts are 0
        MDX_HIP(hipMemcpyAsync(h->d_prev.ptr, h->start.data(), size_t(24) * n, hipMemcpyHostToDevice, h->stream));
        MDX_HIP(hipMemsetAsync(h->d_image.ptr, 0, size_t(12) * n, h->stream));
    }
    const int64_t slab = msid_slab_frames(h->n_partial, n, grouped, h->whole, h->unwrap);
    hipEvent_t ev = h->timer.begin();
    for (int64_t f0 = 0; f0 < n_frames; f0 += slab) {
        const int64_t nf = std::min(slab, n_frames - f0);
        const float *pos = d_pos + f0 * src_rows * 3;
        MDX_TRY(h->d_partials.ensure(size_t(8) * h->n_partial * nf));
        const int *images = nullptr;
        if (grouped || h->whole)
            MDX_TRY(h->d_points.ensure(size_t(24) * n * nf));
        double *points = h->d_points.as<double>();
        if (grouped) {
            hipLaunchKernelGGL(prof_com_f64_kernel, dim3((unsigned)ceil_div(3 * n, 256), (unsigned)nf), dim3(256), 0,
                               h->stream, pos, src_rows, d_index, h->mol.d_offsets.as<int64_t>(),
                               h->mol.d_masses.as<double>(), h->mol.d_total.as<double>(), n, points);
            if (h->unwrap) {
                MDX_TRY(msid_scan(h, (const double *)points, n, nullptr, nf));
                images = h->d_images.as<int>();
            }
            if (h->whole)
                msid_make_whole(h, (const double *)points, n, nullptr, nf, points);
            msid_launch(h, (const double *)points, n, nullptr, nf, images);
        } else if (h->whole) {
            msid_make_whole(h, pos, src_rows, d_index, nf, points);
            msid_launch(h, (const double *)points, n, nullptr, nf, nullptr);
        } else {
            if (h->unwrap) {
                MDX_TRY(msid_scan(h, pos, src_rows, d_index, nf));
                images = h->d_images.as<int>();
            }
            msid_launch(h, pos, src_rows, d_index, nf, images);
        }
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

extern "C" {

int mdx_msid_create(mdx_msid_t *out, int dev, int n_groups, const int64_t *n_chains, const int64_t *n_monomers)
{
    MDX_REQUIRE(out && n_chains && n_monomers, "NULL argument");
    int64_t n_points = 0, n_partial = 0;
    MDX_TRY(msid_layout(n_groups, n_chains, n_monomers, &n_points, &n_partial));
    // the units of the kernel and the groups' ranges of partial sums and rows
    std::vector<MsidUnit> units;
    std::vector<MsidGroup> groups;
    int64_t point = 0, partial = 0, row = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int64_t M = n_chains[g], N = n_monomers[g];
        const int64_t per_unit = msid_chains_per_unit(N);
        groups.push_back(MsidGroup{partial, row, int(ceil_div(M, per_unit)), int(N), M});
        for (int64_t c = 0; c < M; c += per_unit) {
            units.push_back(MsidUnit{int(point + c * N), int(std::min(per_unit, M - c)), int(N), 0, partial});
            partial += 2 * (N - 1);
        }
        point += M * N;
        row += 2 * (N - 1);
    }
    MDX_TRY(set_device(dev));
    mdx_msid *h = new mdx_msid();
    h->dev = dev;
    h->n_groups = n_groups;
    h->n_points = n_points;
    h->n_units = (int64_t)units.size();
    h->n_rows = row;
    h->n_partial = n_partial;       // == partial: the end of the last unit's range
    h->groups = groups;
    int rc = MDX_OK;
    do {
        if ((rc = stream_acquire(&h->stream)) != MDX_OK) break;
        h->timer.stream = h->stream;
        if ((rc = h->d_units.ensure(sizeof(MsidUnit) * units.size())) != MDX_OK) break;
        if ((rc = h->d_groups.ensure(sizeof(MsidGroup) * groups.size())) != MDX_OK) break;
        if (hipMemcpy(h->d_units.ptr, units.data(), sizeof(MsidUnit) * units.size(), hipMemcpyHostToDevice) !=
                hipSuccess ||
            hipMemcpy(h->d_groups.ptr, groups.data(), sizeof(MsidGroup) * groups.size(), hipMemcpyHostToDevice) !=
                hipSuccess) {
            rc = fail(MDX_ERR_HIP, "upload failed");
            break;
        }
    } while (0);
    if (rc != MDX_OK) {
        mdx_msid_destroy(h);
        return rc;
    }
    *out = h;
    return MDX_OK;
}

int mdx_msid_slab_frames(int n_groups, const int64_t *n_chains, const int64_t *n_monomers, int grouped, int whole,
                         int unwrap, int64_t *slab)
{
    MDX_REQUIRE(n_chains && n_monomers && slab, "NULL argument");
    MDX_REQUIRE(!(whole && unwrap), "whole cannot be combined with unwrap");
    int64_t n_points = 0, n_partial = 0;
    MDX_TRY(msid_layout(n_groups, n_chains, n_monomers, &n_points, &n_partial));
    *slab = msid_slab_frames(n_partial, n_points, grouped != 0, whole != 0, unwrap != 0);
    return MDX_OK;
}

int mdx_msid_reserve(mdx_msid_t h, int64_t n_frames)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_REQUIRE(n_frames >= 0, "bad size");
    MDX_TRY(set_device(h->dev));
    return msid_grow_rows(h, n_frames - h->frames_seen, true);
}

int mdx_msid_set_grouping(mdx_msid_t h, int64_t n_molecules, const int64_t *offsets, const double *masses)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_REQUIRE(h->frames_seen == 0, "mdx_msid_set_grouping must be called before the first frame");
    MDX_REQUIRE(n_molecules <= 0 || n_molecules == h->n_points, "%lld molecules given, the groups hold %lld points",
                (long long)n_molecules, (long long)h->n_points);
    MDX_REQUIRE(n_molecules <= 0 || (offsets && offsets[n_molecules] < (int64_t(1) << 31) / 3),
                "the grouping holds too many rows");
    return h->mol.set(n_molecules, offsets, masses);
}

int mdx_msid_set_unwrap(mdx_msid_t h, const double *dims, const double *start)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_REQUIRE(h->frames_seen == 0, "mdx_msid_set_unwrap must be called before the first frame");
    if (!dims) {
        h->unwrap = false;
        return MDX_OK;
    }
    MDX_REQUIRE(!h->whole, "mdx_msid_set_unwrap cannot be combined with mdx_msid_set_whole");
    MDX_REQUIRE(start, "NULL argument");
    for (int k = 0; k < 3; ++k)
        MDX_REQUIRE(dims[k] > 0.0 && std::isfinite(dims[k]), "dims[%d] must be positive and finite", k);
    MDX_TRY(set_device(h->dev));
    MDX_TRY(h->d_prev.ensure(size_t(24) * h->n_points));
    MDX_TRY(h->d_image.ensure(size_t(12) * h->n_points));
    h->start.assign(start, start + 3 * h->n_points);
    for (int k = 0; k < 3; ++k)
        h->dims[k] = dims[k];
    h->unwrap = true;
    return MDX_OK;
}

int mdx_msid_set_whole(mdx_msid_t h, const double *dims)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_REQUIRE(h->frames_seen == 0, "mdx_msid_set_whole must be called before the first frame");
    if (!dims) {
        h->whole = false;
        return MDX_OK;
    }
    MDX_REQUIRE(!h->unwrap, "mdx_msid_set_whole cannot be combined with mdx_msid_set_unwrap");
    for (int k = 0; k < 3; ++k)
        MDX_REQUIRE(dims[k] > 0.0 && std::isfinite(dims[k]), "dims[%d] must be positive and finite", k);
    for (int k = 0; k < 3; ++k)
        h->dims[k] = dims[k];
    h->whole = true;
    return MDX_OK;
}

// what a route prepares before the first kernel
static int msid_prepare(mdx_msid *h, int64_t n_frames)
{
    MDX_TRY(set_device(h->dev));
    return msid_grow_rows(h, n_frames);
}

int mdx_msid_result(mdx_msid_t h, double *out)
{
    MDX_REQUIRE(h && out, "NULL argument");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    h->timer.collect();
    if (h->frames_seen == 0)
        return MDX_OK;
    MDX_HIP(hipMemcpy(out, h->d_rows.ptr, size_t(8) * h->n_rows * h->frames_seen, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_msid_stats(mdx_msid_t h, int64_t *launches, double *kernel_ms, int64_t *frames)
{
    MDX_REQUIRE(h, "NULL handle");
    return h->stats(true, launches, kernel_ms, frames);
}

}  // extern "C"

MDX_FRAME_ROUTES(msid, msid_prepare, msid_accumulate_rows)
MDX_FRAME_LIFE_CYCLE(msid)
MDX_FRAME_RESET(msid)
