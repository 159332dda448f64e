// mdx_profile.hip — per-axis density histograms on gfx950 (MI355X).
//
// Carries DensityProfile._single_frame (reference src/mdhelper/analysis/profile.py:775-818): positions of
// every group (atoms, or float64 centres of mass of residues / segments) -> optional recentring on a group's
// centre of mass (global unwrap, topology.py `unwrap`) -> `wrap` -> numpy.histogram along the requested axes.
// The counts are integers and equal numpy's count for count (contract: mdx_profile_device.hpp); this unit is
// compiled with contraction off and spells its float64 operations out.
//
// One pass over the positions at 12 B per atom-frame.  Counters for every (axis, group, bin) slot sit in LDS as
// uint32, in up to 8 interleaved replicas; a block keeps them over a run of frames and flushes once with integer
// atomics (uint64 totals when averaging, a uint32 row per frame otherwise), so results repeat bit for bit.  When
// the slots do not fit, the replica count steps down and finally the kernels bin straight into global memory.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_molecules.hpp"
#include "mdx_profile_device.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_prof_dev;

namespace {

constexpr size_t PROF_LDS_REPLICATED = size_t(32) << 10;   // replicas only while the block stays at <= 32 KB ...
constexpr size_t PROF_LDS_LIMIT = size_t(60) << 10;        // ... one copy up to here, beyond it global atomics
constexpr int64_t PROF_SLAB_FRAMES = 32768;                // frames per launch (grid y)
constexpr int64_t PROF_SCRATCH_BYTES = int64_t(256) << 20; // centres / image counts of one slab

// frames per slab of prof_accumulate_rows: what its scratch of one frame allows (plain atoms need none); also what
// mdx_prof_slab_frames reports
int64_t prof_slab_frames(int64_t n_points, bool grouped, bool recenter)
{
    const int64_t scratch = (grouped ? 24 * n_points : 0) + (recenter ? 12 * n_points + 24 : 0);
    return scratch ? std::min(PROF_SLAB_FRAMES, std::max<int64_t>(1, PROF_SCRATCH_BYTES / scratch))
                   : PROF_SLAB_FRAMES;
}

}  // namespace

struct mdx_prof : FrameEngine {
    int n_groups = 0, n_axes = 0;
    bool per_frame = false;
    int64_t n_points = 0;
    int axes[3] = {0, 0, 0};
    int64_t n_bins[3] = {0, 0, 0};     // per axis slot
    double dims[3] = {0, 0, 0};
    ProfPlan plan{};
    bool use_lds = true;
    size_t lds_bytes = 0;
    int64_t row_capacity = 0;
    DeviceBuffer d_offsets, d_total, d_rows, d_centres, d_images, d_shift, d_prev, d_image, d_rmass;
    MoleculeStage mol;                 // offsets / masses of the grouping; the centres are formed in float64 here
    // recentring
    int rc_group = -1;
    int64_t rc_lo = 0, rc_hi = 0;
    double rc_mass = 0.0, rc_target[3] = {0, 0, 0};

    int64_t rows_wanted() const { return mol.rows_wanted(n_points); }
    const char *rows_noun() const { return mol.rows_noun(); }
    void free_device()
    {
        release({&d_offsets, &d_total, &d_rows, &d_centres, &d_images, &d_shift, &d_prev, &d_image, &d_rmass});
        mol.recycle();
    }
};

// most LDS copies that fit, at most `limit` of them (limit < 0: no limit, 0: global atomics); -1: global atomics
static int prof_replica_shift(int64_t n_slots, int n_groups, int limit)
{
    const size_t table = size_t(4) * (n_groups + 1);
    const int forced = limit;
    if (forced == 0)
        return -1;
    for (int shift = 3; shift >= 1; --shift)
        if ((forced < 0 || forced >= (1 << shift)) && (size_t(n_slots) << shift) * 4 + table <= PROF_LDS_REPLICATED)
            return shift;
    return size_t(n_slots) * 4 + table <= PROF_LDS_LIMIT ? 0 : -1;
}

static void prof_plan_counters(mdx_prof *h, int limit)
{
    ProfPlan &plan = h->plan;
    const int shift = prof_replica_shift(plan.n_slots, h->n_groups, limit);
    h->use_lds = shift >= 0;
    plan.rep_shift = shift < 0 ? 0 : shift;
    h->lds_bytes = (h->use_lds ? (size_t(plan.n_slots) << plan.rep_shift) * 4 : 0) + size_t(4) * (h->n_groups + 1);
}

// per-frame rows: capacity for `more` frames behind the ones seen
static int prof_grow_rows(mdx_prof *h, int64_t more)
{
    if (!h->per_frame)
        return MDX_OK;
    return grow_rows(h->d_rows, h->stream, int64_t(4) * h->plan.n_slots, h->frames_seen, more, &h->row_capacity);
}

// ... and the rows of the next `more` frames zeroed
static int prof_reserve_rows(mdx_prof *h, int64_t more)
{
    if (!h->per_frame || more <= 0)
        return MDX_OK;
    MDX_TRY(prof_grow_rows(h, more));
    const int64_t S = h->plan.n_slots;
    MDX_HIP(hipMemsetAsync(h->d_rows.as<unsigned int>() + S * h->frames_seen, 0, size_t(4) * S * more, h->stream));
    return MDX_OK;
}

template <typename CT, bool USE_LDS>
static void prof_launch_flat(mdx_prof *h, const float *pos, int64_t nf, int fpb, CT *out, int64_t stride)
{
    const int n_elems = int(3 * h->n_points);
    const unsigned bx = (unsigned)std::max<int64_t>(1, ceil_div(n_elems / 4, PROF_VEC_PER_BLOCK));
    hipLaunchKernelGGL((prof_hist_flat_kernel<CT, USE_LDS>), dim3(bx, (unsigned)ceil_div(nf, fpb)),
                       dim3(PROF_THREADS), h->lds_bytes, h->stream, pos, n_elems, (int)nf, fpb, h->plan,
                       h->d_offsets.as<int>(), out, stride);
}

template <typename SRC, typename CT, bool USE_LDS>
static void prof_launch_points(mdx_prof *h, const SRC *pos, int64_t src_rows, const int *index, int64_t nf, int fpb,
                               const int *images, const double *shift, CT *out, int64_t stride)
{
    const unsigned bx = (unsigned)ceil_div(h->n_points, PROF_POINTS_PER_BLOCK);
    hipLaunchKernelGGL((prof_hist_points_kernel<SRC, CT, USE_LDS>), dim3(bx, (unsigned)ceil_div(nf, fpb)),
                       dim3(PROF_THREADS), h->lds_bytes, h->stream, pos, src_rows, index, (int)h->n_points, (int)nf,
                       fpb, h->plan, h->d_offsets.as<int>(), images, shift, out, stride);
}

// the histogram of nf frames: `flat` walks pos as float32[nf][n_points][3], else the general kernel over SRC rows
template <typename SRC>
static void prof_histogram(mdx_prof *h, bool flat, const SRC *pos, int64_t src_rows, const int *index, int64_t nf,
                           const int *images, const double *shift)
{
    const int64_t S = h->plan.n_slots;
    // averaging: a block keeps its LDS counters over a run of frames, as long as ~4096 blocks remain for the chip
    const int64_t bx = flat ? std::max<int64_t>(1, ceil_div(3 * h->n_points / 4, PROF_VEC_PER_BLOCK))
                            : ceil_div(h->n_points, PROF_POINTS_PER_BLOCK);
    const int fpb = h->per_frame ? 1 : (int)std::min<int64_t>(64, std::max<int64_t>(1, nf * bx / 4096));
    const float *fpos = reinterpret_cast<const float *>(pos);
    if (h->per_frame) {
        unsigned int *out = h->d_rows.as<unsigned int>() + S * h->frames_seen;
        if (flat && h->use_lds) prof_launch_flat<unsigned int, true>(h, fpos, nf, fpb, out, S);
        else if (flat) prof_launch_flat<unsigned int, false>(h, fpos, nf, fpb, out, S);
        else if (h->use_lds) prof_launch_points<SRC, unsigned int, true>(h, pos, src_rows, index, nf, fpb, images, shift, out, S);
        else prof_launch_points<SRC, unsigned int, false>(h, pos, src_rows, index, nf, fpb, images, shift, out, S);
    } else {
        unsigned long long *out = h->d_total.as<unsigned long long>();
        if (flat && h->use_lds) prof_launch_flat<unsigned long long, true>(h, fpos, nf, fpb, out, 0);
        else if (flat) prof_launch_flat<unsigned long long, false>(h, fpos, nf, fpb, out, 0);
        else if (h->use_lds) prof_launch_points<SRC, unsigned long long, true>(h, pos, src_rows, index, nf, fpb, images, shift, out, 0);
        else prof_launch_points<SRC, unsigned long long, false>(h, pos, src_rows, index, nf, fpb, images, shift, out, 0);
    }
}

// recentring of nf frames of points: image counts (state carried in d_prev / d_image), then the per-frame shift
template <typename SRC>
static int prof_recenter(mdx_prof *h, const SRC *pos, int64_t src_rows, const int *index, int64_t nf)
{
    const int n = (int)h->n_points;
    MDX_TRY(h->d_images.ensure(size_t(12) * n * nf));
    MDX_TRY(h->d_shift.ensure(size_t(24) * nf));
    hipLaunchKernelGGL((prof_unwrap_scan_kernel<SRC>), dim3((unsigned)ceil_div(3 * int64_t(n), 256)), dim3(256), 0,
                       h->stream, pos, src_rows, index, n, (int)nf, h->dims[0] / 2, h->dims[1] / 2, h->dims[2] / 2,
                       h->frames_seen == 0 ? 1 : 0, h->d_prev.as<double>(), h->d_image.as<int>(),
                       h->d_images.as<int>());
    hipLaunchKernelGGL((prof_recenter_shift_kernel<SRC>), dim3((unsigned)nf), dim3(256), 0, h->stream, pos, src_rows,
                       index, n, (int)h->rc_lo, (int)h->rc_hi, h->d_rmass.as<double>(), h->rc_mass,
                       h->d_images.as<int>(), h->dims[0], h->dims[1], h->dims[2], h->rc_target[0], h->rc_target[1],
                       h->rc_target[2], h->d_shift.as<double>());
    return MDX_OK;
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int prof_accumulate_rows(mdx_prof *h, const float *d_pos, int64_t src_rows, const int *d_index,
                                int64_t n_rows, int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    const bool grouped = h->mol.active(), recenter = h->rc_group >= 0;
    const int64_t want = grouped ? h->mol.n_atoms : h->n_points;
    MDX_REQUIRE(n_rows == want, "%lld rows given, the groups%s hold %lld", (long long)n_rows,
                grouped ? " (rows of the grouping)" : "", (long long)want);
    MDX_TRY(prof_reserve_rows(h, n_frames));
    const int64_t n = h->n_points;
    const int64_t slab = prof_slab_frames(n, grouped, recenter);
    hipEvent_t ev = h->timer.begin();
    for (int64_t f0 = 0; f0 < n_frames; f0 += slab) {
        const int64_t nf = std::min(slab, n_frames - f0);
        const float *pos = d_pos + f0 * src_rows * 3;
        const int *images = nullptr;
        const double *shift = nullptr;
        if (grouped) {
            MDX_TRY(h->d_centres.ensure(size_t(24) * n * nf));
            hipLaunchKernelGGL(prof_com_f64_kernel, dim3((unsigned)ceil_div(3 * n, 256), (unsigned)nf), dim3(256), 0,
                               h->stream, pos, src_rows, d_index, h->mol.d_offsets.as<int64_t>(),
                               h->mol.d_masses.as<double>(), h->mol.d_total.as<double>(), n,
                               h->d_centres.as<double>());
            const double *centres = h->d_centres.as<double>();
            if (recenter) {
                MDX_TRY(prof_recenter(h, centres, n, nullptr, nf));
                images = h->d_images.as<int>();
                shift = h->d_shift.as<double>();
            }
            prof_histogram(h, false, centres, n, nullptr, nf, images, shift);
        } else {
            if (recenter) {
                MDX_TRY(prof_recenter(h, pos, src_rows, d_index, nf));
                images = h->d_images.as<int>();
                shift = h->d_shift.as<double>();
            }
            prof_histogram(h, !recenter && !d_index && src_rows == n, pos, src_rows, d_index, nf, images, shift);
        }
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

extern "C" {

int mdx_prof_create(mdx_prof_t *out, int dev, int n_groups, const int64_t *group_offsets, int n_axes,
                    const int32_t *axes, const int64_t *n_bins, const double *dims, int per_frame)
{
    MDX_REQUIRE(out && group_offsets && axes && n_bins && dims, "NULL argument");
    MDX_REQUIRE(n_groups >= 1 && n_groups <= 4096, "n_groups out of range");
    MDX_REQUIRE(n_axes >= 1 && n_axes <= 3, "n_axes must be 1, 2 or 3");
    MDX_REQUIRE(group_offsets[0] == 0, "group offsets must start at 0");
    for (int g = 0; g < n_groups; ++g)
        MDX_REQUIRE(group_offsets[g + 1] >= group_offsets[g], "group offsets must not decrease");
    MDX_REQUIRE(group_offsets[n_groups] >= 1 && group_offsets[n_groups] < (int64_t(1) << 31) / 3,
                "the groups must hold between 1 and 2^31 / 3 points");
    int64_t bins_total = 0;
    for (int s = 0; s < n_axes; ++s) {
        MDX_REQUIRE(axes[s] >= 0 && axes[s] <= 2, "axis %d is not 0, 1 or 2", axes[s]);
        for (int t = 0; t < s; ++t)
            MDX_REQUIRE(axes[t] != axes[s], "axis %d is given twice", axes[s]);
        MDX_REQUIRE(n_bins[s] >= 1 && n_bins[s] < (int64_t(1) << 24), "n_bins of axis %d must be in [1, 2^24)",
                    axes[s]);
        bins_total += n_bins[s];
    }
    for (int k = 0; k < 3; ++k)
        MDX_REQUIRE(dims[k] > 0.0 && std::isfinite(dims[k]), "dims[%d] must be positive and finite", k);
    MDX_REQUIRE(bins_total * n_groups < (int64_t(1) << 28), "too many counters (groups x bins)");
    MDX_TRY(set_device(dev));
    mdx_prof *h = new mdx_prof();
    h->dev = dev;
    h->n_groups = n_groups;
    h->n_axes = n_axes;
    h->per_frame = per_frame != 0;
    h->n_points = group_offsets[n_groups];
    ProfPlan &plan = h->plan;
    for (int k = 0; k < 3; ++k) {
        h->dims[k] = dims[k];
        plan.ax[k] = ProfAxis{dims[k], 0.0, 0.0, 0, 0};
    }
    int base = 0;
    for (int s = 0; s < n_axes; ++s) {
        const int k = axes[s];
        h->axes[s] = k;
        h->n_bins[s] = n_bins[s];
        plan.ax[k].n_bins = (int)n_bins[s];
        plan.ax[k].width = dims[k] / double(n_bins[s]);       // numpy.linspace's step
        plan.ax[k].inv_width = double(n_bins[s]) / dims[k];   // numpy.histogram's norm
        plan.ax[k].base = base;
        base += n_groups * (int)n_bins[s];
    }
    plan.n_groups = n_groups;
    plan.n_slots = base;
    prof_plan_counters(h, -1);
    std::vector<int32_t> offs(group_offsets, group_offsets + n_groups + 1);
    int rc = MDX_OK;
    do {
        if ((rc = stream_acquire(&h->stream)) != MDX_OK) break;
        h->timer.stream = h->stream;
        if ((rc = h->d_offsets.ensure(size_t(4) * (n_groups + 1))) != MDX_OK) break;
        if ((rc = h->d_total.ensure(size_t(8) * base)) != MDX_OK) break;
        if (hipMemcpy(h->d_offsets.ptr, offs.data(), size_t(4) * (n_groups + 1), hipMemcpyHostToDevice) !=
            hipSuccess) {
            rc = fail(MDX_ERR_HIP, "upload failed");
            break;
        }
    } while (0);
    if (rc != MDX_OK) {
        mdx_prof_destroy(h);
        return rc;
    }
    *out = h;
    return mdx_prof_reset(h);
}

// the staging slab every per-frame engine's host and file route shares (FrameEngine::accumulate_host / _traj)
int mdx_feed_slab_frames(int64_t n_frames, int64_t rows, int64_t *slab)
{
    MDX_REQUIRE(slab, "NULL argument");
    MDX_REQUIRE(n_frames >= 1 && rows >= 1, "bad size");
    *slab = feed_slab_frames(n_frames, rows);
    return MDX_OK;
}

int mdx_prof_slab_frames(int64_t n_points, int grouped, int recenter, int64_t *slab)
{
    MDX_REQUIRE(slab, "NULL argument");
    MDX_REQUIRE(n_points >= 1 && n_points < (int64_t(1) << 31) / 3,
                "the groups must hold between 1 and 2^31 / 3 points");
    *slab = prof_slab_frames(n_points, grouped != 0, recenter != 0);
    return MDX_OK;
}

// its own rule: the totals start over too
int mdx_prof_reset(mdx_prof_t h)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipMemsetAsync(h->d_total.ptr, 0, size_t(8) * h->plan.n_slots, h->stream));
    return h->reset();      // the unwrap state starts over with the next frame
}

int mdx_prof_set_grouping(mdx_prof_t h, int64_t n_molecules, const int64_t *offsets, const double *masses)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_REQUIRE(h->frames_seen == 0, "mdx_prof_set_grouping must be called before the first frame");
    MDX_REQUIRE(n_molecules <= 0 || n_molecules == h->n_points, "%lld molecules given, the groups hold %lld points",
                (long long)n_molecules, (long long)h->n_points);
    MDX_REQUIRE(n_molecules <= 0 || (offsets && offsets[n_molecules] < (int64_t(1) << 31) / 3),
                "the grouping holds too many rows");
    return h->mol.set(n_molecules, offsets, masses);
}

int mdx_prof_set_recenter(mdx_prof_t h, int group, const double *masses, const double *target)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_REQUIRE(h->frames_seen == 0, "mdx_prof_set_recenter must be called before the first frame");
    if (group < 0) {
        h->rc_group = -1;
        return MDX_OK;
    }
    MDX_REQUIRE(group < h->n_groups, "group %d is not one of the %d groups", group, h->n_groups);
    MDX_REQUIRE(masses && target, "NULL argument");
    std::vector<int32_t> offs((size_t)h->n_groups + 1);
    MDX_HIP(hipMemcpy(offs.data(), h->d_offsets.ptr, size_t(4) * (h->n_groups + 1), hipMemcpyDeviceToHost));
    const int64_t lo = offs[(size_t)group], hi = offs[(size_t)group + 1];
    MDX_REQUIRE(hi > lo, "group %d is empty", group);
    double total = 0.0;
    for (int64_t i = 0; i < hi - lo; ++i)
        total += masses[i];
    MDX_REQUIRE(total > 0.0 && std::isfinite(total), "group %d has no mass", group);
    MDX_TRY(h->d_rmass.ensure(size_t(8) * (hi - lo)));
    MDX_TRY(h->d_prev.ensure(size_t(24) * h->n_points));
    MDX_TRY(h->d_image.ensure(size_t(12) * h->n_points));
    MDX_HIP(hipMemcpy(h->d_rmass.ptr, masses, size_t(8) * (hi - lo), hipMemcpyHostToDevice));
    h->rc_group = group;
    h->rc_lo = lo;
    h->rc_hi = hi;
    h->rc_mass = total;
    for (int k = 0; k < 3; ++k)
        h->rc_target[k] = target[k];
    return MDX_OK;
}

int mdx_prof_set_replicas(mdx_prof_t h, int replicas)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_REQUIRE(replicas == -1 || replicas == 0 || replicas == 1 || replicas == 2 || replicas == 4 || replicas == 8,
                "replicas must be 8, 4, 2, 1, 0 or -1");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_REQUIRE(h->frames_seen == 0, "mdx_prof_set_replicas must be called before the first frame");
    prof_plan_counters(h, replicas);
    return MDX_OK;
}

// what a route prepares before the first kernel
static int prof_prepare(mdx_prof *h, int64_t n_frames)
{
    MDX_TRY(set_device(h->dev));
    return prof_grow_rows(h, n_frames);
}

int mdx_prof_counts(mdx_prof_t h, int axis_slot, int64_t *out)
{
    MDX_REQUIRE(h && out, "NULL argument");
    MDX_REQUIRE(axis_slot >= 0 && axis_slot < h->n_axes, "axis slot %d out of range", axis_slot);
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    h->timer.collect();
    const ProfAxis &ax = h->plan.ax[h->axes[axis_slot]];
    const int64_t per_axis = int64_t(h->n_groups) * ax.n_bins, S = h->plan.n_slots;
    if (!h->per_frame) {
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "totals are copied as they are");
        MDX_HIP(hipMemcpy(out, h->d_total.as<unsigned long long>() + ax.base, size_t(8) * per_axis,
                          hipMemcpyDeviceToHost));
        return MDX_OK;
    }
    const int64_t F = h->frames_seen;
    if (F == 0)
        return MDX_OK;
    std::vector<unsigned int> rows(size_t(F) * per_axis);
    MDX_HIP(hipMemcpy2D(rows.data(), size_t(4) * per_axis, h->d_rows.as<unsigned int>() + ax.base, size_t(4) * S,
                        size_t(4) * per_axis, size_t(F), hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < h->n_groups; ++g)
        for (int64_t f = 0; f < F; ++f)
            for (int64_t b = 0; b < ax.n_bins; ++b)
                out[(g * F + f) * ax.n_bins + b] = rows[size_t(f * per_axis + g * ax.n_bins + b)];
    return MDX_OK;
}

int mdx_prof_stats(mdx_prof_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int *replicas)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(true, launches, kernel_ms, frames));
    if (replicas) *replicas = h->use_lds ? 1 << h->plan.rep_shift : 0;
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(prof, prof_prepare, prof_accumulate_rows)
MDX_FRAME_LIFE_CYCLE(prof)
