// mdx_chi4.hip — self-overlap and four-point susceptibility on gfx950 (MI355X).
//
// Per lag, group and cutoff the number Q of points that moved at most the cutoff between the frames of a pair
// (f0, f0 + lag), and over the time origins f0 the sums of Q and of Q*Q, from which the class forms Q_s(t) and
// chi_4(t).  Contract and kernel shape: mdx_chi4_device.hpp; this unit is compiled with contraction off and spells
// its float64 operations out.
//
// The widened (and unwrapped) points go into a ring of max(lags) + slab frames in HBM, written by the van Hove
// engine's vh_prepare_kernel, so that a lag reaches back across slabs and calls.  Q of the slab's frame pairs is
// counted into a uint32 scratch that is zeroed per slab and folded into the uint64 sums.  Everything added is an
// integer, so the sums repeat bit for bit whatever route the frames take and however they are split into calls, slabs
// or point segments.
//
// A handle touches its device with the first frame (or result): creating one, and every argument error, needs none.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_lag_history.hpp"
#include "mdx_chi4_device.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

// The van Hove engine's device header, for its vh_prepare_kernel.  The header also defines a kernel that is no
// template (vh_fold_kernel), which mdx_vanhove.hip already gives the library once: inside a namespace of this unit
// its second copy has a name of its own and the link sees no duplicate.  Everything the header includes itself is
// included above, so nothing but its own declarations lands in the namespace.
namespace mdx_chi4_ring {
#include "mdx_vanhove_device.hpp"
}

using namespace mdx;
using namespace mdx_chi4_dev;
using mdx_chi4_ring::mdx_vh_dev::vh_prepare_kernel;

namespace {

// what the frames of a default slab take in the ring and in the scratch: the van Hove engine's allowance for its slab
constexpr int64_t CHI4_SLAB_BYTES = int64_t(256) << 20;
constexpr int64_t CHI4_GRID_YZ = 65535;

}  // namespace

struct mdx_chi4 : LazyFrameEngine {
    int n_groups = 0, n_cutoffs = 0, keep = 7;
    int64_t n_points = 0, max_group = 0;
    int64_t n_entries = 0;              // lags * n_groups * n_cutoffs
    int64_t segment_points = 0;         // 0 = the default
    int64_t evaluations = 0;
    LagTable lags;
    LagRing ring;
    UnwrappedHistory hist;
    Chi4Cutoffs cut;
    std::vector<int64_t> offsets;
    DeviceBuffer d_offsets, d_s1, d_s2, d_qslab;

    int64_t rows_wanted() const { return n_points; }
    const char *rows_noun() const { return "groups"; }
    int64_t ring_lag() const { return lags.max_lag; }
    void clear_counters() { evaluations = 0; }
    void free_device()
    {
        release({&d_offsets, &lags.d_lags, &d_s1, &d_s2, &d_qslab, &hist.d_hist, &hist.d_prev, &hist.d_image});
    }
};

static int64_t chi4_slab(const mdx_chi4 *h)
{
    if (h->slab_frames > 0)
        return h->slab_frames;
    const int64_t per_frame = 24 * h->n_points + 4 * h->n_entries;
    return std::min(CHI4_SLAB_MAX, std::max<int64_t>(1, CHI4_SLAB_BYTES / per_frame));
}

// points per segment: the one asked for (or the default), raised until the segments fit grid z
static int64_t chi4_segment(const mdx_chi4 *h)
{
    const int64_t asked = h->segment_points > 0 ? h->segment_points : CHI4_SEGMENT;
    const int64_t least = ceil_div(ceil_div(h->n_points, CHI4_GRID_YZ), int64_t(CHI4_TILE)) * CHI4_TILE;
    return std::max(asked, least);
}

static int chi4_zero(mdx_chi4 *h)
{
    MDX_HIP(hipMemsetAsync(h->d_s1.ptr, 0, size_t(8) * h->n_entries, h->stream));
    MDX_HIP(hipMemsetAsync(h->d_s2.ptr, 0, size_t(8) * h->n_entries, h->stream));
    return MDX_OK;
}

// the device side of the handle: tables and sums
static int chi4_build(mdx_chi4 *h)
{
    MDX_TRY(h->d_offsets.ensure(size_t(8) * (h->n_groups + 1)));
    MDX_TRY(h->d_s1.ensure(size_t(8) * h->n_entries));
    MDX_TRY(h->d_s2.ensure(size_t(8) * h->n_entries));
    MDX_TRY(h->hist.ensure_state(h->n_points));
    MDX_HIP(hipMemcpy(h->d_offsets.ptr, h->offsets.data(), size_t(8) * (h->n_groups + 1), hipMemcpyHostToDevice));
    MDX_TRY(h->lags.upload());
    return chi4_zero(h);
}

static int chi4_ensure_device(mdx_chi4 *h) { return h->ensure_device(chi4_build); }

// What a route prepares before the first kernel: the device side, and before the first frame of a pass the ring and
// the scratch, one row of it per frame of a slab.
static int chi4_prepare(mdx_chi4 *h, int64_t)
{
    MDX_TRY(chi4_ensure_device(h));
    MDX_TRY(h->ring.ensure(h->frames_seen, h->lags.max_lag, chi4_slab(h), 24 * h->n_points,
                           "a history of %lld frames of %lld points is too large", (long long)h->n_points));
    const int64_t slab = h->ring.slab(chi4_slab(h));
    MDX_REQUIRE(slab < (int64_t(1) << 40) / (4 * h->n_entries),
                "a slab of %lld frames of %lld counters is too large", (long long)slab, (long long)h->n_entries);
    MDX_TRY(h->hist.ensure_ring(h->n_points, h->ring.cap));
    return h->d_qslab.ensure(size_t(4) * h->n_entries * slab);
}

template <int NC>
static void chi4_launch_count(mdx_chi4 *h, dim3 grid, int64_t f0, int seg)
{
    hipLaunchKernelGGL(chi4_count_kernel<NC>, grid, dim3(CHI4_THREADS), 0, h->stream, h->hist.d_hist.as<double>(),
                       h->ring.cap, (int)h->n_points, h->d_offsets.as<int64_t>(), h->n_groups,
                       h->lags.d_lags.as<int64_t>(), h->lags.n(), f0, h->lags.origin_step, h->keep, seg, h->cut,
                       h->d_qslab.as<unsigned int>());
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int chi4_accumulate_rows(mdx_chi4 *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                                int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_points, "%lld rows given, the groups hold %lld", (long long)n_rows,
                (long long)h->n_points);
    const int n = (int)h->n_points;
    const int64_t slab = h->ring.slab(chi4_slab(h));
    const int seg = (int)chi4_segment(h);
    const unsigned lag_runs = (unsigned)ceil_div(h->lags.n(), CHI4_BLOCK_LAGS);
    const unsigned segments = (unsigned)ceil_div(h->n_points, int64_t(seg));
    hipEvent_t ev = h->timer.begin();
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        const int64_t f0 = h->frames_seen;
        h->hist.prepare(vh_prepare_kernel<true>, vh_prepare_kernel<false>, h->stream, pos, src_rows, d_index, n, nf, f0,
                        h->ring.cap);
        MDX_HIP(hipMemsetAsync(h->d_qslab.ptr, 0, size_t(4) * h->n_entries * nf, h->stream));
        const dim3 grid((unsigned)nf, lag_runs, segments);
        switch (h->n_cutoffs) {
        case 1: chi4_launch_count<1>(h, grid, f0, seg); break;
        case 2: chi4_launch_count<2>(h, grid, f0, seg); break;
        case 3: chi4_launch_count<3>(h, grid, f0, seg); break;
        case 4: chi4_launch_count<4>(h, grid, f0, seg); break;
        case 5: chi4_launch_count<5>(h, grid, f0, seg); break;
        case 6: chi4_launch_count<6>(h, grid, f0, seg); break;
        case 7: chi4_launch_count<7>(h, grid, f0, seg); break;
        default: chi4_launch_count<8>(h, grid, f0, seg); break;
        }
        hipLaunchKernelGGL(chi4_fold_kernel,
                           dim3((unsigned)ceil_div(h->n_entries, int64_t(256)),
                                (unsigned)ceil_div(nf, int64_t(CHI4_FOLD_FRAMES))),
                           dim3(256), 0, h->stream, h->d_qslab.as<unsigned int>(), (int)nf, h->n_entries,
                           h->n_groups * h->n_cutoffs, h->lags.d_lags.as<int64_t>(), f0, h->lags.origin_step,
                           h->d_s1.as<unsigned long long>(), h->d_s2.as<unsigned long long>());
        // the contract's count: origins f - lag that are multiples of origin_step, f among the new frames
        h->evaluations += h->n_points * h->lags.origins_met(f0, nf);
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

// S2 <= origins * max_g(n_points[g])^2 must stay below 2^63; needs no device and reads no frame
static int chi4_check_overflow(const mdx_chi4 *h, int64_t n_frames)
{
    const int64_t most = std::numeric_limits<int64_t>::max();
    const int64_t square = h->max_group * h->max_group;         // below (2^31 / 3)^2
    MDX_REQUIRE(n_frames <= most - h->frames_seen && h->frames_seen + n_frames <= most / square,
                "%lld frames after the %lld seen would overflow the int64 sums of Q*Q (the largest group holds %lld "
                "points)", (long long)n_frames, (long long)h->frames_seen, (long long)h->max_group);
    return MDX_OK;
}

extern "C" {

int mdx_chi4_create(mdx_chi4_t *out, int dev, int n_groups, const int64_t *n_points, int n_cutoffs,
                    const double *cutoffs, int n_lags, const int64_t *lags, int64_t origin_step, int zero_dims)
{
    MDX_REQUIRE(out && n_points && cutoffs && lags, "NULL argument");
    MDX_REQUIRE(n_groups >= 1 && n_groups <= 4096, "n_groups out of range");
    MDX_REQUIRE(n_cutoffs >= 1 && n_cutoffs <= CHI4_MAX_CUTOFFS, "n_cutoffs must lie in [1, %d]", CHI4_MAX_CUTOFFS);
    MDX_REQUIRE(n_lags >= 1 && n_lags <= (1 << 16), "lags must hold at least one lag and at most 65536");
    MDX_REQUIRE(origin_step >= 1, "origin_step must be at least 1");
    MDX_REQUIRE(zero_dims >= 0 && zero_dims < 7, "zero_dims must leave at least one component");
    const int64_t limit = (int64_t(1) << 31) / 3;
    int64_t total = 0, largest = 0;
    for (int g = 0; g < n_groups; ++g) {
        MDX_REQUIRE(n_points[g] >= 0 && n_points[g] < limit - total,
                    "group %d: a group size is not negative and all groups hold fewer than 2^31 / 3 points", g);
        total += n_points[g];
        largest = std::max(largest, n_points[g]);
    }
    MDX_REQUIRE(total >= 1, "the groups hold no point");
    for (int c = 0; c < n_cutoffs; ++c) {
        MDX_REQUIRE(std::isfinite(cutoffs[c]) && cutoffs[c] >= 0.0, "cutoffs must be finite and not negative");
        MDX_REQUIRE(c == 0 || cutoffs[c] > cutoffs[c - 1], "cutoffs must be strictly increasing");
    }
    MDX_TRY(LagTable::check(n_lags, lags));
    MDX_REQUIRE(int64_t(n_lags) * n_groups * n_cutoffs < (int64_t(1) << 31), "too many counters");
    mdx_chi4 *h = new mdx_chi4();
    h->dev = dev;
    h->n_groups = n_groups;
    h->n_cutoffs = n_cutoffs;
    h->n_entries = int64_t(n_lags) * n_groups * n_cutoffs;
    h->keep = 7 & ~zero_dims;
    h->n_points = total;
    h->max_group = largest;
    h->lags.assign(n_lags, lags, origin_step);
    for (int c = 0; c < CHI4_MAX_CUTOFFS; ++c)
        h->cut.a2[c] = c < n_cutoffs ? cutoffs[c] * cutoffs[c] : -1.0;
    h->offsets.push_back(0);
    for (int g = 0; g < n_groups; ++g)
        h->offsets.push_back(h->offsets.back() + n_points[g]);
    *out = h;
    return MDX_OK;
}

int mdx_chi4_set_unwrap(mdx_chi4_t h, const double *dims)
{
    MDX_REQUIRE(h, "NULL handle");
    return h->hist.set_unwrap(dims, h->frames_seen, "mdx_chi4_set_unwrap");
}

int mdx_chi4_set_segment_points(mdx_chi4_t h, int64_t points)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_REQUIRE(points >= 0 && points < (int64_t(1) << 31) && points % CHI4_TILE == 0,
                "points must be a multiple of %d in [0, 2^31)", CHI4_TILE);
    MDX_REQUIRE(h->frames_seen == 0, "mdx_chi4_set_segment_points must be called before the first frame");
    h->segment_points = points;
    return MDX_OK;
}

// The routes have a rule of their own: frames that would overflow the sums are refused before the route's checks.
int mdx_chi4_accumulate_device(mdx_chi4_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,
                               const int32_t *index, int64_t n_index)
{
    MDX_REQUIRE(h && d_pos, "NULL argument");
    MDX_REQUIRE(n_frames >= 0, "bad size");
    MDX_TRY(chi4_check_overflow(h, n_frames));
    return entry_accumulate_device(h, d_pos, n_atoms, n_frames, index, n_index, chi4_prepare, chi4_accumulate_rows);
}

int mdx_chi4_accumulate(mdx_chi4_t h, const float *pos, int64_t n, int64_t n_frames)
{
    MDX_REQUIRE(h && pos, "NULL argument");
    MDX_REQUIRE(n_frames >= 0, "bad size");
    MDX_TRY(chi4_check_overflow(h, n_frames));
    return entry_accumulate(h, pos, n, n_frames, chi4_prepare, chi4_accumulate_rows);
}

// Frames straight from a trajectory file.  index: host int32[n_index] particle indices in the order of the
// concatenated groups, or NULL for the file's first n_index particles.
int mdx_chi4_accumulate_traj(mdx_chi4_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                             const int32_t *index, int64_t n_index)
{
    MDX_REQUIRE(h && traj, "NULL handle");
    MDX_REQUIRE(n_frames >= 0, "bad frame list");
    MDX_TRY(chi4_check_overflow(h, n_frames));
    return entry_accumulate_traj(h, traj, frames, n_frames, index, n_index, chi4_prepare, chi4_accumulate_rows);
}

int mdx_chi4_result(mdx_chi4_t h, int64_t *sums, int64_t *square_sums, int64_t *n_origins)
{
    MDX_REQUIRE(h && sums && square_sums && n_origins, "NULL argument");
    MDX_TRY(chi4_ensure_device(h));
    MDX_TRY(h->collect());
    // uint64 sums below 2^63 (chi4_check_overflow): they fit an int64
    MDX_HIP(hipMemcpy(sums, h->d_s1.ptr, size_t(8) * h->n_entries, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(square_sums, h->d_s2.ptr, size_t(8) * h->n_entries, hipMemcpyDeviceToHost));
    for (int k = 0; k < h->lags.n(); ++k)
        n_origins[k] = h->lags.origins_seen(h->frames_seen, h->lags.lags[k]);
    return MDX_OK;
}

int mdx_chi4_stats(mdx_chi4_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    if (evaluations) *evaluations = h->evaluations;
    return MDX_OK;
}

}  // extern "C"

MDX_LAZY_FRAME_LIFE_CYCLE(chi4, chi4_zero, unchecked)
MDX_FRAME_SET_SLAB_FRAMES(chi4, CHI4_SLAB_MAX)
MDX_FRAME_RING_PLAN(chi4, chi4_slab)
