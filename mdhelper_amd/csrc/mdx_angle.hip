// mdx_angle.hip — angular distributions (ligand-centre-ligand angles in the first shell) on gfx950 (MI355X).
//
// Per frame the neighbours of every centre among one or several ligand species (minimum-image distance within the
// cutoff of the ligand's species), kept as capped per-centre lists in HBM; from the lists, for every unordered pair of
// neighbours of a centre, the cosine of the angle at the centre, binned against a decreasing table of thresholds per
// pair of ligand species, and the distribution of the per-species coordination numbers.  Contract, cap, kernel shapes
// and the bound that keeps the LDS counters from wrapping: mdx_angle_device.hpp; this unit is compiled with
// contraction off and spells its float64 operations out.
//
// Every result is an integer added with integer atomics, so the results are the same whatever route the frames take
// and however they are split into calls or slabs.
//
// A handle touches its device with the first frame (or result): creating one, and every argument error, needs none.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_pairs_host.hpp"
#include "mdx_angle_device.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

using namespace mdx;
using namespace mdx_ang_dev;

namespace {

constexpr int64_t ANG_SLAB_BYTES = int64_t(256) << 20;  // what the frames of a default slab take in HBM
constexpr int64_t ANG_MAX_BINS = int64_t(1) << 20;

}  // namespace

struct mdx_ang : LazyFrameEngine {
    int n_species = 1, keep = 7;
    bool same = false, uniform = true, lds_hist = true;
    int64_t n0 = 0, n_lig = 0, n_rows = 0, n_bins = 0;
    PairBox box;
    CappedLists lists;                  // the centres' neighbour lists of a slab
    AngGroups groups;
    std::vector<double> inner;          // thresholds[1 ... n_bins - 1]
    // d_counts: uint64 counts [P][n_bins], degenerate [P], coordination [G][max_nb + 1]
    DeviceBuffer d_inner, d_counts, d_slab;

    int64_t pairs() const { return int64_t(n_species) * (n_species + 1) / 2; }
    int64_t words() const { return pairs() * n_bins + pairs() + int64_t(n_species) * (lists.max_nb + 1); }

    int64_t rows_wanted() const { return n_rows; }
    const char *rows_noun() const { return "groups"; }
    void clear_counters() { lists.max_row = 0; }
    void free_device() { release({&d_inner, &d_counts, &lists.d_ctl, &d_slab, &lists.d_len, &lists.d_list}); }
};

// bytes a frame of a slab takes: its gathered rows, its lists and lengths
static int64_t ang_frame_bytes(const mdx_ang *h)
{
    return 12 * h->n_rows + (int64_t(h->lists.max_nb) + 1) * 4 * h->n0;
}

static int64_t ang_slab(const mdx_ang *h)
{
    return pair_slab_frames(h->slab_frames, ANG_SLAB_BYTES, ang_frame_bytes(h));
}

static int ang_zero(mdx_ang *h)
{
    MDX_HIP(hipMemsetAsync(h->d_counts.ptr, 0, size_t(8) * h->words(), h->stream));
    return h->lists.zero(h->stream);
}

// the device side of the handle: thresholds and counters
static int ang_build(mdx_ang *h)
{
    MDX_TRY(h->d_inner.ensure(size_t(8) * std::max<size_t>(h->inner.size(), 1)));
    MDX_TRY(h->d_counts.ensure(size_t(8) * h->words()));
    MDX_TRY(h->lists.ensure_ctl());
    if (!h->inner.empty())
        MDX_HIP(hipMemcpy(h->d_inner.ptr, h->inner.data(), size_t(8) * h->inner.size(), hipMemcpyHostToDevice));
    return ang_zero(h);
}

static int ang_ensure_device(mdx_ang *h) { return h->ensure_device(ang_build); }

// The buffers of a slab, sized before the first frame of a pass.  Nothing is in flight then (a reset waits for the
// stream), so growing them loses nothing.
static int ang_ensure_slab(mdx_ang *h)
{
    if (h->frames_seen > 0)
        return MDX_OK;
    const int64_t slab = ang_slab(h);
    MDX_REQUIRE(slab < (int64_t(1) << 40) / ang_frame_bytes(h),
                "a slab of %lld frames of %lld rows with %d neighbors each is too large", (long long)slab,
                (long long)h->n_rows, h->lists.max_nb);
    MDX_TRY(h->d_slab.ensure(size_t(12) * h->n_rows * slab));
    MDX_TRY(h->lists.ensure(h->n0, slab));
    return MDX_OK;
}

// With the stream idle: the largest row seen; a row beyond the cap refuses the results until a reset.
static int ang_check_rows(mdx_ang *h)
{
    return h->lists.check("center", "neighbors");
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int ang_accumulate_rows(mdx_ang *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                               int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_rows, "%lld rows given, the groups hold %lld", (long long)n_rows,
                (long long)h->n_rows);
    const int n = (int)h->n_rows, n0 = (int)h->n0, n_lig = (int)h->n_lig, off = h->same ? 0 : n0;
    const int max_nb = h->lists.max_nb;
    int *len = h->lists.d_len.as<int>(), *list = h->lists.d_list.as<int>();
    const int64_t slab = ang_slab(h);       // what ang_ensure_slab sized the buffers for
    const int64_t n_jchunks = ceil_div(h->n_lig, ANG_JCHUNK);
    const int64_t blocks = ceil_div(h->n0, ANG_TILE) * n_jchunks;
    const int64_t c_tiles = ceil_div(h->n0, ANG_CTILE);
    const bool all = h->keep == 7;
    unsigned long long *counts = h->d_counts.as<unsigned long long>();
    unsigned long long *degenerate = counts + h->pairs() * h->n_bins;
    unsigned long long *coordination = degenerate + h->pairs();
    const auto contact = h->uniform ? (all ? ang_contact_kernel<true, true> : ang_contact_kernel<false, true>)
                                    : (all ? ang_contact_kernel<true, false> : ang_contact_kernel<false, false>);
    const auto triplet = h->lds_hist ? (all ? ang_triplet_kernel<true, true> : ang_triplet_kernel<false, true>)
                                     : (all ? ang_triplet_kernel<true, false> : ang_triplet_kernel<false, false>);
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        hipEvent_t ev = h->timer.begin();
        launch_gather<false>(h->stream, pos, src_rows, d_index, n, nf, h->d_slab.as<float>());
        MDX_HIP(hipMemsetAsync(len, 0, size_t(4) * n0 * nf, h->stream));
        hipLaunchKernelGGL(contact, dim3((unsigned)blocks, 1, (unsigned)nf), dim3(ANG_THREADS), 0, h->stream,
                           h->d_slab.as<float>(), n, n0, n_lig, off, int(h->same), (int)n_jchunks, h->box, h->keep,
                           h->groups.rc2[0], h->groups, max_nb, len, list, h->lists.d_ctl.as<int>());
        // a block walks at most ANG_BLOCK_TILES tiles: the bound of its uint32 counters (mdx_angle_device.hpp)
        const int64_t n_tiles = c_tiles * nf;
        const int64_t grid = std::max(std::min<int64_t>(n_tiles, ANG_GRID), ceil_div(n_tiles, ANG_BLOCK_TILES));
        hipLaunchKernelGGL(triplet, dim3((unsigned)grid), dim3(ANG_THREADS), 0, h->stream, h->d_slab.as<float>(), n,
                           n0, off, n_tiles, (int)c_tiles, h->box, h->keep, h->groups, h->n_species, max_nb, len, list,
                           h->d_inner.as<double>(), (int)h->n_bins, counts, degenerate, coordination);
        h->frames_seen += nf;
        h->timer.end(ev);
        MDX_HIP(hipGetLastError());
    }
    return MDX_OK;
}

extern "C" {

int mdx_ang_create(mdx_ang_t *out, int dev, int64_t n_centers, int n_species, const int64_t *ligand_sizes, int same,
                   const double *cutoff, int64_t n_bins, const double *thresholds, const double *dims, int zero_dims,
                   int max_neighbors)
{
    MDX_REQUIRE(out && ligand_sizes && cutoff && thresholds && dims, "NULL argument");
    MDX_REQUIRE(n_species >= 1 && n_species <= ANG_MAX_SPECIES, "n_species must lie in [1, %d]", ANG_MAX_SPECIES);
    MDX_REQUIRE(zero_dims >= 0 && zero_dims < 7, "zero_dims must leave at least one component");
    MDX_REQUIRE(max_neighbors >= 1 && max_neighbors <= ANG_MAX_NEIGHBORS, "max_neighbors must lie in [1, %d]",
                ANG_MAX_NEIGHBORS);
    MDX_REQUIRE(n_centers >= 1, "the centers must hold at least one point");
    const int G = n_species;
    int64_t n_lig = 0;
    for (int g = 0; g < G; ++g) {
        MDX_REQUIRE(ligand_sizes[g] >= 1, "ligand group %d must hold at least one point", g);
        MDX_REQUIRE(ligand_sizes[g] < (int64_t(1) << 31) / 3, "the groups must hold fewer than 2^31 / 3 points");
        n_lig += ligand_sizes[g];
    }
    MDX_REQUIRE(!same || (G == 1 && n_lig == n_centers),
                "with same there is one ligand group, of the %lld centers themselves", (long long)n_centers);
    const int64_t n_rows = same ? n_centers : n_centers + n_lig;
    MDX_REQUIRE(n_centers < (int64_t(1) << 31) / 3 && n_rows < (int64_t(1) << 31) / 3,
                "the groups must hold fewer than 2^31 / 3 points");
    MDX_REQUIRE(ceil_div(n_centers, ANG_TILE) * ceil_div(n_lig, ANG_JCHUNK) < (int64_t(1) << 31),
                "%lld centers and %lld ligands are too many pairs for one launch", (long long)n_centers,
                (long long)n_lig);
    double largest = 0.0;
    bool uniform = true;
    for (int g = 0; g < G; ++g) {
        MDX_REQUIRE(cutoff[g] > 0.0 && std::isfinite(cutoff[g]), "cutoff[%d] must be positive and finite", g);
        largest = std::max(largest, cutoff[g]);
        uniform = uniform && cutoff[g] == cutoff[0];
    }
    PairBox box;
    int keep = 7;
    MDX_TRY(check_box_cutoff(dims, zero_dims, largest, &box, &keep));
    MDX_REQUIRE(n_bins >= 1 && n_bins <= ANG_MAX_BINS, "n_bins must lie in [1, %lld]", (long long)ANG_MAX_BINS);
    for (int64_t m = 0; m < n_bins; ++m)
        MDX_REQUIRE(thresholds[m] > thresholds[m + 1],
                    "thresholds must be strictly decreasing: [%lld] = %g, [%lld] = %g", (long long)m, thresholds[m],
                    (long long)(m + 1), thresholds[m + 1]);
    mdx_ang *h = new mdx_ang();
    h->dev = dev;
    h->n0 = n_centers;
    h->n_lig = n_lig;
    h->n_rows = n_rows;
    h->n_species = G;
    h->same = same != 0;
    h->keep = keep;
    h->box = box;
    h->lists.max_nb = max_neighbors;
    h->uniform = uniform;
    h->n_bins = n_bins;
    h->lds_hist = h->pairs() * n_bins <= ANG_HIST_WORDS && n_bins <= ANG_LDS_BINS;
    h->inner.assign(thresholds + 1, thresholds + n_bins);
    int64_t end = 0;
    for (int g = 0; g < ANG_MAX_SPECIES; ++g) {
        end += g < G ? ligand_sizes[g] : 0;
        h->groups.end[g] = g < G ? (int)end : INT_MAX;
        h->groups.rc2[g] = g < G ? cutoff[g] * cutoff[g] : 0.0;
    }
    *out = h;
    return MDX_OK;
}

// what a route prepares before the first kernel
static int ang_prepare(mdx_ang *h, int64_t)
{
    MDX_TRY(ang_ensure_device(h));
    return ang_ensure_slab(h);
}

int mdx_ang_result(mdx_ang_t h, int64_t *counts, int64_t *degenerate, int64_t *coordination)
{
    MDX_REQUIRE(h && counts && degenerate && coordination, "NULL argument");
    MDX_TRY(ang_ensure_device(h));
    MDX_TRY(h->collect());
    MDX_TRY(ang_check_rows(h));
    // uint64 counts of fewer than 2^63 triplets each: they fit an int64
    const size_t n_counts = size_t(8) * h->pairs() * h->n_bins, n_degenerate = size_t(8) * h->pairs();
    const char *src = h->d_counts.as<char>();
    MDX_HIP(hipMemcpy(counts, src, n_counts, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(degenerate, src + n_counts, n_degenerate, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(coordination, src + n_counts + n_degenerate, size_t(8) * h->n_species * (h->lists.max_nb + 1),
                      hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_ang_stats(mdx_ang_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *triplets, int64_t *max_row)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    int64_t sum = 0;
    if (h->ready) {
        MDX_TRY(h->lists.look());
        if (triplets) {
            std::vector<uint64_t> words(size_t(h->pairs() * (h->n_bins + 1)));      // counts, then degenerate
            MDX_HIP(hipMemcpy(words.data(), h->d_counts.ptr, size_t(8) * words.size(), hipMemcpyDeviceToHost));
            for (uint64_t w : words)
                sum += int64_t(w);
        }
    }
    if (evaluations) *evaluations = h->frames_seen * (h->n0 * h->n_lig - (h->same ? h->n0 : 0));
    if (triplets) *triplets = sum;
    if (max_row) *max_row = h->lists.max_row;
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(ang, ang_prepare, ang_accumulate_rows)
MDX_LAZY_FRAME_LIFE_CYCLE(ang, ang_zero, ang_check_rows)
MDX_FRAME_SET_SLAB_FRAMES(ang, ANG_SLAB_MAX)
MDX_FRAME_PLAN(ang, ang_slab)
