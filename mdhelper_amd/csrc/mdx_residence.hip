// mdx_residence.hip — pair residence (contact survival functions) on gfx950 (MI355X).
//
// Per frame the pairs (i of set 1, j of set 2, j != i when both are one set) whose minimum-image distance lies within
// the cutoff, kept as capped per-row contact lists in a ring of frames in HBM; per lag the sizes of the intersections
// of an origin's contact set with the set of the frame a lag later (intermittent) and with the sets of every frame up
// to there (continuous).  Contract, cap and kernel shape: mdx_residence_device.hpp; this unit is compiled with
// contraction off and spells its float64 operations out.
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
#include "mdx_residence_device.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_prs_dev;

namespace {

constexpr int64_t PRS_HISTORY_BYTES = int64_t(256) << 20;   // what the frames of a default slab take in HBM

}  // namespace

struct mdx_prs : LazyFrameEngine {
    int keep = 7;
    bool same = false;
    int64_t n1 = 0, n2 = 0, n_rows = 0;         // n_rows: rows of an incoming frame (n1 with same, else n1 + n2)
    LagTable lags;
    LagRing ring;                       // frames the rings hold
    PairBox box;
    CappedLists lists;                  // the rings of contact lists
    SurvivalWalk walk;
    double rc2 = 0.0;
    DeviceBuffer d_contacts, d_slab;    // d_contacts: uint64, one per frame seen

    int64_t rows_wanted() const { return n_rows; }
    const char *rows_noun() const { return "sets"; }
    int64_t ring_lag() const { return lags.max_lag; }
    void clear_counters() { lists.max_row = 0; }
    void free_device()
    {
        release({&lags.d_lags, &walk.d_sums, &d_contacts, &lists.d_ctl, &d_slab, &lists.d_len, &lists.d_list,
                 &walk.d_mask});
    }
};

// bytes a frame takes: its gathered rows while it is in flight, its lists and masks while it is in the rings
static int64_t prs_frame_bytes(const mdx_prs *h)
{
    return 12 * h->n_rows + (int64_t(h->lists.max_nb) + 1) * 4 * h->n1 + 8 * h->n1;
}

static int64_t prs_slab(const mdx_prs *h)
{
    return pair_slab_frames(h->slab_frames, PRS_HISTORY_BYTES, prs_frame_bytes(h));
}

static int prs_zero(mdx_prs *h)
{
    MDX_TRY(h->walk.zero(h->lags.n(), h->stream));
    if (h->d_contacts.ptr)
        MDX_HIP(hipMemsetAsync(h->d_contacts.ptr, 0, h->d_contacts.bytes, h->stream));
    return h->lists.zero(h->stream);
}

// the device side of the handle: tables and counters
static int prs_build(mdx_prs *h)
{
    MDX_TRY(h->walk.ensure(h->lags.n()));
    MDX_TRY(h->lists.ensure_ctl());
    MDX_TRY(h->lags.upload());
    return prs_zero(h);
}

static int prs_ensure_device(mdx_prs *h) { return h->ensure_device(prs_build); }

// What a route prepares before the first kernel: the device side, and before the first frame of a pass the rings and
// the slab.
static int prs_prepare(mdx_prs *h, int64_t)
{
    MDX_TRY(prs_ensure_device(h));
    MDX_TRY(h->ring.ensure(h->frames_seen, h->lags.max_lag, prs_slab(h), prs_frame_bytes(h),
                           "a history of %lld frames of %lld points with %d neighbors each is too large",
                           (long long)h->n1, h->lists.max_nb));
    MDX_TRY(h->d_slab.ensure(size_t(12) * h->n_rows * h->ring.slab(prs_slab(h))));
    MDX_TRY(h->lists.ensure(h->n1, h->ring.cap));
    return h->walk.ensure_mask(h->n1, h->ring.cap);
}

// With the stream idle: the largest row seen; a row beyond the cap refuses the results until a reset.
static int prs_check_rows(mdx_prs *h)
{
    return h->lists.check("row", "contacts");
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int prs_accumulate_rows(mdx_prs *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                               int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_rows, "%lld rows given, the sets hold %lld", (long long)n_rows, (long long)h->n_rows);
    MDX_TRY(grow_frames(h->d_contacts, h->stream, 8, h->frames_seen, h->frames_seen + n_frames));
    const int n = (int)h->n_rows, n1 = (int)h->n1, max_nb = h->lists.max_nb;
    int *len = h->lists.d_len.as<int>(), *list = h->lists.d_list.as<int>();
    const int64_t slab = h->ring.slab(prs_slab(h));
    const int64_t n_jchunks = ceil_div(h->n2, PRS_JCHUNK);
    const int64_t blocks = ceil_div(h->n1, PRS_TILE) * n_jchunks;
    hipEvent_t ev = h->timer.begin();
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        const int64_t f_lo = h->frames_seen;
        launch_gather<false>(h->stream, pos, src_rows, d_index, n, nf, h->d_slab.as<float>());
        // the rows of the new frames start empty
        MDX_TRY(h->ring.zero_slots(len, size_t(4) * n1, f_lo, nf, h->stream));
        const auto contact = h->keep == 7 ? prs_contact_kernel<true> : prs_contact_kernel<false>;
        hipLaunchKernelGGL(contact, dim3((unsigned)blocks, 1, (unsigned)nf), dim3(PRS_THREADS), 0, h->stream,
                           h->d_slab.as<float>(), h->ring.cap, n, n1, (int)h->n2, h->same ? 0 : n1, h->same ? 1 : 0,
                           (int)n_jchunks, f_lo, h->box, h->keep, h->rc2, max_nb, len, list,
                           h->d_contacts.as<unsigned long long>(), h->lists.d_ctl.as<int>());
        h->walk.walk(prs_walk_kernel<true>, prs_walk_kernel<false>, h->stream, h->lags, h->ring, h->lists, n1, f_lo,
                     nf);
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

extern "C" {

int mdx_prs_create(mdx_prs_t *out, int dev, int64_t n1, int64_t n2, int same, double cutoff, int n_lags,
                   const int64_t *lags, int64_t origin_step, const double *dims, int zero_dims, int max_neighbors,
                   int continuous)
{
    MDX_REQUIRE(out && lags && dims, "NULL argument");
    MDX_REQUIRE(n_lags >= 1, "lags must hold at least one lag");
    MDX_REQUIRE(n_lags < (1 << 24), "at most 2^24 lags");
    MDX_REQUIRE(origin_step >= 1, "origin_step must be at least 1");
    MDX_REQUIRE(zero_dims >= 0 && zero_dims < 7, "zero_dims must leave at least one component");
    MDX_REQUIRE(max_neighbors >= 1 && max_neighbors <= PRS_MAX_NEIGHBORS, "max_neighbors must lie in [1, %d]",
                PRS_MAX_NEIGHBORS);
    MDX_REQUIRE(n1 >= 1 && n2 >= 1, "both sets must hold at least one point");
    MDX_REQUIRE(!same || n1 == n2, "same: both sets are one set, but n1 = %lld and n2 = %lld", (long long)n1,
                (long long)n2);
    const int64_t limit = (int64_t(1) << 31) / 3;
    MDX_REQUIRE(n1 < limit && n2 < limit && (same ? n1 : n1 + n2) < limit,
                "the sets must hold fewer than 2^31 / 3 points");
    MDX_REQUIRE(ceil_div(n1, PRS_TILE) * ceil_div(n2, PRS_JCHUNK) < (int64_t(1) << 31),
                "%lld x %lld points are too many pairs for one launch", (long long)n1, (long long)n2);
    MDX_TRY(LagTable::check(n_lags, lags));
    MDX_REQUIRE(cutoff > 0.0 && std::isfinite(cutoff), "cutoff must be positive and finite");
    PairBox box;
    int keep = 7;
    MDX_TRY(check_box_cutoff(dims, zero_dims, cutoff, &box, &keep));
    mdx_prs *h = new mdx_prs();
    h->dev = dev;
    h->n1 = n1;
    h->n2 = n2;
    h->same = same != 0;
    h->walk.continuous = continuous != 0;
    h->n_rows = same ? n1 : n1 + n2;
    h->keep = keep;
    h->box = box;
    h->lists.max_nb = max_neighbors;
    h->lags.assign(n_lags, lags, origin_step);
    h->rc2 = cutoff * cutoff;
    *out = h;
    return MDX_OK;
}

int mdx_prs_result(mdx_prs_t h, int64_t *intermittent, int64_t *continuous, int64_t *origin_counts)
{
    MDX_REQUIRE(h && intermittent && continuous && origin_counts, "NULL argument");
    MDX_TRY(prs_ensure_device(h));
    MDX_TRY(h->collect());
    MDX_TRY(prs_check_rows(h));
    // sums of at most frames x n1 x max_neighbors each
    return h->walk.result(h->lags.n(), intermittent, continuous, origin_counts);
}

int mdx_prs_contacts(mdx_prs_t h, int64_t *out, int64_t n)
{
    MDX_REQUIRE(h && (out || n == 0), "NULL argument");
    MDX_REQUIRE(n >= 0 && n <= h->frames_seen, "%lld frames asked for, %lld seen", (long long)n,
                (long long)h->frames_seen);
    if (n == 0)
        return MDX_OK;
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(prs_check_rows(h));
    MDX_HIP(hipMemcpy(out, h->d_contacts.ptr, size_t(8) * n, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_prs_stats(mdx_prs_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *max_row)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    if (h->ready)
        MDX_TRY(h->lists.look());
    if (evaluations) *evaluations = h->frames_seen * (h->n1 * h->n2 - (h->same ? h->n1 : 0));
    if (max_row) *max_row = h->lists.max_row;
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(prs, prs_prepare, prs_accumulate_rows)
MDX_LAZY_FRAME_LIFE_CYCLE(prs, prs_zero, prs_check_rows)
MDX_FRAME_SET_SLAB_FRAMES(prs, PRS_SLAB_MAX)
MDX_FRAME_RING_PLAN(prs, prs_slab)
