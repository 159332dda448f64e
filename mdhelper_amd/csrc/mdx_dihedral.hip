// mdx_dihedral.hip — dihedral (torsion) angles, conformer states and their lifetimes on gfx950 (MI355X).
//
// Per frame the cosine and sine of the torsion angle of four rows (with the minimum image where a box is set), its bin
// in a histogram over [-180, 180) degrees and its conformer state; per group the histogram, per frame and group the
// state populations, per group the state-to-state transitions between consecutive frames, and per lag the torsional
// autocorrelation sum of cos(phi(f) - phi(f - lag)), the cases that are in the same state again (intermittent) and
// the cases that never left it (continuous).  Contract, kernel shape and summation order: mdx_dihedral_device.hpp;
// this unit is compiled with contraction off and spells its float64 operations out.
//
// c, s, the state and the run length of a state go into rings of max(max lag, 1) + slab frames in HBM, so that a lag
// reaches back across slabs and calls; every (lag, dihedral) has one float64 accumulator that receives its terms in
// frame order, and everything else is an integer added with integer atomics.  The results repeat bit for bit whatever
// route the frames take and however they are split into calls or slabs.
//
// Not built: improper dihedrals as such (any four distinct rows are taken, but there is no out-of-plane convention),
// varying or triclinic boxes, an origin_step, more than one rank.
//
// A handle touches its device with the first frame (or result): creating one, and every argument error, needs none.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_lag_history.hpp"
#include "mdx_dihedral_device.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_dih_dev;

namespace {

constexpr int64_t DIH_HISTORY_BYTES = int64_t(256) << 20;   // what the frames of a default slab take in the rings
constexpr int64_t DIH_FRAME_BYTES = 21;                     // per dihedral: c and s, the state, the run length
constexpr int64_t DIH_MAX_BINS = int64_t(1) << 20;

}  // namespace

struct mdx_dih : LazyFrameEngine {
    int n_groups = 0, n_bins = 0, n_states = 0;
    int64_t n_dihedrals = 0, n_rows = 0;
    int64_t evaluations = 0;
    int64_t degenerate = 0;             // degenerate dihedrals seen, as of the last look
    LagTable lags;
    LagRing ring;
    bool boxed = false;
    PairBox box = {{0, 0, 0}, {0, 0, 0}};
    std::vector<DihTile> tiles;
    std::vector<int> quads, state_of_bin;
    std::vector<double> inner;          // the inner thresholds t[1] ... t[n_half - 1]
    std::vector<int64_t> offsets;
    // d_tally: uint64 counts [G][n_bins], transitions [G][S][S], same [n_lags][G], stay [n_lags][G], degenerate [1];
    // d_state_counts: uint64 [frames seen][G][S]
    DeviceBuffer d_tiles, d_quads, d_offsets, d_inner, d_state_of_bin, d_acc, d_sums, d_hist, d_state, d_run, d_tally,
        d_state_counts;

    int64_t n_counts() const { return int64_t(n_groups) * n_bins; }
    int64_t n_moves() const { return int64_t(n_groups) * n_states * n_states; }
    int64_t n_lag_groups() const { return int64_t(lags.n()) * n_groups; }
    int64_t tally_words() const { return n_counts() + n_moves() + 2 * n_lag_groups() + 1; }
    unsigned long long *counts() const { return d_tally.as<unsigned long long>(); }
    unsigned long long *moves() const { return counts() + n_counts(); }
    unsigned long long *same() const { return moves() + n_moves(); }
    unsigned long long *stay() const { return same() + n_lag_groups(); }
    unsigned long long *ctl() const { return stay() + n_lag_groups(); }
    int64_t ring_lag() const { return std::max<int64_t>(lags.max_lag, 1); }     // run(f) needs frame f - 1

    int64_t rows_wanted() const { return n_rows; }
    const char *rows_noun() const { return "quads"; }
    void clear_counters() { evaluations = degenerate = 0; }
    void free_device()
    {
        release({&d_tiles, &d_quads, &d_offsets, &d_inner, &d_state_of_bin, &lags.d_lags, &d_acc, &d_sums, &d_hist,
                 &d_state, &d_run, &d_tally, &d_state_counts});
    }
};

static int64_t dih_slab(const mdx_dih *h)
{
    if (h->slab_frames > 0)
        return h->slab_frames;
    return std::min(DIH_SLAB_MAX, std::max<int64_t>(1, DIH_HISTORY_BYTES / (DIH_FRAME_BYTES * h->n_dihedrals)));
}

static int dih_zero(mdx_dih *h)
{
    MDX_HIP(hipMemsetAsync(h->d_acc.ptr, 0, size_t(8) * h->lags.n() * h->n_dihedrals, h->stream));
    MDX_HIP(hipMemsetAsync(h->d_tally.ptr, 0, size_t(8) * h->tally_words(), h->stream));
    if (h->d_state_counts.ptr)
        MDX_HIP(hipMemsetAsync(h->d_state_counts.ptr, 0, h->d_state_counts.bytes, h->stream));
    h->degenerate = 0;
    return MDX_OK;
}

// the device side of the handle: tables, counters and accumulators
static int dih_build(mdx_dih *h)
{
    const size_t n_inner = std::max<size_t>(h->inner.size(), 1);
    MDX_TRY(h->d_tiles.ensure(sizeof(DihTile) * h->tiles.size()));
    MDX_TRY(h->d_quads.ensure(size_t(16) * h->n_dihedrals));
    MDX_TRY(h->d_offsets.ensure(size_t(8) * (h->n_groups + 1)));
    MDX_TRY(h->d_inner.ensure(size_t(8) * n_inner));
    MDX_TRY(h->d_state_of_bin.ensure(size_t(4) * h->n_bins));
    MDX_TRY(h->d_acc.ensure(size_t(8) * h->lags.n() * h->n_dihedrals));
    MDX_TRY(h->d_sums.ensure(size_t(8) * h->n_lag_groups()));
    MDX_TRY(h->d_tally.ensure(size_t(8) * h->tally_words()));
    MDX_HIP(hipMemcpy(h->d_tiles.ptr, h->tiles.data(), sizeof(DihTile) * h->tiles.size(), hipMemcpyHostToDevice));
    MDX_HIP(hipMemcpy(h->d_quads.ptr, h->quads.data(), size_t(16) * h->n_dihedrals, hipMemcpyHostToDevice));
    MDX_HIP(hipMemcpy(h->d_offsets.ptr, h->offsets.data(), size_t(8) * (h->n_groups + 1), hipMemcpyHostToDevice));
    if (!h->inner.empty())
        MDX_HIP(hipMemcpy(h->d_inner.ptr, h->inner.data(), size_t(8) * h->inner.size(), hipMemcpyHostToDevice));
    MDX_HIP(hipMemcpy(h->d_state_of_bin.ptr, h->state_of_bin.data(), size_t(4) * h->n_bins, hipMemcpyHostToDevice));
    MDX_TRY(h->lags.upload());
    return dih_zero(h);
}

static int dih_ensure_device(mdx_dih *h) { return h->ensure_device(dih_build); }

// What a route prepares before the first kernel: the device side, and before the first frame of a pass the rings.
static int dih_prepare(mdx_dih *h, int64_t)
{
    MDX_TRY(dih_ensure_device(h));
    MDX_TRY(h->ring.ensure(h->frames_seen, h->ring_lag(), dih_slab(h), DIH_FRAME_BYTES * h->n_dihedrals,
                           "a history of %lld frames of %lld dihedrals is too large", (long long)h->n_dihedrals));
    MDX_TRY(h->d_hist.ensure(size_t(16) * h->n_dihedrals * h->ring.cap));
    MDX_TRY(h->d_state.ensure(size_t(1) * h->n_dihedrals * h->ring.cap));
    return h->d_run.ensure(size_t(4) * h->n_dihedrals * h->ring.cap);
}

// With the stream idle: the degenerate dihedrals seen; one of them refuses the results until a reset.
static int dih_look(mdx_dih *h)
{
    unsigned long long seen = 0;
    MDX_HIP(hipMemcpy(&seen, h->ctl(), 8, hipMemcpyDeviceToHost));
    h->degenerate = (int64_t)seen;
    return MDX_OK;
}

static int dih_check(mdx_dih *h)
{
    MDX_TRY(dih_look(h));
    MDX_REQUIRE(h->degenerate == 0,
                "%lld dihedrals had no angle (three atoms on a line, two on one point, or a length that is not "
                "finite): their averages are undefined (reset starts over)", (long long)h->degenerate);
    return MDX_OK;
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int dih_accumulate_rows(mdx_dih *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                               int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_rows, "%lld rows given, the quads hold %lld", (long long)n_rows,
                (long long)h->n_rows);
    MDX_TRY(grow_frames(h->d_state_counts, h->stream, size_t(8) * h->n_groups * h->n_states, h->frames_seen,
                        h->frames_seen + n_frames));
    const int n = (int)h->n_dihedrals, n_tiles = (int)h->tiles.size();
    const int64_t slab = h->ring.slab(dih_slab(h)), cap = h->ring.cap;
    const unsigned tile_blocks = (unsigned)ceil_div(n_tiles, DIH_BLOCK_TILES);
    const dim3 cor_grid((unsigned)n_tiles, (unsigned)ceil_div(h->lags.n(), DIH_BLOCK_LAGS));
    const bool lds = h->n_bins <= DIH_LDS_BINS;
    const auto prepare = h->boxed ? (lds ? dih_prepare_kernel<true, true> : dih_prepare_kernel<true, false>)
                                  : (lds ? dih_prepare_kernel<false, true> : dih_prepare_kernel<false, false>);
    hipEvent_t ev = h->timer.begin();
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        const int64_t f0 = h->frames_seen;
        hipLaunchKernelGGL(prepare, dim3(tile_blocks, (unsigned)ceil_div(nf, DIH_BLOCK_FRAMES)), dim3(DIH_THREADS), 0,
                           h->stream, pos, src_rows, d_index, h->d_quads.as<int>(), h->d_tiles.as<DihTile>(), n_tiles,
                           n, h->n_groups, (int)nf, f0, cap, h->box, h->d_inner.as<double>(), h->n_bins,
                           h->d_state_of_bin.as<int>(), h->n_states, h->d_hist.as<double>(),
                           h->d_state.as<unsigned char>(), h->counts(),
                           h->d_state_counts.as<unsigned long long>(), h->ctl());
        hipLaunchKernelGGL(dih_run_kernel, dim3(tile_blocks), dim3(DIH_THREADS), 0, h->stream,
                           h->d_state.as<unsigned char>(), cap, n, h->d_tiles.as<DihTile>(), n_tiles, h->n_states, f0,
                           f0 + nf, h->d_run.as<int>(), h->moves());
        hipLaunchKernelGGL(dih_correlate_kernel, cor_grid, dim3(DIH_TILE * DIH_BLOCK_LAGS), 0, h->stream,
                           h->d_hist.as<double>(), h->d_state.as<unsigned char>(), h->d_run.as<int>(), cap, n,
                           h->n_groups, h->d_tiles.as<DihTile>(), h->lags.d_lags.as<int64_t>(), h->lags.n(), f0,
                           f0 + nf, h->d_acc.as<double>(), h->same(), h->stay());
        h->evaluations += h->n_dihedrals * h->lags.origins_met(f0, nf);
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

// with the stream idle: n uint64 words of the tally as int64 (counts below 2^63 each)
static int dih_read(int64_t *out, const unsigned long long *words, int64_t n)
{
    MDX_HIP(hipMemcpy(out, words, size_t(8) * n, hipMemcpyDeviceToHost));
    return MDX_OK;
}

extern "C" {

int mdx_dih_create(mdx_dih_t *out, int dev, int n_groups, const int64_t *n_dihedrals, int64_t n_rows,
                   const int32_t *quads, int n_bins, const double *thresholds, int n_states,
                   const int32_t *state_of_bin, int n_lags, const int64_t *lags)
{
    MDX_REQUIRE(out && n_dihedrals && quads && thresholds && state_of_bin && lags, "NULL argument");
    MDX_REQUIRE(n_groups >= 1 && n_groups <= 4096, "n_groups out of range");
    MDX_REQUIRE(n_lags >= 1 && n_lags <= (1 << 24), "lags must hold at least one lag");
    MDX_REQUIRE(n_bins >= 2 && n_bins <= DIH_MAX_BINS && n_bins % 2 == 0,
                "n_bins must be even and lie in [2, %lld]", (long long)DIH_MAX_BINS);
    MDX_REQUIRE(n_states >= 1 && n_states <= DIH_MAX_STATES, "n_states must lie in [1, %d]", DIH_MAX_STATES);
    const int64_t limit = (int64_t(1) << 31) / 4;
    MDX_REQUIRE(n_rows >= 4 && n_rows < limit, "n_rows must lie in [4, 2^31 / 4)");
    int64_t total = 0;
    for (int g = 0; g < n_groups; ++g) {
        MDX_REQUIRE(n_dihedrals[g] >= 0 && n_dihedrals[g] < limit - total,
                    "group %d: a group size is not negative and all groups hold fewer than 2^31 / 4 dihedrals", g);
        total += n_dihedrals[g];
    }
    MDX_REQUIRE(total >= 1, "the groups hold no dihedral");
    for (int64_t v = 0; v < total; ++v) {
        const int32_t *q = quads + 4 * v;
        for (int i = 0; i < 4; ++i) {
            MDX_REQUIRE(q[i] >= 0 && q[i] < n_rows, "dihedral %lld: row %d out of range [0, %lld)", (long long)v, q[i],
                        (long long)n_rows);
            for (int j = 0; j < i; ++j)
                MDX_REQUIRE(q[i] != q[j], "dihedral %lld: row %d is named twice", (long long)v, q[i]);
        }
    }
    const int n_half = n_bins / 2;
    for (int m = 0; m < n_half; ++m)
        MDX_REQUIRE(thresholds[m] > thresholds[m + 1],
                    "thresholds must be strictly decreasing: [%d] = %g, [%d] = %g", m, thresholds[m], m + 1,
                    thresholds[m + 1]);
    for (int b = 0; b < n_bins; ++b)
        MDX_REQUIRE(state_of_bin[b] >= 0 && state_of_bin[b] < n_states, "state_of_bin[%d] = %d out of range [0, %d)",
                    b, state_of_bin[b], n_states);
    MDX_TRY(LagTable::check(n_lags, lags));
    MDX_REQUIRE(lags[n_lags - 1] < (int64_t(1) << 31), "lags must lie below 2^31: a run length is an int32");
    MDX_REQUIRE(int64_t(n_lags) * n_groups < (int64_t(1) << 30), "too many sums");
    MDX_REQUIRE(int64_t(n_bins) * n_groups < (int64_t(1) << 30), "too many bins");
    mdx_dih *h = new mdx_dih();
    h->dev = dev;
    h->n_groups = n_groups;
    h->n_bins = n_bins;
    h->n_states = n_states;
    h->n_dihedrals = total;
    h->n_rows = n_rows;
    h->lags.assign(n_lags, lags);
    h->quads.assign(quads, quads + 4 * total);
    h->inner.assign(thresholds + 1, thresholds + n_half);
    h->state_of_bin.assign(state_of_bin, state_of_bin + n_bins);
    // the tiles of every group (a tile never spans two groups) and the groups' dihedral ranges
    h->offsets.push_back(0);
    int64_t first = 0;
    for (int g = 0; g < n_groups; ++g) {
        for (int64_t j = 0; j < n_dihedrals[g]; j += DIH_TILE)
            h->tiles.push_back(DihTile{int(first + j), int(std::min<int64_t>(DIH_TILE, n_dihedrals[g] - j)), g});
        first += n_dihedrals[g];
        h->offsets.push_back(first);
    }
    *out = h;
    return MDX_OK;
}

int mdx_dih_set_box(mdx_dih_t h, const double *dims)
{
    MDX_REQUIRE(h, "NULL handle");
    if (dims)
        for (int c = 0; c < 3; ++c)
            MDX_REQUIRE(dims[c] > 0.0 && std::isfinite(dims[c]), "dims[%d] must be positive and finite", c);
    MDX_REQUIRE(h->frames_seen == 0, "mdx_dih_set_box must be called before the first frame");
    h->boxed = dims != nullptr;
    for (int c = 0; c < 3; ++c) {
        h->box.L[c] = dims ? dims[c] : 0.0;
        h->box.inv[c] = dims ? 1.0 / dims[c] : 0.0;
    }
    return MDX_OK;
}

int mdx_dih_result(mdx_dih_t h, double *sums, int64_t *same, int64_t *stay)
{
    MDX_REQUIRE(h && sums && same && stay, "NULL argument");
    MDX_TRY(dih_ensure_device(h));
    hipLaunchKernelGGL(dih_fold_kernel, dim3((unsigned)ceil_div(h->n_lag_groups(), 256)), dim3(256), 0, h->stream,
                       h->d_acc.as<double>(), (int)h->n_dihedrals, h->d_offsets.as<int64_t>(), h->n_groups,
                       h->lags.n(), h->d_sums.as<double>());
    MDX_TRY(h->collect());
    MDX_TRY(dih_check(h));
    MDX_HIP(hipMemcpy(sums, h->d_sums.ptr, size_t(8) * h->n_lag_groups(), hipMemcpyDeviceToHost));
    MDX_TRY(dih_read(same, h->same(), h->n_lag_groups()));
    return dih_read(stay, h->stay(), h->n_lag_groups());
}

int mdx_dih_dihedral_sums(mdx_dih_t h, double *out)
{
    MDX_REQUIRE(h && out, "NULL argument");
    MDX_TRY(dih_ensure_device(h));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(dih_check(h));
    MDX_HIP(hipMemcpy(out, h->d_acc.ptr, size_t(8) * h->lags.n() * h->n_dihedrals, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_dih_counts(mdx_dih_t h, int64_t *out)
{
    MDX_REQUIRE(h && out, "NULL argument");
    MDX_TRY(dih_ensure_device(h));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(dih_check(h));
    return dih_read(out, h->counts(), h->n_counts());
}

int mdx_dih_transitions(mdx_dih_t h, int64_t *out)
{
    MDX_REQUIRE(h && out, "NULL argument");
    MDX_TRY(dih_ensure_device(h));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(dih_check(h));
    return dih_read(out, h->moves(), h->n_moves());
}

int mdx_dih_state_counts(mdx_dih_t h, int64_t *out, int64_t n)
{
    MDX_REQUIRE(h && (out || n == 0), "NULL argument");
    MDX_REQUIRE(n >= 0 && n <= h->frames_seen, "%lld frames asked for, %lld seen", (long long)n,
                (long long)h->frames_seen);
    if (n == 0)
        return MDX_OK;
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(dih_check(h));
    return dih_read(out, h->d_state_counts.as<unsigned long long>(), n * h->n_groups * h->n_states);
}

int mdx_dih_stats(mdx_dih_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *degenerate)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    if (h->ready)
        MDX_TRY(dih_look(h));
    if (evaluations) *evaluations = h->evaluations;
    if (degenerate) *degenerate = h->degenerate;
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(dih, dih_prepare, dih_accumulate_rows)
MDX_LAZY_FRAME_LIFE_CYCLE(dih, dih_zero, dih_check)
MDX_FRAME_SET_SLAB_FRAMES(dih, DIH_SLAB_MAX)
MDX_FRAME_RING_PLAN(dih, dih_slab)
