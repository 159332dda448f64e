// mdx_bond_order.hip — bond-orientational order (Steinhardt q_l and the neighbour-averaged qbar_l) on gfx950 (MI355X).
//
// Per frame the neighbours of every centre (minimum-image distance within one cutoff), kept as capped per-centre
// lists in HBM and sorted into ascending order; from the lists, per requested degree l, the spherical harmonics of
// every bond summed per centre into q_lm, the rotational invariant q_l, and with `averaged` the invariant of q_lm
// averaged over the centre and its neighbours; then the histograms of the values, their per-frame sums and the
// distribution of the coordination numbers.  Contract, tables, kernel shapes and summation orders:
// mdx_bond_order_device.hpp; this unit is compiled with contraction off and spells its float64 operations out.
//
// The float64 sums run over sorted rows in a fixed order and every tally is an integer atomic, so the results are the
// same bits whatever route the frames take and however they are split into calls or slabs.
//
// A handle touches its device with the first frame (or result): creating one, and every argument error, needs none.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_pairs_host.hpp"
#include "mdx_bond_order_device.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace mdx;
using namespace mdx_boo_dev;

namespace {

constexpr int64_t BOO_SLAB_BYTES = int64_t(256) << 20;  // what the frames of a default slab take in HBM
constexpr int64_t BOO_MAX_BINS = int64_t(1) << 20;
constexpr double BOO_FOUR_PI = 4.0 * 3.141592653589793;

// double(P) of P = (l + m)! / (l - m)! = (l - m + 1) ... (l + m), correctly rounded: the odd part of P is below 2^64
// for l <= 12 and is widened with one rounding; the power of two is exact
double boo_rising_product(int l, int m)
{
    uint64_t odd = 1;
    int twos = 0;
    for (int k = l - m + 1; k <= l + m; ++k) {
        int v = k;
        while (v % 2 == 0) {
            v /= 2;
            ++twos;
        }
        odd *= uint64_t(v);
    }
    return std::ldexp(double(odd), twos);
}

// the contract's host tables
void boo_fill_tables(BooTables *t)
{
    std::memset(t, 0, sizeof *t);
    for (int n = 0; n < BOO_TABLE; ++n)
        for (int m = 0; m + 2 <= n; ++m) {
            t->a[n][m] = double(2 * n - 1) / double(n - m);
            t->b[n][m] = double(n + m - 1) / double(n - m);
        }
    for (int l = 0; l < BOO_TABLE; ++l) {
        for (int m = 0; m <= l; ++m) {
            const double root = std::sqrt(double(2 * l + 1) / (BOO_FOUR_PI * boo_rising_product(l, m)));
            t->norm[l][m] = m % 2 ? -root : root;
        }
        t->k[l] = BOO_FOUR_PI / double(2 * l + 1);
    }
}

using QlmKernel = void (*)(const float *, int, int, int, PairBox, int, const int *, const int *, const BooTables *,
                           double *, double *, int64_t);
using AverageKernel = void (*)(int, int, const int *, const int *, const BooTables *, const double *, double *,
                               int64_t);

template <int L>
void boo_kernels_from(int l, QlmKernel *qlm, AverageKernel *average)
{
    if (l == L) {
        *qlm = boo_qlm_kernel<L>;
        *average = boo_average_kernel<L>;
        return;
    }
    if constexpr (L < BOO_MAX_DEGREE)
        boo_kernels_from<L + 1>(l, qlm, average);
}

}  // namespace

struct mdx_boo : LazyFrameEngine {
    bool same = false, averaged = false, keep_values = false, lds_hist = true;
    int D = 0, K = 1, l_max = 0;
    int degrees[BOO_MAX_DEGREES] = {0, 0, 0, 0};
    QlmKernel qlm_kernel[BOO_MAX_DEGREES] = {};
    AverageKernel average_kernel[BOO_MAX_DEGREES] = {};
    int64_t n0 = 0, n1 = 0, n_rows = 0, n_bins = 0;
    double rc2 = 0.0;
    int64_t degenerate = 0;             // neighbours on their centre, as of the last look
    PairBox box;
    CappedLists lists;                  // the centres' neighbour lists of a slab
    std::vector<double> edges;
    std::vector<double> values;         // keep_values: [frames seen][D][K][n0] on the host
    // d_counts: uint64 counts [D][K][n_bins], outside [D][K], coordination [max_nb + 1], degenerate [1]
    // d_qlm: double [D][slab][2 l_max + 2][n0] at most; d_values: double [slab][D][K][n0]
    // d_frame_sums: double [frames seen][D][K]; d_counted: uint64 [frames seen]
    DeviceBuffer d_edges, d_tables, d_counts, d_slab, d_qlm, d_values, d_frame_sums, d_counted;

    int64_t DK() const { return int64_t(D) * K; }
    int64_t words() const { return DK() * n_bins + DK() + (lists.max_nb + 1) + 1; }
    unsigned long long *outside_words() { return d_counts.as<unsigned long long>() + DK() * n_bins; }
    unsigned long long *coordination_words() { return outside_words() + DK(); }
    unsigned long long *degenerate_word() { return coordination_words() + (lists.max_nb + 1); }
    int64_t qlm_frame_words() const { return int64_t(2) * (l_max + 1) * n0; }     // of one degree

    int64_t rows_wanted() const { return n_rows; }
    const char *rows_noun() const { return "groups"; }
    void clear_counters() { lists.max_row = 0; degenerate = 0; values.clear(); }
    void free_device()
    {
        release({&d_edges, &d_tables, &d_counts, &lists.d_ctl, &d_slab, &lists.d_len, &lists.d_list, &d_qlm, &d_values,
                 &d_frame_sums, &d_counted});
    }
};

// bytes a frame of a slab takes: its gathered rows, its lists and lengths, q_lm of every degree, its values
static int64_t boo_frame_bytes(const mdx_boo *h)
{
    return 12 * h->n_rows + (int64_t(h->lists.max_nb) + 1) * 4 * h->n0 + 8 * h->D * h->qlm_frame_words() +
           8 * h->DK() * h->n0;
}

static int64_t boo_slab(const mdx_boo *h)
{
    return pair_slab_frames(h->slab_frames, BOO_SLAB_BYTES, boo_frame_bytes(h));
}

static int boo_zero(mdx_boo *h)
{
    MDX_HIP(hipMemsetAsync(h->d_counts.ptr, 0, size_t(8) * h->words(), h->stream));
    if (h->d_frame_sums.ptr)
        MDX_HIP(hipMemsetAsync(h->d_frame_sums.ptr, 0, h->d_frame_sums.bytes, h->stream));
    if (h->d_counted.ptr)
        MDX_HIP(hipMemsetAsync(h->d_counted.ptr, 0, h->d_counted.bytes, h->stream));
    h->degenerate = 0;
    h->values.clear();
    return h->lists.zero(h->stream);
}

// the device side of the handle: edges, tables and counters
static int boo_build(mdx_boo *h)
{
    MDX_TRY(h->d_edges.ensure(size_t(8) * h->edges.size()));
    MDX_TRY(h->d_tables.ensure(sizeof(BooTables)));
    MDX_TRY(h->d_counts.ensure(size_t(8) * h->words()));
    MDX_TRY(h->lists.ensure_ctl());
    BooTables tables;
    boo_fill_tables(&tables);
    MDX_HIP(hipMemcpy(h->d_edges.ptr, h->edges.data(), size_t(8) * h->edges.size(), hipMemcpyHostToDevice));
    MDX_HIP(hipMemcpy(h->d_tables.ptr, &tables, sizeof tables, hipMemcpyHostToDevice));
    return boo_zero(h);
}

static int boo_ensure_device(mdx_boo *h) { return h->ensure_device(boo_build); }

// The buffers of a slab, sized before the first frame of a pass.  Nothing is in flight then (a reset waits for the
// stream), so growing them loses nothing.
static int boo_ensure_slab(mdx_boo *h)
{
    if (h->frames_seen > 0)
        return MDX_OK;
    const int64_t slab = boo_slab(h);
    MDX_REQUIRE(slab < (int64_t(1) << 40) / boo_frame_bytes(h),
                "a slab of %lld frames of %lld rows with %d neighbors each is too large", (long long)slab,
                (long long)h->n_rows, h->lists.max_nb);
    MDX_TRY(h->d_slab.ensure(size_t(12) * h->n_rows * slab));
    MDX_TRY(h->lists.ensure(h->n0, slab));
    MDX_TRY(h->d_qlm.ensure(size_t(8) * h->D * h->qlm_frame_words() * slab));
    MDX_TRY(h->d_values.ensure(size_t(8) * h->DK() * h->n0 * slab));
    return MDX_OK;
}

// with the stream idle: the neighbours on their centre seen, without judging them
static int boo_look(mdx_boo *h)
{
    unsigned long long seen = 0;
    MDX_HIP(hipMemcpy(&seen, h->degenerate_word(), 8, hipMemcpyDeviceToHost));
    h->degenerate = (int64_t)seen;
    return MDX_OK;
}

// With the stream idle: a row beyond the cap, or a neighbour on its centre, refuses the results until a reset.
static int boo_check(mdx_boo *h)
{
    MDX_TRY(h->lists.check("center", "neighbors"));
    MDX_TRY(boo_look(h));
    MDX_REQUIRE(h->degenerate == 0,
                "%lld bonds had no direction (a neighbor on its center): their harmonics are undefined (reset starts "
                "over)", (long long)h->degenerate);
    return MDX_OK;
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int boo_accumulate_rows(mdx_boo *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                               int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    MDX_REQUIRE(n_rows == h->n_rows, "%lld rows given, the groups hold %lld", (long long)n_rows,
                (long long)h->n_rows);
    const int64_t DK = h->DK();
    MDX_TRY(grow_frames(h->d_frame_sums, h->stream, size_t(8) * DK, h->frames_seen, h->frames_seen + n_frames));
    MDX_TRY(grow_frames(h->d_counted, h->stream, 8, h->frames_seen, h->frames_seen + n_frames));
    const int n = (int)h->n_rows, n0 = (int)h->n0, n1 = (int)h->n1, off = h->same ? 0 : n0;
    const int max_nb = h->lists.max_nb;
    int *len = h->lists.d_len.as<int>(), *list = h->lists.d_list.as<int>();
    const int64_t slab = boo_slab(h);       // what boo_ensure_slab sized the buffers for
    const int64_t n_jchunks = ceil_div(h->n1, BOO_JCHUNK);
    const int64_t blocks = ceil_div(h->n0, BOO_TILE) * n_jchunks;
    const unsigned lanes = (unsigned)ceil_div(h->n0, BOO_THREADS);
    const BooTables *tables = h->d_tables.as<BooTables>();
    double *values = h->d_values.as<double>();
    const int64_t value_stride = DK * h->n0;
    const auto bin = h->lds_hist ? boo_bin_kernel<true> : boo_bin_kernel<false>;
    for (int64_t s0 = 0; s0 < n_frames; s0 += slab) {
        const int64_t nf = std::min(slab, n_frames - s0);
        const float *pos = d_pos + s0 * src_rows * 3;
        const int64_t f0 = h->frames_seen;
        hipEvent_t ev = h->timer.begin();
        launch_gather<false>(h->stream, pos, src_rows, d_index, n, nf, h->d_slab.as<float>());
        MDX_HIP(hipMemsetAsync(len, 0, size_t(4) * n0 * nf, h->stream));
        hipLaunchKernelGGL(boo_contact_kernel, dim3((unsigned)blocks, 1, (unsigned)nf), dim3(BOO_THREADS), 0,
                           h->stream, h->d_slab.as<float>(), n, n0, n1, off, int(h->same), (int)n_jchunks, h->box,
                           h->rc2, max_nb, len, list, h->lists.d_ctl.as<int>());
        hipLaunchKernelGGL(boo_rows_kernel, dim3(lanes, (unsigned)nf), dim3(BOO_THREADS), 0, h->stream,
                           h->d_slab.as<float>(), n, n0, off, h->box, max_nb, len, list, f0,
                           h->coordination_words(), h->degenerate_word(), h->d_counted.as<unsigned long long>());
        for (int d = 0; d < h->D; ++d) {
            double *qlm = h->d_qlm.as<double>() + int64_t(d) * h->qlm_frame_words() * slab;
            hipLaunchKernelGGL(h->qlm_kernel[d], dim3(lanes, (unsigned)nf), dim3(BOO_THREADS), 0, h->stream,
                               h->d_slab.as<float>(), n, n0, off, h->box, max_nb, len, list, tables, qlm,
                               values + int64_t(d) * h->K * h->n0, value_stride);
            if (h->averaged)
                hipLaunchKernelGGL(h->average_kernel[d], dim3(lanes, (unsigned)nf), dim3(BOO_THREADS), 0, h->stream,
                                   n0, max_nb, len, list, tables, qlm,
                                   values + (int64_t(d) * h->K + 1) * h->n0, value_stride);
        }
        // a block takes BOO_BIN_CHUNK values: the bound of its uint32 counters (mdx_bond_order_device.hpp)
        hipLaunchKernelGGL(bin, dim3((unsigned)ceil_div(nf * h->n0, BOO_BIN_CHUNK), (unsigned)DK), dim3(BOO_THREADS),
                           0, h->stream, values, nf * h->n0, n0, (int)DK, h->d_edges.as<double>(), (int)h->n_bins,
                           h->d_counts.as<unsigned long long>(), h->outside_words());
        hipLaunchKernelGGL(boo_sum_kernel, dim3((unsigned)(nf * DK)), dim3(BOO_THREADS), 0, h->stream, values, n0,
                           (int)DK, f0, h->d_frame_sums.as<double>());
        h->frames_seen += nf;
        h->timer.end(ev);
        MDX_HIP(hipGetLastError());
        if (h->keep_values) {               // the slab's values leave before the next slab overwrites them
            const size_t count = size_t(nf * value_stride);
            const size_t at = h->values.size();
            h->values.resize(at + count);
            MDX_HIP(hipStreamSynchronize(h->stream));
            MDX_HIP(hipMemcpy(h->values.data() + at, values, size_t(8) * count, hipMemcpyDeviceToHost));
        }
    }
    return MDX_OK;
}

extern "C" {

int mdx_boo_create(mdx_boo_t *out, int dev, int64_t n_centers, int64_t n_neighbors, int same, double cutoff,
                   int n_degrees, const int32_t *degrees, int averaged, int64_t n_bins, const double *edges,
                   const double *dims, int max_neighbors, int keep_values)
{
    MDX_REQUIRE(out && degrees && edges && dims, "NULL argument");
    MDX_REQUIRE(n_degrees >= 1 && n_degrees <= BOO_MAX_DEGREES, "degrees must hold between 1 and %d degrees",
                BOO_MAX_DEGREES);
    for (int d = 0; d < n_degrees; ++d) {
        MDX_REQUIRE(degrees[d] >= 1 && degrees[d] <= BOO_MAX_DEGREE, "degrees[%d] = %d must lie in [1, %d]", d,
                    degrees[d], BOO_MAX_DEGREE);
        for (int e = 0; e < d; ++e)
            MDX_REQUIRE(degrees[e] != degrees[d], "degrees holds %d twice", degrees[d]);
    }
    MDX_REQUIRE(max_neighbors >= 1 && max_neighbors <= BOO_MAX_NEIGHBORS, "max_neighbors must lie in [1, %d]",
                BOO_MAX_NEIGHBORS);
    MDX_REQUIRE(n_centers >= 1, "the centers must hold at least one point");
    MDX_REQUIRE(n_neighbors >= 1, "the neighbors must hold at least one point");
    MDX_REQUIRE(!same || n_neighbors == n_centers, "with same the neighbors are the %lld centers themselves",
                (long long)n_centers);
    MDX_REQUIRE(same || !averaged, "averaged needs same: the neighbors of a center must be centers themselves");
    const int64_t n_rows = same ? n_centers : n_centers + n_neighbors;
    const int64_t limit = (int64_t(1) << 31) / 3;
    MDX_REQUIRE(n_centers < limit && n_neighbors < limit && n_rows < limit,
                "the groups must hold fewer than 2^31 / 3 points");
    MDX_REQUIRE(ceil_div(n_centers, BOO_TILE) * ceil_div(n_neighbors, BOO_JCHUNK) < (int64_t(1) << 31),
                "%lld centers and %lld neighbors are too many pairs for one launch", (long long)n_centers,
                (long long)n_neighbors);
    MDX_REQUIRE(cutoff > 0.0 && std::isfinite(cutoff), "cutoff must be positive and finite");
    PairBox box;
    int keep = 7;
    MDX_TRY(check_box_cutoff(dims, 0, cutoff, &box, &keep));
    MDX_REQUIRE(n_bins >= 1 && n_bins <= BOO_MAX_BINS, "n_bins must lie in [1, %lld]", (long long)BOO_MAX_BINS);
    MDX_REQUIRE(std::isfinite(edges[0]) && std::isfinite(edges[n_bins]), "edges must be finite");
    for (int64_t m = 0; m < n_bins; ++m)
        MDX_REQUIRE(edges[m] < edges[m + 1], "edges must be strictly increasing: [%lld] = %g, [%lld] = %g",
                    (long long)m, edges[m], (long long)(m + 1), edges[m + 1]);
    mdx_boo *h = new mdx_boo();
    h->dev = dev;
    h->n0 = n_centers;
    h->n1 = n_neighbors;
    h->n_rows = n_rows;
    h->same = same != 0;
    h->averaged = averaged != 0;
    h->keep_values = keep_values != 0;
    h->D = n_degrees;
    h->K = averaged ? 2 : 1;
    for (int d = 0; d < n_degrees; ++d) {
        h->degrees[d] = degrees[d];
        h->l_max = std::max(h->l_max, degrees[d]);
        boo_kernels_from<1>(degrees[d], &h->qlm_kernel[d], &h->average_kernel[d]);
    }
    h->rc2 = cutoff * cutoff;
    h->box = box;
    h->lists.max_nb = max_neighbors;
    h->n_bins = n_bins;
    h->lds_hist = n_bins <= BOO_LDS_BINS;
    h->edges.assign(edges, edges + n_bins + 1);
    *out = h;
    return MDX_OK;
}

// what a route prepares before the first kernel
static int boo_prepare(mdx_boo *h, int64_t)
{
    MDX_TRY(boo_ensure_device(h));
    return boo_ensure_slab(h);
}

int mdx_boo_result(mdx_boo_t h, int64_t *counts, int64_t *outside, int64_t *coordination)
{
    MDX_REQUIRE(h && counts && outside && coordination, "NULL argument");
    MDX_TRY(boo_ensure_device(h));
    MDX_TRY(h->collect());
    MDX_TRY(boo_check(h));
    // uint64 counts of fewer than 2^63 values each: they fit an int64
    MDX_HIP(hipMemcpy(counts, h->d_counts.ptr, size_t(8) * h->DK() * h->n_bins, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(outside, h->outside_words(), size_t(8) * h->DK(), hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(coordination, h->coordination_words(), size_t(8) * (h->lists.max_nb + 1),
                      hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_boo_frames(mdx_boo_t h, double *sums, int64_t *counted, int64_t n)
{
    MDX_REQUIRE(h && ((sums && counted) || n == 0), "NULL argument");
    MDX_REQUIRE(n >= 0 && n <= h->frames_seen, "%lld frames asked for, %lld seen", (long long)n,
                (long long)h->frames_seen);
    if (n == 0)
        return MDX_OK;
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(boo_check(h));
    MDX_HIP(hipMemcpy(sums, h->d_frame_sums.ptr, size_t(8) * h->DK() * n, hipMemcpyDeviceToHost));
    MDX_HIP(hipMemcpy(counted, h->d_counted.ptr, size_t(8) * n, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_boo_values(mdx_boo_t h, double *values, int64_t n)
{
    MDX_REQUIRE(h && (values || n == 0), "NULL argument");
    MDX_REQUIRE(h->keep_values, "the values are kept only by an engine created with keep_values");
    MDX_REQUIRE(n >= 0 && n <= h->frames_seen, "%lld frames asked for, %lld seen", (long long)n,
                (long long)h->frames_seen);
    if (n == 0)
        return MDX_OK;
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_TRY(boo_check(h));
    std::memcpy(values, h->values.data(), size_t(8) * h->DK() * h->n0 * n);
    return MDX_OK;
}

int mdx_boo_stats(mdx_boo_t h, int64_t *launches, double *kernel_ms, int64_t *frames, int64_t *evaluations,
                  int64_t *bonds, int64_t *degenerate, int64_t *max_row)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->stats(launches, kernel_ms, frames));
    int64_t entries = 0;
    if (h->ready) {
        MDX_TRY(h->lists.look());
        MDX_TRY(boo_look(h));
        if (bonds) {
            std::vector<uint64_t> words(size_t(h->lists.max_nb + 1));
            MDX_HIP(hipMemcpy(words.data(), h->coordination_words(), size_t(8) * words.size(), hipMemcpyDeviceToHost));
            for (size_t m = 0; m < words.size(); ++m)
                entries += int64_t(m) * int64_t(words[m]);
        }
    }
    if (evaluations) *evaluations = h->frames_seen * (h->n0 * h->n1 - (h->same ? h->n0 : 0));
    if (bonds) *bonds = entries;
    if (degenerate) *degenerate = h->degenerate;
    if (max_row) *max_row = h->lists.max_row;
    return MDX_OK;
}

}  // extern "C"

MDX_FRAME_ROUTES(boo, boo_prepare, boo_accumulate_rows)
MDX_LAZY_FRAME_LIFE_CYCLE(boo, boo_zero, boo_check)
MDX_FRAME_SET_SLAB_FRAMES(boo, BOO_SLAB_MAX)
MDX_FRAME_PLAN(boo, boo_slab)
