// mdx_rouse.hip — per-chain linear projections (Rouse mode amplitudes) on gfx950 (MI355X).
//
// Carries the frame work of analysis.polymer.RouseModes: positions (atoms, or the float64 centres of mass of
// monomers) -> optional global unwrap (topology.py `unwrap`) -> per chain and weight row X = sum_n w_n x_n.  The
// weights come from the caller in float64 (no cos on the device), so the engine serves any per-monomer weight set.
// Contract and summation order: mdx_rouse_device.hpp; this unit is compiled with contraction off and spells its
// float64 operations out.
//
// One pass over the positions at 12 B per atom-frame.  The amplitudes stay in HBM as double [frames][S][3], series
// series0[g] + k * n_chains[g] + c for group g, row k, chain c: all chains of a (group, row) are one contiguous range
// of a frame, which is what mdx_msd_push_device takes (mdx_rouse_device_result hands the buffer over).  Nothing is
// added with atomics and no sum is split across lanes, so the rows repeat bit for bit whatever route the frames
// take and however they are split into calls.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_internal.hpp"
#include "mdx_molecules.hpp"
#include "mdx_points_device.hpp"
#include "mdx_rouse_device.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_rouse_dev;
using mdx_prof_dev::prof_com_f64_kernel;
using mdx_prof_dev::prof_unwrap_scan_kernel;

namespace {

constexpr int64_t ROUSE_SLAB_FRAMES = 32768;                // frames per launch (grid y)
constexpr int64_t ROUSE_SCRATCH_BYTES = int64_t(256) << 20; // centres / image counts of one slab

// frames per slab of rouse_accumulate_rows: what its scratch of one frame allows; also what mdx_rouse_slab_frames
// reports
int64_t rouse_slab_frames(int64_t n_points, bool grouped, bool unwrap)
{
    const int64_t scratch = std::max<int64_t>(1, (grouped ? 24 * n_points : 0) + (unwrap ? 12 * n_points : 0));
    return std::min(ROUSE_SLAB_FRAMES, std::max<int64_t>(1, ROUSE_SCRATCH_BYTES / scratch));
}

}  // namespace

struct mdx_rouse : FrameEngine {
    int n_groups = 0;
    int64_t n_points = 0, n_series = 0, n_units = 0;
    int64_t row_capacity = 0;
    bool unwrap = false;
    double dims[3] = {0, 0, 0};
    std::vector<double> start;         // [n_points][3]: x_prev before the first frame
    DeviceBuffer d_units, d_weights, d_rows, d_centres, d_images, d_prev, d_image;
    MoleculeStage mol;                 // offsets / masses of the grouping; the centres are formed in float64 here

    int64_t rows_wanted() const { return mol.rows_wanted(n_points); }
    const char *rows_noun() const { return mol.rows_noun(); }
    void free_device()
    {
        release({&d_units, &d_weights, &d_rows, &d_centres, &d_images, &d_prev, &d_image});
        mol.recycle();
    }
};

static int rouse_grow_rows(mdx_rouse *h, int64_t more, bool exact = false)
{
    return grow_rows(h->d_rows, h->stream, int64_t(24) * h->n_series, h->frames_seen, more, &h->row_capacity, exact);
}

template <typename SRC>
static void rouse_launch(mdx_rouse *h, const SRC *pos, int64_t src_rows, const int *index, int64_t nf,
                         const int *images)
{
    hipLaunchKernelGGL((rouse_project_kernel<SRC>), dim3((unsigned)h->n_units, (unsigned)nf), dim3(ROUSE_THREADS), 0,
                       h->stream, pos, src_rows, index, (int)h->n_points, h->d_units.as<RouseUnit>(),
                       h->d_weights.as<double>(), images, h->dims[0], h->dims[1], h->dims[2], h->n_series,
                       h->d_rows.as<double>() + h->frames_seen * h->n_series * 3);
}

// image counts of nf frames of points (state carried in d_prev / d_image from call to call)
template <typename SRC>
static int rouse_scan(mdx_rouse *h, const SRC *pos, int64_t src_rows, const int *index, int64_t nf)
{
    const int n = (int)h->n_points;
    MDX_TRY(h->d_images.ensure(size_t(12) * n * nf));
    hipLaunchKernelGGL((prof_unwrap_scan_kernel<SRC>), dim3((unsigned)ceil_div(3 * int64_t(n), 256)), dim3(256), 0,
                       h->stream, pos, src_rows, index, n, (int)nf, h->dims[0] / 2, h->dims[1] / 2, h->dims[2] / 2, 0,
                       h->d_prev.as<double>(), h->d_image.as<int>(), h->d_images.as<int>());
    return MDX_OK;
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int rouse_accumulate_rows(mdx_rouse *h, const float *d_pos, int64_t src_rows, const int *d_index,
                                 int64_t n_rows, int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    const bool grouped = h->mol.active();
    const int64_t want = grouped ? h->mol.n_atoms : h->n_points;
    MDX_REQUIRE(n_rows == want, "%lld rows given, the groups%s hold %lld", (long long)n_rows,
                grouped ? " (rows of the grouping)" : "", (long long)want);
    MDX_TRY(rouse_grow_rows(h, n_frames));
    const int64_t n = h->n_points;
    if (h->unwrap && h->frames_seen == 0) {
        // before the first frame x_prev is the starting configuration and the image counts are 0
        MDX_HIP(hipMemcpyAsync(h->d_prev.ptr, h->start.data(), size_t(24) * n, hipMemcpyHostToDevice, h->stream));
        MDX_HIP(hipMemsetAsync(h->d_image.ptr, 0, size_t(12) * n, h->stream));
    }
    const int64_t slab = rouse_slab_frames(n, grouped, h->unwrap);
    hipEvent_t ev = h->timer.begin();
    for (int64_t f0 = 0; f0 < n_frames; f0 += slab) {
        const int64_t nf = std::min(slab, n_frames - f0);
        const float *pos = d_pos + f0 * src_rows * 3;
        const int *images = nullptr;
        if (grouped) {
            MDX_TRY(h->d_centres.ensure(size_t(24) * n * nf));
            hipLaunchKernelGGL(prof_com_f64_kernel, dim3((unsigned)ceil_div(3 * n, 256), (unsigned)nf), dim3(256), 0,
                               h->stream, pos, src_rows, d_index, h->mol.d_offsets.as<int64_t>(),
                               h->mol.d_masses.as<double>(), h->mol.d_total.as<double>(), n,
                               h->d_centres.as<double>());
            const double *centres = h->d_centres.as<double>();
            if (h->unwrap) {
                MDX_TRY(rouse_scan(h, centres, n, nullptr, nf));
                images = h->d_images.as<int>();
            }
            rouse_launch(h, centres, n, nullptr, nf, images);
        } else {
            if (h->unwrap) {
                MDX_TRY(rouse_scan(h, pos, src_rows, d_index, nf));
                images = h->d_images.as<int>();
            }
            rouse_launch(h, pos, src_rows, d_index, nf, images);
        }
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

extern "C" {

int mdx_rouse_create(mdx_rouse_t *out, int dev, int n_groups, const int64_t *n_chains, const int64_t *n_monomers,
                     int64_t n_rows, const double *weights)
{
    MDX_REQUIRE(out && n_chains && n_monomers && weights, "NULL argument");
    MDX_REQUIRE(n_groups >= 1 && n_groups <= 4096, "n_groups out of range");
    const int64_t limit = (int64_t(1) << 31) / 3;
    MDX_REQUIRE(n_rows >= 1 && n_rows < limit, "n_rows must be at least 1");
    int64_t n_points = 0, n_series = 0, n_weights = 0;
    for (int g = 0; g < n_groups; ++g) {
        MDX_REQUIRE(n_chains[g] >= 1 && n_chains[g] < limit, "group %d: n_chains must be at least 1", g);
        MDX_REQUIRE(n_monomers[g] >= 1 && n_monomers[g] < limit, "group %d: n_monomers must be at least 1", g);
        MDX_REQUIRE(n_chains[g] * n_monomers[g] < limit - n_points,
                    "the groups must hold fewer than 2^31 / 3 points");
        MDX_REQUIRE(n_rows * n_chains[g] < limit - n_series,
                    "the groups must give fewer than 2^31 / 3 series (n_rows * chains)");
        MDX_REQUIRE(n_rows * n_monomers[g] < limit, "group %d: n_rows * n_monomers must stay below 2^31 / 3", g);
        n_points += n_chains[g] * n_monomers[g];
        n_series += n_rows * n_chains[g];
        n_weights += n_rows * n_monomers[g];
    }
    for (int64_t i = 0; i < n_weights; ++i)
        MDX_REQUIRE(std::isfinite(weights[i]), "weights must be finite");
    // the units of the kernel and the weights transposed to wT[g][n][k]: lanes hold consecutive rows k
    std::vector<RouseUnit> units;
    std::vector<double> wT((size_t)n_weights);
    int64_t point = 0, series = 0, w0 = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int64_t M = n_chains[g], N = n_monomers[g];
        for (int64_t k = 0; k < n_rows; ++k)
            for (int64_t n = 0; n < N; ++n)
                wT[size_t(w0 + n * n_rows + k)] = weights[w0 + k * N + n];
        const int64_t per_unit = std::max<int64_t>(1, ROUSE_STAGE / N);
        for (int64_t c = 0; c < M; c += per_unit)
            units.push_back(RouseUnit{int(point + c * N), int(series), int(c), int(std::min(per_unit, M - c)), int(N),
                                      int(n_rows), int(M), 0, w0});
        point += M * N;
        series += n_rows * M;
        w0 += n_rows * N;
    }
    MDX_TRY(set_device(dev));
    mdx_rouse *h = new mdx_rouse();
    h->dev = dev;
    h->n_groups = n_groups;
    h->n_points = n_points;
    h->n_series = n_series;
    h->n_units = (int64_t)units.size();
    int rc = MDX_OK;
    do {
        if ((rc = stream_acquire(&h->stream)) != MDX_OK) break;
        h->timer.stream = h->stream;
        if ((rc = h->d_units.ensure(sizeof(RouseUnit) * units.size())) != MDX_OK) break;
        if ((rc = h->d_weights.ensure(size_t(8) * n_weights)) != MDX_OK) break;
        if (hipMemcpy(h->d_units.ptr, units.data(), sizeof(RouseUnit) * units.size(), hipMemcpyHostToDevice) !=
                hipSuccess ||
            hipMemcpy(h->d_weights.ptr, wT.data(), size_t(8) * n_weights, hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(MDX_ERR_HIP, "upload failed");
            break;
        }
    } while (0);
    if (rc != MDX_OK) {
        mdx_rouse_destroy(h);
        return rc;
    }
    *out = h;
    return MDX_OK;
}

int mdx_rouse_slab_frames(int64_t n_points, int grouped, int unwrap, int64_t *slab)
{
    MDX_REQUIRE(slab, "NULL argument");
    MDX_REQUIRE(n_points >= 1 && n_points < (int64_t(1) << 31) / 3,
                "the groups must hold between 1 and 2^31 / 3 points");
    *slab = rouse_slab_frames(n_points, grouped != 0, unwrap != 0);
    return MDX_OK;
}

int mdx_rouse_reserve(mdx_rouse_t h, int64_t n_frames)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_REQUIRE(n_frames >= 0, "bad size");
    MDX_TRY(set_device(h->dev));
    return rouse_grow_rows(h, n_frames - h->frames_seen, true);
}

int mdx_rouse_set_grouping(mdx_rouse_t h, int64_t n_molecules, const int64_t *offsets, const double *masses)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_REQUIRE(h->frames_seen == 0, "mdx_rouse_set_grouping must be called before the first frame");
    MDX_REQUIRE(n_molecules <= 0 || n_molecules == h->n_points, "%lld molecules given, the groups hold %lld points",
                (long long)n_molecules, (long long)h->n_points);
    MDX_REQUIRE(n_molecules <= 0 || (offsets && offsets[n_molecules] < (int64_t(1) << 31) / 3),
                "the grouping holds too many rows");
    return h->mol.set(n_molecules, offsets, masses);
}

int mdx_rouse_set_unwrap(mdx_rouse_t h, const double *dims, const double *start)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_REQUIRE(h->frames_seen == 0, "mdx_rouse_set_unwrap must be called before the first frame");
    if (!dims) {
        h->unwrap = false;
        return MDX_OK;
    }
    MDX_REQUIRE(start, "NULL argument");
    for (int k = 0; k < 3; ++k)
        MDX_REQUIRE(dims[k] > 0.0 && std::isfinite(dims[k]), "dims[%d] must be positive and finite", k);
    MDX_TRY(h->d_prev.ensure(size_t(24) * h->n_points));
    MDX_TRY(h->d_image.ensure(size_t(12) * h->n_points));
    h->start.assign(start, start + 3 * h->n_points);
    for (int k = 0; k < 3; ++k)
        h->dims[k] = dims[k];
    h->unwrap = true;
    return MDX_OK;
}

// what a route prepares before the first kernel
static int rouse_prepare(mdx_rouse *h, int64_t n_frames)
{
    MDX_TRY(set_device(h->dev));
    return rouse_grow_rows(h, n_frames);
}

int mdx_rouse_result(mdx_rouse_t h, double *out)
{
    MDX_REQUIRE(h && out, "NULL argument");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    h->timer.collect();
    if (h->frames_seen == 0)
        return MDX_OK;
    MDX_HIP(hipMemcpy(out, h->d_rows.ptr, size_t(24) * h->n_series * h->frames_seen, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_rouse_device_result(mdx_rouse_t h, const double **d_ptr, int64_t *n_frames, int64_t *n_series)
{
    MDX_REQUIRE(h && d_ptr, "NULL argument");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    h->timer.collect();
    *d_ptr = h->d_rows.as<double>();
    if (n_frames) *n_frames = h->frames_seen;
    if (n_series) *n_series = h->n_series;
    return MDX_OK;
}

int mdx_rouse_stats(mdx_rouse_t h, int64_t *launches, double *kernel_ms, int64_t *frames)
{
    MDX_REQUIRE(h, "NULL handle");
    return h->stats(true, launches, kernel_ms, frames);
}

}  // extern "C"

MDX_FRAME_ROUTES(rouse, rouse_prepare, rouse_accumulate_rows)
MDX_FRAME_LIFE_CYCLE(rouse)
MDX_FRAME_RESET(rouse)
