// mdx_gyration.hip — per-chain radii of gyration on gfx950 (MI355X).
//
// Carries Gyradius._single_frame (reference src/mdhelper/analysis/polymer.py:439-465): positions (atoms, or the
// float64 centres of mass of monomers) -> optional global unwrap (topology.py `unwrap`) -> per chain the centre of
// mass and the mass-weighted second moments about it (algorithm/molecule.py radius_of_gyration) -> square roots ->
// mean over the chains of a group.  Contract and summation orders: mdx_gyration_device.hpp; this unit is compiled
// with contraction off and spells its float64 operations out.
//
// One pass over the positions at 12 B per atom-frame: a wave takes a chain (several short ones), keeps its points in
// registers between the centre and the moments, and folds across lanes by shuffles.  The per-chain values of a slab
// of frames go to a scratch array that a second, small kernel averages per (frame, group).  Nothing is added with
// atomics, so the rows repeat bit for bit whatever route the frames take and however they are split into calls.
#include "mdx_common.hpp"
#include "mdx_frame_entry.hpp"
#include "mdx_gyration_device.hpp"
#include "mdx_internal.hpp"
#include "mdx_molecules.hpp"
#include "mdx_points_device.hpp"

#include <algorithm>
#include <cmath>

using namespace mdx;
using namespace mdx_gyr_dev;
using mdx_prof_dev::prof_com_f64_kernel;
using mdx_prof_dev::prof_unwrap_scan_kernel;

namespace {

constexpr int64_t GYR_SLAB_FRAMES = 32768;                // frames per launch (grid y)
constexpr int64_t GYR_SCRATCH_BYTES = int64_t(256) << 20; // centres / image counts / per-chain values of one slab

// frames per slab of gyr_accumulate_rows: what its scratch of one frame allows; also what mdx_gyr_slab_frames reports
int64_t gyr_slab_frames(int64_t n_chains, int64_t n_points, bool grouped, bool unwrap)
{
    const int64_t scratch = 32 * n_chains + (grouped ? 24 * n_points : 0) + (unwrap ? 12 * n_points : 0);
    return std::min(GYR_SLAB_FRAMES, std::max<int64_t>(1, GYR_SCRATCH_BYTES / scratch));
}

}  // namespace

struct mdx_gyr : FrameEngine {
    int n_groups = 0;
    int64_t n_points = 0, n_chains = 0, n_units = 0;
    int64_t row_capacity = 0;
    bool unwrap = false;
    double dims[3] = {0, 0, 0};
    std::vector<double> start;         // [n_points][3]: x_prev before the first frame
    DeviceBuffer d_units, d_masses, d_chain_mass, d_chain_offsets, d_rows, d_chain_out, d_centres, d_images, d_prev,
        d_image;
    MoleculeStage mol;                 // offsets / masses of the grouping; the centres are formed in float64 here

    int64_t rows_wanted() const { return mol.rows_wanted(n_points); }
    const char *rows_noun() const { return mol.rows_noun(); }
    void free_device()
    {
        release({&d_units, &d_masses, &d_chain_mass, &d_chain_offsets, &d_rows, &d_chain_out, &d_centres, &d_images,
                 &d_prev, &d_image});
        mol.recycle();
    }
};

static int gyr_grow_rows(mdx_gyr *h, int64_t more)
{
    return grow_rows(h->d_rows, h->stream, int64_t(32) * h->n_groups, h->frames_seen, more, &h->row_capacity);
}

template <typename SRC>
static void gyr_launch(mdx_gyr *h, const SRC *pos, int64_t src_rows, const int *index, int64_t nf, const int *images)
{
    hipLaunchKernelGGL((gyr_moments_kernel<SRC>), dim3((unsigned)ceil_div(h->n_units, GYR_WAVES), (unsigned)nf),
                       dim3(GYR_THREADS), 0, h->stream, pos, src_rows, index, (int)h->n_points,
                       h->d_units.as<GyrUnit>(), (int)h->n_units, (int)h->n_chains, h->d_masses.as<double>(),
                       h->d_chain_mass.as<double>(), images, h->dims[0], h->dims[1], h->dims[2],
                       h->d_chain_out.as<double>());
    hipLaunchKernelGGL(gyr_mean_kernel, dim3((unsigned)h->n_groups, (unsigned)nf), dim3(64), 0, h->stream,
                       h->d_chain_out.as<double>(), (int)h->n_chains, h->d_chain_offsets.as<int>(), h->n_groups,
                       h->d_rows.as<double>() + h->frames_seen * h->n_groups * 4);
}

// image counts of nf frames of points (state carried in d_prev / d_image from call to call)
template <typename SRC>
static int gyr_scan(mdx_gyr *h, const SRC *pos, int64_t src_rows, const int *index, int64_t nf)
{
    const int n = (int)h->n_points;
    MDX_TRY(h->d_images.ensure(size_t(12) * n * nf));
    hipLaunchKernelGGL((prof_unwrap_scan_kernel<SRC>), dim3((unsigned)ceil_div(3 * int64_t(n), 256)), dim3(256), 0,
                       h->stream, pos, src_rows, index, n, (int)nf, h->dims[0] / 2, h->dims[1] / 2, h->dims[2] / 2, 0,
                       h->d_prev.as<double>(), h->d_image.as<int>(), h->d_images.as<int>());
    return MDX_OK;
}

// n_frames frames of float32 rows in HBM: row index[i] (or i) of a frame of src_rows rows is incoming row i
static int gyr_accumulate_rows(mdx_gyr *h, const float *d_pos, int64_t src_rows, const int *d_index, int64_t n_rows,
                               int64_t n_frames)
{
    if (n_frames == 0)
        return MDX_OK;
    const bool grouped = h->mol.active();
    const int64_t want = grouped ? h->mol.n_atoms : h->n_points;
    MDX_REQUIRE(n_rows == want, "%lld rows given, the groups%s hold %lld", (long long)n_rows,
                grouped ? " (rows of the grouping)" : "", (long long)want);
    MDX_TRY(gyr_grow_rows(h, n_frames));
    const int64_t n = h->n_points;
    if (h->unwrap && h->frames_seen == 0) {
        // before the first frame x_prev is the starting configuration and the image counts are 0
        MDX_HIP(hipMemcpyAsync(h->d_prev.ptr, h->start.data(), size_t(24) * n, hipMemcpyHostToDevice, h->stream));
        MDX_HIP(hipMemsetAsync(h->d_image.ptr, 0, size_t(12) * n, h->stream));
    }
    const int64_t slab = gyr_slab_frames(h->n_chains, n, grouped, h->unwrap);
    hipEvent_t ev = h->timer.begin();
    for (int64_t f0 = 0; f0 < n_frames; f0 += slab) {
        const int64_t nf = std::min(slab, n_frames - f0);
        const float *pos = d_pos + f0 * src_rows * 3;
        MDX_TRY(h->d_chain_out.ensure(size_t(32) * h->n_chains * nf));
        const int *images = nullptr;
        if (grouped) {
            MDX_TRY(h->d_centres.ensure(size_t(24) * n * nf));
            hipLaunchKernelGGL(prof_com_f64_kernel, dim3((unsigned)ceil_div(3 * n, 256), (unsigned)nf), dim3(256), 0,
                               h->stream, pos, src_rows, d_index, h->mol.d_offsets.as<int64_t>(),
                               h->mol.d_masses.as<double>(), h->mol.d_total.as<double>(), n,
                               h->d_centres.as<double>());
            const double *centres = h->d_centres.as<double>();
            if (h->unwrap) {
                MDX_TRY(gyr_scan(h, centres, n, nullptr, nf));
                images = h->d_images.as<int>();
            }
            gyr_launch(h, centres, n, nullptr, nf, images);
        } else {
            if (h->unwrap) {
                MDX_TRY(gyr_scan(h, pos, src_rows, d_index, nf));
                images = h->d_images.as<int>();
            }
            gyr_launch(h, pos, src_rows, d_index, nf, images);
        }
        h->frames_seen += nf;
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

extern "C" {

int mdx_gyr_create(mdx_gyr_t *out, int dev, int n_groups, const int64_t *n_chains, const int64_t *n_monomers,
                   const double *masses)
{
    MDX_REQUIRE(out && n_chains && n_monomers && masses, "NULL argument");
    MDX_REQUIRE(n_groups >= 1 && n_groups <= 4096, "n_groups out of range");
    const int64_t limit = (int64_t(1) << 31) / 3;
    int64_t n_points = 0, chains = 0;
    for (int g = 0; g < n_groups; ++g) {
        MDX_REQUIRE(n_chains[g] >= 1 && n_chains[g] < limit, "group %d: n_chains must be at least 1", g);
        MDX_REQUIRE(n_monomers[g] >= 1 && n_monomers[g] < limit, "group %d: n_monomers must be at least 1", g);
        MDX_REQUIRE(n_chains[g] * n_monomers[g] < limit - n_points,
                    "the groups must hold fewer than 2^31 / 3 points");
        n_points += n_chains[g] * n_monomers[g];
        chains += n_chains[g];
    }
    // the units of the moment kernel, the chains' masses (sequential sums) and the groups' chain ranges
    std::vector<GyrUnit> units;
    std::vector<double> chain_mass;
    std::vector<int32_t> chain_offsets{0};
    chain_mass.reserve((size_t)chains);
    int64_t point = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int64_t M = n_chains[g], N = n_monomers[g];
        int shift = 6;
        if (N <= 32)
            for (shift = 0; (int64_t(1) << shift) < N; ++shift) {}
        const int64_t per_unit = int64_t(64) >> shift;
        for (int64_t c = 0; c < M; ++c) {
            double m = 0.0;
            for (int64_t j = 0; j < N; ++j) {
                const double mj = masses[point + c * N + j];
                MDX_REQUIRE(mj >= 0.0 && std::isfinite(mj), "masses must be finite and not negative");
                m += mj;
            }
            MDX_REQUIRE(m > 0.0, "chain %lld of group %d has no mass", (long long)c, g);
            chain_mass.push_back(m);
        }
        for (int64_t c = 0; c < M; c += per_unit)
            units.push_back(GyrUnit{int(point + c * N), int(chain_offsets.back() + c),
                                    int(std::min(per_unit, M - c)), int(N), shift, {0, 0, 0}});
        point += M * N;
        chain_offsets.push_back(int32_t(chain_offsets.back() + M));
    }
    MDX_TRY(set_device(dev));
    mdx_gyr *h = new mdx_gyr();
    h->dev = dev;
    h->n_groups = n_groups;
    h->n_points = n_points;
    h->n_chains = chains;
    h->n_units = (int64_t)units.size();
    int rc = MDX_OK;
    do {
        if ((rc = stream_acquire(&h->stream)) != MDX_OK) break;
        h->timer.stream = h->stream;
        if ((rc = h->d_units.ensure(sizeof(GyrUnit) * units.size())) != MDX_OK) break;
        if ((rc = h->d_masses.ensure(size_t(8) * n_points)) != MDX_OK) break;
        if ((rc = h->d_chain_mass.ensure(size_t(8) * chains)) != MDX_OK) break;
        if ((rc = h->d_chain_offsets.ensure(size_t(4) * (n_groups + 1))) != MDX_OK) break;
        if (hipMemcpy(h->d_units.ptr, units.data(), sizeof(GyrUnit) * units.size(), hipMemcpyHostToDevice) !=
                hipSuccess ||
            hipMemcpy(h->d_masses.ptr, masses, size_t(8) * n_points, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_chain_mass.ptr, chain_mass.data(), size_t(8) * chains, hipMemcpyHostToDevice) !=
                hipSuccess ||
            hipMemcpy(h->d_chain_offsets.ptr, chain_offsets.data(), size_t(4) * (n_groups + 1),
                      hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(MDX_ERR_HIP, "upload failed");
            break;
        }
    } while (0);
    if (rc != MDX_OK) {
        mdx_gyr_destroy(h);
        return rc;
    }
    *out = h;
    return MDX_OK;
}

int mdx_gyr_slab_frames(int64_t n_chains, int64_t n_points, int grouped, int unwrap, int64_t *slab)
{
    MDX_REQUIRE(slab, "NULL argument");
    const int64_t limit = (int64_t(1) << 31) / 3;
    MDX_REQUIRE(n_chains >= 1 && n_points >= n_chains && n_points < limit,
                "the groups must hold at least one point per chain and fewer than 2^31 / 3 points");
    *slab = gyr_slab_frames(n_chains, n_points, grouped != 0, unwrap != 0);
    return MDX_OK;
}

int mdx_gyr_set_grouping(mdx_gyr_t h, int64_t n_molecules, const int64_t *offsets, const double *masses)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_REQUIRE(h->frames_seen == 0, "mdx_gyr_set_grouping must be called before the first frame");
    MDX_REQUIRE(n_molecules <= 0 || n_molecules == h->n_points, "%lld molecules given, the groups hold %lld points",
                (long long)n_molecules, (long long)h->n_points);
    MDX_REQUIRE(n_molecules <= 0 || (offsets && offsets[n_molecules] < (int64_t(1) << 31) / 3),
                "the grouping holds too many rows");
    return h->mol.set(n_molecules, offsets, masses);
}

int mdx_gyr_set_unwrap(mdx_gyr_t h, const double *dims, const double *start)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_REQUIRE(h->frames_seen == 0, "mdx_gyr_set_unwrap must be called before the first frame");
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
static int gyr_prepare(mdx_gyr *h, int64_t n_frames)
{
    MDX_TRY(set_device(h->dev));
    return gyr_grow_rows(h, n_frames);
}

int mdx_gyr_result(mdx_gyr_t h, double *out)
{
    MDX_REQUIRE(h && out, "NULL argument");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    h->timer.collect();
    const int64_t F = h->frames_seen, G = h->n_groups;
    if (F == 0)
        return MDX_OK;
    std::vector<double> rows(size_t(F * G * 4));
    MDX_HIP(hipMemcpy(rows.data(), h->d_rows.ptr, size_t(32) * F * G, hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < G; ++g)
        for (int64_t f = 0; f < F; ++f)
            for (int k = 0; k < 4; ++k)
                out[(g * F + f) * 4 + k] = rows[size_t((f * G + g) * 4 + k)];
    return MDX_OK;
}

int mdx_gyr_stats(mdx_gyr_t h, int64_t *launches, double *kernel_ms, int64_t *frames)
{
    MDX_REQUIRE(h, "NULL handle");
    return h->stats(true, launches, kernel_ms, frames);
}

}  // extern "C"

MDX_FRAME_ROUTES(gyr, gyr_prepare, gyr_accumulate_rows)
MDX_FRAME_LIFE_CYCLE(gyr)
MDX_FRAME_RESET(gyr)
