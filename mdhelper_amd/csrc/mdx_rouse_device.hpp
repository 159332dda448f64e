// mdx_rouse_device.hpp — device side of the chain-projection engine (mdx_rouse.hip).
//
// Result contract, everything in float64 with separate multiply and add; float32 coordinates are widened before any
// arithmetic:
//
//     x_n      = (double)r_n + image_n * L                       (image = 0 without unwrap)
//     X[c][k]  = sum_n w[g][k][n] * x_n                          over the monomers n of chain c, k = 0 ... K-1
//
// Summation order: one lane owns one (chain, weight row) and adds the products w_n * x_n one after the other,
// n = 0, 1, ..., N-1, starting from +0.0 — the order of a plain host loop, so the host restatement reproduces the bits.
// No sum is split across lanes: there is no fold, no floating-point atomic, and the result cannot depend on the route
// the frames take or on how they are split into calls.
//
// Work layout.  A workgroup of 256 threads takes a unit — consecutive chains of one group that hold at most
// ROUSE_STAGE points together, or one longer chain — of one frame.  Its threads widen the unit's points once into
// LDS (structure of arrays, 12 B read per point from HBM), then thread t takes the (chain, row) pair number t: lanes
// next to each other hold consecutive rows of one chain, so the point is an LDS broadcast and the weights, stored
// transposed as wT[n][k], one coalesced read per step.  Pairs beyond 256 go in further tiles of 256 over the same
// staged points, which bounds the accumulators at three per lane whatever K is.  A chain longer than ROUSE_STAGE is
// staged chunk by chunk inside every row tile: the first tile reads it from HBM, the others (K > 256 only) from L2.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), float and double source alike: 32 VGPRs, no
// AGPRs, 60 SGPRs, no scratch; 24 KiB of LDS per workgroup (3 * ROUSE_STAGE doubles), so six workgroups (24 waves,
// 6 per SIMD) fit the 160 KiB of a CU and LDS, not the register file, bounds the occupancy.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mdx_points_device.hpp"

namespace mdx_rouse_dev {

constexpr int ROUSE_THREADS = 256;
constexpr int ROUSE_STAGE = 1024;    // points of a unit staged in LDS at a time

// What one workgroup works on: n_chains consecutive chains of one group, n_chains * n_monomers <= ROUSE_STAGE unless
// n_chains == 1.
struct RouseUnit {
    int point0;         // first point of the first chain
    int series0;        // first output series of the group
    int chain0;         // the first chain's number within the group
    int n_chains;
    int n_monomers;
    int n_rows;         // K
    int group_chains;   // chains of the group: series = series0 + k * group_chains + chain
    int pad;
    int64_t weight0;    // wT[n][k] of the group starts here
};

// out[frame][series][3].  Grid: x = units, y = frames.
template <typename SRC>
__global__ __launch_bounds__(ROUSE_THREADS) void rouse_project_kernel(
    const SRC *__restrict__ pos, int64_t src_rows, const int *__restrict__ index, int n_points,
    const RouseUnit *__restrict__ units, const double *__restrict__ weights, const int *__restrict__ images,
    double Lx, double Ly, double Lz, int64_t n_series, double *__restrict__ out)
{
    __shared__ double sx[3][ROUSE_STAGE];
    const RouseUnit unit = units[blockIdx.x];
    const int64_t f = blockIdx.y;
    const mdx_prof_dev::PointSource<SRC> src{pos + f * src_rows * 3, index,
                                             images ? images + f * 3 * int64_t(n_points) : nullptr, {Lx, Ly, Lz}};
    const int N = unit.n_monomers, K = unit.n_rows;
    const int span = unit.n_chains * N;             // > ROUSE_STAGE only for one long chain
    const int n_pairs = unit.n_chains * K;
    const bool once = span <= ROUSE_STAGE;          // one chunk: staged for the first row tile, kept for the others
    double *__restrict__ o = out + f * n_series * 3;

    for (int t0 = 0; t0 < n_pairs; t0 += ROUSE_THREADS) {
        const int pair = t0 + (int)threadIdx.x;
        const bool live = pair < n_pairs;
        const int c = live ? pair / K : 0;
        const int k = live ? pair - c * K : 0;
        double a[3] = {0.0, 0.0, 0.0};
        for (int p0 = 0; p0 < span; p0 += ROUSE_STAGE) {
            const int np = min(ROUSE_STAGE, span - p0);
            if (!once || t0 == 0) {                 // uniform over the workgroup
                __syncthreads();                    // the chunk before has been read
                for (int q = threadIdx.x; q < np; q += ROUSE_THREADS) {
                    double x[3];
                    src.load(unit.point0 + p0 + q, x);
                    sx[0][q] = x[0];
                    sx[1][q] = x[1];
                    sx[2][q] = x[2];
                }
                __syncthreads();
            }
            if (live) {
                // the chain's points inside this chunk, as positions within the unit
                const int lo = max(c * N, p0), hi = min(c * N + N, p0 + np);
                const double *__restrict__ w = weights + unit.weight0 + int64_t(lo - c * N) * K + k;
                for (int q = lo; q < hi; ++q, w += K) {
                    const double wn = *w;
                    a[0] = __dadd_rn(a[0], __dmul_rn(wn, sx[0][q - p0]));
                    a[1] = __dadd_rn(a[1], __dmul_rn(wn, sx[1][q - p0]));
                    a[2] = __dadd_rn(a[2], __dmul_rn(wn, sx[2][q - p0]));
                }
            }
        }
        if (live) {
            double *__restrict__ dst =
                o + (int64_t(unit.series0) + int64_t(k) * unit.group_chains + unit.chain0 + c) * 3;
            dst[0] = a[0];
            dst[1] = a[1];
            dst[2] = a[2];
        }
    }
}

}  // namespace mdx_rouse_dev
