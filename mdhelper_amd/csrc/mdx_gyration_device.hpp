// mdx_gyration_device.hpp — device side of the gyration engine (mdx_gyration.hip).
//
// Result contract (reference src/mdhelper/algorithm/molecule.py:529-564 as analysis/polymer.py Gyradius calls it
// per frame, then .mean(axis=0) over the chains), everything in float64 with separate multiply and add; float32
// coordinates are widened before any arithmetic:
//
//     x      = (double)r + image * L                          (image = 0 without unwrap)
//     c_d    = (sum_j m_j x_jd) / M,   M = sum_j m_j          (pass 1)
//     S_d    = sum_j m_j * ((x_jd - c_d) * (x_jd - c_d))      (pass 2, over the centred coordinates)
//     Rg     = sqrt(((S_x + S_y) + S_z) / M)
//     Rg_x   = sqrt((S_y + S_z) / M),  Rg_y = sqrt((S_x + S_z) / M),  Rg_z = sqrt((S_x + S_y) / M)
//     out    = (sum over the group's chains) / n_chains
//
// Every sum has a fixed order.  Over a chain: lane l of the chain's W lanes (W = 64, or the power of two >= the
// chain length for chains of <= 32 points, which share a wave) adds its points l, l + 64, l + 128, ... in that
// order, then the W partial sums fold in an xor butterfly (offsets W/2 ... 1; a + b == b + a, so every lane ends
// with the same bits).  Over the chains of a group: lane l of one wave adds chains l, l + 64, ... in that order,
// then the same butterfly.  No floating-point atomics.  The one-pass form sum m x^2 - (sum m x)^2 / M is not used:
// it cancels for chains far from the origin.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mdx_points_device.hpp"

namespace mdx_gyr_dev {

constexpr int GYR_THREADS = 256;
constexpr int GYR_WAVES = GYR_THREADS / 64;
constexpr int GYR_HOLD = 4;          // 64-point strides of a chain kept in registers between the two passes

// What one wave works on: n_chains consecutive chains of one group, each of n_monomers points on 1 << shift lanes.
struct GyrUnit {
    int point0;       // first point of the first chain
    int chain0;       // its number among all chains of the engine
    int n_chains;     // 1 ... 64 >> shift
    int n_monomers;   // <= 1 << shift unless shift == 6
    int shift;
    int pad[3];
};

// sum over the 1 << shift lanes of a lane's sub-group, the same bits in every lane of it
__device__ __forceinline__ double gyr_fold(double v, int shift)
{
    for (int off = (1 << shift) >> 1; off > 0; off >>= 1)
        v = __dadd_rn(v, __shfl_xor(v, off, 64));
    return v;
}

// the widened point of a frame (mdx_points_device.hpp), shared with the projection engine
template <typename SRC> using GyrSource = mdx_prof_dev::PointSource<SRC>;

// chain_out[frame][chain][4] = Rg, Rg_x, Rg_y, Rg_z of every chain.  Grid: x = units in fours (one per wave),
// y = frames.  The frame is read once from HBM: the first GYR_HOLD strides of a chain stay in registers between
// the passes, longer chains read the rest a second time (from L2).
template <typename SRC>
__global__ __launch_bounds__(GYR_THREADS) void gyr_moments_kernel(
    const SRC *__restrict__ pos, int64_t src_rows, const int *__restrict__ index, int n_points,
    const GyrUnit *__restrict__ units, int n_units, int n_chains_total, const double *__restrict__ masses,
    const double *__restrict__ chain_mass, const int *__restrict__ images, double Lx, double Ly, double Lz,
    double *__restrict__ chain_out)
{
    const int u = blockIdx.x * GYR_WAVES + (threadIdx.x >> 6);
    if (u >= n_units)       // whole waves leave together
        return;
    const int64_t f = blockIdx.y;
    const GyrUnit unit = units[u];
    const int lane = threadIdx.x & 63;
    const int sub = lane >> unit.shift, j0 = lane & ((1 << unit.shift) - 1);
    const bool live = sub < unit.n_chains;
    const int np = live ? unit.n_monomers : 0;
    const int base = unit.point0 + sub * unit.n_monomers;
    const GyrSource<SRC> src{pos + f * src_rows * 3, index, images ? images + f * 3 * int64_t(n_points) : nullptr,
                             {Lx, Ly, Lz}};

    double hx[GYR_HOLD][3], hm[GYR_HOLD];
    double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int h = 0; h < GYR_HOLD; ++h) {
        const int j = j0 + 64 * h;
        hm[h] = 0.0;
        hx[h][0] = hx[h][1] = hx[h][2] = 0.0;
        if (j < np) {
            hm[h] = masses[base + j];
            src.load(base + j, hx[h]);
        }
        s[0] = __dadd_rn(s[0], __dmul_rn(hm[h], hx[h][0]));
        s[1] = __dadd_rn(s[1], __dmul_rn(hm[h], hx[h][1]));
        s[2] = __dadd_rn(s[2], __dmul_rn(hm[h], hx[h][2]));
    }
    for (int j = j0 + 64 * GYR_HOLD; j < np; j += 64) {
        double x[3];
        const double m = masses[base + j];
        src.load(base + j, x);
        s[0] = __dadd_rn(s[0], __dmul_rn(m, x[0]));
        s[1] = __dadd_rn(s[1], __dmul_rn(m, x[1]));
        s[2] = __dadd_rn(s[2], __dmul_rn(m, x[2]));
    }
    const double M = live ? chain_mass[unit.chain0 + sub] : 1.0;
    double c[3];
#pragma unroll
    for (int d = 0; d < 3; ++d)
        c[d] = __ddiv_rn(gyr_fold(s[d], unit.shift), M);

    double S[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int h = 0; h < GYR_HOLD; ++h)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double e = __dsub_rn(hx[h][d], c[d]);      // hm == 0 where the lane holds no point
            S[d] = __dadd_rn(S[d], __dmul_rn(hm[h], __dmul_rn(e, e)));
        }
    for (int j = j0 + 64 * GYR_HOLD; j < np; j += 64) {
        double x[3];
        const double m = masses[base + j];
        src.load(base + j, x);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double e = __dsub_rn(x[d], c[d]);
            S[d] = __dadd_rn(S[d], __dmul_rn(m, __dmul_rn(e, e)));
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d)
        S[d] = gyr_fold(S[d], unit.shift);
    if (live && j0 == 0) {
        double *o = chain_out + (f * n_chains_total + unit.chain0 + sub) * 4;
        o[0] = sqrt(__ddiv_rn(__dadd_rn(__dadd_rn(S[0], S[1]), S[2]), M));
        o[1] = sqrt(__ddiv_rn(__dadd_rn(S[1], S[2]), M));
        o[2] = sqrt(__ddiv_rn(__dadd_rn(S[0], S[2]), M));
        o[3] = sqrt(__ddiv_rn(__dadd_rn(S[0], S[1]), M));
    }
}

// rows[frame][group][4] = mean over the group's chains [chain_offsets[g], chain_offsets[g + 1]).  One wave per
// (frame, group): grid x = groups, y = frames, 64 threads.
__global__ __launch_bounds__(64) void gyr_mean_kernel(const double *__restrict__ chain_out, int n_chains_total,
                                                      const int *__restrict__ chain_offsets, int n_groups,
                                                      double *__restrict__ rows)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    const int64_t f = blockIdx.y;
    const int lo = chain_offsets[g], hi = chain_offsets[g + 1];
    const double *__restrict__ in = chain_out + f * n_chains_total * 4;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = lo + lane; c < hi; c += 64)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            a[k] = __dadd_rn(a[k], in[int64_t(c) * 4 + k]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        a[k] = gyr_fold(a[k], 6);
    if (lane < 4)
        rows[(f * n_groups + g) * 4 + lane] = __ddiv_rn(lane == 0 ? a[0] : lane == 1 ? a[1] : lane == 2 ? a[2] : a[3],
                                                        (double)(hi - lo));
}

}  // namespace mdx_gyr_dev
