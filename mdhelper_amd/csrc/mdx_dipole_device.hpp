// mdx_dipole_device.hpp — device side of the dipole-moment engine (mdx_dipole.hip).
//
// Result contract (reference src/mdhelper/analysis/electrostatics.py DipoleMoment, M = sum_i q_i z_i): per analysed
// frame f, group g and component d, in float64 with separate multiply and add; float32 coordinates are widened before
// any arithmetic:
//
//     x_id    = (double)r_id + image_id * L_d                  (image = 0 without unwrap)
//     M_gd(f) = sum over the points i of group g of  q_i * x_id
//
// image follows the reference's global unwrap (algorithm/topology.py `unwrap`, the rule of prof_unwrap_scan_kernel):
// d = x_raw(f) - x_raw(f - 1) in float64, and |d| >= L_d / 2 moves the count by -sign(d).  Before the first frame
// x_raw is the engine's `start` array (float64, which is why the carried `prev` is float64 too: from the second
// frame on it holds a widened float32) and the counts are 0.
//
// Summation order.  It depends on the group sizes alone, not on the route the frames take, on how they are split
// into calls or slabs, or on the grid.  A group of n points is cut into ceil(n / DIP_TILE) tiles of DIP_TILE
// consecutive points (the last one shorter); a tile never spans two groups.  With term(j) = q_j * x_j of the j-th
// point of a tile (points past the end of the tile contribute no term):
//
//     lane sum   p_l  = (0 + term(l)) + term(l + 64) + ... + term(l + 64 (DIP_LANE_POINTS - 1)),   l = 0 ... 63
//     tile sum   t    = (((0 + p_0) + p_1) + ...) + p_63                       (one lane adds the 64 in lane order)
//     group sum  M    = (((0 + t_0) + t_1) + ...) + t_last                     (the group's tiles in tile order)
//
// No floating-point atomics, no cross-lane tree: the 64 lane sums of a frame go through LDS, and lane r of the wave
// adds row r (one frame and component of a batch of frames) sequentially, so the fold costs one LDS write per lane,
// frame and component plus 64 reads and adds per batch instead of an 18-step float64 butterfly per frame.
//
// Traffic.  The positions are read once, 12 B per point and frame.  Nothing of size frames x points is written:
// the scan and the sum are fused, a lane owns its DIP_LANE_POINTS points for the whole slab, keeps prev and image in
// registers and walks the slab's frames; what goes to memory is 24 B per tile and frame (partial) and the state of
// the scan once per slab.  Without unwrap the frames of a slab spread over grid y as well.  With unwrap only the
// points give parallelism: three waves per DIP_TILE points (one per component), so a system of 32 768 points runs on
// 768 waves, fewer than the device has SIMDs, and small systems use few blocks; each wave then walks every frame of
// the slab, which is why that kernel keeps DIP_BATCH_SCAN frames of loads in flight.  Measured numbers: DESIGN.md.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mdx_dip_dev {

constexpr int DIP_LANE_POINTS = 2;                  // points a lane owns
constexpr int DIP_TILE = 64 * DIP_LANE_POINTS;      // points per tile = per wave
constexpr int DIP_BATCH = 8;                        // frames loaded ahead and folded through LDS together
constexpr int DIP_BATCH_SCAN = 32;                  // the same with unwrap: few waves, so each keeps more loads in flight
constexpr int DIP_BLOCK_FRAMES = 4 * DIP_BATCH;     // frames per block along grid y (without unwrap)
constexpr int DIP_ROW = 65;                         // padded LDS row: lanes r read rows r without bank conflicts

struct DipTile {
    int point0;     // first point, in concatenated-group order
    int count;      // 1 ... DIP_TILE
};

// partial[frame][tile][3] for frames [blockIdx.y * frames_per_block, ...) of the n_frames at pos.  Grid: x = tiles,
// y = runs of frames_per_block frames (UNWRAP: y = 1 and frames_per_block >= n_frames, the scan is sequential).
// A block is SPLIT waves, each with the tile's points on its lanes and 3 / SPLIT of the components: one wave does all
// three without unwrap (one 12-byte load per point); with unwrap, where the waves are few and the scan is a long
// dependent chain per coordinate, three waves take a component each (the same sums in the same order: a sum never
// mixes components).  prev / image: the scan's state, read at the start and written back at the end (UNWRAP only).
template <bool UNWRAP>
__global__ __launch_bounds__(UNWRAP ? 192 : 64) void dip_tile_kernel(
    const float *__restrict__ pos, int64_t src_rows, const int *__restrict__ index, const DipTile *__restrict__ tiles,
    int n_tiles, const double *__restrict__ charges, int n_frames, int frames_per_block, double Lx, double Ly,
    double Lz, double *__restrict__ prev, int *__restrict__ image, double *__restrict__ partial)
{
    constexpr int SPLIT = UNWRAP ? 3 : 1, D = 3 / SPLIT, BATCH = UNWRAP ? DIP_BATCH_SCAN : DIP_BATCH;
    __shared__ double fold[BATCH * 3][DIP_ROW];
    const int lane = threadIdx.x & 63;
    const int d0 = (threadIdx.x >> 6) * D;          // first component of this wave
    const int t = blockIdx.x;
    const DipTile tile = tiles[t];
    const int f_lo = blockIdx.y * frames_per_block;
    const int f_hi = min(n_frames, f_lo + frames_per_block);
    double L[D], half[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        L[d] = d0 + d == 0 ? Lx : d0 + d == 1 ? Ly : Lz;
        half[d] = L[d] / 2;
    }

    bool live[DIP_LANE_POINTS];
    int64_t row[DIP_LANE_POINTS];       // first float of this wave's components of the point within a frame
    double q[DIP_LANE_POINTS];
    double old[DIP_LANE_POINTS][D];
    int im[DIP_LANE_POINTS][D];
#pragma unroll
    for (int k = 0; k < DIP_LANE_POINTS; ++k) {
        const int j = lane + 64 * k;
        live[k] = j < tile.count;
        const int p = tile.point0 + (live[k] ? j : 0);      // lanes without a point read the tile's first one
        row[k] = int64_t(index ? index[p] : p) * 3 + d0;
        q[k] = charges[p];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            old[k][d] = UNWRAP ? prev[int64_t(p) * 3 + d0 + d] : 0.0;
            im[k][d] = UNWRAP ? image[int64_t(p) * 3 + d0 + d] : 0;
        }
    }

    // the loads of a whole batch are issued one batch ahead of its arithmetic: their addresses do not depend on the scan
    float raw[BATCH][DIP_LANE_POINTS][D], next[BATCH][DIP_LANE_POINTS][D];
    const auto load = [&](float (&into)[BATCH][DIP_LANE_POINTS][D], int f0) {
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            const int f = min(f0 + b, f_hi - 1);
            const float *__restrict__ frame = pos + int64_t(f) * src_rows * 3;
#pragma unroll
            for (int k = 0; k < DIP_LANE_POINTS; ++k)
#pragma unroll
                for (int d = 0; d < D; ++d)
                    into[b][k][d] = frame[row[k] + d];
        }
    };
    load(next, f_lo);
    for (int f0 = f_lo; f0 < f_hi; f0 += BATCH) {
#pragma unroll
        for (int b = 0; b < BATCH; ++b)
#pragma unroll
            for (int k = 0; k < DIP_LANE_POINTS; ++k)
#pragma unroll
                for (int d = 0; d < D; ++d)
                    raw[b][k][d] = next[b][k][d];
        load(next, f0 + BATCH);     // past the end: the last frame again, unused
        // no branch on the frame number, so that the loads above stay ahead of the arithmetic: past the last frame
        // the last one is taken again, which leaves the scan where it is (d = 0), and its sums are not stored
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            double s[D];
#pragma unroll
            for (int d = 0; d < D; ++d)
                s[d] = 0.0;
#pragma unroll
            for (int k = 0; k < DIP_LANE_POINTS; ++k)
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    double x = (double)raw[b][k][d];
                    if (UNWRAP) {
                        const double dx = __dsub_rn(x, old[k][d]);
                        if (fabs(dx) >= half[d])
                            im[k][d] -= (dx > 0.0) - (dx < 0.0);
                        old[k][d] = x;
                        x = __dadd_rn(x, __dmul_rn((double)im[k][d], L[d]));
                    }
                    if (live[k])
                        s[d] = __dadd_rn(s[d], __dmul_rn(q[k], x));
                }
#pragma unroll
            for (int d = 0; d < D; ++d)
                fold[b * 3 + d0 + d][lane] = s[d];
        }
        __syncthreads();
        // lane r of a wave adds one of the rows its own wave wrote: frame r / D of the batch, component d0 + r % D
        const int nb = min(BATCH, f_hi - f0);
        if (lane < nb * D) {
            const int b = lane / D, d = d0 + lane - D * b;
            double s = 0.0;
#pragma unroll 8
            for (int l = 0; l < 64; ++l)
                s = __dadd_rn(s, fold[b * 3 + d][l]);
            partial[(int64_t(f0 + b) * n_tiles + t) * 3 + d] = s;
        }
        __syncthreads();
    }

    if (UNWRAP)
#pragma unroll
        for (int k = 0; k < DIP_LANE_POINTS; ++k)
            if (live[k]) {
                const int64_t p = tile.point0 + lane + 64 * k;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    prev[p * 3 + d0 + d] = old[k][d];
                    image[p * 3 + d0 + d] = im[k][d];
                }
            }
}

// rows[frame][group][3] = the group's tile sums [tile_offsets[g], tile_offsets[g + 1]) added in tile order.  One
// thread per (frame, group, component).
__global__ __launch_bounds__(256) void dip_fold_kernel(const double *__restrict__ partial, int n_tiles,
                                                       const int *__restrict__ tile_offsets, int n_groups,
                                                       int64_t n_frames, double *__restrict__ rows)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_frames * n_groups * 3)
        return;
    const int d = int(i % 3);
    const int g = int((i / 3) % n_groups);
    const int64_t f = i / (int64_t(3) * n_groups);
    const double *__restrict__ in = partial + f * n_tiles * 3 + d;
    double s = 0.0;
    for (int t = tile_offsets[g]; t < tile_offsets[g + 1]; ++t)
        s = __dadd_rn(s, in[int64_t(t) * 3]);
    rows[i] = s;
}

}  // namespace mdx_dip_dev
