// mdx_orient_device.hpp — device side of the orientational relaxation engine (mdx_orient.hip).
//
// Result contract.  A frame delivers n_rows points (the distinct atoms, picked by the feed's index); the table
// pairs int32 [V][2] of row numbers (tail, head) defines V vectors, and group g holds n_vectors[g] consecutive ones (a
// group may be empty).  Analysed frames are numbered f = 0, 1, ... in the order fed; `lags` is a strictly increasing
// list of non-negative frame offsets.  Everything is float64, one operation at a time (the unit is built with
// contraction off); float32 coordinates are widened before any arithmetic.
//
// Prepare, per vector v and frame f:
//
//     d_c = x_head,c - x_tail,c
//     w_c = d_c - L_c * rint(d_c * inv_c)         with a box: min_image of mdx_pairs_device.hpp, inv_c = 1.0 / L_c
//                                                 formed once on the host;  w_c = d_c without a box;
//                                                 w_c = +0.0 for a component that zero_dims drops
//     n2  = (w_x*w_x + w_y*w_y) + w_z*w_z         (r2_of) ;  n = sqrt(n2), correctly rounded
//     u_c = w_c / n                               a correctly rounded divide
//
// A vector with n2 == 0 or n2 not finite is degenerate: its u is stored as (0, 0, 0) and an integer counter in HBM
// counts it (an integer atomic: the count does not depend on arrival order).  Once the counter is not zero the host
// refuses synchronize, result and the other read-outs until a reset, as CappedLists of mdx_pairs_host.hpp does for an
// over-full row: an error, never a silently wrong average.
//
// Correlate, per vector v, lag k and frame f >= lags[k]:
//
//     c = (u_x(f)*u_x(f-lag) + u_y(f)*u_y(f-lag)) + u_z(f)*u_z(f-lag)
//     acc[k][v][0] += c ;  acc[k][v][1] += (1.5 * (c*c)) - 0.5
//
// No floating-point atomics and no cross-lane sums.  The accumulator of (lag k, vector v) lives in HBM, starts at
// +0.0 and receives its terms one after the other in frame order: a thread owns one (vector, lag), reads the
// accumulator at the start of a slab, walks the slab's frames and writes it back.  ori_fold_kernel then adds the
// accumulators of a group's vectors one after the other in row order from +0.0 into sums[k][g][2].  A plain host loop
// gives the same bits, whatever route the frames take and however they are split into calls or slabs.
//
// Order tensor, per frame f, group g and each of the six products ab = xx, xy, xz, yy, yz, zz: a tile partial is the
// sum of u_a*u_b over the tile's vectors in row order from +0.0; the group's sum is the sum of its tile partials in
// tile order from +0.0, stored as frame_sums[f][g][6].  No floating-point atomics here either.
//
// Shape.  Tiles of ORI_TILE consecutive vectors never span two groups.  ori_prepare_kernel: a wave has a tile on its
// lanes, forms u, writes it into a ring of frames in HBM, hist[f % cap][c][v] (component-major, so that the lanes of a
// wave read consecutive doubles), cap = max(lags) + the frames of a slab, and leaves u in LDS, from where six lanes
// each add one product of the tile in row order.  ori_group_kernel adds the tile partials of a group.
// ori_correlate_kernel has vh_bin_kernel's shape (mdx_vanhove_device.hpp): a block is ORI_BLOCK_LAGS waves; every
// wave has the same tile on its lanes and a lag of its own, so u(f) of the tile is fetched once per block from
// HBM / L2 and ORI_BLOCK_LAGS - 1 more times from the CU's L1.
#pragma once

#include "mdx_pairs_device.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mdx_ori_dev {

using mdx_pairs_dev::PairBox;

constexpr int ORI_TILE = 64;                  // vectors per tile = lanes of a wave
constexpr int ORI_BLOCK_LAGS = 4;             // lags (waves) per block of the correlate kernel
constexpr int ORI_BLOCK_TILES = 4;            // tiles (waves) per block of the prepare kernel
constexpr int ORI_THREADS = ORI_TILE * ORI_BLOCK_LAGS;
constexpr int64_t ORI_SLAB_MAX = 32768;       // frames per launch, at most (grid y of the prepare kernel)

struct OriTile {
    int vector0;    // first vector, in concatenated-group order
    int count;      // 1 ... ORI_TILE
    int group;
};

// u of the tiles' vectors in n_frames frames into the ring, hist[((f0 + f) % cap) * 3 + c][v], and the six products
// of every tile, part[f][tile][6].  Grid: x = runs of ORI_BLOCK_TILES tiles, y = frames; wave w of a block takes tile
// blockIdx.x * ORI_BLOCK_TILES + w.  Row index[r] (or r) of a frame of src_rows rows is point r.  keep: bit c set ->
// component c takes part.
template <bool BOX>
__global__ __launch_bounds__(ORI_TILE * ORI_BLOCK_TILES) void ori_prepare_kernel(
    const float *__restrict__ pos, int64_t src_rows, const int *__restrict__ index, const int *__restrict__ pairs,
    const OriTile *__restrict__ tiles, int n_tiles, int n_vectors, int64_t f0, int64_t cap, PairBox box, int keep,
    double *__restrict__ hist, double *__restrict__ part, unsigned long long *__restrict__ degenerate)
{
    __shared__ double ori_u[ORI_BLOCK_TILES][3][ORI_TILE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t = blockIdx.x * ORI_BLOCK_TILES + w;
    const bool have = t < n_tiles;                  // the same in every lane of the wave
    const OriTile tile = tiles[have ? t : 0];
    const int64_t f = blockIdx.y;
    double ux = 0.0, uy = 0.0, uz = 0.0;
    if (have && lane < tile.count) {
        const int v = tile.vector0 + lane;
        const int tail = pairs[2 * int64_t(v)], head = pairs[2 * int64_t(v) + 1];
        const float *__restrict__ a = pos + (f * src_rows + (index ? index[tail] : tail)) * 3;
        const float *__restrict__ b = pos + (f * src_rows + (index ? index[head] : head)) * 3;
        double wx = __dsub_rn((double)b[0], (double)a[0]);
        double wy = __dsub_rn((double)b[1], (double)a[1]);
        double wz = __dsub_rn((double)b[2], (double)a[2]);
        if (BOX) {
            wx = mdx_pairs_dev::min_image(wx, box.L[0], box.inv[0]);
            wy = mdx_pairs_dev::min_image(wy, box.L[1], box.inv[1]);
            wz = mdx_pairs_dev::min_image(wz, box.L[2], box.inv[2]);
        }
        wx = keep & 1 ? wx : 0.0;
        wy = keep & 2 ? wy : 0.0;
        wz = keep & 4 ? wz : 0.0;
        const double n2 = mdx_pairs_dev::r2_of(wx, wy, wz);
        if (n2 > 0.0 && n2 <= 1.7976931348623157e308) {
            const double n = __dsqrt_rn(n2);
            ux = __ddiv_rn(wx, n);
            uy = __ddiv_rn(wy, n);
            uz = __ddiv_rn(wz, n);
        } else {
            atomicAdd(degenerate, 1ull);            // n2 == 0, infinite or NaN: u stays (0, 0, 0)
        }
        double *__restrict__ out = hist + ((f0 + f) % cap) * 3 * n_vectors + v;
        out[0] = ux;
        out[n_vectors] = uy;
        out[2 * int64_t(n_vectors)] = uz;
    }
    ori_u[w][0][lane] = ux;
    ori_u[w][1][lane] = uy;
    ori_u[w][2][lane] = uz;
    __syncthreads();
    if (have && lane < 6) {
        // lane 0 ... 5: xx, xy, xz, yy, yz, zz
        const int a = lane < 3 ? 0 : lane < 5 ? 1 : 2;
        const int b = lane < 3 ? lane : lane < 5 ? lane - 2 : 2;
        double s = 0.0;
        for (int i = 0; i < tile.count; ++i)
            s = __dadd_rn(s, __dmul_rn(ori_u[w][a][i], ori_u[w][b][i]));
        part[(f * n_tiles + t) * 6 + lane] = s;
    }
}

// frame_sums[f0 + f][g][q] = the partials part[f][t][q] of the group's tiles [tile_offsets[g], tile_offsets[g + 1])
// added in tile order from +0.0.  One thread per (frame, group, product).
__global__ __launch_bounds__(256) void ori_group_kernel(const double *__restrict__ part, int n_tiles,
                                                        const int *__restrict__ tile_offsets, int n_groups,
                                                        int n_frames, int64_t f0, double *__restrict__ frame_sums)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= int64_t(n_frames) * n_groups * 6)
        return;
    const int q = int(i % 6);
    const int g = int((i / 6) % n_groups);
    const int64_t f = i / 6 / n_groups;
    double s = 0.0;
    for (int t = tile_offsets[g]; t < tile_offsets[g + 1]; ++t)
        s = __dadd_rn(s, part[(f * n_tiles + t) * 6 + q]);
    frame_sums[f0 * n_groups * 6 + i] = s;
}

// Frames [f_lo, f_hi) (numbers since the first analysed frame) against the frames `lag` before them.  Grid: x = tiles,
// y = runs of ORI_BLOCK_LAGS lags; wave w of a block takes lag blockIdx.y * ORI_BLOCK_LAGS + w.
// acc: double [n_lags][n_vectors][2].
__global__ __launch_bounds__(ORI_THREADS) void ori_correlate_kernel(
    const double *__restrict__ hist, int64_t cap, int n_vectors, const OriTile *__restrict__ tiles,
    const int64_t *__restrict__ lags, int n_lags, int64_t f_lo, int64_t f_hi, double *__restrict__ acc)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const OriTile tile = tiles[blockIdx.x];
    const int k = blockIdx.y * ORI_BLOCK_LAGS + w;
    if (k >= n_lags)                                // the same in every lane of the wave
        return;
    const int64_t lag = lags[k];
    const bool live = lane < tile.count;
    const int v = tile.vector0 + (live ? lane : 0);         // lanes without a vector read the tile's first one
    double *__restrict__ mine = acc + (int64_t(k) * n_vectors + v) * 2;
    double c1 = mine[0], c2 = mine[1];
    const int64_t f_first = f_lo > lag ? f_lo : lag;
    int64_t sa = f_first % cap, sb = (f_first - lag) % cap;
    const int64_t stride = n_vectors;
#pragma unroll 4
    for (int64_t f = f_first; f < f_hi; ++f) {
        const double *__restrict__ a = hist + sa * 3 * stride + v;
        const double *__restrict__ b = hist + sb * 3 * stride + v;
        const double c = __dadd_rn(__dadd_rn(__dmul_rn(a[0], b[0]), __dmul_rn(a[stride], b[stride])),
                                   __dmul_rn(a[2 * stride], b[2 * stride]));
        c1 = __dadd_rn(c1, c);
        c2 = __dadd_rn(c2, __dsub_rn(__dmul_rn(1.5, __dmul_rn(c, c)), 0.5));
        if (++sa == cap)
            sa = 0;
        if (++sb == cap)
            sb = 0;
    }
    if (live) {
        mine[0] = c1;
        mine[1] = c2;
    }
}

// sums[k][g][m] = the accumulators of the group's vectors [offsets[g], offsets[g + 1]) added in row order from +0.0.
// One thread per (lag, group, m).
__global__ __launch_bounds__(256) void ori_fold_kernel(const double *__restrict__ acc, int n_vectors,
                                                       const int64_t *__restrict__ offsets, int n_groups, int n_lags,
                                                       double *__restrict__ sums)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= int64_t(n_lags) * n_groups * 2)
        return;
    const int m = int(i & 1);
    const int g = int((i >> 1) % n_groups);
    const int64_t k = (i >> 1) / n_groups;
    const double *__restrict__ in = acc + k * n_vectors * 2 + m;
    double s = 0.0;
    for (int64_t p = offsets[g]; p < offsets[g + 1]; ++p)
        s = __dadd_rn(s, in[p * 2]);
    sums[i] = s;
}

}  // namespace mdx_ori_dev
