// mdx_pairs_device.hpp — the device pieces the pair engines share (mdx_vanhove_distinct, mdx_residence, mdx_cluster,
// mdx_angle): the gather of a slab, the box and pair arithmetic, the walk over i tiles x j chunks x LDS stages, the
// capped lists and the block tally.  Each engine's *_device.hpp states its own results and refers to this text for
// the arithmetic; its kernels are set-up, the loop over the stages of their chunk (staging with stage_partners, the
// pairs of a stage with stage_pairs and a per-pair rule), and their epilogue.  The loop over the stages stands in
// each kernel: as one template over the four it measured 0.5 - 0.8 % slower than the loops it replaced (NOTES.md,
// round 10).
//
// Box and pair arithmetic (a result contract, stated here once).  One constant orthorhombic box, lengths L_c;
// inv_c = 1.0 / L_c is formed once on the host in float64.  Everything is float64, one operation at a time (the units
// are built with contraction off); float32 coordinates are widened before any arithmetic.  For a lane's point i and a
// partner j:
//
//     d_c = x_jc - x_ic ;  s = d_c * inv_c ;  w_c = d_c - L_c * rint(s)        (rint: ties to even, as numpy.rint;
//                                                                              w_c = +0.0 for a dropped component)
//     r2  = (w_x*w_x + w_y*w_y) + w_z*w_z
//
// A bound is compared as r2 <= rc2 with rc2 formed once on the host in float64: a NaN r2 is never inside, and no
// square root is taken for a comparison.  With `same` both sides are one set and the pair i == j is left out.
//
// Capped lists.  A row holds at most max_nb entries in one frame.  A row that would hold more is an error, never a
// silent truncation: append_capped stores only into the row's max_nb slots but keeps counting, block_tally keeps the
// largest row seen in one word in HBM, and the host (CappedLists in mdx_pairs_host.hpp) refuses to hand out results
// from the next synchronize / result on until a reset.
//
// The walk (in each engine's kernel).  grid x = i tiles x j chunks.  A block holds PAIR_TILE points in registers, one
// per lane, widened, and walks its chunk of at most JCHUNK partners in stages of PAIR_STAGE points through LDS
// (widened once when staged; every lane reads the same j at once, a broadcast).  14 float64 operations to r2 per pair.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mdx_pairs_dev {

constexpr int PAIR_TILE = 256;                // points per block on the lane side, one per lane
constexpr int PAIR_THREADS = PAIR_TILE;
constexpr int PAIR_WAVES = PAIR_THREADS / 64;
constexpr int PAIR_STAGE = PAIR_THREADS;      // partners per LDS stage, one staged per thread
constexpr int PAIR_MAX_NEIGHBORS = 64;        // slots of a capped row at most
constexpr int64_t PAIR_SLAB_MAX = 32768;      // frames per launch, at most (grid y / z)

struct PairBox {
    double L[3], inv[3];
};

// w = d - L * rint(d * inv), one operation at a time
__device__ __forceinline__ double min_image(double d, double L, double inv)
{
    return __dsub_rn(d, __dmul_rn(L, rint(__dmul_rn(d, inv))));
}

// r2 = (wx*wx + wy*wy) + wz*wz
__device__ __forceinline__ double r2_of(double wx, double wy, double wz)
{
    return __dadd_rn(__dadd_rn(__dmul_rn(wx, wx), __dmul_rn(wy, wy)), __dmul_rn(wz, wz));
}

// (wx, wy, wz) of the partner (xj, yj, zj) seen from (xi, yi, zi).  keep: bit c set -> component c takes part; ALL:
// keep == 7, known when compiled.
template <bool ALL>
__device__ __forceinline__ void min_image_of(double xj, double yj, double zj, double xi, double yi, double zi,
                                             const PairBox &box, int keep, double &wx, double &wy, double &wz)
{
    const double dx = __dsub_rn(xj, xi), dy = __dsub_rn(yj, yi), dz = __dsub_rn(zj, zi);
    wx = ALL || keep & 1 ? min_image(dx, box.L[0], box.inv[0]) : 0.0;
    wy = ALL || keep & 2 ? min_image(dy, box.L[1], box.inv[1]) : 0.0;
    wz = ALL || keep & 4 ? min_image(dz, box.L[2], box.inv[2]) : 0.0;
}

// what gather_kernel does per point beyond the gather: nothing
struct NoPointHook {
    __device__ __forceinline__ void operator()(int64_t, int, int) const {}
};

// Row index[p] (or p) of n_frames float32 frames of src_rows rows, component-major: out[(slot * 3 + c) * n_points + p],
// slot = f, or with RING (f0 + f) % cap (the plain form has no 64-bit modulo).  One thread per coordinate
// (t = c * n_points + p: a wave writes consecutive floats); grid y = frames.  The threads of component 0 also call
// hook(f, p, n_points).
template <bool RING, typename Hook>
__global__ __launch_bounds__(256) void gather_kernel(const float *__restrict__ pos, int64_t src_rows,
                                                     const int *__restrict__ index, int n_points, int64_t f0,
                                                     int64_t cap, float *__restrict__ out, Hook hook)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 3 * n_points)
        return;
    const int c = t / n_points, p = t - c * n_points;
    const int64_t r = index ? index[p] : p;
    const int64_t f = blockIdx.y;
    int64_t slot = f;
    if (RING)
        slot = (f0 + f) % cap;
    out[(slot * 3 + c) * n_points + p] = pos[(f * src_rows + r) * 3 + c];
    if (c == 0)
        hook(f, p, n_points);
}

// partner js + t of the component-major frame b (n_points rows) into stage[4 * t + 0 ... 2], t = the thread
__device__ __forceinline__ void stage_partners(double *__restrict__ stage, const float *__restrict__ b, int n_points,
                                               int js)
{
    const float *__restrict__ src = b + js + threadIdx.x;
    stage[4 * threadIdx.x + 0] = (double)src[0];
    stage[4 * threadIdx.x + 1] = (double)src[n_points];
    stage[4 * threadIdx.x + 2] = (double)src[2 * int64_t(n_points)];
}

// Appends j to a slot-major capped row (entries `stride` words apart): other j chunks append to the same row, so the
// slot comes from an atomic; beyond max_nb nothing is stored but the count goes on.  row: the lane's longest so far.
__device__ __forceinline__ void append_capped(int *__restrict__ my_len, int *__restrict__ my_list, int64_t stride,
                                              int max_nb, int j, unsigned int &row)
{
    const int slot = atomicAdd(my_len, 1);
    if (slot < max_nb)
        my_list[int64_t(slot) * stride] = j;
    row = (unsigned int)slot + 1u > row ? (unsigned int)slot + 1u : row;
}

// The block's tally: `found` summed and `row` maximised over the wave by shuffles, over the block in two LDS words
// (zero, and a barrier since), then one integer add to *total and one atomicMax into *max_row per block: integer
// adds and max commute.  COUNT = false is the max-only form: found, block_found and total are not touched.
template <bool COUNT>
__device__ __forceinline__ void block_tally(unsigned int found, unsigned int row, unsigned int *block_found,
                                            unsigned int *block_row, unsigned long long *__restrict__ total,
                                            int *__restrict__ max_row)
{
    for (int off = 32; off > 0; off >>= 1) {
        if (COUNT)
            found += __shfl_down(found, off);
        const unsigned int other = __shfl_down(row, off);
        row = other > row ? other : row;
    }
    if ((threadIdx.x & 63) == 0 && (COUNT ? found | row : row)) {
        if (COUNT)
            atomicAdd(block_found, found);
        atomicMax(block_row, row);
    }
    __syncthreads();
    if (threadIdx.x == 0 && (COUNT ? *block_found : *block_row)) {
        if (COUNT)
            atomicAdd(total, (unsigned long long)*block_found);
        atomicMax(max_row, (int)*block_row);
    }
}

// The pairs of one stage: the staged partners js ... js + nj - 1 against the lane's point (xi, yi, zi).
// on_pair(jj, j, wx, wy, wz, r2, other) is called per pair, j = js + jj; other: j is not the lane's own point (stage
// entry `skip`, -1 for none).  It is called for the own point too, and a rule tests `other` in one condition with its
// bound, behind it: the arithmetic of a stage then runs without a branch around it.
template <bool ALL, typename Pair>
__device__ __forceinline__ void stage_pairs(const double *__restrict__ stage, int nj, int js, int skip, double xi,
                                            double yi, double zi, const PairBox &box, int keep, Pair on_pair)
{
#pragma unroll 4
    for (int jj = 0; jj < nj; ++jj) {
        double wx, wy, wz;
        min_image_of<ALL>(stage[4 * jj + 0], stage[4 * jj + 1], stage[4 * jj + 2], xi, yi, zi, box, keep, wx, wy, wz);
        on_pair(jj, js + jj, wx, wy, wz, r2_of(wx, wy, wz), jj != skip);
    }
}

}  // namespace mdx_pairs_dev
