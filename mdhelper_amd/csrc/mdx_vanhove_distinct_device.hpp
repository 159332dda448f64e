// mdx_vanhove_distinct_device.hpp — device side of the distinct van Hove engine (mdx_vanhove_distinct.hip).
//
// Result contract.  Set 1 holds n1 rows, set 2 holds n2 rows; incoming rows are set 1 then set 2.  With `same` both
// are one set (n1 == n2, the rows arrive once) and the pair i == j is left out.  Analysed frames are numbered
// f = 0, 1, ... in the order fed; `lags` is strictly increasing and non-negative; origin_step >= 1.  The frame pairs
// of lag k are (f0, f0 + lags[k]) with f0 % origin_step == 0 and f0 + lags[k] < F.  Box and pair arithmetic: those of
// mdx_pairs_device.hpp, for every such frame pair and every pair (i of set 1 at f0, j of set 2 at f0 + lag):
//
//     d_c = x2_jc(f0 + lag) - x1_ic(f0) ;  w_c and r2 as stated there ;  r = sqrt(r2), correctly rounded
//     counts[k][b] += 1   where  edges[b] <= r < edges[b+1]    (the last bin also takes r == edges[n_bins];
//                                                              r outside the edges or not finite: not counted)
//
// There is no unwrap: the minimum image of a difference does not need one.  The contract is on the coordinates as
// given, and the box is one box for every frame.
//
// Counts.  With edges = numpy.linspace(r_min, r_max, n_bins + 1) they equal numpy.histogram(r, n_bins, (r_min,
// r_max)) count for count: the bin rule is that of vh_bin in mdx_vanhove_device.hpp (candidate bin by one multiply,
// fix-up against edges[b] and edges[b + 1]).  They are integers (uint64 in HBM), added with integer atomics only:
// their value does not depend on arrival order, so the work shards over i tiles, j chunks and frame pairs, and splits
// into calls and slabs, with no effect on the result.  This engine has no floating-point atomics at all.
//
// evaluations is the contract's pair count, sum_k n_origins(k) * (n1*n2 - (same ? n1 : 0)), not what the kernel
// happened to compute.
//
// Early rejection.  A pair is dropped before the square root when r2 > r2_hi or r2 < r2_lo, with
// r2_hi = fl(fl(hi*hi) * (1 + 2^-40)) and r2_lo = fl(fl(lo*lo) * (1 - 2^-40)) (0 for lo <= 0), hi = edges[n_bins],
// lo = edges[0].  fl(hi*hi) >= hi^2 (1 - 2^-53), so r2 > r2_hi gives r2 > hi^2 (1 + 2^-41), sqrt(r2) > hi (1 + 2^-43)
// in real numbers, which lies beyond the next double above hi (at most hi (1 + 2^-52)); rounding is monotone, so the
// correctly rounded r is greater than hi and would not have been counted.  The lower side is the mirror image.  A
// NaN r2 fails both comparisons of the keep test and is dropped, as the contract says.
//
// Shape.  gather_kernel (its ring form) gathers the rows of each incoming frame into a ring of frames in HBM,
// ring[f % cap][c][p] (component-major float32: widening is exact and happens in registers), cap = max(lags) + the
// frames of a slab, so that a lag reaches back across slabs and calls.  vhd_pair_kernel is the walk of
// mdx_pairs_device.hpp with y = lags, z = the new frames f of the launch and VHD_JCHUNK points of set 2 per block;
// the block of (f, k) is the frame pair (f - lags[k], f) and leaves at once when that is no pair of the contract:
// the lanes hold set 1 at f0 and the stages set 2 at f0 + lag.  The edges are
// copied to LDS once per block, so the bin rule's fix-up reads no global memory.  Every wave counts
// into its own uint32 histogram in LDS; at the end the block adds the waves' histograms bin by bin and sends the
// non-zero sums to the global uint64 counts with one integer atomic each.  A wave's LDS counter receives at most
// 64 lanes x VHD_JCHUNK = 2^15 counts per launch (a block is one launch's share of one frame pair), far below 2^32.
// Histograms of more than VHD_LDS_BINS bins are counted in HBM directly.
//
// No cell list and no spatial culling: with r_max a sizeable share of the box nearly every wave holds a pair inside
// the range, so the early rejection rarely spares a whole wave.  Culling by cells is the follow-up.
#pragma once

#include "mdx_pairs_device.hpp"

namespace mdx_vhd_dev {

using namespace mdx_pairs_dev;

constexpr int VHD_TILE = PAIR_TILE;           // set-1 points per block, one per lane
constexpr int VHD_THREADS = PAIR_THREADS;
constexpr int VHD_WAVES = PAIR_WAVES;
constexpr int VHD_STAGE = PAIR_STAGE;         // set-2 points per LDS stage, one staged per thread
constexpr int VHD_JCHUNK = 2 * VHD_STAGE;     // set-2 points per block; 64 lanes x VHD_JCHUNK = 2^15 < 2^32 counts
                                              // per wave's uint32 LDS counter and launch
// n_bins up to which the edges and the waves' histograms live in LDS: 2049 x 8 B + 4 waves x 2048 x 4 B = 48 KiB next
// to the 8 KiB stage: inside the 64 KiB a launch gets without asking for more
constexpr int VHD_LDS_BINS = 2048;
constexpr int64_t VHD_SLAB_MAX = PAIR_SLAB_MAX;         // frames per launch, at most (grid z)
constexpr int VHD_LAGS_MAX = 65535;           // lags, at most (grid y)

// The b with edges[b] <= r < edges[b + 1] (the last bin closed on the right), or -1: vh_bin of mdx_vanhove_device.hpp,
// copied because that header also defines the self engine's kernels and belongs in one unit only.
__device__ __forceinline__ int vhd_bin(double r, const double *__restrict__ edges, int n_bins, double inv_width)
{
    const double lo = edges[0], hi = edges[n_bins];
    if (!(r >= lo && r <= hi))
        return -1;
    int b = (int)__dmul_rn(__dsub_rn(r, lo), inv_width);
    b = b > n_bins - 1 ? n_bins - 1 : b;
    while (b > 0 && r < edges[b])
        --b;
    while (b < n_bins - 1 && r >= edges[b + 1])
        ++b;
    return b;
}

// The frame pairs (f - lags[k], f), f = f_lo + blockIdx.z, k = blockIdx.y.  n_points: rows of a ring frame; set 2
// starts at row off2 (0 with same).  keep: bit c set -> component c takes part; ALL: keep == 7, known when compiled,
// so that the loop over j has no branch before the range test.  counts: uint64 [n_lags][n_bins].
template <bool USE_LDS, bool ALL>
__global__ __launch_bounds__(VHD_THREADS) void vhd_pair_kernel(
    const float *__restrict__ ring, int64_t cap, int n_points, int n1, int n2, int off2, int same, int n_jchunks,
    const int64_t *__restrict__ lags, int64_t f_lo, int64_t origin_step, PairBox box, int keep,
    const double *__restrict__ edges, int n_bins, double inv_width, double r2_lo, double r2_hi,
    unsigned long long *__restrict__ counts)
{
    // double [VHD_STAGE][4] stage; with USE_LDS then double [n_bins + 1] edges and uint32 [VHD_WAVES][n_bins]
    extern __shared__ __attribute__((aligned(16))) double vhd_lds[];
    double *__restrict__ stage = vhd_lds;
    double *__restrict__ edges_lds = vhd_lds + 4 * VHD_STAGE;
    unsigned int *__restrict__ hist = reinterpret_cast<unsigned int *>(edges_lds + n_bins + 1);
    const int k = blockIdx.y;
    const int64_t f = f_lo + blockIdx.z;
    const int64_t f0 = f - lags[k];
    if (f0 < 0 || f0 % origin_step != 0)    // the same in every thread of the block: nobody waits at a barrier
        return;
    const int tile = blockIdx.x / n_jchunks, chunk = blockIdx.x - tile * n_jchunks;
    const int i = tile * VHD_TILE + threadIdx.x;
    const bool live = i < n1;
    const int w = threadIdx.x >> 6;
    const float *__restrict__ a = ring + (f0 % cap) * 3 * n_points + (live ? i : n1 - 1);
    const float *__restrict__ b = ring + (f % cap) * 3 * n_points + off2;
    const double xi = (double)a[0], yi = (double)a[n_points], zi = (double)a[2 * int64_t(n_points)];
    if (USE_LDS) {
        for (int t = threadIdx.x; t < VHD_WAVES * n_bins; t += VHD_THREADS)
            hist[t] = 0u;
        for (int t = threadIdx.x; t <= n_bins; t += VHD_THREADS)
            edges_lds[t] = edges[t];
    }
    const double *__restrict__ bin_edges = USE_LDS ? edges_lds : edges;
    unsigned int *__restrict__ mine = hist + w * n_bins;
    unsigned long long *__restrict__ row = counts + int64_t(k) * n_bins;
    const int j_begin = chunk * VHD_JCHUNK;
    const int j_end = n2 - j_begin < VHD_JCHUNK ? n2 : j_begin + VHD_JCHUNK;
    for (int js = j_begin; js < j_end; js += VHD_STAGE) {
        const int nj = j_end - js < VHD_STAGE ? j_end - js : VHD_STAGE;
        __syncthreads();                    // the stage is free (and, the first time, histograms and edges are set)
        if ((int)threadIdx.x < nj)
            stage_partners(stage, b, n_points, js);
        __syncthreads();
        if (!live)
            continue;
        const int skip = same ? i - js : -1;        // the stage entry that is this lane's own point
        stage_pairs<ALL>(stage, nj, js, skip, xi, yi, zi, box, keep,
                         [&](int, int, double, double, double, double r2, bool other) {
                             if (r2 >= r2_lo && r2 <= r2_hi && other) {
                                 const int bin = vhd_bin(__dsqrt_rn(r2), bin_edges, n_bins, inv_width);
                                 if (bin >= 0) {
                                     if (USE_LDS)
                                         atomicAdd(&mine[bin], 1u);
                                     else
                                         atomicAdd(&row[bin], 1ull);
                                 }
                             }
                         });
    }
    if (USE_LDS) {
        __syncthreads();
        // one integer atomic per non-empty bin and block: integer adds commute
        for (int bin = threadIdx.x; bin < n_bins; bin += VHD_THREADS) {
            unsigned int v = 0;
            for (int q = 0; q < VHD_WAVES; ++q)
                v += hist[q * n_bins + bin];
            if (v)
                atomicAdd(&row[bin], (unsigned long long)v);
        }
    }
}

}  // namespace mdx_vhd_dev
