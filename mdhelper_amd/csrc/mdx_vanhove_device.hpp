// mdx_vanhove_device.hpp — device side of the self van Hove engine (mdx_vanhove.hip).
//
// Result contract.  Rows arrive in the order of the concatenated groups: group g holds n_points[g] consecutive points.
// Analysed frames are numbered f = 0, 1, ... in the order fed; `lags` is a strictly increasing list of non-negative
// frame offsets.  Everything is float64 with separate multiply and add (the unit is built with contraction off);
// float32 coordinates are widened before any arithmetic.  Per point p, component d, lag k and frame f >= lags[k]:
//
//     x_pd(f)  = (double)r_pd(f) + image_pd(f) * L_d              (image = 0 without unwrap)
//     d_d      = x_pd(f) - x_pd(f - lag)                           (d_d = +0.0 for a component that zero_dims drops)
//     r2       = (d_x*d_x + d_y*d_y) + d_z*d_z ;  r = sqrt(r2), correctly rounded ;  r4 = r2*r2
//     counts[k][g][b] += 1   where  edges[b] <= r < edges[b+1]     (the last bin also takes r == edges[n_bins];
//                                                                   r outside the edges or not finite: not counted)
//     m2[k][p] += r2 ,  m4[k][p] += r4                             (whether or not r was counted)
//
// image follows the reference's global unwrap (algorithm/topology.py `unwrap`, the rule of prof_unwrap_scan_kernel in
// mdx_points_device.hpp): d = x_raw(f) - x_raw(f - 1) in float64, and |d| >= L_d / 2 moves the count by -sign(d).
// The first analysed frame is its own start with image 0: a displacement does not depend on the starting image.
//
// Counts.  With edges = numpy.linspace(r_min, r_max, n_bins + 1) they equal numpy.histogram(r, n_bins, (r_min, r_max))
// count for count: the candidate bin is one multiply, the fix-up compares r against edges[b] and edges[b + 1].  They
// are integers (uint64 in HBM), added with integer atomics: their value does not depend on arrival order.
//
// Moments.  No floating-point atomics and no cross-lane sums.  The accumulator of (lag k, point p) lives in HBM
// (acc[k][p][2] = m2, m4), starts at +0.0 and receives its terms one after the other in frame order: a thread owns
// one (point, lag), reads the accumulator at the start of a slab, walks the slab's frames and writes it back.
// vh_fold_kernel then adds the accumulators of a group's points one after the other in row order, from +0.0.  A plain
// host loop gives the same bits, whatever route the frames take and however they are split into calls or slabs.
//
// Shape.  vh_prepare_kernel writes the widened, image-shifted points into a ring of frames in HBM,
// hist[f % cap][d][p] (component-major, so that the lanes of a wave read consecutive doubles), cap = max(lags) + the
// frames of a slab: a lag reaches back across slabs and calls.  vh_bin_kernel: a block is VH_BLOCK_LAGS waves; every
// wave has the same tile of VH_TILE consecutive points (a tile never spans two groups) on its lanes and a lag of its
// own, so x(f) of the tile is fetched once per block from HBM / L2 and VH_BLOCK_LAGS - 1 more times from the CU's L1.
//
// LDS counters and contention.  At short lags nearly all displacements of a tile fall into one or two bins (at lag 0
// all of them into the bin that holds 0), so the lanes of a wave meet on one LDS word.  Every wave has its own uint32
// histogram in LDS (its lag's): waves never meet on a counter, and what is left is the 64 lanes of one ds_add.
// Folding equal bins within the wave before the atomic (ballot of the lanes with the first lane's bin, one add of
// their number, two rounds, the rest singly) was measured against the plain per-lane add on an MI355X, 32 768 points
// x 1 024 frames x 64 lags: 10.69 / 9.30 ms folded against 10.08 / 8.90 ms plain at 201 bins (lags 0 ... 63 / lags
// 0, 8 ... 504), and 10.44 / 9.32 against 9.94 / 8.93 ms with 4 bins, where every lag puts a whole wave into one or
// two bins.  The same-address adds of one wave are not what the loop waits for, so the plain add is used.  At the
// end of the slab the non-zero LDS bins go to the global uint64 counts with one integer atomic each.  A wave's
// counter receives at most 64 lanes x VH_SLAB_MAX frames = 2^21 per launch, so the uint32 cannot overflow.
// Histograms of more than VH_LDS_BINS bins do not fit and are counted in HBM directly.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mdx_vh_dev {

constexpr int VH_TILE = 64;                   // points per tile = lanes of a wave
constexpr int VH_BLOCK_LAGS = 4;              // lags (waves) per block
constexpr int VH_THREADS = VH_TILE * VH_BLOCK_LAGS;
constexpr int VH_LDS_BINS = 4096;             // n_bins up to which the block's histograms live in LDS (64 KiB)
constexpr int64_t VH_SLAB_MAX = 32768;        // frames per launch, at most

struct VhTile {
    int point0;     // first point, in concatenated-group order
    int count;      // 1 ... VH_TILE
    int group;
};

// x = (double)r + image * L of n_frames frames into the ring: hist[((f0 + f) % cap) * 3 + d][p].  One thread per
// coordinate (c = d * n_points + p, so that a wave writes consecutive doubles).  UNWRAP: the thread walks the frames
// and carries prev / image as prof_unwrap_scan_kernel does (first: this is the first analysed frame, whose
// displacement is zero); the state is read at the start and written back at the end.  Without it grid y spreads
// the frames.
template <bool UNWRAP>
__global__ __launch_bounds__(256) void vh_prepare_kernel(const float *__restrict__ pos, int64_t src_rows,
                                                         const int *__restrict__ index, int n_points, int n_frames,
                                                         int64_t f0, int64_t cap, double Lx, double Ly, double Lz,
                                                         int first, double *__restrict__ prev,
                                                         int *__restrict__ image, double *__restrict__ hist)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= 3 * n_points)
        return;
    const int d = c / n_points, p = c - d * n_points;
    const int64_t r = index ? index[p] : p;
    if (!UNWRAP) {
        const int f = blockIdx.y;
        const int64_t slot = (f0 + f) % cap;
        hist[(slot * 3 + d) * n_points + p] = (double)pos[(int64_t(f) * src_rows + r) * 3 + d];
        return;
    }
    const double L = d == 0 ? Lx : d == 1 ? Ly : Lz;
    const double half = L / 2;
    double old = first ? 0.0 : prev[c];
    int im = first ? 0 : image[c];
    int64_t slot = f0 % cap;
    for (int f = 0; f < n_frames; ++f) {
        const double x = (double)pos[(int64_t(f) * src_rows + r) * 3 + d];
        if (!(first && f == 0)) {
            const double dx = __dsub_rn(x, old);
            if (fabs(dx) >= half)
                im -= (dx > 0.0) - (dx < 0.0);
        }
        old = x;
        hist[(slot * 3 + d) * n_points + p] = __dadd_rn(x, __dmul_rn((double)im, L));
        if (++slot == cap)
            slot = 0;
    }
    prev[c] = old;
    image[c] = im;
}

// the b with edges[b] <= r < edges[b + 1] (the last bin closed on the right), or -1
__device__ __forceinline__ int vh_bin(double r, const double *__restrict__ edges, int n_bins, double inv_width)
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

// Frames [f_lo, f_hi) (numbers since the first analysed frame) against the frames `lag` before them.  Grid: x = tiles,
// y = runs of VH_BLOCK_LAGS lags; wave w of a block takes lag blockIdx.y * VH_BLOCK_LAGS + w.  keep: bit d set ->
// component d takes part.  counts: uint64 [n_lags][n_groups][n_bins]; acc: double [n_lags][n_points][2].
template <bool USE_LDS>
__global__ __launch_bounds__(VH_THREADS) void vh_bin_kernel(
    const double *__restrict__ hist, int64_t cap, int n_points, const VhTile *__restrict__ tiles,
    const int64_t *__restrict__ lags, int n_lags, int64_t f_lo, int64_t f_hi, int keep,
    const double *__restrict__ edges, int n_bins, double inv_width, int n_groups,
    unsigned long long *__restrict__ counts, double *__restrict__ acc)
{
    extern __shared__ unsigned int vh_lds[];        // [VH_BLOCK_LAGS][n_bins] (USE_LDS)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const VhTile tile = tiles[blockIdx.x];
    const int k = blockIdx.y * VH_BLOCK_LAGS + w;
    if (USE_LDS) {
        for (int i = threadIdx.x; i < VH_BLOCK_LAGS * n_bins; i += VH_THREADS)
            vh_lds[i] = 0u;
        __syncthreads();
    }
    if (k < n_lags) {                               // the same in every lane of the wave
        const int64_t lag = lags[k];
        const bool live = lane < tile.count;
        const int p = tile.point0 + (live ? lane : 0);      // lanes without a point read the tile's first one
        double *__restrict__ mine = acc + (int64_t(k) * n_points + p) * 2;
        double m2 = mine[0], m4 = mine[1];
        const int64_t f_first = f_lo > lag ? f_lo : lag;
        int64_t sa = f_first % cap, sb = (f_first - lag) % cap;
        unsigned long long *__restrict__ row = counts + (int64_t(k) * n_groups + tile.group) * n_bins;
        for (int64_t f = f_first; f < f_hi; ++f) {
            const double *__restrict__ a = hist + sa * 3 * n_points + p;
            const double *__restrict__ b = hist + sb * 3 * n_points + p;
            const double dx = keep & 1 ? __dsub_rn(a[0], b[0]) : 0.0;
            const double dy = keep & 2 ? __dsub_rn(a[n_points], b[n_points]) : 0.0;
            const double dz = keep & 4 ? __dsub_rn(a[2 * int64_t(n_points)], b[2 * int64_t(n_points)]) : 0.0;
            const double r2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
            const double r = __dsqrt_rn(r2);
            m2 = __dadd_rn(m2, r2);
            m4 = __dadd_rn(m4, __dmul_rn(r2, r2));
            const int bin = live ? vh_bin(r, edges, n_bins, inv_width) : -1;
            if (bin >= 0) {
                if (USE_LDS)
                    atomicAdd(&vh_lds[w * n_bins + bin], 1u);
                else
                    atomicAdd(&row[bin], 1ull);
            }
            if (++sa == cap)
                sa = 0;
            if (++sb == cap)
                sb = 0;
        }
        if (live) {
            mine[0] = m2;
            mine[1] = m4;
        }
    }
    if (USE_LDS) {
        __syncthreads();
        // one integer atomic per non-empty bin, lag and block: integer adds commute
        for (int i = threadIdx.x; i < VH_BLOCK_LAGS * n_bins; i += VH_THREADS) {
            const int wi = i / n_bins, b = i - wi * n_bins;
            const int ki = blockIdx.y * VH_BLOCK_LAGS + wi;
            const unsigned int v = vh_lds[i];
            if (v && ki < n_lags)
                atomicAdd(&counts[(int64_t(ki) * n_groups + tile.group) * n_bins + b], (unsigned long long)v);
        }
    }
}

// moments[k][g][m] = the accumulators of the group's points [offsets[g], offsets[g + 1]) added in row order from
// +0.0.  One thread per (lag, group, moment).
__global__ __launch_bounds__(256) void vh_fold_kernel(const double *__restrict__ acc, int n_points,
                                                      const int64_t *__restrict__ offsets, int n_groups, int n_lags,
                                                      double *__restrict__ moments)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= int64_t(n_lags) * n_groups * 2)
        return;
    const int m = int(i & 1);
    const int g = int((i >> 1) % n_groups);
    const int64_t k = (i >> 1) / n_groups;
    const double *__restrict__ in = acc + k * n_points * 2 + m;
    double s = 0.0;
    for (int64_t p = offsets[g]; p < offsets[g + 1]; ++p)
        s = __dadd_rn(s, in[p * 2]);
    moments[i] = s;
}

}  // namespace mdx_vh_dev
