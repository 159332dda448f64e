// mdx_hbond_device.hpp — device side of the hydrogen-bond engine (mdx_hbond.hip).
//
// Result contract.
//
// Rows.  The incoming rows of a frame are n_rows distinct atoms.  Three int32 tables name rows: h_row[n_h], the
// hydrogens; d_row[n_h], the donor each hydrogen is bonded to, which may repeat (both hydrogens of a water molecule
// name one oxygen); a_row[n_a], the acceptors.  h_row holds no row twice, a_row holds no row twice, no row is both a
// hydrogen and an acceptor, and d_row[i] != h_row[i].  A donor may also be an acceptor.  Analysed frames are numbered
// f = 0, 1, ... in the order fed; `lags` is strictly increasing and non-negative; origin_step >= 1.
//
// Box and pair arithmetic: those of mdx_pairs_device.hpp.  For hydrogen i and acceptor j of frame f, with H, D, A the
// positions of h_row[i], d_row[i] and a_row[j]:
//
//     w_DA = min_image(A - D);  r2_DA = r2_of(w_DA)
//     w_HD = min_image(D - H);  w_HA = min_image(A - H)
//     dot  = (w_HDx*w_HAx + w_HDy*w_HAy) + w_HDz*w_HAz
//     c    = dot / sqrt(r2_of(w_HD) * r2_of(w_HA))       (one multiply, one correctly rounded sqrt, one correctly
//                                                        rounded divide)
//     inside_ij = r2_DA <= rc2  and  a_row[j] != d_row[i]
//     bond_ij   = inside_ij and c <= cos_max
//
// rc2 = distance * distance and cos_max are formed once on the host in float64.  c is the cosine of the angle
// D-H...A at the hydrogen: cos_max = cos(150 degrees) keeps angles of at least 150 degrees.  A NaN r2_DA is never
// inside.  A NaN c (a hydrogen on its donor or on the acceptor) is never a bond: an inside pair with NaN c adds 1 to
// `degenerate`.  c is evaluated only for inside pairs.  zero_dims drops components (w_c = +0.0) in all three vectors.
//
// Results, all integers (uint64 in HBM, handed out as int64), added with integer atomics only.  With B(f) the set of
// (i, j) with bond_ij at frame f:
//
//     bonds[f]            = |B(f)|                                       for every analysed frame
//     origin_counts[k], intermittent[k], continuous[k]
//                         per lag those of mdx_residence_device.hpp with C(f) replaced by B(f): origins are the
//                         multiples of origin_step, and the continuous form looks at every analysed frame in between
//     donated[m]          m = 0 ... max_neighbors: the (frame, hydrogen) cases with exactly m bonds, so that
//                         sum_m donated[m] == F * n_h
//     distance_counts[b]  every bond binned on r2_DA against a strictly increasing float64 table t[0 ... n_r]:
//                         b = #{ m in 1 ... n_r - 1 : r2_DA >= t[m] }; only the inner thresholds are compared
//     cosine_counts[b]    every bond binned on c by the rule of mdx_angle_device.hpp: strictly decreasing thresholds
//                         t[0 ... n_c], b = #{ m in 1 ... n_c - 1 : c <= t[m] }
//     degenerate          inside pairs with NaN c
//
// evaluations is the contract's count F * (n_h * n_a - #{(i, j) : a_row[j] == d_row[i]}), and
// sum distance_counts == sum cosine_counts == sum bonds.
//
// Capped lists (mdx_pairs_device.hpp).  A hydrogen holds at most max_neighbors (1 ... 64) bonds in one frame; a row
// that would hold more refuses the results (MDX_ERR_INVALID_VALUE, naming max_neighbors and the largest row) until a
// reset.  Exactly full is no error.
//
// Set membership, c and the bins are functions of the frame alone, and every tally is an integer add or max (atomics
// on integers commute): the numbers are the same whatever the input route, the index, the split into calls or slabs,
// the grid, or the arrival order of the atomics.  There is no floating-point atomic anywhere in this engine.
//
// Shape.  gather_kernel gathers the rows of a slab of incoming frames, component-major float32; positions live only
// as long as the slab in flight: the history is lists of acceptor numbers.
// hb_contact_kernel (the hot path, F * n_h * n_a evaluations) is the walk of mdx_pairs_device.hpp with z = the new
// frames, HB_TILE hydrogens per block, one per lane, and HB_JCHUNK acceptors per block.  A lane reads its H and its D
// from the slab through h_row / d_row, once, widened; the distance of the walk is taken from D.  The thread that stages
// acceptor j reads slab[a_row[j]] (an indexed read) and puts a_row[j], as a float64, into the fourth word of its stage
// entry, so that the exclusion a_row[j] != d_row[i] is one compare.  The rule tests r2_DA <= rc2 first, and only
// behind that test forms w_HD, w_HA and c: a miss costs the 14 float64 operations of the other pair engines.  A bond
// takes slot = atomicAdd(&len[f % cap][i], 1) and stores the acceptor's number j (not its row) at
// list[f % cap][slot][i] when slot < max_neighbors.  Each block adds its bonds to bonds[f] with one integer atomic,
// its largest row to max_row with one atomicMax and, where not zero, its degenerate pairs to `degenerate` with one
// integer atomic.
// hb_geometry_kernel runs after the contact kernel of the slab, one thread per (frame of the slab, hydrogen).  It
// reads the row's length (capped at max_neighbors; an overflowing row: the host refuses the results) and adds
// donated[len]; for every slot it re-derives r2_DA and c from the slab with the contract's own operations, so that
// nothing but acceptor numbers lives in HBM: the same inputs and the same operations give the bits the contact kernel
// saw.  Both bins come from binary searches over the inner thresholds.  With LDS_HIST (n_r <= HB_LDS_BINS and
// n_c <= HB_LDS_BINS) the thresholds and uint32 histograms live in LDS per block and are flushed with one uint64
// atomic per non-zero bin; otherwise the kernel counts in HBM directly, one uint64 atomic per bond, and reads the
// thresholds from HBM.  donated is counted in LDS in both forms.
//   The uint32 counters cannot wrap: a block is HB_GEO_THREADS = 256 (frame, hydrogen) cases of one launch, each of
//   which adds one donated count and at most HB_MAX_NEIGHBORS = 64 bonds: at most 256 x 64 = 16 384 adds to all the
//   counters of a histogram together.
// Lags: prs_walk_kernel<CONTINUOUS> of mdx_residence_device.hpp as it is, on rings of len / list / mask keyed by
// hydrogen, cap = max(lags) + the frames of a slab.
//
// No cell list and no spatial culling: every (hydrogen, acceptor) pair is evaluated.  Culling by cells is the
// follow-up.
#pragma once

#include "mdx_pairs_device.hpp"
#include "mdx_residence_device.hpp"

namespace mdx_hb_dev {

using namespace mdx_pairs_dev;

constexpr int HB_TILE = PAIR_TILE;            // hydrogens per block of the contact kernel, one per lane
constexpr int HB_THREADS = PAIR_THREADS;
constexpr int HB_STAGE = PAIR_STAGE;          // acceptors per LDS stage, one staged per thread
constexpr int HB_JCHUNK = 4 * HB_STAGE;       // acceptors per block
constexpr int HB_MAX_NEIGHBORS = PAIR_MAX_NEIGHBORS;    // slots of a row at most: one bit each in the alive mask
constexpr int64_t HB_SLAB_MAX = PAIR_SLAB_MAX;          // frames per launch, at most (grid z / y)
constexpr int HB_GEO_THREADS = 256;           // (frame, hydrogen) cases per block of the geometry kernel
constexpr int HB_LDS_BINS = 512;              // bins of either histogram at most for the LDS form

// the cosine at the hydrogen H of the angle D-H...A, from the two minimum-image vectors that start at H
__device__ __forceinline__ double hb_cosine(double hdx, double hdy, double hdz, double hax, double hay, double haz)
{
    const double dot = __dadd_rn(__dadd_rn(__dmul_rn(hdx, hax), __dmul_rn(hdy, hay)), __dmul_rn(hdz, haz));
    return __ddiv_rn(dot, __dsqrt_rn(__dmul_rn(r2_of(hdx, hdy, hdz), r2_of(hax, hay, haz))));
}

// The bonds of frame f = f_lo + blockIdx.z among the rows of slab frame blockIdx.z.  n_rows: rows of a slab frame.
// keep: bit c set -> component c takes part; ALL: keep == 7, known when compiled.  len: int32 [cap][n_h], zero for
// the new frames; list: int32 [cap][max_nb][n_h], acceptor numbers j; bonds: uint64 [F]; degenerate: one uint64.
template <bool ALL>
__global__ __launch_bounds__(HB_THREADS) void hb_contact_kernel(
    const float *__restrict__ slab, int64_t cap, int n_rows, int n_h, int n_a, const int *__restrict__ h_row,
    const int *__restrict__ d_row, const int *__restrict__ a_row, int n_jchunks, int64_t f_lo, PairBox box, int keep,
    double rc2, double cos_max, int max_nb, int *__restrict__ len, int *__restrict__ list,
    unsigned long long *__restrict__ bonds, int *__restrict__ max_row, unsigned long long *__restrict__ degenerate)
{
    __shared__ __attribute__((aligned(16))) double stage[4 * HB_STAGE];
    __shared__ unsigned int block_found, block_row, block_degenerate;
    const int64_t f = f_lo + blockIdx.z;
    const int tile = blockIdx.x / n_jchunks, chunk = blockIdx.x - tile * n_jchunks;
    const int i = tile * HB_TILE + threadIdx.x;
    const bool live = i < n_h;
    const float *__restrict__ frame = slab + int64_t(blockIdx.z) * 3 * n_rows;
    const int hr = h_row[live ? i : n_h - 1], dr = d_row[live ? i : n_h - 1];
    const double xh = (double)frame[hr], yh = (double)frame[n_rows + hr], zh = (double)frame[2 * int64_t(n_rows) + hr];
    const double xd = (double)frame[dr], yd = (double)frame[n_rows + dr], zd = (double)frame[2 * int64_t(n_rows) + dr];
    const double donor = (double)dr;            // beside the staged a_row[j]: the exclusion is one compare
    const int64_t slot_f = f % cap;
    int *__restrict__ my_len = len + slot_f * n_h + (live ? i : 0);
    int *__restrict__ my_list = list + slot_f * max_nb * n_h + (live ? i : 0);
    if (threadIdx.x == 0) {
        block_found = 0u;
        block_row = 0u;
        block_degenerate = 0u;
    }
    __syncthreads();
    unsigned int found = 0u, row = 0u, degen = 0u;
    const int j_begin = chunk * HB_JCHUNK;
    const int j_end = n_a - j_begin < HB_JCHUNK ? n_a : j_begin + HB_JCHUNK;
    for (int js = j_begin; js < j_end; js += HB_STAGE) {
        const int nj = j_end - js < HB_STAGE ? j_end - js : HB_STAGE;
        __syncthreads();                    // the stage is free
        if ((int)threadIdx.x < nj) {
            const int ar = a_row[js + threadIdx.x];
            stage[4 * threadIdx.x + 0] = (double)frame[ar];
            stage[4 * threadIdx.x + 1] = (double)frame[n_rows + ar];
            stage[4 * threadIdx.x + 2] = (double)frame[2 * int64_t(n_rows) + ar];
            stage[4 * threadIdx.x + 3] = (double)ar;
        }
        __syncthreads();
        if (!live)
            continue;
        stage_pairs<ALL>(stage, nj, js, -1, xd, yd, zd, box, keep,
                         [&](int jj, int j, double, double, double, double r2, bool) {
                             if (r2 <= rc2 && stage[4 * jj + 3] != donor) {
                                 double hdx, hdy, hdz, hax, hay, haz;
                                 min_image_of<ALL>(xd, yd, zd, xh, yh, zh, box, keep, hdx, hdy, hdz);
                                 min_image_of<ALL>(stage[4 * jj + 0], stage[4 * jj + 1], stage[4 * jj + 2], xh, yh, zh,
                                                   box, keep, hax, hay, haz);
                                 const double c = hb_cosine(hdx, hdy, hdz, hax, hay, haz);
                                 const bool bond = c <= cos_max;        // false for a NaN c
                                 degen += c != c;
                                 found += bond;
                                 if (bond)
                                     append_capped(my_len, my_list, n_h, max_nb, j, row);
                             }
                         });
    }
    for (int off = 32; off > 0; off >>= 1)
        degen += __shfl_down(degen, off);
    if ((threadIdx.x & 63) == 0 && degen)
        atomicAdd(&block_degenerate, degen);
    block_tally<true>(found, row, &block_found, &block_row, &bonds[f], max_row);     // its barrier: block_degenerate
    if (threadIdx.x == 0 && block_degenerate)
        atomicAdd(degenerate, (unsigned long long)block_degenerate);
}

// The geometry of the bonds of frame f = f_lo + blockIdx.y (slab frame blockIdx.y), hydrogen
// blockIdx.x * HB_GEO_THREADS + threadIdx.x.  inner_r: the n_r - 1 inner thresholds t[1] ... t[n_r - 1] of r2_DA in
// HBM, increasing; inner_c: the n_c - 1 inner thresholds of c, decreasing.  LDS_HIST: n_r <= HB_LDS_BINS and
// n_c <= HB_LDS_BINS.  distance_counts: uint64 [n_r]; cosine_counts: uint64 [n_c]; donated: uint64 [max_nb + 1].
template <bool LDS_HIST>
__global__ __launch_bounds__(HB_GEO_THREADS) void hb_geometry_kernel(
    const float *__restrict__ slab, int64_t cap, int n_rows, int n_h, const int *__restrict__ h_row,
    const int *__restrict__ d_row, const int *__restrict__ a_row, int64_t f_lo, PairBox box, int keep, int max_nb,
    const int *__restrict__ len, const int *__restrict__ list, const double *__restrict__ inner_r, int n_r,
    const double *__restrict__ inner_c, int n_c, unsigned long long *__restrict__ distance_counts,
    unsigned long long *__restrict__ cosine_counts, unsigned long long *__restrict__ donated)
{
    __shared__ double lds_r[LDS_HIST ? HB_LDS_BINS : 1], lds_c[LDS_HIST ? HB_LDS_BINS : 1];
    __shared__ unsigned int hist_r[LDS_HIST ? HB_LDS_BINS : 1], hist_c[LDS_HIST ? HB_LDS_BINS : 1];
    __shared__ unsigned int given[HB_MAX_NEIGHBORS + 1];
    const int t = threadIdx.x;
    if (LDS_HIST) {
        for (int m = t; m < n_r; m += HB_GEO_THREADS)
            hist_r[m] = 0u;
        for (int m = t; m < n_c; m += HB_GEO_THREADS)
            hist_c[m] = 0u;
        for (int m = t; m < n_r - 1; m += HB_GEO_THREADS)
            lds_r[m] = inner_r[m];
        for (int m = t; m < n_c - 1; m += HB_GEO_THREADS)
            lds_c[m] = inner_c[m];
    }
    if (t <= max_nb)
        given[t] = 0u;
    __syncthreads();
    const double *__restrict__ thr_r = LDS_HIST ? lds_r : inner_r;
    const double *__restrict__ thr_c = LDS_HIST ? lds_c : inner_c;
    const int i = blockIdx.x * HB_GEO_THREADS + t;
    if (i < n_h) {
        const float *__restrict__ frame = slab + int64_t(blockIdx.y) * 3 * n_rows;
        const int64_t slot_f = (f_lo + blockIdx.y) % cap;
        int m = len[slot_f * n_h + i];
        m = m > max_nb ? max_nb : m;
        atomicAdd(&given[m], 1u);
        if (m > 0) {
            const int hr = h_row[i], dr = d_row[i];
            const double xh = (double)frame[hr], yh = (double)frame[n_rows + hr],
                         zh = (double)frame[2 * int64_t(n_rows) + hr];
            const double xd = (double)frame[dr], yd = (double)frame[n_rows + dr],
                         zd = (double)frame[2 * int64_t(n_rows) + dr];
            double hdx, hdy, hdz;
            min_image_of<false>(xd, yd, zd, xh, yh, zh, box, keep, hdx, hdy, hdz);
            const int *__restrict__ my_list = list + slot_f * max_nb * n_h + i;
            for (int s = 0; s < m; ++s) {
                const int ar = a_row[my_list[int64_t(s) * n_h]];
                const double xa = (double)frame[ar], ya = (double)frame[n_rows + ar],
                             za = (double)frame[2 * int64_t(n_rows) + ar];
                double wx, wy, wz, hax, hay, haz;
                min_image_of<false>(xa, ya, za, xd, yd, zd, box, keep, wx, wy, wz);
                min_image_of<false>(xa, ya, za, xh, yh, zh, box, keep, hax, hay, haz);
                const double r2 = r2_of(wx, wy, wz);
                const double c = hb_cosine(hdx, hdy, hdz, hax, hay, haz);
                int lo = 0, hi = n_r - 1;       // the inner thresholds that are <= r2: a prefix, t increases
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (r2 >= thr_r[mid])
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                const int b_r = lo;
                lo = 0, hi = n_c - 1;           // the inner thresholds that are >= c: a prefix, t decreases
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (c <= thr_c[mid])
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                if (LDS_HIST) {
                    atomicAdd(&hist_r[b_r], 1u);
                    atomicAdd(&hist_c[lo], 1u);
                } else {
                    atomicAdd(&distance_counts[b_r], 1ull);
                    atomicAdd(&cosine_counts[lo], 1ull);
                }
            }
        }
    }
    __syncthreads();
    if (LDS_HIST) {
        for (int w = t; w < n_r; w += HB_GEO_THREADS)
            if (hist_r[w])
                atomicAdd(&distance_counts[w], (unsigned long long)hist_r[w]);
        for (int w = t; w < n_c; w += HB_GEO_THREADS)
            if (hist_c[w])
                atomicAdd(&cosine_counts[w], (unsigned long long)hist_c[w]);
    }
    if (t <= max_nb && given[t])
        atomicAdd(&donated[t], (unsigned long long)given[t]);
}

}  // namespace mdx_hb_dev
