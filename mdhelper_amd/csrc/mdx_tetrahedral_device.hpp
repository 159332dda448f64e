// mdx_tetrahedral_device.hpp — device side of the tetrahedral order engine (mdx_tetrahedral.hip).
//
// Result contract.
//
// Rows.  The rule of mdx_bond_order_device.hpp.  With `same` the candidates are the centres themselves: a frame
// delivers n0 rows, candidate j is row j, and j == i never counts.  Otherwise the incoming rows of a frame are the n0
// centres followed by the n1 candidates, two disjoint sets of atoms: candidate j = 0 ... n1 - 1 is row n0 + j.  One
// constant orthorhombic box, no dropped component (q is a quantity of three dimensions).
//
// Box and pair arithmetic: those of mdx_pairs_device.hpp, for centre i and candidate j of frame f, with w_ij and
// r2_ij its w and r2, float64, one operation at a time (the unit is built with contraction off).
//
// Candidates in range.  j is in range of i iff r2_ij <= rc2, rc2 = cutoff * cutoff formed once on the host.  A NaN r2
// is never in range.  m_i is the number of candidates in range of i in the frame.
//
// Total order.  The candidates of a centre are ordered by ascending r2 as float64, ties by ascending j.  The
// neighbours of i are the first min(k, m_i) candidates in range in that order, k = n_nearest, 4 <= k <= 8: a
// function of the frame alone, so chunking, grid and atomics cannot change it.
//
// Short centres.  A centre with m_i < 4 is short: its two values are NaN, it is not binned and adds nothing to the
// sums.  found[min(m_i, k)] takes every (frame, centre) case: sum found == F * n0.
//
// Values.  For a centre with at least four neighbours, a, b numbering them in the order above (0 ... 3):
//
//     r_a    = sqrt(r2_a)                                              (correctly rounded)
//     cos_ab = dot_ab / sqrt(r2_a * r2_b)
//     dot_ab = (w_ax*w_bx + w_ay*w_by) + w_az*w_bz                     (the angle engine's expression)
//     THIRD  = 1.0 / 3.0
//     acc    = +0.0;  for the pairs in the order (0,1) (0,2) (1,2) (0,3) (1,3) (2,3):
//                  t = cos_ab + THIRD;  acc = acc + t*t
//     q      = 1.0 - 0.375 * acc
//     sum    = ((+0.0 + r_0) + r_1 ...) + r_3
//     rbar   = sum * 0.25
//     v      = +0.0;  for a = 0 ... 3:  e = r_a - rbar;  v = v + e*e
//     S_k    = 1.0 - v / (12.0 * (rbar * rbar))
//
// q is the orientational tetrahedral order of Chau-Hardwick in the scaling of Errington-Debenedetti (1 for a regular
// tetrahedron, 0 on average for an ideal gas), S_k its translational counterpart.
//
// A neighbour on its centre.  A neighbour among the first four of a centre that is not short, with r2 == 0, has no
// direction: it is tallied in `degenerate` (an integer atomic) and the host refuses the results until a reset, as the
// bond-order engine does.
//
// Results.
//     q_counts[b], q_outside, s_counts[b], s_outside
//                          uint64, integer atomics, each quantity against its own increasing float64 table
//                          edges[0 ... n_bins] by the rule of boo_bin_kernel (mdx_bond_order_device.hpp):
//                          b = #{m in 1 ... n_bins - 1 : x >= edges[m]}, counted iff edges[0] <= x <= edges[n_bins],
//                          else outside
//                          (numpy.histogram(x, bins=edges), count for count)
//     distance_counts[a][b], distance_outside[a],  a = 0 ... k - 1
//                          rank a's r2 by the same rule against an increasing float64 table t[0 ... n_d] of r2 that the
//                          host builds from distance edges so that the counts equal numpy.histogram(sqrt(r2), edges);
//                          every (frame, centre) with m_i > a is counted: short centres take part here
//     found[m]             m = 0 ... k
//     sums[f][2]           float64 (q, S_k): per tile of 64 centres in row order from +0.0, then the tiles in tile
//                          order from +0.0, a short centre left out: the order of boo_sum_kernel
//     counted[f]           the centres of the frame with m_i >= 4
//     values[f][2][i]      float64, NaN for a short centre   } kept only where the host asks for them
//     neighbors[f][a][i]   int32, candidate numbers, -1 beyond m_i  }
// evaluations = F * (n0 * n1 - (same ? n0 : 0)).
//
// Reproducibility.  Every integer comes from integer atomics, every float64 from a fixed sequence of operations on the
// ordered list; there is no floating-point atomic.  The bits are the same across the three input routes, the index,
// any split into calls, slabs or candidate chunks, and after a reset.
//
// Shape.  Per slab of frames; a frame never needs another.
//
// Phase 1, tet_select_kernel<K> (the hot path, F * n0 * n1 evaluations).  gather_kernel, then the walk of
// mdx_pairs_device.hpp with z = frames and `chunk` candidates per block, one centre per lane.  Each lane keeps its K
// best (r2, j) in registers, sorted; the registers are indexed with compile-time constants only (tet_insert, a fully
// unrolled compare-and-shift chain with K a template parameter: a runtime index would send the arrays through scratch,
// see the comment at ang_bound in mdx_angle_device.hpp).  The common path is one comparison, r2 < bound, in the same
// condition as `other`.  bound starts as the smallest float64 above rc2 (the host passes nextafter(rc2, inf), so the
// test is r2 <= rc2 exactly); once the lane's list is full, bound is its K-th r2.  j only ascends during a lane's
// walk, so the strict < of the test and of the shift chain IS the tie rule: an equal r2 of a later j never displaces.
// A block writes its lanes' lists as indices only, int32 [slab][chunk][K][n0], slot-major, -1 for an empty slot: the
// layout of the capped lists.  Nothing but indices lives in HBM; the later kernels re-derive w and r2 from the slab
// with the contract's operations, as ang_triplet_kernel does.
//
// Candidate chunks are a launch decision (tet_chunk_for in mdx_tetrahedral.hip): by record statistics a lane's bound
// drops about K / t times at step t of its walk, a wave has an insert in about min(1, 64 K / t) of its steps, and
// every new chunk starts that count again.  One chunk wherever i tiles x slab frames fills the device's compute
// units; only below that are the candidates split, in multiples of the stage.
//
// Phase 2, tet_finish_kernel<K>, one lane per (frame, centre).  Merges the C >= 1 chunk lists in chunk order with the
// same tet_insert on a re-derived r2: chunk order is ascending j, and inside a chunk equal r2 arrive in ascending j,
// so the strict < keeps the tie rule.  Forms q and S_k, writes the values and, when kept, the neighbours, and tallies
// found, degenerate, counted and the distance histograms.
//   Where the switch is: with n_d <= TET_LDS_BINS the table and one uint32 histogram [K][n_d] per block live in LDS
//   (a block adds at most TET_THREADS * K to all its counters together, so they cannot wrap) and leave with one uint64
//   atomic per non-zero word.  One histogram per block rather than per wave: K = 8 rows of 1024 bins for four waves
//   would not fit the 64 KiB of a block.  Beyond TET_LDS_BINS the kernel counts in HBM directly, one uint64 atomic per
//   value, and reads the table from HBM.
//
// Phase 3.  tet_bin_kernel and tet_sum_kernel: the rules of boo_bin_kernel and boo_sum_kernel.  The unit has its own
// because mdx_bond_order_device.hpp also defines kernels that are no templates, which a second unit of the library
// cannot include (their host stubs would be defined twice).  tet_bin_kernel takes one quantity per launch, each
// against its own table: a block takes TET_BIN_CHUNK consecutive (frame, centre) values, every wave counts into its
// own uint32 histogram in LDS (a block adds at most TET_BIN_CHUNK to all its counters together), the edges sit in LDS
// too, and the block sends the non-zero sums to the uint64 counts with one integer atomic each; beyond TET_LDS_BINS it
// counts in HBM directly, one uint64 atomic per value.  tet_sum_kernel: one block per (frame, quantity); its waves
// take the frame's tiles four at a time, lane 0 of a wave adds its tile in row order, thread 0 adds the partials in
// tile order.
//
// No cell list and no spatial culling: every (centre, candidate) pair is evaluated.
#pragma once

#include "mdx_pairs_device.hpp"

namespace mdx_tet_dev {

using namespace mdx_pairs_dev;

constexpr int TET_TILE = PAIR_TILE;           // centres per block of phase 1, one per lane
constexpr int TET_THREADS = PAIR_THREADS;
constexpr int TET_STAGE = PAIR_STAGE;         // candidates per LDS stage; a chunk is a multiple of it
constexpr int TET_MIN_NEAREST = 4;            // what q and S_k need
constexpr int TET_MAX_NEAREST = 8;            // the largest k
constexpr int TET_WAVES = PAIR_WAVES;
constexpr int TET_LDS_BINS = 1024;            // bins at most for a histogram and its table in LDS
constexpr int TET_SUM_TILE = 64;              // centres per tile of the frame sums
constexpr int TET_BIN_CHUNK = 16384;          // values a block of the bin kernel takes: the bound of its counters
constexpr int64_t TET_SLAB_MAX = PAIR_SLAB_MAX;         // frames per launch, at most (grid y / z)

__device__ __forceinline__ double tet_nan()
{
    return __longlong_as_double(0x7ff8000000000000ll);
}

__device__ __forceinline__ double tet_inf()
{
    return __longlong_as_double(0x7ff0000000000000ll);
}

// (r2, j) into the sorted list (r[s], n[s]), s = 0 ... K - 1, behind every entry with r[s] <= r2; the last entry
// falls off.  The caller has tested r2 < r[K - 1] or the list is not full (its empty slots hold +inf, -1).
template <int K>
__device__ __forceinline__ void tet_insert(double (&r)[K], int (&n)[K], double r2, int j)
{
#pragma unroll
    for (int s = K - 1; s > 0; --s) {
        const bool shift = r2 < r[s - 1];       // the entry below moves up into slot s
        const bool here = r2 < r[s];
        r[s] = shift ? r[s - 1] : here ? r2 : r[s];
        n[s] = shift ? n[s - 1] : here ? j : n[s];
    }
    const bool first = r2 < r[0];
    r[0] = first ? r2 : r[0];
    n[0] = first ? j : n[0];
}

// The K nearest candidates in range of every centre among the candidates of chunk blockIdx.x % n_chunks, slab frame
// blockIdx.z.  n_rows: rows of a slab frame; the n1 candidates start at row off (0 with same).  chunk: candidates per
// block, a multiple of TET_STAGE.  bound0: the smallest float64 above rc2.  list: int32 [slab][n_chunks][K][n0].
template <int K>
__global__ __launch_bounds__(TET_THREADS) void tet_select_kernel(
    const float *__restrict__ slab, int n_rows, int n0, int n1, int off, int same, int n_chunks, int chunk,
    PairBox box, double bound0, int *__restrict__ list)
{
    __shared__ __attribute__((aligned(16))) double stage[4 * TET_STAGE];
    const int64_t fs = blockIdx.z;
    const int tile = blockIdx.x / n_chunks, c = blockIdx.x - tile * n_chunks;
    const int i = tile * TET_TILE + threadIdx.x;
    const bool live = i < n0;
    const float *__restrict__ a = slab + fs * 3 * n_rows + (live ? i : n0 - 1);
    const float *__restrict__ b = slab + fs * 3 * n_rows + off;
    const double xi = (double)a[0], yi = (double)a[n_rows], zi = (double)a[2 * int64_t(n_rows)];
    double best_r2[K];
    int best_j[K];
#pragma unroll
    for (int s = 0; s < K; ++s) {
        best_r2[s] = tet_inf();
        best_j[s] = -1;
    }
    double bound = bound0;
    const int j_begin = c * chunk;
    const int j_end = n1 - j_begin < chunk ? n1 : j_begin + chunk;
    for (int js = j_begin; js < j_end; js += TET_STAGE) {
        const int nj = j_end - js < TET_STAGE ? j_end - js : TET_STAGE;
        __syncthreads();                    // the stage is free
        if ((int)threadIdx.x < nj)
            stage_partners(stage, b, n_rows, js);
        __syncthreads();
        if (!live)
            continue;
        const int skip = same ? i - js : -1;        // the stage entry that is this lane's own row
        stage_pairs<true>(stage, nj, js, skip, xi, yi, zi, box, 7,
                          [&](int, int j, double, double, double, double r2, bool other) {
                              if (r2 < bound && other) {
                                  tet_insert<K>(best_r2, best_j, r2, j);
                                  bound = best_r2[K - 1] < bound ? best_r2[K - 1] : bound;
                              }
                          });
    }
    if (!live)
        return;
    int *__restrict__ out = list + ((fs * n_chunks + c) * K) * n0 + i;
#pragma unroll
    for (int s = 0; s < K; ++s)
        out[int64_t(s) * n0] = best_j[s];
}

// One lane per (slab frame blockIdx.y, centre): merges the centre's n_chunks lists, forms q and S_k, and tallies.
// table: the n_d + 1 thresholds of r2 in HBM, increasing; LDS_HIST: n_d <= TET_LDS_BINS.  values: float64
// [slab][2][n0]; neighbors: int32 [slab][K][n0] or nullptr.  distance_counts: uint64 [K][n_d]; distance_outside:
// uint64 [K]; found: uint64 [K + 1]; degenerate: uint64 [1]; counted: uint64 [frames], frame f0 + blockIdx.y.
template <int K, bool LDS_HIST>
__global__ __launch_bounds__(TET_THREADS) void tet_finish_kernel(
    const float *__restrict__ slab, int n_rows, int n0, int off, PairBox box, int n_chunks,
    const int *__restrict__ list, const double *__restrict__ table, int n_d, int64_t f0,
    double *__restrict__ values, int *__restrict__ neighbors, unsigned long long *__restrict__ distance_counts,
    unsigned long long *__restrict__ distance_outside, unsigned long long *__restrict__ found,
    unsigned long long *__restrict__ degenerate, unsigned long long *__restrict__ counted)
{
    __shared__ double lds_table[LDS_HIST ? TET_LDS_BINS + 1 : 1];
    __shared__ unsigned int hist[LDS_HIST ? K * TET_LDS_BINS : 1];
    __shared__ unsigned int block_outside[K], block_found[K + 1], block_degenerate, block_counted;
    const int t = threadIdx.x;
    const int64_t fs = blockIdx.y;
    const int i = blockIdx.x * TET_THREADS + t;
    if (LDS_HIST) {
        for (int w = t; w < K * n_d; w += TET_THREADS)
            hist[(w / n_d) * TET_LDS_BINS + w % n_d] = 0u;
        for (int m = t; m <= n_d; m += TET_THREADS)
            lds_table[m] = table[m];
    }
    if (t < K)
        block_outside[t] = 0u;
    if (t <= K)
        block_found[t] = 0u;
    if (t == 0)
        block_degenerate = block_counted = 0u;
    __syncthreads();
    if (i < n0) {
        const float *__restrict__ frame = slab + fs * 3 * n_rows;
        const double xi = (double)frame[i], yi = (double)frame[n_rows + i], zi = (double)frame[2 * int64_t(n_rows) + i];
        double best_r2[K];
        int best_j[K];
#pragma unroll
        for (int s = 0; s < K; ++s) {
            best_r2[s] = tet_inf();
            best_j[s] = -1;
        }
        const int *__restrict__ mine = list + fs * n_chunks * K * n0 + i;
        for (int c = 0; c < n_chunks; ++c)
            for (int s = 0; s < K; ++s) {
                const int j = mine[(int64_t(c) * K + s) * n0];
                if (j < 0)
                    break;
                const float *__restrict__ src = frame + off + j;
                double wx, wy, wz;
                min_image_of<true>((double)src[0], (double)src[n_rows], (double)src[2 * int64_t(n_rows)], xi, yi, zi,
                                   box, 7, wx, wy, wz);
                const double r2 = r2_of(wx, wy, wz);
                if (r2 < best_r2[K - 1])
                    tet_insert<K>(best_r2, best_j, r2, j);
            }
        int m = 0;
#pragma unroll
        for (int s = 0; s < K; ++s)
            m += best_j[s] >= 0;
        atomicAdd(&block_found[m], 1u);
        if (neighbors) {
            int *__restrict__ out = neighbors + fs * K * n0 + i;
#pragma unroll
            for (int s = 0; s < K; ++s)
                out[int64_t(s) * n0] = best_j[s];
        }
        // rank a's r2 into its row of the distance histogram
        const double *__restrict__ e = LDS_HIST ? lds_table : table;
        const double lowest = e[0], highest = e[n_d];
#pragma unroll
        for (int a = 0; a < K; ++a) {
            if (a >= m)
                continue;
            const double x = best_r2[a];
            if (!(x >= lowest && x <= highest)) {
                atomicAdd(&block_outside[a], 1u);
                continue;
            }
            int lo = 0, hi = n_d - 1;           // the inner thresholds that are <= x: a prefix, the table increases
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (x >= e[mid + 1])
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (LDS_HIST)
                atomicAdd(&hist[a * TET_LDS_BINS + lo], 1u);
            else
                atomicAdd(&distance_counts[int64_t(a) * n_d + lo], 1ull);
        }
        double q = tet_nan(), sk = tet_nan();
        if (m >= TET_MIN_NEAREST) {
            double wx[4], wy[4], wz[4], r[4];
            unsigned int zero = 0u;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float *__restrict__ src = frame + off + best_j[a];
                min_image_of<true>((double)src[0], (double)src[n_rows], (double)src[2 * int64_t(n_rows)], xi, yi, zi,
                                   box, 7, wx[a], wy[a], wz[a]);
                r[a] = __dsqrt_rn(best_r2[a]);
                zero += best_r2[a] == 0.0;
            }
            const double third = 1.0 / 3.0;
            double acc = 0.0;
#pragma unroll
            for (int bb = 1; bb < 4; ++bb)
#pragma unroll
                for (int aa = 0; aa < bb; ++aa) {
                    const double dot = __dadd_rn(__dadd_rn(__dmul_rn(wx[aa], wx[bb]), __dmul_rn(wy[aa], wy[bb])),
                                                 __dmul_rn(wz[aa], wz[bb]));
                    const double c = __ddiv_rn(dot, __dsqrt_rn(__dmul_rn(best_r2[aa], best_r2[bb])));
                    const double u = __dadd_rn(c, third);
                    acc = __dadd_rn(acc, __dmul_rn(u, u));
                }
            q = __dsub_rn(1.0, __dmul_rn(0.375, acc));
            double sum = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
                sum = __dadd_rn(sum, r[a]);
            const double rbar = __dmul_rn(sum, 0.25);
            double v = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const double d = __dsub_rn(r[a], rbar);
                v = __dadd_rn(v, __dmul_rn(d, d));
            }
            sk = __dsub_rn(1.0, __ddiv_rn(v, __dmul_rn(12.0, __dmul_rn(rbar, rbar))));
            atomicAdd(&block_counted, 1u);
            if (zero)
                atomicAdd(&block_degenerate, zero);
        }
        values[(fs * 2 + 0) * n0 + i] = q;
        values[(fs * 2 + 1) * n0 + i] = sk;
    }
    __syncthreads();
    if (LDS_HIST)
        for (int w = t; w < K * n_d; w += TET_THREADS) {
            const int a = w / n_d, bin = w - a * n_d;
            const unsigned int sum = hist[a * TET_LDS_BINS + bin];
            if (sum)
                atomicAdd(&distance_counts[int64_t(a) * n_d + bin], (unsigned long long)sum);
        }
    if (t < K && block_outside[t])
        atomicAdd(&distance_outside[t], (unsigned long long)block_outside[t]);
    if (t <= K && block_found[t])
        atomicAdd(&found[t], (unsigned long long)block_found[t]);
    if (t == 0 && block_counted)
        atomicAdd(&counted[f0 + fs], (unsigned long long)block_counted);
    if (t == 0 && block_degenerate)
        atomicAdd(degenerate, (unsigned long long)block_degenerate);
}

// Quantity `which` (0: q, 1: S_k) of the values [frames][2][n0] of a slab into its histogram.  grid x: chunks of
// TET_BIN_CHUNK consecutive (frame, centre) numbers v = frame * n0 + i < n_values.  edges: float64 [n_bins + 1] in
// HBM.  LDS_HIST: n_bins <= TET_LDS_BINS.  counts: uint64 [n_bins]; outside: uint64 [1].
template <bool LDS_HIST>
__global__ __launch_bounds__(TET_THREADS) void tet_bin_kernel(
    const double *__restrict__ values, int64_t n_values, int n0, int which, const double *__restrict__ edges,
    int n_bins, unsigned long long *__restrict__ counts, unsigned long long *__restrict__ outside)
{
    __shared__ double lds_edges[LDS_HIST ? TET_LDS_BINS + 1 : 1];
    __shared__ unsigned int hist[LDS_HIST ? TET_WAVES * TET_LDS_BINS : 1];
    __shared__ unsigned int block_outside;
    const int t = threadIdx.x;
    if (LDS_HIST) {
        for (int w = t; w < TET_WAVES * n_bins; w += TET_THREADS)
            hist[(w / n_bins) * TET_LDS_BINS + w % n_bins] = 0u;
        for (int m = t; m <= n_bins; m += TET_THREADS)
            lds_edges[m] = edges[m];
    }
    if (t == 0)
        block_outside = 0u;
    __syncthreads();
    const double *__restrict__ e = LDS_HIST ? lds_edges : edges;
    unsigned int *__restrict__ my_hist = hist + (LDS_HIST ? (t >> 6) * TET_LDS_BINS : 0);
    const double lowest = e[0], highest = e[n_bins];
    const int64_t v0 = int64_t(blockIdx.x) * TET_BIN_CHUNK;
    const int64_t v1 = n_values - v0 < TET_BIN_CHUNK ? n_values : v0 + TET_BIN_CHUNK;
    for (int64_t v = v0 + t; v < v1; v += TET_THREADS) {
        const int64_t f = v / n0;
        const double x = values[(f * 2 + which) * n0 + (v - f * n0)];
        if (x != x)                         // a short centre
            continue;
        if (!(x >= lowest && x <= highest)) {
            atomicAdd(&block_outside, 1u);
            continue;
        }
        int lo = 0, hi = n_bins - 1;        // the inner edges that are <= x: a prefix, the edges increase
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (x >= e[mid + 1])
                lo = mid + 1;
            else
                hi = mid;
        }
        if (LDS_HIST)
            atomicAdd(&my_hist[lo], 1u);
        else
            atomicAdd(&counts[lo], 1ull);
    }
    __syncthreads();
    if (LDS_HIST)
        for (int w = t; w < n_bins; w += TET_THREADS) {
            unsigned int sum = 0u;
            for (int v = 0; v < TET_WAVES; ++v)
                sum += hist[v * TET_LDS_BINS + w];
            if (sum)
                atomicAdd(&counts[w], (unsigned long long)sum);
        }
    if (t == 0 && block_outside)
        atomicAdd(outside, (unsigned long long)block_outside);
}

// sums[f0 + frame][which] of a slab: block blockIdx.x = frame * 2 + which adds the n0 values of its row of `values`,
// per tile of TET_SUM_TILE in row order from +0.0 (a NaN, a short centre, is left out), then the tiles in tile order
// from +0.0.
__global__ __launch_bounds__(TET_THREADS) void tet_sum_kernel(const double *__restrict__ values, int n0, int64_t f0,
                                                              double *__restrict__ sums)
{
    __shared__ double buf[TET_WAVES][TET_SUM_TILE];
    __shared__ double part[TET_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double *__restrict__ in = values + int64_t(blockIdx.x) * n0;
    const int n_tiles = (n0 + TET_SUM_TILE - 1) / TET_SUM_TILE;
    double total = 0.0;
    for (int t0 = 0; t0 < n_tiles; t0 += TET_WAVES) {
        const int64_t i = int64_t(t0 + w) * TET_SUM_TILE + lane;
        buf[w][lane] = i < n0 ? in[i] : tet_nan();
        __syncthreads();
        if (lane == 0) {
            double s = 0.0;
            for (int k = 0; k < TET_SUM_TILE; ++k) {
                const double x = buf[w][k];
                if (x == x)
                    s = __dadd_rn(s, x);
            }
            part[w] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int v = 0; v < TET_WAVES && t0 + v < n_tiles; ++v)
                total = __dadd_rn(total, part[v]);
    }
    if (threadIdx.x == 0)
        sums[f0 * 2 + blockIdx.x] = total;
}

}  // namespace mdx_tet_dev
