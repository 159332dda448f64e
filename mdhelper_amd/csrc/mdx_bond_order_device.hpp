// mdx_bond_order_device.hpp — device side of the bond-orientational order engine (mdx_bond_order.hip).
//
// Result contract.
//
// Rows.  With `same` the neighbour candidates are the centres themselves: a frame delivers n0 rows, candidate j is
// row j, and j == i never counts.  Otherwise the incoming rows of a frame are the n0 centres followed by the n1
// candidates, two disjoint sets of atoms: candidate j = 0 ... n1 - 1 is row n0 + j.  One cutoff, one constant
// orthorhombic box, no dropped component (q_l is a quantity of three dimensions).
//
// Box and pair arithmetic: those of mdx_pairs_device.hpp, for centre i and candidate j of frame f, with w_ij and
// r2_ij its w and r2:
//
//     j is a neighbour of i  iff  r2_ij <= rc2,  rc2 = cutoff * cutoff formed once on the host
//
// A NaN r2 is never a neighbour.  m_i is the number of neighbours of i in the frame.
//
// Per bond (i, j) and requested degree l, float64, one operation at a time (the unit is built with contraction off):
//
//     r = sqrt(r2);  ux = wx / r;  uy = wy / r;  uz = wz / r                  (correctly rounded sqrt and divides)
//     (c_0, s_0) = (1, 0);  c_m = c_{m-1}*ux - s_{m-1}*uy;  s_m = c_{m-1}*uy + s_{m-1}*ux             m = 1 ... l
//     T_m^m     = (2m - 1)!!                                                  (exact in float64 up to m = 12)
//     T_{m+1}^m = ((2m + 1) * uz) * T_m^m
//     T_n^m     = (a[n][m] * uz) * T_{n-1}^m - b[n][m] * T_{n-2}^m            n = m + 2 ... l
//     y = N[l][m] * T_l^m;  term_re = y * c_m;  term_im = y * s_m             m = 0 ... l
//
// which is Y_lm of the bond's direction with the Condon-Shortley phase (scipy.special.sph_harm_y): c_m + i s_m is
// (ux + i uy)^m = sin^m(theta) e^{i m phi}, and T_n^m is the associated Legendre function without that factor and
// without its sign.  The kernel forms, for m = 0, 1, ... l in turn, (c_m, s_m) from (c_{m-1}, s_{m-1}), then the T
// of that m upwards in n, then y and the two terms: no operation takes an operand from another order, so this is the
// order of the text above.  Only m >= 0 is formed: the weights are real, so q_{l,-m} = (-1)^m conj(q_{l,m}).
// term_im of m = 0 is y * 0 and is not kept.
//
// Host tables (BooTables, float64, part of the contract): from exact integers, one division each,
//
//     a[n][m] = double(2n - 1) / double(n - m);   b[n][m] = double(n + m - 1) / double(n - m)
//     FOUR_PI = 4.0 * 3.141592653589793   (exact: a power of two times the float64 nearest to pi)
//     N[l][m] = (-1)^m sqrt(double(2l + 1) / (FOUR_PI * double(P))),   P = (l + m)! / (l - m)! as an exact integer,
//               double(P) correctly rounded (P < 2^80; its odd part is below 2^64 and is widened, the power of two
//               is applied with ldexp)
//     k[l]    = FOUR_PI / double(2l + 1)
//
// Per centre i with m_i >= 1 neighbours and degree l:
//
//     Q_lm(i) = the terms of the neighbours j of i IN ASCENDING j, added one after the other from +0.0, re and im apart
//     q_lm(i) = Q_lm(i) / double(m_i)
//     S = q_l0.re*q_l0.re;  for m = 1 ... l:  S = S + 2.0 * (q_lm.re*q_lm.re + q_lm.im*q_lm.im)
//     q_l(i) = sqrt(k[l] * S)
//
// and with `averaged` (same only; Lechner-Dellago):
//
//     A_lm(i) = q_lm(i), then + q_lm(j) for the neighbours j of i in ascending j
//     qbar_lm(i) = A_lm(i) / double(m_i + 1);   qbar_l(i) from qbar_lm by the same S and sqrt
//
// The minimum image is bit-symmetric in i and j (d changes sign, rint is odd), so every neighbour j of i has i among
// its own: m_j >= 1.
//
// Ascending j.  The contact kernel appends to a centre's row in the order its atomics arrive, so a row is a function
// of the frame only as a set.  boo_rows_kernel sorts the at most 64 entries of every row in place (an insertion sort
// by the lane that owns the row), and every later kernel walks the slots in order: the float64 sums are then a
// function of the set.  There is no floating-point atomic anywhere in this engine.
//
// Isolated and degenerate centres.  A centre with m_i == 0 is isolated: its values are NaN, it is not binned and adds
// nothing to the sums.  A neighbour on top of its centre (r2 == 0: u = 0 / 0) is data without a direction: it is
// tallied in `degenerate` (an integer atomic) and the host refuses the results until a reset.  A row beyond
// max_neighbors (1 ... 64) refuses them through CappedLists::check (mdx_pairs_host.hpp); exactly full is no error.
//
// Results.  D requested degrees (1 <= l <= 12, at most 4, distinct), K = 2 with `averaged`, else 1; k = 0 is q_l,
// k = 1 is qbar_l.
//     counts[d][k][b]      uint64, integer atomics: a histogram over all (frame, centre) pairs against an increasing
//                          float64 table edges[0 ... n_bins]: b = #{m in 1 ... n_bins - 1 : q >= edges[m]}; a value is
//                          counted iff edges[0] <= q <= edges[n_bins], else it adds 1 to outside[d][k]
//                          (numpy.histogram(q, bins=edges), count for count)
//     coordination[m]      m = 0 ... max_neighbors: the (frame, centre) cases with exactly m neighbours; sums to F * n0
//     sums[f][d][k]        float64: the values of the frame's centres, added per tile of 64 centres in row order from
//                          +0.0, then the tiles in tile order from +0.0 (the order of mdx_orient_device.hpp's frame
//                          sums); an isolated centre is left out of its tile's sum
//     counted[f]           the centres of the frame with m_i >= 1
//     values[f][d][k][i]   float64, NaN for an isolated centre (kept only where the host asks for them)
// evaluations = F * (n0 * n1 - (same ? n0 : 0)); bonds = the list entries = sum m * coordination[m].
//
// The lists are a function of the frame alone as sets, every float64 result a function of the sorted row by a fixed
// sequence of operations, and every tally an integer add or max: the bits are the same whatever the input route, the
// index, the split into calls or slabs, the grid, or the arrival order of the atomics.
//
// Shape.  Per slab of frames; a frame never needs another.
//
// Phase 1, lists (the hot path, F * n0 * n1 evaluations).  gather_kernel, then boo_contact_kernel: the walk of
// mdx_pairs_device.hpp with z = frames and BOO_JCHUNK candidates per block, the uniform-cutoff form of
// ang_contact_kernel with its own loop over the stages (NOTES.md, round 10), append_capped into slot-major lists and
// the max-only block_tally.  boo_rows_kernel, one lane per (frame, centre): sorts the row, re-derives w of every
// entry to count the degenerate ones, and tallies coordination and counted once for all degrees.
//
// Phase 2, boo_qlm_kernel<L>, one launch per requested degree with the degree a template parameter: the recurrences
// unroll fully and the 2L + 1 accumulators stay in registers (a runtime degree would index them through scratch).
// One lane per (frame, centre); the slot-major list gives consecutive lanes consecutive words.  w is re-derived from
// the slab with the contract's own operations, as ang_triplet_kernel does, so nothing but indices lives in HBM.  It
// writes q_lm component-major, qlm[f][component][i] with component 0 = re of m = 0, 2m - 1 = re and 2m = im of
// m >= 1, and q_l into the slab's values.  The tables come through a pointer with indices known when compiled.
//
// Phase 3, boo_average_kernel<L> (averaged only): the same lanes; reads the neighbours' q_lm of the frame from the
// buffer in ascending j (scattered reads of 8 (2L + 1) bytes per neighbour out of L2) and writes qbar_l.
//
// Phase 4.  boo_bin_kernel: a block takes BOO_BIN_CHUNK consecutive (frame, centre) values of one (d, k).  Each wave
// counts into its own uint32 histogram in LDS, the edges sit in LDS too, and the block sends the non-zero sums to
// the uint64 counts with one integer atomic each.
//   The uint32 counters cannot wrap: a block adds at most BOO_BIN_CHUNK = 16 384 values to all its counters together.
//   Where the switch is: the LDS form needs n_bins <= BOO_LDS_BINS (1024).  Beyond it the same kernel counts in HBM
//   directly, one uint64 atomic per value, and reads the edges from HBM, as the angle and van Hove engines do.
// boo_sum_kernel: one block per (frame, d, k); its waves take the frame's tiles four at a time, lane 0 of a wave adds
// its tile in row order, thread 0 adds the partials in tile order.
//
// No cell list and no spatial culling: every (centre, candidate) pair is evaluated.
#pragma once

#include "mdx_pairs_device.hpp"

namespace mdx_boo_dev {

using namespace mdx_pairs_dev;

constexpr int BOO_TILE = PAIR_TILE;           // centres per block of phase 1, one per lane
constexpr int BOO_THREADS = PAIR_THREADS;
constexpr int BOO_WAVES = PAIR_WAVES;
constexpr int BOO_STAGE = PAIR_STAGE;         // candidates per LDS stage, one staged per thread
constexpr int BOO_JCHUNK = 4 * BOO_STAGE;     // candidates per block
constexpr int BOO_MAX_NEIGHBORS = PAIR_MAX_NEIGHBORS;   // slots of a row at most
constexpr int BOO_MAX_DEGREE = 12;            // the largest l
constexpr int BOO_MAX_DEGREES = 4;            // degrees per engine at most
constexpr int BOO_TABLE = BOO_MAX_DEGREE + 1;
constexpr int BOO_SUM_TILE = 64;              // centres per tile of the frame sums
constexpr int BOO_LDS_BINS = 1024;            // n_bins at most for the histogram and the edges in LDS
constexpr int BOO_BIN_CHUNK = 16384;          // values a block of the bin kernel takes: the bound of its counters
constexpr int64_t BOO_SLAB_MAX = PAIR_SLAB_MAX;         // frames per launch, at most (grid y / z)

// the host tables of the contract, in HBM; entries outside n > m + 1 (a, b) and m <= l (norm) are zero
struct BooTables {
    double a[BOO_TABLE][BOO_TABLE], b[BOO_TABLE][BOO_TABLE], norm[BOO_TABLE][BOO_TABLE], k[BOO_TABLE];
};

// (2m - 1)!!, exact in float64 for m <= 12
__host__ __device__ constexpr double boo_double_factorial(int m)
{
    double p = 1.0;
    for (int k = 1; k <= m; ++k)
        p *= double(2 * k - 1);
    return p;
}

__device__ __forceinline__ double boo_nan()
{
    return __longlong_as_double(0x7ff8000000000000ll);
}

// The neighbour lists of slab frame blockIdx.z.  n_rows: rows of a slab frame; the n1 candidates start at row off
// (0 with same).  len: int32 [slab][n0], zero; list: int32 [slab][max_nb][n0], candidate numbers j.
__global__ __launch_bounds__(BOO_THREADS) void boo_contact_kernel(
    const float *__restrict__ slab, int n_rows, int n0, int n1, int off, int same, int n_jchunks, PairBox box,
    double rc2, int max_nb, int *__restrict__ len, int *__restrict__ list, int *__restrict__ max_row)
{
    __shared__ __attribute__((aligned(16))) double stage[4 * BOO_STAGE];
    __shared__ unsigned int block_row;
    const int64_t fs = blockIdx.z;
    const int tile = blockIdx.x / n_jchunks, chunk = blockIdx.x - tile * n_jchunks;
    const int i = tile * BOO_TILE + threadIdx.x;
    const bool live = i < n0;
    const float *__restrict__ a = slab + fs * 3 * n_rows + (live ? i : n0 - 1);
    const float *__restrict__ b = slab + fs * 3 * n_rows + off;
    const double xi = (double)a[0], yi = (double)a[n_rows], zi = (double)a[2 * int64_t(n_rows)];
    int *__restrict__ my_len = len + fs * n0 + (live ? i : 0);
    int *__restrict__ my_list = list + fs * max_nb * n0 + (live ? i : 0);
    if (threadIdx.x == 0)
        block_row = 0u;
    unsigned int row = 0u;
    const int j_begin = chunk * BOO_JCHUNK;
    const int j_end = n1 - j_begin < BOO_JCHUNK ? n1 : j_begin + BOO_JCHUNK;
    for (int js = j_begin; js < j_end; js += BOO_STAGE) {
        const int nj = j_end - js < BOO_STAGE ? j_end - js : BOO_STAGE;
        __syncthreads();                    // the stage is free
        if ((int)threadIdx.x < nj)
            stage_partners(stage, b, n_rows, js);
        __syncthreads();
        if (!live)
            continue;
        const int skip = same ? i - js : -1;        // the stage entry that is this lane's own row
        stage_pairs<true>(stage, nj, js, skip, xi, yi, zi, box, 7,
                          [&](int, int j, double, double, double, double r2, bool other) {
                              if (r2 <= rc2 && other)
                                  append_capped(my_len, my_list, n0, max_nb, j, row);
                          });
    }
    __syncthreads();                        // block_row is zero (no stage at all: the barrier above never ran)
    block_tally<false>(0u, row, nullptr, &block_row, nullptr, max_row);
}

// One lane per (slab frame blockIdx.y, centre): sorts the row into ascending j in place, counts its entries with
// r2 == 0, and tallies coordination[m], counted[f0 + frame] and degenerate through uint32 words in LDS (a block adds
// at most BOO_THREADS rows and BOO_THREADS * 64 entries) and one integer atomic per non-zero word.
__global__ __launch_bounds__(BOO_THREADS) void boo_rows_kernel(
    const float *__restrict__ slab, int n_rows, int n0, int off, PairBox box, int max_nb,
    const int *__restrict__ len, int *__restrict__ list, int64_t f0, unsigned long long *__restrict__ coordination,
    unsigned long long *__restrict__ degenerate, unsigned long long *__restrict__ counted)
{
    __shared__ unsigned int coord[BOO_MAX_NEIGHBORS + 1];
    __shared__ unsigned int block_degenerate, block_counted;
    const int t = threadIdx.x;
    const int64_t fs = blockIdx.y;
    const int i = blockIdx.x * BOO_THREADS + t;
    if (t <= BOO_MAX_NEIGHBORS)
        coord[t] = 0u;
    if (t == 0)
        block_degenerate = block_counted = 0u;
    __syncthreads();
    if (i < n0) {
        int m = len[fs * n0 + i];
        m = m > max_nb ? max_nb : m;
        const int64_t stride = n0;
        int *__restrict__ row = list + fs * max_nb * stride + i;
        for (int s = 1; s < m; ++s) {
            const int key = row[s * stride];
            int at = s - 1;
            while (at >= 0) {
                const int v = row[at * stride];
                if (v <= key)
                    break;
                row[(at + 1) * stride] = v;
                --at;
            }
            row[(at + 1) * stride] = key;
        }
        const float *__restrict__ frame = slab + fs * 3 * n_rows;
        const double xi = (double)frame[i], yi = (double)frame[n_rows + i], zi = (double)frame[2 * int64_t(n_rows) + i];
        unsigned int zero = 0u;
        for (int s = 0; s < m; ++s) {
            const float *__restrict__ src = frame + off + row[s * stride];
            double wx, wy, wz;
            min_image_of<true>((double)src[0], (double)src[n_rows], (double)src[2 * int64_t(n_rows)], xi, yi, zi, box,
                               7, wx, wy, wz);
            zero += r2_of(wx, wy, wz) == 0.0;
        }
        atomicAdd(&coord[m], 1u);
        if (m > 0)
            atomicAdd(&block_counted, 1u);
        if (zero)
            atomicAdd(&block_degenerate, zero);
    }
    __syncthreads();
    if (t <= max_nb && coord[t])
        atomicAdd(&coordination[t], (unsigned long long)coord[t]);
    if (t == 0 && block_counted)
        atomicAdd(&counted[f0 + fs], (unsigned long long)block_counted);
    if (t == 0 && block_degenerate)
        atomicAdd(degenerate, (unsigned long long)block_degenerate);
}

// q_l from the 2L + 1 kept components of q_lm (or qbar_lm): S and the root of the contract
template <int L>
__device__ __forceinline__ double boo_invariant(const double (&re)[L + 1], const double (&im)[L + 1], double k)
{
    double S = __dmul_rn(re[0], re[0]);
#pragma unroll
    for (int m = 1; m <= L; ++m)
        S = __dadd_rn(S, __dmul_rn(2.0, __dadd_rn(__dmul_rn(re[m], re[m]), __dmul_rn(im[m], im[m]))));
    return __dsqrt_rn(__dmul_rn(k, S));
}

// q_lm and q_l of degree L for slab frame blockIdx.y, one lane per centre, over the sorted rows.
// qlm: float64 [slab][2L + 1][n0]; values: the slab's values at (d, k = 0), value_stride doubles from frame to frame.
template <int L>
__global__ __launch_bounds__(BOO_THREADS) void boo_qlm_kernel(
    const float *__restrict__ slab, int n_rows, int n0, int off, PairBox box, int max_nb,
    const int *__restrict__ len, const int *__restrict__ list, const BooTables *__restrict__ tab,
    double *__restrict__ qlm, double *__restrict__ values, int64_t value_stride)
{
    const int64_t fs = blockIdx.y;
    const int i = blockIdx.x * BOO_THREADS + threadIdx.x;
    if (i >= n0)
        return;
    int m_i = len[fs * n0 + i];
    m_i = m_i > max_nb ? max_nb : m_i;
    const int64_t stride = n0;
    const int *__restrict__ row = list + fs * max_nb * stride + i;
    const float *__restrict__ frame = slab + fs * 3 * n_rows;
    const double xi = (double)frame[i], yi = (double)frame[n_rows + i], zi = (double)frame[2 * int64_t(n_rows) + i];
    double re[L + 1], im[L + 1];
#pragma unroll
    for (int m = 0; m <= L; ++m)
        re[m] = im[m] = 0.0;
    for (int s = 0; s < m_i; ++s) {
        const float *__restrict__ src = frame + off + row[s * stride];
        double wx, wy, wz;
        min_image_of<true>((double)src[0], (double)src[n_rows], (double)src[2 * int64_t(n_rows)], xi, yi, zi, box, 7,
                           wx, wy, wz);
        const double r = __dsqrt_rn(r2_of(wx, wy, wz));
        const double ux = __ddiv_rn(wx, r), uy = __ddiv_rn(wy, r), uz = __ddiv_rn(wz, r);
        double c = 1.0, sn = 0.0;
#pragma unroll
        for (int m = 0; m <= L; ++m) {
            if (m > 0) {
                const double c_next = __dsub_rn(__dmul_rn(c, ux), __dmul_rn(sn, uy));
                sn = __dadd_rn(__dmul_rn(c, uy), __dmul_rn(sn, ux));
                c = c_next;
            }
            double below = boo_double_factorial(m), T = below;        // T_m^m
            if (m < L) {
                T = __dmul_rn(__dmul_rn(double(2 * m + 1), uz), below);       // T_{m+1}^m
#pragma unroll
                for (int n = m + 2; n <= L; ++n) {
                    const double next = __dsub_rn(__dmul_rn(__dmul_rn(tab->a[n][m], uz), T),
                                                  __dmul_rn(tab->b[n][m], below));
                    below = T;
                    T = next;
                }
            }
            const double y = __dmul_rn(tab->norm[L][m], T);
            re[m] = __dadd_rn(re[m], __dmul_rn(y, c));
            if (m > 0)
                im[m] = __dadd_rn(im[m], __dmul_rn(y, sn));
        }
    }
    double *__restrict__ out = qlm + fs * (2 * L + 1) * stride + i;
    double *__restrict__ value = values + fs * value_stride + i;
    if (m_i == 0) {                         // isolated: NaN all through
#pragma unroll
        for (int comp = 0; comp < 2 * L + 1; ++comp)
            out[comp * stride] = boo_nan();
        *value = boo_nan();
        return;
    }
    const double count = (double)m_i;
#pragma unroll
    for (int m = 0; m <= L; ++m) {
        re[m] = __ddiv_rn(re[m], count);
        im[m] = __ddiv_rn(im[m], count);
    }
    out[0] = re[0];
#pragma unroll
    for (int m = 1; m <= L; ++m) {
        out[(2 * m - 1) * stride] = re[m];
        out[(2 * m) * stride] = im[m];
    }
    *value = boo_invariant<L>(re, im, tab->k[L]);
}

// qbar_l of degree L (same only: neighbour j is centre j), one lane per centre of slab frame blockIdx.y.
// values: the slab's values at (d, k = 1).
template <int L>
__global__ __launch_bounds__(BOO_THREADS) void boo_average_kernel(
    int n0, int max_nb, const int *__restrict__ len, const int *__restrict__ list,
    const BooTables *__restrict__ tab, const double *__restrict__ qlm, double *__restrict__ values,
    int64_t value_stride)
{
    const int64_t fs = blockIdx.y;
    const int i = blockIdx.x * BOO_THREADS + threadIdx.x;
    if (i >= n0)
        return;
    int m_i = len[fs * n0 + i];
    m_i = m_i > max_nb ? max_nb : m_i;
    const int64_t stride = n0;
    const int *__restrict__ row = list + fs * max_nb * stride + i;
    const double *__restrict__ frame = qlm + fs * (2 * L + 1) * stride;
    double *__restrict__ value = values + fs * value_stride + i;
    if (m_i == 0) {
        *value = boo_nan();
        return;
    }
    double re[L + 1], im[L + 1];
    re[0] = frame[i];
    im[0] = 0.0;
#pragma unroll
    for (int m = 1; m <= L; ++m) {
        re[m] = frame[(2 * m - 1) * stride + i];
        im[m] = frame[(2 * m) * stride + i];
    }
    for (int s = 0; s < m_i; ++s) {
        const double *__restrict__ src = frame + row[s * stride];
        re[0] = __dadd_rn(re[0], src[0]);
#pragma unroll
        for (int m = 1; m <= L; ++m) {
            re[m] = __dadd_rn(re[m], src[(2 * m - 1) * stride]);
            im[m] = __dadd_rn(im[m], src[(2 * m) * stride]);
        }
    }
    const double count = (double)(m_i + 1);
#pragma unroll
    for (int m = 0; m <= L; ++m) {
        re[m] = __ddiv_rn(re[m], count);
        im[m] = __ddiv_rn(im[m], count);
    }
    *value = boo_invariant<L>(re, im, tab->k[L]);
}

// The values [frames][DK][n0] of a slab into the histograms.  grid x: chunks of BOO_BIN_CHUNK consecutive (frame,
// centre) numbers v = frame * n0 + i < n_values; grid y: dk = d * K + k.  edges: float64 [n_bins + 1] in HBM.
// LDS_HIST: n_bins <= BOO_LDS_BINS.  counts: uint64 [DK][n_bins]; outside: uint64 [DK].
template <bool LDS_HIST>
__global__ __launch_bounds__(BOO_THREADS) void boo_bin_kernel(
    const double *__restrict__ values, int64_t n_values, int n0, int DK, const double *__restrict__ edges,
    int n_bins, unsigned long long *__restrict__ counts, unsigned long long *__restrict__ outside)
{
    __shared__ double lds_edges[LDS_HIST ? BOO_LDS_BINS + 1 : 1];
    __shared__ unsigned int hist[LDS_HIST ? BOO_WAVES * BOO_LDS_BINS : 1];
    __shared__ unsigned int block_outside;
    const int t = threadIdx.x, dk = blockIdx.y;
    if (LDS_HIST) {
        for (int w = t; w < BOO_WAVES * n_bins; w += BOO_THREADS)
            hist[(w / n_bins) * BOO_LDS_BINS + w % n_bins] = 0u;
        for (int m = t; m <= n_bins; m += BOO_THREADS)
            lds_edges[m] = edges[m];
    }
    if (t == 0)
        block_outside = 0u;
    __syncthreads();
    const double *__restrict__ e = LDS_HIST ? lds_edges : edges;
    unsigned int *__restrict__ my_hist = hist + (LDS_HIST ? (t >> 6) * BOO_LDS_BINS : 0);
    const double lowest = e[0], highest = e[n_bins];
    const int64_t v0 = int64_t(blockIdx.x) * BOO_BIN_CHUNK;
    const int64_t v1 = n_values - v0 < BOO_BIN_CHUNK ? n_values : v0 + BOO_BIN_CHUNK;
    for (int64_t v = v0 + t; v < v1; v += BOO_THREADS) {
        const int64_t f = v / n0;
        const double q = values[(f * DK + dk) * n0 + (v - f * n0)];
        if (q != q)                         // an isolated centre
            continue;
        if (!(q >= lowest && q <= highest)) {
            atomicAdd(&block_outside, 1u);
            continue;
        }
        int lo = 0, hi = n_bins - 1;        // the inner edges that are <= q: a prefix, the edges increase
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (q >= e[mid + 1])
                lo = mid + 1;
            else
                hi = mid;
        }
        if (LDS_HIST)
            atomicAdd(&my_hist[lo], 1u);
        else
            atomicAdd(&counts[int64_t(dk) * n_bins + lo], 1ull);
    }
    __syncthreads();
    if (LDS_HIST)
        for (int w = t; w < n_bins; w += BOO_THREADS) {
            unsigned int sum = 0u;
            for (int v = 0; v < BOO_WAVES; ++v)
                sum += hist[v * BOO_LDS_BINS + w];
            if (sum)
                atomicAdd(&counts[int64_t(dk) * n_bins + w], (unsigned long long)sum);
        }
    if (t == 0 && block_outside)
        atomicAdd(&outside[dk], (unsigned long long)block_outside);
}

// sums[f0 + frame][dk] of a slab: block blockIdx.x = frame * DK + dk adds the n0 values of its row of `values`, per
// tile of BOO_SUM_TILE in row order from +0.0 (a NaN, an isolated centre, is left out), then the tiles in tile order
// from +0.0.
__global__ __launch_bounds__(BOO_THREADS) void boo_sum_kernel(const double *__restrict__ values, int n0, int DK,
                                                              int64_t f0, double *__restrict__ sums)
{
    __shared__ double buf[BOO_WAVES][BOO_SUM_TILE];
    __shared__ double part[BOO_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double *__restrict__ in = values + int64_t(blockIdx.x) * n0;
    const int n_tiles = (n0 + BOO_SUM_TILE - 1) / BOO_SUM_TILE;
    double total = 0.0;
    for (int t0 = 0; t0 < n_tiles; t0 += BOO_WAVES) {
        const int64_t i = int64_t(t0 + w) * BOO_SUM_TILE + lane;
        buf[w][lane] = i < n0 ? in[i] : boo_nan();
        __syncthreads();
        if (lane == 0) {
            double s = 0.0;
            for (int k = 0; k < BOO_SUM_TILE; ++k) {
                const double x = buf[w][k];
                if (x == x)
                    s = __dadd_rn(s, x);
            }
            part[w] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int v = 0; v < BOO_WAVES && t0 + v < n_tiles; ++v)
                total = __dadd_rn(total, part[v]);
    }
    if (threadIdx.x == 0)
        sums[f0 * DK + blockIdx.x] = total;
}

}  // namespace mdx_boo_dev
