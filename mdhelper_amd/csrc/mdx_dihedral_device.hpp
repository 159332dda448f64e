// mdx_dihedral_device.hpp — device side of the dihedral engine (mdx_dihedral.hip).
//
// Result contract.  A frame delivers n_rows points (the distinct atoms, picked by the feed's index); the table
// quads int32 [D][4] of row numbers (a, b, c, d), four distinct rows each, defines D dihedrals, and group g holds
// n_dihedrals[g] consecutive ones (a group may be empty; a row may sit in many dihedrals).  Analysed frames are
// numbered f = 0, 1, ... in the order fed; `lags` is a strictly increasing list of non-negative frame offsets below
// 2^31; every frame is a time origin (there is no origin_step).  Everything is float64, one operation at a time (the
// unit is built with contraction off); float32 coordinates are widened before any arithmetic.
//
// Geometry, per dihedral v and frame f:
//
//     b1 = x_b - x_a,  b2 = x_c - x_b,  b3 = x_d - x_c      each component, with a box, through min_image of
//                                                           mdx_pairs_device.hpp (inv_c = 1.0 / L_c formed once on
//                                                           the host); the raw difference without a box
//     m  = b1 x b2,  n = b2 x b3        m_x = (b1y*b2z) - (b1z*b2y) and cyclically: two multiplies, one subtract
//     m2 = r2_of(m),  n2 = r2_of(n),  l2 = r2_of(b2)
//     p  = (m_x*n_x + m_y*n_y) + m_z*n_z
//     q  = (b1x*n_x + b1y*n_y) + b1z*n_z
//     den = sqrt(m2 * n2)                                   one multiply, one correctly rounded sqrt
//     c  = p / den                                          cos(phi)
//     s  = (sqrt(l2) * q) / den                             sin(phi), IUPAC sign: a = (1, 0, 0), b = 0, c = (0, 0, 1),
//                                                           d = (cos phi, sin phi, 1) gives phi
//
// A dihedral whose m2 * n2 is not > 0 or not finite (three atoms on a line, two on one point) is degenerate: it stores
// c = s = 0, is put in state 0 (its bin is not counted) and an integer counter in HBM counts it.  Once the counter is
// not zero the host refuses synchronize and every read-out until a reset (the rule of mdx_orient_device.hpp): an
// error, never a silently wrong average.
//
// Bin.  n_bins is even, n_half = n_bins / 2; thresholds float64 t[0 ... n_half] are strictly decreasing, and only the
// inner ones t[1 ... n_half - 1] are compared (the rule of mdx_angle_device.hpp):
//
//     h   = #{ m in 1 ... n_half - 1 : c <= t[m] }
//     bin = (q < 0) ? n_half - 1 - h : n_half + h
//
// With t[m] = cos(m pi / n_half) bin b covers phi in [-180 + b W, -180 + (b + 1) W), W = 360 / n_bins degrees; the
// exact trans case (c = -1, q = +-0) lands in the last bin, which is closed as in numpy.histogram.  No acos and no
// atan2 is taken anywhere: the rule is stated on c and on the sign of q.
//
// State.  state_of_bin int32 [n_bins] holds values 0 ... S - 1, 1 <= S <= DIH_MAX_STATES;
// state(f) = state_of_bin[bin(f)].
//
// Integer results (uint64 in HBM, integer atomics only, handed out as int64):
//
//     counts[g][b]             the (dihedral of g, frame) cases in bin b
//     state_counts[f][g][s]    the dihedrals of g in state s at frame f, for every frame seen
//     transitions[g][s0][s1]   the (dihedral, f >= 1) cases with state(f - 1) = s0 and state(f) = s1, the diagonal too
//     run(0) = 0;  run(f) = state(f) == state(f - 1) ? min(run(f - 1) + 1, 2^31 - 1) : 0
//     same[k][g]               the cases f >= lag_k with state(f) == state(f - lag_k)          (intermittent)
//     stay[k][g]               the cases f >= lag_k with run(f) >= lag_k                       (continuous: no change
//                                                                                              of state in between)
//
// Float result.  acc[k][v] += (c(f)*c(f - lag_k)) + (s(f)*s(f - lag_k)) for f >= lag_k: the accumulator of
// (lag k, dihedral v) lives in HBM, starts at +0.0 and receives its terms one after the other in frame order — a
// thread owns one (dihedral, lag), reads the accumulator at the start of a slab, walks the slab's frames and writes it
// back.  dih_fold_kernel adds the accumulators of a group's dihedrals one after the other in row order from +0.0 into
// sums[k][g].  No floating-point atomics and no cross-lane float sums: a plain host loop gives the same bits, whatever
// route the frames take and however they are split into calls or slabs.  evaluations = D * sum_k origins met.
//
// Shape.  Tiles of DIH_TILE consecutive dihedrals never span two groups.  Three rings of cap = max(max lag, 1) + slab
// frames in HBM, frame f in slot f % cap: hist double [cap][2][D] (c, then s: component-major, the lanes of a wave read
// consecutive doubles), state uint8 [cap][D], run int32 [cap][D].
//   dih_prepare_kernel<BOX, LDS_HIST>: grid x = runs of DIH_BLOCK_TILES tiles, y = runs of DIH_BLOCK_FRAMES frames of
//   the slab; a wave has a tile on its lanes and walks the frames of its run.  It gathers the twelve floats, forms c,
//   s, bin and state and writes the first two rings.  A wave's tile lies in one group, so a wave counts its bins in
//   n_bins uint32 words of LDS of its own and flushes the non-zero words with one uint64 atomic each after its run of
//   frames (one flush per tile and frame put 60 000 atomics a slab on every bin's word at 97 000 dihedrals: 4 ms of
//   the 7 ms of a slab); beyond DIH_LDS_BINS bins it counts in HBM directly, one uint64 atomic per dihedral.  (A wave
//   adds at most DIH_TILE x DIH_BLOCK_FRAMES = 2 048 to the words of its histogram before it flushes: they cannot
//   wrap.)
//   state_counts come from one wave ballot and popcount per state and one atomic per non-zero count.
//   dih_run_kernel: run is sequential in f, so one lane per dihedral walks the slab's frames in order, reads state
//   and run of frame f0 - 1 from the rings (cap holds at least one frame before the slab) and writes run(f).  The same
//   walk tallies the transitions in S x S uint32 LDS words per wave (a wave adds at most DIH_TILE x DIH_SLAB_MAX
//   = 2^21 to them) and flushes the non-zero ones with one uint64 atomic each.
//   dih_correlate_kernel has ori_correlate_kernel's shape (mdx_orient_device.hpp): a block is DIH_BLOCK_LAGS waves;
//   every wave has the same tile on its lanes and a lag of its own.  A lane keeps `same` and `stay` in uint32
//   registers over the slab's frames (at most DIH_SLAB_MAX each); the wave adds them with integer shuffles and one
//   uint64 atomic each.
//   dih_fold_kernel: ori_fold_kernel for one column.
#pragma once

#include "mdx_pairs_device.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mdx_dih_dev {

using mdx_pairs_dev::PairBox;

constexpr int DIH_TILE = 64;                  // dihedrals per tile = lanes of a wave
constexpr int DIH_BLOCK_LAGS = 4;             // lags (waves) per block of the correlate kernel
constexpr int DIH_BLOCK_TILES = 4;            // tiles (waves) per block of the prepare and run kernels
constexpr int DIH_BLOCK_FRAMES = 32;          // frames a block of the prepare kernel walks
constexpr int DIH_THREADS = DIH_TILE * DIH_BLOCK_TILES;
constexpr int DIH_MAX_STATES = 8;
constexpr int DIH_LDS_BINS = 1024;            // bins at most for the LDS form of the histogram
constexpr int64_t DIH_SLAB_MAX = 32768;       // frames per launch, at most (grid y of the prepare kernel)

struct DihTile {
    int first;      // first dihedral, in concatenated-group order
    int count;      // 1 ... DIH_TILE
    int group;
};

// c, s, bin and state of the tiles' dihedrals in the frames of a slab: hist[((f0 + f) % cap) * 2 + {0, 1}][v],
// state[(f0 + f) % cap][v], counts[g][bin] and state_counts[f0 + f][g][s].  Grid: x = runs of DIH_BLOCK_TILES tiles,
// y = runs of DIH_BLOCK_FRAMES of the n_frames frames; wave w of a block takes tile blockIdx.x * DIH_BLOCK_TILES + w.
// Row index[r] (or r) of a frame of src_rows rows is point r.  inner: the n_half - 1 inner thresholds t[1] ...
// t[n_half - 1] in HBM, decreasing.  LDS_HIST: n_bins <= DIH_LDS_BINS.
template <bool BOX, bool LDS_HIST>
__global__ __launch_bounds__(DIH_THREADS) void dih_prepare_kernel(
    const float *__restrict__ pos, int64_t src_rows, const int *__restrict__ index, const int *__restrict__ quads,
    const DihTile *__restrict__ tiles, int n_tiles, int n_dihedrals, int n_groups, int n_frames, int64_t f0,
    int64_t cap, PairBox box, const double *__restrict__ inner, int n_bins, const int *__restrict__ state_of_bin,
    int n_states, double *__restrict__ hist, unsigned char *__restrict__ state,
    unsigned long long *__restrict__ counts, unsigned long long *__restrict__ state_counts,
    unsigned long long *__restrict__ degenerate)
{
    __shared__ unsigned int dih_bins[DIH_BLOCK_TILES][LDS_HIST ? DIH_LDS_BINS : 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t = blockIdx.x * DIH_BLOCK_TILES + w;
    const bool have = t < n_tiles;                  // the same in every lane of the wave
    const DihTile tile = tiles[have ? t : 0];
    const bool live = have && lane < tile.count;
    if (LDS_HIST)
        for (int b = lane; b < n_bins; b += DIH_TILE)
            dih_bins[w][b] = 0u;
    __syncthreads();
    const int f_begin = blockIdx.y * DIH_BLOCK_FRAMES;
    const int f_end = n_frames - f_begin < DIH_BLOCK_FRAMES ? n_frames : f_begin + DIH_BLOCK_FRAMES;
    for (int64_t f = f_begin; f < f_end; ++f) {     // the same trips in every lane of the block
        int st = -1;                                    // no dihedral on this lane
        if (live) {
            const int v = tile.first + lane;
            const int *__restrict__ quad = quads + 4 * int64_t(v);
            const float *__restrict__ frame = pos + f * src_rows * 3;
            double x[4][3];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = quad[i];
                const float *__restrict__ at = frame + int64_t(index ? index[r] : r) * 3;
                x[i][0] = (double)at[0];
                x[i][1] = (double)at[1];
                x[i][2] = (double)at[2];
            }
            double b[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double d = __dsub_rn(x[i + 1][k], x[i][k]);
                    b[i][k] = BOX ? mdx_pairs_dev::min_image(d, box.L[k], box.inv[k]) : d;
                }
            const double mx = __dsub_rn(__dmul_rn(b[0][1], b[1][2]), __dmul_rn(b[0][2], b[1][1]));
            const double my = __dsub_rn(__dmul_rn(b[0][2], b[1][0]), __dmul_rn(b[0][0], b[1][2]));
            const double mz = __dsub_rn(__dmul_rn(b[0][0], b[1][1]), __dmul_rn(b[0][1], b[1][0]));
            const double nx = __dsub_rn(__dmul_rn(b[1][1], b[2][2]), __dmul_rn(b[1][2], b[2][1]));
            const double ny = __dsub_rn(__dmul_rn(b[1][2], b[2][0]), __dmul_rn(b[1][0], b[2][2]));
            const double nz = __dsub_rn(__dmul_rn(b[1][0], b[2][1]), __dmul_rn(b[1][1], b[2][0]));
            const double m2 = mdx_pairs_dev::r2_of(mx, my, mz), n2 = mdx_pairs_dev::r2_of(nx, ny, nz);
            const double l2 = mdx_pairs_dev::r2_of(b[1][0], b[1][1], b[1][2]);
            const double p = __dadd_rn(__dadd_rn(__dmul_rn(mx, nx), __dmul_rn(my, ny)), __dmul_rn(mz, nz));
            const double q = __dadd_rn(__dadd_rn(__dmul_rn(b[0][0], nx), __dmul_rn(b[0][1], ny)),
                                       __dmul_rn(b[0][2], nz));
            const double mn = __dmul_rn(m2, n2);
            double c = 0.0, s = 0.0;
            st = 0;
            if (mn > 0.0 && mn <= 1.7976931348623157e308) {
                const double den = __dsqrt_rn(mn);
                c = __ddiv_rn(p, den);
                s = __ddiv_rn(__dmul_rn(__dsqrt_rn(l2), q), den);
                int lo = 0, hi = (n_bins >> 1) - 1;     // the inner thresholds that are >= c: a prefix, t decreases
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (c <= inner[mid])
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                const int bin = q < 0.0 ? (n_bins >> 1) - 1 - lo : (n_bins >> 1) + lo;
                st = state_of_bin[bin];
                if (LDS_HIST)
                    atomicAdd(&dih_bins[w][bin], 1u);
                else
                    atomicAdd(&counts[int64_t(tile.group) * n_bins + bin], 1ull);
            } else {
                atomicAdd(degenerate, 1ull);            // m2 * n2 zero, infinite or NaN: c = s = 0, state 0, no bin
            }
            const int64_t slot = (f0 + f) % cap;
            double *__restrict__ out = hist + slot * 2 * n_dihedrals + v;
            out[0] = c;
            out[n_dihedrals] = s;
            state[slot * n_dihedrals + v] = (unsigned char)st;
        }
        // the dihedrals of the tile in every state: lane s keeps the count of state s
        unsigned int mine = 0u;
        for (int k = 0; k < n_states; ++k) {
            const unsigned int n = (unsigned int)__popcll(__ballot(st == k));
            mine = lane == k ? n : mine;
        }
        if (have && lane < n_states && mine)
            atomicAdd(&state_counts[((f0 + f) * n_groups + tile.group) * n_states + lane], (unsigned long long)mine);
    }
    __syncthreads();
    if (LDS_HIST && have)
        for (int b = lane; b < n_bins; b += DIH_TILE)
            if (dih_bins[w][b])
                atomicAdd(&counts[int64_t(tile.group) * n_bins + b], (unsigned long long)dih_bins[w][b]);
}

// run(f) of the frames [f_lo, f_hi) into run[f % cap][v], and the transitions into them.  One lane per dihedral, wave
// w of a block takes tile blockIdx.x * DIH_BLOCK_TILES + w.  transitions: uint64 [G][S][S].
__global__ __launch_bounds__(DIH_THREADS) void dih_run_kernel(
    const unsigned char *__restrict__ state, int64_t cap, int n_dihedrals, const DihTile *__restrict__ tiles,
    int n_tiles, int n_states, int64_t f_lo, int64_t f_hi, int *__restrict__ run,
    unsigned long long *__restrict__ transitions)
{
    __shared__ unsigned int dih_moves[DIH_BLOCK_TILES][DIH_MAX_STATES * DIH_MAX_STATES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t = blockIdx.x * DIH_BLOCK_TILES + w;
    const bool have = t < n_tiles;                  // the same in every lane of the wave
    const DihTile tile = tiles[have ? t : 0];
    dih_moves[w][lane] = 0u;
    __syncthreads();
    if (have && lane < tile.count) {
        const int v = tile.first + lane;
        int64_t slot = (f_lo > 0 ? f_lo - 1 : 0) % cap;
        int before = 0, length = 0;
        if (f_lo > 0) {
            before = state[slot * n_dihedrals + v];
            length = run[slot * n_dihedrals + v];
            if (++slot == cap)
                slot = 0;
        }
        for (int64_t f = f_lo; f < f_hi; ++f) {
            const int now = state[slot * n_dihedrals + v];
            if (f > 0) {
                length = now == before ? (length < 2147483647 ? length + 1 : length) : 0;
                atomicAdd(&dih_moves[w][before * n_states + now], 1u);
            }
            run[slot * n_dihedrals + v] = length;
            before = now;
            if (++slot == cap)
                slot = 0;
        }
    }
    __syncthreads();
    if (have && lane < n_states * n_states && dih_moves[w][lane])
        atomicAdd(&transitions[int64_t(tile.group) * n_states * n_states + lane],
                  (unsigned long long)dih_moves[w][lane]);
}

// Frames [f_lo, f_hi) (numbers since the first analysed frame) against the frames `lag` before them.  Grid: x = tiles,
// y = runs of DIH_BLOCK_LAGS lags; wave w of a block takes lag blockIdx.y * DIH_BLOCK_LAGS + w.
// acc: double [n_lags][n_dihedrals]; same, stay: uint64 [n_lags][n_groups].
__global__ __launch_bounds__(DIH_TILE * DIH_BLOCK_LAGS) void dih_correlate_kernel(
    const double *__restrict__ hist, const unsigned char *__restrict__ state, const int *__restrict__ run, int64_t cap,
    int n_dihedrals, int n_groups, const DihTile *__restrict__ tiles, const int64_t *__restrict__ lags, int n_lags,
    int64_t f_lo, int64_t f_hi, double *__restrict__ acc, unsigned long long *__restrict__ same,
    unsigned long long *__restrict__ stay)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const DihTile tile = tiles[blockIdx.x];
    const int k = blockIdx.y * DIH_BLOCK_LAGS + w;
    if (k >= n_lags)                                // the same in every lane of the wave
        return;
    const int64_t lag = lags[k];
    const bool live = lane < tile.count;
    const int v = tile.first + (live ? lane : 0);           // lanes without a dihedral read the tile's first one
    double *__restrict__ mine = acc + int64_t(k) * n_dihedrals + v;
    double sum = *mine;
    unsigned int n_same = 0u, n_stay = 0u;
    const int64_t f_first = f_lo > lag ? f_lo : lag;
    int64_t sa = f_first % cap, sb = (f_first - lag) % cap;
    const int64_t stride = n_dihedrals;
#pragma unroll 4
    for (int64_t f = f_first; f < f_hi; ++f) {
        const double *__restrict__ a = hist + sa * 2 * stride + v;
        const double *__restrict__ b = hist + sb * 2 * stride + v;
        sum = __dadd_rn(sum, __dadd_rn(__dmul_rn(a[0], b[0]), __dmul_rn(a[stride], b[stride])));
        n_same += state[sa * stride + v] == state[sb * stride + v];
        n_stay += int64_t(run[sa * stride + v]) >= lag;
        if (++sa == cap)
            sa = 0;
        if (++sb == cap)
            sb = 0;
    }
    if (live)
        *mine = sum;
    n_same = live ? n_same : 0u;
    n_stay = live ? n_stay : 0u;
    for (int off = 32; off > 0; off >>= 1) {
        n_same += __shfl_down(n_same, off);
        n_stay += __shfl_down(n_stay, off);
    }
    if (lane == 0) {
        if (n_same)
            atomicAdd(&same[int64_t(k) * n_groups + tile.group], (unsigned long long)n_same);
        if (n_stay)
            atomicAdd(&stay[int64_t(k) * n_groups + tile.group], (unsigned long long)n_stay);
    }
}

// sums[k][g] = the accumulators of the group's dihedrals [offsets[g], offsets[g + 1]) added in row order from +0.0.
// One thread per (lag, group).
__global__ __launch_bounds__(256) void dih_fold_kernel(const double *__restrict__ acc, int n_dihedrals,
                                                       const int64_t *__restrict__ offsets, int n_groups, int n_lags,
                                                       double *__restrict__ sums)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= int64_t(n_lags) * n_groups)
        return;
    const int g = int(i % n_groups);
    const int64_t k = i / n_groups;
    const double *__restrict__ in = acc + k * n_dihedrals;
    double s = 0.0;
    for (int64_t p = offsets[g]; p < offsets[g + 1]; ++p)
        s = __dadd_rn(s, in[p]);
    sums[i] = s;
}

}  // namespace mdx_dih_dev
