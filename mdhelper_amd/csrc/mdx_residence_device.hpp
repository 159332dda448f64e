// mdx_residence_device.hpp — device side of the pair residence engine (mdx_residence.hip).
//
// Result contract.  The sets, the box, the frames, lags, origin_step, zero_dims and `same` mean what they mean in
// mdx_vanhove_distinct_device.hpp: set 1 holds n1 rows, set 2 holds n2 rows, incoming rows are set 1 then set 2; with
// `same` both are one set (n1 == n2, the rows arrive once), the ordered pairs (i, j) and (j, i) both count and i == j
// does not.  Analysed frames are numbered f = 0, 1, ... in the order fed; `lags` is strictly increasing and
// non-negative; origin_step >= 1.  Box and pair arithmetic: those of mdx_pairs_device.hpp, for the pair (i of set 1,
// j of set 2), both at frame f:
//
//     h_ij(f) = 1  where  r2 <= rc2 ,  rc2 = cutoff * cutoff formed once on the host in float64
//
// A NaN r2 is never a contact (the comparison fails); no square root is taken.  C(f) is the set of pairs with h = 1.
// The results, all integers (uint64 in HBM, handed out as int64):
//
//     contacts[f]      = |C(f)|                                          for every analysed frame
//   and per lag k, summed over every origin f0 of the lag (f0 % origin_step == 0, f0 + lags[k] < F):
//     origin_counts[k] += |C(f0)|
//     intermittent[k]  += |C(f0) & C(f0 + lags[k])|
//     continuous[k]    += |C(f0) & C(f0 + 1) & ... & C(f0 + lags[k])|    over every analysed frame in between, not only
//                                                                        those that are lags
//
// Capped lists (mdx_pairs_device.hpp).  A row i holds at most max_neighbors (1 ... 64) contacts in one frame; a row
// that would hold more refuses the results (MDX_ERR_INVALID_VALUE, naming max_neighbors and the largest row).
//
// All accumulation is integer adds (atomics on integers commute), set membership does not depend on the order in
// which a row's contacts were appended, and popcounts do not either: the numbers are the same whatever the input
// route, the split into calls or slabs, the grid, or the arrival order of the atomics.
//
// evaluations is the contract's count F * (n1*n2 - (same ? n1 : 0)).
//
// Shape.  gather_kernel gathers the rows of a slab of incoming frames, component-major float32 (widening is exact
// and happens in registers); positions live only as long as the slab in flight: the history is contact lists.
// prs_contact_kernel (the hot path, F * n1 * n2 evaluations) is the walk of mdx_pairs_device.hpp with z = the new
// frames and PRS_JCHUNK points of set 2 per block; its rule is one compare per pair against a kernel argument.  A
// contact takes slot = atomicAdd(&len[f % cap][i], 1) and is stored at list[f % cap][slot][i] when
// slot < max_neighbors (slot-major: the walk kernel's lanes read consecutive i).  Each block adds its contacts to
// contacts[f] with one integer atomic and its largest row to max_row with one atomicMax.
// prs_walk_kernel: one thread per (origin f0, point i); its state is a 64-bit alive mask over the slots of
// list[f0 % cap][.][i], kept in HBM and ring-indexed by f0, so that an origin survives slab and call boundaries.  For
// every new frame f of the launch in order, f0 <= f <= f0 + max(lags): member = the origin's slots whose j is also in
// list[f % cap][.][i]; alive &= member; where f - f0 is lag k, popc(member), popc(alive) and len(f0) are summed over
// the wave and added to intermittent[k], continuous[k] and origin_counts[k] with one uint64 atomic each.  A frame
// that is no lag only has to test the slots still alive.  Without `continuous` the walk visits lag frames only and
// keeps no mask.
// The rings of lists (and masks) hold cap = max(lags) + the frames of a slab: (max_neighbors + 1) * n1 * 4 B plus
// 8 * n1 B per frame.
//
// No cell list and no spatial culling: every pair is evaluated.  Culling by cells is the follow-up.
#pragma once

#include "mdx_pairs_device.hpp"

namespace mdx_prs_dev {

using namespace mdx_pairs_dev;

constexpr int PRS_TILE = PAIR_TILE;           // set-1 points per block, one per lane
constexpr int PRS_THREADS = PAIR_THREADS;
constexpr int PRS_STAGE = PAIR_STAGE;         // set-2 points per LDS stage, one staged per thread
constexpr int PRS_JCHUNK = 4 * PRS_STAGE;     // set-2 points per block
constexpr int PRS_MAX_NEIGHBORS = PAIR_MAX_NEIGHBORS;   // slots of a row at most: one bit each in the alive mask
constexpr int64_t PRS_SLAB_MAX = PAIR_SLAB_MAX;         // frames per launch, at most (grid z)
constexpr int PRS_WALK_THREADS = 256;
constexpr int PRS_WALK_ORIGINS = 65535;       // origins per walk launch, at most (grid y)

// The contacts of frame f = f_lo + blockIdx.z among the rows of slab frame blockIdx.z.  n_points: rows of a slab
// frame; set 2 starts at row off2 (0 with same).  keep: bit c set -> component c takes part; ALL: keep == 7, known
// when compiled.  len: int32 [cap][n1], zero for the new frames; list: int32 [cap][max_nb][n1]; contacts: uint64 [F].
template <bool ALL>
__global__ __launch_bounds__(PRS_THREADS) void prs_contact_kernel(
    const float *__restrict__ slab, int64_t cap, int n_points, int n1, int n2, int off2, int same, int n_jchunks,
    int64_t f_lo, PairBox box, int keep, double rc2, int max_nb, int *__restrict__ len, int *__restrict__ list,
    unsigned long long *__restrict__ contacts, int *__restrict__ max_row)
{
    __shared__ __attribute__((aligned(16))) double stage[4 * PRS_STAGE];
    __shared__ unsigned int block_found, block_row;
    const int64_t f = f_lo + blockIdx.z;
    const int tile = blockIdx.x / n_jchunks, chunk = blockIdx.x - tile * n_jchunks;
    const int i = tile * PRS_TILE + threadIdx.x;
    const bool live = i < n1;
    const float *__restrict__ a = slab + int64_t(blockIdx.z) * 3 * n_points + (live ? i : n1 - 1);
    const float *__restrict__ b = slab + int64_t(blockIdx.z) * 3 * n_points + off2;
    const double xi = (double)a[0], yi = (double)a[n_points], zi = (double)a[2 * int64_t(n_points)];
    const int64_t slot_f = f % cap;
    int *__restrict__ my_len = len + slot_f * n1 + (live ? i : 0);
    int *__restrict__ my_list = list + slot_f * max_nb * n1 + (live ? i : 0);
    if (threadIdx.x == 0) {
        block_found = 0u;
        block_row = 0u;
    }
    __syncthreads();
    unsigned int found = 0u, row = 0u;
    const int j_begin = chunk * PRS_JCHUNK;
    const int j_end = n2 - j_begin < PRS_JCHUNK ? n2 : j_begin + PRS_JCHUNK;
    for (int js = j_begin; js < j_end; js += PRS_STAGE) {
        const int nj = j_end - js < PRS_STAGE ? j_end - js : PRS_STAGE;
        __syncthreads();                    // the stage is free
        if ((int)threadIdx.x < nj)
            stage_partners(stage, b, n_points, js);
        __syncthreads();
        if (!live)
            continue;
        const int skip = same ? i - js : -1;        // the stage entry that is this lane's own point
        stage_pairs<ALL>(stage, nj, js, skip, xi, yi, zi, box, keep,
                         [&](int, int j, double, double, double, double r2, bool other) {
                             if (r2 <= rc2 && other) {
                                 append_capped(my_len, my_list, n1, max_nb, j, row);
                                 ++found;
                             }
                         });
    }
    block_tally<true>(found, row, &block_found, &block_row, &contacts[f], max_row);
}

// bits 0 ... n - 1
__device__ __forceinline__ unsigned long long prs_full(int n)
{
    return n >= 64 ? ~0ull : (1ull << n) - 1ull;
}

// The slots s (bits of `want`) of the origin's row whose j is among the n_f entries of the frame's row.  Both rows
// are read with stride n1 (slot-major lists).
__device__ __forceinline__ unsigned long long prs_member(const int *__restrict__ origin_row, unsigned long long want,
                                                         const int *__restrict__ frame_row, int n_f, int64_t n1)
{
    unsigned long long member = 0ull;
    while (want) {
        const int s = __ffsll((long long)want) - 1;
        want &= want - 1ull;
        const int j = origin_row[s * n1];
        for (int t = 0; t < n_f; ++t)
            if (frame_row[t * n1] == j) {
                member |= 1ull << s;
                break;
            }
    }
    return member;
}

// Adds v over the wave and, where the sum is not zero, to *dst with one atomic.  Every lane of the wave calls it.
__device__ __forceinline__ void prs_wave_add(unsigned long long *dst, unsigned int v)
{
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0 && v)
        atomicAdd(dst, (unsigned long long)v);
}

// Origins f0 = (o_lo + blockIdx.y) * origin_step against the new frames [f_lo, f_lo + nf).  grid x = i tiles.  A
// block's threads share the origin, so the loops over frames and lags are uniform in a wave (lanes beyond n1 take
// part with empty rows).  mask: uint64 [cap][n1]; sums: uint64 [3][n_lags] = intermittent, continuous, origin_counts.
template <bool CONTINUOUS>
__global__ __launch_bounds__(PRS_WALK_THREADS) void prs_walk_kernel(
    int64_t cap, int n1, int max_nb, const int *__restrict__ len, const int *__restrict__ list,
    unsigned long long *__restrict__ mask, const int64_t *__restrict__ lags, int n_lags, int64_t max_lag,
    int64_t o_lo, int64_t origin_step, int64_t f_lo, int64_t nf, unsigned long long *__restrict__ sums)
{
    const int64_t f0 = (o_lo + blockIdx.y) * origin_step;
    const int i = blockIdx.x * PRS_WALK_THREADS + threadIdx.x;
    const bool live = i < n1;
    const int64_t slot0 = f0 % cap;
    const int64_t row = live ? i : 0;
    const int *__restrict__ origin_row = list + slot0 * max_nb * n1 + row;
    int len0 = live ? len[slot0 * n1 + row] : 0;
    len0 = len0 > max_nb ? max_nb : len0;           // an overflowing row: the host refuses the results
    const unsigned long long full = prs_full(len0);
    unsigned long long *__restrict__ intermittent = sums, *__restrict__ continuous = sums + n_lags,
                                     *__restrict__ origin_counts = sums + 2 * int64_t(n_lags);
    const int64_t f_end = f_lo + nf;                // one past the last new frame
    if (CONTINUOUS) {
        unsigned long long alive = full;
        if (f0 < f_lo && live)
            alive = mask[slot0 * n1 + row];
        const int64_t f_first = f0 > f_lo ? f0 : f_lo;
        const int64_t f_last = f0 + max_lag < f_end - 1 ? f0 + max_lag : f_end - 1;
        int k = 0;
        while (k < n_lags && lags[k] < f_first - f0)
            ++k;
        for (int64_t f = f_first; f <= f_last; ++f) {
            const bool is_lag = k < n_lags && lags[k] == f - f0;
            unsigned long long member = full;
            if (f != f0) {
                const int64_t slot_f = f % cap;
                int len_f = live ? len[slot_f * n1 + row] : 0;
                len_f = len_f > max_nb ? max_nb : len_f;
                member = prs_member(origin_row, is_lag ? full : alive, list + slot_f * max_nb * n1 + row, len_f, n1);
            }
            alive &= member;
            if (is_lag) {
                prs_wave_add(&intermittent[k], (unsigned int)__popcll(member));
                prs_wave_add(&continuous[k], (unsigned int)__popcll(alive));
                prs_wave_add(&origin_counts[k], (unsigned int)len0);
                ++k;
            }
        }
        if (live)
            mask[slot0 * n1 + row] = alive;
    } else {
        for (int k = 0; k < n_lags; ++k) {
            const int64_t f = f0 + lags[k];
            if (f < f_lo)
                continue;
            if (f >= f_end)
                break;
            unsigned long long member = full;
            if (f != f0) {
                const int64_t slot_f = f % cap;
                int len_f = live ? len[slot_f * n1 + row] : 0;
                len_f = len_f > max_nb ? max_nb : len_f;
                member = prs_member(origin_row, full, list + slot_f * max_nb * n1 + row, len_f, n1);
            }
            prs_wave_add(&intermittent[k], (unsigned int)__popcll(member));
            prs_wave_add(&origin_counts[k], (unsigned int)len0);
        }
    }
}

}  // namespace mdx_prs_dev
