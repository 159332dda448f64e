// mdx_chi4_device.hpp — device side of the four-point engine (mdx_chi4.hip): the self-overlap Q of every frame pair and
// the sums of Q and Q*Q over the time origins, from which the class forms Q_s(t) and chi_4(t).
//
// Result contract.  Rows arrive in the order of the concatenated groups: group g holds n_points[g] consecutive points.
// Analysed frames are numbered f = 0, 1, ... in the order fed; `lags` is a strictly increasing list of non-negative
// frame offsets; origin_step >= 1.  Everything is float64 with separate multiply and add (the unit is built with
// contraction off); float32 coordinates are widened before any arithmetic.  x, image and the unwrap rule are exactly
// those of the self van Hove engine (mdx_vanhove_device.hpp: x_pd(f) = (double)r_pd(f) + image_pd(f) * L_d, the
// reference's global unwrap, the first analysed frame its own start); the ring of widened points is written by that
// header's vh_prepare_kernel.  Per lag k, cutoff c and frame f >= lags[k] whose origin f0 = f - lags[k] satisfies
// f0 % origin_step == 0:
//
//     d_d   = x_pd(f) - x_pd(f0)                          (d_d = +0.0 for a component that zero_dims drops)
//     r2    = (d_x*d_x + d_y*d_y) + d_z*d_z
//     w     = r2 <= a2[c]                                 (a2[c] = cutoffs[c] * cutoffs[c], one float64 multiply on the
//                                                          host; no sqrt on the device; a NaN r2 is not counted)
//     Q[k][g][c](f0) = number of points p of group g with w
//     S1[k][g][c] += Q ;  S2[k][g][c] += Q*Q              (uint64 in HBM, returned as int64)
//     n_origins[k]  = number of such f0                    (host arithmetic, returned with the result)
//
// Q of a frame pair is an integer, so S1 and S2 are integers and integer adds commute: S1, S2 and n_origins do not
// depend on the route (host array, HBM, file), on how the frames are split into calls, on the slab length or on the
// point-segment length.  There is no summation-order clause.  S2 <= n_origins * max_g(n_points[g])^2: a call after
// which (frames seen) * max_g(n_points[g])^2 would reach 2^63 is refused on the host before anything is touched.
//
// Shape.  chi4_count_kernel: grid x = frames of the slab, y = runs of CHI4_BLOCK_LAGS lags, z = segments of `seg`
// consecutive points (a multiple of 64) of the concatenated groups.  The four waves of a block take one lag each and
// walk the same 64-point loads of the segment, so x(f) of a load comes from HBM / L2 once and from the CU's L1 three
// times; x(f0) is the wave's own.  A lane forms r2 of its point and compares it with every cutoff (at most 8, kernel
// arguments, so they sit in scalar registers); the wave adds __popcll(__ballot(w)) — 64 bits wide on gfx950 — to a
// wave-uniform counter per cutoff.  Lanes past the end of a group or segment read the first point of the load's range
// and contribute 0.  A load never spans two groups: at a group boundary (and at the end of the segment) the wave
// flushes its counters with one integer atomicAdd per non-zero (lag, group, cutoff) into the uint32 scratch
// Qslab[f - f_lo][k][g][c] in HBM, which is zeroed per slab (a group holds fewer than 2^31 / 3 points, so Q fits).  No
// LDS, no __syncthreads.  chi4_fold_kernel then adds Q and Q*Q of the slab's frame pairs into S1 and S2, skipping the
// pairs that are not origins or have f < lag (their scratch words stayed zero anyway).
//
// Sizes.  The default slab keeps the slab's share of the ring plus the scratch within the 256 MiB the van Hove engine
// allows its own slab (mdx_chi4.hip).  The default segment is CHI4_SEGMENT = 1024 points: 24 KiB of x(f0) per wave,
// one flush per 16 loads, and a single frame pair of 10^6 points still makes 977 blocks per lag run.  Measured on an
// MI355X (scripts/four_point_time.py, 32 768 points in two groups x 1 024 frames in HBM, 64 lags, unwrap, one cutoff,
// medians of 5 warmed runs of all kernels, lags 0 ... 63 / lags 0, 8 ... 504; profiles/four_point_time.txt):
//     segment   128     256     512    1024    2048    4096    8192   16384   32768
//     ms       8.56    6.89    6.45    6.49    7.05    7.41    7.52    7.60    7.74     (lags 0 ... 63)
//     ms       7.20    5.97    5.56    5.39    5.37    5.46    5.62    5.98    6.72     (lags 0, 8 ... 504)
// Three cutoffs cost the same as one from 1024 points on (6.49 / 5.41 ms) and up to 8 % more below (9.20 / 7.59 ms at
// 128): there the flushes show.  The van Hove engine in the same job (scripts/vanhove_time.py, 201 bins): 10.01 ms
// (min 9.98, max 10.39) and 8.91 ms (min 8.90, max 8.92) for the same evaluations.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mdx_chi4_dev {

constexpr int CHI4_TILE = 64;                 // points per load = lanes of a wave
constexpr int CHI4_BLOCK_LAGS = 4;            // lags (waves) per block
constexpr int CHI4_THREADS = CHI4_TILE * CHI4_BLOCK_LAGS;
constexpr int CHI4_MAX_CUTOFFS = 8;
constexpr int CHI4_SEGMENT = 1024;            // points per segment by default
constexpr int CHI4_FOLD_FRAMES = 32;          // frames a thread of the fold kernel walks
constexpr int64_t CHI4_SLAB_MAX = 32768;      // frames per launch, at most

struct Chi4Cutoffs {
    double a2[CHI4_MAX_CUTOFFS];              // squared cutoffs; the first n_cutoffs are used
};

// r2 of point p between the ring frames a and b (component-major: component d of point p at [d * n_points + p])
__device__ __forceinline__ double chi4_r2(const double *__restrict__ a, const double *__restrict__ b, int64_t p,
                                          int64_t n_points, int keep)
{
    const double dx = keep & 1 ? __dsub_rn(a[p], b[p]) : 0.0;
    const double dy = keep & 2 ? __dsub_rn(a[n_points + p], b[n_points + p]) : 0.0;
    const double dz = keep & 4 ? __dsub_rn(a[2 * n_points + p], b[2 * n_points + p]) : 0.0;
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// Frames f_lo + blockIdx.x of the slab against the frames `lag` before them.  offsets: int64 [n_groups + 1], the
// groups' point ranges.  keep: bit d set -> component d takes part.  seg: points per segment, a multiple of 64.
// qslab: uint32 [frames of the slab][n_lags][n_groups][NC], zero at launch.
template <int NC>
__global__ __launch_bounds__(CHI4_THREADS) void chi4_count_kernel(
    const double *__restrict__ hist, int64_t cap, int n_points, const int64_t *__restrict__ offsets, int n_groups,
    const int64_t *__restrict__ lags, int n_lags, int64_t f_lo, int64_t origin_step, int keep, int seg,
    Chi4Cutoffs cut, unsigned int *__restrict__ qslab)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // the same in every lane of the wave
    const int k = blockIdx.y * CHI4_BLOCK_LAGS + w;
    if (k >= n_lags)
        return;
    const int64_t f = f_lo + blockIdx.x, lag = lags[k];
    if (f < lag || (f - lag) % origin_step != 0)
        return;
    const int64_t n = n_points;
    const int64_t p_lo = int64_t(blockIdx.z) * seg;
    const int64_t p_hi = p_lo + seg < n ? p_lo + seg : n;
    if (p_lo >= p_hi)
        return;
    const double *__restrict__ a = hist + (f % cap) * 3 * n;
    const double *__restrict__ b = hist + ((f - lag) % cap) * 3 * n;
    unsigned int *__restrict__ out = qslab + (int64_t(blockIdx.x) * n_lags + k) * n_groups * NC;

    // the group that holds p_lo: the last g with offsets[g] <= p_lo that is not empty there (offsets[n_groups] = n > p_lo)
    int g = 0, top = n_groups;
    while (top - g > 1) {
        const int mid = (g + top) >> 1;
        if (offsets[mid] <= p_lo)
            g = mid;
        else
            top = mid;
    }
    for (; g < n_groups; ++g) {
        const int64_t g_lo = offsets[g], g_hi = offsets[g + 1];
        if (g_lo >= p_hi)
            break;
        const int64_t lo = g_lo > p_lo ? g_lo : p_lo, hi = g_hi < p_hi ? g_hi : p_hi;
        if (lo >= hi)
            continue;                           // an empty group
        unsigned int count[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c)
            count[c] = 0u;
        int64_t p0 = lo;
        for (; p0 + 2 * CHI4_TILE <= hi; p0 += 2 * CHI4_TILE) { // whole loads, two at a time: twelve reads in flight
            const double r2 = chi4_r2(a, b, p0 + lane, n, keep);
            const double s2 = chi4_r2(a, b, p0 + CHI4_TILE + lane, n, keep);
#pragma unroll
            for (int c = 0; c < NC; ++c)
                count[c] += (unsigned int)(__popcll(__ballot(r2 <= cut.a2[c])) + __popcll(__ballot(s2 <= cut.a2[c])));
        }
        if (p0 + CHI4_TILE <= hi) {                             // one more whole load: every lane has a point
            const double r2 = chi4_r2(a, b, p0 + lane, n, keep);
#pragma unroll
            for (int c = 0; c < NC; ++c)
                count[c] += (unsigned int)__popcll(__ballot(r2 <= cut.a2[c]));
            p0 += CHI4_TILE;
        }
        if (p0 < hi) {                                          // the tail: lanes past the end contribute 0
            const bool live = p0 + lane < hi;
            const double r2 = chi4_r2(a, b, live ? p0 + lane : lo, n, keep);
#pragma unroll
            for (int c = 0; c < NC; ++c)
                count[c] += (unsigned int)__popcll(__ballot(live && r2 <= cut.a2[c]));
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (count[c])
                    atomicAdd(&out[g * NC + c], count[c]);     // integer adds commute
        }
    }
}

// S1 += Q, S2 += Q*Q over the slab's frame pairs.  Thread x = one (lag, group, cutoff) entry e of n_entries =
// n_lags * n_groups * n_cutoffs, grid y = runs of CHI4_FOLD_FRAMES frames; one pair of integer atomics per thread.
__global__ __launch_bounds__(256) void chi4_fold_kernel(const unsigned int *__restrict__ qslab, int n_frames,
                                                        int64_t n_entries, int per_lag,
                                                        const int64_t *__restrict__ lags, int64_t f_lo,
                                                        int64_t origin_step, unsigned long long *__restrict__ s1,
                                                        unsigned long long *__restrict__ s2)
{
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n_entries)
        return;
    const int64_t lag = lags[e / per_lag];
    const int i_lo = blockIdx.y * CHI4_FOLD_FRAMES;
    const int i_hi = i_lo + CHI4_FOLD_FRAMES < n_frames ? i_lo + CHI4_FOLD_FRAMES : n_frames;
    unsigned long long q1 = 0, q2 = 0;
    for (int i = i_lo; i < i_hi; ++i) {
        const int64_t f = f_lo + i;
        if (f < lag || (f - lag) % origin_step != 0)
            continue;
        const unsigned long long q = qslab[int64_t(i) * n_entries + e];
        q1 += q;
        q2 += q * q;
    }
    if (q1) {
        atomicAdd(&s1[e], q1);
        atomicAdd(&s2[e], q2);
    }
}

}  // namespace mdx_chi4_dev
