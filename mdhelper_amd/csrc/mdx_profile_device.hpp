// mdx_profile_device.hpp — device side of the density-profile engine (mdx_profile.hip).
//
// Result contract (reference src/mdhelper/analysis/profile.py:775-818 with algorithm/topology.py
// `unwrap` / `wrap` and numpy.histogram), everything in float64 with separate multiply and add:
//
//     wrap:  if x < 0 or x > L:  x -= floor(x / L) * L          (x == L stays, a tiny negative x becomes L)
//     bin:   the b with e[b] <= x < e[b+1],  e[k] = k * (L / n_bins) for k < n_bins,  e[n_bins] = L;
//            the last bin is closed on the right; x outside [0, L] after the wrap (NaN, inf) is not counted
//
// which is numpy.histogram(x, n_bins, (0, L)) count for count.  The candidate index is one multiply, the
// fix-up compares against e[b] and e[b+1]; the division only runs for coordinates outside the box.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mdx_points_device.hpp"

namespace mdx_prof_dev {

constexpr int PROF_THREADS = 256;
constexpr int PROF_VEC_ITERS = 8;                          // float4 loads per thread and frame in the flat walk
constexpr int PROF_VEC_PER_BLOCK = PROF_THREADS * PROF_VEC_ITERS;
constexpr int PROF_POINTS_PER_BLOCK = PROF_THREADS * 4;

// per coordinate k of a point (0: x, 1: y, 2: z); n_bins == 0: the axis was not asked for
struct ProfAxis {
    double L, width, inv_width;   // box length, L / n_bins, n_bins / L
    int n_bins;
    int base;                     // first counter of the axis: slot = base + group * n_bins + bin
};

struct ProfPlan {
    ProfAxis ax[3];
    int n_groups;
    int n_slots;        // counters per frame row: n_groups * sum of n_bins
    int rep_shift;      // LDS replicas = 1 << rep_shift, replica r of slot s at word (s << rep_shift) | r
};

__device__ __forceinline__ int prof_bin(double x, double L, double width, double inv_width, int n_bins)
{
    if (x < 0.0 || x > L)
        x = __dsub_rn(x, __dmul_rn(floor(__ddiv_rn(x, L)), L));
    if (!(x >= 0.0 && x <= L))
        return -1;
    int b = (int)__dmul_rn(x, inv_width);
    b = b > n_bins - 1 ? n_bins - 1 : b;
    while (b > 0 && x < __dmul_rn((double)b, width))
        --b;
    while (b < n_bins - 1 && x >= __dmul_rn((double)(b + 1), width))
        ++b;
    return b;
}

// the group of point p: offs[g] <= p < offs[g + 1] (offs in LDS, empty groups allowed)
__device__ __forceinline__ int prof_group(const int *offs, int n_groups, int p)
{
    int lo = 0, hi = n_groups;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p >= offs[mid])
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Counters of one block: uint32 in LDS, REPLICAS interleaved copies of every slot (a lane adds to copy
// lane % REPLICAS, so lanes that hit one bin — a slab puts most particles into a few — spread over that
// many banks), or the global row itself when the slots do not fit.
template <typename CT, bool USE_LDS> struct ProfCounters {
    unsigned int *lds;
    CT *out;
    int rep_shift, rep;
    __device__ __forceinline__ void add(int slot) const
    {
        if (USE_LDS)
            atomicAdd(&lds[(slot << rep_shift) | rep], 1u);
        else
            atomicAdd(&out[slot], CT(1));
    }
};

template <typename CT, bool USE_LDS>
__device__ __forceinline__ void prof_count(const ProfCounters<CT, USE_LDS> &c, const ProfPlan &plan, int k, int g,
                                           double x)
{
    const int nb = prof_pick(k, plan.ax[0].n_bins, plan.ax[1].n_bins, plan.ax[2].n_bins);
    if (nb == 0)
        return;
    const double L = prof_pick(k, plan.ax[0].L, plan.ax[1].L, plan.ax[2].L);
    const double w = prof_pick(k, plan.ax[0].width, plan.ax[1].width, plan.ax[2].width);
    const double iw = prof_pick(k, plan.ax[0].inv_width, plan.ax[1].inv_width, plan.ax[2].inv_width);
    const int base = prof_pick(k, plan.ax[0].base, plan.ax[1].base, plan.ax[2].base);
    const int b = prof_bin(x, L, w, iw, nb);
    if (b >= 0)
        c.add(base + g * nb + b);
}

// LDS layout of both histogram kernels: [n_slots << rep_shift] counters (USE_LDS), then n_groups + 1 offsets
template <typename CT, bool USE_LDS>
__device__ __forceinline__ const int *prof_block_setup(unsigned int *lds, const ProfPlan &plan,
                                                       const int *__restrict__ offsets)
{
    const int n_words = USE_LDS ? plan.n_slots << plan.rep_shift : 0;
    for (int i = threadIdx.x; i < n_words; i += PROF_THREADS)
        lds[i] = 0u;
    int *offs = reinterpret_cast<int *>(lds + n_words);
    for (int i = threadIdx.x; i <= plan.n_groups; i += PROF_THREADS)
        offs[i] = offsets[i];
    __syncthreads();
    return offs;
}

// one integer atomic per non-empty slot and block: integer adds commute, so the totals do not depend on scheduling
template <typename CT, bool USE_LDS>
__device__ __forceinline__ void prof_block_flush(const unsigned int *lds, const ProfPlan &plan, CT *out)
{
    if (!USE_LDS)
        return;
    __syncthreads();
    const int reps = 1 << plan.rep_shift;
    for (int s = threadIdx.x; s < plan.n_slots; s += PROF_THREADS) {
        unsigned int sum = 0;
        for (int r = 0; r < reps; ++r)
            sum += lds[(s << plan.rep_shift) | r];
        if (sum)
            atomicAdd(&out[s], CT(sum));
    }
}

// Plain particles, all rows in group order, nothing to shift: the three coordinates of a point are independent, so
// the frame is walked as a flat float array with 16-byte loads; element e is coordinate e % 3 of point e / 3.
// Grid: x = pieces of PROF_VEC_PER_BLOCK float4 of a frame, y = runs of frames_per_block frames that share one set
// of LDS counters (1 when every frame has its own output row: out_stride = n_slots, else 0).
template <typename CT, bool USE_LDS>
__global__ __launch_bounds__(PROF_THREADS) void prof_hist_flat_kernel(
    const float *__restrict__ pos, int n_elems, int n_frames, int frames_per_block, ProfPlan plan,
    const int *__restrict__ offsets, CT *__restrict__ out, int64_t out_stride)
{
    extern __shared__ unsigned int prof_lds[];
    const int *offs = prof_block_setup<CT, USE_LDS>(prof_lds, plan, offsets);
    const int f0 = blockIdx.y * frames_per_block;
    const int f1 = min(n_frames, f0 + frames_per_block);
    out += int64_t(f0) * out_stride;
    ProfCounters<CT, USE_LDS> ctr{prof_lds, out, plan.rep_shift, int(threadIdx.x) & ((1 << plan.rep_shift) - 1)};
    const int ng = plan.n_groups;
    auto one = [&](int e, float v) {
        const int p = e / 3;
        prof_count(ctr, plan, e - 3 * p, ng > 1 ? prof_group(offs, ng, p) : 0, (double)v);
    };
    for (int f = f0; f < f1; ++f) {
        const float *__restrict__ row = pos + int64_t(f) * n_elems;
        // 16-byte loads start at the first aligned element of the frame; the few elements before it and after the
        // last whole float4 go one by one
        const int head = min(n_elems, int((4 - ((reinterpret_cast<uintptr_t>(row) >> 2) & 3)) & 3));
        const int n_vec = (n_elems - head) >> 2;
        const int v_lo = blockIdx.x * PROF_VEC_PER_BLOCK;
        const int v_hi = min(n_vec, v_lo + PROF_VEC_PER_BLOCK);
        for (int v = v_lo + threadIdx.x; v < v_hi; v += PROF_THREADS) {
            const int e0 = head + 4 * v;
            const float4 a = *reinterpret_cast<const float4 *>(row + e0);
            const int p0 = e0 / 3;
            int k = e0 - 3 * p0;
            const int g0 = ng > 1 ? prof_group(offs, ng, p0) : 0;
            const int g1 = ng > 1 ? prof_group(offs, ng, p0 + 1) : 0;
            int g = g0;
            const float vals[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                prof_count(ctr, plan, k, g, (double)vals[j]);
                if (++k == 3) {
                    k = 0;
                    g = g1;
                }
            }
        }
        if (blockIdx.x == 0) {
            const int t = threadIdx.x, tail0 = head + 4 * n_vec;
            if (t < head)
                one(t, row[t]);
            else if (t >= 64 && t - 64 < n_elems - tail0)
                one(tail0 + t - 64, row[tail0 + t - 64]);
        }
    }
    prof_block_flush<CT, USE_LDS>(prof_lds, plan, out);
}

// The general form, one thread per point: rows gathered through an index, float64 centres of mass, image counts
// and the per-frame shift of `recenter` (x + image * L - shift, the reference's order of operations).
template <typename SRC, typename CT, bool USE_LDS>
__global__ __launch_bounds__(PROF_THREADS) void prof_hist_points_kernel(
    const SRC *__restrict__ pos, int64_t src_rows, const int *__restrict__ index, int n_points, int n_frames,
    int frames_per_block, ProfPlan plan, const int *__restrict__ offsets, const int *__restrict__ images,
    const double *__restrict__ shift, CT *__restrict__ out, int64_t out_stride)
{
    extern __shared__ unsigned int prof_lds[];
    const int *offs = prof_block_setup<CT, USE_LDS>(prof_lds, plan, offsets);
    const int f0 = blockIdx.y * frames_per_block;
    const int f1 = min(n_frames, f0 + frames_per_block);
    out += int64_t(f0) * out_stride;
    ProfCounters<CT, USE_LDS> ctr{prof_lds, out, plan.rep_shift, int(threadIdx.x) & ((1 << plan.rep_shift) - 1)};
    const int p_lo = blockIdx.x * PROF_POINTS_PER_BLOCK;
    const int p_hi = min(n_points, p_lo + PROF_POINTS_PER_BLOCK);
    for (int p = p_lo + threadIdx.x; p < p_hi; p += PROF_THREADS) {
        const int64_t r = index ? index[p] : p;
        const int g = plan.n_groups > 1 ? prof_group(offs, plan.n_groups, p) : 0;
        for (int f = f0; f < f1; ++f) {
            const SRC *__restrict__ q = pos + (int64_t(f) * src_rows + r) * 3;
            double x[3] = {(double)q[0], (double)q[1], (double)q[2]};
            if (images) {
                const int *im = images + (int64_t(f) * n_points + p) * 3;
                x[0] = __dadd_rn(x[0], __dmul_rn((double)im[0], plan.ax[0].L));
                x[1] = __dadd_rn(x[1], __dmul_rn((double)im[1], plan.ax[1].L));
                x[2] = __dadd_rn(x[2], __dmul_rn((double)im[2], plan.ax[2].L));
            }
            if (shift) {
                x[0] = __dsub_rn(x[0], shift[3 * int64_t(f)]);
                x[1] = __dsub_rn(x[1], shift[3 * int64_t(f) + 1]);
                x[2] = __dsub_rn(x[2], shift[3 * int64_t(f) + 2]);
            }
            prof_count(ctr, plan, 0, g, x[0]);
            prof_count(ctr, plan, 1, g, x[1]);
            prof_count(ctr, plan, 2, g, x[2]);
        }
    }
    prof_block_flush<CT, USE_LDS>(prof_lds, plan, out);
}

// shift[frame][k] = scom_k - target_k (0 where target_k is NaN), scom the mass-weighted centre of the unwrapped
// points [p_lo, p_hi).  One block per frame; every thread sums its points in index order and the 256 partial sums
// fold in a fixed tree, so the centre — and with it every count — repeats bit for bit.
template <typename SRC>
__global__ __launch_bounds__(256) void prof_recenter_shift_kernel(
    const SRC *__restrict__ pos, int64_t src_rows, const int *__restrict__ index, int n_points, int p_lo, int p_hi,
    const double *__restrict__ masses, double total_mass, const int *__restrict__ images, double Lx, double Ly,
    double Lz, double tx, double ty, double tz, double *__restrict__ shift)
{
    __shared__ double red[3][256];
    const int f = blockIdx.x, t = threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int p = p_lo + t; p < p_hi; p += 256) {
        const int64_t r = index ? index[p] : p;
        const SRC *__restrict__ q = pos + (int64_t(f) * src_rows + r) * 3;
        const int *im = images + (int64_t(f) * n_points + p) * 3;
        const double m = masses[p - p_lo];
        acc[0] = __dadd_rn(acc[0], __dmul_rn(m, __dadd_rn((double)q[0], __dmul_rn((double)im[0], Lx))));
        acc[1] = __dadd_rn(acc[1], __dmul_rn(m, __dadd_rn((double)q[1], __dmul_rn((double)im[1], Ly))));
        acc[2] = __dadd_rn(acc[2], __dmul_rn(m, __dadd_rn((double)q[2], __dmul_rn((double)im[2], Lz))));
    }
    red[0][t] = acc[0];
    red[1][t] = acc[1];
    red[2][t] = acc[2];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            red[0][t] = __dadd_rn(red[0][t], red[0][t + s]);
            red[1][t] = __dadd_rn(red[1][t], red[1][t + s]);
            red[2][t] = __dadd_rn(red[2][t], red[2][t + s]);
        }
        __syncthreads();
    }
    if (t < 3) {
        const double target = prof_pick(t, tx, ty, tz);
        shift[3 * int64_t(f) + t] = target != target ? 0.0 : __dsub_rn(__ddiv_rn(red[t][0], total_mass), target);
    }
}

}  // namespace mdx_prof_dev
