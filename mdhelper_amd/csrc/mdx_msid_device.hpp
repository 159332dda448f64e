// mdx_msid_device.hpp — device side of the chain internal-distance engine (mdx_msid.hip).
//
// Result contract, everything in float64 with separate multiply and add; float32 coordinates are widened before any
// arithmetic.  Per frame and group of M chains of N >= 2 points x_{c,n} (x = (double)r + image * L under the global
// unwrap, the float64 monomer centres under a grouping, the chain made whole under `whole`, see below):
//
//     R2(s) = 1 / (M (N - s))     * sum_c sum_{i=0}^{N-1-s} |x_{c,i+s} - x_{c,i}|^2           s = 1 ... N-1
//     b_i   = x_{i+1} - x_i,   u_i = b_i / sqrt(b_i . b_i)   (u_i = 0 where b_i . b_i == 0)    i = 0 ... N-2
//     C(s)  = 1 / (M (N - 1 - s)) * sum_c sum_{i=0}^{N-2-s} u_{c,i} . u_{c,i+s}               s = 0 ... N-2
//
// with |d|^2 = (dx*dx + dy*dy) + dz*dz and a . b = (ax*bx + ay*by) + az*bz.  u_i is formed once per bond, three
// divisions by one square root.
//
// Summation order, fixed by the group sizes alone (no floating-point atomic, nothing that depends on scheduling):
//   1. per chain and separation one lane adds the terms one after the other, i = 0, 1, ..., starting from +0.0;
//   2. the chains a workgroup holds (its unit) are added in ascending chain order, starting from +0.0;
//   3. msid_rows_kernel adds the units of a group in ascending order, starting from +0.0, and divides once by the
//      integer M (N - s) resp. M (N - 1 - s), exact in float64.
// The units depend on (M, N) only (msid_chains_per_unit), so the rows repeat bit for bit whatever route the frames
// take, however they are split into calls and whatever the slab size is.
//
// Work layout.  A workgroup of 256 threads takes a unit of one frame: consecutive chains of one group, or one chain.
// It widens the unit's points once into LDS (structure of arrays), forms the unit bond vectors once into LDS, and
// spreads items over its lanes.  An item is (chain, j), j = 0 ... ceil(N / 2) - 1, and carries four sums:
// R2(j + 1) with R2(N - 1 - j), and C(j) with C(N - 1 - j).  Separation s has N - s terms and its partner N - s has
// s, so every lane walks N steps for the distances and N - 1 for the cosines, whatever j is: at step k it pairs
// point k with point (k + j + 1) mod N — separation j + 1 while k + j + 1 < N, the partner N - 1 - j after the index
// has wrapped (the pair then comes as x_i - x_{i+s}; the square is the same number) — and bond k with bond
// (k + j) mod (N - 1) likewise.  The middle separation (N even: s = N / 2; the cosines of N odd: s = (N - 1) / 2) is
// its own partner and is taken once: that lane stops where the index would wrap.  Lanes next to each other hold
// consecutive j, so x[(k + j + 1) mod N] is a run of consecutive doubles, free of bank conflicts inside a chain
// (ds_read_b64 serves 32 lanes per cycle from 64 banks of 4 B), and x[k] is a broadcast per chain.  Runs of
// different chains inside one half-wave, and a run that wraps, may meet on a bank (2-way); the chain stride is
// not padded.
//
// Short chains: a unit holds as many chains as give at most 256 items and at most MSID_STAGE points, so one turn of
// the lanes covers every (chain, j) of the unit; each lane puts its four sums into LDS (over the bond vectors, which
// are no longer read), and the lanes then add the chains of one row each, in ascending order.  A single chain
// (N > 256: more items than lanes, or the remainder of a group) needs no such sum: its lanes take the items in turns
// of 256 and write the rows themselves.
//
// Long chains: a chain of more than MSID_STAGE points is not staged.  Its lanes walk the same items and steps in the
// same order and read the points where they lie (HBM through L2), forming every unit bond vector again at each use
// from the same operations — the same bits as the staged path at several times its cost per step.  This path is
// plain on purpose; no limit is set on N.
//
// `whole` (msid_whole_kernel): every chain is made whole in every frame by itself, before the main kernel and in
// float64: x_0 = r_0; d = r_{n+1} - r_n per component; |d| >= L / 2 (the test of prof_unwrap_scan_kernel) moves d by
// -sign(d) * L; x_{n+1} = x_n + d.  One lane per (frame, chain, component) walks its chain and writes
// double[frames][points][3] into the slab scratch the grouped centres use (in place on the centres under a
// grouping); the main kernel then reads a double source.  Bonds must be shorter than half the shortest box length.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):
//   msid_unit_kernel<float>   56 VGPRs, no AGPRs, 50 SGPRs, no scratch, 49152 B of LDS, 3 waves per SIMD
//   msid_unit_kernel<double>  56 VGPRs, no AGPRs, 52 SGPRs, no scratch, 49152 B of LDS, 3 waves per SIMD
//   msid_whole_kernel         16 VGPRs, 26 SGPRs, no scratch, no LDS (float and double source alike)
//   msid_rows_kernel          16 VGPRs, 34 SGPRs, no scratch, no LDS
// 48 KiB of LDS per workgroup (6 * MSID_STAGE doubles): three workgroups (12 waves, 3 per SIMD) fit the 160 KiB of a
// CU, and LDS, not the register file, bounds the occupancy.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mdx_points_device.hpp"

namespace mdx_msid_dev {

constexpr int MSID_THREADS = 256;
constexpr int MSID_STAGE = 1024;     // points of a unit staged in LDS; a longer chain is read where it lies

// Chains of N points that one unit holds (mdx_msid_create builds the units with it): at most 256 items and
// MSID_STAGE points.
constexpr int64_t msid_chains_per_unit(int64_t N)
{
    const int64_t items = (N + 1) / 2;
    const int64_t by_items = MSID_THREADS / items, by_points = MSID_STAGE / N;
    const int64_t n = by_items < by_points ? by_items : by_points;
    return n < 1 ? 1 : n;
}

// What one workgroup works on: n_chains consecutive chains of one group.
struct MsidUnit {
    int point0;         // first point of the first chain
    int n_chains;
    int n_monomers;
    int pad;
    int64_t partial0;   // the unit's 2 (N - 1) partial rows inside a frame's partials
};

// What msid_rows_kernel turns into rows: the units of one group.
struct MsidGroup {
    int64_t partial0;   // first unit's partial rows inside a frame's partials
    int64_t row0;       // the group's first row inside a frame's rows: 2 sum_{h<g} (N_h - 1)
    int n_units;
    int n_monomers;
    int64_t n_chains;
};

__device__ __forceinline__ double msid_dot(const double a[3], const double b[3])
{
    return __dadd_rn(__dadd_rn(__dmul_rn(a[0], b[0]), __dmul_rn(a[1], b[1])), __dmul_rn(a[2], b[2]));
}

// u = (x1 - x0) / sqrt(|x1 - x0|^2), 0 for a bond of no length
__device__ __forceinline__ void msid_unit_bond(const double x0[3], const double x1[3], double u[3])
{
    const double b[3] = {__dsub_rn(x1[0], x0[0]), __dsub_rn(x1[1], x0[1]), __dsub_rn(x1[2], x0[2])};
    const double bb = msid_dot(b, b);
    const double len = __dsqrt_rn(bb);
    u[0] = bb == 0.0 ? 0.0 : __ddiv_rn(b[0], len);
    u[1] = bb == 0.0 ? 0.0 : __ddiv_rn(b[1], len);
    u[2] = bb == 0.0 ? 0.0 : __ddiv_rn(b[2], len);
}

// points and unit bond vectors of one chain, staged (chain at `base`) ...
struct MsidStaged {
    const double (*sx)[MSID_STAGE];
    const double (*su)[MSID_STAGE];
    int base;

    __device__ __forceinline__ void x(int i, double v[3]) const
    {
        v[0] = sx[0][base + i];
        v[1] = sx[1][base + i];
        v[2] = sx[2][base + i];
    }
    __device__ __forceinline__ void u(int i, double v[3]) const
    {
        v[0] = su[0][base + i];
        v[1] = su[1][base + i];
        v[2] = su[2][base + i];
    }
};

// ... or where they lie (the long-chain path)
template <typename SRC> struct MsidUnstaged {
    const mdx_prof_dev::PointSource<SRC> &src;
    int base;

    __device__ __forceinline__ void x(int i, double v[3]) const { src.load(base + i, v); }
    __device__ __forceinline__ void u(int i, double v[3]) const
    {
        double x0[3], x1[3];
        src.load(base + i, x0);
        src.load(base + i + 1, x1);
        msid_unit_bond(x0, x1, v);
    }
};

// The four sums of item j of a chain of N points: acc = {R2 sum of s = j + 1, of s = N - 1 - j, C sum of s = j, of
// s = N - 1 - j}; a sum that the item does not own stays 0 (msid_store knows which).
template <typename CHAIN>
__device__ __forceinline__ void msid_item(const CHAIN &chain, int N, int j, double acc[4])
{
    const int B = N - 1, sa = j + 1, sb = B - j;
    const int wrap_r = N - sa, wrap_c = B - j;                      // steps before the index wraps
    const int lim_r = sb > sa ? N : sb == sa ? wrap_r : 0;          // the middle separation once; none: N odd, last j
    const int lim_c = sb > j ? B : wrap_c;
    int ir = sa, ic = j;
    acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
    for (int k = 0; k < N; ++k) {
        if (k < lim_r) {
            double x0[3], x1[3];
            chain.x(k, x0);
            chain.x(ir, x1);
            const double d[3] = {__dsub_rn(x1[0], x0[0]), __dsub_rn(x1[1], x0[1]), __dsub_rn(x1[2], x0[2])};
            const double r2 = msid_dot(d, d);
            if (k < wrap_r)
                acc[0] = __dadd_rn(acc[0], r2);
            else
                acc[1] = __dadd_rn(acc[1], r2);
        }
        if (k < lim_c) {
            double u0[3], u1[3];
            chain.u(k, u0);
            chain.u(ic, u1);
            const double c = msid_dot(u0, u1);
            if (k < wrap_c)
                acc[2] = __dadd_rn(acc[2], c);
            else
                acc[3] = __dadd_rn(acc[3], c);
        }
        if (++ir == N)
            ir = 0;
        if (++ic >= B)
            ic = 0;
    }
}

// acc of item j into the 2 (N - 1) rows of a chain: R2(1 ... N-1), then C(0 ... N-2)
__device__ __forceinline__ void msid_store(double *__restrict__ rows, int N, int j, const double acc[4])
{
    const int B = N - 1, sa = j + 1, sb = B - j;
    if (sa <= sb)
        rows[sa - 1] = acc[0];
    if (sb > sa)
        rows[sb - 1] = acc[1];
    rows[B + j] = acc[2];
    if (sb > j && j >= 1)
        rows[B + sb] = acc[3];
}

// partials[frame][n_partial]: per unit the sums over its chains, not yet divided.  Grid: x = units, y = frames.
template <typename SRC>
__global__ __launch_bounds__(MSID_THREADS) void msid_unit_kernel(
    const SRC *__restrict__ pos, int64_t src_rows, const int *__restrict__ index, int n_points,
    const MsidUnit *__restrict__ units, const int *__restrict__ images, double Lx, double Ly, double Lz,
    int64_t n_partial, double *__restrict__ partials)
{
    __shared__ double sx[3][MSID_STAGE];
    __shared__ double su[3][MSID_STAGE];
    const MsidUnit unit = units[blockIdx.x];
    const int64_t f = blockIdx.y;
    const mdx_prof_dev::PointSource<SRC> src{pos + f * src_rows * 3, index,
                                             images ? images + f * 3 * int64_t(n_points) : nullptr, {Lx, Ly, Lz}};
    const int N = unit.n_monomers, B = N - 1, J = (N + 1) >> 1;
    double *__restrict__ part = partials + f * n_partial + unit.partial0;
    double acc[4];

    if (N > MSID_STAGE) {                       // one long chain, read where it lies
        const MsidUnstaged<SRC> chain{src, unit.point0};
        for (int j = threadIdx.x; j < J; j += MSID_THREADS) {
            msid_item(chain, N, j, acc);
            msid_store(part, N, j, acc);
        }
        return;
    }

    const int span = unit.n_chains * N;         // <= MSID_STAGE
    for (int q = threadIdx.x; q < span; q += MSID_THREADS) {
        double x[3];
        src.load(unit.point0 + q, x);
        sx[0][q] = x[0];
        sx[1][q] = x[1];
        sx[2][q] = x[2];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < span; q += MSID_THREADS) {
        if (q % N == B)
            continue;                           // the last point of a chain starts no bond
        const double x0[3] = {sx[0][q], sx[1][q], sx[2][q]}, x1[3] = {sx[0][q + 1], sx[1][q + 1], sx[2][q + 1]};
        double u[3];
        msid_unit_bond(x0, x1, u);
        su[0][q] = u[0];
        su[1][q] = u[1];
        su[2][q] = u[2];
    }
    __syncthreads();

    const int n_items = unit.n_chains * J;      // > MSID_THREADS only for a single chain
    if (unit.n_chains == 1) {
        const MsidStaged chain{sx, su, 0};
        for (int j = threadIdx.x; j < J; j += MSID_THREADS) {
            msid_item(chain, N, j, acc);
            msid_store(part, N, j, acc);
        }
        return;
    }
    const int item = threadIdx.x;
    const bool live = item < n_items;
    const int c = live ? item / J : 0;
    const int j = item - c * J;
    if (live)
        msid_item(MsidStaged{sx, su, c * N}, N, j, acc);
    __syncthreads();                            // the bond vectors have been read: their LDS takes the chains' rows
    double *chain_rows = &su[0][0];             // [n_chains][2 B], 2 B n_chains < 4 * MSID_THREADS doubles
    if (live)
        msid_store(chain_rows + c * 2 * B, N, j, acc);
    __syncthreads();
    for (int r = threadIdx.x; r < 2 * B; r += MSID_THREADS) {
        double sum = 0.0;
        for (int k = 0; k < unit.n_chains; ++k)
            sum = __dadd_rn(sum, chain_rows[k * 2 * B + r]);
        part[r] = sum;
    }
}

// rows[frame][n_rows] from the partials: the units of a group in ascending order, one division.
// Grid: x = groups, y = frames.
__global__ __launch_bounds__(MSID_THREADS) void msid_rows_kernel(const double *__restrict__ partials,
                                                                  int64_t n_partial,
                                                                  const MsidGroup *__restrict__ groups,
                                                                  int64_t n_rows, double *__restrict__ rows)
{
    const MsidGroup g = groups[blockIdx.x];
    const int64_t f = blockIdx.y;
    const int B = g.n_monomers - 1;
    const double *__restrict__ part = partials + f * n_partial + g.partial0;
    double *__restrict__ out = rows + f * n_rows + g.row0;
    for (int r = threadIdx.x; r < 2 * B; r += MSID_THREADS) {
        double sum = 0.0;
        for (int u = 0; u < g.n_units; ++u)
            sum = __dadd_rn(sum, part[int64_t(u) * 2 * B + r]);
        // R2(s), s = r + 1: N - s terms per chain;  C(s), s = r - B: N - 1 - s
        const int64_t terms = r < B ? g.n_monomers - (r + 1) : B - (r - B);
        out[r] = __ddiv_rn(sum, (double)(g.n_chains * terms));
    }
}

// `whole`: out[frame][point0 + chain * N + n][k] for the n_chains chains of N points from point0 on, every chain made
// whole from its first point (the rule in the header).  One lane per (chain, component); grid y = frames.  out may be
// pos itself (SRC = double, no index): a lane reads r_{n+1} before it writes x_{n+1} and no other lane touches
// either.
template <typename SRC>
__global__ __launch_bounds__(256) void msid_whole_kernel(const SRC *pos, int64_t src_rows,
                                                         const int *__restrict__ index, int n_points, int point0,
                                                         int n_chains, int N, double Lx, double Ly, double Lz,
                                                         double *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * n_chains)
        return;
    const int chain = i / 3, k = i - 3 * chain;
    const int64_t f = blockIdx.y;
    const SRC *p = pos + f * src_rows * 3 + k;
    double *o = out + f * int64_t(n_points) * 3 + k;
    const double L = mdx_prof_dev::prof_pick(k, Lx, Ly, Lz);
    const double half = L / 2;
    const int first = point0 + chain * N;
    double raw = (double)p[3 * (index ? int64_t(index[first]) : int64_t(first))];
    double x = raw;
    o[3 * int64_t(first)] = x;
    for (int n = 1; n < N; ++n) {
        const int q = first + n;
        const double next = (double)p[3 * (index ? int64_t(index[q]) : int64_t(q))];
        double d = __dsub_rn(next, raw);
        if (fabs(d) >= half)
            d = d > 0.0 ? __dsub_rn(d, L) : __dadd_rn(d, L);
        x = __dadd_rn(x, d);
        o[3 * int64_t(q)] = x;
        raw = next;
    }
}

}  // namespace mdx_msid_dev
