// mdx_sdf_device.hpp — device side of the spatial-distribution engine (mdx_sdf.hip).
//
// Result contract.
//
// Rows.  The incoming rows of a frame are n_rows distinct atoms.  The int32 tables name rows: o_row[n_ref],
// a_row[n_ref] and b_row[n_ref], the origin, the axis atom and the plane atom of every reference molecule (o_row
// holds no row twice, the three rows of a molecule differ pairwise); p_row[n_p], the partner atoms, group after
// group, with group_start[G + 1] non-decreasing from 0 to n_p and 1 <= G <= SDF_MAX_GROUPS (p_row holds no row
// twice); owner[n_p], the reference molecule partner j belongs to, or -1.  The pair (i, j) with owner[j] == i is never
// evaluated.
//
// Box and pair arithmetic: those of mdx_pairs_device.hpp, with one constant orthorhombic box and no dropped component.
// Everything is float64, one operation at a time; float32 coordinates are widened first.
//
// The frame of molecule i, from the positions O, A, B of o_row[i], a_row[i], b_row[i] in that frame:
//
//     a = min_image(A - O);  b = min_image(B - O)
//     mode AXIS:      p = a
//     mode BISECTOR:  p = a / sqrt(r2_of(a)) + b / sqrt(r2_of(b))     (component-wise: one sqrt, three divides per
//                                                                      vector, then three adds)
//     e1 = p / sqrt(r2_of(p))
//     c  = (p_y*b_z - p_z*b_y,  p_z*b_x - p_x*b_z,  p_x*b_y - p_y*b_x)     (each product rounded, then the subtraction)
//     e3 = c / sqrt(r2_of(c))
//     e2 = (e3_y*e1_z - e3_z*e1_y,  e3_z*e1_x - e3_x*e1_z,  e3_x*e1_y - e3_y*e1_x)      (not renormalised)
//
// sqrt and divide are correctly rounded.  A molecule whose e1, e2 or e3 has a non-finite component (an atom on
// another, the three atoms collinear) is degenerate in that frame: it adds 1 to `degenerate`, once per (frame,
// molecule), and none of its pairs count.
//
// Pair (i, j), with P the position of p_row[j]:
//
//     w  = min_image(P - O);  r2 = r2_of(w)
//     near   = r2 <= rc2  and  owner[j] != i  and  molecule i not degenerate
//     u = (w_x*e1_x + w_y*e1_y) + w_z*e1_z ;  v likewise with e2 ;  t likewise with e3
//     inside = near and ex[0] <= u <= ex[nx] and ey[0] <= v <= ey[ny] and ez[0] <= t <= ez[nz]
//     bin_x  = #{ m in 1 ... nx - 1 : u >= ex[m] }        (likewise y, z)
//
// rc2 = cutoff * cutoff is formed once on the host.  ex, ey, ez are strictly increasing float64 tables of n + 1 edges,
// n <= SDF_MAX_AXIS_BINS per axis: the rule of numpy.histogramdd, the last bin closed above.  u, v and t are formed
// only behind `near`.  A NaN is never inside.
//
// Results, all integers (uint64 in HBM, handed out as int64), added with integer atomics only:
//
//     counts[g][bin_x][bin_y][bin_z]   the inside pairs of group g
//     inside[f]                        the inside pairs of every analysed frame
//     degenerate                       as above
//
// evaluations is the contract's count F * (n_ref * n_p - #{(i, j) : owner[j] == i}), and sum counts == sum inside.
// G * nx * ny * nz may not exceed SDF_MAX_COUNTERS = 2^26 (512 MB of counters).
//
// u, v, t and the bins are functions of the frame alone, and every tally is an integer add (atomics on integers
// commute): the numbers are the same whatever the input route, the index, the split into calls or slabs, the grid, or
// the arrival order of the atomics.  There is no floating-point atomic anywhere in this engine.
//
// Shape.  gather_kernel gathers the rows of a slab of incoming frames, component-major float32; positions live only
// as long as the slab in flight.
// sdf_pair_kernel (the hot path, F * n_ref * n_p evaluations) is the walk of mdx_pairs_device.hpp with z = the frames
// of the slab, SDF_TILE reference molecules per block, one per lane, and SDF_JCHUNK partners per block.  A lane reads
// its O, A and B from the slab through the tables, once, widened, and forms e1, e2, e3 in the prologue (BISECTOR is
// known when compiled).  A degenerate lane walks with a bound of -1.0 in place of rc2, which no r2 meets: its pairs
// need no test of their own.  The thread that stages partner j reads slab[p_row[j]] (an indexed read) and puts
// owner[j], as a float64, into the fourth word of its stage entry, so that the exclusion is one compare.  The rule
// tests r2 <= rc2 first; only behind that test come the three dot products, the six compares against the outer edges
// (kernel arguments), the three bins (sdf_bin: a guess by one multiply, tested against its two edges, bisection
// where the edges are not evenly spaced) and one uint64 atomic into counts: a miss costs the 14 float64 operations of
// the other pair engines and the compare.  The edge tables live in LDS (3 x 513 doubles at most, read by the lanes
// that hit); the histogram does not fit LDS and is counted in HBM directly, where its accesses spread over the volume.
// The group of a hit comes from j against group_start (a kernel argument, padded with INT_MAX).  Each block adds its
// inside pairs to inside[f] with one integer atomic where not zero; the blocks of chunk 0 add their degenerate
// molecules to `degenerate` likewise.
//
// No cell list and no spatial culling: every (molecule, partner) pair is evaluated.  Culling by cells is the
// follow-up.
#pragma once

#include "mdx_pairs_device.hpp"

#include <climits>

namespace mdx_sdf_dev {

using namespace mdx_pairs_dev;

constexpr int SDF_TILE = PAIR_TILE;             // reference molecules per block, one per lane
constexpr int SDF_THREADS = PAIR_THREADS;
constexpr int SDF_STAGE = PAIR_STAGE;           // partners per LDS stage, one staged per thread
constexpr int SDF_JCHUNK = 4 * SDF_STAGE;       // partners per block
constexpr int SDF_MAX_GROUPS = 8;
constexpr int SDF_MAX_AXIS_BINS = 512;          // bins per axis at most: the edges of all three axes fit LDS
constexpr int64_t SDF_MAX_COUNTERS = int64_t(1) << 26;
constexpr int64_t SDF_SLAB_MAX = PAIR_SLAB_MAX; // frames per launch, at most (grid z)
constexpr int SDF_AXIS = 0, SDF_BISECTOR = 1;   // mode

// start[g]: the first partner of group g; start[g] = INT_MAX for g >= G
struct SdfGroups {
    int start[SDF_MAX_GROUPS];
};

// bins per axis: the one table ex | ey | ez holds n[0] + 1, n[1] + 1 and n[2] + 1 edges
struct SdfAxes {
    int n[3];
    double lo[3], hi[3];    // the first and the last edge: the test for `inside` reads no table
    double scale[3];        // n / (hi - lo): the guess of sdf_bin
};

// v / sqrt(r2_of(v)), component-wise
__device__ __forceinline__ void sdf_unit(double x, double y, double z, double &ux, double &uy, double &uz)
{
    const double len = __dsqrt_rn(r2_of(x, y, z));
    ux = __ddiv_rn(x, len);
    uy = __ddiv_rn(y, len);
    uz = __ddiv_rn(z, len);
}

// p x q, each product rounded, then the subtraction
__device__ __forceinline__ void sdf_cross(double px, double py, double pz, double qx, double qy, double qz, double &cx,
                                          double &cy, double &cz)
{
    cx = __dsub_rn(__dmul_rn(py, qz), __dmul_rn(pz, qy));
    cy = __dsub_rn(__dmul_rn(pz, qx), __dmul_rn(px, qz));
    cz = __dsub_rn(__dmul_rn(px, qy), __dmul_rn(py, qx));
}

__device__ __forceinline__ double sdf_dot(double wx, double wy, double wz, double ex, double ey, double ez)
{
    return __dadd_rn(__dadd_rn(__dmul_rn(wx, ex), __dmul_rn(wy, ey)), __dmul_rn(wz, ez));
}

__device__ __forceinline__ bool sdf_finite(double x, double y, double z)
{
    return isfinite(x) && isfinite(y) && isfinite(z);
}

// #{ m in 1 ... n - 1 : value >= e[m] } of the increasing edges e[0 ... n] by bisection: the inner edges that are
// <= value are a prefix
__device__ __forceinline__ int sdf_bin_search(const double *__restrict__ e, int n, double value)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (value >= e[mid + 1])
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// The same number for a value in [lo, e[n]], lo = e[0], from a guess: b = (value - lo) * scale with
// scale = n / (e[n] - lo) names the bin of evenly spaced edges up to rounding, so the guess or a neighbour of it is
// tested against its own two edges (b is the count where e[b] <= value < e[b + 1], the outermost bins open to the
// outside), and whatever fails that test (edges of unequal width) is bisected.  The guess decides nothing: the edges
// do.
__device__ __forceinline__ int sdf_bin(const double *__restrict__ e, int n, double lo, double scale, double value)
{
    int b = (int)((value - lo) * scale);
    b = b < 0 ? 0 : (b > n - 1 ? n - 1 : b);
    if (b > 0 && value < e[b])
        --b;
    else if (b < n - 1 && value >= e[b + 1])
        ++b;
    if ((b == 0 || value >= e[b]) && (b == n - 1 || value < e[b + 1]))
        return b;
    return sdf_bin_search(e, n, value);
}

// The wave's sum by shuffles, the block's in one LDS word (zero, and a barrier since); after the caller's next
// barrier *block_word holds the block's sum.
__device__ __forceinline__ void sdf_block_add(unsigned int value, unsigned int *block_word)
{
    for (int off = 32; off > 0; off >>= 1)
        value += __shfl_down(value, off);
    if ((threadIdx.x & 63) == 0 && value)
        atomicAdd(block_word, value);
}

// The inside pairs of frame f = f_lo + blockIdx.z among the rows of slab frame blockIdx.z.  n_rows: rows of a slab
// frame.  edges: ex[nx + 1] | ey[ny + 1] | ez[nz + 1] in HBM.  counts: uint64 [G][nx][ny][nz]; inside: uint64 [F];
// degenerate: one uint64.
template <bool BISECTOR>
__global__ __launch_bounds__(SDF_THREADS) void sdf_pair_kernel(
    const float *__restrict__ slab, int n_rows, int n_ref, int n_p, const int *__restrict__ o_row,
    const int *__restrict__ a_row, const int *__restrict__ b_row, const int *__restrict__ p_row,
    const int *__restrict__ owner, int n_jchunks, int64_t f_lo, PairBox box, double rc2, SdfGroups groups,
    const double *__restrict__ edges, SdfAxes axes, unsigned long long *__restrict__ counts,
    unsigned long long *__restrict__ inside, unsigned long long *__restrict__ degenerate)
{
    __shared__ __attribute__((aligned(16))) double stage[4 * SDF_STAGE];
    __shared__ double lds_edges[3 * (SDF_MAX_AXIS_BINS + 1)];
    __shared__ unsigned int block_found, block_degenerate;
    const int64_t f = f_lo + blockIdx.z;
    const int tile = blockIdx.x / n_jchunks, chunk = blockIdx.x - tile * n_jchunks;
    const int i = tile * SDF_TILE + threadIdx.x;
    const bool live = i < n_ref;
    const float *__restrict__ frame = slab + int64_t(blockIdx.z) * 3 * n_rows;
    const int nx = axes.n[0], ny = axes.n[1], nz = axes.n[2];
    const int n_edges = nx + ny + nz + 3;
    for (int m = threadIdx.x; m < n_edges; m += SDF_THREADS)
        lds_edges[m] = edges[m];
    if (threadIdx.x == 0) {
        block_found = 0u;
        block_degenerate = 0u;
    }
    const double *__restrict__ ex = lds_edges, *__restrict__ ey = ex + nx + 1, *__restrict__ ez = ey + ny + 1;

    // the lane's molecule: its origin and its frame
    const int mol = live ? i : n_ref - 1;
    const int ro = o_row[mol], ra = a_row[mol], rb = b_row[mol];
    const double xo = (double)frame[ro], yo = (double)frame[n_rows + ro], zo = (double)frame[2 * int64_t(n_rows) + ro];
    double ax, ay, az, bx, by, bz;
    min_image_of<true>((double)frame[ra], (double)frame[n_rows + ra], (double)frame[2 * int64_t(n_rows) + ra], xo, yo,
                       zo, box, 7, ax, ay, az);
    min_image_of<true>((double)frame[rb], (double)frame[n_rows + rb], (double)frame[2 * int64_t(n_rows) + rb], xo, yo,
                       zo, box, 7, bx, by, bz);
    double px = ax, py = ay, pz = az;
    if (BISECTOR) {
        double ux, uy, uz, vx, vy, vz;
        sdf_unit(ax, ay, az, ux, uy, uz);
        sdf_unit(bx, by, bz, vx, vy, vz);
        px = __dadd_rn(ux, vx);
        py = __dadd_rn(uy, vy);
        pz = __dadd_rn(uz, vz);
    }
    double e1x, e1y, e1z, cx, cy, cz, e3x, e3y, e3z, e2x, e2y, e2z;
    sdf_unit(px, py, pz, e1x, e1y, e1z);
    sdf_cross(px, py, pz, bx, by, bz, cx, cy, cz);
    sdf_unit(cx, cy, cz, e3x, e3y, e3z);
    sdf_cross(e3x, e3y, e3z, e1x, e1y, e1z, e2x, e2y, e2z);
    const bool sound = sdf_finite(e1x, e1y, e1z) && sdf_finite(e2x, e2y, e2z) && sdf_finite(e3x, e3y, e3z);
    const double reach = sound ? rc2 : -1.0;    // no r2 is <= -1.0: a degenerate molecule has no near pair
    const double me = (double)i;                // beside the staged owner[j]: the exclusion is one compare

    unsigned int found = 0u;
    const int j_begin = chunk * SDF_JCHUNK;
    const int j_end = n_p - j_begin < SDF_JCHUNK ? n_p : j_begin + SDF_JCHUNK;
    for (int js = j_begin; js < j_end; js += SDF_STAGE) {
        const int nj = j_end - js < SDF_STAGE ? j_end - js : SDF_STAGE;
        __syncthreads();                    // the stage is free (the first time: the edges and the words are there)
        if ((int)threadIdx.x < nj) {
            const int pr = p_row[js + threadIdx.x];
            stage[4 * threadIdx.x + 0] = (double)frame[pr];
            stage[4 * threadIdx.x + 1] = (double)frame[n_rows + pr];
            stage[4 * threadIdx.x + 2] = (double)frame[2 * int64_t(n_rows) + pr];
            stage[4 * threadIdx.x + 3] = (double)owner[js + threadIdx.x];
        }
        __syncthreads();
        if (!live)
            continue;
        stage_pairs<true>(stage, nj, js, -1, xo, yo, zo, box, 7,
                          [&](int jj, int j, double wx, double wy, double wz, double r2, bool) {
                              if (r2 <= reach && stage[4 * jj + 3] != me) {
                                  const double u = sdf_dot(wx, wy, wz, e1x, e1y, e1z);
                                  const double v = sdf_dot(wx, wy, wz, e2x, e2y, e2z);
                                  const double t = sdf_dot(wx, wy, wz, e3x, e3y, e3z);
                                  if (u >= axes.lo[0] && u <= axes.hi[0] && v >= axes.lo[1] && v <= axes.hi[1] &&
                                      t >= axes.lo[2] && t <= axes.hi[2]) {
                                      int g = 0;
#pragma unroll
                                      for (int m = 1; m < SDF_MAX_GROUPS; ++m)
                                          g += j >= groups.start[m];
                                      const int64_t cell =
                                          ((int64_t(g) * nx + sdf_bin(ex, nx, axes.lo[0], axes.scale[0], u)) * ny +
                                           sdf_bin(ey, ny, axes.lo[1], axes.scale[1], v)) * nz +
                                          sdf_bin(ez, nz, axes.lo[2], axes.scale[2], t);
                                      atomicAdd(&counts[cell], 1ull);
                                      ++found;
                                  }
                              }
                          });
    }
    sdf_block_add(found, &block_found);
    if (chunk == 0)
        sdf_block_add(live && !sound ? 1u : 0u, &block_degenerate);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (block_found)
            atomicAdd(&inside[f], (unsigned long long)block_found);
        if (block_degenerate)
            atomicAdd(degenerate, (unsigned long long)block_degenerate);
    }
}

}  // namespace mdx_sdf_dev
