// mdx_rdf.hip — radial pair-distance histogram on gfx950 (MI355X).
//
// Carries reference src/mdhelper/analysis/structure.py:32-104 (radial_histogram:
// capped pair search + exclusion + numpy.histogram) for a batch of frames, i.e.
// the `counts +=` body of RadialDistributionFunction._single_frame (:750-791).
//
// Result contract: for every ordered pair (i, j)
//     fd  = (float)(x_j - x_i)                       float32 subtract
//     s   = (double)(float)(1.0 / L) * (double)fd     exact in double
//     w   = (double)L * (s - round(s))                one rounding
//     rsq = (w_x*w_x + w_y*w_y) + w_z*w_z             no FMA contraction
//     d   = sqrt(rsq);   kept when  r0 - eps < d <= r1  and  i/e0 != j/e1
//     bin = numpy.histogram(d, n_bins, (r0, r1))
// Bin *decisions* are bit-exact with that contract.  Nothing here computes a
// double sqrt: sqrt is monotone, so every comparison `d >= edge` is replaced by
// `rsq >= T(edge)` with T(edge) = the smallest double whose correctly rounded
// sqrt is >= edge (computed on the host, see make_thresholds()).
//
// Three pair kernels share one skeleton (LDS-staged j tile read by broadcast,
// i atoms in registers, per-wave LDS histograms, one uint64 flush per block):
//   EXACT   the contract arithmetic on every pair (fp64 VALU bound);
//   FILTER  float32 distance with a proven error bound; only pairs whose
//           float32 distance falls within that bound of a bin edge (or of the
//           range ends) are re-evaluated with the contract arithmetic;
//   CELL    (mdx_rdf_cell.hip) cell-sorted tiles with culled tile pairs on
//           top of FILTER.
//
// This translation unit is compiled with -ffp-contract=off.

#include "mdx_common.hpp"
#include "mdx_internal.hpp"
#include "mdx_molecules.hpp"
#include "mdx_rdf_device.hpp"
#include "mdx_rdf_cell.hpp"
#include "mdx_traj.hpp"

#include <cstring>
#include <cmath>

namespace mdx {

// ---------------------------------------------------------------- host helpers

// smallest double t >= 0 with sqrt(t) >= e   (e >= 0; IEEE sqrt is correctly rounded)
static double thresh_ge(double e)
{
    if (!(e > 0.0))
        return 0.0;
    double t = e * e;
    while (std::sqrt(t) >= e && t > 0.0)
        t = std::nextafter(t, 0.0);
    while (std::sqrt(t) < e)
        t = std::nextafter(t, INFINITY);
    return t;
}

// smallest double t with sqrt(t) > e
static double thresh_gt(double e)
{
    if (e < 0.0)
        return 0.0;
    return thresh_ge(std::nextafter(e, INFINITY));
}

}  // namespace mdx

using namespace mdx;

// ------------------------------------------------------------------- kernels

// xyz float32[F][n][3] -> float4[F][n_pad] with w = exclusion tag; pads are NaN.
// Also folds max |coordinate| into *maxabs_bits (non-negative floats order as ints).
__global__ __launch_bounds__(256) void rdf_pack_kernel(const float *__restrict__ pos,
                                                       float4 *__restrict__ out, int n, int n_pad,
                                                       int64_t excl, unsigned *maxabs_bits)
{
    const int frame = blockIdx.y;
    const int a = blockIdx.x * 256 + threadIdx.x;
    float m = 0.0f;
    if (a < n_pad) {
        float4 v;
        if (a < n) {
            const float *p = pos + (int64_t(frame) * n + a) * 3;
            v.x = p[0];
            v.y = p[1];
            v.z = p[2];
            int tag = excl > 0 ? int(int64_t(a) / excl) : a;
            v.w = __int_as_float(tag);
            m = fmaxf(fabsf(v.x), fmaxf(fabsf(v.y), fabsf(v.z)));
        } else {
            v.x = v.y = v.z = __int_as_float(0x7fc00000);
            v.w = __int_as_float(-1);
        }
        out[int64_t(frame) * n_pad + a] = v;
    }
    // NaN/inf coordinates propagate into the bound and force the exact path
    unsigned bits = __float_as_uint(m == m ? m : __int_as_float(0x7f800000));
    for (int off = 32; off > 0; off >>= 1)
        bits = max(bits, (unsigned)__shfl_xor((int)bits, off));
    if ((threadIdx.x & 63) == 0 && bits)
        atomicMax(maxabs_bits, bits);
}

// status bit 0: non-orthorhombic or non-positive box
__global__ void rdf_check_boxes_kernel(const float *__restrict__ boxes, int64_t n_frames,
                                       unsigned *status)
{
    int64_t f = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (f >= n_frames)
        return;
    const float *b = boxes + f * 6;
    bool ok = b[0] > 0.f && b[1] > 0.f && b[2] > 0.f && b[3] == 90.f && b[4] == 90.f &&
              b[5] == 90.f;
    if (!ok)
        atomicOr(status, 1u);
}

// GH: the histogram (and the threshold table) stay in global memory — only for bin
// counts whose tables do not fit the LDS budget.
template <int MODE, int IPT, bool PBC, bool EXCL, bool GH>
__global__ __launch_bounds__(256) void rdf_tile_kernel(RdfArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    constexpr int T = 256 * IPT;
    float4 *sj = reinterpret_cast<float4 *>(smem_raw);                       // [T]
    double *sT = reinterpret_cast<double *>(smem_raw + sizeof(float4) * T);  // [n_bins+1]
    unsigned *sh = reinterpret_cast<unsigned *>(sT + (a.n_bins + 1));        // [n_hist][n_bins]
    __shared__ unsigned s_exact;

    const int tid = threadIdx.x;
    const int frame = blockIdx.z + a.frame0;
    const int I = blockIdx.y;
    int J0 = blockIdx.x * a.chunk;
    int J1 = min(J0 + a.chunk, a.nt2);
    if (a.self)
        J0 = max(J0, I);
    if (J0 >= J1)
        return;

    if (!GH) {
        for (int b = tid; b <= a.n_bins; b += 256)
            sT[b] = a.thresh[b];
        for (int b = tid; b < a.n_hist * a.n_bins; b += 256)
            sh[b] = 0u;
    }
    if (tid == 0)
        s_exact = 0u;

    PairCtx<PBC> ctx;
    ctx.init(a, frame);
    unsigned long long *out =
        a.counts + int64_t((blockIdx.x + 3 * blockIdx.y + 7 * blockIdx.z) % a.n_rep) * a.n_bins;
    const double *thr = GH ? a.thresh : sT;
    HistLds hl{sh + (GH ? 0 : ((tid >> 6) % a.n_hist) * a.n_bins)};
    HistGlobal hg{out};

    float4 pi[IPT];
    const float4 *P1 = a.p1 + int64_t(frame) * a.n1p + int64_t(I) * T;
#pragma unroll
    for (int u = 0; u < IPT; ++u)
        pi[u] = P1[tid + 256 * u];

    unsigned n_exact = 0;
    for (int J = J0; J < J1; ++J) {
        const float4 *P2 = a.p2 + int64_t(frame) * a.n2p + int64_t(J) * T;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < IPT; ++u)
            sj[tid + 256 * u] = P2[tid + 256 * u];
        __syncthreads();
        const unsigned w = (a.self && J != I) ? 2u : 1u;
#pragma unroll 4
        for (int jj = 0; jj < T; ++jj) {
            const float4 pj = sj[jj];
#pragma unroll
            for (int u = 0; u < IPT; ++u) {
                if (MODE == MDX_RDF_ALGO_EXACT_F64) {
                    if (GH) pair_exact<PBC, EXCL>(ctx, a, thr, hg, pi[u], pj, w);
                    else pair_exact<PBC, EXCL>(ctx, a, thr, hl, pi[u], pj, w);
                } else {
                    if (GH) pair_filter<PBC, EXCL>(ctx, a, thr, hg, pi[u], pj, w, n_exact);
                    else pair_filter<PBC, EXCL>(ctx, a, thr, hl, pi[u], pj, w, n_exact);
                }
            }
        }
    }
    __syncthreads();
    if (MODE != MDX_RDF_ALGO_EXACT_F64) {
        for (int off = 32; off > 0; off >>= 1)
            n_exact += __shfl_xor((int)n_exact, off);
        if ((tid & 63) == 0 && n_exact)
            atomicAdd(&s_exact, n_exact);
        __syncthreads();
        if (tid == 0 && s_exact)
            atomicAdd(a.exact_counter + rdf_stat_offset(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)),
                      (unsigned long long)s_exact);
    }
    if (!GH) {
        for (int b = tid; b < a.n_bins; b += 256) {
            unsigned long long s = 0;
            for (int h = 0; h < a.n_hist; ++h)
                s += sh[h * a.n_bins + b];
            if (s)
                atomicAdd(out + b, s);
        }
    }
}

// ------------------------------------------------------------------ triclinic cells
//
// Contract (restating MDAnalysis' brute-force triclinic path):
// both sets are moved into the central cell (c, then b, then a axis; double arithmetic on the
// float32 coordinates, result stored as float32), dx = (double)(float)(x_j - x_i), and the
// squared distance is the strictly smallest of the 27 images dx + ix a + iy b + iz c scanned in
// double with ix outermost.  tri: float[frames][9], row-major lower-triangular cell matrix.
__global__ __launch_bounds__(256) void rdf_tri_pack_kernel(const float *__restrict__ pos,
                                                           const float *__restrict__ tri,
                                                           float4 *__restrict__ out, int n,
                                                           int n_pad, int64_t excl)
{
    const int frame = blockIdx.y;
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n_pad)
        return;
    float4 v;
    if (a < n) {
        const float *p = pos + (int64_t(frame) * n + a) * 3;
        const float *B = tri + int64_t(frame) * 9;
        double r[3] = {(double)p[0], (double)p[1], (double)p[2]};
#pragma unroll
        for (int k = 2; k >= 0; --k) {
            const double s = floor(r[k] / (double)B[4 * k]);
#pragma unroll
            for (int c = 0; c <= k; ++c)
                r[c] -= s * (double)B[3 * k + c];
        }
        v.x = (float)r[0];
        v.y = (float)r[1];
        v.z = (float)r[2];
        v.w = __int_as_float(excl > 0 ? int(int64_t(a) / excl) : a);
    } else {
        v.x = v.y = v.z = __int_as_float(0x7fc00000);
        v.w = __int_as_float(-1);
    }
    out[int64_t(frame) * n_pad + a] = v;
}

struct TriArgs {
    const float4 *p1, *p2;
    const float *tri;
    const double *thresh;
    unsigned long long *counts;
    double t_lo, t_hi;
    float r0f, inv_wf;
    int n1p, n2p, nt1, nt2;
    int n_bins, n_hist, n_rep;
    int chunk, self, frame0;
};

template <bool EXCL, bool GH>
__global__ __launch_bounds__(256) void rdf_tri_tile_kernel(TriArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    float4 *sj = reinterpret_cast<float4 *>(smem_raw);                         // [256]
    double *sT = reinterpret_cast<double *>(smem_raw + sizeof(float4) * 256);  // [n_bins+1]
    unsigned *sh = reinterpret_cast<unsigned *>(sT + (a.n_bins + 1));          // [n_hist][n_bins]

    const int tid = threadIdx.x;
    const int frame = blockIdx.z + a.frame0;
    const int I = blockIdx.y;
    int J0 = blockIdx.x * a.chunk;
    int J1 = min(J0 + a.chunk, a.nt2);
    if (a.self)
        J0 = max(J0, I);
    if (J0 >= J1)
        return;
    if (!GH) {
        for (int b = tid; b <= a.n_bins; b += 256)
            sT[b] = a.thresh[b];
        for (int b = tid; b < a.n_hist * a.n_bins; b += 256)
            sh[b] = 0u;
    }
    const float *Bf = a.tri + int64_t(frame) * 9;
    const double b00 = Bf[0], b10 = Bf[3], b11 = Bf[4], b20 = Bf[6], b21 = Bf[7], b22 = Bf[8];
    unsigned long long *out =
        a.counts + int64_t((blockIdx.x + 3 * blockIdx.y + 7 * blockIdx.z) % a.n_rep) * a.n_bins;
    const double *thr = GH ? a.thresh : sT;
    HistLds hl{sh + (GH ? 0 : ((tid >> 6) % a.n_hist) * a.n_bins)};
    HistGlobal hg{out};
    const float4 pi = a.p1[int64_t(frame) * a.n1p + int64_t(I) * 256 + tid];

    for (int J = J0; J < J1; ++J) {
        __syncthreads();
        sj[tid] = a.p2[int64_t(frame) * a.n2p + int64_t(J) * 256 + tid];
        __syncthreads();
        const unsigned w = (a.self && J != I) ? 2u : 1u;
        for (int jj = 0; jj < 256; ++jj) {
            const float4 pj = sj[jj];
            const double dx = (double)(pj.x - pi.x), dy = (double)(pj.y - pi.y),
                         dz = (double)(pj.z - pi.z);
            double best = 1.0e300;
#pragma unroll
            for (int ix = -1; ix < 2; ++ix) {
                const double rx = dx + b00 * (double)ix;
#pragma unroll
                for (int iy = -1; iy < 2; ++iy) {
                    const double ry0 = rx + b10 * (double)iy;
                    const double ry1 = dy + b11 * (double)iy;
#pragma unroll
                    for (int iz = -1; iz < 2; ++iz) {
                        const double rz0 = ry0 + b20 * (double)iz;
                        const double rz1 = ry1 + b21 * (double)iz;
                        const double rz2 = dz + b22 * (double)iz;
                        const double dsq = (rz0 * rz0 + rz1 * rz1) + rz2 * rz2;
                        best = dsq < best ? dsq : best;
                    }
                }
            }
            // NaN (padding) fails both comparisons
            bool in = (best >= a.t_lo) && (best < a.t_hi);
            if (EXCL)
                in = in && (__float_as_int(pi.w) != __float_as_int(pj.w));
            if (in) {
                const int k = rdf_bin_exact(best, thr, a.n_bins, a.r0f, a.inv_wf);
                if (GH) hg.add(k, w);
                else hl.add(k, w);
            }
        }
    }
    __syncthreads();
    if (!GH) {
        for (int b = tid; b < a.n_bins; b += 256) {
            unsigned long long s = 0;
            for (int h = 0; h < a.n_hist; ++h)
                s += sh[h * a.n_bins + b];
            if (s)
                atomicAdd(out + b, s);
        }
    }
}

__global__ void rdf_reduce_kernel(const unsigned long long *__restrict__ rep, int n_rep, int n_bins,
                                  unsigned long long *__restrict__ total)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bins)
        return;
    unsigned long long s = 0;
    for (int r = 0; r < n_rep; ++r)
        s += rep[int64_t(r) * n_bins + b];
    total[b] = s;
}

// -------------------------------------------------------------- host planning
//
// Every choice among the pair kernels' instantiations, their histogram form, the padded sizes and the slab lengths is
// a pure function of the engine's arguments, the set sizes, the frames' cells and the environment.  rdf_plan_run makes
// them all, once per run, into an RdfRunPlan: the routes launch from that struct and mdx_rdf_plan (which touches no
// device) copies it out, so what the query says is what runs.

enum {
    RDF_FAMILY_TILE_EXACT = 0,   // rdf_tile_kernel<MDX_RDF_ALGO_EXACT_F64, ...>
    RDF_FAMILY_TILE_FILTER = 1,  // rdf_tile_kernel<MDX_RDF_ALGO_FILTER_F32, ...>
    RDF_FAMILY_CELL_ORTHO = 2,   // rdf_cell_pair_kernel<..., TRI = false, ...>
    RDF_FAMILY_TRI_BRUTE = 3,    // rdf_tri_tile_kernel
    RDF_FAMILY_TRI_CULLED = 4    // rdf_cell_pair_kernel<..., TRI = true>
};

constexpr size_t RDF_LDS_BUDGET = 64 * 1024;      // dynamic LDS of one block: keeps >= 2 blocks per CU resident
constexpr size_t RDF_LDS_ATTR_LINE = 48 * 1024;   // above it the tile kernels ask for the size with hipFuncSetAttribute
constexpr int64_t RDF_MAX_SLAB = 32768;           // frames per slab of every route: no grid z beyond it

// The pair kernel's step that leaves when none of its 64 pairs is a candidate (cell_step<..., SKIP>) pays one
// scalar branch per step for the tail of the empty steps.  Fitted to the A/B series of round 7 (NOTES.md), a skipped
// tail is worth 0.44 of a step and the branch costs 0.05: the step pays where more than 0.12 of the steps of the
// shifted row loops are empty.  That share falls as the range grows against the 64-particle units — modelled at the
// bench's density (scripts/cull_model.py): 0.17 at a range end of 0.22 L (C2(i): faster), 0.14 at 0.30 L, 0.12 at
// 0.35 L, 0.07 at 0.5 L (C2(ii): slower) — so the launch takes the step up to 0.3 of the SHORTEST box length over its
// frames and the unconditional tail beyond.  min_edge: that length (0 = not known: unconditional tail).
constexpr float CELL_SKIP_MAX_RANGE = 0.3f;
constexpr int CELL_FIXED_MAX_BINS = 32766;   // the LDS form's bin position is 16.16 fixed point (rdf_cell_hist)

// the histogram of one pair kernel: LDS replicas, or the global form where the tables do not fit
struct RdfHist {
    int n_hist = 0;       // LDS replicas (what the kernel is told; unused by the global form)
    bool gh = false;      // tables too large for LDS: thresholds and histogram stay in global memory
    size_t lds = 0;       // dynamic LDS bytes of the launch
};

// brute-force tiles (rdf_tile_kernel with T = 256 IPT rows, rdf_tri_tile_kernel with T = 256): the j tile, the
// thresholds and up to four per-wave histograms
static RdfHist rdf_tile_hist(int n_bins, int T)
{
    const size_t base = sizeof(float4) * T + sizeof(double) * (size_t(n_bins) + 1);
    RdfHist r;
    r.n_hist = 4;
    while (r.n_hist > 1 && base + size_t(r.n_hist) * n_bins * 4 > RDF_LDS_BUDGET)
        r.n_hist >>= 1;
    r.lds = base + size_t(r.n_hist) * n_bins * 4;
    r.gh = r.lds > RDF_LDS_BUDGET;
    if (r.gh)
        r.lds = sizeof(float4) * T;
    return r;
}

// cell-sorted pair kernel: 4 wave slabs + thresholds + the histogram in n_hist interleaved replicas (HistLdsRep):
// 8 while seven blocks of a CU still fit (the kernel's static LDS is 8 992 B), fewer for long bin tables
static RdfHist rdf_cell_hist(int n_bins)
{
    const size_t base = sizeof(float4) * 256 + sizeof(double) * (size_t(n_bins) + 1);
    const size_t lds_seven_blocks = 13 * 1024;   // (160 KB / 7 = 22.8 KB) - 8.8 KB static = 14.0 KB
    const size_t words = size_t(cell_hist_stride(n_bins));
    RdfHist r;
    r.n_hist = 8;
    while (r.n_hist > 4 && base + size_t(r.n_hist) * words * 4 > lds_seven_blocks)
        r.n_hist >>= 1;
    while (r.n_hist > 1 && base + size_t(r.n_hist) * words * 4 > RDF_LDS_BUDGET)
        r.n_hist >>= 1;
    r.lds = base + size_t(r.n_hist) * words * 4;
    // The LDS form bins in 16.16 fixed point (cell_fixed_q): the bin is the high half of a signed 32-bit value, so
    // n_bins + 1 <= 32 767.  The budget above is the tighter bound by far (some 5 000 bins); stated, not relied on.
    r.gh = r.lds > RDF_LDS_BUDGET || n_bins > CELL_FIXED_MAX_BINS;
    if (r.gh)
        r.lds = sizeof(float4) * 256;
    return r;
}

// orthorhombic frames (or none): the pair kernel an algorithm stands for
static int rdf_resolve_ortho_algo(int algo, bool has_boxes)
{
    // AUTO: the cell-sorted kernel whenever there is a periodic box — at every size.  Below 1 024 particles the
    // tiles cannot be culled (the cutoff spans the cell), but its hot step (13 VALU instructions + the
    // hand-placed tail per 64 evaluations, symmetric tile pairs evaluated once) is what the brute-force tile kernel
    // spends 48 on: measured 1.1 x (16 particles) .. 3.4 x (1 000 particles, range to L/2: 0.88 -> 3.0 M frames/s)
    // the frames per second, counts identical (scripts/diag/rdf_small_sweep.py, round 4).  Without a box: the
    // brute-force tiles with the float32 filter.
    if (algo == MDX_RDF_ALGO_AUTO)
        algo = has_boxes ? MDX_RDF_ALGO_CELL : MDX_RDF_ALGO_FILTER_F32;
    if (algo == MDX_RDF_ALGO_CELL && !has_boxes)
        algo = MDX_RDF_ALGO_FILTER_F32;   // the cell grid is defined by the periodic box
    return algo;
}

// frames per slab of the cell-sorted routes for a call of n_frames frames
static int64_t rdf_cell_slab_frames(int64_t n1p, int64_t n2p, bool self, int64_t n_frames)
{
    // per frame: wrapped + original float4 copies, one box per 64 and per 16 particles
    // (two-particle chunks take their boxes from the staged rows: no chunk-box array)
    constexpr int64_t CHUNK_BOX_BYTES = CELL_CHUNK >= 4 ? 32 / CELL_CHUNK : 0;
    const int64_t per_frame = (32 + 1 + CHUNK_BOX_BYTES) * (n1p + (self ? 0 : n2p));
    // (MDX_RDF_SLAB_BYTES: test hook, so that small inputs run through several slabs and both sets)
    const char *slab_env = getenv("MDX_RDF_SLAB_BYTES");
    // (2.5 GiB = 2 304 frames at C2: the persistent kernel ends on a tail of about one item per block, so long
    // launches pay — measured while the sort between two launches was still serial: 1 024 frames 45.3 k, 2 048
    // 45.6–45.8 k, 4 096 45.7 k frames/s)
    const int64_t slab_bytes = slab_env ? std::max<int64_t>(1, atoll(slab_env)) : (int64_t(5) << 29);
    int64_t slab = std::max<int64_t>(1, slab_bytes / per_frame);
    slab = std::min<int64_t>(slab, RDF_MAX_SLAB);
    // whole rounds of the sort kernel: one 1 024-thread block per frame, one block per CU (65 VGPRs) —
    // 993 frames were 3.9 rounds of 256 CUs and took 4
    if (slab >= 256)
        slab -= slab % 256;
    return std::min<int64_t>(slab, n_frames);
}

// Items of the cell-sorted pair kernel: an i tile against a chunk of its candidate j tiles — every `chunks`-th of
// them, so that each of an i tile's items gets its share of the tiles that survive the cull, which lie close
// together.  A wave takes an item through alone, and a launch ends with its longest items: where nearly every tile
// survives (the launches beyond the skipping step's range) a chunk is as many tiles as one cull pass tests, 64 —
// about what a block took over a whole i tile; elsewhere a quarter of the j tiles: four items to an i tile, as four
// waves shared it before.  (MDX_RDF_CHUNK_TILES, tiles per chunk: test hook.)  Returns the items of an i tile;
// *tiles_per_chunk: the 64-row j tiles of one.
static int rdf_cell_chunks(int64_t n2p, bool skip, int64_t *tiles_per_chunk)
{
    const char *ct = getenv("MDX_RDF_CHUNK_TILES");
    int64_t c = ct ? atoll(ct) : (skip ? ceil_div(n2p / 64, 4) : 64);
    c = ceil_div(std::max<int64_t>(c, 1), 64) * 64;
    c = std::min<int64_t>(c, ceil_div(n2p / 64, 64) * 64);
    if (tiles_per_chunk)
        *tiles_per_chunk = c;
    return (int)ceil_div(n2p / 64, c);
}

// cell matrix of (lx, ly, lz, alpha, beta, gamma): float64 arithmetic through libm, float32
// entries, exact zeros for right angles
static void tri_vectors(const float *box6, float *B)
{
    const double lx = box6[0], ly = box6[1], lz = box6[2];
    const double deg = 3.14159265358979323846 / 180.0;
    const double ca = box6[3] == 90.0f ? 0.0 : std::cos((double)box6[3] * deg);
    const double cb = box6[4] == 90.0f ? 0.0 : std::cos((double)box6[4] * deg);
    const double cg = box6[5] == 90.0f ? 0.0 : std::cos((double)box6[5] * deg);
    const double sg = box6[5] == 90.0f ? 1.0 : std::sin((double)box6[5] * deg);
    for (int i = 0; i < 9; ++i)
        B[i] = 0.0f;
    B[0] = (float)lx;
    B[3] = (float)(ly * cg);
    B[4] = (float)(ly * sg);
    const double cx = lz * cb;
    const double cy = lz * (ca - cb * cg) / sg;
    B[6] = (float)cx;
    B[7] = (float)cy;
    B[8] = (float)std::sqrt(lz * lz - cx * cx - cy * cy);
}

static inline bool box_is_ortho(const float *b) { return b[3] == 90.f && b[4] == 90.f && b[5] == 90.f; }

// A batch is dispatched in runs of one cell kind: the run that starts at frame f0 ends before the returned frame.
// *ortho: its kind; *min_edge: the shortest box length over its frames (CELL_SKIP_MAX_RANGE; orthorhombic runs only).
static int64_t rdf_next_run(const float *h_boxes, int64_t f0, int64_t n_frames, bool *ortho, float *min_edge)
{
    *ortho = box_is_ortho(h_boxes + 6 * f0);
    int64_t f1 = f0 + 1;
    while (f1 < n_frames && box_is_ortho(h_boxes + 6 * f1) == *ortho)
        ++f1;
    *min_edge = h_boxes[6 * f0];
    for (int64_t f = f0; f < f1; ++f)
        *min_edge = std::min(*min_edge, std::min(h_boxes[6 * f], std::min(h_boxes[6 * f + 1], h_boxes[6 * f + 2])));
    return f1;
}

// the cell matrices float[n_frames][9] of a run of triclinic frames, or why a frame has none
static int rdf_tri_cells(const float *h_boxes, int64_t n_frames, std::vector<float> &tri)
{
    tri.resize(size_t(9) * n_frames);
    for (int64_t f = 0; f < n_frames; ++f) {
        const float *b = h_boxes + 6 * f;
        if (!(b[0] > 0.f && b[1] > 0.f && b[2] > 0.f && b[3] > 0.f && b[3] < 180.f && b[4] > 0.f &&
              b[4] < 180.f && b[5] > 0.f && b[5] < 180.f))
            return fail(MDX_ERR_INVALID_VALUE, "frame %lld: invalid cell (%g %g %g %g %g %g)",
                        (long long)f, b[0], b[1], b[2], b[3], b[4], b[5]);
        tri_vectors(b, tri.data() + 9 * f);
        if (!(tri[9 * f + 8] > 0.f) || !(tri[9 * f + 4] > 0.f))
            return fail(MDX_ERR_INVALID_VALUE, "frame %lld: the cell angles do not span a volume",
                        (long long)f);
    }
    return MDX_OK;
}

// Triclinic frames: the culled cell-sorted kernel (27 tile images, float32 filter, 27-image contract for the
// undecided pairs) when the range ends below half the smallest cell height in every frame: then at most one image
// of a pair can come within the cut.  Otherwise (or for small systems, or algo = exact / filter, or with
// MDX_RDF_TRI_BRUTE set) the brute-force 27-image kernel.
static bool rdf_tri_culled(int algo, int64_t n1, int64_t n2, double r1, const float *tri, int64_t n_frames)
{
    bool culled = algo == MDX_RDF_ALGO_AUTO || algo == MDX_RDF_ALGO_CELL;
    culled = culled && std::max(n1, n2) >= 1024 && !getenv("MDX_RDF_TRI_BRUTE");
    for (int64_t f = 0; culled && f < n_frames; ++f) {
        const float *B = tri + 9 * f;
        const double b00 = B[0], b10 = B[3], b11 = B[4], b20 = B[6], b21 = B[7], b22 = B[8];
        const double vol = b00 * b11 * b22;
        const double bcx = b11 * b22, bcy = -b10 * b22, bcz = b10 * b21 - b11 * b20;
        const double hx = vol / std::sqrt(bcx * bcx + bcy * bcy + bcz * bcz);
        const double hy = b11 * b22 / std::sqrt(b22 * b22 + b21 * b21);
        const double r_in = 0.5 * std::min(hx, std::min(hy, b22));
        culled = r1 * 1.02 + 1e-3 < r_in;
    }
    return culled;
}

// what mdx_rdf_create fixes for every run of an engine
struct RdfConfig {
    int n_bins;
    double r0, r1;
    int64_t excl1, excl2;
    int algo;
};

// What one run (frames of one cell kind, handed over whole) launches: the slots of mdx_rdf_plan (mdx.h) in their
// order.  The rows of a tile, T = 256 ipt, derive from ipt; n_slabs == 0 stands for "no run yet".
struct RdfRunPlan {
    int family = RDF_FAMILY_TILE_EXACT, ipt = 1;
    bool self = false, excl = false, pbc = false, lower = false, skip = false;
    RdfHist hist;
    bool lds_attribute = false;
    int64_t n1p = 0, n2p = 0, tiles1 = 0, tiles2 = 0;
    int64_t chunk = 0, grid_x = 0;   // j tiles per chunk, chunks
    int64_t slab = 0, n_slabs = 0;
    bool lazy_orig = false;
    int T() const { return 256 * ipt; }
    bool cell() const { return family == RDF_FAMILY_CELL_ORTHO || family == RDF_FAMILY_TRI_CULLED; }
};

// The plan of one run of n_frames frames: `ortho` frames with boxes (has_boxes; min_edge: rdf_next_run) or without,
// or triclinic frames with the cell matrices tri[n_frames][9].  Touches no device; reads MDX_RDF_SLAB_BYTES,
// MDX_RDF_TRI_BRUTE and MDX_RDF_CHUNK_TILES at every call.
static RdfRunPlan rdf_plan_run(const RdfConfig &c, int64_t n1, int64_t n2, bool same, bool has_boxes, bool ortho,
                               float min_edge, const float *tri, int64_t n_frames)
{
    RdfRunPlan p;
    // one set against itself: the same rows AND the same tags, so that a tile pair may stand for its mirror image
    p.excl = c.excl1 > 0;
    p.self = same && (!p.excl || c.excl1 == c.excl2);
    p.pbc = has_boxes;
    if (ortho) {
        const int a = rdf_resolve_ortho_algo(c.algo, has_boxes);
        p.family = a == MDX_RDF_ALGO_CELL ? RDF_FAMILY_CELL_ORTHO
                                          : a == MDX_RDF_ALGO_EXACT_F64 ? RDF_FAMILY_TILE_EXACT : RDF_FAMILY_TILE_FILTER;
    } else {
        p.family = rdf_tri_culled(c.algo, n1, n2, c.r1, tri, n_frames) ? RDF_FAMILY_TRI_CULLED : RDF_FAMILY_TRI_BRUTE;
    }
    if (p.cell()) {
        p.n1p = ceil_div(n1, 128) * 128;
        p.n2p = ceil_div(n2, 128) * 128;
        p.tiles1 = p.n1p / 128;   // 128-row i tiles, 64-row j tiles
        p.tiles2 = p.n2p / 64;
        p.lower = c.r0 > 0.0;
        // (triclinic launches keep the step: their range ends below half the smallest cell height)
        p.skip = !ortho || (float)c.r1 <= CELL_SKIP_MAX_RANGE * min_edge;
        p.hist = rdf_cell_hist(c.n_bins);   // (the cell-sorted launches never ask for the LDS attribute)
        p.grid_x = rdf_cell_chunks(p.n2p, p.skip, &p.chunk);
        p.slab = rdf_cell_slab_frames(p.n1p, p.n2p, p.self, n_frames);
        // exclusion 0 or 1: a particle's tag is its row, and the exact path reads the frames as they came in —
        // no sorted copy of the original coordinates (half of the sort kernel's scattered stores)
        p.lazy_orig = ortho && c.excl1 <= 1 && c.excl2 <= 1;
    } else {
        p.ipt = ortho && std::max(n1, n2) >= 2048 ? 2 : 1;
        const int T = p.T();
        p.n1p = ceil_div(n1, T) * T;
        p.n2p = ceil_div(n2, T) * T;
        p.tiles1 = p.n1p / T;
        p.tiles2 = p.n2p / T;
        p.hist = rdf_tile_hist(c.n_bins, T);
        p.lds_attribute = p.hist.lds > RDF_LDS_ATTR_LINE;
        p.chunk = p.self ? 4 : 8;   // j tiles one block of the brute-force kernels walks
        p.grid_x = ceil_div(p.tiles2, p.chunk);
        // the packed float4 copies of a slab stay within 1 GiB; a slab is ONE pair launch with its frames on grid z,
        // which rests on the cut to RDF_MAX_SLAB here
        const int64_t slab = std::max<int64_t>(1, (int64_t(1) << 30) / (16 * (p.n1p + (p.self ? 0 : p.n2p))));
        p.slab = std::min(std::min(slab, RDF_MAX_SLAB), n_frames);
    }
    p.n_slabs = ceil_div(n_frames, p.slab);
    return p;
}

// the plan as mdx_rdf_plan and mdx_rdf_last_plan report it
static void rdf_plan_slots(const RdfRunPlan &p, int64_t out[MDX_RDF_PLAN_SLOTS])
{
    const int64_t slots[] = {p.family, p.ipt, p.self, p.excl, p.pbc, p.lower, p.skip, p.hist.gh,
                             p.hist.gh ? 0 : p.hist.n_hist, (int64_t)p.hist.lds, p.lds_attribute, p.n1p, p.n2p,
                             p.tiles1, p.tiles2, p.chunk, p.grid_x, p.slab, p.n_slabs, p.lazy_orig};
    constexpr int n = sizeof(slots) / sizeof(slots[0]);
    static_assert(n <= MDX_RDF_PLAN_SLOTS, "more plan fields than slots");
    for (int k = 0; k < MDX_RDF_PLAN_SLOTS; ++k)
        out[k] = k < n ? slots[k] : 0;
}

// The pair kernel a plan stands for: one function per kernel family, over a table of its instantiations
// (tests/rdf_cases.py::instantiation states the same mapping).  `true` comes first in every table, the order in which
// the instantiations are emitted into the unit's device code.
static auto rdf_tile_kernel_of(const RdfRunPlan &p) -> void (*)(RdfArgs)
{
    constexpr int X = MDX_RDF_ALGO_EXACT_F64, F = MDX_RDF_ALGO_FILTER_F32;
    static void (*const kern[2][2][2][2][2])(RdfArgs) = {   // [filter][IPT - 1][!PBC][!EXCL][!GH]
        {{{{rdf_tile_kernel<X, 1, true, true, true>, rdf_tile_kernel<X, 1, true, true, false>},
           {rdf_tile_kernel<X, 1, true, false, true>, rdf_tile_kernel<X, 1, true, false, false>}},
          {{rdf_tile_kernel<X, 1, false, true, true>, rdf_tile_kernel<X, 1, false, true, false>},
           {rdf_tile_kernel<X, 1, false, false, true>, rdf_tile_kernel<X, 1, false, false, false>}}},
         {{{rdf_tile_kernel<X, 2, true, true, true>, rdf_tile_kernel<X, 2, true, true, false>},
           {rdf_tile_kernel<X, 2, true, false, true>, rdf_tile_kernel<X, 2, true, false, false>}},
          {{rdf_tile_kernel<X, 2, false, true, true>, rdf_tile_kernel<X, 2, false, true, false>},
           {rdf_tile_kernel<X, 2, false, false, true>, rdf_tile_kernel<X, 2, false, false, false>}}}},
        {{{{rdf_tile_kernel<F, 1, true, true, true>, rdf_tile_kernel<F, 1, true, true, false>},
           {rdf_tile_kernel<F, 1, true, false, true>, rdf_tile_kernel<F, 1, true, false, false>}},
          {{rdf_tile_kernel<F, 1, false, true, true>, rdf_tile_kernel<F, 1, false, true, false>},
           {rdf_tile_kernel<F, 1, false, false, true>, rdf_tile_kernel<F, 1, false, false, false>}}},
         {{{rdf_tile_kernel<F, 2, true, true, true>, rdf_tile_kernel<F, 2, true, true, false>},
           {rdf_tile_kernel<F, 2, true, false, true>, rdf_tile_kernel<F, 2, true, false, false>}},
          {{rdf_tile_kernel<F, 2, false, true, true>, rdf_tile_kernel<F, 2, false, true, false>},
           {rdf_tile_kernel<F, 2, false, false, true>, rdf_tile_kernel<F, 2, false, false, false>}}}}};
    return kern[p.family == RDF_FAMILY_TILE_FILTER][p.ipt - 1][!p.pbc][!p.excl][!p.hist.gh];
}

static auto rdf_cell_kernel_of(const RdfRunPlan &p) -> void (*)(CellArgs)
{
    // [!EXCL][!LOWER][form]: triclinic frames with the global and with the LDS histogram; orthorhombic frames with the
    // LDS histogram and the step that leaves when it is empty or the unconditional tail, and with the global histogram
    static void (*const kern[2][2][5])(CellArgs) = {
        {{rdf_cell_pair_kernel<true, true, 1, true>, rdf_cell_pair_kernel<true, true, 0, true>,
          rdf_cell_pair_kernel<true, true, 0, false, true>, rdf_cell_pair_kernel<true, true, 0, false, false>,
          rdf_cell_pair_kernel<true, true, 1>},
         {rdf_cell_pair_kernel<true, false, 1, true>, rdf_cell_pair_kernel<true, false, 0, true>,
          rdf_cell_pair_kernel<true, false, 0, false, true>, rdf_cell_pair_kernel<true, false, 0, false, false>,
          rdf_cell_pair_kernel<true, false, 1>}},
        {{rdf_cell_pair_kernel<false, true, 1, true>, rdf_cell_pair_kernel<false, true, 0, true>,
          rdf_cell_pair_kernel<false, true, 0, false, true>, rdf_cell_pair_kernel<false, true, 0, false, false>,
          rdf_cell_pair_kernel<false, true, 1>},
         {rdf_cell_pair_kernel<false, false, 1, true>, rdf_cell_pair_kernel<false, false, 0, true>,
          rdf_cell_pair_kernel<false, false, 0, false, true>, rdf_cell_pair_kernel<false, false, 0, false, false>,
          rdf_cell_pair_kernel<false, false, 1>}}};
    const bool gh = p.hist.gh;
    return kern[!p.excl][!p.lower][p.family == RDF_FAMILY_TRI_CULLED ? (gh ? 0 : 1) : gh ? 4 : p.skip ? 2 : 3];
}

// The contract binds the edges to numpy.linspace (mdx.h): the float32 filter and the cell kernel's sure path take
// a pair's bin from floor((d - r0) * n_bins / (r1 - r0)) and only pairs near an edge of THAT grid go to the threshold
// table, so any other increasing array would be binned wrongly there and rightly on the exact routes.  linspace
// (one division, one multiplication, one addition) stays within 2 ulp of the real grid; 4 ulp(edges[n_bins]) are
// allowed.  Precedes every device call, for every algorithm.
static int rdf_check_edges(int n_bins, const double *edges)
{
    for (int b = 0; b < n_bins; ++b)
        MDX_REQUIRE(edges[b] < edges[b + 1], "edges must increase strictly (edges[%d] = %.17g, edges[%d] = %.17g)",
                    b, edges[b], b + 1, edges[b + 1]);
    MDX_REQUIRE(edges[0] >= 0.0 && std::isfinite(edges[n_bins]), "range must be finite and >= 0");
    const double top = std::fabs(edges[n_bins]);
    const long double tol = 4.0L * ((long double)std::nextafter(top, INFINITY) - (long double)top);
    const long double r0 = edges[0], span = (long double)edges[n_bins] - (long double)edges[0];
    for (int k = 0; k <= n_bins; ++k) {
        const long double want = r0 + (long double)k * span / (long double)n_bins;
        const long double off = (long double)edges[k] - want;
        if (!((off < 0 ? -off : off) <= tol))
            return fail(MDX_ERR_INVALID_VALUE,
                        "edges must be numpy.linspace(edges[0], edges[n_bins], n_bins + 1): edges[%d] = %.17g lies "
                        "%.3g from the uniform grid's %.17g", k, edges[k], (double)off, (double)want);
    }
    return MDX_OK;
}

// what mdx_rdf_create and mdx_rdf_plan ask of an engine's arguments, before any device call
static int rdf_check_engine_args(const void *out, int n_bins, const double *edges, int64_t excl1, int64_t excl2,
                                 int algo)
{
    MDX_REQUIRE(out && edges, "NULL argument");
    MDX_REQUIRE(n_bins >= 1 && n_bins <= (1 << 20), "n_bins=%d out of range", n_bins);
    MDX_REQUIRE((excl1 > 0) == (excl2 > 0) && excl1 >= 0 && excl2 >= 0,
                "exclusion must be two positive integers (or 0, 0 for none)");
    MDX_REQUIRE(algo >= MDX_RDF_ALGO_AUTO && algo <= MDX_RDF_ALGO_CELL, "unknown algo %d", algo);
    return rdf_check_edges(n_bins, edges);
}

// the sets of a run, as the engine and mdx_rdf_plan bound them (the kernels index padded rows with 32-bit ints)
static int rdf_check_set_sizes(int64_t n1, int64_t n2)
{
    MDX_REQUIRE(n1 < (int64_t(1) << 30) && n2 < (int64_t(1) << 30), "too many particles");
    return MDX_OK;
}

// --------------------------------------------------------------------- handle

struct mdx_rdf {
    int dev = 0;
    hipStream_t stream = nullptr;
    int n_bins = 0;
    std::vector<double> edges;
    std::vector<double> thresh;
    double t_lo = 0, t_hi = 0;
    int64_t excl1 = 0, excl2 = 0;
    int algo = MDX_RDF_ALGO_AUTO;
    int n_rep = 32;
    DeviceBuffer d_thresh, d_counts, d_total, d_pack1, d_pack2, d_misc, d_tri;
    DeviceBuffer d_stats;   // RDF_STAT_SHARDS x RDF_STAT_STRIDE 64-bit words (mdx_rdf_device.hpp)
    DeviceBuffer d_work;    // work counters of the persistent pair kernel (one line per XCD)
    DeviceBuffer d_frame_geo;   // frame constants of one pair launch (rdf_cell_frame_geo_kernel)
    const void *occ_kernel = nullptr;   // occupancy of the persistent pair kernel: last kernel / LDS size asked for
    size_t occ_lds = 0;
    int64_t occ_blocks_per_xcd = 1;
    RdfRunPlan last_plan;   // of the most recent run since reset (mdx_rdf_last_plan)
    // what mdx_rdf_debug_sorted needs beside it to find the most recent slab of the cell-sorted route: its set of
    // sorted copies and its frame count
    size_t last_offset = 0;   // float4 elements from the start of d_pw1 / d_po1 to the slab
    int64_t last_frames = 0;
    // optional centre-of-mass stage per set: incoming rows are particles grouped into molecules
    MoleculeStage grouping[2];
    // drop_axis (2-D mode, structure.py:761-770): coordinate zeroed, box length -> max(lx, ly, lz)
    int drop_axis = -1;
    DeviceBuffer d_drop[2], d_drop_box;
    // host-buffer entry point: double-buffered staging, copy stream, hand-over events
    DeviceBuffer d_stage1[2], d_stage2[2], d_boxes[2], d_index[2];
    DeviceBuffer d_rawslab[2];   // trajectory files: a slab of raw frames between the copy and the unpack kernel
    StagePipeline pipe;
    DeviceBuffer d_pw1, d_po1, d_bb1, d_pw2, d_po2, d_bb2;   // cell path: sorted copies + tile boxes
    DeviceBuffer d_bb16_1, d_bb16_2;                         // boxes of the CELL_CHUNK-particle chunks
    // cell path: the sort of slab k + 1 runs on its own stream beside the pair kernel of slab k (two sets of the
    // sorted copies at offsets 0 and one slab into the buffers above); events hand the sets back and forth
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr;                  // h->stream at the entry of a call -> side
    hipEvent_t ev_sorted[2] = {nullptr, nullptr};  // side: the set holds its slab -> h->stream
    hipEvent_t ev_read[2] = {nullptr, nullptr};    // h->stream: the pair kernel has read the set -> side
    hipEvent_t ev_join = nullptr;                  // side at the exit of a call -> h->stream
    int64_t slabs_sorted_beside = 0;               // slabs whose sort ran beside a pair kernel since reset
    size_t occ_static_lds = 0;                     // static LDS of the pair kernel asked for last
    int occ_per_cu = 1;
    StreamTimer timer;
    int64_t pairs_evaluated = 0;    // ordered pair space covered: frames * n1 * n2
    int64_t pairs_bruteforce = 0;   // distance evaluations executed by the brute-force tiles
    bool reduced_global = false;   // counts replica 0 holds an all-reduced total
};

// ------------------- routes: each takes a run through the kernels of its plan and recomputes nothing the plan holds

// The frames of one run on the device: pos float[n_frames][n][3] (pos2 == pos1 for one set against itself), and
// boxes float[n_frames][6] for orthorhombic frames (nullptr: no cell) or tri float[n_frames][9] for triclinic ones.
struct RdfFrames {
    const float *pos1, *pos2;
    int64_t n1, n2;
    const float *boxes, *tri;
};

// The brute-force routes walk a run in slabs so that the packed float4 copies stay bounded.  Per slab, the fields
// RdfArgs and TriArgs have in common are set here from the plan; pack(a, f0, nf) packs frames [f0, f0 + nf) into
// d_pack1 / d_pack2 and sets what is its kernel's own; then the pair kernel, frames on grid z.
template <typename Args, typename Pack>
static int tile_slabs(mdx_rdf *h, const RdfRunPlan &p, const RdfFrames &in, int64_t n_frames, void (*kern)(Args),
                      Pack pack)
{
    if (p.lds_attribute)
        MDX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.hist.lds));
    MDX_TRY(h->d_pack1.ensure(size_t(16) * p.n1p * p.slab));
    if (!p.self)
        MDX_TRY(h->d_pack2.ensure(size_t(16) * p.n2p * p.slab));
    const int64_t tile_pairs = p.self ? p.tiles1 * (p.tiles1 + 1) / 2 : p.tiles1 * p.tiles2;
    for (int64_t f0 = 0; f0 < n_frames; f0 += p.slab) {
        const int64_t nf = std::min(p.slab, n_frames - f0);
        Args a{};
        a.p1 = h->d_pack1.as<float4>();
        a.p2 = p.self ? a.p1 : h->d_pack2.as<float4>();
        a.n1p = (int)p.n1p;
        a.n2p = (int)p.n2p;
        a.nt1 = (int)p.tiles1;
        a.nt2 = (int)p.tiles2;
        a.self = p.self ? 1 : 0;
        a.n_bins = h->n_bins;
        a.thresh = h->d_thresh.as<double>();
        a.t_lo = h->t_lo;
        a.t_hi = h->t_hi;
        a.counts = h->d_counts.as<unsigned long long>();
        a.n_rep = h->n_rep;
        a.n_hist = p.hist.n_hist;
        a.chunk = (int)p.chunk;
        pack(a, f0, nf);
        hipEvent_t ev = h->timer.begin();
        hipLaunchKernelGGL(kern, dim3((unsigned)p.grid_x, (unsigned)p.tiles1, (unsigned)nf), dim3(256), p.hist.lds,
                           h->stream, a);
        h->timer.end(ev);
        MDX_HIP(hipGetLastError());
        h->pairs_bruteforce += nf * tile_pairs * p.T() * p.T();
    }
    h->pairs_evaluated += n_frames * in.n1 * in.n2;
    return MDX_OK;
}

// Orthorhombic frames (or none), brute-force tiles: exact arithmetic or the float32 filter.
static int accumulate_tiles(mdx_rdf *h, const RdfRunPlan &p, const RdfFrames &in, int64_t n_frames)
{
    unsigned *d_misc = h->d_misc.as<unsigned>();   // [0] maxabs bits, [1] status
    return tile_slabs(h, p, in, n_frames, rdf_tile_kernel_of(p), [&](RdfArgs &a, int64_t f0, int64_t nf) {
        hipLaunchKernelGGL(rdf_pack_kernel, dim3((unsigned)(p.n1p / 256), (unsigned)nf), dim3(256), 0,
                           h->stream, in.pos1 + f0 * in.n1 * 3, h->d_pack1.as<float4>(), (int)in.n1,
                           (int)p.n1p, p.excl ? h->excl1 : 0, d_misc);
        if (!p.self)
            hipLaunchKernelGGL(rdf_pack_kernel, dim3((unsigned)(p.n2p / 256), (unsigned)nf), dim3(256),
                               0, h->stream, in.pos2 + f0 * in.n2 * 3, h->d_pack2.as<float4>(), (int)in.n2,
                               (int)p.n2p, p.excl ? h->excl2 : 0, d_misc);
        a.boxes = in.boxes ? in.boxes + f0 * 6 : nullptr;
        a.r0 = h->edges.front();
        a.r1 = h->edges.back();
        a.maxabs_bits = d_misc;
        a.exact_counter = h->d_stats.as<unsigned long long>();
    });
}

// The cell-sorted route (mdx_rdf_cell.hpp), for orthorhombic frames and for culled triclinic ones: sort + tile boxes
// per frame, then the culled pair kernel.  The plan fixes the kernel, its LDS, the padding, the items and the slab.
// What the functions below decide on top of it depends on the device or on switches that only they read — the pair
// kernel's occupancy, the memory that is free, MDX_RDF_SORT_BESIDE, MDX_RDF_LDS_FLUSH_UNITS — and is no part of the
// plan: whether the next slab is sorted beside a pair launch, the quarter and half slabs that route starts with, the
// grid of the persistent pair blocks.
struct CellSide {   // the sorted copies of one particle set: wrapped and original rows, boxes of the 64-row tiles and
    DeviceBuffer *pw, *po, *bb, *bc;   // of the chunks — and the float4 elements a slab of p.slab frames takes in each
    size_t e_p, e_b, e_c;
};

struct CellSet {   // one set of sorted copies, [particle set 1 | 2] (the same pointers for one set against itself)
    float4 *pw[2], *po[2], *bb[2], *bc[2];
};

struct CellRun {
    mdx_rdf *h;
    const RdfRunPlan &p;
    const RdfFrames &in;
    void (*kern)(CellArgs);
    CellSide side[2];
    bool beside;                 // the sort of slab k + 1 runs beside the pair kernel of slab k
    std::vector<int64_t> lens;   // slab lengths of this run

    bool tri() const { return p.family == RDF_FAMILY_TRI_CULLED; }
};

// resident blocks per XCD (32 CUs each) of the pair kernel at its LDS size (asked once per kernel and size)
static int cell_occupancy(mdx_rdf *h, const void *kern, size_t lds)
{
    if (h->occ_kernel == kern && h->occ_lds == lds)
        return MDX_OK;
    int per_cu = 0, cus = 0;
    hipFuncAttributes fa{};
    MDX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds));
    MDX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->dev));
    MDX_HIP(hipFuncGetAttributes(&fa, kern));
    h->occ_kernel = kern;
    h->occ_lds = lds;
    h->occ_static_lds = fa.sharedSizeBytes;
    h->occ_per_cu = std::max(per_cu, 1);
    h->occ_blocks_per_xcd = std::max<int64_t>(1, int64_t(std::max(per_cu, 1)) * std::max(cus, 8) / 8);
    return MDX_OK;
}

static int cell_sets_ensure(const CellRun &r, size_t n_sets)
{
    for (int g = 0; g < (r.p.self ? 1 : 2); ++g) {
        const CellSide &d = r.side[g];
        MDX_TRY(d.pw->ensure(16 * d.e_p * n_sets));
        if (!r.p.lazy_orig)
            MDX_TRY(d.po->ensure(16 * d.e_p * n_sets));
        MDX_TRY(d.bb->ensure(16 * d.e_b * n_sets));
        MDX_TRY(d.bc->ensure(16 * d.e_c * n_sets));
    }
    return MDX_OK;
}

static CellSet cell_set_of(const CellRun &r, int b)
{
    CellSet s;
    for (int g = 0; g < 2; ++g) {
        const CellSide &d = r.side[r.p.self ? 0 : g];
        s.pw[g] = d.pw->as<float4>() + b * d.e_p;
        s.po[g] = r.p.lazy_orig ? nullptr : d.po->as<float4>() + b * d.e_p;
        s.bb[g] = d.bb->as<float4>() + b * d.e_b;
        s.bc[g] = d.bc->as<float4>() + b * d.e_c;
    }
    return s;
}

// The sort of slab k + 1 BESIDE the pair kernel of slab k.  Round 2 put it on a second stream (+1 %); with
// persistent pair blocks that lost 3 % (NOTES.md round 3): they hold every wave slot and nearly every register
// until their last items, and a 1 024-thread sort block could enter only where four of them had retired.  Here
// the sort is a block of the pair block's own shape (rdf_cell_sort_small_kernel), and the pair kernel is launched
// with S fewer blocks than the chip holds (S a multiple of 8: every XCD gives up the same number): S persistent
// sort blocks on the side stream have a place from the start, and neither kernel waits for the other to retire
// anything.  Two sets of the sorted copies alternate.  The first slab of a call has nothing to hide behind: the
// big kernel sorts it on the handle's stream, and it is a quarter slab, the second a half (the shape of the host
// and file routes), S scaled by the ratio of the sorted slab's length to the pair launch's.
// Today's serial route (one set, the big kernel) remains for: triclinic frames, more than 65 535 particles in a
// set (packed 16-bit counters), a pair kernel whose blocks leave the sort block's 33 KB of LDS no room beside
// all but one of them, calls of a single slab, a device without room for the second set, and
// MDX_RDF_SORT_BESIDE=0.
// S = 16 (profiles/r06_sort_beside_S_choice.txt): 16 blocks sort a slab of 2 304 C2 frames in half the time of
// its pair launch; with 8 the sort would take all of it
constexpr int64_t CELL_SORT_BESIDE_BLOCKS = 16;

// decides r.beside (after cell_occupancy), creates the side stream and its events at the first need, and sizes the
// buffers for two sets or one
static int cell_sort_beside(CellRun &r, int64_t n_frames)
{
    mdx_rdf *h = r.h;
    const char *sb_env = getenv("MDX_RDF_SORT_BESIDE");
    const size_t cu_lds = size_t(160) * 1024;
    r.beside = !r.tri() && !(sb_env && strcmp(sb_env, "0") == 0) && n_frames > r.p.slab &&
               r.in.n1 <= SORT_SMALL_MAX_N && r.in.n2 <= SORT_SMALL_MAX_N && h->occ_blocks_per_xcd >= 2 &&
               size_t(h->occ_per_cu - 1) * (h->occ_static_lds + r.p.hist.lds) + sort_small_lds_bytes() <= cu_lds;
    if (r.beside && !h->ev_join) {
        // (the last event created is the guard: after a failure half-way the next call starts over)
        if (!h->side)
            MDX_TRY(stream_acquire(&h->side));
        for (hipEvent_t *e : {&h->ev_fork, &h->ev_sorted[0], &h->ev_sorted[1], &h->ev_read[0], &h->ev_read[1], &h->ev_join})
            if (!*e)
                MDX_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    // two sets are twice the memory (5 GiB at C2): a device too full for them still has the serial route's one
    // (buffers the failed attempt had already grown stay at that size, and its message stays in mdx_last_error()
    // although the call then succeeds: nobody reads it after MDX_OK)
    if (r.beside && cell_sets_ensure(r, 2) == MDX_ERR_OUT_OF_MEMORY)
        r.beside = false;
    return cell_sets_ensure(r, r.beside ? 2 : 1);
}

// slab lengths of a run: with the sort beside, a quarter and a half slab first (whole rounds of the big kernel)
static std::vector<int64_t> cell_slab_lengths(int64_t slab, bool beside, int64_t n_frames)
{
    std::vector<int64_t> lens;
    for (int64_t f0 = 0; f0 < n_frames;) {
        int64_t step = slab;
        if (beside && slab >= 8 && lens.size() < 2) {
            step = slab >> (2 - lens.size());
            if (step >= 256)
                step -= step % 256;
        }
        step = std::min(step, n_frames - f0);
        lens.push_back(step);
        f0 += step;
    }
    return lens;
}

// the sort of frames [f0, f0 + nf) into a set: the big kernel (small_grid == 0) or `small_grid` persistent
// blocks of the small one
static void cell_launch_sort(const CellRun &r, const CellSet &s, int64_t f0, int64_t nf, hipStream_t stream,
                             unsigned small_grid)
{
    // (Measured and dropped, round 3: the sort as a GATHER — slots noted per particle in LDS, rows written
    // in slot order as whole lines — 0.66 ms per 1 000 frames against 0.74–0.82, +0.5 % on the step, but its
    // 12-byte reads scattered over frames that are no longer in L2 fetch 4.0 MB per frame where the scatter's
    // partial-sector stores cost 1.1: 6.5 MB per frame in all against 4.4.  Neither two blocks per CU (the
    // kernel sits at 65 VGPRs: one over), float32 cell keys, a DPP box reduction nor a two-barrier scan moved
    // the kernel's time: all 256 blocks of a round read, then write, in step — 25 µs counting from HBM, 81 µs
    // writing rows — and the memory system sets the pace.)
    mdx_rdf *h = r.h;
    const float *pos[2] = {r.in.pos1 + f0 * r.in.n1 * 3, r.in.pos2 + f0 * r.in.n2 * 3};
    const float *cells = r.tri() ? r.in.tri + f0 * 9 : r.in.boxes + f0 * 6;
    const int n[2] = {(int)r.in.n1, (int)r.in.n2}, n_pad[2] = {(int)r.p.n1p, (int)r.p.n2p};
    const int64_t excl[2] = {r.p.excl ? h->excl1 : 0, r.p.excl ? h->excl2 : 0};
    unsigned *d_maxabs = h->d_misc.as<unsigned>();
    for (int g = 0; g < (r.p.self ? 1 : 2); ++g) {
        if (small_grid)
            hipLaunchKernelGGL(rdf_cell_sort_small_kernel<SORT_SMALL_THREADS>, dim3(small_grid),
                               dim3(SORT_SMALL_THREADS), sort_small_lds_bytes(), stream, pos[g], cells, n[g], n_pad[g],
                               excl[g], s.pw[g], s.po[g], s.bb[g], s.bc[g], d_maxabs, (int)nf);
        else
            hipLaunchKernelGGL(r.tri() ? rdf_cell_sort_kernel<true> : rdf_cell_sort_kernel<false>, dim3((unsigned)nf),
                               dim3(SORT_THREADS), 0, stream, pos[g], cells, n[g], n_pad[g], excl[g], s.pw[g], s.po[g],
                               s.bb[g], s.bc[g], d_maxabs);
    }
}

// the pair kernel over the sorted frames [f0, f0 + nf) of a set; holes: blocks it leaves to a sort beside it
static int cell_launch_pairs(const CellRun &r, const CellSet &s, int64_t f0, int64_t nf, int64_t holes)
{
    mdx_rdf *h = r.h;
    const RdfRunPlan &p = r.p;
    const RdfFrames &in = r.in;
    CellArgs a{};
    a.pw1 = s.pw[0];
    a.po1 = s.po[0];
    a.bb1 = s.bb[0];
    a.pw2 = s.pw[1];
    a.po2 = s.po[1];
    a.bb2 = s.bb[1];
    a.bb16_2 = s.bc[1];
    a.in1 = p.lazy_orig ? in.pos1 + f0 * in.n1 * 3 : nullptr;
    a.in2 = p.lazy_orig ? in.pos2 + f0 * in.n2 * 3 : nullptr;
    a.n1_in = (int)in.n1;
    a.n2_in = (int)in.n2;
    a.tags_everywhere = (p.self && h->excl1 == 1 && h->excl2 == 1) ? 0 : 1;
    a.boxes = r.tri() ? nullptr : in.boxes + f0 * 6;
    a.tri = r.tri() ? in.tri + f0 * 9 : nullptr;
    a.thresh = h->d_thresh.as<double>();
    a.counts = h->d_counts.as<unsigned long long>();
    // the batch's largest |coordinate| (the filter's error bound grows with it) is folded by the sort into ONE word
    // per handle.  A pair kernel beside which the next slab is sorted may read the maximum of that slab as well:
    // that only widens the filter's margin — more pairs take the exact path, which bins them as the contract does,
    // so the counts cannot change (the exact-path statistics can, by a few pairs).
    a.maxabs_bits = h->d_misc.as<unsigned>();
    a.exact_counter = h->d_stats.as<unsigned long long>();
    a.tilepair_counter = a.exact_counter + 1;
    a.clock_counter = h->timer.enabled ? a.exact_counter + 3 : nullptr;
    a.t_lo = h->t_lo;
    a.t_hi = h->t_hi;
    a.r0 = h->edges.front();
    a.r1 = h->edges.back();
    a.n1p = (int)p.n1p;
    a.n2p = (int)p.n2p;
    a.n_bins = h->n_bins;
    a.n_hist = p.hist.n_hist;
    a.n_rep = h->n_rep;
    a.self = p.self ? 1 : 0;
    a.work = h->d_work.as<unsigned>();
    {
        const char *fu = getenv("MDX_RDF_LDS_FLUSH_UNITS");   // test hook: flush the LDS bins (much) more often
        // (the cap: 1024 + 2 x flush_units <= 2^18, see the pair kernel)
        const long long cap = (1 << 17) - 512;
        a.flush_units = fu ? (unsigned)std::min<long long>(std::max<long long>(atoll(fu), 1), cap) : (unsigned)cap;
    }
    // items: an i tile against a chunk of its candidate j tiles
    a.chunks = (int)p.grid_x;
    const int64_t tiles = p.tiles1 * p.grid_x;   // items of a frame
    // (frames per launch: the item index is 32 bits wide)
    const int64_t launch_frames = std::max<int64_t>(8, std::min<int64_t>(32768, ((int64_t(1) << 30) / tiles) * 8));
    // (sized for the longest slab: it does not grow, and so is not freed, between the launches of a call)
    MDX_TRY(h->d_frame_geo.ensure(sizeof(float) * CELL_GEO_FLOATS * size_t(std::min<int64_t>(launch_frames, p.slab))));
    a.frame_geo = h->d_frame_geo.as<float>();
    hipEvent_t ev = h->timer.begin();
    for (int64_t g0 = 0; g0 < nf; g0 += launch_frames) {
        a.frame0 = (int)g0;
        a.n_frames = (int)std::min<int64_t>(launch_frames, nf - g0);
        a.spread = a.n_frames < 8 ? 1 : 0;
        // persistent blocks: what the chip holds at once (blocks per CU from the kernel's own occupancy), a
        // multiple of 8 so that every XCD gets the same number — less the holes of a sort that runs beside
        // this launch; fewer when there is less work than that
        const int64_t items_per_xcd = a.spread ? ceil_div(int64_t(a.n_frames) * tiles, 8)
                                               : ceil_div(a.n_frames, 8) * tiles;
        const unsigned grid = 8u * (unsigned)std::min<int64_t>(h->occ_blocks_per_xcd - holes / 8, items_per_xcd);
        MDX_HIP(hipMemsetAsync(h->d_work.ptr, 0, CELL_WORK_BYTES, h->stream));
        // the frames' constants, once per frame: behind this slab's sort (and the previous launch, which
        // read the table), in front of the items that load them
        hipLaunchKernelGGL(r.tri() ? rdf_cell_frame_geo_kernel<true> : rdf_cell_frame_geo_kernel<false>,
                           dim3((unsigned)ceil_div(a.n_frames, 256)), dim3(256), 0, h->stream, a);
        hipLaunchKernelGGL(r.kern, dim3(grid), dim3(256), p.hist.lds, h->stream, a);
    }
    h->timer.end(ev);
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

// slab after slab: its sort (unless it ran beside the slab before), the sort of the next slab on the side stream,
// its pair kernel
static int cell_slabs(const CellRun &r)
{
    mdx_rdf *h = r.h;
    int64_t f0 = 0;
    for (size_t k = 0; k < r.lens.size(); f0 += r.lens[k], ++k) {
        const int64_t nf = r.lens[k];
        const int b = r.beside ? int(k & 1) : 0;
        const CellSet s = cell_set_of(r, b);
        h->last_offset = b * r.side[0].e_p;
        h->last_frames = nf;
        if (!r.beside || k == 0)
            cell_launch_sort(r, s, f0, nf, h->stream, 0);
        else
            MDX_HIP(hipStreamWaitEvent(h->stream, h->ev_sorted[b], 0));
        // blocks the pair kernel of this slab leaves to the sort of the next
        int64_t holes = 0;
        if (r.beside && k + 1 < r.lens.size()) {
            const int64_t nf_next = r.lens[k + 1];
            holes = ceil_div(ceil_div(CELL_SORT_BESIDE_BLOCKS * nf_next, nf), 8) * 8;
            holes = std::min<int64_t>(holes, 8 * (h->occ_blocks_per_xcd / 2));
            // the other set: free once the pair kernel of slab k - 1 has read it (before the first slab of a
            // call: whatever the handle's stream held at the fork)
            if (k > 0)
                MDX_HIP(hipStreamWaitEvent(h->side, h->ev_read[b ^ 1], 0));
            cell_launch_sort(r, cell_set_of(r, b ^ 1), f0 + nf, nf_next, h->side,
                             (unsigned)std::min<int64_t>(holes, nf_next));
            MDX_HIP(hipEventRecord(h->ev_sorted[b ^ 1], h->side));
            h->slabs_sorted_beside += 1;
        }
        MDX_TRY(cell_launch_pairs(r, s, f0, nf, holes));
        if (r.beside)
            MDX_HIP(hipEventRecord(h->ev_read[b], h->stream));
    }
    return MDX_OK;
}

// cell_slabs between a fork and a join of the side stream.  Fork: what the caller queued on the handle's stream (the
// unpack kernel of the file route, an earlier call's pair kernels that still read a set) is ahead of everything on
// the side stream; join: the handle's stream ends behind the side stream's last kernel — on the error exits too — so
// that synchronize(), counts(), reset() and close() mean what they meant
static int cell_slabs_forked(const CellRun &r)
{
    mdx_rdf *h = r.h;
    MDX_HIP(hipEventRecord(h->ev_fork, h->stream));
    MDX_HIP(hipStreamWaitEvent(h->side, h->ev_fork, 0));
    int rc = cell_slabs(r);
    hipError_t e = hipEventRecord(h->ev_join, h->side);
    if (e == hipSuccess)
        e = hipStreamWaitEvent(h->stream, h->ev_join, 0);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->side);
        if (rc == MDX_OK)
            rc = fail(MDX_ERR_HIP, "joining the sort stream failed: %s", hipGetErrorString(e));
    }
    return rc;
}

// one run through the cell-sorted route
static int accumulate_cell(mdx_rdf *h, const RdfRunPlan &p, const RdfFrames &in, int64_t n_frames)
{
    // (two-particle chunks take their boxes from the staged rows: a token chunk-box array)
    auto side = [&](DeviceBuffer &pw, DeviceBuffer &po, DeviceBuffer &bb, DeviceBuffer &bc, int64_t n_pad) {
        const size_t slab = size_t(p.slab);
        return CellSide{&pw, &po, &bb, &bc, size_t(n_pad) * slab, size_t(n_pad / 64) * 2 * slab,
                        CELL_CHUNK >= 4 ? size_t(n_pad / CELL_CHUNK) * 2 * slab : 16};
    };
    CellRun r{h, p, in, rdf_cell_kernel_of(p),
              {side(h->d_pw1, h->d_po1, h->d_bb1, h->d_bb16_1, p.n1p), side(h->d_pw2, h->d_po2, h->d_bb2, h->d_bb16_2, p.n2p)},
              false, {}};
    MDX_TRY(cell_occupancy(h, reinterpret_cast<const void *>(r.kern), p.hist.lds));
    MDX_TRY(cell_sort_beside(r, n_frames));
    r.lens = cell_slab_lengths(p.slab, r.beside, n_frames);
    MDX_TRY(r.beside ? cell_slabs_forked(r) : cell_slabs(r));
    h->pairs_evaluated += n_frames * in.n1 * in.n2;
    return MDX_OK;
}

static auto rdf_tri_tile_kernel_of(const RdfRunPlan &p) -> void (*)(TriArgs)
{
    static void (*const kern[2][2])(TriArgs) = {   // [!EXCL][!GH]
        {rdf_tri_tile_kernel<true, true>, rdf_tri_tile_kernel<true, false>},
        {rdf_tri_tile_kernel<false, true>, rdf_tri_tile_kernel<false, false>}};
    return kern[!p.excl][!p.hist.gh];
}

// Triclinic frames, brute-force tiles: the 27-image search in double on every pair.
static int accumulate_tri_tiles(mdx_rdf *h, const RdfRunPlan &p, const RdfFrames &in, int64_t n_frames)
{
    const double width = (h->edges.back() - h->edges.front()) / h->n_bins;
    return tile_slabs(h, p, in, n_frames, rdf_tri_tile_kernel_of(p), [&](TriArgs &a, int64_t f0, int64_t nf) {
        a.tri = in.tri + f0 * 9;
        hipLaunchKernelGGL(rdf_tri_pack_kernel, dim3((unsigned)(p.n1p / 256), (unsigned)nf), dim3(256),
                           0, h->stream, in.pos1 + f0 * in.n1 * 3, a.tri, h->d_pack1.as<float4>(),
                           (int)in.n1, (int)p.n1p, p.excl ? h->excl1 : 0);
        if (!p.self)
            hipLaunchKernelGGL(rdf_tri_pack_kernel, dim3((unsigned)(p.n2p / 256), (unsigned)nf),
                               dim3(256), 0, h->stream, in.pos2 + f0 * in.n2 * 3, a.tri,
                               h->d_pack2.as<float4>(), (int)in.n2, (int)p.n2p, p.excl ? h->excl2 : 0);
        a.r0f = (float)h->edges.front();
        a.inv_wf = (float)(1.0 / width);
    });
}

// Every accumulate entry point ends here, with points on the device.  Frames are dispatched in runs of one cell kind
// (rdf_next_run): each run is planned once (rdf_plan_run) and goes to the route of its plan's family.  h_boxes: the
// same boxes on the host, or nullptr (then they are copied back from d_boxes — 24 bytes per frame and one stream
// synchronisation).
static int accumulate_device_points(mdx_rdf *h, const float *d_pos1, int64_t n1, const float *d_pos2, int64_t n2,
                                    const float *d_boxes, const float *h_boxes, int64_t n_frames)
{
    if (n_frames == 0 || n1 == 0 || n2 == 0)
        return MDX_OK;
    if (h->reduced_global)
        return fail(MDX_ERR_STATE, "handle holds all-reduced counts; call mdx_rdf_reset() first");
    const bool same = (d_pos2 == nullptr || (d_pos2 == d_pos1 && n2 == n1));
    if (d_pos2 == nullptr) {
        d_pos2 = d_pos1;
        n2 = n1;
    }
    MDX_TRY(rdf_check_set_sizes(n1, n2));
    const RdfConfig cfg{h->n_bins, h->edges.front(), h->edges.back(), h->excl1, h->excl2, h->algo};
    std::vector<float> copy, tri;
    if (d_boxes && !h_boxes) {
        copy.resize(size_t(6) * n_frames);
        MDX_HIP(hipMemcpyAsync(copy.data(), d_boxes, size_t(24) * n_frames, hipMemcpyDeviceToHost,
                               h->stream));
        MDX_HIP(hipStreamSynchronize(h->stream));
        h_boxes = copy.data();
    }
    for (int64_t f0 = 0, f1; f0 < n_frames; f0 = f1) {
        bool ortho = true;
        float min_edge = 0.f;
        f1 = d_boxes ? rdf_next_run(h_boxes, f0, n_frames, &ortho, &min_edge) : n_frames;
        const int64_t nf = f1 - f0;
        RdfFrames in{d_pos1 + f0 * n1 * 3, d_pos2 + f0 * n2 * 3, n1, n2, nullptr, nullptr};
        if (!ortho)
            MDX_TRY(rdf_tri_cells(h_boxes + 6 * f0, nf, tri));
        const RdfRunPlan p = rdf_plan_run(cfg, n1, n2, same, d_boxes != nullptr, ortho, min_edge,
                                          ortho ? nullptr : tri.data(), nf);
        h->last_plan = p;
        if (ortho && d_boxes) {
            // once per orthorhombic run, ahead of its packs and sorts; mdx_rdf_synchronize reads the verdict
            in.boxes = d_boxes + f0 * 6;
            hipLaunchKernelGGL(rdf_check_boxes_kernel, dim3((unsigned)ceil_div(nf, 256)), dim3(256), 0, h->stream,
                               in.boxes, nf, h->d_misc.as<unsigned>() + 1);
        } else if (!ortho) {
            // the previous call's kernels may still read the cell matrices
            MDX_HIP(hipStreamSynchronize(h->stream));
            MDX_TRY(h->d_tri.ensure(size_t(36) * nf));
            MDX_HIP(hipMemcpyAsync(h->d_tri.ptr, tri.data(), size_t(36) * nf, hipMemcpyHostToDevice, h->stream));
            MDX_HIP(hipStreamSynchronize(h->stream));   // `tri` is filled again for the next run
            in.tri = h->d_tri.as<float>();
        }
        switch (p.family) {
        case RDF_FAMILY_TRI_BRUTE: MDX_TRY(accumulate_tri_tiles(h, p, in, nf)); break;
        case RDF_FAMILY_CELL_ORTHO:
        case RDF_FAMILY_TRI_CULLED: MDX_TRY(accumulate_cell(h, p, in, nf)); break;
        default: MDX_TRY(accumulate_tiles(h, p, in, nf));
        }
    }
    return MDX_OK;
}

// Entry of every accumulate variant: sets with a grouping are reduced to centres of mass first.
// drop_axis: dst = src with coordinate `axis` set to zero (may run in place)
__global__ __launch_bounds__(256) void rdf_drop_axis_kernel(const float *src, float *dst,
                                                            int64_t n_rows, int axis)
{
    const int64_t i = blockIdx.x * int64_t(256) + threadIdx.x;
    if (i >= n_rows * 3)
        return;
    dst[i] = (int)(i % 3) == axis ? 0.f : src[i];
}

// ... and the frame's cell: lengths[axis] = max(lengths) (structure.py:766)
__global__ __launch_bounds__(256) void rdf_drop_box_kernel(const float *__restrict__ src,
                                                           float *__restrict__ dst, int64_t n_frames,
                                                           int axis)
{
    const int64_t f = blockIdx.x * int64_t(256) + threadIdx.x;
    if (f >= n_frames)
        return;
    float b[6];
    for (int k = 0; k < 6; ++k)
        b[k] = src[6 * f + k];
    b[axis] = fmaxf(b[0], fmaxf(b[1], b[2]));
    for (int k = 0; k < 6; ++k)
        dst[6 * f + k] = b[k];
}

static int accumulate_device(mdx_rdf *h, const float *d_pos1, int64_t n1, const float *d_pos2,
                             int64_t n2, const float *d_boxes, const float *h_boxes,
                             int64_t n_frames)
{
    if (!h->grouping[0].n_groups && !h->grouping[1].n_groups && h->drop_axis < 0)
        return accumulate_device_points(h, d_pos1, n1, d_pos2, n2, d_boxes, h_boxes, n_frames);
    if (n_frames == 0)
        return MDX_OK;
    const bool same = (d_pos2 == nullptr || (d_pos2 == d_pos1 && n2 == n1));
    const float *src[2] = {d_pos1, same ? d_pos1 : d_pos2};
    int64_t n[2] = {n1, same ? n1 : n2};
    const float *pts[2] = {src[0], src[1]};
    bool owned[2] = {false, false};
    MDX_REQUIRE(!same || !h->grouping[1].n_groups || h->grouping[0].n_groups,
                "a self histogram takes the grouping of set 1");
    for (int g = 0; g < (same ? 1 : 2); ++g) {
        MoleculeStage &G = h->grouping[g];
        if (!G.active())
            continue;
        MDX_REQUIRE(n[g] == G.n_atoms, "set %d holds %lld particles, its grouping was defined for %lld",
                    g + 1, (long long)n[g], (long long)G.n_atoms);
        MDX_TRY(G.run(h->stream, src[g], n_frames, nullptr, &pts[g]));
        n[g] = G.n_groups;
        owned[g] = true;
    }
    std::vector<float> boxes_host;
    if (h->drop_axis >= 0) {
        // after the centres of mass, as the reference orders it (structure.py:753-766)
        for (int g = 0; g < (same ? 1 : 2); ++g) {
            float *dst = const_cast<float *>(pts[g]);
            if (!owned[g]) {
                MDX_TRY(h->d_drop[g].ensure(size_t(12) * n[g] * n_frames));
                dst = h->d_drop[g].as<float>();
            }
            const int64_t rows = n[g] * n_frames;
            hipLaunchKernelGGL(rdf_drop_axis_kernel, dim3((unsigned)ceil_div(rows * 3, 256)), dim3(256), 0,
                               h->stream, pts[g], dst, rows, h->drop_axis);
            pts[g] = dst;
        }
        if (d_boxes) {
            MDX_TRY(h->d_drop_box.ensure(size_t(24) * n_frames));
            hipLaunchKernelGGL(rdf_drop_box_kernel, dim3((unsigned)ceil_div(n_frames, 256)), dim3(256), 0,
                               h->stream, d_boxes, h->d_drop_box.as<float>(), n_frames, h->drop_axis);
            d_boxes = h->d_drop_box.as<float>();
            if (h_boxes) {
                boxes_host.assign(h_boxes, h_boxes + 6 * n_frames);
                for (int64_t f = 0; f < n_frames; ++f) {
                    float *b = boxes_host.data() + 6 * f;
                    b[h->drop_axis] = std::max(b[0], std::max(b[1], b[2]));
                }
                h_boxes = boxes_host.data();
            }
        }
    }
    MDX_HIP(hipGetLastError());
    if (same)
        return accumulate_device_points(h, pts[0], n[0], nullptr, n[0], d_boxes, h_boxes, n_frames);
    return accumulate_device_points(h, pts[0], n[0], pts[1], n[1], d_boxes, h_boxes, n_frames);
}

static int check_host_boxes(const float *boxes, int64_t n_frames)
{
    for (int64_t f = 0; boxes && f < n_frames; ++f) {
        const float *b = boxes + 6 * f;
        MDX_REQUIRE(b[0] > 0.f && b[1] > 0.f && b[2] > 0.f,
                    "frame %lld: box lengths must be positive", (long long)f);
    }
    return MDX_OK;
}

// Host-buffer and trajectory-file entry points: slabs of frames go through the double-buffered
// staging sets (StagePipeline).  fill(b, f0, nf) queues on the copy stream whatever brings
// frames [f0, f0+nf) into d_stage1[b] (and d_stage2[b] unless `same`).
// prepare(b, f0, nf): queued on the COMPUTE stream ahead of the slab's kernels (the unpack of raw frames).
template <typename Fill, typename Prepare>
static int accumulate_pipelined(mdx_rdf *h, int64_t n1, int64_t n2, bool same, const float *boxes,
                                int64_t n_frames, int64_t source_bytes_per_frame, Fill fill, Prepare prepare)
{
    // slabs of ~256 MiB (MDX_RDF_PIPE_MB), the first two a quarter and a half of that: each slab is one sort + one
    // pair launch on the compute stream; the persistent pair kernel ends on a tail of about one item per block
    // (2 % of a launch of 336 frames at C2, 0.7 % of one of 1 000) and a call of one slab sorts serially, so longer
    // launches are worth more than finer overlap; a multiple of 8 frames, so that every XCD gets the same number
    const char *mb_env = getenv("MDX_RDF_PIPE_MB");
    const int64_t pipe_mb = mb_env ? std::min<long long>(std::max<long long>(atoll(mb_env), 1), 4096) : 256;
    int64_t slab = std::max<int64_t>(1, (pipe_mb << 20) / source_bytes_per_frame);
    if (slab >= 8)
        slab -= slab % 8;
    slab = std::min<int64_t>(n_frames, slab);
    return h->pipe.run(
        h->stream, n_frames, slab,
        [&](int b, int64_t f0, int64_t nf) -> int {
            MDX_TRY(h->d_stage1[b].ensure(size_t(12) * n1 * slab));
            if (!same)
                MDX_TRY(h->d_stage2[b].ensure(size_t(12) * n2 * slab));
            MDX_TRY(fill(b, f0, nf, slab));
            if (boxes) {
                MDX_TRY(h->d_boxes[b].ensure(size_t(24) * slab));
                MDX_HIP(hipMemcpyAsync(h->d_boxes[b].ptr, boxes + f0 * 6, size_t(24) * nf,
                                       hipMemcpyHostToDevice, h->pipe.copy_stream));
            }
            return MDX_OK;
        },
        [&](int b, int64_t f0, int64_t nf) -> int {
            MDX_TRY(prepare(b, f0, nf));
            return accumulate_device(h, h->d_stage1[b].as<float>(), n1,
                                     same ? nullptr : h->d_stage2[b].as<float>(), n2,
                                     boxes ? h->d_boxes[b].as<float>() : nullptr,
                                     boxes ? boxes + f0 * 6 : nullptr, nf);
        },
        8);
}

extern "C" {

int mdx_rdf_create(mdx_rdf_t *out, int dev, int n_bins, const double *edges, int64_t excl1,
                   int64_t excl2, int algo)
{
    MDX_TRY(rdf_check_engine_args(out, n_bins, edges, excl1, excl2, algo));
    MDX_TRY(set_device(dev));
    mdx_rdf *h = new mdx_rdf();
    h->dev = dev;
    h->n_bins = n_bins;
    h->edges.assign(edges, edges + n_bins + 1);
    h->excl1 = excl1;
    h->excl2 = excl2;
    h->algo = algo;
    // thresholds in the squared-distance domain
    h->thresh.resize(n_bins + 1);
    for (int b = 0; b <= n_bins; ++b)
        h->thresh[b] = thresh_ge(edges[b]);
    // capped_distance: d > r0 - eps (structure.py:94); numpy.histogram: r0 <= d <= r1
    const double min_cut = edges[0] - 2.220446049250313e-16;
    h->t_lo = std::max(h->thresh[0], thresh_gt(min_cut));
    h->t_hi = thresh_gt(edges[n_bins]);
    int rc = MDX_OK;
    do {
        if ((rc = stream_acquire(&h->stream)) != MDX_OK)
            break;
        h->timer.stream = h->stream;
        if ((rc = h->d_thresh.ensure(sizeof(double) * (n_bins + 1))) != MDX_OK) break;
        if ((rc = h->d_counts.ensure(sizeof(uint64_t) * size_t(h->n_rep) * n_bins)) != MDX_OK) break;
        if ((rc = h->d_total.ensure(sizeof(uint64_t) * n_bins)) != MDX_OK) break;
        if ((rc = h->d_misc.ensure(64)) != MDX_OK) break;
        if ((rc = h->d_stats.ensure(RDF_STAT_BYTES)) != MDX_OK) break;
        if ((rc = h->d_work.ensure(CELL_WORK_BYTES)) != MDX_OK) break;
        if (hipMemcpy(h->d_thresh.ptr, h->thresh.data(), sizeof(double) * (n_bins + 1),
                      hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(MDX_ERR_HIP, "threshold upload failed");
            break;
        }
    } while (0);
    if (rc != MDX_OK) {
        mdx_rdf_destroy(h);
        return rc;
    }
    *out = h;
    return mdx_rdf_reset(h);
}

// The float32 filter constants the cell-sorted pair kernel takes for an orthorhombic frame with cell lengths `box`
// and a batch whose largest |coordinate| is max_abs; touches no device.  The slots are documented in mdx.h.
int mdx_rdf_filter_constants(int n_bins, double r0, double r1, const float box[3], float max_abs,
                             double out[MDX_RDF_FILTER_SLOTS])
{
    MDX_REQUIRE(box && out, "NULL argument");
    MDX_REQUIRE(n_bins >= 1 && n_bins <= (1 << 20), "n_bins=%d out of range", n_bins);
    MDX_REQUIRE(r0 >= 0.0 && r1 > r0, "bad range");
    MDX_REQUIRE(box[0] > 0.f && box[1] > 0.f && box[2] > 0.f, "bad cell");
    const double Lmax = std::max((double)box[0], std::max((double)box[1], (double)box[2]));
    const RdfFilterConst f = rdf_filter_const(Lmax, (double)max_abs, r0, r1, n_bins);
    const float pos0 = cell_pos0(f.r0f, f.inv_wf, f.eta), sure_w = cell_sure_w(f.eta);
    out[0] = f.eta;
    out[1] = sure_w;
    out[2] = cell_fixed_tq(sure_w);
    out[3] = f.inv_wf;
    out[4] = pos0;
    out[5] = f.inv_wf * 65536.0f;
    out[6] = pos0 * 65536.0f;
    out[7] = f.cand_hi;
    out[8] = f.cand_lo;
    out[9] = 0.0;
    return MDX_OK;
}

// What an engine created with these arguments would launch for one run of n_frames frames of one cell kind; touches
// no device.  The slots are documented in mdx.h.
int mdx_rdf_plan(int n_bins, const double *edges, int64_t excl1, int64_t excl2, int algo, int64_t n1, int64_t n2,
                 int same, const float *boxes, int64_t n_frames, int64_t out[MDX_RDF_PLAN_SLOTS])
{
    MDX_TRY(rdf_check_engine_args(out, n_bins, edges, excl1, excl2, algo));
    if (same)
        n2 = n1;
    MDX_REQUIRE(n1 >= 1 && n2 >= 1 && n_frames >= 1, "bad size");
    MDX_TRY(rdf_check_set_sizes(n1, n2));
    bool ortho = true;
    float min_edge = 0.f;
    std::vector<float> tri;
    if (boxes) {
        MDX_TRY(check_host_boxes(boxes, n_frames));
        const int64_t f1 = rdf_next_run(boxes, 0, n_frames, &ortho, &min_edge);
        MDX_REQUIRE(f1 == n_frames,
                    "frame %lld: orthorhombic and triclinic frames in one run (plan each run of one kind)",
                    (long long)f1);
        if (!ortho)
            MDX_TRY(rdf_tri_cells(boxes, n_frames, tri));
    }
    const RdfConfig cfg{n_bins, edges[0], edges[n_bins], excl1, excl2, algo};
    rdf_plan_slots(rdf_plan_run(cfg, n1, n2, same != 0, boxes != nullptr, ortho, min_edge,
                                ortho ? nullptr : tri.data(), n_frames), out);
    return MDX_OK;
}

// The plan of the handle's most recent run, as it was launched.
int mdx_rdf_last_plan(mdx_rdf_t h, int64_t out[MDX_RDF_PLAN_SLOTS])
{
    MDX_REQUIRE(h && out, "NULL argument");
    if (h->last_plan.n_slabs == 0)
        return fail(MDX_ERR_STATE, "no run since the handle was created or reset");
    rdf_plan_slots(h->last_plan, out);
    return MDX_OK;
}

int mdx_rdf_destroy(mdx_rdf_t h)
{
    if (!h)
        return MDX_OK;
    (void)hipSetDevice(h->dev);
    // every stream that may still touch the handle's memory drains first: the blocks go back to the device's
    // cache (DeviceBuffer::recycle), not through hipFree, which would wait for the device itself
    if (h->stream)
        (void)hipStreamSynchronize(h->stream);
    if (h->pipe.copy_stream)
        (void)hipStreamSynchronize(h->pipe.copy_stream);
    if (h->side)
        (void)hipStreamSynchronize(h->side);
    h->timer.destroy();
    h->pipe.destroy();
    for (hipEvent_t e : {h->ev_fork, h->ev_join, h->ev_sorted[0], h->ev_sorted[1], h->ev_read[0], h->ev_read[1]})
        if (e)
            (void)hipEventDestroy(e);
    for (DeviceBuffer *b : {&h->d_thresh, &h->d_counts, &h->d_total, &h->d_pack1, &h->d_pack2,
                            &h->d_stage1[0], &h->d_stage2[0], &h->d_boxes[0], &h->d_stage1[1],
                            &h->d_stage2[1], &h->d_boxes[1], &h->d_rawslab[0], &h->d_rawslab[1], &h->d_index[0], &h->d_index[1], &h->d_tri, &h->d_misc, &h->d_stats, &h->d_work, &h->d_frame_geo, &h->d_pw1,
                            &h->d_po1, &h->d_bb1, &h->d_pw2, &h->d_po2, &h->d_bb2, &h->d_bb16_1,
                            &h->d_bb16_2, &h->d_drop[0], &h->d_drop[1], &h->d_drop_box})
        b->recycle();
    h->grouping[0].recycle();
    h->grouping[1].recycle();
    if (h->side)
        stream_release(h->side);
    if (h->stream)
        stream_release(h->stream);
    delete h;
    return MDX_OK;
}

int mdx_rdf_reset(mdx_rdf_t h)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_HIP(hipMemsetAsync(h->d_counts.ptr, 0, sizeof(uint64_t) * size_t(h->n_rep) * h->n_bins,
                           h->stream));
    MDX_HIP(hipMemsetAsync(h->d_misc.ptr, 0, 64, h->stream));
    MDX_HIP(hipMemsetAsync(h->d_stats.ptr, 0, RDF_STAT_BYTES, h->stream));
    MDX_HIP(hipStreamSynchronize(h->stream));
    h->timer.reset();
    h->pairs_evaluated = 0;
    h->pairs_bruteforce = 0;
    h->slabs_sorted_beside = 0;
    h->reduced_global = false;
    h->last_plan = RdfRunPlan();
    return MDX_OK;
}

int mdx_rdf_set_drop_axis(mdx_rdf_t h, int axis)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_REQUIRE(axis >= -1 && axis <= 2, "axis must be 0, 1, 2 or -1 (none)");
    h->drop_axis = axis;
    return MDX_OK;
}

int mdx_rdf_set_grouping(mdx_rdf_t h, int which, int64_t n_groups, const int64_t *offsets,
                         const double *masses)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_REQUIRE(which == 1 || which == 2, "which must be 1 or 2");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    return h->grouping[which - 1].set(n_groups, offsets, masses);
}

int mdx_rdf_accumulate_device(mdx_rdf_t h, const float *d_pos1, int64_t n1, const float *d_pos2,
                              int64_t n2, const float *d_boxes, int64_t n_frames)
{
    MDX_REQUIRE(h && d_pos1, "NULL argument");
    MDX_REQUIRE(n1 >= 0 && n2 >= 0 && n_frames >= 0, "negative size");
    MDX_TRY(set_device(h->dev));
    return accumulate_device(h, d_pos1, n1, d_pos2, n2, d_boxes, nullptr, n_frames);
}

int mdx_rdf_accumulate(mdx_rdf_t h, const float *pos1, int64_t n1, const float *pos2, int64_t n2,
                       const float *boxes, int64_t n_frames)
{
    MDX_REQUIRE(h && pos1, "NULL argument");
    MDX_REQUIRE(n1 >= 0 && n2 >= 0 && n_frames >= 0, "negative size");
    MDX_TRY(set_device(h->dev));
    if (n_frames == 0 || n1 == 0)
        return MDX_OK;
    const bool same = (pos2 == nullptr || (pos2 == pos1 && n2 == n1));
    if (pos2 == nullptr)
        n2 = n1;
    if (n2 == 0)
        return MDX_OK;
    MDX_TRY(check_host_boxes(boxes, n_frames));
    return accumulate_pipelined(
        h, n1, n2, same, boxes, n_frames, 12 * std::max(n1, n2),
        [&](int b, int64_t f0, int64_t nf, int64_t) -> int {
            // caller memory -> pinned ring (host threads) -> HBM; pinned / registered caller
            // memory is read by the DMA engine where it lies
            MDX_TRY(device_stager(h->dev).upload(h->dev, h->pipe.copy_stream, h->d_stage1[b].ptr,
                                          pos1 + f0 * n1 * 3, size_t(12) * n1 * nf));
            if (!same)
                MDX_TRY(device_stager(h->dev).upload(h->dev, h->pipe.copy_stream, h->d_stage2[b].ptr,
                                              pos2 + f0 * n2 * 3, size_t(12) * n2 * nf));
            return MDX_OK;
        },
        [](int, int64_t, int64_t) -> int { return MDX_OK; });
}

// Frames straight from a trajectory file (mdx_traj.hip): raw records -> pinned -> HBM ->
// unpack/gather into the staging slabs, overlapped with the pair kernels of the previous slab.
int mdx_rdf_accumulate_traj(mdx_rdf_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,
                            const float *boxes, const int32_t *index1, int64_t n1,
                            const int32_t *index2, int64_t n2)
{
    MDX_REQUIRE(h && traj, "NULL handle");
    MDX_REQUIRE(n1 >= 0 && n2 >= 0 && n_frames >= 0, "negative size");
    MDX_REQUIRE(n_frames == 0 || frames, "NULL frame list");
    MDX_TRY(set_device(h->dev));
    Trajectory *t = mdx_traj_internal(traj);
    const bool same = (index2 == nullptr && n2 == 0);
    if (index1 == nullptr)
        n1 = t->n_atoms;
    if (same)
        n2 = n1;
    else if (index2 == nullptr)
        n2 = t->n_atoms;
    if (n_frames == 0 || n1 == 0 || n2 == 0)
        return MDX_OK;
    MDX_TRY(check_host_boxes(boxes, n_frames));
    // particle selections live on the device for the unpack kernel
    const int32_t *host_idx[2] = {index1, same ? nullptr : index2};
    const int64_t n_idx[2] = {n1, n2};
    const int *d_idx[2] = {nullptr, nullptr};
    for (int g = 0; g < 2; ++g) {
        if (!host_idx[g])
            continue;
        for (int64_t i = 0; i < n_idx[g]; ++i)
            if (host_idx[g][i] < 0 || host_idx[g][i] >= t->n_atoms)
                return fail(MDX_ERR_INVALID_VALUE, "particle index %d out of range [0, %lld)",
                            host_idx[g][i], (long long)t->n_atoms);
        MDX_TRY(h->pipe.ensure());
        // an earlier call's unpack kernels may still be reading the previous selection
        MDX_HIP(hipStreamSynchronize(h->pipe.copy_stream));
        MDX_TRY(h->d_index[g].ensure(size_t(4) * n_idx[g]));
        MDX_HIP(hipMemcpy(h->d_index[g].ptr, host_idx[g], size_t(4) * n_idx[g],
                          hipMemcpyHostToDevice));
        d_idx[g] = h->d_index[g].as<int>();
    }
    // raw frames -> pinned ring -> HBM by DMA on the ring's stream, beside the kernels of the previous slab;
    // the unpack kernel (byte swap / plane transpose / gather) is queued on the compute stream ahead of the
    // slab's sort: the persistent pair kernel leaves no wave slot for a kernel on another stream
    return accumulate_pipelined(
        h, n1, n2, same, boxes, n_frames, 12 * t->n_atoms,
        [&](int b, int64_t f0, int64_t nf, int64_t slab) -> int {
            MDX_TRY(h->d_rawslab[b].ensure(size_t(12) * t->n_atoms * slab));
            return t->stage_raw_async(h->dev, h->pipe.copy_stream, frames + f0, nf, h->d_rawslab[b].ptr);
        },
        [&](int b, int64_t, int64_t nf) -> int {
            TrajSelection sel[2] = {{d_idx[0], n1, h->d_stage1[b].as<float>()},
                                    {d_idx[1], n2, same ? nullptr : h->d_stage2[b].as<float>()}};
            return t->unpack_async(h->stream, h->d_rawslab[b].ptr, nf, sel, same ? 1 : 2);
        });
}

// Sum of the statistics shards after the stream has drained: [0] exact pairs, [1] units, [2] general units,
// [3] engine-clock ticks, [4] 100 MHz ticks.
static int read_stats(mdx_rdf *h, unsigned long long out[5])
{
    MDX_HIP(hipStreamSynchronize(h->stream));
    std::vector<unsigned long long> raw(size_t(RDF_STAT_SHARDS) * RDF_STAT_STRIDE);
    MDX_HIP(hipMemcpy(raw.data(), h->d_stats.ptr, RDF_STAT_BYTES, hipMemcpyDeviceToHost));
    for (int k = 0; k < 5; ++k)
        out[k] = 0;
    for (unsigned sh = 0; sh < RDF_STAT_SHARDS; ++sh)
        for (int k = 0; k < 5; ++k)
            out[k] += raw[size_t(sh) * RDF_STAT_STRIDE + k];
    return MDX_OK;
}

int mdx_rdf_synchronize(mdx_rdf_t h)
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    h->timer.collect();
    unsigned misc[4] = {0, 0, 0, 0};
    MDX_HIP(hipMemcpy(misc, h->d_misc.ptr, sizeof(misc), hipMemcpyDeviceToHost));
    if (misc[1] & 1u)
        return fail(MDX_ERR_UNSUPPORTED,
                    "a frame has a non-orthorhombic or non-positive box; counts are invalid");
    return MDX_OK;
}

static int reduce_to_total(mdx_rdf *h)
{
    hipLaunchKernelGGL(rdf_reduce_kernel, dim3((unsigned)ceil_div(h->n_bins, 256)), dim3(256), 0,
                       h->stream, h->d_counts.as<unsigned long long>(), h->n_rep, h->n_bins,
                       h->d_total.as<unsigned long long>());
    MDX_HIP(hipGetLastError());
    return MDX_OK;
}

int mdx_rdf_counts(mdx_rdf_t h, int64_t *counts)
{
    MDX_REQUIRE(h && counts, "NULL argument");
    MDX_TRY(set_device(h->dev));
    MDX_TRY(reduce_to_total(h));
    MDX_TRY(mdx_rdf_synchronize(h));
    MDX_HIP(hipMemcpy(counts, h->d_total.ptr, sizeof(int64_t) * h->n_bins, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_rdf_stats(mdx_rdf_t h, int64_t *launches, double *kernel_ms, int64_t *pairs_evaluated,
                  int64_t *pairs_exact, int64_t *pairs_computed)
{
    if (pairs_computed && h) {
        // distance evaluations actually executed: brute-force tiles + culled cell tiles
        unsigned long long st[5];
        if (set_device(h->dev) == MDX_OK && read_stats(h, st) == MDX_OK)
            *pairs_computed = h->pairs_bruteforce + (int64_t)st[1] * 64 * CELL_CHUNK;
    }
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    h->timer.collect();
    if (launches) *launches = h->timer.launches;
    if (kernel_ms) *kernel_ms = h->timer.total_ms;
    if (pairs_evaluated) *pairs_evaluated = h->pairs_evaluated;
    if (pairs_exact) {
        unsigned long long st[5];
        MDX_TRY(read_stats(h, st));
        *pairs_exact = (int64_t)st[0];
    }
    return MDX_OK;
}

int mdx_rdf_kernel_clock(mdx_rdf_t h, double *hz)
{
    MDX_REQUIRE(h && hz, "NULL argument");
    MDX_TRY(set_device(h->dev));
    unsigned long long st[5];
    MDX_TRY(read_stats(h, st));
    // s_memrealtime counts at 100 MHz
    *hz = st[4] ? double(st[3]) / double(st[4]) * 1.0e8 : 0.0;
    return MDX_OK;
}

int mdx_rdf_debug_counters(mdx_rdf_t h, int64_t out[4])
{
    MDX_REQUIRE(h && out, "NULL argument");
    MDX_TRY(set_device(h->dev));
    unsigned long long raw[5];
    MDX_TRY(read_stats(h, raw));
    out[0] = (int64_t)raw[0];   // pairs re-evaluated exactly
    out[1] = (int64_t)raw[1];   // (64 i) x (16 j) units evaluated by the cell kernel
    out[2] = (int64_t)raw[2];   // ... of which on the per-pair image-search path
    out[3] = h->pairs_bruteforce;
    return MDX_OK;
}

int mdx_rdf_slabs_sorted_beside(mdx_rdf_t h, int64_t *out)
{
    MDX_REQUIRE(h && out, "NULL argument");
    *out = h->slabs_sorted_beside;
    return MDX_OK;
}

int mdx_rdf_debug_sorted(mdx_rdf_t h, int64_t frame, int64_t n_pad, float *pw, float *po)
{
    MDX_REQUIRE(h && pw && po, "NULL argument");
    MDX_TRY(set_device(h->dev));
    MDX_HIP(hipStreamSynchronize(h->stream));
    MDX_REQUIRE(h->last_frames > 0 && h->last_plan.cell(), "no slab has gone through the cell-sorted path yet");
    MDX_REQUIRE(frame >= 0 && frame < h->last_frames, "frame %lld outside the last slab (%lld frames)",
                (long long)frame, (long long)h->last_frames);
    MDX_REQUIRE(n_pad == h->last_plan.n1p, "n_pad is %lld for the last slab", (long long)h->last_plan.n1p);
    // the slab's own set of sorted copies (two sets alternate when the sort runs beside the pair kernel)
    MDX_HIP(hipMemcpy(pw, h->d_pw1.as<float4>() + h->last_offset + frame * n_pad, size_t(16) * n_pad,
                      hipMemcpyDeviceToHost));
    if (h->last_plan.lazy_orig)
        // exclusion 0 or 1: no sorted copy of the original coordinates exists (the exact path reads the
        // incoming frame by the tag in pw[..].w); say so instead of returning something else in its place
        return fail(MDX_ERR_STATE, "the last slab has no sorted originals (exclusion 0 or 1): pw is filled, "
                    "po is not; MDX_RDF_SORTED_ORIGINALS=1 materialises them");
    MDX_HIP(hipMemcpy(po, h->d_po1.as<float4>() + h->last_offset + frame * n_pad, size_t(16) * n_pad,
                      hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_rdf_enable_timing(mdx_rdf_t h, int on)
{
    MDX_REQUIRE(h, "NULL handle");
    h->timer.enabled = on != 0;
    return MDX_OK;
}

// used by mdx_comm.hip
int mdx_rdf_internal_total(mdx_rdf_t h, unsigned long long **d_total, hipStream_t *stream)
{
    MDX_TRY(set_device(h->dev));
    MDX_TRY(reduce_to_total(h));
    *d_total = h->d_total.as<unsigned long long>();
    *stream = h->stream;
    return MDX_OK;
}

int mdx_rdf_internal_nbins(mdx_rdf_t h) { return h->n_bins; }

int mdx_rdf_internal_adopt_total(mdx_rdf_t h)
{
    // replica 0 <- all-reduced total, other replicas <- 0
    MDX_HIP(hipMemsetAsync(h->d_counts.ptr, 0, sizeof(uint64_t) * size_t(h->n_rep) * h->n_bins,
                           h->stream));
    MDX_HIP(hipMemcpyAsync(h->d_counts.ptr, h->d_total.ptr, sizeof(uint64_t) * h->n_bins,
                           hipMemcpyDeviceToDevice, h->stream));
    h->reduced_global = true;
    return MDX_OK;
}

int mdx_radial_histogram(int dev, const float *pos1, int64_t n1, const float *pos2, int64_t n2,
                         int n_bins, const double *edges, const float dims[6], int64_t excl1,
                         int64_t excl2, int64_t *counts)
{
    MDX_REQUIRE(counts, "counts is NULL");
    mdx_rdf_t h = nullptr;
    // (checks the arguments, the edges among them, before it touches the device)
    MDX_TRY(mdx_rdf_create(&h, dev, n_bins, edges, excl1, excl2, MDX_RDF_ALGO_AUTO));
    int rc = mdx_rdf_accumulate(h, pos1, n1, pos2, n2, dims, 1);
    if (rc == MDX_OK)
        rc = mdx_rdf_counts(h, counts);
    mdx_rdf_destroy(h);
    return rc;
}

}  // extern "C"
