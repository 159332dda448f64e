// mdx_angle_device.hpp — device side of the angular distribution engine (mdx_angle.hip).
//
// Result contract.
//
// Rows.  The incoming rows of a frame are the n0 centres, then the ligands group by group: G ligand groups,
// 1 <= G <= 4, of sizes n_g; ligand j = 0 ... n_lig - 1 (n_lig = sum n_g) is row n0 + j, and species(j) is the group
// whose range of j holds it.  With `same`, G = 1 and the ligands are the centres themselves: the rows arrive once, n0
// of them, ligand j is row j, and j == i never counts.  Otherwise the centres and all ligand groups are pairwise
// disjoint sets of atoms.
//
// Box and pair arithmetic: those of mdx_pairs_device.hpp, for centre i and ligand j of frame f, with r2_ij its r2:
//
//     j is a neighbour of i  iff  r2_ij <= rc2[species(j)],  rc2[g] = cutoff[g] * cutoff[g] formed once on the host
//
// A NaN r2 is never a neighbour (the comparison fails).
//
// Triplets.  For every frame, every centre i and every unordered pair {j, k}, j != k, of its neighbours:
//
//     dot = (w_ijx*w_ikx + w_ijy*w_iky) + w_ijz*w_ikz
//     c   = dot / sqrt(r2_ij * r2_ik)            (one multiply, one correctly rounded sqrt, one correctly rounded divide)
//
// Every operation is symmetric in j and k (products and sums of two operands commute), so c does not depend on the
// order in which the neighbours were appended to the list of i.
//
// Bins.  thresholds is a float64 array t[0 ... n_bins], strictly decreasing (the host refuses any other).  The bin of a
// triplet is
//
//     b = #{ m in 1 ... n_bins - 1 : c <= t[m] }
//
// so bin b holds t[b + 1] < c <= t[b]; the first bin also takes c > t[0] (rounding above 1) and the last one
// c <= t[n_bins] (theta = 180 degrees stays inside, as the last bin of numpy.histogram is closed).  Only the inner
// thresholds t[1] ... t[n_bins - 1] are ever compared.  A c that is NaN goes into no bin: a ligand sits on its centre
// (r2 == 0, so c = 0 / 0) and the triplet adds 1 to degenerate[p].  The contract is stated on thresholds of c, not on
// an angle: acos is correctly rounded on neither side, while /, sqrt and the comparisons are.
//
// Results, all integers (uint64 in HBM, handed out as int64), added with integer atomics only:
//     counts[p][b]         p numbers the unordered pair of ligand species (a <= b) of the triplet's two ligands:
//                          p = a*G - a*(a-1)/2 + (b-a), P = G (G + 1) / 2
//     degenerate[p]
//     coordination[g][m]   m = 0 ... max_neighbors: the (frame, centre) cases in which the centre had exactly m
//                          neighbours of species g, so that sum_m coordination[g][m] == F * n0
//
// Capped lists (mdx_pairs_device.hpp).  A centre holds at most max_neighbors (1 ... 64) neighbours of all species
// together in one frame; a row that would hold more refuses the results (MDX_ERR_INVALID_VALUE, naming max_neighbors
// and the largest row).  Exactly full is no error.
//
// evaluations is the contract's count F * (n0 * n_lig - (same ? n0 : 0)); triplets = sum counts + sum degenerate.
//
// The lists are a function of the frame alone as sets, c and its bin a function of the set alone, and every tally is
// an integer add or max (atomics on integers commute): the numbers are the same whatever the input route, the index,
// the split into calls or slabs, the grid, or the arrival order of the atomics.  There is no floating-point atomic
// anywhere in this engine.
//
// Shape.  Two phases per slab of frames; a frame never needs another, so there is no history.
//
// Phase 1, neighbour lists (the hot path, F * n0 * n_lig evaluations).  gather_kernel gathers the rows of a slab
// component-major float32.  ang_contact_kernel is the walk of mdx_pairs_device.hpp with z = frames and ANG_JCHUNK
// ligands per block.  The thread that stages ligand j puts rc2[species(j)] into the fourth word of its stage entry.
// Ligands arrive group by group, so a stage holds one species where species(first) == species(last): the lane then
// takes its bound once for the stage, and only a stage that spans two groups reads the bound beside each partner, as
// clu_contact_kernel does.  UNIFORM (every cutoff is one value): rc2 is a kernel argument.  A neighbour takes
// slot = atomicAdd(&len[f][i], 1) and is stored at list[f][slot][i] when slot < max_neighbors (slot-major: the angle
// kernel's lanes read consecutive i); several j chunks append to one row.  Each block adds its largest row to max_row
// with one atomicMax (the max-only block_tally).
//
// Phase 2, angles (ang_triplet_kernel).  A centre with m neighbours has m (m - 1) / 2 pairs, 6 ... 28 in a real first
// shell and 2016 at the cap, so neither a lane nor a wave per centre keeps the lanes busy.  A block walks tiles of
// ANG_CTILE centres of one frame (a grid-stride loop over (frame, tile), so that its histograms live across tiles).
// Per tile it
//   - reads the tile's row lengths (capped at max_neighbors; an overflowing row: the host refuses the results) and
//     widens the centres into LDS;
//   - re-derives w_ij for every list entry from the slab with the contract's own operations, so that nothing but the
//     row indices lives in HBM: the same inputs and the same operations give the bits phase 1 saw.  w and the species
//     go to LDS, entry (centre c, slot s) at c * ANG_MAX_NEIGHBORS + s; r2_ij is formed again from w by the lane that
//     needs it (three multiplies and two adds, the contract's own);
//   - forms the prefix sum of the centres' pair counts and deals the flattened (centre, pair) items to the lanes,
//     256 at a time: item q of a centre is the pair (a, b), a < b, with q = b (b - 1) / 2 + a;
//   - adds coordination[g][m] per centre and species, into uint32 counters in LDS.
// Each wave counts into its own uint32 histogram in LDS (LDS atomics: lanes of a wave may meet in a bin); the inner
// thresholds sit in LDS too and the bin is found by a binary search for the number of thresholds that are >= c, which
// is the rule above because t decreases.  At the end the block adds the waves' histograms and sends the non-zero sums
// to the uint64 counts with one integer atomic each.
//   The uint32 counters cannot wrap: a tile adds at most ANG_CTILE * 2016 = 32 256 triplets, and the host sizes the
//   grid so that a block walks at most ANG_BLOCK_TILES = 65 536 tiles in a launch: at most 2 113 929 216 < 2^31 adds
//   to all the counters of a block together (coordination: at most ANG_CTILE adds a tile and species).
//   Where the switch is: the LDS form needs P * n_bins <= ANG_HIST_WORDS (1920: four species at 180 bins fit) and
//   n_bins <= ANG_LDS_BINS (512).  Beyond either the same kernel counts in HBM directly, one uint64 atomic per
//   triplet, and reads the thresholds from HBM, as vhd_pair_kernel does for its large histograms.
//
// No cell list and no spatial culling: every (centre, ligand) pair is evaluated.  Culling by cells is the follow-up
// (DESIGN.md §10).
#pragma once

#include "mdx_pairs_device.hpp"

namespace mdx_ang_dev {

using namespace mdx_pairs_dev;

constexpr int ANG_TILE = PAIR_TILE;           // centres per block of phase 1, one per lane
constexpr int ANG_THREADS = PAIR_THREADS;
constexpr int ANG_WAVES = PAIR_WAVES;
constexpr int ANG_STAGE = PAIR_STAGE;         // ligands per LDS stage, one staged per thread
constexpr int ANG_JCHUNK = 4 * ANG_STAGE;     // ligands per block
constexpr int ANG_MAX_NEIGHBORS = PAIR_MAX_NEIGHBORS;   // slots of a row at most
constexpr int ANG_MAX_SPECIES = 4;
constexpr int ANG_MAX_PAIRS = ANG_MAX_SPECIES * (ANG_MAX_SPECIES + 1) / 2;
constexpr int64_t ANG_SLAB_MAX = PAIR_SLAB_MAX;         // frames per launch, at most (grid z)
constexpr int ANG_CTILE = 16;                 // centres per tile of phase 2
constexpr int ANG_ENTRIES = ANG_CTILE * ANG_MAX_NEIGHBORS;
constexpr int ANG_HIST_WORDS = 1920;          // uint32 words of a wave's histogram in LDS: P * n_bins at most
constexpr int ANG_LDS_BINS = 512;             // n_bins at most for thresholds in LDS
constexpr int64_t ANG_BLOCK_TILES = 65536;    // tiles a block of phase 2 walks in one launch, at most
constexpr int ANG_GRID = 2048;                // blocks of phase 2 unless ANG_BLOCK_TILES asks for more

// end[g]: one past the last ligand j of species g (INT_MAX for g >= G); rc2[g] = cutoff[g]^2
struct AngGroups {
    int end[ANG_MAX_SPECIES];
    double rc2[ANG_MAX_SPECIES];
};

__device__ __forceinline__ int ang_species(const AngGroups &groups, int j)
{
    return (j >= groups.end[0]) + (j >= groups.end[1]) + (j >= groups.end[2]);
}

// rc2 of ligand j (selects: a kernel argument indexed by a lane's value would go through scratch)
__device__ __forceinline__ double ang_bound(const AngGroups &groups, int j)
{
    return j < groups.end[0] ? groups.rc2[0] : j < groups.end[1] ? groups.rc2[1] : j < groups.end[2] ? groups.rc2[2]
                                                                                                     : groups.rc2[3];
}

// the number p of the unordered pair of species (a, b) among G
__device__ __forceinline__ int ang_pair(int a, int b, int G)
{
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return lo * G - lo * (lo - 1) / 2 + (hi - lo);
}

// The neighbour lists of slab frame blockIdx.z.  n_rows: rows of a slab frame; the n_lig ligands start at row off
// (0 with same).  keep: bit c set -> component c takes part; ALL: keep == 7, known when compiled.  UNIFORM: every
// species has the bound rc2; else groups names the species of a ligand and its bound.  len: int32 [slab][n0], zero;
// list: int32 [slab][max_nb][n0], ligand numbers j.
template <bool ALL, bool UNIFORM>
__global__ __launch_bounds__(ANG_THREADS) void ang_contact_kernel(
    const float *__restrict__ slab, int n_rows, int n0, int n_lig, int off, int same, int n_jchunks, PairBox box,
    int keep, double rc2, AngGroups groups, int max_nb, int *__restrict__ len, int *__restrict__ list,
    int *__restrict__ max_row)
{
    __shared__ __attribute__((aligned(16))) double stage[4 * ANG_STAGE];
    __shared__ unsigned int block_row;
    const int64_t fs = blockIdx.z;
    const int tile = blockIdx.x / n_jchunks, chunk = blockIdx.x - tile * n_jchunks;
    const int i = tile * ANG_TILE + threadIdx.x;
    const bool live = i < n0;
    const float *__restrict__ a = slab + fs * 3 * n_rows + (live ? i : n0 - 1);
    const float *__restrict__ b = slab + fs * 3 * n_rows + off;
    const double xi = (double)a[0], yi = (double)a[n_rows], zi = (double)a[2 * int64_t(n_rows)];
    int *__restrict__ my_len = len + fs * n0 + (live ? i : 0);
    int *__restrict__ my_list = list + fs * max_nb * n0 + (live ? i : 0);
    if (threadIdx.x == 0)
        block_row = 0u;
    unsigned int row = 0u;
    const int j_begin = chunk * ANG_JCHUNK;
    const int j_end = n_lig - j_begin < ANG_JCHUNK ? n_lig : j_begin + ANG_JCHUNK;
    for (int js = j_begin; js < j_end; js += ANG_STAGE) {
        const int nj = j_end - js < ANG_STAGE ? j_end - js : ANG_STAGE;
        __syncthreads();                    // the stage is free
        if ((int)threadIdx.x < nj) {
            stage_partners(stage, b, n_rows, js);
            if (!UNIFORM)                   // the bound of a ligand lies beside it
                stage[4 * threadIdx.x + 3] = ang_bound(groups, js + threadIdx.x);
        }
        __syncthreads();
        if (!live)
            continue;
        const int skip = same ? i - js : -1;        // the stage entry that is this lane's own row
        // groups are ranges of j: a stage holds one species where its first and last ligand are of one
        if (UNIFORM || ang_species(groups, js) == ang_species(groups, js + nj - 1)) {
            const double bound = UNIFORM ? rc2 : stage[3];
            stage_pairs<ALL>(stage, nj, js, skip, xi, yi, zi, box, keep,
                             [&](int, int j, double, double, double, double r2, bool other) {
                                 if (r2 <= bound && other)
                                     append_capped(my_len, my_list, n0, max_nb, j, row);
                             });
        } else {
            stage_pairs<ALL>(stage, nj, js, skip, xi, yi, zi, box, keep,
                             [&](int jj, int j, double, double, double, double r2, bool other) {
                                 if (r2 <= stage[4 * jj + 3] && other)
                                     append_capped(my_len, my_list, n0, max_nb, j, row);
                             });
        }
    }
    __syncthreads();                        // block_row is zero (no stage at all: the barrier above never ran)
    block_tally<false>(0u, row, nullptr, &block_row, nullptr, max_row);
}

// The pair (a, b), a < b, with q = b (b - 1) / 2 + a.  q < 2016, so the float root is off by one at most.
__device__ __forceinline__ void ang_unrank(int q, int &a, int &b)
{
    b = (int)((1.0f + __fsqrt_rn(1.0f + 8.0f * (float)q)) * 0.5f);
    while (b * (b - 1) / 2 > q)
        --b;
    while ((b + 1) * b / 2 <= q)
        ++b;
    a = q - b * (b - 1) / 2;
}

// The triplets of the nf frames of a slab.  A block walks the tiles T = blockIdx.x, blockIdx.x + gridDim.x, ... of
// n_tiles = nf * c_tiles: frame T / c_tiles, centres (T % c_tiles) * ANG_CTILE onwards.  inner: the n_bins - 1 inner
// thresholds t[1] ... t[n_bins - 1] in HBM.  LDS_HIST: P * n_bins <= ANG_HIST_WORDS and n_bins <= ANG_LDS_BINS.
// counts: uint64 [P][n_bins]; degenerate: uint64 [P]; coordination: uint64 [G][max_nb + 1].
template <bool ALL, bool LDS_HIST>
__global__ __launch_bounds__(ANG_THREADS) void ang_triplet_kernel(
    const float *__restrict__ slab, int n_rows, int n0, int off, int64_t n_tiles, int c_tiles, PairBox box, int keep,
    AngGroups groups, int G, int max_nb, const int *__restrict__ len, const int *__restrict__ list,
    const double *__restrict__ inner, int n_bins, unsigned long long *__restrict__ counts,
    unsigned long long *__restrict__ degenerate, unsigned long long *__restrict__ coordination)
{
    __shared__ double ent_w[3][ANG_ENTRIES];                // w_ij of entry (centre c, slot s) at c * 64 + s
    __shared__ double centre[3][ANG_CTILE];
    __shared__ double lds_inner[LDS_HIST ? ANG_LDS_BINS : 1];
    __shared__ unsigned int hist[LDS_HIST ? ANG_WAVES * ANG_HIST_WORDS : 1];
    __shared__ unsigned int coord[ANG_MAX_SPECIES * (ANG_MAX_NEIGHBORS + 1)];
    __shared__ unsigned int degen[ANG_MAX_PAIRS];
    __shared__ unsigned char ent_species[ANG_ENTRIES];
    __shared__ int row_len[ANG_CTILE], first_item[ANG_CTILE + 1], longest;
    const int t = threadIdx.x;
    const int P = G * (G + 1) / 2;
    const int words = P * n_bins;
    if (LDS_HIST) {
        for (int w = t; w < ANG_WAVES * words; w += ANG_THREADS)
            hist[(w / words) * ANG_HIST_WORDS + w % words] = 0u;
        for (int m = t; m < n_bins - 1; m += ANG_THREADS)
            lds_inner[m] = inner[m];
    }
    for (int w = t; w < G * (max_nb + 1); w += ANG_THREADS)
        coord[w] = 0u;
    if (t < ANG_MAX_PAIRS)
        degen[t] = 0u;
    const double *__restrict__ thr = LDS_HIST ? lds_inner : inner;
    unsigned int *__restrict__ my_hist = hist + (LDS_HIST ? (t >> 6) * ANG_HIST_WORDS : 0);

    for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        const int64_t fs = T / c_tiles;
        const int c0 = (int)(T - fs * c_tiles) * ANG_CTILE;
        const float *__restrict__ frame = slab + fs * 3 * n_rows;
        __syncthreads();                    // the tile before is counted (and the counters are zero)
        if (t == 0)
            longest = 0;
        if (t < ANG_CTILE) {
            const int i = c0 + t;
            int m = 0;
            if (i < n0) {
                m = len[fs * n0 + i];
                m = m > max_nb ? max_nb : m;
                centre[0][t] = (double)frame[i];
                centre[1][t] = (double)frame[n_rows + i];
                centre[2][t] = (double)frame[2 * int64_t(n_rows) + i];
            }
            row_len[t] = m;
        }
        __syncthreads();
        if (t < ANG_CTILE) {
            int before = 0;
            for (int c = 0; c < t; ++c)
                before += row_len[c] * (row_len[c] - 1) / 2;
            first_item[t] = before;
            if (t == ANG_CTILE - 1)
                first_item[ANG_CTILE] = before + row_len[t] * (row_len[t] - 1) / 2;
            atomicMax(&longest, row_len[t]);
        }
        __syncthreads();
        // entry e = (slot s, centre c), c fastest: a wave reads 16 consecutive words of four slots of the lists
        const int n_entries = longest * ANG_CTILE;
        for (int e = t; e < n_entries; e += ANG_THREADS) {
            const int c = e & (ANG_CTILE - 1), s = e / ANG_CTILE;
            if (s >= row_len[c])
                continue;
            const int j = list[(fs * max_nb + s) * n0 + c0 + c];
            const float *__restrict__ src = frame + off + j;
            const double dx = __dsub_rn((double)src[0], centre[0][c]), dy = __dsub_rn((double)src[n_rows], centre[1][c]),
                         dz = __dsub_rn((double)src[2 * int64_t(n_rows)], centre[2][c]);
            const int at = c * ANG_MAX_NEIGHBORS + s;
            ent_w[0][at] = ALL || keep & 1 ? min_image(dx, box.L[0], box.inv[0]) : 0.0;
            ent_w[1][at] = ALL || keep & 2 ? min_image(dy, box.L[1], box.inv[1]) : 0.0;
            ent_w[2][at] = ALL || keep & 4 ? min_image(dz, box.L[2], box.inv[2]) : 0.0;
            ent_species[at] = (unsigned char)ang_species(groups, j);
        }
        __syncthreads();
        if (t < ANG_CTILE && c0 + t < n0) {
            int of0 = 0, of1 = 0, of2 = 0, of3 = 0;     // the centre's neighbours of each species
            for (int s = 0; s < row_len[t]; ++s) {
                const int g = ent_species[t * ANG_MAX_NEIGHBORS + s];
                of0 += g == 0;
                of1 += g == 1;
                of2 += g == 2;
                of3 += g == 3;
            }
            atomicAdd(&coord[of0], 1u);
            if (G > 1)
                atomicAdd(&coord[(max_nb + 1) + of1], 1u);
            if (G > 2)
                atomicAdd(&coord[2 * (max_nb + 1) + of2], 1u);
            if (G > 3)
                atomicAdd(&coord[3 * (max_nb + 1) + of3], 1u);
        }
        const int n_items = first_item[ANG_CTILE];
        for (int item = t; item < n_items; item += ANG_THREADS) {
            int c = 0;
            for (int step = ANG_CTILE / 2; step > 0; step >>= 1)
                c += first_item[c + step] <= item ? step : 0;
            int sa, sb;
            ang_unrank(item - first_item[c], sa, sb);
            const int ea = c * ANG_MAX_NEIGHBORS + sa, eb = c * ANG_MAX_NEIGHBORS + sb;
            const double ax = ent_w[0][ea], ay = ent_w[1][ea], az = ent_w[2][ea];
            const double bx = ent_w[0][eb], by = ent_w[1][eb], bz = ent_w[2][eb];
            const double dot = __dadd_rn(__dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)), __dmul_rn(az, bz));
            const double cosine = __ddiv_rn(dot, __dsqrt_rn(__dmul_rn(r2_of(ax, ay, az), r2_of(bx, by, bz))));
            const int p = ang_pair(ent_species[ea], ent_species[eb], G);
            if (cosine != cosine) {
                atomicAdd(&degen[p], 1u);
                continue;
            }
            int lo = 0, hi = n_bins - 1;        // the inner thresholds that are >= cosine: a prefix, t decreases
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cosine <= thr[mid])
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (LDS_HIST)
                atomicAdd(&my_hist[p * n_bins + lo], 1u);
            else
                atomicAdd(&counts[int64_t(p) * n_bins + lo], 1ull);
        }
    }
    __syncthreads();
    if (LDS_HIST)
        for (int w = t; w < words; w += ANG_THREADS) {
            unsigned int sum = 0u;
            for (int v = 0; v < ANG_WAVES; ++v)
                sum += hist[v * ANG_HIST_WORDS + w];
            if (sum)
                atomicAdd(&counts[w], (unsigned long long)sum);
        }
    for (int w = t; w < G * (max_nb + 1); w += ANG_THREADS)
        if (coord[w])
            atomicAdd(&coordination[w], (unsigned long long)coord[w]);
    if (t < P && degen[t])
        atomicAdd(&degenerate[t], (unsigned long long)degen[t]);
}

}  // namespace mdx_ang_dev
