// mdx_cluster_device.hpp — device side of the cluster engine (mdx_cluster.hip).
//
// Result contract.
//
// Nodes.  The n incoming rows of a frame are the atoms of group 0, then group 1, and so on; species[i] in 0 ... G-1 is
// the group of row i, 1 <= G <= 8.
//
// Box and pair arithmetic: those of mdx_pairs_device.hpp, for rows i != j of frame f.
//
// Bond rule.  cutoff is a symmetric G x G table of non-negative finite values, at least one of them positive.
// rc2[a][b] = cutoff[a][b] * cutoff[a][b], formed once on the host in float64, where the entry is positive, and -1.0
// where it is 0: that pair of species never bonds, not even at distance 0.  Rows i != j are bonded in frame f iff
// r2 <= rc2[species[i]][species[j]].  A NaN r2 is never a bond (the comparison fails); no square root is taken.  Every
// operation above gives the same r2 for (i, j) and (j, i) (d changes sign, rint is odd), so the bonds are symmetric.
//
// Labels.  label[f][i] is the smallest row index in the connected component of i in the bond graph of frame f.
//
// Results, all integers (uint64 in HBM, handed out as int64).  Per frame f:
//     bonds[f]        the unordered bonded pairs
//     n_clusters[f]   the connected components
//     largest[f]      the rows of the largest component
//     sum_squares[f]  the sum over the components of size * size
// and summed over the frames seen:
//     size_counts[s],       s = 0 ... n: components of s rows (entry 0 stays 0)
//     species_counts[g][s]: rows of species g that sit in a component of s rows, so that
//                           sum_g species_counts[g][s] == s * size_counts[s]
// With keep_labels the engine also hands out label, int32 [F][n].
//
// Capped lists (mdx_pairs_device.hpp).  A row holds at most max_neighbors (1 ... 64) bonds in one frame, both
// directions counted (every bond is in the rows of both its ends); a row that would hold more refuses the results
// (MDX_ERR_INVALID_VALUE, naming max_neighbors and the largest row).  The slab that holds such a row is not labelled.
//
// The bonds are a function of the frame alone, the labels a function of the bonds alone, and every tally is an integer
// add or max (atomics on integers commute): the numbers are the same whatever the input route, the split into calls
// or slabs, the grid, or the arrival order of the atomics.
//
// evaluations is the contract's count F * n * (n - 1) / 2.
//
// Shape.  Three phases per slab of frames; a frame never needs another, so there is no history.
//
// Phase 1, contact lists (the hot path, F * n * (n - 1) ordered evaluations).  gather_kernel gathers the rows of a
// slab component-major float32 and, through CluStart, sets label[f][i] = i and size[f][i] = 0.  clu_contact_kernel is
// the walk of mdx_pairs_device.hpp with z = frames and CLU_JCHUNK partners per block.  The species of a staged
// partner lies beside its coordinates in LDS, and the lane picks rc2 from the table in LDS at [species_j][species_i]:
// one row of 8 doubles per partner, so the lanes of a wave read at most 8 neighbouring words.  Rows arrive group by
// group, so the partners of nearly every stage are of one species: the block finds that out while it stages (one
// barrier with a vote), the lane then takes its bound once for the stage, and only a stage that spans two groups
// looks it up pair by pair.  UNIFORM (one species, or a table whose entries are all one positive value): rc2 is a
// kernel argument and neither species nor table is touched.  Ordered pairs are evaluated, so that a row is filled by
// its own lane: a bond takes slot = atomicAdd(&len[f][i], 1) and is stored at list[f][slot][i] when
// slot < max_neighbors (slot-major: the labelling's lanes read consecutive i).  Each block adds its ordered bonds to
// the frame's count with one integer atomic (bonds[f] is half of that count) and its largest row to max_row with one
// atomicMax.
//
// Phase 2, labelling, from the lists only: in place, hooking plus pointer jumping.  A sweep (clu_sweep_kernel, one
// thread per (frame, row i)) reads li = label[i], takes m = min(li, label[j] over the row's list), jumps once,
// m = label[m], and where m < li lowers both label[i] and label[li] to m with atomicMin.  A sweep records "lowered"
// with an integer atomic, where an atomicMin returned a value above m, into a word that the host reads after a few
// sweeps; a slab is finished when a whole sweep lowered nothing.
//   Why in place: labels only ever decrease and atomicMin is performed at the memory side, so the final value of a
//   word does not depend on which workgroup's store another one saw.  Plain loads may be stale within a launch (the
//   L2s of the XCDs are not coherent for them); a stale label is an older label of the same word, hence larger and
//   still a row of the same component: it costs at most an extra sweep, never a wrong answer.  No wave waits on
//   another one.
//   Invariants: label[i] <= i, and label[i] is a row of i's component (m is always a label of a row of the component,
//   and li is one).
//   Fixed point: the sweep that lowered nothing launched no store that changed a word, so all its loads saw the words
//   as they were before its launch, which a kernel boundary makes visible.  Then label[i] <= label[j] for every bond,
//   and since every bond is in both rows, label is one value c on a component.  The smallest row i0 of the component
//   has label[i0] <= i0 inside the component, so label[i0] = i0 and c = i0.
//   Termination: every load returns at most the word's value at the launch of its sweep.  By induction, after sweep k
//   label[i] is at most the smallest row within k bonds of i; a component's diameter is at most n - 1, so sweep n at
//   the latest lowers nothing.  The host caps the sweeps of a slab at n + 1 and reports MDX_ERR_INTERNAL beyond.
//
// Phase 3, tallies, all integer atomics.  clu_size_kernel: size[f][label[i]] += 1.  clu_tally_kernel: per row,
// species_counts[species[i]][size[label[i]]] += 1; per root (label[i] == i), size_counts[s] += 1 and the frame's
// n_clusters, largest and sum_squares.  Free ions make size 1 the hot destination, and a percolating cluster makes
// one word per frame hot: size 1 and the per-frame numbers are summed in LDS per block, and a wave whose lanes share
// the destination of its first lane adds once for all of them.
//
// No cell list and no spatial culling: every ordered pair is evaluated.  Walking only the upper triangle of tile
// pairs, a labelling in LDS for small n and culling by cells are follow-ups.
#pragma once

#include "mdx_pairs_device.hpp"

namespace mdx_clu_dev {

using namespace mdx_pairs_dev;

constexpr int CLU_TILE = PAIR_TILE;           // rows per block, one per lane
constexpr int CLU_THREADS = PAIR_THREADS;
constexpr int CLU_STAGE = PAIR_STAGE;         // partners per LDS stage, one staged per thread
constexpr int CLU_JCHUNK = 4 * CLU_STAGE;     // partners per block
constexpr int CLU_MAX_NEIGHBORS = PAIR_MAX_NEIGHBORS;   // slots of a row at most
constexpr int CLU_MAX_SPECIES = 8;
constexpr int64_t CLU_SLAB_MAX = PAIR_SLAB_MAX;         // frames per launch, at most (grid y / z)
constexpr int CLU_ROW_THREADS = 256;          // threads of the per-row kernels (sweep, size, tally)
constexpr int CLU_FRAME_WORDS = 4;            // uint64 per frame: ordered bonds, n_clusters, largest, sum_squares

// what gather_kernel does per row beyond the gather: the labels start (label[f][p] = p) and the sizes are zero
struct CluStart {
    int *__restrict__ label, *__restrict__ size;
    __device__ __forceinline__ void operator()(int64_t f, int p, int n) const
    {
        label[f * n + p] = p;
        size[f * n + p] = 0;
    }
};

// The bonds of frame f_lo + blockIdx.z among the n rows of slab frame blockIdx.z.  keep: bit c set -> component c
// takes part; ALL: keep == 7, known when compiled.  UNIFORM: every pair of species bonds within rc2; else
// table[8 * b + a] is rc2 of species a and b (-1.0: no bond) and species holds the n rows' species.  A stage whose
// partners are all of one species (rows arrive group by group, so nearly every stage is) takes the lane's bound from
// the table once; only a stage that spans two groups looks the bound up pair by pair.  len: int32 [slab][n], zero;
// list: int32 [slab][max_nb][n]; frames: uint64 [F][CLU_FRAME_WORDS].
template <bool ALL, bool UNIFORM>
__global__ __launch_bounds__(CLU_THREADS) void clu_contact_kernel(
    const float *__restrict__ slab, int n, int n_jchunks, int64_t f_lo, PairBox box, int keep, double rc2,
    const double *__restrict__ table, const int *__restrict__ species, int max_nb, int *__restrict__ len,
    int *__restrict__ list, unsigned long long *__restrict__ frames, int *__restrict__ max_row)
{
    __shared__ __attribute__((aligned(16))) double stage[4 * CLU_STAGE];
    __shared__ int stage_species[CLU_STAGE];
    __shared__ double lds_table[CLU_MAX_SPECIES * CLU_MAX_SPECIES];
    __shared__ unsigned int block_found, block_row;
    const int64_t fs = blockIdx.z;
    const int tile = blockIdx.x / n_jchunks, chunk = blockIdx.x - tile * n_jchunks;
    const int i = tile * CLU_TILE + threadIdx.x;
    const bool live = i < n;
    const float *__restrict__ b = slab + fs * 3 * n;
    const float *__restrict__ a = b + (live ? i : n - 1);
    const double xi = (double)a[0], yi = (double)a[n], zi = (double)a[2 * int64_t(n)];
    int *__restrict__ my_len = len + fs * n + (live ? i : 0);
    int *__restrict__ my_list = list + fs * max_nb * n + (live ? i : 0);
    int my_species = 0;
    if (!UNIFORM) {
        my_species = species[live ? i : n - 1];
        if (threadIdx.x < CLU_MAX_SPECIES * CLU_MAX_SPECIES)
            lds_table[threadIdx.x] = table[threadIdx.x];
    }
    if (threadIdx.x == 0) {
        block_found = 0u;
        block_row = 0u;
    }
    __syncthreads();
    unsigned int found = 0u, row = 0u;
    const int j_begin = chunk * CLU_JCHUNK;
    const int j_end = n - j_begin < CLU_JCHUNK ? n : j_begin + CLU_JCHUNK;
    for (int js = j_begin; js < j_end; js += CLU_STAGE) {
        const int nj = j_end - js < CLU_STAGE ? j_end - js : CLU_STAGE;
        __syncthreads();                    // the stage is free
        int mixed = 0;                      // a partner of another species than the stage's first
        if ((int)threadIdx.x < nj) {
            stage_partners(stage, b, n, js);
            if (!UNIFORM) {
                const int sj = species[js + threadIdx.x];
                stage_species[threadIdx.x] = sj;
                mixed = sj != species[js];
            }
        }
        if (UNIFORM)
            __syncthreads();
        else
            mixed = __syncthreads_or(mixed);
        if (!live)
            continue;
        const int skip = i - js;            // the stage entry that is this lane's own row
        const auto bond = [&](int j) {
            append_capped(my_len, my_list, n, max_nb, j, row);
            ++found;
        };
        if (UNIFORM || !mixed) {
            const double bound = UNIFORM ? rc2 : lds_table[CLU_MAX_SPECIES * stage_species[0] + my_species];
            stage_pairs<ALL>(stage, nj, js, skip, xi, yi, zi, box, keep,
                             [&](int, int j, double, double, double, double r2, bool other) {
                                 if (r2 <= bound && other)
                                     bond(j);
                             });
        } else {
            stage_pairs<ALL>(stage, nj, js, skip, xi, yi, zi, box, keep,
                             [&](int jj, int j, double, double, double, double r2, bool other) {
                                 if (r2 <= lds_table[CLU_MAX_SPECIES * stage_species[jj] + my_species] && other)
                                     bond(j);
                             });
        }
    }
    block_tally<true>(found, row, &block_found, &block_row, &frames[(f_lo + fs) * CLU_FRAME_WORDS], max_row);
}

// One labelling sweep over the slab: grid x = row tiles, y = frames.  label: int32 [slab][n]; *lowered becomes 1 where
// an atomicMin lowered a word.  Rows are read up to max_nb entries (an overflowing row: the host refuses the results).
__global__ __launch_bounds__(CLU_ROW_THREADS) void clu_sweep_kernel(int n, int max_nb, const int *__restrict__ len,
                                                                    const int *__restrict__ list, int *label,
                                                                    int *__restrict__ lowered)
{
    const int i = blockIdx.x * CLU_ROW_THREADS + threadIdx.x;
    const int64_t f = blockIdx.y;
    bool low = false;
    if (i < n) {
        int *lab = label + f * n;
        const int li = lab[i];
        int m = li;
        int count = len[f * n + i];
        count = count > max_nb ? max_nb : count;
        const int *__restrict__ row = list + f * max_nb * n + i;
        for (int t = 0; t < count; ++t) {
            const int lj = lab[row[int64_t(t) * n]];
            m = lj < m ? lj : m;
        }
        m = lab[m];                         // one jump: label[m] <= m
        if (m < li) {
            low = atomicMin(&lab[i], m) > m;
            low |= atomicMin(&lab[li], m) > m;      // hooking: the row i pointed at follows
        }
    }
    if (__any(low) && (threadIdx.x & 63) == 0)
        atomicOr(lowered, 1);
}

// Adds 1 to *(base + key) for every lane whose key is not negative: the lanes that share the key of the wave's first
// lane add once for all of them.  Every lane of the wave calls it (a wave's dead lanes are its last ones, key < 0).
template <typename T>
__device__ __forceinline__ void clu_wave_count(T *base, int64_t key)
{
    const int lo = __builtin_amdgcn_readfirstlane((int)(key & 0xffffffff));
    const int hi = __builtin_amdgcn_readfirstlane((int)(key >> 32));
    const int64_t lead = (int64_t(hi) << 32) | (unsigned int)lo;
    const unsigned long long same = __ballot(key == lead);
    if (key == lead) {
        if ((threadIdx.x & 63) == 0 && key >= 0)
            atomicAdd(base + key, (T)__popcll(same));
    } else if (key >= 0) {
        atomicAdd(base + key, (T)1);
    }
}

// size[f][label[f][i]] += 1; grid x = row tiles, y = frames
__global__ __launch_bounds__(CLU_ROW_THREADS) void clu_size_kernel(int n, const int *__restrict__ label,
                                                                   int *__restrict__ size)
{
    const int i = blockIdx.x * CLU_ROW_THREADS + threadIdx.x;
    const int64_t f = blockIdx.y;
    const int64_t key = i < n ? label[f * n + i] : -1;
    clu_wave_count(size + f * n, key);
}

// The tallies of frame f_lo + blockIdx.y.  size_counts: uint64 [n + 1]; species_counts: uint64 [G][n + 1]; frames:
// uint64 [F][CLU_FRAME_WORDS].
__global__ __launch_bounds__(CLU_ROW_THREADS) void clu_tally_kernel(
    int n, int64_t f_lo, const int *__restrict__ label, const int *__restrict__ size,
    const int *__restrict__ species, unsigned long long *__restrict__ size_counts,
    unsigned long long *__restrict__ species_counts, unsigned long long *__restrict__ frames)
{
    __shared__ unsigned int free_rows[CLU_MAX_SPECIES];     // rows of each species in a cluster of one
    __shared__ unsigned int block_roots, block_largest;
    __shared__ unsigned long long block_squares;
    if (threadIdx.x < CLU_MAX_SPECIES)
        free_rows[threadIdx.x] = 0u;
    if (threadIdx.x == 0) {
        block_roots = 0u;
        block_largest = 0u;
        block_squares = 0ull;
    }
    __syncthreads();
    const int i = blockIdx.x * CLU_ROW_THREADS + threadIdx.x;
    const int64_t f = blockIdx.y;
    const bool live = i < n;
    int root = -1, s = 0, g = 0;
    if (live) {
        root = label[f * n + i];
        s = size[f * n + root];
        g = species[i];
    }
    if (live && s == 1)
        atomicAdd(&free_rows[g], 1u);
    clu_wave_count(species_counts, live && s != 1 ? int64_t(g) * (int64_t(n) + 1) + s : int64_t(-1));
    const bool is_root = live && root == i;
    clu_wave_count(size_counts, is_root && s != 1 ? int64_t(s) : int64_t(-1));
    unsigned int roots = is_root ? 1u : 0u, largest = is_root ? (unsigned int)s : 0u;
    unsigned long long squares = is_root ? (unsigned long long)s * (unsigned long long)s : 0ull;
    for (int off = 32; off > 0; off >>= 1) {
        roots += __shfl_down(roots, off);
        squares += __shfl_down(squares, off);
        const unsigned int other = __shfl_down(largest, off);
        largest = other > largest ? other : largest;
    }
    if ((threadIdx.x & 63) == 0 && roots) {
        atomicAdd(&block_roots, roots);
        atomicMax(&block_largest, largest);
        atomicAdd(&block_squares, squares);
    }
    __syncthreads();
    unsigned long long *__restrict__ frame = frames + (f_lo + f) * CLU_FRAME_WORDS;
    if (threadIdx.x == 0 && block_roots) {
        atomicAdd(&frame[1], (unsigned long long)block_roots);
        atomicMax(&frame[2], (unsigned long long)block_largest);
        atomicAdd(&frame[3], block_squares);
    }
    if (threadIdx.x < CLU_MAX_SPECIES && free_rows[threadIdx.x]) {
        const unsigned long long count = free_rows[threadIdx.x];
        atomicAdd(&species_counts[threadIdx.x * (int64_t(n) + 1) + 1], count);
        atomicAdd(&size_counts[1], count);      // a cluster of one is its own root
    }
}

}  // namespace mdx_clu_dev
