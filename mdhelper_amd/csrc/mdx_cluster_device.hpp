// mdx_cluster_device.hpp — device side of the cluster engine (mdx_cluster.hip).
//
// Result contract.
//
// Nodes.  The n incoming rows of a frame are the atoms of group 0, then group 1, and so on; species[i] in 0 ... G-1 is
// the group of row i, 1 <= G <= 8.
//
// Box and pair arithmetic: those of mdx_residence_device.hpp.  One constant orthorhombic box, lengths L_c;
// inv_c = 1.0 / L_c is formed once on the host in float64.  Everything is float64, one operation at a time (the unit
// is built with contraction off); float32 coordinates are widened before any arithmetic.  For rows i != j of frame f:
//
//     d_c = x_jc(f) - x_ic(f) ;  s = d_c * inv_c ;  w_c = d_c - L_c * rint(s)       (rint: ties to even, as numpy.rint;
//                                                                                   w_c = +0.0 for a dropped component)
//     r2  = (w_x*w_x + w_y*w_y) + w_z*w_z
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
// Capped lists.  A row holds at most max_neighbors (1 ... 64) bonds in one frame, both directions counted (every bond
// is in the rows of both its ends).  A row that would hold more is an error, never a silent truncation: the contact
// kernel stores only into the row's max_neighbors slots but keeps counting, the largest row seen is kept in HBM, and
// the host refuses to hand out results (MDX_ERR_INVALID_VALUE, naming max_neighbors and the largest row) from the
// next synchronize / result on until a reset.  The slab that holds such a row is not labelled.
//
// The bonds are a function of the frame alone, the labels a function of the bonds alone, and every tally is an integer
// add or max (atomics on integers commute): the numbers are the same whatever the input route, the split into calls
// or slabs, the grid, or the arrival order of the atomics.
//
// evaluations is the contract's count F * n * (n - 1) / 2.
//
// Shape.  Three phases per slab of frames; a frame never needs another, so there is no history.
//
// Phase 1, contact lists (the hot path, F * n * (n - 1) ordered evaluations).  clu_prepare_kernel gathers the rows of
// a slab component-major float32, sets label[f][i] = i and size[f][i] = 0.  clu_contact_kernel has the shape of
// prs_contact_kernel: grid x = i tiles x j chunks, z = frames; a block holds CLU_TILE rows in registers, one per
// lane, widened, and walks its chunk of at most CLU_JCHUNK partners in stages of CLU_STAGE through LDS (widened once
// when staged; every lane reads the same j at once, a broadcast).  The species of a staged partner lies beside its
// coordinates in LDS, and the lane picks rc2 from the table in LDS at [species_j][species_i]: one row of 8 doubles per
// partner, so the lanes of a wave read at most 8 neighbouring words.  Rows arrive group by group, so the partners of
// nearly every stage are of one species: the block finds that out while it stages (one barrier with a vote), the lane
// then takes its bound once for the stage, and only a stage that spans two groups looks it up pair by pair.  UNIFORM
// (one species, or a table whose entries are all one positive value): rc2 is a kernel argument and neither species
// nor table is touched.  Ordered pairs are evaluated, so that a row is filled by its own lane: a bond takes
// slot = atomicAdd(&len[f][i], 1) and is stored at list[f][slot][i] when slot < max_neighbors (slot-major: the
// labelling's lanes read consecutive i).  Each block adds its ordered bonds to the frame's count with one integer
// atomic (bonds[f] is half of that count) and its largest row to max_row with one atomicMax.
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

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mdx_clu_dev {

constexpr int CLU_TILE = 256;                 // rows per block, one per lane
constexpr int CLU_THREADS = CLU_TILE;
constexpr int CLU_STAGE = CLU_THREADS;        // partners per LDS stage, one staged per thread
constexpr int CLU_JCHUNK = 4 * CLU_STAGE;     // partners per block
constexpr int CLU_MAX_NEIGHBORS = 64;         // slots of a row at most
constexpr int CLU_MAX_SPECIES = 8;
constexpr int64_t CLU_SLAB_MAX = 32768;       // frames per launch, at most (grid y / z)
constexpr int CLU_ROW_THREADS = 256;          // threads of the per-row kernels (sweep, size, tally)
constexpr int CLU_FRAME_WORDS = 4;            // uint64 per frame: ordered bonds, n_clusters, largest, sum_squares

// Row index[p] (or p) of n_frames float32 frames of src_rows rows into the slab: slab[(f * 3 + c) * n + p].  One
// thread per coordinate (t = c * n + p: a wave writes consecutive floats); grid y = frames.  The threads of component
// 0 also start the labels (label[f][p] = p) and zero the sizes.
__global__ __launch_bounds__(256) void clu_prepare_kernel(const float *__restrict__ pos, int64_t src_rows,
                                                          const int *__restrict__ index, int n,
                                                          float *__restrict__ slab, int *__restrict__ label,
                                                          int *__restrict__ size)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 3 * n)
        return;
    const int c = t / n, p = t - c * n;
    const int64_t r = index ? index[p] : p;
    const int64_t f = blockIdx.y;
    slab[(f * 3 + c) * n + p] = pos[(f * src_rows + r) * 3 + c];
    if (c == 0) {
        label[f * n + p] = p;
        size[f * n + p] = 0;
    }
}

struct CluBox {
    double L[3], inv[3];
};

// w = d - L * rint(d * inv), one operation at a time
__device__ __forceinline__ double clu_min_image(double d, double L, double inv)
{
    return __dsub_rn(d, __dmul_rn(L, rint(__dmul_rn(d, inv))));
}

// The staged partners js ... js + nj - 1 against this lane's row (xi, yi, zi).  LOOKUP: the bound of a pair is
// table[8 * species_j + my_species] from LDS; else it is `bound` for every partner of the stage.
template <bool ALL, bool LOOKUP>
__device__ __forceinline__ void clu_stage_pairs(const double *__restrict__ stage,
                                                const int *__restrict__ stage_species,
                                                const double *__restrict__ lds_table, int my_species, double bound,
                                                int nj, int js, int skip, double xi, double yi, double zi,
                                                const CluBox &box, int keep, int n, int max_nb,
                                                int *__restrict__ my_len, int *__restrict__ my_list,
                                                unsigned int &found, unsigned int &row)
{
#pragma unroll 4
    for (int jj = 0; jj < nj; ++jj) {
        const double dx = __dsub_rn(stage[4 * jj + 0], xi), dy = __dsub_rn(stage[4 * jj + 1], yi),
                     dz = __dsub_rn(stage[4 * jj + 2], zi);
        const double wx = ALL || keep & 1 ? clu_min_image(dx, box.L[0], box.inv[0]) : 0.0;
        const double wy = ALL || keep & 2 ? clu_min_image(dy, box.L[1], box.inv[1]) : 0.0;
        const double wz = ALL || keep & 4 ? clu_min_image(dz, box.L[2], box.inv[2]) : 0.0;
        const double r2 = __dadd_rn(__dadd_rn(__dmul_rn(wx, wx), __dmul_rn(wy, wy)), __dmul_rn(wz, wz));
        const double rc2 = LOOKUP ? lds_table[CLU_MAX_SPECIES * stage_species[jj] + my_species] : bound;
        if (r2 <= rc2 && jj != skip) {
            const int slot = atomicAdd(my_len, 1);          // other j chunks append to the same row
            if (slot < max_nb)
                my_list[int64_t(slot) * n] = js + jj;
            ++found;
            row = (unsigned int)slot + 1u > row ? (unsigned int)slot + 1u : row;
        }
    }
}

// The bonds of frame f_lo + blockIdx.z among the n rows of slab frame blockIdx.z.  keep: bit c set -> component c
// takes part; ALL: keep == 7, known when compiled.  UNIFORM: every pair of species bonds within rc2; else
// table[8 * b + a] is rc2 of species a and b (-1.0: no bond) and species holds the n rows' species.  A stage whose
// partners are all of one species (rows arrive group by group, so nearly every stage is) takes the lane's bound from
// the table once; only a stage that spans two groups looks the bound up pair by pair.  len: int32 [slab][n], zero;
// list: int32 [slab][max_nb][n]; frames: uint64 [F][CLU_FRAME_WORDS].
template <bool ALL, bool UNIFORM>
__global__ __launch_bounds__(CLU_THREADS) void clu_contact_kernel(
    const float *__restrict__ slab, int n, int n_jchunks, int64_t f_lo, CluBox box, int keep, double rc2,
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
            const float *__restrict__ src = b + js + threadIdx.x;
            stage[4 * threadIdx.x + 0] = (double)src[0];
            stage[4 * threadIdx.x + 1] = (double)src[n];
            stage[4 * threadIdx.x + 2] = (double)src[2 * int64_t(n)];
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
        if (UNIFORM || !mixed) {
            const double bound = UNIFORM ? rc2 : lds_table[CLU_MAX_SPECIES * stage_species[0] + my_species];
            clu_stage_pairs<ALL, false>(stage, stage_species, lds_table, my_species, bound, nj, js, skip, xi, yi, zi,
                                        box, keep, n, max_nb, my_len, my_list, found, row);
        } else {
            clu_stage_pairs<ALL, true>(stage, stage_species, lds_table, my_species, 0.0, nj, js, skip, xi, yi, zi, box,
                                       keep, n, max_nb, my_len, my_list, found, row);
        }
    }
    // one integer atomic per block for the frame's ordered bonds, one for the largest row: integer adds and max commute
    for (int off = 32; off > 0; off >>= 1) {
        found += __shfl_down(found, off);
        const unsigned int other = __shfl_down(row, off);
        row = other > row ? other : row;
    }
    if ((threadIdx.x & 63) == 0 && (found | row)) {
        atomicAdd(&block_found, found);
        atomicMax(&block_row, row);
    }
    __syncthreads();
    if (threadIdx.x == 0 && block_found) {
        atomicAdd(&frames[(f_lo + fs) * CLU_FRAME_WORDS], (unsigned long long)block_found);
        atomicMax(max_row, (int)block_row);
    }
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
