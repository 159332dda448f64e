// mdx_pairs_host.hpp — the host side that goes with mdx_pairs_device.hpp: the box and cutoff checks of the pair
// engines, the launch of the gather, and the capped lists with the word that refuses an overflowing row.
#pragma once

#include "mdx_frame_feed.hpp"
#include "mdx_pairs_device.hpp"

#include <cmath>

namespace mdx {

using mdx_pairs_dev::PairBox;

// dims positive and finite, and the largest cutoff within half the shortest kept box length (beyond it the minimum
// image is not the nearest image).  *keep: bit c set -> component c takes part; box->inv = 1.0 / L in float64.
// too_far: the message of an engine whose reach is no cutoff, with the reach and the shortest length as %g.
inline int check_box_cutoff(const double *dims, int zero_dims, double largest_cutoff, PairBox *box, int *keep,
                            const char *too_far = "cutoff %g reaches beyond half the shortest box length %g")
{
    for (int c = 0; c < 3; ++c)
        MDX_REQUIRE(dims[c] > 0.0 && std::isfinite(dims[c]), "dims[%d] must be positive and finite", c);
    double shortest = HUGE_VAL;
    for (int c = 0; c < 3; ++c)
        if (!(zero_dims >> c & 1))
            shortest = std::min(shortest, dims[c]);
    MDX_REQUIRE(largest_cutoff <= shortest / 2, too_far, largest_cutoff, shortest);
    *keep = 7 & ~zero_dims;
    for (int c = 0; c < 3; ++c) {
        box->L[c] = dims[c];
        box->inv[c] = 1.0 / dims[c];
    }
    return MDX_OK;
}

// frames of a default slab: what `bytes` of HBM hold of frames of frame_bytes each, at most PAIR_SLAB_MAX
inline int64_t pair_slab_frames(int64_t slab_frames, int64_t bytes, int64_t frame_bytes)
{
    if (slab_frames > 0)
        return slab_frames;
    return std::min(mdx_pairs_dev::PAIR_SLAB_MAX, std::max<int64_t>(1, bytes / frame_bytes));
}

// gather_kernel for nf frames of n rows: out slot f, or with RING slot (f0 + f) % cap
template <bool RING, typename Hook = mdx_pairs_dev::NoPointHook>
inline void launch_gather(hipStream_t stream, const float *pos, int64_t src_rows, const int *d_index, int n, int64_t nf,
                          float *out, int64_t f0 = 0, int64_t cap = 1, Hook hook = Hook())
{
    hipLaunchKernelGGL((mdx_pairs_dev::gather_kernel<RING, Hook>), dim3((unsigned)ceil_div(3 * int64_t(n), 256),
                       (unsigned)nf), dim3(256), 0, stream, pos, src_rows, d_index, n, f0, cap, out, hook);
}

// The capped per-row lists of the list engines: len int32 [frames][rows], list int32 [frames][max_nb][rows], and the
// control words in HBM, the first of which is the largest row seen (block_tally's atomicMax); an engine may keep
// further int32 words behind it (ctl_words).
struct CappedLists {
    DeviceBuffer d_len, d_list, d_ctl;
    int max_nb = 32, ctl_words = 1;
    int max_row = 0;                    // the largest row seen, as of the last look

    int ensure_ctl() { return d_ctl.ensure(size_t(4) * ctl_words); }

    int ensure(int64_t rows, int64_t frames)
    {
        MDX_TRY(d_len.ensure(size_t(4) * rows * frames));
        return d_list.ensure(size_t(4) * max_nb * rows * frames);
    }

    // the control words start over
    int zero(hipStream_t stream)
    {
        MDX_HIP(hipMemsetAsync(d_ctl.ptr, 0, size_t(4) * ctl_words, stream));
        max_row = 0;
        return MDX_OK;
    }

    // with the stream idle: the largest row seen, without judging it
    int look()
    {
        int32_t row = 0;
        MDX_HIP(hipMemcpy(&row, d_ctl.ptr, 4, hipMemcpyDeviceToHost));
        max_row = row;
        return MDX_OK;
    }

    // With the stream idle: the largest row seen; a row beyond the cap refuses the results until a reset.
    int check(const char *noun_row, const char *noun_item)
    {
        MDX_TRY(look());
        MDX_REQUIRE(max_row <= max_nb,
                    "a %s held %d %s in one frame, more than max_neighbors = %d: raise max_neighbors or lower the "
                    "cutoff (reset starts over)", noun_row, max_row, noun_item, max_nb);
        return MDX_OK;
    }
};

}  // namespace mdx
