// mdx_lag_history.hpp — what the lag engines (van Hove, chi4, orientation, distinct van Hove, residence, hydrogen
// bonds) share about time on the host side: the table of lags and its origin arithmetic, the sizing of a ring of
// max(lags) + slab frames, the unwrapped float64 history of van Hove and chi4, and the survival sums of residence
// and hydrogen bonds.  Small structs a handle holds as members, in the style of CappedLists.
//
// Host code only, and it names no kernel: a unit hands over the instantiations it launches (prepare, walk), so a unit
// that includes this header compiles no kernel it does not use, and chi4 can pass the vh_prepare_kernel of the
// namespace it includes the van Hove device header in.
#pragma once

#include "mdx_pairs_host.hpp"
#include "mdx_residence_device.hpp"     // PRS_WALK_ORIGINS, PRS_WALK_THREADS

#include <cmath>

namespace mdx {

struct LagTable {
    std::vector<int64_t> lags;
    int64_t max_lag = 0, origin_step = 1;       // origins are the multiples of origin_step
    DeviceBuffer d_lags;                        // int64 [n()]; in the handle's release list

    int n() const { return (int)lags.size(); }

    // The list of a create, which needs no device.  How many lags an engine takes, and in which words it says so, is
    // the engine's own line, as is its check of origin_step: they stand among its other scalar checks.
    static int check(int n_lags, const int64_t *list)
    {
        for (int k = 0; k < n_lags; ++k) {
            MDX_REQUIRE(list[k] >= 0, "lags must not be negative");
            MDX_REQUIRE(k == 0 || list[k] > list[k - 1], "lags must be strictly increasing");
        }
        return MDX_OK;
    }

    void assign(int n_lags, const int64_t *list, int64_t step = 1)
    {
        lags.assign(list, list + n_lags);
        max_lag = list[n_lags - 1];
        origin_step = step;
    }

    int upload()
    {
        MDX_TRY(d_lags.ensure(size_t(8) * n()));
        MDX_HIP(hipMemcpy(d_lags.ptr, lags.data(), size_t(8) * n(), hipMemcpyHostToDevice));
        return MDX_OK;
    }

    // the origins o with o + lag among the frames [f0, f0 + nf)
    int64_t origins_met(int64_t f0, int64_t nf, int64_t lag) const
    {
        const int64_t o_lo = std::max<int64_t>(0, f0 - lag), o_hi = f0 + nf - lag;      // origins [o_lo, o_hi)
        return o_hi > o_lo ? ceil_div(o_hi, origin_step) - ceil_div(o_lo, origin_step) : 0;
    }

    // the same over all lags: the contract's evaluations of a slab, per point, vector or pair
    int64_t origins_met(int64_t f0, int64_t nf) const
    {
        int64_t sum = 0;
        for (int64_t lag : lags)
            sum += origins_met(f0, nf, lag);
        return sum;
    }

    // the origins of a lag after frames_seen frames: the multiples of origin_step below frames_seen - lag
    int64_t origins_seen(int64_t frames_seen, int64_t lag) const { return origins_met(0, frames_seen, lag); }
};

// A ring of cap = max(lags) + slab frames in HBM, frame f in slot f % cap, so that a lag reaches back across slabs and
// calls.  The buffers are the engine's own.
struct LagRing {
    int64_t cap = 0, max_lag = 0;

    // Sizes the ring before the first frame of a pass and leaves it alone afterwards; frames of frame_bytes each,
    // refused above 2^40 bytes in the words of too_large (cap as %lld, then args).  Nothing is in flight before the
    // first frame (a reset waits for the stream), so the engine may then grow its buffers to cap (and slab) frames:
    // it asks for them after every call of this, which costs nothing once they have their size.
    template <typename... Args>
    int ensure(int64_t frames_seen, int64_t lag, int64_t slab, int64_t frame_bytes, const char *too_large, Args... args)
    {
        if (frames_seen > 0)
            return MDX_OK;
        const int64_t frames = planned_cap(frames_seen, lag, slab);
        MDX_REQUIRE(frames < (int64_t(1) << 40) / frame_bytes, too_large, (long long)frames, args...);
        cap = frames;
        max_lag = lag;
        return MDX_OK;
    }

    // the frames the ring holds once ensure has run with these arguments: the ring a pass already has, or before the
    // first frame of a pass a new one of lag + slab frames
    int64_t planned_cap(int64_t frames_seen, int64_t lag, int64_t slab) const
    {
        return frames_seen > 0 ? cap : lag + slab;
    }

    // frames per slab: no more than the ring was sized for
    int64_t slab(int64_t asked) const { return slab_within(asked, cap, max_lag); }

    static int64_t slab_within(int64_t asked, int64_t frames, int64_t lag) { return std::min(asked, frames - lag); }

    // The body of X_plan of a ring engine, asked = X_slab(h): what the next prepare and the loop after it use.  Needs
    // no device and sizes nothing.
    int plan(int64_t frames_seen, int64_t lag, int64_t asked, int64_t *slab_frames, int64_t *ring_frames) const
    {
        MDX_REQUIRE(slab_frames && ring_frames, "NULL argument");
        *ring_frames = planned_cap(frames_seen, lag, asked);
        *slab_frames = slab_within(asked, *ring_frames, lag);
        return MDX_OK;
    }

    // Empties the slots of frames [f_lo, f_lo + nf) of a ring of slot_bytes per frame: one range, or two where the
    // ring wraps.
    int zero_slots(void *ring, size_t slot_bytes, int64_t f_lo, int64_t nf, hipStream_t stream) const
    {
        const int64_t first = f_lo % cap, head = std::min(nf, cap - first);
        MDX_HIP(hipMemsetAsync(static_cast<char *>(ring) + slot_bytes * first, 0, slot_bytes * head, stream));
        if (nf > head)
            MDX_HIP(hipMemsetAsync(ring, 0, slot_bytes * (nf - head), stream));
        return MDX_OK;
    }
};

// The widened (and, with a box, unwrapped) points of van Hove and chi4: d_hist double [cap][3][n], written by
// vh_prepare_kernel; d_prev double [3][n] and d_image int [3][n] carry the unwrap state from frame to frame.
struct UnwrappedHistory {
    bool unwrap = false;
    double dims[3] = {0, 0, 0};
    DeviceBuffer d_hist, d_prev, d_image;       // in the handle's release list

    // the body of X_set_unwrap; box = NULL: the points are taken as they come
    int set_unwrap(const double *box, int64_t frames_seen, const char *entry_name)
    {
        if (box)
            for (int k = 0; k < 3; ++k)
                MDX_REQUIRE(box[k] > 0.0 && std::isfinite(box[k]), "dims[%d] must be positive and finite", k);
        MDX_REQUIRE(frames_seen == 0, "%s must be called before the first frame", entry_name);
        unwrap = box != nullptr;
        for (int k = 0; k < 3; ++k)
            dims[k] = box ? box[k] : 0.0;
        return MDX_OK;
    }

    int ensure_state(int64_t n)
    {
        MDX_TRY(d_prev.ensure(size_t(24) * n));
        return d_image.ensure(size_t(12) * n);
    }

    int ensure_ring(int64_t n, int64_t cap) { return d_hist.ensure(size_t(24) * n * cap); }

    // nf frames from f0 on into the ring: wrapped = vh_prepare_kernel<true>, which walks the frames in order in one
    // launch; plain = vh_prepare_kernel<false>, a block row per frame
    template <typename Kernel>
    void prepare(Kernel wrapped, Kernel plain, hipStream_t stream, const float *pos, int64_t src_rows,
                 const int *d_index, int n, int64_t nf, int64_t f0, int64_t cap)
    {
        if (unwrap)
            hipLaunchKernelGGL(wrapped, dim3((unsigned)ceil_div(3 * int64_t(n), 256)), dim3(256), 0, stream, pos,
                               src_rows, d_index, n, (int)nf, f0, cap, dims[0], dims[1], dims[2], f0 == 0 ? 1 : 0,
                               d_prev.as<double>(), d_image.as<int>(), d_hist.as<double>());
        else
            hipLaunchKernelGGL(plain, dim3((unsigned)ceil_div(3 * int64_t(n), 256), (unsigned)nf), dim3(256), 0,
                               stream, pos, src_rows, d_index, n, (int)nf, f0, cap, 0.0, 0.0, 0.0, 0,
                               (double *)nullptr, (int *)nullptr, d_hist.as<double>());
    }
};

// The survival sums of residence and hydrogen bonds over the rings of a CappedLists: d_sums uint64 [3][n_lags] =
// intermittent, continuous, origin_counts; d_mask uint64 [cap][rows], the slots of an origin's row still alive.
struct SurvivalWalk {
    bool continuous = true;
    DeviceBuffer d_sums, d_mask;                // in the handle's release list

    int ensure(int n_lags) { return d_sums.ensure(size_t(24) * n_lags); }

    int ensure_mask(int64_t rows, int64_t cap) { return continuous ? d_mask.ensure(size_t(8) * rows * cap) : MDX_OK; }

    int zero(int n_lags, hipStream_t stream)
    {
        MDX_HIP(hipMemsetAsync(d_sums.ptr, 0, size_t(24) * n_lags, stream));
        return MDX_OK;
    }

    // prs_walk_kernel (on = <true>, off = <false>) for the origins that meet the new frames [f_lo, f_lo + nf): the
    // multiples of origin_step in [f_lo - max_lag, f_lo + nf), PRS_WALK_ORIGINS of them per launch
    template <typename Kernel>
    void walk(Kernel on, Kernel off, hipStream_t stream, const LagTable &lags, const LagRing &ring,
              const CappedLists &lists, int rows, int64_t f_lo, int64_t nf)
    {
        using mdx_prs_dev::PRS_WALK_ORIGINS;
        using mdx_prs_dev::PRS_WALK_THREADS;
        const int64_t o_lo = ceil_div(std::max<int64_t>(0, f_lo - lags.max_lag), lags.origin_step);
        const int64_t o_hi = ceil_div(f_lo + nf, lags.origin_step);
        const int64_t tiles = ceil_div(rows, PRS_WALK_THREADS);
        for (int64_t o = o_lo; o < o_hi; o += PRS_WALK_ORIGINS) {
            const int64_t n_o = std::min<int64_t>(PRS_WALK_ORIGINS, o_hi - o);
            hipLaunchKernelGGL(continuous ? on : off, dim3((unsigned)tiles, (unsigned)n_o), dim3(PRS_WALK_THREADS), 0,
                               stream, ring.cap, rows, lists.max_nb, lists.d_len.as<int>(), lists.d_list.as<int>(),
                               d_mask.as<unsigned long long>(), lags.d_lags.as<int64_t>(), lags.n(), lags.max_lag, o,
                               lags.origin_step, f_lo, nf, d_sums.as<unsigned long long>());
        }
    }

    // with the stream idle; uint64 sums below 2^63 each: they fit an int64
    int result(int n_lags, int64_t *intermittent, int64_t *continuous_sums, int64_t *origin_counts) const
    {
        const size_t bytes = size_t(8) * n_lags;
        const char *sums = d_sums.as<char>();
        MDX_HIP(hipMemcpy(intermittent, sums, bytes, hipMemcpyDeviceToHost));
        MDX_HIP(hipMemcpy(continuous_sums, sums + bytes, bytes, hipMemcpyDeviceToHost));
        MDX_HIP(hipMemcpy(origin_counts, sums + 2 * bytes, bytes, hipMemcpyDeviceToHost));
        return MDX_OK;
    }
};

}  // namespace mdx
