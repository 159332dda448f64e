// mdx_frame_feed.hpp — what the per-frame engines share between their C entry points and their
// X_accumulate_rows(h, d_pos, src_rows, d_index, n_rows, n_frames): the staged host-memory and trajectory-file routes,
// the particle index in HBM, the growing per-frame rows and the common part of a handle.  Host code only.
//
// An engine writes its preparation (set_device + grow_rows, or X_prepare: its ensure_device and the sizing of its
// slab or ring) and X_accumulate_rows; the rest of a route is one call of FrameEngine::accumulate_device / _host /
// _traj.  An engine whose handle touches its device only with the first frame (or result) derives from
// LazyFrameEngine, which holds that life cycle: ensure_device, reset, synchronize, collect.  The entry points
// themselves, their NULL checks included, come from mdx_frame_entry.hpp.  What the lag engines share about time is in
// mdx_lag_history.hpp.
#pragma once

#include "mdx_common.hpp"
#include "mdx_traj.hpp"

#include <algorithm>
#include <initializer_list>

namespace mdx {

// frames per staged slab: ~64 MB of coordinates of frames of `rows` rows (the caller's n on the host route, the
// file's n_atoms on the file route)
inline int64_t feed_slab_frames(int64_t n_frames, int64_t rows)
{
    return std::min<int64_t>(std::max<int64_t>(n_frames, 1), std::max<int64_t>(1, (int64_t(64) << 20) / (12 * rows)));
}

// the rows a file call selects: the index's, else the file's first n_index (all of them when n_index <= 0)
inline int traj_selection(const Trajectory *t, const int32_t *index, int64_t n_index, int64_t *n)
{
    *n = index ? n_index : (n_index > 0 ? n_index : t->n_atoms);
    MDX_REQUIRE(*n > 0 && (index || *n <= t->n_atoms), "selection larger than the trajectory");
    return MDX_OK;
}

// a host particle index (or NULL) against [0, n_atoms): needs no device
inline int check_particle_index(const int32_t *index, int64_t n_index, int64_t n_atoms)
{
    for (int64_t i = 0; index && i < n_index; ++i)
        MDX_REQUIRE(index[i] >= 0 && index[i] < n_atoms, "particle index %d out of range [0, %lld)", index[i],
                    (long long)n_atoms);
    return MDX_OK;
}

struct FrameFeed {
    StagePipeline pipe;
    DeviceBuffer d_stage[2], d_index;
    std::vector<int32_t> index_host;   // what d_index holds

    // A checked host index in HBM for the kernels on `compute`: d_index is kept while the index does not change.
    // *out = nullptr when index is NULL.  `compute` and the copy stream are waited for before the buffer is rewritten.
    int upload_index(hipStream_t compute, const int32_t *index, int64_t n_index, const int **out)
    {
        *out = nullptr;
        if (!index)
            return MDX_OK;
        if (int64_t(index_host.size()) != n_index || memcmp(index_host.data(), index, size_t(4) * n_index) != 0) {
            // kernels and staging copies of earlier calls may still read the old one
            MDX_HIP(hipStreamSynchronize(compute));
            if (pipe.copy_stream)
                MDX_HIP(hipStreamSynchronize(pipe.copy_stream));
            MDX_TRY(d_index.ensure(size_t(4) * std::max<int64_t>(n_index, 1)));
            MDX_HIP(hipMemcpy(d_index.ptr, index, size_t(4) * n_index, hipMemcpyHostToDevice));
            index_host.assign(index, index + n_index);
        }
        *out = d_index.as<int>();
        return MDX_OK;
    }

    // pos float32[n_frames][n][3] in host memory, `slab` frames at a time: the copies of slab k+1 overlap what
    // rows_fn(d_pos, nf) queues on `compute` for slab k (StagePipeline)
    template <typename Rows>
    int host(int dev, hipStream_t compute, const float *pos, int64_t n, int64_t n_frames, int64_t slab, Rows rows_fn)
    {
        return pipe.run(
            compute, n_frames, slab,
            [&](int b, int64_t f0, int64_t nf) -> int {
                MDX_TRY(d_stage[b].ensure(size_t(12) * n * slab));
                return device_stager(dev).upload(dev, pipe.copy_stream, d_stage[b].ptr, pos + f0 * n * 3,
                                                 size_t(12) * n * nf);
            },
            [&](int b, int64_t, int64_t nf) -> int { return rows_fn(d_stage[b].as<float>(), nf); });
    }

    // the same for the listed frames of a trajectory file, gathered to the n rows of d_index (nullptr: the first n)
    template <typename Rows>
    int traj(int dev, hipStream_t compute, Trajectory *t, const int64_t *frames, int64_t n_frames, const int *d_index,
             int64_t n, int64_t slab, Rows rows_fn)
    {
        return pipe.run(
            compute, n_frames, slab,
            [&](int b, int64_t f0, int64_t nf) -> int {
                MDX_TRY(d_stage[b].ensure(size_t(12) * n * slab));
                TrajSelection sel{d_index, n, d_stage[b].as<float>()};
                return t->stage_async(dev, pipe.copy_stream, frames + f0, nf, &sel, 1);
            },
            [&](int b, int64_t, int64_t nf) -> int { return rows_fn(d_stage[b].as<float>(), nf); });
    }

    // destroy paths, after the compute stream has been synchronised
    void destroy()
    {
        pipe.destroy();     // waits for its copy stream
        for (DeviceBuffer *b : {&d_stage[0], &d_stage[1], &d_index})
            b->recycle();
    }
};

// Per-frame result rows of row_bytes each: capacity for `more` rows behind the frames_seen ones (doubling unless
// `exact`).  Growing copies the rows and waits for the stream, so the host and file routes ask once per call, before
// their copy / kernel pipeline starts.
inline int grow_rows(DeviceBuffer &rows, hipStream_t stream, int64_t row_bytes, int64_t frames_seen, int64_t more,
                     int64_t *capacity, bool exact = false)
{
    const int64_t need = frames_seen + more;
    if (more <= 0 || need <= *capacity)
        return MDX_OK;
    const int64_t cap = exact ? need : std::max<int64_t>(need, std::max<int64_t>(64, 2 * *capacity));
    DeviceBuffer grown;
    MDX_TRY(grown.ensure(size_t(row_bytes * cap)));
    if (frames_seen > 0)
        MDX_HIP(hipMemcpyAsync(grown.ptr, rows.ptr, size_t(row_bytes * frames_seen), hipMemcpyDeviceToDevice, stream));
    MDX_HIP(hipStreamSynchronize(stream));
    rows.recycle();
    rows = grown;
    *capacity = cap;
    return MDX_OK;
}

// Per-frame words of frame_bytes each that start at zero: room for `frames` frames (doubling); what the frames_seen
// frames hold moves along.  Growing waits for the stream.
inline int grow_frames(DeviceBuffer &buf, hipStream_t stream, size_t frame_bytes, int64_t frames_seen, int64_t frames)
{
    if (frame_bytes * frames <= buf.bytes)
        return MDX_OK;
    DeviceBuffer grown;
    MDX_TRY(grown.ensure(std::max(frame_bytes * frames, 2 * buf.bytes)));
    MDX_HIP(hipMemsetAsync(grown.ptr, 0, grown.bytes, stream));
    if (frames_seen > 0)
        MDX_HIP(hipMemcpyAsync(grown.ptr, buf.ptr, frame_bytes * frames_seen, hipMemcpyDeviceToDevice, stream));
    MDX_HIP(hipStreamSynchronize(stream));          // nobody reads the old block any more
    buf.recycle();
    buf = grown;
    return MDX_OK;
}

// what every per-frame engine handle starts with
struct FrameEngine {
    int dev = 0;
    hipStream_t stream = nullptr;
    int64_t frames_seen = 0, slab_frames = 0;   // slab_frames: 0 = the default
    StreamTimer timer;
    FrameFeed feed;

    int enable_timing(int on)
    {
        timer.enabled = on != 0;
        return MDX_OK;
    }

    // the body of X_set_slab_frames (entry_name); most: the frames a launch of the engine takes
    int set_slab_frames(int64_t frames, int64_t most, const char *entry_name)
    {
        MDX_REQUIRE(frames >= 0 && frames <= most, "frames must lie in [0, %lld]", (long long)most);
        MDX_REQUIRE(frames_seen == 0, "%s must be called before the first frame", entry_name);
        slab_frames = frames;
        return MDX_OK;
    }

    // the body of X_synchronize of an engine whose handle holds its stream from create on ...
    int synchronize()
    {
        MDX_TRY(set_device(dev));
        MDX_HIP(hipStreamSynchronize(stream));
        return MDX_OK;
    }

    // ... and of its X_reset: an unwrap state starts over from `start` with the next frame
    int reset()
    {
        MDX_TRY(synchronize());
        timer.reset();
        frames_seen = 0;
        return MDX_OK;
    }

    // the head of X_stats; live = false: the handle has not touched its device yet
    int stats(bool live, int64_t *launches, double *kernel_ms, int64_t *frames)
    {
        if (live) {
            MDX_TRY(set_device(dev));
            MDX_HIP(hipStreamSynchronize(stream));
            timer.collect();
        }
        if (launches) *launches = timer.launches;
        if (kernel_ms) *kernel_ms = timer.total_ms;
        if (frames) *frames = frames_seen;
        return MDX_OK;
    }

    // the head of LazyFrameEngine::ensure_device: the handle's device is current and its stream exists
    int acquire_stream()
    {
        MDX_TRY(set_device(dev));
        if (!stream) {
            MDX_TRY(stream_acquire(&stream));
            timer.stream = stream;
        }
        return MDX_OK;
    }

    // The three input routes of the engine H (its handle derives from FrameEngine), after the entry point's NULL
    // checks.  want: the rows a frame must hold, `noun` holds them ("groups", "sets").  prepare(h, n_frames): what
    // has to exist before the first kernel (the device side of a lazy handle, room for the frames' rows);
    // rows_fn: the engine's X_accumulate_rows(h, d_pos, src_rows, d_index, n_rows, nf).  Argument errors come before
    // anything touches the device, and no frames touch nothing; only rows_too_large, which bounds the kernels' int
    // offsets into a source frame, comes where the engines used to make it, behind prepare.
    template <typename H> using PrepareFn = int (*)(H *, int64_t);
    template <typename H> using RowsFn = int (*)(H *, const float *, int64_t, const int *, int64_t, int64_t);

    static int rows_too_large(int64_t src_rows)
    {
        MDX_REQUIRE(src_rows < (int64_t(1) << 31) / 3, "frames of %lld particles are too large", (long long)src_rows);
        return MDX_OK;
    }

    // d_pos float32[n_frames][n_atoms][3] in HBM; index: host int32[n_index] rows of a frame, or NULL for all
    template <typename H>
    int accumulate_device(const float *d_pos, int64_t n_atoms, int64_t n_frames, const int32_t *index, int64_t n_index,
                          int64_t want, const char *noun, PrepareFn<H> prepare, RowsFn<H> rows_fn)
    {
        H *h = static_cast<H *>(this);
        MDX_REQUIRE(n_atoms > 0 && n_frames >= 0 && (!index || n_index > 0), "bad size");
        const int64_t n = index ? n_index : n_atoms;
        MDX_REQUIRE(n == want, "%lld rows given, the %s hold %lld", (long long)n, noun, (long long)want);
        MDX_TRY(check_particle_index(index, n_index, n_atoms));
        if (n_frames == 0)
            return MDX_OK;
        MDX_TRY(prepare(h, n_frames));
        const int *d_index = nullptr;
        MDX_TRY(feed.upload_index(stream, index, n_index, &d_index));
        MDX_TRY(rows_too_large(n_atoms));
        return rows_fn(h, d_pos, n_atoms, d_index, n, n_frames);
    }

    // pos float32[n_frames][n][3] in host memory, staged in slabs sized by n
    template <typename H>
    int accumulate_host(const float *pos, int64_t n, int64_t n_frames, int64_t want, const char *noun,
                        PrepareFn<H> prepare, RowsFn<H> rows_fn)
    {
        H *h = static_cast<H *>(this);
        MDX_REQUIRE(n > 0 && n_frames >= 0, "bad size");
        MDX_REQUIRE(n == want, "%lld rows given, the %s hold %lld", (long long)n, noun, (long long)want);
        if (n_frames == 0)
            return MDX_OK;
        MDX_TRY(prepare(h, n_frames));
        MDX_TRY(rows_too_large(n));
        return feed.host(dev, stream, pos, n, n_frames, feed_slab_frames(n_frames, n),
                         [&](const float *d_pos, int64_t nf) -> int { return rows_fn(h, d_pos, n, nullptr, n, nf); });
    }

    // the listed frames of a trajectory file, gathered to the index's rows (NULL: the file's first n_index) while
    // they are staged, in slabs sized by the file's n_atoms
    template <typename H>
    int accumulate_traj(Trajectory *t, const int64_t *frames, int64_t n_frames, const int32_t *index, int64_t n_index,
                        int64_t want, const char *noun, PrepareFn<H> prepare, RowsFn<H> rows_fn)
    {
        H *h = static_cast<H *>(this);
        MDX_REQUIRE(n_frames >= 0 && (n_frames == 0 || frames), "bad frame list");
        int64_t n = 0;
        MDX_TRY(traj_selection(t, index, n_index, &n));
        MDX_REQUIRE(n == want, "%lld rows selected, the %s hold %lld", (long long)n, noun, (long long)want);
        MDX_TRY(check_particle_index(index, n_index, t->n_atoms));
        if (n_frames == 0)
            return MDX_OK;
        MDX_TRY(prepare(h, n_frames));
        const int *d_index = nullptr;
        MDX_TRY(feed.upload_index(stream, index, n_index, &d_index));
        MDX_TRY(rows_too_large(n));
        return feed.traj(dev, stream, t, frames, n_frames, d_index, n, feed_slab_frames(n_frames, t->n_atoms),
                         [&](const float *d_pos, int64_t nf) -> int { return rows_fn(h, d_pos, n, nullptr, n, nf); });
    }

    // the device side of X_destroy: everything idle, then blocks and stream back to the per-device pools
    void release(std::initializer_list<DeviceBuffer *> own)
    {
        (void)hipSetDevice(dev);
        if (stream)
            (void)hipStreamSynchronize(stream);
        timer.destroy();
        feed.destroy();
        for (DeviceBuffer *b : own)
            b->recycle();
        if (stream)
            stream_release(stream);
    }
};

// A handle that touches its device only with the first frame (or result): creating one, and every argument error,
// needs none.  A struct of its own rather than a flag in FrameEngine, whose other engines (gyration, rouse, msid,
// dipole, profile) acquire their stream in create and would carry a field that is always true.
struct LazyFrameEngine : FrameEngine {
    bool ready = false;                 // the device side exists

    // build(h): the engine's ensures, uploads and zero, on the stream that exists by then
    template <typename H>
    int ensure_device(int (*build)(H *))
    {
        if (ready)
            return set_device(dev);
        MDX_TRY(acquire_stream());
        MDX_TRY(build(static_cast<H *>(this)));
        MDX_HIP(hipStreamSynchronize(stream));
        ready = true;
        return MDX_OK;
    }

    // a handle that never touched its device has nothing to give back
    void release(std::initializer_list<DeviceBuffer *> own)
    {
        if (stream)
            FrameEngine::release(own);
    }

    // the host counters a reset clears: an engine that has some declares its own
    void clear_counters() {}

    // the body of X_reset, after the engine has cleared its own host counters; zero(h): the device side starts over
    template <typename H>
    int reset(int (*zero)(H *))
    {
        frames_seen = 0;
        if (!ready)
            return MDX_OK;
        MDX_TRY(set_device(dev));
        MDX_HIP(hipStreamSynchronize(stream));
        timer.reset();
        MDX_TRY(zero(static_cast<H *>(this)));
        MDX_HIP(hipStreamSynchronize(stream));
        return MDX_OK;
    }

    // the body of X_synchronize; where `ready`, the engine may look at its control words afterwards
    int synchronize()
    {
        if (!ready)
            return MDX_OK;
        MDX_TRY(set_device(dev));
        MDX_HIP(hipStreamSynchronize(stream));
        return MDX_OK;
    }

    // the head of X_result behind the engine's ensure_device (and its fold, where it has one)
    int collect()
    {
        MDX_HIP(hipStreamSynchronize(stream));
        timer.collect();
        return MDX_OK;
    }

    int stats(int64_t *launches, double *kernel_ms, int64_t *frames)
    {
        return FrameEngine::stats(ready, launches, kernel_ms, frames);
    }
};

}  // namespace mdx
