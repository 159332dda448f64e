// mdx_frame_entry.hpp — the C entry points every per-frame engine has: its three input routes, enable_timing,
// synchronize, reset and destroy, and for the engines that work in slabs set_slab_frames and plan.  An entry point is
// its NULL checks and one call; the templates below hold both, and the macro lines at the end of an engine's unit turn
// them into its extern "C" symbols (declared, with their documentation, in include/mdx.h).  Host code only.
//
// What the handle H of an engine X provides, as ordinary members the templates find by name:
//   int64_t rows_wanted() const      the rows a frame must hold ...
//   const char *rows_noun() const    ... and what holds them, for the message ("groups", "sets", "tables")
//   void free_device()               release({&d_a, &d_b, ...}) of every DeviceBuffer the handle owns (and
//                                    mol.recycle() where it has a MoleculeStage)
//   void clear_counters()            the host counters a reset of a lazy handle clears; LazyFrameEngine's clears none
//   int64_t ring_lag() const         the lag the `ring` of a ring engine is sized by
// and as static functions of the unit, named in its macro lines: X_prepare and X_accumulate_rows
// (FrameEngine::PrepareFn / RowsFn); for a lazy engine X_zero (LazyFrameEngine::reset) and X_check, the look at its
// control words that follows a synchronize (`unchecked` where it has none); for a slabbed one X_slab(h), the frames
// of a launch.  Those are arguments rather than members because a member function of a handle has external linkage
// and would join the symbols the library exports; the templates are static for the same reason.
//
// An entry point whose rule differs stays written out in its engine, with a comment that names the difference.
#pragma once

#include "mdx_frame_feed.hpp"
#include "mdx_internal.hpp"

namespace mdx {

template <typename H>
static int entry_accumulate(H *h, const float *pos, int64_t n, int64_t n_frames, FrameEngine::PrepareFn<H> prepare,
                            FrameEngine::RowsFn<H> rows_fn)
{
    MDX_REQUIRE(h && pos, "NULL argument");
    return h->accumulate_host(pos, n, n_frames, h->rows_wanted(), h->rows_noun(), prepare, rows_fn);
}

template <typename H>
static int entry_accumulate_device(H *h, const float *d_pos, int64_t n_atoms, int64_t n_frames, const int32_t *index,
                                   int64_t n_index, FrameEngine::PrepareFn<H> prepare, FrameEngine::RowsFn<H> rows_fn)
{
    MDX_REQUIRE(h && d_pos, "NULL argument");
    return h->accumulate_device(d_pos, n_atoms, n_frames, index, n_index, h->rows_wanted(), h->rows_noun(), prepare,
                                rows_fn);
}

template <typename H>
static int entry_accumulate_traj(H *h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames, const int32_t *index,
                                 int64_t n_index, FrameEngine::PrepareFn<H> prepare, FrameEngine::RowsFn<H> rows_fn)
{
    MDX_REQUIRE(h && traj, "NULL handle");
    return h->accumulate_traj(mdx_traj_internal(traj), frames, n_frames, index, n_index, h->rows_wanted(),
                              h->rows_noun(), prepare, rows_fn);
}

template <typename H>
static int entry_enable_timing(H *h, int on)
{
    MDX_REQUIRE(h, "NULL handle");
    return h->enable_timing(on);
}

template <typename H>
static int entry_destroy(H *h)
{
    if (!h)
        return MDX_OK;
    h->free_device();
    delete h;
    return MDX_OK;
}

// an eager engine: FrameEngine::synchronize and ::reset
template <typename H>
static int entry_synchronize(H *h)
{
    MDX_REQUIRE(h, "NULL handle");
    return h->synchronize();
}

template <typename H>
static int entry_reset(H *h)
{
    MDX_REQUIRE(h, "NULL handle");
    return h->reset();
}

// a lazy engine: check(h) looks at the control words of a handle whose device side exists
template <typename H>
static int entry_synchronize(H *h, int (*check)(H *))
{
    MDX_REQUIRE(h, "NULL handle");
    MDX_TRY(h->synchronize());
    return h->ready ? check(h) : MDX_OK;
}

template <typename H>
static int unchecked(H *)
{
    return MDX_OK;
}

template <typename H>
static int entry_reset(H *h, int (*zero)(H *))
{
    MDX_REQUIRE(h, "NULL handle");
    h->clear_counters();
    return h->reset(zero);      // frames_seen = 0: a history or an unwrap state starts over with the next frame
}

// most: the frames a launch of the engine takes
template <typename H>
static int entry_set_slab_frames(H *h, int64_t frames, int64_t most, const char *entry_name)
{
    MDX_REQUIRE(h, "NULL handle");
    return h->set_slab_frames(frames, most, entry_name);
}

// slab = X_slab; an engine without a ring ...
template <typename H>
static int entry_plan(H *h, int64_t (*slab)(const H *), int64_t *slab_frames, int64_t *ring_frames)
{
    MDX_REQUIRE(h && slab_frames && ring_frames, "NULL argument");
    *slab_frames = slab(h);
    *ring_frames = 0;           // no frame outlives its slab
    return MDX_OK;
}

// ... and one with a ring
template <typename H>
static int entry_ring_plan(H *h, int64_t (*slab)(const H *), int64_t *slab_frames, int64_t *ring_frames)
{
    MDX_REQUIRE(h, "NULL handle");
    return h->ring.plan(h->frames_seen, h->ring_lag(), slab(h), slab_frames, ring_frames);
}

}  // namespace mdx

// The three input routes of engine X.
#define MDX_FRAME_ROUTES(X, prepare, accumulate_rows)                                                                  \
    extern "C" int mdx_##X##_accumulate(mdx_##X##_t h, const float *pos, int64_t n, int64_t n_frames)                  \
    {                                                                                                                  \
        return mdx::entry_accumulate(h, pos, n, n_frames, prepare, accumulate_rows);                                   \
    }                                                                                                                  \
    extern "C" int mdx_##X##_accumulate_device(mdx_##X##_t h, const float *d_pos, int64_t n_atoms, int64_t n_frames,   \
                                               const int32_t *index, int64_t n_index)                                  \
    {                                                                                                                  \
        return mdx::entry_accumulate_device(h, d_pos, n_atoms, n_frames, index, n_index, prepare, accumulate_rows);    \
    }                                                                                                                  \
    extern "C" int mdx_##X##_accumulate_traj(mdx_##X##_t h, mdx_traj_t traj, const int64_t *frames, int64_t n_frames,  \
                                             const int32_t *index, int64_t n_index)                                    \
    {                                                                                                                  \
        return mdx::entry_accumulate_traj(h, traj, frames, n_frames, index, n_index, prepare, accumulate_rows);        \
    }

// enable_timing, synchronize and destroy of an eager engine (FrameEngine), and its reset where that clears nothing of
// the engine's own ...
#define MDX_FRAME_LIFE_CYCLE(X)                                                                                        \
    extern "C" int mdx_##X##_enable_timing(mdx_##X##_t h, int on) { return mdx::entry_enable_timing(h, on); }          \
    extern "C" int mdx_##X##_synchronize(mdx_##X##_t h) { return mdx::entry_synchronize(h); }                          \
    extern "C" int mdx_##X##_destroy(mdx_##X##_t h) { return mdx::entry_destroy(h); }

#define MDX_FRAME_RESET(X)                                                                                             \
    extern "C" int mdx_##X##_reset(mdx_##X##_t h) { return mdx::entry_reset(h); }

// ... and all four of a lazy one (LazyFrameEngine)
#define MDX_LAZY_FRAME_LIFE_CYCLE(X, zero, check)                                                                      \
    extern "C" int mdx_##X##_enable_timing(mdx_##X##_t h, int on) { return mdx::entry_enable_timing(h, on); }          \
    extern "C" int mdx_##X##_synchronize(mdx_##X##_t h) { return mdx::entry_synchronize(h, check); }                   \
    extern "C" int mdx_##X##_reset(mdx_##X##_t h) { return mdx::entry_reset(h, zero); }                                \
    extern "C" int mdx_##X##_destroy(mdx_##X##_t h) { return mdx::entry_destroy(h); }

// set_slab_frames of an engine whose launches take at most `most` frames
#define MDX_FRAME_SET_SLAB_FRAMES(X, most)                                                                             \
    extern "C" int mdx_##X##_set_slab_frames(mdx_##X##_t h, int64_t frames)                                            \
    {                                                                                                                  \
        return mdx::entry_set_slab_frames(h, frames, most, "mdx_" #X "_set_slab_frames");                              \
    }

// plan of an engine without a ring ...
#define MDX_FRAME_PLAN(X, slab)                                                                                        \
    extern "C" int mdx_##X##_plan(mdx_##X##_t h, int64_t *slab_frames, int64_t *ring_frames)                           \
    {                                                                                                                  \
        return mdx::entry_plan(h, slab, slab_frames, ring_frames);                                                     \
    }

// ... and of one with a ring
#define MDX_FRAME_RING_PLAN(X, slab)                                                                                   \
    extern "C" int mdx_##X##_plan(mdx_##X##_t h, int64_t *slab_frames, int64_t *ring_frames)                           \
    {                                                                                                                  \
        return mdx::entry_ring_plan(h, slab, slab_frames, ring_frames);                                                \
    }
