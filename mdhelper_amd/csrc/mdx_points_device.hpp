// mdx_points_device.hpp — kernels that prepare the points of a frame, shared by the density-profile engine
// (mdx_profile.hip), the gyration engine (mdx_gyration.hip) and the chain-projection engine (mdx_rouse.hip): float64
// centres of mass of molecules, the image scan of the reference's global unwrap (algorithm/topology.py `unwrap`)
// and the widened, image-shifted point the chain kernels read.  float64 throughout, with separate multiply and add.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mdx_prof_dev {

template <typename T> __device__ __forceinline__ T prof_pick(int k, T a, T b, T c)
{
    return k == 0 ? a : k == 1 ? b : c;
}

// One frame as the chain kernels read it: x = (double)r + image * L, the shift applied in float64.
template <typename SRC> struct PointSource {
    const SRC *__restrict__ pos;        // frame of src_rows rows
    const int *__restrict__ index;      // row of point p, or nullptr: p
    const int *__restrict__ images;     // int[n_points][3] of the frame, or nullptr
    double L[3];

    __device__ __forceinline__ void load(int p, double x[3]) const
    {
        const int64_t r = index ? index[p] : p;
        const SRC *__restrict__ q = pos + r * 3;
        x[0] = (double)q[0];
        x[1] = (double)q[1];
        x[2] = (double)q[2];
        if (images) {
            const int *im = images + int64_t(p) * 3;
            x[0] = __dadd_rn(x[0], __dmul_rn((double)im[0], L[0]));
            x[1] = __dadd_rn(x[1], __dmul_rn((double)im[1], L[1]));
            x[2] = __dadd_rn(x[2], __dmul_rn((double)im[2], L[2]));
        }
    }
};

namespace {   // internal linkage: compiled into several translation units

// out[frame][m][k] = sum_a m_a x_a / M_m over the rows a of molecule m, in row order, float64 throughout:
// molecule_com_kernel (mdx_molecules.hpp) without its cast to float32 — the reference keeps these centres in a
// float64 array (profile.py:778-780).
__global__ __launch_bounds__(256) void prof_com_f64_kernel(const float *__restrict__ pos, int64_t src_rows,
                                                           const int *__restrict__ index,
                                                           const int64_t *__restrict__ offsets,
                                                           const double *__restrict__ masses,
                                                           const double *__restrict__ total_mass,
                                                           int64_t n_molecules, double *__restrict__ out)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;   // (molecule, k)
    const int64_t frame = blockIdx.y;
    if (i >= n_molecules * 3)
        return;
    const int64_t m = i / 3;
    const int k = int(i - 3 * m);
    const float *p = pos + frame * src_rows * 3 + k;
    double acc = 0.0;
    for (int64_t a = offsets[m]; a < offsets[m + 1]; ++a)
        acc = __dadd_rn(acc, __dmul_rn(masses[a], (double)p[3 * (index ? int64_t(index[a]) : a)]));
    out[(frame * n_molecules + m) * 3 + k] = __ddiv_rn(acc, total_mass[m]);
}

}  // namespace

// Global unwrap (topology.py `unwrap`), a scan along the frames of the call per coordinate: a displacement since
// the previous analysed frame of |d| >= L / 2 moves the image count by -sign(d).  prev / image carry the state from
// call to call; `first`: this is the first analysed frame, whose displacement is zero.  (The gyration engine
// passes first = 0 with prev = its starting points and image = 0, so its first frame is compared with them.)
template <typename SRC>
__global__ __launch_bounds__(256) void prof_unwrap_scan_kernel(const SRC *__restrict__ pos, int64_t src_rows,
                                                               const int *__restrict__ index, int n_points,
                                                               int n_frames, double hx, double hy, double hz,
                                                               int first, double *__restrict__ prev,
                                                               int *__restrict__ image, int *__restrict__ images)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= 3 * n_points)
        return;
    const int p = c / 3, k = c - 3 * p;
    const int64_t r = index ? index[p] : p;
    const double half = prof_pick(k, hx, hy, hz);
    double old = first ? 0.0 : prev[c];
    int im = first ? 0 : image[c];
    for (int f = 0; f < n_frames; ++f) {
        const double x = (double)pos[(int64_t(f) * src_rows + r) * 3 + k];
        if (!(first && f == 0)) {
            const double d = __dsub_rn(x, old);
            if (fabs(d) >= half)
                im -= (d > 0.0) - (d < 0.0);
        }
        old = x;
        images[int64_t(f) * 3 * n_points + c] = im;
    }
    prev[c] = old;
    image[c] = im;
}

}  // namespace mdx_prof_dev
