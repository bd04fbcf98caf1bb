// The pixel test and the box window of the measurement kernels (cy_measure, cy_background, cy_islands, cy_deblend, cy_fit, cy_blend,
// cy_residual, cy_peaks, cy_forced): what "valid" means and how a window that arrives from the host is held inside the image, once.
#pragma once
#include "cy_kernels.h"
#include <cfloat>

namespace cy {
namespace {

__device__ __forceinline__ bool valid_px(float v) { return v != 0.0f && fabsf(v) <= FLT_MAX; }      // NaN fails the second test
__device__ __forceinline__ bool noisy_px(float r) { return r > 0.0f && r <= FLT_MAX; }             // a usable rms (cy_peaks, cy_forced); NaN fails both tests

struct Win { int x0, y0; unsigned W, H, A; };

// wn = {x0, x1, y0, y1}, inclusive.  The host's windows are already inside the image; clamped again so that no index can leave it
// whatever arrives here (a clamp only shrinks a window, so the slices the host sized for it still hold it).  -> the area, 0 for an
// empty window; w is meaningful for an area in 1 .. 2^32 - 1 (the callers stop at ISL_MAX_AREA).
__device__ __forceinline__ long long window_of(const int* wn, const int MW, const int MH, Win& w) {
    const int bx0 = max(wn[0], 0), bx1 = min(wn[1], MW - 1), by0 = max(wn[2], 0), by1 = min(wn[3], MH - 1);
    const long long area = bx1 < bx0 || by1 < by0 ? 0 : (long long)(bx1 - bx0 + 1) * (by1 - by0 + 1);
    w.x0 = bx0; w.y0 = by0; w.W = (unsigned)(bx1 - bx0 + 1); w.H = (unsigned)(by1 - by0 + 1); w.A = (unsigned)area;
    return area;
}

}  // namespace
}  // namespace cy
