// Source islands (cy_measure_islands): per source box, on the HBM-resident fp32 mosaic as cy_mosaic_prepare leaves it, the connected
// components of the thresholded box window that hold a seed (definitions: include/caesar_yolo_hip.h, DESIGN.md "Source islands").
//   candidate  valid pixel (value != 0 and finite) with (double)v >= merge_thr;   seed  candidate with (double)v >= seed_thr
//   component  maximal set of candidates connected through 8 or 4 neighbours inside the box window
//   island set components with a seed;   main island  the component of the window's peak pixel
// One workgroup of 256 threads owns one source from start to finish; no workgroup reads what another one wrote.  Labels are one
// u32 per pixel of the window (index i = dy * W + dx), in LDS when the window has at most ISL_LDS_MAX pixels, else in the slice of
// the per-call global workspace the host gave this source.  Five sweeps over the window, whatever the shape of the components:
//   1 init     label = first pixel of the candidate's horizontal run inside its wave's 64 consecutive pixels (one ballot), NOLAB
//              for a non-candidate; the window's peak pixel and the number of seeds on the way (no seed: zero row, done)
//   2 link     union-find by label equivalence: a pixel joins the run to its left across a 64-pixel boundary, and the run(s) of the
//              row above where its own left neighbour has not already made that link.  unite() hangs the larger root under the
//              smaller one with atomicMin; when the atomic finds the root already re-hung it carries on with what it displaced
//   3 flatten  label = root = smallest index of the component (so the labels do not depend on the order of the atomics)
//   4 seeds    bit 31 of the root's own label is set when the component holds a seed
//   5 sums     counts, bounding box, moments and mask bytes of the pixels whose root carries that bit
// Every loop has a bound fixed before it starts: sweeps run over the A pixels of the window, a walk to the root follows strictly
// decreasing labels (at most A steps), and unite() lowers the larger of its two roots with every retry (at most A retries).
// Workspace labels are read and written with agent-scope atomics (they go to L2, never to a stale line of the vector cache).
// Sums: float64 per lane over increasing pixel index, then the block reduction of cy_reduce.h, finished by thread 0.  The atomics
// are integer minima / ors on labels only.
#include "cy_label.h"                   // Lab, label_window: sweeps 1-4, and Moments, shared with cy_deblend.hip; Win, window_of (cy_px.h)

#pragma clang fp contract(off)          // w * (dx * dx) is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

struct ISmem {
    unsigned lab[ISL_LDS_MAX];
    LabRed lr;
    RedSlots<INT, 15> red;
};

template <bool LDS>
__device__ void islands(ISmem& s, const Lab<LDS> L, const IslandArgs& a, const Win wn, const double seed, const double merge,
                        const double bkg, unsigned char* __restrict__ mask, double* __restrict__ out) {
    const int tid = threadIdx.x;
    const size_t MW = (size_t)a.MW;
    const float* __restrict__ img = a.img + (size_t)wn.y0 * MW + (size_t)wn.x0;
    const unsigned W = wn.W, A = wn.A;

    // ---- 1-4 init, link, flatten, seeds (cy_label.h)
    float pv; unsigned pi;
    const unsigned nseed = label_window<LDS>(s.lr, L, img, MW, a.conn == 8, wn, seed, merge, pv, pi);
    if (nseed == 0) {                                         // uniform (from LDS): no island; the mask bytes are 0 already
        if (tid < ISL_FIELDS) out[tid] = (tid >= 6 && tid <= 9) ? -1.0 : 0.0;
        return;
    }

    // ---- 5 sums (the peak pixel is a seed, so its component is in the island set)
    const unsigned mainroot = L.ld(pi) & ROOT;
    Moments M;
    double Sm = 0.0;
    unsigned nisl = 0, npix = 0, nmain = 0, nborder = 0;
    int xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
    for (unsigned i = tid; i < A; i += INT) {
        const unsigned l = L.ld(i);
        if (l == NOLAB) continue;
        const unsigned r = l & ROOT;
        if (!(L.ld(r) & SEEDED)) continue;
        const unsigned dy = i / W, dx = i - dy * W;
        const double wt = (double)img[(size_t)dy * MW + dx] - bkg, fx = (double)dx, fy = (double)dy;
        const bool mn = r == mainroot;
        M.add(wt, fx, fy);
        if (mn) { Sm += wt; ++nmain; }
        ++npix; nisl += r == i;
        nborder += dx == 0 || dy == 0 || dx == W - 1 || dy == wn.H - 1;
        xmin = min(xmin, (int)dx); xmax = max(xmax, (int)dx); ymin = min(ymin, (int)dy); ymax = max(ymax, (int)dy);
        if (mask) mask[i] = mn ? 2 : 1;
    }
    const auto red = reduction(red_sum(M.m), red_sum(Sm), red_sum(nisl), red_sum(npix), red_sum(nmain), red_sum(nborder),
                               red_min(xmin), red_max(xmax), red_min(ymin), red_max(ymax));
    red.wave();
    red.park(s.red);
    __syncthreads();
    if (tid == 0) {
        red.total(s.red);
        out[0] = 0.0; out[1] = (double)nseed; out[2] = (double)nisl; out[3] = (double)npix; out[4] = (double)nmain; out[5] = (double)nborder;
        out[6] = (double)(wn.x0 + xmin); out[7] = (double)(wn.x0 + xmax); out[8] = (double)(wn.y0 + ymin); out[9] = (double)(wn.y0 + ymax);
        M.store(out + 10); out[16] = Sm;
        out[17] = 0.0; out[18] = 0.0; out[19] = 0.0;
    }
}

__global__ __launch_bounds__(INT) void islands_kernel(const IslandArgs a) {
    __shared__ ISmem s;
    const int b = blockIdx.x, tid = threadIdx.x;
    Win w;
    const long long area = window_of(a.win + (size_t)b * 4, a.MW, a.MH, w);       // held inside the image (cy_px.h)
    double* out = a.out + (size_t)b * ISL_FIELDS;
    const long long wo = a.off[(size_t)b * 2], mo = a.off[(size_t)b * 2 + 1];
    const bool lds = wo < 0;
    if (area == 0 || area > ISL_MAX_AREA || wo == ISL_OFF_TOO_LARGE) {
        // empty window: nothing to measure.  Above the supported maximum: status 1, nothing measured
        if (tid < ISL_FIELDS) out[tid] = tid == 0 ? (area ? 1.0 : 0.0) : (tid >= 6 && tid <= 9) ? -1.0 : 0.0;
        return;
    }
    if (lds && area > ISL_LDS_MAX) {
        // the host gave no workspace to a window that needs one.  launch_islands' caller cannot produce this; should it ever
        // happen, nothing is labelled (the LDS array would not hold it) and the row is NaN throughout: not a measurement and not
        // "window too large"
        if (tid < ISL_FIELDS) out[tid] = __longlong_as_double(0x7FF8000000000000LL);
        return;
    }
    const double seed = a.thr[(size_t)b * 3], merge = a.thr[(size_t)b * 3 + 1], bkg = a.thr[(size_t)b * 3 + 2];
    unsigned char* mask = a.mask ? a.mask + mo : nullptr;
    if (lds) islands<true>(s, Lab<true>{s.lab}, a, w, seed, merge, bkg, mask, out);
    else islands<false>(s, Lab<false>{a.ws + wo}, a, w, seed, merge, bkg, mask, out);
}

}  // namespace

hipError_t launch_islands(const IslandArgs& a, hipStream_t s) {
    if (a.n < 1 || a.MH < 1 || a.MW < 1 || (a.conn != 4 && a.conn != 8)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(islands_kernel, dim3(a.n), dim3(INT), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
