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
// Sums: float64 per lane over increasing pixel index, __shfl_down tree per wave, the four waves added in order by thread 0:
// fixed association, so two runs give the same bits.  The atomics are integer minima / ors on labels only.
#include "cy_label.h"                   // Lab, label_window: sweeps 1-4, shared with cy_deblend.hip; Win, window_of (cy_px.h)

#pragma clang fp contract(off)          // w * (dx * dx) is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

struct ISmem {
    unsigned lab[ISL_LDS_MAX];
    LabRed lr;
    double red[7][INW];
    unsigned cnt[5][INW];
    int box[4][INW];
};

template <bool LDS>
__device__ void islands(ISmem& s, const Lab<LDS> L, const IslandArgs& a, const Win wn, const double seed, const double merge,
                        const double bkg, unsigned char* __restrict__ mask, double* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
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
    double S = 0.0, Sx = 0.0, Sy = 0.0, Sxx = 0.0, Syy = 0.0, Sxy = 0.0, Sm = 0.0;
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
        S += wt; Sx += wt * fx; Sy += wt * fy; Sxx += wt * (fx * fx); Syy += wt * (fy * fy); Sxy += wt * (fx * fy);
        if (mn) { Sm += wt; ++nmain; }
        ++npix; nisl += r == i;
        nborder += dx == 0 || dy == 0 || dx == W - 1 || dy == wn.H - 1;
        xmin = min(xmin, (int)dx); xmax = max(xmax, (int)dx); ymin = min(ymin, (int)dy); ymax = max(ymax, (int)dy);
        if (mask) mask[i] = mn ? 2 : 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        S += __shfl_down(S, o); Sx += __shfl_down(Sx, o); Sy += __shfl_down(Sy, o); Sxx += __shfl_down(Sxx, o);
        Syy += __shfl_down(Syy, o); Sxy += __shfl_down(Sxy, o); Sm += __shfl_down(Sm, o);
        nisl += __shfl_down(nisl, o); npix += __shfl_down(npix, o); nmain += __shfl_down(nmain, o); nborder += __shfl_down(nborder, o);
        xmin = min(xmin, __shfl_down(xmin, o)); xmax = max(xmax, __shfl_down(xmax, o));
        ymin = min(ymin, __shfl_down(ymin, o)); ymax = max(ymax, __shfl_down(ymax, o));
    }
    if (lane == 0) {
        s.red[0][w] = S; s.red[1][w] = Sx; s.red[2][w] = Sy; s.red[3][w] = Sxx; s.red[4][w] = Syy; s.red[5][w] = Sxy; s.red[6][w] = Sm;
        s.cnt[1][w] = nisl; s.cnt[2][w] = npix; s.cnt[3][w] = nmain; s.cnt[4][w] = nborder;
        s.box[0][w] = xmin; s.box[1][w] = xmax; s.box[2][w] = ymin; s.box[3][w] = ymax;
    }
    __syncthreads();
    if (tid == 0) {
        for (int j = 1; j < INW; ++j) {
            S += s.red[0][j]; Sx += s.red[1][j]; Sy += s.red[2][j]; Sxx += s.red[3][j]; Syy += s.red[4][j]; Sxy += s.red[5][j]; Sm += s.red[6][j];
            nisl += s.cnt[1][j]; npix += s.cnt[2][j]; nmain += s.cnt[3][j]; nborder += s.cnt[4][j];
            xmin = min(xmin, s.box[0][j]); xmax = max(xmax, s.box[1][j]); ymin = min(ymin, s.box[2][j]); ymax = max(ymax, s.box[3][j]);
        }
        out[0] = 0.0; out[1] = (double)nseed; out[2] = (double)nisl; out[3] = (double)npix; out[4] = (double)nmain; out[5] = (double)nborder;
        out[6] = (double)(wn.x0 + xmin); out[7] = (double)(wn.x0 + xmax); out[8] = (double)(wn.y0 + ymin); out[9] = (double)(wn.y0 + ymax);
        out[10] = S; out[11] = Sx; out[12] = Sy; out[13] = Sxx; out[14] = Syy; out[15] = Sxy; out[16] = Sm;
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
