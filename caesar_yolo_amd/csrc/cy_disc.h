// Membership addressed by position, shared by the fit of a peak (cy_peakfit.hip) and the joint fit of a group of peaks
// (cy_peakgroup.hip): window pixel (qx, qy) is a member of job e when d2_e = (qx - cx_e)^2 + (qy - cy_e)^2 <= R_e^2 and d2_f >= d2_e
// for each of the at most DISC_NB neighbours f the disc was given (a pixel goes to the nearest centre; a tie belongs to both).
// Distances in image coordinates, two products and one sum, not contracted.
#pragma once
#include "cy_measure_jobs.h"

#pragma clang fp contract(off)          // every product is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int DISC_NB = PFIT_NEIGH_MAX;

// what membership needs, all uniform: the window's first pixel and width, the job's centre and squared radius, its neighbours
struct Disc {
    int bx0, by0; unsigned W;
    double cx, cy, r2;
    int nn;
    double ncx[DISC_NB], ncy[DISC_NB];
};

// window pixel i: inside the disc (in) and nearer to no kept neighbour than to the job's own centre (returned)
__device__ __forceinline__ bool member(const Disc& d, const unsigned i, unsigned& wx, unsigned& wy, bool& in) {
    wy = i / d.W; wx = i - wy * d.W;
    const double qx = (double)(d.bx0 + (int)wx), qy = (double)(d.by0 + (int)wy);
    const double ex = qx - d.cx, ey = qy - d.cy;
    const double exx = ex * ex, eyy = ey * ey;
    const double d2 = exx + eyy;
    in = d2 <= d.r2;
    bool mine = in;
#pragma unroll
    for (int k = 0; k < DISC_NB; ++k) {
        const double fx = qx - d.ncx[k], fy = qy - d.ncy[k];
        const double fxx = fx * fx, fyy = fy * fy;
        const double f2 = fxx + fyy;
        mine = mine && (k >= d.nn || f2 >= d2);
    }
    return mine;
}

}  // namespace
}  // namespace cy
