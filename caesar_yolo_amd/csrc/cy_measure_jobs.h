// Job records and limits shared by the measurement kernels (cy_islands.hip, cy_deblend.hip, cy_fit.hip, cy_blend.hip, cy_aperture.hip,
// cy_peakfit.hip, cy_peakgroup.hip, cy_disc_residual.hip, cy_forced.hip) and the
// host-side planner that fills them (cy_measure_plan.cpp).  No HIP include: the planner also builds as plain C++.
#pragma once

namespace cy {

constexpr int ISL_LDS_MAX = 4096;              // largest window (pixels) whose labels live in LDS: 16 KiB of labels per workgroup
constexpr long long ISL_MAX_AREA = 1LL << 24;  // largest supported window; a larger one gets status 1
constexpr long long ISL_OFF_LDS = -1, ISL_OFF_TOO_LARGE = -2;
constexpr int DBL_MAX_COMP = 16;               // CY_DBL_MAX_COMP
constexpr int FIT_FIELDS = 32;                 // CY_FIT_FIELDS
constexpr long long FIT_MAX_AREA = 1LL << 24;  // largest supported window; the components of a larger one get status 1 from the runtime
constexpr int BLEND_FIELDS = 36;               // CY_BLEND_FIELDS
constexpr int BLEND_MAX_MEMBERS = 4;           // CY_BLEND_MAX_MEMBERS
constexpr int RND_FIELDS = 8;                  // CY_RND_FIELDS
constexpr int RND_HALF_MAX = 256;              // CY_RND_HALF_MAX: largest half-width of a support rectangle
constexpr int RND_TILE = 32;                   // side of an image tile of the render kernel: one workgroup each
constexpr int RND_MAX_COMP = 1 << 20;          // most components of one cy_render_gaussians call
constexpr long long RND_MAX_LIST = 1LL << 27;  // most entries of its tile table
constexpr int RES_FIELDS = 12;                 // CY_RES_FIELDS
constexpr int PEAK_FIELDS = 12;                // CY_PEAK_FIELDS
constexpr int PEAK_RADIUS_MAX = 8;             // CY_PEAK_RADIUS_MAX
constexpr int PEAK_CAP_MAX = 1 << 20;          // CY_PEAK_CAP_MAX
constexpr int PEAK_SEG = 1024;                 // pixels of a segment of the peak search: one workgroup of 256 threads, four pixels each
constexpr int PEAK_SEG_WORDS = PEAK_SEG / 64;  // 64-bit words of a segment's peak bitmap
constexpr long long PEAK_MAX_SEG = 1LL << 24;  // most segments of one cy_find_peaks call
constexpr int ATR_STEP_MAX = 64;               // CY_ATROUS_STEP_MAX
constexpr int ATR_COLS = 256;                  // columns of a column block of the a trous pass: one workgroup, one column per thread
constexpr int ATR_CHUNK = 64;                  // output rows of one residue class (y mod step) that a work item walks
constexpr int ATR_GRID_MAX = 1 << 13;          // 4 rounds of the 2048 workgroups a 256-CU chip holds; more work items are walked with the grid's stride
constexpr int APER_RINGS_MAX = 8;              // CY_APER_RINGS_MAX
constexpr int APER_RADIUS_MAX = 256;           // CY_APER_RADIUS_MAX: largest outer radius in pixels; a window has at most 513 x 513 pixels
constexpr int APER_HEAD = 8;                   // CY_APER_HEAD
constexpr int APER_RING_FIELDS = 4;            // CY_APER_RING_FIELDS: npix sum sumsq svar
constexpr int APER_FIELDS = APER_HEAD + APER_RING_FIELDS * APER_RINGS_MAX;     // CY_APER_FIELDS
constexpr int APER_JOBS_MAX = 1 << 20;         // CY_APER_JOBS_MAX: one workgroup per job, the grid in x only
constexpr int PFIT_JOB_FIELDS = 11;            // CY_PFIT_JOB_FIELDS: cx cy R bkg sign A x0 y0 a b c
constexpr int PFIT_FIELDS = 40;                // CY_PFIT_FIELDS
constexpr int PFIT_RADIUS_MAX = 256;           // CY_PFIT_RADIUS_MAX: largest disc radius in pixels; a window has at most 513 x 513 pixels
constexpr int PFIT_NEIGH_MAX = 8;              // CY_PFIT_NEIGH_MAX: neighbours a job shares its disc with
constexpr int PFIT_JOBS_MAX = 1 << 20;         // CY_PFIT_JOBS_MAX: one workgroup per fitted job, the grid in x only
constexpr int PGRP_FIELDS = 44;                // CY_PGRP_FIELDS: the 36 fields of a blend row, wx0 wx1 wy0 wy1 clipped nexcluded nlinked 0
constexpr int DRES_FIELDS = 16;                // CY_DRES_FIELDS: status npix nexcluded sum sumsq maxabs x_max y_max model_sum 0, wx0 wx1 wy0 wy1 clipped nneigh
constexpr int FORCED_JOB_FIELDS = 6;            // CY_FORCED_JOB_FIELDS: x0 y0 a b c bkg
constexpr int FORCED_FIELDS = 24;               // CY_FORCED_FIELDS
constexpr int FORCED_NEIGH_MAX = 7;             // CY_FORCED_NEIGH_MAX: neighbours whose amplitudes are solved with a job's
constexpr int FORCED_JOBS_MAX = 1 << 20;        // CY_FORCED_JOBS_MAX: one workgroup per runnable job, the grid in x only
constexpr int FORCED_SIDE_MAX = 2 * RND_HALF_MAX + 2;      // a support rectangle has at most 514 x 514 pixels

struct FitJob {
    long long list_off;             // first list entry of the job in FitArgs::list
    unsigned npos;                  // list entries: window pixels whose mask byte is the job's component + 1, valid or not
    int x0, y0;                     // first column / row of the box window, inside the image
    unsigned W, A;                  // width and pixel count of the window; A <= FIT_MAX_AREA
    int row;                        // output row: source * DBL_MAX_COMP + component
    double bkg;
    double p0[6];                   // start {A, x0, y0, a, b, c}, x0 / y0 relative to the window's first pixel
};

struct BlendJob {
    long long list_off;             // first list entry of the job in BlendArgs::list
    unsigned npos;                  // list entries: window pixels whose mask byte belongs to a member, valid or not
    int x0, y0;                     // first column / row of the box window, inside the image
    unsigned W, A;                  // width and pixel count of the window; A <= FIT_MAX_AREA
    int row0;                       // output row of the source's component 0: source * DBL_MAX_COMP
    int M;                          // members, 2 .. BLEND_MAX_MEMBERS
    int comp[BLEND_MAX_MEMBERS];    // their component indices, increasing; comp[0] is the group's id
    double bkg;
    double p0[6 * BLEND_MAX_MEMBERS];   // starts in slot order, x0 / y0 relative to the window's first pixel
};

struct AperJob {
    double cx, cy;                  // centre in image pixels, as given
    double r2[APER_RINGS_MAX];      // squared radii (factors[k] * unit, squared, each rounded on its own); 0 above K and when not measured
    int x0, x1, y0, y1;             // the window, inclusive, inside the image; {0, -1, 0, -1} when not measured
    int status;                     // 0 measured, 1 unit or outer radius out of range, 2 centre not finite or no pixel of the image in reach
    int clipped;                    // 1: the unclipped window leaves the image
};

struct PeakFitJob {
    double cx, cy;                  // centre in image pixels, as given
    double r2;                      // R * R
    double bkg, sign;               // y = sign * (v - bkg); sign is +1 or -1
    double p0[6];                   // start {A, x0, y0, a, b, c}, x0 / y0 relative to the window's first pixel
    int x0, x1, y0, y1;             // the window, inclusive, inside the image; {0, -1, 0, -1} when not fitted
    int status;                     // 0 fitted, 1 R, sign or bkg out of range, 5 centre not finite or no pixel of the image in reach
    int clipped;                    // 1: the unclipped window leaves the image
    int nneigh, crowded;            // kept neighbours; 1: there were more than PFIT_NEIGH_MAX
    int neigh[PFIT_NEIGH_MAX];      // their job indices in (squared distance, index) order; -1 beyond nneigh
};

struct PeakGroupJob {
    int M;                          // members, 2 .. BLEND_MAX_MEMBERS
    int member[BLEND_MAX_MEMBERS];  // their indices in the PeakFitJob table, increasing; member[0] is the group's id; -1 beyond M
    int nout[BLEND_MAX_MEMBERS];    // per member: its kept neighbours that are not members of the group
    int out[BLEND_MAX_MEMBERS][PFIT_NEIGH_MAX];     // their indices in the PeakFitJob table, in the member's own order; -1 beyond nout
    int x0, x1, y0, y1;             // the group window: the bounding box of the members' windows, inclusive, inside the image
    double bkg, sign;               // those of the member in slot 0
    double p0[6 * BLEND_MAX_MEMBERS];   // starts in slot order, x0 / y0 relative to the group window's first pixel
};

struct ForcedJob {
    double cx, cy, a, b, c;         // x0, y0 (image pixels) and the shape, as given
    double bkg;                     // y = (double)v - bkg
    int x0, x1, y0, y1;             // the support rectangle, inclusive, inside the image; {0, -1, 0, -1} when not run
    int status;                     // 0 run, 1 not admissible, 2 run with a capped half-width, 3 the rectangle misses the image
    int nneigh, crowded, ndup;      // kept neighbours; 1: there were more than FORCED_NEIGH_MAX; exact duplicates dropped
    int neigh[FORCED_NEIGH_MAX];    // their job indices in (squared centre distance, index) order; -1 beyond nneigh
};

}  // namespace cy
