// Host-side planning of the measurement entries (cy_measure_sources, cy_measure_islands, cy_deblend_islands, cy_fit_components,
// cy_fit_blends, cy_render_gaussians, cy_measure_residuals, cy_find_peaks, cy_atrous_step, cy_aperture_sums, cy_fit_peaks, cy_fit_peak_groups, cy_disc_residuals, cy_forced_fit): box windows, the island table, the fit and blend job tables with their pixel lists, and the write-back of the
// fitted rows.  Plain C++: host pointers in, vectors out, no context and no HIP type, so that tests/host/measure_plan_main.cpp runs
// it under the host sanitizers.  A planner returns null, or the message of the first source (in index order) it rejects.
#pragma once
#include "cy_measure_jobs.h"
#include <vector>

namespace cy {

// Inclusive pixel window of a float64 box {x1, y1, x2, y2}: columns [max(0, ceil(x1)), min(MW - 1, floor(x2))], rows likewise with MH.
// A side that misses the image or holds no pixel centre, or a NaN edge, makes the whole window empty: {0, -1, 0, -1}, area 0.
struct BoxWindow { int x0, x1, y0, y1; long long area; };
BoxWindow box_window(const double* box, int MH, int MW);

// win[n][8] of MeasureArgs: the box window, then the box window grown by `ring` and clipped to the image
std::vector<int> ring_windows(const double* boxes, int n, int ring, int MH, int MW);

// win[n][4] and off[n][2] of IslandArgs / DeblendArgs.  nws: pixels of the windows labelled in the workspace (above ISL_LDS_MAX, up
// to ISL_MAX_AREA); nmask: pixels of all windows.  thr: rows of thr_stride doubles {seed_thr, merge_thr, ..}; mask_off: [n + 1]
// byte offsets the caller claims for the windows, checked against their areas, or null.
struct IslandTable { std::vector<int> win; std::vector<long long> off; long long nws = 0, nmask = 0; };
const char* plan_islands(const double* boxes, const double* thr, int thr_stride, const long long* mask_off, int n, int MH, int MW, IslandTable& t);

// Inputs of cy_fit_components / cy_fit_blends: per source a box, a background, ncomp components with a start of six parameters
// each ([n][DBL_MAX_COMP][6]) and the bytes of its window in mask, from mask_off[i] to mask_off[i + 1] (byte k + 1: component k).
struct FitInputs {
    int MH, MW, n;
    const double* boxes; const double* bkg; const int* ncomp; const double* start;
    const unsigned char* mask; const long long* mask_off;
};
struct FitPlan {
    std::vector<FitJob> jobs;           // one per component of every window up to FIT_MAX_AREA pixels
    std::vector<unsigned> list;         // the jobs' window indices, job after job, increasing inside a job
    std::vector<int> win0;              // [n][2] first column and row of the windows
    std::vector<char> large;            // [n] 1: window above FIT_MAX_AREA, no job; its components report status 1
};
const char* plan_fit(const FitInputs& in, FitPlan& p);
struct BlendPlan {
    std::vector<BlendJob> jobs;         // one per group of 2 .. BLEND_MAX_MEMBERS touching components
    std::vector<unsigned> list;         // the jobs' window indices (pixels of any member), job after job, increasing inside a job
    std::vector<int> win0;              // [n][2] as FitPlan
    std::vector<double> rows;           // [n][DBL_MAX_COMP][BLEND_FIELDS] what the host decides: {group, members, slot} in fields 5 .. 7 of
                                        // every component; status 1 (large window), 6 (alone), 5 with the start in fields 8 .. 13 (group above the limit)
};
const char* plan_blend(const FitInputs& in, BlendPlan& p);

// cy_render_gaussians.  comp: [m][6] {A, x0, y0, a, b, c} with x0, y0 in image pixels.  Per component the status and the support
// rectangle (float64, every operation rounded on its own: det = a*c - b*b, hx = min(ceil(nsigma * sqrt(c / det)), RND_HALF_MAX),
// hy likewise with a; columns [max(0, floor(x0) - hx), min(MW - 1, floor(x0) + 1 + hx)], rows likewise with MH), and a CSR table over
// the RND_TILE x RND_TILE tiles of the image (row-major): per tile the rendered components whose rectangle meets it, in increasing
// index.  Returns the message of a size limit: m outside [0, RND_MAX_COMP], or a table above RND_MAX_LIST entries.
struct RenderPlan {
    std::vector<double> rows;           // [m][RND_FIELDS] {status, sx0, sx1, sy0, sy1, ntiles, 0, 0}: status 0 rendered, 1 not admissible,
                                        // 2 rendered with a capped half-width, 3 the rectangle misses the image; rectangle -1 when skipped
    std::vector<int> rect;              // [m][4] the rectangles as integers ({0, -1, 0, -1} when skipped)
    std::vector<int> tile_off;          // [ntx * nty + 1]
    std::vector<int> tile_list;
    int ntx = 0, nty = 0;
};
// signed_amp (cy_render_signed_gaussians): a component is admissible with A < 0 too (A != 0 in place of A > 0); nothing else differs.
const char* plan_render(const double* comp, int m, double nsigma, int MH, int MW, RenderPlan& p, bool signed_amp = false);

// The support rectangle of one Gaussian, shared by plan_render and plan_forced.  q: {x0, y0, a, b, c}; r: the rectangle {sx0, sx1,
// sy0, sy1} as plan_render describes it, {0, -1, 0, -1} when there is none.  Returns 0, 1 (a field not finite, a <= 0, c <= 0 or
// a*c - b*b <= 0), 2 (a capped half-width) or 3 (the rectangle misses the image).  hx_out, when given and the status is not 1: the
// half-width in columns after the cap.
int support_rect(const double* q, double nsigma, int MH, int MW, int* r, double* hx_out = nullptr);

// cy_measure_residuals: the box windows and checked mask offsets, as plan_islands gives them (off[i][0] is ISL_OFF_TOO_LARGE for a
// window above ISL_MAX_AREA pixels, off[i][1] the window's first mask byte)
const char* plan_residuals(const double* boxes, const long long* mask_off, int n, int MH, int MW, IslandTable& t);

// cy_find_peaks.  The image is cut into segments of PEAK_SEG consecutive pixels of one row (the last of a row holds the remaining
// MW - (nsx - 1) * PEAK_SEG), segment s = iy * nsx + sx, which is the row-major order of their pixels.  Sizes in 64-bit: a
// (2^24) x 127 image has 2^24 segments of 127 pixels.  Returns the message of a limit: an image of 2^31 pixels or more, more than
// PEAK_MAX_SEG segments, or a row so wide that a column of its last segment plus the radius leaves the 32-bit range the kernels
// index columns in.  radius and cap are in range (the entry checks them before).
struct PeakPlan {
    int nsx = 0;                        // segments of a row: ceil(MW / PEAK_SEG)
    long long nseg = 0;                 // MH * nsx: entries of the count table and of the offset table
    long long words = 0;                // 64-bit words of the peak bitmap: nseg * PEAK_SEG_WORDS
    long long row_values = 0;           // float64 values of the device row table: cap * PEAK_FIELDS
};
const char* plan_peaks(int MH, int MW, int radius, int cap, PeakPlan& p);

// cy_atrous_step.  Rows y, y +- step, y +- 2 step of one residue class r = y mod step form a 1-D problem of their own: output row t
// of class r is y = r + t * step, t < ceil((MH - r) / step).  A work item is a column block (ATR_COLS columns), a residue class
// (there are min(step, MH) that hold a row) and a chunk of ATR_CHUNK consecutive t; item = (chunk * nres + r) * ncb + cb, so that
// items that follow each other work on neighbouring memory.  The last chunks of the shorter classes may be empty.  in, smooth,
// detail: the buffers' addresses as integers (0: null), each MH * MW floats.  Returns the message of a limit: MH or MW <= 0, step
// outside 1 .. ATR_STEP_MAX, no input, no output, an image of 2^31 pixels or more, or an output whose bytes overlap the input's or
// the other output's (buffers that touch do not overlap).  Integers only; sizes in 64-bit.
struct AtrousPlan {
    int ncb = 0;                        // column blocks: ceil(MW / ATR_COLS)
    int nres = 0;                       // residue classes with at least one row: min(step, MH)
    int nchunk = 0;                     // chunks of the longest class (r = 0): ceil(ceil(MH / step) / ATR_CHUNK)
    long long items = 0;                // ncb * nres * nchunk
    int grid = 0;                       // workgroups: min(items, ATR_GRID_MAX)
    long long bytes = 0;                // of one map: MH * MW * 4
};
const char* plan_atrous(int MH, int MW, int step, unsigned long long in, unsigned long long smooth, unsigned long long detail, AtrousPlan& p);

// cy_aperture_sums.  jobs: [n][3] {cx, cy, unit} in image pixels; factors: [K], finite, positive, strictly increasing.  Per job, all
// in float64 with every operation rounded on its own: r_k = factors[k] * unit, r2_k = r_k * r_k.  Status 1 when unit is not
// finite or <= 0, or r_K is not finite or above APER_RADIUS_MAX.  Otherwise the window is decided in double before any conversion
// to int: columns [ceil(cx - r_K), floor(cx + r_K)] clipped to [0, MW - 1], rows likewise with cy and MH; status 2 when the centre is
// not finite, a side misses the image or holds no pixel centre.  clipped: the unclipped window of a measured job leaves the image.
// have_map, have_jobs, have_out: whether the caller's pointers are non-null (they count only for n > 0; factors is read here and
// may be null only for n == 0).  Returns the message of the first failed check, in this order: MH or MW <= 0, an image of 2^31
// pixels or more, n outside [0, APER_JOBS_MAX], K outside [1, APER_RINGS_MAX], a null pointer, a bad factor table.
struct AperPlan { std::vector<AperJob> jobs; int measured = 0; };
const char* plan_apertures(const double* jobs, int n, const double* factors, int K, int MH, int MW, bool have_map, bool have_jobs,
                           bool have_out, AperPlan& p);

// cy_fit_peaks.  jobs: [n][PFIT_JOB_FIELDS] {cx, cy, R, bkg, sign, A, x0, y0, a, b, c}, positions in image pixels.  Per job, in
// float64 with every operation rounded on its own: status 1 when R is not finite, <= 0 or above PFIT_RADIUS_MAX, sign is not exactly
// +1 or -1, or bkg is not finite.  Otherwise the window is decided in double before any conversion to int: columns [ceil(cx - R),
// floor(cx + R)] clipped to [0, MW - 1], rows likewise with cy and MH; status 5 when the centre is not finite, a side misses the
// image or holds no pixel centre.  clipped: the unclipped window of a status 0 job leaves the image.  The neighbours of a status 0
// job e are the other status 0 jobs f with D2 = (cx_f - cx_e)^2 + (cy_f - cy_e)^2 < 4 * (R_e * R_e), ordered by (D2, f); the first
// PFIT_NEIGH_MAX are kept, crowded says that there were more.  They are found by a scan of the jobs sorted by column over the columns
// within 2 R_e, so the cost is the number of jobs in such a band, not n, per job.  run: the status 0 jobs in increasing index, one
// workgroup each.  have_map, have_out: whether the caller's pointers are non-null (they and `jobs` count only for n > 0).  Returns
// the message of the first failed check, in this order: MH or MW <= 0, an image of 2^31 pixels or more, n outside
// [0, PFIT_JOBS_MAX], max_iter outside [1, 256], a null pointer.
struct PeakFitPlan { std::vector<PeakFitJob> jobs; std::vector<int> run; };
const char* plan_peak_fits(const double* jobs, int n, int max_iter, int MH, int MW, bool have_map, bool have_out, PeakFitPlan& p);

// Row [PFIT_FIELDS] of cy_fit_peaks for job j.  A job the planner turned away (status 1 or 5, got == null): the status, the window
// as -1 and zeros elsewhere.  Otherwise `got` is the row the kernel wrote: taken over, with the window, clipped, nneigh and crowded
// of the plan, the centre back in image pixels, and for the kernel's status 3 or 4 the start exactly as given in `job`
// ([PFIT_JOB_FIELDS]).
void peak_fit_row(const PeakFitJob& j, const double* job, const double* got, double* row);

// Row [DRES_FIELDS] of cy_disc_residuals for job j of plan_peak_fits, which that entry reuses as it stands (max_iter 1; the start of a
// job is planned and ignored).  A job the planner turned away (status 1 or 5, got == null): the status, the window and the
// position of the largest |r| as -1 and zeros elsewhere.  Otherwise `got` is the row the kernel wrote: taken over, with the window,
// clipped and nneigh of the plan.
void disc_residual_row(const PeakFitJob& j, const double* got, double* row);

// cy_forced_fit.  jobs: [n][FORCED_JOB_FIELDS] {x0, y0, a, b, c, bkg}, positions in image pixels.  Per job: status 1 when one of the
// six fields is not finite or the shape is not admissible, otherwise the status and rectangle of support_rect (0, 2 or 3).  run: the
// jobs of status 0 and 2 in increasing index, one workgroup each.  The NEIGHBOURS of a run job e are the other run jobs f whose
// rectangle intersects e's (both clipped to the image), ordered by (D2, f) with D2 = dx*dx + dy*dy of the centres, every operation
// rounded on its own.  Walking that order: a candidate whose x0, y0, a, b, c compare equal to e's or to those of a neighbour kept
// before it is dropped and counted in ndup; otherwise it is kept while fewer than FORCED_NEIGH_MAX are, and sets crowded when they
// are full.  Candidates come from the scan of the run jobs sorted by column (scan_band) over |cx_f - cx_e| < hx_e + hmax + 3, hmax
// the largest half-width of a run job: the cost per job is the number of jobs in such a band, not n.  have_map, have_out: whether
// the caller's pointers are non-null.  Returns the message of the first failed check, in this order: a null map; MH or MW <= 0; an
// image of 2^31 pixels or more; nsigma outside [1, 8] or NaN; fit_bkg not 0 or 1; n outside [0, FORCED_JOBS_MAX]; with n > 0 a null
// jobs or out pointer.
struct ForcedPlan { std::vector<ForcedJob> jobs; std::vector<int> run; };
const char* plan_forced(const double* jobs, int n, double nsigma, int fit_bkg, int MH, int MW, bool have_map, bool have_out, ForcedPlan& p);

// Row [FORCED_FIELDS] of cy_forced_fit for job j.  A job the planner turned away (status 1 or 3, got == null): the status, the
// window (fields 17 .. 20) as -1 and zeros elsewhere.  Otherwise `got` is the row the kernel wrote: taken over, with K, nneigh,
// crowded, ndup, the window and capped of the plan.
void forced_row(const ForcedJob& j, int fit_bkg, const double* got, double* row);

// cy_fit_peak_groups.  jobs as for plan_peak_fits, whose statuses (1 / 5), windows, clipped flags and kept-neighbour lists are taken
// over (p.fits).  Two status 0 jobs e, f with equal sign are LINKED when D2 < Lm * Lm, Lm = link * max(R_e, R_f), D2 formed as
// plan_peak_fits forms it; strict, symmetric, coincident centres are linked.  A pair is looked for from the side of its larger
// radius (from the lower index when the radii are equal), in the stretch of the jobs sorted by column whose |cx_f - cx_e| is
// below link * R_e, found by bisection: the cost per job is the number of jobs in such a band, not n.  A GROUP is a connected set
// of the link graph (union-find); its id is its lowest job index, its members are taken in increasing job index (slot).  Per job:
// group, size (members of its group), slot, nlinked (jobs directly linked to it) and status: 1 / 5 the planner's, 6 alone, 7 in a
// group above BLEND_MAX_MEMBERS, 0 member of a group job.  groups: one PeakGroupJob per group with 2 .. BLEND_MAX_MEMBERS members,
// in increasing id: the bounding box of the members' windows, per member its kept neighbours that are not members (indices, in
// its own order), the starts relative to the group window, bkg and sign of slot 0.  job_of: [n] index into groups, -1 without one.
// rows: [n][PGRP_FIELDS] what the host decides for every job: status 1 / 5 as peak_fit_row writes them (the window, fields 36 ..
// 39, as -1); otherwise group, size and slot in fields 5 .. 7, the window of the group (the job's own for status 6), clipped (any
// member's), nlinked, and for status 7 the start as given in fields 8 .. 13.  Returns the message of the first failed check, in
// this order: those of plan_peak_fits up to max_iter, link not finite, <= 0 or > 2, a null pointer.
struct PeakGroupPlan {
    PeakFitPlan fits;
    std::vector<int> group, size, slot, nlinked, status, job_of;
    std::vector<PeakGroupJob> groups;
    std::vector<double> rows;
};
const char* plan_peak_groups(const double* jobs, int n, double link, int max_iter, int MH, int MW, bool have_map, bool have_out, PeakGroupPlan& p);

// The rows of the members of every group job from the device's table `got` ([groups][BLEND_MAX_MEMBERS][PGRP_FIELDS]) into `out`
// ([n][PGRP_FIELDS], already holding p.rows): fields 0 .. 35 and nexcluded taken over, the centre back in image pixels; a row that
// was not fitted (status 3, 4) reports its start exactly as given in `jobs`.
void peak_group_rows(const PeakGroupPlan& p, const double* jobs, const double* got, double* out);

// Rows `rows[0 .. nrows)` of one job (source = row / DBL_MAX_COMP) from the device's table `got` into `out`, both [..][width]: the
// centre (fields par + 1, par + 2) back in image pixels; a row that was not fitted (status 3, 4) reports its start exactly as given.
void write_back(const double* got, const double* start, const int* win0, int width, int par, const int* rows, int nrows, double* out);

}  // namespace cy
