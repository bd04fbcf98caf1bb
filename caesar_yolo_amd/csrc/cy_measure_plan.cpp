// Host-side planning of the measurement entries (see cy_measure_plan.h).
#include "cy_measure_plan.h"
#include <algorithm>
#include <cmath>

namespace cy {

namespace {
const char* const MASK_OFF_MSG = "h_mask_off disagrees with the areas of the box windows";

// Inclusive integer window [max(0, ceil(lo)), min(N - 1, floor(hi))] of a float64 box side; empty (first > last) when the side
// misses the image or holds no pixel centre.  A NaN edge makes it empty.
void window_1d(double lo, double hi, int N, int* first, int* last) {
    *first = 0; *last = -1;
    if (std::isnan(lo) || std::isnan(hi)) return;
    const double c = std::ceil(lo), f = std::floor(hi);
    if (c > (double)(N - 1) || f < 0.0) return;
    *first = c > 0.0 ? (int)c : 0;
    *last = f < (double)(N - 1) ? (int)f : N - 1;
}

// One source of the mask walk: its window, its bytes and whether its pixels are collected (a window above FIT_MAX_AREA is only checked)
struct MaskSource { int i, nc; BoxWindow w; long long W; const unsigned char* m; bool collect; };

// The pass over the mask bytes that the fit and the blend planner share.  Per source, in this order: ncomp in range, the window,
// its claimed offsets, then every byte (17 .. 254 is no component, no 255).  pixel(s, q, x, k) gets every collected pixel of a
// component k < ncomp in increasing window index q (x: its column); done(s) closes the source.
template <class Pixel, class Done>
const char* walk_masks(const FitInputs& in, std::vector<int>& win0, Pixel&& pixel, Done&& done) {
    win0.assign((size_t)in.n * 2, 0);
    long long nmask = 0;
    for (int i = 0; i < in.n; ++i) {
        MaskSource s;
        s.i = i; s.nc = in.ncomp[i];
        if (s.nc < 0 || s.nc > DBL_MAX_COMP) return "h_ncomp outside 0 .. CY_DBL_MAX_COMP";
        s.w = box_window(in.boxes + (size_t)i * 4, in.MH, in.MW);
        if (in.mask_off[i] != nmask || in.mask_off[i + 1] != nmask + s.w.area) return MASK_OFF_MSG;
        win0[(size_t)i * 2] = s.w.x0; win0[(size_t)i * 2 + 1] = s.w.y0;
        s.m = in.mask + nmask;
        nmask += s.w.area;
        s.collect = s.w.area <= FIT_MAX_AREA;
        s.W = (long long)s.w.x1 - s.w.x0 + 1;
        long long x = 0;
        for (long long q = 0; q < s.w.area; ++q, ++x) {
            if (x == s.W) x = 0;
            if (s.m[q] > DBL_MAX_COMP && s.m[q] != 255) return "mask byte in 17 .. 254";
            const int k = (int)s.m[q] - 1;
            if (s.collect && k >= 0 && k < s.nc) pixel(s, q, x, k);
        }
        done(s);
    }
    return nullptr;
}

// start of component k of source i with the centre relative to the window's first pixel
void relative_start(const FitInputs& in, const MaskSource& s, int k, double* p0) {
    const double* p = in.start + ((size_t)s.i * DBL_MAX_COMP + k) * 6;
    for (int t = 0; t < 6; ++t) p0[t] = p[t];
    p0[1] = p[1] - (double)s.w.x0; p0[2] = p[2] - (double)s.w.y0;
}
}  // namespace

BoxWindow box_window(const double* b, int MH, int MW) {
    BoxWindow w;
    window_1d(b[0], b[2], MW, &w.x0, &w.x1);
    window_1d(b[1], b[3], MH, &w.y0, &w.y1);
    if (w.x1 < w.x0 || w.y1 < w.y0) { w.x0 = w.y0 = 0; w.x1 = w.y1 = -1; }        // empty in one axis = empty
    w.area = w.x1 < w.x0 ? 0 : (long long)(w.x1 - w.x0 + 1) * (w.y1 - w.y0 + 1);
    return w;
}

std::vector<int> ring_windows(const double* boxes, int n, int ring, int MH, int MW) {
    std::vector<int> win((size_t)n * 8);
    const long long rg = ring;
    for (int i = 0; i < n; ++i) {
        const BoxWindow b = box_window(boxes + (size_t)i * 4, MH, MW);
        int* w = &win[(size_t)i * 8];
        w[0] = b.x0; w[1] = b.x1; w[2] = b.y0; w[3] = b.y1;
        // the ring's outer window: the box window grown by `ring`, clipped to the image (an empty box window has no ring)
        w[4] = (int)std::max(0LL, w[0] - rg); w[5] = (int)std::min((long long)MW - 1, w[1] + rg);
        w[6] = (int)std::max(0LL, w[2] - rg); w[7] = (int)std::min((long long)MH - 1, w[3] + rg);
    }
    return win;
}

const char* plan_islands(const double* boxes, const double* thr, int thr_stride, const long long* mask_off, int n, int MH, int MW, IslandTable& t) {
    t.win.assign((size_t)n * 4, 0);
    t.off.assign((size_t)n * 2, 0);
    t.nws = t.nmask = 0;
    for (int i = 0; i < n; ++i) {
        if (thr[(size_t)i * thr_stride] < thr[(size_t)i * thr_stride + 1]) return "seed_thr below merge_thr";
        const BoxWindow b = box_window(boxes + (size_t)i * 4, MH, MW);
        int* w = &t.win[(size_t)i * 4];
        w[0] = b.x0; w[1] = b.x1; w[2] = b.y0; w[3] = b.y1;
        if (mask_off && (mask_off[i] != t.nmask || mask_off[i + 1] != t.nmask + b.area)) return MASK_OFF_MSG;
        t.off[(size_t)i * 2] = b.area > ISL_MAX_AREA ? ISL_OFF_TOO_LARGE : b.area > ISL_LDS_MAX ? t.nws : ISL_OFF_LDS;
        t.off[(size_t)i * 2 + 1] = t.nmask;
        if (b.area > ISL_LDS_MAX && b.area <= ISL_MAX_AREA) t.nws += b.area;
        t.nmask += b.area;
    }
    return nullptr;
}

const char* plan_fit(const FitInputs& in, FitPlan& p) {
    p.jobs.clear(); p.list.clear();
    p.large.assign((size_t)in.n, 0);
    std::vector<unsigned> per[DBL_MAX_COMP];                  // the pixels of the current source, by component
    return walk_masks(in, p.win0,
        [&](const MaskSource&, long long q, long long, int k) { per[k].push_back((unsigned)q); },
        [&](const MaskSource& s) {
            if (!s.collect) { p.large[s.i] = 1; return; }
            for (int k = 0; k < s.nc; ++k) {
                FitJob j{};
                j.list_off = (long long)p.list.size(); j.npos = (unsigned)per[k].size();
                j.x0 = s.w.x0; j.y0 = s.w.y0; j.W = (unsigned)s.W; j.A = (unsigned)s.w.area;
                j.row = s.i * DBL_MAX_COMP + k; j.bkg = in.bkg[s.i];
                relative_start(in, s, k, j.p0);
                if (s.w.area == 0) { j.x0 = j.y0 = 0; j.W = 1; j.A = 1; }       // an empty window has no pixel: a job without a list entry
                p.list.insert(p.list.end(), per[k].begin(), per[k].end());
                p.jobs.push_back(j);
                per[k].clear();
            }
        });
}

const char* plan_blend(const FitInputs& in, BlendPlan& p) {
    // per source: the member pixels in increasing window index and the 16 x 16 adjacency bits; from them the groups by union-find,
    // then the source's jobs and every job's list, dealt out from the collected pixels in the same order
    struct Px { unsigned q; int k; };
    p.jobs.clear(); p.list.clear();
    p.rows.assign((size_t)in.n * DBL_MAX_COMP * BLEND_FIELDS, 0.0);
    std::vector<Px> px;
    std::vector<unsigned> per[DBL_MAX_COMP / 2];              // a source has at most DBL_MAX_COMP / 2 jobs (two members each)
    unsigned adj[DBL_MAX_COMP] = {};
    return walk_masks(in, p.win0,
        [&](const MaskSource& s, long long q, long long x, int k) {
            px.push_back(Px{(unsigned)q, k});
            // the four neighbours already passed (left, and the three of the row above); the other four see this pixel from theirs
            const long long W = s.W;
            const long long nb[4] = {x > 0 ? q - 1 : -1, q >= W && x > 0 ? q - W - 1 : -1, q >= W ? q - W : -1, q >= W && x + 1 < W ? q - W + 1 : -1};
            for (int t = 0; t < 4; ++t) {
                if (nb[t] < 0) continue;
                const int l = (int)s.m[nb[t]] - 1;
                if (l >= 0 && l < s.nc && l != k) { adj[k] |= 1u << l; adj[l] |= 1u << k; }
            }
        },
        [&](const MaskSource& s) {
            const int nc = s.nc;
            double* srow = &p.rows[(size_t)s.i * DBL_MAX_COMP * BLEND_FIELDS];
            if (!s.collect) {
                for (int k = 0; k < nc; ++k) srow[(size_t)k * BLEND_FIELDS] = 1.0;
                return;
            }
            int root[DBL_MAX_COMP];
            for (int k = 0; k < nc; ++k) root[k] = k;
            auto find = [&](int k) { while (root[k] != k) k = root[k] = root[root[k]]; return k; };
            for (int k = 0; k < nc; ++k)
                for (int l = k + 1; l < nc; ++l)
                    if (adj[k] >> l & 1u) {
                        const int a = find(k), b = find(l);
                        if (a != b) root[std::max(a, b)] = std::min(a, b);       // the root of a group is its lowest member
                    }
            int slot[DBL_MAX_COMP], size[DBL_MAX_COMP] = {}, job_of[DBL_MAX_COMP];
            for (int k = 0; k < nc; ++k) { root[k] = find(k); slot[k] = size[root[k]]++; job_of[k] = -1; }
            const size_t first_job = p.jobs.size();
            for (int k = 0; k < nc; ++k) {
                const int g = root[k], M = size[g];
                double* o = srow + (size_t)k * BLEND_FIELDS;
                o[5] = (double)g; o[6] = (double)M; o[7] = (double)slot[k];
                if (M == 1) { o[0] = 6.0; continue; }
                if (M > BLEND_MAX_MEMBERS) {
                    o[0] = 5.0;
                    const double* st = in.start + ((size_t)s.i * DBL_MAX_COMP + k) * 6;
                    for (int t = 0; t < 6; ++t) o[8 + t] = st[t];
                    continue;
                }
                if (k == g) {
                    BlendJob j{};
                    j.x0 = s.w.x0; j.y0 = s.w.y0; j.W = (unsigned)s.W; j.A = (unsigned)s.w.area;
                    j.row0 = s.i * DBL_MAX_COMP; j.M = M; j.bkg = in.bkg[s.i];
                    job_of[g] = (int)(p.jobs.size() - first_job);
                    p.jobs.push_back(j);
                }
                BlendJob& j = p.jobs[first_job + job_of[g]];
                j.comp[slot[k]] = k;
                relative_start(in, s, k, j.p0 + 6 * slot[k]);
            }
            const size_t njob = p.jobs.size() - first_job;
            for (const Px& e : px)
                if (job_of[root[e.k]] >= 0) per[job_of[root[e.k]]].push_back(e.q);
            for (size_t t = 0; t < njob; ++t) {
                BlendJob& j = p.jobs[first_job + t];
                j.list_off = (long long)p.list.size(); j.npos = (unsigned)per[t].size();
                p.list.insert(p.list.end(), per[t].begin(), per[t].end());
                per[t].clear();
            }
            px.clear();
            std::fill(adj, adj + DBL_MAX_COMP, 0u);
        });
}

int support_rect(const double* q, double nsigma, int MH, int MW, int* r, double* hx_out) {
#pragma clang fp contract(off)          // a*c - b*b: both products are rounded before the subtraction, whatever the build's default
    // one side of a rectangle: [max(0, floor(c0) - h), min(N - 1, floor(c0) + 1 + h)], compared in double; false when it misses
    auto side = [](double c0, double h, int N, int* lo, int* hi) {
        const double f = std::floor(c0), l = f - h, u = (f + 1.0) + h;
        if (u < 0.0 || l > (double)(N - 1)) return false;
        *lo = l > 0.0 ? (int)l : 0;
        *hi = u < (double)(N - 1) ? (int)u : N - 1;
        return true;
    };
    r[0] = r[2] = 0; r[1] = r[3] = -1;
    bool fin = true;
    for (int t = 0; t < 5; ++t) fin = fin && std::isfinite(q[t]);
    const double a = q[2], b = q[3], c = q[4];
    const double ac = a * c, bb = b * b;
    const double det = ac - bb;
    if (!(fin && a > 0.0 && c > 0.0 && det > 0.0)) return 1;
    double hx = std::ceil(nsigma * std::sqrt(c / det)), hy = std::ceil(nsigma * std::sqrt(a / det));
    bool capped = false;
    if (!(hx <= (double)RND_HALF_MAX)) { hx = (double)RND_HALF_MAX; capped = true; }      // a half-width that is not finite is above the cap
    if (!(hy <= (double)RND_HALF_MAX)) { hy = (double)RND_HALF_MAX; capped = true; }
    if (hx_out) *hx_out = hx;
    if (!side(q[0], hx, MW, &r[0], &r[1]) || !side(q[1], hy, MH, &r[2], &r[3])) {
        r[0] = r[2] = 0; r[1] = r[3] = -1;
        return 3;
    }
    return capped ? 2 : 0;
}

const char* plan_render(const double* comp, int m, double nsigma, int MH, int MW, RenderPlan& p, bool signed_amp) {
    p.rows.clear(); p.rect.clear(); p.tile_off.clear(); p.tile_list.clear();
    p.ntx = (MW + RND_TILE - 1) / RND_TILE; p.nty = (MH + RND_TILE - 1) / RND_TILE;
    if (m < 0 || m > RND_MAX_COMP) return "m outside 0 .. 2^20";
    p.rows.assign((size_t)m * RND_FIELDS, 0.0);
    p.rect.assign((size_t)m * 4, 0);
    const size_t ntiles = (size_t)p.ntx * p.nty;
    p.tile_off.assign(ntiles + 1, 0);
    long long total = 0;
    for (int k = 0; k < m; ++k) {
        const double* q = comp + (size_t)k * 6;
        double* row = &p.rows[(size_t)k * RND_FIELDS];
        int* r = &p.rect[(size_t)k * 4];
        r[0] = r[2] = 0; r[1] = r[3] = -1;
        row[1] = row[2] = row[3] = row[4] = -1.0;
        const bool amp = std::isfinite(q[0]) && (signed_amp ? q[0] != 0.0 : q[0] > 0.0);
        const int st = amp ? support_rect(q + 1, nsigma, MH, MW, r) : 1;
        row[0] = (double)st;
        if (st == 1 || st == 3) continue;
        for (int t = 0; t < 4; ++t) row[1 + t] = (double)r[t];
        const int tx0 = r[0] / RND_TILE, tx1 = r[1] / RND_TILE, ty0 = r[2] / RND_TILE, ty1 = r[3] / RND_TILE;
        row[5] = (double)((long long)(tx1 - tx0 + 1) * (ty1 - ty0 + 1));
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx) ++p.tile_off[(size_t)ty * p.ntx + tx + 1];
        total += (long long)row[5];
        if (total > RND_MAX_LIST) return "tile table above 2^27 entries";
    }
    for (size_t t = 0; t < ntiles; ++t) p.tile_off[t + 1] += p.tile_off[t];
    p.tile_list.assign((size_t)total, 0);
    std::vector<int> next(p.tile_off.begin(), p.tile_off.end() - 1);
    for (int k = 0; k < m; ++k) {                             // increasing k: every tile's list comes out in increasing index
        const int* r = &p.rect[(size_t)k * 4];
        if (r[1] < r[0]) continue;
        for (int ty = r[2] / RND_TILE; ty <= r[3] / RND_TILE; ++ty)
            for (int tx = r[0] / RND_TILE; tx <= r[1] / RND_TILE; ++tx) p.tile_list[(size_t)next[(size_t)ty * p.ntx + tx]++] = k;
    }
    return nullptr;
}

const char* plan_residuals(const double* boxes, const long long* mask_off, int n, int MH, int MW, IslandTable& t) {
    static const double no_thr[2] = {0.0, 0.0};               // plan_islands' windows and offsets; there is no threshold to check
    return plan_islands(boxes, no_thr, 0, mask_off, n, MH, MW, t);
}

const char* plan_peaks(int MH, int MW, int radius, int cap, PeakPlan& p) {
    p = PeakPlan();
    if ((long long)MH * MW >= (1LL << 31)) return "image of 2^31 pixels or more (32-bit pixel indices and peak counts)";
    p.nsx = (int)(((long long)MW + PEAK_SEG - 1) / PEAK_SEG);
    // the kernels hold columns in int: the last column a thread of the last segment names, plus the radius, has to fit
    if ((long long)p.nsx * PEAK_SEG + radius > 2147483647LL) return "row too wide (its last segment ends beyond column 2^31 - 1 - radius)";
    p.nseg = (long long)MH * p.nsx;
    if (p.nseg > PEAK_MAX_SEG) return "segment table above 2^24 entries";
    p.words = p.nseg * PEAK_SEG_WORDS;
    p.row_values = (long long)cap * PEAK_FIELDS;
    return nullptr;
}

const char* plan_atrous(int MH, int MW, int step, unsigned long long in, unsigned long long smooth, unsigned long long detail, AtrousPlan& p) {
    p = AtrousPlan();
    if (MH <= 0 || MW <= 0) return "MH, MW > 0 required";
    if (step < 1 || step > ATR_STEP_MAX) return "step outside 1 .. CY_ATROUS_STEP_MAX";
    if (!in) return "null argument";
    if (!smooth && !detail) return "d_smooth and d_detail are both null";
    const long long px = (long long)MH * MW;
    if (px >= (1LL << 31)) return "image of 2^31 pixels or more";
    p.bytes = px * 4;
    // [a, a + bytes) and [b, b + bytes) share a byte; an address so high that its range would wrap is no buffer
    const unsigned long long bytes = (unsigned long long)p.bytes;
    auto wraps = [&](unsigned long long a) { return a > ~0ULL - bytes; };
    auto overlap = [&](unsigned long long a, unsigned long long b) { return a && b && a < b + bytes && b < a + bytes; };
    if (wraps(in) || wraps(smooth) || wraps(detail)) return "buffer beyond the address range";
    if (overlap(in, smooth) || overlap(in, detail)) return "an output overlaps the input";
    if (overlap(smooth, detail)) return "d_smooth overlaps d_detail";
    p.ncb = (int)(((long long)MW + ATR_COLS - 1) / ATR_COLS);
    p.nres = step < MH ? step : MH;
    const long long rows0 = ((long long)MH + step - 1) / step;                // rows of class 0, the longest
    p.nchunk = (int)((rows0 + ATR_CHUNK - 1) / ATR_CHUNK);
    p.items = (long long)p.ncb * p.nres * p.nchunk;
    if (p.items > 2147483647LL) return "work item table above 2^31 - 1 entries";       // not reachable below 2^31 pixels: (MW / 256 + 1) (MH / 64 + 64)
    p.grid = (int)(p.items < ATR_GRID_MAX ? p.items : ATR_GRID_MAX);
    return nullptr;
}

const char* plan_apertures(const double* jobs, int n, const double* factors, int K, int MH, int MW, bool have_map, bool have_jobs,
                           bool have_out, AperPlan& p) {
    p = AperPlan();
    if (MH <= 0 || MW <= 0) return "MH, MW > 0 required";
    if ((long long)MH * MW >= (1LL << 31)) return "image of 2^31 pixels or more";
    if (n < 0 || n > APER_JOBS_MAX) return "n outside 0 .. CY_APER_JOBS_MAX";
    if (K < 1 || K > APER_RINGS_MAX) return "K outside 1 .. CY_APER_RINGS_MAX";
    if (n > 0 && !(have_map && have_jobs && have_out && factors)) return "null argument";
    for (int k = 0; factors && k < K; ++k)
        if (!std::isfinite(factors[k]) || !(factors[k] > 0.0) || (k > 0 && !(factors[k] > factors[k - 1])))
            return "factors must be finite, positive and strictly increasing";
    // one side of a window: [ceil(c - r), floor(c + r)] compared in double with the image, then clipped; false when it holds no pixel
    auto side = [](double c, double r, int N, int* lo, int* hi, int* clipped) {
        const double l = std::ceil(c - r), u = std::floor(c + r);
        if (u < 0.0 || l > (double)(N - 1) || l > u) return false;
        if (l < 0.0 || u > (double)(N - 1)) *clipped = 1;
        *lo = l > 0.0 ? (int)l : 0;
        *hi = u < (double)(N - 1) ? (int)u : N - 1;
        return true;
    };
    p.jobs.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        const double* q = jobs + (size_t)i * 3;
        AperJob& j = p.jobs[(size_t)i];
        j = AperJob();
        j.cx = q[0]; j.cy = q[1];
        j.x0 = j.y0 = 0; j.x1 = j.y1 = -1;
        const double unit = q[2], rK = factors[K - 1] * unit;
        if (!std::isfinite(unit) || !(unit > 0.0) || !std::isfinite(rK) || rK > (double)APER_RADIUS_MAX) { j.status = 1; continue; }
        int clipped = 0;
        if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !side(q[0], rK, MW, &j.x0, &j.x1, &clipped) ||
            !side(q[1], rK, MH, &j.y0, &j.y1, &clipped)) {
            j.x0 = j.y0 = 0; j.x1 = j.y1 = -1;
            j.status = 2;
            continue;
        }
        j.clipped = clipped;
        for (int k = 0; k < K; ++k) { const double r = factors[k] * unit; j.r2[k] = r * r; }
        ++p.measured;
    }
    return nullptr;
}

namespace {
// the checks of cy_fit_peaks that come before its pointers, in their order
const char* peak_fit_sizes(int n, int max_iter, int MH, int MW) {
    if (MH <= 0 || MW <= 0) return "MH, MW > 0 required";
    if ((long long)MH * MW >= (1LL << 31)) return "image of 2^31 pixels or more";
    if (n < 0 || n > PFIT_JOBS_MAX) return "n outside 0 .. CY_PFIT_JOBS_MAX";
    if (max_iter < 1 || max_iter > 256) return "max_iter outside 1 .. 256";
    return nullptr;
}

// the run jobs (PeakFitJob or ForcedJob: anything with a centre cx, cy) sorted by column (ties by index)
template <class Job>
std::vector<int> sorted_by_column(const std::vector<Job>& jobs, const std::vector<int>& run) {
    std::vector<int> by_x(run);
    std::sort(by_x.begin(), by_x.end(), [&](int a, int b) { return jobs[(size_t)a].cx < jobs[(size_t)b].cx || (jobs[(size_t)a].cx == jobs[(size_t)b].cx && a < b); });
    return by_x;
}
std::vector<int> sorted_by_column(const PeakFitPlan& p) { return sorted_by_column(p.jobs, p.run); }

// Job e = by_x[s] looks at the stretch of the sorted jobs whose |cx_f - cx_e| (as the test below rounds it) is below `band`:
// visit(f, D2) for every other job f in it, D2 = (cx_f - cx_e)^2 + (cy_f - cy_e)^2.  The stretch holds every f with D2 < band^2,
// because dx*dx <= D2 and rounding is monotonic
template <class Job, class Visit>
void scan_band(const std::vector<Job>& jobs, const std::vector<int>& by_x, size_t s, double band, Visit&& visit) {
#pragma clang fp contract(off)          // dx*dx + dy*dy: every product is rounded before it is used, whatever the build's default
    const size_t m = by_x.size();
    const int e = by_x[s];
    const Job& j = jobs[(size_t)e];
    // the band's left end by bisection on the sorted columns (it does not move monotonically when the radii differ)
    size_t lo = 0, hi = s;
    while (lo < hi) { const size_t mid = (lo + hi) / 2; if (j.cx - jobs[(size_t)by_x[mid]].cx < band) hi = mid; else lo = mid + 1; }
    for (size_t t = lo; t < m; ++t) {
        const int f = by_x[t];
        if (f == e) continue;
        const Job& g = jobs[(size_t)f];
        const double dx = g.cx - j.cx, dy = g.cy - j.cy;
        if (t > s && !(dx < band)) break;
        const double xx = dx * dx, yy = dy * dy;
        visit(f, xx + yy);
    }
}
}  // namespace

const char* plan_peak_fits(const double* jobs, int n, int max_iter, int MH, int MW, bool have_map, bool have_out, PeakFitPlan& p) {
#pragma clang fp contract(off)          // R*R: every product is rounded before it is used, whatever the build's default
    p = PeakFitPlan();
    if (const char* msg = peak_fit_sizes(n, max_iter, MH, MW)) return msg;
    if (n > 0 && !(have_map && jobs && have_out)) return "null argument";
    // one side of a window, as plan_apertures decides it
    auto side = [](double c, double r, int N, int* lo, int* hi, int* clipped) {
        const double l = std::ceil(c - r), u = std::floor(c + r);
        if (u < 0.0 || l > (double)(N - 1) || l > u) return false;
        if (l < 0.0 || u > (double)(N - 1)) *clipped = 1;
        *lo = l > 0.0 ? (int)l : 0;
        *hi = u < (double)(N - 1) ? (int)u : N - 1;
        return true;
    };
    p.jobs.resize((size_t)n);
    std::vector<double> lim((size_t)n, 0.0);                  // 2 R of the fitted jobs
    for (int i = 0; i < n; ++i) {
        const double* q = jobs + (size_t)i * PFIT_JOB_FIELDS;
        PeakFitJob& j = p.jobs[(size_t)i];
        j = PeakFitJob();
        j.cx = q[0]; j.cy = q[1]; j.bkg = q[3]; j.sign = q[4];
        j.x0 = j.y0 = 0; j.x1 = j.y1 = -1;
        for (int k = 0; k < PFIT_NEIGH_MAX; ++k) j.neigh[k] = -1;
        const double R = q[2];
        if (!std::isfinite(R) || !(R > 0.0) || R > (double)PFIT_RADIUS_MAX || !(q[4] == 1.0 || q[4] == -1.0) || !std::isfinite(q[3])) { j.status = 1; continue; }
        int clipped = 0;
        if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !side(q[0], R, MW, &j.x0, &j.x1, &clipped) || !side(q[1], R, MH, &j.y0, &j.y1, &clipped)) {
            j.x0 = j.y0 = 0; j.x1 = j.y1 = -1;
            j.status = 5;
            continue;
        }
        j.clipped = clipped;
        j.r2 = R * R;
        for (int t = 0; t < 6; ++t) j.p0[t] = q[5 + t];
        j.p0[1] = q[6] - (double)j.x0; j.p0[2] = q[7] - (double)j.y0;
        lim[(size_t)i] = 2.0 * R;
        p.run.push_back(i);
    }
    // neighbours: the fitted jobs sorted by column; job e looks at the stretch within 2 R_e, which holds every f with D2 < 4 R_e^2
    const std::vector<int> by_x = sorted_by_column(p);
    const size_t m = by_x.size();
    std::vector<std::pair<double, int>> cand;
    for (size_t s = 0; s < m; ++s) {
        const int e = by_x[s];
        PeakFitJob& j = p.jobs[(size_t)e];
        const double limit = 4.0 * j.r2;
        cand.clear();
        scan_band(p.jobs, by_x, s, lim[(size_t)e], [&](int f, double D2) { if (D2 < limit) cand.emplace_back(D2, f); });
        const size_t keep = std::min<size_t>(cand.size(), (size_t)PFIT_NEIGH_MAX);
        std::partial_sort(cand.begin(), cand.begin() + (long)keep, cand.end());
        j.nneigh = (int)keep; j.crowded = cand.size() > (size_t)PFIT_NEIGH_MAX ? 1 : 0;
        for (size_t k = 0; k < keep; ++k) j.neigh[k] = cand[k].second;
    }
    return nullptr;
}

void peak_fit_row(const PeakFitJob& j, const double* job, const double* got, double* row) {
    for (int f = 0; f < PFIT_FIELDS; ++f) row[f] = 0.0;
    if (!got) {
        row[0] = (double)j.status;
        row[32] = row[33] = row[34] = row[35] = -1.0;
        return;
    }
    for (int f = 0; f < PFIT_FIELDS; ++f) row[f] = got[f];
    if (got[0] == 3.0 || got[0] == 4.0) {
        for (int f = 0; f < 6; ++f) row[5 + f] = job[5 + f];
    } else {
        row[6] = got[6] + (double)j.x0; row[7] = got[7] + (double)j.y0;
    }
    row[32] = (double)j.x0; row[33] = (double)j.x1; row[34] = (double)j.y0; row[35] = (double)j.y1;
    row[36] = (double)j.clipped; row[37] = (double)j.nneigh; row[38] = (double)j.crowded;
}

void disc_residual_row(const PeakFitJob& j, const double* got, double* row) {
    for (int f = 0; f < DRES_FIELDS; ++f) row[f] = 0.0;
    if (!got) {
        row[0] = (double)j.status;
        row[6] = row[7] = -1.0;
        row[10] = row[11] = row[12] = row[13] = -1.0;
        return;
    }
    for (int f = 0; f < DRES_FIELDS; ++f) row[f] = got[f];
    row[10] = (double)j.x0; row[11] = (double)j.x1; row[12] = (double)j.y0; row[13] = (double)j.y1;
    row[14] = (double)j.clipped; row[15] = (double)j.nneigh;
}

const char* plan_forced(const double* jobs, int n, double nsigma, int fit_bkg, int MH, int MW, bool have_map, bool have_out, ForcedPlan& p) {
    p = ForcedPlan();
    if (!have_map) return "null argument";
    if (MH <= 0 || MW <= 0) return "MH, MW > 0 required";
    if ((long long)MH * MW >= (1LL << 31)) return "image of 2^31 pixels or more";
    if (!(nsigma >= 1.0 && nsigma <= 8.0)) return "nsigma outside [1, 8]";
    if (fit_bkg != 0 && fit_bkg != 1) return "fit_bkg must be 0 or 1";
    if (n < 0 || n > FORCED_JOBS_MAX) return "n outside 0 .. CY_FORCED_JOBS_MAX";
    if (n > 0 && !(jobs && have_out)) return "null argument";
    p.jobs.resize((size_t)n);
    std::vector<double> half((size_t)n, 0.0);                 // hx of the run jobs
    double hmax = 0.0;
    for (int i = 0; i < n; ++i) {
        const double* q = jobs + (size_t)i * FORCED_JOB_FIELDS;
        ForcedJob& j = p.jobs[(size_t)i];
        j = ForcedJob();
        j.cx = q[0]; j.cy = q[1]; j.a = q[2]; j.b = q[3]; j.c = q[4]; j.bkg = q[5];
        for (int k = 0; k < FORCED_NEIGH_MAX; ++k) j.neigh[k] = -1;
        int r[4] = {0, -1, 0, -1};
        j.status = std::isfinite(q[5]) ? support_rect(q, nsigma, MH, MW, r, &half[(size_t)i]) : 1;
        j.x0 = r[0]; j.x1 = r[1]; j.y0 = r[2]; j.y1 = r[3];
        if (j.status == 1 || j.status == 3) continue;
        hmax = std::max(hmax, half[(size_t)i]);
        p.run.push_back(i);
    }
    // neighbours: the run jobs sorted by column.  The rectangles of e and f share a column only when |floor(cx_e) - floor(cx_f)| <=
    // hx_e + hx_f + 1, so |cx_f - cx_e| < hx_e + hmax + 2 as a real number and <= that once rounded: the band is one wider
    const std::vector<int> by_x = sorted_by_column(p.jobs, p.run);
    auto same = [](const ForcedJob& u, const ForcedJob& v) { return u.cx == v.cx && u.cy == v.cy && u.a == v.a && u.b == v.b && u.c == v.c; };
    std::vector<std::pair<double, int>> cand;
    for (size_t s = 0; s < by_x.size(); ++s) {
        const int e = by_x[s];
        ForcedJob& j = p.jobs[(size_t)e];
        cand.clear();
        scan_band(p.jobs, by_x, s, half[(size_t)e] + hmax + 3.0, [&](int f, double D2) {
            const ForcedJob& g = p.jobs[(size_t)f];
            if (g.x0 <= j.x1 && j.x0 <= g.x1 && g.y0 <= j.y1 && j.y0 <= g.y1) cand.emplace_back(D2, f);
        });
        std::partial_sort(cand.begin(), cand.end(), cand.end());      // all of them: a duplicate is dropped wherever it stands in the order
        for (const std::pair<double, int>& cd : cand) {
            const ForcedJob& g = p.jobs[(size_t)cd.second];
            bool dup = same(g, j);
            for (int k = 0; k < j.nneigh && !dup; ++k) dup = same(g, p.jobs[(size_t)j.neigh[k]]);
            if (dup) ++j.ndup;
            else if (j.nneigh < FORCED_NEIGH_MAX) j.neigh[j.nneigh++] = cd.second;
            else j.crowded = 1;
        }
    }
    return nullptr;
}

void forced_row(const ForcedJob& j, int fit_bkg, const double* got, double* row) {
    for (int f = 0; f < FORCED_FIELDS; ++f) row[f] = 0.0;
    if (!got) {
        row[0] = (double)j.status;
        row[17] = row[18] = row[19] = row[20] = -1.0;
        return;
    }
    for (int f = 0; f < FORCED_FIELDS; ++f) row[f] = got[f];
    row[3] = (double)(1 + j.nneigh + fit_bkg); row[4] = (double)j.nneigh; row[5] = (double)j.crowded; row[6] = (double)j.ndup;
    row[17] = (double)j.x0; row[18] = (double)j.x1; row[19] = (double)j.y0; row[20] = (double)j.y1;
    row[21] = j.status == 2 ? 1.0 : 0.0;
}

const char* plan_peak_groups(const double* jobs, int n, double link, int max_iter, int MH, int MW, bool have_map, bool have_out, PeakGroupPlan& p) {
#pragma clang fp contract(off)          // link * R and Lm * Lm: every product is rounded before it is used, whatever the build's default
    p = PeakGroupPlan();
    if (const char* msg = peak_fit_sizes(n, max_iter, MH, MW)) return msg;
    if (!std::isfinite(link) || !(link > 0.0) || link > 2.0) return "link outside (0, 2]";
    if (const char* msg = plan_peak_fits(jobs, n, max_iter, MH, MW, have_map, have_out, p.fits)) return msg;
    const std::vector<PeakFitJob>& J = p.fits.jobs;
    const size_t N = (size_t)n;
    p.group.assign(N, 0); p.size.assign(N, 0); p.slot.assign(N, 0); p.nlinked.assign(N, 0); p.status.assign(N, 0); p.job_of.assign(N, -1);
    p.rows.assign(N * PGRP_FIELDS, 0.0);
    std::vector<int>& root = p.group;
    for (int i = 0; i < n; ++i) root[(size_t)i] = i;
    auto find = [&](int k) { while (root[(size_t)k] != k) k = root[(size_t)k] = root[(size_t)root[(size_t)k]]; return k; };
    auto radius = [&](int i) { return jobs[(size_t)i * PFIT_JOB_FIELDS + 2]; };
    // links: a pair is found from the side of its larger radius, whose band link * R holds it
    const std::vector<int> by_x = sorted_by_column(p.fits);
    for (size_t s = 0; s < by_x.size(); ++s) {
        const int e = by_x[s];
        const double Re = radius(e), Lm = link * Re;
        const double Lm2 = Lm * Lm;
        scan_band(J, by_x, s, Lm, [&](int f, double D2) {
            const double Rf = radius(f);
            if (Rf > Re || (Rf == Re && f < e)) return;       // job f finds this pair
            if (J[(size_t)f].sign != J[(size_t)e].sign || !(D2 < Lm2)) return;
            ++p.nlinked[(size_t)e]; ++p.nlinked[(size_t)f];
            const int a = find(e), b = find(f);
            if (a != b) root[(size_t)std::max(a, b)] = std::min(a, b);           // the root of a group is its lowest member
        });
    }
    // groups, slots, statuses; the bounding box and the clipped flag of every group, kept at its root
    std::vector<int> box(N * 5, 0);
    for (int i = 0; i < n; ++i) {
        const PeakFitJob& j = J[(size_t)i];
        const int g = root[(size_t)i] = find(i);
        p.slot[(size_t)i] = p.size[(size_t)g]++;
        if (j.status != 0) continue;
        int* b = &box[(size_t)g * 5];
        if (g == i) { b[0] = j.x0; b[1] = j.x1; b[2] = j.y0; b[3] = j.y1; b[4] = j.clipped; }
        else { b[0] = std::min(b[0], j.x0); b[1] = std::max(b[1], j.x1); b[2] = std::min(b[2], j.y0); b[3] = std::max(b[3], j.y1); b[4] |= j.clipped; }
    }
    for (int i = 0; i < n; ++i) {
        const PeakFitJob& j = J[(size_t)i];
        const int g = root[(size_t)i], M = p.size[(size_t)i] = p.size[(size_t)g];   // g <= i: the root's size is final
        double* row = &p.rows[(size_t)i * PGRP_FIELDS];
        if (j.status != 0) {
            p.status[(size_t)i] = j.status;
            row[0] = (double)j.status; row[36] = row[37] = row[38] = row[39] = -1.0;
            continue;
        }
        const int st = p.status[(size_t)i] = M == 1 ? 6 : M > BLEND_MAX_MEMBERS ? 7 : 0;
        const int* b = &box[(size_t)g * 5];
        row[0] = (double)st; row[5] = (double)g; row[6] = (double)M; row[7] = (double)p.slot[(size_t)i];
        for (int t = 0; t < 4; ++t) row[36 + t] = (double)b[t];
        row[40] = (double)b[4]; row[42] = (double)p.nlinked[(size_t)i];
        const double* q = jobs + (size_t)i * PFIT_JOB_FIELDS;
        if (st == 7)
            for (int t = 0; t < 6; ++t) row[8 + t] = q[5 + t];
        if (st != 0) continue;
        if (g == i) {
            PeakGroupJob gj{};
            gj.M = M; gj.x0 = b[0]; gj.x1 = b[1]; gj.y0 = b[2]; gj.y1 = b[3]; gj.bkg = j.bkg; gj.sign = j.sign;
            for (int t = 0; t < BLEND_MAX_MEMBERS; ++t) {
                gj.member[t] = -1;
                for (int k = 0; k < PFIT_NEIGH_MAX; ++k) gj.out[t][k] = -1;
            }
            p.job_of[(size_t)g] = (int)p.groups.size();
            p.groups.push_back(gj);
        }
        const int at = p.job_of[(size_t)i] = p.job_of[(size_t)g];
        PeakGroupJob& gj = p.groups[(size_t)at];
        const int s = p.slot[(size_t)i];
        gj.member[s] = i;
        for (int k = 0; k < j.nneigh; ++k)
            if (root[(size_t)j.neigh[k]] != g) gj.out[s][gj.nout[s]++] = j.neigh[k];
        double* p0 = gj.p0 + 6 * s;
        for (int t = 0; t < 6; ++t) p0[t] = q[5 + t];
        p0[1] = q[6] - (double)gj.x0; p0[2] = q[7] - (double)gj.y0;
    }
    return nullptr;
}

void peak_group_rows(const PeakGroupPlan& p, const double* jobs, const double* got, double* out) {
    for (size_t t = 0; t < p.groups.size(); ++t) {
        const PeakGroupJob& g = p.groups[t];
        for (int s = 0; s < g.M; ++s) {
            const double* src = got + (t * BLEND_MAX_MEMBERS + (size_t)s) * PGRP_FIELDS;
            double* row = out + (size_t)g.member[s] * PGRP_FIELDS;
            for (int f = 0; f < BLEND_FIELDS; ++f) row[f] = src[f];
            row[41] = src[41];
            if (src[0] == 3.0 || src[0] == 4.0) {
                for (int f = 0; f < 6; ++f) row[8 + f] = jobs[(size_t)g.member[s] * PFIT_JOB_FIELDS + 5 + f];
            } else {
                row[9] = src[9] + (double)g.x0; row[10] = src[10] + (double)g.y0;
            }
        }
    }
}

void write_back(const double* got, const double* start, const int* win0, int width, int par, const int* rows, int nrows, double* out) {
    for (int r = 0; r < nrows; ++r) {
        const size_t row = (size_t)rows[r];
        const double* g = got + row * width;
        double* o = out + row * width;
        for (int f = 0; f < width; ++f) o[f] = g[f];
        if (g[0] == 3.0 || g[0] == 4.0) {
            for (int f = 0; f < 6; ++f) o[par + f] = start[row * 6 + f];
        } else {
            const int* w0 = win0 + row / DBL_MAX_COMP * 2;
            o[par + 1] = g[par + 1] + (double)w0[0]; o[par + 2] = g[par + 2] + (double)w0[1];
        }
    }
}

}  // namespace cy
