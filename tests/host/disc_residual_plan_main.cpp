// Stand-alone driver of the host side of cy_disc_residuals (caesar_yolo_amd/csrc/cy_measure_plan.cpp) for
// tests/test_disc_residual_plan_cpu.py, which builds it with the host sanitizers: no HIP, no GPU library.  It does what the entry
// does around its launch: plan_peak_fits with max_iter 1, a table of one row per planner-status-0 job in place of the kernel's, and
// disc_residual_row for every job.
//
//     disc_residual_plan_main MH MW N NULLS [COLS] < numbers
// NULLS: a string of the letters m, j, o naming the pointers that are passed as null ("-": none).  Without COLS, standard input holds N
// jobs of eleven numbers (cx cy R bkg sign A x0 y0 a b c), as C99 hexadecimal floats or "nan" / "inf" / "-inf"; with a negative or
// oversize N nothing is read.  With COLS nothing is read and job i is made here: a lattice of COLS columns with 3 pixels between
// neighbours, cx = 3 (i % COLS) + 0.25, cy = 3 (i / COLS) + 0.5, R = 2, bkg = i, sign +1 (-1 for odd i); every 7th job has R = 0
// (status 1) and every 11th a centre of 1e300 (status 5).
// The stand-in for the kernel's row t (the t-th status 0 job) holds 1000 t + f + 0.5 in field f.
// Prints "error <message>", or "ok <measured>" and then
//     without COLS  one line per job: the CY_DRES_FIELDS numbers of its row as hexadecimal floats
//     with COLS     "counts <status 0> <status 1> <status 5>", "sums <nneigh> <widths> <heights> <clipped>" over the rows, the number of
//                   rows whose fields 0 .. 9 are not what the stand-in (or the turned-away rule) says, and the rows of jobs 0, 1, COLS
//                   and N - 1
#include "../../caesar_yolo_amd/csrc/cy_measure_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace cy;

static bool number(double* v) {
    char tok[128];
    if (std::scanf("%127s", tok) != 1) return false;
    *v = std::strtod(tok, nullptr);
    return true;
}

static void print_row(const double* r) {
    for (int f = 0; f < DRES_FIELDS; ++f) std::printf(f ? " %a" : "%a", r[f]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 5 && argc != 6) { std::fprintf(stderr, "usage: disc_residual_plan_main MH MW N NULLS [COLS]\n"); return 2; }
    int v[3];
    for (int i = 0; i < 3; ++i) v[i] = (int)std::strtol(argv[1 + i], nullptr, 10);
    const int MH = v[0], MW = v[1], n = v[2];
    const char* nulls = argv[4];
    const int cols = argc == 6 ? (int)std::strtol(argv[5], nullptr, 10) : 0;
    const bool in_range = n >= 0 && n <= PFIT_JOBS_MAX;
    std::vector<double> jobs(in_range ? (size_t)n * PFIT_JOB_FIELDS : 0);       // exactly sized: a read past n jobs is a sanitizer report
    if (cols > 0) {
        for (int i = 0; in_range && i < n; ++i) {
            double* q = &jobs[(size_t)i * PFIT_JOB_FIELDS];
            q[0] = 3.0 * (i % cols) + 0.25; q[1] = 3.0 * (i / cols) + 0.5; q[2] = i % 7 == 6 ? 0.0 : 2.0; q[3] = (double)i; q[4] = i & 1 ? -1.0 : 1.0;
            if (i % 11 == 10) q[0] = 1e300;
            for (int k = 5; k < PFIT_JOB_FIELDS; ++k) q[k] = 0.0;                // the start is planned and ignored
        }
    } else {
        for (double& j : jobs) if (!number(&j)) { std::fprintf(stderr, "short input\n"); return 2; }
    }
    PeakFitPlan p;
    const char* msg = plan_peak_fits(std::strchr(nulls, 'j') ? nullptr : jobs.data(), n, 1, MH, MW, !std::strchr(nulls, 'm'), !std::strchr(nulls, 'o'), p);
    if (msg) { std::printf("error %s\n", msg); return 0; }
    if ((long long)p.jobs.size() != n) { std::fprintf(stderr, "%zu jobs planned for n = %d\n", p.jobs.size(), n); return 3; }
    // what the entry does after its launch, with exactly sized buffers
    std::vector<double> got(p.run.size() * DRES_FIELDS), out((size_t)n * DRES_FIELDS);
    for (size_t t = 0; t < p.run.size(); ++t)
        for (int f = 0; f < DRES_FIELDS; ++f) got[t * DRES_FIELDS + f] = 1000.0 * (double)t + f + 0.5;
    size_t next = 0;
    for (int i = 0; i < n; ++i) {
        const bool ran = next < p.run.size() && p.run[next] == i;
        disc_residual_row(p.jobs[(size_t)i], ran ? &got[next * DRES_FIELDS] : nullptr, &out[(size_t)i * DRES_FIELDS]);
        next += ran;
    }
    if (next != p.run.size()) { std::fprintf(stderr, "%zu of %zu rows dealt out\n", next, p.run.size()); return 3; }
    std::printf("ok %zu\n", p.run.size());
    if (cols <= 0) {
        for (int i = 0; i < n; ++i) print_row(&out[(size_t)i * DRES_FIELDS]);
        return 0;
    }
    long long cnt[3] = {0, 0, 0}, nneigh = 0, w = 0, h = 0, clipped = 0, wrong = 0;
    size_t t = 0;
    for (int i = 0; i < n; ++i) {
        const double* r = &out[(size_t)i * DRES_FIELDS];
        const PeakFitJob& j = p.jobs[(size_t)i];
        if (j.status == 0) {
            ++cnt[0];
            for (int f = 0; f < 10; ++f) wrong += r[f] != 1000.0 * (double)t + f + 0.5;
            nneigh += (long long)r[15]; w += (long long)(r[11] - r[10] + 1.0); h += (long long)(r[13] - r[12] + 1.0); clipped += (long long)r[14];
            ++t;
        } else {
            ++cnt[j.status == 1 ? 1 : 2];
            for (int f = 0; f < DRES_FIELDS; ++f) {
                const double want = f == 0 ? (double)j.status : (f == 6 || f == 7 || (f >= 10 && f <= 13)) ? -1.0 : 0.0;
                wrong += r[f] != want;
            }
        }
    }
    std::printf("counts %lld %lld %lld\nsums %lld %lld %lld %lld\nwrong %lld\n", cnt[0], cnt[1], cnt[2], nneigh, w, h, clipped, wrong);
    const int show[4] = {0, 1, cols, n - 1};
    for (int k = 0; k < 4; ++k)
        if (show[k] >= 0 && show[k] < n) print_row(&out[(size_t)show[k] * DRES_FIELDS]);
    return 0;
}
