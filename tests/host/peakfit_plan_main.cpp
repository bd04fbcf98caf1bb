// Stand-alone driver of plan_peak_fits (caesar_yolo_amd/csrc/cy_measure_plan.cpp) for tests/test_peakfit_plan_cpu.py, which builds it
// with the host sanitizers: no HIP, no GPU library.
//
//     peakfit_plan_main MH MW N MAX_ITER NULLS < numbers
// NULLS: a string of the letters m, j, o naming the pointers that are passed as null ("-": none).  Standard input: N jobs of eleven
// numbers (cx cy R bkg sign A x0 y0 a b c), as C99 hexadecimal floats or "nan" / "inf" / "-inf"; with a negative or oversize N
// nothing is read.  Prints "error <message>", or "ok <fitted>", one line per job:
//     status x0 x1 y0 y1 clipped nneigh crowded neigh[0] .. neigh[7] r2 p0[1] p0[2]
// (r2 and the start's centre relative to the window as hexadecimal floats), the indices of the fitted jobs on one line after "run",
// and last "plan_ms <milliseconds the planner took>".
#include "../../caesar_yolo_amd/csrc/cy_measure_plan.h"
#include <chrono>
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

int main(int argc, char** argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: peakfit_plan_main MH MW N MAX_ITER NULLS\n"); return 2; }
    int v[4];
    for (int i = 0; i < 4; ++i) v[i] = (int)std::strtol(argv[1 + i], nullptr, 10);
    const int MH = v[0], MW = v[1], n = v[2], max_iter = v[3];
    const char* nulls = argv[5];
    const bool in_range = n >= 0 && n <= PFIT_JOBS_MAX;
    std::vector<double> jobs(in_range ? (size_t)n * PFIT_JOB_FIELDS : 0);       // exactly sized: a read past n jobs is a sanitizer report
    for (double& j : jobs) if (!number(&j)) { std::fprintf(stderr, "short input\n"); return 2; }
    PeakFitPlan p;
    const auto t0 = std::chrono::steady_clock::now();
    const char* msg = plan_peak_fits(std::strchr(nulls, 'j') ? nullptr : jobs.data(), n, max_iter, MH, MW, !std::strchr(nulls, 'm'), !std::strchr(nulls, 'o'), p);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (msg) { std::printf("error %s\n", msg); return 0; }
    if ((long long)p.jobs.size() != n) { std::fprintf(stderr, "%zu jobs planned for n = %d\n", p.jobs.size(), n); return 3; }
    std::printf("ok %zu\n", p.run.size());
    for (const PeakFitJob& j : p.jobs) {
        std::printf("%d %d %d %d %d %d %d %d", j.status, j.x0, j.x1, j.y0, j.y1, j.clipped, j.nneigh, j.crowded);
        for (int k = 0; k < PFIT_NEIGH_MAX; ++k) std::printf(" %d", j.neigh[k]);
        std::printf(" %a %a %a\n", j.r2, j.p0[1], j.p0[2]);
    }
    std::printf("run");
    for (int e : p.run) std::printf(" %d", e);
    std::printf("\nplan_ms %.3f\n", ms);
    return 0;
}
