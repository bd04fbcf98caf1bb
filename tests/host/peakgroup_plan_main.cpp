// Stand-alone driver of plan_peak_groups and peak_group_rows (caesar_yolo_amd/csrc/cy_measure_plan.cpp) for
// tests/test_peakgroup_plan_cpu.py, which builds it with the host sanitizers: no HIP, no GPU library.
//
//     peakgroup_plan_main MH MW N MAX_ITER LINK NULLS < numbers
// LINK: a C99 hexadecimal float or "nan" / "inf".  NULLS: a string of the letters m, j, o naming the pointers that are passed as null
// ("-": none).  Standard input: N jobs of eleven numbers (cx cy R bkg sign A x0 y0 a b c), as C99 hexadecimal floats or "nan" / "inf" /
// "-inf"; with a negative or oversize N nothing is read.  Prints "error <message>", or "ok <group jobs>", one line per job:
//     status group size slot nlinked job_of
// one line per group job:
//     group M member[0..3] x0 x1 y0 y1 bkg sign | nout[s] out[s][0..7] p0[6 s + 1] p0[6 s + 2]   for s < M
// (bkg, sign and the starts' centres relative to the group window as hexadecimal floats), then for N <= 1000 one line per job
// "row" with the PGRP_FIELDS values that the host writes when the device table says: status 3 for the members of the even group jobs
// and status 0 with the centre (1.5, 2.5) and nexcluded 7 for the odd ones.  Last "plan_ms <milliseconds the planner took>".
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
    if (argc != 7) { std::fprintf(stderr, "usage: peakgroup_plan_main MH MW N MAX_ITER LINK NULLS\n"); return 2; }
    int v[4];
    for (int i = 0; i < 4; ++i) v[i] = (int)std::strtol(argv[1 + i], nullptr, 10);
    const int MH = v[0], MW = v[1], n = v[2], max_iter = v[3];
    const double link = std::strtod(argv[5], nullptr);
    const char* nulls = argv[6];
    const bool in_range = n >= 0 && n <= PFIT_JOBS_MAX;
    std::vector<double> jobs(in_range ? (size_t)n * PFIT_JOB_FIELDS : 0);       // exactly sized: a read past n jobs is a sanitizer report
    for (double& j : jobs) if (!number(&j)) { std::fprintf(stderr, "short input\n"); return 2; }
    PeakGroupPlan p;
    const auto t0 = std::chrono::steady_clock::now();
    const char* msg = plan_peak_groups(std::strchr(nulls, 'j') ? nullptr : jobs.data(), n, link, max_iter, MH, MW, !std::strchr(nulls, 'm'),
                                       !std::strchr(nulls, 'o'), p);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (msg) { std::printf("error %s\n", msg); return 0; }
    if ((long long)p.status.size() != n || (long long)p.rows.size() != (long long)n * PGRP_FIELDS) { std::fprintf(stderr, "%zu jobs planned for n = %d\n", p.status.size(), n); return 3; }
    std::printf("ok %zu\n", p.groups.size());
    for (size_t i = 0; i < p.status.size(); ++i)
        std::printf("%d %d %d %d %d %d\n", p.status[i], p.group[i], p.size[i], p.slot[i], p.nlinked[i], p.job_of[i]);
    for (const PeakGroupJob& g : p.groups) {
        std::printf("group %d %d %d %d %d %d %d %d %d %a %a", g.M, g.member[0], g.member[1], g.member[2], g.member[3], g.x0, g.x1, g.y0, g.y1, g.bkg, g.sign);
        for (int s = 0; s < g.M; ++s) {
            std::printf(" | %d", g.nout[s]);
            for (int k = 0; k < PFIT_NEIGH_MAX; ++k) std::printf(" %d", g.out[s][k]);
            std::printf(" %a %a", g.p0[6 * s + 1], g.p0[6 * s + 2]);
        }
        std::printf("\n");
    }
    if (n > 0 && n <= 1000) {
        std::vector<double> got(p.groups.size() * BLEND_MAX_MEMBERS * PGRP_FIELDS, 0.0), out(p.rows);       // exactly sized
        for (size_t t = 0; t < p.groups.size(); ++t)
            for (int s = 0; s < p.groups[t].M; ++s) {
                double* r = &got[(t * BLEND_MAX_MEMBERS + (size_t)s) * PGRP_FIELDS];
                r[0] = t % 2 ? 0.0 : 3.0; r[5] = (double)p.groups[t].member[0]; r[6] = (double)p.groups[t].M; r[7] = (double)s;
                r[8] = 9.0; r[9] = 1.5; r[10] = 2.5; r[41] = 7.0;
            }
        peak_group_rows(p, jobs.data(), got.data(), out.data());
        for (int i = 0; i < n; ++i) {
            std::printf("row");
            for (int f = 0; f < PGRP_FIELDS; ++f) std::printf(" %a", out[(size_t)i * PGRP_FIELDS + f]);
            std::printf("\n");
        }
    }
    std::printf("plan_ms %.3f\n", ms);
    return 0;
}
