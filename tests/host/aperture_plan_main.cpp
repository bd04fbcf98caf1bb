// Stand-alone driver of plan_apertures (caesar_yolo_amd/csrc/cy_measure_plan.cpp) for tests/test_aperture_plan_cpu.py, which builds it
// with the host sanitizers: no HIP, no GPU library.
//
//     aperture_plan_main MH MW N K NULLS < numbers
// NULLS: a string of the letters m, j, f, o naming the pointers that are passed as null ("-": none).  Standard input: K factors, then
// N jobs of three numbers (cx cy unit), as C99 hexadecimal floats or "nan" / "inf" / "-inf"; with a negative or oversize N, or an
// oversize K, nothing is read beyond min(K, 64) factors.  Prints "error <message>", or "ok <measured>" and one line per job:
// status x0 x1 y0 y1 clipped r2[0] .. r2[7], the squared radii as hexadecimal floats.
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

int main(int argc, char** argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: aperture_plan_main MH MW N K NULLS\n"); return 2; }
    int v[4];
    for (int i = 0; i < 4; ++i) v[i] = (int)std::strtol(argv[1 + i], nullptr, 10);
    const int MH = v[0], MW = v[1], n = v[2], K = v[3];
    const char* nulls = argv[5];
    const bool in_range = n >= 0 && n <= APER_JOBS_MAX && K >= 1 && K <= APER_RINGS_MAX;
    std::vector<double> factors((size_t)(K > 0 && K <= 64 ? K : 0)), jobs(in_range ? (size_t)n * 3 : 0);
    for (double& f : factors) if (!number(&f)) { std::fprintf(stderr, "short input\n"); return 2; }
    for (double& j : jobs) if (!number(&j)) { std::fprintf(stderr, "short input\n"); return 2; }
    // exactly sized heap buffers: a read past K factors or n jobs is a sanitizer report
    AperPlan p;
    const char* msg = plan_apertures(std::strchr(nulls, 'j') ? nullptr : jobs.data(), n, std::strchr(nulls, 'f') ? nullptr : factors.data(), K, MH, MW,
                                     !std::strchr(nulls, 'm'), !std::strchr(nulls, 'j'), !std::strchr(nulls, 'o'), p);
    if (msg) { std::printf("error %s\n", msg); return 0; }
    if ((long long)p.jobs.size() != n) { std::fprintf(stderr, "%zu jobs planned for n = %d\n", p.jobs.size(), n); return 3; }
    std::printf("ok %d\n", p.measured);
    for (const AperJob& j : p.jobs) {
        std::printf("%d %d %d %d %d %d", j.status, j.x0, j.x1, j.y0, j.y1, j.clipped);
        for (int k = 0; k < APER_RINGS_MAX; ++k) std::printf(" %a", j.r2[k]);
        std::printf("\n");
    }
    return 0;
}
