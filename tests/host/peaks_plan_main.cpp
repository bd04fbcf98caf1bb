// Stand-alone driver of plan_peaks (caesar_yolo_amd/csrc/cy_measure_plan.cpp) for tests/test_peaks_plan_cpu.py, which builds it with
// the host sanitizers: no HIP, no GPU library.
//
//     peaks_plan_main MH MW RADIUS CAP
// prints one line: "ok nsx nseg words row_values", or "error <message>".
#include "../../caesar_yolo_amd/csrc/cy_measure_plan.h"
#include <cstdio>
#include <cstdlib>

using namespace cy;

int main(int argc, char** argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: peaks_plan_main MH MW RADIUS CAP\n"); return 2; }
    int v[4];
    for (int i = 0; i < 4; ++i) v[i] = (int)std::strtol(argv[1 + i], nullptr, 10);
    PeakPlan p;
    if (const char* msg = plan_peaks(v[0], v[1], v[2], v[3], p)) { std::printf("error %s\n", msg); return 0; }
    std::printf("ok %d %lld %lld %lld\n", p.nsx, p.nseg, p.words, p.row_values);
    return 0;
}
