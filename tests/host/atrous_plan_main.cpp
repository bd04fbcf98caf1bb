// Stand-alone driver of plan_atrous (caesar_yolo_amd/csrc/cy_measure_plan.cpp) for tests/test_atrous_plan_cpu.py, which builds it with
// the host sanitizers: no HIP, no GPU library.
//
//     atrous_plan_main MH MW STEP IN SMOOTH DETAIL
// IN, SMOOTH, DETAIL: the buffers' addresses as unsigned integers (0: null).  Prints one line: "ok ncb nres nchunk items grid bytes",
// or "error <message>".
#include "../../caesar_yolo_amd/csrc/cy_measure_plan.h"
#include <cstdio>
#include <cstdlib>

using namespace cy;

int main(int argc, char** argv) {
    if (argc != 7) { std::fprintf(stderr, "usage: atrous_plan_main MH MW STEP IN SMOOTH DETAIL\n"); return 2; }
    int v[3];
    for (int i = 0; i < 3; ++i) v[i] = (int)std::strtol(argv[1 + i], nullptr, 10);
    unsigned long long a[3];
    for (int i = 0; i < 3; ++i) a[i] = std::strtoull(argv[4 + i], nullptr, 10);
    AtrousPlan p;
    if (const char* msg = plan_atrous(v[0], v[1], v[2], a[0], a[1], a[2], p)) { std::printf("error %s\n", msg); return 0; }
    std::printf("ok %d %d %d %lld %d %lld\n", p.ncb, p.nres, p.nchunk, p.items, p.grid, p.bytes);
    return 0;
}
