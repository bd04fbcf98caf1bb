// Stand-alone driver of the planner functions of the model / residual step (plan_render, plan_residuals of
// caesar_yolo_amd/csrc/cy_measure_plan.cpp) for tests/test_render_plan_cpu.py, which builds it with the host sanitizers: no HIP, no
// GPU library.
//
//     render_plan_main render CASE OUT      CASE: int32 {MH, MW, m}, float64 nsigma, comp f64 [m][6]; m < 0 or m > 2^20: no comp,
//                                           or `repeat` (int32, after comp) > 1: the one given component m times
//     render_plan_main residuals CASE OUT   CASE: int32 {MH, MW, n}, boxes f64 [n][4], mask_off i64 [n + 1]
// OUT: int32 0 and the planner's outputs as blobs (int64 byte count + bytes), or int32 1 and the error message.
//   render: rows f64 [m][8], rect i32 [m][4], tile_off i32, tile_list i32, {ntx, nty} i32;   residuals: win i32 [n][4], off i64 [n][2],
//   {nws, nmask} i64
#include "../../caesar_yolo_amd/csrc/cy_measure_plan.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace cy;

namespace {
[[noreturn]] void die(const char* what) { std::fprintf(stderr, "render_plan_main: %s\n", what); std::exit(2); }

struct In {
    FILE* f;
    template <class T> std::vector<T> take(size_t count) {
        std::vector<T> v(count);
        if (count && std::fread(v.data(), sizeof(T), count, f) != count) die("truncated case file");
        return v;
    }
};

struct Out {
    FILE* f;
    void i32(int32_t v) { std::fwrite(&v, sizeof(v), 1, f); }
    template <class T> void blob(const std::vector<T>& v) {
        const int64_t bytes = (int64_t)(v.size() * sizeof(T));
        std::fwrite(&bytes, sizeof(bytes), 1, f);
        if (bytes) std::fwrite(v.data(), 1, (size_t)bytes, f);
    }
    void error(const char* msg) { i32(1); std::fwrite(msg, 1, std::strlen(msg), f); }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) die("usage: render_plan_main {render|residuals} CASE OUT");
    In in{std::fopen(argv[2], "rb")};
    if (!in.f) die("cannot open the case file");
    Out out{std::fopen(argv[3], "wb")};
    if (!out.f) die("cannot open the result file");
    const std::vector<int32_t> hdr = in.take<int32_t>(3);
    const int MH = hdr[0], MW = hdr[1], n = hdr[2];
    if (!std::strcmp(argv[1], "render")) {
        const double nsigma = in.take<double>(1)[0];
        const int32_t repeat = in.take<int32_t>(1)[0];
        std::vector<double> comp;
        if (n >= 0 && n <= RND_MAX_COMP) {
            if (repeat > 1) {
                const std::vector<double> one = in.take<double>(6);
                comp.resize((size_t)n * 6);
                for (size_t k = 0; k < (size_t)n; ++k) std::memcpy(&comp[k * 6], one.data(), 6 * sizeof(double));
            } else {
                comp = in.take<double>((size_t)n * 6);
            }
        }
        RenderPlan p;
        if (const char* msg = plan_render(comp.data(), n, nsigma, MH, MW, p)) { out.error(msg); return 0; }
        out.i32(0);
        out.blob(p.rows); out.blob(p.rect); out.blob(p.tile_off); out.blob(p.tile_list);
        out.blob(std::vector<int32_t>{p.ntx, p.nty});
    } else if (!std::strcmp(argv[1], "residuals")) {
        const std::vector<double> boxes = in.take<double>((size_t)n * 4);
        const std::vector<long long> off = in.take<long long>((size_t)n + 1);
        IslandTable t;
        if (const char* msg = plan_residuals(boxes.data(), off.data(), n, MH, MW, t)) { out.error(msg); return 0; }
        out.i32(0);
        out.blob(t.win); out.blob(t.off);
        out.blob(std::vector<long long>{t.nws, t.nmask});
    } else {
        die("unknown mode");
    }
    std::fclose(in.f);
    std::fclose(out.f);
    return 0;
}
