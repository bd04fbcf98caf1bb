// Stand-alone driver of the weight-file reader and plan checks (caesar_yolo_amd/csrc/cy_plan.cpp) for tests/test_plan_host_cpu.py,
// which builds it with the host sanitizers: no HIP, no GPU library.
//
//     plan_main IMAGE            the verdict on one weight-file image, in full
//     plan_main --graph SCALE NC the same for the built-in YOLOv8 graph of (SCALE, NC), which a CYW1 file only names
//     plan_main IMAGE CASES      one short verdict per line of CASES, a text file of
//                                    set OFFSET VALUE    the u32 at byte OFFSET of the image replaced by VALUE
//                                    cut LENGTH          the first LENGTH bytes of the image
//
// Every verdict runs what a load runs on the host, in its order: parse_header, next_conv for every record, validate_plan,
// mark_fusions.  The image lies in a heap buffer of exactly its size (a cut one in a buffer of exactly LENGTH bytes), so that
// AddressSanitizer sees a read behind it; the first and the last value of every filter, bias and scale span are read.
// Full verdict: "error: MESSAGE", or "ops N", one "mark I KIND" per marked op (1 stem+down, 2 pixel-wise pair, 3 bottleneck pair)
// and one "conv NAME CIN COUT K S ACT GROUPS" per convolution.  Short verdict: "error: MESSAGE" or "ok N".
#include "../../caesar_yolo_amd/csrc/cy_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace cy;

namespace {
[[noreturn]] void die(const char* what) { std::fprintf(stderr, "plan_main: %s\n", what); std::exit(2); }

// a message may quote a layer name out of a damaged file: bytes outside printable ASCII are shown as '?'
std::string printable(std::string m) { for (char& ch : m) if (ch < 0x20 || ch > 0x7E) ch = '?'; return m; }

float value_at(const float* p) { float v; std::memcpy(&v, p, sizeof(v)); return v; }

// -> "" and the accepted plan, or the message a load would report
std::string verdict(const unsigned char* buf, size_t n, Plan* plan, double* sum) {
    Reader r{buf, n};
    FileHeader h;
    std::string msg = parse_header(r, plan, &h);
    if (!msg.empty()) return msg;
    for (uint32_t i = 0; i < h.nconv; ++i) {
        ConvRecord rec;
        msg = next_conv(r, h, plan, i, &rec);
        if (!msg.empty()) return msg;
        const size_t nw = (size_t)rec.d.cout * (rec.d.cin / rec.d.groups) * rec.d.k * rec.d.k;
        *sum += value_at(rec.W) + value_at(rec.W + nw - 1) + value_at(rec.b) + value_at(rec.b + rec.d.cout - 1);
        if (rec.wscale) *sum += value_at(rec.wscale) + value_at(rec.wscale + rec.d.cout - 1);
    }
    if (h.v2) {
        msg = validate_plan(*plan);
        if (!msg.empty()) return msg;
    }
    mark_fusions(*plan);
    return "";
}

void print_short(const unsigned char* buf, size_t n) {
    Plan plan;
    double sum = 0.0;
    const std::string msg = verdict(buf, n, &plan, &sum);
    if (msg.empty()) std::printf("ok %zu\n", plan.ops.size());
    else std::printf("error: %s\n", printable(msg).c_str());
}

void print_full(const Plan& plan) {
    std::printf("ops %zu\n", plan.ops.size());
    for (size_t i = 0; i < plan.ops.size(); ++i) if (plan.ops[i].fuse != FUSE_NONE) std::printf("mark %zu %d\n", i, (int)plan.ops[i].fuse);
    for (const ConvDesc& d : plan.convs) std::printf("conv %s %d %d %d %d %d %d\n", d.name.c_str(), d.cin, d.cout, d.k, d.s, d.act, d.groups);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "--graph")) {
        Plan plan = build_plan(argv[2][0], std::atoi(argv[3]));
        if (!plan.ok) { std::printf("error: %s\n", plan.err.c_str()); return 0; }
        mark_fusions(plan);
        print_full(plan);
        return 0;
    }
    if (argc != 2 && argc != 3) die("usage: plan_main IMAGE [CASES] | --graph SCALE NC");
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) die("cannot open the image");
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (size < 0) die("cannot size the image");
    const size_t n = (size_t)size;
    unsigned char* buf = (unsigned char*)std::malloc(n ? n : 1);
    if (!buf || std::fread(buf, 1, n, f) != n) die("cannot read the image");
    std::fclose(f);
    if (argc == 2) {
        Plan plan;
        double sum = 0.0;
        const std::string msg = verdict(buf, n, &plan, &sum);
        if (!msg.empty()) std::printf("error: %s\n", printable(msg).c_str());
        else print_full(plan);
    } else {
        FILE* cases = std::fopen(argv[2], "r");
        if (!cases) die("cannot open the case file");
        char what[8];
        unsigned long long a, b;
        while (std::fscanf(cases, "%7s", what) == 1) {
            if (!std::strcmp(what, "set")) {
                if (std::fscanf(cases, "%llu %llu", &a, &b) != 2 || a + 4 > n || b > 0xFFFFFFFFull) die("bad set case");
                const uint32_t v = (uint32_t)b;
                unsigned char old[4];
                std::memcpy(old, buf + a, 4);
                std::memcpy(buf + a, &v, 4);
                print_short(buf, n);
                std::memcpy(buf + a, old, 4);
            } else if (!std::strcmp(what, "cut")) {
                if (std::fscanf(cases, "%llu", &a) != 1 || a > n) die("bad cut case");
                unsigned char* part = (unsigned char*)std::malloc(a ? (size_t)a : 1);
                if (!part) die("out of memory");
                if (a) std::memcpy(part, buf, (size_t)a);
                print_short(part, (size_t)a);
                std::free(part);
            } else die("unknown case");
        }
        std::fclose(cases);
    }
    std::free(buf);
    return 0;
}
