// Stand-alone driver of the conv dispatch for tests/test_direct_persist_plan_cpu.py: the rule that gives a launch of the pixels-direct
// 256-channel tile its persistent form (conv_kernel, caesar_yolo_amd/csrc/cy_conv_plan.cpp).  Host code only, built with the host
// sanitizers.
//
//     direct_persist_plan_main --cases CASES     per line of CASES, every field an integer,
//                                                    prec B Hi Wi Cin Cout k s c1 res wgt2 inv direct_min_blocks direct_persist direct_persist_grid
//                                                a line "VARIANT-NAME | KERNEL-NAME | persist_grid"
//     direct_persist_plan_main IMAGE QUERIES     a CYW1 / CYW2 weight image; per line "B H W prec inv direct_persist" of QUERIES a line
//                                                "query ..." and one line per convolution op of the plan "CONV-NAME | B Ho Wo Cin Cout k | VARIANT-NAME | KERNEL-NAME"
//                                                (wgt2 set as a forward pass sets it: conv_plan_main.cpp)
#include "../../caesar_yolo_amd/csrc/cy_conv_plan.h"
#include "../../caesar_yolo_amd/csrc/cy_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace cy;

namespace {
[[noreturn]] void die(const char* what) { std::fprintf(stderr, "direct_persist_plan_main: %s\n", what); std::exit(2); }

const int kSome = 0;
const void* some(bool on) { return on ? &kSome : nullptr; }

void run_cases(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) die("cannot open the case file");
    long v[15];
    for (;;) {
        int n = 0;
        while (n < 15 && std::fscanf(f, "%ld", &v[n]) == 1) ++n;
        if (n == 0) break;
        if (n != 15) die("a case has 15 integers");
        const Precision prec = (Precision)v[0];
        if (prec != PREC_F16 && prec != PREC_F32 && prec != PREC_F16X3) die("bad precision");
        const bool x3 = prec == PREC_F16X3;
        ConvArgs a{};
        a.B = (int)v[1]; a.Hi = (int)v[2]; a.Wi = (int)v[3]; a.Cin = (int)v[4]; a.Cout = (int)v[5]; a.k = (int)v[6]; a.s = (int)v[7];
        if (a.B < 1 || a.Hi < 1 || a.Wi < 1 || a.Cin < 8 || a.Cout < 1 || (a.k != 1 && a.k != 3) || (a.s != 1 && a.s != 2)) die("bad geometry");
        const int pad = a.k / 2;
        a.Ho = (a.Hi + 2 * pad - a.k) / a.s + 1; a.Wo = (a.Wi + 2 * pad - a.k) / a.s + 1;
        a.c1 = (int)v[8]; a.c0 = a.Cin - a.c1;
        a.in0 = some(true); a.in1 = some(a.c1 != 0); a.wgt = some(true); a.bias = (const float*)some(true); a.out = const_cast<void*>(some(true));
        a.out_bs = a.Ho * a.Wo; a.act = 1;
        a.res = some(v[9] != 0); a.wgt2 = some(v[10] != 0);
        a.split = x3 ? 3 : 0; a.oscale = (const float*)some(x3);
        a.wgt32 = some(conv_second_copy(prec, a.Cin, a.Cout, a.k, a.s, false));
        ConvKnobs k;
        k.batch_invariant = (int)v[11]; k.direct_min_blocks = v[12]; k.direct_persist = (int)v[13]; k.direct_persist_grid = (int)v[14];
        const ConvChoice ch = conv_choose(prec, a, k);
        std::printf("%s | %s | %d\n", conv_variant_name(ch.variant), conv_choice_name(ch), ch.persist_grid);
    }
    std::fclose(f);
}

Plan load_plan(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) die("cannot open the image");
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (size < 0) die("cannot size the image");
    std::vector<unsigned char> buf((size_t)size);
    if (std::fread(buf.data(), 1, buf.size(), f) != buf.size()) die("cannot read the image");
    std::fclose(f);
    Plan plan;
    Reader r{buf.data(), buf.size()};
    FileHeader h;
    std::string msg = parse_header(r, &plan, &h);
    for (uint32_t i = 0; msg.empty() && i < h.nconv; ++i) { ConvRecord rec; msg = next_conv(r, h, &plan, i, &rec); }
    if (msg.empty() && h.v2) msg = validate_plan(plan);
    if (!msg.empty()) die(msg.c_str());
    mark_fusions(plan);
    return plan;
}

void run_queries(const Plan& plan, const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) die("cannot open the query file");
    int B, H, W, pr, inv, persist;
    while (std::fscanf(f, "%d %d %d %d %d %d", &B, &H, &W, &pr, &inv, &persist) == 6) {
        const Precision prec = (Precision)pr;
        if (B < 1 || H < 32 || W < 32 || H % 32 || W % 32 || (prec != PREC_F16 && prec != PREC_F32 && prec != PREC_F16X3)) die("bad query");
        const bool x3 = prec == PREC_F16X3;
        ConvKnobs k;
        k.batch_invariant = inv; k.direct_persist = persist;
        int a_off[3], A = 0;
        for (int l = 0; l < 3; ++l) { a_off[l] = A; A += (H >> (3 + l)) * (W >> (3 + l)); }
        std::printf("query %d %d %d %d %d %d\n", B, H, W, pr, inv, persist);
        for (const Op& o : plan.ops) {
            if (o.kind != OPK_CONV) continue;
            ConvArgs a = conv_geometry(plan, o, B, H, W, x3 ? 2 : 1, A, a_off);
            a.in0 = some(true); a.in1 = some(o.in1 >= 0); a.wgt = some(true); a.bias = (const float*)some(true); a.out = const_cast<void*>(some(true));
            a.res = some(o.res >= 0);
            a.split = x3 ? 3 : 0; a.oscale = (const float*)some(x3);
            a.wgt32 = some(conv_second_copy(prec, a.Cin, a.Cout, a.k, a.s, true));
            if (prec == PREC_F16 && o.fuse == FUSE_PW_PAIR && conv_choose(prec, a, k).variant == CONV_DIRECT_256) a.wgt2 = some(true);
            const ConvChoice ch = conv_choose(prec, a, k);
            std::printf("%s | %d %d %d %d %d %d | %s | %s\n", plan.convs[o.conv].name.c_str(), a.B, a.Ho, a.Wo, a.Cin, a.Cout, a.k, conv_variant_name(ch.variant),
                        conv_choice_name(ch));
        }
    }
    std::fclose(f);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) die("usage: direct_persist_plan_main --cases CASES | IMAGE QUERIES");
    if (!std::strcmp(argv[1], "--cases")) run_cases(argv[2]);
    else run_queries(load_plan(argv[1]), argv[2]);
    return 0;
}
