// Stand-alone driver of the conv dispatch (caesar_yolo_amd/csrc/cy_conv_plan.cpp) for tests/test_conv_plan_cpu.py, which builds it
// with the host sanitizers: no HIP, no GPU library.
//
//     conv_plan_main --names            "variant I NAME" for every ConvVariant, "kernel I NAME" for every ConvKernel
//     conv_plan_main --cases CASES      one "VARIANT-NAME | KERNEL-NAME" per line of CASES: a convolution as cy_conv_slices lays it out.
//                                       Every field an integer:
//                                           prec B Hi Wi Cin Cout k s  c1 up0  rows out_bs out_ro  act res split wgt2
//                                           inv strip dual direct_min_blocks head_direct narrow_direct head_pair wide_persist x3_persist
//                                       (prec 0 fp16, 1 fp32, 2 fp16x3; c1: channels of a second segment; rows: fp32 prediction rows;
//                                       res / wgt2: non-null or null; the last nine: the ConvKnobs fields in their order)
//     conv_plan_main IMAGE QUERIES      a CYW1 / CYW2 weight image; per line "B H W prec split inv" of QUERIES a line "query ..." and
//                                       one line per convolution op of the plan, through conv_geometry:
//                                           B Hi Wi Cin Cout k s c0 c1 up0 out_f32 out_bs out_ro act res wgt32 wgt2 | VARIANT-NAME | KERNEL-NAME
//
// wgt32 is non-null exactly when conv_second_copy says so (down_copy as the loader passes it: true; the test entry: false); in
// the fp16x3 context oscale is non-null and split as given.  IMAGE mode runs the knobs at their defaults with batch_invariant = inv
// and sets wgt2 as a forward pass does: on the first op of a marked pixel-wise pair in the fp16 context whose variant is the
// 256-channel pixels-direct kernel.
#include "../../caesar_yolo_amd/csrc/cy_conv_plan.h"
#include "../../caesar_yolo_amd/csrc/cy_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace cy;

namespace {
[[noreturn]] void die(const char* what) { std::fprintf(stderr, "conv_plan_main: %s\n", what); std::exit(2); }

const int kSome = 0;                                   // a non-null address for the pointers the decision only tests
const void* some(bool on) { return on ? &kSome : nullptr; }

void print_choice(Precision prec, const ConvArgs& a, const ConvKnobs& k) {
    const ConvChoice ch = conv_choose(prec, a, k);
    std::printf("%s | %s\n", conv_variant_name(ch.variant), conv_kernel_name(ch.kernel));
}

void run_cases(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) die("cannot open the case file");
    long v[26];
    for (;;) {
        int n = 0;
        while (n < 26 && std::fscanf(f, "%ld", &v[n]) == 1) ++n;
        if (n == 0) break;
        if (n != 26) die("a case has 26 integers");
        const Precision prec = (Precision)v[0];
        if (prec != PREC_F16 && prec != PREC_F32 && prec != PREC_F16X3) die("bad precision");
        const bool x3 = prec == PREC_F16X3, rows = v[10] != 0;
        ConvArgs a{};
        a.B = (int)v[1]; a.Hi = (int)v[2]; a.Wi = (int)v[3]; a.Cin = (int)v[4]; a.Cout = (int)v[5]; a.k = (int)v[6]; a.s = (int)v[7];
        if (a.B < 1 || a.Hi < 1 || a.Wi < 1 || a.Cin < 8 || a.Cout < 1 || (a.k != 1 && a.k != 3) || (a.s != 1 && a.s != 2)) die("bad geometry");
        const int pad = a.k / 2;
        a.Ho = (a.Hi + 2 * pad - a.k) / a.s + 1; a.Wo = (a.Wi + 2 * pad - a.k) / a.s + 1;
        a.c1 = (int)v[8]; a.c0 = a.Cin - a.c1; a.up0 = v[9] != 0;
        a.in0 = some(true); a.in1 = some(a.c1 != 0); a.wgt = some(true); a.bias = (const float*)some(true); a.out = const_cast<void*>(some(true));
        if (rows) { a.out_bs = (int)v[11]; a.out_ro = (int)v[12]; a.out_f32 = 1; }
        else a.out_bs = a.Ho * a.Wo;
        a.act = (int)v[13]; a.res = some(v[14] != 0); a.split = x3 ? (int)v[15] : 0; a.oscale = (const float*)some(x3);
        a.wgt2 = some(v[16] != 0);
        a.wgt32 = some(conv_second_copy(prec, a.Cin, a.Cout, a.k, a.s, false));
        ConvKnobs k;
        k.batch_invariant = (int)v[17]; k.strip = (int)v[18]; k.wide_dual = (int)v[19]; k.direct_min_blocks = v[20]; k.head_direct = (int)v[21];
        k.narrow_direct = (int)v[22]; k.head_pair = (int)v[23]; k.wide_persist = (int)v[24]; k.x3_persist = (int)v[25];
        print_choice(prec, a, k);
    }
    std::fclose(f);
}

// the plan of an image, as a load accepts it
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
    int B, H, W, pr, split, inv;
    while (std::fscanf(f, "%d %d %d %d %d %d", &B, &H, &W, &pr, &split, &inv) == 6) {
        const Precision prec = (Precision)pr;
        if (B < 1 || H < 32 || W < 32 || H % 32 || W % 32 || (prec != PREC_F16 && prec != PREC_F32 && prec != PREC_F16X3)) die("bad query");
        const bool x3 = prec == PREC_F16X3;
        ConvKnobs k;
        k.batch_invariant = inv;
        int a_off[3], A = 0;
        for (int l = 0; l < 3; ++l) { a_off[l] = A; A += (H >> (3 + l)) * (W >> (3 + l)); }
        std::printf("query %d %d %d %d %d %d\n", B, H, W, pr, split, inv);
        for (const Op& o : plan.ops) {
            if (o.kind != OPK_CONV) continue;
            ConvArgs a = conv_geometry(plan, o, B, H, W, x3 ? 2 : 1, A, a_off);
            a.in0 = some(true); a.in1 = some(o.in1 >= 0); a.wgt = some(true); a.bias = (const float*)some(true); a.out = const_cast<void*>(some(true));
            a.res = some(o.res >= 0);
            a.split = x3 ? split : 0; a.oscale = (const float*)some(x3);
            a.wgt32 = some(conv_second_copy(prec, a.Cin, a.Cout, a.k, a.s, true));
            if (prec == PREC_F16 && o.fuse == FUSE_PW_PAIR && conv_choose(prec, a, k).variant == CONV_DIRECT_256) a.wgt2 = some(true);
            std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d | ", a.B, a.Hi, a.Wi, a.Cin, a.Cout, a.k, a.s, a.c0, a.c1, a.up0, a.out_f32,
                        a.out_bs, a.out_ro, a.act, a.res != nullptr, a.wgt32 != nullptr, a.wgt2 != nullptr);
            print_choice(prec, a, k);
        }
    }
    std::fclose(f);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--names")) {
        for (int i = 0; i < CONV_NUM_VARIANTS; ++i) std::printf("variant %d %s\n", i, conv_variant_name(i));
        for (int i = 0; i < CK_NUM_KERNELS; ++i) std::printf("kernel %d %s\n", i, conv_kernel_name((ConvKernel)i));
        return 0;
    }
    if (argc != 3) die("usage: conv_plan_main --names | --cases CASES | IMAGE QUERIES");
    if (!std::strcmp(argv[1], "--cases")) run_cases(argv[2]);
    else run_queries(load_plan(argv[1]), argv[2]);
    return 0;
}
