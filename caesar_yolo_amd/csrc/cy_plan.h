// Execution plan of the YOLOv8 detection graph on NHWC buffers (host side, no HIP).
// Graph per the public yolov8.yaml as summarised in SURVEY.md Appendix A.1 step 4; what the reference runs through
// `self.model(...)` at caesar_yolo/evaluation.py:181-193.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace cy {

struct ConvDesc { std::string name; int cin, cout, k, s, act; int groups = 1; };

struct Tensor { int level; int C; };          // spatial size = (H >> level, W >> level), C channels per pixel

enum OpKind { OPK_STEM = 0, OPK_CONV = 1, OPK_POOL = 2, OPK_DWCONV = 3, OPK_ATTN = 4 };   // 3, 4: YOLO11 plans (CYW2 files)

// What ops[i] and ops[i + 1] can run as ONE launch, by the shape of the plan alone (mark_fusions); whether a forward pass does so
// is decided per call by the run-time gate of that launch (environment knob, precision, batch size, kernel variant).
enum FuseMark { FUSE_NONE = 0, FUSE_STEM_DOWN, FUSE_PW_PAIR, FUSE_BNECK_PAIR };

struct Op {
    OpKind kind;
    int conv;                                  // index into Plan::convs (STEM/CONV)
    int in0, in0_coff, c0, up0;                // segment 0 (tensor id, channel offset, channels, read through x2 nearest upsample)
    int in1, in1_coff, c1;                     // segment 1 or in1 = -1
    int out, out_coff;                         // destination tensor slice, or out = -1 for the head output
    int res, res_coff;                         // residual tensor slice or res = -1
    int pred_level, pred_coff;                 // when out == -1: which stride level, channel offset inside [64+nc]
    int p0 = 0, p1 = 0, p2 = 0, p3 = 0;        // DWCONV: input channel map (blk, gstride, goff); ATTN: heads, key_dim, head_dim
    FuseMark fuse = FUSE_NONE;                 // this op is the first of a pair that one kernel can run (mark_fusions)
    int box = 0;                               // 1, 2, 3: the three ops of a detect-head box branch (3x3, 3x3 64->64, 1x1 into columns 0..63) whose
                                               // result is read at candidate anchors only (mark_fusions); 0: any other op
};

struct Plan {
    char scale; int nc;
    std::string arch = "yolov8";
    std::vector<ConvDesc> convs;               // canonical (state_dict) order == weight-file order
    std::vector<Tensor> tensors;               // tensor 0 is the network input [B,H,W,4]
    std::vector<Op> ops;                       // execution order
    int feat_level[3];
    bool ok; std::string err;
};

Plan build_plan(char scale, int nc);
int py_round(double x);                        // Python round(): half to even

// ---- weight files (CYW1: the graph is build_plan's; CYW2: the execution plan travels in the file: weights.py:write_cyw2,
// yolo11_graph.py).  A file is untrusted data: everything here is host code without HIP, reports through a returned message
// ("" = fine) and is run under the host sanitizers by tests/test_plan_host_cpu.py.
struct Reader {
    const unsigned char* p; size_t n, o = 0; bool bad = false;
    uint32_t u32() { if (n - o < 4) { bad = true; return 0; } uint32_t v; memcpy(&v, p + o, 4); o += 4; return v; }
    std::string str(uint32_t len) { if (n - o < len) { bad = true; return ""; } std::string s((const char*)p + o, len); o += std::min<size_t>((len + (size_t)3) / 4 * 4, n - o); return s; }
    const float* f32(size_t cnt) { if ((n - o) / 4 < cnt) { bad = true; return nullptr; } const float* r = (const float*)(p + o); o += 4 * cnt; return r; }
};
struct FileHeader { bool v2 = false, has_flags = false, unsupported = false; uint32_t nconv = 0; std::vector<std::string> names; };
// one convolution of the file: its description and where its folded fp32 filter, bias and per-channel scale (or null) lie in the buffer
struct ConvRecord { ConvDesc d; const float* W; const float* b; const float* wscale; };

// magic, version, class names and the plan (CYW2: tensors and ops as the file gives them, convs still empty).  h->unsupported:
// the file is sound but names a graph that build_plan does not know.
std::string parse_header(Reader& r, Plan* plan, FileHeader* h);
// the i-th conv record, read where `r` stands; CYW2: checked and appended to plan->convs, CYW1: compared with plan->convs[i]
std::string next_conv(Reader& r, const FileHeader& h, Plan* plan, uint32_t i, ConvRecord* out);
std::string validate_plan(const Plan& p);      // CYW2, once every conv is known: each op's channel slices lie inside its tensors
void mark_fusions(Plan& p);                    // sets Op::fuse and Op::box of every op; the plan is accepted

}  // namespace cy
