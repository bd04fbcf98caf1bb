// Builds the conv list (canonical order) and the NHWC execution plan for a (scale, nc) pair; reads and checks the plan and the
// conv records of a weight file, and marks the pairs of ops that one kernel can run.
#include "cy_plan.h"
#include <algorithm>
#include <cmath>
#include <map>

namespace cy {

namespace {
struct Scale { double d, w; int mc; };
bool scale_of(char s, Scale* o) {
    switch (s) {
        case 'n': *o = {0.33, 0.25, 1024}; return true;
        case 's': *o = {0.33, 0.50, 1024}; return true;
        case 'm': *o = {0.67, 0.75, 768}; return true;
        case 'l': *o = {1.00, 1.00, 512}; return true;
        case 'x': *o = {1.00, 1.25, 512}; return true;
    }
    return false;
}
int make_div8(double x) { return (int)std::ceil(x / 8.0) * 8; }

struct Builder {
    Plan p;
    std::map<std::string, int> idx;
    int T(int level, int C) { p.tensors.push_back({level, C}); return (int)p.tensors.size() - 1; }
    void add_conv(const std::string& name, int cin, int cout, int k, int s, int act = 1) {
        idx[name] = (int)p.convs.size();
        p.convs.push_back({name, cin, cout, k, s, act});
    }
    void decl_c2f(int i, int cin, int cout, int n) {
        const int h = cout / 2;
        const std::string b = "model." + std::to_string(i);
        add_conv(b + ".cv1", cin, 2 * h, 1, 1);
        add_conv(b + ".cv2", (2 + n) * h, cout, 1, 1);
        for (int j = 0; j < n; ++j) {
            add_conv(b + ".m." + std::to_string(j) + ".cv1", h, h, 3, 1);
            add_conv(b + ".m." + std::to_string(j) + ".cv2", h, h, 3, 1);
        }
    }
    Op base(const std::string& name) {
        Op o{};
        o.kind = OPK_CONV; o.conv = idx.at(name);
        o.in1 = -1; o.res = -1; o.pred_level = -1;
        return o;
    }
    void conv(const std::string& name, int in, int in_coff, int out, int out_coff, int res = -1, int res_coff = 0) {
        Op o = base(name);
        o.in0 = in; o.in0_coff = in_coff; o.c0 = p.convs[o.conv].cin;
        o.out = out; o.out_coff = out_coff; o.res = res; o.res_coff = res_coff;
        p.ops.push_back(o);
    }
    // C2f: cv1 -> [y0|y1] into the head of a (2+n)*h-channel buffer; bottleneck j reads slice 1+j and appends slice 2+j
    // (in place "concat"); cv2 reads the whole buffer.  `first` is the already-filled cv1 op description.
    void c2f(int i, Op first, int level, int cout, int n, bool shortcut, int dst, int dst_coff) {
        const int h = cout / 2;
        const std::string b = "model." + std::to_string(i);
        const int buf = T(level, (2 + n) * h), tmp = T(level, h);
        first.out = buf; first.out_coff = 0;
        p.ops.push_back(first);
        for (int j = 0; j < n; ++j) {
            const std::string m = b + ".m." + std::to_string(j);
            conv(m + ".cv1", buf, (1 + j) * h, tmp, 0);
            conv(m + ".cv2", tmp, 0, buf, (2 + j) * h, shortcut ? buf : -1, (1 + j) * h);
        }
        conv(b + ".cv2", buf, 0, dst, dst_coff);
    }
    Op cv1_single(int i, int in, int coff) {
        Op o = base("model." + std::to_string(i) + ".cv1");
        o.in0 = in; o.in0_coff = coff; o.c0 = p.convs[o.conv].cin;
        return o;
    }
};
}  // namespace

int py_round(double x) {
    double f = std::floor(x), d = x - f;
    if (d > 0.5) return (int)f + 1;
    if (d < 0.5) return (int)f;
    return ((long)f % 2 == 0) ? (int)f : (int)f + 1;
}

Plan build_plan(char scale, int nc) {
    Builder B;
    Plan& p = B.p;
    p.scale = scale; p.nc = nc; p.ok = false;
    Scale sc;
    if (!scale_of(scale, &sc) || nc < 1 || nc > 1000) { p.err = "unknown scale or bad nc"; return p; }
    auto ch = [&](int c) { return make_div8(std::min(c, sc.mc) * sc.w); };
    auto rep = [&](int n) { return std::max(py_round(n * sc.d), 1); };
    const int c1 = ch(64), c2 = ch(128), c3 = ch(256), c4 = ch(512), c5 = ch(1024), n3 = rep(3), n6 = rep(6);

    // ---- conv declarations, canonical order (must match caesar_yolo_amd/yolov8_spec.py:conv_list)
    B.add_conv("model.0", 3, c1, 3, 2);
    B.add_conv("model.1", c1, c2, 3, 2);
    B.decl_c2f(2, c2, c2, n3);
    B.add_conv("model.3", c2, c3, 3, 2);
    B.decl_c2f(4, c3, c3, n6);
    B.add_conv("model.5", c3, c4, 3, 2);
    B.decl_c2f(6, c4, c4, n6);
    B.add_conv("model.7", c4, c5, 3, 2);
    B.decl_c2f(8, c5, c5, n3);
    B.add_conv("model.9.cv1", c5, c5 / 2, 1, 1);
    B.add_conv("model.9.cv2", c5 * 2, c5, 1, 1);
    B.decl_c2f(12, c5 + c4, c4, n3);
    B.decl_c2f(15, c4 + c3, c3, n3);
    B.add_conv("model.16", c3, c3, 3, 2);
    B.decl_c2f(18, c3 + c4, c4, n3);
    B.add_conv("model.19", c4, c4, 3, 2);
    B.decl_c2f(21, c4 + c5, c5, n3);
    const int chs[3] = {c3, c4, c5};
    const int cb = std::max(16, std::max(chs[0] / 4, 64));
    const int cc = std::max(chs[0], std::min(nc, 100));
    for (int l = 0; l < 3; ++l) {
        const std::string b = "model.22.cv2." + std::to_string(l);
        B.add_conv(b + ".0", chs[l], cb, 3, 1);
        B.add_conv(b + ".1", cb, cb, 3, 1);
        B.add_conv(b + ".2", cb, 64, 1, 1, 0);
    }
    for (int l = 0; l < 3; ++l) {
        const std::string b = "model.22.cv3." + std::to_string(l);
        B.add_conv(b + ".0", chs[l], cc, 3, 1);
        B.add_conv(b + ".1", cc, cc, 3, 1);
        B.add_conv(b + ".2", cc, nc, 1, 1, 0);
    }

    // ---- execution plan
    const int in = B.T(0, 4);
    const int t0 = B.T(1, c1), t1 = B.T(2, c2), t2 = B.T(2, c2), t3 = B.T(3, c3), t4 = B.T(3, c3);
    const int t5 = B.T(4, c4), t6 = B.T(4, c4), t7 = B.T(5, c5), t8 = B.T(5, c5);
    const int sppf = B.T(5, 2 * c5);             // [a | mp5 | mp9 | mp13], each c5/2
    const int cat20 = B.T(5, c4 + c5);           // Concat[19, 9]: [model.19 out | model.9 out]
    const int cat17 = B.T(4, c3 + c4);           // Concat[16, 12]: [model.16 out | model.12 out]
    const int t15 = B.T(3, c3), t18 = B.T(4, c4), t21 = B.T(5, c5);
    {   // model.0
        Op o = B.base("model.0");
        o.kind = OPK_STEM; o.in0 = in; o.c0 = 3; o.out = t0;
        p.ops.push_back(o);
    }
    B.conv("model.1", t0, 0, t1, 0);
    B.c2f(2, B.cv1_single(2, t1, 0), 2, c2, n3, true, t2, 0);
    B.conv("model.3", t2, 0, t3, 0);
    B.c2f(4, B.cv1_single(4, t3, 0), 3, c3, n6, true, t4, 0);
    B.conv("model.5", t4, 0, t5, 0);
    B.c2f(6, B.cv1_single(6, t5, 0), 4, c4, n6, true, t6, 0);
    B.conv("model.7", t6, 0, t7, 0);
    B.c2f(8, B.cv1_single(8, t7, 0), 5, c5, n3, true, t8, 0);
    // SPPF: cv1 -> slice 0; three chained 5x5 max pools -> slices 1..3; cv2 -> cat20[c4:]
    B.conv("model.9.cv1", t8, 0, sppf, 0);
    for (int j = 0; j < 3; ++j) {
        Op o{};
        o.kind = OPK_POOL; o.conv = -1; o.in0 = sppf; o.in0_coff = j * (c5 / 2); o.c0 = c5 / 2;
        o.in1 = -1; o.res = -1; o.pred_level = -1; o.out = sppf; o.out_coff = (j + 1) * (c5 / 2);
        p.ops.push_back(o);
    }
    B.conv("model.9.cv2", sppf, 0, cat20, c4);
    {   // model.12: Concat[Upsample(9), 6] folded into cv1's gather
        Op o = B.base("model.12.cv1");
        o.in0 = cat20; o.in0_coff = c4; o.c0 = c5; o.up0 = 1;
        o.in1 = t6; o.in1_coff = 0; o.c1 = c4;
        B.c2f(12, o, 4, c4, n3, false, cat17, c3);
    }
    {   // model.15: Concat[Upsample(12), 4]
        Op o = B.base("model.15.cv1");
        o.in0 = cat17; o.in0_coff = c3; o.c0 = c4; o.up0 = 1;
        o.in1 = t4; o.in1_coff = 0; o.c1 = c3;
        B.c2f(15, o, 3, c3, n3, false, t15, 0);
    }
    B.conv("model.16", t15, 0, cat17, 0);
    B.c2f(18, B.cv1_single(18, cat17, 0), 4, c4, n3, false, t18, 0);
    B.conv("model.19", t18, 0, cat20, 0);
    B.c2f(21, B.cv1_single(21, cat20, 0), 5, c5, n3, false, t21, 0);
    const int feats[3] = {t15, t18, t21};
    for (int l = 0; l < 3; ++l) {
        const int lev = 3 + l;
        p.feat_level[l] = lev;
        const int b0 = B.T(lev, cb), b1 = B.T(lev, cb), k0 = B.T(lev, cc), k1 = B.T(lev, cc);
        const std::string bb = "model.22.cv2." + std::to_string(l), kk = "model.22.cv3." + std::to_string(l);
        B.conv(bb + ".0", feats[l], 0, b0, 0);
        B.conv(bb + ".1", b0, 0, b1, 0);
        { Op o = B.base(bb + ".2"); o.in0 = b1; o.c0 = cb; o.out = -1; o.pred_level = l; o.pred_coff = 0; p.ops.push_back(o); }
        B.conv(kk + ".0", feats[l], 0, k0, 0);
        B.conv(kk + ".1", k0, 0, k1, 0);
        { Op o = B.base(kk + ".2"); o.in0 = k1; o.c0 = cc; o.out = -1; o.pred_level = l; o.pred_coff = 64; p.ops.push_back(o); }
    }
    p.ok = true;
    return p;
}

// ---- weight files
namespace {
constexpr uint32_t MAX_CHANNELS = 65536;               // of a tensor and of a convolution's input / output

std::string parse_plan_v2(Reader& r, Plan* plan, FileHeader* h) {
    const uint32_t version = r.u32();                    // 3: conv headers carry a flags word (bit 0: a per-channel scale vector follows the bias)
    if (version != 2 && version != 3) return "unsupported CYW2 version";
    h->has_flags = version == 3;
    if (r.o + 12 > r.n) return "truncated weight file";
    plan->arch = std::string((const char*)r.p + r.o, strnlen((const char*)r.p + r.o, 8)); r.o += 8;
    plan->scale = (char)r.p[r.o]; r.o += 4;
    const uint32_t nc = r.u32(), nnames = r.u32(), nt = r.u32(), nops = r.u32(), nconv = r.u32();
    for (int l = 0; l < 3; ++l) plan->feat_level[l] = (int)r.u32();
    if (r.bad || nc < 1 || nc > 1000 || nt < 2 || nt > 4096 || nops < 1 || nops > 8192 || nconv < 1 || nconv > 4096)
        return "implausible CYW2 header";
    plan->nc = (int)nc;
    for (uint32_t i = 0; i < nnames && !r.bad; ++i) { uint32_t l = r.u32(); h->names.push_back(r.str(l)); }
    for (uint32_t i = 0; i < nt; ++i) { const int lev = (int)r.u32(), C = (int)r.u32(); plan->tensors.push_back({lev, C}); }
    for (uint32_t i = 0; i < nops; ++i) {
        int v[20];
        for (int j = 0; j < 20; ++j) v[j] = (int)r.u32();
        if (r.bad || v[0] < 0 || v[0] > OPK_ATTN) return "malformed op in CYW2 plan";
        Op o{};
        o.kind = (OpKind)v[0]; o.conv = v[1]; o.in0 = v[2]; o.in0_coff = v[3]; o.c0 = v[4]; o.up0 = v[5];
        o.in1 = v[6]; o.in1_coff = v[7]; o.c1 = v[8]; o.out = v[9]; o.out_coff = v[10]; o.res = v[11]; o.res_coff = v[12];
        o.pred_level = v[13]; o.pred_coff = v[14]; o.p0 = v[15]; o.p1 = v[16]; o.p2 = v[17]; o.p3 = v[18];
        const bool no_conv = o.kind == OPK_POOL || o.kind == OPK_ATTN;
        auto tok = [&](int t, bool opt) { return (opt && t < 0) || (t >= 0 && t < (int)nt); };
        if (!tok(o.in0, false) || !tok(o.in1, true) || !tok(o.out, true) || !tok(o.res, true) ||
            (!no_conv && (o.conv < 0 || o.conv >= (int)nconv)) || (o.out < 0 && (o.pred_level < 0 || o.pred_level > 2)))
            return "malformed op in CYW2 plan";
        if (no_conv) o.conv = -1;                        // pool and attention ops carry no convolution: whatever the file says there is never an index
        plan->ops.push_back(o);
    }
    for (auto& t : plan->tensors) if (t.level < 0 || t.level > 5 || t.C < 1 || t.C > (int)MAX_CHANNELS) return "malformed tensor in CYW2 plan";
    h->nconv = nconv;
    return "";
}
}  // namespace

std::string parse_header(Reader& r, Plan* plan, FileHeader* h) {
    if (r.n < 24 || (memcmp(r.p, "CYW1", 4) != 0 && memcmp(r.p, "CYW2", 4) != 0)) return "not a CYW weight file";
    h->v2 = memcmp(r.p, "CYW2", 4) == 0;
    r.o = 4;
    plan->ok = false;
    if (h->v2) {
        const std::string msg = parse_plan_v2(r, plan, h);
        plan->ok = msg.empty();
        return msg;
    }
    const uint32_t version = r.u32();
    if (version != 1 && version != 2) return "unsupported CYW version";
    h->has_flags = version == 2;                         // a flags word per conv header, as CYW2 version 3
    const char scale = (char)r.p[r.o]; r.o += 4;
    const uint32_t nc = r.u32();
    h->nconv = r.u32();
    const uint32_t nnames = r.u32();
    *plan = build_plan(scale, (int)nc);
    if (!plan->ok) { h->unsupported = true; return plan->err; }
    if (plan->convs.size() != h->nconv) return "weight file conv count does not match the graph";
    for (uint32_t i = 0; i < nnames && !r.bad; ++i) { uint32_t l = r.u32(); h->names.push_back(r.str(l)); }
    return "";
}

std::string next_conv(Reader& r, const FileHeader& h, Plan* plan, uint32_t i, ConvRecord* out) {
    const uint32_t co = r.u32(), ci = r.u32(), k = r.u32(), s = r.u32(), act = r.u32();
    const uint32_t groups = h.v2 ? r.u32() : 1u;
    const uint32_t flags = h.has_flags ? r.u32() : 0u;
    const uint32_t nl = r.u32();
    const std::string name = r.str(nl);
    if (r.bad) return "truncated weight file";
    if (h.v2) {
        if (co < 1 || ci < 1 || co > MAX_CHANNELS || ci > MAX_CHANNELS || groups < 1 || ci % groups || (k != 1 && k != 3) || (s != 1 && s != 2))
            return "malformed conv header: " + name;
        ConvDesc d; d.name = name; d.cin = (int)ci; d.cout = (int)co; d.k = (int)k; d.s = (int)s; d.act = (int)act; d.groups = (int)groups;
        plan->convs.push_back(d);
    } else {
        const ConvDesc& d = plan->convs[i];
        if (name != d.name || co != (uint32_t)d.cout || ci != (uint32_t)d.cin || k != (uint32_t)d.k || s != (uint32_t)d.s || act != (uint32_t)d.act)
            return "weight file layer " + name + " does not match graph layer " + d.name;
    }
    out->d = plan->convs[i];
    out->W = r.f32((size_t)co * (ci / groups) * k * k);      // (every factor is bounded above: at most 2^32 * 9 elements, no wrap)
    out->b = r.f32(co);
    // flags bit 0: scale[cout] with W[n] = fl32(w16[n] * scale[n]), w16 the checkpoint's fp16 filter (weights.py: fold(with_scale=True))
    out->wscale = (flags & 1u) ? r.f32(co) : nullptr;
    return r.bad ? "truncated weight file" : "";
}

// A CYW2 file carries its own execution plan; it is untrusted data.  Every channel slice an op names must lie inside its
// tensor, or the kernels would address outside the workspace (the tensors' extents are the buffer-resource bounds).
static std::string slice_fault(const Plan& p) {
    auto T = [&](int t) -> const Tensor& { return p.tensors[t]; };
    auto inside = [&](int t, int coff, long n) { return coff >= 0 && n >= 1 && (long)coff + n <= T(t).C; };      // (untrusted u32 fields: no int overflow)
    auto small = [](int v) { return v >= 1 && v <= (int)MAX_CHANNELS; };
    for (size_t i = 0; i < p.ops.size(); ++i) {
        const Op& o = p.ops[i];
        const std::string at = " in op " + std::to_string(i);
        if (o.kind == OPK_POOL) {
            if (o.out < 0 || !inside(o.in0, o.in0_coff, o.c0) || !inside(o.out, o.out_coff, o.c0) || T(o.in0).level != T(o.out).level)
                return "pool slice outside its tensor" + at;
            continue;
        }
        if (o.kind == OPK_ATTN) {
            if (o.out < 0 || !small(o.p0) || !small(o.p1) || !small(o.p2) || !inside(o.in0, o.in0_coff, (long)o.p0 * (2L * o.p1 + o.p2)) ||
                !inside(o.out, o.out_coff, (long)o.p0 * o.p2))
                return "attention slice outside its tensor" + at;
            continue;
        }
        const ConvDesc& d = p.convs[o.conv];
        if (o.kind == OPK_DWCONV) {
            // input channel of output channel ch: (ch / blk) * gstride + goff + ch % blk   (blk = 0: ch)
            const int last = d.cout - 1;
            const long cin_last = o.p0 > 0 ? (long)(last / o.p0) * o.p1 + o.p2 + last % o.p0 : last;
            if (o.out < 0 || o.p0 < 0 || o.p1 < 0 || o.p2 < 0 || (o.p0 > 0 && o.p0 % 8) || o.in0_coff < 0 ||
                o.in0_coff + cin_last + 1 > T(o.in0).C || !inside(o.out, o.out_coff, d.cout) ||
                (o.res >= 0 && !inside(o.res, o.res_coff, d.cout)))
                return "depth-wise slice outside its tensor" + at;
            continue;
        }
        if (o.kind == OPK_STEM) {
            if (o.out < 0 || !inside(o.out, o.out_coff, d.cout) || T(o.in0).C != 4 || d.cin != 3) return "malformed stem" + at;
            continue;
        }
        if (!inside(o.in0, o.in0_coff, o.c0) || (o.in1 >= 0 ? !inside(o.in1, o.in1_coff, o.c1) : o.c1 != 0) || o.c0 + o.c1 != d.cin)
            return "conv input slice does not match " + d.name + at;
        if (o.in1 >= 0 && (d.k != 1 || o.c0 % 64)) return "two-segment input needs a 1x1 conv and a 64-aligned boundary" + at;
        if (o.up0 && (d.k != 1 || T(o.in0).level < 1)) return "upsampled input needs a 1x1 conv" + at;
        if (o.out >= 0 && !inside(o.out, o.out_coff, d.cout)) return "conv output slice outside its tensor" + at;
        if (o.out < 0 && (o.pred_coff < 0 || (long)o.pred_coff + d.cout > 64 + p.nc)) return "head slice outside the prediction row" + at;
        if (o.res >= 0 && (!inside(o.res, o.res_coff, d.cout) || (o.out >= 0 && T(o.res).level != T(o.out).level)))
            return "residual slice outside its tensor" + at;
    }
    return "";
}

std::string validate_plan(const Plan& p) {
    const std::string bad = slice_fault(p);
    return bad.empty() ? bad : "malformed CYW2 plan: " + bad;
}

namespace {
bool plain_conv_pair(const Op& o, const Op& n) {          // two convolutions into tensors, the second reading the slice the first writes
    return n.kind == OPK_CONV && o.conv >= 0 && n.conv >= 0 && o.out >= 0 && n.out >= 0 && n.in0 == o.out && n.in0_coff == o.out_coff &&
           n.in1 < 0 && !n.up0;
}
int readers_of(const Plan& p, int t) {
    int readers = 0;
    for (const Op& q : p.ops) readers += (q.in0 == t) + (q.in1 == t) + (q.res == t);
    return readers;
}

// ops[i] = the stem, ops[i+1] = a 3x3 stride-2 SiLU convolution that is the ONLY reader of the stem's output and reads all of it:
// the candidate of stem_down_kernel (model.0 + model.1 in one launch).  The kernel exists for 64 -> 128 channels in the fp16
// context only; the forward pass sees that by the weight copies the loader packed for exactly those widths.
bool stem_down_pair(const Plan& p, size_t i) {
    const Op& o = p.ops[i]; const Op& n = p.ops[i + 1];
    if (o.kind != OPK_STEM || !plain_conv_pair(o, n) || n.res >= 0) return false;
    const ConvDesc& d0 = p.convs[o.conv]; const ConvDesc& d = p.convs[n.conv];
    if (d.k != 3 || d.s != 2 || !d.act || d.groups != 1 || d.cin != d0.cout || n.c0 != d0.cout) return false;
    return p.tensors[o.in0].C == 4 && p.tensors[o.out].C == d0.cout && readers_of(p, o.out) == 1;
}

// ops[i], ops[i+1] = the two 3x3 convs of a 64-channel Bottleneck (x [+] cv2(cv1(x))) whose intermediate has no other reader:
// with CY_BNECK_FUSE=1 they run as ONE kernel in the fp16 context (bneck64.hip; off by default: measured slower so far)
bool bneck_pair(const Plan& p, size_t i) {
    const Op& o = p.ops[i]; const Op& n = p.ops[i + 1];
    if (o.kind != OPK_CONV || !plain_conv_pair(o, n)) return false;
    const ConvDesc& d1 = p.convs[o.conv]; const ConvDesc& d2 = p.convs[n.conv];
    auto c64 = [](const ConvDesc& d) { return d.k == 3 && d.s == 1 && d.cin == 64 && d.cout == 64 && d.act && d.groups == 1; };
    if (!c64(d1) || !c64(d2)) return false;
    if (o.in1 >= 0 || o.up0 || o.res >= 0 || o.c0 != 64 || n.c0 != 64) return false;
    if (p.tensors[o.in0].level != p.tensors[o.out].level || p.tensors[o.in0].level != p.tensors[n.out].level) return false;
    if (n.res >= 0 && (n.res != o.in0 || n.res_coff != o.in0_coff)) return false;      // the shortcut adds the bottleneck's own input
    if (n.out == o.in0 && n.out_coff == o.in0_coff) return false;                        // in place: patches would read overwritten halos
    // the intermediate must be dead after cv2: the next op that touches its tensor (C2f reuses one scratch tensor for all its
    // bottlenecks) has to overwrite exactly this slice before anything reads it
    for (size_t j = i + 2; j < p.ops.size(); ++j) {
        const Op& q = p.ops[j];
        if (q.in0 == o.out || q.in1 == o.out || q.res == o.out) return false;
        if (q.out == o.out) return q.out_coff == o.out_coff && q.conv >= 0 && p.convs[q.conv].cout == 64;
    }
    return true;
}

// ops[i] = a convolution whose 256 output channels all sit in one tile of the pixels-direct kernel (3x3 stride 2 or 1x1, SiLU, no
// residual, one input segment), ops[i+1] = the 1x1 convolution (256 -> <= 256 channels, one input segment, no residual) that is the ONLY
// reader of its output: in the fp16 context the pair runs as one kernel, the first layer's accumulators feeding the second GEMM in
// registers (conv1x1_direct_kernel<..., FUSE2>; yolov8l: model.3 -> model.4.cv1).  CY_FUSE_PW=0 turns it off.
bool pw_pair(const Plan& p, size_t i) {
    const Op& o = p.ops[i]; const Op& n = p.ops[i + 1];
    if (o.kind != OPK_CONV || !plain_conv_pair(o, n)) return false;
    const ConvDesc& d1 = p.convs[o.conv]; const ConvDesc& d2 = p.convs[n.conv];
    if (d1.groups != 1 || d2.groups != 1 || d1.cout != 256 || !d1.act || d1.cin % 64) return false;
    if (!((d1.k == 3 && d1.s == 2 && d1.cin >= 128) || (d1.k == 1 && d1.s == 1))) return false;
    if (d2.k != 1 || d2.s != 1 || d2.cin != 256 || d2.cout > 256 || d2.cout % 16) return false;
    if (o.in1 >= 0 || o.up0 || o.res >= 0 || n.res >= 0 || n.c0 != 256) return false;
    if (p.tensors[o.out].level != p.tensors[n.out].level || n.out == o.out) return false;
    return readers_of(p, o.out) == 1;                     // nothing else may read the first layer's output (a later op may overwrite that tensor)
}

// ops[i], ops[i+1], ops[i+2] = the box branch of one detect-head level: a 3x3 s1 SiLU conv reading a feature map into a tensor of its
// own, a 3x3 s1 SiLU 64 -> 64 conv as its only reader, and the 1x1 (no activation) of THAT tensor's only reader into columns 0..63 of
// the prediction rows.  decode_kernel reads those columns at candidate anchors only, so the detect pass may compute the branch there
// alone (cy_sparse_box.hip; the gate is the forward pass's).
bool box_branch(const Plan& p, size_t i) {
    if (i + 2 >= p.ops.size()) return false;
    const Op& o = p.ops[i]; const Op& n = p.ops[i + 1]; const Op& h = p.ops[i + 2];
    if (o.kind != OPK_CONV || !plain_conv_pair(o, n) || h.kind != OPK_CONV || h.conv < 0) return false;
    const ConvDesc& d0 = p.convs[o.conv]; const ConvDesc& d1 = p.convs[n.conv]; const ConvDesc& d2 = p.convs[h.conv];
    auto c3 = [](const ConvDesc& d) { return d.k == 3 && d.s == 1 && d.act && d.groups == 1 && d.cout == 64; };
    if (!c3(d0) || !c3(d1) || d1.cin != 64 || d0.cin % 64 || o.c0 != d0.cin || n.c0 != 64) return false;
    if (d2.k != 1 || d2.s != 1 || d2.act || d2.groups != 1 || d2.cin != 64 || d2.cout != 64) return false;
    if (o.in1 >= 0 || o.up0 || o.res >= 0 || n.res >= 0 || o.out_coff != 0 || n.out_coff != 0) return false;
    if (h.out >= 0 || h.pred_coff != 0 || h.in0 != n.out || h.in0_coff != 0 || h.c0 != 64 || h.in1 >= 0 || h.up0 || h.res >= 0) return false;
    if (p.tensors[o.out].C != 64 || p.tensors[n.out].C != 64 || o.out == n.out || o.in0 == o.out || o.in0 == n.out) return false;
    const int lev = p.tensors[o.in0].level;
    if (lev != 3 + h.pred_level || p.tensors[o.out].level != lev || p.tensors[n.out].level != lev) return false;
    // the two intermediates belong to the branch: written by it alone, read by it alone
    int writers0 = 0, writers1 = 0;
    for (const Op& q : p.ops) { writers0 += q.out == o.out; writers1 += q.out == n.out; }
    return writers0 == 1 && writers1 == 1 && readers_of(p, o.out) == 1 && readers_of(p, n.out) == 1;
}
}  // namespace

void mark_fusions(Plan& p) {
    for (size_t i = 0; i < p.ops.size(); ++i) {
        Op& o = p.ops[i];
        o.fuse = FUSE_NONE;
        if (o.box == 0 && box_branch(p, i)) { o.box = 1; p.ops[i + 1].box = 2; p.ops[i + 2].box = 3; }
        if (i + 1 >= p.ops.size()) continue;
        if (bneck_pair(p, i)) o.fuse = FUSE_BNECK_PAIR;         // (the three exclude one another: 64 / 256 output channels, the stem)
        else if (stem_down_pair(p, i)) o.fuse = FUSE_STEM_DOWN;
        else if (pw_pair(p, i)) o.fuse = FUSE_PW_PAIR;
    }
}

}  // namespace cy
