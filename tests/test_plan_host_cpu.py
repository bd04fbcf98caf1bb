"""The host side of a weight load (caesar_yolo_amd/csrc/cy_plan.cpp) on the CPU: the CYW1 / CYW2 header and plan parse, the walk over
the conv records, the plan's slice checks and the fusion marks.  A weight file is untrusted data (a CYW2 file carries its own
execution plan), so the code is linked alone into tests/host/plan_main.cpp, built here with AddressSanitizer and UBSan and run as a
child process on images in exactly sized heap buffers; a sanitizer report ends the child with a non-zero status and fails the test.
Inputs: weights.write_cyw / write_cyw2 on seeded graphs (YOLOv8 n and l, YOLO11 n and l, nc = 3)."""
import copy
import os
import shutil
import struct
import subprocess

import pytest

from caesar_yolo_amd import weights as W
from caesar_yolo_amd import yolo11_graph as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
NAMES = {0: "a", 1: "b", 2: "c"}
VALUES = (0, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 65537)
STEM_DOWN, PW_PAIR, BNECK_PAIR = 1, 2, 3
PREFIX = "malformed CYW2 plan: "
# Fusion marks {op index: mark} of the seven plans.  Generated once by a scratch program (not part of the repository) that linked the
# predicate text of the commit before the marks existed (bneck_pair and pw_pair as they stood in cy_runtime.hip; the structural lines
# of stem_fusable with the stem's own width in place of the kernel's 64: the kernel's widths are seen at run time by the weight
# copies packed for them, so op 0 of "l" -- 64 channels -- is the one candidate a forward pass can take).
MARKS = {"yolov8n": {0: 1, 15: 3, 17: 3, 20: 2, 24: 2, 31: 3, 40: 3, 48: 3, 51: 3},
         "yolov8s": {0: 1, 8: 3, 10: 3, 13: 2, 35: 3},
         "yolov8m": {0: 1},
         "yolov8l": {0: 1, 3: 3, 5: 3, 7: 3, 10: 2},
         "yolov8x": {0: 1},
         "yolo11n": {0: 1, 21: 2, 25: 3, 27: 3, 30: 2, 35: 2, 61: 3, 63: 3, 67: 3},
         "yolo11l": {0: 1, 18: 2, 22: 3, 24: 3, 29: 3, 31: 3, 107: 3, 109: 3, 114: 3, 116: 3}}
OPS = {"yolov8n": 66, "yolov8s": 66, "yolov8m": 86, "yolov8l": 106, "yolov8x": 106, "yolo11n": 91, "yolo11l": 178}


@pytest.fixture(scope="session")
def tool(tmp_path_factory):
    """The sanitized program, built once: the clang++ beside hipcc, else g++; no compiler is a failure."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    near = [os.path.join(os.path.dirname(hipcc), d, "clang++") for d in (".", "../llvm/bin", "../lib/llvm/bin")]
    cxx = next((c for c in near if os.path.exists(c)), None) or shutil.which("g++")
    assert cxx, "no clang++ beside hipcc and no g++: the plan checks cannot be checked"
    d = tmp_path_factory.mktemp("plan_host")
    exe = str(d / "plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "plan_main.cpp"), os.path.join(CSRC, "cy_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, "plan_main %s: exit %d\n%s" % (" ".join(str(a) for a in args)[:200], r.returncode, r.stderr[-4000:])
        return r.stdout.splitlines()
    run.dir = d
    return run


def full(lines):
    """The full verdict -> the error message, or {"ops": n, "marks": {op: mark}, "convs": [(name, cin, cout, k, s, act, groups)]}."""
    if lines[0].startswith("error: "):
        return lines[0][7:]
    out = {"ops": int(lines[0].split()[1]), "marks": {}, "convs": []}
    for ln in lines[1:]:
        f = ln.split()
        if f[0] == "mark":
            out["marks"][int(f[1])] = int(f[2])
        else:
            out["convs"].append((f[1],) + tuple(int(v) for v in f[2:]))
    return out


def cases(tool, image, lines):
    """Short verdicts ("ok N" / the message) of the mutations `lines` of one image file."""
    path = str(tool.dir / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = tool(image, path)
    assert len(out) == len(lines)
    return [ln[7:] if ln.startswith("error: ") else ln for ln in out]


def write11(path, g):
    wd = W.seeded11_draw(g)
    W.write_cyw2(str(path), g, [(cs,) + wd[cs.name] for cs in g.convs], NAMES)
    return str(path)


@pytest.fixture(scope="session")
def images(tool):
    """{name: (path, graph or None)} of the four seeded files."""
    out = {}
    for sc in "nl":
        g = G.build(sc, 3)
        out["yolo11" + sc] = (write11(tool.dir / ("y11%s.cyw" % sc), g), g)
        p = str(tool.dir / ("y8%s.cyw" % sc))
        W.write_cyw(p, W.fold(W.seeded_checkpoint(sc, 3), sc, 3, with_scale=sc == "n"), NAMES, sc)      # (n: flags word and scale vectors)
        out["yolov8" + sc] = (p, None)
    return out


class Layout:
    """Byte offsets of the u32 fields of an image: header counts, op records (CYW2) and conv headers, with every conv's spans."""
    def __init__(self, path):
        buf = open(path, "rb").read()
        self.size, self.v2 = len(buf), buf[:4] == b"CYW2"
        u = lambda o: struct.unpack_from("<I", buf, o)[0]
        if self.v2:
            flags = u(4) == 3
            self.counts = {"nc": 20, "nnames": 24, "nt": 28, "nops": 32, "nconv": 36, "feat0": 40, "feat1": 44, "feat2": 48}
            nnames, nt, nops, nconv = u(24), u(28), u(32), u(36)
            o = 52
        else:
            flags = u(4) == 2
            self.counts = {"nc": 12, "nconv": 16, "nnames": 20}
            nnames, nt, nops, nconv = u(20), 0, 0, u(16)
            o = 24
        for _ in range(nnames):
            o += 4 + (u(o) + 3) // 4 * 4
        o += 8 * nt
        self.ops = [o + 80 * i for i in range(nops)]
        o += 80 * nops
        self.plan_end = o
        self.convs = []                                    # (name, {field: offset}, weights offset, bias offset, end)
        keys = ["co", "ci", "k", "s", "act"] + (["groups"] if self.v2 else []) + (["flags"] if flags else []) + ["nl"]
        for _ in range(nconv):
            fld = {k: o + 4 * i for i, k in enumerate(keys)}
            co, ci, k = u(fld["co"]), u(fld["ci"]), u(fld["k"])
            groups = u(fld["groups"]) if self.v2 else 1
            nl = u(fld["nl"])
            o = fld["nl"] + 4
            name = buf[o:o + nl].decode()
            o += (nl + 3) // 4 * 4
            w0 = o
            b0 = w0 + 4 * co * (ci // groups) * k * k
            o = b0 + 4 * co * (2 if flags and u(fld["flags"]) & 1 else 1)
            self.convs.append((name, fld, w0, b0, o))
        assert o == len(buf), (o, len(buf))


# ---- accepted files and their marks
def test_fusion_marks_of_the_seven_plans(tool, images):
    got = {name: full(tool(path)) for name, (path, _) in images.items()}
    for sc in "smx":
        got["yolov8" + sc] = full(tool("--graph", sc, 3))
    for name, res in got.items():
        assert not isinstance(res, str), (name, res)
        assert res["ops"] == OPS[name] and res["marks"] == MARKS[name], name
    for sc in "nl":                                        # the built-in graph and the file that names it agree
        assert full(tool("--graph", sc, 3)) == got["yolov8" + sc]
    # yolov8 l has exactly one pixel-wise pair, model.3 -> model.4.cv1: op 10 (before it the stem, model.1, model.2.cv1, three
    # bottlenecks of two convolutions and model.2.cv2), model.4.cv1 the conv record behind model.3's
    l8 = got["yolov8l"]
    assert [i for i, m in l8["marks"].items() if m == PW_PAIR] == [10]
    names = [c[0] for c in l8["convs"]]
    assert names[:2] == ["model.0", "model.1"] and names.index("model.4.cv1") == names.index("model.3") + 1 == 11
    # n and l have the stem+down candidate (op 0, the stem; a stride-2 3x3 behind it), the stem having 64 output channels in l
    for name in ("yolov8n", "yolov8l", "yolo11n", "yolo11l"):
        res = got[name]
        assert res["marks"][0] == STEM_DOWN and res["convs"][0][0] == "model.0" and res["convs"][1][3:5] == (3, 2), name
        assert res["convs"][0][2] == (64 if name.endswith("l") else 16) and res["convs"][1][1] == res["convs"][0][2], name
    # conv descriptors as the graphs give them
    for name, (_, g) in images.items():
        if g is not None:
            assert got[name]["convs"] == [(cs.name, cs.cin, cs.cout, cs.k, cs.s, int(cs.act), cs.groups) for cs in g.convs], name


# ---- messages
def mutated(tool, g, edit):
    g = copy.deepcopy(g)
    edit(g)
    return full(tool(write11(tool.dir / "bad.cyw", g)))


@pytest.mark.parametrize("field,delta,message", [("out_coff", 8, "conv output slice outside its tensor"),
                                                 ("in0_coff", 8, "conv input slice does not match"),
                                                 ("res_coff", 1 << 20, "residual slice outside its tensor"),
                                                 ("c0", 64, "conv input slice does not match")])
def test_the_four_gpu_mutations_give_the_same_messages(tool, images, field, delta, message):
    """The mutations of test_gpu_yolo11.py::test_malformed_cyw2_plan_is_refused, refused with the message the GPU load reports."""
    g = images["yolo11n"][1]
    k = [i for i, o in enumerate(g.ops) if o["kind"] == 1 and o["out"] >= 0 and (field != "res_coff" or o["res"] >= 0)][3]

    def edit(g):
        g.ops[k][field] += delta
    msg = mutated(tool, g, edit)
    assert isinstance(msg, str) and msg.startswith(PREFIX + message) and msg.endswith(" in op %d" % k), msg


def first(g, pred):
    return next(i for i, o in enumerate(g.ops) if pred(o))


def test_every_kind_of_op_has_a_refused_mutation(tool, images):
    g0 = images["yolo11n"][1]
    conv3 = lambda g, o: o["kind"] == 1 and g.convs[o["conv"]].k == 3

    def two_segment(g):                                  # the boundary between the segments moved by 8 channels, both slices still inside
        k = first(g, lambda o: o["in1"] >= 0)
        o = g.ops[k]
        lev, C = g.tensors[o["in1"]]
        g.tensors[o["in1"]] = (lev, C + 8)
        o["c0"] -= 8
        o["c1"] += 8
        return k
    edits = [("pool slice outside its tensor", lambda g: g.ops[first(g, lambda o: o["kind"] == 2)].__setitem__("out_coff", 1 << 20)),
             ("attention slice outside its tensor", lambda g: g.ops[first(g, lambda o: o["kind"] == 4)].__setitem__("p0", 1000)),
             ("attention slice outside its tensor", lambda g: g.ops[first(g, lambda o: o["kind"] == 4)].__setitem__("p1", 0x7FFFFFFF)),
             ("depth-wise slice outside its tensor", lambda g: g.ops[first(g, lambda o: o["kind"] == 3)].__setitem__("out_coff", 1 << 20)),
             ("depth-wise slice outside its tensor", lambda g: g.ops[first(g, lambda o: o["kind"] == 3)].__setitem__("p0", 4)),
             ("malformed stem", lambda g: g.ops[first(g, lambda o: o["kind"] == 0)].__setitem__("out_coff", 8)),
             ("two-segment input needs a 1x1 conv and a 64-aligned boundary", two_segment),
             ("upsampled input needs a 1x1 conv", lambda g: g.ops[first(g, lambda o: conv3(g, o) and o["out"] >= 0)].__setitem__("up0", 1)),
             ("head slice outside the prediction row", lambda g: g.ops[first(g, lambda o: o["out"] < 0 and o["pred_coff"] == 64)].__setitem__("pred_coff", 72)),
             ("head slice outside the prediction row", lambda g: g.ops[first(g, lambda o: o["out"] < 0)].__setitem__("pred_coff", 0x7FFFFFFF))]
    for message, edit in edits:
        msg = mutated(tool, g0, edit)
        assert isinstance(msg, str) and msg.startswith(PREFIX + message + " in op "), (message, msg)
    # a pool op's conv field is no index: whatever stands there, the file loads and the marks are the same
    res = mutated(tool, g0, lambda g: g.ops[first(g, lambda o: o["kind"] == 2)].__setitem__("conv", 65537))
    assert not isinstance(res, str) and res["marks"] == MARKS["yolo11n"]


# ---- field sweep
def test_field_sweep_gives_a_verdict_for_every_value(tool, images):
    """Each u32 field of every op record, the header counts and each field of every conv header, set in turn to 0, 0xFFFFFFFF,
    0x7FFFFFFF, 0x80000000 and 65537: a verdict (accepted or a message) each time, never a sanitizer report."""
    for name in ("yolo11n", "yolov8n"):
        path = images[name][0]
        lay = Layout(path)
        assert lay.v2 == (name == "yolo11n")
        sets = [("count " + k, o) for k, o in lay.counts.items()]
        sets += [("op %d field %d" % (i, j), o + 4 * j) for i, o in enumerate(lay.ops) for j in range(20)]
        sets += [("conv %s %s" % (cname, k), o) for cname, fld, _, _, _ in lay.convs for k, o in fld.items()]
        lines = ["set %d %d" % (o, v) for _, o in sets for v in VALUES]
        got = cases(tool, path, lines)
        assert all(v == "ok %d" % OPS[name] or (v and not v.startswith("ok")) for v in got)
        verdicts = {(what, v): got[5 * i + j] for i, (what, _) in enumerate(sets) for j, v in enumerate(VALUES)}
        refused = sum(not v.startswith("ok") for v in got)
        print("%s: %d mutations, %d refused" % (name, len(got), refused))
        assert refused > len(got) // 2
        if not lay.v2:
            continue
        # a conv header with co or ci above 65536 is refused by the header check, which names the layer
        for cname, fld, _, _, _ in lay.convs:
            for k in ("co", "ci"):
                for v in VALUES[1:]:
                    assert verdicts[("conv %s %s" % (cname, k), v)] == "malformed conv header: " + cname, (cname, k, v)
        assert verdicts[("count nconv", 0)] == "implausible CYW2 header" and verdicts[("count nnames", 0xFFFFFFFF)] == "malformed op in CYW2 plan"


# ---- truncation
def test_every_cut_is_refused(tool, images):
    """The file cut at every 4-byte boundary of the header and plan section, and inside the weights and inside the bias of the
    first, the middle and the last conv record: "truncated", "malformed" or "implausible" every time (below the 24 bytes of the
    shortest header: "not a CYW weight file", before anything is read), never a sanitizer report."""
    for name in ("yolo11n", "yolov8n"):
        path = images[name][0]
        lay = Layout(path)
        cuts = list(range(0, lay.plan_end + 4, 4))
        for cname, fld, w0, b0, end in (lay.convs[0], lay.convs[len(lay.convs) // 2], lay.convs[-1]):
            cuts += [fld["co"] + 4, fld["nl"], w0, w0 + 4, (w0 + b0) // 8 * 4, b0 - 4, b0, b0 + 4, end - 4]
        cuts += [lay.size - 4]
        got = cases(tool, path, ["cut %d" % c for c in cuts])
        for c, v in zip(cuts, got):
            if c < 24:
                assert v == "not a CYW weight file", (name, c, v)
            else:
                assert any(w in v for w in ("truncated", "malformed", "implausible")) and not v.startswith("ok"), (name, c, v)
        assert cases(tool, path, ["cut %d" % lay.size]) == ["ok %d" % OPS[name]]
