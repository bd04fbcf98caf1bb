"""The conv dispatch (caesar_yolo_amd/csrc/cy_conv_plan.cpp: conv_choose, conv_second_copy, conv_geometry) on the CPU.  The code is
linked with cy_plan.cpp alone into tests/host/conv_plan_main.cpp, built here with AddressSanitizer and UBSan and run as a child
process; a sanitizer report ends the child with a non-zero status and fails the test.

What is asked of it:
  * every row of the tables the GPU test runs (conv_slices_ref.SHAPES / X3 / F32 / ROW_CASES) selects the variant that test asserts,
    and the rows whose comments name an instantiation select that instantiation;
  * the 25 cases of test_gpu_conv_tail.py select the instantiation each case's comment names;
  * every ConvKernel value is selected by some row;
  * the four graphs (YOLOv8 n, l, YOLO11 n, l) at four input sizes, three batch sizes and five contexts, at default knobs, select
    what tests/golden/conv_dispatch.txt records.

tests/golden/conv_dispatch.txt was written once, by `dispatch_lines` below, from the text of the commit BEFORE the dispatch moved
into cy_conv_plan.cpp, not from the code under test: a scratch program (not part of the repository) held that commit's conv_variant_x3,
conv_variant, head_direct, strip_* / *_cover and upload_conv's `second` predicate verbatim (reading the environment, which the
scratch program set per query), that commit's conv_args geometry, and its launch_conv / launch_strip with every
`return launch_x<...>(a, s)` replaced by the name conv_kernel_name now gives that launcher call.  File format: the legend of
variant and kernel numbers, then one line per distinct layer geometry,
    Hi Wi Cin Cout k s c0 c1 up0 out_f32 out_bs out_ro act res : 15 tokens
a token per (context, B) in the order of CONTEXTS x BATCHES: variant/kernel, then `s` when the layer has the second weight copy
(wgt32) and `f` when the forward pass sets wgt2 (first op of a pixel-wise pair)."""
import os
import shutil
import subprocess

import pytest

import conv_slices_ref as R
import test_gpu_conv_tail as TAIL
from test_plan_host_cpu import NAMES, write11
from caesar_yolo_amd import weights as W
from caesar_yolo_amd import yolo11_graph as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_dispatch.txt")
PREC = {"fp16": 0, "fp32": 1, "fp16x3": 2}
# ConvKnobs in field order: environment name, default
KNOBS = (("CY_BATCH_INVARIANT", 1), ("CY_STRIP", 1), ("CY_WIDE_DUAL", 1), ("CY_DIRECT_MIN_BLOCKS", 256), ("CY_HEAD_DIRECT", 1),
         ("CY_NARROW_DIRECT", 1), ("CY_HEAD_PAIR", 1), ("CY_WIDE_PERSIST", 1), ("CY_X3_PERSIST", 0))
SIZES = ((512, 512), (640, 640), (416, 512), (128, 128))
BATCHES = (1, 64, 256)
CONTEXTS = (("fp16", 0, 1), ("fp16", 0, 0), ("fp16x3", 2, 1), ("fp16x3", 3, 1), ("fp32", 0, 1))      # precision, passes, CY_BATCH_INVARIANT

ONE_PATCH, PERSIST, STRIP10, STRIP12 = ("conv3x3_wide_kernel<2> one patch", "conv3x3_widep_kernel<0> persistent", "conv3x3_widep_kernel<10> strip",
                                        "conv3x3_widep_kernel<12> strip")
# the rows of the shared tables whose comments name the instantiation
NAMED = {"halo": "conv3x3_halo_kernel<2,2>", "halo2": "conv3x3_halo2_kernel", "wide": ONE_PATCH, "wide-persist": PERSIST, "strip": STRIP10,
         "direct256-3x3s2": "conv1x1_direct_kernel<4,2,3,K3>", "direct128-3x3s2": "conv1x1_direct_kernel<2,4,2,K3>"}
# the geometries of test_gpu_conv_tail.FP16 (X3 and F32 reuse them): the instantiation each case's comment names
TAIL_KERNEL = {(1, 10, 32, 128, 200, 3, 1): ONE_PATCH,
               (3, 9, 15, 128, 200, 3, 1): "conv3x3_wide_kernel<2,dual>",
               (1, 10, 20, 128, 200, 3, 1): "conv3x3_halo2_kernel",
               (1, 10, 20, 64, 200, 3, 1): "conv3x3_halo_kernel<2,2>",
               (1, 10, 32, 128, 40, 3, 1): "conv3x3_wide_kernel<1>",
               (2, 10, 18, 128, 40, 3, 1): "conv3x3_pp_kernel<2>",
               (2, 20, 18, 64, 40, 3, 1): "conv3x3_c64_kernel<64>",
               (2, 9, 11, 128, 200, 1, 1): "conv1x1_direct_kernel<4,2,3>",
               (2, 9, 11, 128, 72, 1, 1): "conv1x1_direct_kernel<2,2,2>",
               (2, 18, 22, 128, 200, 3, 2): "conv1x1_direct_kernel<4,2,3,K3>",
               (2, 9, 11, 128, 40, 1, 1): "head1x1_kernel",
               (2, 9, 15, 72, 200, 1, 1): "conv_igemm_kernel<4,2,4,3>",
               (2, 9, 11, 72, 40, 1, 1): "conv_igemm_kernel<4,1,2>",
               (2, 9, 11, 72, 200, 1, 1): "conv_igemm_kernel<2,2,4>"}
# instantiations no row above selects: the wider strip (maps above 62 px), the 32-channel persistent kernel's partner is in SHAPES;
# the fused pairs (wgt2 set, as the forward pass does for the first op of a pixel-wise pair) and their refusals
EXTRA = (("fp16", (2, 20, 70, 128, 208, 3, 1), {"CY_STRIP": "2"}, dict(), STRIP12),
         ("fp16x3", (2, 20, 70, 128, 208, 3, 1), {}, dict(), STRIP12),
         ("fp16", (2, 9, 11, 128, 256, 1, 1), R.DIRECT, dict(wgt2=1, res=0), "conv1x1_direct_kernel<4,2,3,FUSE2>"),
         ("fp16", (2, 18, 22, 128, 256, 3, 2), R.DIRECT, dict(wgt2=1, res=0), "conv1x1_direct_kernel<4,2,3,K3,FUSE2>"),
         ("fp16", (2, 9, 11, 128, 256, 1, 1), R.DIRECT, dict(wgt2=1, res=1), "conv1x1_direct_kernel<4,2,3>"),            # a residual: no pair
         ("fp16", (2, 9, 11, 128, 320, 1, 1), R.DIRECT, dict(wgt2=1, res=0), "conv1x1_direct_kernel<4,2,3>"),            # two channel tiles: no pair
         ("fp16x3", (2, 9, 11, 128, 256, 1, 1), {}, dict(wgt2=1, res=0), "conv1x1_direct_kernel<4,2,3>"))


@pytest.fixture(scope="session")
def tool(tmp_path_factory):
    """The sanitized program, built once: the clang++ beside hipcc, else g++; no compiler is a failure."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    near = [os.path.join(os.path.dirname(hipcc), d, "clang++") for d in (".", "../llvm/bin", "../lib/llvm/bin")]
    cxx = next((c for c in near if os.path.exists(c)), None) or shutil.which("g++")
    assert cxx, "no clang++ beside hipcc and no g++: the conv dispatch cannot be checked"
    d = tmp_path_factory.mktemp("conv_plan_host")
    exe = str(d / "conv_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "conv_plan_main.cpp"), os.path.join(CSRC, "cy_conv_plan.cpp"), os.path.join(CSRC, "cy_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, "conv_plan_main %s: exit %d\n%s" % (" ".join(str(a) for a in args)[:200], r.returncode, r.stderr[-4000:])
        return r.stdout.splitlines()
    run.dir = d
    return run


def case_line(prec, geom, inv, env, layout="dense", rows=None, act=1, res=1, split=3, wgt2=0):
    """One line of a conv_plan_main case file: the convolution as cy_conv_slices lays it out (conv_slices_ref.build)."""
    two = layout in ("concat", "upcat")
    knobs = dict(KNOBS, CY_BATCH_INVARIANT=int(inv))
    knobs.update({k: int(v) for k, v in env.items()})
    assert set(knobs) == set(k for k, _ in KNOBS)
    f = [PREC[prec]] + list(geom) + [geom[3] - R.SEG0 if two else 0, int(layout == "upcat")]
    f += [1, rows["out_bs"], rows["out_ro"]] if rows else [0, 0, 0]
    f += [int(act), int(res), split, wgt2] + [knobs[k] for k, _ in KNOBS]
    return " ".join(str(v) for v in f)


def choose(tool, lines):
    """-> [(variant name, kernel name)] of the case lines"""
    path = str(tool.dir / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = tool("--cases", path)
    assert len(out) == len(lines)
    return [tuple(ln.split(" | ")) for ln in out]


def table_cases():
    """(id, expected first word of the variant, expected kernel or None, case line) of every row of the shared tables, in every layout"""
    out = []
    for prec, table in (("fp16", R.SHAPES), ("fp16x3", R.X3), ("fp32", R.F32)):
        for name, (geom, inv, env, variant, two) in table.items():
            for layout in ("dense",) + (R.TWO if two else ()):
                g = (geom[0], geom[1] + geom[1] % 2, geom[2] + geom[2] % 2) + geom[3:] if layout == "upcat" else geom
                for split in (2, 3) if prec == "fp16x3" else (0,):
                    out.append(("%s-%s-%s-%d" % (prec, name, layout, split), variant, NAMED.get(name) if prec != "fp32" else None,
                                case_line(prec, g, inv if prec == "fp16" else "1", env, layout, split=split)))
    for what, prec, geom, hd, variant, rows, _ in R.ROW_CASES:
        for split in (2, 3) if prec == "fp16x3" else (0,):
            out.append(("%s-%d" % (what, split), variant, None, case_line(prec, geom, "1", {"CY_HEAD_DIRECT": hd}, "rows", rows, act=0, res=0, split=split)))
    return out


def tail_cases():
    """(id, kernel, case line) of the 25 cases of test_gpu_conv_tail.py as its check runs them: dense, residual, CY_WIDE_DUAL=2"""
    assert len(TAIL.ALL) == 25 and set(c[0] for c in TAIL.FP16) == set(TAIL_KERNEL)
    return [("%s-%s" % (prec, "x".join(map(str, geom))), TAIL_KERNEL[geom], case_line(prec, geom, inv, dict(knobs, CY_WIDE_DUAL="2"), act=n % 2 == 0))
            for n, (prec, geom, inv, knobs) in enumerate(TAIL.ALL)]


def test_shared_tables_select_the_variants_the_gpu_test_asserts(tool):
    cases = table_cases()
    got = choose(tool, [c[3] for c in cases])
    for (what, variant, kernel, _), (v, k) in zip(cases, got):
        assert v.split(" ")[0] == variant, "%s: %r, the table says %s" % (what, v, variant)
        assert kernel is None or k == kernel, "%s: %r, the row's comment names %s" % (what, k, kernel)
    named = set(c[0].split("-%s-" % "dense")[0] for c in cases if c[2])
    assert named == set("fp16-" + n for n in NAMED) | set("fp16x3-" + n for n in NAMED if n in R.X3)
    # the persistent form in both contexts, each by its own switch
    both = dict((c[0], k) for c, (_, k) in zip(cases, got))
    assert both["fp16-wide-persist-dense-0"] == both["fp16x3-wide-persist-dense-3"] == PERSIST


def test_tail_cases_select_the_instantiation_their_comments_name(tool):
    cases = tail_cases()
    got = choose(tool, [c[2] for c in cases])
    for (what, kernel, _), (v, k) in zip(cases, got):
        assert k == kernel, "%s: %r (%s), the comment names %s" % (what, k, v, kernel)


def test_wide_kernel_takes_the_persistent_form_by_the_real_batch(tool):
    """Under CY_BATCH_INVARIANT=1 the variant does not move with the batch; the persistent / one-patch form below it does (512
    patches; bit-identical results) -- model.4's bottleneck convs on 512-px tiles: 64 x 64 maps, 128 channels."""
    geom = lambda B: (B, 64, 64, 128, 128, 3, 1)
    got = choose(tool, [case_line("fp16", geom(B), "1", {}) for B in (1, 63, 64, 256)])
    assert [v.split(" ")[0] for v, _ in got] == [R.WIDE] * 4
    assert [k for _, k in got] == [ONE_PATCH, ONE_PATCH, PERSIST, PERSIST]
    # not above two slab pairs, not with a ragged 16-channel group, not when switched off
    assert choose(tool, [case_line("fp16", (256, 64, 64, 192, 128, 3, 1), "1", {}), case_line("fp16", (256, 64, 64, 128, 200, 3, 1), "1", {}),
                         case_line("fp16", geom(256), "1", {"CY_WIDE_PERSIST": "0"})]) == [(got[0][0], ONE_PATCH)] * 3


def test_fp16x3_without_passes_or_scale_is_an_argument_error(tool):
    got = choose(tool, [case_line("fp16x3", (2, 9, 11, 128, 200, 1, 1), "1", {}, split=s) for s in (0, 1, 4, 3)])
    assert [k for _, k in got] == ["bad fp16x3 arguments"] * 3 + ["conv1x1_direct_kernel<4,2,3>"]
    assert len(set(v for v, _ in got)) == 1                      # the variant is named all the same


def write_images(d):
    """{name: path} of the four seeded weight files, as test_plan_host_cpu.py writes them"""
    out = {}
    for sc in "nl":
        out["yolo11" + sc] = write11(d / ("y11%s.cyw" % sc), G.build(sc, 3))
        out["yolov8" + sc] = str(d / ("y8%s.cyw" % sc))
        W.write_cyw(out["yolov8" + sc], W.fold(W.seeded_checkpoint(sc, 3), sc, 3, with_scale=sc == "n"), NAMES, sc)
    return out


def dispatch_lines(run, images, workdir):
    """The golden file's lines from a conv_plan_main-like program `run` (module docstring: the file format)."""
    names = run("--names")
    num = {}
    for ln in names:
        kind, i, name = ln.split(" ", 2)
        num[(kind, name)] = i
    combos = [(B, PREC[prec], split, inv) for prec, split, inv in CONTEXTS for B in BATCHES]
    lines = set()
    for name in sorted(images):
        qpath = os.path.join(str(workdir), "queries.txt")
        with open(qpath, "w") as f:
            for H, W_ in SIZES:
                for B, p, split, inv in combos:
                    f.write("%d %d %d %d %d %d\n" % (B, H, W_, p, split, inv))
        out = run(images[name], qpath)
        blocks = []
        for ln in out:
            if ln.startswith("query "):
                blocks.append([])
            else:
                blocks[-1].append(ln)
        assert len(blocks) == len(SIZES) * len(combos) and len(set(len(b) for b in blocks)) == 1
        for si in range(len(SIZES)):
            per = blocks[si * len(combos):(si + 1) * len(combos)]
            for rows in zip(*per):                              # one op under every (context, B)
                keys, toks = set(), []
                for (B, _, _, _), ln in zip(combos, rows):
                    geo, variant, kernel = ln.split(" | ")
                    g = geo.split()
                    assert int(g[0]) == B
                    keys.add(" ".join(g[1:15]))
                    toks.append("%s/%s%s%s" % (num[("variant", variant)], num[("kernel", kernel)], "s" if g[15] == "1" else "", "f" if g[16] == "1" else ""))
                assert len(keys) == 1, keys
                lines.add(keys.pop() + " : " + " ".join(toks))
    return names + sorted(lines, key=lambda ln: [int(v) for v in ln.split(" : ")[0].split()] + [ln])


def test_the_four_graphs_select_what_the_parent_commit_selected(tool):
    got = dispatch_lines(tool, write_images(tool.dir), tool.dir)
    want = open(GOLDEN).read().splitlines()
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g == w
    num = dict((ln.split(" ", 2)[2], ln.split(" ", 2)[1]) for ln in want if ln.startswith("kernel "))
    rows = [ln.split(" : ") for ln in want if " : " in ln]
    # one layer whose wide kernel runs one-patch at B = 1 and persistent at B = 256 with batch invariance on (tokens 0 and 2)
    assert any(t.split()[0].split("/")[1].rstrip("sf") == num[ONE_PATCH] and t.split()[2].split("/")[1].rstrip("sf") == num[PERSIST] for _, t in rows)
    assert os.path.getsize(GOLDEN) < 256 * 1024


def test_every_kernel_value_is_selected_by_some_row(tool):
    extra = choose(tool, [case_line(prec, geom, "1", env, **kw) for prec, geom, env, kw, _ in EXTRA])
    assert [k for _, k in extra] == [e[4] for e in EXTRA]
    seen = set(k for _, k in extra)
    seen |= set(k for _, k in choose(tool, [c[3] for c in table_cases()] + [c[2] for c in tail_cases()]))
    listed = [ln.split(" ", 2)[2] for ln in tool("--names") if ln.startswith("kernel ")]
    assert len(listed) == len(set(listed)) and set(listed) == seen, (sorted(set(listed) - seen), sorted(seen - set(listed)))
