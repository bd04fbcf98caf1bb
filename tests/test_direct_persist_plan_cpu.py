"""The dispatch rule of the persistent pixels-direct kernel (conv_kernel, caesar_yolo_amd/csrc/cy_conv_plan.cpp) on the CPU, through the
host-side planner as tests/test_conv_plan_cpu.py does it: cy_conv_plan.cpp and cy_plan.cpp linked into
tests/host/direct_persist_plan_main.cpp, built with AddressSanitizer and UBSan and run as a child process.

The rule (CY_DIRECT_PERSIST = 1, the default): a launch of the 256 px x 256 ch pixels-direct tile takes its persistent form in the
fp16 context when it is not the fused pair, a tile has at least three K chunks (the ring's slots) and the launch has at least 512
tiles (two per CU), counted with the REAL batch -- below 1024 tiles only with at least 16 chunks per tile (measured: model.8.cv1).  0 = never, 2 = whatever the launch size (still fp16, not the pair, three chunks)."""
import os
import shutil
import subprocess

import pytest

from caesar_yolo_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
PREC = {"fp16": 0, "fp32": 1, "fp16x3": 2}
ONE_K1, ONE_K3 = "conv1x1_direct_kernel<4,2,3>", "conv1x1_direct_kernel<4,2,3,K3>"
PER_K1, PER_K3 = "conv1x1_direct_kernel<4,2,3,PERSIST>", "conv1x1_direct_kernel<4,2,3,K3,PERSIST>"
PAIR = ("conv1x1_direct_kernel<4,2,3,FUSE2>", "conv1x1_direct_kernel<4,2,3,K3,FUSE2>")
# the layers of seeded:l:5 that take the persistent form in a pass over 256 tiles of 512 x 512 (model.4.cv1 runs inside model.3's
# launch, the fused pair, model.9.cv1 has 256 tiles, model.8.cv1 512 tiles of 8 chunks)
FLAGSHIP = {"model.4.cv1": PER_K1, "model.4.cv2": PER_K1, "model.5": PER_K3, "model.6.cv1": PER_K1, "model.6.cv2": PER_K1, "model.7": PER_K3,
            "model.8.cv2": PER_K1, "model.9.cv2": PER_K1, "model.12.cv1": PER_K1, "model.12.cv2": PER_K1,
            "model.15.cv1": PER_K1, "model.15.cv2": PER_K1, "model.16": PER_K3, "model.18.cv1": PER_K1, "model.18.cv2": PER_K1, "model.19": PER_K3,
            "model.21.cv1": PER_K1, "model.21.cv2": PER_K1}


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    near = [os.path.join(os.path.dirname(hipcc), d, "clang++") for d in (".", "../llvm/bin", "../lib/llvm/bin")]
    cxx = next((c for c in near if os.path.exists(c)), None) or shutil.which("g++")
    assert cxx, "no clang++ beside hipcc and no g++: the dispatch rule cannot be checked"
    d = tmp_path_factory.mktemp("direct_persist_plan")
    exe = str(d / "direct_persist_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "direct_persist_plan_main.cpp"), os.path.join(CSRC, "cy_conv_plan.cpp"), os.path.join(CSRC, "cy_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, "direct_persist_plan_main: exit %d\n%s" % (r.returncode, r.stderr[-4000:])
        return r.stdout.splitlines()
    run.dir = d
    run.image = str(d / "l5.cyw")
    W.make_seeded_file(run.image, "l", 5)
    return run


def choose(tool, cases):
    """cases: (prec, (B, Hi, Wi, Cin, Cout, k, s), c1, res, wgt2, inv, min_blocks, persist, grid) -> [(variant, kernel, persist_grid)]"""
    path = str(tool.dir / "cases.txt")
    with open(path, "w") as f:
        for prec, geom, c1, res, wgt2, inv, mb, persist, grid in cases:
            f.write(" ".join(str(v) for v in (PREC[prec],) + tuple(geom) + (c1, res, wgt2, inv, mb, persist, grid)) + "\n")
    out = tool("--cases", path)
    assert len(out) == len(cases)
    return [tuple(ln.split(" | ")) for ln in out]


def network(tool, queries):
    """queries: (B, H, prec, inv, persist) -> per query {conv name: ((B, Ho, Wo, Cin, Cout, k), variant, kernel)}"""
    path = str(tool.dir / "queries.txt")
    with open(path, "w") as f:
        for B, H, prec, inv, persist in queries:
            f.write("%d %d %d %d %d %d\n" % (B, H, H, PREC[prec], inv, persist))
    out, cur = [], None
    for ln in tool(tool.image, path):
        if ln.startswith("query "):
            cur = {}
            out.append(cur)
        else:
            name, geom, variant, kernel = ln.split(" | ")
            cur[name] = (tuple(int(v) for v in geom.split()), variant, kernel)
    assert len(out) == len(queries)
    return out


def rule(geom, kernel_off):
    """The kernel the rule gives a layer whose one-tile choice is kernel_off."""
    B, Ho, Wo, Cin, Cout, k = geom
    if kernel_off not in (ONE_K1, ONE_K3):
        return kernel_off
    tiles = ((B * Ho * Wo + 255) // 256) * ((Cout + 255) // 256)
    chunks = Cin // 64 * k * k
    if tiles >= 512 and chunks >= 3 and (tiles >= 1024 or chunks >= 16):
        return PER_K3 if k == 3 else PER_K1
    return kernel_off


def test_the_flagship_layers_by_name(tool):
    on, off = network(tool, [(256, 512, "fp16", 1, 1), (256, 512, "fp16", 1, 0)])
    got = dict((n, v[2]) for n, v in on.items() if v[2] in (PER_K1, PER_K3))
    assert got == FLAGSHIP
    # ... which is the rule applied to what runs with the switch off, layer by layer; the variant (the profile's key) does not move
    for name, (geom, variant, kernel) in on.items():
        assert kernel == rule(geom, off[name][2]), name
        assert variant == off[name][1], name
    assert on["model.3"][2] in PAIR and on["model.9.cv1"][2] == ONE_K1 and on["model.8.cv1"][2] == ONE_K1


@pytest.mark.parametrize("H", [512, 640])
def test_switch_off_restores_the_one_tile_choice_everywhere(tool, H):
    """CY_DIRECT_PERSIST=0: no layer of seeded:l:5 runs a persistent pixels-direct kernel, at any batch, with or without batch
    invariance; with the switch on, only the form below the variant differs, and only by the rule."""
    queries = [(B, H, "fp16", inv, p) for B in (1, 63, 64, 256) for inv in (1, 0) for p in (0, 1)]
    res = network(tool, queries)
    for (B, _, _, inv, p), off, on in zip(queries[::2], res[::2], res[1::2]):
        assert not [n for n, v in off.items() if "PERSIST" in v[2]]
        for name in off:
            assert on[name][1] == off[name][1] and on[name][2] == rule(on[name][0], off[name][2]), (B, inv, name)


def test_never_for_fp16x3_the_pair_or_the_128_channel_tile(tool):
    big = (256, 32, 32, 512, 512, 1, 1)
    got = choose(tool, [("fp16x3", big, 0, 0, 0, 1, 256, 2, 0), ("fp32", big, 0, 0, 0, 1, 256, 2, 0),
                        ("fp16", (256, 64, 64, 128, 256, 1, 1), 0, 0, 1, 1, 256, 2, 0), ("fp16", (256, 64, 64, 128, 256, 3, 2), 0, 0, 1, 1, 256, 2, 0),
                        ("fp16", (256, 64, 64, 256, 128, 1, 1), 0, 0, 0, 1, 256, 2, 0), ("fp16", (256, 128, 128, 64, 128, 3, 2), 0, 0, 0, 1, 256, 2, 0)])
    assert got[0][1] == ONE_K1 and got[1][1].startswith("conv_igemm_kernel")
    assert (got[2][1], got[3][1]) == PAIR
    assert got[4][1] == "conv1x1_direct_kernel<2,2,2>" and got[5][1] == "conv1x1_direct_kernel<2,4,2,K3>"
    for name in network(tool, [(256, 512, "fp16x3", 1, 2)])[0].values():
        assert "PERSIST" not in name[2]


def test_two_tiles_per_cu_and_three_chunks(tool):
    """Knob 1: 512 tiles by the real batch (batch invariance or not); below that the one-tile form.  Knob 2: any launch size.  Fewer
    than three K chunks (Cin 64, 128): the one-tile form at every knob.  The grid cap travels with the choice."""
    g = lambda B, Cin=1024, Cout=512: (B, 32, 32, Cin, Cout, 1, 1)            # 4 * B pixel tiles x 2 channel tiles, 16 chunks
    got = choose(tool, [("fp16", g(64), 0, 0, 0, 1, 256, 1, 0), ("fp16", g(63), 0, 0, 0, 1, 256, 1, 0), ("fp16", g(63), 0, 0, 0, 0, 256, 1, 0),
                        ("fp16", g(128, Cout=256), 0, 0, 0, 1, 256, 1, 0), ("fp16", g(127, Cout=256), 0, 0, 0, 1, 256, 1, 0),
                        ("fp16", g(2), 0, 0, 0, 1, 0, 2, 3), ("fp16", g(2), 0, 0, 0, 1, 0, 1, 3), ("fp16", g(2), 0, 1, 0, 1, 0, 2, 0),
                        ("fp16", g(256, Cin=64), 0, 0, 0, 1, 256, 1, 0), ("fp16", g(256, Cin=128), 0, 0, 0, 1, 256, 2, 0), ("fp16", g(256, Cin=192), 0, 0, 0, 1, 256, 1, 0),
                        ("fp16", (2, 48, 48, 128, 256, 3, 2), 0, 0, 0, 1, 0, 2, 3), ("fp16", g(256, Cin=192), 128, 0, 0, 1, 256, 1, 0),
                        ("fp16", g(256), 0, 0, 0, 1, 256, 0, 0),
                        ("fp16", g(64, Cin=960), 0, 0, 0, 1, 256, 1, 0), ("fp16", g(128, Cin=960), 0, 0, 0, 1, 256, 1, 0)])      # 15 chunks: from 1024 tiles on
    assert [k for _, k, _ in got] == [PER_K1, ONE_K1, ONE_K1, PER_K1, ONE_K1, PER_K1, ONE_K1, PER_K1, ONE_K1, ONE_K1, PER_K1, PER_K3, PER_K1, ONE_K1, ONE_K1, PER_K1]
    assert [int(n) for _, _, n in got][5:8] == [3, 3, 0]
    assert len(set(v for v, _, _ in got)) == 1
