"""tests/view_shapes.py against the dispatch of this tree, on the CPU: conv_plan_main (built by test_conv_plan_cpu.py's helper, with
the host sanitizers) is asked in its IMAGE mode for the B = 1 forwards at 256, 224 and 192 px of the two seeded images, in the fp16
context and in fp16x3 with split 2 and 3 (queries `1 H W prec split 0`, and the same with batch invariance on, which is what a
forward pass runs by default), and the rows the two view sizes take beyond the 256-px ones must be the table's.  The cases of
tests/test_gpu_neighbour.py are that table, so they are derived from the dispatch and not typed by hand.

Also asked here, because the GPU test relies on it: every row, laid out as the GPU test lays it out for cy_conv_slices (dense, or
prediction rows for the head's outputs), selects the kernel and the variant the row names."""
import pytest

import view_shapes as V
from test_conv_plan_cpu import tool, case_line, choose, PREC          # noqa: F401 (tool: the session fixture that builds the program)
from caesar_yolo_amd import weights as W

STRIP, G64 = "conv3x3_widep_kernel<10> strip", "conv_igemm_kernel<4,1,2>"


@pytest.fixture(scope="module")
def images(tool):
    out = {"seeded:l:5": str(tool.dir / "view_v8l.cyw"), "seeded11:l:5": str(tool.dir / "view_y11l.cyw")}
    W.make_seeded_file(out["seeded:l:5"], "l", 5)
    W.make_seeded11_file(out["seeded11:l:5"], "l", 5)
    return out


def forwards(tool, image, prec, split, inv):
    """-> {size: set of (kernel, Hi, Wi, Cin, Cout, k, s, res)}, {kernel: variant name} of the B = 1 forwards of one context"""
    qpath = str(tool.dir / "view_queries.txt")
    with open(qpath, "w") as f:
        for s in V.SIZES:
            f.write("1 %d %d %d %d %d\n" % (s, s, PREC[prec], split, inv))
    sets, variant, cur = {}, {}, None
    for ln in tool(image, qpath):
        if ln.startswith("query "):
            cur = sets.setdefault(int(ln.split()[2]), set())
            continue
        geo, var, kernel = ln.split(" | ")
        g = [int(v) for v in geo.split()]
        assert g[0] == 1
        cur.add((kernel, g[1], g[2], g[3], g[4], g[5], g[6], g[14]))
        assert variant.setdefault(kernel, var) == var
    assert sorted(sets) == sorted(V.SIZES)
    return sets, variant


@pytest.mark.parametrize("inv", V.INVS)
@pytest.mark.parametrize("prec,splits", V.CONTEXTS)
@pytest.mark.parametrize("image", V.IMAGES)
def test_views_take_the_rows_of_the_table(tool, images, image, prec, splits, inv):
    for split in splits:
        sets, variant = forwards(tool, images[image], prec, split, inv)
        diff = (sets[224] | sets[192]) - sets[256]
        want = V.TABLE[(image, prec, inv)]
        assert len(want) == len(set(want))
        assert diff == set(want), "%s %s split %d inv %d: the views take %s beyond the table, the table has %s the views do not take" % (
            image, prec, split, inv, sorted(diff - set(want)), sorted(set(want) - diff))
        for kernel, var in variant.items():
            assert kernel not in V.KERNEL_VARIANT or var.split(" ")[0] == V.KERNEL_VARIANT[kernel], (kernel, var)
        # the rest of the B = 1 dispatch: every kernel of the 256-px forward that no view row of this context names has one row
        named = set(r[0] for key, t in V.TABLE.items() if key[1] == prec for r in t)
        rest = set(r[0] for key, t in V.REST_256.items() if key[1] == prec for r in t)
        assert not rest & named
        assert set(r[0] for r in sets[256]) - named <= rest
        for r in V.REST_256.get((image, prec, inv), ()):
            assert r in sets[256] and r[1] in (8, 16, 32), r


def test_table_has_what_the_issue_names():
    rows = V.TABLE[("seeded:l:5", "fp16x3", 0)]
    strip = [r for r in rows if r[0] == STRIP]
    assert set(r[1] for r in strip) == {28, 24, 12, 7, 6}
    for m in (28, 24, 12, 7, 6):
        assert set(r[7] for r in strip if r[1] == m) == {0, 1}, m
    assert set(r[1] for r in strip if r[3] == 512) == {12, 7, 6}
    assert set(r[1] for r in rows if r[0] == G64) == {56, 48, 28, 24, 14, 12, 7, 6}
    assert all(r[1] == r[2] for t in V.TABLE.values() for r in t)
    assert sorted(V.TABLE) == sorted((im, p, i) for im in V.IMAGES for p, _ in V.CONTEXTS for i in V.INVS)
    for im in V.IMAGES:                                          # fp16x3 selects by geometry alone
        assert V.TABLE[(im, "fp16x3", 0)] == V.TABLE[(im, "fp16x3", 1)]


@pytest.mark.parametrize("prec,splits", V.CONTEXTS)
def test_rows_select_their_kernel_through_the_conv_entry(tool, prec, splits):
    """What tests/test_gpu_neighbour.py hands cy_conv_slices (B = 1, dense with the row's residual and SiLU, or prediction rows;
    CY_BATCH_INVARIANT as the case says) selects the row's kernel."""
    cases = V.gpu_cases(prec)
    assert len(cases) == len(set(c[0] for c in cases))
    want = set((V.UNFUSED.get(r[0], r[0]),) + r[1:] for tab in (V.TABLE, V.REST_256) for key, t in tab.items() if key[1] == prec for r in t)
    assert set(c[1] for c in cases) == want
    for split in splits:
        lines = []
        for _, row, inv in cases:
            rows = V.rows_layout(row)
            geom = (1,) + row[1:7]
            lines.append(case_line(prec, geom, inv, {}, "rows", rows, act=0, res=0, split=split) if rows
                         else case_line(prec, geom, inv, {}, "dense", act=1, res=row[7], split=split))
        for (what, row, inv), (var, kernel) in zip(cases, choose(tool, lines)):
            assert kernel == row[0], "%s (split %d, CY_BATCH_INVARIANT=%s) runs %r" % (what, split, inv, kernel)
            assert var.split(" ")[0] == V.KERNEL_VARIANT[row[0]], (what, var)
