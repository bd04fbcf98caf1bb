"""tests/bigmap_cases.py is what it claims to be, shown on the reference side without a GPU: where the patches and decoys lie, that
no patch is degenerate for any reference, that a result read from a decoy would not pass the GPU comparison (sensitivity), and that
the reference on a crop equals the reference on the full image (on a small stand-in, not on the 8 GiB twin).

Sensitivity.  For a job at `u32`, `hi` or `end` and the same job moved onto the decoy 2^30 pixels earlier, the two reference rows
(positions taken relative to the job) have to differ in a field the GPU test compares exactly.  The two Gaussian fits of a disc
compare exactly only status, counts and the window, which a decoy of the same layout shares; for them the rows have to differ in a
fitted parameter by more than 1000 times the tolerance of the GPU comparison, which fails that comparison as surely."""
import numpy as np

import atrous_ref
import bigmap_cases as B
import bkg_ref
import blend_cases
import blend_ref
import fit_cases
import fit_ref
import peakfit_ref
import peakgroup_ref
import peaks_ref
import residual_ref

NB, NA, NP = len(B.BOX_NAMES), 5, len(B.PEAK_NAMES)


def test_places():
    assert B.disjoint()
    y, x = B.PLACES["s31"]
    assert (y + 64) * B.MW + x + 64 == 1 << 29 and B.rc(1 << 29) == (11585, 33597)
    y, x = B.PLACES["hi"]
    assert (y + 64) * B.MW + x + 64 == 3 << 29
    y, x = B.PLACES["u32"]
    assert (y + 8) * B.MW + x == 1 << 30 and B.rc(1 << 30) == (23171, 20855)
    assert B.PLACES["end"] == (B.MH - B.P, B.MW - B.P) and B.PLACES["edge_r"][1] + B.P == B.MW and B.PLACES["edge_b"][0] + B.P == B.MH
    assert 0 < B.PLACES["edge_r"][0] < B.MH - 2 * B.P and 0 < B.PLACES["edge_b"][1] < B.MW - 2 * B.P
    host = B.host()
    for nm, index in B.THRESHOLD_PIXEL.items():
        py, px = B.PLACES[nm]
        first, last = py * B.MW + px, (py + B.P - 1) * B.MW + px + B.P - 1
        y, x = B.rc(index)
        assert first <= index <= last and py <= y < py + B.P and px <= x < px + B.P and host[y, x] != 0, nm
        if nm != "end":                                            # pixels of the patch on both sides of it
            assert first < index < last and host[y - 1, x] != 0 and host[y + 1, x] != 0 and host[y, x + 1] != 0, nm
    ye, xe = B.rc(B.MH * B.MW - 1 - B.WRAP)
    assert (ye, xe) == (23169, 25483) and B.PLACES["end_decoy"] == (ye - B.P + 1, xe - B.P + 1)
    assert host.shape == (B.MH, B.MW) and host.size < 1 << 31


def test_decoys():
    host = B.host()
    for nm, decoy in B.DECOY_OF.items():
        (py, px), (qy, qx) = B.PLACES[nm], B.PLACES[decoy]
        assert (py * B.MW + px) - (qy * B.MW + qx) == B.WRAP and 0 <= qx and qx + B.P <= B.MW, nm
        dy, dx = B.shift(nm)
        first = B.top(decoy)
        a, b = host[py + first:py + B.P, px:px + B.P], host[py + first + dy:py + B.P + dy, px + dx:px + B.P + dx]
        assert np.array_equal(b, B.patch(decoy)[0][first:]) and np.array_equal(a, B.patch(nm)[0][first:])
        assert (a != b).mean() > 0.99, nm                          # data, and other data
        assert (B.host_rms()[py + first:py + B.P, px:px + B.P] != B.host_rms()[py + first + dy:py + B.P + dy, px + dx:px + B.P + dx]).mean() > 0.99


def test_every_patch_is_non_degenerate():
    meas = B.measure_reference(8)[0]
    isl, dbl = B.island_reference()[0], B.deblend_reference()[0]
    _, ncomp, _, _ = B.fit_inputs()
    fit, (blend, bcond) = B.fit_reference(), B.blend_reference()
    pfit, (pgrp, gcond) = B.peakfit_reference(), B.peakgroup_reference()
    res, aper = B.residual_reference()[0], B.aperture_reference(True)
    # nothing is left to the leave-out rules of the random tests: every variant agrees and every job is well conditioned
    assert not fit_cases.excluded(fit, ncomp).any() and not blend_cases.excluded(blend, bcond, ncomp).any()
    assert not peakgroup_ref.excluded(pgrp, gcond).any() and not peakfit_ref.spread(pfit)[2].any()
    assert max(peakfit_ref.cond_H(r) for r in pfit[0]) < 1e10
    for nm in B.names():
        b, a, p = B.rows_of(nm, NB), B.rows_of(nm, NA), B.rows_of(nm, NP)
        assert (meas[b, 1] % 2 == 1).any() and (meas[b, 1] % 2 == 0).any() and (meas[b, 0] > 0).all(), nm      # odd and even ring counts
        assert (isl[b, 2] >= 2).any() and (isl[b, 1] > 0).sum() >= 4, nm                  # two islands in one box
        assert (dbl[b, 3] >= 2).any() and (dbl[b, 0] == 0).all(), nm                      # an island set of two components
        rows = [fit[0][i, k] for i in range(b.start, b.stop) for k in range(ncomp[i])]
        assert len(rows) >= 7 and all(r[0] == 0 for r in rows), nm                        # converged fits
        assert sum(blend[0][i, k, 0] == 0 and blend[0][i, k, 6] == 2 for i in range(b.start, b.stop) for k in range(ncomp[i])) >= 4, nm      # blends
        assert (pfit[0][p, 0] == 0).all() and (pfit[0][p, 37] >= 1).sum() >= 4, nm        # discs shared with a neighbour
        assert (pgrp[0][p, 6] == 2).sum() == 4 and (pgrp[0][p][pgrp[0][p, 6] == 2, 0] == 0).all(), nm          # two linked groups
        assert (res[b, 2] > 0).sum() >= 4 and (aper[a, 0] == 0).all(), nm
        if nm != "u32_decoy":
            c = B.crop(nm, B.HALO_PEAKS)
            assert len(B.peaks_on_crop(B.host(), B.host_rms(), c, 5.0, 1)[0]) >= 3 and len(B.peaks_on_crop(B.host(), B.host_rms(), c, 5.0, -1)[0]) >= 1, nm
    # the far corner: boxes, discs and apertures that leave the image past the last row and the last column
    e = B.rows_of("end", NB).start + B.BOX_NAMES.index("corner")
    assert B.all_boxes()[e, 2] > B.MW and B.all_boxes()[e, 3] > B.MH and meas[e, 0] == 19 * 19
    ep = B.rows_of("end", NP).start + B.PEAK_NAMES.index("corner_a")
    assert pfit[0][ep, 36] == 1 and pfit[0][ep, 33] == B.MW - 1 and pfit[0][ep, 35] == B.MH - 1 and pgrp[0][ep, 40] == 1
    assert aper[B.rows_of("end", NA).stop - 1, 5] == 1 and aper[B.rows_of("end", NA).stop - 1, 2] == B.MW - 1


def _far(a, b, cols, tol):
    return bool((np.abs(a[cols] - b[cols]) > 1000 * tol * (np.abs(b[cols]) + 1e-3)).any())


def test_a_result_read_from_the_decoy_would_not_pass():
    meas0, meas8 = B.measure_reference(0)[0], B.measure_reference(8)[0]
    isl, imasks, _ = B.island_reference()
    dbl, dcomp, dmasks, _ = B.deblend_reference()
    _, ncomp, _, _ = B.fit_inputs()
    fit, blend = B.fit_reference()[0], B.blend_reference()[0][0]
    res, pfit, pgrp = B.residual_reference()[0], B.peakfit_reference()[0], B.peakgroup_reference()[0][0]
    for nm, decoy in B.DECOY_OF.items():
        p, q = B.rows_of(nm, NB), B.rows_of(decoy, NB)
        for j, box in enumerate(B.BOX_NAMES):
            i, d = p.start + j, q.start + j
            if decoy == "u32_decoy" and B._BOXES[j, 1] - 8 < 8:
                continue                                           # its ring leaves the image at the top: not the same job
            what = "%s / %s" % (nm, box)
            assert meas0[i, 4] != meas0[d, 4], what                                    # peak
            assert meas8[i, 2] != meas8[d, 2] and meas8[i, 3] != meas8[d, 3], what     # bkg, rms
            if isl[i, 1] > 0:
                assert imasks[i].tobytes() != imasks[d].tobytes() or not np.array_equal(isl[i, 1:6], isl[d, 1:6]), what
                assert dmasks[i].tobytes() != dmasks[d].tobytes() or dcomp[i, 0, 1] != dcomp[d, 0, 1], what         # a component's peak value
                assert res[i, 7] != res[d, 7], what                                    # the largest |residual|
            for k in range(min(ncomp[i], ncomp[d])):
                assert fit[i, k, 2] != fit[d, k, 2] or _far(fit[i, k], fit[d, k], [5, 8, 9, 10], fit_ref.TOL), what
                if blend[i, k, 0] == 0 and blend[d, k, 0] == 0:
                    assert blend[i, k, 2] != blend[d, k, 2] or _far(blend[i, k], blend[d, k], [8, 11, 12, 13], blend_ref.TOL), what
        for with_rms in (True, False):
            a = B.aperture_reference(with_rms)
            ap, aq = a[B.rows_of(nm, NA)], a[B.rows_of(decoy, NA)]
            assert (ap[:, 6] != aq[:, 6]).all() and (ap[:, 9] != aq[:, 9]).all(), nm    # the annulus median, the first ring's sum
            if with_rms:
                assert (ap[:, 11] != aq[:, 11]).all(), nm                              # the first ring's variance
        p, q = B.rows_of(nm, NP), B.rows_of(decoy, NP)
        for j in range(NP):
            assert _far(pfit[p][j], pfit[q][j], [5, 8, 9, 10], peakfit_ref.TOL), (nm, B.PEAK_NAMES[j])
            if pgrp[p][j, 6] == 2:
                assert _far(pgrp[p][j], pgrp[q][j], [8, 11, 12, 13], peakgroup_ref.TOL), (nm, B.PEAK_NAMES[j])


def test_a_map_read_from_the_decoy_would_not_pass():
    """The whole-map entries are compared bit for bit (planes, mesh rows, peak rows) or within half an fp32 ulp (model, residual): on
    the pixels of a patch the references of patch and decoy have to differ, peak for peak and pixel for pixel."""
    host, rms, comp = B.host(), B.host_rms(), B.render_components()
    for nm, decoy in B.DECOY_OF.items():
        first = B.top(decoy)

        def on_patch(name, plane, c):                              # the rows of the patch that both have, out of a plane on the crop c
            py, px = B.PLACES[name]
            return plane[py + first - c[0]:py + B.P - c[0], px - c[2]:px + B.P - c[2]]
        for step in (1, 64):
            ca, cb = B.crop(nm, B.halo_atrous(step)), B.crop(decoy, B.halo_atrous(step))
            for a, b in zip(B.atrous_on_crop(host, ca, step), B.atrous_on_crop(host, cb, step)):
                assert (on_patch(nm, a, ca) != on_patch(decoy, b, cb)).mean() > 0.99, (nm, step)
        ca, cb = B.crop(nm, B.HALO_RENDER), B.crop(decoy, B.HALO_RENDER)
        a, b = B.render_on_crop(host, comp, ca, (B.MH, B.MW)), B.render_on_crop(host, comp, cb, (B.MH, B.MW))
        for k in (1, 2):
            x, y = on_patch(nm, a[k], ca), on_patch(decoy, b[k], cb)
            drawn = (x != 0) | (y != 0)                            # the model is 0 outside the components' rectangles
            assert drawn.sum() > 500 and (np.abs(x - y) > 2.0 ** -20 * np.abs(x))[drawn].mean() > 0.9, (nm, k)
        for sign in (1, -1):
            (pa, _), (pb, _) = (B.peaks_on_crop(host, rms, B.crop(n, B.HALO_PEAKS), 5.0, sign) for n in (nm, decoy))
            va, vb = set(pa[:, 2].tolist()), set(pb[:, 2].tolist())
            assert va and vb and not va & vb, (nm, sign)            # no peak value in common
        for cell in (128, 300):
            ra, rb = (B.background_on_crop(host, B.crop(n, 0, cell), cell, 3.0, 3)[0] for n in (nm, decoy))
            ma, mb = set(ra[ra[:, :, 0] > 0][:, 2].tolist()), set(rb[rb[:, :, 0] > 0][:, 2].tolist())
            assert ma and mb and not ma & mb, (nm, cell)            # no cell median in common


# ---- the reference on a crop is the reference on the full image, on a stand-in of 1000 x 1100 pixels
SH, SW = 1000, 1100
STAND_IN = {"low": (300, 400), "end": (SH - B.P, SW - B.P), "edge_r": (200, SW - B.P), "edge_b": (SH - B.P, 100)}


def stand_in(of):
    a = np.zeros((SH, SW), np.float32)
    for nm, (y, x) in STAND_IN.items():
        a[y:y + B.P, x:x + B.P] = of(nm)
    return a


def stand_in_crops(halo, grid=1):
    c = [B.crop_at(y, x, 0, halo, grid, SH, SW) for y, x in STAND_IN.values()]
    assert all(a[1] <= b[0] or b[1] <= a[0] or a[3] <= b[2] or b[3] <= a[2] for i, a in enumerate(c) for b in c[i + 1:])      # as B.crops() asserts
    return dict(zip(STAND_IN, c))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_crop_reference_equals_full_reference():
    img, rms = stand_in(lambda nm: B.patch(nm)[0]), stand_in(B.rms_patch)
    for sign in (1, -1):
        table = stand_in_crops(B.HALO_PEAKS)
        full, fabs = peaks_ref.find_peaks(img, rms, 5.0, B.RADIUS_PEAKS, sign)
        rows, absum = B.merged_peaks(img, rms, table, 5.0, sign)
        assert len(full) >= 4 and np.array_equal(bits(rows), bits(full)) and np.array_equal(bits(absum), bits(fabs))
    for step in (1, 64):
        full = atrous_ref.atrous_step(img, step)
        table = stand_in_crops(B.halo_atrous(step))
        inside = np.zeros(img.shape, bool)
        for nm, c in table.items():
            for got, want in zip(B.atrous_on_crop(img, c, step), full):
                assert np.array_equal(bits(got), bits(B.cut(want, c))), (nm, step)
            B.cut(inside, c)[:] = True
        assert not full[0][~inside].any() and not full[1][~inside].any()           # and the full planes are blank outside the crops
    for cell in (128, 300):
        full = bkg_ref.background(img, cell, 3.0, 3)
        for nm, c in stand_in_crops(0, cell).items():
            got, (cy0, cx0) = B.background_on_crop(img, c, cell, 3.0, 3)
            assert np.array_equal(bits(got), bits(full[cy0:cy0 + got.shape[0], cx0:cx0 + got.shape[1]])), (nm, cell)
    comp = B.render_components(STAND_IN)
    f_rows, f_model, f_resid = residual_ref.render(img, comp, B.NSIGMA)
    inside = np.zeros(img.shape, bool)
    for nm, c in stand_in_crops(B.HALO_RENDER).items():
        rows, model, resid = B.render_on_crop(img, comp, c, (SH, SW))
        assert np.array_equal(rows, f_rows) and np.array_equal(bits(model), bits(B.cut(f_model, c))) and np.array_equal(bits(resid), bits(B.cut(f_resid, c))), nm
        B.cut(inside, c)[:] = True
    assert (f_rows[:, 0] == 0).all() and not f_model[~inside].any() and not f_resid[~inside].any()


def test_outside_ranges_cover_the_rest_of_the_image_once():
    for halo, grid in ((B.HALO_PEAKS, 1), (B.HALO_RENDER, 1), (B.halo_atrous(1), 1), (B.halo_atrous(64), 1), (0, 128), (0, 300), (0, 1)):
        table = B.crops(halo, grid)
        area = sum((c[1] - c[0]) * (c[3] - c[2]) for c in table.values())
        rest = 0
        for a, b, cols in B.outside_ranges(table):
            assert 0 <= a < b <= B.MH and all(0 <= x0 < x1 <= B.MW for x0, x1 in cols)
            assert all(c[1] <= a or b <= c[0] or all(x1 <= c[2] or c[3] <= x0 for x0, x1 in cols) for c in table.values())
            rest += (b - a) * sum(x1 - x0 for x0, x1 in cols)
        assert area + rest == B.MH * B.MW
