"""Cost of --measure_sources, --measure_islands and --bkg_map (developer tool): the S16k tiled run of scripts/run.py (README recipe:
seeded:l:5, zscale + minmax, 512-px tiles at step 0.8) in ONE process, switches off / --measure_sources / --measure_islands
alternating, `--runs` timed runs each after a warm-up.

    python tools/time_measure.py [--size 16384] [--runs 3] [--ring 8] [--off-only] [--no-islands] [--no-bkg] [--no-deblend] [--no-fit] [--no-blend] [--no-residual] [--no-peaks] [--no-scales] [--no-apertures] [--no-peakfits] [--no-peakgroups] [--only a,b] [--host-ref]

Per run: SFinder.run_parallel's own wall time (image ingest, detect pass, gather, catalog, measurement, files).  With the switch on
also the measurement step's wall time (resident image looked up or uploaded + kernel + copies + annotate), the kernel's time
(hipEvents around the launch, cy_measure_kernel_ms) and the number of sources.  --host-ref times tests/measure_ref.py (numpy
float64) on the same boxes.  With --measure_islands the same three numbers for the island step (islands_ms, islands_kernel_ms), the
histogram of the box-window areas of the catalog and the share of sources whose window is labelled in LDS (up to 4096 pixels); --host-ref
then also times tests/island_ref.py.  Unless --no-bkg is given there is a fourth variant, --bkg_map (background_ms, background_kernel_ms), and after the runs
the kernels alone on the same image: cy_measure_background at cell 64 / 128 / 256 (k 3, 3 clips) and cy_expand_background of the
cell-128 mesh to both maps, `--runs` calls each after a warm-up; --host-ref then also times tests/bkg_ref.py at cell 128.
Unless --no-residual (or --no-blend) is given there is a variant `residual`, --fit_blends --residual_map (residual_ms, render_kernel_ms,
residual_kernel_ms, the numbers of rendered, duplicated and capped components beside the blend_ms of the same runs).
Unless --no-peaks (or --no-residual) is given there is a variant `peaks`, --fit_blends --residual_map --residual_peaks (peaks_ms,
peaks_kernel_ms, the numbers of peaks found and kept beside the render_kernel_ms of the same runs; the switch implies --bkg_map);
peaks_added_ms is its run time over that of the `residual` variant.
Unless --no-scales (or --no-residual) is given there is a variant `scales`, --fit_blends --residual_map --residual_scales 4 (scales_ms,
atrous_kernel_ms, scales_background_kernel_ms and scales_peaks_kernel_ms, each summed over the levels, the numbers of scale peaks found,
kept and strongest beside the render_kernel_ms of the same runs; the switch implies --bkg_map); scales_added_ms is its run time over
that of the `residual` variant.  After the runs the kernels of every level alone on the same image (atrous_levels): cy_atrous_step
with both outputs and with the smooth plane only, cy_measure_background on the detail plane at the cell the chain uses, and
cy_find_peaks on it, `--runs` calls each after a warm-up, with the bytes moved per second; six levels, so that the cells of 256 and
512 pixels of scales 5 and 6 are timed too.
Unless --no-apertures (or --no-scales, --no-residual) is given there is a variant `apertures`, --fit_blends --residual_map --residual_peaks
--residual_scales 4 --peak_apertures (apertures_ms, aperture_kernel_ms summed over the calls, the numbers of jobs, measured and clipped
ones beside the scales_ and peaks_ kernel times of the same runs); apertures_added_ms is its run time over that of the `scales` variant.
Unless --no-peakfits (or --no-apertures, --no-scales, --no-residual) is given there is a variant `peakfits`, the flags of `apertures` plus
--fit_peaks (peakfit_ms, peakfit_kernel_ms summed over the calls, the numbers of jobs, converged and crowded ones and the iterations);
peakfits_added_ms is its run time over that of the `apertures` variant of the same runs.
Unless --no-peakgroups (or --no-peakfits, ..) is given there is a variant `peakgroups`, the flags of `peakfits` plus --fit_peak_groups
(peakgroup_ms, peakgroup_kernel_ms summed over the calls beside peakfit_kernel_ms of the same runs, the numbers of group jobs, members,
converged jobs and groups above the member limit, the iterations, and peakgroup_groups: the groups of the catalog counted by size and
status); peakgroups_added_ms is its run time over that of the `peakfits` variant of the same runs.
Unless --no-subtract (or --no-peakgroups, ..) is given there is a variant `subtract`, the flags of `peakgroups` plus --subtract_peaks
(subtract_ms, subtract_render_kernel_ms, disc_residual_kernel_ms summed over the calls, left_peaks_kernel_ms of the two searches beside
peakgroup_kernel_ms of the same runs, the numbers of selected, rendered, wandered and duplicate components and of the entries of the
two left lists); subtract_added_ms is its run time over that of the `peakgroups` variant of the same runs.
Unless --no-forced (or --no-residual, ..) is given there is a variant `forced`, the flags of `residual` plus --forced_fit (forced_ms,
forced_kernel_ms beside residual_ms and render_kernel_ms of the same runs, the numbers of maps, jobs, fitted, crowded and singular
ones); forced_added_ms is its run time over that of the `residual` variant of the same runs.
--only a,b keeps the named variants (and `off`) and drops the others.
Unless --no-blend (or --no-fit) is given there is a variant --fit_blends (blend_ms, blend_kernel_ms, the number of joint jobs, their
iterations and the groups above the member limit).  Unless --no-fit (or --no-deblend) is given there is a variant --fit_components (fit_ms, fit_kernel_ms, the number of fitted jobs and
their mean and largest niter beside the deblend_ms and deblend_kernel_ms of the same runs).
Unless --no-deblend is given there is a variant --deblend_islands (deblend_ms, deblend_kernel_ms beside the islands_ms and
islands_kernel_ms of the same run: both steps on the same boxes).
--off-only serves a tree without the switch (the comparison against an earlier commit).  Prints one
JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
import __graft_entry__ as ge


def background_kernels(img, runs, host_ref):
    """The two background kernels alone on `img`: medians of `runs` calls after a warm-up."""
    import torch
    from caesar_yolo_amd import measure
    from caesar_yolo_amd.model import YOLO
    det = YOLO("seeded:l:5", precision="fp16x3", max_batch=1, max_imgsz=64).engine(0)
    dev = det.mosaic_to_device(img)
    out = {}
    for cell in (64, 128, 256):
        ms = []
        for i in range(runs + 1):
            raw = det.measure_background(dev, cell=cell, k=3.0, niter=3)
            ms.append(det.background_kernel_ms())
        out["background_kernel_ms_cell%d" % cell] = [round(v, 3) for v in ms[1:]]
        out["background_kernel_ms_cell%d_median" % cell] = statistics.median(ms[1:])
        if cell == 128:
            mesh, out["defined_cells"] = measure.fill_mesh(raw, 64)
    ms = []
    for i in range(runs + 1):                              # wall time of the call: upload of the mesh, kernel, synchronisation
        torch.cuda.synchronize()
        t0 = time.time()
        maps = det.expand_background(mesh, 128, img.shape)
        ms.append(1e3 * (time.time() - t0))
        del maps
    out["expand_call_ms"] = [round(v, 3) for v in ms[1:]]
    out["expand_call_ms_median"] = statistics.median(ms[1:])
    if host_ref:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import bkg_ref
        host = np.where(np.isfinite(img), img, np.float32(0)).astype(np.float32)
        t0 = time.time()
        bkg_ref.background(host, 128, 3.0, 3)
        out["host_bkg_ref_ms"] = 1e3 * (time.time() - t0)
    return out


def atrous_levels(img, runs, nscales=6, bkg_cell=128):
    """The kernels of the scale search alone, level by level on `img`: medians of `runs` calls after a warm-up."""
    from caesar_yolo_amd import measure
    from caesar_yolo_amd.model import YOLO
    det = YOLO("seeded:l:5", precision="fp16x3", max_batch=1, max_imgsz=64).engine(0)
    c = det.mosaic_to_device(img)
    px, out = float(img.size), []
    for j in range(1, nscales + 1):
        step = 1 << (j - 1)
        cell, radius = measure.scale_cell(bkg_cell, step), measure.scale_radius(2, step)
        both, smooth_only, bkg, peaks = [], [], [], []
        for i in range(runs + 1):
            det.atrous_step(c, step, want=("smooth",))
            smooth_only.append(det.atrous_kernel_ms())
            smooth, w = det.atrous_step(c, step)
            both.append(det.atrous_kernel_ms())
            raw = det.measure_background(w, cell=cell, k=3.0, niter=3)
            bkg.append(det.background_kernel_ms())
            rms = det.expand_background(measure.fill_mesh(raw, 64)[0], cell, img.shape, want=("rms",))[1]
            _, total = det.find_peaks(w, rms, k_sigma=5.0, radius=radius, sign=1, cap=65536)
            peaks.append(det.peaks_kernel_ms())
        med = lambda v: statistics.median(v[1:])
        out.append({"scale": j, "step": step, "cell": cell, "radius": radius, "found": int(total),
                    "atrous_kernel_ms": [round(v, 4) for v in both[1:]], "atrous_kernel_ms_median": med(both),
                    "atrous_TBps_12B_per_px": 12.0 * px / (med(both) * 1e-3) / 1e12,
                    "atrous_smooth_only_kernel_ms_median": med(smooth_only), "atrous_smooth_only_TBps_8B_per_px": 8.0 * px / (med(smooth_only) * 1e-3) / 1e12,
                    "background_kernel_ms": [round(v, 3) for v in bkg[1:]], "background_kernel_ms_median": med(bkg),
                    "peaks_kernel_ms_median": med(peaks)})
        c = smooth
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ring", type=int, default=8)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--no-islands", action="store_true")
    ap.add_argument("--no-bkg", action="store_true")
    ap.add_argument("--no-deblend", action="store_true")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--no-blend", action="store_true")
    ap.add_argument("--no-residual", action="store_true")
    ap.add_argument("--no-peaks", action="store_true")
    ap.add_argument("--no-scales", action="store_true")
    ap.add_argument("--no-apertures", action="store_true")
    ap.add_argument("--no-peakfits", action="store_true")
    ap.add_argument("--no-peakgroups", action="store_true")
    ap.add_argument("--no-subtract", action="store_true")
    ap.add_argument("--no-forced", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated variants to keep beside `off`")
    ap.add_argument("--host-ref", action="store_true")
    args = ap.parse_args()
    ge.build()
    import run
    from caesar_yolo_amd import synth, utils, inference
    seen = []
    orig = inference.SFinder.run_parallel

    def timed(self):
        rc = orig(self)
        seen.append(dict({k: v for k, v in self.stats.items() if isinstance(v, (int, float))}, run_ms=1e3 * self.runtime,
                         sources=len(self.sources["sources"]), kernel_ms=self.stats.get("measure_kernel_ms")))
        if "peakgroup_jobs" in self.stats:                  # the groups by size and status, counted on their first members
            groups = {}
            for lst in ("residual_peaks", "residual_holes", "residual_scale_peaks"):
                for e in self.sources.get(lst) or []:
                    if e.get("gblend_slot") == 0:
                        key = "size %d status %d" % (e["gblend_size"], e["gblend_status"])
                        groups[key] = groups.get(key, 0) + 1
            seen[-1]["peakgroup_groups"] = dict(sorted(groups.items()))
        return rc
    inference.SFinder.run_parallel = timed
    res = {"size": args.size, "runs": args.runs, "ring": args.ring}
    with tempfile.TemporaryDirectory() as d:
        img = synth.make_mosaic(args.size, seed=20260104)
        path = os.path.join(d, "s16k.fits")
        utils.write_fits_image(path, img, synth.FITS_CARDS + [("CTYPE1", "RA---SIN"), ("CTYPE2", "DEC--SIN"), ("CRVAL1", 254.5),
                                                              ("CRVAL2", -41.25), ("CRPIX1", args.size / 2.0), ("CRPIX2", args.size / 2.0)])
        base = ["--image=" + path, "--weights=seeded:l:5", "--preprocessing", "--zscale_stretch", "--normalize_minmax", "--norm_max=255",
                "--imgsize=512", "--split_img_in_tiles", "--tile_xsize=512", "--tile_ysize=512", "--tile_xstep=0.8", "--tile_ystep=0.8",
                "--devices=0"]
        on = ["--measure_sources", "--measure_ring=%d" % args.ring]
        cwd = os.getcwd()
        os.chdir(d)
        try:
            # variant -> (extra flags, timed keys, count keys); every switch implies the steps before it (measure.plan), so a variant
            # also reports the step its own builds on.  "islands" is the last one: its catalog is read below
            table = {"on": ([], (), ()),
                     "bkg": (["--bkg_map"], ("background_ms", "background_kernel_ms"), ()),
                     "deblend": (["--deblend_islands"], ("islands_ms", "islands_kernel_ms", "deblend_ms", "deblend_kernel_ms"), ()),
                     "fit": (["--fit_components"], ("deblend_ms", "deblend_kernel_ms", "fit_ms", "fit_kernel_ms"),
                             ("fit_jobs", "fit_niter_mean", "fit_niter_max")),
                     "blend": (["--fit_blends"], ("fit_ms", "fit_kernel_ms", "blend_ms", "blend_kernel_ms"),
                               ("blend_jobs", "blend_niter_mean", "blend_niter_max", "blend_over_limit")),
                     "residual": (["--fit_blends", "--residual_map"], ("blend_ms", "residual_ms", "render_kernel_ms", "residual_kernel_ms"),
                                  ("residual_rendered", "residual_duplicates", "residual_capped")),
                     "peaks": (["--fit_blends", "--residual_map", "--residual_peaks"], ("render_kernel_ms", "peaks_ms", "peaks_kernel_ms"),
                               ("peaks_found", "peaks_kept")),
                     "scales": (["--fit_blends", "--residual_map", "--residual_scales=4"],
                                ("render_kernel_ms", "scales_ms", "atrous_kernel_ms", "scales_background_kernel_ms", "scales_peaks_kernel_ms"),
                                ("scales_found", "scales_kept", "scales_strongest")),
                     "apertures": (["--fit_blends", "--residual_map", "--residual_peaks", "--residual_scales=4", "--peak_apertures"],
                                   ("render_kernel_ms", "peaks_kernel_ms", "scales_ms", "atrous_kernel_ms", "scales_background_kernel_ms", "scales_peaks_kernel_ms",
                                    "apertures_ms", "aperture_kernel_ms"),
                                   ("peaks_kept", "scales_kept", "apertures_jobs", "apertures_measured", "apertures_clipped")),
                     "peakfits": (["--fit_blends", "--residual_map", "--residual_peaks", "--residual_scales=4", "--peak_apertures", "--fit_peaks"],
                                  ("apertures_ms", "aperture_kernel_ms", "peakfit_ms", "peakfit_kernel_ms"),
                                  ("peaks_kept", "scales_kept", "scales_strongest", "peakfit_jobs", "peakfit_converged", "peakfit_niter_mean", "peakfit_niter_max",
                                   "peakfit_crowded")),
                     "peakgroups": (["--fit_blends", "--residual_map", "--residual_peaks", "--residual_scales=4", "--peak_apertures", "--fit_peaks",
                                     "--fit_peak_groups"],
                                    ("peakfit_ms", "peakfit_kernel_ms", "peakgroup_ms", "peakgroup_kernel_ms"),
                                    ("peakfit_jobs", "peakfit_crowded", "peakgroup_jobs", "peakgroup_members", "peakgroup_converged", "peakgroup_niter_mean",
                                     "peakgroup_niter_max", "peakgroup_over_limit", "peakgroup_groups")),
                     "subtract": (["--fit_blends", "--residual_map", "--residual_peaks", "--residual_scales=4", "--peak_apertures", "--fit_peaks",
                                   "--fit_peak_groups", "--subtract_peaks"],
                                  ("peakgroup_ms", "peakgroup_kernel_ms", "subtract_ms", "subtract_render_kernel_ms", "disc_residual_kernel_ms",
                                   "left_peaks_kernel_ms"),
                                  ("peakfit_jobs", "subtract_selected", "subtract_rendered", "subtract_wandered", "subtract_duplicates", "left_peaks",
                                   "left_holes", "left_truncated")),
                     "forced": (["--fit_blends", "--residual_map", "--forced_fit"], ("residual_ms", "render_kernel_ms", "forced_ms", "forced_kernel_ms"),
                                ("residual_rendered", "forced_maps", "forced_jobs", "forced_fitted", "forced_crowded", "forced_singular")),
                     "islands": (["--measure_islands"], ("islands_ms", "islands_kernel_ms"), ())}
            skip = {"bkg": args.no_bkg, "deblend": args.no_deblend, "fit": args.no_deblend or args.no_fit,
                    "blend": args.no_deblend or args.no_fit or args.no_blend,
                    "residual": args.no_deblend or args.no_fit or args.no_blend or args.no_residual,
                    "peaks": args.no_deblend or args.no_fit or args.no_blend or args.no_residual or args.no_peaks,
                    "scales": args.no_deblend or args.no_fit or args.no_blend or args.no_residual or args.no_scales,
                    "apertures": args.no_deblend or args.no_fit or args.no_blend or args.no_residual or args.no_scales or args.no_apertures,
                    "peakfits": (args.no_deblend or args.no_fit or args.no_blend or args.no_residual or args.no_scales or args.no_apertures or
                                 args.no_peakfits),
                    "peakgroups": (args.no_deblend or args.no_fit or args.no_blend or args.no_residual or args.no_scales or args.no_apertures or
                                   args.no_peakfits or args.no_peakgroups),
                    "subtract": (args.no_deblend or args.no_fit or args.no_blend or args.no_residual or args.no_scales or args.no_apertures or
                                 args.no_peakfits or args.no_peakgroups or args.no_subtract),
                    "forced": args.no_deblend or args.no_fit or args.no_blend or args.no_residual or args.no_forced,
                    "islands": args.no_islands}
            if args.only:
                skip.update({name: True for name in table if name not in args.only.split(",")})
            variants = [("off", base)] + [(name, base + on + t[0]) for name, t in table.items() if not (args.off_only or skip.get(name))]
            for name, argv in variants:                    # warm-up of each variant
                assert run.main(argv) == 0
            seen.clear()
            got = {name: [] for name, _ in variants}
            for _ in range(args.runs):                     # alternating
                for name, argv in variants:
                    assert run.main(argv) == 0
                    got[name].append(seen.pop())
            for name, rows in got.items():
                res[name] = {"run_ms": [round(r["run_ms"], 1) for r in rows], "run_ms_median": statistics.median(r["run_ms"] for r in rows),
                             "sources": rows[0]["sources"]}
                if name == "off":
                    continue
                for k in table[name][1]:
                    res[name][k] = [round(r[k], 3) for r in rows]
                    res[name][k + "_median"] = statistics.median(r[k] for r in rows)
                res[name].update({k: rows[0][k] for k in table[name][2]})
                res[name]["measure_ms"] = [round(r["measure_ms"], 2) for r in rows]
                res[name]["measure_ms_median"] = statistics.median(r["measure_ms"] for r in rows)
                res[name]["kernel_ms"] = [round(r["kernel_ms"], 3) for r in rows]
                res[name]["kernel_ms_median"] = statistics.median(r["kernel_ms"] for r in rows)
            for name, key in (("on", "added_ms"), ("fit", "fit_added_ms"), ("blend", "blend_added_ms"), ("residual", "residual_added_ms"),
                              ("deblend", "deblend_added_ms"), ("bkg", "bkg_added_ms")):
                if name in got:
                    res[key] = res[name]["run_ms_median"] - res["off"]["run_ms_median"]
            if "peaks" in got and "residual" in got:
                res["peaks_added_ms"] = res["peaks"]["run_ms_median"] - res["residual"]["run_ms_median"]
            if "scales" in got and "residual" in got:
                res["scales_added_ms"] = res["scales"]["run_ms_median"] - res["residual"]["run_ms_median"]
            if "apertures" in got and "scales" in got:
                res["apertures_added_ms"] = res["apertures"]["run_ms_median"] - res["scales"]["run_ms_median"]
            if "peakfits" in got and "apertures" in got:
                res["peakfits_added_ms"] = res["peakfits"]["run_ms_median"] - res["apertures"]["run_ms_median"]
            if "peakgroups" in got and "peakfits" in got:
                res["peakgroups_added_ms"] = res["peakgroups"]["run_ms_median"] - res["peakfits"]["run_ms_median"]
            if "subtract" in got and "peakgroups" in got:
                res["subtract_added_ms"] = res["subtract"]["run_ms_median"] - res["peakgroups"]["run_ms_median"]
            if "forced" in got and "residual" in got:
                res["forced_added_ms"] = res["forced"]["run_ms_median"] - res["residual"]["run_ms_median"]
            if "scales" in got:
                res["atrous_levels"] = atrous_levels(img, args.runs)
            if "bkg" in got:
                res.update(background_kernels(img, args.runs, args.host_ref))
            if "islands" in got:                            # read before the next variant overwrites the catalog: it was the last to run
                from caesar_yolo_amd import measure
                res["islands_added_ms"] = res["islands"]["run_ms_median"] - res["off"]["run_ms_median"]
                src = json.load(open(os.path.join(d, "catalog_s16k.json")))["sources"]
                area = np.array([np.prod(measure.box_window(b, args.size, args.size)[2:]) for b in measure.boxes_of(src)])
                edges = [0, 1, 256, 1024, 4097, 16384, 65536, 262144, 1 << 24, 1 << 62]
                res["window_area_histogram"] = {"[%d, %d)" % (a, b): int(((area >= a) & (area < b)).sum()) for a, b in zip(edges, edges[1:])}
                res["window_area_max"] = int(area.max()) if area.size else 0
                res["lds_share"] = float((area <= 4096).mean()) if area.size else 0.0
                res["with_island"] = int(sum(bool(s["island_count"]) for s in src))
            if args.host_ref and "on" in got:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import measure_ref
                from caesar_yolo_amd import measure
                src = json.load(open(os.path.join(d, "catalog_s16k.json")))["sources"]
                host = np.where(np.isfinite(img), img, np.float32(0)).astype(np.float32)
                t0 = time.time()
                measure_ref.measure(host, measure.boxes_of(src), args.ring)
                res["host_ref_ms"] = 1e3 * (time.time() - t0)
                if "islands" in got:
                    import island_ref
                    t0 = time.time()
                    island_ref.islands(host, measure.boxes_of(src), measure.island_thresholds(src, 5.0, 2.5), 8)
                    res["host_island_ref_ms"] = 1e3 * (time.time() - t0)
        finally:
            os.chdir(cwd)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
