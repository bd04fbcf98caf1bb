#!/usr/bin/env python
"""Command line of the detect path: same flags as the reference's scripts/run.py:58-155 (unused cosmetic flags are
accepted and ignored), same stage order for --preprocessing (:272-302), same CONFIG keys (:311-338).

Differences that come with the MI355X engine:
  --weights  takes a CYW1 file (caesar_yolo_amd/weights.py) or "seeded:<scale>:<nc>[:seed]";
  --devices  lists GPU indices ("0", "cuda:0", "0,1,2,3"); "cpu" (the reference's default) selects GPU LOCAL_RANK with a
             warning: there is no CPU path;
  --max_ntasks_per_worker  has no default here (the reference's 100 would refuse BASELINE configs 3-5); given, it is honoured;
  multi-GPU  = one process per GPU: `python -m torch.distributed.run --nproc-per-node N scripts/run.py ...`
             (replaces `mpirun -np N`, test/run_inference_parallel.sh:47-52);
  --precision fp16x3|fp32|fp16 (default fp16x3 = the fast parity context: fp16 high + low halves, fp32 accumulate; fp32 = exact fp32
  FMA chains, 2.7x slower; fp16 = throughput mode, 3x faster, ~2 % of detections differ), --tile_batch N  are new;
  --augment  (new) test-time augmentation of every model call, ultralytics' augment=True: the tile, its 0.83-scale left-right
             flip and its 0.67-scale view through the network, one NMS over the three (about 2.2x the network work per tile);
  --measure_sources  (new) every source of the final catalog (serial: out_<id>.json, tiled: catalog_<id>.json) also carries
             npix, bkg, rms, peak, snr, x_peak, y_peak, x0, y0, flux_sum, flux, ra, dec, measured on the device-resident image
             (cy_measure_sources; definitions in DESIGN.md); --measure_ring N (default 8) is the width of the background ring.
  --measure_islands  (new; implies --measure_sources) every source also carries the islands of its box: pixels at or above
             bkg + --island_merge_sigma * rms (default 2.5) connected (--island_conn 8 or 4) to a pixel at or above
             bkg + --island_seed_sigma * rms (default 5): island_count, island_npix, island_npix_main, island_border,
             island_x1 / x2 / y1 / y2, island_flux_sum, island_flux, island_flux_main, x_isl, y_isl, ra_isl, dec_isl, major, minor, pa
             (cy_measure_islands; DESIGN.md "Source islands").
  --bkg_map  (new; implies --measure_sources) a global background and noise mesh: clipped median and MAD (--bkg_clip_sigma, default
             3; --bkg_clip_iters, default 3) of every --bkg_cell x --bkg_cell cell (default 128), cells with fewer than --bkg_min_pix
             (default 64) surviving pixels filled from the nearest one, bilinear between the cell centres; every source also
             carries bkg_map, rms_map, snr_map, and with --measure_islands the island thresholds come from them.  --save_bkg_maps
             (implies --bkg_map) writes the per-pixel maps as bkg_<catalog name>.fits / rms_<catalog name>.fits beside the catalog
             (cy_measure_background, cy_expand_background; DESIGN.md "Background mesh").
  --deblend_islands  (new; implies --measure_islands) the island set of every box split into components: local peaks (no
             higher island pixel within --deblend_radius pixels, default 2, 1..8; at or above bkg + --deblend_peak_sigma * rms,
             default = --island_seed_sigma, or the highest pixel of their island) and their steepest-ascent basins, at most 16 per
             box.  Every source also carries npeaks, ncomponents, components_truncated, components_unassigned_npix and components,
             a list of {x, y, ra, dec, peak, x_peak, y_peak, npix, flux_sum, flux, major, minor, pa, main, nsummits}
             (cy_deblend_islands; DESIGN.md "Source components").
  --fit_components  (new; implies --deblend_islands) one elliptical Gaussian fitted to every component by Levenberg-Marquardt on
             the pixels of its basin, at most --fit_max_iter iterations (default 64, 1..256).  Every component also carries
             fit_status, fit_niter, fit_npix, fit_chi2, fit_peak, fit_x, fit_y, fit_ra, fit_dec, fit_major, fit_minor, fit_pa,
             fit_flux and fit_peak_err, fit_x_err, fit_y_err, fit_flux_err (cy_fit_components; DESIGN.md "Component fits").
  --fit_blends  (new; implies --fit_components) every group of two to four touching components fitted jointly, the sum of their
             Gaussians on the union of their basins, from the single fits as starts and with --fit_max_iter.  Every component
             also carries blend_group, blend_size, blend_status and the blend_ namesakes of the fit_ keys (cy_fit_blends;
             DESIGN.md "Joint fits of blends").
  --residual_map  (new; implies --fit_components) the sum of the fitted components (the joint fit where --fit_blends gave one, every
             peak pixel once) rendered over the whole image, each inside --residual_nsigma (default 5, 1..8) marginal sigmas, and
             the residual image - background - model measured in every source's box and island set.  Every source also carries
             res_npix, res_mean, res_rms, res_rms_box, res_max, res_x_max, res_y_max, res_flux, res_model_flux, res_ratio, every
             component rendered and render_status; with --bkg_map the residual is background-subtracted.  --save_residual_maps
             (implies --residual_map) writes model_<catalog name>.fits / resid_<catalog name>.fits beside the catalog
             (cy_render_gaussians, cy_measure_residuals; DESIGN.md "Model and residual maps").
  --residual_peaks  (new; implies --residual_map and --bkg_map) the residual map searched for what the model does not explain: its
             local maxima within --residual_peaks_radius pixels (default 2, 1..8) at or above --residual_peaks_sigma (default 5)
             times the rms map of the mesh, at most --residual_peaks_max of them (default 65536, up to 2^20), kept when at least
             --residual_peaks_min_above (default 3) pixels of the neighbourhood are above the threshold.  The catalog file gains a
             list "residual_peaks" beside the sources (x_peak, y_peak, x, y, ra, dec, peak, rms, snr, npix, nabove, flux_sum, flux,
             in_source) in decreasing snr, and every source res_npeaks and res_peak_snr.  --residual_holes (implies the same) also
             searches the negated residual: "residual_holes", res_nholes, res_hole_snr (cy_find_peaks; DESIGN.md "Residual peaks").
  --residual_scales J  (new; 0..6, default 0 = off; implies --residual_map and --bkg_map) the residual map split into J a trous
             (B3-spline) wavelet planes on the GPU, plane j with its taps 2^(j-1) pixels apart, and every plane from
             --residual_scale_first on (default 2, 1..J) searched for local maxima at or above --residual_scales_sigma (default 5)
             times a noise map measured on that plane: emission that is faint per pixel but many pixels wide.  The catalog file
             gains a list "residual_scale_peaks" (the keys of "residual_peaks", then scale, step, strongest) in decreasing snr over
             all scales, and every source res_nscale_peaks and res_scale_peak_snr.  Radius, min_above and the cap are those of
             --residual_peaks (the radius at least the step, at most 8).  --save_scale_maps writes the searched planes as
             wav<j>_<catalog name>.fits beside the catalog (cy_atrous_step; DESIGN.md "Residual scales").
  --peak_apertures  (new; implies --residual_map and --bkg_map, and --residual_peaks when no search of the residual map is on)
             every entry of "residual_peaks", "residual_holes" and "residual_scale_peaks" measured on the residual map in
             concentric circular apertures of --aperture_radii (default 1,2,3,4; at most 7) times --aperture_unit (default 1)
             pixels, times the entry's step for a scale peak, with the median of the annulus from the last radius out to
             --aperture_annulus (default 6) as local background and the rms map of the mesh as noise: ap_status, ap_clipped,
             ap_radius, ap_npix, ap_sum, ap_bkg, ap_bkg_rms, ap_nbkg, ap_flux_sum, ap_flux, ap_flux_err, ap_snr, ap_best per
             entry, a curve of growth (cy_aperture_sums; DESIGN.md "Peak apertures").
  --fit_peaks  (new; implies what --peak_apertures implies) one elliptical Gaussian fitted on the GPU to the residual map around every
             entry of the peak lists (of "residual_scale_peaks" the strongest ones), inside a disc of --fit_peaks_radius (default 6)
             pixels times the entry's step that it shares with neighbouring entries by a nearest-centre rule, from a circular start
             of --fit_peaks_sigma (default 1.5) pixels, at most --fit_peaks_max_iter (default 64) iterations; holes are fitted with
             a sign: gfit_status .. gfit_flux_err per entry (cy_fit_peaks; DESIGN.md "Peak fits").
  --fit_peak_groups  (new; implies --fit_peaks) the entries of a list whose centres are closer than --fit_peaks_link (default 1.5, at
             most 2) times the larger of their disc radii are fitted together on the GPU, two to four Gaussians on the union of
             their discs, started from the single fits; larger groups keep their single fits: gblend_group, gblend_size,
             gblend_slot, gblend_status .. gblend_flux_err per entry (cy_fit_peak_groups; DESIGN.md "Peak groups").
  --subtract_peaks  (new; implies --fit_peaks) the fitted peaks (the group fit of an entry where there is one, else its single fit;
             a fit that left its disc and a scale peak that repeats a pixel peak left out) are rendered on the GPU and subtracted
             from the residual map: a second residual.  Holes are rendered with a negative amplitude, so the emission they were
             fitted on is subtracted as well.  Every fitted entry gains gres_subtracted, gres_source,
             gres_render_status, gres_npix, gres_mean, gres_rms, gres_max, gres_x_max, gres_y_max, gres_ratio, gres_chi2 and
             gres_model_flux, measured on the second residual over the pixels of its fit; the catalog file gains the lists
             "residual_peaks_left" and "residual_holes_left" (the keys of "residual_peaks"), the search of --residual_peaks run
             on the second residual in both signs, and every source res_npeaks_left and res_nholes_left.  With
             --save_residual_maps the peak model and the second residual are written as peakmodel_<catalog name>.fits and
             resid2_<catalog name>.fits (cy_render_gaussians, cy_disc_residuals; DESIGN.md "Second residual").
  --forced_fit  (new; implies --residual_map) forced photometry: every component of the model map is measured again with its
             fitted position and shape fixed; only its amplitude, those of its overlapping neighbours (at most seven) and a local
             constant (--forced_fit_bkg 1, the default) are solved, a weighted linear least-squares problem per component on the
             pixels within --forced_nsigma (default 3) sigma, with the rms map of --bkg_map as weights when there is one.  Every
             rendered component gains "forced": one dict per measured map with image, status, npix, nneigh, crowded, peak,
             peak_err, bkg, chi2, corr_max, flux, flux_err (cy_forced_fit; DESIGN.md "Forced photometry").
  --forced_images a.fits,b.fits  (new; implies --forced_fit) co-registered maps of the image's shape (another frequency, epoch or
             Stokes plane) measured the same way after the image itself ("self"), each with its own background mesh, beam and
             frequency; a map of another shape ends the run before detection.  The catalog file gains "forced_images" (tag, path,
             freq, beam_area, mesh_ndef per map) and, when two maps carry a frequency, every component forced_alpha,
             forced_alpha_err and forced_alpha_n.
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from caesar_yolo_amd.config import CONFIG                                     # noqa: E402
from caesar_yolo_amd.preprocessing import (DataPreprocessor, BkgSubtractor, SigmaClipShifter, SigmaClipper, ChanResizer,  # noqa: E402
                                           ZScaleTransformer, Chan3Trasformer, MinMaxNormalizer)
from caesar_yolo_amd.inference import SFinder                                 # noqa: E402
from caesar_yolo_amd.measure import aperture_config, peakfit_config, peakgroup_config, plan, wants_peaks, wants_scales  # noqa: E402
from caesar_yolo_amd.model import YOLO                                        # noqa: E402

logging.basicConfig(format="%(asctime)-15s %(levelname)s - %(message)s", datefmt='%Y-%m-%d %H:%M:%S')
logger = logging.getLogger("caesar_yolo_amd")
logger.setLevel(logging.INFO)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='CAESAR-YOLO options (MI355X build)')
    p.add_argument('--image', required=False, type=str)
    p.add_argument('--datalist', required=False)
    p.add_argument('--maxnimgs', required=False, type=int, default=-1)
    p.add_argument('--weights', required=True)
    p.add_argument('--imgsize', dest='imgsize', type=int, default=640)
    p.add_argument('--preprocessing', dest='preprocessing', action='store_true')
    p.add_argument('--normalize_minmax', dest='normalize_minmax', action='store_true')
    p.add_argument('-norm_min', '--norm_min', dest='norm_min', type=float, default=0.)
    p.add_argument('-norm_max', '--norm_max', dest='norm_max', type=float, default=1.)
    p.add_argument('--subtract_bkg', dest='subtract_bkg', action='store_true')
    p.add_argument('-sigma_bkg', '--sigma_bkg', dest='sigma_bkg', type=float, default=3)
    p.add_argument('--use_box_mask_in_bkg', dest='use_box_mask_in_bkg', action='store_true')
    p.add_argument('-bkg_box_mask_fract', '--bkg_box_mask_fract', dest='bkg_box_mask_fract', type=float, default=0.7)
    p.add_argument('-bkg_chid', '--bkg_chid', dest='bkg_chid', type=int, default=-1)
    p.add_argument('--clip_shift_data', dest='clip_shift_data', action='store_true')
    p.add_argument('-sigma_clip', '--sigma_clip', dest='sigma_clip', type=float, default=1)
    p.add_argument('--clip_data', dest='clip_data', action='store_true')
    p.add_argument('-sigma_clip_low', '--sigma_clip_low', dest='sigma_clip_low', type=float, default=10)
    p.add_argument('-sigma_clip_up', '--sigma_clip_up', dest='sigma_clip_up', type=float, default=10)
    p.add_argument('-clip_chid', '--clip_chid', dest='clip_chid', type=int, default=-1)
    p.add_argument('--zscale_stretch', dest='zscale_stretch', action='store_true')
    p.add_argument('--zscale_contrasts', dest='zscale_contrasts', type=str, default='0.25,0.25,0.25')
    p.add_argument('--chan3_preproc', dest='chan3_preproc', action='store_true')
    p.add_argument('-sigma_clip_baseline', '--sigma_clip_baseline', dest='sigma_clip_baseline', type=float, default=0)
    p.add_argument('-nchannels', '--nchannels', dest='nchannels', type=int, default=1)
    p.add_argument('--scoreThr', default=0.7, type=float)
    p.add_argument('--iouThr', default=0.5, type=float)
    p.add_argument('--merge_overlap_iou_thr_soft', default=0.3, type=float)
    p.add_argument('--merge_overlap_iou_thr_hard', default=0.8, type=float)
    for a in ('xmin', 'xmax', 'ymin', 'ymax'):
        p.add_argument('--' + a, dest=a, type=int, default=-1)
    p.add_argument('--split_img_in_tiles', dest='split_img_in_tiles', action='store_true')
    p.add_argument('--tile_xsize', type=int, default=512)
    p.add_argument('--tile_ysize', type=int, default=512)
    p.add_argument('--tile_xstep', type=float, default=1.0)
    p.add_argument('--tile_ystep', type=float, default=1.0)
    p.add_argument('--max_ntasks_per_worker', type=int, default=None,
                   help='refuse the run if a rank holds more tiles (reference default 100; here: no limit unless given)')
    p.add_argument('--devices', type=str, default="cpu")
    p.add_argument('--multigpu', dest='multigpu', action='store_true')
    for a in ('draw_plots', 'draw_class_label_in_caption', 'save_plots', 'save_tile_catalog', 'save_tile_region', 'save_tile_img'):
        p.add_argument('--' + a, dest=a, action='store_true')
    p.add_argument('--detect_outfile', type=str, default="")
    p.add_argument('--detect_outfile_json', type=str, default="")
    p.add_argument('--precision', type=str, default="fp16x3", choices=["fp16", "fp16x3", "fp32"],
                   help='arithmetic of the detector.  fp16x3 (default): parity context -- activations and weights as fp16 high + low halves, '
                        'fp32 accumulate; kept boxes identical to the fp32 oracle, boxes within 1e-4 of the image size (<= 0.06 px), scores 2e-5.  '
                        'fp32: exact fp32 FMA chains (the reference\'s own arithmetic), ~2.7x slower than fp16x3.  fp16: throughput mode, fp16 '
                        'operands / fp32 accumulate, ~3x the fp16x3 rate; 2-4 %% of the detections differ from the fp32 run (DESIGN.md section 2)')
    p.add_argument('--tile_batch', type=int, default=64)
    p.add_argument('--augment', dest='augment', action='store_true',
                   help='test-time augmentation (ultralytics augment=True): three views per tile, one joint NMS')
    p.add_argument('--measure_sources', dest='measure_sources', action='store_true',
                   help='measure every catalog source on the GPU: background, rms, peak, centroid, flux and sky position')
    p.add_argument('--measure_ring', dest='measure_ring', type=int, default=8,
                   help='width in pixels of the background ring around a source box (with --measure_sources)')
    p.add_argument('--measure_islands', dest='measure_islands', action='store_true',
                   help='extract the seed / merge-threshold islands of every source box on the GPU: pixel count, flux, centroid, shape '
                        '(implies --measure_sources)')
    p.add_argument('--island_seed_sigma', dest='island_seed_sigma', type=float, default=5.0,
                   help='an island needs a pixel at or above bkg + this many rms (with --measure_islands)')
    p.add_argument('--island_merge_sigma', dest='island_merge_sigma', type=float, default=2.5,
                   help='an island grows over connected pixels at or above bkg + this many rms (with --measure_islands)')
    p.add_argument('--island_conn', dest='island_conn', type=int, choices=[4, 8], default=8,
                   help='neighbours that connect the pixels of an island (with --measure_islands)')
    p.add_argument('--bkg_map', dest='bkg_map', action='store_true',
                   help='estimate a global background / noise mesh on the GPU and add bkg_map, rms_map, snr_map to every source; the island '
                        'thresholds of --measure_islands then come from it (implies --measure_sources)')
    p.add_argument('--bkg_cell', dest='bkg_cell', type=int, default=128, help='side of a mesh cell in pixels, 4 .. 4096 (with --bkg_map)')
    p.add_argument('--bkg_clip_sigma', dest='bkg_clip_sigma', type=float, default=3.0,
                   help='a clip keeps the pixels within this many rms of the cell median (with --bkg_map)')
    p.add_argument('--bkg_clip_iters', dest='bkg_clip_iters', type=int, default=3, help='number of clips, 0 .. 32 (with --bkg_map)')
    p.add_argument('--bkg_min_pix', dest='bkg_min_pix', type=int, default=64,
                   help='a cell with fewer surviving pixels takes the values of the nearest cell that has them (with --bkg_map)')
    p.add_argument('--save_bkg_maps', dest='save_bkg_maps', action='store_true',
                   help='write the per-pixel background and noise maps as bkg_<catalog>.fits / rms_<catalog>.fits beside the catalog '
                        '(implies --bkg_map)')
    p.add_argument('--deblend_islands', dest='deblend_islands', action='store_true',
                   help='split the islands of every source box into components by local peaks and steepest-ascent basins on the GPU '
                        '(implies --measure_islands)')
    p.add_argument('--deblend_peak_sigma', dest='deblend_peak_sigma', type=float, default=None,
                   help='a local peak becomes a component at or above bkg + this many rms (default: --island_seed_sigma; with --deblend_islands)')
    p.add_argument('--deblend_radius', dest='deblend_radius', type=int, choices=list(range(1, 9)), default=2,
                   help='a peak is the highest island pixel within this many pixels in x and y (with --deblend_islands)')
    p.add_argument('--fit_components', dest='fit_components', action='store_true',
                   help='fit one elliptical Gaussian to every component on the GPU (implies --deblend_islands)')
    p.add_argument('--fit_max_iter', dest='fit_max_iter', type=int, choices=list(range(1, 257)), default=64, metavar='N',
                   help='Levenberg-Marquardt iterations per component at most, 1..256 (with --fit_components)')
    p.add_argument('--fit_blends', dest='fit_blends', action='store_true',
                   help='fit every group of touching components jointly on the GPU (implies --fit_components; reuses --fit_max_iter)')
    p.add_argument('--residual_map', dest='residual_map', action='store_true',
                   help='render the fitted components into a model map on the GPU and measure the residual of every source '
                        '(implies --fit_components; uses the joint fits with --fit_blends)')
    p.add_argument('--residual_nsigma', dest='residual_nsigma', type=float, default=5.0,
                   help='a component is rendered within this many marginal sigmas of its centre, 1..8 (with --residual_map)')
    p.add_argument('--save_residual_maps', dest='save_residual_maps', action='store_true',
                   help='write the model and residual maps as model_<catalog name>.fits / resid_<catalog name>.fits beside the catalog '
                        '(implies --residual_map)')
    p.add_argument('--residual_peaks', dest='residual_peaks', action='store_true',
                   help='list the local maxima of the residual map above the noise map on the GPU (implies --residual_map and --bkg_map)')
    p.add_argument('--residual_peaks_sigma', dest='residual_peaks_sigma', type=float, default=5.0,
                   help='a residual peak lies at or above this many times the rms map (with --residual_peaks)')
    p.add_argument('--residual_peaks_radius', dest='residual_peaks_radius', type=int, choices=list(range(1, 9)), default=2, metavar='R',
                   help='a residual peak is the highest pixel within this many pixels in x and y, 1..8 (with --residual_peaks)')
    p.add_argument('--residual_peaks_min_above', dest='residual_peaks_min_above', type=int, default=3,
                   help='a residual peak is kept when this many pixels of its neighbourhood are above the threshold (with --residual_peaks)')
    p.add_argument('--residual_peaks_max', dest='residual_peaks_max', type=int, default=65536,
                   help='residual peaks read back at most, 0..2^20, in row-major order (with --residual_peaks)')
    p.add_argument('--residual_holes', dest='residual_holes', action='store_true',
                   help='also list the local minima of the residual map below minus the threshold (implies what --residual_peaks implies)')
    p.add_argument('--residual_scales', dest='residual_scales', type=int, choices=list(range(0, 7)), default=0, metavar='J',
                   help='search J a trous wavelet planes of the residual map on the GPU, 0..6, 0 = off (implies --residual_map and --bkg_map)')
    p.add_argument('--residual_scale_first', dest='residual_scale_first', type=int, default=2,
                   help='first wavelet scale that is searched, 1..J (with --residual_scales)')
    p.add_argument('--residual_scales_sigma', dest='residual_scales_sigma', type=float, default=5.0,
                   help='a peak of a wavelet plane lies at or above this many times the rms map of that plane (with --residual_scales)')
    p.add_argument('--save_scale_maps', dest='save_scale_maps', action='store_true',
                   help='write every searched wavelet plane as wav<j>_<catalog name>.fits beside the catalog (with --residual_scales)')
    p.add_argument('--peak_apertures', dest='peak_apertures', action='store_true',
                   help='aperture photometry of every residual peak, hole and scale peak on the residual map (implies what --residual_peaks implies; alone it turns --residual_peaks on)')
    p.add_argument('--aperture_unit', dest='aperture_unit', type=float, default=1.0,
                   help='pixels of one radius unit at step 1; a scale peak multiplies it by its step (with --peak_apertures)')
    p.add_argument('--aperture_radii', dest='aperture_radii', default="1,2,3,4",
                   help='comma-separated aperture radii in units of --aperture_unit, strictly increasing, at most 7 (with --peak_apertures)')
    p.add_argument('--aperture_annulus', dest='aperture_annulus', type=float, default=6.0,
                   help='outer radius of the background annulus, which starts at the last aperture radius (with --peak_apertures)')
    p.add_argument('--fit_peaks', dest='fit_peaks', action='store_true',
                   help='fit a Gaussian to the residual map around every residual peak, hole and strongest scale peak (implies what --peak_apertures implies; alone it turns --residual_peaks on)')
    p.add_argument('--fit_peaks_radius', dest='fit_peaks_radius', type=float, default=6.0,
                   help='radius in pixels of the disc that is fitted at step 1; a scale peak multiplies it by its step (with --fit_peaks)')
    p.add_argument('--fit_peaks_sigma', dest='fit_peaks_sigma', type=float, default=1.5,
                   help='sigma in pixels of the circular start at step 1; a scale peak multiplies it by its step (with --fit_peaks)')
    p.add_argument('--fit_peaks_max_iter', dest='fit_peaks_max_iter', type=int, default=64,
                   help='iterations of a peak fit at most, 1..256 (with --fit_peaks)')
    p.add_argument('--fit_peak_groups', dest='fit_peak_groups', action='store_true',
                   help='fit neighbouring entries of a peak list jointly, two to four Gaussians on the union of their discs (implies --fit_peaks)')
    p.add_argument('--fit_peaks_link', dest='fit_peaks_link', type=float, default=1.5,
                   help='entries closer than this times the larger of their disc radii are fitted together, in (0, 2] (with --fit_peak_groups)')
    p.add_argument('--subtract_peaks', dest='subtract_peaks', action='store_true',
                   help='subtract the fitted peaks from the residual map, measure every fit on that second residual and search it again in both signs (implies --fit_peaks)')
    p.add_argument('--forced_fit', dest='forced_fit', action='store_true',
                   help='forced photometry: the amplitude of every rendered component with its fitted position and shape fixed, on the image itself (implies --residual_map)')
    p.add_argument('--forced_images', dest='forced_images', type=str, default='',
                   help='comma-separated FITS maps of the same field and shape that are measured the same way (implies --forced_fit)')
    p.add_argument('--forced_nsigma', dest='forced_nsigma', type=float, default=3.0,
                   help='the pixels of a forced fit lie within this many sigma of the component, in [1, 8] (with --forced_fit)')
    p.add_argument('--forced_fit_bkg', dest='forced_fit_bkg', type=int, default=1, choices=(0, 1),
                   help='1: a local constant is fitted beside the amplitudes; 0: the background is the one given (with --forced_fit)')
    args = p.parse_args(argv)
    if args.forced_images:
        args.forced_fit = True
    if args.forced_fit and not 1.0 <= args.forced_nsigma <= 8.0:
        p.error("--forced_nsigma must be in [1, 8]")
    if args.subtract_peaks:
        args.fit_peaks = True                                 # what is subtracted are the fits
    if args.fit_peak_groups:
        try:
            peakgroup_config(vars(args))
        except ValueError as e:
            p.error("--fit_peak_groups: %s" % e)
        args.fit_peaks = True                                 # the joint fits start from the single ones
    if args.fit_peaks:
        try:
            peakfit_config(vars(args))
        except ValueError as e:
            p.error("--fit_peaks: %s" % e)
        if not (wants_peaks(vars(args)) or wants_scales(vars(args))):
            args.residual_peaks = True                        # fits need a list, as apertures do
    if args.peak_apertures:
        try:
            aperture_config(vars(args))
        except ValueError as e:
            p.error("--peak_apertures: %s" % e)
        if not (wants_peaks(vars(args)) or wants_scales(vars(args))):
            args.residual_peaks = True                        # apertures need a list: the pixel search, as the other implied flags are set
    if args.residual_scales > 0 and not 1 <= args.residual_scale_first <= args.residual_scales:
        p.error("--residual_scale_first must be in [1, --residual_scales]")
    steps = plan(vars(args))                                  # the "implies" of the switches above: one rule, measure.plan
    args.measure_sources, args.bkg_map, args.measure_islands = "measure" in steps, "background" in steps, "islands" in steps
    args.deblend_islands, args.fit_components, args.residual_map = "deblend" in steps, "fit" in steps, "residual" in steps
    if args.deblend_peak_sigma is None:
        args.deblend_peak_sigma = args.island_seed_sigma
    return args


def validate_args(args):
    if not args.image:
        logger.error("Argument --image is required for detect task!")
        return -1
    if not os.path.isfile(args.image):
        logger.error("Image argument must be an existing image on filesystem!")
        return -1
    if not args.image.endswith('.fits'):
        logger.error("Image must have .fits extension on the HIP path!")
        return -1
    if not args.weights.startswith("seeded:") and not os.path.isfile(args.weights):
        logger.error("Given weight file %s not existing or not a file!" % args.weights)
        return -1
    if args.measure_ring < 0:
        logger.error("--measure_ring must be >= 0!")
        return -1
    if args.measure_islands and not args.island_seed_sigma >= args.island_merge_sigma:
        logger.error("--island_seed_sigma must not be below --island_merge_sigma!")
        return -1
    if not 4 <= args.bkg_cell <= 4096:
        logger.error("--bkg_cell must be in [4, 4096]!")
        return -1
    if not args.bkg_clip_sigma > 0:
        logger.error("--bkg_clip_sigma must be > 0!")
        return -1
    if not 0 <= args.bkg_clip_iters <= 32:
        logger.error("--bkg_clip_iters must be in [0, 32]!")
        return -1
    if args.bkg_min_pix < 1:
        logger.error("--bkg_min_pix must be >= 1!")
        return -1
    if not (args.residual_peaks_sigma > 0 and args.residual_peaks_sigma < float("inf")):
        logger.error("--residual_peaks_sigma must be > 0 and finite!")
        return -1
    if not (args.residual_scales_sigma > 0 and args.residual_scales_sigma < float("inf")):
        logger.error("--residual_scales_sigma must be > 0 and finite!")
        return -1
    if not 0 <= args.residual_peaks_max <= (1 << 20):
        logger.error("--residual_peaks_max must be in [0, 2^20]!")
        return -1
    if args.split_img_in_tiles and (args.xmin >= 0 or args.xmax >= 0 or args.ymin >= 0 or args.ymax >= 0):
        # serial runs crop like the reference (inference.py:499-505); the tiled run of the reference derives its grid from
        # attributes it has not set yet when a range is given (inference.py:374-381): refused here
        logger.error("Sub-image ranges together with --split_img_in_tiles are not supported (broken in the reference: inference.py:374-381)")
        return -1
    return 0


def build_preprocessor(args):
    """Stage list in the reference's fixed order (scripts/run.py:272-302)."""
    zc = [float(x) for x in args.zscale_contrasts.split(',')]
    st = []
    if args.subtract_bkg:
        st.append(BkgSubtractor(sigma=args.sigma_bkg, use_mask_box=args.use_box_mask_in_bkg, mask_fract=args.bkg_box_mask_fract, chid=args.bkg_chid))
    if args.clip_shift_data:
        st.append(SigmaClipShifter(sigma=args.sigma_clip, chid=args.clip_chid))
    if args.clip_data:
        st.append(SigmaClipper(sigma_low=args.sigma_clip_low, sigma_up=args.sigma_clip_up, chid=args.clip_chid))
    if args.nchannels > 1:
        st.append(ChanResizer(nchans=args.nchannels))
    if args.zscale_stretch:
        st.append(ZScaleTransformer(contrasts=zc))
    if args.chan3_preproc:
        st.append(Chan3Trasformer(sigma_clip_baseline=args.sigma_clip_baseline, sigma_clip_low=args.sigma_clip_low,
                                  sigma_clip_up=args.sigma_clip_up, zscale_contrast=zc[0]))
    if args.normalize_minmax:
        st.append(MinMaxNormalizer(norm_min=args.norm_min, norm_max=args.norm_max))
    if not args.preprocessing:
        return None
    if not st:
        logger.warning("No pre-processing steps defined ...")
        return None
    return DataPreprocessor(st)


MEASURE_KEYS = ('measure_sources', 'measure_ring', 'measure_islands', 'island_seed_sigma', 'island_merge_sigma', 'island_conn', 'deblend_islands',
                'deblend_peak_sigma', 'deblend_radius', 'fit_components', 'fit_max_iter', 'fit_blends', 'residual_map', 'residual_nsigma',
                'save_residual_maps', 'bkg_map', 'bkg_cell', 'bkg_clip_sigma', 'bkg_clip_iters', 'bkg_min_pix', 'save_bkg_maps',
                'residual_peaks', 'residual_peaks_sigma', 'residual_peaks_radius', 'residual_peaks_min_above', 'residual_peaks_max',
                'residual_holes', 'residual_scales', 'residual_scale_first', 'residual_scales_sigma', 'save_scale_maps',
                'peak_apertures', 'aperture_unit', 'aperture_radii', 'aperture_annulus',
                'fit_peaks', 'fit_peaks_radius', 'fit_peaks_sigma', 'fit_peaks_max_iter', 'fit_peak_groups', 'fit_peaks_link',
                'subtract_peaks', 'forced_fit', 'forced_images', 'forced_nsigma', 'forced_fit_bkg')


def measure_config(args):
    """The CONFIG entries of the measurement steps: the parsed arguments of the same names (parse_args set the implied ones)."""
    return {k: getattr(args, k) for k in MEASURE_KEYS}


def main(argv=None):
    args = parse_args(argv)
    if validate_args(args) < 0:
        return 1
    if args.chan3_preproc and args.nchannels != 3:
        logger.error("You selected chan3_preproc pre-processing options, you must set nchannels options to 3!")
        return 1
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    C = CONFIG
    C.update({'img_size': args.imgsize, 'preprocess_fcn': build_preprocessor(args), 'image_path': args.image,
              'image_xmin': args.xmin, 'image_xmax': args.xmax, 'image_ymin': args.ymin, 'image_ymax': args.ymax,
              'split_image_in_tiles': args.split_img_in_tiles, 'tile_xsize': args.tile_xsize, 'tile_ysize': args.tile_ysize,
              'tile_xstep': args.tile_xstep, 'tile_ystep': args.tile_ystep, 'max_ntasks_per_worker': args.max_ntasks_per_worker,
              'devices': [str(x) for x in args.devices.split(',')], 'use_multi_gpu': args.multigpu, 'iou_thr': args.iouThr,
              'score_thr': args.scoreThr, 'merge_overlap_iou_thr_soft': args.merge_overlap_iou_thr_soft,
              'merge_overlap_iou_thr_hard': args.merge_overlap_iou_thr_hard, 'outfile': args.detect_outfile,
              'outfile_json': args.detect_outfile_json, 'save_region': True, 'tile_batch': args.tile_batch,
              'draw_plot': args.draw_plots, 'draw_class_label_in_caption': args.draw_class_label_in_caption,
              'save_plot': args.save_plots,
              'save_tile_catalog': args.save_tile_catalog, 'save_tile_region': args.save_tile_region,
              'save_tile_img': args.save_tile_img,
              'precision': args.precision, 'augment': args.augment})
    C.update(measure_config(args))
    model = YOLO(args.weights, precision=args.precision, max_batch=args.tile_batch if args.split_img_in_tiles else 1,
                 max_imgsz=max(args.imgsize, 32))
    sfinder = SFinder(model, C)
    status = sfinder.run_parallel() if args.split_img_in_tiles else sfinder.run()
    if world > 1:
        dist.destroy_process_group()
    if status < 0:
        logger.error("sfinder run failed, see logs...")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
