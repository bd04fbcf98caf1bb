"""Run configuration: the same global dict, same keys and defaults as the reference's caesar_yolo/config.py:4-59
(filled by scripts/run.py:311-338), plus the device-path knobs this build adds (marked NEW)."""

CONFIG = {
    # detection
    'img_size': 640,
    'preprocess_fcn': None,
    'image_path': '',
    'image_xmin': 0, 'image_xmax': 0, 'image_ymin': 0, 'image_ymax': 0,
    # tiling
    'mpi': None,                       # kept for interface compatibility; ranks come from torch.distributed here
    'split_image_in_tiles': False,
    'tile_xsize': 256, 'tile_ysize': 256,
    'tile_xstep': 1.0, 'tile_ystep': 1.0,
    'max_ntasks_per_worker': None,     # reference: 100 (its sequential engine refuses more tiles per rank, inference.py:1151-1160);
                                       # the batched engine has no limit: the guard applies only when a number is given
    # source finding
    'devices': ['cpu'],
    'use_multi_gpu': False,
    'iou_thr': 0.5,
    'merge_overlap_iou_thr_soft': 0.3,
    'merge_overlap_iou_thr_hard': 0.8,
    'score_thr': 0.7,
    # outputs
    'save_catalog': True, 'save_tile_catalog': False, 'outfile_json': '',
    'save_region': True, 'save_tile_region': False, 'outfile': '',
    'save_img': False, 'save_tile_img': False,
    'draw_plot': False, 'draw_class_label_in_caption': True, 'save_plot': False,
    # NEW: HIP tile pipeline
    'tile_batch': 64,                  # tiles per kernel launch sequence
    'precision': 'fp16x3',             # 'fp16x3' (default: parity context), 'fp32' (exact fp32, ~2.7x slower), 'fp16' (throughput, ~3x faster)
    'augment': False,                  # test-time augmentation of every model call (ultralytics augment=True: 3 views, joint NMS)
    'measure_sources': False,          # NEW: flux, peak, centroid, local background and sky position of every catalog source
    'measure_ring': 8,                 # width in pixels of the background ring around a source's box
    'measure_islands': False,          # NEW: seed / merge-threshold islands of every source's box: pixel count, flux, centroid, shape
    'island_seed_sigma': 5.0,          # a pixel at or above bkg + island_seed_sigma * rms seeds an island ...
    'island_merge_sigma': 2.5,         # ... which grows over connected pixels at or above bkg + island_merge_sigma * rms
    'island_conn': 8,                  # 8 or 4 neighbours
    'deblend_islands': False,          # NEW: the island set of every box split into components by local peaks and their basins
    'deblend_peak_sigma': None,        # a local peak at or above bkg + this many rms becomes a component; None: island_seed_sigma
    'deblend_radius': 2,               # a peak is the highest island pixel within this many pixels in x and y (1 .. 8)
    'fit_components': False,           # NEW: one elliptical Gaussian fitted to every component (implies deblend_islands)
    'fit_blends': False,               # NEW: groups of touching components fitted jointly (implies fit_components)
    'fit_max_iter': 64,                # Levenberg-Marquardt iterations per component at most (1 .. 256)
    'residual_map': False,             # NEW: model map of the fitted components, residual map and per-source residuals (implies fit_components)
    'residual_nsigma': 5.0,            # a component is rendered within this many marginal sigmas of its centre (1 .. 8)
    'save_residual_maps': False,       # write the model and residual maps as FITS images beside the catalog (implies residual_map)
    'bkg_map': False,                  # NEW: global background / noise mesh; bkg_map, rms_map, snr_map per source, island thresholds from it
    'bkg_cell': 128,                   # side of a mesh cell in pixels (4 .. 4096)
    'bkg_clip_sigma': 3.0,             # a clip keeps the pixels within this many rms of the cell median ...
    'bkg_clip_iters': 3,               # ... and is applied this many times (0 .. 32)
    'bkg_min_pix': 64,                 # a cell with fewer surviving pixels is filled from the nearest cell that has them
    'save_bkg_maps': False,            # write the per-pixel maps as FITS images beside the catalog
}
