"""Cost of test-time augmentation (developer tool): S16k tiles/s of the tile engine with and without augment, in the same process
and precision, and the achieved bandwidth of the view kernel alone.

    python tools/time_augment.py [--precision fp16x3|fp16|fp32] [--passes N] [--batch B]

The S16k workload is bench.py's: the seeded synthetic 16384 x 16384 mosaic, 512 x 512 tiles at step 0.8 (1600 tiles, ragged edge
classes included), zscale + minmax, imgsz 512, yolov8l nc = 5.  Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats`
the view kernel (augment_pack_kernel) and the augmented decode (decode_augmented_kernel) appear by name."""
import argparse
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge

HBM_PEAK_GBS = 8000.0                  # MI355X HBM3E peak (MI355X_MICROARCH.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp16x3")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--size", type=int, default=16384)
    args = ap.parse_args()
    ge.build()
    from caesar_yolo_amd import synth, utils
    from caesar_yolo_amd import pipelines as CP
    from caesar_yolo_amd.model import YOLO
    from caesar_yolo_amd.inference import TileEngine
    from caesar_yolo_amd import lib as L
    batch = args.batch or (256 if args.precision == "fp16" else 128)
    m = YOLO("seeded:l:5", precision=args.precision, max_batch=batch, max_imgsz=512, device=0)
    det = m.engine(0)
    host = synth.make_mosaic(args.size, seed=20260104)
    mosaic = det.mosaic_to_device(host)
    grid = utils.generate_tiles(0, args.size - 1, 0, args.size - 1, 512, 512, 0.8, 0.8)
    cfg = CP.device_pipeline("zscale+minmax").program()
    res = {"precision": args.precision, "tiles": len(grid), "tile_batch": batch}
    for aug in (False, True):
        eng = TileEngine(det, mosaic, grid, cfg, 512, 0.7, 0.5, 0.3, 0.8, batch=batch, augment=aug)
        eng.run_local()                                  # warm-up (first-call allocations, kernel selection)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(args.passes):
            eng.run_local()
        torch.cuda.synchronize()
        dt = (time.time() - t0) / args.passes
        res["augment" if aug else "plain"] = {"pass_ms": 1000.0 * dt, "tiles_per_s": len(grid) / dt,
                                              "detections": int(eng.cnt_all.sum())}
        del eng
    res["augmented_over_plain"] = res["augment"]["tiles_per_s"] / res["plain"]["tiles_per_s"]
    # the view kernel alone: a batch of letterboxed 512 x 512 fp32 tiles -> views 1 and 2 (and view 0 in fp16)
    src = torch.rand((batch, 512, 512, 4), device="cuda")
    for _ in range(3):
        det.augment_pack(src)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    outs = None
    e0.record()
    for _ in range(10):
        outs = det.augment_pack(src)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 10
    written = sum(o.numel() * o.element_size() for o in (outs if args.precision == "fp16" else outs[1:]))
    moved = src.numel() * 4 + written                    # the source read once (re-reads of neighbouring rows hit the caches) + stores
    views, _ = L.augment_geometry(512, 512)
    res["view_kernel"] = {"ms_per_batch": ms, "bytes": moved, "GB_per_s": moved / ms / 1e6,
                          "fraction_of_hbm_peak": moved / ms / 1e6 / HBM_PEAK_GBS,
                          "views": [(v["ch"], v["Hp"]) for v in views]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
