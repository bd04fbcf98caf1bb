"""Cost of the detect head's box branch, dense against deferred to the candidate anchors, on benchmark tiles (developer tool).

A batch of 256 full 512-px tiles of the seeded synthetic sky runs the forward pass (a) dense, as cy_forward does, and (b) with the
box branch computed only where the best class score passes `conf` (cy_debug_sparse_box), for several conf: milliseconds per pass
(median of N, hipEvents around the pass alone) and the share of anchors that are candidates.  The difference (a) - (b) is what
the deferred form saves or costs at that candidate density; CY_SPARSE_BOX's conf floor is read off this table.
usage: python tools/sparse_box_cost.py [mosaic edge, default 8192] [passes, default 9]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
ge.build()
from caesar_yolo_amd import synth, utils, preprocessing as PP
from caesar_yolo_amd.model import YOLO
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
m = YOLO("seeded:l:5", precision="fp16", max_batch=256, max_imgsz=512, device=0)
det = m.engine(0)
mos = det.mosaic_to_device(synth.make_mosaic(n, seed=20260104))
grid = [t for t in utils.generate_tiles(0, n - 1, 0, n - 1, 512, 512, 0.8, 0.8) if t[1] - t[0] == 512 and t[3] - t[2] == 512][:256]
cfg = PP.DataPreprocessor([PP.ZScaleTransformer([0.25] * 3), PP.MinMaxNormalizer(0, 255)]).program()
netin, st, lb = det.preproc(mos, [(t[0], t[2]) for t in grid], 512, 512, 512, cfg)
pred = det.forward(netin)
torch.cuda.synchronize()
best = torch.sigmoid(pred[:, :, 64:]).max(dim=2).values


def timed(fn):
    ms = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms[2:])
    return float(np.median(ms)), float(ms.min()), float(ms.max())


out = torch.empty_like(pred)
d = timed(lambda: det.forward(netin, out=out))
print("tiles %d  dense forward: %.3f ms (%.3f .. %.3f)" % (len(grid), d[0], d[1], d[2]))
print("| conf | candidates / anchors | deferred forward ms (min .. max) | dense - deferred ms |")
print("|---|---|---|---|")
for conf in (0.9, 0.7, 0.5, 0.25, 0.1, 0.05, 0.02, 0.01, 0.001, 0.0):
    s = timed(lambda: det.forward_sparse_box(netin, conf, out))
    frac = float((best > conf).float().mean())
    print("| %.3f | %.4f | %.3f (%.3f .. %.3f) | %+.3f |" % (conf, frac, s[0], s[1], s[2], d[0] - s[0]))
