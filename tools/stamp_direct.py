"""Phase anatomy of the pixels-direct 1x1 / 3x3-s2 kernel (developer tool; diagnostic build `CY_STAMPS=1 python __graft_entry__.py
--force`, run with CY_DBG=64; CY_DIRECT_PERSIST=0 / 2 chooses the one-tile / persistent form of the 256-channel tile).
python tools/stamp_direct.py B H W Cin Cout [k s]
Prints the phases of the one-tile form (entry -> loop, loop, epilogue), and for either form the workgroups' whole lives and the
gaps between consecutive workgroups of one CU (entry of the next minus exit of the one before), from the per-workgroup records."""
import os, sys, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from caesar_yolo_amd.model import HipDetector
from caesar_yolo_amd import weights as W, lib as L
B, H, Wd, Cin, Cout = [int(x) for x in sys.argv[1:6]]
k = int(sys.argv[6]) if len(sys.argv) > 6 else 1
s = int(sys.argv[7]) if len(sys.argv) > 7 else 1
wp = "/tmp/cy_bench_seed.cyw"
if not os.path.exists(wp):
    W.make_seeded_file(wp, "l", 5)
det = HipDetector(wp, device=0, precision="fp16", max_batch=1, max_imgsz=64)
x = torch.randn((B, H, Wd, Cin), device="cuda").half()
w = (np.random.default_rng(0).standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
b = np.zeros(Cout, np.float32)
st = (C.c_ulonglong * 8)()
for i in range(5):
    if i == 2:
        L.load().cy_debug_stamps(st, 1)
    det.conv_bn_silu(x, w, b, k, s, True)
L.load().cy_debug_stamps(st, 0)
pro, loop, epi, cyc, tot, _, n = [float(st[i]) for i in range(7)]
chunks = Cin // 64 * k * k
u = 0.01
persist = os.environ.get("CY_DIRECT_PERSIST", "1") != "0"
if n and not persist:
    print("workgroups sampled %d, %d chunks; us per workgroup: entry->loop %.2f | loop %.2f (%.3f per chunk) | epilogue %.2f | clock in the loop %.0f MHz"
          % (n, chunks, u * pro / n, u * loop / n, u * loop / n / chunks, u * epi / n, cyc / (u * loop)))
# whole lives and hand-overs of the LAST launch: (entry, exit, CU) per workgroup
Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (Wd + 2 * (k // 2) - k) // s + 1
tiles = ((B * Ho * Wo + 255) // 256) * ((Cout + 255) // 256)
nrec = min(tiles, 4096)
raw = (C.c_ulonglong * (nrec * 3))()
L.load().cy_debug_stamps(raw, -(1 << 20) - nrec)
rec = np.array(list(raw), np.float64).reshape(nrec, 3)
rec = rec[rec[:, 1] > 0]
life = (rec[:, 1] - rec[:, 0]) * u
gaps = []
for cu in np.unique(rec[:, 2]):
    r = rec[rec[:, 2] == cu]
    r = r[np.argsort(r[:, 0])]
    gaps += list((r[1:, 0] - r[:-1, 1]) * u)
gaps = np.array(gaps) if gaps else np.zeros(1)
span = (rec[:, 1].max() - rec[:, 0].min()) * u
print("%d workgroup records on %d CUs, %d tiles: life us min %.2f median %.2f p90 %.2f max %.2f | gap to the next workgroup of the CU us median %.2f p90 %.2f "
      "| launch span %.1f us = %.2f us per tile and CU" % (len(rec), len(np.unique(rec[:, 2])), tiles, life.min(), np.median(life), np.percentile(life, 90),
                                                          life.max(), np.median(gaps), np.percentile(gaps, 90), span, span / (tiles / max(1, len(np.unique(rec[:, 2]))))))
