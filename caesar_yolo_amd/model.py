"""`YOLO`-compatible detector object backed by the HIP library.

Mirrors the slice of `ultralytics.YOLO` that the reference touches:
  * construction with a weights path            scripts/run.py:347
  * `.names` (dict class id -> label)           caesar_yolo/evaluation.py:46-47, :265
  * `model(image, device=, imgsz=, conf=, iou=, augment=, **ignored)` returning an iterable of results whose
    `.boxes.xyxy / .conf / .cls` support `.cpu().numpy()`      caesar_yolo/evaluation.py:181-193, :261-265
plus the additive batched entry the tile scheduler uses (`detect_tiles`): B same-shape tiles cropped from an
HBM-resident mosaic -> merged detections, everything on device.

PyTorch is used only for device memory and streams; all arithmetic is in libcaesar_yolo_hip.so.  There is no CPU
path: constructing a detector without a visible GPU, or without the built library, raises.
"""
import ctypes as C
import logging
import os
import numpy as np
import torch

from . import lib as L
from . import weights as W


_CPU_WARNED = False


def _dev_index(device):
    if isinstance(device, int):
        return device
    s = str(device)
    if s in ("", "cuda", "gpu"):
        return torch.cuda.current_device()
    if s.startswith("cuda:"):
        return int(s.split(":")[1])
    if s.isdigit():
        return int(s)
    if s == "cpu":
        # The reference's DEFAULT is --devices=cpu (scripts/run.py:130) and Analyzer passes it straight to the model call
        # (caesar_yolo/evaluation.py:183).  This build has no CPU path; raising here would make every tile fail inside the
        # reference's try/except (evaluation.py:194-196) and the run would "succeed" with an empty catalog.  So 'cpu' selects
        # the process's GPU (LOCAL_RANK under torch.distributed, else 0) -- the same rule scripts/run.py applies -- and says so once.
        global _CPU_WARNED
        if not _CPU_WARNED:
            logging.getLogger("caesar_yolo_amd").warning(
                "device='cpu' requested: this build has no CPU path, running on GPU %s instead", os.environ.get("LOCAL_RANK", "0"))
            _CPU_WARNED = True
        return int(os.environ.get("LOCAL_RANK", "0"))
    raise L.CyError("unknown device %r" % (device,))


class HipDetector(object):
    """One library context on one GPU.  Thin, explicit wrappers over the C-ABI stage entry points."""

    def __init__(self, weights_path, device=0, precision="fp16x3", max_batch=64, max_imgsz=640, max_cand=0):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.CyError("no GPU visible: the HIP detector cannot run (no CPU fallback exists)")
        self.device = _dev_index(device)
        self.tdev = torch.device("cuda", self.device)
        if isinstance(precision, str):
            if precision.lower() not in L.PRECISIONS:
                raise L.CyError("unknown precision %r (fp16 | fp16x3 | fp32)" % (precision,))
            precision = L.PRECISIONS[precision.lower()]
        if precision not in (L.F16, L.F32, L.F16X3):
            raise L.CyError("unknown precision %r" % (precision,))
        self.precision = precision
        # dtype of the tensors that cross the C-ABI (network input, conv test entry): fp16 in the fp16 context, fp32 otherwise
        self.dtype = torch.float16 if self.precision == L.F16 else torch.float32
        self.max_batch = int(max_batch)
        m = (int(max_imgsz) + 31) // 32 * 32
        cfg = L.cy_config(self.precision, self.max_batch, m, m, int(max_cand))
        self.ctx = C.c_void_p()
        L.check(self.lib.cy_create(self.device, C.byref(cfg), C.byref(self.ctx)))
        L.check(self.lib.cy_load_weights(self.ctx, os.fsencode(weights_path)), self.ctx)
        nc = self.lib.cy_num_classes(self.ctx)
        self.names = {i: self.lib.cy_class_name(self.ctx, i).decode() for i in range(nc)}
        self.nc = nc
        # pinned staging buffers of the mosaic upload: part of the context (the first pinned allocation of a process costs
        # ~110 ms of runtime initialisation, which belongs here and not in the first image's ingest)
        self._stage = [torch.empty((self.STAGE_BYTES // 4,), dtype=torch.int32, pin_memory=True) for _ in range(2)]

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.cy_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.tdev).cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr())

    def _chk(self, rc):
        return L.check(rc, self.ctx)

    # ---- stages
    def mosaic_to_device(self, data, big_endian=None, file_rows=None):
        """Host fp32 image [H,W] (either byte order) -> resident device mosaic with read_fits value semantics.
        file_rows = (path, byte offset of the first row of `data` in that file): `data` is a run of whole rows of a memory-mapped
        file; a large one is then read with pread() straight into the pinned staging buffers (no page faults on the map)."""
        arr = np.asarray(data)
        if arr.dtype.kind != "f" or arr.dtype.itemsize != 4:
            arr = arr.astype("<f4")
        if big_endian is None:
            big_endian = arr.dtype.byteorder == ">"
        if arr.ndim == 2 and arr.nbytes >= self.STAGED_UPLOAD_MIN_BYTES:
            t = self._staged_upload(arr, file_rows)
        else:
            raw = np.ascontiguousarray(arr).view(np.uint32).view(np.int32)
            t = torch.from_numpy(raw.copy() if not raw.flags.writeable else raw).to(self.tdev).view(torch.float32)
        self._chk(self.lib.cy_mosaic_prepare(self.ctx, self._p(t), t.numel(), int(bool(big_endian)), self._stream()))
        return t

    STAGED_UPLOAD_MIN_BYTES = 64 << 20
    STAGE_BYTES = 32 << 20
    STAGE_THREADS = 4

    def _staged_upload(self, arr, file_rows=None):
        """Large host image (typically a slice of the memory-mapped FITS payload, file byte order) -> device, in row chunks
        through two pinned staging buffers: filling chunk i+1 (several threads: pread() of the file when the rows are whole
        rows of it, else numpy copies out of the map; both release the GIL) runs while chunk i is on the wire."""
        from concurrent.futures import ThreadPoolExecutor
        H, Wd = arr.shape
        fd = os.open(file_rows[0], os.O_RDONLY) if file_rows else -1
        out = torch.empty((H, Wd), dtype=torch.int32, device=self.tdev)
        rows = max(1, min(H, self.STAGE_BYTES // (Wd * 4)))
        if getattr(self, "_stage", None) is None or self._stage[0].numel() < rows * Wd:         # (a single row wider than a buffer)
            self._stage = [torch.empty((rows * Wd,), dtype=torch.int32, pin_memory=True) for _ in range(2)]
        views = [st[:rows * Wd].view(rows, Wd).numpy().view(arr.dtype) for st in self._stage]      # same item size: a raw byte copy
        done = [None, None]
        nthr = self.STAGE_THREADS
        with ThreadPoolExecutor(nthr) as pool:
            for i, y in enumerate(range(0, H, rows)):
                k = i & 1
                if done[k] is not None:
                    done[k].synchronize()                        # the previous transfer out of this buffer has finished
                n = min(rows, H - y)
                cuts = [n * j // nthr for j in range(nthr + 1)]
                if fd >= 0:
                    def fill(j, k=k, y=y, cuts=cuts):
                        if cuts[j + 1] > cuts[j]:
                            buf = memoryview(views[k][cuts[j]:cuts[j + 1]]).cast("B")
                            got = os.preadv(fd, [buf], file_rows[1] + (y + cuts[j]) * Wd * 4)
                            if got != len(buf):
                                raise L.CyError("short read of %s" % (file_rows[0],))
                else:
                    def fill(j, k=k, y=y, cuts=cuts):
                        np.copyto(views[k][cuts[j]:cuts[j + 1]], arr[y + cuts[j]:y + cuts[j + 1]])
                list(pool.map(fill, range(nthr)))
                out[y:y + n].copy_(self._stage[k][:n * Wd].view(n, Wd), non_blocking=True)
                done[k] = torch.cuda.Event()
                done[k].record()
        for e in done:
            if e is not None:
                e.synchronize()
        if fd >= 0:
            os.close(fd)
        return out.view(torch.float32)

    def preproc(self, mosaic, tiles_xy, th, tw, imgsz, cfg):
        B = len(tiles_xy)
        lb = L.letterbox(th, tw, imgsz)
        netin = torch.empty((B, lb.H, lb.W, 4), dtype=self.dtype, device=self.tdev)
        status = torch.empty((B,), dtype=torch.int32, device=self.tdev)
        t = (C.c_int * (2 * B))(*[int(v) for xy in tiles_xy for v in xy])
        self._chk(self.lib.cy_preproc(self.ctx, self._p(mosaic), mosaic.shape[0], mosaic.shape[1], t, B, th, tw, imgsz,
                                      C.byref(cfg), self._p(netin), self._p(status), self._stream()))
        return netin, status, lb

    def preproc_planes(self, mosaic, tiles_xy, th, tw, cfg):
        """-> (float64 [B,3,th,tw] preprocessed images in image channel order, status [B]) on device."""
        B = len(tiles_xy)
        planes = torch.empty((B, 3, th, tw), dtype=torch.float64, device=self.tdev)
        status = torch.empty((B,), dtype=torch.int32, device=self.tdev)
        t = (C.c_int * (2 * B))(*[int(v) for xy in tiles_xy for v in xy])
        self._chk(self.lib.cy_preproc_planes(self.ctx, self._p(mosaic), mosaic.shape[0], mosaic.shape[1], t, B, th, tw,
                                             C.byref(cfg), self._p(planes), self._p(status), self._stream()))
        return planes, status

    def preproc_params(self, B):
        out = np.zeros((B, 3, L.CY_MAX_STAGES, 4), np.float64)
        self._chk(self.lib.cy_preproc_params(self.ctx, out.ctypes.data_as(C.POINTER(C.c_double)), B))
        return out

    def letterbox_pack(self, planes, imgsz):
        """planes: device float64 [B,3,h0,w0] (image channel order, [0,255])."""
        B, _, h0, w0 = planes.shape
        lb = L.letterbox(h0, w0, imgsz)
        netin = torch.empty((B, lb.H, lb.W, 4), dtype=self.dtype, device=self.tdev)
        self._chk(self.lib.cy_letterbox_pack(self.ctx, self._p(planes), B, h0, w0, imgsz, self._p(netin), self._stream()))
        return netin, lb

    def forward(self, netin, out=None):
        """out: the caller's prediction tensor [B, A, 64 + nc] fp32 (e.g. NaN-filled before a stopped pass), else a new one."""
        B, H, Wd, _ = netin.shape
        A = self.lib.cy_num_anchors(H, Wd)
        pred = out if out is not None else torch.empty((B, A, 64 + self.nc), dtype=torch.float32, device=self.tdev)
        assert pred.shape == (B, A, 64 + self.nc) and pred.dtype == torch.float32 and pred.is_contiguous() and pred.device == self.tdev
        self._chk(self.lib.cy_forward(self.ctx, self._p(netin), B, H, Wd, self._p(pred), self._stream()))
        return pred

    def forward_sparse_box(self, netin, conf, out):
        """Test hook (cy_debug_sparse_box): the forward pass with the box branch of the detect head computed only at the anchors
        whose best class score passes `conf`, into the caller's prediction tensor `out` (e.g. NaN-filled).  Returns (out, sparse)
        with sparse[l] = 1 where stride level l was deferred and 0 where its shape kept the dense branch."""
        B, H, Wd, _ = netin.shape
        A = self.lib.cy_num_anchors(H, Wd)
        assert out.shape == (B, A, 64 + self.nc) and out.dtype == torch.float32 and out.is_contiguous() and out.device == self.tdev
        sparse = (C.c_int * 3)()
        self._chk(self.lib.cy_debug_sparse_box(self.ctx, self._p(netin), B, H, Wd, self._p(out), float(conf), sparse, self._stream()))
        return out, [int(v) for v in sparse]

    def weight_passes(self):
        """fp16x3 context: (convolutions on the two-pass form, on the three-pass form); (0, 0) in the other contexts."""
        out = (C.c_int * 2)()
        self._chk(self.lib.cy_weight_passes(self.ctx, out))
        return int(out[0]), int(out[1])

    def profile(self, on):
        self._chk(self.lib.cy_profile_enable(self.ctx, int(on)))            # True/1: every forward call; N > 1: every N-th

    def profile_summary(self, lane=-1):
        """lane: -1 all launches, 0 the main lane of detect_tiles (full batches), 1 its small-batch lane."""
        ent = (L.cy_prof_entry * 32)()
        n = self._chk(self.lib.cy_profile_summary_lane(self.ctx, ent, 32, int(lane)))
        return [dict(kernel=ent[i].kernel.decode(), ms=ent[i].ms, flops=ent[i].flops, launches=ent[i].launches) for i in range(n)]

    def profile_layers(self):
        ent = (L.cy_prof_entry * 256)()
        n = self._chk(self.lib.cy_profile_layers(self.ctx, ent, 256))
        return [dict(name=ent[i].kernel.decode(), ms=ent[i].ms, flops=ent[i].flops, launches=ent[i].launches) for i in range(n)]

    def layer_variant(self, name):
        """Kernel variant of the last timed launch of the named convolution (profile(1) before the forward); '' when the layer
        ran inside a neighbouring layer's kernel."""
        buf = C.create_string_buffer(96)
        self._chk(self.lib.cy_profile_layer_variant(self.ctx, name.encode(), buf, 96))
        return buf.value.decode()

    def read_conv(self, name, shape_hint_elems):
        buf = np.zeros(shape_hint_elems, np.float32)
        dims = (C.c_int * 4)()
        self._chk(self.lib.cy_debug_read_conv(self.ctx, name.encode(), buf.ctypes.data_as(C.POINTER(C.c_float)),
                                              buf.size, dims))
        d = tuple(dims)
        return buf[:int(np.prod(d))].reshape(d)

    def stop_after(self, n_ops):
        """Test hook: the following forward() calls end after the first n_ops plan ops (<= 0: the whole plan again)."""
        self._chk(self.lib.cy_debug_stop_after(self.ctx, int(n_ops)))

    def ops_done(self):
        """Plan ops the last forward() completed (one more than asked for when a two-op launch straddled the stop)."""
        return self._chk(self.lib.cy_debug_ops_done(self.ctx))

    def read_tensor(self, tensor, coff, nch, shape_hint_elems):
        """Channels [coff, coff + nch) of a plan tensor after the last forward() -> float32 [B, nch, h, w]."""
        buf = np.zeros(shape_hint_elems, np.float32)
        dims = (C.c_int * 4)()
        self._chk(self.lib.cy_debug_read_tensor(self.ctx, int(tensor), int(coff), int(nch), buf.ctypes.data_as(C.POINTER(C.c_float)),
                                                buf.size, dims))
        d = tuple(dims)
        return buf[:int(np.prod(d))].reshape(d)

    def lds_fill(self, pattern):
        """Test hook (cy_debug_lds_fill): queue one workgroup per CU on the current stream that writes the 32-bit `pattern` over
        all of its LDS, so that the kernels behind it inherit that pattern.  -> LDS bytes written per workgroup.  Not waited for."""
        return self._chk(self.lib.cy_debug_lds_fill(self.ctx, int(pattern) & 0xFFFFFFFF, self._stream()))

    def _det_out(self, B, out):
        """(det [B,300,6] fp32, index [B,300] int32, count [B] int32): the caller's tensors (out) or zero-filled new ones."""
        if out is not None:
            det, anch, cnt = out
            assert det.shape == (B, L.CY_MAX_DET, 6) and anch.shape == (B, L.CY_MAX_DET) and cnt.shape == (B,)
            assert det.dtype == torch.float32 and anch.dtype == torch.int32 and cnt.dtype == torch.int32
            assert det.is_contiguous() and anch.is_contiguous() and cnt.is_contiguous()
            return det, anch, cnt
        return (torch.zeros((B, L.CY_MAX_DET, 6), dtype=torch.float32, device=self.tdev),
                torch.zeros((B, L.CY_MAX_DET), dtype=torch.int32, device=self.tdev),
                torch.zeros((B,), dtype=torch.int32, device=self.tdev))

    def decode_nms(self, pred, H, Wd, h0, w0, conf, iou, out=None):
        """pred [B, A, 64+nc] fp32 raw head output -> (det, anchor index, count); out: optional (det, index, count) to write."""
        B = pred.shape[0]
        det, anch, cnt = self._det_out(B, out)
        self._chk(self.lib.cy_decode_nms(self.ctx, self._p(pred), B, H, Wd, h0, w0, conf, iou, self._p(det),
                                         self._p(anch), self._p(cnt), self._stream()))
        return det, anch, cnt

    def iou_merge(self, det, cnt, score_thr, soft, hard, out=None):
        """-> (merged det, count, source row); out: optional (det, count, source row) tensors to write."""
        B = det.shape[0]
        if out is not None:
            out, ocnt, osrc = out
            assert out.shape == det.shape and ocnt.shape == (B,) and osrc.shape == (B, L.CY_MAX_DET)
            assert out.dtype == torch.float32 and ocnt.dtype == torch.int32 and osrc.dtype == torch.int32
            assert out.is_contiguous() and ocnt.is_contiguous() and osrc.is_contiguous()
        else:
            out = torch.zeros_like(det)
            ocnt = torch.zeros((B,), dtype=torch.int32, device=self.tdev)
            osrc = torch.zeros((B, L.CY_MAX_DET), dtype=torch.int32, device=self.tdev)
        self._chk(self.lib.cy_iou_merge(self.ctx, self._p(det), self._p(cnt), B, score_thr, soft, hard, self._p(out),
                                        self._p(ocnt), self._p(osrc), self._stream()))
        return out, ocnt, osrc

    def flush(self):
        """Order the current stream behind every batch queued by detect_tiles (they run on internal side streams)."""
        self._chk(self.lib.cy_detect_flush(self.ctx, self._stream()))

    def compact_records(self, gathered, perm, hdr, out):
        """gathered [R, rows, 1803] fp32, perm [T] int64 (row of tile t over all ranks) -> hdr [3T+1] int32, out [T*300*6] fp32 (device)."""
        T = int(perm.shape[0])
        rows = int(gathered.numel() // gathered.shape[-1])
        self._chk(self.lib.cy_compact_records_ctx(self.ctx, self._p(gathered), rows, self._p(perm), T, int(gathered.shape[-1]), self._p(hdr),
                                                  self._p(out), self._stream()))

    def fence(self):
        """Work queued on the current stream since the last detect_tiles call (an upload into a mosaic buffer already in use, a
        memset of an output buffer) is ordered before the next call's internal streams (cy_detect_fence)."""
        self._chk(self.lib.cy_detect_fence(self.ctx, self._stream()))

    def counters(self, reset=False):
        """-> dict(degenerate_boxes, cand_overflow_tiles) accumulated since the last reset (synchronises the device)."""
        out = (C.c_longlong * 4)()
        self._chk(self.lib.cy_detect_counters(self.ctx, out, int(bool(reset))))
        return {"degenerate_boxes": int(out[0]), "cand_overflow_tiles": int(out[1]), "median_bracket_hits": int(out[2]),
                "median_bracket_misses": int(out[3])}

    # ---- measurement steps (an addition to the reference's catalog): helpers shared by the methods below
    def _image_2d(self, img_dev, what):
        if img_dev.dim() != 2 or img_dev.dtype != torch.float32 or not img_dev.is_contiguous() or img_dev.device != self.tdev:
            raise L.CyError("%s: a contiguous 2-D float32 image on %s is required" % (what, self.tdev))
        return int(img_dev.shape[0]), int(img_dev.shape[1])

    @staticmethod
    def _boxes4(boxes):
        return np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 4))

    @staticmethod
    def _mask_layout(boxes, MH, MW):
        """-> (shapes [(h, w)] of the box windows, off int64 [n + 1]: first byte of every window in one buffer of all of them)."""
        from .measure import box_window
        shapes = [box_window(b, MH, MW)[2:] for b in boxes]
        off = np.zeros(len(shapes) + 1, np.int64)
        np.cumsum([h * w for h, w in shapes], out=off[1:])
        return shapes, off

    def _pack_masks(self, what, boxes, masks, MH, MW):
        """The window masks of the boxes in one buffer -> (mask uint8 of at least one byte, off as _mask_layout)."""
        shapes, off = self._mask_layout(boxes, MH, MW)
        for i, ((h, w), m) in enumerate(zip(shapes, masks)):
            if np.asarray(m).size != h * w:
                raise L.CyError("%s: mask %d has %d bytes but the box window %d x %d" % (what, i, np.asarray(m).size, h, w))
        mask = np.zeros(max(int(off[-1]), 1), np.uint8)
        if off[-1]:
            mask[:off[-1]] = np.concatenate([np.asarray(m, np.uint8).reshape(-1) for m in masks])
        return mask, off

    def _kernel_ms(self, fn):
        ms = C.c_double(-1.0)
        self._chk(fn(self.ctx, C.byref(ms)))
        return float(ms.value)

    # ---- catalog source measurement
    def measure_sources(self, img_dev, boxes, ring=8):
        """img_dev: device fp32 image [MH, MW] as mosaic_to_device leaves it; boxes: [n, 4] float64 {x1, y1, x2, y2} in its 0-based
        pixels (they may leave the image).  -> numpy float64 [n, CY_MEAS_FIELDS] (lib.MEAS_NAMES), cy_measure_sources."""
        boxes = self._boxes4(boxes)
        n = boxes.shape[0]
        out = np.zeros((n, L.CY_MEAS_FIELDS), np.float64)
        MH, MW = self._image_2d(img_dev, "measure_sources")
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.cy_measure_sources(self.ctx, self._p(img_dev), MH, MW, boxes.ctypes.data_as(dp), n, int(ring),
                                              out.ctypes.data_as(dp), self._stream()))
        return out

    def measure_kernel_ms(self):
        """Kernel time of the last measure_sources call in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_measure_kernel_ms)

    # ---- source islands (the second measurement step)
    def measure_islands(self, img_dev, boxes, thr, conn=8, return_masks=False):
        """Seed / merge-threshold islands of the box windows (cy_measure_islands).  img_dev, boxes: as measure_sources; thr: [n, 3]
        float64 {seed_thr, merge_thr, bkg} per source.  -> numpy float64 [n, CY_ISL_FIELDS] (lib.ISL_NAMES); with return_masks
        also a list of n uint8 arrays shaped like the box windows (0 outside the island set, 1 in it, 2 in the main island; an
        empty window gives an array of shape (0, 0))."""
        boxes = self._boxes4(boxes)
        thr = np.ascontiguousarray(np.asarray(thr, np.float64).reshape(-1, 3))
        n = boxes.shape[0]
        if thr.shape[0] != n:
            raise L.CyError("measure_islands: %d boxes but %d threshold rows" % (n, thr.shape[0]))
        out = np.zeros((n, L.CY_ISL_FIELDS), np.float64)
        MH, MW = self._image_2d(img_dev, "measure_islands")
        masks = self._island_call(self.lib.cy_measure_islands, img_dev, MH, MW, boxes, thr, (int(conn),), (out,), return_masks)
        return (out, masks) if return_masks else out

    def _island_call(self, entry, img_dev, MH, MW, boxes, thr, params, outs, return_masks):
        """cy_measure_islands / cy_deblend_islands: (.., boxes, thr, n, *params, *outs, mask, mask offsets, stream).  -> the window
        masks, or None when they are not wanted."""
        dp = C.POINTER(C.c_double)
        mask = off = None
        if return_masks:
            shapes, off = self._mask_layout(boxes, MH, MW)
            mask = np.zeros(max(int(off[-1]), 1), np.uint8)
        self._chk(entry(self.ctx, self._p(img_dev), MH, MW, boxes.ctypes.data_as(dp), thr.ctypes.data_as(dp), boxes.shape[0], *params,
                        *[o.ctypes.data_as(dp) for o in outs], C.c_void_p(mask.ctypes.data) if return_masks else None,
                        off.ctypes.data_as(C.POINTER(C.c_longlong)) if return_masks else None, self._stream()))
        if return_masks:
            return [mask[off[i]:off[i + 1]].reshape(shapes[i]) for i in range(boxes.shape[0])]

    def islands_kernel_ms(self):
        """Kernel time of the last measure_islands call in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_islands_kernel_ms)

    # ---- source components (the fourth measurement step)
    def deblend_islands(self, img_dev, boxes, thr4, conn=8, radius=2, return_masks=False):
        """Components of the island set of every box window by local peaks and steepest-ascent basins (cy_deblend_islands).
        img_dev, boxes: as measure_sources; thr4: [n, 4] float64 {seed_thr, merge_thr, bkg, peak_thr} per source.  -> (rows numpy
        float64 [n, CY_DBL_FIELDS] (lib.DBL_NAMES), component rows [n, CY_DBL_MAX_COMP, CY_DBL_COMP_FIELDS] (lib.DBL_COMP_NAMES));
        with return_masks also a list of n uint8 arrays shaped like the box windows (0 outside the island set, k + 1 component k,
        255 unassigned; an empty window gives an array of shape (0, 0))."""
        boxes = self._boxes4(boxes)
        thr4 = np.ascontiguousarray(np.asarray(thr4, np.float64).reshape(-1, 4))
        n = boxes.shape[0]
        if thr4.shape[0] != n:
            raise L.CyError("deblend_islands: %d boxes but %d threshold rows" % (n, thr4.shape[0]))
        out = np.zeros((n, L.CY_DBL_FIELDS), np.float64)
        comp = np.zeros((n, L.CY_DBL_MAX_COMP, L.CY_DBL_COMP_FIELDS), np.float64)
        MH, MW = self._image_2d(img_dev, "deblend_islands")
        masks = self._island_call(self.lib.cy_deblend_islands, img_dev, MH, MW, boxes, thr4, (int(conn), int(radius)), (out, comp), return_masks)
        return (out, comp, masks) if return_masks else (out, comp)

    def deblend_kernel_ms(self):
        """Kernel time of the last deblend_islands call in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_deblend_kernel_ms)

    # ---- component fits (the fifth measurement step) and joint fits of blends (the sixth)
    def _fit_call(self, what, entry, fields, img_dev, boxes, bkg, ncomp, start, masks, max_iter):
        """cy_fit_components / cy_fit_blends, which take the same arguments.  -> numpy float64 [n, CY_DBL_MAX_COMP, fields]."""
        boxes = self._boxes4(boxes)
        n = boxes.shape[0]
        bkg = np.ascontiguousarray(np.asarray(bkg, np.float64).reshape(-1))
        ncomp = np.ascontiguousarray(np.asarray(ncomp).reshape(-1).astype(np.int32))
        start = np.ascontiguousarray(np.asarray(start, np.float64).reshape(-1, L.CY_DBL_MAX_COMP, 6))
        if bkg.shape[0] != n or ncomp.shape[0] != n or start.shape[0] != n or len(masks) != n:
            raise L.CyError("%s: %d boxes but %d bkg, %d ncomp, %d start rows and %d masks" % (
                what, n, bkg.shape[0], ncomp.shape[0], start.shape[0], len(masks)))
        if not 1 <= int(max_iter) <= 256:
            raise L.CyError("%s: max_iter must be in [1, 256]" % what)
        MH, MW = self._image_2d(img_dev, what)
        out = np.zeros((n, L.CY_DBL_MAX_COMP, fields), np.float64)
        if n == 0:
            return out
        mask, off = self._pack_masks(what, boxes, masks, MH, MW)
        dp = C.POINTER(C.c_double)
        self._chk(entry(self.ctx, self._p(img_dev), MH, MW, boxes.ctypes.data_as(dp), bkg.ctypes.data_as(dp),
                        ncomp.ctypes.data_as(C.POINTER(C.c_int)), start.ctypes.data_as(dp), n, int(max_iter),
                        C.c_void_p(mask.ctypes.data), off.ctypes.data_as(C.POINTER(C.c_longlong)), out.ctypes.data_as(dp), self._stream()))
        return out

    def fit_components(self, img_dev, boxes, bkg, ncomp, start, masks, max_iter=64):
        """One elliptical Gaussian per component by Levenberg-Marquardt (cy_fit_components).  img_dev, boxes: as measure_sources;
        bkg: [n] float64; ncomp: [n] components per source (0 .. CY_DBL_MAX_COMP); start: [n, CY_DBL_MAX_COMP, 6] float64
        {A, x0, y0, a, b, c} with x0, y0 in image pixels (measure.fit_start); masks: the n uint8 arrays deblend_islands returns
        with return_masks (shaped like the box windows: byte k + 1 = component k).  -> numpy float64
        [n, CY_DBL_MAX_COMP, CY_FIT_FIELDS] (lib.FIT_NAMES); rows at and beyond ncomp are 0."""
        return self._fit_call("fit_components", self.lib.cy_fit_components, L.CY_FIT_FIELDS, img_dev, boxes, bkg, ncomp, start, masks, max_iter)

    def fit_kernel_ms(self):
        """Kernel time of the last fit_components call that launched a kernel, in ms (hipEvents around the launch); -1 before it."""
        return self._kernel_ms(self.lib.cy_fit_kernel_ms)

    def fit_blends(self, img_dev, boxes, bkg, ncomp, start, masks, max_iter=64):
        """The sum of the Gaussians of every group of touching components fitted jointly by Levenberg-Marquardt (cy_fit_blends).
        Arguments as fit_components; start: one start per component, for instance measure.blend_start().  -> numpy float64
        [n, CY_DBL_MAX_COMP, CY_BLEND_FIELDS] (lib.BLEND_NAMES); rows at and beyond ncomp are 0."""
        return self._fit_call("fit_blends", self.lib.cy_fit_blends, L.CY_BLEND_FIELDS, img_dev, boxes, bkg, ncomp, start, masks, max_iter)

    def blend_kernel_ms(self):
        """Kernel time of the last fit_blends call that launched a kernel, in ms (hipEvents around the launch); -1 before it."""
        return self._kernel_ms(self.lib.cy_blend_kernel_ms)

    # ---- model and residual maps (the seventh measurement step)
    def render_gaussians(self, img_dev, comp, nsigma=5.0, bkg_dev=None, want=("model", "resid"), signed=False):
        """The sum of the Gaussians comp [m, 6] float64 {A, x0, y0, a, b, c} (x0, y0 in image pixels) over the whole image, each
        inside its support rectangle of nsigma marginal sigmas (cy_render_gaussians).  img_dev: as measure_sources; bkg_dev: a
        device fp32 map of its shape, or None (0).  -> (rows numpy float64 [m, CY_RND_FIELDS] (lib.RND_NAMES), model, resid): the two
        device fp32 maps [MH, MW]; one not named in `want` is None.  signed: amplitudes of either sign are rendered
        (cy_render_signed_gaussians: A != 0 in place of A > 0), as the second residual needs them for fitted holes."""
        MH, MW = self._image_2d(img_dev, "render_gaussians")
        comp = np.ascontiguousarray(np.asarray(comp, np.float64).reshape(-1, 6))
        m = comp.shape[0]
        if bkg_dev is not None and (bkg_dev.shape != img_dev.shape or self._image_2d(bkg_dev, "render_gaussians (bkg_dev)") != (MH, MW)):
            raise L.CyError("render_gaussians: bkg_dev must have the shape of the image")
        rows = np.zeros((m, L.CY_RND_FIELDS), np.float64)
        maps = [torch.empty((MH, MW), dtype=torch.float32, device=self.tdev) if n in want else None for n in ("model", "resid")]
        dp = C.POINTER(C.c_double)
        entry = self.lib.cy_render_signed_gaussians if signed else self.lib.cy_render_gaussians
        self._chk(entry(self.ctx, self._p(img_dev), MH, MW, comp.ctypes.data_as(dp) if m else None, m, float(nsigma),
                        self._p(bkg_dev) if bkg_dev is not None else None, *[self._p(t) if t is not None else None for t in maps],
                        rows.ctypes.data_as(dp) if m else None, self._stream()))
        return rows, maps[0], maps[1]

    def render_kernel_ms(self):
        """Kernel time of the last render_gaussians call in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_render_kernel_ms)

    def measure_residuals(self, img_dev, model_dev, boxes, bkg, masks):
        """The residual ((v - bkg) - model) of every box window and of its island set (cy_measure_residuals).  img_dev, boxes: as
        measure_sources; model_dev: the model map render_gaussians returns; bkg: [n] float64; masks: the n uint8 arrays
        deblend_islands returns with return_masks (non-zero: in the island set).  -> numpy float64 [n, CY_RES_FIELDS]
        (lib.RES_NAMES)."""
        boxes = self._boxes4(boxes)
        n = boxes.shape[0]
        bkg = np.ascontiguousarray(np.asarray(bkg, np.float64).reshape(-1))
        if bkg.shape[0] != n or len(masks) != n:
            raise L.CyError("measure_residuals: %d boxes but %d bkg and %d masks" % (n, bkg.shape[0], len(masks)))
        MH, MW = self._image_2d(img_dev, "measure_residuals")
        if self._image_2d(model_dev, "measure_residuals (model_dev)") != (MH, MW):
            raise L.CyError("measure_residuals: model_dev must have the shape of the image")
        out = np.zeros((n, L.CY_RES_FIELDS), np.float64)
        if n == 0:
            return out
        mask, off = self._pack_masks("measure_residuals", boxes, masks, MH, MW)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.cy_measure_residuals(self.ctx, self._p(img_dev), self._p(model_dev), MH, MW, boxes.ctypes.data_as(dp),
                                                bkg.ctypes.data_as(dp), n, C.c_void_p(mask.ctypes.data),
                                                off.ctypes.data_as(C.POINTER(C.c_longlong)), out.ctypes.data_as(dp), self._stream()))
        return out

    def residual_kernel_ms(self):
        """Kernel time of the last measure_residuals call in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_residual_kernel_ms)

    # ---- residual peaks (after the seventh measurement step)
    def find_peaks(self, map_dev, rms_dev, k_sigma=5.0, radius=2, sign=1, cap=65536):
        """The local maxima of sign * map_dev over (2 radius + 1)^2 neighbourhoods that lie at or above k_sigma * rms_dev
        (cy_find_peaks).  map_dev, rms_dev: contiguous 2-D float32 device maps of one shape: the residual map of render_gaussians and
        the rms map of expand_background.  -> (rows numpy float64 [min(total, cap), CY_PEAK_FIELDS] (lib.PEAK_NAMES) in increasing
        (y, x), total: the number of peaks of the whole image)."""
        MH, MW = self._image_2d(map_dev, "find_peaks")
        if rms_dev.shape != map_dev.shape or self._image_2d(rms_dev, "find_peaks (rms_dev)") != (MH, MW):
            raise L.CyError("find_peaks: rms_dev must have the shape of the map")
        cap = int(cap)
        rows = np.zeros((max(cap, 0), L.CY_PEAK_FIELDS), np.float64)
        total = C.c_longlong(0)
        self._chk(self.lib.cy_find_peaks(self.ctx, self._p(map_dev), self._p(rms_dev), MH, MW, float(k_sigma), int(radius), int(sign), cap,
                                         rows.ctypes.data_as(C.POINTER(C.c_double)) if cap > 0 else None, C.byref(total), self._stream()))
        total = int(total.value)
        return rows[:min(total, cap)].copy(), total

    def peaks_kernel_ms(self):
        """Kernel time of the last find_peaks call in ms (hipEvents around its launches); -1 before the first."""
        return self._kernel_ms(self.lib.cy_peaks_kernel_ms)

    # ---- a trous wavelet levels (the multi-scale search of the residual map)
    def atrous_step(self, in_dev, step, want=("smooth", "detail"), out=(None, None)):
        """One level of the a trous (B3-spline) decomposition of in_dev, a contiguous 2-D float32 device map, with the taps `step`
        pixels apart (cy_atrous_step).  -> (smooth, detail): two device fp32 maps of its shape, detail = in - smooth; one not named
        in `want` is None.  out: (smooth, detail) maps to write into instead of new ones (None: a new one); neither may overlap
        in_dev or the other."""
        MH, MW = self._image_2d(in_dev, "atrous_step")
        if not set(want) & {"smooth", "detail"}:
            raise L.CyError("atrous_step: at least one of smooth and detail is required")
        maps = []
        for name, o in zip(("smooth", "detail"), out):
            if name not in want:
                o = None
            elif o is None:
                o = torch.empty((MH, MW), dtype=torch.float32, device=self.tdev)
            elif o.shape != in_dev.shape or self._image_2d(o, "atrous_step (out)") != (MH, MW):
                raise L.CyError("atrous_step: an output map must have the shape of the input")
            maps.append(o)
        self._chk(self.lib.cy_atrous_step(self.ctx, self._p(in_dev), MH, MW, int(step),
                                          *[self._p(m) if m is not None else None for m in maps], self._stream()))
        return maps[0], maps[1]

    def atrous_kernel_ms(self):
        """Kernel time of the last atrous_step call in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_atrous_kernel_ms)

    # ---- aperture sums at given positions (the curve of growth of the peak lists)
    def aperture_sums(self, map_dev, rms_dev, jobs, factors):
        """Concentric circular apertures at given positions on map_dev (cy_aperture_sums).  map_dev: a contiguous 2-D float32 device
        map, the residual map of render_gaussians; rms_dev: the rms map of its shape, or None; jobs: [n, 3] float64 (cx, cy, unit)
        in the pixels of map_dev; factors: the K <= CY_APER_RINGS_MAX strictly increasing radii in units of `unit`, the last one the
        outer edge of the background annulus.  -> numpy float64 [n, CY_APER_FIELDS]: lib.APER_NAMES, then lib.APER_RING_NAMES per
        ring."""
        MH, MW = self._image_2d(map_dev, "aperture_sums")
        if rms_dev is not None and (rms_dev.shape != map_dev.shape or self._image_2d(rms_dev, "aperture_sums (rms_dev)") != (MH, MW)):
            raise L.CyError("aperture_sums: rms_dev must have the shape of the map")
        jobs = np.ascontiguousarray(np.asarray(jobs, np.float64).reshape(-1, 3))
        factors = np.ascontiguousarray(np.asarray(factors, np.float64).reshape(-1))
        n = jobs.shape[0]
        out = np.zeros((n, L.CY_APER_FIELDS), np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.cy_aperture_sums(self.ctx, self._p(map_dev), self._p(rms_dev) if rms_dev is not None else None, MH, MW,
                                            jobs.ctypes.data_as(dp), n, factors.ctypes.data_as(dp), int(factors.shape[0]),
                                            out.ctypes.data_as(dp), self._stream()))
        return out

    def aperture_kernel_ms(self):
        """Kernel time of the last aperture_sums call that launched in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_aperture_kernel_ms)

    # ---- Gaussian fits at given positions (a shape for every entry of the peak lists)
    def fit_peaks(self, map_dev, jobs, max_iter=64):
        """One elliptical Gaussian per job on the pixels of a disc around a given position of map_dev (cy_fit_peaks).  map_dev: a
        contiguous 2-D float32 device map, the residual map of render_gaussians; jobs: [n, CY_PFIT_JOB_FIELDS] float64
        (lib.PFIT_JOB_NAMES): the centre and radius of the disc, the background, the sign (-1 fits a hole) and the start, all
        positions in the pixels of map_dev.  -> numpy float64 [n, CY_PFIT_FIELDS] (lib.PFIT_NAMES)."""
        MH, MW = self._image_2d(map_dev, "fit_peaks")
        jobs = np.ascontiguousarray(np.asarray(jobs, np.float64).reshape(-1, L.CY_PFIT_JOB_FIELDS))
        n = jobs.shape[0]
        out = np.zeros((n, L.CY_PFIT_FIELDS), np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.cy_fit_peaks(self.ctx, self._p(map_dev), MH, MW, jobs.ctypes.data_as(dp), n, int(max_iter),
                                        out.ctypes.data_as(dp), self._stream()))
        return out

    def peakfit_kernel_ms(self):
        """Kernel time of the last fit_peaks call that launched in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_peakfit_kernel_ms)

    # ---- joint fits of groups of peaks (neighbouring entries of a peak list fitted together)
    def fit_peak_groups(self, map_dev, jobs, link=1.5, max_iter=64):
        """The sum of 2 .. CY_BLEND_MAX_MEMBERS elliptical Gaussians per group of linked jobs on the union of their discs
        (cy_fit_peak_groups).  map_dev and jobs as fit_peaks, the starts usually that call's results; two jobs of equal sign are
        linked when their centres are closer than link times the larger of their radii.  -> numpy float64 [n, CY_PGRP_FIELDS]
        (lib.PGRP_NAMES), one row per job."""
        MH, MW = self._image_2d(map_dev, "fit_peak_groups")
        jobs = np.ascontiguousarray(np.asarray(jobs, np.float64).reshape(-1, L.CY_PFIT_JOB_FIELDS))
        n = jobs.shape[0]
        out = np.zeros((n, L.CY_PGRP_FIELDS), np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.cy_fit_peak_groups(self.ctx, self._p(map_dev), MH, MW, jobs.ctypes.data_as(dp), n, float(link), int(max_iter),
                                              out.ctypes.data_as(dp), self._stream()))
        return out

    def peakgroup_kernel_ms(self):
        """Kernel time of the last fit_peak_groups call that launched in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_peakgroup_kernel_ms)

    # ---- residuals on the discs of given jobs (what the second residual holds where a peak was fitted)
    def disc_residuals(self, map_dev, model_dev, jobs):
        """Count, sum, sum of squares and largest |v - bkg| of map_dev on the pixel set of every job, and the sum of model_dev over
        the same pixels (cy_disc_residuals).  map_dev: a contiguous 2-D float32 device map, the second residual of
        measure.Chain.subtract(); model_dev: a map of its shape (the peak model), or None; jobs: [n, CY_PFIT_JOB_FIELDS] float64 as
        fit_peaks takes them (the start is ignored).  -> numpy float64 [n, CY_DRES_FIELDS] (lib.DRES_NAMES)."""
        MH, MW = self._image_2d(map_dev, "disc_residuals")
        if model_dev is not None and (model_dev.shape != map_dev.shape or self._image_2d(model_dev, "disc_residuals (model_dev)") != (MH, MW)):
            raise L.CyError("disc_residuals: model_dev must have the shape of the map")
        jobs = np.ascontiguousarray(np.asarray(jobs, np.float64).reshape(-1, L.CY_PFIT_JOB_FIELDS))
        n = jobs.shape[0]
        out = np.zeros((n, L.CY_DRES_FIELDS), np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.cy_disc_residuals(self.ctx, self._p(map_dev), self._p(model_dev) if model_dev is not None else None, MH, MW,
                                             jobs.ctypes.data_as(dp), n, out.ctypes.data_as(dp), self._stream()))
        return out

    def disc_residual_kernel_ms(self):
        """Kernel time of the last disc_residuals call that launched in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_disc_residual_kernel_ms)

    # ---- forced photometry (the amplitudes of fixed shapes on any map)
    def forced_fit(self, map_dev, rms_dev, jobs, nsigma=3.0, fit_bkg=True):
        """The amplitude of a Gaussian of fixed position and shape per job on map_dev, solved together with its overlapping
        neighbours' and a local constant (cy_forced_fit).  map_dev: a contiguous 2-D float32 device map; rms_dev: a noise map of its
        shape, or None (unit weights); jobs: [n, CY_FORCED_JOB_FIELDS] float64 (lib.FORCED_JOB_NAMES), positions in the pixels of
        map_dev.  -> numpy float64 [n, CY_FORCED_FIELDS] (lib.FORCED_NAMES)."""
        MH, MW = self._image_2d(map_dev, "forced_fit")
        if rms_dev is not None and (rms_dev.shape != map_dev.shape or self._image_2d(rms_dev, "forced_fit (rms_dev)") != (MH, MW)):
            raise L.CyError("forced_fit: rms_dev must have the shape of the map")
        jobs = np.ascontiguousarray(np.asarray(jobs, np.float64).reshape(-1, L.CY_FORCED_JOB_FIELDS))
        n = jobs.shape[0]
        out = np.zeros((n, L.CY_FORCED_FIELDS), np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.cy_forced_fit(self.ctx, self._p(map_dev), self._p(rms_dev) if rms_dev is not None else None, MH, MW,
                                         jobs.ctypes.data_as(dp), n, float(nsigma), int(bool(fit_bkg)), out.ctypes.data_as(dp), self._stream()))
        return out

    def forced_kernel_ms(self):
        """Kernel time of the last forced_fit call that launched in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_forced_kernel_ms)

    # ---- background and noise mesh (the global noise map of the measurement steps)
    def measure_background(self, img_dev, cell=128, k=3.0, niter=3):
        """Clipped median / MAD of every cell of the mesh over img_dev (as measure_sources takes it), cy_measure_background.
        -> numpy float64 [ncy, ncx, CY_BKG_FIELDS] (lib.BKG_NAMES), ncy = ceil(MH / cell), ncx = ceil(MW / cell)."""
        MH, MW = self._image_2d(img_dev, "measure_background")
        cell = int(cell)
        if cell < 1:
            raise L.CyError("measure_background: cell must be in [4, 4096]")
        out = np.zeros((-(-MH // cell), -(-MW // cell), L.CY_BKG_FIELDS), np.float64)
        self._chk(self.lib.cy_measure_background(self.ctx, self._p(img_dev), MH, MW, cell, float(k), int(niter),
                                                 out.ctypes.data_as(C.POINTER(C.c_double)), self._stream()))
        return out

    def background_kernel_ms(self):
        """Kernel time of the last measure_background call in ms (hipEvents around the launch); -1 before the first."""
        return self._kernel_ms(self.lib.cy_background_kernel_ms)

    def expand_background(self, mesh, cell, shape, want=("bkg", "rms")):
        """mesh: filled [ncy, ncx, 2] float64 {bkg, rms} (measure.fill_mesh); shape = (MH, MW).  -> (bkg, rms) device fp32 maps
        [MH, MW], bilinear between the cell centres (cy_expand_background; measure.sample_mesh at every pixel, rounded to fp32);
        a map not named in `want` is None."""
        mesh = np.ascontiguousarray(np.asarray(mesh, np.float64))
        if mesh.ndim != 3 or mesh.shape[2] != 2:
            raise L.CyError("expand_background: a [ncy, ncx, 2] mesh is required")
        MH, MW = int(shape[0]), int(shape[1])
        if MH <= 0 or MW <= 0 or not want:
            raise L.CyError("expand_background: a non-empty image shape and at least one map are required")
        maps = [torch.empty((MH, MW), dtype=torch.float32, device=self.tdev) if n in want else None for n in ("bkg", "rms")]
        self._chk(self.lib.cy_expand_background(self.ctx, mesh.ctypes.data_as(C.POINTER(C.c_double)), int(mesh.shape[0]), int(mesh.shape[1]),
                                                int(cell), MH, MW, *[self._p(m) if m is not None else None for m in maps], self._stream()))
        return tuple(maps)

    # ---- test-time augmentation (ultralytics `augment=True`): views 1 (0.83, flipped) and 2 (0.67) beside view 0
    def enable_augment(self):
        """Allocate the context's view buffers (cy_enable_augment; once, on the first augmented call)."""
        if not getattr(self, "_aug", False):
            self._chk(self.lib.cy_enable_augment(self.ctx))
            self._aug = True

    def letterbox_pack_f32(self, planes, imgsz):
        """letterbox_pack into an fp32 canvas whatever the context precision (the views' source)."""
        B, _, h0, w0 = planes.shape
        lb = L.letterbox(h0, w0, imgsz)
        out = torch.empty((B, lb.H, lb.W, 4), dtype=torch.float32, device=self.tdev)
        self._chk(self.lib.cy_letterbox_pack_f32(self.ctx, self._p(planes), B, h0, w0, imgsz, self._p(out), self._stream()))
        return out, lb

    def augment_pack(self, src):
        """View kernel: src fp32 [B,H,W,4] letterboxed -> [view 0, view 1, view 2] network inputs of the context dtype (view 0 is src
        itself in the fp32 / fp16x3 contexts, its fp16 copy in the fp16 context)."""
        self.enable_augment()
        B, H, Wd, _ = src.shape
        views, _ = L.augment_geometry(H, Wd)
        outs = [torch.empty((B, v["Hp"], v["Wp"], 4), dtype=self.dtype, device=self.tdev) for v in views]
        if self.precision != L.F16:
            outs[0] = src
        self._chk(self.lib.cy_augment_pack(self.ctx, self._p(src), B, H, Wd, self._p(outs[0]) if self.precision == L.F16 else None,
                                           self._p(outs[1]), self._p(outs[2]), self._stream()))
        return outs

    def decode_nms_augmented(self, preds, H, Wd, h0, w0, conf, iou, out=None):
        """preds: the three views' raw head outputs (forward()); H, Wd: view 0.  -> (det, concatenated index, count) as decode_nms."""
        self.enable_augment()
        B = preds[0].shape[0]
        det, anch, cnt = self._det_out(B, out)
        self._chk(self.lib.cy_decode_nms_augmented(self.ctx, self._p(preds[0]), self._p(preds[1]), self._p(preds[2]), B, H, Wd, h0, w0,
                                                   conf, iou, self._p(det), self._p(anch), self._p(cnt), self._stream()))
        return det, anch, cnt

    def detect_tiles(self, mosaic, tiles_xy, th, tw, imgsz, cfg, conf, iou, soft, hard, out=None, flush=True, augment=False):
        """Whole per-tile path for B same-shape tiles.  Returns (det [B,300,6], count [B], status [B]) on device.
        With flush=False consecutive calls overlap (give each its own `out` buffers and call flush() before reading).
        augment=True: ultralytics' test-time augmentation (three views per tile, cy_detect_tiles_augmented)."""
        B = len(tiles_xy)
        if out is None:
            det = torch.empty((B, L.CY_MAX_DET, 6), dtype=torch.float32, device=self.tdev)
            cnt = torch.empty((B,), dtype=torch.int32, device=self.tdev)
            status = torch.empty((B,), dtype=torch.int32, device=self.tdev)
        else:
            det, cnt, status = out
        t = (C.c_int * (2 * B))(*[int(v) for xy in tiles_xy for v in xy])
        if augment:
            self.enable_augment()
            self._chk(self.lib.cy_detect_tiles_augmented(self.ctx, self._p(mosaic), mosaic.shape[0], mosaic.shape[1], t, B, th, tw,
                                                         imgsz, C.byref(cfg), conf, iou, soft, hard, 1, self._p(det), self._p(cnt),
                                                         self._p(status), self._stream()))
        else:
            self._chk(self.lib.cy_detect_tiles(self.ctx, self._p(mosaic), mosaic.shape[0], mosaic.shape[1], t, B, th, tw,
                                               imgsz, C.byref(cfg), conf, iou, soft, hard, self._p(det), self._p(cnt),
                                               self._p(status), self._stream()))
        if flush:
            self.flush()
        return det, cnt, status

    def bottleneck64(self, x_nhwc, w1, b1, w2, b2, shortcut=True):
        """Fused 64-channel Bottleneck (kernel-level test entry): x [B,H,W,64] fp16 -> [B,H,W,64]."""
        B, H, Wd, Cin = x_nhwc.shape
        out = torch.empty_like(x_nhwc)
        arrs = [np.ascontiguousarray(v, np.float32) for v in (w1, b1, w2, b2)]
        ptr = [v.ctypes.data_as(C.POINTER(C.c_float)) for v in arrs]
        self._chk(self.lib.cy_bottleneck64(self.ctx, self._p(x_nhwc), B, H, Wd, ptr[0], ptr[1], ptr[2], ptr[3], int(bool(shortcut)),
                                           self._p(out), self._stream()))
        return out

    def conv_bn_silu(self, x_nhwc, w, b, k, s, act=True, res=None):
        B, Hi, Wi, Cin = x_nhwc.shape
        Cout = w.shape[0]
        pad = k // 2
        Ho, Wo = (Hi + 2 * pad - k) // s + 1, (Wi + 2 * pad - k) // s + 1
        out = torch.empty((B, Ho, Wo, Cout), dtype=self.dtype, device=self.tdev)
        w = np.ascontiguousarray(w, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        self._chk(self.lib.cy_conv_bn_silu(self.ctx, self._p(x_nhwc), B, Hi, Wi, Cin,
                                           w.ctypes.data_as(C.POINTER(C.c_float)), b.ctypes.data_as(C.POINTER(C.c_float)),
                                           Cout, k, s, int(act), self._p(res) if res is not None else None,
                                           self._p(out), self._stream()))
        return out

    def conv_slices(self, w, b, k, s, act, in0, c0, out, in0_coff=0, up0=False, in1=None, in1_coff=0, c1=0, res=None, res_coff=0,
                    out_coff=0, rows=None):
        """One convolution in the forward's layout (cy_conv_slices): in0 [B,H0,W0,in0_ct] (H0 = Hi / 2 with up0), in1
        [B,Hi,Wi,in1_ct], res [B,Ho,Wo,res_ct] (may be `out`), out [B,Ho,Wo,out_ct] written in place in its slice, or with
        rows = out_ro the fp32 prediction rows [B,out_bs,out_ct].  -> (variant name, fp16x3 pass count)."""
        B = in0.shape[0]
        Hi, Wi = (in1.shape[1], in1.shape[2]) if in1 is not None else (in0.shape[1] << int(bool(up0)), in0.shape[2] << int(bool(up0)))
        w = np.ascontiguousarray(w, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        a = L.cy_conv_layout()
        a.d_in0, a.in0_ct, a.in0_coff, a.c0, a.up0 = in0.data_ptr(), in0.shape[-1], int(in0_coff), int(c0), int(bool(up0))
        if in1 is not None:
            a.d_in1, a.in1_ct, a.in1_coff, a.c1 = in1.data_ptr(), in1.shape[-1], int(in1_coff), int(c1)
        if res is not None:
            a.d_res, a.res_ct, a.res_coff = res.data_ptr(), res.shape[-1], int(res_coff)
        a.d_out, a.out_ct, a.out_coff = out.data_ptr(), out.shape[-1], int(out_coff)
        if rows is not None:
            a.rows, a.out_bs, a.out_ro = 1, out.shape[1], int(rows)
        a.B, a.Hi, a.Wi, a.Cin, a.Cout, a.k, a.s, a.act = B, Hi, Wi, w.shape[1], w.shape[0], int(k), int(s), int(bool(act))
        name = C.create_string_buffer(128)
        passes = C.c_int(0)
        self._chk(self.lib.cy_conv_slices(self.ctx, C.byref(a), w.ctypes.data_as(C.POINTER(C.c_float)),
                                          b.ctypes.data_as(C.POINTER(C.c_float)), name, 128, C.byref(passes), self._stream()))
        return name.value.decode(), passes.value

    # kernel-level test entries of the YOLO11 / SPPF operators: NHWC tensors [B,H,W,ct] of the context dtype, the op on channel
    # slices of them (the forward's layout); the output tensor is written in place (channels outside its slice untouched)
    def dwconv3x3(self, x, nch, w, b, out, in_coff=0, out_coff=0, act=True, res=None, res_coff=0, chmap=(0, 0, 0)):
        """Depth-wise 3x3 (+SiLU)(+residual): out[..., out_coff:out_coff+nch] from x through chmap = (blk, gstride, goff)
        (blk = 0: input channel in_coff + c); w [C,1,3,3], b [C]."""
        B, H, Wd, in_ct = x.shape
        w = np.ascontiguousarray(w, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        self._chk(self.lib.cy_dwconv3x3(self.ctx, self._p(x), B, H, Wd, int(nch), in_ct, int(in_coff),
                                        w.ctypes.data_as(C.POINTER(C.c_float)), b.ctypes.data_as(C.POINTER(C.c_float)),
                                        int(bool(act)), int(chmap[0]), int(chmap[1]), int(chmap[2]),
                                        self._p(res) if res is not None else None, res.shape[-1] if res is not None else 0,
                                        int(res_coff), self._p(out), out.shape[-1], int(out_coff), self._stream()))
        return out

    def attention(self, qkv, heads, kd, hd, out, coff=0, out_coff=0):
        """C2PSA attention core: qkv [B,N,ct] with per-head [q kd | k kd | v hd] blocks from channel coff on -> out[..., out_coff:]."""
        B, N, ct = qkv.shape
        self._chk(self.lib.cy_attention(self.ctx, self._p(qkv), B, N, ct, int(coff), int(heads), int(kd), int(hd), self._p(out),
                                        out.shape[-1], int(out_coff), self._stream()))
        return out

    def maxpool5(self, src, nch, dst, src_coff=0, dst_coff=0):
        """MaxPool2d(5, 1, 2) of src[..., src_coff:src_coff+nch] into dst[..., dst_coff:]; dst may be src (SPPF, disjoint slices)."""
        B, H, Wd, ct = src.shape
        assert tuple(dst.shape) == tuple(src.shape)
        self._chk(self.lib.cy_maxpool5(self.ctx, self._p(src), B, H, Wd, int(nch), ct, int(src_coff), self._p(dst), int(dst_coff),
                                       self._stream()))
        return dst


class _Boxes(object):
    def __init__(self, det):
        self.xyxy, self.conf, self.cls = det[:, :4], det[:, 4], det[:, 5]


class Results(object):
    def __init__(self, det):
        self.boxes = _Boxes(det)


class YOLO(object):
    """Drop-in for `ultralytics.YOLO(weights)` on the reference's detect path.

    `weights` is a CYW1 file (caesar_yolo_amd.weights) or an ultralytics YOLOv8 detection `.pt` checkpoint (read as
    data by caesar_yolo_amd.pt_import: no ultralytics needed); the string "seeded:<scale>:<nc>[:seed]" builds the
    deterministic random-init checkpoint used by the tests and the benchmark (no trained weights ship with the
    reference)."""

    def __init__(self, weights, precision="fp16x3", max_batch=64, max_imgsz=640, device=None):
        # precision: "fp16x3" (default: the parity context -- the reference runs ultralytics in fp32), "fp32" (exact, slow), "fp16" (3x faster)
        self._wpath = self._resolve(weights)
        self._kw = dict(precision=precision, max_batch=max_batch, max_imgsz=max_imgsz)
        self._det = None
        self._dev = device
        scale, names, _, _ = W.read_cyw_header(self._wpath)
        self.names = names
        self.scale = scale

    @staticmethod
    def _resolve(weights):
        if isinstance(weights, str) and weights.startswith("seeded:"):
            parts = weights.split(":")
            scale, nc = parts[1], int(parts[2])
            seed = int(parts[3]) if len(parts) > 3 else 20260104
            import tempfile
            cache = os.environ.get("CAESAR_YOLO_CACHE", os.path.join(tempfile.gettempdir(), "caesar_yolo_amd_%d" % os.getuid()))
            os.makedirs(cache, exist_ok=True)
            path = os.path.join(cache, "seeded_%s_nc%d_%d.cyw" % (scale, nc, seed))
            if not os.path.exists(path):
                tmp = path + ".%d.tmp" % os.getpid()
                W.make_seeded_file(tmp, scale, nc, seed)
                os.replace(tmp, path)
            return path
        if isinstance(weights, str) and weights.startswith("seeded11:"):           # seeded YOLO11: "seeded11:<scale>:<nc>[:seed]"
            parts = weights.split(":")
            scale, nc = parts[1], int(parts[2])
            seed = int(parts[3]) if len(parts) > 3 else 11
            import tempfile
            cache = os.environ.get("CAESAR_YOLO_CACHE", os.path.join(tempfile.gettempdir(), "caesar_yolo_amd_%d" % os.getuid()))
            os.makedirs(cache, exist_ok=True)
            path = os.path.join(cache, "seeded11_%s_nc%d_%d.cyw" % (scale, nc, seed))
            if not os.path.exists(path):
                tmp = path + ".%d.tmp" % os.getpid()
                W.make_seeded11_file(tmp, scale, nc, seed)
                os.replace(tmp, path)
            return path
        if not os.path.isfile(weights):
            raise FileNotFoundError(weights)
        with open(weights, "rb") as fp:
            magic = fp.read(4)
        if magic in (b"CYW1", b"CYW2"):
            return weights
        # an ultralytics checkpoint (scripts/run.py:347 passes the .pt path): converted once, without unpickling any of
        # its classes (pt_import), and cached next to the seeded files
        import tempfile
        from . import pt_import
        st = os.stat(weights)
        cache = os.environ.get("CAESAR_YOLO_CACHE", os.path.join(tempfile.gettempdir(), "caesar_yolo_amd_%d" % os.getuid()))
        os.makedirs(cache, exist_ok=True)
        path = os.path.join(cache, "%s_%d_%d.cyw" % (os.path.splitext(os.path.basename(weights))[0], st.st_size, int(st.st_mtime)))
        if not os.path.exists(path):
            tmp = path + ".%d.tmp" % os.getpid()
            pt_import.convert_pt_to_cyw(weights, tmp)
            os.replace(tmp, path)
        return path

    def engine(self, device=None):
        if self._det is None:
            dev = device if device is not None else (self._dev if self._dev is not None else
                                                     int(os.environ.get("LOCAL_RANK", "0")))
            self._det = HipDetector(self._wpath, device=dev, **self._kw)
        return self._det

    def __call__(self, image, device=None, imgsz=640, conf=0.25, iou=0.7, augment=False, **ignored):
        """augment=True: ultralytics' test-time augmentation -- the letterboxed image, its 0.83-scale left-right flip and its
        0.67-scale view through the network, one NMS over the three predictions (DetectionModel._predict_augment)."""
        det = self.engine(device)
        img = np.asarray(image, dtype=np.float64)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("expected an (H,W,3) image")
        planes = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))[None]).to(det.tdev)
        if augment:
            src, lb = det.letterbox_pack_f32(planes, int(imgsz))
            preds = [det.forward(v) for v in det.augment_pack(src)]
            d, _, cnt = det.decode_nms_augmented(preds, lb.H, lb.W, img.shape[0], img.shape[1], float(conf), float(iou))
            n = int(cnt[0].item())
            return [Results(d[0, :n])]
        netin, lb = det.letterbox_pack(planes, int(imgsz))
        pred = det.forward(netin)
        d, _, cnt = det.decode_nms(pred, lb.H, lb.W, img.shape[0], img.shape[1], float(conf), float(iou))
        n = int(cnt[0].item())
        return [Results(d[0, :n])]

    def predict_tiles(self, device_mosaic, tile_coords, pre_cfg, device=None, imgsz=640, conf=0.25, iou=0.7,
                      merge_overlap_iou_thr_soft=0.3, merge_overlap_iou_thr_hard=0.8, augment=False, **ignored):
        """Batched entry of the tile queue (SURVEY §8b "additive" entry; no counterpart in ultralytics).

        device_mosaic : [ny,nx] fp32 tensor on the GPU (HipDetector.mosaic_to_device)
        tile_coords   : B rows (xmin, xmax_excl, ymin, ymax_excl) like utils.generate_tiles, all of ONE shape
        pre_cfg       : cy_preproc_cfg (DataPreprocessor.program())
        Runs TileTask.find_sources' per-tile chain (caesar_yolo/inference.py:173-275: crop, preprocessing, model call,
        process_detections) for the whole batch; returns one Results per tile (boxes in TILE pixel coordinates), or None
        where the reference would skip the tile (pipeline gave None / constant rows).  augment=True: test-time augmentation
        of every tile's model call (see __call__)."""
        det = self.engine(device)
        tc = np.asarray(tile_coords, dtype=np.int64).reshape(-1, 4)
        if len(tc) == 0:
            return []
        tw, th = tc[:, 1] - tc[:, 0], tc[:, 3] - tc[:, 2]
        if (tw != tw[0]).any() or (th != th[0]).any():
            raise ValueError("predict_tiles needs tiles of one shape per call (group ragged edge tiles separately)")
        d, cnt, status = det.detect_tiles(device_mosaic, [(int(r[0]), int(r[2])) for r in tc], int(th[0]), int(tw[0]),
                                          int(imgsz), pre_cfg, float(conf), float(iou),
                                          float(merge_overlap_iou_thr_soft), float(merge_overlap_iou_thr_hard), augment=bool(augment))
        cnt, status = cnt.cpu().numpy(), status.cpu().numpy()
        return [Results(d[b, :int(cnt[b])]) if status[b] == 0 else None for b in range(len(tc))]
