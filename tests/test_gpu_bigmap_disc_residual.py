"""cy_disc_residuals on the 46341 x 46339 map of tests/bigmap_cases.py: the peak jobs of every patch and decoy in one call, on
patches that hold pixel 2^29, 2^30, 3 * 2^29 and the last pixel of a map just below 2^31 pixels, with the drawn Gaussians as the
model map.  The reference is tests/disc_residual_ref.py on the host twins and the comparison is its rule (disc_residual_ref.compare):
no tolerance is new here.  A kernel whose 32-bit pixel offset wrapped would read the decoy 2^30 pixels before a patch, in the map or
in the model; tests/test_disc_residual_cpu.py shows that such a row does not pass.

No skip path: when the maps cannot be allocated the test errors."""
import numpy as np
import pytest
import torch

import bigmap_cases as B
import disc_residual_ref as DR
from gpu_common import detector

pytestmark = pytest.mark.gpu


def test_disc_residuals_on_the_big_map():
    det = detector("fp32", max_batch=1, max_imgsz=160)
    jobs = B.all_peak_jobs()
    ref, ab = DR.disc_residuals(B.host(), B.host_model(), jobs)
    assert (ref[:, 0] == 0).all() and (ref[:, 1] > 0).all() and ref[:, 14].any()      # every job measured; the corner discs leave the image at `end`
    dev = B.device(det.tdev)
    model = B.device(det.tdev, lambda nm: B.patch(nm)[1])
    try:
        got = det.disc_residuals(dev, model, jobs)
        DR.compare(got, ref, ab, B.job_names(B.PEAK_NAMES))
        assert det.disc_residuals(dev, model, jobs).tobytes() == got.tobytes()
        print("disc_residuals: %d jobs; kernel %.3f ms" % (len(ref), det.disc_residual_kernel_ms()))
    finally:
        del dev, model
        torch.cuda.empty_cache()
