"""cy_forced_fit on the 46341 x 46339 map of tests/bigmap_cases.py: the drawn Gaussians of every patch and decoy as forced jobs (their
true positions and shapes) in one call, weighted by the rms map, on patches that hold pixel 2^29, 2^30, 3 * 2^29 and the last pixel
of a map just below 2^31 pixels.  The reference is tests/forced_ref.py on the host twins and the comparison is its rule
(forced_ref.compare): no tolerance is new here.  A kernel whose 32-bit pixel offset wrapped would read the decoy 2^30 pixels before
a patch, in the map or in the rms map: the decoys hold other amplitudes and other noise, so such a row does not pass (asserted
below on the reference rows themselves).

No skip path: when the maps cannot be allocated the test errors."""
import numpy as np
import pytest
import torch

import bigmap_cases as B
import forced_ref as FR
from gpu_common import detector

pytestmark = pytest.mark.gpu


def forced_jobs(name):
    """[6, 6] forced jobs on the blobs of one patch: the drawn centre and shape in image coordinates, bkg 0."""
    y0, x0 = B.PLACES[name]
    truth = B.patch(name)[2]
    return np.array([[truth[nm][1] + x0, truth[nm][2] + y0, truth[nm][3], truth[nm][4], truth[nm][5], 0.0] for nm in B.PEAK_NAMES], np.float64)


def test_forced_fit_on_the_big_map():
    det = detector("fp32", max_batch=1, max_imgsz=160)
    jobs = np.concatenate([forced_jobs(nm) for nm in B.names()])
    names = B.job_names(B.PEAK_NAMES)
    ref, aux = FR.forced_fit(B.host(), B.host_rms(), jobs, 3.0, 1)
    assert np.isin(ref[:, 0], (0, 2)).all() and (ref[:, 1] > 3).all() and (ref[:, 4] > 0).any()       # every job fitted; the pairs are neighbours
    # a row read from the decoy would not pass: the patch and its decoy differ by far more than the bounds
    for nm, decoy in B.DECOY_OF.items():
        a, b = ref[B.rows_of(nm, len(B.PEAK_NAMES))], ref[B.rows_of(decoy, len(B.PEAK_NAMES))]
        tol = np.array([FR.tolerances(aux[k])["dx"][0] for k in range(*B.rows_of(nm, len(B.PEAK_NAMES)).indices(len(ref)))])
        assert (np.abs(a[:, 7] - b[:, 7]) > 1e6 * tol).all()
    dev = B.device(det.tdev)
    rms = B.device(det.tdev, B.rms_patch)
    try:
        got = det.forced_fit(dev, rms, jobs, 3.0, True)
        report = []
        FR.compare(got, ref, aux, names, report)
        assert det.forced_fit(dev, rms, jobs, 3.0, True).tobytes() == got.tobytes()
        truth = np.array([B.patch(nm)[2][b][0] * s for nm in B.names() for b, s in zip(B.PEAK_NAMES, [bl[4] for bl in B.BLOBS])])
        print("forced_fit: %d jobs; kernel %.3f ms; worst |gpu - ref| / bound: %s; largest |amp - drawn| / sqrt(amp_var): %.2f" % (
            len(ref), det.forced_kernel_ms(), ", ".join("%s %.3g" % (f, r) for _, f, r in report),
            float(np.abs((got[:, 7] - truth) / np.sqrt(got[:, 8])).max())))
    finally:
        del dev, rms
        torch.cuda.empty_cache()
