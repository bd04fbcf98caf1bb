"""bench.py's two kinds of run on a reduced mosaic (8192^2, 400 tiles): a plain run reports the headline only, --full adds the
parity pass and the per-kernel figures, and --dump-outputs writes the catalog the last timed step returned -- the same catalog
from both runs (seeded inputs), the one the line's digest names."""
import hashlib
import json
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "8192"] + list(flags)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _outputs(d, line):
    cat = np.load(os.path.join(d, "catalog.npy"))
    st = np.load(os.path.join(d, "tile_stats.npy"))
    assert cat.dtype == np.float64 and cat.shape == (line["config"]["sources_in_catalog"], 8)
    assert hashlib.sha1(cat.tobytes()).hexdigest() == line["config"]["catalog_sha1"]
    assert st.dtype == np.float64 and st.tolist() == [line["config"]["tiles"], line["config"]["tiles_skipped"],
                                                      line["config"]["per_tile_detections"], line["config"]["degenerate_boxes_dropped"],
                                                      line["config"]["candidate_overflow_tiles"]]
    return cat, st


def test_plain_and_full_runs_dump_the_same_catalog(tmp_path):
    plain = _bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain"))
    assert all(k in plain for k in HEADLINE) and plain["steps"] == 2 and plain["full"] is False
    assert plain["unit"] == "tiles/s" and plain["higher_is_better"] is True and plain["dtype"] == "f16"
    assert plain["value"] == pytest.approx(plain["config"]["tiles"] * 1000.0 / plain["ms_per_step"])
    for k in ("parity_mode", "roofline", "forward_kernels", "cpu_baseline"):
        assert k not in plain, k
    full = _bench("--full", "--no-cpu-baseline", "--steps", "1", "--warmup", "1", "--dump-outputs", str(tmp_path / "full"))
    assert full["full"] is True and full["steps"] == 1
    for k in ("parity_mode", "roofline", "forward_kernels"):
        assert k in full, k
    assert full["ms_ingest_warm_rank0"] is not None and full["parity_value"] == full["parity_mode"]["value"]
    cp, sp = _outputs(str(tmp_path / "plain"), plain)
    cf, sf = _outputs(str(tmp_path / "full"), full)
    assert np.array_equal(cp, cf) and np.array_equal(sp, sf)
    assert len(cp) > 0
    print("plain %.0f tiles/s, --full %.0f tiles/s (parity %.0f); %d sources from both" % (
        plain["value"], full["value"], full["parity_value"], len(cp)))
