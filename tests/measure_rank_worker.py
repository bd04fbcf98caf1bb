"""One rank of tests/test_gpu_measure_cli.py's two-rank run: scripts/run.py's main() inside a gloo process group, so that two
ranks can share one card (run.py itself opens an RCCL group, one GPU per rank).  Started by torch.distributed.run as a fresh
process; the arguments are run.py's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

if __name__ == "__main__":
    import torch.distributed as dist
    dist.init_process_group("gloo")
    import run
    sys.exit(run.main(sys.argv[1:]))
