"""Times MPI_Alltoallw of the transpose types (a resized-vector column type out, a vector corner
type in) with the batched block pack against the per-block route of the same build
(mv2h_set_tuning("pack_blocks", 0)), N ranks sharing one GPU.

  python tools/alltoallw_timing.py [-n 4] [--iters 200] [--warmup 20] [pair_bytes ...]

Prints one line per size: the median over warm calls of each route (the slowest rank's median, in
microseconds), their ratio, and the fastest call seen.  The worker is the tests' own
(tests/mp_alltoallw_worker.py, kind "timing"), which also checks the transposed result once."""
import argparse
import os
import subprocess
import sys
import tempfile
import uuid
import json

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("pair", type=int, nargs="*", default=[1 << 10, 64 << 10, 4 << 20])
    a = ap.parse_args()
    cases = [{"id": f"t{p}", "kind": "timing", "pair": p, "iters": a.iters if p < (1 << 20) else max(a.iters // 4, 10),
              "warmup": a.warmup} for p in a.pair]
    with tempfile.TemporaryDirectory() as tmp:
        spec = os.path.join(tmp, "spec.json")
        json.dump({"cases": cases}, open(spec, "w"))
        jobid = "t" + uuid.uuid4().hex[:12]
        procs = []
        for r in range(a.n):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(a.n), LOCAL_RANK=str(r), LOCAL_WORLD_SIZE=str(a.n),
                       MV2AMD_JOBID=jobid, MV2AMD_TIMEOUT_S="60")
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_alltoallw_worker.py"), spec, tmp],
                                          env=env))
        rcs = [p.wait(timeout=900) for p in procs]
        if any(rcs):
            sys.exit(f"workers failed: {rcs}")
        for c in cases:
            us = np.array([np.load(os.path.join(tmp, f"{c['id']}_us_r{r}.npy")) for r in range(a.n)])
            b, bmin, p, pmin = us[:, 0].max(), us[:, 1].max(), us[:, 2].max(), us[:, 3].max()
            print(f"alltoallw_timing n={a.n} pair_bytes={c['pair']} iters={c['iters']} batched_median_us={b:.1f} "
                  f"per_block_median_us={p:.1f} ratio={p / b:.2f} batched_min_us={bmin:.1f} per_block_min_us={pmin:.1f}",
                  flush=True)


if __name__ == "__main__":
    main()
