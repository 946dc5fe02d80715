"""The reference's own scan tests (MPICH test/mpi/coll scantst.c, exscan.c, exscan2.c, shipped
with MVAPICH2 2.3.7), restated as one C program (tests/mpich_scan/scan_suite.c) that links the
drop-in libmpi.so like an application, calls MPI_Scan and MPI_Exscan on hipMalloc'd (and on
host) buffers and checks each test's closed-form answers: MPI_SUM, the tests' two user ops (one
of them non-commutative and order-checking), MPI_IN_PLACE, and rank 0's untouched buffer."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITE = os.path.join(ROOT, "tests", "mpich_scan")
EXE = os.path.join(SUITE, "scan_suite")
CASES = ["scantst", "exscan", "exscan2"]


def _exe():
    src = os.path.join(SUITE, "scan_suite.c")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(src):
        subprocess.run(["make", "-C", SUITE], check=True, capture_output=True)
    return EXE


def test_suite_lists_every_case():
    """the Python list and the C program's case table agree (CPU: reads the source)"""
    src = open(os.path.join(SUITE, "scan_suite.c")).read()
    table = src[src.index("kCases[] = {"):]
    for c in CASES:
        assert f'{{"{c}", t_{c}}}' in table, c


@pytest.mark.gpu
@pytest.mark.parametrize("mem,n", [("device", 2), ("device", 5), ("device", 8), ("host", 3), ("host", 8)])
def test_reference_scan_suite(mem, n):
    cmd = [sys.executable, "-m", "mvapich2_amd.mv2run", "-n", str(n), "--share-gpu", "--timeout", "170", _exe(), mem]
    env = dict(os.environ, MV2AMD_TIMEOUT_S="30", PYTHONPATH=ROOT)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith(mem + " ")]
    per_case = {ln[1]: int(ln[2]) for ln in lines if ln[1] != "TOTAL"}
    assert p.returncode == 0 and set(per_case) == set(CASES) and not any(per_case.values()), \
        (p.returncode, p.stdout, p.stderr[-3000:])
