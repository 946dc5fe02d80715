"""The properties the reference's MPI_Alltoallw tests check (MPICH test/mpi/coll alltoallw1.c,
alltoallw2.c, alltoallw_zeros.c, shipped with MVAPICH2 2.3.7), written anew as one C program
(tests/mpich_alltoallw/alltoallw_suite.c) that links the drop-in libmpi.so like an application and
calls MPI_Alltoallw (and MPI_Alltoallv) on hipMalloc'd and on host buffers: the transpose of a
block-distributed matrix with a resized-vector send type and one vector receive type per peer;
i items to rank i at byte displacements with untouched space between the receive blocks, plain
and strided, and the exchange in place; zero counts against zero-size types, in place with
signatures that differ between odd and even ranks."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITE = os.path.join(ROOT, "tests", "mpich_alltoallw")
EXE = os.path.join(SUITE, "alltoallw_suite")
CASES = ["alltoallw1", "alltoallw2", "alltoallw_zeros"]


def _exe():
    src = os.path.join(SUITE, "alltoallw_suite.c")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(src):
        subprocess.run(["make", "-C", SUITE], check=True, capture_output=True)
    return EXE


def test_suite_lists_every_case():
    """the Python list and the C program's case table agree (CPU: reads the source)"""
    src = open(os.path.join(SUITE, "alltoallw_suite.c")).read()
    table = src[src.index("kCases[] = {"):]
    for c in CASES:
        assert f'{{"{c}", t_{c}}}' in table, c


@pytest.mark.gpu
@pytest.mark.parametrize("mem", ["device", "host"])
def test_reference_alltoallw_suite(mem):
    cmd = [sys.executable, "-m", "mvapich2_amd.mv2run", "-n", "4", "--share-gpu", "--timeout", "170", _exe(), mem]
    env = dict(os.environ, MV2AMD_TIMEOUT_S="30", PYTHONPATH=ROOT)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith(mem + " ")]
    per_case = {ln[1]: int(ln[2]) for ln in lines if ln[1] != "TOTAL"}
    assert p.returncode == 0 and set(per_case) == set(CASES) and not any(per_case.values()), \
        (p.returncode, p.stdout, p.stderr[-3000:])
