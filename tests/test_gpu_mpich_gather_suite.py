"""The properties the reference's gather / scatter / allgatherv tests check (MPICH test/mpi/coll
gather.c, gather2.c, scatter2.c, scatter3.c, scattern.c, scatterv.c, allgatherv2.c, allgatherv3.c
and the gather / scatter members of coll2.c - coll6.c, shipped with MVAPICH2 2.3.7), written anew
as one C program (tests/mpich_gather/gather_suite.c) that links the drop-in libmpi.so like an
application and calls MPI_Gather(v), MPI_Scatter(v) and MPI_Allgatherv on hipMalloc'd (and on
host) buffers: vector types on the side that owns one block and on the side that owns n, every
root in turn, MPI_IN_PLACE with its ignored arguments, zero-size calls, a matrix dealt out as
interleaved tiles through a resized type, and the table exercises, each against its closed form."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITE = os.path.join(ROOT, "tests", "mpich_gather")
EXE = os.path.join(SUITE, "gather_suite")
CASES = ["gather", "gather2", "scatter2", "scatter3", "scattern", "scatterv", "allgatherv2", "allgatherv3",
         "coll2", "coll3", "coll4", "coll5", "coll6"]


def _exe():
    src = os.path.join(SUITE, "gather_suite.c")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(src):
        subprocess.run(["make", "-C", SUITE], check=True, capture_output=True)
    return EXE


def test_suite_lists_every_case():
    """the Python list and the C program's case table agree (CPU: reads the source)"""
    src = open(os.path.join(SUITE, "gather_suite.c")).read()
    table = src[src.index("kCases[] = {"):]
    for c in CASES:
        assert f'{{"{c}", t_{c}}}' in table, c


@pytest.mark.gpu
@pytest.mark.parametrize("mem,n", [("device", 2), ("device", 3), ("device", 4), ("device", 8), ("host", 2), ("host", 5)])
def test_reference_gather_suite(mem, n):
    cmd = [sys.executable, "-m", "mvapich2_amd.mv2run", "-n", str(n), "--share-gpu", "--timeout", "170", _exe(), mem]
    env = dict(os.environ, MV2AMD_TIMEOUT_S="30", PYTHONPATH=ROOT)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith(mem + " ")]
    per_case = {ln[1]: int(ln[2]) for ln in lines if ln[1] != "TOTAL"}
    assert p.returncode == 0 and set(per_case) == set(CASES) and not any(per_case.values()), \
        (p.returncode, p.stdout, p.stderr[-3000:])
