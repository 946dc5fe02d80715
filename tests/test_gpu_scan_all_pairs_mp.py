"""Every legal (op, type) pair the device supports through MPI_Scan and MPI_Exscan at 3 and 5 ranks,
every rank's bytes against tests/ref_scan.py exactly as test_gpu_scan_mp.check_case compares them
(MPI_Exscan's rank 0 must hand its receive buffer back untouched).

Sizes (tests/all_pairs_cases.py, checked on the CPU by tests/test_all_pairs_table.py): 520 B, the
compact one-shot scan kernel; 1,552 B, its vector body (leaves folded in any order for the order-free
pairs, the program evaluator otherwise) and an element tail; 40,976 B, the pipelined scan, whose
segments differ in length at 3 and 5 ranks.  The "small" pipeline geometry with the one-shot limit
at 16 KiB, as in test_gpu_collectives_all_pairs_mp.py; every rank runs the matrix on one pair of
device buffers (worker kind "scan_batch")."""
import pytest

from mvapich2_amd.consts import TYPES
from tests import all_pairs_cases as apc
from tests.test_gpu_scan_mp import check_case, run_scan_workers

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(300)
@pytest.mark.parametrize("coll", ["scan", "exscan"])
@pytest.mark.parametrize("n", apc.NS)
def test_scan_all_pairs(n, coll, tmp_path):
    cases = apc.scan_cases(n, coll)
    spec = [{"id": "batch", "kind": "scan_batch", "cases": cases}, {"id": "info", "kind": "info", "keys": ["oneshot_max"]}]
    get, _ = run_scan_workers(n, spec, tmp_path, timeout=200, extra_env=apc.ENV_D)
    blobs = []
    for r in range(n):
        assert get("info", r)[0] == apc.ONESHOT_MAX, (r, get("info", r))
        blobs.append(get("batch", r))
    off, bad = 0, []
    for c in cases:
        ln = c["count"] * TYPES[c["type"]][3]
        try:
            check_case(c, n, None, got=[b[off:off + ln] for b in blobs])
        except AssertionError as e:
            bad.append(f"{c['op']} {c['type']} size {c['size']} [{c['path']}]: {e}")
        off += ln
    assert all(len(b) == off for b in blobs)
    assert not bad, f"{len(bad)} results differ from the reference order:\n" + "\n".join(bad[:40])
