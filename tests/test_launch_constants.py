"""The launch constants that the branch tests restate (tile sizes, grid caps, the LDS span) against
the sources they come from.  mv2h_get_info exports the tunings (rl_tiny_max, rl_grid, max_grid) but
not these compile-time constants, so a change of one of them must fail here instead of silently
moving the shapes of test_gpu_*_branches.py off the branches they name."""
import os
import re

from tests import test_gpu_pack_branches as pk
from tests import test_gpu_reduce_local_branches as rl
from tests import test_gpu_reduce_n_branches as rn

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvapich2_amd", "csrc")


def source(*path):
    with open(os.path.join(CSRC, *path)) as f:
        return f.read()


def constant(text, name):
    found = re.findall(r"^constexpr int " + name + r" = (\d+);", text, flags=re.M)
    assert len(found) == 1, name
    return int(found[0])


def test_reduce_kernels_tiles():
    impl, util = source("coll", "kernels_impl.h"), source("device_util.h")
    assert constant(impl, "kRLThreads") == rl.RL_THREADS
    assert f"k_reduce_local<Rd, {rl.RL_U}>" in impl and f"(size_t)kRLThreads * {rl.RL_U};" in impl
    assert constant(util, "kThreads") == rl.ELEM_THREADS == rn.RN_THREADS
    assert "k_reduce_n<Rd, 1>" in impl  # one vector per thread: a tile is kThreads vectors
    coll = source("runtime", "coll.cpp")
    assert coll.count(f"std::min(world().rl_grid, {rn.RN_GRID_CAP})") == 2  # mv2h_reduce_n, mv2h_reduce_n_prog


def test_pack_kernels_constants():
    pack = source("pack", "pack.hip")
    assert constant(pack, "kPackThreads") * constant(pack, "kPackU") == pk.UNITS_TILE
    assert constant(pack, "kLdsSpan") == pk.LDS_SPAN
    assert "(kLdsSpan - 32) / stride" in pack
    assert constant(pack, "kRunLds") == pk.RUNS_LDS
    assert constant(source("device_util.h"), "kThreads") == pk.RUNS_THREADS
    assert f"if (grid > {pk.RUNS_GRID}) grid = {pk.RUNS_GRID};" in pack
