"""The search's diagnostics on a PHASES=1 build (csrc/diag.h; make PHASES=1), each case in a fresh child on that library as in
tests/test_gpu_diag_build.py (the product library is already loaded here):

  * queue_kind_mismatch == 0: the kind a search takes from its place in the queue (front: the probe row is read; back: it is rebuilt without
    being read) is what pc_key[] - which only this build still keeps - says, for every search of the scene of
    tests/helpers/search_chain_scenes.py and of 10 sweeps of the benchmark's sequence of seed 1000 on a team of two;
  * the rows the executed-work counters call rebuilt are the rows the diagnostics counted, and on the scene they are the sweep's 4096 first
    searches plus every crossing of a voxel face in the oracle's iterations;
  * the laps of a scan's FIRST iteration are there and non-zero, and its searches are the scans' source points;
  * in iteration 1 or 2 the fronts of workgroup 0 are no multiple of 64: a wavefront of the search holds groups of both kinds;
  * the diagnostics change no result."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import search_chain_diag_case as case
from tests.helpers import search_chain_scenes as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptudes-lab_amd", "csrc")
IT0 = ("search_it0_row_key", "search_it0_rebuild", "search_it0_first_round", "search_it0_survivors", "search_it0_answer_row", "searches_timed_it0",
       "searches_it0")


@pytest.fixture(scope="module")
def phases_lib():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the diagnostic library cannot be built")
    out = os.path.join(CSRC, "libptudes_mi_phases.so")  # (beside the product library: make leaves it alone while no source is newer)
    subprocess.run(["make", "-C", CSRC, "-j16", "OUT=" + out, "PHASES=1", out], check=True, capture_output=True, timeout=900)
    return out


def _child(lib, name):
    env = dict(os.environ, PTL_LIB_PATH=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "search_chain_diag_case.py"), name], env=env, capture_output=True, text=True,
                       timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("SEARCH_CHAIN_CASE ")][-1][len("SEARCH_CHAIN_CASE "):])


@pytest.mark.parametrize("name", ["scene", "bench"])
def test_queue_kinds_rebuilt_rows_and_first_iteration_laps(phases_lib, name):
    got = _child(phases_lib, name)
    ref = case.run_case(name)  # the product library, in this process
    assert ref["build"] == 0 and got["build"] == 1
    for s, (m, p) in enumerate(zip(got["members"], ref["members"])):
        d = m["diag"]
        print(name, s, {k: v for k, v in d.items() if v})
        assert (m["kiss"], m["stats"], m["exec"]) == (p["kiss"], p["stats"], p["exec"]), s  # diagnostics change no result
        assert d["queue_kind_mismatch"] == 0
        assert d["searches"] == m["exec"]["searches"] > 0 and d["rows_rebuilt"] == m["exec"]["rows_rebuilt"] > 0
        for k in IT0:
            assert d[k] > 0, k
        assert d["searches_it0"] == sum(st["n_src"] for st in m["stats"] if st["iterations"] > 0)
        assert 0 <= d["survivor_rounds_it0"] <= d["survivor_rounds"]
        assert d["searches_timed"] > 0 and d["search_row_key"] > 0  # the later iterations' laps as before
        if name == "scene":
            its = sc.iterations()
            vox = [np.floor(q / sc.VOXEL_SIZE).astype(np.int64) for q, _ in its]
            crossed = [(vox[i] != vox[i - 1]).any(axis=1) for i in range(1, len(its))]
            assert d["rows_rebuilt"] == sc.CELLS + sum(int(c.sum()) for c in crossed)
            wg0 = ((np.arange(sc.CELLS) >> 6) & 1) == 0
            fronts = [d["misses_at_iteration_%d" % i] - int(crossed[i - 1][wg0].sum()) for i in (1, 2)]
            assert all(f > 0 for f in fronts) and any(f % 64 for f in fronts), fronts
