"""A library with every diagnostic flavour compiled in (make PHASES=1 STAGES=1 EXTRA=-DMAP_DIAG, csrc/diag.h): the flavours share one build,
their values land in named slots inside the allocation for every team size and gn_workgroups, and they change no result.

The product library is already loaded in this process, so every case runs in a fresh child with PTL_LIB_PATH on the diagnostic library
(tests/helpers/diag_case.py prints JSON) and is compared with the same case run here on the product library.  Until the slots had storage
of their own, case (a) had per-workgroup words and fixed slots in the same words, (b) and (c) wrote the fixed slots behind the allocation,
and ptl_icp_linear_system shared DevState's sums with three flavours."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from helpers import diag_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptudes-lab_amd", "csrc")
STAGE_SLOTS = ["sq_prologue", "sq_wait_prologue", "sq_deskew_vds1", "sq_wait_deskew_vds1", "sq_compact_fd", "sq_wait_compact_fd", "sq_vds2", "sq_wait_vds2",
               "sq_compact_src", "sq_insert_a", "sq_wait_insert_a", "sq_insert_b", "sq_wait_insert_b", "sq_prune",
               "k1_entry", "k1_load_deskew_store", "k1_claim", "k1_bid", "k1_slot1", "k1_count"]


@pytest.fixture(scope="module")
def diag_lib(tmp_path_factory):
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the diagnostic library cannot be built")
    out = str(tmp_path_factory.mktemp("diag") / "libptudes_mi_diag.so")
    subprocess.run(["make", "-C", CSRC, "-j16", "OUT=" + out, "PHASES=1", "STAGES=1", "EXTRA=-DMAP_DIAG", out], check=True, capture_output=True, timeout=900)
    return out


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_all_flavours_in_one_build(diag_lib, name):
    env = dict(os.environ, PTL_LIB_PATH=diag_lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "diag_case.py"), name], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DIAG_CASE ")][-1][len("DIAG_CASE "):])
    ref = diag_case.run_case(name)  # the product library, in this process
    assert ref["build"] == 0 and got["build"] == 1 | 4 | 8
    assert (got["team"], got["gn_workgroups"]) == (ref["team"], ref["gn_workgroups"])
    if name == "a":
        assert got["team"] == 32 and got["gn_workgroups"] > 32
    G, team = got["gn_workgroups"], got["team"]
    for s, (m, p) in enumerate(zip(got["members"], ref["members"])):
        d = m["diag"]
        print(name, s, {k: v for k, v in d.items() if v})
        # diagnostics change no result
        assert (m["kiss"], m["res"], m["stats"]) == (p["kiss"], p["res"], p["stats"]), s
        assert not any(p["diag"].values())  # the product build collects nothing
        if name != "c":
            assert m["exec"] == p["exec"]
            assert d["searches"] == m["exec"]["searches"] and d["rows_rebuilt"] == m["exec"]["rows_rebuilt"]
            for k in STAGE_SLOTS:
                assert d[k] > 0, k
        hist = sum(d["bound_ratio_%d" % i] for i in range(5))
        assert d["bound_candidate"] + d["bound_box"] == hist <= d["searches"] and hist > 0
        assert 0 < d["miss_other_neighbour"] + d["miss_voxel_changed"] + d["miss_no_answer"] + d["miss_same_neighbour"] <= d["searches"]
        for k in ("phase_a_chunks", "search_passes", "searches_timed", "tails"):
            assert d[k] > 0, k
        assert not any(v for k, v in d.items() if k.startswith("map_"))  # no capacity error was raised
        assert any(d.values()) and not any(m["diag_after_cold_start"].values())  # a cold start clears the slots
        # the 2 * gn_workgroups per-workgroup words: the team's 2 x team in front, nothing behind them
        wc = m["wg_clocks"]
        assert any(wc[:2 * team]) and not any(wc[2 * team:2 * G]) and not any(wc[2 * G:])
        if name == "c":
            # the linear system's totals and the slots no longer share memory
            assert m["lin"][0] == m["lin"][1] == p["lin"][0] == m["lin_kept"] and m["lin"][0][1] > 0
            assert m["diag_after_lin"][0] == m["diag_after_lin"][1] == d
