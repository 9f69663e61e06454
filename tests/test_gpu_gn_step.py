"""The Gauss-Newton step of every per-call form of the registration - weights, the 27 sums of k_gn_loop, the 16 moments of the 8-lane
kernel and sums_from_moments, solve6_ldlt_wave, se3_exp_gn, the composition into the pose - against the long-double reference of
tests/helpers/gn_longdouble.py on the scenes of tests/helpers/gn_step_scenes.py: the room up to 100 km from the origin (cond(JTJ) from 3e2 to
above 1e16), under a guess turned by 170 degrees, steps on both sides of the series switch of se3_exp_gn and up to 1 rad, sources of 1, 2, 3,
40 collinear, 40 coincident and 40 nearly collinear points, and source sizes around the chunk, queue-region and LDS sizes of the 8-lane kernel.
tests/test_gn_step_cpu.py shows without a GPU that the scenes are what they claim.

The yardsticks (none of them comes from device output):
  step   E_dev <= 4 E_orc + floor.  E is the largest distance between where a pose and the reference's pose put a source point; E_orc is the
         C oracle's largest E over 16 orders of the source, computed in this process; the floor is E_orc of far[0]; the 4 is DESIGN.md 3.15.2's
  sums   (32-lane kernel, where they can be read) per entry |S_dev - S_ref| <= (n_pairs + 19) 2^-53 T, T the absolute-value shadow of the sum;
         the count of 19 roundings per term stands beside gs.C_TERM
  rank < 6: what is defined, not equality (test_few_*)
Forms: sparse32 (k_gn_loop<P, false>), dense32 (k_gn_loop<P, true>: one workgroup of 256 threads, reached through a priming scan - see PRIMED),
lanes8_gc32 / gc8 / gc0 (k_gn_loop8 with 32, 8 and a run-time number of workgroups) and, on the sizes, lanes8_wg1.  linear_system and align
run the sparse template only; their rows are named sparse32 and sparse32_wg1.
Every figure asserted on goes to tests/helpers/gn_step_report.py (profiles/r021_gn_step_errors.json is one run of it).
"""
import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401  (import shim)
from ptudes_lab_amd import core
from tests.helpers import gn_longdouble as gl
from tests.helpers import gn_step_report as rep
from tests.helpers import gn_step_scenes as gs
from tests.test_gpu_search_edges import PER_CALL_FORMS, SMALL, _sorted_rows

pytestmark = pytest.mark.gpu

FORMS = {k: PER_CALL_FORMS[k] for k in ("sparse32", "dense32", "lanes8_gc32", "lanes8_gc8", "lanes8_gc0")}
ONE_WG = dict(gn_lanes_per_point=8, gn_threads=512, gn_workgroups=1)  # 3 073 sources cross GN8_LDS_PTS into src_cur, 513 a queue region
SIZES_FORMS = dict(FORMS, lanes8_wg1=ONE_WG)
# linear_system and align launch k_gn_loop<P, false> whatever the handle's form: under these two names they are two launch shapes of the sparse
# template (the default grid, and 1 workgroup x 256 threads), not the dense one
LANES32 = {"sparse32": FORMS["sparse32"], "sparse32_wg1": FORMS["dense32"]}
# register_frame runs the dense template k_gn_loop<P, true> (probe rows kept in memory across iterations) only when the PREVIOUS scan's source count,
# the hint, exceeds the handle's 32-lane groups: gn_workgroups * gn_threads / 32 = 8 on dense32.  A fresh handle's hint is 0, so the form is primed
PRIMED = ("dense32",)
PRIME_POINTS = 16
ONE_STEP = [n for n in gs.CATALOGUE if n.startswith(("far", "turned", "weights", "bigstep"))] + ["few[3]", "few[nearline]"]
DEFICIENT = ["few[1]", "few[2]", "few[collinear]", "few[coincident]"]


def _handle(sc, over, iterations=1):
    """a fresh handle with the scene's map in it, bit for bit the oracle's export"""
    icp = core.Icp(1e6, 0.0, voxel_size=gs.VS, max_points_per_voxel=gs.CAP, max_iterations=iterations, deskew=0, initial_threshold=sc.sigma,
                   max_points_per_scan=1 << 16, **SMALL, **over)
    icp.map_add(sc.map_in)
    assert np.array_equal(_sorted_rows(icp.map_points()), _sorted_rows(sc.stored)), sc.name
    return icp


def _prime(icp, sc, over):
    """a scan before the scene's, so that the scene's runs k_gn_loop<P, true>: 16 points 3 m apart, registered 500 m above the scene, where
    they pair with nothing (the pose is the guess) and enter the map out of every source's reach.  What the scene's scan then sees is unchanged
    - sigma stays initial_threshold while the sensor has not moved 0.5 m from its FIRST pose (one pose: it has not), nothing is deskewed, the
    guess is given, the 27 voxels of every source hold the same points - and _step asserts it: sigma, source, pair and candidate counts"""
    pts = np.outer(np.arange(1, PRIME_POINTS + 1) * 3.0, [0.6, 0.64, 0.48]) + np.array([0.013, 0.017, 0.011])
    g = np.array(sc.guess, dtype=np.float64)
    g[:3, 3] += [0.0, 0.0, 500.0]
    n_map = icp.map_size()[1]
    T = icp.register_frame(pts, None, g)
    st = icp.stats[-1]
    assert st["n_corr_last"] == 0 and st["sum_cand"] == 0 and np.abs(T - g).max() <= 1e-9, (sc.name, st)
    # the rule of ptl_icp_register (csrc/ptudes_mi.hip): dense when the previous scan's N_s > G * (gn_threads / 32); map_size() joins the map
    # stream, behind the copy that brings the hint to the host
    assert st["n_src"] == PRIME_POINTS > over["gn_workgroups"] * (over["gn_threads"] // 32), (sc.name, st)
    assert icp.map_size()[1] == n_map + PRIME_POINTS


def _step(sc, form, iterations=1):
    """register_frame on a fresh handle (primed where the form needs it): (pose, stats) after the source, sigma, the pair count and the candidate
    count have been checked against the reference's (iterations <= the steps the scene is guarded for)"""
    over = SIZES_FORMS[form]
    icp = _handle(sc, over, iterations)
    if form in PRIMED:
        _prime(icp, sc, over)
    T = icp.register_frame(sc.source, None, sc.guess)
    st = icp.stats[-1]
    assert np.array_equal(icp.last_source(), sc.source), sc.name  # sigma is initial_threshold and nothing is deskewed
    assert st["sigma"] == sc.sigma and st["n_src"] == len(sc.source)
    if iterations <= sc.steps:
        steps = sc.ref["steps"][:iterations]
        assert st["iterations"] == iterations, (sc.name, st)
        assert st["n_corr_last"] == steps[-1]["sys"]["n_pairs"], (sc.name, st)
        assert st["sum_cand"] == sum(s["corr"]["n_cand"] for s in steps), (sc.name, st)
    icp.close()
    return T, st


def _check_step(name, form, T, steps, what):
    sc = gs.scene(name)
    sp = gs.oracle_spread(name, steps)
    e = gl.step_error(T, sp["ref_pose"], sc.source)
    bound = gs.step_bound(name, steps)
    print(f"{name} {form} {what}: E_dev {e['E']:.3e} E_orc {sp['E']:.3e} bound {bound:.3e} dt {e['dt']:.3e} dr {e['dr']:.3e}")
    rep.record(name, form, what, E_dev=e["E"], E_orc=sp["E"], ratio=rep.ratio(e["E"], sp["E"]), bound=bound, dt=e["dt"], dr=e["dr"])
    assert e["E"] <= bound, (name, form, what, e, sp["E"], bound)
    return e["E"]


def _facts(name):
    sc = gs.scene(name)
    st = sc.ref["steps"][0]
    dx = st["sol"]["dx"].astype(np.float64)
    rep.scene_facts(name, sources=len(sc.source), pairs=st["sys"]["n_pairs"], cond=min(st["sol"]["cond"], 1e300), rank=st["sol"]["rank"],
                    step_translation=float(np.linalg.norm(dx[:3])), step_angle=float(np.linalg.norm(dx[3:])), removed_by_guard=sc.removed,
                    floor=gs.floor())


# ------------------------------------------------------------------------------------------------ sums of the 32-lane kernel
@pytest.mark.parametrize("name", list(gs.CATALOGUE))
def test_sums_of_the_32_lane_kernel_within_the_running_error_bound(name):
    sc = gs.scene(name)
    _facts(name)
    lin = sc.lin
    assert gs.oracle_spread(name)["sum_fraction"] <= 1.0  # the oracle meets the bound in all 16 orders before the device is asked to
    for form, over in LANES32.items():
        icp = _handle(sc, over)
        sums, nc, cand = icp.linear_system(sc.world64, sc.max_dist, sc.kernel)
        icp.close()
        assert (nc, cand) == (lin["n_pairs"], sc.ref["steps"][0]["corr"]["n_cand"]), (name, form, nc, cand)
        frac = gs.sum_fraction(sums, lin)
        print(f"{name} {form}: sum error {frac:.4f} of the bound (oracle {gs.oracle_spread(name)['sum_fraction']:.4f})")
        rep.record(name, form, "sums", fraction_of_bound=frac, oracle_fraction_of_bound=gs.oracle_spread(name)["sum_fraction"])
        assert frac <= 1.0, (name, form, frac)


# ------------------------------------------------------------------------------------------------ one step, two steps, to convergence
@pytest.mark.parametrize("name", ONE_STEP)
def test_one_step_of_every_form(name):
    sc = gs.scene(name)
    assert sc.ref["steps"][0]["sol"]["rank"] == 6
    for form in FORMS:
        T, _ = _step(sc, form)
        _check_step(name, form, T, 1, "step")


@pytest.mark.parametrize("name", gs.TWO_STEP)
def test_two_steps_of_every_form(name):
    """the second step runs on lazily moved positions and, on the 8-lane forms, on cached answer rows"""
    sc = gs.scene(name)
    assert sc.steps == 2
    for form in FORMS:
        T, _ = _step(sc, form, 2)
        _check_step(name, form, T, 2, "two_steps")


@pytest.mark.parametrize("o", gs.OFFSETS)
def test_to_convergence(o):
    """500 iterations allowed.  Up to 10 km: the iteration count is within 1 of the oracle's and the pose within the scene's largest two-step bound
    of the oracle's converged pose.  At 100 km the step noise competes with the stopping rule |dx| < 1e-4: the call returns, and the counts
    are recorded"""
    name = f"far[{gs.okey(o)}]"
    sc = gs.scene(name)
    ref_pose, it_ref, _, _ = gs.oracle_map(sc).register(sc.source, sc.guess, sc.max_dist, sc.kernel, max_iter=500)
    for form in FORMS:
        T, st = _step(sc, form, 500)
        E = gl.step_error(T, ref_pose, sc.source)["E"]
        print(f"{name} {form} converged: {st['iterations']} iterations (oracle {it_ref}), E against the oracle's pose {E:.3e}")
        rep.record(name, form, "converged", iterations=int(st["iterations"]), oracle_iterations=int(it_ref), E_to_oracle=E)
        assert 1 <= st["iterations"] <= 500 and np.isfinite(T).all()
        if o < 1e5:
            assert abs(st["iterations"] - it_ref) <= 1, (name, form, st["iterations"], it_ref)
            assert E <= gs.step_bound(name, 2), (name, form, E, gs.step_bound(name, 2))


# ------------------------------------------------------------------------------------------------ rank below 6
def _check_deficient(name, form, T):
    """what is defined when the system has a null space: the step solves the reference's system as well as the oracle's steps do, a noise
    pivot has not become a step of metres, and the pose is a rotation"""
    sc = gs.scene(name)
    st = sc.ref["steps"][0]
    sp = gs.oracle_spread(name)
    dx = gs.dx_of(T, sc)
    _, g = gl.unpack(st["sys"]["sums"])
    res, gnorm = gl.residual(st["sys"]["sums"], dx), float(np.sqrt((g * g).sum()))
    size, mn = float(np.sqrt((dx * dx).sum())), float(np.sqrt((st["sol"]["minnorm"] ** 2).sum()))
    dist = max(gl.step_error(T, P, sc.source)["E"] for P in sp["poses"])
    print(f"{name} {form}: residual {res:.3e} (oracle {sp['residual']:.3e}) |dx| {size:.4g} (min-norm {mn:.4g}) distance to the oracle's poses {dist:.3e}")
    rep.record(name, form, "deficient", residual=res, oracle_residual=sp["residual"], step_norm=size, minnorm=mn, distance_to_oracle_poses=dist,
               rank=st["sol"]["rank"])
    assert res <= 4.0 * sp["residual"] + 1e-14 * gnorm, (name, form, res, sp["residual"], gnorm)
    assert size <= 10.0 * mn + 1e-3, (name, form, size, mn)
    R = np.asarray(T)[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and np.array_equal(np.asarray(T)[3], [0.0, 0.0, 0.0, 1.0]), (name, form)
    return dist


@pytest.mark.parametrize("name", DEFICIENT)
def test_few_pairs_leave_a_null_space(name):
    """1 pair (rank 3), 2 pairs (5), 40 collinear sources (5), 40 coincident ones (3; they do not survive register_frame's down-sampling and go
    through align, which runs the 32-lane kernel whatever the handle's form)"""
    sc = gs.scene(name)
    assert sc.ref["steps"][0]["sol"]["rank"] == gs.FEW_RANK[name[4:-1]] < 6
    poses = {}
    if sc.via_align:
        for form, over in LANES32.items():
            icp = _handle(sc, over)
            T, it = icp.align(sc.source, sc.guess, sc.max_dist, sc.kernel)
            icp.close()
            assert it == 1
            _check_deficient(name, form, T)
        for form in ("dense32", "lanes8_gc32", "lanes8_gc8", "lanes8_gc0"):  # said, not passed over: rank 3 reaches them as ONE pair only
            rep.record(name, form, "not_run", reason="40 coincident sources do not survive register_frame's down-sampling, and align runs "
                                                     "k_gn_loop<P, false> only; few[1] and sizes[1] give this form a rank-3 system")
        return
    for form in FORMS:
        T, _ = _step(sc, form)
        _check_deficient(name, form, T)
        poses[form] = T
    # do the 8-lane and 32-lane kernels land on the same member of the solution family?  Recorded, not asserted
    d = gl.step_error(poses["lanes8_gc32"], poses["sparse32"], sc.source)["E"]
    print(f"{name}: 8-lane against 32-lane pose {d:.3e}")
    rep.record(name, "lanes8_gc32", "against_sparse32", E=d)


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", gs.SIZES)
def test_source_sizes_around_chunk_queue_and_lds(n):
    """far[1e4] (cond 1.5e14) cut to n sources; the 8-lane kernel also on one workgroup.  One source is one pair: rank 3, checked as such"""
    name = f"sizes[{n}]"
    sc = gs.scene(name)
    for form in SIZES_FORMS:
        T, _ = _step(sc, form)
        if n == 1:
            _check_deficient(name, form, T)
        else:
            _check_step(name, form, T, 1, "step")


def test_one_workgroup_and_four_agree_on_3073_sources():
    """association only, as in test_gn_launch_shapes_agree: the 8-lane kernel on one workgroup (sources beyond its LDS copy) and on four.
    The system is far[1e4]'s (cond 1.5e14, E_orc 4e-10 m over the orders of its sums): compared as E over the source points"""
    sc = gs.scene("sizes[3073]")
    T1, s1 = _step(sc, "lanes8_wg1")
    T4, s4 = _step(sc, "lanes8_gc0")
    e = gl.step_error(T1, T4, sc.source)
    print(f"sizes[3073] one workgroup against four: E {e['E']:.3e} dt {e['dt']:.3e} dr {e['dr']:.3e}")
    rep.record("sizes[3073]", "lanes8_wg1", "launch_shapes", E_to_four_workgroups=e["E"], dt=e["dt"], dr=e["dr"])
    for key in ("n_src", "iterations", "n_corr_last", "sum_cand"):
        assert s1[key] == s4[key], key
    assert e["E"] <= 1e-10, e
