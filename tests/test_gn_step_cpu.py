"""What the scenes of tests/helpers/gn_step_scenes.py claim, from the long-double reference alone, and the C oracle's spread over 16 orders of
every source: no GPU.  tests/test_gpu_gn_step.py holds the device against the same arrays and the same bounds.
"""
import numpy as np
import pytest

import ptudes_lab_amd  # noqa: F401  (import shim)
from oracle import cpu as orc
from oracle import icp_numpy as inp
from tests.helpers import gn_longdouble as gl
from tests.helpers import gn_step_scenes as gs

ALL = list(gs.CATALOGUE)
ROOM = [n for n in ALL if n.startswith(("far", "turned", "weights"))]

# pairs of the first step (and of the second where the scene is used for two): the reference's, written down
PAIRS = {"far[0]": (3090, 3090), "far[1e3]": (3090, 3090), "far[1e4]": (3090, 3090), "far[1e5]": (3090,), "far[0]s": (1718,), "far[1e3]s": (1733,),
         "far[1e4]s": (1730,), "far[1e5]s": (1732,), "turned": (3090, 3090), "weights[0.02]": (435,), "weights[20]": (3090,), "weights[0.8]": (40,)}
COND = {"0": 2.8e2, "1e3": 1.5e10, "1e4": 1.5e14}  # (measured with the C oracle's sums on the bare room; 1e5: > 1e16)


def _first(name):
    return gs.scene(name).ref["steps"][0]


@pytest.mark.parametrize("name", ALL)
def test_sizes_guard_and_invariance_under_the_down_samplings(name):
    sc = gs.scene(name)
    assert len(sc.stored) <= 60000 and len(sc.source) <= 3100
    n0 = len(sc.source) + sc.removed
    assert sc.removed <= 0.02 * n0 and (sc.removed == 0 or not name.startswith(("few", "sizes", "bigstep"))), (name, sc.removed)
    for st in sc.ref["steps"]:  # the guard holds on what is left, in every step the scene is used for
        c = st["corr"]
        assert not gl.guard_fails(c, gs.MARGIN).any()
        assert c["face"].min() >= gs.MARGIN and c["gap_gate"][c["found"]].min(initial=np.inf) >= gs.MARGIN
        assert c["gap_second"][c["paired"]].min(initial=np.inf) >= gs.MARGIN
    if not sc.via_align:  # register_frame's range filter and two down-samplings hand the kernel exactly this source
        assert np.array_equal(orc.voxel_downsample(orc.voxel_downsample(sc.source, 0.5 * gs.VS), 1.5 * gs.VS), sc.source)
        assert np.linalg.norm(sc.source, axis=1).min() > 0.0
    else:
        assert len(orc.voxel_downsample(sc.source, 0.5 * gs.VS)) == 1


@pytest.mark.parametrize("name", ROOM)
def test_pair_counts_and_conditioning_of_the_room_scenes(name):
    sc = gs.scene(name)
    assert tuple(st["sys"]["n_pairs"] for st in sc.ref["steps"]) == PAIRS[name]
    sol = _first(name)["sol"]
    assert sol["rank"] == 6
    if name.startswith("far"):
        o = name[4:name.index("]")]
        if o == "1e5":
            assert sol["cond"] > 1e16
        else:
            assert COND[o] / 3 <= sol["cond"] <= COND[o] * 3, sol["cond"]
    if name == "turned":  # the guess's rotation is far from the identity: as_se3 takes a branch of the largest diagonal entry
        R = sc.guess[:3, :3]
        assert np.trace(R) < 0 and 1e14 / 3 <= sol["cond"] <= 1e15


def test_weights_span_what_the_search_allows():
    """r < min(gate, reach of the 27 voxels) and k = sigma / 3 bound k / (k + r^2) from below: the smallest weight of a step is 0.43 of its
    largest at sigma = 0.02 (gate 0.06 m: r^2 / k up to 0.54) and 0.91 at sigma = 20; a weight of (k / (k + r^2))^2 = 1e-4 would
    need r^2 = 99 k, which no sigma reaches with 0.7 m voxels (r^2 / k <= min(27 sigma, 3 * 5.9 / sigma) <= 22).  weights[0.8] goes to that
    limit on a sparse map: residuals up to 2.37 m under a gate of 2.4 m, the smallest weight 2e-3 of the largest"""
    for s, lo, hi in ((0.02, 0.40, 0.45), (20.0, 0.90, 0.93), (0.8, 1.9e-3, 2.2e-3)):
        w = _first(f"weights[{s:g}]")["sys"]["w"]
        assert lo <= float(w.min() / w.max()) <= hi, (s, float(w.min() / w.max()))
        assert float(w.max()) <= 1.0


@pytest.mark.parametrize("angle", gs.BIG_ANGLES)
def test_bigstep_takes_the_step_it_was_built_for(angle):
    sc = gs.bigstep(angle)
    dx = sc.ref["steps"][0]["sol"]["dx"].astype(np.float64)
    assert abs(np.linalg.norm(dx[3:]) - angle) <= 1e-9 and np.abs(dx[3:] - angle * gs.AXIS_D).max() <= 1e-9
    assert (np.linalg.norm(dx[3:]) < 0.05) == (angle < 0.05)
    assert [st["sys"]["n_pairs"] for st in sc.ref["steps"]] == [gs.STATIONS, gs.STATIONS]
    assert np.linalg.norm(sc.ref["steps"][1]["sol"]["dx"].astype(np.float64)) > 1e-4 * angle  # the second step has work left: Exp is not I + hat


@pytest.mark.parametrize("kind", gs.FEW)
def test_few_ranks_and_pairs(kind):
    sc = gs.few(kind)
    st = sc.ref["steps"][0]
    assert st["sys"]["n_pairs"] == gs.FEW_PAIRS[kind] and st["sol"]["rank"] == gs.FEW_RANK[kind]
    assert st["sol"]["null"].shape == (6, 6 - gs.FEW_RANK[kind])
    if kind in "123":
        assert len(sc.source) == int(kind) + 8 and int((~st["corr"]["found"]).sum()) == 8  # 8 sources with 27 empty voxels
    res = np.sqrt(((st["sys"]["s"] - st["sys"]["t"]) ** 2).sum(axis=1)).astype(np.float64)
    assert res.max() <= (0.5 if kind == "3" else 0.07) and res.min() >= 0.03
    A, g = gl.unpack(st["sys"]["sums"])
    if gs.FEW_RANK[kind] < 6:  # the minimum-norm step solves the system, is orthogonal to the null space, and the null space is one
        assert gl.residual(st["sys"]["sums"], st["sol"]["minnorm"]) <= 1e-15 * max(1.0, float(np.abs(g).max()))
        assert float(np.abs(st["sol"]["null"].T @ st["sol"]["minnorm"]).max()) <= 1e-15
        assert float(np.abs(A @ st["sol"]["null"]).max()) <= 1e-12 * float(np.abs(A).max())
        assert float(np.sqrt((st["sol"]["minnorm"] ** 2).sum())) < 0.2
    else:
        assert float(np.sqrt((st["sol"]["dx"][3:] ** 2).sum())) > (1.0 if kind == "nearline" else 0.0)  # near a line: a step of radians


@pytest.mark.parametrize("n", gs.SIZES)
def test_sizes_are_cuts_of_far_1e4(n):
    sc, f = gs.sizes(n), gs.far(1e4)
    assert len(sc.source) == n and np.array_equal(sc.source, f.source[:n]) and np.array_equal(sc.stored, f.stored)
    assert sc.ref["steps"][0]["sys"]["n_pairs"] == n
    assert sc.ref["steps"][0]["sol"]["rank"] == (3 if n == 1 else 6)
    if n > 1:
        assert 1e14 / 3 <= sc.ref["steps"][0]["sol"]["cond"] <= 1.5e14 * 3


def test_reference_sums_of_far_0_are_the_numpy_restatement_s():
    """the long-double sums against fp64 numpy sums on the same fp64 world-frame source: the search and the map are oracle/icp_numpy.py's
    (VoxelMap, nearest); the weights, J, JTJ and JTr are restated here from the lines of its register(), which keeps them inline.  1e-12 of
    every entry's absolute-value shadow; and the reference's moments give its sums (two associations, both in long double)"""
    sc = gs.far(0.0)
    vm = inp.VoxelMap(gs.VS, 1e9, gs.CAP)
    vm.add(sc.map_in)
    s = sc.world64
    nn, d2, found, ncand = inp.nearest(s, vm.tables(), gs.VS)
    m = found & (np.sqrt(d2) < sc.max_dist)
    c = sc.ref["steps"][0]["corr"]
    assert np.array_equal(m, c["paired"]) and np.array_equal(nn[m], c["target"][m]) and ncand == c["n_cand"]
    sp, r = s[m], s[m] - nn[m]
    w = sc.kernel ** 2 / (sc.kernel + np.sum(r * r, axis=1)) ** 2
    J = np.zeros((len(sp), 3, 6))
    J[:, :, :3] = inp.I3
    J[:, 0, 4], J[:, 0, 5] = sp[:, 2], -sp[:, 1]
    J[:, 1, 3], J[:, 1, 5] = -sp[:, 2], sp[:, 0]
    J[:, 2, 3], J[:, 2, 4] = sp[:, 1], -sp[:, 0]
    JTJ = np.einsum("n,nai,naj->ij", w, J, J)
    JTr = np.einsum("n,nai,na->i", w, J, r)
    packed = np.array([JTJ[a, b] for a, b in gl.PAIRS] + list(JTr))
    lin = sc.lin
    err = np.abs((packed.astype(gl.LD) - lin["sums"]).astype(np.float64))
    assert np.all(err <= 1e-12 * lin["shadow"].astype(np.float64)), err / lin["shadow"].astype(np.float64)
    for name in ("far[0]", "far[1e5]", "turned"):
        sy = gs.scene(name).lin
        d = np.abs((gl.sums_from_moments(sy["moments"]) - sy["sums"]).astype(np.float64))
        assert np.all(d <= sy["n_pairs"] * 2.0 ** -62 * sy["shadow"].astype(np.float64)), (name, d)


@pytest.mark.parametrize("name", ALL)
def test_oracle_spread(name):
    """the C oracle on 16 orders of the source: its targets are the reference's on every point (or the guard is too weak), its sums meet the
    running-error bound the device will be asked to meet, and where a step is defined its error is a number, not a wreck"""
    sc = gs.scene(name)
    sp = gs.oracle_spread(name)
    assert sp["targets_equal"]
    assert sp["sum_fraction"] <= 1.0, sp["sum_fraction"]
    if sc.ref["steps"][0]["sol"]["rank"] == 6:
        assert np.isfinite(sp["E"]) and sp["E"] < 1e-6, sp["E"]
    if name in gs.TWO_STEP:
        sp2 = gs.oracle_spread(name, 2)
        assert np.isfinite(sp2["E"]) and sp2["E"] < 1e-6


def test_the_oracle_s_step_error_grows_with_the_distance_from_the_origin():
    """E_orc grows with the square of the distance from the origin; the floor is rounding of the pose itself"""
    E = [gs.oracle_spread(f"far[{gs.okey(o)}]")["E"] for o in gs.OFFSETS]
    assert E[0] < 1e-13 and E[0] < E[1] < E[2] < E[3] and E[3] > 1e-9
    assert gs.floor() == E[0]
