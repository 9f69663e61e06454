"""tests/helpers/search_chain_scenes.py is what it claims (numpy + the CPU oracle, no GPU): what the first search of every source point
meets, and - from the positions of every iteration of the registration, restated with the oracle's pieces - the queue arithmetic of the
8-lane kernel's phase A on a team of two workgroups (blocks of 64 points dealt round robin, 64 searches per pass and workgroup)."""
import numpy as np

import ptudes_lab_amd  # noqa: F401  (import shim)
from tests.helpers import search_chain_scenes as sc


def test_the_scans_are_exact_and_every_point_has_its_cell():
    f0, f1 = sc.frame0(), sc.frame1()
    assert f0.shape == f1.shape == (sc.N, 3) and f0.dtype == np.float32
    src = sc.source()
    assert len(np.unique(np.floor(src / (1.5 * sc.VOXEL_SIZE)), axis=0)) == sc.CELLS  # pass 2 of the down-sampling keeps every one
    m = f0[np.abs(f0).sum(axis=1) > 0].astype(np.float64)
    assert len(np.unique(np.floor(m / (0.5 * sc.VOXEL_SIZE)), axis=0)) == len(m) > 3 * sc.CELLS  # ... and pass 1 every map point
    assert (m > 1.0).all() and (src > 1.0).all() and np.linalg.norm(m, axis=1).max() < sc.MAX_RANGE
    ref = sc.reference()
    assert ref["stats"][1]["n_src"] == sc.CELLS and np.array_equal(ref["source"], src)
    assert ref["stats"][0]["map_points"] == len(m)


def test_what_the_first_search_meets():
    fi, kind = sc.first_iteration(), sc.kinds()
    for name, n in sc.COUNTS.items():
        assert (kind == name).sum() == n
    k = lambda name: kind == name  # noqa: E731
    # exactly three other occupied boxes, the nearest neighbour in the third-nearest: the filled slot supplies the answer
    assert (fi["others"][k("third")] == 3).all() and (fi["rank"][k("third")] == 2).all() and fi["own"][k("third")].all()
    # the nearest neighbour in the fourth-nearest box: a survivor round is still needed
    assert (fi["others"][k("fourth")] == 4).all() and (fi["rank"][k("fourth")] == 3).all()
    # an exact tie between the third box and the own voxel, decided by the order id either way
    assert fi["tie"][k("tie_own")].all() and (fi["nearest_entry"][k("tie_own")] == 13).all() and (fi["others"][k("tie_own")] == 3).all()
    assert fi["tie"][k("tie_box")].all() and (fi["nearest_entry"][k("tie_box")] == 12).all() and (fi["others"][k("tie_box")] == 3).all()
    assert fi["tie"].sum() == sc.COUNTS["tie_own"] + sc.COUNTS["tie_box"]
    # zero, one and two other occupied boxes around a winner in the own voxel
    a = k("anchor")
    assert (fi["rank"][a] == -1).all()
    for n in (0, 1, 2):
        assert (fi["others"][a] == n).sum() > 300
    # one occupied box and 26 empty neighbours: the own voxel, or one of the others
    assert (fi["others"][k("alone")] == 0).all() and fi["own"][k("alone")].all()
    assert (fi["others"][k("one_box")] == 1).all() and not fi["own"][k("one_box")].any()
    # nothing in reach at all, and up to six other boxes
    assert (fi["rank"] == -2).sum() > 20 and (fi["others"] == 6).sum() > 100
    # winners in another voxel: their voxel keeps the second slot in the searches that follow
    assert (fi["rank"] >= 0).sum() > 600


def test_the_queue_arithmetic_of_a_team_of_two():
    its = sc.iterations()
    ref = sc.reference()
    assert len(its) == ref["stats"][1]["iterations"] >= 4
    vox = [np.floor(s / sc.VOXEL_SIZE).astype(np.int64) for s, _ in its]
    wg = (np.arange(sc.CELLS) >> 6) & 1
    spans = 0
    for it in range(1, len(its)):
        crossed = (vox[it] != vox[it - 1]).any(axis=1)  # queued at the back: the row is rebuilt
        # same voxel, another neighbour than an iteration ago: no answer row settles these - queued at the front
        front_at_least = ~crossed & (its[it][1] != its[it - 1][1]).any(axis=1)
        had = np.isfinite(its[it - 1][1]).all(axis=1)  # (a point without a neighbour has no target)
        last_vox = np.floor(np.where(had[:, None], its[it - 1][1], 0.0) / sc.VOXEL_SIZE).astype(np.int64)
        last_elsewhere = had & (last_vox != vox[it]).any(axis=1) & ~crossed
        print(it, "back", [int(crossed[wg == g].sum()) for g in (0, 1)], "front >=", [int(front_at_least[wg == g].sum()) for g in (0, 1)],
              "last winner in another voxel", int(last_elsewhere.sum()))
        if it <= 2:
            assert 40 < crossed.sum() < 500 and front_at_least.sum() > 100 and last_elsewhere.sum() > 300
            # the crossers' neighbours in the same 64-point block keep their voxel
            blocks = np.unique(np.flatnonzero(crossed) >> 6)
            assert all(0 < crossed[64 * b:64 * b + 64].sum() < 64 for b in blocks)
        spans += sum(crossed[wg == g].sum() > 64 for g in (0, 1))
    assert spans >= 1  # the backs of one flush span more than one search pass
    assert (sc.kinds()[(vox[-1] != vox[0]).any(axis=1)] == "crosser").mean() > 0.9
