"""top2_update() of csrc/top2.h - what a lane of the voxel scan keeps of the stored points it has seen: its two nearest under
(squared distance, then id) and the smallest distance of the rest - against the sequential three-branch rule it replaced
(tests/helpers/top2_probe.py reference()), bit for bit in every field: bd, border, bp, b2d, b2o, b2p, sd.  The host compile and
the gfx950 compile of the same header (tests/hip/top2_probe.hip), at the widths scan_voxelsL calls it with: 12 slots (4 voxels x
3 chunks), 6 (2 x 3) and 1 (the loop over stored points of voxels with more than 24).

The function does not form distances: a slot comes with its d2, so the cases choose d2 freely - exact ties included.  Every active
slot has a position of its own that spells its id, an inactive slot a poisoned one with the smallest distance and id of the case:
whatever is selected wrongly shows.
"""
import itertools

import numpy as np
import pytest

from tests.helpers import top2_probe
from tests.helpers.top2_probe import DBL_MAX, EMPTY, NO_ID, NSTATE

SIDES = ["host", pytest.param("device", marks=pytest.mark.gpu)]
POISON = [-9.0, -9.0, -9.0, 0.0, 0.0, 0.0]  # an inactive slot: nearer than anything, id 0 - it must lose all the same


@pytest.fixture(scope="session")
def probe(tmp_path_factory):
    return top2_probe.build(tmp_path_factory.mktemp("top2_probe"))


def pos(pid):
    return [pid + 0.25, -pid - 0.5, pid * 0.125]


def slot(d2, pid):
    return pos(pid) + [float(d2), float(pid), 1.0]


def state(kind, d=(0.5, 0.75, 1.25), ids=(13 * 32 + 3, 22 * 32 + 9)):
    """incoming states: 'empty', 'one' candidate seen, 'two', and 'sd' (three or more seen: a finite sd)"""
    s = EMPTY.copy()
    if kind in ("one", "two", "sd"):
        s[0], s[3], s[5:8] = d[0], ids[0], pos(ids[0])
    if kind in ("two", "sd"):
        s[1], s[4], s[8:11] = d[1], ids[1], pos(ids[1])
    if kind == "sd":
        s[2] = d[2]
    return s


KINDS = ("empty", "one", "two", "sd")


def row(st, slots, width, where=None):
    """one input: the state and `slots` at the positions `where` (default: the first ones) of `width`, the others inactive"""
    where = range(len(slots)) if where is None else where
    body = [POISON] * width
    for w, s in zip(where, slots):
        body[w] = s
    return np.concatenate([st, np.array(body, dtype=np.float64).ravel()])


def check(probe, side, width, x):
    x = np.array(x)
    ref = top2_probe.reference(x, width)
    out = probe.run(width, side, x)
    same = out.view(np.uint64) == ref.view(np.uint64)
    bad = np.flatnonzero(~same.all(axis=1))
    assert len(bad) == 0, (side, width, len(bad), int(bad[0]), x[bad[0]].tolist(), out[bad[0]].tolist(), ref[bad[0]].tolist())
    assert not (out[:, 5:] == -9.0).any()  # nothing of an inactive slot anywhere
    return ref


def test_reference_takes_every_branch():
    """the restated rule on the hand-made states: each of its three bodies, and nothing for an inactive slot"""
    st = state("sd")
    r = top2_probe.reference(np.array([row(st, [slot(0.25, 7)], 1), row(st, [slot(0.6, 7)], 1), row(st, [slot(1.0, 7)], 1),
                                       row(st, [slot(2.0, 7)], 1), row(st, [], 1)]), 1)
    assert r[0].tolist() == [0.25, 0.5, 0.75, 7, st[3], *pos(7), *st[5:8]]
    assert r[1].tolist() == [0.5, 0.6, 0.75, st[3], 7, *st[5:8], *pos(7)]
    assert r[2].tolist() == [0.5, 0.75, 1.0, *st[3:]]
    assert r[3].tolist() == st.tolist() and r[4].tolist() == st.tolist()
    e = top2_probe.reference(np.array([row(state("empty"), [slot(3.0, 40)], 1)]), 1)[0]
    assert e.tolist() == [3.0, DBL_MAX, DBL_MAX, 40, NO_ID, *pos(40), 0, 0, 0]


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("width", [12, 6])
def test_every_activity_mask(probe, side, width):
    """0 to `width` active slots in every position (all 2^width masks), on each kind of incoming state; the distances of a case
    are drawn around those of the state, so that slots land before the best, between the two, between second and sd, and behind"""
    rng = np.random.default_rng(2501 + width)
    x = []
    for mask in range(1 << width):
        where = [w for w in range(width) if mask >> w & 1]
        d = rng.integers(1, 48, len(where)) / 32.0
        ids = rng.permutation(27 * 32)[: len(where)] + 1000
        x.append(row(state(KINDS[mask % 4]), [slot(a, b) for a, b in zip(d, ids)], width, where))
    ref = check(probe, side, width, x)
    assert (ref[:, 2] < DBL_MAX).sum() > (1 << width) // 2


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("width", [12, 6])
def test_every_permutation_of_five(probe, side, width):
    """five candidates in all 120 orders: distinct distances, and distance multisets with ties (the id decides); the answer is the
    same for every order"""
    rng = np.random.default_rng(2502)
    for dist in ([5, 3, 1, 4, 2], [2, 2, 1, 1, 3], [1, 1, 1, 2, 2], [4, 4, 4, 4, 4], [1, 2, 2, 2, 2]):
        cands = [slot(d / 4.0, 300 + 7 * j) for j, d in enumerate(dist)]
        for kind in KINDS:
            st = state(kind, d=(0.375, 0.5, 1.0))
            x = []
            for perm in itertools.permutations(range(5)):
                where = sorted(rng.permutation(width)[:5].tolist())
                x.append(row(st, [cands[p] for p in perm], width, where))
            ref = check(probe, side, width, x)
            assert (ref.view(np.uint64) == ref[0].view(np.uint64)).all(), (dist, kind)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("width", [12, 6, 1])
def test_ties_on_distance(probe, side, width):
    """equal distances with different ids in two and three candidates, every order; and one candidate that ties the incoming best,
    or the incoming second, on distance with a lower and with a higher id"""
    x = []
    if width > 1:
        for n in (2, 3):
            for ids in itertools.permutations([100, 228, 356][:n]):
                for kind in KINDS:
                    for d in (0.25, 0.5, 0.625, 0.75, 1.0, 1.25, 2.0):  # before, at and between the state's 0.5 / 0.75 / 1.25
                        x.append(row(state(kind), [slot(d, i) for i in ids], width, range(width - n, width)))
    for kind in ("one", "two", "sd"):
        st = state(kind)
        for which in (0, 1):  # tie with the best / the second
            if st[which] == DBL_MAX:
                continue
            for pid in (st[3 + which] - 1, st[3 + which] + 1, 5.0, 800.0):
                x.append(row(st, [slot(st[which], pid)], width, [width - 1]))
        x.append(row(state(kind, d=(0.5, 0.5, 0.5)), [slot(0.5, 5)], width))      # everything at one distance
        x.append(row(state(kind, d=(0.5, 0.5, 0.5)), [slot(0.5, 900)], width))
    check(probe, side, width, x)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("width", [12, 6, 1])
def test_seeded_random_draws(probe, side, width):
    """4000 draws: distances from a grid of 12 values (ties abound) or continuous, any activity, ids as the scan forms them
    (voxel * 32 + index, a voxel scanned once), states that a scan of earlier voxels would have left"""
    rng = np.random.default_rng(2503 + width)
    x = []
    for n in range(4000):
        draw = (lambda k: rng.integers(1, 13, k) / 8.0) if n % 2 else (lambda k: rng.uniform(0.0, 1.5, k))
        ids = rng.permutation(27 * 32)
        seen = int(rng.integers(0, 5))  # the state: what `seen` earlier candidates leave behind an empty one
        st = top2_probe.reference(row(EMPTY, [slot(a, b) for a, b in zip(draw(seen), ids[:seen])], 4), 4)[0]
        where = np.flatnonzero(rng.random(width) < rng.random())
        x.append(row(st, [slot(a, b) for a, b in zip(draw(len(where)), ids[4: 4 + len(where)])], width, where))
    ref = check(probe, side, width, x)
    assert (ref[:, 0] == ref[:, 1]).sum() > 20  # the two nearest tie on distance often enough
