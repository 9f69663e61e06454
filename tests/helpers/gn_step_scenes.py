"""Seeded scenes for one (or two) Gauss-Newton steps, each with its long-double reference (tests/helpers/gn_longdouble.py), built once per
process and replayed by every consumer: tests/test_gn_step_cpu.py asserts what the scenes claim, tests/test_gpu_gn_step.py holds the device
against them.  Voxel size 0.7, 20 points per voxel.

  far[o], far[o]s    the room of test_gpu_parity._room_points with a box of 0.27 of its size in the middle (map: one draw of 55 000 + 4 000;
                     source: two down-samplings of a second draw of 60 000 + 6 000, cut to 3 090 points)
                     with room and sensor moved by o (1, -0.7, 0.1), o = 0, 1e3, 1e4, 1e5 m; the guess is that offset times a seeded twist of
                     (0.05 m, 0.01 rad) about the cloud's centre at sigma = 2.0, and of (0.005 m, 0.0005 rad) at sigma = 0.05 (the "s" scenes)
  turned             far[1e4] under test_gpu_parity._rotated_world: the guess's rotation is 170 degrees from the identity
  weights[s]         far[0] with initial_threshold 0.02 and 20 (gates 0.06 and 60 m) and the small twist; weights[0.8]: 40 sources with one target
                     each at residuals from 0.02 m to the far corner of the 27 voxels, 2.37 m: weights from 1 down to 2e-3 in one sum
  bigstep[a]         40 sources within 0.4 m of an axis, 1.9 m apart along it, and a map of one target each, placed where the linearised
                     system has the exact solution (v, omega), |omega| = a = 0.049, 0.051, 0.3, 0.49, 1.0 rad: t = s + v + omega x s.  The step is
                     that twist by construction (to the rounding of the targets), on either side of se3_exp_gn's series switch at 0.05 rad
  few[...]           1, 2 and 3 sources in reach of the map plus 8 with 27 empty voxels; 40 collinear sources; 40 coincident ones; 40 within
                     1 mm of a line.  Non-dyadic coordinates, residuals of 0.05 m (0.4 m on the third source of few[3], which leaves the line to
                     make rank 6), sigma 2.0.  Ranks 3, 5, 6, 5, 3, 6
  sizes[N]           far[1e4] cut to its first N sources, N around the chunk (64), queue-region (512) and LDS (3 072) sizes of the 8-lane kernel

The guard is a condition: a source point stays only if, in the reference's run of every step the scene is used for, its nearest and
second-nearest candidates differ by >= 1e-6 m, its nearest distance and the gate by >= 1e-6 m, and it is >= 1e-6 m from every voxel face.
Points that fail are removed here, before any implementation sees the scene: at most 2 % of a scene's sources, and none of few[...].

The oracle spread (E_orc, the largest sum error) is the C oracle on 16 seeded permutations of the source: a permutation changes the association
of its sums and nothing else.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import cpu as orc
from tests.helpers import gn_longdouble as gl

VS, CAP = 0.7, 20
DIRECTION = np.array([1.0, -0.7, 0.1])
OFFSETS = (0.0, 1e3, 1e4, 1e5)
MARGIN = 1e-6
N_ORDERS = 16
SIZES = (1, 63, 64, 65, 511, 512, 513, 3071, 3072, 3073)
BIG_ANGLES = (0.049, 0.051, 0.3, 0.49, 1.0)
SEED = 2101
# the room's walls alone fill 2 922 voxels of the second down-sampling however many points are drawn, and sizes[3073] needs more sources than
# that: a box of 0.27 of the room's size stands in the middle of it (map and source alike), and the source is cut to 3 090
INNER_BOX = 0.27
SOURCE_POINTS = 3090


def okey(o):
    return "0" if o == 0 else f"1e{int(round(np.log10(o)))}"


@dataclass
class Scene:
    name: str
    stored: np.ndarray            # the map's stored points: the oracle's export after add_points(map_in)
    map_in: np.ndarray            # what goes into map_add / add_points
    source: np.ndarray            # sensor frame, fp64; the guard has been applied
    guess: np.ndarray             # 4 x 4 fp64
    sigma: float
    steps: int                    # steps the guard covers (1 or 2)
    removed: int                  # sources the guard took out
    ref: dict = field(repr=False, default=None)   # gl.register(..., steps=steps)
    table: gl.MapTable = field(repr=False, default=None)
    via_align: bool = False       # the source does not survive the down-samplings of register_frame (coincident points)

    @property
    def max_dist(self):
        return 3.0 * self.sigma

    @property
    def kernel(self):
        return self.sigma / 3.0

    @property
    def world64(self):
        """the fp64 world-frame source linear_system is given: the reference's, rounded"""
        return np.ascontiguousarray(self.ref["steps"][0]["world"].astype(np.float64))

    @functools.cached_property
    def lin(self):
        """the reference's system of exactly that fp64 input (the sums linear_system returns are held against this one; the pairs are the
        first step's: the guard's margin is five orders above the rounding of the input, and the oracle's targets confirm it)"""
        c = self.ref["steps"][0]["corr"]
        return gl.system(self.world64, c["target"], c["paired"], self.kernel)


def _se3(xi):
    return orc.se3_exp(np.asarray(xi, dtype=np.float64))


def _trans(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def _twist(rng, dt, dr):
    a, b = rng.normal(size=3), rng.normal(size=3)
    return np.concatenate([dt * a / np.linalg.norm(a), dr * b / np.linalg.norm(b)])


def _apply64(T, p):
    return p @ T[:3, :3].T + T[:3, 3]


@functools.lru_cache(maxsize=None)
def room():
    """(map draw, source): the room about the origin; the source is one point per 1.05 m voxel, so register_frame's own down-samplings keep it"""
    from tests.test_gpu_parity import _room_points
    rng = np.random.default_rng(SEED)
    m = np.concatenate([_room_points(rng, 55000), INNER_BOX * _room_points(rng, 4000)])
    draw = np.concatenate([_room_points(rng, 60000), INNER_BOX * _room_points(rng, 6000)])
    s = orc.voxel_downsample(orc.voxel_downsample(draw, 0.5 * VS), 1.5 * VS)[:SOURCE_POINTS]
    assert len(s) == SOURCE_POINTS, len(s)
    assert np.array_equal(orc.voxel_downsample(orc.voxel_downsample(s, 0.5 * VS), 1.5 * VS), s)
    return m, s


def _build(name, map_in, source, guess, sigma, steps, max_loss=0.02, via_align=False):
    """export the map through the oracle, run the reference, drop the sources the guard rejects (and run again: a smaller source is another
    step) until none is left"""
    m = orc.Map(VS, 1e9, CAP)
    m.add_points(map_in)
    stored = m.points()
    assert len(stored) <= 60000
    table = gl.MapTable(stored, VS, CAP)
    n0 = len(source)
    for _ in range(6):
        ref = gl.register(source, guess, table, 3.0 * sigma, sigma / 3.0, steps=steps)
        bad = np.zeros(len(source), bool)
        for st in ref["steps"]:
            bad |= gl.guard_fails(st["corr"], MARGIN)
        if not bad.any():
            break
        source = np.ascontiguousarray(source[~bad])
    else:
        raise AssertionError(f"{name}: the guard does not settle")
    removed = n0 - len(source)
    assert removed <= max_loss * n0, (name, removed, n0)
    return Scene(name, stored, np.ascontiguousarray(map_in), np.ascontiguousarray(source), guess, sigma, steps, removed, ref, table, via_align)


# ------------------------------------------------------------------------------------------------ the room, far from the origin
def _far_inputs(o, small):
    m, s = room()
    rng = np.random.default_rng(SEED + 1 + int(small))
    tw = _twist(rng, 0.005, 0.0005) if small else _twist(rng, 0.05, 0.01)
    return m + o * DIRECTION, s, _trans(o * DIRECTION) @ _se3(tw)


@functools.lru_cache(maxsize=None)
def far(o, small=False):
    mp_, s, g = _far_inputs(o, small)
    return _build(f"far[{okey(o)}]" + ("s" if small else ""), mp_, s, g, 0.05 if small else 2.0, 2 if (o < 1e5 and not small) else 1)


@functools.lru_cache(maxsize=None)
def turned():
    from tests.test_gpu_parity import _rotated_world
    mp_, s, g = _far_inputs(1e4, False)
    W = _rotated_world()
    return _build("turned", _apply64(W, mp_), s, W @ g, 2.0, 2)


@functools.lru_cache(maxsize=None)
def weights(sigma):
    mp_, s, g = _far_inputs(0.0, True)
    return _build(f"weights[{sigma:g}]", mp_, s, g, sigma, 1)


WIDE_SIGMA = 0.8   # gate 2.4 m, k = 0.267: r^2 / k reaches 21 at the far corner of the 27 voxels, the most any threshold allows at 0.7 m voxels


@functools.lru_cache(maxsize=None)
def weights_wide():
    """40 sources 0.01 m inside the low corner of their voxels, 6.3 m apart on a 4 x 4 x 3 lattice of positive coordinates, and a map of one
    target each at residuals from 0.02 m to 2.37 m (a geometric ladder): up to 0.7 m in seeded directions, beyond that along (1, 1, 1), where
    the neighbouring voxel still holds a target 1.37 m away on every axis.  Weights from 1 down to (k / (k + r^2))^2 = 2e-3 in one sum"""
    rng = np.random.default_rng(SEED + 30)
    ijk = np.array([(a, b, c) for a in range(4) for b in range(4) for c in range(3)][:STATIONS], dtype=np.float64)
    s = (10.0 + 9.0 * ijk) * VS + np.array([0.013, 0.017, 0.011])
    rho = 0.02 * (2.37 / 0.02) ** (np.arange(STATIONS) / (STATIONS - 1.0))
    d = np.where((rho <= 0.7)[:, None], _unit(rng, STATIONS), np.ones(3) / np.sqrt(3.0))
    return _build(f"weights[{WIDE_SIGMA:g}]", s + rho[:, None] * d, s, np.eye(4), WIDE_SIGMA, 1, max_loss=0.0)


@functools.lru_cache(maxsize=None)
def sizes(n):
    f = far(1e4)
    src = np.ascontiguousarray(f.source[:n])
    assert len(src) == n, (n, len(f.source))
    return _build(f"sizes[{n}]", f.map_in, src, f.guess, 2.0, 1, max_loss=0.0)


# ------------------------------------------------------------------------------------------------ sources about an axis
AXIS_C = np.array([3.1, -2.3, 1.7])
AXIS_D = np.array([0.62, 0.53, 0.58]) / np.linalg.norm([0.62, 0.53, 0.58])
STATIONS = 40
SPACING = 1.9   # > 1.05 sqrt(3): no two stations share a voxel of the second down-sampling


def _stations(rng, radius):
    """40 points along the axis, `radius` (a scalar or per-station bounds) off it in seeded directions"""
    along = AXIS_C + np.outer((np.arange(STATIONS) - 0.37 * STATIONS) * SPACING, AXIS_D)
    q = rng.normal(size=(STATIONS, 3))
    q -= np.outer(q @ AXIS_D, AXIS_D)
    q /= np.linalg.norm(q, axis=1)[:, None]
    return along + q * np.reshape(radius, (-1, 1))


def _unit(rng, n):
    q = rng.normal(size=(n, 3))
    return q / np.linalg.norm(q, axis=1)[:, None]


@functools.lru_cache(maxsize=None)
def bigstep(angle):
    """the linearised system has the exact solution (v, omega): omega = angle * axis, v = -omega x c, so that r = -(omega x (s - c)) stays below
    0.4 m * angle.  The sources go in through the identity guess"""
    rng = np.random.default_rng(SEED + 10)
    s = _stations(rng, rng.uniform(0.05, 0.4, STATIONS))
    omega = angle * AXIS_D
    v = -np.cross(omega, AXIS_C) + np.array([0.011, -0.007, 0.003])
    t = s + v + np.cross(omega, s)
    return _build(f"bigstep[{angle:g}]", t, s, np.eye(4), 2.0, 2, max_loss=0.0)


@functools.lru_cache(maxsize=None)
def _few_parts():
    rng = np.random.default_rng(SEED + 20)
    on_line = _stations(rng, 0.0)
    near_line = _stations(rng, rng.uniform(2e-4, 1e-3, STATIONS))
    res = 0.05 * _unit(rng, STATIONS)
    empty = _stations(rng, 12.0)[:8]           # 12 m off the axis: nothing stored within 17 voxels
    return on_line, near_line, on_line + res, empty


FEW = ("1", "2", "3", "collinear", "coincident", "nearline")
FEW_RANK = {"1": 3, "2": 5, "3": 6, "collinear": 5, "coincident": 3, "nearline": 6}
FEW_PAIRS = {"1": 1, "2": 2, "3": 3, "collinear": 40, "coincident": 40, "nearline": 40}


@functools.lru_cache(maxsize=None)
def few(kind):
    on_line, near_line, map_in, empty = _few_parts()
    rng = np.random.default_rng(SEED + 21)
    if kind in ("1", "2", "3"):
        n = int(kind)
        idx = [5, 17, 30][:n]
        src = near_line[idx] + (np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.31, -0.27, 0.12]])[:n])  # (the third leaves the line: rank 6)
        src = np.concatenate([src, empty])
    elif kind == "collinear":
        src = on_line
    elif kind == "coincident":
        src = np.repeat(on_line[11:12] + 0.01 * _unit(rng, 1), STATIONS, axis=0)
    else:
        src = near_line
    return _build(f"few[{kind}]", map_in, np.ascontiguousarray(src), np.eye(4), 2.0, 1, max_loss=0.0, via_align=(kind == "coincident"))


# ------------------------------------------------------------------------------------------------ the catalogue
def catalogue():
    """name -> builder of every scene, in the order of the tables"""
    c = {}
    for o in OFFSETS:
        c[f"far[{okey(o)}]"] = functools.partial(far, o)
    for o in OFFSETS:
        c[f"far[{okey(o)}]s"] = functools.partial(far, o, True)
    c["turned"] = turned
    for s in (0.02, 20.0):
        c[f"weights[{s:g}]"] = functools.partial(weights, s)
    c[f"weights[{WIDE_SIGMA:g}]"] = weights_wide
    for a in BIG_ANGLES:
        c[f"bigstep[{a:g}]"] = functools.partial(bigstep, a)
    for k in FEW:
        c[f"few[{k}]"] = functools.partial(few, k)
    for n in SIZES:
        c[f"sizes[{n}]"] = functools.partial(sizes, n)
    return c


CATALOGUE = catalogue()
TWO_STEP = ("far[0]", "far[1e3]", "far[1e4]", "turned") + tuple(f"bigstep[{a:g}]" for a in BIG_ANGLES)


def scene(name):
    return CATALOGUE[name]()


# ------------------------------------------------------------------------------------------------ bounds and the oracle's spread
# Roundings of one term w * dot(col_a, col_b) of a sum, relative to the term's absolute-value shadow, first order in 2^-53:
#   w = k2 / (den * den), den = k + (rx rx + ry ry + rz rz), r = s - t, k2 = k * k
#     k2: 1.  r_i: 1 each, so r_i r_i: 2 + 1 (product).  The two additions: 2.  r2 <= 5.  den = k + r2 (positive terms): 5 + 1 = 6.
#     den * den: 12 + 1 = 13.  The quotient: 13 + 1 (k2) + 1 (division) = 15
#   dot(col_a, col_b): at most two non-zero products (1 each) and one addition that is not with 0.0 (1); in JTr the column r brings its own
#     rounding (1): 3 at most
#   w * dot: 1
# c = 15 + 3 + 1 = 19.  The C oracle forms (J w) J per row instead of w (J . J): the same count.  Adding n such terms in any order adds at
# most n - 1 <= n_pairs roundings of a partial sum that the shadow bounds: |S - S_ref| <= (n_pairs + c) 2^-53 T
C_TERM = 19


def sum_bound(sysd):
    """per entry (27,) fp64: (n_pairs + C_TERM) 2^-53 T (the running-error bound; any order of summation)"""
    return ((sysd["n_pairs"] + C_TERM) * gl.U * sysd["shadow"]).astype(np.float64)


def sum_fraction(sums, sysd):
    """largest |S - S_ref| / bound over the 27 entries (entries whose shadow is 0 must be exact)"""
    err = np.abs((np.asarray(sums, dtype=gl.LD) - sysd["sums"]).astype(np.float64))
    b = sum_bound(sysd)
    assert np.all(err[b == 0] == 0), (err, b)
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


def orders(n):
    """the identity and 15 seeded permutations of n sources"""
    rng = np.random.default_rng(SEED + 99)
    return [np.arange(n)] + [rng.permutation(n) for _ in range(N_ORDERS - 1)]


def oracle_map(sc):
    m = orc.Map(VS, 1e9, CAP)
    m.add_points(sc.map_in)
    return m


def dx_of(pose, sc):
    """Log(pose * as_se3(guess)^-1): the step an implementation took, from its pose"""
    return gl.log_se3(gl.mul(np.asarray(pose, dtype=gl.LD), gl.inv_rigid(sc.ref["guess_se3"])))


@functools.lru_cache(maxsize=None)
def oracle_spread(name, steps=1):
    """the C oracle over the 16 orders.  dict(E: the largest step error against the reference's `steps`-step pose; sum_fraction: the
    largest share of the sum bound (first step); residual: the largest |JTJ_ref dx + JTr_ref| (first step, steps == 1); poses; targets_equal)"""
    sc = scene(name)
    assert steps <= sc.steps
    ref_pose = sc.ref["pose"] if steps == sc.steps else gl.mul(sc.ref["steps"][0]["exp"], sc.ref["guess_se3"])
    m = oracle_map(sc)
    st0 = sc.ref["steps"][0]
    w64 = sc.world64
    E, frac, res, poses, same = 0.0, 0.0, 0.0, [], True
    for p in orders(len(sc.source)):
        sums, nc, cand, tgt = m.linear_system(w64[p], sc.max_dist, sc.kernel, want_targets=True)
        same &= bool(np.array_equal(tgt, st0["corr"]["target"][p], equal_nan=True)) and nc == st0["sys"]["n_pairs"] and cand == st0["corr"]["n_cand"]
        frac = max(frac, sum_fraction(sums, sc.lin))
        pose, it, _, _ = m.register(sc.source[p], sc.guess, sc.max_dist, sc.kernel, max_iter=steps, conv=0.0)
        assert it == steps
        poses.append(pose)
        E = max(E, gl.step_error(pose, ref_pose, sc.source)["E"])
        if steps == 1:
            res = max(res, gl.residual(st0["sys"]["sums"], dx_of(pose, sc)))
    return dict(E=E, sum_fraction=frac, residual=res, poses=poses, targets_equal=same, ref_pose=ref_pose)


def floor():
    """E_orc of far[0]: what two correct fp64 implementations differ by where nothing is ill-conditioned"""
    return oracle_spread("far[0]")["E"]


FACTOR = 4.0  # DESIGN.md 3.15.2's: two correct fp64 implementations differ from the truth by roundings of the same order


def step_bound(name, steps=1):
    return FACTOR * oracle_spread(name, steps)["E"] + floor()
