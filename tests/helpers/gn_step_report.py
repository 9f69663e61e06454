"""Collects the measured errors of the Gauss-Newton step scenes and writes them as JSON when the environment variable
GN_STEP_REPORT names a path:

    GN_STEP_REPORT=OUT.json python -m pytest tests/test_gpu_gn_step.py

tests/test_gpu_gn_step.py calls record() with every figure it asserts on (per scene and form: E_orc, E_dev, their ratio, the sum errors as
fractions of their bounds, the iteration counts, the distances between the poses of the rank-deficient scenes); the file is written when the
process ends.  profiles/r021_gn_step_errors.json is this output."""
import atexit
import json
import os

ENV = "GN_STEP_REPORT"
_rows = {}


def ratio(a, b):
    return float(a / b) if b > 0 else (0.0 if a == 0 else float("inf"))


def record(scene, form, what, **figures):
    """figures of one check (`what`: step, two_steps, converged, sums, deficient, launch_shapes) of one form on one scene"""
    _rows.setdefault(scene, {}).setdefault(form, {})[what] = {k: (v if isinstance(v, (int, str, bool, list, dict)) else float(v)) for k, v in figures.items()}


def scene_facts(scene, **facts):
    _rows.setdefault(scene, {})["scene"] = {k: (v if isinstance(v, (int, str, bool, list)) else float(v)) for k, v in facts.items()}


def write(path):
    with open(path, "w") as fh:
        json.dump(dict(rule="E = max over the source points of |T p - T_ref p| against the long-double reference, metres; step: E_dev <= 4 E_orc + "
                            "floor, E_orc = the C oracle's largest over 16 orders of the source, floor = E_orc of far[0]; sums: |S_dev - S_ref| as "
                            "a fraction of (n_pairs + 19) 2^-53 T, T the absolute-value shadow of the sum", scenes=_rows), fh, indent=1)
        fh.write("\n")


@atexit.register
def _flush():
    if os.environ.get(ENV) and _rows:
        write(os.environ[ENV])
