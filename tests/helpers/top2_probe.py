"""Builds tests/hip/top2_probe.hip (top2_update() of csrc/top2.h on the host and in a kernel, one input per thread) with the
compiler, target and code-generation flags of the product Makefile, and loads it with ctypes; and restates the sequential
three-branch rule the function replaces (reference())."""
import ctypes
import os
import subprocess

import numpy as np

from tests.helpers.devmath_probe import ROOT, makefile_toolchain

SOURCE = os.path.join(ROOT, "tests", "hip", "top2_probe.hip")
WIDTHS = (12, 6, 1)
NSTATE = 11          # bd, b2d, sd, border, b2o, bp xyz, b2p xyz
DBL_MAX = float(np.finfo(np.float64).max)
NO_ID = float(0xFFFFFFFF)
EMPTY = np.array([DBL_MAX, DBL_MAX, DBL_MAX, NO_ID, NO_ID, 0, 0, 0, 0, 0, 0], dtype=np.float64)


class Probe:
    def __init__(self, path):
        self.path = path
        self.lib = ctypes.CDLL(path)
        for w in WIDTHS:
            for side in ("host", "device"):
                fn = getattr(self.lib, f"probe_top2_w{w}_{side}")
                fn.restype = ctypes.c_int
                fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
            assert getattr(self.lib, f"probe_top2_w{w}_ni")() == NSTATE + 6 * w
            assert getattr(self.lib, f"probe_top2_w{w}_no")() == NSTATE

    def run(self, width, side, x):
        """x: (n, 11 + 6 width) float64 -> (n, 11) float64 from the host loop (side='host') or the kernel (side='device')."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, NSTATE + 6 * width)
        out = np.full((len(x), NSTATE), np.nan)
        rc = getattr(self.lib, f"probe_top2_w{width}_{side}")(len(x), x.ctypes.data, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"probe_top2_w{width}_{side}: hipError_t {rc}")
        return out


def build(outdir):
    hipcc, flags = makefile_toolchain()
    so = os.path.join(str(outdir), "libtop2_probe.so")
    subprocess.run([hipcc, *flags, "-o", so, SOURCE], check=True)
    return Probe(so)


def reference(x, width):
    """The rule of the voxel scan before top2.h, slot after slot in the order given, on one row per case (layout of the probe):
         if (act) { if (c < best) {...} else if (c < second) {...} else sd = fmin(sd, d2); }   with c < x under (distance, id)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, NSTATE + 6 * width)
    out = np.empty((len(x), NSTATE))
    for n, row in enumerate(x):
        bd, b2d, sd, border, b2o = (float(v) for v in row[:5])
        bp, b2p = row[5:8].copy(), row[8:11].copy()
        for j in range(width):
            px, py, pz, d2, pid, act = (float(v) for v in row[NSTATE + 6 * j: NSTATE + 6 * j + 6])
            if not act:
                continue
            if d2 < bd or (d2 == bd and pid < border):
                sd = min(sd, b2d)
                b2d, b2o, b2p = bd, border, bp
                bd, border, bp = d2, pid, np.array([px, py, pz])
            elif d2 < b2d or (d2 == b2d and pid < b2o):
                sd = min(sd, b2d)
                b2d, b2o, b2p = d2, pid, np.array([px, py, pz])
            else:
                sd = min(sd, d2)
        out[n] = [bd, b2d, sd, border, b2o, *bp, *b2p]
    return out
