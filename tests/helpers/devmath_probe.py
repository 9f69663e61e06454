"""Builds tests/hip/devmath_probe.hip (csrc/devmath.h on the host and in a kernel, one input per thread) with the
compiler, target and code-generation flags of the product Makefile, and loads it with ctypes."""
import ctypes
import os
import shlex
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "ptudes-lab_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "hip", "devmath_probe.hip")
FUNCTIONS = ("R_to_quat", "quat_to_R", "rotvec_to_R", "R_to_rotvec", "rot_angle", "rt_project", "mat3_polar", "se3_exp",
             "se3_exp_gn", "se3_log", "rt_inv", "rt_mul", "mat4_inv", "solve6_ldlt")


def makefile_toolchain():
    """(HIPCC, flags) as the product Makefile expands them; the -D switches (code id, kernel geometry) are the library's own."""
    out = subprocess.run(["make", "-C", CSRC, "-s", "--no-print-directory",
                          "--eval", "probe-print: ; @echo $(HIPCC) ; echo $(ARCH) ; echo '$(HIPFLAGS)'", "probe-print"],
                         check=True, capture_output=True, text=True).stdout.splitlines()
    hipcc, arch, flags = out[0].strip(), out[1].strip(), [f for f in shlex.split(out[2]) if not f.startswith("-D")]
    for need in ("-O3", "-std=c++17", "-ffp-contract=off", f"--offload-arch={arch}"):
        assert need in flags, (need, flags)
    return hipcc, flags


class Probe:
    def __init__(self, path):
        self.path = path
        self.lib = ctypes.CDLL(path)
        self.width = {}
        for name in FUNCTIONS:
            for side in ("host", "device"):
                fn = getattr(self.lib, f"probe_{name}_{side}")
                fn.restype = ctypes.c_int
                fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
            self.width[name] = (getattr(self.lib, f"probe_{name}_ni")(), getattr(self.lib, f"probe_{name}_no")())

    def run(self, name, side, x):
        """x: (n, NI) float64 -> (n, NO) float64 from the host loop (side='host') or the kernel (side='device')."""
        ni, no = self.width[name]
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, ni)
        out = np.full((len(x), no), np.nan)
        rc = getattr(self.lib, f"probe_{name}_{side}")(len(x), x.ctypes.data, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"probe_{name}_{side}: hipError_t {rc}")
        return out


def build(outdir):
    hipcc, flags = makefile_toolchain()
    so = os.path.join(str(outdir), "libdevmath_probe.so")
    subprocess.run([hipcc, *flags, "-o", so, SOURCE], check=True)
    return Probe(so)
