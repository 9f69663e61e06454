"""Revisited places: what a describe, a match and the loop-closure batch form cost on the device; one JSON line
(profiles/r28_place_cost.json).  Each figure stands beside two others: the numpy restatement's time on the host, and the count of
lane-operations divided by the part's plain vector rate - the least time the vector ALUs could take, not a time anybody measured.

  describe   HIP-event ms per 128 x 1024 sweep (float32 xyz of the seed-1000 synthetic sequence): upload, binning, pack.  Lane-operations:
             per point 3 per sector step (two products, one subtraction) times S, the ring walk R, about 20 for the rest.
  match      one query against 1 000 and 10 000 random sparse descriptors (R = 20, S = 60) at every shift: S^2 Rpad / 4 packed
             sum-of-absolute-differences steps per pair = 18 000 lane-operations.
  match_all  10 000 entries, min_gap 0: every entry against all before it, 5 10^7 pairs.
  restatement  tests/helpers/place_numpy.py: `describe` on the same sweep; `pair_table` rows on a sample of pairs, scaled to the pair count
             by its measured time per pair (the whole batch would take hours) - the scaling is said in the figure's name.
Medians over `--repeats` runs after one warm-up, with the spread (max - min).  Nothing here is asserted anywhere.

python tools/place_cost.py [--repeats 5] [--out profiles/r28_place_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ptudes_lab_amd  # noqa: E402,F401
from ptudes_lab_amd import core, synth  # noqa: E402
from tests.helpers import place_cases as pc  # noqa: E402
from tests.helpers import place_numpy as pn  # noqa: E402

VECTOR_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9  # CUs x SIMDs x lanes x clock: one plain vector operation per lane and clock


def stat(v):
    return {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "runs": [float(x) for x in v]}


def describe_cost(repeats):
    seq = synth.make_sequence(seed=1000, n_scans=2)
    sweep = seq.scan(1)
    ix = core.PlaceIndex(capacity=4)
    R, S = ix.n_ring, ix.n_sector
    ms = []
    for rep in range(repeats + 1):
        ix.profile(reset=True)
        _, info = ix.describe(sweep, keep=False)
        if rep:
            ms.append(ix.profile()[0])
    e, d = ix.tables()
    t0 = time.perf_counter()
    want, winfo = pn.describe(sweep, e, d, ix.cfg.z_min, ix.cfg.z_step)
    host_ms = 1000.0 * (time.perf_counter() - t0)
    ix.describe(sweep, keep=True)
    same = bool(np.array_equal(ix.descriptors()[0][0], want) and info.as_dict() == winfo)
    ix.close()
    lane_ops = len(sweep) * (3 * S + R + 20)
    return {"shape": [seq.H, seq.W], "n_ring": R, "n_sector": S, "info": winfo, "device_ms": stat(ms), "restatement_host_ms": host_ms,
            "device_equals_restatement": same, "lane_ops": lane_ops, "lane_ops_over_vector_rate_ms": 1000.0 * lane_ops / VECTOR_LANE_OPS_PER_S}


def match_cost(repeats, sample_pairs=200):
    R, S = 20, 60
    pair_ops = S * S * ((R + 3) // 4)
    descs = pc.random_descriptors(28, 10000, R, S)
    ix = core.PlaceIndex(capacity=10000)
    ix.load(descs, pn.infos_of(descs))
    t0 = time.perf_counter()
    td, ts = pn.pair_table(descs[:sample_pairs], full_rows={0})
    host_ms_per_pair = 1000.0 * (time.perf_counter() - t0) / (sample_pairs * (sample_pairs + 1) // 2 + sample_pairs - 1)
    out = {"n_ring": R, "n_sector": S, "lane_ops_per_pair": pair_ops, "restatement_host_ms_per_pair_on_a_sample": host_ms_per_pair,
           "restatement_sample_pairs": sample_pairs}
    for name, last in (("match_1000", 999), ("match_10000", 9999)):
        ms = []
        for rep in range(repeats + 1):
            m = ix.match(0, 0, last)
            if rep:
                ms.append(m.device_ms)
        pairs = last + 1
        out[name] = {"pairs": pairs, "device_ms": stat(ms), "device_equals_restatement_on_the_sample":
                     bool(np.array_equal(m.dist[:sample_pairs], td[0]) and np.array_equal(m.shift[:sample_pairs], ts[0])),
                     "restatement_host_ms_scaled_from_the_sample": host_ms_per_pair * pairs, "lane_ops": pairs * pair_ops,
                     "lane_ops_over_vector_rate_ms": 1000.0 * pairs * pair_ops / VECTOR_LANE_OPS_PER_S}
        print(name, json.dumps(out[name]), flush=True)
    ms = []
    for rep in range(repeats + 1):
        g = ix.match_all(0)
        if rep:
            ms.append(g.device_ms)
    we, wd, ws = pn.match_all(descs[:sample_pairs], 0, table=(td, ts))
    out["match_all_10000"] = {"pairs": g.n_compared, "min_gap": 0, "device_ms": stat(ms), "device_equals_restatement_on_the_sample":
                              bool(np.array_equal(g.entry[:sample_pairs], we) and np.array_equal(g.dist[:sample_pairs], wd)
                                   and np.array_equal(g.shift[:sample_pairs], ws)),
                              "restatement_host_ms_scaled_from_the_sample": host_ms_per_pair * g.n_compared, "lane_ops": g.n_compared * pair_ops,
                              "lane_ops_over_vector_rate_ms": 1000.0 * g.n_compared * pair_ops / VECTOR_LANE_OPS_PER_S}
    print("match_all_10000", json.dumps(out["match_all_10000"]), flush=True)
    ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"what": "place descriptors: HIP-event ms of a describe, a match and the loop-closure batch form beside the numpy restatement's host "
                   "time and beside lane-operations over the plain vector rate (DESIGN.md 3.31)",
           "code_id": core.L.lib().ptl_code_id().decode(), "vector_lane_ops_per_s": VECTOR_LANE_OPS_PER_S,
           "describe_128x1024": describe_cost(a.repeats)}
    print("describe", json.dumps(res["describe_128x1024"]), flush=True)
    res["match"] = match_cost(a.repeats)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
