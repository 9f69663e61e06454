"""Writes the measured errors of the filter's edge streams as JSON:

    python -m tests.helpers.ekf_edges_report OUT.json [--gpu]

Without --gpu: the conditions the streams reach and the C oracle's error against the longdouble restatement.  With --gpu (an
MI355X): also the device's error, the ratio, and the runners' rows.  profiles/r020_ekf_edges_errors.json is this output."""
import json
import sys

import numpy as np

from tests.helpers import ekf_edge_streams as es


def cpu_report():
    floor = es.golden_floor()
    out = dict(rule=f"e_dev <= {es.FACTOR:g} * e_orc + floor; errors against the longdouble restatement; nav: max abs (quaternion up "
                    "to sign), cov / Phi: max abs / max(1, max|ref|)",
               floor=dict(nav=floor[0], cov=floor[1], Phi=floor[2]), goldens={}, streams={})
    for v, r in es.golden_replays().items():
        out["goldens"][v] = dict(restatement_vs_golden=dict(nav=r["golden"][0], cov=r["golden"][1]),
                                 oracle_vs_restatement=dict(nav=r["oracle"][0], cov=r["oracle"][1], Phi=r["oracle"][2]),
                                 row_swaps=sum(len(x["swaps"]) for x in r["reports"]), max_cond_S=max(x["cond"] for x in r["reports"]))
    for name in es.STREAMS:
        s, (_, f), (en, ec) = es.stream(name), es.restatement(name), es.oracle_errors(name)
        sw = np.zeros(6, dtype=int)
        for r in f.reports:
            for c in r["swaps"]:
                sw[c] += 1
        ang = [float(np.sqrt(r["innovation"][3:] @ r["innovation"][3:])) for r in f.reports]
        out["streams"][name] = dict(
            samples=sum(e[0] == "imu" for e in s.events), updates=len(f.reports),
            row_swaps_at_pivot_column=[int(x) for x in sw], max_zero_factors=max(r["zero_factors"] for r in f.reports),
            max_cond_S=max(r["cond"] for r in f.reports), innovation_angle=dict(min=min(ang), max=max(ang)),
            e_orc=dict(nav=en, cov=ec))
    return out


def gpu_report(out):
    from tests import test_gpu_ekf_edges as t
    from tests.helpers import ekf_longdouble as eld
    for name in es.STREAMS:
        e_dev, e_orc = es.errors(t.feed_stream(name), es.restatement(name)[0]), es.oracle_errors(name)
        out["streams"][name].update(e_dev=dict(nav=e_dev[0], cov=e_dev[1]),
                                    ratio=dict(nav=t._ratio(e_dev[0], e_orc[0]), cov=t._ratio(e_dev[1], e_orc[1])))
    runs, rows, end = t._run_runners()
    out["runners"] = {}
    for s, (res, log) in enumerate(runs["free"]):
        ref = es.runner_replay(eld.EkfLD(), rows, end, res["kiss_poses"])
        e_orc = es.runner_errors(es.runner_replay(es._PhiTracker(), rows, end, res["kiss_poses"]), ref)
        e_dev = es.runner_errors(dict(log, res_poses=res["res_poses"]), ref)
        out["runners"][f"sequence_{s}"] = {q: dict(e_dev=e_dev[i], e_orc=e_orc[i], ratio=t._ratio(e_dev[i], e_orc[i]))
                                           for i, q in enumerate(("nav", "cov", "Phi"))}
    return out


if __name__ == "__main__":
    rep = cpu_report()
    if "--gpu" in sys.argv[2:]:
        rep = gpu_report(rep)
    with open(sys.argv[1], "w") as fh:
        json.dump(rep, fh, indent=1)
        fh.write("\n")
