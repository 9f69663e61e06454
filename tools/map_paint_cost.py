"""The map painted: what the second pass over a map's sweeps costs per 128 x 1024 sweep beside the map update whose input
it re-reads, and what the field pass of the packet decoder costs beside the decode it follows; one JSON line
(profiles/r24_map_paint_cost.json).

Expectation, written down before the first run: a paint of a sweep does ONE table probe per return and no insert - no compaction, no
allocation, no block header written - where `map_add_posed` of the same sweep compacts the returns and runs the three insert passes over them,
so a paint should not take longer than the add of the same sweep.  The field pass reads the staged packets once more from device memory and
writes n_fields images; the decode it follows does that for one image and also resolves owners, initialises and finishes, so a field pass
should cost less than the decode it follows, for one field and for three.  No rate is fixed in advance; whatever the run says is printed beside
this text, and DESIGN.md 3.27 carries the correction if it disagrees.

  paint    the seed-1000 synthetic sequence of `--sweeps` sweeps of 128 x 1024 as range images (fly.synthetic_range_scans), ground-truth
           knots, two maps at 0.5 m built from all of them by Icp.map_add_posed: the map that is painted and a scratch copy that takes the
           adds.  Alternated in one process over every `--stride`-th sweep, `--repeats` rounds after one warm-up round:
             add     Icp.map_add_posed of the sweep into the scratch copy (its voxels hold the sweep already: the steady state of a map that
                     is being built over ground it has seen): wall ms around a call that ends in a device synchronise
             paint   Painter.add_posed of the same sweep with its range image as the field: wall ms likewise, and the handle's HIP-event ms
           per sweep, median and spread (max - min) over the rounds.  Both calls stage the sweep from pageable host memory.
  fields   `--decode-sweeps` sweeps of 128 x 1024 RNG19_RFL8_SIG16_NIR16 packets (valid headers, random pixels) in one call: PacketDecoder
           .decode_arrays against .decode_field_arrays with 1 (reflectivity) and 3 (reflectivity, signal, near_ir) fields, alternated; per
           call the HIP-event ms of the decoder's launches (ptl_pktdec_profile; the field pass is the difference to the plain decode's) and
           the wall ms, median and spread

python tools/map_paint_cost.py [--sweeps 100] [--stride 5] [--repeats 5] [--decode-sweeps 8] [--out profiles/r24_map_paint_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptudes_lab_amd  # noqa: E402,F401
from ptudes_lab_amd import core, fly, synth  # noqa: E402
from ptudes_lab_amd import packets as pk  # noqa: E402

BOUNDS = 1.5
EXPECTATION = ("a paint does one probe per return and no insert: it should not take longer than map_add_posed of the same sweep; a field pass "
               "re-reads the staged packets and writes its images without resolving owners: it should cost less than the decode it follows, "
               "for one field and for three")


def gt_knots(seq, n, step=0.02):
    kt = np.arange(0, n * seq.scan_dt + 0.3, step)
    return [(seq.t_base + float(t), seq.pose_at(np.array([t]))[0]) for t in kt]


def stat(v):
    return {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "runs": [float(x) for x in v]}


def new_map(lut):
    return core.Icp(1.0e9, 0.0, voxel_size=0.5, scan_cols=lut.W, max_points_per_scan=lut.H * lut.W, map_block_capacity=1 << 21,
                    map_table_capacity=1 << 23)


def paint_cost(n, stride, repeats):
    seq = synth.make_sequence(seed=1000, n_scans=n)
    lut, scans = fly.synthetic_range_scans(seq)
    knots = gt_knots(seq, n)
    traj = core.Traj([k[0] for k in knots], [k[1] for k in knots], BOUNDS, BOUNDS)
    ts = [np.asarray(s.timestamp, dtype=np.float64) * 1e-9 for s in scans]
    m, scratch = new_map(lut), new_map(lut)
    for h in (m, scratch):
        for k in range(n):
            assert not h.map_add_posed(traj, ts[k], range_mm=scans[k].range_mm, lut=lut)[1]
    size = list(m.map_size())
    picked = list(range(0, n, stride))
    add_wall, paint_wall, paint_dev = [], [], []
    result = None
    for rep in range(repeats + 1):  # (round 0: code object load, first touch)
        painter = core.Painter(m)
        before = painter.values().result.device_ms  # (the prefixes of create and this read's reduction)
        aw = pw = 0.0
        for k in picked:
            core.device_sync()
            t0 = time.perf_counter()
            scratch.map_add_posed(traj, ts[k], range_mm=scans[k].range_mm, lut=lut)
            aw += time.perf_counter() - t0
            core.device_sync()
            t0 = time.perf_counter()
            painter.add_posed(traj, ts[k], scans[k].range_mm, range_mm=scans[k].range_mm, lut=lut)
            pw += time.perf_counter() - t0
        result = painter.values().result
        pd = result.device_ms - before  # (includes the second read's reduction: one launch over the counts)
        painter.close()
        if rep:
            add_wall.append(1e3 * aw / len(picked)); paint_wall.append(1e3 * pw / len(picked)); paint_dev.append(pd / len(picked))
    out = {"sweeps_in_the_map": n, "sweeps_timed_per_round": len(picked), "shape": [seq.H, seq.W], "voxel_size": 0.5, "map_size": size,
           "scratch_map_size_after": list(scratch.map_size()),
           "add_wall_ms_per_sweep": stat(add_wall), "paint_wall_ms_per_sweep": stat(paint_wall), "paint_device_ms_per_sweep": stat(paint_dev),
           "paint_over_add_wall": float(np.median(paint_wall) / np.median(add_wall)),
           "last_round": {k: int(getattr(result, k)) for k in ("n_points", "n_points_painted", "n_scans", "n_scans_skipped", "n_rays_matched",
                                                               "n_rays_unmatched", "n_no_return", "sum_count")}}
    for h in (m, scratch, traj, lut):
        h.close()
    return out


def random_packets(fmt, n_sweeps, seed=0):
    """n_sweeps sweeps of packets with valid column headers (consecutive measurement ids, status bit 0, rising times) and random pixel bytes"""
    rng = np.random.default_rng(seed)
    H, W, C = fmt.pixels_per_column, fmt.columns_per_frame, fmt.columns_per_packet
    per = W // C
    a = rng.integers(0, 256, (n_sweeps * per, fmt.lidar_packet_size), dtype=np.uint8)
    sop = np.repeat(np.arange(n_sweeps, dtype=np.int32), per)
    for i in range(len(a)):
        s, j = divmod(i, per)
        a[i, fmt.frame_id_offset:fmt.frame_id_offset + 2] = np.frombuffer(np.uint16(100 + s).tobytes(), np.uint8)
        for c in range(C):
            o = fmt.packet_header_size + c * fmt.col_size
            col = j * C + c
            a[i, o:o + 8] = np.frombuffer(np.uint64(10**9 * (s + 1) + 97_657 * col).tobytes(), np.uint8)
            a[i, o + 8:o + 10] = np.frombuffer(np.uint16(col).tobytes(), np.uint8)
            a[i, o + fmt.status_offset:o + fmt.status_offset + 2] = np.frombuffer(np.uint16(1).tobytes(), np.uint8)
    return a, sop


def field_cost(n_sweeps, repeats):
    from types import SimpleNamespace
    info = SimpleNamespace(format=SimpleNamespace(pixels_per_column=128, columns_per_frame=1024, columns_per_packet=16,
                                                  udp_profile_lidar="RNG19_RFL8_SIG16_NIR16"))
    fmt = pk.OusterPacketFormat.from_info(info)
    a, sop = random_packets(fmt, n_sweeps)
    dec = core.PacketDecoder(fmt, max_sweeps=n_sweeps, max_packets=len(a))
    forms = {"decode": lambda: dec.decode_arrays(a, sop, n_sweeps),
             "decode_fields_1": lambda: dec.decode_field_arrays(a, sop, ["reflectivity"], n_sweeps),
             "decode_fields_3": lambda: dec.decode_field_arrays(a, sop, ["reflectivity", "signal", "near_ir"], n_sweeps)}
    dev, wall = {k: [] for k in forms}, {k: [] for k in forms}
    for rep in range(repeats + 1):
        for name, call in forms.items():
            dec.profile(enable=True, reset=True)
            core.device_sync()
            t0 = time.perf_counter()
            call()
            w = 1e3 * (time.perf_counter() - t0)
            ms, _ = dec.profile(enable=True, reset=True)
            if rep:
                dev[name].append(ms); wall[name].append(w)
    dec.close()
    out = {"sweeps_per_call": n_sweeps, "packets_per_call": int(len(a)), "packet_bytes": int(fmt.lidar_packet_size),
           "device_ms_per_call": {k: stat(v) for k, v in dev.items()}, "wall_ms_per_call": {k: stat(v) for k, v in wall.items()}}
    base = np.median(dev["decode"])
    out["field_pass_device_ms_per_call"] = {k: float(np.median(dev[k]) - base) for k in ("decode_fields_1", "decode_fields_3")}
    out["field_pass_over_decode"] = {k: float(v / base) for k, v in out["field_pass_device_ms_per_call"].items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--decode-sweeps", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"what": "the map painted: wall and device ms per 128 x 1024 sweep of a paint beside map_add_posed of the same sweep; device and wall "
                   "ms per call of the packet decoder with 1 and 3 field images beside the plain decode (DESIGN.md 3.27)",
           "code_id": core.L.lib().ptl_code_id().decode(), "expectation_before_the_run": EXPECTATION}
    res["fields"] = field_cost(a.decode_sweeps, a.repeats)
    print(json.dumps(res["fields"]), flush=True)
    res["paint"] = paint_cost(a.sweeps, a.stride, a.repeats)
    print(json.dumps(res["paint"]), flush=True)
    p, f = res["paint"], res["fields"]
    res["outcome_beside_the_expectation"] = {
        "paint_not_longer_than_add": bool(p["paint_wall_ms_per_sweep"]["median"] <= p["add_wall_ms_per_sweep"]["median"]),
        "field_pass_cheaper_than_decode": {k: bool(v < 1.0) for k, v in f["field_pass_over_decode"].items()}}
    print("expectation: " + EXPECTATION)
    print(f"paint {p['paint_wall_ms_per_sweep']['median']:.3f} ms wall ({p['paint_device_ms_per_sweep']['median']:.3f} ms device) per sweep against "
          f"add {p['add_wall_ms_per_sweep']['median']:.3f} ms wall; field pass / decode (device): {f['field_pass_over_decode']}")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
