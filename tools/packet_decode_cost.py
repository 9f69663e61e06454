"""What decoding lidar packets on the device costs; one JSON line (profiles/r12_packet_decode_cost.json).

128 x 1024 RNG19_RFL8_SIG16_NIR16 sweeps (64 packets of 24 832 bytes: 1.59 MB of payload, 0.52 MB of it range), two steps, each a
child process of its own with its own time limit; the first failure ends the run:

  upload   time per sweep of BatchRunner.upload_packets (ptl_batch_upload_packets: packets up, decoded into the sweep's slot) against
           BatchRunner.upload_range of the READY image (ptl_batch_upload_range: what a host-side decoder would leave to be uploaded), both
           from page-locked host memory, alternated sweep block by sweep block in one process; host clock around calls that return after
           the stream has drained.  The slots are compared afterwards through a run (bit-equal poses).
  kernel   device time of the decode itself (ptl_pktdec_profile: HIP events around the initialisation and the three passes of one call) for 1, 8
           and 32 sweeps per call, against the bytes it moves: packets read once by the decode pass + column headers by the owner pass +
           image, column times, statuses and owner words written.

python tools/packet_decode_cost.py [--sweeps 32] [--repeats 5] [--out profiles/r12_packet_decode_cost.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, C = 128, 1024, 16
PROFILE = "RNG19_RFL8_SIG16_NIR16"
STEP_LIMIT_S = {"upload": 240, "kernel": 120}


def _format():
    from types import SimpleNamespace
    from ptudes_lab_amd import packets as pk
    return pk.OusterPacketFormat.from_info(SimpleNamespace(format=SimpleNamespace(
        pixels_per_column=H, columns_per_frame=W, columns_per_packet=C, udp_profile_lidar=PROFILE)))


def make_packets(fmt, images, t0_ns=10**9):
    """(n, 64, packet bytes) u8: the sweeps' packets, written with array operations (tests/helpers holds the plain-loop encoder)"""
    n = len(images)
    buf = np.zeros((n, W // C, fmt.lidar_packet_size), np.uint8)
    cols = buf[:, :, fmt.packet_header_size:fmt.packet_header_size + C * fmt.col_size].reshape(n, W // C, C, fmt.col_size)
    ids = np.arange(W, dtype=np.uint64).reshape(W // C, C)
    for k in range(n):
        buf[k, :, 2:4] = np.frombuffer(np.uint16(k & 0xffff).tobytes(), np.uint8)
        ts = np.uint64(t0_ns + k * 10**8) + ids * np.uint64(97_656)
        cols[k, :, :, 0:8] = ts[..., None].view(np.uint8).reshape(W // C, C, 8)
        cols[k, :, :, 8:10] = ids.astype(np.uint16)[..., None].view(np.uint8).reshape(W // C, C, 2)
        cols[k, :, :, 10] = 1
        px = cols[k, :, :, fmt.col_header_size:].reshape(W // C, C, H, fmt.pixel_size)
        img = np.ascontiguousarray(images[k].T).reshape(W // C, C, H)  # [packet][column][row]
        px[..., 0:4] = img[..., None].view(np.uint8).reshape(W // C, C, H, 4)
    return buf


def step_upload(sweeps, repeats):
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core, synth
    fmt = _format()
    seq = synth.make_sequence(seed=1000, n_scans=sweeps)
    images = np.empty((sweeps, H, W), np.uint32)
    for k in range(sweeps):
        x = seq.scan(k).reshape(H, W, 3)
        images[k] = np.round(np.linalg.norm(x[:, (W - np.arange(W)) % W, :], axis=2) * 1000.0).astype(np.uint32)
    pkts = make_packets(fmt, images)
    core.host_pin(pkts)
    core.host_pin(images)
    lut = core.Lut(H, W, np.linspace(45.0, -45.0, H), np.zeros(H))
    dec = core.PacketDecoder(fmt, max_sweeps=1)
    runners = {}
    for name in ("packets", "range"):
        b = core.BatchRunner(1, sweeps, H * W, 0, with_ekf=False, range_input=True)
        b.set_lut(lut)
        b.upload_imu(0, np.zeros((0, 7)), [0] * sweeps)
        runners[name] = b

    def up(name, k):
        if name == "packets":
            runners[name].upload_packets(0, dec, k, pkts[k])
        else:
            runners[name].upload_range(0, k, images[k])

    for name in runners:  # warm-up: every shape of the timed window
        for k in range(sweeps):
            up(name, k)
    per_sweep = {"packets": [], "range": []}
    for _ in range(repeats):
        for name in ("packets", "range"):
            core.device_sync()
            t0 = time.perf_counter()
            for k in range(sweeps):
                up(name, k)
            per_sweep[name].append((time.perf_counter() - t0) / sweeps * 1e6)
    n_run = min(sweeps, 4)
    poses = {}
    for name, b in runners.items():
        b.run(n_run)
        poses[name] = b.results(0)["kiss_poses"]
        b.close()
    core.host_unpin(pkts)
    core.host_unpin(images)
    return {"sweeps": sweeps, "repeats": repeats, "source": "page-locked host memory (ptl_host_pin)",
            "bus_bytes_per_sweep": {"packets": int(pkts[0].nbytes), "range": int(images[0].nbytes)},
            "us_per_sweep": {k: {"median": float(np.median(v)), "spread": float(max(v) - min(v)), "runs": v} for k, v in per_sweep.items()},
            "runs_bit_equal": bool(np.array_equal(poses["packets"], poses["range"])), "scans_compared": n_run}


def step_kernel(sweeps, repeats):
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import core
    fmt = _format()
    rng = np.random.default_rng(3)
    images = rng.integers(0, 1 << 19, (sweeps, H, W), dtype=np.uint32)
    pkts = make_packets(fmt, images)
    core.host_pin(pkts)
    out = {}
    for per_call in (1, 8, 32):
        if per_call > sweeps:
            continue
        dec = core.PacketDecoder(fmt, max_sweeps=per_call)
        a = pkts[:per_call].reshape(-1, fmt.lidar_packet_size)
        sop = np.repeat(np.arange(per_call, dtype=np.int32), W // C)
        got = dec.decode_arrays(a, sop, per_call)  # warm-up, and the result is checked
        assert np.array_equal(got[0], images[:per_call]), "decoded images differ from what was encoded"
        ms = []
        for _ in range(repeats):
            dec.profile(True, reset=True)
            for _ in range(20):
                dec.decode_arrays(a, sop, per_call)
            total, calls = dec.profile(True)
            ms.append(total / max(calls, 1))
        dec.close()
        n_pkt = per_call * (W // C)
        # decode pass: the packets once; owner pass: one 64-byte line per column header; written: image, times, statuses, owners (+ their initialisation)
        moved = n_pkt * fmt.lidar_packet_size + n_pkt * C * 64 + per_call * (H * W * 4 + W * (8 + 2 + 4 + 4))
        med = float(np.median(ms))
        out[str(per_call)] = {"device_us_per_call": med * 1e3, "device_us_per_sweep": med * 1e3 / per_call, "spread_us_per_call": (max(ms) - min(ms)) * 1e3,
                              "bytes_moved_per_call": int(moved), "GB_per_s": moved / (med * 1e-3) / 1e9 if med > 0 else None}
    core.host_unpin(pkts)
    return {"calls_per_repeat": 20, "repeats": repeats, "sweeps_per_call": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), default=None, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps({"upload": step_upload, "kernel": step_kernel}[a.step](a.sweeps, a.repeats)), flush=True)
        return 0
    import ptudes_lab_amd  # noqa: F401
    from ptudes_lab_amd import _lib
    if _lib.lib().ptl_backend() != 1:
        print("no HIP device: nothing is measured without one", file=sys.stderr)
        return 2
    res = {"what": "lidar packets decoded on the device: upload_packets against upload_range, and the decode's own device time (DESIGN.md 3.16)",
           "shape": [H, W], "profile": PROFILE, "code_id": _lib.lib().ptl_code_id().decode()}
    for step, limit in STEP_LIMIT_S.items():  # a fresh process per step, its own time limit, the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--sweeps", str(a.sweeps), "--repeats", str(a.repeats)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {step}: no result within {limit} s - stopping", file=sys.stderr)
            return 3
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"step {step}: exit status {p.returncode} - stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 4
        res[step] = json.loads(line[-1][len("RESULT "):])
        print(step, json.dumps(res[step]), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
