"""The drive of tests/helpers/hash_scenes.py drive_sequence through the CPU oracle and the table simulator (no GPU): which table size the run
needs with a rebuild every few scans, what the table holds at the end, and at which scan the same run without rebuilds is refused.
tests/test_hash_scenes_cpu.py asserts these answers; tests/test_gpu_hash_tables.py holds every driver of the device against them."""
import functools

import numpy as np

from oracle import cpu as orc
from tests.helpers import hash_scenes as hs

DRIVE_N, DRIVE_H, DRIVE_W, DRIVE_RANGE, DRIVE_MIN = 23, 16, 512, 12.0, 0.5
DRIVE_PTS = DRIVE_H * DRIVE_W
REBUILD_EVERY = 3


def simulate_drive(worlds, poses, cap, rebuild_every):
    """(simulator after the last scan, `used` after every scan's insert, first scan at which it passes 3/4 of the table or None)"""
    sim, used, first = hs.MapSim(cap, 1.0, DRIVE_RANGE), [], None
    for k, (w, T) in enumerate(zip(worlds, poses)):
        sim.add(w)
        used.append(sim.tab.used)
        if first is None and sim.tab.exhausted:
            first = k
        if sim.tab.used >= cap:
            break  # (a full table: nothing beyond this scan is asked of the device)
        sim.prune(T[:3, 3])
        if rebuild_every > 0 and (k + 1) % rebuild_every == 0:
            sim.rebuild()
    return sim, used, first


@functools.lru_cache(maxsize=None)
def drive_reference():
    """the oracle's run of the drive, and the table size the simulator - fed the oracle's per-scan creations - asks for"""
    frames, _ = hs.drive_sequence(DRIVE_N, DRIVE_H, DRIVE_W, DRIVE_RANGE)
    orc.set_threads(1)
    ref = orc.ICP(DRIVE_RANGE, DRIVE_MIN, voxel_size=1.0, deskew=0)
    poses, worlds = [], []
    for f in frames:
        T = ref.register_frame(f.astype(np.float64), None)
        poses.append(T)
        worlds.append(ref.last_frame_down() @ T[:3, :3].T + T[:3, 3])
    assert poses[-1][0, 3] > 1.5 * DRIVE_RANGE  # it followed the drive
    cap = 1 << 8
    while simulate_drive(worlds, poses, cap, REBUILD_EVERY)[2] is not None:
        cap <<= 1
    sim, used, _ = simulate_drive(worlds, poses, cap, REBUILD_EVERY)
    assert max(used) >= cap // 2, (cap, max(used))  # the table is needed: a peak load of at least 1/2
    assert sim.tab.tombstones() > 100 and (sim.tab.chain_stats()[0] > 0).mean() > 0.2
    refused = simulate_drive(worlds, poses, cap, 0)[2]
    assert refused is not None and refused > REBUILD_EVERY
    return dict(frames=frames, poses=np.array(poses), stats=ref.stats, cap=cap, sim=sim, used=used, refused=refused)
