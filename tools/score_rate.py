#!/usr/bin/env python3
"""What scoring a batch costs: on the device (kr_dtw_batch + kr_pose_mse_batch inside knode.simulate_batch) against the
host path it replaces (not bench.py; one process, one GPU).

    python tools/score_rate.py [--out profiles/<tag>_score_rate.json] [--rods 1024] [--steps 100] [--repeats 3]

Workload: B = 1024 rods, T = 100 steps, N = 100, fp64, MLP off, every rod its own sine tensions; the reference is rod 0's
own trajectory of an earlier run (T states, shared by all rods), the scored path the tip's.
  (i)  device: wall time of simulate_batch(..., score=..., return_states=False) minus the same call without score
       (medians of the repeats; both include the uploads and the small copies back).
  (ii) host:   wall time of simulate_batch(..., return_states=True) minus the call without states - the unpack launches
       and the copy of [B, T+1, 25, N] - plus krod_eval.dtw_distance and pos_euler_mse per rod, timed on 32 rods and
       SCALED to B (the output says so).
  kernels: HIP-event durations of the two launches alone on a state history left by the same run.
Acceptance is (i) < (ii).  The device metrics are checked against the host's on the 32 rods before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "knode-cosserat_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

HOST_RODS = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rods", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--nodes-per-rod", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    import cosserat_oracle as orc
    import krod_native as kn
    from cosserat_ode import CosseratRod
    from knode import setup_robot, simulate_batch
    from krod_eval import dtw_distance, pos_euler_mse

    assert torch.cuda.is_available(), "score_rate.py measures on the MI355X"
    B, T, N, R = args.rods, args.steps, args.nodes_per_rod, args.repeats
    robot = CosseratRod(use_fsolve=True)
    setup_robot(robot)
    robot.N = N
    robot.compute_intermediate_terms()
    ctl = orc.batch_sine_controls(B, T, robot.del_t, 1235)
    n_host = min(HOST_RODS, B)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    med = lambda v: float(np.median(v))
    # the reference, and the first use of every kernel (untimed)
    first = simulate_batch(robot, ctl[:n_host])
    ref = first["traj"][0, :T]
    score = {"reference": ref}
    scored = simulate_batch(robot, ctl[:n_host], score=score)
    host_dtw = np.array([dtw_distance(scored["traj"][b, :T, :3, N - 1], ref[:, :3, N - 1]) for b in range(n_host)])
    host_mse = np.array([pos_euler_mse(scored["traj"][b, :T], ref) for b in range(n_host)])
    dtw_bitwise = bool(np.array_equal(scored["dtw"], host_dtw))
    mse_rel = float(np.max(np.abs(scored["mse"][1:] - host_mse[1:]) / host_mse[1:])) if n_host > 1 else 0.0
    simulate_batch(robot, ctl, score=score, return_states=False)

    plain, dev_scored, with_states = [], [], []
    for _ in range(R):  # interleaved: the three see the same clock
        plain.append(wall(lambda: simulate_batch(robot, ctl, return_states=False))[0])
        dev_scored.append(wall(lambda: simulate_batch(robot, ctl, score=score, return_states=False))[0])
        s, out = wall(lambda: simulate_batch(robot, ctl, return_states=True))
        with_states.append(s)
    unconverged = int((out["status"] != 0).sum())
    traj = out["traj"]
    host_dtw_s, host_mse_s = [], []
    for _ in range(R):
        t0 = time.perf_counter()
        for b in range(n_host):
            dtw_distance(traj[b, :T, :3, N - 1], ref[:, :3, N - 1])
        t1 = time.perf_counter()
        for b in range(n_host):
            pos_euler_mse(traj[b, :T], ref)
        t2 = time.perf_counter()
        host_dtw_s.append(t1 - t0)
        host_mse_s.append(t2 - t1)
    del traj, out

    # the two kernels alone, by HIP events
    h = robot._native()
    dev, dt = "cuda:0", torch.float64
    states = h.new_state(B, dt, n_slots=T + 1)
    h.init_straight(states[0])
    G = torch.zeros((B, 6), dtype=dt, device=dev)
    h.simulate(torch.as_tensor(ctl, device=dev).contiguous(), states, G)
    ref_states = h.pack_poses(ref[None], dt)
    a = states[:T, :, N - 1, 12:15].permute(1, 0, 2)
    b = ref_states[:, 0, N - 1, 12:15]

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    k_dtw, k_mse = [], []
    for i in range(R + 2):
        d, m = event_ms(lambda: h.dtw(a, b)), event_ms(lambda: h.pose_mse(states[:T], ref_states))
        if i >= 2:
            k_dtw.append(d)
            k_mse.append(m)

    scale = B / n_host
    i_dev = med(dev_scored) - med(plain)
    ii_host = (med(with_states) - med(plain)) + scale * (med(host_dtw_s) + med(host_mse_s))
    mse_bytes = T * B * N * kn.KR_SLOTS * 8  # the rods' records (whole cache lines are fetched); the shared reference stays in cache
    res = dict(
        B=B, T=T, N=N, dtype="f64", repeats=R, device=torch.cuda.get_device_name(0), unconverged=unconverged,
        checked_on_rods=n_host, dtw_bitwise_equal_to_host=dtw_bitwise, mse_max_rel_error_vs_host=mse_rel,
        seconds=dict(simulate_plain=plain, simulate_scored_on_device=dev_scored, simulate_with_states=with_states,
                     host_dtw_32_rods=host_dtw_s, host_mse_32_rods=host_mse_s),
        i_device_scoring_s=i_dev,
        ii_host_scoring_s=ii_host,
        ii_parts_s=dict(unpack_and_copy_of_trajectories=med(with_states) - med(plain),
                        host_dtw_scaled=scale * med(host_dtw_s), host_mse_scaled=scale * med(host_mse_s)),
        ii_note=f"host metrics timed on {n_host} rods and SCALED by {scale:g} to B = {B}",
        accepted_i_below_ii=bool(i_dev < ii_host),
        kernel_ms=dict(kr_dtw_batch=dict(median=med(k_dtw), all=k_dtw), kr_pose_mse_batch=dict(median=med(k_mse), all=k_mse)),
        dtw_cells_per_s=B * T * T / (med(k_dtw) * 1e-3),
        pose_mse_bytes_per_s_states_only=mse_bytes / (med(k_mse) * 1e-3),
    )
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
