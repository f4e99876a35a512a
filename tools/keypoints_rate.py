#!/usr/bin/env python3
"""Rate of the key-point call next to the parent's boundary call (not bench.py; one process, one GPU).

    python tools/keypoints_rate.py [--out profiles/<tag>_keypoints_rate.json] [--steps 1000] [--repeats 3]

After a clock ramp of the kind bench.py uses (RK4 launches of the persistent solver on a second handle), B = 1024,
N = 100, fp64, every run from the straight rod with constant rows = the rows' own base and wrench, alternating a, b, c, d
per round so that all four see the same clock:
  (a) the boundary call on a 3-slot ring (tips only),
  (b) the boundary call with the full trajectory, states[T + 1][B][N][28] - what a scored long run needed so far,
  (c) the key-point call on a ring with the points {33, 55, 77, 99},
  (d) the key-point call on a ring with 16 points.
(c)'s tips are compared bit for bit with (a)'s and its kp with the marked records of (b)'s states once, untimed.
Times are HIP-event durations of the simulate call on the stream; rates are rod-steps per second, medians of the
rounds.  `keypoints4_vs_full_trajectory` reports the median ratio next to the max - min spread of (b)'s own repeats and
`keypoints4_beats_full_trajectory_by_more_than_its_spread` the expectation; the distance of (c) and (d) to (a) is
reported, not bounded."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "knode-cosserat_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--nodes-per-rod", type=int, default=100)
    args = ap.parse_args()
    import torch
    import cosserat_oracle as orc
    from cosserat_ode import CosseratRod
    from knode import setup_robot

    def robot(N):
        r = CosseratRod(use_fsolve=True)
        setup_robot(r, None)
        r.N = N
        r.compute_intermediate_terms()
        return r

    N, T, R, B = args.nodes_per_rod, args.steps, args.repeats, args.batch
    dev, dt = "cuda:0", torch.float64
    carrier = robot(N)
    h = carrier._native()
    h2 = robot(N)._native()  # ramp handle
    ctl = torch.as_tensor(orc.batch_sine_controls(B, T, carrier.del_t, 1235), device=dev).contiguous()
    st, G = h.new_state(B, dt, n_slots=3), torch.zeros((B, 6), dtype=dt, device=dev)
    st_full = h.new_state(B, dt, n_slots=T + 1)
    pts4 = [33 * N // 100, 55 * N // 100, 77 * N // 100, N - 1]
    pts16 = sorted({(k + 1) * N // 16 - 1 for k in range(16)})
    kp4 = torch.empty((T, B, len(pts4), 28), dtype=dt, device=dev)
    kp16 = torch.empty((T, B, len(pts16), 28), dtype=dt, device=dev)
    tip = torch.empty((B, T, 3), dtype=dt, device=dev)
    status = torch.zeros((B, T), dtype=torch.int32, device=dev)
    own = np.concatenate([np.asarray(x, float) for x in (carrier.p0, carrier.h0, carrier.q0, carrier.w0, carrier.F_tip, carrier.M_tip)])
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev).contiguous()
    bnd = up(np.broadcast_to(own, (B, T, 19)))
    loads = {"boundary_ring": dict(states=st, ring=True),
             "boundary_full_trajectory": dict(states=st_full, ring=False),
             "keypoints4_ring": dict(states=st, ring=True, key_points=pts4, kp=kp4),
             "keypoints16_ring": dict(states=st, ring=True, key_points=pts16, kp=kp16)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def run(tab, key):
        kw = dict(loads[key])
        s = kw.pop("states")
        h.init_straight(s[0], table=tab)
        G.zero_()
        secs = timed(lambda: h.simulate(ctl, s, G, tip=tip, status=status, table=tab, bnd=bnd, **kw))
        return secs, int((status != 0).sum())

    def ramp(seconds):
        c2 = torch.as_tensor(orc.batch_sine_controls(1024, 100, carrier.del_t, 7), device=dev).contiguous()
        s2, G2 = h2.new_state(1024, dt, n_slots=3), torch.zeros((1024, 6), dtype=dt, device=dev)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            for _ in range(8):
                h2.init_straight(s2[0])
                G2.zero_()
                h2.simulate(c2, s2, G2, ring=True, scheme=1)  # KR_RK4
            torch.cuda.synchronize()

    def stats(secs):
        rates = [B * T / s for s in secs]
        return dict(rod_steps_per_s=dict(min=round(min(rates), 1), median=round(float(np.median(rates)), 1), max=round(max(rates), 1)),
                    seconds=[round(s, 6) for s in secs])

    res = dict(B=B, N=N, steps=T, repeats=R, dtype="f64", device=torch.cuda.get_device_name(0), key_points4=pts4, key_points16=pts16)
    with h.param_table([carrier._params()] * B) as tab:
        first = {}
        for key in loads:  # first use of every kernel instantiation, untimed
            run(tab, key)
            first[key] = tip.clone()
        res["keypoints_tips_bit_identical_to_boundary"] = bool(all(torch.equal(first["boundary_ring"], first[k]) for k in first))
        res["kp_bit_identical_to_full_trajectory"] = bool(torch.equal(kp4, st_full[1:][:, :, pts4]) and torch.equal(kp16, st_full[1:][:, :, pts16]))
        res["overlap_kernel"] = h.get_option("last_overlap")
        ramp(0.8)
        secs = {k: [] for k in loads}
        bad = {k: 0 for k in loads}
        for _ in range(R):
            for key in loads:
                s, nb = run(tab, key)
                secs[key].append(s)
                bad[key] += nb
    for k, v in secs.items():
        res[k] = dict(stats(v), unconverged=bad[k])
    a, b, c, d = (res[k]["rod_steps_per_s"] for k in loads)
    res["keypoints4_vs_full_trajectory"] = dict(median_ratio=round(c["median"] / b["median"], 4),
                                                full_trajectory_min_max_spread=round((b["max"] - b["min"]) / b["median"], 4))
    res["keypoints4_beats_full_trajectory_by_more_than_its_spread"] = bool(c["median"] - b["median"] > b["max"] - b["min"])
    res["keypoints4_vs_boundary_ring"] = dict(median_ratio=round(c["median"] / a["median"], 4))
    res["keypoints16_vs_boundary_ring"] = dict(median_ratio=round(d["median"] / a["median"], 4))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
