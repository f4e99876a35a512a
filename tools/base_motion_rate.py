#!/usr/bin/env python3
"""Rate of the boundary kernels next to their table and loads twins (not bench.py; one process, one GPU).

    python tools/base_motion_rate.py [--out profiles/<tag>_base_motion_rate.json] [--steps 1000] [--repeats 3]

After a clock ramp of the kind bench.py uses (RK4 launches of the persistent solver on a second handle), B = 1024,
N = 100, fp64, 3-slot ring, every run from the straight rod, alternating a, b, c, d per round so that all four see the
same clock:
  (a) the table call with 1024 identical rows,
  (b) the loads call with constant loads = the rows' own wrench,
  (c) the boundary call with constant rows = the rows' own base and wrench (the work of (b) plus 13 values loaded and
      stored per step outside the sweeps; its tips and states are compared bit for bit with (a)'s once, untimed),
  (d) the boundary call with the `slide` history of tests/base_motion_cases.py scaled per rod by 0.5 + b / B.
Times are HIP-event durations of the simulate call on the stream; rates are rod-steps per second, medians of the
rounds.  `boundary_constant_vs_loads` reports the median ratio next to the max - min spread of (b)'s own repeats, and
`boundary_constant_within_twice_loads_spread` whether (c)'s median lies within twice that spread of (b)'s."""
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
    tip = torch.empty((B, T, 3), dtype=dt, device=dev)
    status = torch.zeros((B, T), dtype=torch.int32, device=dev)
    t = np.arange(T, dtype=np.float64)
    own = np.concatenate([np.asarray(x, float) for x in (carrier.p0, carrier.h0, carrier.q0, carrier.w0, carrier.F_tip, carrier.M_tip)])
    om = 2 * np.pi / (8 * carrier.del_t)  # the `slide` history (tests/base_motion_cases.py): a carriage along x
    scale = 0.5 + np.arange(B) / B
    slide = np.ascontiguousarray(np.broadcast_to(own, (B, T, 19))).copy()
    slide[:, :, 0] = scale[:, None] * 0.02 * np.sin(om * t * carrier.del_t)[None]
    slide[:, :, 7] = scale[:, None] * 0.02 * om * np.cos(om * t * carrier.del_t)[None]
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev).contiguous()
    loads = {"table": {},
             "loads_constant": dict(loads=up(np.broadcast_to(own[13:], (B, T, 6)))),
             "boundary_constant": dict(bnd=up(np.broadcast_to(own, (B, T, 19)))),
             "boundary_slide": dict(bnd=up(slide))}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def run(tab, key):
        h.init_straight(st[0], table=tab)
        G.zero_()
        secs = timed(lambda: h.simulate(ctl, st, G, ring=True, tip=tip, status=status, table=tab, **loads[key]))
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

    res = dict(B=B, N=N, steps=T, repeats=R, dtype="f64", ring=True, device=torch.cuda.get_device_name(0))
    with h.param_table([carrier._params()] * B) as tab:
        first = {}
        for key in loads:  # first use of every kernel instantiation, untimed; (a), (b) and (c) must agree bit for bit
            run(tab, key)
            first[key] = (tip.clone(), st.clone())
        res["constant_rows_bit_identical_to_table"] = bool(all(torch.equal(first["table"][i], first[k][i]) for i in (0, 1)
                                                                 for k in ("loads_constant", "boundary_constant")))
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
    a, b, c = (res[k]["rod_steps_per_s"] for k in ("table", "loads_constant", "boundary_constant"))
    res["loads_constant_vs_table"] = dict(median_ratio=round(b["median"] / a["median"], 4))
    res["boundary_constant_vs_loads"] = dict(median_ratio=round(c["median"] / b["median"], 4),
                                             loads_min_max_spread=round((b["max"] - b["min"]) / b["median"], 4))
    res["boundary_slide_vs_boundary_constant"] = dict(median_ratio=round(res["boundary_slide"]["rod_steps_per_s"]["median"] / c["median"], 4))
    res["boundary_constant_within_twice_loads_spread"] = bool(b["median"] - c["median"] <= 2 * (b["max"] - b["min"]))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
