#!/usr/bin/env python3
"""What the backward pass over a stored rollout costs next to the forward rollout it differentiates (not bench.py; one
process, one GPU; run it under a time limit of its own: `timeout -k 10 300 python tools/adjoint_rate.py ...`).

    python tools/adjoint_rate.py [--out profiles/<tag>_adjoint_rate.json] [--rods 1024] [--N 100] [--steps 64] [--repeats 3]

B rods, N grid points, T steps, fp64, MLP off, sine tensions per rod (cosserat_oracle.batch_sine_controls), every buffer
allocated beforehand.  After a clock ramp (two seconds of the legs themselves), HIP-event durations of back-to-back calls - as
many per leg as fill `--window` seconds, counted from one trial call -, the legs alternating per round, medians of the rounds:
  (a) kr_simulate_batch with the full history (tol 1e-12: the states the adjoint is taken at),
  (b) kr_simulate_vjp_batch over that history with a tip cotangent on every step.
Reported: both legs in ms and M rod-steps/s, the ratio (b) / (a), and the COMPUTED cost of the route the backward pass
replaces - central differences of the tip path in the tension history, 4 T + 1 forward rollouts = (4 T + 1) x (a); it is
not run.  No ratio is set in advance.  Before anything is timed the call is checked: every status 0, resid <= 1e-10."""
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
    ap.add_argument("--rods", type=int, default=1024)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per timing")
    args = ap.parse_args()
    import torch
    import cosserat_oracle as orc
    import krod_native as kn
    from cosserat_ode import CosseratRod
    from knode import setup_robot

    assert torch.cuda.is_available(), "adjoint_rate.py measures on the MI355X"
    B, N, T, R = args.rods, args.N, args.steps, args.repeats
    dev = "cuda:0"
    r = CosseratRod(use_fsolve=True)
    setup_robot(r)
    r.N = N
    r.compute_intermediate_terms()
    h = r._native()
    ctl = torch.as_tensor(orc.batch_sine_controls(B, T, r.del_t, 1911), device=dev).contiguous()
    states = h.new_state(B, torch.float64, n_slots=T + 1)
    h.init_straight(states[0])
    G = torch.zeros((B, 6), dtype=torch.float64, device=dev)
    tip = torch.empty((B, T, 3), dtype=torch.float64, device=dev)
    status = torch.zeros((B, T), dtype=torch.int32, device=dev)
    g0 = torch.zeros_like(states)
    g0[1:, :, N - 1, 12:15] = 1.0
    g = g0.clone()
    g_ctl = torch.empty((B, T, 4), dtype=torch.float64, device=dev)
    g_bnd = torch.empty((B, kn.KR_BND), dtype=torch.float64, device=dev)
    resid = torch.empty((B, T), dtype=torch.float64, device=dev)
    ast = torch.empty((B, T), dtype=torch.int32, device=dev)
    stream = kn._stream()

    def forward():
        G.zero_()
        h.simulate(ctl, states, G, ring=False, tip=tip, status=status, tol=1e-12)

    def backward():
        g.copy_(g0)
        kn.check(h.lib.kr_simulate_vjp_batch(h._h, B, T, kn.KR_EULER, kn._ptr(ctl), kn._ptr(states), None, kn._ptr(g), None,
                                             kn._ptr(g_ctl), kn._ptr(g_bnd), kn._ptr(resid), kn._ptr(ast), 0, kn.KR_F64, stream))

    legs = {"kr_simulate_batch": forward, "kr_simulate_vjp_batch": backward}
    forward()
    backward()
    torch.cuda.synchronize()
    checked = dict(forward_status_zero=bool((status == 0).all()), adjoint_status_zero=bool((ast == 0).all()),
                   resid_max=float(resid.max()), g_ctl_finite=bool(torch.isfinite(g_ctl).all()))
    assert checked["forward_status_zero"] and checked["adjoint_status_zero"] and checked["resid_max"] <= 1e-10, checked

    def event_ms(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:  # the clock ramp
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
    n_launch = {k: max(3, int(np.ceil(args.window * 1e3 / event_ms(fn, 1)))) for k, fn in legs.items()}
    times = {k: [] for k in legs}
    for _ in range(R):
        for k, fn in legs.items():
            times[k].append(event_ms(fn, n_launch[k]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    fwd, bwd = med["kr_simulate_batch"], med["kr_simulate_vjp_batch"]
    res = dict(
        B=B, N=N, T=T, dtype="f64", repeats=R, launches_per_timing=n_launch, device=torch.cuda.get_device_name(0), checked=checked,
        last_sim_path=h.get_option("last_sim_path"),
        ms={k: dict(median=round(med[k], 4), all=[round(x, 4) for x in v]) for k, v in times.items()},
        M_rod_steps_per_s={k: round(B * T / med[k] / 1e3, 3) for k in legs},
        backward_over_forward=round(bwd / fwd, 3),
        finite_difference_route=dict(forward_rollouts=4 * T + 1, computed_ms=round((4 * T + 1) * fwd, 2),
                                     over_forward_plus_backward=round((4 * T + 1) * fwd / (fwd + bwd), 1),
                                     note="computed from the forward leg, not run"),
    )
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
