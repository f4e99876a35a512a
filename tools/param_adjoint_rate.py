#!/usr/bin/env python3
"""What the gradient of the rod's material parameters costs over the backward pass it rides on (not bench.py; one process,
one GPU; run it under a time limit of its own: `timeout -k 10 300 python tools/param_adjoint_rate.py ...`).

    python tools/param_adjoint_rate.py [--out profiles/<tag>_param_adjoint_rate.json] [--rods 1024] [--N 100] [--steps 64] [--repeats 3]

B rods, N grid points, T steps, fp64, MLP off, sine tensions per rod (cosserat_oracle.batch_sine_controls), every buffer
allocated beforehand.  After a clock ramp (two seconds of the legs themselves), HIP-event durations of back-to-back calls - as
many per leg as fill `--window` seconds, counted from one trial call -, the legs alternating per round, medians of the rounds:
  (a) kr_simulate_batch with the full history (tol 1e-12: the states the adjoint is taken at),
  (b) kr_simulate_vjp_batch over that history with a tip cotangent on every step,
  (c) kr_simulate_vjp_par_batch with g_par == NULL (the same kernel as (b) by construction),
  (d) kr_simulate_vjp_par_batch with g_par.
Reported: every leg in ms and M rod-steps/s; (d) / (b), what the parameter gradient costs over the backward pass, next to
the spread of (b)'s own repeats; and the COMPUTED cost of the route (d) replaces - central differences in the 43
parameters, 2 x 43 + 1 = 87 forward rollouts = 87 x (a); it is not run.  No ratio is set in advance.  Before anything is
timed the calls are checked: every status 0, resid <= 1e-10, g_par finite, and (c), (d) give (b)'s g_ctl bit for bit."""
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

    assert torch.cuda.is_available(), "param_adjoint_rate.py measures on the MI355X"
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
    g_par = torch.empty((B, kn.KR_PAR), dtype=torch.float64, device=dev)
    stream = kn._stream()

    def forward():
        G.zero_()
        h.simulate(ctl, states, G, ring=False, tip=tip, status=status, tol=1e-12)

    def backward():
        g.copy_(g0)
        kn.check(h.lib.kr_simulate_vjp_batch(h._h, B, T, kn.KR_EULER, kn._ptr(ctl), kn._ptr(states), None, kn._ptr(g), None,
                                             kn._ptr(g_ctl), kn._ptr(g_bnd), kn._ptr(resid), kn._ptr(ast), 0, kn.KR_F64, stream))

    def backward_par(with_par):
        g.copy_(g0)
        kn.check(h.lib.kr_simulate_vjp_par_batch(h._h, B, T, kn.KR_EULER, kn._ptr(ctl), kn._ptr(states), None, kn._ptr(g), None,
                                                 kn._ptr(g_ctl), kn._ptr(g_bnd), kn._ptr(g_par) if with_par else None, kn._ptr(resid),
                                                 kn._ptr(ast), kn.KR_F64, stream))

    legs = {"kr_simulate_batch": forward, "kr_simulate_vjp_batch": backward,
            "kr_simulate_vjp_par_batch(g_par=NULL)": lambda: backward_par(False), "kr_simulate_vjp_par_batch": lambda: backward_par(True)}
    forward()
    backward()
    torch.cuda.synchronize()
    ref_ctl = g_ctl.clone()
    checked = dict(forward_status_zero=bool((status == 0).all()), adjoint_status_zero=bool((ast == 0).all()),
                   resid_max=float(resid.max()), g_ctl_finite=bool(torch.isfinite(g_ctl).all()))
    backward_par(False)
    checked["null_call_same_bits"] = bool(torch.equal(g_ctl, ref_ctl))
    backward_par(True)
    torch.cuda.synchronize()
    checked.update(par_call_same_bits=bool(torch.equal(g_ctl, ref_ctl)), par_status_zero=bool((ast == 0).all()),
                   g_par_finite=bool(torch.isfinite(g_par).all()))
    assert checked["forward_status_zero"] and checked["adjoint_status_zero"] and checked["resid_max"] <= 1e-10, checked
    assert checked["null_call_same_bits"] and checked["par_call_same_bits"] and checked["par_status_zero"] and checked["g_par_finite"], checked

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
    fwd, bwd, par = med["kr_simulate_batch"], med["kr_simulate_vjp_batch"], med["kr_simulate_vjp_par_batch"]
    spread = times["kr_simulate_vjp_batch"]
    res = dict(
        B=B, N=N, T=T, dtype="f64", repeats=R, launches_per_timing=n_launch, device=torch.cuda.get_device_name(0), checked=checked,
        last_sim_path=h.get_option("last_sim_path"),
        ms={k: dict(median=round(med[k], 4), all=[round(x, 4) for x in v]) for k, v in times.items()},
        M_rod_steps_per_s={k: round(B * T / med[k] / 1e3, 3) for k in legs},
        backward_over_forward=round(bwd / fwd, 3),
        par_over_backward=round(par / bwd, 3),
        null_over_backward=round(med["kr_simulate_vjp_par_batch(g_par=NULL)"] / bwd, 3),
        backward_repeat_spread=round((max(spread) - min(spread)) / bwd, 4),
        finite_difference_route=dict(forward_rollouts=2 * kn.KR_PAR + 1, computed_ms=round((2 * kn.KR_PAR + 1) * fwd, 2),
                                     over_forward_plus_par_backward=round((2 * kn.KR_PAR + 1) * fwd / (fwd + par), 1),
                                     note="computed from the forward leg, not run"),
    )
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
