#!/usr/bin/env python3
"""What the table form of the rollout adjoint costs beside the handle's (not bench.py; one process, one GPU; run it under a
time limit of its own: `timeout -k 10 300 python tools/table_adjoint_rate.py ...`).

    python tools/table_adjoint_rate.py [--out profiles/<tag>_table_adjoint_rate.json] [--rods 1024] [--N 100] [--steps 64] [--repeats 3]

B rods, N grid points, T steps, fp64, MLP off, sine tensions per rod, a tip cotangent on every step, every buffer allocated
beforehand.  After a clock ramp (two seconds of the legs themselves), HIP-event durations of back-to-back calls - as many per
leg as fill `--window` seconds -, the legs alternating per round, medians of the rounds:
  (a) kr_simulate_vjp_batch on the handle                               (the parent's call, the yardstick)
  (b) kr_simulate_vjp_table_batch, a table of B identical rows = the handle's parameters, on the same stored rollout
  (c) the same with the eight presets of knode.setup_robot cycled over the rods, on the rollout of that table
  (d) kr_simulate_vjp_par_batch with g_par on the handle                (the yardstick of (e))
  (e) (b) with g_par
  (f) (b) with bnd_per_step = 1
Acceptance (the rule of profiles/r17a_*): rate(b) >= rate(a) x (1 - repeat spread of (a) - 0.02), and (e) likewise against (d);
the margin is the spread plus what another base address and reloads through it may cost, judged against the handle's call in
the same process.  The verdicts are REPORTED (`accept`), never enforced: a miss is a finding.  Before anything is timed the
calls are checked: every status 0, resid <= 1e-10, and (b), (e), (f) against (a), (d) bit for bit where the rows are the
handle's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "knode-cosserat_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

PRESETS = (None, "noair", "nsw", "short", "damping", "dampstiff", "lengthstiff", "youngs")


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

    assert torch.cuda.is_available(), "table_adjoint_rate.py measures on the MI355X"
    B, N, T, R = args.rods, args.N, args.steps, args.repeats
    dev = "cuda:0"

    def robot(mod):
        r = CosseratRod(use_fsolve=True)
        setup_robot(r, mod)
        r.N = N
        r.compute_intermediate_terms()
        return r
    robots = [robot(m) for m in PRESETS]
    h = robots[0]._native()
    t_same = h.param_table([robots[0]._params()] * B)
    t_mixed = h.param_table([robots[b % len(PRESETS)]._params() for b in range(B)])
    ctl = torch.as_tensor(orc.batch_sine_controls(B, T, robots[0].del_t, 1911), device=dev).contiguous()
    new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
    status = torch.zeros((B, T), dtype=torch.int32, device=dev)

    def forward(table):
        states = h.new_state(B, torch.float64, n_slots=T + 1)
        h.init_straight(states[0], table=table)
        G = torch.zeros((B, 6), dtype=torch.float64, device=dev)
        h.simulate(ctl, states, G, ring=False, status=status, tol=1e-12, table=table)
        torch.cuda.synchronize()
        return states, bool((status == 0).all())
    (states, ok), (states_mixed, ok_mixed) = forward(None), forward(t_mixed)
    assert ok, "the handle's forward run did not converge"
    g0 = torch.zeros_like(states)
    g0[1:, :, N - 1, 12:15] = 1.0
    g = g0.clone()
    g_ctl, g_bnd, g_bnd_t, g_par = new(B, T, 4), new(B, kn.KR_BND), new(B, T, kn.KR_BND), new(B, kn.KR_PAR)
    resid, ast = new(B, T), new(B, T, dtype=torch.int32)
    stream, p = kn._stream(), kn._ptr

    def handle(with_par):
        g.copy_(g0)
        if with_par:
            kn.check(h.lib.kr_simulate_vjp_par_batch(h._h, B, T, kn.KR_EULER, p(ctl), p(states), None, p(g), None, p(g_ctl), p(g_bnd),
                                                     p(g_par), p(resid), p(ast), kn.KR_F64, stream))
        else:
            kn.check(h.lib.kr_simulate_vjp_batch(h._h, B, T, kn.KR_EULER, p(ctl), p(states), None, p(g), None, p(g_ctl), p(g_bnd),
                                                 p(resid), p(ast), 0, kn.KR_F64, stream))

    def table(t, st, with_par=False, per_step=False):
        g.copy_(g0)
        kn.check(h.lib.kr_simulate_vjp_table_batch(h._h, t._t, T, kn.KR_EULER, p(ctl), p(st), None, p(g), None, p(g_ctl),
                                                   p(g_bnd_t if per_step else g_bnd), int(per_step), p(g_par) if with_par else None,
                                                   p(resid), p(ast), kn.KR_F64, stream))

    legs = {"a_handle": lambda: handle(False), "b_table_identical_rows": lambda: table(t_same, states),
            "c_table_eight_presets": lambda: table(t_mixed, states_mixed), "d_handle_g_par": lambda: handle(True),
            "e_table_identical_rows_g_par": lambda: table(t_same, states, with_par=True),
            "f_table_identical_rows_bnd_per_step": lambda: table(t_same, states, per_step=True)}
    checked, ref = {"forward_status_zero": ok, "forward_eight_presets_status_zero": ok_mixed}, {}
    for k, fn in legs.items():
        fn()
        torch.cuda.synchronize()
        checked[k + "_status_zero"], checked[k + "_resid_max"] = bool((ast == 0).all()), float(resid.max())
        assert k.startswith("c_") or (checked[k + "_status_zero"] and checked[k + "_resid_max"] <= 1e-10), (k, checked)
        ref[k] = (g_ctl.clone(), g.clone(), g_par.clone())
    same = lambda x, y, i: bool(torch.equal(ref[x][i], ref[y][i]))
    checked["b_equals_a_bit_for_bit"] = same("a_handle", "b_table_identical_rows", 0) and same("a_handle", "b_table_identical_rows", 1)
    checked["e_equals_d_bit_for_bit"] = all(same("d_handle_g_par", "e_table_identical_rows_g_par", i) for i in range(3))
    checked["f_equals_b_bit_for_bit"] = same("b_table_identical_rows", "f_table_identical_rows_bnd_per_step", 0)
    checked["largest_rel_difference_b_a"] = float(((ref["a_handle"][0] - ref["b_table_identical_rows"][0]).abs().max() / ref["a_handle"][0].abs().max()))
    checked["largest_rel_difference_g_par_e_d"] = float(((ref["d_handle_g_par"][2] - ref["e_table_identical_rows_g_par"][2]).abs()
                                                        / ref["d_handle_g_par"][2].abs().clamp_min(1e-300)).max())

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
    spread = lambda k: (max(times[k]) - min(times[k])) / med[k]
    rate = {k: B * T / med[k] / 1e3 for k in legs}

    def verdict(new_leg, base):
        need = rate[base] * (1.0 - spread(base) - 0.02)
        return dict(rate=round(rate[new_leg], 3), yardstick=round(rate[base], 3), yardstick_repeat_spread=round(spread(base), 4),
                    needed=round(need, 3), ratio=round(rate[new_leg] / rate[base], 4), met=bool(rate[new_leg] >= need))
    res = dict(B=B, N=N, T=T, dtype="f64", repeats=R, launches_per_timing=n_launch, device=torch.cuda.get_device_name(0), checked=checked,
               ms={k: dict(median=round(med[k], 4), all=[round(x, 4) for x in v]) for k, v in times.items()},
               M_rod_steps_per_s={k: round(v, 3) for k, v in rate.items()},
               accept=dict(b_against_a=verdict("b_table_identical_rows", "a_handle"),
                           e_against_d=verdict("e_table_identical_rows_g_par", "d_handle_g_par")),
               c_over_b=round(med["c_table_eight_presets"] / med["b_table_identical_rows"], 4),
               f_over_b=round(med["f_table_identical_rows_bnd_per_step"] / med["b_table_identical_rows"], 4))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
