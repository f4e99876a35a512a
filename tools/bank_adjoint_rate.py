#!/usr/bin/env python3
"""What the bank form of the rollout adjoint costs beside the handle's MLP-on call (not bench.py; one process, one GPU; run it
under a time limit of its own: `timeout -k 10 420 python tools/bank_adjoint_rate.py ...`).

    python tools/bank_adjoint_rate.py [--out profiles/<tag>_bank_adjoint_rate.json] [--rods 1024] [--N 100] [--steps 64] [--repeats 3]

B rods, N grid points, T steps, fp64, sine tensions per rod, a tip cotangent on every step, the rows of the weight gradient
emitted, every buffer allocated beforehand.  Per network shape - 28 -> 64 -> 64 -> 25 (the two-hidden-layer Jacobian kernel)
and 28 -> 512 -> 25 (the one-hidden-layer kernel over eight chunks) - after a clock ramp (two seconds of the legs themselves),
HIP-event durations of back-to-back calls - as many per leg as fill `--window` seconds -, the legs alternating per round,
medians of the rounds:
  (a) kr_simulate_vjp_nn_batch on the handle, its network = network 0                  (the parent's call, the yardstick)
  (b) kr_simulate_vjp_bank_batch, K = 1, a table of B identical rows = the handle's parameters, on the same stored rollout:
      one Jacobian launch per step either way, so only the row reads and the permutation (the identity) differ
  (c) kr_simulate_vjp_bank_batch, K = 8, rod b on network b % 8 (interleaved: the permutation moves every rod), on the stored
      rollout of that bank: eight Jacobian launches per step
Acceptance (the margin earlier bank work was given): time(b) <= time(a) x (1 + repeat spread of (a) + 0.02).  (c) is reported
without a bound.  The verdict is REPORTED (`accept`), never enforced: a miss is a finding.  Before anything is timed the calls
are checked: every status 0, resid, and (b) against (a) - the largest relative difference and whether it is bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "knode-cosserat_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

SHAPES = {"28x64x64x25": ((64, 64), 4), "28x512x25": ((512,), 4)}  # hidden widths, activation code (ELU)
K_MANY = 8


def network(hidden, act, seed, gain=0.05):
    """(weights, biases, acts) as Handle.set_mlp and MlpBank take them: fp32, signed, gain N(0, 1) / sqrt(fan_in)"""
    rng = np.random.default_rng(seed)
    sizes = [28, *hidden, 25]
    Ws = [(gain * rng.normal(size=(sizes[k + 1], sizes[k])) / np.sqrt(sizes[k])).astype(np.float32) for k in range(len(sizes) - 1)]
    bs = [(0.01 * rng.normal(size=(sizes[k + 1],))).astype(np.float32) for k in range(len(sizes) - 1)]
    return Ws, bs, [act] * len(hidden) + [0]


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

    assert torch.cuda.is_available(), "bank_adjoint_rate.py measures on the MI355X"
    B, N, T, R = args.rods, args.N, args.steps, args.repeats
    dev = "cuda:0"
    robot = CosseratRod(use_fsolve=True)
    setup_robot(robot, None)
    robot.N = N
    robot.compute_intermediate_terms()
    h = robot._native()
    table = h.param_table([robot._params()] * B)
    ctl = torch.as_tensor(orc.batch_sine_controls(B, T, robot.del_t, 1911), device=dev).contiguous()
    new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
    status = torch.zeros((B, T), dtype=torch.int32, device=dev)
    g_ctl, g_bnd, resid, ast = new(B, T, 4), new(B, kn.KR_BND), new(B, T), new(B, T, dtype=torch.int32)
    nn_x, nn_g = new(T, B, N - 1, 32), new(T, B, N - 1, 32)
    stream, p = kn._stream(), kn._ptr
    one = np.zeros(B, dtype=np.int32)
    many = (np.arange(B) % K_MANY).astype(np.int32)
    ip = lambda a: a.ctypes.data_as(kn.C.POINTER(kn.C.c_int32))
    res = dict(B=B, N=N, T=T, dtype="f64", repeats=R, device=torch.cuda.get_device_name(0), shapes={})

    for name, (hidden, act) in SHAPES.items():
        nets = [network(hidden, act, 100 + k) for k in range(K_MANY)]
        h.set_mlp(*nets[0])
        bank1, bank8 = h.mlp_bank(nets[:1]), h.mlp_bank(nets)

        def forward(**kw):
            states = h.new_state(B, torch.float64, n_slots=T + 1)
            h.init_straight(states[0], table=table)
            G = torch.zeros((B, 6), dtype=torch.float64, device=dev)
            h.simulate(ctl, states, G, ring=False, status=status, tol=1e-12, **kw)
            torch.cuda.synchronize()
            return states, bool((status == 0).all())
        (states, ok), (states8, ok8) = forward(use_nn=True), forward(table=table, bank=bank8, net_of_rod=many)
        g0 = torch.zeros_like(states)
        g0[1:, :, N - 1, 12:15] = 1.0
        g = g0.clone()

        def handle():
            g.copy_(g0)
            kn.check(h.lib.kr_simulate_vjp_nn_batch(h._h, B, T, kn.KR_EULER, p(ctl), p(states), None, p(g), None, p(g_ctl), p(g_bnd),
                                                    p(resid), p(ast), p(nn_x), p(nn_g), kn.KR_F64, stream))

        def banked(bank, nets_host, st):
            g.copy_(g0)
            kn.check(h.lib.kr_simulate_vjp_bank_batch(h._h, table._t, bank._b, ip(nets_host), T, kn.KR_EULER, p(ctl), p(st), None, p(g), None,
                                                      p(g_ctl), p(g_bnd), 0, p(resid), p(ast), p(nn_x), p(nn_g), kn.KR_F64, stream))
        legs = {"a_handle_nn": handle, "b_bank_K1_identical_rows": lambda: banked(bank1, one, states),
                "c_bank_K8_interleaved": lambda: banked(bank8, many, states8)}
        checked, ref = {"forward_status_zero": ok, "forward_K8_status_zero": ok8}, {}
        for k, fn in legs.items():
            fn()
            torch.cuda.synchronize()
            checked[k + "_status_zero"], checked[k + "_resid_max"] = bool((ast == 0).all()), float(resid.max())
            ref[k] = (g_ctl.clone(), g.clone(), nn_g.clone())
        a, b = ref["a_handle_nn"], ref["b_bank_K1_identical_rows"]
        checked["b_equals_a_bit_for_bit"] = all(bool(torch.equal(x, y)) for x, y in zip(a, b))
        checked["largest_rel_difference_b_a"] = float((a[0] - b[0]).abs().max() / a[0].abs().max())
        del ref, a, b

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
        spread = (max(times["a_handle_nn"]) - min(times["a_handle_nn"])) / med["a_handle_nn"]
        allowed = med["a_handle_nn"] * (1.0 + spread + 0.02)
        res["shapes"][name] = dict(
            launches_per_timing=n_launch, checked=checked,
            ms={k: dict(median=round(med[k], 4), all=[round(x, 4) for x in v]) for k, v in times.items()},
            M_rod_steps_per_s={k: round(B * T / med[k] / 1e3, 3) for k in legs},
            accept=dict(b_against_a=dict(ms=round(med["b_bank_K1_identical_rows"], 4), yardstick_ms=round(med["a_handle_nn"], 4),
                                         yardstick_repeat_spread=round(spread, 4), allowed_ms=round(allowed, 4),
                                         ratio=round(med["b_bank_K1_identical_rows"] / med["a_handle_nn"], 4),
                                         met=bool(med["b_bank_K1_identical_rows"] <= allowed))),
            c_over_b=round(med["c_bank_K8_interleaved"] / med["b_bank_K1_identical_rows"], 4),
            c_extra_ms_per_step=round((med["c_bank_K8_interleaved"] - med["b_bank_K1_identical_rows"]) / T, 5))
        torch.cuda.synchronize()
        bank1.close()
        bank8.close()
        del states, states8, g0, g
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
