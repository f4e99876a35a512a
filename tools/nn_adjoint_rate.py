#!/usr/bin/env python3
"""What the backward pass through the KNODE model (physics plus the residual MLP in every sweep) costs (not bench.py; one
process, one GPU; run it under a time limit of its own: `timeout -k 10 500 python tools/nn_adjoint_rate.py ...`).

    python tools/nn_adjoint_rate.py [--out profiles/<tag>_nn_adjoint_rate.json] [--rods 1024] [--N 100] [--steps 64] [--repeats 3]

B rods, N grid points, T steps, fp64, sine tensions per rod, networks 28->64->64->25 and 28->512->25 (elu, signed weights
gain N(0, 1) / sqrt(fan_in)), every buffer allocated beforehand.  After a clock ramp, HIP-event durations of back-to-back
calls, the legs alternating per round, medians of the rounds.  Legs, per network:
  forward_nn     kr_simulate_batch with the MLP on and the full history (tol 1e-12)
  backward_nn    kr_simulate_vjp_nn_batch over that history with a tip cotangent on every step, rows emitted
  jacobian       T calls of kr_mlp_input_jacobian_batch on the Q = B (N - 1) rows of a step: the Jacobian launches of the
                 backward pass, through the public entry point (same kernel, the row-major store)
  weights        krod_grad.weight_grads over the emitted rows (kr_mlp_forward + kr_mlp_backward, fp32)
and once: backward_off, the parent's kr_simulate_vjp_batch (MLP off) on the same shapes, and forward_off.
The rows kernel, the recursion and the accumulations have no entry point of their own and are NOT measured one by one:
`rows`, `adjoint`, `adds` are reported as "not measured", and `backward_nn_minus_jacobian` is the difference of two measured
legs, computed, for all three together (the jacobian leg stores row-major, the backward pass column-major).  No target is set in advance.  Before anything is timed the calls are checked: every adjoint status 0
where the forward status is 0, resid <= 1e-10."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "knode-cosserat_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def signed_net(hidden, gain, seed):
    rng = np.random.default_rng(seed)
    sizes = [28, *hidden, 25]
    Ws = [(gain * rng.normal(size=(sizes[k + 1], sizes[k])) / np.sqrt(sizes[k])).astype(np.float32) for k in range(len(sizes) - 1)]
    bs = [(0.05 * rng.normal(size=(sizes[k + 1],))).astype(np.float32) for k in range(len(sizes) - 1)]
    return Ws, bs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rods", type=int, default=1024)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--gain", type=float, default=0.2)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per timing")
    args = ap.parse_args()
    import torch
    import cosserat_oracle as orc
    import krod_grad as kg
    import krod_native as kn
    from cosserat_ode import CosseratRod
    from knode import setup_robot

    assert torch.cuda.is_available(), "nn_adjoint_rate.py measures on the MI355X"
    B, N, T, R = args.rods, args.N, args.steps, args.repeats
    dev = "cuda:0"
    r = CosseratRod(use_fsolve=True)
    setup_robot(r)
    r.N = N
    r.compute_intermediate_terms()
    h = r._native()
    f64 = torch.float64
    ctl = torch.as_tensor(orc.batch_sine_controls(B, T, r.del_t, 1911), device=dev).contiguous()
    states = h.new_state(B, f64, n_slots=T + 1)
    h.init_straight(states[0])
    G = torch.zeros((B, 6), dtype=f64, device=dev)
    tip = torch.empty((B, T, 3), dtype=f64, device=dev)
    status = torch.zeros((B, T), dtype=torch.int32, device=dev)
    g0 = torch.zeros_like(states)
    g0[1:, :, N - 1, 12:15] = 1.0
    g = g0.clone()
    g_ctl = torch.empty((B, T, 4), dtype=f64, device=dev)
    g_bnd = torch.empty((B, kn.KR_BND), dtype=f64, device=dev)
    resid = torch.empty((B, T), dtype=f64, device=dev)
    ast = torch.empty((B, T), dtype=torch.int32, device=dev)
    nn_x = torch.empty((T, B, N - 1, 32), dtype=f64, device=dev)
    nn_g = torch.empty_like(nn_x)
    Q = B * (N - 1)
    jac = torch.empty((Q, 25, 28), dtype=f64, device=dev)
    stream = kn._stream()
    use_nn = [False]

    def forward():
        G.zero_()
        h.simulate(ctl, states, G, ring=False, tip=tip, status=status, tol=1e-12, use_nn=use_nn[0])

    def backward_off():
        g.copy_(g0)
        kn.check(h.lib.kr_simulate_vjp_batch(h._h, B, T, kn.KR_EULER, kn._ptr(ctl), kn._ptr(states), None, kn._ptr(g), None,
                                             kn._ptr(g_ctl), kn._ptr(g_bnd), kn._ptr(resid), kn._ptr(ast), 0, kn.KR_F64, stream))

    def backward_nn():
        g.copy_(g0)
        kn.check(h.lib.kr_simulate_vjp_nn_batch(h._h, B, T, kn.KR_EULER, kn._ptr(ctl), kn._ptr(states), None, kn._ptr(g), None,
                                                kn._ptr(g_ctl), kn._ptr(g_bnd), kn._ptr(resid), kn._ptr(ast), kn._ptr(nn_x),
                                                kn._ptr(nn_g), kn.KR_F64, stream))

    xq = [None]

    def jacobian():
        for _ in range(T):
            kn.check(h.lib.kr_mlp_input_jacobian_batch(h._h, Q, kn._ptr(xq[0]), kn._ptr(jac), kn.KR_F64, stream))

    def event_ms(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def measure(legs):
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
        return {k: dict(median=round(float(np.median(v)), 4), all=[round(x, 4) for x in v], launches=n_launch[k]) for k, v in times.items()}

    def check(tag):
        torch.cuda.synchronize()
        ok_fwd = status == 0
        c = dict(forward_status_zero=int(ok_fwd.sum()), of=B * T, adjoint_status_zero_where_forward_is=bool((ast[ok_fwd] == 0).all()),
                 resid_max=float(resid[ast == 0].max()), g_ctl_finite_rods=int(torch.isfinite(g_ctl).all(dim=2).all(dim=1).sum()))
        assert c["adjoint_status_zero_where_forward_is"] and c["resid_max"] <= 1e-10, (tag, c)
        return c

    res = dict(B=B, N=N, T=T, dtype="f64", repeats=R, gain=args.gain, device=torch.cuda.get_device_name(0), networks={})
    forward()
    backward_off()
    res["mlp_off"] = dict(checked=check("off"), ms=measure({"forward_off": forward, "backward_off": backward_off}))
    for name, hidden in (("28-64-64-25", (64, 64)), ("28-512-25", (512,))):
        Ws, bs = signed_net(hidden, args.gain, 7)
        acts = [kn.ACT_ELU] * len(hidden) + [kn.ACT_NONE]
        h.set_mlp(Ws, bs, acts)
        use_nn[0] = True
        forward()
        backward_nn()
        checked = check(name)
        xq[0] = nn_x[0].reshape(Q, 32)[:, :28].contiguous()
        p32 = []
        for W, b in zip(Ws, bs):
            p32 += [torch.as_tensor(W, device=dev), torch.as_tensor(b, device=dev)]
        legs = {"forward_nn": forward, "backward_nn": backward_nn, "jacobian": jacobian,
                "weights": lambda: kg.weight_grads(h, p32, acts, nn_x, nn_g)}
        ms = measure(legs)
        for part in ("rows", "adjoint", "adds"):
            ms[part] = "not measured"
        ms["backward_nn_minus_jacobian"] = dict(computed=round(ms["backward_nn"]["median"] - ms["jacobian"]["median"], 4),
                                                note="rows + adjoint + adds together: the difference of two measured legs, not timed")
        res["networks"][name] = dict(checked=checked, last_sim_path=h.get_option("last_sim_path"), ms=ms,
                                     per_step_ms={k: round(v["median"] / T, 4) for k, v in ms.items() if isinstance(v, dict) and "median" in v},
                                     backward_nn_over_backward_off=round(ms["backward_nn"]["median"] / res["mlp_off"]["ms"]["backward_off"]["median"], 3))
        use_nn[0] = False
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
