#!/usr/bin/env python3
"""What soft-DTW on the device costs next to the exact DTW it softens (not bench.py; one process, one GPU; run it under a
time limit of its own: `timeout -k 10 300 python tools/softdtw_rate.py ...`).  Reported, not gated.

    python tools/softdtw_rate.py [--out profiles/<tag>_softdtw_rate.json] [--rods 1024] [--len 101] [--repeats 3]

Inputs: B pairs of random walks (step 2e-3 around 0.1) of `--len` samples a side, fp64, the same arrays for every leg, gamma
1e-2, L1.  After a clock ramp (two seconds of the legs themselves), HIP-event durations of `--launches` back-to-back calls
through the C ABI with every buffer allocated beforehand, the legs alternating per round, medians of the rounds:
  (a) kr_dtw_batch on the same inputs: the yardstick,
  (b) kr_softdtw_batch, value only (g_a = NULL),
  (c) kr_softdtw_batch, value and gradient.
Before anything is timed the values and gradients of 8 rods are compared with krod_eval.softdtw_grad (largest differences
reported, relative to the largest entry)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "knode-cosserat_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

HOST_RODS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rods", type=int, default=1024)
    ap.add_argument("--len", type=int, default=101)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--gamma", type=float, default=1e-2)
    args = ap.parse_args()
    import torch
    import krod_native as kn
    from cosserat_ode import CosseratRod
    from knode import setup_robot
    from krod_eval import softdtw_grad

    assert torch.cuda.is_available(), "softdtw_rate.py measures on the MI355X"
    B, T, R, n_launch, gamma = args.rods, args.len, args.repeats, args.launches, args.gamma
    dev = "cuda:0"
    r = CosseratRod(use_fsolve=True)
    setup_robot(r)
    r.N = 10
    r.compute_intermediate_terms()
    h = r._native()
    lib, stream = h.lib, kn._stream()
    rng = np.random.default_rng(1811)
    a = 0.1 + np.cumsum(2e-3 * rng.standard_normal((B, T, 3)), axis=1)
    b = 0.1 + np.cumsum(2e-3 * rng.standard_normal((B, T, 3)), axis=1)
    ad, bd = torch.as_tensor(a, device=dev).contiguous(), torch.as_tensor(b, device=dev).contiguous()
    value = torch.empty((B,), dtype=torch.float64, device=dev)
    g = torch.empty((B, T, 3), dtype=torch.float64, device=dev)
    ws_bytes = int(lib.kr_softdtw_ws_bytes(B, T, T, 1))
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    med = lambda v: float(np.median(v))

    def exact():
        kn.check(lib.kr_dtw_batch(h._h, B, kn._ptr(ad), T, 3 * T, 3, kn._ptr(bd), T, 3 * T, 3, kn._ptr(value), kn.KR_F64, stream))

    def soft(grad):
        kn.check(lib.kr_softdtw_batch(h._h, B, kn._ptr(ad), T, 3 * T, 3, kn._ptr(bd), T, 3 * T, 3, gamma, 0, kn._ptr(value),
                                      kn._ptr(g) if grad else None, 3 * T, 3, kn._ptr(ws), kn.KR_F64, stream))

    legs = {"kr_dtw_batch": exact, "kr_softdtw_batch_value": lambda: soft(False), "kr_softdtw_batch_value_grad": lambda: soft(True)}

    # checked before anything is timed
    n_host = min(HOST_RODS, B)
    soft(True)
    got_v, got_g = value.cpu().numpy().copy(), g.cpu().numpy().copy()
    host = [softdtw_grad(a[k], b[k], gamma, "l1") for k in range(n_host)]
    dv = max(abs(got_v[k] - host[k][0]) / abs(host[k][0]) for k in range(n_host))
    dg = max(float(np.abs(got_g[k] - host[k][1]).max() / np.abs(host[k][1]).max()) for k in range(n_host))

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n_launch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n_launch

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:  # the clock ramp
        for fn in legs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(R):
        for k, fn in legs.items():
            times[k].append(event_us(fn))
    kernel_us = {k: dict(median=round(med(v), 3), all=[round(x, 3) for x in v]) for k, v in times.items()}
    ratio = lambda k: round(med(times[k]) / med(times["kr_dtw_batch"]), 3)
    cells = B * T * T
    res = dict(
        B=B, Ta=T, Tb=T, dtype="f64", gamma=gamma, cost="l1", repeats=R, launches_per_timing=n_launch,
        device=torch.cuda.get_device_name(0), workspace_bytes=ws_bytes, checked_on_rods=n_host,
        largest_relative_difference_to_host=dict(value=float(dv), gradient=dg), kernel_us=kernel_us,
        gcells_per_s={k: round(cells / med(v) * 1e-3, 2) for k, v in times.items()},
        ratio_to_exact_dtw=dict(value=ratio("kr_softdtw_batch_value"), value_grad=ratio("kr_softdtw_batch_value_grad")),
    )
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
