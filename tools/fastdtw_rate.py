#!/usr/bin/env python3
"""What FastDTW on the device costs next to the exact DTW it stands beside (not bench.py; one process, one GPU; run it
under a time limit of its own: `timeout -k 10 300 python tools/fastdtw_rate.py ...`).

    python tools/fastdtw_rate.py [--out profiles/<tag>_fastdtw_rate.json] [--rods 1024] [--len 101] [--repeats 3]

Inputs: B pairs of random walks (steps N(0, 0.01)) of `--len` samples a side, fp64, the same arrays for every leg.  After
a clock ramp (two seconds of the legs themselves), HIP-event durations of `--launches` back-to-back calls through the
C ABI with every buffer allocated beforehand, the legs alternating per round, medians of the rounds:
  (a) kr_dtw_batch, the parent's kernel: the yardstick,
  (b) kr_fastdtw_batch radius 1, distance only,
  (c) ... radius 1 with the path,
  (d) ... radius 3, distance only,
  (e) (a) and (b) at B = 8.
No ratio is set in advance; `ratio_to_exact` reports (b) / (a).  Before anything is timed the distances of 32 rods are
compared bit for bit with krod_eval.fastdtw_distance, and the number of rods whose FastDTW differs from the exact DTW is
reported.
Wall time of knode.simulate_bank (B rods over 8 robots with two networks, T = 100, N = 100, tip-only with the tip as the
one key point) scored with either metric, and unscored: medians of the repeats; `fastdtw_minus_dtw_s` against
`dtw_spread_s` + 1 ms is the acceptance the change set itself.
The host path the device call replaces: krod_eval.fastdtw_distance timed on 32 rods and SCALED to B (the output says
so)."""
import argparse
import ctypes as C
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
    ap.add_argument("--len", type=int, default=101)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--no-bank", action="store_true", help="skip the simulate_bank legs")
    args = ap.parse_args()
    import torch
    import cosserat_oracle as orc
    import krod_native as kn
    from cosserat_ode import CosseratRod
    from knode import setup_robot, simulate_bank, simulate_batch
    from krod_eval import dtw_distance, fastdtw_distance

    assert torch.cuda.is_available(), "fastdtw_rate.py measures on the MI355X"
    B, T, R, n_launch = args.rods, args.len, args.repeats, args.launches
    dev = "cuda:0"

    def robot(N, mod=None):
        r = CosseratRod(use_fsolve=True)
        setup_robot(r, mod)
        r.N = N
        r.compute_intermediate_terms()
        return r

    h = robot(10)._native()
    lib, stream = h.lib, kn._stream()
    rng = np.random.default_rng(1811)
    a = np.cumsum(rng.normal(size=(B, T, 3)) * 0.01, axis=1)
    b = np.cumsum(rng.normal(size=(B, T, 3)) * 0.01, axis=1)
    ad, bd = torch.as_tensor(a, device=dev).contiguous(), torch.as_tensor(b, device=dev).contiguous()
    dist = torch.empty((B,), dtype=torch.float64, device=dev)
    steps = torch.zeros((B, 2 * T - 1, 2), dtype=torch.int32, device=dev)
    plen = torch.zeros((B,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(int(lib.kr_fastdtw_ws_bytes(B, T, T, 3)), 16),), dtype=torch.uint8, device=dev)
    med = lambda v: float(np.median(v))

    def exact(n):
        kn.check(lib.kr_dtw_batch(h._h, n, kn._ptr(ad), T, 3 * T, 3, kn._ptr(bd), T, 3 * T, 3, kn._ptr(dist), kn.KR_F64, stream))

    def fast(n, radius, path):
        kn.check(lib.kr_fastdtw_batch(h._h, n, kn._ptr(ad), T, 3 * T, 3, kn._ptr(bd), T, 3 * T, 3, radius, kn._ptr(dist),
                                      kn._ptr(steps) if path else None, kn._ptr(plen) if path else None, kn._ptr(ws), kn.KR_F64,
                                      stream))

    legs = {
        "kr_dtw_batch": lambda: exact(B),
        "kr_fastdtw_batch_r1": lambda: fast(B, 1, False),
        "kr_fastdtw_batch_r1_path": lambda: fast(B, 1, True),
        "kr_fastdtw_batch_r3": lambda: fast(B, 3, False),
        "kr_dtw_batch_B8": lambda: exact(8),
        "kr_fastdtw_batch_r1_B8": lambda: fast(8, 1, False),
    }

    # checked before anything is timed
    n_host = min(HOST_RODS, B)
    fast(B, 1, False)
    got_fast = dist.cpu().numpy().copy()
    exact(B)
    got_exact = dist.cpu().numpy().copy()
    host_fast = np.array([fastdtw_distance(a[r], b[r]) for r in range(n_host)])
    bitwise = bool(np.array_equal(got_fast[:n_host], host_fast))
    differ = int(np.count_nonzero(got_fast != got_exact))

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
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(R):
        for k, fn in legs.items():
            times[k].append(event_us(fn))
    kernel_us = {k: dict(median=round(med(v), 3), all=[round(x, 3) for x in v]) for k, v in times.items()}
    ratio = lambda k, base: round(med(times[k]) / med(times[base]), 3)

    host_s = []
    for _ in range(R):
        t0 = time.perf_counter()
        for r in range(n_host):
            fastdtw_distance(a[r], b[r])
        host_s.append(time.perf_counter() - t0)

    res = dict(
        B=B, Ta=T, Tb=T, dtype="f64", repeats=R, launches_per_timing=n_launch, device=torch.cuda.get_device_name(0),
        checked_on_rods=n_host, fastdtw_bitwise_equal_to_host=bitwise, rods_where_fastdtw_differs_from_dtw=differ,
        kernel_us=kernel_us,
        ratio_to_exact=dict(r1=ratio("kr_fastdtw_batch_r1", "kr_dtw_batch"), r1_path=ratio("kr_fastdtw_batch_r1_path", "kr_dtw_batch"),
                            r3=ratio("kr_fastdtw_batch_r3", "kr_dtw_batch"), r1_B8=ratio("kr_fastdtw_batch_r1_B8", "kr_dtw_batch_B8")),
        host_fastdtw_s=dict(rods=n_host, seconds=[round(s, 4) for s in host_s], scaled_to_B=round(med(host_s) * B / n_host, 3),
                            note=f"krod_eval.fastdtw_distance timed on {n_host} rods and SCALED by {B / n_host:g} to B = {B}"),
    )

    if not args.no_bank:
        N, Ts = 100, 100
        carrier = robot(N)
        nets = [orc.make_mlp([28, 64, 64, 25], "elu", seed=100 + k) for k in range(2)]
        names = {orc.ACT_TANH: "Tanh()", orc.ACT_SOFTPLUS: "Softplus(beta=1.0, threshold=20.0)", orc.ACT_RELU: "ReLU()",
                 orc.ACT_ELU: "ELU(alpha=1.0)"}
        eight = []
        for k, mod in enumerate([None, "noair", "nsw", "short", "damping", "dampstiff", "lengthstiff", "youngs"]):
            r = robot(N, mod)
            m = nets[k % 2]
            model, params = [], []
            for W, bb, act in zip(m.weights, m.biases, m.acts):
                model.append(f"Linear(in_features={W.shape[1]}, out_features={W.shape[0]}, bias=True)")
                params += [W, bb]
                if act != orc.ACT_NONE:
                    model.append(names[act])
            r.nn_model, r.param_ls, r.nn_path, r.nn_input_history = model, params, "whatever", m.history
            eight.append(r)
        robots = [eight[i % 8] for i in range(B)]
        ctl = orc.batch_sine_controls(B, Ts, carrier.del_t, 1235)
        ref = simulate_batch(robot(N), ctl[:1])["traj"][0, :Ts]
        kw = dict(tip_only=True, key_points=[N - 1])

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        runs = {
            "unscored": lambda: simulate_bank(carrier, robots, ctl, **kw),
            "scored_dtw": lambda: simulate_bank(carrier, robots, ctl, score={"reference": ref}, **kw),
            "scored_fastdtw": lambda: simulate_bank(carrier, robots, ctl, score={"reference": ref, "metric": "fastdtw"}, **kw),
        }
        for fn in runs.values():
            fn()  # first use, untimed
        secs = {k: [] for k in runs}
        for _ in range(R):
            for k, fn in runs.items():
                s, out = wall(fn)
                secs[k].append(s)
        spread = max(secs["scored_dtw"]) - min(secs["scored_dtw"])
        extra = med(secs["scored_fastdtw"]) - med(secs["scored_dtw"])
        res["simulate_bank"] = dict(
            B=B, T=Ts, N=N, seconds={k: [round(s, 5) for s in v] for k, v in secs.items()},
            dtw_spread_s=round(spread, 5), fastdtw_minus_dtw_s=round(extra, 5),
            accepted_extra_within_spread_plus_1ms=bool(extra <= spread + 1e-3), unconverged=int((out["status"] != 0).sum()))

    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
