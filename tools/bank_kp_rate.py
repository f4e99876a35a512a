#!/usr/bin/env python3
"""Rate of the bank key-point call next to the parent's bank call, and of an in-place bank refresh next to create +
destroy (not bench.py; one process, one GPU; run it under a time limit of its own:
`timeout -k 10 300 python tools/bank_kp_rate.py ...`).

    python tools/bank_kp_rate.py [--out profiles/<tag>_bank_kp_rate.json] [--steps 64] [--repeats 3]

After a clock ramp of the kind bench.py uses (RK4 launches of the persistent solver on a second handle), B = 1024,
N = 100, T = 64 on a 3-slot ring, a bank of eight networks 28 -> 64 -> 64 -> 25 (rod b runs network b mod 8), fp64 and
fp32, every run from the straight rod, the legs alternating per round so that all see the same clock:
  (a) kr_simulate_batch_bank, the parent,
  (b) the new call with constant rows (bnd = the rows' own base and wrench on every step) and K = 0,
  (c) ... with K = 4 at {33, 55, 77, 99},
  (d) ... with K = 16,
  (e) K = 0 with the `slide` base history of tests/base_motion_cases.py scaled per rod.
(b)'s tips are compared bit for bit with (a)'s once, untimed.  Times are HIP-event durations of the simulate call on the
stream; rates are rod-steps per second, medians of the rounds.
Acceptance, constant rows and K = 0: no slower than the parent's bank call by more than the max - min spread of that
call's own repeats plus 2 % (`const_rows_k0_vs_bank`: the median ratio, the spread, `accepted`).  The other legs are
reported, not bounded.
kr_mlp_bank_repack from device sources against kr_mlp_bank_create + kr_mlp_bank_destroy from the same sources, K = 8 and
K = 32: host wall time of the calls with the stream drained after them, medians of `--repeats` x 5 calls."""
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
    ap.add_argument("--steps", type=int, default=64)
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
    dev = "cuda:0"
    carrier = robot(N)
    h = carrier._native()
    h2 = robot(N)._native()  # ramp handle
    nets = [orc.make_mlp([28, 64, 64, 25], "elu", seed=100 + k) for k in range(32)]
    as_network = lambda m: (m.weights, m.biases, m.acts)
    net_of_rod = [b % 8 for b in range(B)]
    pts4 = [33 * N // 100, 55 * N // 100, 77 * N // 100, N - 1]
    pts16 = sorted({(k + 1) * N // 16 - 1 for k in range(16)})
    own = np.concatenate([np.asarray(x, float) for x in (carrier.p0, carrier.h0, carrier.q0, carrier.w0, carrier.F_tip, carrier.M_tip)])
    om = 2 * np.pi / (8 * carrier.del_t)
    t = np.arange(T) * carrier.del_t
    slide = np.broadcast_to(own, (B, T, 19)).copy()  # (the `slide` history: a carriage along x, amplitude scaled per rod)
    amp = 0.02 * (0.5 + np.arange(B) / B)
    slide[:, :, 0] = amp[:, None] * np.sin(om * t)[None]
    slide[:, :, 7] = amp[:, None] * om * np.cos(om * t)[None]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def ramp(seconds):
        c2 = torch.as_tensor(orc.batch_sine_controls(1024, 100, carrier.del_t, 7), device=dev).contiguous()
        s2, G2 = h2.new_state(1024, torch.float64, n_slots=3), torch.zeros((1024, 6), dtype=torch.float64, device=dev)
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

    res = dict(B=B, N=N, steps=T, repeats=R, device=torch.cuda.get_device_name(0), network="28-64-64-25 elu", bank_K=8,
               key_points4=pts4, key_points16=pts16)
    with h.param_table([carrier._params()] * B) as tab, h.mlp_bank([as_network(m) for m in nets[:8]]) as bank:
        for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
            up = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev).to(dt).contiguous()
            ctl = up(orc.batch_sine_controls(B, T, carrier.del_t, 1235))
            st, G = h.new_state(B, dt, n_slots=3), torch.zeros((B, 6), dtype=dt, device=dev)
            tip = torch.empty((B, T, 3), dtype=dt, device=dev)
            status = torch.zeros((B, T), dtype=torch.int32, device=dev)
            const, moved = up(np.broadcast_to(own, (B, T, 19))), up(slide)
            kp4 = torch.empty((T, B, len(pts4), 28), dtype=dt, device=dev)
            kp16 = torch.empty((T, B, len(pts16), 28), dtype=dt, device=dev)
            legs = {"bank": {}, "const_rows_k0": dict(bnd=const), "const_rows_k4": dict(bnd=const, key_points=pts4, kp=kp4),
                    "const_rows_k16": dict(bnd=const, key_points=pts16, kp=kp16), "slide_k0": dict(bnd=moved)}

            def run(key):
                h.init_straight(st[0], table=tab)
                G.zero_()
                secs = timed(lambda: h.simulate(ctl, st, G, ring=True, tip=tip, status=status, table=tab, bank=bank, net_of_rod=net_of_rod,
                                                **legs[key]))
                return secs, int((status != 0).sum())

            first = {}
            for key in legs:  # first use of every kernel instantiation, untimed
                run(key)
                first[key] = tip.clone()
            r = dict(const_rows_k0_tips_bit_identical_to_bank=bool(torch.equal(first["bank"], first["const_rows_k0"])),
                     key_point_tips_bit_identical_to_bank=bool(torch.equal(first["bank"], first["const_rows_k4"]) and
                                                               torch.equal(first["bank"], first["const_rows_k16"])))
            ramp(0.8)
            secs = {k: [] for k in legs}
            bad = {k: 0 for k in legs}
            for _ in range(R):
                for key in legs:
                    s, nb = run(key)
                    secs[key].append(s)
                    bad[key] += nb
            for k, v in secs.items():
                r[k] = dict(stats(v), unconverged=bad[k])
            a, b = r["bank"]["rod_steps_per_s"], r["const_rows_k0"]["rod_steps_per_s"]
            spread = (a["max"] - a["min"]) / a["median"]
            ratio = b["median"] / a["median"]
            r["const_rows_k0_vs_bank"] = dict(median_ratio=round(ratio, 4), bank_min_max_spread=round(spread, 4),
                                              accepted=bool(ratio >= 1.0 - spread - 0.02))
            for k in ("const_rows_k4", "const_rows_k16", "slide_k0"):
                r[k + "_vs_bank"] = dict(median_ratio=round(r[k]["rod_steps_per_s"]["median"] / a["median"], 4))
            res[name] = r
    # in-place refresh against create + destroy, device sources
    res["repack"] = {}
    for K in (8, 32):
        srcs = [([torch.as_tensor(w, device=dev).contiguous() for w in m.weights], [torch.as_tensor(b, device=dev).contiguous() for b in m.biases],
                 m.acts) for m in nets[:K]]
        torch.cuda.synchronize()

        def wall(fn):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        with h.mlp_bank(srcs) as bk:
            bk.repack(srcs)
            torch.cuda.synchronize()
            rep = [wall(lambda: bk.repack(srcs)) for _ in range(5 * R)]
        new = [wall(lambda: h.mlp_bank(srcs).close()) for _ in range(5 * R)]
        res["repack"][f"K{K}"] = dict(repack_ms=round(1e3 * float(np.median(rep)), 4), create_destroy_ms=round(1e3 * float(np.median(new)), 4),
                                      ratio=round(float(np.median(new) / np.median(rep)), 2))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
