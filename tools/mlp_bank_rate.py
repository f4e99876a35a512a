#!/usr/bin/env python3
"""Rate of the network-bank kernel next to its one-network table twin (not bench.py; one process, one GPU).

    python tools/mlp_bank_rate.py [--out profiles/<tag>_mlp_bank.json] [--steps 64] [--repeats 7]

After a clock ramp of the kind bench.py uses (RK4 launches of the persistent solver on a second handle), N = 100, fp64,
MLP on (28 -> 64 -> 64 -> 25, ELU), 3-slot ring, every run from the straight rod, every rod the plain preset:
  B = 1024:  (a) the one-network table call (kr_set_mlp + kr_simulate_batch_table: the parent's path), a bank of K = 1
             and a bank of K = 8 IDENTICAL networks cycled over the batch - the regression guard of the kernel prologue;
             (b) a bank of K = 8 DISTINCT networks cycled over the batch (the L2 footprint of eight weight sets).
             Interleaved per repeat so that all four see the same clock; the spread of the plain call's own repeats is
             reported next to every ratio.
  B = 8:     (c) eight (mod, network) pairs in one bank launch against eight kr_set_mlp + one-rod table launches on
             one handle (host time from the first call to the end of the last kernel: kr_set_mlp synchronises).
Times of (a), (b) are HIP-event durations of the simulate call on the stream; rates are rod-steps per second."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "knode-cosserat_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

PRESETS = [None, "noair", "nsw", "short", "damping", "dampstiff", "lengthstiff", "youngs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--nodes-per-rod", type=int, default=100)
    args = ap.parse_args()
    import torch
    import cosserat_oracle as orc
    from cosserat_ode import CosseratRod
    from knode import setup_robot

    def robot(mod, N):
        r = CosseratRod(use_fsolve=True)
        setup_robot(r, mod)
        r.N = N
        r.compute_intermediate_terms()
        return r

    N, T, R = args.nodes_per_rod, args.steps, args.repeats
    dev, dt = "cuda:0", torch.float64
    carrier = robot(None, N)
    h = carrier._native()
    h2 = robot(None, N)._native()  # ramp handle
    rows = [robot(m, N)._params() for m in PRESETS]
    nets = [orc.make_mlp([28, 64, 64, 25], "elu", seed=11 + k) for k in range(8)]
    net = lambda m: (m.weights, m.biases, m.acts)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def problem(B):
        ctl = torch.as_tensor(orc.batch_sine_controls(B, T, carrier.del_t, 1235), device=dev).contiguous()
        return dict(B=B, ctl=ctl, st=h.new_state(B, dt, n_slots=3), G=torch.zeros((B, 6), dtype=dt, device=dev),
                    status=torch.zeros((B, T), dtype=torch.int32, device=dev))

    def run(P, table, bank=None, idx=None, rows_of=slice(None), clock=timed):
        st, G = P["st"][:, rows_of], P["G"][rows_of]
        if rows_of != slice(None):
            st, G = st.contiguous(), G.contiguous()
        h.init_straight(st[0], table=table)
        G.zero_()
        ctl, status = P["ctl"][rows_of].contiguous(), P["status"][rows_of].contiguous()
        if bank is None:
            secs = clock(lambda: h.simulate(ctl, st, G, ring=True, status=status, table=table, use_nn=True))
        else:
            secs = clock(lambda: h.simulate(ctl, st, G, ring=True, status=status, table=table, bank=bank, net_of_rod=idx))
        return secs, int((status != 0).sum()), G.clone()

    def ramp(seconds):
        B = 1024
        ctl = torch.as_tensor(orc.batch_sine_controls(B, 100, carrier.del_t, 7), device=dev).contiguous()
        st, G = h2.new_state(B, dt, n_slots=3), torch.zeros((B, 6), dtype=dt, device=dev)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            for _ in range(8):
                h2.init_straight(st[0])
                G.zero_()
                h2.simulate(ctl, st, G, ring=True, scheme=1)  # KR_RK4
            torch.cuda.synchronize()

    def stats(secs, B):
        rates = [B * T / s for s in secs]
        return dict(rod_steps_per_s=dict(min=round(min(rates), 1), median=round(float(np.median(rates)), 1), max=round(max(rates), 1)),
                    seconds=[round(s, 6) for s in secs])

    res = dict(N=N, steps=T, repeats=R, dtype="f64", ring=True, mlp="28-64-64-25 elu", device=torch.cuda.get_device_name(0))
    # ---- B = 1024 ------------------------------------------------------------------------------------------------
    B = 1024
    P = problem(B)
    cyc = [b % 8 for b in range(B)]
    h.set_mlp(*net(nets[0]))
    tab = h.param_table([rows[0]] * B)
    bank1, bank8same, bank8 = h.mlp_bank([net(nets[0])]), h.mlp_bank([net(nets[0])] * 8), h.mlp_bank([net(m) for m in nets])
    legs = (("plain_one_network_table", None, None), ("bank_K1", bank1, [0] * B), ("bank_K8_identical", bank8same, cyc),
            ("bank_K8_distinct", bank8, cyc))
    first = {}
    for key, bk, idx in legs:  # first use of every kernel instantiation, untimed
        first[key] = run(P, tab, bk, idx)[2]
    res["identical_networks_bit_identical_G"] = bool(torch.equal(first["plain_one_network_table"], first["bank_K1"]) and
                                                     torch.equal(first["plain_one_network_table"], first["bank_K8_identical"]))
    ramp(0.8)
    secs = {k: [] for k, _, _ in legs}
    bad = {k: 0 for k in secs}
    for _ in range(R):
        for key, bk, idx in legs:
            s, nb, _ = run(P, tab, bk, idx)
            secs[key].append(s)
            bad[key] += nb
    res["B1024"] = {k: dict(stats(v, B), unconverged=bad[k]) for k, v in secs.items()}
    a = res["B1024"]["plain_one_network_table"]["rod_steps_per_s"]
    res["B1024"]["plain_min_max_spread"] = round((a["max"] - a["min"]) / a["median"], 4)
    for key in ("bank_K1", "bank_K8_identical", "bank_K8_distinct"):
        res["B1024"][key + "_vs_plain_median_ratio"] = round(res["B1024"][key]["rod_steps_per_s"]["median"] / a["median"], 4)
    for x in (tab, bank1, bank8same):
        x.close()
    # ---- B = 8: the use case -------------------------------------------------------------------------------------
    P8 = problem(8)
    t8 = h.param_table(rows)
    t1 = [h.param_table([r]) for r in rows]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def eight_launches():
        total = 0.0
        for b in range(8):
            total += wall(lambda: h.set_mlp(*net(nets[b])))
            total += run(P8, t1[b], rows_of=slice(b, b + 1), clock=wall)[0]
        return total

    def one_launch_with_upload():  # the bank built inside the timed region, as a caller that has only the weights pays it
        made = []
        t = wall(lambda: made.append(h.mlp_bank([net(m) for m in nets])))
        t += run(P8, t8, made[0], list(range(8)), clock=wall)[0]
        made[0].close()
        return t

    run(P8, t8, bank8, list(range(8)))
    eight_launches()
    ramp(0.3)
    one, one_up, eight = [], [], []
    for _ in range(R):
        one.append(run(P8, t8, bank8, list(range(8)), clock=wall)[0])
        one_up.append(one_launch_with_upload())
        eight.append(eight_launches())
    res["B8"] = dict(one_bank_launch=stats(one, 8), one_bank_launch_incl_bank_create=stats(one_up, 8),
                     eight_set_mlp_plus_one_rod_launches=stats(eight, 8),
                     speedup_median=round(float(np.median(eight) / np.median(one)), 3),
                     speedup_median_incl_bank_create=round(float(np.median(eight) / np.median(one_up)), 3))
    for x in [t8, bank8] + t1:
        x.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
