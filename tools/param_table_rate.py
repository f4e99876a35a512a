#!/usr/bin/env python3
"""Rate of the parameter-table kernels next to the plain ones (not bench.py; one process, one GPU).

    python tools/param_table_rate.py [--out profiles/<tag>_param_table.json] [--steps 1000] [--repeats 5]

After a clock ramp of the kind bench.py uses (RK4 launches of the persistent solver on a second handle), N = 100, fp64,
3-slot ring, every run from the straight rod:
  B = 1024:  (a) kr_simulate_batch, (b) the table call with 1024 identical rows, (c) the table call with the eight
             presets cycled over the batch - interleaved a, b, c per repeat so that all three see the same clock;
             plus every preset on its own as a table of 1024 identical rows (what each costs: a stiffer rod takes other
             sweep counts - the counters themselves need the -DKR_MS_STAMPS build, which does not cover the table units);
  B = 8:     one table launch of the eight presets against eight one-rod launches on eight handles.
Times are HIP-event durations of the simulate call(s) on the stream; rates are rod-steps per second."""
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
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
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

    def run(P, handle=None, table=None, rows_of=slice(None)):
        hh = handle or h
        st, G = P["st"][:, rows_of], P["G"][rows_of]
        if rows_of != slice(None):
            st, G = st.contiguous(), G.contiguous()
        hh.init_straight(st[0], table=table)
        G.zero_()
        ctl, status = P["ctl"][rows_of].contiguous(), P["status"][rows_of].contiguous()
        secs = timed(lambda: hh.simulate(ctl, st, G, ring=True, status=status, table=table))
        return secs, int((status != 0).sum())

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

    res = dict(N=N, steps=T, repeats=R, dtype="f64", ring=True, device=torch.cuda.get_device_name(0))
    # ---- B = 1024 ------------------------------------------------------------------------------------------------
    B = 1024
    P = problem(B)
    t_same = h.param_table([rows[0]] * B)
    t_mix = h.param_table([rows[b % 8] for b in range(B)])
    h.simulate_prepare(B, dt)
    for tab in (None, t_same, t_mix):  # first use of every kernel instantiation, untimed
        run(P, table=tab)
    ramp(0.8)
    secs = {"plain": [], "table_identical": [], "table_presets": []}
    bad = {k: 0 for k in secs}
    for _ in range(R):
        for key, tab in (("plain", None), ("table_identical", t_same), ("table_presets", t_mix)):
            s, nb = run(P, table=tab)
            secs[key].append(s)
            bad[key] += nb
    res["B1024"] = {k: dict(stats(v, B), unconverged=bad[k]) for k, v in secs.items()}
    a = res["B1024"]["plain"]["rod_steps_per_s"]
    b = res["B1024"]["table_identical"]["rod_steps_per_s"]
    res["B1024"]["table_identical_vs_plain"] = dict(median_ratio=round(b["median"] / a["median"], 4),
                                                    plain_min_max_spread=round((a["max"] - a["min"]) / a["median"], 4))
    per = {}
    for m, row in zip(PRESETS, rows):
        with h.param_table([row] * B) as tab:
            run(P, table=tab)
            per[str(m)] = stats([run(P, table=tab)[0] for _ in range(3)], B)["rod_steps_per_s"]
    res["B1024"]["each_preset_alone_as_table"] = per
    t_same.close()
    t_mix.close()
    # ---- B = 8: the use case's real baseline ---------------------------------------------------------------------
    P8 = problem(8)
    handles = [robot(m, N)._native() for m in PRESETS]
    t8 = h.param_table(rows)
    run(P8, table=t8)
    for b, hb in enumerate(handles):
        run(P8, handle=hb, rows_of=slice(b, b + 1))
    ramp(0.3)
    one, eight = [], []
    for _ in range(R):
        one.append(run(P8, table=t8)[0])
        eight.append(sum(run(P8, handle=hb, rows_of=slice(b, b + 1))[0] for b, hb in enumerate(handles)))
    res["B8"] = dict(one_table_launch=stats(one, 8), eight_one_rod_launches=stats(eight, 8),
                     speedup_median=round(float(np.median(eight) / np.median(one)), 3))
    t8.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
