#!/usr/bin/env python3
"""Epoch time of a bank of trainings next to the same trainings queued one after the other (not bench.py; one process,
one GPU).

    python tools/train_bank_rate.py [--out profiles/<tag>_train_bank_rate.json] [--epochs 200] [--repeats 5]

Size: the reference's own training set - N = 10, T = 30 (29 window steps), key points [3, 5, 7, 9]: Q = 116 rows per
training (seeded synthetic rows: the kernels' time does not depend on the values).  Networks 28 -> 512 -> 25 and
28 -> 64 -> 64 -> 25; n_nets = 1, 8, 32, 128.  Both paths in this one process, after a clock ramp and 300 untimed epochs
of each:
  bank   `epochs` epochs of kr_train_bank_epochs (one call: 3 launches per epoch for all n_nets trainings);
  solo   `epochs` epochs of each of the n_nets trainings through kr_train_epochs on n_nets handles, queued back to back
         on the same stream (n_nets calls: 3 launches per epoch and training).
HIP-event durations on the stream, bank and solo alternating, `repeats` of each; min / median / max in microseconds per
epoch (of all n_nets trainings).  Two conditions are evaluated and written out, not enforced:
  n_nets = 1:   bank median <= solo median + (solo max - solo min);
  n_nets = 32:  bank median <  solo median - (solo max - solo min)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "knode-cosserat_amd"))

TANH = 1
K, S, DENOM = 4, 29, 29.0
ADAM = (0.9, 0.999, 1e-8, 0.0)          # beta1, beta2, eps, weight_decay
PLATEAU = (0.5, 80, 1e-4, 0.0)          # factor, patience, threshold, min_lr
SHAPES = {"28-512-25": [28, 512, 25], "28-64-64-25": [28, 64, 64, 25]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--nets", type=int, nargs="+", default=[1, 8, 32, 128])
    args = ap.parse_args()
    import torch
    import krod_native as kn
    dev = "cuda:0"
    lib = kn.load()
    p = kn.KrParams()
    kn.check(lib.kr_default_params(C.byref(p)))
    p.N = 10
    n_max = max(args.nets)
    handles = [kn.Handle(p) for _ in range(n_max)]
    ds = float(handles[0].derived().ds)
    Q = S * K

    def training(seed, dims):
        g = torch.Generator(device="cpu").manual_seed(seed)
        x = torch.zeros(Q, 32)
        x[:, :28] = 0.5 * torch.randn(Q, 28, generator=g)
        base = 0.3 * torch.randn(Q, 25, generator=g)
        base[:, 3:7] = torch.nn.functional.normalize(torch.randn(Q, 4, generator=g) + torch.tensor([2.0, 0, 0, 0]), dim=1)
        target = base + 0.05 * torch.randn(Q, 25, generator=g)
        ps = []
        for k in range(len(dims) - 1):
            b = 1.0 / np.sqrt(dims[k])
            ps += [((torch.rand(dims[k + 1], dims[k], generator=g) * 2 - 1) * b).reshape(-1),
                   (torch.rand(dims[k + 1], generator=g) * 2 - 1) * b]
        prm = torch.cat(ps)
        n = prm.numel()
        t = dict(x=x, base=base, target_rows=target, params=prm, grads=torch.zeros(n + 1), exp_avg=torch.zeros(n),
                 exp_avg_sq=torch.zeros(n), sched=torch.tensor([1e-2, 1e-2, float("inf"), 0, 0, 0], dtype=torch.float64))
        return {k: v.to(dev).contiguous() for k, v in t.items()}

    def ramp(seconds):
        a = torch.randn(4096, 4096, device=dev)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            for _ in range(8):
                a = torch.tanh(a @ a * 1e-4)
            torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def stats(secs, epochs):
        us = [1e6 * s / epochs for s in secs]
        return dict(us_per_epoch=dict(min=round(min(us), 2), median=round(float(np.median(us)), 2), max=round(max(us), 2)),
                    seconds=[round(s, 6) for s in secs])

    res = dict(N=10, T=30, key_points=[3, 5, 7, 9], rows_per_training=Q, epochs=args.epochs, repeats=args.repeats,
               warm_epochs=args.warm, device=torch.cuda.get_device_name(0), shapes={})
    for name, dims in SHAPES.items():
        n = len(dims) - 1
        dims_c, acts_c = (C.c_int32 * (n + 1))(*dims), (C.c_int32 * n)(*([TANH] * (n - 1) + [0]))
        ws_bytes = lib.kr_mlp_ws_bytes(n, dims_c, Q)
        out = {}
        for n_nets in args.nets:
            bank_t = [training(100 + k, dims) for k in range(n_nets)]
            solo_t = [{k: v.clone() for k, v in t.items()} for t in bank_t]
            ws = [torch.empty(ws_bytes, dtype=torch.uint8, device=dev) for _ in range(n_nets)]
            dout = [torch.zeros(Q, 32, device=dev) for _ in range(n_nets)]
            nets = (kn.KrTrainBankNet * n_nets)()
            for k, t in enumerate(bank_t):
                nets[k].S, nets[k].ds = S, ds
                for f in ("params", "grads", "exp_avg", "exp_avg_sq", "sched", "x", "base", "target_rows"):
                    setattr(nets[k], f, t[f].data_ptr())
            bank = C.c_void_p()
            h0 = handles[0]
            kn.check(lib.kr_train_bank_create(h0._h, n_nets, nets, K, n, dims_c, acts_c, 32, DENOM, C.byref(bank)))
            step = {"bank": 1, "solo": 1}

            def run_bank(epochs):
                kn.check(lib.kr_train_bank_epochs(h0._h, bank, epochs, step["bank"], *ADAM, *PLATEAU, 0, 0, kn._stream()))
                step["bank"] += epochs

            def run_solo(epochs):
                s = kn._stream()
                for k, t in enumerate(solo_t):
                    h = handles[k]
                    kn.check(lib.kr_train_epochs(
                        h._h, epochs, S, K, n, dims_c, acts_c, kn._ptr(t["params"]), kn._ptr(t["grads"]), kn._ptr(t["exp_avg"]),
                        kn._ptr(t["exp_avg_sq"]), None, kn._ptr(t["sched"]), kn._ptr(t["x"]), 32, kn._ptr(t["base"]),
                        kn._ptr(t["target_rows"]), DENOM, kn._ptr(dout[k]), kn._ptr(ws[k]), *ADAM, step["solo"], *PLATEAU, None,
                        1 if step["solo"] == 1 else 0, s))
                step["solo"] += epochs

            ramp(0.8)
            run_bank(args.warm)
            run_solo(args.warm)
            torch.cuda.synchronize()
            same = all(torch.equal(a["params"], b["params"]) for a, b in zip(bank_t, solo_t))
            tb, ts = [], []
            for _ in range(args.repeats):
                tb.append(timed(lambda: run_bank(args.epochs)))
                ts.append(timed(lambda: run_solo(args.epochs)))
            lib.kr_train_bank_destroy(bank)
            b, s_ = stats(tb, args.epochs), stats(ts, args.epochs)
            spread = s_["us_per_epoch"]["max"] - s_["us_per_epoch"]["min"]
            out[str(n_nets)] = dict(bank=b, solo=s_, solo_spread_us=round(spread, 2),
                                    solo_over_bank_median=round(s_["us_per_epoch"]["median"] / b["us_per_epoch"]["median"], 3),
                                    bit_identical_after_warm_epochs=bool(same))
            del bank_t, solo_t, ws, dout
            torch.cuda.empty_cache()
        cond = {}
        if "1" in out:
            o = out["1"]
            cond["n1_bank_not_slower_than_solo_by_more_than_its_spread"] = bool(
                o["bank"]["us_per_epoch"]["median"] <= o["solo"]["us_per_epoch"]["median"] + o["solo_spread_us"])
        if "32" in out:
            o = out["32"]
            cond["n32_bank_faster_than_solo_by_more_than_its_spread"] = bool(
                o["bank"]["us_per_epoch"]["median"] < o["solo"]["us_per_epoch"]["median"] - o["solo_spread_us"])
        res["shapes"][name] = dict(n_nets=out, conditions=cond)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
