"""GPU tests of the four-term training loss and its gradient (csrc/kr_loss_device.hpp in loss_kernel<false / true>, in the
epilogues of mlp_fwd3_kernel, mlp_fwd2_kernel and mlp_fwd_fused_kernel, and in the bank forms), ``-m gpu``, through the
C ABI: every path against the fp64 oracle of tests/loss_cases.py, per row and per block, on every family, inside the
bounds that module derives from the reference's own fp32 error (tests/golden/loss_terms.npz).

The MLP is taken out of the comparison: its last layer has zero weights and a bias beta, so every row's output is exactly
beta and the prediction is base + [ds beta[:19], beta[19:]].  One-row calls (S = K = 1) give the loss of a single row:
they are what holds the angles.  The worst observed fraction of each bound per path is printed (LABBOOK)."""
import ctypes as C

import numpy as np
import pytest

import loss_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIRECT = ("fwd_bwd", "rows_pred", "rows_null")
PATHS = DIRECT + tuple(lc.MLP_SHAPES)
WORST = {}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import krod_native as kn
    hs = {}
    for N in (10, 7):
        p = kn.KrParams()
        kn.check(kn.load().kr_default_params(C.byref(p)))
        p.N = N
        hs[N] = kn.Handle(p)
    return torch, kn, hs


def note(path, res):
    w = WORST.setdefault(path, {})
    for k, v in res.items():
        w[k] = max(w.get(k, 0.0), v[0])


class Net:
    """a network of one of MLP_SHAPES with a zero last weight matrix and the bias beta; workspace for up to 68 rows"""

    def __init__(self, env, shape, beta):
        torch, kn, hs = env
        self.dims, self.acts = lc.MLP_SHAPES[shape]
        n = self.n = len(self.acts)
        rng = np.random.default_rng(3)
        Ws = [0.3 * rng.standard_normal((self.dims[k + 1], self.dims[k])) / np.sqrt(self.dims[k]) for k in range(n)]
        bs = [0.1 * rng.standard_normal(self.dims[k + 1]) for k in range(n)]
        Ws[-1], bs[-1] = np.zeros_like(Ws[-1]), beta
        self.Ws, self.bs = [w.astype(np.float32) for w in Ws], [np.asarray(b, np.float32) for b in bs]
        self.W = [torch.tensor(w, device=DEV).contiguous() for w in self.Ws]
        self.b = [torch.tensor(b, device=DEV).contiguous() for b in self.bs]
        self.dims_c, self.acts_c = (C.c_int32 * (n + 1))(*self.dims), (C.c_int32 * n)(*self.acts)
        self.Wp = (C.c_void_p * n)(*[w.data_ptr() for w in self.W])
        self.bp = (C.c_void_p * n)(*[b.data_ptr() for b in self.b])
        self.ws = torch.empty(max(hs[10].lib.kr_mlp_ws_bytes(n, self.dims_c, 68), 16), dtype=torch.uint8, device=DEV)
        x = np.zeros((68, 32), np.float32)
        x[:, :28] = rng.standard_normal((68, 28))
        self.x = torch.tensor(x, device=DEV)
        self.out = torch.zeros((68, 32), dtype=torch.float32, device=DEV)

    def flat_params(self, torch):
        return torch.cat([torch.cat([w.reshape(-1), b]) for w, b in zip(self.W, self.b)]).contiguous()


class Runner:
    """one family on the device, once: base, target rows, and the rows scattered into [M][25][N] states for K = 1"""

    def __init__(self, env, name):
        self.env, self.name = env, name
        torch = env[0]
        c = lc.family(name)
        self.base_h, self.rows_h = c["base"], c["target"]
        self.base, self.rows = torch.tensor(c["base"], device=DEV), torch.tensor(c["target"], device=DEV)
        self.one = {N: torch.tensor(lc.scatter_targets(c["target"], 1, N, lc.IDX[(N, 1)]), device=DEV) for N in (10, 7)}
        self.idx1 = {N: torch.tensor(lc.IDX[(N, 1)], dtype=torch.int32, device=DEV) for N in (10, 7)}
        # a one-row call reads its row from these (allocation-aligned, as a caller's buffers are)
        self.base1, self.rows1 = torch.empty_like(self.base[:1]), torch.empty_like(self.rows[:1])
        self.states1 = {N: torch.empty_like(self.one[N][:1]) for N in (10, 7)}
        self.nets, self.outs = {}, {}
        self.dout = torch.empty((68, 32), dtype=torch.float32, device=DEV)
        self.pred = torch.empty((68, 25), dtype=torch.float32, device=DEV)
        self.loss = torch.empty(1, dtype=torch.float32, device=DEV)

    def net(self, shape, beta):
        if (shape, beta) not in self.nets:
            self.nets[shape, beta] = Net(self.env, shape, lc.BETAS[beta])
        return self.nets[shape, beta]

    def out_rows(self, beta):
        if beta not in self.outs:
            torch = self.env[0]
            o = np.zeros((68, 32), np.float32)
            o[:, :25] = lc.BETAS[beta]
            self.outs[beta] = torch.tensor(o, device=DEV)
        return self.outs[beta]

    def call(self, path, N, base, rows, S, K, denom, beta, states=None, idx=None, accumulate=0, start=None):
        """base, rows: device pointers of [S K][25]; states / idx: the [S][25][N] form for kr_loss_fwd_bwd.
        -> loss, dout [Q, 32], pred [Q, 25] or None (NumPy)"""
        torch, kn, hs = self.env
        h, Q = hs[N], S * K
        self.dout.fill_(7.0)
        self.pred.fill_(7.0)
        self.loss.fill_(0.25 if start is None else start)
        st, P = kn._stream(), kn._ptr
        with_pred = path in ("fwd_bwd", "rows_pred")
        if accumulate:
            h.set_option("mlp_grad_accumulate", 1)
        if path == "generic":
            h.set_option("fused_mlp", 0)
        try:
            if path == "fwd_bwd":
                kn.check(h.lib.kr_loss_fwd_bwd(h._h, S, K, base, P(self.out_rows(beta)), states, idx, denom, P(self.pred),
                                               P(self.loss), P(self.dout), st))
            elif path in ("rows_pred", "rows_null"):
                kn.check(h.lib.kr_loss_rows_fwd_bwd(h._h, S, K, base, P(self.out_rows(beta)), rows, denom,
                                                    P(self.pred) if with_pred else None, P(self.loss), P(self.dout), st))
            else:
                net = self.net(path, beta)
                kn.check(h.lib.kr_mlp_forward_loss(h._h, S, K, net.n, net.dims_c, net.acts_c, net.Wp, net.bp, P(net.x), 32, base,
                                                   rows, denom, P(net.out), P(self.loss), P(self.dout), P(net.ws), st))
            torch.cuda.synchronize()
        finally:
            if accumulate:
                h.set_option("mlp_grad_accumulate", 0)
            if path == "generic":
                h.set_option("fused_mlp", 1)
        return float(self.loss), self.dout[:Q].cpu().numpy(), self.pred[:Q].cpu().numpy() if with_pred else None

    def one_row(self, path, N, i, denom, beta):
        kn = self.env[1]
        self.base1.copy_(self.base[i:i + 1])
        self.rows1.copy_(self.rows[i:i + 1])
        self.states1[N].copy_(self.one[N][i:i + 1])
        return self.call(path, N, kn._ptr(self.base1), kn._ptr(self.rows1), 1, 1, denom, beta, kn._ptr(self.states1[N]),
                         kn._ptr(self.idx1[N]))


@pytest.fixture(scope="module")
def runners(env):
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = Runner(env, name)
        return memo[name]
    return get


def ds_of(env, N):
    return float(np.float32(env[2][N].derived().ds))


def check_pred(pred, base, beta, ds, what):
    """every entry bit for bit one of the two roundings of base + ds out between which the compiler's contraction decides:
    the fused multiply-add (the oracle's) or the rounded product added"""
    if pred is not None:
        out = np.tile(lc.BETAS[beta], (len(base), 1))
        fused, plain = lc.predict(base, out, ds), lc.predict_uncontracted(base, out, ds)
        bad = (pred != fused) & (pred != plain)
        assert not bad.any(), (what, np.argwhere(bad)[:4].tolist(), pred[bad][:4], fused[bad][:4], plain[bad][:4])


@pytest.mark.parametrize("name", list(lc.FAMILIES))
@pytest.mark.parametrize("path", PATHS)
def test_one_row_calls(env, runners, path, name):
    """S = K = 1 on at most 64 rows of the family (the octant-boundary rows always), MLP output zero and mixed: the row's
    loss - with the plain columns equal that is w_e sum (e_p - e_t)^2, the angles themselves - and every block of its dout
    row inside the row's bounds; identity against identity gives exactly 0; q and -q give the same loss and opposite
    h gradients bit for bit"""
    torch, kn, hs = env
    r = runners(name)
    sel = lc.one_row_sample(name)
    N, denom = (7, 1.0) if path == "rows_null" else (10, 29.0)
    ds = ds_of(env, N)
    zero_rows = set(lc.family(name)["exact_zero"].tolist())
    for beta in lc.BETAS:
        o = lc.oracle(r.base_h[sel], np.tile(lc.BETAS[beta], (len(sel), 1)), r.rows_h[sel], ds, 1, denom)
        b = lc.bounds(o)
        losses, douts = np.zeros(len(sel)), np.zeros((len(sel), 32))
        for j, i in enumerate(sel):
            losses[j], d, pred = r.one_row(path, N, int(i), denom, beta)
            douts[j] = d[0]
            check_pred(pred, r.base_h[i:i + 1], beta, ds, (path, name, beta, int(i)))
            if beta == "zero" and int(i) in zero_rows:
                assert losses[j] == 0.0 and np.all(d[0] == 0.0), (path, name, int(i), losses[j])
        res = lc.held(o, b, douts, losses)
        note(path, res)
        assert not lc.missed(res), (path, name, beta, lc.missed(res))
    if name == "negated":
        got = [r.one_row(path, N, i, denom, "zero")[:2] for i in range(32)]
        for a, m in zip(got[0::2], got[1::2]):
            assert a[0] == m[0] and np.array_equal(a[1][0, 3:7], -m[1][0, 3:7]) and np.abs(a[1][0, 3:7]).max() > 0


@pytest.mark.parametrize("name", list(lc.FAMILIES))
@pytest.mark.parametrize("path", PATHS)
def test_batched_calls(env, runners, path, name):
    """Q = S K rows of the family for every (Q, K) of ROW_COUNTS, denom 29 and 1, MLP output zero and mixed: every block of
    every dout row inside its bound, columns 25 .. 31 zero, the loss the fp64 sum of the oracle's row losses within the
    summed row bounds; kr_loss_fwd_bwd at N = 10 and 7 with idx containing 1 and N - 1, its pred bit for bit (1 ulp),
    kr_gather_targets exact; the accumulate option adds to a slot that held 0.5 and its absence overwrites it"""
    torch, kn, hs = env
    r = runners(name)
    for (Q, K) in lc.ROW_COUNTS:
        sel = lc.pick(name, Q)
        assert len(sel) == Q
        S = Q // K
        base, rows = torch.tensor(r.base_h[sel], device=DEV), torch.tensor(r.rows_h[sel], device=DEV)
        for N in ((10, 7) if path == "fwd_bwd" else (10,)):
            ds = ds_of(env, N)
            idx = torch.tensor(lc.IDX[(N, K)], dtype=torch.int32, device=DEV)
            states = torch.tensor(lc.scatter_targets(r.rows_h[sel], K, N, lc.IDX[(N, K)]), device=DEV)
            if path == "fwd_bwd":
                gathered = torch.full((Q, 25), 7.0, dtype=torch.float32, device=DEV)
                kn.check(hs[N].lib.kr_gather_targets(hs[N]._h, S, K, kn._ptr(states), kn._ptr(idx), kn._ptr(gathered), kn._stream()))
                assert torch.equal(gathered, rows), (name, Q, K, N)
            for denom in lc.DENOMS:
                for beta in lc.BETAS:
                    o = lc.oracle(r.base_h[sel], np.tile(lc.BETAS[beta], (Q, 1)), r.rows_h[sel], ds, K, denom)
                    b = lc.bounds(o)
                    what = (path, name, Q, K, N, denom, beta)
                    loss, dout, pred = r.call(path, N, kn._ptr(base), kn._ptr(rows), S, K, denom, beta, kn._ptr(states), kn._ptr(idx))
                    check_pred(pred, r.base_h[sel], beta, ds, what)
                    res = lc.held(o, b, dout, loss=loss)
                    note(path, res)
                    assert not lc.missed(res), (what, lc.missed(res))
                    if path != "fwd_bwd" and denom == 29.0:
                        acc, dacc, _ = r.call(path, N, kn._ptr(base), kn._ptr(rows), S, K, denom, beta, accumulate=1, start=0.5)
                        res = lc.held(o, b, dacc, loss=acc, extra=0.5)
                        note(path, {"loss_accumulated": res["loss"]})
                        assert not lc.missed(res), (what, "accumulate", lc.missed(res))
                        over, _, _ = r.call(path, N, kn._ptr(base), kn._ptr(rows), S, K, denom, beta, accumulate=0, start=0.5)
                        assert over == loss, (what, over, loss)


# ---- kr_train_epoch (phase 1) and a bank of two trainings ------------------------------------------------------------------------
def training(env, net, name, S, K, beta):
    """buffers of one training in the layout of test_gpu_train_bank.make_training, on the first S K rows of a family"""
    torch = env[0]
    c = lc.family(name)
    Q = S * K
    p = net.flat_params(torch)
    n = p.numel()
    z = lambda m: torch.zeros(m, dtype=torch.float32, device=DEV)
    rng = np.random.default_rng(9)
    x = np.zeros((Q, 32), np.float32)
    x[:, :28] = rng.standard_normal((Q, 28))
    return dict(S=S, x=torch.tensor(x, device=DEV), base=torch.tensor(c["base"][:Q], device=DEV),
                target_rows=torch.tensor(c["target"][:Q], device=DEV), params=p, grads=z(n + 1), exp_avg=z(n), exp_avg_sq=z(n),
                lower=None, sched=torch.tensor([1e-2, 1e-2, float("inf"), 0.0, 0.0, 0.0], dtype=torch.float64, device=DEV),
                loss_log=z(16), base_h=c["base"][:Q], rows_h=c["target"][:Q], beta=beta)


@pytest.mark.parametrize("shape", ["fwd3", "fwd2"])
@pytest.mark.parametrize("beta", list(lc.BETAS))
def test_train_epoch_phase_1(env, shape, beta):
    """kr_train_epoch, phase 1, on 33 near-identity rows (K = 3): the loss slot within the summed row bounds and the last
    layer's bias gradient = sum over the rows of dout, entry by entry within the rows' summed bounds"""
    torch, kn, hs = env
    import test_gpu_train_bank as tb
    h, K, denom = hs[10], 3, 29.0
    net = Net(env, shape, lc.BETAS[beta])
    t = training(env, net, "near_identity", 11, K, beta)
    Q = 33
    dout = torch.full((Q, 32), 7.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(max(h.lib.kr_mlp_ws_bytes(net.n, net.dims_c, Q), 16), dtype=torch.uint8, device=DEV)
    A = tb.ADAM
    kn.check(h.lib.kr_train_epoch(
        h._h, 11, K, net.n, net.dims_c, net.acts_c, kn._ptr(t["params"]), kn._ptr(t["grads"]), kn._ptr(t["exp_avg"]),
        kn._ptr(t["exp_avg_sq"]), None, kn._ptr(t["sched"]), kn._ptr(t["x"]), 32, kn._ptr(t["base"]), kn._ptr(t["target_rows"]),
        denom, kn._ptr(dout), kn._ptr(ws), A["beta1"], A["beta2"], A["eps"], A["weight_decay"], 1, 0.5, 80, A["threshold"],
        A["min_lr"], kn._ptr(t["loss_log"]), 1, 1, kn._stream()))
    torch.cuda.synchronize()
    o = lc.oracle(t["base_h"], np.tile(lc.BETAS[beta], (Q, 1)), t["rows_h"], ds_of(env, 10), K, denom)
    b = lc.bounds(o)
    g = t["grads"].cpu().numpy().astype(np.float64)
    n = g.size - 1
    res = lc.held(o, b, dout.cpu().numpy(), loss=g[n])
    entry = b["plain"].copy()
    entry[:, 3:7] = b["h"][:, None]
    want = o["dout"][:, :25].sum(axis=0)
    bound = entry.sum(axis=0) + 0.5 * (Q - 1) * lc.EPS32 * np.abs(o["dout"][:, :25]).sum(axis=0)
    rb = lc.ratio(np.abs(g[n - 25:n] - want), bound)
    res["bias_gradient"] = (float(rb.max()), int((rb > 1).sum()))
    note("epoch_" + shape, res)
    assert np.abs(want).max() > 0 and not lc.missed(res), (shape, beta, lc.missed(res))


@pytest.mark.parametrize("shape", ["fwd3", "fwd2"])
def test_bank_of_two_trainings(env, shape):
    """kr_train_bank_epochs, one epoch of two trainings over different families (near-identity, 8 x 4 rows, MLP output
    zero; generic, 17 x 4 rows, mixed): loss_log[0] of each within its summed row bounds"""
    torch, kn, hs = env
    import test_gpu_train_bank as tb
    benv = (torch, kn, hs[10])
    dims, acts = lc.MLP_SHAPES[shape]
    ts = [training(env, Net(env, shape, lc.BETAS["zero"]), "near_identity", 8, tb.K, "zero"),
          training(env, Net(env, shape, lc.BETAS["mixed"]), "generic", 17, tb.K, "mixed")]
    rc, bank = tb.bank_create(benv, ts, dims, acts)
    assert rc == 0, kn.load().kr_last_error()
    try:
        assert tb.bank_epochs(benv, bank, 1) == 0, kn.load().kr_last_error()
    finally:
        hs[10].lib.kr_train_bank_destroy(bank)
    for k, t in enumerate(ts):
        Q = t["S"] * tb.K
        o = lc.oracle(t["base_h"], np.tile(lc.BETAS[t["beta"]], (Q, 1)), t["rows_h"], ds_of(env, 10), tb.K, tb.DENOM)
        r = float(lc.ratio(abs(float(t["loss_log"][0]) - o["loss"]), lc.sum_bound(o, lc.bounds(o))))
        note("bank_" + shape, {"loss": (r, int(r > 1))})
        assert o["loss"] > 0 and r <= 1, (shape, k, float(t["loss_log"][0]), o["loss"], r)


def test_report_worst_fractions():
    """(last in the file) what the device used of each bound, per path"""
    for path, w in WORST.items():
        print(f"worst fraction of the bound, {path}: " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))
    assert all(v <= 1.0 for w in WORST.values() for v in w.values())
