"""GPU tests of the training kernels (csrc/kr_mlp_fused.hip, kr_mlp_fused_bodies.inc) past one row block per wavefront
(``-m gpu``), against the fp64 NumPy reference of tests/train_kernel_cases.py.

C1  integer networks: forward, backward and both slab reductions BIT FOR BIT (every sum is exact in fp32 in any order);
C2  real-valued networks: a row of kr_mlp_forward / kr_mlp_forward_loss does not depend on the batch it travels in;
C3  real-valued gradients of the two-layer kernels at Q_B against fp64;
C4  kr_train_epoch at Q_B: phase 1 against the separate calls, phases 1 + 2 against phase 0, and a bank with one
    training of that size;
C5  the split three-layer backward pass (KR_BWD3_MERGED=0), in a child process of its own: the library reads the
    variable once per process.

Run as a script (``python test_gpu_train_kernels_exact.py split-backward``) this file is that child."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_l2
import train_kernel_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DENOM = 29.0
ADAM = (0.9, 0.999, 1e-8, 0.0)          # beta1, beta2, eps, weight decay
PLATEAU = dict(factor=0.5, patience=80, threshold=1e-4, min_lr=0.0)


def make_env():
    import torch
    assert torch.cuda.is_available()
    import krod_native as kn
    p = kn.KrParams()
    kn.check(kn.load().kr_default_params(C.byref(p)))
    p.N = 10
    return torch, kn, kn.Handle(p)


@pytest.fixture(scope="module")
def env():
    return make_env()


class DevNet:
    """One network on the device with a workspace for up to Qmax rows, and the three calls on it"""

    def __init__(self, env, dims, acts, Ws, bs, Qmax):
        torch, kn, h = env
        self.env, self.dims, self.n = env, list(dims), len(acts)
        n = self.n
        self.dims_c, self.acts_c = (C.c_int32 * (n + 1))(*dims), (C.c_int32 * n)(*acts)
        self.W = [torch.tensor(np.asarray(w, np.float32), device=DEV).contiguous() for w in Ws]
        self.b = [torch.tensor(np.asarray(b, np.float32), device=DEV).contiguous() for b in bs]
        self.Wp = (C.c_void_p * n)(*[w.data_ptr() for w in self.W])
        self.bp = (C.c_void_p * n)(*[b.data_ptr() for b in self.b])
        self.ws = torch.empty(max(h.lib.kr_mlp_ws_bytes(n, self.dims_c, Qmax), 16), dtype=torch.uint8, device=DEV)

    def forward(self, x):
        torch, kn, h = self.env
        Q = x.shape[0]
        out = torch.full((Q, 32), 7.0, dtype=torch.float32, device=DEV)  # (poisoned: columns nout.. must come back zero)
        kn.check(h.lib.kr_mlp_forward(h._h, Q, self.n, self.dims_c, self.acts_c, self.Wp, self.bp, kn._ptr(x), 32,
                                      kn._ptr(out), kn._ptr(self.ws), kn._stream()))
        return out

    def forward_loss(self, K, x, base, target):
        torch, kn, h = self.env
        Q = x.shape[0]
        assert Q % K == 0
        out = torch.zeros((Q, 32), dtype=torch.float32, device=DEV)
        dout = torch.full((Q, 32), 7.0, dtype=torch.float32, device=DEV)
        loss = torch.zeros(1, dtype=torch.float32, device=DEV)
        kn.check(h.lib.kr_mlp_forward_loss(h._h, Q // K, K, self.n, self.dims_c, self.acts_c, self.Wp, self.bp, kn._ptr(x), 32,
                                           kn._ptr(base), kn._ptr(target), DENOM, kn._ptr(out), kn._ptr(loss), kn._ptr(dout),
                                           kn._ptr(self.ws), kn._stream()))
        return float(loss), dout

    def backward(self, x, dout, ordered, prefill=None):
        """-> dW, db.  prefill (lists of tensors): option mlp_grad_accumulate on, the gradient is added to copies of them"""
        torch, kn, h = self.env
        if prefill is None:
            dW = [torch.full_like(w, 7.0) for w in self.W]  # (poisoned: the call overwrites)
            db = [torch.full_like(b, 7.0) for b in self.b]
        else:
            dW, db = [t.clone() for t in prefill[0]], [t.clone() for t in prefill[1]]
        dWp = (C.c_void_p * self.n)(*[t.data_ptr() for t in dW])
        dbp = (C.c_void_p * self.n)(*[t.data_ptr() for t in db])
        h.set_option("mlp_grad_ordered", ordered)
        h.set_option("mlp_grad_accumulate", 0 if prefill is None else 1)
        try:
            kn.check(h.lib.kr_mlp_backward(h._h, x.shape[0], self.n, self.dims_c, self.acts_c, self.Wp, kn._ptr(x), 32,
                                           kn._ptr(dout), kn._ptr(self.ws), dWp, dbp, kn._stream()))
            torch.cuda.synchronize()
        finally:
            h.set_option("mlp_grad_ordered", 0)
            h.set_option("mlp_grad_accumulate", 0)
        return dW, db


def same(torch, got, want, what):
    """bit for bit, with a report that says where"""
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = tuple(bad[0].tolist())
    raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} entries differ, first at {first}: got {got[first].item()!r}, "
                         f"want {want[first].item()!r}; rows {sorted(set(bad[:, 0].tolist()))[:8]} ...")


# ---- C1 -------------------------------------------------------------------------------------------------------------------
def check_int_case(env, name, Q):
    """kr_mlp_forward + kr_mlp_backward on an integer case: outputs, every dW and db equal the reference bit for bit,
    with the slab sum by atomics and in fixed order, overwriting and accumulating"""
    torch = env[0]
    c = tc.int_case(name, Q)
    ref_out, ref_dW, ref_db = tc.int_reference(name, Q)
    dev = lambda a: torch.tensor(np.asarray(a, np.float32), device=DEV)
    net = DevNet(env, c["dims"], c["acts"], c["Ws"], c["bs"], Q)
    x, dout = dev(c["x"]), dev(c["dout"])
    nout = c["dims"][-1]
    out = net.forward(x)
    torch.cuda.synchronize()
    same(torch, out[:, :nout], dev(ref_out), f"{name} Q={Q} out")
    assert not bool(out[:, nout:].any()), "columns past the last layer's width must be zero"
    want_W, want_b = [dev(g) for g in ref_dW], [dev(g) for g in ref_db]
    rng = np.random.default_rng(7)
    pre = ([dev(rng.integers(-3, 4, size=w.shape)) for w in c["Ws"]], [dev(rng.integers(-3, 4, size=b.shape)) for b in c["bs"]])
    for ordered in (0, 1):
        dW, db = net.backward(x, dout, ordered)
        for k in range(net.n):
            same(torch, dW[k], want_W[k], f"{name} Q={Q} ordered={ordered} dW[{k}]")
            same(torch, db[k], want_b[k], f"{name} Q={Q} ordered={ordered} db[{k}]")
        dW, db = net.backward(x, dout, ordered, prefill=pre)
        for k in range(net.n):
            same(torch, dW[k], pre[0][k] + want_W[k], f"{name} Q={Q} ordered={ordered} accumulated dW[{k}]")
            same(torch, db[k], pre[1][k] + want_b[k], f"{name} Q={Q} ordered={ordered} accumulated db[{k}]")


INT_CASES = [(name, Q) for name in tc.INT_NETS for Q in tc.SMALL_Q + (tc.Q_A,)] + [(name, tc.Q_B) for name in tc.QB_NETS]


@pytest.mark.parametrize("name,Q", INT_CASES, ids=[f"{n}-{q}" for n, q in INT_CASES])
def test_integer_networks_bit_for_bit(env, name, Q):
    """Q_A = 65 573: a few wavefronts of mlp_fwd2 / mlp_fwd3 / mlp_bwd3_kernel take a second row block, ragged tail;
    Q_B = 131 297: every wavefront takes two, some three; 4104 row blocks for the 4096 workgroups of mlp_fwd_fused_kernel
    (networks 600, 32x64x64x32, 64to26); mlp_bwd2_kernel at its slab cap; both slab reductions over every slab."""
    check_int_case(env, name, Q)


# ---- C2 -------------------------------------------------------------------------------------------------------------------
K_LOSS = 3
Q_LOSS = tc.rows_for(tc.Q_B, K_LOSS)               # S x 3 rows: Q_B + 1, the same 4104 row blocks
SLICE_LOSS = tc.ONE_TRIP_SLICE // K_LOSS * K_LOSS  # a multiple of 3 rows


@pytest.fixture(scope="module")
def real(env):
    """name -> the network on the device, the rows, and kr_mlp_forward_loss in one-trip slices (dout rows, fp64 sum of
    the slices' losses): computed once, shared by C2 and C4, left unchanged"""
    torch = env[0]
    memo = {}

    def get(name):
        if name not in memo:
            dims, acts, Ws, bs = tc.real_net(name)
            xs, douts, bases, targets = tc.real_rows(Q_LOSS)
            dev = lambda a: torch.tensor(a, device=DEV).contiguous()
            r = dict(net=DevNet(env, dims, acts, Ws, bs, Q_LOSS), x=dev(xs), dout=dev(douts), base=dev(bases), target=dev(targets),
                     dims=dims, acts=acts, Ws=Ws, bs=bs)
            parts, total = [], 0.0
            for r0 in range(0, Q_LOSS, SLICE_LOSS):
                r1 = min(r0 + SLICE_LOSS, Q_LOSS)
                loss, d = r["net"].forward_loss(K_LOSS, r["x"][r0:r1], r["base"][r0:r1], r["target"][r0:r1])
                parts.append(d)
                total += loss
            r["dout_sliced"], r["loss_sliced"] = torch.cat(parts), total
            memo[name] = r
        return memo[name]
    return get


@pytest.mark.parametrize("name", list(tc.REAL_NETS))
def test_a_row_does_not_depend_on_its_batch(env, real, name):
    """kr_mlp_forward on Q_B rows against the same rows in slices of 32 768 (one trip of every row-block loop), and the
    same for kr_mlp_forward_loss with K = 3: rows bit for bit; the loss against the fp64 sum of the slices' losses within
    2e-5 relative (the bound of test_loss_kernel_vs_torch_autograd for this quantity)."""
    torch = env[0]
    r = real(name)
    net, x = r["net"], r["x"][:tc.Q_B]
    full = net.forward(x)
    for r0 in range(0, tc.Q_B, tc.ONE_TRIP_SLICE):
        r1 = min(r0 + tc.ONE_TRIP_SLICE, tc.Q_B)
        same(torch, full[r0:r1], net.forward(x[r0:r1]), f"{name} forward rows {r0}..{r1}")
    assert not bool(full[:, 25:].any()) and float(full[:, :25].abs().max()) > 0.1
    loss, dout = net.forward_loss(K_LOSS, r["x"], r["base"], r["target"])
    same(torch, dout, r["dout_sliced"], f"{name} forward_loss dout")
    assert not bool(dout[:, 25:].any()) and float(dout[:, :25].abs().max()) > 0.0
    rel = abs(loss - r["loss_sliced"]) / abs(r["loss_sliced"])
    print(f"C2 {name}: loss {loss!r} at {Q_LOSS} rows, fp64 sum of {-(-Q_LOSS // SLICE_LOSS)} slices {r['loss_sliced']!r}, rel {rel:.2e}")
    assert rel < 2e-5


# ---- C3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["100_tanh", "512_elu"])
def test_two_layer_gradients_at_q_b(env, real, name):
    """act' on real data through mlp_fwd2_kernel / mlp_bwd2_kernel at Q_B against the fp64 reference, with the bounds of
    test_mlp_forward_backward_vs_torch (forward rel_l2 < 3e-6, gradients < 2e-5; passing there at Q = 33 333).
    Observed on the MI355X at 131 297 rows: see LABBOOK, "training kernels past one row block per wavefront"."""
    torch = env[0]
    r = real(name)
    net, x, dout = r["net"], r["x"][:tc.Q_B], r["dout"][:tc.Q_B]
    ref_out, ref_dW, ref_db = tc.reference(r["dims"], r["acts"], r["Ws"], r["bs"], x.cpu().numpy(), dout.cpu().numpy())
    out = net.forward(x)
    figures = [("out", rel_l2(out[:, :25].cpu().numpy(), ref_out))]
    for ordered in (0, 1):
        dW, db = net.backward(x, dout, ordered)
        for k in range(net.n):
            figures.append((f"dW[{k}] ordered={ordered}", rel_l2(dW[k].cpu().numpy(), ref_dW[k])))
            figures.append((f"db[{k}] ordered={ordered}", rel_l2(db[k].cpu().numpy(), ref_db[k])))
    print(f"C3 {name} at Q = {tc.Q_B}: " + ", ".join(f"{w} {v:.2e}" for w, v in figures))
    for what, v in figures:
        assert v < (3e-6 if what == "out" else 2e-5), (what, v)


# ---- C4 -------------------------------------------------------------------------------------------------------------------
def epoch_state(torch, Ws, bs, lr=1e-2):
    p = torch.cat([torch.cat([torch.tensor(W).reshape(-1), torch.tensor(b)]) for W, b in zip(Ws, bs)]).to(DEV)
    n = p.numel()
    z = lambda m: torch.zeros(m, dtype=torch.float32, device=DEV)
    return dict(params=p, grads=z(n + 1), exp_avg=z(n), exp_avg_sq=z(n), loss_log=z(8),
                sched=torch.tensor([lr, lr, float("inf"), 0.0, 0.0, 0.0], dtype=torch.float64, device=DEV))


def epoch_call(env, net, st, r, dout, ws, step, phase, repack):
    torch, kn, h = env
    kn.check(h.lib.kr_train_epoch(
        h._h, Q_LOSS // K_LOSS, K_LOSS, net.n, net.dims_c, net.acts_c, kn._ptr(st["params"]), kn._ptr(st["grads"]),
        kn._ptr(st["exp_avg"]), kn._ptr(st["exp_avg_sq"]), None, kn._ptr(st["sched"]), kn._ptr(r["x"]), 32, kn._ptr(r["base"]),
        kn._ptr(r["target"]), DENOM, kn._ptr(dout), kn._ptr(ws), *ADAM, step, PLATEAU["factor"], PLATEAU["patience"],
        PLATEAU["threshold"], PLATEAU["min_lr"], st["loss_log"].data_ptr() + 4 * (step - 1), phase, repack, kn._stream()))


@pytest.mark.parametrize("name", ["64x64_elu", "512_elu"])
def test_epoch_at_q_b(env, real, name):
    """kr_train_epoch on 131 298 rows (K = 3).  Phase 1 leaves dout - bit for bit the rows of the sliced
    kr_mlp_forward_loss - and the summed gradients and loss, compared with kr_mlp_backward (ordered) on that dout and with
    the loss of the one call, in the bounds of test_train_epoch_equals_the_separate_calls (2e-6 of the largest entry,
    5e-6 relative on the loss: the two paths add the same slabs in another order).  Then two epochs as phase 0 against two
    epochs as phases 1 + 2: every piece of state bit for bit."""
    torch = env[0]
    r = real(name)
    net = r["net"]
    new_ws = lambda: torch.empty_like(net.ws)
    st, ws, dout = epoch_state(torch, r["Ws"], r["bs"]), new_ws(), torch.full((Q_LOSS, 32), 7.0, device=DEV)
    epoch_call(env, net, st, r, dout, ws, 1, 1, 1)
    torch.cuda.synchronize()
    same(torch, dout, r["dout_sliced"], f"{name} dout of phase 1")
    loss_one, dout_one = net.forward_loss(K_LOSS, r["x"], r["base"], r["target"])
    dW, db = net.backward(r["x"], dout_one, 1)
    want = torch.cat([torch.cat([w.reshape(-1), b]) for w, b in zip(dW, db)])
    got, n = st["grads"], want.numel()
    gerr = float((got[:n] - want).abs().max()) / max(1.0, float(want.abs().max()))
    lerr = abs(float(got[n]) - loss_one) / abs(loss_one)
    print(f"C4 {name}: gradients of phase 1 against kr_mlp_backward: max abs diff / max(1, max |g| = {float(want.abs().max()):.3g}) = "
          f"{gerr:.2e}; loss slot {float(got[n])!r} against {loss_one!r}: rel {lerr:.2e}")
    assert float(want.abs().max()) > 0.0 and gerr < 2e-6 and lerr < 5e-6
    del st, ws
    runs = []
    for phases in ((0,), (1, 2)):
        st, ws = epoch_state(torch, r["Ws"], r["bs"]), new_ws()
        for step in (1, 2):
            for ph in phases:
                epoch_call(env, net, st, r, dout, ws, step, ph, 1 if (step == 1 and ph != 2) else 0)
        torch.cuda.synchronize()
        runs.append(st)
        del ws
    for f in runs[0]:
        same(torch, runs[1][f], runs[0][f], f"{name} phases 1 + 2 against phase 0: {f}")
    a = runs[0]
    assert float(a["grads"].abs().max()) == 0.0 and bool(torch.isfinite(a["loss_log"][:2]).all()) and float(a["loss_log"][:2].min()) > 0
    assert not torch.equal(a["params"], epoch_state(torch, r["Ws"], r["bs"])["params"])


@pytest.mark.parametrize("dims,acts", [([28, 64, 64, 25], [tc.ELU, tc.ELU, tc.NONE]), ([28, 512, 25], [tc.ELU, tc.NONE])])
def test_bank_with_one_training_at_q_b(env, dims, acts):
    """mlp_fwd2/3_bank_kernel, mlp_bwd2/3_bank_kernel, train_tail_bank_kernel with a network whose wavefronts take three
    row blocks (S x K = 131 300, K = 4) next to one of 12 rows: each bit for bit the training run alone."""
    import test_gpu_train_bank as tb
    benv = env
    torch, kn, h = benv
    S = (tc.rows_for(tc.Q_B, tb.K) // tb.K, 3)
    solo = [tb.make_training(torch, 90 + i, s, dims, clamp=(i == 0)) for i, s in enumerate(S)]
    inb = [tb.clone_training(torch, t) for t in solo]
    rc, bank = tb.bank_create(benv, inb, dims, acts)
    assert rc == 0, kn.load().kr_last_error()
    try:
        assert tb.bank_epochs(benv, bank, 2) == 0, kn.load().kr_last_error()
    finally:
        h.lib.kr_train_bank_destroy(bank)
    for k, t in enumerate(solo):
        tb.run_solo(benv, t, dims, acts, 2)
        tb.assert_same(torch, inb[k], t, f"network {k} (S = {S[k]})")
        assert bool(torch.isfinite(t["loss_log"][:2]).all()) and float(t["loss_log"][:2].min()) > 0.0
        assert not torch.equal(t["params"], tb.make_training(torch, 90 + k, S[k], dims)["params"])


# ---- C5 -------------------------------------------------------------------------------------------------------------------
SPLIT_CASES = [(name, Q) for Q in (4099, tc.Q_A) for name in ("64x64", "33x20")]


def test_split_backward_pass():
    """mlp_bwd3a_kernel / mlp_bwd3b_kernel (KR_BWD3_MERGED=0): C1's three-layer cases at Q = 4099 and Q_A in a fresh child
    process with its own time limit."""
    env = dict(os.environ, KR_BWD3_MERGED="0")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "split-backward"], env=env, capture_output=True, text=True,
                         timeout=240)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("exact") == len(SPLIT_CASES) and "split backward ok" in out.stdout, out.stdout


if __name__ == "__main__":
    assert sys.argv[1:] == ["split-backward"] and os.environ.get("KR_BWD3_MERGED") == "0"
    child_env = make_env()
    for case in SPLIT_CASES:
        check_int_case(child_env, *case)
        print("exact:", *case, flush=True)
    print("split backward ok")
