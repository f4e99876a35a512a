"""The test of the tests of the training loss (tests/loss_cases.py), on the CPU: the oracle against mpmath at 50 digits,
against fp64 autograd and against the reference's fixture; the families inside the conditioning limits; the fp32
emulation of csrc/kr_loss_device.hpp inside every bound on every row; every mutant outside one; and what the suite's
earlier assertion (one rel_l2 over 25 columns of one input family) saw of them."""
import mpmath
import numpy as np
import pytest
import torch

import loss_cases as lc

DS = lc.default_ds(10)
SETTINGS = ((1, 29.0), (3, 1.0), (4, 29.0))      # (K, denom)


def rows_of(name, beta, K):
    c = lc.family(name)
    Q = len(c["base"]) // K * K
    return c["base"][:Q], np.tile(lc.BETAS[beta], (Q, 1)), c["target"][:Q]


def through_gather(target, K, mut=None):
    idx = lc.IDX[(10, K)]
    return lc.gather_targets(lc.scatter_targets(target, K, 10, idx), idx, mut)


@pytest.mark.parametrize("name", list(lc.FAMILIES))
def test_oracle_angles_against_mpmath(name):
    """48 rows per family, prediction and target: the oracle's fp64 angles against 50 digits, within 8 eps64 / rho"""
    c = lc.family(name)
    sel = lc.one_row_sample(name, 48)
    for q in (c["base"][sel, 3:7], c["target"][sel, 3:7]):
        e, rho, _, _ = lc.euler_parts(q)
        with mpmath.workdps(50):
            for i, row in enumerate(q):
                w, x, y, z = (mpmath.mpf(float(v)) for v in row)
                n = mpmath.sqrt(w * w + x * x + y * y + z * z)
                w, x, y, z = w / n, x / n, y / n, z / n
                want = (mpmath.atan2(2 * (w * y + x * z), 1 - 2 * (y * y + z * z)), mpmath.asin(2 * (w * z - x * y)),
                        mpmath.atan2(2 * (w * x + y * z), 1 - 2 * (x * x + z * z)))
                for k in range(3):
                    assert abs(mpmath.mpf(float(e[i, k])) - want[k]) <= 8 * 2.0 ** -52 / rho[i, k] * max(1.0, abs(float(e[i, k]))), (name, i, k)


def torch_loss(pred, target, K, denom, dtype, q2e=None):
    """physics_train.py:252-259 restated around quaternion_to_euler for rows [S * K, 25] -> the summed loss / denom"""
    from Utils.transformations import quaternion_to_euler
    q2e = q2e or quaternion_to_euler
    mse = torch.nn.MSELoss()
    S = pred.shape[0] // K
    p3, t3 = pred.reshape(S, K, 25).transpose(1, 2), target.reshape(S, K, 25).transpose(1, 2)
    total = 0
    for s in range(S):
        total = total + (mse(p3[s][:3], t3[s][:3]) + mse(p3[s][7:19], t3[s][7:19]) + mse(q2e(p3[s][3:7]), q2e(t3[s][3:7]))
                         + mse(p3[s][19:], t3[s][19:]))
    return total / denom


def q2e_f64(q):
    q = q / q.norm(p=2, dim=0, keepdim=True)
    w, x, y, z = q.unbind(0)
    return torch.stack((torch.atan2(2 * (w * y + x * z), 1 - 2 * (y * y + z * z)), torch.asin((2 * (w * z - x * y)).clamp(-1.0, 1.0)),
                        torch.atan2(2 * (w * x + y * z), 1 - 2 * (x * x + z * z))), dim=0)


@pytest.mark.parametrize("name", list(lc.FAMILIES))
def test_oracle_against_fp64_autograd(name):
    """loss and d loss / d out of the oracle against torch autograd of the same expression in fp64 (nn.MSELoss means,
    the prediction through ds): the analytic gradient, its ds chain and the projection through the normalisation"""
    K, denom = 4, 29.0
    base, out, target = rows_of(name, "mixed", K)
    o = lc.oracle(base, out, target, DS, K, denom)
    pred = torch.tensor(o["p"], requires_grad=True)
    loss = torch_loss(pred, torch.tensor(o["t"]), K, denom, torch.float64, q2e_f64)
    loss.backward()
    want = pred.grad.numpy() * o["scale"]
    assert abs(loss.item() - o["loss"]) <= 1e-12 * o["loss"]
    err = np.abs(o["dout"][:, :25] - want).max(axis=1)
    assert np.all(err <= 1e-10 * (np.abs(want).max(axis=1) + 1e-30)), (name, float(err.max()))
    assert np.all(o["dout"][:, 25:] == 0)


def test_reference_constants_and_the_package_s_own_function():
    """C_ANG and C_VJP come from the fixture; Utils/transformations.py gives the fixture's angles bit for bit"""
    from Utils.transformations import quaternion_to_euler
    g = np.load(lc.FIXTURE)
    a, v, per = lc.reference_constants(g)
    print(f"reference needs {a:.3f} eps32 / rho for an angle, {v:.3f} eps32 kappa for the Jacobian-transpose product; per family {per}")
    assert abs(a - lc.REF_ANG_RECORDED) < 0.005 and abs(v - lc.REF_VJP_RECORDED) < 0.005
    assert lc.constants() == (lc.MARGIN * a, lc.MARGIN * v)
    for name in lc.FAMILIES:
        q = torch.tensor(g[name + "_qp"].T.copy(), requires_grad=True)
        e = quaternion_to_euler(q)
        (e * torch.tensor(g[name + "_ge"].T.copy())).sum().backward()
        assert np.array_equal(e.detach().numpy().T, g[name + "_ep"]), name
        assert np.array_equal(quaternion_to_euler(torch.tensor(g[name + "_qt"].T.copy())).numpy().T, g[name + "_et"]), name
        # the oracle's ge is what the fixture's gradient was taken for
        c = lc.family(name)
        o = lc.oracle(c["base"], np.zeros((len(c["base"]), 25), np.float32), c["target"], DS, 1, 1.0)
        # (the gradients are two fp32 backward passes - y * y here, y**2 there: each within the reference's constant of fp64)
        gap = np.abs(q.grad.numpy().T.astype(np.float64) - g[name + "_gq"]).max(axis=1)
        assert np.all(gap <= 2 * v * lc.EPS32 * o["kappa"]), name
        assert np.array_equal(o["ge"].astype(np.float32), g[name + "_ge"]), name


def test_families_are_inside_the_conditioning_limits():
    """no row is skipped at run time: every row of every family, with either MLP output, has min rho >= RHO_MIN and a
    quaternion norm in [0.5, 3]; the near-gimbal rows have rho in [1e-2, 1e-1]; the Euler rows' targets convert to 0"""
    for name in lc.FAMILIES:
        c = lc.family(name)
        for beta in lc.BETAS:
            for N in (10, 7):
                o = lc.oracle(c["base"], np.tile(lc.BETAS[beta], (len(c["base"]), 1)), c["target"], lc.default_ds(N), 1, 1.0)
                assert min(o["rho_p"].min(), o["rho_t"].min()) >= lc.RHO_MIN, (name, beta)
        nrm = np.linalg.norm(c["target"][:, 3:7].astype(np.float64), axis=1)
        assert 0.5 <= nrm.min() and nrm.max() <= 3.0 and len(lc.one_row_sample(name)) <= 64
        assert set(c["must"].tolist()) <= set(lc.one_row_sample(name).tolist())
    c = lc.family("near_gimbal")
    for q in (c["base"][:, 3:7], c["target"][:, 3:7]):
        rho = lc.euler_parts(q)[1][:, 1]
        assert 1e-2 <= rho.min() and rho.max() <= 1e-1
    v = np.abs(lc.family("near_identity")["base"][:, 4:7] / lc.family("near_identity")["base"][:, 3:4])
    assert v.min() < 1e-4 and v.max() < 0.5
    c = lc.family("euler_rows")
    e = lc.emulate(c["base"], np.zeros((len(c["base"]), 25)), c["target"], DS, 1, 29.0)
    assert np.all(e["et"] == 0)
    z = c["exact_zero"]
    assert len(z) == 16 and np.all(e["row_loss"][z] == 0) and np.all(e["dout"][z] == 0)
    # the pure-axis families touch every fix-up of atan2_short and both branches of asin_short
    n = lambda q: q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = n(lc.family("axis_y")["base"][:, 3:7].astype(np.float64)).T
    a, b = 2 * w * y, 1 - 2 * y * y
    assert (np.abs(a) > np.abs(b)).any() and (np.abs(a) < np.abs(b)).any() and (b < 0).any() and (a < 0).any() and ((a == 0) & (b < 0)).any()
    w, x, y, z = n(lc.family("axis_z")["base"][:, 3:7].astype(np.float64)).T
    s = np.abs(2 * w * z)
    assert ((s > 0.5) & (s < 0.50001)).any() and ((s < 0.5) & (s > 0.49999)).any()


@pytest.mark.parametrize("name", list(lc.FAMILIES))
def test_emulation_is_inside_every_bound(name):
    """the header's text in fp32 NumPy, every row of the family, MLP output zero and mixed, every (K, denom): angles, row
    losses and every block of dout - a test must not reach the GPU with bounds that the source text itself misses"""
    worst = {}
    for beta in lc.BETAS:
        for K, denom in SETTINGS:
            base, out, target = rows_of(name, beta, K)
            o = lc.oracle(base, out, target, DS, K, denom)
            b = lc.bounds(o)
            e = lc.emulate(base, out, through_gather(target, K), DS, K, denom)
            assert np.array_equal(e["pred"], o["pred"])
            res = lc.held(o, b, e["dout"], e["row_loss"], float(e["row_loss"].astype(np.float64).sum()))
            res["angle"] = (max(float(lc.ratio(np.abs(e["ep"] - o["ep"]), b["ang_p"]).max()),
                                float(lc.ratio(np.abs(e["et"] - o["et"]), b["ang_t"]).max())), 0)
            for k, v in res.items():
                worst[k] = max(worst.get(k, 0.0), v[0])
    print(name, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def test_q_and_minus_q_agree():
    """rows 2 i, 2 i + 1 of the family: the same angles, the opposite gradient - exactly, in the oracle and in the text"""
    c = lc.family("negated")
    out = np.zeros((len(c["base"]), 25), np.float32)
    o = lc.oracle(c["base"], out, c["target"], DS, 1, 29.0)
    e = lc.emulate(c["base"], out, c["target"], DS, 1, 29.0)
    for r in (o, e):
        assert np.array_equal(r["ep"][0::2], r["ep"][1::2]) and np.array_equal(r["et"][0::2], r["et"][1::2])
        assert np.array_equal(r["dout"][0::2, 3:7], -r["dout"][1::2, 3:7]) and np.abs(r["dout"][:, 3:7]).max() > 0
    assert np.array_equal(e["row_loss"][0::2], e["row_loss"][1::2])


def mutant_counts(mut):
    """(bounds missed over family x MLP output x held quantity at K = 4, denom = 29; does the old assertion pass?)"""
    K, denom, n = 4, 29.0, 0
    for name in lc.FAMILIES:
        for beta in lc.BETAS:
            base, out, target = rows_of(name, beta, K)
            o = lc.oracle(base, out, target, DS, K, denom)
            e = lc.emulate(base, out, through_gather(target, K, mut), DS, K, denom, mut)
            n += len(lc.missed(lc.held(o, lc.bounds(o), e["dout"], e["row_loss"])))
    base, out, target, Ko, dn = lc.old_family()
    idx = [3, 5, 7, 9]
    e = lc.emulate(base, out, lc.gather_targets(lc.scatter_targets(target, Ko, 10, idx), idx, mut), DS, Ko, dn, mut)
    return n, lc.old_assertion_passes(e["dout"], lc.oracle(base, out, target, DS, Ko, dn))


def test_the_unmutated_text_passes_the_old_assertion_too():
    assert mutant_counts(None) == (0, True)


@pytest.mark.parametrize("mut", lc.MUTANTS)
def test_every_mutant_misses_a_bound(mut):
    """one thing wrong in the text: at least one held quantity of one family is past its bound (of 9 families x 2 MLP
    outputs x 6 quantities), and whether rel_l2 < 5e-5 over [:, :25] on the w + 2 family would have seen it - both as
    recorded in loss_cases.MUTANT_RECORD (listed in DESIGN.md)"""
    n, old_passes = mutant_counts(mut)
    print(f"{mut}: {n} bounds missed, old assertion {'passes' if old_passes else 'fails'}")
    assert (n, old_passes) == lc.MUTANT_RECORD[mut]
    if mut in lc.OUTSIDE_THE_LIMITS:
        assert n == 0
    else:
        assert n >= 1


def test_the_clamp_acts_only_at_exact_gimbal_lock():
    """drop_clamp is invisible on every family: the fp32 argument of asin leaves [-1, 1] only when 1 - s^2 <= 2 eps32,
    rho <= 5e-4, below RHO_MIN.  At exact lock it is what keeps the text finite - the mutant is a real change."""
    r = np.linspace(0.5, 3.0, 64)
    q = np.stack([r, 0 * r, 0 * r, r], axis=1).astype(np.float32)
    rows = np.zeros((64, 25), np.float32)
    rows[:, 3:7] = q
    good = lc.emulate(rows, np.zeros((64, 25)), rows, DS, 1, 29.0)
    bad = lc.emulate(rows, np.zeros((64, 25)), rows, DS, 1, 29.0, "drop_clamp")
    assert np.isfinite(good["ep"]).all() and not np.isfinite(bad["ep"]).all()


def test_the_angle_error_has_to_be_carried_into_the_h_block():
    """the bound of dout's h block without the angle term, C_VJP eps32 kappa alone, is missed by the text itself and by the
    reference's own fp32 arithmetic (rows whose e_p - e_t is small against the angles' error): the term is not slack"""
    from Utils.transformations import quaternion_to_euler
    K, denom = 4, 29.0
    base, out, target = rows_of("near_gimbal", "zero", K)
    o = lc.oracle(base, out, target, DS, K, denom)
    lit = lc.constants()[1] * lc.EPS32 * o["kappa"] * o["scale"][3]
    e = lc.emulate(base, out, target, DS, K, denom)
    pred = torch.tensor(o["pred"], requires_grad=True)
    torch_loss(pred, torch.tensor(target), K, denom, torch.float32, quaternion_to_euler).backward()
    ref = pred.grad.numpy()[:, 3:7] * np.float32(DS)
    for got in (e["dout"][:, 3:7], ref):
        err = np.abs(got - o["dout"][:, 3:7]).max(axis=1)
        assert (err > lit).sum() >= 3
        assert np.all(err <= lc.bounds(o)["h"])
