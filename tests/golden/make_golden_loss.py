"""Writes tests/golden/loss_terms.npz: the UNMODIFIED reference's ``Utils/transformations.quaternion_to_euler`` on the
quaternions of every family of tests/loss_cases.py.  Runs only where the reference is (as make_golden.py); the file holds
data only.  physics_train.py itself cannot be imported (fastdtw), so the four-term sum around the function is restated in
the tests, as ``four_term_loss`` of test_gpu_train.py does.

    python tests/golden/make_golden_loss.py

Per family ``<name>``: ``_qp`` / ``_qt`` fp32 [M, 4] (the rows' predicted and target quaternions, MLP output 0), ``_ep`` /
``_et`` fp32 [M, 3] the reference's angles, ``_ge`` fp32 [M, 3] = fl32(2 w_e (e_p - e_t)) of the fp64 oracle with K = 1 and
denom = 1, ``_gq`` fp32 [M, 4] the reference's fp32 autograd gradient of sum(ge * e) at qp.  tests/loss_cases.py computes
C_ANG and C_VJP from this file."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/knode_cosserat"
sys.path.insert(0, REF)
from Utils.transformations import quaternion_to_euler as ref_q2e  # noqa: E402  (reference)

sys.path.insert(0, os.path.join(HERE, ".."))
import loss_cases as lc  # noqa: E402


def main():
    out = {}
    for name in lc.FAMILIES:
        c = lc.family(name)
        qp, qt = np.ascontiguousarray(c["base"][:, 3:7]), np.ascontiguousarray(c["target"][:, 3:7])
        ep64, et64 = lc.euler_parts(qp)[0], lc.euler_parts(qt)[0]
        ge = (2.0 / 3.0 * (ep64 - et64)).astype(np.float32)
        q = torch.tensor(qp.T.copy(), requires_grad=True)
        ep = ref_q2e(q)
        (ep * torch.tensor(ge.T.copy())).sum().backward()
        et = ref_q2e(torch.tensor(qt.T.copy()))
        assert ep.dtype == torch.float32 and q.grad.dtype == torch.float32
        out[name + "_qp"], out[name + "_qt"] = qp, qt
        out[name + "_ep"], out[name + "_et"] = ep.detach().numpy().T.copy(), et.numpy().T.copy()
        out[name + "_ge"], out[name + "_gq"] = ge, q.grad.numpy().T.copy()
        assert all(np.isfinite(v).all() for v in out.values()), name
    path = os.path.join(HERE, "loss_terms.npz")
    np.savez_compressed(path, **out)
    a, v, per = lc.reference_constants(np.load(path))
    for name, (fa, fv) in per.items():
        print(f"{name}: angles {fa:.2f} eps32 / rho, Jacobian-transpose product {fv:.2f} eps32 kappa")
    print(f"reference: {a:.3f}, {v:.3f}; C_ANG = {lc.MARGIN * a:.2f}, C_VJP = {lc.MARGIN * v:.2f}; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
