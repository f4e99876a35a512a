"""CPU-only tests of the bank of trainings (``kr_train_bank_*``): the host-side rule check ``kr_train_bank_check`` through
the built library, and the C layout of the ctypes mirror of ``kr_train_bank_net``.  Nothing here touches a GPU: the
pointers handed to the check are never dereferenced."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def kn():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    kn.load()
    return kn


TANH, SOFTPLUS, RELU = 1, 2, 3


def _nets(kn, S, null=None):
    """len(S) rows with distinct non-null fake device addresses; null = (row, field) sets one pointer to NULL."""
    nets = (kn.KrTrainBankNet * max(len(S), 1))()
    for k, s in enumerate(S):
        t = nets[k]
        t.S, t.ds = s, 0.05 + 0.01 * k
        for j, f in enumerate(("params", "grads", "exp_avg", "exp_avg_sq", "lower", "sched", "x", "base", "target_rows",
                               "loss_log")):
            setattr(t, f, 0x10000 * (k + 1) + 0x100 * j)
    if null is not None:
        setattr(nets[null[0]], null[1], None)
    return nets


def _check(kn, S, dims, acts, K=4, in_pad=32, denom=29.0, n_nets=None, null=None):
    lib = kn.load()
    n = len(dims) - 1
    rc = lib.kr_train_bank_check(len(S) if n_nets is None else n_nets, _nets(kn, S, null), K, n,
                                 (C.c_int32 * (n + 1))(*dims), (C.c_int32 * n)(*acts), in_pad, denom)
    return rc, (lib.kr_last_error() or b"").decode()


@pytest.mark.parametrize("S,dims,acts", [
    ((29,) * 8, [28, 512, 25], [TANH, 0]),                 # the reference's shape, one trajectory each
    ((58, 87, 58, 87), [28, 512, 25], [TANH, 0]),          # its data sets of 2 and 3 trajectories: differing S_k
    ((29, 3), [28, 64, 64, 25], [SOFTPLUS, SOFTPLUS, 0]),  # three layers
    ((29, 3), [28, 96, 25], [RELU, 0]),                    # ragged widths
    ((29, 3), [28, 40, 24, 25], [RELU, RELU, 0]),
    ((1,), [28, 512, 25], [TANH, 0]),
])
def test_bank_check_accepts(kn, S, dims, acts):
    rc, msg = _check(kn, S, dims, acts)
    assert rc == 0, msg


@pytest.mark.parametrize("kw,code,words", [
    (dict(S=(), n_nets=0), "ARG", ["n_nets"]),
    (dict(S=(29, 0, 29)), "ARG", ["network 1", "S must"]),
    (dict(S=(29, 29, -3)), "ARG", ["network 2", "S must"]),
    (dict(K=0), "ARG", ["K"]),
    (dict(denom=0.0), "ARG", ["denom"]),
    (dict(denom=-29.0), "ARG", ["denom"]),
    (dict(in_pad=64), "UNSUPPORTED", ["in_pad"]),
    (dict(acts=[TANH, TANH]), "UNSUPPORTED", ["activation after the last layer"]),
    (dict(dims=[28, 128, 64, 25], acts=[TANH, TANH, 0]), "UNSUPPORTED", ["H1, H2 <= 64"]),
    (dict(dims=[28, 64, 65, 25], acts=[TANH, TANH, 0]), "UNSUPPORTED", ["H1, H2 <= 64"]),
    (dict(null=(2, "params")), "ARG", ["network 2", "params"]),
    (dict(null=(1, "target_rows")), "ARG", ["network 1", "target_rows"]),
    (dict(null=(0, "sched")), "ARG", ["network 0", "sched"]),
    (dict(dims=[28, 32, 32, 32, 25], acts=[TANH, TANH, TANH, 0]), "UNSUPPORTED", ["4 layers"]),
])
def test_bank_check_refuses_naming_the_rule_and_the_network(kn, kw, code, words):
    args = dict(S=(29, 29, 29), dims=[28, 512, 25], acts=[TANH, 0])
    args.update(kw)
    rc, msg = _check(kn, **args)
    assert rc == {"ARG": kn.KR_E_ARG, "UNSUPPORTED": kn.KR_E_UNSUPPORTED}[code], (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_nullable_pointers_are_accepted(kn):
    for f in ("lower", "loss_log"):
        rc, msg = _check(kn, (29, 29), [28, 512, 25], [TANH, 0], null=(1, f))
        assert rc == 0, (f, msg)


def test_bank_net_layout_matches_header(kn, tmp_path):
    """The ctypes mirror of kr_train_bank_net has the C layout (checked by compiling a probe)."""
    fields = [f for f, _ in kn.KrTrainBankNet._fields_]
    probe = str(tmp_path / "_bank_layout_probe")
    with open(probe + ".c", "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "knode_rod.h"\n'
                'int main(){printf("%zu", sizeof(kr_train_bank_net));\n'
                + "".join(f'printf(" %zu", offsetof(kr_train_bank_net, {name}));\n' for name in fields)
                + 'printf("\\n");return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), probe + ".c", "-o", probe], check=True)
    vals = [int(v) for v in subprocess.run([probe], capture_output=True, text=True, check=True).stdout.split()]
    assert vals == [C.sizeof(kn.KrTrainBankNet)] + [getattr(kn.KrTrainBankNet, name).offset for name in fields]
    assert len(fields) == 12
