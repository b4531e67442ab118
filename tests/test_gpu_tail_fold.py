"""The small launches in front of the solve and behind the reverse sweep folded into their neighbours, one host switch each, read per call
(the tests set every one of them explicitly; the library's defaults: the first off, the other three on):

    RNDE_X3_PACK_FOLD   the x3 weight split (rnde_x3_pack_kernel) inside the pack launch (rnde_pack_all_kernel)
    RNDE_BINIT_PAIR     the reverse of the initial-step rule as two paired launches (rnde_binit_pair_kernel) instead of four
    RNDE_WGRAD_PAIR     both layers' full-width weight-gradient launches behind the sweep as one (rnde_wgrad4x_pair_kernel)
    RNDE_REDUCE_FOLD    the two passes of the weight-gradient reduction as one launch (rnde_wgrad_reduce_fold_pair)

Every folded form runs the instructions of the launches it replaces on the same values and forms every sum in the same order, so every output must be
BIT-identical between the settings: end state, NFE, step log, callback values, x-bar, p-bar and tspan-bar (track_initdt on: the reverse of the initial-step
rule reaches all three).  rnde_node_tail_folds counts the launches that took a folded form: a comparison in which the folded form did not run would
compare the old code with itself.

Headline geometry (D = 784, H = 100, col_tile 16: the folded paths exist for it alone), one handle per case; the same taped forward and reverse pass with
all switches off, all on, and all on again (the second folded pass finds the hand-off slabs as the first left them).
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_forward import _cfg
from tests.test_gpu_launch_fold import D, _assert_identical, _problem, _raw_forward

pytestmark = pytest.mark.gpu

SWITCHES = ("RNDE_REDUCE_FOLD", "RNDE_WGRAD_PAIR", "RNDE_X3_PACK_FOLD", "RNDE_BINIT_PAIR")      # (the order of rnde_node_tail_folds' counts)


def _folds(node):
    node.L.rnde_node_tail_folds.restype = None
    node.L.rnde_node_tail_folds.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    c = (C.c_int64 * 4)()
    node.L.rnde_node_tail_folds(node.h, c)
    return np.array(list(c), dtype=np.int64)


def _set(monkeypatch, on):
    """`on`: the switches that are on; every other one is set to 0"""
    for s in SWITCHES:
        monkeypatch.setenv(s, "1" if s in on else "0")


def _run(monkeypatch, B, tol, act2, reg, settings, side=False, max_attempts=96, min_attempts=0, env=()):
    """One handle; for each entry of `settings` (a tuple of the switches that are on) the same taped forward and reverse pass.  Returns the result tuples
    (the layout _assert_identical compares) and, per setting, how many launches took each folded form."""
    from tests.util import Node
    for k in ("RNDE_X3", "RNDE_PERSIST"):      # (read at creation; the library's defaults -- matrix mode 1, persistent kernels -- unless `env` says otherwise)
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    if not side:
        monkeypatch.setenv("RNDE_WGRAD_SIDE", "0")      # (one partition of the weight-gradient GEMMs; `side`: the default share runs underneath the sweep)
    else:
        monkeypatch.delenv("RNDE_WGRAD_SIDE", raising=False)
    arch, p, x = _problem(B, act2, 5, 2.0)
    node = Node(_cfg(arch, B, reltol=tol, abstol=tol, col_tile=16, max_attempts=max_attempts, regularize=reg, track_initdt=1))
    outs, took = [], []
    for on in settings:
        _set(monkeypatch, on)
        before = _folds(node)
        st, u, nfe, sv, steps = _raw_forward(node, x, p, 0.0, 1.0, keep_tape=True)
        assert st == 0 and len(steps) >= min_attempts
        ubar = np.random.default_rng(9).standard_normal((B, D)).astype(np.float32)
        grads = node.backward(ubar, np.full(len(sv), 3.0, dtype=np.float32))
        assert node.L.rnde_node_fallback_count(node.h) == 0
        outs.append((st, u, nfe, sv, steps, grads))
        took.append(_folds(node) - before)
    node.close()
    return outs, took


ALL = tuple(SWITCHES)


@pytest.mark.parametrize("B,tol,act2,reg,side", [
    (16, 1e-3, 1, 1, False),         # one column tile
    (37, 1e-3, 1, 0, False),         # a ragged last tile, no regulariser
    (100, 1e-3, 0, 3, False),        # 7 tiles, the other dynamics form, the stiffness regulariser
    (272, 1e-3, 1, 1, False),        # 17 tiles: more than 16 chunks' worth of slabs, the grouped branch of the reduction
    (37, 1e-3, 0, 1, False),
    (16, 1.4e-8, 1, 1, True)])       # the headline tolerance; n_att >= 8 and the default side share: the side-stream launches run beside the merged one
def test_folded_tail_is_bit_identical(B, tol, act2, reg, side, monkeypatch):
    outs, took = _run(monkeypatch, B, tol, act2, reg, ((), ALL, ALL), side=side, min_attempts=8 if side else 0)
    assert outs[0][2] >= 15 and np.isfinite(outs[0][1]).all() and all(np.isfinite(g).all() for g in outs[0][5])
    _assert_identical(outs)
    assert not took[0].any()
    for t in took[1:]:      # every folded form ran: one merged weight-gradient launch, one pack launch with the x3 split in it, two paired launches
        assert t[1] == 1 and t[2] == 1 and t[3] == 2
        if B == 272 or side:
            assert t[0] == 1      # (more than 16 chunks per layer: the grouped reduction, as one launch)


@pytest.mark.parametrize("switch", SWITCHES)
def test_each_fold_alone_is_bit_identical(switch, monkeypatch):
    """one switch at a time against all of them off (B = 37: three column tiles, the last one ragged)"""
    outs, took = _run(monkeypatch, 37, 1e-3, 1, 1, ((), (switch,)))
    _assert_identical(outs)
    i = SWITCHES.index(switch)
    assert not took[0].any() and not np.delete(took[1], i).any()
    if switch != "RNDE_REDUCE_FOLD":      # (the reduction folds only above 16 chunks per layer: whether this solve has that many is the step controller's business)
        assert took[1][i] == (2 if switch == "RNDE_BINIT_PAIR" else 1)


def test_four_binit_launches_serve_without_the_persistent_kernels(monkeypatch):
    """RNDE_PERSIST=0 (read at creation): the paired launches are not used, the four stand-alone ones serve, whatever the switch says -- and give the bits of
    the handle that runs the persistent kernels (fp32 matrix mode, one weight-gradient partition: the setting in which the launch-per-stage kernels and the
    persistent ones are bit-identical, tests/test_gpu_forward.py::test_persistent_attempt_is_bit_identical)."""
    env = (("RNDE_X3", "0"),)
    ref, took_ref = _run(monkeypatch, 37, 1e-3, 1, 1, ((), ALL), env=env)
    assert took_ref[1][3] == 2
    got, took = _run(monkeypatch, 37, 1e-3, 1, 1, ((), ALL), env=env + (("RNDE_PERSIST", "0"),))
    assert took[0][3] == 0 and took[1][3] == 0
    _assert_identical(ref + got)
