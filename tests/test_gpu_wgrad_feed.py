"""The quarter-form weight-gradient kernel's operand feed (csrc/rnde_wgradx.h, FEED 1 -- neighbouring lanes load neighbouring 16-byte pieces of one column,
threads without a unit load nothing, unpadded XOR-swizzled LDS image; RNDE_X3_WGRAD_FEED=1) against the kernel as first built (FEED 0, RNDE_X3_WGRAD_Q0=1).  Both issue the same
six terms per 32 columns on the same operand values in the same order into the same chunks and slabs, so the parameter gradient is the same BITS; the
switch sits behind the reverse sweep, so x-bar is too.  A swizzled image can pass a spot check on wrong data: every entry of p-bar is compared, and the rows
the remapping can misplace on their own -- the synthetic {t, 1} quad, i.e. the time columns and biases of both layers -- once more by themselves.

MNIST geometry 784-100-784, matrix mode 1, regularize = 1, Glorot x 3.  At tolerance 1e-3 a solve is 6 attempts (measured, B = 16 .. 272), and the launches
underneath the sweep start at eight: the two cases that are about them run at 1e-5 (about 15 attempts, Tsit5: attempts ~ tol^(-1/5)) and assert that they got
their eight.  Shapes, the smallest at which the feed can go wrong:
    B =  16, side   0   every evaluation is a single half-empty 32-column step
    B =  37, side   0   a full step plus one of five columns
    B = 100, side 100   every launch is the 32-workgroup side form; last step of 4 columns
    B = 272, side  30   chunks span evaluation boundaries; both launch forms"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, H = 784, 100


def _run(B, side, q0, monkeypatch):
    tol = 1e-3 if side == 0 else 1e-5
    from tests.test_gpu_x3 import _cfg, _problem
    from tests.util import Node
    arch, p, x, ubar = _problem(B, 41, 3.0)
    monkeypatch.setenv("RNDE_WGRAD_SIDE", str(side))
    monkeypatch.delenv("RNDE_X3_WGRAD_HALF", raising=False)
    monkeypatch.delenv("RNDE_X3_WGRAD_OFF", raising=False)
    monkeypatch.delenv("RNDE_X3_WGRAD_FEED", raising=False)
    if q0:
        monkeypatch.setenv("RNDE_X3_WGRAD_Q0", "1")
    else:
        monkeypatch.delenv("RNDE_X3_WGRAD_Q0", raising=False)
        monkeypatch.setenv("RNDE_X3_WGRAD_FEED", "1")
    node = Node(_cfg(B, tol, regularize=1), matrix_mode=1)
    got = node.forward(x, p, keep_tape=True)
    n = len(got["saveval"])
    xb, pb, _ = node.backward(ubar, np.full(n, 10.0 / n, np.float32))
    node.close()
    return got["nattempts"], np.array(xb, copy=True), np.array(pb, copy=True)


@pytest.mark.parametrize("B,side", [(16, 0), (37, 0), (100, 100), (272, 30)])
def test_wgrad_feed_is_bit_identical_to_the_first_quarter_form(B, side, monkeypatch):
    att1, xb1, pb1 = _run(B, side, False, monkeypatch)
    att0, xb0, pb0 = _run(B, side, True, monkeypatch)
    assert att1 == att0 and (side == 0 or att1 >= 8)           # (the launches underneath the sweep start at eight attempts)
    assert np.array_equal(xb1, xb0)                            # the switch does not touch the sweep
    assert np.abs(pb1).max() > 0 and np.all(np.isfinite(pb1))
    # Flux.destructure order: W1 (H x (D + 1), column-major, last column = time), b1, W2 (D x (H + 1), last column = time), b2
    o_w1t, o_b1, o_w2, o_end = H * D, H * (D + 1), H * (D + 1) + H, H * (D + 1) + H + D * (H + 1) + D
    assert pb1.size == o_end
    syn = np.r_[o_w1t:o_w2, o_w2 + D * H:o_end]               # layer 1: time column and bias; layer 2: time column and bias
    assert np.abs(pb1[syn]).max() > 0
    assert np.array_equal(pb1[syn], pb0[syn])
    assert np.array_equal(pb1, pb0)
