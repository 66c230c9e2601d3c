"""CPU-only: the tolerances tests/test_row_kernels_abi_gpu.py holds the fp32 row kernels to (tests/row_kernel_bounds.py) tell the
formulation the kernels use from the nearest wrong one. Each bound is derived there; here an fp32 restatement of the right form
has to pass it and a restatement of the wrong form has to miss it by a wide margin - so that a later change that makes a bound
soft (or a data set harmless) fails here, on any machine."""
import pytest
import torch

import row_kernel_bounds as RB

OFFSET_COLS = [64, 768, 1024, 4096, 8192]


@pytest.mark.parametrize("cols", OFFSET_COLS)
def test_large_offset_tolerance_accepts_two_pass_and_rejects_one_pass(cols):
    x, g, b = RB.ln_offset_rows(RB.OFFSET_ROWS, cols, seed=cols)
    ref = RB.ln64(x, g, b, 1e-12)
    mean_tol, y_tol = RB.ln_offset_tolerances(x, g, ref)
    two, one = RB.ln_two_pass_f32(x, g, b, 1e-12), RB.ln_one_pass_f32(x, g, b, 1e-12)
    err_mean = (two["mean"].double() - ref["mean"]).abs()
    err_two = (two["y"].double() - ref["y"]).abs()
    err_one = (one["y"].double() - ref["y"]).abs()
    print("cols %5d: two-pass y err %.3e (worst err / tol %.3f), mean err %.3e (tol %.3e); one-pass y err %.3e (%.0f x tol)" % (
        cols, err_two.max(), (err_two / y_tol).max(), err_mean.max(), mean_tol.min(), err_one.max(), (err_one / y_tol).max()))
    assert (err_mean <= mean_tol).all()
    assert (err_two <= y_tol).all()
    # the one-pass variance E[x^2] - E[x]^2 cancels 6 of fp32's 7 digits at |mean| / std = 1000
    assert (err_one / y_tol).max() > 100
    # and the bound itself stays far below the ordinary 2e-5-class bar times the 1000-fold offset: it is not a blanket
    assert y_tol.max() < 5e-3


@pytest.mark.parametrize("cols", [260, 1028, 4100])
def test_small_variance_rows_reject_eps_ignored_and_eps_outside_the_root(cols):
    x, g, b = RB.ln_small_variance_rows(5, cols, seed=cols)
    for eps in (1e-12, 1e-5, 1e-1):
        ref = RB.ln64(x, g, b, eps)
        _, y_tol = RB.ln_offset_tolerances(x, g, ref)
        two = RB.ln_two_pass_f32(x, g, b, eps)
        assert ((two["y"].double() - ref["y"]).abs() <= y_tol).all(), eps
        if eps == 1e-5:
            for wrong in (RB.ln64_eps_ignored, RB.ln64_eps_outside):
                ratio = ((wrong(x, g, b, eps) - ref["y"]).abs() / y_tol).max().item()
                print("cols %d eps %g %s: %.0f x tolerance" % (cols, eps, wrong.__name__, ratio))
                assert ratio > 10


@pytest.mark.parametrize("shift", [64.0, 1000.0])
def test_cross_entropy_shift_tolerance_rejects_the_rounded_lse_form(shift):
    logits, labels = RB.xent_shift_case(37, 1601, seed=5)
    want = RB.xent64(logits, labels)["row_loss"]
    tol = RB.loss_tolerance(want)
    shifted = logits + shift                                # (fp32: the kernel sees these values)
    want_s = RB.xent64(shifted, labels)["row_loss"]
    old = (RB.xent_row_loss_f32(shifted, labels, shift_free=False).double() - want_s).abs()
    new = (RB.xent_row_loss_f32(shifted, labels, shift_free=True).double() - want_s).abs()
    print("shift %g: lse - x[label] err %.3e, log(s) - (x[label] - max) err %.3e, tolerance %.3e" % (
        shift, old.max(), new.max(), tol.min()))
    assert (new <= tol).all()
    if shift == 1000.0:
        assert (old > tol).any()
    # without a shift both forms pass: the tolerance is the one the unshifted test already uses
    for form in (False, True):
        assert ((RB.xent_row_loss_f32(logits, labels, shift_free=form).double() - want).abs() <= tol).all()


def test_activation_references_agree_with_autograd():
    x = RB.act_sweep()
    assert x.numel() == 4104 and x.dtype == torch.float32
    for act in ("gelu", "relu", "swish"):
        x64 = x.double().requires_grad_(True)
        val = {"gelu": lambda t: t * 0.5 * (1.0 + torch.erf(t / 2.0 ** 0.5)), "relu": torch.relu,
               "swish": lambda t: t * torch.sigmoid(t)}[act](x64)
        val.sum().backward()
        want_v, want_d = RB.act64(act, x)
        assert (val.detach() - want_v).abs().max() <= 1e-15 * 1e4
        assert (x64.grad - want_d).abs().max() <= 1e-12
