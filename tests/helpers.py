"""Shared comparison helpers for the parity tests."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases  # noqa: E402

# Parity bar from BASELINE.json north_star: fp32 1e-4. Checked as |got - want| <= ATOL + RTOL * |want|.
# vision_logit carries +(-10000) on masked regions where one fp32 ulp is 9.8e-4 and the reference
# itself is only good to ~5e-4 against fp64; the relative term covers those entries.
ATOL = 1e-4
RTOL = 1e-4


def assert_close(got, want, name="", atol=ATOL, rtol=RTOL):
    got = torch.as_tensor(np.asarray(got.detach().cpu()) if isinstance(got, torch.Tensor) else got).double()
    want = torch.as_tensor(np.asarray(want.detach().cpu()) if isinstance(want, torch.Tensor) else want).double()
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got).all(), "%s: non-finite values" % name
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    worst = (err - bound).max().item()
    assert worst <= 0, "%s: max abs err %.3e exceeds %.1e + %.1e*|ref| (max |ref| %.3e)" % (
        name, err.max().item(), atol, rtol, want.abs().max().item())
    return err.max().item()


def load_golden(case):
    with np.load(cases.path(case)) as z:
        return {k: z[k] for k in z.files}


def to_device(args, device):
    return tuple(a.to(device) if isinstance(a, torch.Tensor) else a for a in args)


# ---------------------------------------------------------------------------------------------------------------------
# the bf16 training path (tests/test_bf16_stream_gpu.py, test_bf16_helpers_gpu.py, test_bf16_round.py)
# ---------------------------------------------------------------------------------------------------------------------
def close16(got, want64, mag64, what, extra64=0.0):
    """got (bf16 or fp32 tensor) vs float64 `want`: fp32 accumulation + one bf16 rounding (fp32 outputs: accumulation only).
    extra64: a further error term of the operation itself that the caller has derived (default none)."""
    g = got.detach().cpu().double()
    assert g.shape == want64.shape and torch.isfinite(g).all(), what
    tol = 3e-6 * mag64 + 1e-5 + (want64.abs() / 256 if got.dtype == torch.bfloat16 else 0.0) + extra64
    err = (g - want64).abs()
    assert (err <= tol).all(), "%s: worst err / tol %.3f" % (what, float((err / tol).max()))


def layernorm16_reference(x, dy, g, b, eps):
    """float64 BertLayerNorm forward / backward on the bf16 values x, dy [rows, cols] (CPU) with fp32 g, b [cols]:
    dict of y, mean, var (per row), xh, dx, dgamma, dbeta."""
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    xh = (xd - mu) / torch.sqrt(var + eps)
    gd = dy.double() * g.double()
    dx = (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True)) / torch.sqrt(var + eps)
    return {"y": g.double() * xh + b.double(), "mean": mu[:, 0], "var": var[:, 0], "xh": xh, "dx": dx,
            "dgamma": (dy.double() * xh).sum(0), "dbeta": dy.double().sum(0)}


BF16_ROUND_LOWS = (0x0000, 0x0001, 0x7ffe, 0x7fff, 0x8000, 0x8001, 0xfffe, 0xffff)


def rounding_patterns():
    """uint32 [65536 * 8]: the fp32 bit patterns (hi << 16) | lo of every upper half and eight lower halves (hi-major) - every
    rounding decision of fp32 -> bf16: below / at / above a tie with an even and an odd kept bit, for every exponent and both
    signs; fp32 subnormals, the largest finites (which round to Inf), +-Inf and every NaN class."""
    hi = np.arange(1 << 16, dtype=np.uint32)[:, None] << 16
    return (hi | np.array(BF16_ROUND_LOWS, dtype=np.uint32)[None, :]).reshape(-1)


def torch_cast_bits(bits32):
    """bits (uint16 array) of torch's CPU fp32 -> bf16 cast of the fp32 values with the bits `bits32` (uint32 array)."""
    x = torch.from_numpy(bits32.view(np.int32).copy()).view(torch.float32)
    return x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def check_rounding_contract(bits32, got16, what):
    """The rounding contract of every fp32 -> bf16 store: a non-NaN input gives torch's CPU cast bit for bit, a NaN input
    gives a bf16 NaN. bits32 uint32 / got16 uint16 arrays of one shape; returns the mask of the NaN inputs."""
    bits32, got16 = np.asarray(bits32).reshape(-1), np.asarray(got16).reshape(-1)
    assert bits32.dtype == np.uint32 and got16.dtype == np.uint16 and bits32.shape == got16.shape, what
    nan = (bits32 & 0x7fffffff) > 0x7f800000
    want = torch_cast_bits(bits32)
    bad = np.flatnonzero(~nan & (got16 != want))
    assert bad.size == 0, "%s: %d non-NaN values differ from torch's cast, first fp32 0x%08x -> 0x%04x, want 0x%04x" % (
        what, bad.size, bits32[bad[0]], got16[bad[0]], want[bad[0]])
    lost = np.flatnonzero(nan & ((got16 & 0x7fff) <= 0x7f80))
    assert lost.size == 0, "%s: %d NaN inputs did not stay NaN, first fp32 0x%08x -> bf16 0x%04x" % (
        what, lost.size, bits32[lost[0]], got16[lost[0]])
    return nan
