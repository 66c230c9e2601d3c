"""References, derived tolerances and fp32 restatements for the direct tests of the fp32 row kernels (csrc/layernorm.hip,
embed.hip, loss.hip, elementwise.hip). Test infrastructure shared by tests/test_row_kernels_abi_gpu.py (which holds the kernels
to these bounds) and tests/test_row_kernels_tolerances.py (which shows on the CPU that each bound accepts the formulation the
kernels use and rejects the nearest wrong one). Nothing here is fitted to what a kernel returns.

LayerNorm (TF style, vilbert.py:313-317): y = gamma (x - mean) / sqrt(var + eps) + beta, biased variance, eps inside the root.

Tolerance of a row whose |mean| is large against its spread (`ln_offset_tolerances`). The kernel sums a row as: per lane the
chunks in order, each chunk as (x0 + x1) + (x2 + x3), then six butterfly steps over the 64 lanes (rowops.h ln_finish). The longest
chain of additions a value passes through is D = ceil(cols / 256) + 8 (the lane's chunks, the two in-chunk pair sums, six
shuffle steps); each addition rounds a partial sum that is at most the whole sum, so
    |mean error| <= D 2^-24 mean|x|.
The deviations x - mean are then exact up to one rounding and all carry that mean error; the variance changes by its square
(second order). So
    |y error| <= D 2^-24 mean|x| rstd |gamma| + 8 2^-24 |y| + 1e-6
(the second term: the roundings of the deviation, of rstd, of the two products and of the final add; the last: an absolute
floor for values next to zero).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32


# ---- LayerNorm -------------------------------------------------------------------------------------------------------
def ln64(x, gamma, beta, eps):
    """float64 reference from the fp32 values x [rows, cols], gamma, beta [cols]: dict y, mean, rstd, xhat."""
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    var = (xd - mu).pow(2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (xd - mu) * rstd
    return {"y": gamma.double() * xh + beta.double(), "mean": mu[:, 0], "rstd": rstd[:, 0], "xhat": xh, "var": var[:, 0]}


def ln64_eps_ignored(x, gamma, beta, eps):
    """The wrong formulation that drops eps."""
    return ln64(x, gamma, beta, 0.0)["y"]


def ln64_eps_outside(x, gamma, beta, eps):
    """The wrong formulation that adds eps outside the square root (the torch.nn.LayerNorm-unlike `std + eps` form)."""
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    var = (xd - mu).pow(2).mean(-1, keepdim=True)
    return gamma.double() * ((xd - mu) / (torch.sqrt(var) + eps)) + beta.double()


def ln_chain_length(cols):
    return (cols + 255) // 256 + 8


def ln_offset_tolerances(x, gamma, ref):
    """(mean_tol [rows], y_tol [rows, cols]) float64 - the module docstring's bounds for the fp32 rows x and ln64's `ref`."""
    d = ln_chain_length(x.shape[-1])
    mean_tol = d * U * x.double().abs().mean(-1)
    y_tol = mean_tol[:, None] * ref["rstd"][:, None] * gamma.double().abs()[None, :] + 8 * U * ref["y"].abs() + 1e-6
    return mean_tol, y_tol


def _kernel_row_sum(v):
    """fp32 sum of each row of v [rows, cols] (float32 numpy, cols % 4 == 0) in ln_finish's order: lane l of 64 owns columns
    (64 i + l) 4 .. + 3 of chunk i, adds its chunks in order as (v0 + v1) + (v2 + v3), then the butterfly over the lanes."""
    rows, cols = v.shape
    nv = (cols + 255) // 256
    pad = np.zeros((rows, nv * 256), dtype=np.float32)
    pad[:, :cols] = v
    q = pad.reshape(rows, nv, 64, 4)
    lane = np.zeros((rows, 64), dtype=np.float32)
    for i in range(nv):
        lane = lane + ((q[:, i, :, 0] + q[:, i, :, 1]) + (q[:, i, :, 2] + q[:, i, :, 3]))
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[:, idx ^ off]
    assert lane.dtype == np.float32
    return lane[:, 0]


def ln_two_pass_f32(x, gamma, beta, eps):
    """fp32 restatement of the kernel's two-pass form: dict y, mean, rstd (float32 torch tensors)."""
    v = x.numpy().astype(np.float32)
    n = np.float32(v.shape[1])
    mean = _kernel_row_sum(v) / n
    d = v - mean[:, None]
    var = _kernel_row_sum(d * d) / n
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps))
    y = gamma.numpy() * (d * rstd[:, None]) + beta.numpy()
    return {"y": torch.from_numpy(y), "mean": torch.from_numpy(mean), "rstd": torch.from_numpy(rstd)}


def ln_one_pass_f32(x, gamma, beta, eps):
    """The wrong formulation E[x^2] - E[x]^2 in fp32, same summation order."""
    v = x.numpy().astype(np.float32)
    n = np.float32(v.shape[1])
    mean = _kernel_row_sum(v) / n
    var = np.maximum(_kernel_row_sum(v * v) / n - mean * mean, np.float32(0.0))
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps))
    y = gamma.numpy() * ((v - mean[:, None]) * rstd[:, None]) + beta.numpy()
    return {"y": torch.from_numpy(y), "mean": torch.from_numpy(mean), "rstd": torch.from_numpy(rstd)}


OFFSET_ROWS = 32       # rows per large-offset case: the worst row of a wrong formulation needs a few rows to show


def ln_offset_rows(rows, cols, seed):
    """Rows with mean 1000 and standard deviation 1, and a gamma / beta pair."""
    g = torch.Generator().manual_seed(seed)
    x = 1000.0 + torch.randn(rows, cols, generator=g)
    return x, 1 + 0.1 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)


def ln_small_variance_rows(rows, cols, seed):
    """Rows with mean 0.5 and standard deviation 1e-3 (variance about 1e-6: eps = 1e-5 and 1e-1 dominate it)."""
    g = torch.Generator().manual_seed(seed)
    x = 0.5 + 1e-3 * torch.randn(rows, cols, generator=g)
    return x, 1 + 0.1 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)


def ln_backward64(x, dy, gamma, eps):
    """float64 autograd of the TF-style formula (mean / rstd recomputed in float64): dict dx, dgamma, dbeta and the per-column
    sums of |term| of the two column reductions (dgamma_mag, dbeta_mag)."""
    x64, g64 = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    b64 = torch.zeros_like(g64).requires_grad_(True)
    mu = x64.mean(-1, keepdim=True)
    var = (x64 - mu).pow(2).mean(-1, keepdim=True)
    xh = (x64 - mu) / torch.sqrt(var + eps)
    (g64 * xh + b64).backward(dy.double())
    return {"dx": x64.grad, "dgamma": g64.grad, "dbeta": b64.grad,
            "dgamma_mag": (dy.double() * xh.detach()).abs().sum(0), "dbeta_mag": dy.double().abs().sum(0)}


# ---- cross entropy ---------------------------------------------------------------------------------------------------
XENT_LOSS_RTOL, XENT_LOSS_ATOL = 2e-6, 1e-6       # tests/test_kernels_gpu.py::test_cross_entropy_forward_backward
XENT_GRAD_RTOL, XENT_GRAD_ATOL = 2e-5, 2e-7


def xent64(logits, labels, ignore=-1):
    """float64 reference: dict row_loss [rows] (0 for ignored rows), lse, p (softmax), count."""
    x = logits.double()
    lse = torch.logsumexp(x, -1)
    live = labels != ignore
    picked = x.gather(1, labels.clamp(0, x.shape[1] - 1)[:, None])[:, 0]
    return {"row_loss": torch.where(live, lse - picked, torch.zeros_like(lse)), "lse": lse,
            "p": torch.exp(x - lse[:, None]), "count": int(live.sum())}


def xent_row_loss_f32(logits, labels, shift_free):
    """fp32 restatement of xent_fwd_kernel's row loss (every label valid): the maximum, the sum of expf(x - max) in fp32, then
    either the rounded lse = max + log(s) minus x[label] (shift_free False: the result carries half an ulp of |lse|, which grows
    with a common shift of the logits) or log(s) - (x[label] - max) (True: every term is of the size of the loss)."""
    x = logits.numpy().astype(np.float32)
    mx = x.max(1)
    s = np.exp(x - mx[:, None]).astype(np.float32).sum(1, dtype=np.float32)
    picked = x[np.arange(x.shape[0]), labels.numpy()]
    logs = np.log(s).astype(np.float32)
    if shift_free:
        out = logs - (picked - mx)
    else:
        out = (mx + logs) - picked
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def xent_shift_case(rows, n, seed):
    """Unit-variance logits and labels without ignored rows: the row loss is about log(n) + 1/2."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, n, generator=g), torch.randint(0, n, (rows,), generator=g)


def loss_tolerance(want64):
    return XENT_LOSS_ATOL + XENT_LOSS_RTOL * want64.abs()


# ---- activations -----------------------------------------------------------------------------------------------------
def act_sweep():
    """fp32 [4104]: 4,096 points over [-12, 12] and +-0, +-1e-30, +-40, +-1e4."""
    x = torch.linspace(-12.0, 12.0, 4096, dtype=torch.float64).float()
    extra = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 40.0, -40.0, 1e4, -1e4], dtype=torch.float32)
    return torch.cat([x, extra])


def _phi64(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))      # (erfc: no cancellation in the negative tail)


def act64(act, x):
    """(value, derivative) in float64 of gelu (erf form, vilbert.py:117) | relu | swish (x sigmoid(x), :120-121) at fp32 x."""
    x = x.double()
    if act == "gelu":
        phi = _phi64(x)
        return x * phi, phi + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if act == "relu":
        return torch.where(x > 0, x, torch.zeros_like(x)), (x > 0).double()
    s = torch.sigmoid(x)
    return x * s, s + x * s * (1.0 - s)


def act_grad_tolerance(act, x):
    """GELU: 4e-7 max(1, |x|) - twice the 1.5e-7 the polynomial erfc of csrc/common.h states, plus three fp32 roundings.
    SWISH: 16 2^-24 max(1, |x|). RELU: exact."""
    scale = x.double().abs().clamp(min=1.0)
    return {"gelu": 4e-7 * scale, "swish": 16 * U * scale, "relu": 0.0 * scale}[act]


def act_value_tolerance(act, x, want64):
    """GELU: |x| 4e-7 (x times the error of Phi) + 2^-24 |gelu| (the product's rounding). SWISH: x / (1 + exp(-x)) is an expf,
    an add and a division: 16 2^-24 |x| (the same budget as its derivative) + a denormal floor. RELU: exact."""
    ax = x.double().abs()
    return {"gelu": 4e-7 * ax + U * want64.abs(), "swish": 16 * U * ax + 1e-37, "relu": 0.0 * ax}[act]
