"""Every kernel that draws a dropout mask, against the mask computed on the host.

include/vilbert_hip.h promises keep(seed, element index) - csrc/rng.h - at every site; that is what lets forward and backward agree
without a stored mask and the fused sites stand in for the two-launch forms. The other tests read the mask off the kernel under
test (`probs != 0`, one kernel against another, an identity that holds for any mask): they cannot see a mask that repeats across
heads or samples, a wrong row stride, a forward and backward that are wrong in the same way, a bf16 build that differs from the
fp32 build in both directions, or a step counter mixed in with the wrong constant. Here the mask comes from
tests/dropout_restatement.py (pinned bit for bit to rng.h by tests/test_dropout_mask.py) and never from a kernel output.

Per site two checks. PATTERN: inputs chosen so that the output IS the mask - zeros exactly where the host drops (torch.equal on
booleans), the survivors equal to the expected constant. NUMERIC: random inputs, outputs and gradients against float64 torch
autograd using the host mask, within the bounds the project's tests of the same kernels already use.

Sites: vb_dropout; the fp32 linear epilogues (gemm_core.h fast + generic, both branches of gemm_v2.h, the persistent kernel's,
the bf16-planes kernels', fp8.hip's); HB_DROPRES of gemm_bf16.hip; the dx_dropped twin of the LayerNorm backward (fp32, bf16); the
attention kernels of both builds, one case per kernel path (the two-kernel LDS backward in a child process: its switch is read
once per process), key chunks included; the device step counter. Not repeated here, because they are already tied bit for bit
to the per-op path pinned here: row_drop_add_kernel, the whole-layer launcher (tests/test_layers_native_gpu.py) and the
pre-training row maps (tests/test_last_layer_rows_gpu.py).
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":            # the child process of the two-kernel case: no conftest has set the paths
    ROOT = os.path.dirname(TESTS)
    for _p in (TESTS, os.path.join(ROOT, "vilbert-multi-task_amd"), ROOT):
        sys.path.insert(0, _p)

import dropout_restatement as DR  # noqa: E402
import helpers  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
SEED = 0xC0FFEE1234567891          # top bit set
PS = [0.1, 0.5]


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _keep(idx, seed, p):
    """Host mask over the index array `idx` as a CPU bool tensor of its shape."""
    return torch.from_numpy(DR.keep(seed, idx, p))


def _scale(p):
    """The survivors' factor as the launchers compute it (fp32), as a Python float."""
    return float(DR.drop_scale(p))


def _close(got, want64, rtol=3e-5, atol=3e-5):
    """tests/test_backward_gpu.py's bound: fp32 round-off class, relative to the largest reference magnitude."""
    got = got.detach().cpu().double()
    assert got.shape == want64.shape, (got.shape, want64.shape)
    assert torch.isfinite(got).all()
    scale = max(1.0, want64.abs().max().item())
    err = (got - want64).abs().max().item()
    assert err <= atol * scale + rtol * scale, "max err %.3e (scale %.3e)" % (err, scale)


def _assert_pattern(got, keep, survivor, rtol=0.0, what=""):
    """got: CPU tensor whose zeros must be exactly the host's dropped elements, every survivor equal to `survivor`."""
    got = got.detach().cpu()
    assert got.shape == keep.shape, (got.shape, keep.shape)
    nz = got != 0
    assert torch.equal(nz, keep), "%s: %d elements differ from the host mask (kept fraction %.4f, host %.4f)" % (
        what, int((nz != keep).sum()), float(nz.float().mean()), float(keep.float().mean()))
    s = got[keep].double()
    if s.numel():
        assert float((s - survivor).abs().max()) <= rtol * abs(survivor), "%s: survivors %r .. %r, expected %r" % (
            what, float(s.min()), float(s.max()), survivor)


@pytest.fixture(scope="module")
def ops():
    from vilbert import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------------------------------
# vb_dropout: flat index; the float4 body and the n & 3 tail
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4099])
def test_vb_dropout(ops, n, residual, p):
    keep = _keep(DR.flat_index(n), SEED, p)
    # pattern: x = 1 -> exactly drop_scale or 0 (+ a constant residual, added un-masked)
    base = np.float32(2.0 if residual else 0.0)
    r = torch.full((n,), float(base)).to(DEV) if residual else None
    y = ops.dropout(torch.ones(n, device=DEV), p, SEED, r).cpu()
    want = torch.where(keep, torch.tensor(float(base + DR.drop_scale(p))), torch.tensor(float(base)))
    assert torch.equal(y != float(base), keep) and torch.equal(y, want)
    # numeric
    x, rr = _rand(n, seed=n), _rand(n, seed=n + 1)
    y = ops.dropout(x.to(DEV), p, SEED, rr.to(DEV) if residual else None).cpu()
    want = torch.where(keep, x.double() * _scale(p), torch.zeros(n, dtype=torch.float64)) + (rr.double() if residual else 0.0)
    assert torch.allclose(y.double(), want, rtol=1e-5, atol=1e-6)     # (test_dropout_mask_is_a_function_of_seed_and_index's)
    if not residual:
        assert torch.equal(y == 0, ~keep | (x == 0))


# ---------------------------------------------------------------------------------------------------------------------
# fp32 linear with residual and dropout: index row * N + col, N = all output columns of the launch
# ---------------------------------------------------------------------------------------------------------------------
# (tile code, persistent-kernel mode, M, seg_n, K, nseg). Which EPI_RES_DROP implementation a launch reaches (gemm.hip launch_gemm):
LINEAR_CASES = [
    # -1: round-1 kernel only (gemm_core.h tile_epilogue). 192 x 384 is re-cut into 64 x 64 tiles, all interior: the branch-free
    # epilogue_full<EPI_RES_DROP>; 100 x 200, K = 52 (no multiple of 16: round-1 kernel whatever the code) has interior tiles
    # (epilogue_full) and ragged edge tiles (the generic per-element loop)
    (-1, 0, 192, 384, 64, 1), (-1, 0, 100, 200, 52, 1), (0, 2, 100, 200, 52, 1),
    # 22, persistent kernels off: gemm_v2.h, 64 x 64 tiles, all full -> epilogue_v2's `EXT && full` branch (residual prefetched)
    (22, 0, 192, 384, 64, 1),
    # 44, off: 128 x 128 tiles, rows 128 .. 191 a ragged tile -> epilogue_v2's per-fragment branch (and the other on rows 0 .. 127)
    (44, 0, 192, 384, 64, 1),
    # 0 (cost model), off: whatever tile the planner takes by default
    (0, 0, 192, 384, 64, 1),
    # persistent kernel forced wherever eligible (mode 2): gemm_v4.h's own instantiation of epilogue_v2 (EXT_DEPTH 0 in the forward
    # layout: the per-fragment branch on every tile, rows and columns from the persistent tile map); with a forced v2 tile too
    # (plan_v4 runs after plan_v2 accepted the launch, so the code must not change the mask)
    (0, 2, 192, 384, 64, 1), (33, 2, 192, 384, 64, 1),
    # three stacked segments: N in row * N + col is nseg * seg_n, not seg_n
    (0, 0, 96, 128, 64, 3), (-1, 0, 96, 128, 64, 3), (0, 2, 96, 128, 64, 3),
]


@pytest.fixture
def gemm_knobs():
    """Sets (tile code, persistent mode, gemm mode) for one test and restores all three."""
    from vilbert import _native
    prev_tile, prev_v4 = _native.set_gemm_tile(0), _native.set_gemm_v4(1)
    _native.set_gemm_tile(prev_tile)
    _native.set_gemm_v4(prev_v4)
    prev_mode = _native.set_gemm_mode("f32")
    _native.set_gemm_mode(prev_mode)

    def use(code, v4, mode):
        _native.set_gemm_tile(code)
        _native.set_gemm_v4(v4)
        _native.set_gemm_mode(mode)
    try:
        yield use
    finally:
        _native.set_gemm_tile(prev_tile)
        _native.set_gemm_v4(prev_v4)
        _native.set_gemm_mode(prev_mode)


def _linear_checks(ops, M, seg_n, K, nseg, p, mode):
    N = nseg * seg_n
    keep = _keep(DR.linear_index(M, N), SEED, p)
    x = _rand(M, K, seed=1)
    # pattern: W = 0, bias = 1, residual = 0 -> drop_scale or 0
    zw = [torch.zeros(seg_n, K, device=DEV) for _ in range(nseg)]
    ones = [torch.ones(seg_n, device=DEV) for _ in range(nseg)]
    y, _ = ops.linear_fwd(x.to(DEV), zw, ones, residual=torch.zeros(M, N, device=DEV), drop_p=p, seed=SEED)
    _assert_pattern(y, keep, _scale(p), what="linear %dx%dx%d" % (M, N, K))
    # numeric
    ws = [_rand(seg_n, K, seed=10 + s, scale=0.1) for s in range(nseg)]
    bs = [_rand(seg_n, seed=20 + s) for s in range(nseg)]
    r = _rand(M, N, seed=3)
    y, _ = ops.linear_fwd(x.to(DEV), [w.to(DEV) for w in ws], [b.to(DEV) for b in bs], residual=r.to(DEV), drop_p=p, seed=SEED)
    if mode == "fp8":
        from oracle import fp8_oracle as F
        pre = torch.from_numpy(np.asarray(F.linear_fp8(x.numpy(), ws[0].numpy(), bs[0].numpy()))).double()
    else:
        pre = torch.cat([x.double() @ w.double().t() + b.double() for w, b in zip(ws, bs)], 1)
    want = torch.where(keep, pre * _scale(p), torch.zeros_like(pre)) + r.double()
    got = y.cpu().double()
    assert torch.isfinite(got).all()
    err = (got - want).abs()
    if mode == "f32":        # tests/test_kernels_gpu.py test_linear_forward_dgrad_wgrad_every_tile: element-wise 3e-5 + 3e-5 |want|
        assert (err <= 3e-5 + 3e-5 * want.abs()).all(), "max err %.3e" % err.max().item()
    else:                    # tests/test_gemm_modes_gpu.py (bf16x6: 3e-5 of the range), tests/test_fp8_gpu.py's epilogue test (2e-5)
        tol = 3e-5 if mode == "bf16x6" else 2e-5
        assert err.max().item() <= tol * max(1.0, want.abs().max().item()), "max err %.3e (mode %s)" % (err.max().item(), mode)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("code,v4,M,seg_n,K,nseg", LINEAR_CASES)
def test_linear_epilogue_fp32(ops, gemm_knobs, code, v4, M, seg_n, K, nseg, p):
    gemm_knobs(code, v4, "f32")
    _linear_checks(ops, M, seg_n, K, nseg, p, "f32")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("M,seg_n,K,nseg", [(192, 384, 64, 1), (100, 200, 52, 1), (96, 128, 64, 3)])
def test_linear_epilogue_bf16x6(ops, gemm_knobs, M, seg_n, K, nseg, p):
    """The bf16-planes kernels (gemm_planes.hip) end in gemm_core.h's tile_epilogue: both of its forms."""
    gemm_knobs(0, 1, "bf16x6")
    _linear_checks(ops, M, seg_n, K, nseg, p, "bf16x6")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("M,N,K", [(192, 384, 128), (100, 200, 128)])
def test_linear_epilogue_fp8(ops, gemm_knobs, M, N, K, p):
    """fp8.hip's row-scaled epilogue (MODE 0); K a multiple of 128 keeps the launch on the fp8 kernel."""
    gemm_knobs(0, 1, "fp8")
    assert ops._fp8_eligible(torch.empty(1, device=DEV), K, N, None)
    _linear_checks(ops, M, N, K, 1, p, "fp8")


# ---------------------------------------------------------------------------------------------------------------------
# bf16 linear, HB_DROPRES: index m * N + n
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("M,N,K", [(300, 384, 64), (1024, 1024, 64), (4352, 1024, 64), (5120, 1024, 64), (8448, 1024, 64),
                                   (1, 256, 128)])      # the branches of the tile map (tests/test_bf16_stream_gpu.py) + one row
def test_linear16_dropres(M, N, K, p):
    from vilbert import ops16
    keep = _keep(DR.linear_index(M, N), SEED, p)
    x = _rand(M, K, seed=1).to(BF16)
    y, _ = ops16.linear_fwd(x.to(DEV), [torch.zeros(N, K, device=DEV)], [torch.ones(N, device=DEV)], None,
                            torch.zeros(M, N, dtype=BF16, device=DEV), drop_p=p, seed=SEED)
    survivor = float(torch.tensor(_scale(p), dtype=torch.float32).to(BF16))
    _assert_pattern(y.float(), keep, survivor, what="bf16 linear %dx%dx%d" % (M, N, K))
    w, b, r = _rand(N, K, seed=2, scale=0.05), _rand(N, seed=3), _rand(M, N, seed=4).to(BF16)
    y, _ = ops16.linear_fwd(x.to(DEV), [w.to(DEV)], [b.to(DEV)], None, r.to(DEV), drop_p=p, seed=SEED)
    w16 = w.to(BF16).double()
    pre = x.double() @ w16.t() + b.double()
    mag = (x.double().abs() @ w16.abs().t() + 1.0) * _scale(p)        # (the accumulation error is scaled with the value)
    helpers.close16(y, torch.where(keep, pre * _scale(p), torch.zeros_like(pre)) + r.double(), mag, "bf16 dropout + residual")


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward twin: index row * n_cols + col
# ---------------------------------------------------------------------------------------------------------------------
def _ln_inputs(rows, cols, dtype):
    x = (_rand(rows, cols, seed=rows, scale=2.0) + 0.3).to(dtype)
    dy = _rand(rows, cols, seed=rows + 1).to(dtype)
    g, b = 1 + 0.1 * _rand(cols, seed=3), 0.1 * _rand(cols, seed=4)
    ref = helpers.layernorm16_reference(x, dy, g, b, 1e-12)
    mean, rstd = ref["mean"].float().to(DEV), (1.0 / torch.sqrt(ref["var"] + 1e-12)).float().to(DEV)
    return x, dy, g, ref, mean, rstd


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("rows,cols", [(5, 64), (37, 768), (9, 1024), (6, 5000)])
def test_layernorm_backward_twin_fp32(ops, rows, cols, p):
    x, dy, g, ref, mean, rstd = _ln_inputs(rows, cols, torch.float32)
    keep = _keep(DR.layernorm_index(rows, cols), SEED, p)
    res = ops.layernorm_bwd(dy.to(DEV), x.to(DEV), mean, rstd, g.to(DEV), drop=(p, SEED))
    dx = res[0]
    if cols <= 4096:
        assert len(res) == 4
        dxd = res[3]
    else:
        # rows wider than 4096 columns: vb_layernorm_bwd_drop does not offer the twin (VB_E_RANGE) and the launcher returns none;
        # the dense layer's backward then runs vb_dropout over dx - the two-launch form, held to the same mask
        assert len(res) == 3
        dxd = ops.dropout(dx, p, SEED)
    _close(dx, ref["dx"])
    dxc, dxdc = dx.cpu(), dxd.cpu()
    assert torch.equal(dxdc != 0, keep & (dxc != 0)) and bool((dxc != 0).all())
    assert torch.equal(dxdc, torch.where(keep, dxc * torch.tensor(_scale(p), dtype=torch.float32), torch.zeros_like(dxc)))
    _close(dxd, torch.where(keep, ref["dx"] * _scale(p), torch.zeros_like(ref["dx"])))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("rows,cols", [(5, 256), (37, 768), (4101, 64)])
def test_layernorm_backward_twin_bf16(rows, cols, p):
    from vilbert import ops16
    x, dy, g, ref, mean, rstd = _ln_inputs(rows, cols, BF16)
    keep = _keep(DR.layernorm_index(rows, cols), SEED, p)
    dx, _, _, dxd = ops16.layernorm_bwd(dy.to(DEV), x.to(DEV), mean, rstd, g.to(DEV), drop=(p, SEED))
    want = ref["dx"]
    mag = torch.ones(rows, cols, dtype=torch.float64) * float(want.abs().max()) * 4      # (tests/test_bf16_stream_gpu.py's)
    helpers.close16(dx, want, mag, "LayerNorm backward dx")
    assert torch.equal(dxd.cpu() != 0, keep & (dx.cpu() != 0))
    helpers.close16(dxd, torch.where(keep, want * _scale(p), torch.zeros_like(want)), mag * _scale(p), "dx under the dropout mask")


# ---------------------------------------------------------------------------------------------------------------------
# attention: index ((b * heads + h) * n_q + q) * n_k + key, n_k the launch's own key count
# ---------------------------------------------------------------------------------------------------------------------
B_ATT, HEADS = 2, 3
SINGLE_LAUNCH = [
    pytest.param(128, 36, 37, id="lds_fwd+fused_lds_bwd_over_v"),       # attn_q_lds_kernel<false>, attn_bwd_fused_lds_kernel (Pd | dS over V)
    pytest.param(32, 17, 40, id="lds_fwd+fused_lds_bwd_own_block"),     # ... with over_v false (Pd | dS behind the operands)
    pytest.param(64, 50, 40, id="generic_nt3"),                         # attn_q_kernel<D, 3, *>, attn_bwd_kv_kernel
    pytest.param(64, 50, 101, id="generic_nt8"),                        # attn_q_kernel<D, 8, *>
    pytest.param(128, 20, 300, id="generic_nt20"),                      # attn_q_kernel<D, 20, *>
]
CHUNKED = [
    pytest.param(64, 20, 702, id="chunked_3x234"),      # generic kernels with VB_DVEC_ACCUMULATE / VB_DVEC_GIVEN, three equal chunks
    pytest.param(64, 20, 330, id="chunked_165+165"),
]


def _attention_keep(ops, Sq, Sk, p, seed):
    """Host mask [B, heads, Sq, Sk]; more than MAX_KEYS keys: chunk c's own index space and seed."""
    if Sk <= ops.MAX_KEYS:
        return _keep(DR.attention_index(B_ATT, HEADS, Sq, Sk), seed, p)
    return torch.cat([_keep(DR.attention_index(B_ATT, HEADS, Sq, c1 - c0), ops._chunk_seed(seed, c), p)
                      for c, (c0, c1) in enumerate(ops._key_chunks(Sk))], dim=-1)


def _identity_v_probs(fwd, d, Sq, Sk, dtype):
    """The dropped probability matrix [B, heads, Sq, Sk] read through the context: Q = K = 0 (uniform softmax) and
    V[key, h * d + col] = 1 where key == col + j * d, one forward per j - the context of pass j IS columns j d .. of the matrix."""
    H = HEADS * d
    q = torch.zeros(B_ATT, Sq, H, dtype=dtype, device=DEV)
    k = torch.zeros(B_ATT, Sk, H, dtype=dtype, device=DEV)
    cols = []
    for j in range((Sk + d - 1) // d):
        v = torch.zeros(B_ATT, Sk, HEADS, d, dtype=dtype)
        n = min(d, Sk - j * d)
        v[:, j * d + torch.arange(n), :, torch.arange(n)] = 1
        ctx = fwd(q, k, v.reshape(B_ATT, Sk, H).to(DEV))
        cols.append(ctx.float().cpu().reshape(B_ATT, Sq, HEADS, d).permute(0, 2, 1, 3)[..., :n])
    return torch.cat(cols, dim=-1)


def _masks(Sk):
    """Additive key masks [B, Sk]: a prefix on sample 0, holes on sample 1."""
    valid = torch.ones(B_ATT, Sk)
    valid[0, max(1, (2 * Sk) // 3):] = 0
    valid[1, 1::3] = 0
    return (1.0 - valid) * -10000.0


def _attn_ref(q, k, v, madd, keep, p):
    """float64 statement of vilbert.py:429-449 with the given keep mask."""
    d = q.shape[-1] // HEADS
    sp = lambda t: t.view(t.shape[0], t.shape[1], HEADS, d).permute(0, 2, 1, 3)
    s = sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(d) + madd.view(B_ATT, 1, 1, -1)
    pr = torch.softmax(s, -1) * keep.double() * _scale(p)
    return (pr @ sp(v)).permute(0, 2, 1, 3).reshape(q.shape)


def _attention_numeric_fp32(ops, d, Sq, Sk, p, seed, keep):
    H = HEADS * d
    g = torch.Generator().manual_seed(Sq * 1000 + Sk)
    q, k, v = (torch.randn(B_ATT, n, H, generator=g) * 0.5 for n in (Sq, Sk, Sk))
    d_out = torch.randn(B_ATT, Sq, H, generator=g)
    madd = _masks(Sk)
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    ref = _attn_ref(q64, k64, v64, madd.double(), keep, p)
    ref.backward(d_out.double())
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    with torch.no_grad():
        out, _, lse = ops.attention_fwd(qd, kd, vd, madd.to(DEV), HEADS, False, True, p, seed)
        dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
        ops.attention_bwd(d_out.to(DEV), qd, kd, vd, madd.to(DEV), HEADS, lse, dq, dk, dv, p, seed)
    _close(out, ref.detach())
    _close(dq, q64.grad)
    _close(dk, k64.grad)
    _close(dv, v64.grad)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("d,Sq,Sk", SINGLE_LAUNCH + CHUNKED)
def test_attention_fp32(ops, d, Sq, Sk, p):
    keep = _attention_keep(ops, Sq, Sk, p, SEED)
    survivor = _scale(p) / Sk
    H = HEADS * d
    if Sk <= ops.MAX_KEYS:
        zq, zk = torch.zeros(B_ATT, Sq, H, device=DEV), torch.zeros(B_ATT, Sk, H, device=DEV)
        probs = ops.attention_fwd(zq, zk, torch.zeros(B_ATT, Sk, H, device=DEV), None, HEADS, True, False, p, SEED)[1]
        _assert_pattern(probs, keep, survivor, rtol=1e-5, what="probs")
    with torch.no_grad():
        got = _identity_v_probs(lambda q, k, v: ops.attention_fwd(q, k, v, None, HEADS, False, False, p, SEED)[0], d, Sq, Sk,
                                torch.float32)
    _assert_pattern(got, keep, survivor, rtol=1e-5, what="context of the identity V")
    _attention_numeric_fp32(ops, d, Sq, Sk, p, SEED, keep)


def _attention_numeric_bf16(d, Sq, Sk, p, seed, keep):
    from vilbert import ops16
    H = HEADS * d
    g = torch.Generator().manual_seed(Sq * 1000 + Sk)
    q, k, v = ((torch.randn(B_ATT, n, H, generator=g) * 0.7).to(BF16) for n in (Sq, Sk, Sk))
    d_out = torch.randn(B_ATT, Sq, H, generator=g).to(BF16)
    madd = _masks(Sk)
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    ref = _attn_ref(q64, k64, v64, madd.double(), keep, p)
    ref.backward(d_out.double())
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    out, lse = ops16.attention_fwd(qd, kd, vd, madd.to(DEV), HEADS, True, p, seed)
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    ops16.attention_bwd(d_out.to(DEV), qd, kd, vd, madd.to(DEV), HEADS, lse, dq, dk, dv, p, seed)
    for got, want, nm in ((out, ref.detach(), "context"), (dq, q64.grad, "dq"), (dk, k64.grad, "dk"), (dv, v64.grad, "dv")):
        got = got.cpu().double()
        assert got.dtype == torch.float64 and torch.isfinite(got).all(), nm
        l2 = float((got - want).norm() / want.norm().clamp_min(1e-30))
        mx = float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))
        # test_attention16_matches_the_fp32_kernels_on_the_same_values' bounds
        assert l2 <= 1.5e-2 and mx <= 2.0 ** -6, "%s: relative L2 %.3e, max error %.3e of the range" % (nm, l2, mx)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("d,Sq,Sk", SINGLE_LAUNCH)
def test_attention_bf16(d, Sq, Sk, p):
    from vilbert import ops, ops16
    keep = _attention_keep(ops, Sq, Sk, p, SEED)
    got = _identity_v_probs(lambda q, k, v: ops16.attention_fwd(q, k, v, None, HEADS, False, p, SEED)[0], d, Sq, Sk, BF16)
    # 1 / Sk * drop_scale goes through two bf16 roundings (the probability, the context): 2^-8 each at the most
    _assert_pattern(got, keep, _scale(p) / Sk, rtol=2.0 ** -7, what="bf16 context of the identity V")
    _attention_numeric_bf16(d, Sq, Sk, p, SEED, keep)


def _two_kernel_lds_backward():
    """Body of the child process (VB_ATTN_FUSED_BWD=0): attn_q_lds_kernel<BWD> + attn_bwd_kv_lds_kernel, both builds."""
    from vilbert import ops
    for d, Sq, Sk in ((128, 36, 37), (32, 17, 40)):
        for p in PS:
            keep = _attention_keep(ops, Sq, Sk, p, SEED)
            _attention_numeric_fp32(ops, d, Sq, Sk, p, SEED, keep)
            _attention_numeric_bf16(d, Sq, Sk, p, SEED, keep)
    print("two-kernel LDS backward: ok")


def test_attention_two_kernel_lds_backward_in_a_child_process():
    """VB_ATTN_FUSED_BWD is read once per process, so the two-kernel LDS backward gets a process of its own: this file run as a
    script with the variable set. The child has its own time limit; its exit status and its last line are checked."""
    env = dict(os.environ, VB_ATTN_FUSED_BWD="0")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "two-kernel-lds-backward"], env=env, timeout=240,
                          capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip().endswith("two-kernel LDS backward: ok"), \
        "exit status %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])


# ---------------------------------------------------------------------------------------------------------------------
# the device step counter: seed + *counter * 0xD1B54A32D192ED03, mixed in inside the kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epoch", [1, 5])
def test_device_step_counter(ops, epoch):
    from vilbert import _native as N
    from vilbert import graphed, ops16
    p = 0.5
    seed_e = DR.seed_with_epoch(SEED, epoch)
    counter = torch.tensor([epoch], dtype=torch.int64, device=DEV)      # one 64-bit word: the uint64 the kernels read
    before = graphed._ACTIVE["epoch_ptr"]                              # a GraphedTrainStep that is still alive, if any
    N.check(N.lib().vb_set_seed_epoch(counter.data_ptr()), "vb_set_seed_epoch")
    try:
        # vb_dropout
        n = 1023
        y = ops.dropout(torch.ones(n, device=DEV), p, SEED).cpu()
        keep0, keep = _keep(DR.flat_index(n), SEED, p), _keep(DR.flat_index(n), seed_e, p)
        assert not torch.equal(keep, keep0)
        _assert_pattern(y, keep, _scale(p), what="vb_dropout under the step counter")
        # one fp32 linear epilogue
        M, Nn, K = 192, 384, 64
        y, _ = ops.linear_fwd(_rand(M, K, seed=1).to(DEV), [torch.zeros(Nn, K, device=DEV)], [torch.ones(Nn, device=DEV)],
                              residual=torch.zeros(M, Nn, device=DEV), drop_p=p, seed=SEED)
        keep0, keep = _keep(DR.linear_index(M, Nn), SEED, p), _keep(DR.linear_index(M, Nn), seed_e, p)
        assert not torch.equal(keep, keep0)
        _assert_pattern(y, keep, _scale(p), what="linear epilogue under the step counter")
        # fp32 attention, forward (probabilities) and backward (against float64 with the host mask of this step)
        d, Sq, Sk = 32, 17, 40
        H = HEADS * d
        keep0, keep = _attention_keep(ops, Sq, Sk, p, SEED), _attention_keep(ops, Sq, Sk, p, seed_e)
        assert not torch.equal(keep, keep0)
        z = torch.zeros(B_ATT, Sq, H, device=DEV), torch.zeros(B_ATT, Sk, H, device=DEV), torch.zeros(B_ATT, Sk, H, device=DEV)
        _assert_pattern(ops.attention_fwd(*z, None, HEADS, True, False, p, SEED)[1], keep, _scale(p) / Sk, rtol=1e-5,
                        what="probs under the step counter")
        _attention_numeric_fp32(ops, d, Sq, Sk, p, SEED, keep)
        _attention_numeric_fp32(ops, 64, 50, 40, p, SEED, _attention_keep(ops, 50, 40, p, seed_e))       # (generic kernels)
        # bf16 attention forward
        got = _identity_v_probs(lambda q, k, v: ops16.attention_fwd(q, k, v, None, HEADS, False, p, SEED)[0], d, Sq, Sk, BF16)
        _assert_pattern(got, keep, _scale(p) / Sk, rtol=2.0 ** -7, what="bf16 context under the step counter")
        torch.cuda.synchronize()
    finally:
        N.lib().vb_set_seed_epoch(before)
    # unregistered again (nothing else had a counter registered): the plain seed
    if before is None:
        _assert_pattern(ops.dropout(torch.ones(1023, device=DEV), p, SEED).cpu(), _keep(DR.flat_index(1023), SEED, p), _scale(p))


if __name__ == "__main__":
    assert sys.argv[1:] == ["two-kernel-lds-backward"] and os.environ.get("VB_ATTN_FUSED_BWD") == "0"
    _two_kernel_lds_backward()
