"""The fp32 row kernels called directly through the C ABI: LayerNorm forward / backward (csrc/layernorm.hip, fp32 entries), the
embedding forwards and the additive mask (embed.hip), the cross-entropy and KL losses (loss.hip), activation backward and dropout
(elementwise.hip). The fp32 stream is the parity mode every other mode is judged against; through vilbert.ops these kernels only
ever see contiguous tensors, fresh scratch and the model's constants.

Rules of this file (those of tests/test_bf16_helpers_gpu.py):
  * the C entry points are called through vilbert._native.lib() with raw pointers (strides, offsets, optional outputs);
  * references are float64 on the CPU from the same fp32 values;
  * every output, scratch AND input buffer lies between two canary margins (bytes 0x5A, as fp32 1.5e16): the margins of outputs
    and scratch are checked afterwards, a read past an input shows in the result; where a kernel writes a rectangle inside a
    larger buffer, the padding must still hold the canary;
  * a call that returns an error leaves every output byte untouched;
  * tolerances are the ones the wrapper-level tests already use (tests/test_kernels_gpu.py, test_backward_gpu.py), or are derived
    in tests/row_kernel_bounds.py, where tests/test_row_kernels_tolerances.py shows on the CPU what each of them rejects.

What the wrapper-level tests could not see, and the test here that does (profiles/row_kernels_abi_gpu_tests.txt: the GPU run and
the one-line kernel mutations each of these catches):
  eps dropped / outside the root            test_layernorm_forward_eps_is_inside_the_root
  one-pass variance                         test_layernorm_forward_large_offset_needs_the_two_pass_variance
  mean / rstd / presum of the embeddings,   test_text_embedding_statistics_presum_position_offset_and_task_row,
  pos_offset, the task-row mapping          test_image_embedding_four_outputs_and_four_byte_aligned_location_operands
  zero partial of a rowless wave, > 16      test_layernorm_backward_every_reduce_path_on_a_nan_workspace
  partials on every reduce path
  swish backward, GELU tails                test_activation_derivative_over_a_sweep_with_the_tails,
                                            test_activation_values_through_the_gemm_epilogue
  grid-stride loops                         test_activation_backward_grid_stride_loop_wraps,
                                            test_dropout_grid_stride_loop_wraps_and_the_tail
  device-side KL divisor, loss[1], strides  test_kl_divergence_host_and_device_divisor_on_padded_rows
  ldd != ld, a common shift of the logits   test_cross_entropy_on_padded_rows_with_a_separate_gradient_stride,
                                            test_cross_entropy_does_not_depend_on_a_common_shift_of_the_logits
  error returns                             test_error_returns_leave_every_output_untouched
"""
import ctypes

import numpy as np
import pytest
import torch

import dropout_restatement as DR
import row_kernel_bounds as RB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I64 = torch.float32, torch.int64
E_BADARG, E_ALIGN, E_RANGE = -1, -2, -3
CANARY, CANARY32 = 0x5A, 0x5A5A5A5A
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SWISH = 0, 1, 2, 3
ACTS = {"gelu": ACT_GELU, "relu": ACT_RELU, "swish": ACT_SWISH}
SEED = 0xC0FFEE1234567891          # top bit set
NAN = float("nan")
U = RB.U


def _N():
    from vilbert import _native
    return _native


def _lib():
    return _N().lib()


def _st():
    return _N().stream_ptr()


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


class Guard:
    """n elements of `dtype` on the device between two canary margins; the payload starts as canary bytes too
    (tests/test_bf16_helpers_gpu.py's, with fp32 / int64 readers)."""
    MARGIN = 512

    def __init__(self, n, dtype=F32):
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((2 * self.MARGIN + self.nbytes,), CANARY, dtype=torch.uint8, device=DEV)
        self.t = self.buf[self.MARGIN:self.MARGIN + self.nbytes].view(dtype)
        assert self.t.data_ptr() % 16 == 0

    @classmethod
    def of(cls, tensor):
        """A guarded copy of a CPU tensor (inputs: what lies past the last element is canary, not a neighbour's data)."""
        g = cls(tensor.numel(), tensor.dtype)
        g.t.copy_(tensor.reshape(-1))
        return g

    @classmethod
    def filled(cls, n, value):
        g = cls(n, F32)
        g.t.fill_(value)
        return g

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        torch.cuda.synchronize()
        m = self.MARGIN
        assert bool((self.buf[:m] == CANARY).all()) and bool((self.buf[m + self.nbytes:] == CANARY).all()), \
            "%s: wrote outside its buffer" % what

    def untouched(self, what):
        self.check(what)
        assert bool((self.buf == CANARY).all()), "%s: wrote although it returned an error" % what

    def cpu(self, what):
        self.check(what)
        return self.t.cpu()

    def u32(self, what):
        self.check(what)
        return self.t.view(torch.int32).cpu().numpy().view(np.uint32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _close(got, want64, rtol=2e-5, atol=2e-5, what=""):
    """tests/test_kernels_gpu.py's bar."""
    got = got.double()
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    assert torch.isfinite(got).all(), what
    err = (got - want64).abs()
    assert (err <= atol + rtol * want64.abs()).all(), "%s: max err %.3e (max |ref| %.3e)" % (
        what, err.max().item(), want64.abs().max().item())


def _within(got, want64, tol64, what):
    got = got.double()
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    assert torch.isfinite(got).all(), what
    err = (got - want64).abs()
    assert (err <= tol64).all(), "%s: worst err / tol %.3f (max err %.3e)" % (
        what, float((err / tol64.clamp(min=1e-300)).max()), float(err.max()))
    return float(err.max())


@pytest.fixture
def plain_seed():
    """No device step counter mixed into the dropout seeds for the duration of a test (vb_set_seed_epoch)."""
    from vilbert import graphed
    before = graphed._ACTIVE["epoch_ptr"]
    _lib().vb_set_seed_epoch(None)
    yield
    _lib().vb_set_seed_epoch(before)


# ---------------------------------------------------------------------------------------------------------------------
# 1. vb_layernorm_fwd
# ---------------------------------------------------------------------------------------------------------------------
def _ln_fwd(x, x2, g, b, eps, want_mean=True, want_rstd=True):
    """One vb_layernorm_fwd launch on guarded buffers: (y [rows, cols], mean or None, rstd or None) on the CPU."""
    rows, cols = x.shape
    xd, gd, bd = Guard.of(x), Guard.of(g), Guard.of(b)
    x2d = Guard.of(x2) if x2 is not None else None
    y = Guard(rows * cols)
    mean = Guard(rows) if want_mean else None
    rstd = Guard(rows) if want_rstd else None
    rc = _lib().vb_layernorm_fwd(_st(), rows, cols, xd.ptr, x2d.ptr if x2d else None, gd.ptr, bd.ptr, eps, y.ptr,
                                 mean.ptr if mean else None, rstd.ptr if rstd else None)
    assert rc == 0, rc
    what = "vb_layernorm_fwd %dx%d" % (rows, cols)
    return (y.cpu(what).view(rows, cols), mean.cpu(what) if mean else None, rstd.cpu(what) if rstd else None)


def _ln_params(cols, seed):
    return 1 + 0.1 * _rand(cols, seed=seed), 0.1 * _rand(cols, seed=seed + 1)


LN_FWD_SHAPES = [(1, 4), (3, 252), (5, 260), (6, 1024), (6, 1028), (4, 4096), (3, 4100), (2, 8192), (4101, 64)]


@pytest.mark.parametrize("rows,cols", LN_FWD_SHAPES)
def test_layernorm_forward_shapes_x2_and_the_four_statistics_combinations(rows, cols):
    x, x2 = _rand(rows, cols, seed=1, scale=3.0) + 0.7, _rand(rows, cols, seed=2)
    g, b = _ln_params(cols, 3)
    seen = {}
    for with_x2, want_mean, want_rstd in [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]:
        y, mean, rstd = _ln_fwd(x, x2 if with_x2 else None, g, b, 1e-12, want_mean, want_rstd)
        ref = RB.ln64(x.double() + x2.double() if with_x2 else x, g, b, 1e-12)
        what = "%dx%d x2=%s" % (rows, cols, with_x2)
        _close(y, ref["y"], what=what + " y")
        if mean is not None:
            _close(mean, ref["mean"], what=what + " mean")
        if rstd is not None:
            _close(rstd, ref["rstd"], 1e-5, 1e-6, what=what + " rstd")
        # which statistics are asked for must not change the row
        if with_x2 in seen:
            assert torch.equal(_bits(seen[with_x2]), _bits(y)), what
        seen[with_x2] = y


@pytest.mark.parametrize("eps", [1e-12, 1e-5, 1e-1])
@pytest.mark.parametrize("rows,cols", [(5, 260), (6, 1028), (3, 4100)])
def test_layernorm_forward_eps_is_inside_the_root(rows, cols, eps):
    # variance about 1e-6: eps = 1e-5 and 1e-1 dominate it. Bound: row_kernel_bounds (the mean error of rows around 0.5 times
    # rstd up to 1000 is above the ordinary 2e-5 bar); "eps ignored" / "eps outside the root" miss it by > 10,000 times
    # at eps = 1e-5 (tests/test_row_kernels_tolerances.py)
    x, g, b = RB.ln_small_variance_rows(rows, cols, seed=cols)
    ref = RB.ln64(x, g, b, eps)
    mean_tol, y_tol = RB.ln_offset_tolerances(x, g, ref)
    y, mean, rstd = _ln_fwd(x, None, g, b, eps)
    _within(y, ref["y"], y_tol, "eps %g y" % eps)
    _within(mean, ref["mean"], mean_tol, "eps %g mean" % eps)
    _close(rstd, ref["rstd"], 1e-5, 1e-6, what="eps %g rstd" % eps)


@pytest.mark.parametrize("cols", [64, 768, 1024, 4096, 8192])
def test_layernorm_forward_large_offset_needs_the_two_pass_variance(cols):
    # mean 1000, standard deviation 1: E[x^2] - E[x]^2 in fp32 is wrong by 0.2 .. 0.4 here (> 100 times the bound)
    x, g, b = RB.ln_offset_rows(RB.OFFSET_ROWS, cols, seed=cols)
    ref = RB.ln64(x, g, b, 1e-12)
    mean_tol, y_tol = RB.ln_offset_tolerances(x, g, ref)
    y, mean, rstd = _ln_fwd(x, None, g, b, 1e-12)
    err_y = (y.double() - ref["y"]).abs()
    err_m = (mean.double() - ref["mean"]).abs()
    print("LayerNorm large offset, %4d columns: y max err %.3e (bound %.3e, worst err / bound %.3f), mean max err %.3e "
          "(bound %.3e)" % (cols, err_y.max(), y_tol.max(), (err_y / y_tol).max(), err_m.max(), mean_tol.min()))
    _within(y, ref["y"], y_tol, "y")
    _within(mean, ref["mean"], mean_tol, "mean")
    _close(rstd, ref["rstd"], 1e-5, 1e-6, what="rstd")


@pytest.mark.parametrize("cols", [64, 1028])
def test_layernorm_forward_constant_row_is_finite_and_exactly_zero(cols):
    x = torch.full((3, cols), 2.5)
    x[1] = -1000.25
    g, _ = _ln_params(cols, 5)
    y, mean, rstd = _ln_fwd(x, None, g, torch.zeros(cols), 1e-12)
    assert torch.isfinite(y).all() and torch.isfinite(rstd).all()
    assert float(y.abs().max()) == 0.0
    assert torch.equal(mean, x[:, 0])
    _close(rstd, torch.full((3,), 1e6, dtype=torch.float64), 1e-5, 0, what="rstd = 1 / sqrt(eps)")


def test_layernorm_forward_a_non_finite_value_poisons_its_row_only():
    rows, cols = 8, 260                                   # two blocks of four rows
    x = _rand(rows, cols, seed=11)
    g, b = _ln_params(cols, 12)
    clean = _ln_fwd(x, None, g, b, 1e-12)
    bad = x.clone()
    bad[1, 5], bad[6, 259] = float("inf"), NAN
    got = _ln_fwd(bad, None, g, b, 1e-12)
    keep = [0, 2, 3, 4, 5, 7]
    for c, p in zip(clean, got):
        assert torch.equal(_bits(c[keep]), _bits(p[keep])), "a neighbouring row changed"
    assert torch.isnan(got[0][[1, 6]]).all()
    assert not torch.isfinite(got[1][[1, 6]]).any() and torch.isnan(got[2][[1, 6]]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. vb_layernorm_bwd, vb_layernorm_bwd_drop
# ---------------------------------------------------------------------------------------------------------------------
def _ln_bwd(x, dy, mean, rstd, g, drop=None):
    """One backward launch; workspace of exactly vb_layernorm_bwd_workspace floats, NaN-filled like dgamma / dbeta.
    drop = (p, seed): vb_layernorm_bwd_drop. CPU tensors dx, dgamma, dbeta (, dx_dropped)."""
    rows, cols = x.shape
    lib = _lib()
    ws_n = lib.vb_layernorm_bwd_workspace(rows, cols)
    assert ws_n >= 2 * cols
    ins = [Guard.of(t) for t in (dy, x, mean, rstd, g)]
    dx, dg, db, ws = Guard(rows * cols), Guard.filled(cols, NAN), Guard.filled(cols, NAN), Guard.filled(ws_n, NAN)
    head = [_st(), rows, cols] + [i.ptr for i in ins] + [dx.ptr, dg.ptr, db.ptr, ws.ptr]
    what = "vb_layernorm_bwd %dx%d" % (rows, cols)
    if drop is None:
        assert lib.vb_layernorm_bwd(*head) == 0
        dxd = None
    else:
        dxd = Guard(rows * cols)
        assert lib.vb_layernorm_bwd_drop(*(head + [dxd.ptr, drop[0], drop[1]])) == 0
    ws.check(what + " workspace")
    out = [dx.cpu(what).view(rows, cols), dg.cpu(what), db.cpu(what)]
    return out + ([dxd.cpu(what).view(rows, cols)] if dxd is not None else [])


LN_BWD_SHAPES = [(1, 4), (17, 64), (300, 768), (70, 1028), (70, 4096), (19, 4100), (19, 8192),      # > 16 partials on each path
                 (1, 768), (15, 768), (16, 768), (17, 768)]                                         # blocks end at row 16


@pytest.mark.parametrize("rows,cols", LN_BWD_SHAPES)
def test_layernorm_backward_every_reduce_path_on_a_nan_workspace(rows, cols, plain_seed):
    x, dy = _rand(rows, cols, seed=1, scale=2.0) + 0.3, _rand(rows, cols, seed=2)
    g, b = _ln_params(cols, 3)
    fwd = RB.ln64(x, g, b, 1e-12)
    mean, rstd = fwd["mean"].float(), fwd["rstd"].float()
    ref = RB.ln_backward64(x, dy, g, 1e-12)
    dx, dg, db = _ln_bwd(x, dy, mean, rstd, g)
    # dx: tests/test_backward_gpu.py::test_layernorm_backward's bar
    scale = max(1.0, float(ref["dx"].abs().max()))
    assert torch.isfinite(dx).all()
    assert float((dx.double() - ref["dx"]).abs().max()) <= 6e-5 * scale
    # column sums: fp32 accumulation, 3e-6 sum|terms| + 1e-6 (helpers.close16's accumulation form)
    _within(dg, ref["dgamma"], 3e-6 * ref["dgamma_mag"] + 1e-6, "dgamma")
    _within(db, ref["dbeta"], 3e-6 * ref["dbeta_mag"] + 1e-6, "dbeta")
    again = _ln_bwd(x, dy, mean, rstd, g)
    for a, c in zip((dx, dg, db), again):
        assert torch.equal(_bits(a), _bits(c)), "two calls differ"
    if cols > 4096:
        return
    for p in (0.1, 0.5):
        dx2, dg2, db2, dxd = _ln_bwd(x, dy, mean, rstd, g, drop=(p, SEED))
        for a, c in zip((dx, dg, db), (dx2, dg2, db2)):
            assert torch.equal(_bits(a), _bits(c)), "the twin changed the plain results"
        keep = torch.from_numpy(DR.keep(SEED, DR.layernorm_index(rows, cols), p))
        want = torch.where(keep, dx * torch.tensor(DR.drop_scale(p)), torch.zeros_like(dx))
        assert torch.equal(dxd, want), "dx_dropped is not keep ? dx / (1 - p) : 0 of the host mask (p = %g)" % p
        assert bool(((dxd == 0) | keep).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3. embeddings
# ---------------------------------------------------------------------------------------------------------------------
V, N_TYPES, N_TASKS = 11, 2, 3


def _text_embed(ids, seg, pos_offset, word, pos, typ, task_ids, temb, g, b, eps=1e-12, n_types=None):
    """One vb_text_embed_ln_fwd launch; every table in a guarded buffer of exactly its size, the outputs guarded at exactly
    batch * n_out rows. CPU tensors out, mean, rstd, presum."""
    batch, n_tok = ids.shape
    hidden = word.shape[1]
    n_out = n_tok + (1 if task_ids is not None else 0)
    tabs = [Guard.of(t) for t in (ids, seg, word, pos, typ, g, b)]
    tk = Guard.of(task_ids) if task_ids is not None else None
    te = Guard.of(temb) if temb is not None else None
    out, presum = Guard(batch * n_out * hidden), Guard(batch * n_out * hidden)
    mean, rstd = Guard(batch * n_out), Guard(batch * n_out)
    rc = _lib().vb_text_embed_ln_fwd(_st(), batch, n_tok, hidden, word.shape[0], n_types or typ.shape[0],
                                     temb.shape[0] if temb is not None else 0, tabs[0].ptr, tabs[1].ptr, pos_offset,
                                     tabs[2].ptr, tabs[3].ptr, tabs[4].ptr, tk.ptr if tk else None, te.ptr if te else None,
                                     tabs[5].ptr, tabs[6].ptr, eps, out.ptr, mean.ptr, rstd.ptr, presum.ptr)
    assert rc == 0, rc
    what = "vb_text_embed_ln_fwd"
    return (out.cpu(what).view(batch, n_out, hidden), mean.cpu(what).view(batch, n_out), rstd.cpu(what).view(batch, n_out),
            presum.cpu(what).view(batch, n_out, hidden))


def _text_embed64(ids, seg, pos_offset, word, pos, typ, task_ids, temb):
    """float64 pre-LayerNorm sum and the sum of the |terms| (ids outside their table: zero rows)."""
    batch, n_tok = ids.shape

    def rows_of(table, idx):
        ok = ((idx >= 0) & (idx < table.shape[0])).double()[..., None]
        return table.double()[idx.clamp(0, table.shape[0] - 1)] * ok

    w, t = rows_of(word, ids), rows_of(typ, seg)
    p = pos.double()[torch.arange(n_tok) + pos_offset][None].expand(batch, -1, -1)
    e, mag = w + p + t, w.abs() + p.abs() + t.abs()
    if task_ids is not None:
        tr = rows_of(temb, task_ids.view(batch, 1))
        e, mag = torch.cat([e[:, :1], tr, e[:, 1:]], 1), torch.cat([mag[:, :1], tr.abs(), mag[:, 1:]], 1)
    return e, mag


def _check_embed(got, e64, mag64, g, b, eps, what):
    out, mean, rstd, presum = got
    h = e64.shape[-1]
    ref = RB.ln64(e64.reshape(-1, h), g, b, eps)
    _within(presum, e64, 3 * U * mag64 + 1e-37, what + " presum")          # two fp32 additions
    _close(out.reshape(-1, h), ref["y"], what=what + " out")
    _close(mean.reshape(-1), ref["mean"], what=what + " mean")
    _close(rstd.reshape(-1), ref["rstd"], 1e-5, 1e-6, what=what + " rstd")


@pytest.mark.parametrize("batch,n_tok", [(1, 1), (3, 7), (2, 37)])
@pytest.mark.parametrize("hidden", [4, 96, 768, 1028])
def test_text_embedding_statistics_presum_position_offset_and_task_row(hidden, batch, n_tok):
    gen = torch.Generator().manual_seed(hidden + n_tok)
    ids = torch.randint(0, V, (batch, n_tok), generator=gen)
    seg = torch.randint(0, N_TYPES, (batch, n_tok), generator=gen)
    tid = torch.randint(0, N_TASKS, (batch,), generator=gen)
    word, typ, temb = _rand(V, hidden, seed=1), _rand(N_TYPES, hidden, seed=3), _rand(N_TASKS, hidden, seed=4)
    g, b = _ln_params(hidden, 5)
    for task in (False, True):
        for pos_offset in (0, 2):
            pos = _rand(n_tok + pos_offset, hidden, seed=2)                # exactly the rows the launch may read
            args = (ids, seg, pos_offset, word, pos, typ, tid if task else None, temb if task else None)
            got = _text_embed(*args, g, b)
            assert got[0].shape[1] == n_tok + (1 if task else 0)
            e64, mag = _text_embed64(*args)
            if task:                                                       # output row 1 is the task row, bit for bit
                assert torch.equal(_bits(got[3][:, 1]), _bits(temb[tid]))
            _check_embed(got, e64, mag, g, b, 1e-12, "hidden %d %dx%d task=%s pos_offset=%d" % (
                hidden, batch, n_tok, task, pos_offset))


def test_text_embedding_single_type_table_and_ids_outside_their_tables():
    batch, n_tok, hidden = 3, 7, 96
    gen = torch.Generator().manual_seed(9)
    ids = torch.randint(0, V, (batch, n_tok), generator=gen)
    seg = torch.zeros(batch, n_tok, dtype=I64)
    ids[0, 1], ids[1, 2], ids[2, 6] = V + 5, -3, V
    seg[2, 3], seg[0, 0] = 1, -1                                           # n_types = 1: 1 is outside the table
    tid = torch.tensor([N_TASKS, -1, 1])
    word, pos, typ, temb = _rand(V, hidden, seed=1), _rand(n_tok, hidden, seed=2), _rand(1, hidden, seed=3), \
        _rand(N_TASKS, hidden, seed=4)
    g, b = _ln_params(hidden, 5)
    for task in (False, True):
        args = (ids, seg, 0, word, pos, typ, tid if task else None, temb if task else None)
        got = _text_embed(*args, g, b)
        e64, mag = _text_embed64(*args)
        if task:
            # a task id outside its table: a zero row - constant, so its LayerNorm output is beta
            assert float(got[3][0, 1].abs().max()) == 0.0 and float(got[3][1, 1].abs().max()) == 0.0
        _check_embed(got, e64, mag, g, b, 1e-12, "task=%s" % task)


@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("hidden", [4, 768, 1024])
def test_image_embedding_four_outputs_and_four_byte_aligned_location_operands(hidden, rows):
    proj, wl, bl = _rand(rows, hidden, seed=1), _rand(hidden, 5, seed=3), _rand(hidden, seed=4)
    loc = torch.rand(rows, 5, generator=torch.Generator().manual_seed(2))
    g, b = _ln_params(hidden, 5)
    # loc and w_loc one float into their buffers: read one float at a time, 4-byte alignment must do
    locd = Guard.of(torch.cat([torch.zeros(1), loc.reshape(-1)]))
    wld = Guard.of(torch.cat([torch.zeros(1), wl.reshape(-1)]))
    ins = [Guard.of(t) for t in (proj, bl, g, b)]
    out, presum, mean, rstd = Guard(rows * hidden), Guard(rows * hidden), Guard(rows), Guard(rows)
    assert (locd.ptr + 4) % 16 == 4
    rc = _lib().vb_image_embed_ln_fwd(_st(), rows, hidden, ins[0].ptr, locd.ptr + 4, wld.ptr + 4, ins[1].ptr, ins[2].ptr,
                                      ins[3].ptr, 1e-12, out.ptr, mean.ptr, rstd.ptr, presum.ptr)
    assert rc == 0, rc
    what = "vb_image_embed_ln_fwd %dx%d" % (rows, hidden)
    terms = loc.double()[:, None, :] * wl.double()[None, :, :]             # [rows, hidden, 5]
    e64 = proj.double() + terms.sum(-1) + bl.double()
    mag = proj.double().abs() + terms.abs().sum(-1) + bl.double().abs()
    got = (out.cpu(what).view(rows, hidden), mean.cpu(what), rstd.cpu(what), presum.cpu(what).view(rows, hidden))
    ref = RB.ln64(e64, g, b, 1e-12)
    _within(got[3], e64, 8 * U * mag, what + " presum")                    # five fused multiply-adds and two additions
    _close(got[0], ref["y"], what=what + " out")
    _close(got[1], ref["mean"], what=what + " mean")
    _close(got[2], ref["rstd"], 1e-5, 1e-6, what=what + " rstd")


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("is_f32", [0, 1])
def test_additive_mask_is_exact(n, is_f32):
    m = torch.randint(0, 2, (n,), generator=torch.Generator().manual_seed(n))
    src = Guard.of(m.float() if is_f32 else m)
    out = Guard(n)
    assert _lib().vb_additive_mask(_st(), n, src.ptr, is_f32, out.ptr) == 0
    assert torch.equal(out.cpu("vb_additive_mask"), (1.0 - m.float()) * -10000.0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. losses
# ---------------------------------------------------------------------------------------------------------------------
def _padded(x, ld, fill=NAN):
    """[rows, ld] with x in the first columns and `fill` (NaN: must never be read) in the padding."""
    out = torch.full((x.shape[0], ld), fill, dtype=x.dtype)
    out[:, :x.shape[1]] = x
    return out


def _rect(guard, rows, n, ld, what):
    """The [rows, n] rectangle a kernel wrote into the guarded [rows, ld] buffer; the padding columns still hold the canary."""
    bits = guard.u32(what).reshape(rows, ld)
    assert (bits[:, n:] == CANARY32).all(), "%s: wrote into the padding columns" % what
    return guard.t.cpu().view(rows, ld)[:, :n].contiguous()


def _xent(logits, labels, ld, ldd, grad_loss, ignore=-1):
    """vb_xent_fwd then vb_xent_bwd on padded rows: dict of CPU tensors row_loss, lse, loss, count, dlogits [rows, n]."""
    rows, n = logits.shape
    xd, lab, gl = Guard.of(_padded(logits, ld)), Guard.of(labels), Guard.of(torch.tensor([grad_loss]))
    row_loss, lse, loss, count = Guard(rows), Guard(rows), Guard(1), Guard(1)
    assert _lib().vb_xent_fwd(_st(), rows, n, xd.ptr, ld, lab.ptr, ignore, row_loss.ptr, lse.ptr, loss.ptr, count.ptr) == 0
    d = Guard(rows * ldd)
    assert _lib().vb_xent_bwd(_st(), rows, n, xd.ptr, ld, lab.ptr, ignore, lse.ptr, gl.ptr, count.ptr, d.ptr, ldd) == 0
    what = "vb_xent %dx%d" % (rows, n)
    return {"row_loss": row_loss.cpu(what), "lse": lse.cpu(what), "loss": loss.cpu(what)[0], "count": count.cpu(what)[0],
            "dlogits": _rect(d, rows, n, ldd, what)}


XENT_SHAPES = [(1, 2, 2, 3), (5, 7, 12, 9), (37, 1601, 1604, 1608)]       # rows, n, ld, ldd (ldd != ld)


@pytest.mark.parametrize("rows,n,ld,ldd", XENT_SHAPES)
def test_cross_entropy_on_padded_rows_with_a_separate_gradient_stride(rows, n, ld, ldd):
    gen = torch.Generator().manual_seed(rows * 31 + n)
    logits = torch.randn(rows, n, generator=gen) * 3.0
    labels = torch.randint(0, n, (rows,), generator=gen)
    if rows > 2:
        labels[torch.rand(rows, generator=gen) < 0.3] = -1
        labels[0], labels[1] = n - 1, -1
    got = _xent(logits, labels, ld, ldd, 1.7)
    x64 = logits.double().requires_grad_(True)
    want = torch.nn.CrossEntropyLoss(ignore_index=-1)(x64, labels)
    (want * 1.7).backward()
    ref = RB.xent64(logits, labels)
    assert float(got["count"]) == ref["count"]
    _close(got["loss"], want.detach(), RB.XENT_LOSS_RTOL, RB.XENT_LOSS_ATOL, "loss")
    _within(got["row_loss"], ref["row_loss"], RB.loss_tolerance(ref["row_loss"]), "row_loss")
    live = labels != -1
    _close(got["lse"][live], ref["lse"][live], RB.XENT_LOSS_RTOL, RB.XENT_LOSS_ATOL, "lse")
    assert float(got["row_loss"][~live].abs().sum()) == 0.0 and float(got["dlogits"][~live].abs().sum()) == 0.0
    # p - onehot cancels when p -> 1: absolute error is fp32 roundoff of p (6e-8) times the loss scale
    _close(got["dlogits"], x64.grad, RB.XENT_GRAD_RTOL, RB.XENT_GRAD_ATOL, "dlogits")


def test_cross_entropy_all_rows_ignored_out_of_range_label_and_no_rows():
    rows, n, ld, ldd = 5, 7, 12, 9
    logits = _rand(rows, n, seed=2)
    got = _xent(logits, torch.full((rows,), -1, dtype=I64), ld, ldd, 1.0)
    assert torch.isnan(got["loss"]) and float(got["count"]) == 0.0
    assert float(got["dlogits"].abs().max()) == 0.0
    got = _xent(logits, torch.tensor([1, -1, n, 3, -5]), ld, ldd, 1.0)     # n and -5 are outside [0, n)
    assert torch.isnan(got["loss"]) and float(got["count"]) == 4.0
    assert torch.isnan(got["row_loss"][[2, 4]]).all() and torch.isfinite(got["row_loss"][[0, 1, 3]]).all()
    assert torch.isfinite(got["dlogits"]).all()
    # rows = 0: the forward still writes loss (0 / 0) and count, the backward writes nothing and returns 0
    xd, lab, gl = Guard.of(logits), Guard.of(torch.zeros(1, dtype=I64)), Guard.of(torch.ones(1))
    row_loss, lse, loss, count, d = Guard(1), Guard(1), Guard(1), Guard(1), Guard(ldd)
    assert _lib().vb_xent_fwd(_st(), 0, n, xd.ptr, ld, lab.ptr, -1, row_loss.ptr, lse.ptr, loss.ptr, count.ptr) == 0
    assert torch.isnan(loss.cpu("loss")[0]) and float(count.cpu("count")[0]) == 0.0
    row_loss.untouched("row_loss")
    lse.untouched("lse")
    assert _lib().vb_xent_bwd(_st(), 0, n, xd.ptr, ld, lab.ptr, -1, lse.ptr, gl.ptr, count.ptr, d.ptr, ldd) == 0
    d.untouched("dlogits")


@pytest.mark.parametrize("shift", [64.0, 1000.0])
def test_cross_entropy_does_not_depend_on_a_common_shift_of_the_logits(shift):
    """The row loss of logits + c is held to the tolerance of the unshifted test, per row (the mean over the rows averages the
    roundings away). lse - x[label] from the rounded lse carries half an ulp of |lse| = c + ... (2.6e-5 at c = 1000 against a
    tolerance of 1.3e-5: tests/test_row_kernels_tolerances.py); log(s) - (x[label] - max) does not."""
    rows, n, ld, ldd = 37, 1601, 1604, 1608
    logits, labels = RB.xent_shift_case(rows, n, seed=5)
    shifted = logits + shift
    got = _xent(shifted, labels, ld, ldd, float(rows))                     # grad_loss / count = 1: dlogits = p - onehot
    ref = RB.xent64(shifted, labels)
    err = (got["row_loss"].double() - ref["row_loss"]).abs()
    print("cross entropy, logits + %g: row-loss max err %.3e (tolerance %.3e), mean-loss err %.3e" % (
        shift, err.max(), RB.loss_tolerance(ref["row_loss"]).min(), abs(float(got["loss"]) - float(ref["row_loss"].mean()))))
    _within(got["row_loss"], ref["row_loss"], RB.loss_tolerance(ref["row_loss"]), "row_loss")
    _close(got["loss"], ref["row_loss"].mean(), RB.XENT_LOSS_RTOL, RB.XENT_LOSS_ATOL, "loss")
    _close(got["lse"], ref["lse"], RB.XENT_LOSS_RTOL, RB.XENT_LOSS_ATOL, "lse")
    # the backward reads the saved lse, which is rounded to fp32: off by up to half an ulp, 2^-24 |lse|, so exp(x - lse) is off by
    # that factor: 2^-24 |lse| p, plus the unshifted test's absolute term
    onehot = torch.nn.functional.one_hot(labels, n).double()
    _within(got["dlogits"], ref["p"] - onehot, U * ref["lse"].abs()[:, None] * ref["p"] + 2e-7, "dlogits")


def _kl(scores, target, ld, ldt, ldd, divisor, grad_loss, on_device):
    """vb_kl_fwd then vb_kl_bwd on padded rows. on_device: the divisor comes through divisor_dev and the host argument is wrong."""
    rows, n = scores.shape
    sd, td, gl = Guard.of(_padded(scores, ld)), Guard.of(_padded(target, ldt)), Guard.of(torch.tensor([grad_loss]))
    dv = Guard.of(torch.tensor([divisor])) if on_device else None
    host = 12345.0 if on_device else divisor
    row_loss, lse, tsum, loss = Guard(rows), Guard(rows), Guard(rows), Guard(2)
    assert _lib().vb_kl_fwd(_st(), rows, n, sd.ptr, ld, td.ptr, ldt, host, row_loss.ptr, lse.ptr, tsum.ptr, loss.ptr,
                            dv.ptr if dv else None) == 0
    d = Guard(rows * ldd)
    assert _lib().vb_kl_bwd(_st(), rows, n, sd.ptr, ld, td.ptr, ldt, lse.ptr, tsum.ptr, gl.ptr, host, d.ptr, ldd,
                            dv.ptr if dv else None) == 0
    what = "vb_kl %dx%d" % (rows, n)
    return {"row_loss": row_loss.cpu(what), "lse": lse.cpu(what), "tsum": tsum.cpu(what), "loss": loss.cpu(what),
            "dscores": _rect(d, rows, n, ldd, what)}


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("rows,n,ld,ldt,ldd", [(1, 33, 33, 33, 33), (9, 1601, 1604, 1608, 1612)])
def test_kl_divergence_host_and_device_divisor_on_padded_rows(rows, n, ld, ldt, ldd, on_device):
    gen = torch.Generator().manual_seed(rows + n)
    scores = torch.randn(rows, n, generator=gen) * 2.0
    target = torch.softmax(torch.randn(rows, n, generator=gen) * 2.0, -1)
    target[:, ::5] = 0.0
    if rows > 2:
        target[2] = 0.0                                                    # a row the fixed-capacity gather left empty
    divisor = float(rows - 1) if rows > 2 else 1.0
    got = _kl(scores, target, ld, ldt, ldd, divisor, 0.6, on_device)
    s64 = scores.double().requires_grad_(True)
    per_row = torch.nn.KLDivLoss(reduction="none")(torch.log_softmax(s64, 1), target.double()).sum(1)
    want = per_row.sum() / divisor
    (want * 0.6).backward()
    assert float(got["loss"][1]) == divisor
    _close(got["loss"][0], want.detach(), 5e-6, 1e-6, "loss")
    _close(got["row_loss"], per_row.detach(), 5e-6, 1e-6, "row_loss")
    _close(got["tsum"], target.double().sum(1), 5e-6, 1e-6, "tsum")
    _close(got["dscores"], s64.grad, 2e-5, 2e-7, "dscores")
    if rows > 2:
        assert float(got["row_loss"][2]) == 0.0 and float(got["tsum"][2]) == 0.0
        assert float(got["dscores"][2].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 5. elementwise
# ---------------------------------------------------------------------------------------------------------------------
def _act_bwd(act, dy, pre):
    n = pre.numel()
    dyd, pd, out = Guard.of(dy), Guard.of(pre), Guard(n)
    assert _lib().vb_act_bwd(_st(), n, ACTS[act], dyd.ptr, pd.ptr, out.ptr) == 0
    return out.cpu("vb_act_bwd " + act)


@pytest.mark.parametrize("act", ["gelu", "relu", "swish"])
def test_activation_derivative_over_a_sweep_with_the_tails(act):
    x = RB.act_sweep()
    got = _act_bwd(act, torch.ones_like(x), x)
    _, want = RB.act64(act, x)
    tol = RB.act_grad_tolerance(act, x)
    err = (got.double() - want).abs()
    core = x.abs() <= 12
    print("vb_act_bwd %s over [-12, 12] + tails: max err %.3e, worst err / bar %s" % (
        act, err.max(), "%.3f" % float((err / tol)[tol > 0].max()) if act != "relu" else "(exact)"))
    assert torch.isfinite(got).all()
    if act == "relu":
        assert torch.equal(got, want.float())                              # 0 at +-0 and below, 1 above
    else:
        assert (err[core] <= tol[core]).all(), "worst err / bar %.3f at x = %g" % (
            float((err / tol).max()), float(x[(err / tol).argmax()]))
        assert (err <= tol).all()


@pytest.fixture
def f32_gemm():
    """fp32 GEMM arithmetic and a chosen tile code for one test; both restored."""
    N = _N()
    prev_mode, prev_tile = N.set_gemm_mode("f32"), N.set_gemm_tile(0)
    yield N.set_gemm_tile
    N.set_gemm_tile(prev_tile)
    N.set_gemm_mode(prev_mode)


@pytest.mark.parametrize("code", [-1, 0])
@pytest.mark.parametrize("act", ["gelu", "relu", "swish"])
def test_activation_values_through_the_gemm_epilogue(f32_gemm, act, code):
    """The forward values of the epilogue activations over the same sweep: A carries x in column 0 and zeros elsewhere, every
    row of W is the first unit vector, so the pre-activation is exactly x (fp32 mode). Tile code -1: the round-1 kernel and its
    post-pass, 0: the cost model's choice (fused epilogue)."""
    f32_gemm(code)
    N = _N()
    x = RB.act_sweep()
    M, K, Nn = x.numel(), 16, 4
    A, W = torch.zeros(M, K), torch.zeros(Nn, K)
    A[:, 0], W[:, 0] = x, 1.0
    ad, wd = Guard.of(A), Guard.of(W)
    c = Guard(M * Nn)
    grad = Guard(M * Nn) if act != "swish" else None                       # act_grad: gelu and relu (include/vilbert_hip.h)
    a = N.LinearArgs()
    a.M, a.K, a.nseg, a.seg_n = M, K, 1, Nn
    a.A, a.lda, a.ldw = ad.ptr, K, K
    a.W[0] = wd.ptr
    a.C, a.ldc = c.ptr, Nn
    if grad is not None:
        a.act_grad, a.ldg = grad.ptr, Nn
    a.act = ACTS[act]
    assert N.lib().vb_linear_fwd(_st(), ctypes.byref(a)) == 0
    what = "vb_linear_fwd %s tile %d" % (act, code)
    want_v, want_d = RB.act64(act, x)
    got = c.cpu(what).view(M, Nn)
    err = (got.double() - want_v[:, None]).abs()
    tol = RB.act_value_tolerance(act, x, want_v)[:, None].expand(-1, Nn)
    print("%s: value max err %.3e%s" % (what, err.max(), "" if act == "relu" else
                                        ", worst err / bar %.3f" % float((err / tol.clamp(min=1e-300)).max())))
    assert torch.isfinite(got).all()
    if act == "relu":
        assert torch.equal(got, want_v.float()[:, None].expand(-1, Nn))
    else:
        assert (err <= tol).all(), "worst err / bar %.3f" % float((err / tol.clamp(min=1e-300)).max())
    if grad is not None:
        gd = grad.cpu(what).view(M, Nn)
        if act == "relu":
            assert torch.equal(gd, want_d.float()[:, None].expand(-1, Nn))
        else:
            _within(gd, want_d[:, None].expand(-1, Nn), RB.act_grad_tolerance(act, x)[:, None].expand(-1, Nn), what + " act_grad")


EW_WRAP = 2048 * 256 * 4            # elements one pass of the capped grid covers (EW_MAX_BLOCKS x 256 threads x 4)


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_activation_backward_grid_stride_loop_wraps(act):
    n = EW_WRAP + 1028
    dy, pre = _rand(n, seed=1), _rand(n, seed=2, scale=2.0)
    got = _act_bwd(act, dy, pre)
    _, d64 = RB.act64(act, pre)
    _within(got, dy.double() * d64, dy.double().abs() * RB.act_grad_tolerance(act, pre) + U * (dy.double() * d64).abs(),
            "vb_act_bwd %s, %d elements" % (act, n))


@pytest.mark.parametrize("residual", [False, True])
def test_dropout_grid_stride_loop_wraps_and_the_tail(residual, plain_seed):
    n, p = EW_WRAP + 1031, 0.1                                              # the loop wraps; a 3-element tail
    x, res = _rand(n, seed=3), _rand(n, seed=4)
    x[x == 0] = 1.0                                                         # (the mask is read off the non-zero outputs)
    xd, rd, y = Guard.of(x), Guard.of(res) if residual else None, Guard(n)
    assert _lib().vb_dropout(_st(), n, xd.ptr, rd.ptr if rd else None, y.ptr, p, SEED) == 0
    got = y.cpu("vb_dropout")
    keep = torch.from_numpy(DR.keep(SEED, DR.flat_index(n), p))
    assert 0.88 < float(keep.double().mean()) < 0.92
    base = res if residual else torch.zeros(n)
    # dropped elements: the residual alone, bit for bit (unmasked; 0 without one); without a residual the non-zero outputs ARE the
    # mask, at every index (with one, a kept element that the mask had dropped would miss its value bound below)
    assert torch.equal(got[~keep], base[~keep]), "the mask differs from the host restatement"
    if not residual:
        assert torch.equal(got != 0, keep), "the mask differs from the host restatement"
    # kept elements: x / (1 - p) to one ulp (the fp32 scale 1 / (1 - p) and the product round once each), then the addition
    scaled = x.double()[keep] / (1.0 - float(np.float32(p)))
    want = scaled + base.double()[keep]
    _within(got[keep], want, 2 * U * scaled.abs() + (U * want.abs() if residual else 0.0), "kept values")


def test_dropout_with_p_zero_copies_exactly(plain_seed):
    n = 1031
    x = _rand(n, seed=5)
    xd, y = Guard.of(x), Guard(n)
    assert _lib().vb_dropout(_st(), n, xd.ptr, None, y.ptr, 0.0, SEED) == 0
    assert torch.equal(y.cpu("vb_dropout p = 0"), x)


# ---------------------------------------------------------------------------------------------------------------------
# 6. error contracts: the return code, and every output byte untouched. Argument checks only - each of these is refused by
#    the host code before any launch (buffers are nevertheless sized for the shape the call names).
# ---------------------------------------------------------------------------------------------------------------------
class Call:
    """A valid call of one entry point as an ordered name -> value table; `outs` are its guarded outputs."""

    def __init__(self, fn, args, outs, keep):
        self.fn, self.args, self.outs, self.keep = fn, args, outs, keep

    def run(self):
        return getattr(_lib(), self.fn)(_st(), *self.args.values())


def _g(n):
    return Guard(n, F32)


def _inp(n, dtype=F32):
    """Input buffer with n harmless elements plus one spare (so that a 4-byte offset stays inside it)."""
    g = Guard(n + 4, dtype)
    g.t.zero_()
    return g


def _call_ln_fwd(rows=2, cols=8):
    r, c = max(rows, 1), max((cols + 3) // 4 * 4, 4)
    ins = {k: _inp(n) for k, n in (("x", r * c), ("x2", r * c), ("gamma", c), ("beta", c))}
    outs = {"y": _g(r * c + 4), "mean": _g(r), "rstd": _g(r)}
    args = dict(rows=rows, n_cols=cols, x=ins["x"].ptr, x2=ins["x2"].ptr, gamma=ins["gamma"].ptr, beta=ins["beta"].ptr,
                eps=1e-12, y=outs["y"].ptr, mean=outs["mean"].ptr, rstd=outs["rstd"].ptr)
    return Call("vb_layernorm_fwd", args, outs, ins)


def _call_ln_bwd(rows=2, cols=8, drop=False):
    r, c = max(rows, 1), max((cols + 3) // 4 * 4, 4)
    ws_n = max(int(_lib().vb_layernorm_bwd_workspace(r, c)), 2 * c)
    ins = {k: _inp(n) for k, n in (("dy", r * c), ("x", r * c), ("mean", r), ("rstd", r), ("gamma", c))}
    outs = {"dx": _g(r * c + 4), "dgamma": _g(c), "dbeta": _g(c), "workspace": _g(ws_n + 4)}
    args = dict(rows=rows, n_cols=cols, dy=ins["dy"].ptr, x=ins["x"].ptr, mean=ins["mean"].ptr, rstd=ins["rstd"].ptr,
                gamma=ins["gamma"].ptr, dx=outs["dx"].ptr, dgamma=outs["dgamma"].ptr, dbeta=outs["dbeta"].ptr,
                workspace=outs["workspace"].ptr)
    if drop:
        outs["dx_dropped"] = _g(r * c + 4)
        args.update(dx_dropped=outs["dx_dropped"].ptr, dropout_p=0.1, seed=SEED)
    return Call("vb_layernorm_bwd_drop" if drop else "vb_layernorm_bwd", args, outs, ins)


def _call_ln_bwd_drop(rows=2, cols=8):
    return _call_ln_bwd(rows, cols, drop=True)


def _call_act_bwd(n=1032):
    ins = {"dy": _inp(n), "preact": _inp(n)}
    outs = {"dx": _g(n + 4)}
    return Call("vb_act_bwd", dict(n=n, act=ACT_GELU, dy=ins["dy"].ptr, preact=ins["preact"].ptr, dx=outs["dx"].ptr), outs, ins)


def _call_dropout(n=1031):
    ins = {"x": _inp(n), "residual": _inp(n)}
    outs = {"y": _g(n + 4)}
    return Call("vb_dropout", dict(n=n, x=ins["x"].ptr, residual=ins["residual"].ptr, y=outs["y"].ptr, p=0.1, seed=SEED),
                outs, ins)


def _call_xent_fwd(rows=3, n=7, ld=12):
    ins = {"logits": _inp(rows * ld), "labels": _inp(rows, I64)}
    outs = {k: _g(m) for k, m in (("row_loss", rows), ("lse", rows), ("loss", 1), ("count", 1))}
    args = dict(rows=rows, n=n, logits=ins["logits"].ptr, ld=ld, labels=ins["labels"].ptr, ignore_index=-1,
                row_loss=outs["row_loss"].ptr, lse=outs["lse"].ptr, loss=outs["loss"].ptr, count=outs["count"].ptr)
    return Call("vb_xent_fwd", args, outs, ins)


def _call_xent_bwd(rows=3, n=7, ld=12, ldd=9):
    ins = {k: _inp(m, dt) for k, m, dt in (("logits", rows * ld, F32), ("labels", rows, I64), ("lse", rows, F32),
                                           ("grad_loss", 1, F32), ("count", 1, F32))}
    outs = {"dlogits": _g(rows * max(ldd, ld))}
    args = dict(rows=rows, n=n, logits=ins["logits"].ptr, ld=ld, labels=ins["labels"].ptr, ignore_index=-1, lse=ins["lse"].ptr,
                grad_loss=ins["grad_loss"].ptr, count=ins["count"].ptr, dlogits=outs["dlogits"].ptr, ldd=ldd)
    return Call("vb_xent_bwd", args, outs, ins)


def _call_kl_fwd(rows=3, n=7, ld=12, ldt=8):
    ins = {"scores": _inp(rows * ld), "target": _inp(rows * ld)}
    outs = {k: _g(m) for k, m in (("row_loss", rows), ("lse", rows), ("tsum", rows), ("loss", 2))}
    args = dict(rows=rows, n=n, scores=ins["scores"].ptr, ld=ld, target=ins["target"].ptr, ldt=ldt, divisor=3.0,
                row_loss=outs["row_loss"].ptr, lse=outs["lse"].ptr, tsum=outs["tsum"].ptr, loss=outs["loss"].ptr,
                divisor_dev=None)
    return Call("vb_kl_fwd", args, outs, ins)


def _call_kl_bwd(rows=3, n=7, ld=12, ldt=8, ldd=9):
    ins = {k: _inp(m) for k, m in (("scores", rows * ld), ("target", rows * ld), ("lse", rows), ("tsum", rows),
                                   ("grad_loss", 1))}
    outs = {"dscores": _g(rows * ld)}
    args = dict(rows=rows, n=n, scores=ins["scores"].ptr, ld=ld, target=ins["target"].ptr, ldt=ldt, lse=ins["lse"].ptr,
                tsum=ins["tsum"].ptr, grad_loss=ins["grad_loss"].ptr, divisor=3.0, dscores=outs["dscores"].ptr, ldd=ldd,
                divisor_dev=None)
    return Call("vb_kl_bwd", args, outs, ins)


def _call_text_embed(batch=2, n_tok=3, hidden=8):
    rows = batch * (n_tok + 1)
    ins = {k: _inp(m, dt) for k, m, dt in (("ids", batch * n_tok, I64), ("seg", batch * n_tok, I64), ("word_emb", V * hidden, F32),
                                           ("pos_emb", n_tok * hidden, F32), ("type_emb", N_TYPES * hidden, F32),
                                           ("task_ids", batch, I64), ("task_emb", N_TASKS * hidden, F32),
                                           ("gamma", hidden, F32), ("beta", hidden, F32))}
    outs = {k: _g(m) for k, m in (("out", rows * hidden), ("mean", rows), ("rstd", rows), ("presum", rows * hidden))}
    args = dict(batch=batch, n_tok=n_tok, hidden=hidden, vocab=V, n_types=N_TYPES, n_tasks=N_TASKS, ids=ins["ids"].ptr,
                seg=ins["seg"].ptr, pos_offset=0, word_emb=ins["word_emb"].ptr, pos_emb=ins["pos_emb"].ptr,
                type_emb=ins["type_emb"].ptr, task_ids=ins["task_ids"].ptr, task_emb=ins["task_emb"].ptr,
                gamma=ins["gamma"].ptr, beta=ins["beta"].ptr, eps=1e-12, out=outs["out"].ptr, mean=outs["mean"].ptr,
                rstd=outs["rstd"].ptr, presum=outs["presum"].ptr)
    return Call("vb_text_embed_ln_fwd", args, outs, ins)


def _call_image_embed(rows=3, hidden=8):
    ins = {k: _inp(m) for k, m in (("feat_proj", rows * hidden), ("loc", rows * 5), ("w_loc", hidden * 5), ("b_loc", hidden),
                                   ("gamma", hidden), ("beta", hidden))}
    outs = {k: _g(m) for k, m in (("out", rows * hidden), ("mean", rows), ("rstd", rows), ("presum", rows * hidden))}
    args = dict(rows=rows, hidden=hidden, feat_proj=ins["feat_proj"].ptr, loc=ins["loc"].ptr, w_loc=ins["w_loc"].ptr,
                b_loc=ins["b_loc"].ptr, gamma=ins["gamma"].ptr, beta=ins["beta"].ptr, eps=1e-12, out=outs["out"].ptr,
                mean=outs["mean"].ptr, rstd=outs["rstd"].ptr, presum=outs["presum"].ptr)
    return Call("vb_image_embed_ln_fwd", args, outs, ins)


def _set(**kw):
    return lambda a: a.update(kw)


def _offset4(name):
    def f(a):
        a[name] += 4
    return f


LN_ENTRIES = [_call_ln_fwd, _call_ln_bwd, _call_ln_bwd_drop]
ERROR_CASES = []        # (id, builder, builder kwargs, mutation, expected code)
for _b in LN_ENTRIES:
    _n = _b.__name__[6:]
    ERROR_CASES += [(_n + "-cols0", _b, dict(cols=0), None, E_BADARG), (_n + "-cols6", _b, dict(cols=6), None, E_ALIGN),
                    (_n + "-cols8196", _b, dict(cols=8196), None, E_RANGE), (_n + "-rows0", _b, dict(rows=0), None, E_BADARG)]
ERROR_CASES += [("ln_fwd-offset-" + k, _call_ln_fwd, {}, _offset4(k), E_ALIGN) for k in ("x", "x2", "y", "gamma", "beta")]
for _b, _c in ((_call_ln_bwd, 8), (_call_ln_bwd, 4100), (_call_ln_bwd_drop, 8)):
    ERROR_CASES += [("%s-%d-offset-%s" % (_b.__name__[6:], _c, k), _b, dict(cols=_c), _offset4(k), E_ALIGN)
                    for k in ("dy", "x", "gamma", "dx", "workspace")]
ERROR_CASES += [
    ("ln_bwd_drop-offset-dx_dropped", _call_ln_bwd_drop, {}, _offset4("dx_dropped"), E_ALIGN),
    ("ln_bwd_drop-cols4100", _call_ln_bwd_drop, dict(cols=4100), None, E_RANGE),
    ("ln_bwd_drop-p0", _call_ln_bwd_drop, {}, _set(dropout_p=0.0), E_BADARG),
    ("ln_bwd_drop-p1", _call_ln_bwd_drop, {}, _set(dropout_p=1.0), E_BADARG),
    ("ln_bwd_drop-pnan", _call_ln_bwd_drop, {}, _set(dropout_p=NAN), E_BADARG),
    ("ln_bwd_drop-null-dx_dropped", _call_ln_bwd_drop, {}, _set(dx_dropped=None), E_BADARG),
    ("act_bwd-n1030", _call_act_bwd, dict(n=1030), None, E_ALIGN),
    ("act_bwd-act7", _call_act_bwd, {}, _set(act=7), E_BADARG),
    ("act_bwd-act-none", _call_act_bwd, {}, _set(act=ACT_NONE), E_BADARG),
    ("act_bwd-offset-dx", _call_act_bwd, {}, _offset4("dx"), E_ALIGN),
    ("dropout-p-negative", _call_dropout, {}, _set(p=-0.1), E_BADARG),
    ("dropout-p1", _call_dropout, {}, _set(p=1.0), E_BADARG),
    ("dropout-pnan", _call_dropout, {}, _set(p=NAN), E_BADARG),
    ("xent_fwd-ld-below-n", _call_xent_fwd, {}, _set(ld=6), E_BADARG),
    ("xent_fwd-n0", _call_xent_fwd, {}, _set(n=0), E_BADARG),
    ("xent_bwd-ld-below-n", _call_xent_bwd, {}, _set(ld=6), E_BADARG),
    ("xent_bwd-ldd-below-n", _call_xent_bwd, {}, _set(ldd=6), E_BADARG),
    ("xent_bwd-n0", _call_xent_bwd, {}, _set(n=0), E_BADARG),
    ("kl_fwd-ld-below-n", _call_kl_fwd, {}, _set(ld=6), E_BADARG),
    ("kl_fwd-ldt-below-n", _call_kl_fwd, {}, _set(ldt=6), E_BADARG),
    ("kl_fwd-n0", _call_kl_fwd, {}, _set(n=0), E_BADARG),
    ("kl_bwd-ld-below-n", _call_kl_bwd, {}, _set(ld=6), E_BADARG),
    ("kl_bwd-ldt-below-n", _call_kl_bwd, {}, _set(ldt=6), E_BADARG),
    ("kl_bwd-ldd-below-n", _call_kl_bwd, {}, _set(ldd=6), E_BADARG),
    ("kl_bwd-n0", _call_kl_bwd, {}, _set(n=0), E_BADARG),
    ("text_embed-task_ids-without-task_emb", _call_text_embed, {}, _set(task_emb=None), E_BADARG),
    ("text_embed-task_ids-without-tasks", _call_text_embed, {}, _set(n_tasks=0), E_BADARG),
    ("text_embed-hidden6", _call_text_embed, {}, _set(hidden=6), E_ALIGN),
    ("image_embed-hidden0", _call_image_embed, {}, _set(hidden=0), E_BADARG),
    ("image_embed-rows0", _call_image_embed, {}, _set(rows=0), E_BADARG),
]
ERROR_CASES += [("text_embed-offset-" + k, _call_text_embed, {}, _offset4(k), E_ALIGN)
                for k in ("word_emb", "pos_emb", "type_emb", "task_emb", "out", "gamma")]
ERROR_CASES += [("image_embed-offset-" + k, _call_image_embed, {}, _offset4(k), E_ALIGN)
                for k in ("feat_proj", "b_loc", "out", "beta")]


@pytest.mark.parametrize("builder,kwargs,mutate,code", [pytest.param(*c[1:], id=c[0]) for c in ERROR_CASES])
def test_error_returns_leave_every_output_untouched(builder, kwargs, mutate, code):
    call = builder(**kwargs)
    if mutate is not None:
        mutate(call.args)
    assert call.run() == code
    for name, g in call.outs.items():
        g.untouched("%s (%s)" % (call.fn, name))
