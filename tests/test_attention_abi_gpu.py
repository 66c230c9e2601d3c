"""The four attention entry points of csrc/attention.hip, called directly: vb_attention_fwd / vb_attention_bwd and the same
source compiled with -DVB_ATTN_BF16, vb_attention_fwd_bf16 / vb_attention_bwd_bf16. The launchers (ops.attention_*,
ops16.attention_*, layers.hip) pass one narrow slice of what include/vilbert_hip.h promises - dense O and dO, ldv = ldk,
lddv = lddk, no key-side broadcast, dvec_mode only on chunks of 161+ keys - so a kernel that reads V with K's stride, or
ignores a given D vector, would pass every test that goes through them. This file pins the rest of the contract.

Rules of this file:
  * ctypes calls on vilbert._native.lib() with _native.AttentionArgs / AttentionGrads and raw pointers;
  * every output (O, probs, lse, dQ, dK, dV, dvec) lies in a Guard: a byte buffer full of canary bytes (0x5A) with a margin
    in front and behind. A strided output keeps canary bytes in its gap columns. After every call everything except the
    cells the call owns must still be canary; after a refused call everything must be;
  * strided inputs have NaN in their gap columns;
  * the reference is float64 torch arithmetic of vilbert.py:429-449 (scores / sqrt(d) + mask, softmax, dropout, context) and
    its hand-written backward, on the same input values (bf16 build: the bf16 values widened). The keep mask is the host
    restatement tests/dropout_restatement.py, never the kernel's own probabilities;
  * bounds are the project's own. fp32 tensors (O, dQ, dK, dV of the fp32 build; lse, probs, dvec of both builds):
    test_backward_gpu._close, 3e-5 + 3e-5 of max(1, largest reference magnitude). bf16 tensors: relative L2 <= 1.5e-2 and
    max error <= 2^-6 of the range, the bounds test_bf16_stream_gpu.py holds the bf16 kernels to against the fp32 kernels
    (which are within 6e-5 of float64);
  * every comparison prints one "parity" line with the measured error (profiles/attention_abi_parity.txt is that output).

Which kernel a shape reaches (launch_q / launch_kv / use_lds_path / the entry points at the end of attention.hip): with at
most 48 queries AND keys and no broadcast the LDS family (attn_q_lds_kernel forward, attn_bwd_fused_lds_kernel backward;
output strides not all % 4 == 0, fp32 only: attn_q_lds_kernel<BWD> + attn_bwd_kv_lds_kernel; a given D vector:
attn_q_kernel<BWD> + attn_bwd_kv_lds_kernel), otherwise attn_q_kernel with 3, 8 or 20 key tiles + attn_bwd_kv_kernel.
"""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":            # the VB_ATTN_LDS=0 child process: no conftest has set the paths
    ROOT = os.path.dirname(TESTS)
    for _p in (TESTS, os.path.join(ROOT, "vilbert-multi-task_amd"), ROOT):
        sys.path.insert(0, _p)

import dropout_restatement as DR
from test_backward_gpu import _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
E_BADARG, E_ALIGN, E_RANGE = -1, -2, -3
CANARY = 0x5A
NAN = float("nan")
SEED = 0x5EED0A77E27104
BUILDS = ["f32", "bf16"]
DTYPE = {"f32": torch.float32, "bf16": BF16}
FWD = {"f32": "vb_attention_fwd", "bf16": "vb_attention_fwd_bf16"}
BWD = {"f32": "vb_attention_bwd", "bf16": "vb_attention_bwd_bf16"}


def _N():
    from vilbert import _native
    return _native


def _st():
    return _N().stream_ptr()


def _heads(d):
    return 2 if d == 128 else 3


# ---------------------------------------------------------------------------------------------------------------------
# guarded outputs
# ---------------------------------------------------------------------------------------------------------------------
class Guard:
    """n elements of `dtype` on the device, canary bytes everywhere (payload included) and a canary margin on both sides.
    region() declares a [rows, width] rectangle with row stride ld that a call may write; fetch() checks that every other
    byte is still canary and returns the rectangles."""
    MARGIN = 512

    def __init__(self, n, dtype):
        self.dtype, self.n = dtype, n
        self.es = torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((2 * self.MARGIN + n * self.es,), CANARY, dtype=torch.uint8, device=DEV)
        self.t = self.buf[self.MARGIN:self.MARGIN + n * self.es].view(dtype)
        assert self.t.data_ptr() % 16 == 0
        self.regions = []

    @classmethod
    def matrix(cls, rows, width, ld, dtype, offset=0):
        """One [rows, width] output with row stride ld that starts `offset` elements into its buffer, in a buffer that
        ends with its last element. Returns (guard, pointer)."""
        g = cls(offset + (rows - 1) * ld + width, dtype)
        return g, g.region(offset, rows, width, ld)

    def region(self, offset, rows, width, ld):
        assert offset + (rows - 1) * ld + width <= self.n
        self.regions.append((offset, rows, width, ld))
        return self.t.data_ptr() + offset * self.es

    def fetch(self, what):
        """CPU copies of the declared rectangles, after checking that nothing else was written."""
        torch.cuda.synchronize()
        host = self.buf.cpu()
        payload = host[self.MARGIN:self.MARGIN + self.n * self.es]
        owned = torch.zeros(self.n, dtype=torch.bool)
        out = []
        for offset, rows, width, ld in self.regions:
            idx = (offset + torch.arange(rows)[:, None] * ld + torch.arange(width)[None, :]).reshape(-1)
            assert not bool(owned[idx].any()), "%s: two outputs share an element" % what
            owned[idx] = True
            out.append(payload.view(self.dtype)[idx].reshape(rows, width).clone())
        stray = payload.view(self.n, self.es)[~owned]
        assert bool((host[:self.MARGIN] == CANARY).all()) and bool((host[self.MARGIN + self.n * self.es:] == CANARY).all()), \
            "%s: wrote outside its buffer" % what
        assert bool((stray == CANARY).all()), "%s: wrote a gap column or a row that is not its own" % what
        return out

    def untouched(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf == CANARY).all()), "%s: wrote although it should not have" % what

    def fill(self, values):
        """Set the whole payload (a dense input / output such as dvec)."""
        self.t.copy_(values.reshape(-1).to(self.dtype))


def _input(t, ld):
    """CPU tensor [..., rows, width] -> device buffer [all rows, ld] cut after the last element, gap columns NaN."""
    t2 = t.reshape(-1, t.shape[-1])
    rows, width = t2.shape
    img = torch.full((rows, ld), NAN, dtype=t.dtype)
    img[:, :width] = t2
    return img.reshape(-1)[:(rows - 1) * ld + width].clone().to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# problems and their float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _mask(kv_batch, n_k):
    """Additive mask [kv_batch, n_k]: sample 0 keeps a prefix, sample 1 has holes, a third sample keeps every other key."""
    keep = torch.ones(kv_batch, n_k)
    keep[0, n_k - n_k // 3:] = 0
    if kv_batch > 1:
        keep[1, 1::3] = 0
    if kv_batch > 2:
        keep[2, 1::2] = 0
    return (1.0 - keep) * -10000.0


def _split(x, heads):
    B, S, H = x.shape
    return x.reshape(B, S, heads, H // heads).permute(0, 2, 1, 3)


def _merge(x):
    B, h, S, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, S, h * d)


def reference(q, k, v, mask, d_out, heads, scale, p, seed, lse=None, dvec=None):
    """float64 attention of vilbert.py:429-449 and its backward. q [B, n_q, H], k / v [B, n_k, H], mask [B, n_k] or None, all
    float64. lse / dvec given: the key-chunk protocol of the header (P = exp(S - lse), D = dvec); the dropout index counts
    the keys of THIS call. Returns a dict of float64 tensors."""
    B, n_q, _ = q.shape
    n_k = k.shape[1]
    qh, kh, vh = _split(q, heads), _split(k, heads), _split(v, heads)
    s = qh @ kh.transpose(-1, -2) * scale
    if mask is not None:
        s = s + mask[:, None, None, :]
    r = {"lse": torch.logsumexp(s, dim=-1)}
    P = torch.exp(s - (r["lse"] if lse is None else lse)[..., None])
    r["keep"] = torch.ones(B, heads, n_q, n_k, dtype=torch.bool)
    km = torch.ones_like(P)
    if p > 0:
        r["keep"] = torch.from_numpy(DR.keep(seed, DR.attention_index(B, heads, n_q, n_k), p))
        km = r["keep"].double() * float(DR.drop_scale(p))
    r["P"] = P
    r["probs"] = P * km
    r["O"] = _merge(r["probs"] @ vh)
    if d_out is not None:
        doh = _split(d_out, heads)
        dP = doh @ vh.transpose(-1, -2) * km
        r["D"] = (P * dP).sum(-1)
        dS = P * (dP - (r["D"] if dvec is None else dvec)[..., None]) * scale
        r["dQ"] = _merge(dS @ kh)
        r["dK"] = _merge(dS.transpose(-1, -2) @ qh)
        r["dV"] = _merge(r["probs"].transpose(-1, -2) @ doh)
    return r


class Problem:
    """Inputs of one call on the CPU in the build's dtype, and the float64 reference of the expanded tensors."""

    def __init__(self, build, d, n_q, n_k, masked, p, batch, q_batch, kv_batch):
        self.build, self.d, self.n_q, self.n_k, self.p = build, d, n_q, n_k, p
        self.batch, self.q_batch, self.kv_batch = batch, q_batch, kv_batch
        self.heads = _heads(d)
        self.H = self.heads * d
        self.scale = 1.0 / math.sqrt(d)
        dt, key = DTYPE[build], 1000 * n_q + n_k + d
        self.q = _rand(q_batch, n_q, self.H, seed=key, scale=0.7).to(dt)
        self.k = _rand(kv_batch, n_k, self.H, seed=key + 1, scale=0.7).to(dt)
        self.v = _rand(kv_batch, n_k, self.H, seed=key + 2, scale=0.7).to(dt)
        self.d_out = _rand(batch, n_q, self.H, seed=key + 3).to(dt)
        self.mask = _mask(kv_batch, n_k) if masked else None
        self.seed = SEED + key
        for t in (self.q, self.k, self.v, self.d_out):
            t.requires_grad_(False)

    def expanded(self, t):
        return t.double().expand(self.batch, -1, -1)

    @functools.cached_property
    def ref(self):
        mask = None if self.mask is None else self.mask.double().expand(self.batch, -1)
        return reference(self.expanded(self.q), self.expanded(self.k), self.expanded(self.v), mask, self.d_out.double(),
                         self.heads, float(np.float32(self.scale)), self.p, self.seed)

    def name(self):
        return "%s d=%d %dx%d%s%s" % (self.build, self.d, self.n_q, self.n_k, " mask" if self.mask is not None else "",
                                      " p=%.1f" % self.p if self.p else "")


@functools.lru_cache(maxsize=None)
def problem(build, d, n_q, n_k, masked=True, p=0.0, batch=2, q_batch=None, kv_batch=None):
    return Problem(build, d, n_q, n_k, masked, p, batch, q_batch or batch, kv_batch or batch)


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
def check32(got, want, what):
    """An fp32 tensor against float64: test_backward_gpu._close."""
    want = want.double()
    err = (got.double() - want).abs().max().item() if got.shape == want.shape else float("nan")
    print("parity %-58s max err %.3e  (bound %.3e)" % (what, err, 6e-5 * max(1.0, want.abs().max().item())))
    _close(got, want)


def check16(got, want, what):
    """A bf16 tensor against float64: the bounds of test_attention16_matches_the_fp32_kernels_on_the_same_values."""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    l2 = float((got - want).norm() / want.norm().clamp_min(1e-30))
    mx = float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))
    print("parity %-58s relative L2 %.3e  max err / range %.3e  (bounds 1.5e-02, 1.562e-02)" % (what, l2, mx))
    assert l2 <= 1.5e-2 and mx <= 2.0 ** -6, "%s: relative L2 %.3e, max error %.3e of the range" % (what, l2, mx)


def check_io(build, got, want, what):
    (check32 if build == "f32" else check16)(got, want, what)


def same_bits(a, b, what):
    ia, ib = (t.view(torch.int16 if t.dtype == BF16 else torch.int32) for t in (a, b))
    assert a.shape == b.shape and bool((ia == ib).all()), "%s: %d elements differ" % (what, int((ia != ib).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------
DENSE = {}


def _ld(lay, name, H):
    return H + lay.get(name, 0)


class Call:
    """Device buffers of one problem in one layout and the argument structs that point at them. lay: extra columns per row
    stride (ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv; default 0 = dense), `fused`: dQ | dK | dV as column slices of one
    [rows, 3H] buffer, `out_offset`: elements the gradients start into their buffers."""

    def __init__(self, pb, lay=DENSE, probs=False, lse="guard", chunk=None, dvec_mode=0):
        N = _N()
        self.pb, H, dt = pb, pb.H, DTYPE[pb.build]
        k, v, mask = pb.k, pb.v, pb.mask
        self.n_k, self.seed = pb.n_k, pb.seed
        if chunk is not None:                                 # keys [c0, c1) of the problem as a launch of their own
            c0, c1 = chunk
            k, v, mask = k[:, c0:c1], v[:, c0:c1], None if mask is None else mask[:, c0:c1].contiguous()
            self.n_k, self.seed = c1 - c0, pb.seed + 7919 * (c0 + 1)
        rq, rk = pb.batch * pb.n_q, pb.batch * self.n_k
        self.hold = [_input(pb.q, _ld(lay, "ldq", H)), _input(k, _ld(lay, "ldk", H)), _input(v, _ld(lay, "ldv", H)),
                     _input(pb.d_out, _ld(lay, "lddo", H)), None if mask is None else mask.to(DEV)]
        a = self.a = N.AttentionArgs()
        a.batch, a.heads, a.head_dim, a.n_q, a.n_k = pb.batch, pb.heads, pb.d, pb.n_q, self.n_k
        a.q_batch, a.kv_batch = pb.q_batch, pb.kv_batch
        a.Q, a.ldq = self.hold[0].data_ptr(), _ld(lay, "ldq", H)
        a.K, a.ldk = self.hold[1].data_ptr(), _ld(lay, "ldk", H)
        a.V, a.ldv = self.hold[2].data_ptr(), _ld(lay, "ldv", H)
        a.mask_add = None if mask is None else self.hold[4].data_ptr()
        a.scale, a.dropout_p, a.seed = pb.scale, pb.p, self.seed
        self.O, a.O = Guard.matrix(rq, H, _ld(lay, "ldo", H), dt)
        a.ldo = _ld(lay, "ldo", H)
        self.lse = Guard(pb.batch * pb.heads * pb.n_q, torch.float32)
        self.lse.region(0, pb.batch * pb.heads, pb.n_q, pb.n_q)
        a.lse = self.lse.t.data_ptr() if lse is not None else None
        self.probs = Guard(pb.batch * pb.heads * pb.n_q * self.n_k, torch.float32)
        self.probs.region(0, pb.batch * pb.heads * pb.n_q, self.n_k, self.n_k)
        a.probs = self.probs.t.data_ptr() if probs else None
        # backward
        g = self.g = N.AttentionGrads()
        g.dO, g.lddo = self.hold[3].data_ptr(), _ld(lay, "lddo", H)
        off = lay.get("out_offset", 0)
        if lay.get("fused"):
            rows = max(rq, rk)
            self.dq = self.dk = self.dv = fused = Guard(rows * 3 * H, dt)
            g.dQ, g.dK, g.dV = fused.region(0, rq, H, 3 * H), fused.region(H, rk, H, 3 * H), fused.region(2 * H, rk, H, 3 * H)
            g.lddq = g.lddk = g.lddv = 3 * H
        else:
            self.dq, g.dQ = Guard.matrix(rq, H, _ld(lay, "lddq", H), dt, off)
            self.dk, g.dK = Guard.matrix(rk, H, _ld(lay, "lddk", H), dt, off)
            self.dv, g.dV = Guard.matrix(rk, H, _ld(lay, "lddv", H), dt, off)
            g.lddq, g.lddk, g.lddv = (_ld(lay, n, H) for n in ("lddq", "lddk", "lddv"))
        self.dvec = Guard(pb.batch * pb.heads * pb.n_q, torch.float32)
        self.dvec.region(0, pb.batch * pb.heads, pb.n_q, pb.n_q)
        g.dvec, g.dvec_mode = self.dvec.t.data_ptr(), dvec_mode

    def outputs(self):
        seen = []
        for gd in (self.O, self.lse, self.probs, self.dq, self.dk, self.dv, self.dvec):
            if not any(gd is s for s in seen):
                seen.append(gd)
        return seen

    def fwd(self):
        return getattr(_N().lib(), FWD[self.pb.build])(_st(), ctypes.byref(self.a))

    def bwd(self):
        return getattr(_N().lib(), BWD[self.pb.build])(_st(), ctypes.byref(self.a), ctypes.byref(self.g))

    def set_lse(self, lse64):
        self.lse.fill(lse64.float())

    def forward(self, what):
        """Run the forward; returns (O [B, n_q, H], lse [B, heads, n_q] or None) on the CPU, guards checked."""
        pb = self.pb
        assert self.fwd() == 0, what
        out = self.O.fetch(what + " O")[0].reshape(pb.batch, pb.n_q, pb.H)
        lse = self.lse.fetch(what + " lse")[0].reshape(pb.batch, pb.heads, pb.n_q) if self.a.lse else None
        if not self.a.lse:
            self.lse.untouched(what + " lse (not asked for)")
        if not self.a.probs:
            self.probs.untouched(what + " probs (not asked for)")
        return out, lse

    def backward(self, what):
        """Run the backward (lse already in place); returns dQ, dK, dV on the CPU, guards checked."""
        pb = self.pb
        assert self.bwd() == 0, what
        if self.dq is self.dk:
            dq, dk, dv = self.dq.fetch(what + " fused dQ | dK | dV")
        else:
            dq, dk, dv = (gd.fetch(what + " " + nm)[0] for gd, nm in ((self.dq, "dQ"), (self.dk, "dK"), (self.dv, "dV")))
        self.dvec.fetch(what + " dvec")
        return (dq.reshape(pb.batch, pb.n_q, pb.H), dk.reshape(pb.batch, self.n_k, pb.H), dv.reshape(pb.batch, self.n_k, pb.H))


def run_fwd_bwd(pb, lay=DENSE, what=None):
    """Forward, then backward on the forward's own lse. Returns the dict of CPU results (O, lse, dQ, dK, dV)."""
    what = what or pb.name()
    c = Call(pb, lay)
    out, lse = c.forward(what)
    dq, dk, dv = c.backward(what)
    return {"O": out, "lse": lse, "dQ": dq, "dK": dk, "dV": dv}


def check_against_reference(pb, got, what, names=("O", "lse", "dQ", "dK", "dV")):
    for nm in names:
        if nm == "lse":
            check32(got[nm], pb.ref[nm], "%s lse" % what)
        else:
            check_io(pb.build, got[nm], pb.ref[nm], "%s %s" % (what, nm))


@functools.lru_cache(maxsize=None)
def dense_result(build, d, n_q, n_k, masked, p):
    return run_fwd_bwd(problem(build, d, n_q, n_k, masked, p))


# ---------------------------------------------------------------------------------------------------------------------
# every kernel family, dense layout
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [
    pytest.param(128, 36, 37, id="lds_fwd+fused_lds_bwd_over_v-128x36x37"),
    pytest.param(64, 16, 48, id="lds_fwd+fused_lds_bwd_over_v-64x16x48"),
    pytest.param(128, 48, 33, id="lds_fwd+fused_lds_bwd_over_v-128x48x33"),
    pytest.param(32, 17, 40, id="lds_fwd+fused_lds_bwd_own_block-32x17x40"),
    pytest.param(32, 1, 1, id="lds_fwd+fused_lds_bwd_over_v-32x1x1"),      # 2 x 1 x 8 floats of Pd | dS fit over one V row
    pytest.param(64, 49, 48, id="generic_nt3+bwd_kv-64x49x48"),
    pytest.param(32, 50, 17, id="generic_nt3+bwd_kv-32x50x17"),
    pytest.param(64, 20, 49, id="generic_nt8+bwd_kv-64x20x49"),
    pytest.param(128, 33, 128, id="generic_nt8+bwd_kv-128x33x128"),
    pytest.param(32, 17, 129, id="generic_nt20+bwd_kv-32x17x129"),
    pytest.param(64, 20, 320, id="generic_nt20+bwd_kv-64x20x320"),
]
LDS_SHAPES = [(128, 36, 37), (64, 16, 48), (128, 48, 33)]


def test_the_table_names_the_kernel_the_code_selects():
    """The ids above restate launch_bwd_fused_lds (over_v) and launch_q (the tile counts) - this keeps them honest."""
    for prm in SHAPES:
        d, n_q, n_k = prm.values
        lds = n_q <= 48 and n_k <= 48
        assert prm.id.startswith("lds_fwd") == lds
        if lds:
            ldp = (n_k + 3) // 4 * 4 + 4
            assert ("over_v" in prm.id) == (2 * n_q * ldp <= n_k * (d + 4)), prm.id
        else:
            n_kt = (n_k + 15) // 16
            assert "nt%d+" % (3 if n_kt <= 3 else 8 if n_kt <= 8 else 20) in prm.id, prm.id


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("d,n_q,n_k", SHAPES)
def test_forward_and_backward(d, n_q, n_k, build, masked):
    pb = problem(build, d, n_q, n_k, masked, 0.0)
    check_against_reference(pb, dense_result(build, d, n_q, n_k, masked, 0.0), pb.name())


# ---------------------------------------------------------------------------------------------------------------------
# strides
# ---------------------------------------------------------------------------------------------------------------------
STRIDED = {"ldq": 12, "ldk": 4, "ldv": 20, "ldo": 8, "lddo": 4, "lddq": 16, "lddk": 8, "lddv": 24}
FAMILY_SHAPES = [
    pytest.param(128, 36, 37, id="lds_over_v-128x36x37"),
    pytest.param(32, 17, 40, id="lds_own_block-32x17x40"),
    pytest.param(64, 49, 48, id="generic_nt3-64x49x48"),
    pytest.param(64, 20, 49, id="generic_nt8-64x20x49"),
    pytest.param(32, 17, 129, id="generic_nt20-32x17x129"),
]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("d,n_q,n_k", FAMILY_SHAPES)
def test_every_tensor_has_its_own_stride(d, n_q, n_k, build, p):
    """Q, K, V in three buffers with three strides (ldv > ldk), O with ldo = H + 8, dO with lddo = H + 4, three gradient
    strides; then dQ | dK | dV as column slices of one [rows, 3H] buffer. Bit for bit the dense call, which meets the
    float64 bounds."""
    pb = problem(build, d, n_q, n_k, True, p)
    dense = dense_result(build, d, n_q, n_k, True, p)
    check_against_reference(pb, dense, pb.name() + " dense")
    for lay, nm in ((STRIDED, "strided"), ({"fused": True, "ldq": 8, "ldk": 16, "ldv": 24}, "fused")):
        got = run_fwd_bwd(pb, lay, "%s %s" % (pb.name(), nm))
        for t in ("O", "lse", "dQ", "dK", "dV"):
            same_bits(got[t], dense[t], "%s %s: %s against the dense call" % (pb.name(), nm, t))


@pytest.mark.parametrize("d,n_q,n_k", [pytest.param(128, 36, 37, id="q_lds_bwd+bwd_kv_lds-128x36x37"),
                                       pytest.param(32, 17, 40, id="q_lds_bwd+bwd_kv_lds-32x17x40")])
def test_odd_output_strides_take_the_two_kernel_lds_backward(d, n_q, n_k):
    """fp32 outputs are stored one float at a time: any stride and any float pointer are legal (include/vilbert_hip.h).
    Strides that are not all multiples of 4 leave the fused backward for attn_q_lds_kernel<BWD> + attn_bwd_kv_lds_kernel."""
    pb = problem("f32", d, n_q, n_k, True, 0.1)
    lay = {"ldo": 1, "lddq": 1, "lddk": 3, "lddv": 5, "out_offset": 1}
    check_against_reference(pb, run_fwd_bwd(pb, lay, pb.name() + " odd strides"), pb.name() + " odd strides")


# ---------------------------------------------------------------------------------------------------------------------
# batch broadcast (forward only)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,q_batch,kv_batch", [(2, 1, 2), (2, 2, 1), (3, 1, 1)], ids=["q1", "kv1", "q1_kv1_batch3"])
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("d,n_q,n_k", [pytest.param(128, 12, 36, id="generic_nt3-128x12x36"),
                                       pytest.param(64, 20, 49, id="generic_nt8-64x20x49")])
def test_broadcast_forward(d, n_q, n_k, build, batch, q_batch, kv_batch):
    """One sample of queries for all, one sample of keys / values / MASK ROW for all, or both: the float64 attention of the
    expanded tensors. Broadcast leaves the LDS path (use_lds_path). The backward refuses it and writes nothing."""
    pb = problem(build, d, n_q, n_k, True, 0.0, batch, q_batch, kv_batch)
    what = "%s broadcast q_batch=%d kv_batch=%d batch=%d" % (pb.name(), q_batch, kv_batch, batch)
    c = Call(pb)
    out, lse = c.forward(what)
    check_io(build, out, pb.ref["O"], what + " O")
    check32(lse, pb.ref["lse"], what + " lse")
    c2 = Call(pb)
    c2.set_lse(pb.ref["lse"])
    assert c2.bwd() == E_BADARG
    for gd in (c2.O, c2.probs, c2.dq, c2.dk, c2.dv, c2.dvec):
        gd.untouched(what + " backward")


# ---------------------------------------------------------------------------------------------------------------------
# lse and probs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("d,n_q,n_k", [pytest.param(128, 36, 37, id="lds-128x36x37"), pytest.param(64, 20, 49, id="generic_nt8-64x20x49")])
def test_probs_and_lse_under_dropout(d, n_q, n_k, build):
    """dropout_p = 0.5: zeros exactly where the host restatement of the mask drops, P / (1 - p) elsewhere; lse rows (n_q no
    multiple of 16) in a guard; and the optional outputs are optional - without them the same context."""
    pb = problem(build, d, n_q, n_k, True, 0.5)
    what = pb.name() + " probs"
    c = Call(pb, probs=True)
    out, lse = c.forward(what)
    probs = c.probs.fetch(what)[0].reshape(pb.batch, pb.heads, n_q, n_k)
    keep = pb.ref["keep"]
    assert 0.4 < keep.float().mean().item() < 0.6
    assert bool((probs[~keep] == 0).all()), "a dropped probability is not zero"
    assert bool((probs[keep & (pb.ref["P"] > 1e-30)] > 0).all()), "a kept probability is zero"
    check32(probs, pb.ref["probs"], what)
    check32(lse, pb.ref["lse"], what + " lse")
    check_io(build, out, pb.ref["O"], what + " O")
    bare = Call(pb, lse=None)
    out2, lse2 = bare.forward(what + " (no probs, no lse)")
    assert lse2 is None
    same_bits(out2, out, what + ": the context without the optional outputs")


# ---------------------------------------------------------------------------------------------------------------------
# dvec_mode: key chunks of a longer sequence
# ---------------------------------------------------------------------------------------------------------------------
CHUNKED = [
    pytest.param(64, 20, 40, 17, id="generic_nt3+bwd_kv_lds-64x20x(17+23)"),
    pytest.param(64, 20, 49, 30, id="generic_nt3+bwd_kv_lds-64x20x(30+19)"),
    pytest.param(128, 33, 129, 49, id="generic_nt8+bwd_kv-128x33x(49+80)"),
]


def _chunk_ref(pb, chunk, p, seed, dvec=None):
    """float64 reference of ONE chunk's launch: P from the log-sum-exp over all keys, the chunk's own dropout indices."""
    c0, c1 = chunk
    mask = None if pb.mask is None else pb.mask.double()[:, c0:c1]
    return reference(pb.q.double(), pb.k.double()[:, c0:c1], pb.v.double()[:, c0:c1], mask, pb.d_out.double(), pb.heads,
                     float(np.float32(pb.scale)), p, seed, lse=pb.ref["lse"], dvec=dvec)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("d,n_q,n_k,cut", CHUNKED)
def test_dvec_accumulate_adds_the_chunk_share_and_writes_nothing_else(d, n_q, n_k, cut, build):
    pb = problem(build, d, n_q, n_k, True, 0.1)
    for chunk in ((0, cut), (cut, n_k)):
        what = "%s ACCUMULATE keys %d..%d" % (pb.name(), chunk[0], chunk[1])
        c = Call(pb, chunk=chunk, dvec_mode=_N().DVEC_ACCUMULATE)
        c.set_lse(pb.ref["lse"])
        before = _rand(pb.batch, pb.heads, n_q, seed=chunk[0] + 5, scale=3.0) + 0.5
        c.dvec.fill(before)
        assert c.bwd() == 0
        got = c.dvec.fetch(what)[0].reshape(pb.batch, pb.heads, n_q)
        check32(got, before.double() + _chunk_ref(pb, chunk, pb.p, c.seed)["D"], what + " dvec")
        for gd in (c.dq, c.dk, c.dv, c.O, c.probs):
            gd.untouched(what)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("d,n_q,n_k,cut", CHUNKED)
def test_dvec_given_is_used_as_given(d, n_q, n_k, cut, build):
    """A D vector that is NOT rowsum(P dP) of anything the kernel could compute: the true one plus an offset of order 1 per
    row. dS = P (dP - D_given) scale; a kernel that recomputes D fails."""
    pb = problem(build, d, n_q, n_k, True, 0.1)
    given = pb.ref["D"] + (_rand(pb.batch, pb.heads, n_q, seed=77) + 1.5).double()
    given = given.float()
    for chunk in ((0, cut), (cut, n_k)):
        what = "%s GIVEN keys %d..%d" % (pb.name(), chunk[0], chunk[1])
        c = Call(pb, chunk=chunk, dvec_mode=_N().DVEC_GIVEN)
        c.set_lse(pb.ref["lse"])
        c.dvec.fill(given)
        dq, dk, dv = c.backward(what)
        assert bool((c.dvec.fetch(what)[0].reshape(given.shape) == given).all()), "the given D vector was overwritten"
        want = _chunk_ref(pb, chunk, pb.p, c.seed, dvec=given.double())
        for got, nm in ((dq, "dQ"), (dk, "dK"), (dv, "dV")):
            check_io(build, got, want[nm], "%s %s" % (what, nm))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("d,n_q,n_k,cut", CHUNKED)
def test_two_pass_protocol_over_two_unequal_chunks(d, n_q, n_k, cut, build):
    """ACCUMULATE over both chunks into a zeroed dvec, then GIVEN per chunk: the summed dQ shares and the concatenated
    dK / dV against the float64 backward of ONE launch over all keys."""
    pb = problem(build, d, n_q, n_k, True, 0.0)
    what = "%s two-pass %d+%d" % (pb.name(), cut, n_k - cut)
    chunks = ((0, cut), (cut, n_k))
    calls = [Call(pb, chunk=ch) for ch in chunks]
    dvec = calls[0].dvec
    dvec.fill(torch.zeros(pb.batch, pb.heads, n_q))
    for c in calls:
        c.set_lse(pb.ref["lse"])
        c.g.dvec, c.g.dvec_mode = dvec.t.data_ptr(), _N().DVEC_ACCUMULATE
        assert c.bwd() == 0
    check32(dvec.fetch(what)[0].reshape(pb.batch, pb.heads, n_q), pb.ref["D"], what + " dvec")
    shares, dks, dvs = [], [], []
    for c in calls:
        c.g.dvec_mode = _N().DVEC_GIVEN
        assert c.bwd() == 0
        shares.append(c.dq.fetch(what)[0].reshape(pb.batch, n_q, pb.H))
        dks.append(c.dk.fetch(what)[0].reshape(pb.batch, c.n_k, pb.H))
        dvs.append(c.dv.fetch(what)[0].reshape(pb.batch, c.n_k, pb.H))
    if build == "f32":
        check32(shares[0] + shares[1], pb.ref["dQ"], what + " dQ (sum of the shares)")
    else:                                   # the caller's sum of two bf16 shares, in fp32 as ops._attention_bwd_long does
        check16(shares[0].float() + shares[1].float(), pb.ref["dQ"], what + " dQ (sum of the shares)")
    check_io(build, torch.cat(dks, 1), pb.ref["dK"], what + " dK")
    check_io(build, torch.cat(dvs, 1), pb.ref["dV"], what + " dV")


# ---------------------------------------------------------------------------------------------------------------------
# error returns
# ---------------------------------------------------------------------------------------------------------------------
def _refusals(build):
    """(name, expected code, forward?, mutate(call)) - every refused call of the header, on a (64, 20, 40) problem."""
    es = 4 if build == "f32" else 2
    nan32 = float("nan")
    out = []

    def add(name, code, where, fn):
        out.append((name, code, where, fn))

    def seta(**kw):
        def fn(c):
            for k, v in kw.items():
                setattr(c.a, k, v)
        return fn

    def setg(**kw):
        def fn(c):
            for k, v in kw.items():
                setattr(c.g, k, v)
        return fn

    def move(struct, field, n):
        def fn(c):
            s = getattr(c, struct)
            setattr(s, field, getattr(s, field) + n * es)
        return fn

    add("NULL a", E_BADARG, "both", lambda c: setattr(c, "null_a", True))
    for f in ("Q", "K", "V"):
        add("NULL " + f, E_BADARG, "both", seta(**{f: None}))
    add("NULL O", E_BADARG, "fwd", seta(O=None))
    for f in ("batch", "heads", "n_q", "n_k"):
        for val in (0, -1):
            add("%s = %d" % (f, val), E_BADARG, "both", seta(**{f: val}))
    for f in ("q_batch", "kv_batch"):
        for val in (0, 3):
            add("%s = %d" % (f, val), E_BADARG, "both", seta(**{f: val}))
    for val in (-0.1, 1.0, nan32):
        add("dropout_p = %r" % val, E_BADARG, "both", seta(dropout_p=val))
    add("NULL gr", E_BADARG, "bwd", lambda c: setattr(c, "null_g", True))
    for f in ("dO", "dQ", "dK", "dV", "dvec"):
        add("NULL " + f, E_BADARG, "bwd", setg(**{f: None}))
    add("NULL lse", E_BADARG, "bwd", seta(lse=None))
    for val in (-1, 3):
        add("dvec_mode = %d" % val, E_BADARG, "bwd", setg(dvec_mode=val))
    add("n_k = 321", E_RANGE, "both", seta(n_k=321))
    for val in (16, 48, 256):
        add("head_dim = %d" % val, E_RANGE, "both", seta(head_dim=val))
    for f in ("ldq", "ldk", "ldv"):
        for extra in (1, 2, 3):
            add("%s = H + %d" % (f, extra), E_ALIGN, "both", (lambda f, extra: lambda c: setattr(c.a, f, c.pb.H + extra))(f, extra))
    for extra in (1, 2, 3):
        add("lddo = H + %d" % extra, E_ALIGN, "bwd", (lambda extra: lambda c: setattr(c.g, "lddo", c.pb.H + extra))(extra))
    shifts = (1,) if build == "f32" else (1, 2, 3)
    for n in shifts:
        for f in ("Q", "K", "V"):
            add("%s moved by %d" % (f, n), E_ALIGN, "both", move("a", f, n))
        add("dO moved by %d" % n, E_ALIGN, "bwd", move("g", "dO", n))
    if build == "bf16":                     # the outputs of the bf16 build: two columns per dword (store_cols)
        for n in (1, 2, 3):
            add("O moved by %d" % n, E_ALIGN, "fwd", move("a", "O", n))
            add("ldo = H + %d" % n, E_ALIGN, "fwd", (lambda n: lambda c: setattr(c.a, "ldo", c.pb.H + n))(n))
            for f, ld in (("dQ", "lddq"), ("dK", "lddk"), ("dV", "lddv")):
                add("%s moved by %d" % (f, n), E_ALIGN, "bwd", move("g", f, n))
                add("%s = H + %d" % (ld, n), E_ALIGN, "bwd", (lambda ld, n: lambda c: setattr(c.g, ld, c.pb.H + n))(ld, n))
    return out


@pytest.mark.parametrize("build", BUILDS)
def test_refused_calls_write_nothing(build):
    """Every argument error of include/vilbert_hip.h, forward and backward: the code, and every guarded output untouched
    (the buffers are those of a valid call, with room behind every stride that is tried)."""
    pb = problem(build, 64, 20, 40, True, 0.0)
    lay = {n: 4 for n in ("ldq", "ldk", "ldv", "ldo", "lddo", "lddq", "lddk", "lddv")}
    lib = _N().lib()
    n_checked = 0
    for name, code, where, mutate in _refusals(build):
        for direction in ("fwd", "bwd"):
            if where not in ("both", direction):
                continue
            c = Call(pb, lay, probs=True)
            c.null_a = c.null_g = False
            c.set_lse(pb.ref["lse"])
            lse_bits = c.lse.t.clone()
            mutate(c)
            a = None if c.null_a else ctypes.byref(c.a)
            if direction == "fwd":
                rc = getattr(lib, FWD[build])(_st(), a)
            else:
                rc = getattr(lib, BWD[build])(_st(), a, None if c.null_g else ctypes.byref(c.g))
            what = "%s %s: %s" % (build, direction, name)
            assert rc == code, "%s returned %d, not %d" % (what, rc, code)
            for gd in (c.O, c.probs, c.dq, c.dk, c.dv, c.dvec):
                gd.untouched(what)
            c.lse.fetch(what)
            assert torch.equal(c.lse.t, lse_bits), "%s: wrote lse" % what
            n_checked += 1
    print("parity %s: %d refused calls, every output untouched" % (build, n_checked))


def test_the_valid_call_of_the_refusal_test_is_accepted():
    """The unmutated arguments of test_refused_calls_write_nothing run, both builds: the refusals are the mutations'."""
    for build in BUILDS:
        pb = problem(build, 64, 20, 40, True, 0.0)
        lay = {n: 4 for n in ("ldq", "ldk", "ldv", "ldo", "lddo", "lddq", "lddk", "lddv")}
        check_against_reference(pb, run_fwd_bwd(pb, lay, pb.name() + " ld + 4"), pb.name() + " ld + 4")


# ---------------------------------------------------------------------------------------------------------------------
# VB_ATTN_LDS=0: the generic kernels on the short shapes, in a process of their own
# ---------------------------------------------------------------------------------------------------------------------
CHILD_OK = "generic kernels on the LDS shapes: ok"


def _generic_kernels_on_the_lds_shapes():
    for d, n_q, n_k in LDS_SHAPES:
        for build in BUILDS:
            pb = problem(build, d, n_q, n_k, True, 0.1)
            check_against_reference(pb, run_fwd_bwd(pb, STRIDED, pb.name()), pb.name() + " VB_ATTN_LDS=0")
    print(CHILD_OK)


def test_generic_kernels_serve_the_short_shapes_in_a_child_process():
    """VB_ATTN_LDS is read once per process, so attn_q_kernel<3> / attn_bwd_kv_kernel at n <= 48 get a process of their own:
    this file run as a script with the variable set. The child has its own time limit; its exit status and its last line
    are checked, its parity lines are passed on."""
    env = dict(os.environ, VB_ATTN_LDS="0")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "generic-on-lds-shapes"], env=env, timeout=240,
                          capture_output=True, text=True)
    print("\n".join(l for l in done.stdout.splitlines() if l.startswith("parity")))
    assert done.returncode == 0 and done.stdout.strip().endswith(CHILD_OK), \
        "exit status %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])


if __name__ == "__main__":
    assert sys.argv[1:] == ["generic-on-lds-shapes"] and os.environ.get("VB_ATTN_LDS") == "0"
    _generic_kernels_on_the_lds_shapes()
