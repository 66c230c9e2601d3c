"""SHA-256 of every output tensor of the LayerNorm / embedding row kernels (csrc/layernorm.hip, embed.hip) over a fixed seed
and shape list - run it on two builds of the library and diff the outputs: identical lines = identical bits. Only vilbert.ops /
vilbert.ops16 calls. Rows cross the partial last wave, the rows < 4096 rule and the 2-versus-4 rows-per-wave rule of both bf16
launchers ((16400 + 7) / 8 > 2048); the MX forms take only their legal widths (cols % 128 == 0)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vilbert-multi-task_amd"))
from vilbert import _native, ops, ops16  # noqa: E402

dev = "cuda:0"
ROWS = (1, 5, 17, 4100, 16400)
COLS16 = (64, 260, 768, 1024)
COLS32 = COLS16 + (2048, 5000, 8192)


def sha(t):
    t = t.detach().contiguous()
    raw = t.view(torch.uint8) if t.dtype != torch.uint8 else t
    return hashlib.sha256(raw.cpu().numpy().tobytes()).hexdigest()[:16]


def show(tag, rows, cols, outs):
    torch.cuda.synchronize()
    print("%-22s %6d x %4d  %s" % (tag, rows, cols, " ".join("-" if o is None else o if isinstance(o, str) else sha(o) for o in outs)), flush=True)


def mx_codes(y):
    m = y._vb_mx[0]
    return [y, m.q, m.s]


g = torch.Generator().manual_seed(1234)
for rows in ROWS:
    for cols in COLS32:
        x = torch.randn(rows, cols, generator=g).to(dev)
        x2 = torch.randn(rows, cols, generator=g).to(dev)
        dy = torch.randn(rows, cols, generator=g).to(dev)
        gam, bet = (1 + 0.1 * torch.randn(cols, generator=g)).to(dev), (0.1 * torch.randn(cols, generator=g)).to(dev)
        with torch.enable_grad():     # (the code-emitting forms are inference-only)
            show("f32 fwd", rows, cols, ops.layernorm_fwd(x, gam, bet, 1e-12))
            y, mean, rstd = ops.layernorm_fwd(x, gam, bet, 1e-12, x2=x2, want_stats=True)
            show("f32 fwd x2 stats", rows, cols, (y, mean, rstd))
        show("f32 bwd", rows, cols, ops.layernorm_bwd(dy, x + x2, mean, rstd, gam))
        if cols <= 4096:
            show("f32 bwd drop", rows, cols, ops.layernorm_bwd(dy, x + x2, mean, rstd, gam, drop=(0.1, 7)))
        with torch.no_grad():
            if cols % 16 == 0:
                prev = _native.set_gemm_mode("fp8")
                y = ops.layernorm_fwd(x, gam, bet, 1e-12, x2=x2)[0]
                show("f32 fwd fp8 codes", rows, cols, (y,) + tuple(y._vb_fp8[:2]) if hasattr(y, "_vb_fp8") else (y, "no-codes"))
                _native.set_gemm_mode(prev)
            if cols % 128 == 0:
                prev = _native.set_gemm_mode("mxfp8")
                y = ops.layernorm_fwd(x, gam, bet, 1e-12, x2=x2)[0]
                show("f32 fwd mx codes", rows, cols, mx_codes(y) if hasattr(y, "_vb_mx") else (y, "no-codes"))
                if cols in COLS16 or cols == 2048:
                    y = ops.layernorm_fwd(x.to(torch.bfloat16), gam, bet, 1e-12)[0]
                    show("mx16 fwd", rows, cols, mx_codes(y))
                _native.set_gemm_mode(prev)
        if cols in COLS16:
            x16, dy16 = x.to(torch.bfloat16), dy.to(torch.bfloat16)
            y, mean, rstd = ops16.layernorm_fwd(x16, gam, bet, 1e-12, want_stats=True)
            show("bf16 fwd stats", rows, cols, (y, mean, rstd))
            show("bf16 bwd", rows, cols, ops16.layernorm_bwd(dy16, x16, mean, rstd, gam))
            show("bf16 bwd drop", rows, cols, ops16.layernorm_bwd(dy16, x16, mean, rstd, gam, drop=(0.1, 7)))

# embeddings: batch x tokens rows; the backward in the non-deterministic setting on ids without repeats (atomics order cannot matter)
for batch, n_tok, hidden in ((1, 5, 64), (3, 7, 260), (16, 36, 768), (4, 9, 1024), (2, 3, 2048)):
    vocab = batch * n_tok + 8
    word, pos, typ = (torch.randn(n, hidden, generator=g).to(dev) for n in (vocab, n_tok, 2))
    task_emb = torch.randn(4, hidden, generator=g).to(dev)
    gam, bet = (1 + 0.1 * torch.randn(hidden, generator=g)).to(dev), (0.1 * torch.randn(hidden, generator=g)).to(dev)
    ids = (1 + torch.randperm(vocab - 1, generator=g)[:batch * n_tok]).view(batch, n_tok).to(dev)
    seg = torch.randint(0, 2, (batch, n_tok), generator=g).to(dev)
    task_ids = torch.arange(batch).remainder(4).to(dev)   # (repeats only where batch > 4: left out of the backward below)
    for tag, tk, te in (("text embed", None, None), ("text embed + task", task_ids, task_emb)):
        show(tag, batch * n_tok, hidden, ops.text_embed_ln_fwd(ids, seg, word, pos, typ, gam, bet, 1e-12, task_ids=tk,
                                                                task_emb=te, want_stats=True))
    feat = torch.randn(batch, n_tok, hidden, generator=g).to(dev)
    loc, w_loc, b_loc = torch.rand(batch, n_tok, 5, generator=g).to(dev), torch.randn(hidden, 5, generator=g).to(dev), \
        torch.randn(hidden, generator=g).to(dev)
    show("image embed", batch * n_tok, hidden, ops.image_embed_ln_fwd(feat, loc, w_loc, b_loc, gam, bet, 1e-12, want_stats=True))
    dx = torch.randn(batch, n_tok, hidden, generator=g).to(dev)
    prev = _native.set_deterministic(False)
    try:
        # atomics meet where gradient rows share a table row: one sample keeps dword (distinct ids) and dpos (one row per
        # position) single-term; dtype sums over the positions of a type, so it is hashed from two tokens of types 0 and 1
        outs = ops.text_embed_bwd(dx[:1], ids[:1], seg[:1], None, word.shape, pos.shape, typ.shape, None)
        two = ops.text_embed_bwd(dx[:1, :2], ids[:1, :2], torch.tensor([[0, 1]], device=dev), None, word.shape, pos.shape,
                                 typ.shape, None)
    finally:
        _native.set_deterministic(prev)
    show("text embed bwd", n_tok, hidden, outs[:2] + two[:3])
