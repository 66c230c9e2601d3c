"""A host restatement of the arithmetic of the bf16-plane GEMM modes (csrc/gemm_planes.hip) and of the launch decisions the
direct tests of that kernel rely on (csrc/gemm_plan.h). Test infrastructure: tests/test_gemm_planes_host.py pins it (the plane
split is exact, the restated arithmetic stays under a fifth of every mode's bound on the inputs the GPU tests use, the tile /
split rules equal the header's, compiled for the host); tests/test_gemm_planes_gpu.py then uses it to tell, when a launch misses
its bound, whether the kernel or the arithmetic moved.

    split8:  x = x0 + x1 (+ x2),  x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)    round to nearest even, fp32 residuals
    kstep:   bf16x6 (3 planes)  a2b0 a0b2 a1b1 a1b0 a0b1 a0b0
             bf16x3 (2 planes)  a1b0 a0b1 a0b0
             bf16   (1 plane)   a0b0
every product exact (bf16 x bf16 fits fp32), accumulated in fp32 by the matrix cores - in float64 here, so what this file
computes is the arithmetic WITHOUT the accumulation error (about 4e-7 of the result's scale at these lengths).
"""
import torch

PLANES = {"f32": 0, "bf16x6": 3, "bf16x3": 2, "bf16": 1}
PRODUCTS = {3: ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)), 2: ((1, 0), (0, 1), (0, 0)), 1: ((0, 0),)}
# tests/test_gemm_modes_gpu.py _check / _check_bf16: |got - want| <= BOUND * max(1, max|want|)
BOUND = {"f32": 3e-5, "bf16x6": 3e-5, "bf16x3": 6e-4, "bf16": 2.0 ** -6}


def split(x, planes):
    """fp32 tensor -> list of `planes` fp32 tensors holding bf16 values: split8 of gemm_planes.hip."""
    assert x.dtype == torch.float32
    out, r = [], x.clone()
    for pl in range(planes):
        p = r.to(torch.bfloat16).float()
        out.append(p)
        if pl + 1 < planes:
            r = r - p
    return out


def matmul(a, b, mode):
    """float64 [m, n]: a [m, k] times b [k, n] (fp32 tensors) in the arithmetic of `mode`, without accumulation error."""
    planes = PLANES[mode]
    if planes == 0:
        return a.double() @ b.double()
    pa, pb = [p.double() for p in split(a, planes)], [p.double() for p in split(b, planes)]
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float64)
    for i, j in PRODUCTS[planes]:
        acc += pa[i] @ pb[j]
    return acc


def arithmetic_error(a, b, mode):
    """max |restated product - exact product| relative to max(1, max |exact|): the figure BOUND[mode] is about."""
    want = a.double() @ b.double()
    return float((matmul(a, b, mode) - want).abs().max()) / max(1.0, float(want.abs().max()))


# ---- the input families of tests/test_gemm_planes_gpu.py -----------------------------------------------------------------------
def rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


FAMILIES = {"linear": (1.0, 0.1),      # activations / gradients N(0, 1) against weights N(0, 0.1)
            "decoder": (0.1, 0.05)}    # the MLM decoder's hidden states against its embedding rows


def operands(family, m, n, k, seed=0):
    """(a [m, k], b [n, k]) of a family: the two GEMM operands, contraction along the last dimension."""
    sa, sb = FAMILIES[family]
    return rand(m, k, seed=seed + 1, scale=sa), rand(n, k, seed=seed + 2, scale=sb)


# ---- launch decisions (csrc/gemm_plan.h) ---------------------------------------------------------------------------------------
def tile_census(m, n, splits=1, planes_mode=True, cseg=None):
    """plan_tiles: (n_big 128 x 128 blocks, n_small 64 x 64 blocks) of an [m, n] output on the round-1 / bf16-plane kernels."""
    cseg = (m + 127) // 128 * 128 if cseg is None else cseg
    total = ((m + 127) // 128) * ((n + 127) // 128)
    left = total % 256
    limit = 2 if planes_mode else 4
    recut = splits == 1 and left > 0 and (4 * left + 255) // 256 < limit and cseg % 64 == 0
    return (total - left, 4 * left) if recut else (total, 0)


def wgrad_splits(tiles, kt_total, rmax=4):
    """plan_wgrad_splits: split count of a weight gradient of `tiles` 128 x 128 tiles over kt_total 16-row K tiles."""
    splits, best = 1, -1.0
    for r in range(rmax, 1, -1):
        s = max(1, (256 * r) // tiles)
        if s > kt_total // 4:
            s = kt_total // 4 if kt_total // 4 > 0 else 1
        blocks = tiles * s
        fill = blocks / (256.0 * ((blocks + 255) // 256))
        if fill > best + 1e-9:
            best, splits = fill, s
        if fill >= 0.93:
            break
    return splits


def dgrad_splits(m, n, k):
    """plan_planes_dgrad_splits: split count of the split-K input gradient in the plane modes."""
    tiles = ((m + 127) // 128) * ((n + 127) // 128)
    sp = min((768 + tiles - 1) // tiles, k // 1024)
    return max(1, min(32, sp))


# ---- the shape table of tests/test_gemm_planes_gpu.py --------------------------------------------------------------------------
# (output rows, output columns, contraction, (n_big, n_small) in the plane modes, (n_big, n_small) of the round-1 fp32 kernel)
SHAPES = {
    "small_vec": (100, 200, 52, (0, 8), (0, 8)),              # all 64 x 64, ragged, 16-byte loads
    "small_scalar": (100, 200, 37, (0, 8), (0, 8)),           # all 64 x 64, ragged, scalar loads
    "big_full": (640, 1664, 32, (65, 0), (0, 260)),           # all 128 x 128, every tile interior, K % 16 == 0 (FULL)
    "big_ragged": (600, 1700, 40, (70, 0), (0, 280)),         # all 128 x 128, ragged edges, a half K tile
    "big_ragged_scalar": (600, 1700, 37, (70, 0), (0, 280)),
    "mixed": (256, 16512, 16, (256, 8), (256, 8)),            # one round of 128 x 128 and 2 leftover tiles re-cut
    "mixed_ragged": (256, 16500, 16, (256, 8), (256, 8)),
    "one": (1, 1, 4, (0, 4), (0, 4)),
}

# every problem of that file: name -> (family, rows of a, rows of b, contraction); the operands are problem(name). The eight
# shapes above are the forward launches x [M, K] w [N, K] and the input gradients dY [M, contraction] W^T [K_in, contraction];
# weight gradients are a = dY^T [nseg seg_n, rows], b = X^T [K, rows].
PROBLEMS = {name: ("linear",) + v[:3] for name, v in SHAPES.items()}
PROBLEMS.update({
    "decoder_fwd": ("decoder", 100, 200, 52),
    "seg": ("linear", 100, 192, 52),                  # 1 .. 4 weight segments of 192 / 96 / 64 / 48 columns, 64 x 64 tiles
    "seg_big": ("linear", 768, 1536, 64),             # the same on 72 tiles of 128 x 128
    "dgrad_seg48": ("linear", 100, 200, 144),         # 3 segments of 48 stacked along the contraction: one launch
    "dgrad_seg20": ("linear", 100, 200, 60),          # 3 segments of 20: one launch per segment
    "dgrad_ragged": ("linear", 100, 200, 264),        # contraction 264 = bulk 256 + tail 8
    "dgrad_splitk": ("decoder", 64, 64, 4096),
    "dgrad_splitk_ragged": ("decoder", 64, 64, 4100),
    "wgrad_recut": ("linear", 100, 200, 48),
    "wgrad_split4": ("linear", 128, 128, 256),
    "wgrad_ragged_rows": ("linear", 128, 128, 263),   # rows 263 = bulk 256 + tail 7
    "wgrad_seg128": ("linear", 384, 200, 48),
    "wgrad_seg128_split": ("linear", 384, 200, 256),
    "wgrad_seg96": ("linear", 288, 200, 48),
    "wgrad_odd": ("linear", 61, 200, 48),             # ldy = seg_n + 2, seg_n odd
    "wgrad_pad2": ("linear", 122, 200, 272),          # ldy = seg_n + 2, seg_n % 4 == 2: the 30522 / 30524 form
    "wgrad_skinny": ("linear", 128, 5, 300),
})


# a ragged twin is cut out of its aligned problem (same draw, fewer columns)
TWINS = {"mixed_ragged": "mixed"}


def problem(name):
    """The operands (a [m, k], b [n, k]) of a problem: a fixed draw per name. (In the one-plane mode the arithmetic error of
    such a draw sits at 2.1e-3 .. 3.0e-3 of the scale for contractions of 16 .. 64 - close to the fifth of 2^-6 that
    tests/test_gemm_planes_host.py requires of every problem, which is why that test looks at every one of them.)"""
    family, m, n, k = PROBLEMS[name]
    if name in TWINS:
        a, b = problem(TWINS[name])
        assert a.shape == (m, k) and b.shape[0] >= n
        return a, b[:n].contiguous()
    return operands(family, m, n, k, seed=100 * list(PROBLEMS).index(name))
