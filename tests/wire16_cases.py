"""Inputs shared by tests/test_wire16.py (CPU) and tests/test_wire16_gpu.py: float16 arrays with full mantissas and the special
values a widening can get wrong, and the one masking case both files must agree on (the CPU file checks that it is not empty,
the GPU file runs it)."""
import numpy as np

import masking_restatement as mr

VOCAB, MASK_ID = 30522, 103
# GPU test 3 (fused row clearing): B, T, R, F, p_select, data seed, masking seed
MASK_CASE = dict(B=4, T=9, R=7, F=16, p=0.5, data_seed=1, seed=0x5EED16, n_box=[7, 5, 3, 6])
SPECIALS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x3C00, 0x3555], dtype=np.uint16)
#                    +0      -0      smallest subnormals   largest subnormals  2^-14  +-65504        1.0     ~1/3


def f16_values(shape, seed):
    """float16 array of `shape`: random 16-bit patterns (every exponent, full mantissas, both signs) with the non-finite ones
    replaced, and SPECIALS written over the leading elements (as many as fit)."""
    g = np.random.RandomState(seed)
    bits = g.randint(0, 1 << 16, size=int(np.prod(shape))).astype(np.uint16)
    nonfinite = (bits & 0x7C00) == 0x7C00
    bits[nonfinite] &= np.uint16(0xBFFF)                    # exponent 30 instead of 31: a large finite value
    k = min(len(SPECIALS), bits.size)
    bits[:k] = SPECIALS[:k]
    x = bits.view(np.float16).reshape(shape)
    assert np.isfinite(x).all()
    return x


def widen(x):
    """The exact fp32 values of a float16 array (numpy's cast is exact: every binary16 is an fp32)."""
    return np.asarray(x, dtype=np.float16).astype(np.float32)


def mask_case_raw():
    """The unmasked batch of MASK_CASE with fp32 features that ARE float16 values (so narrowing them loses nothing)."""
    c = MASK_CASE
    raw = mr.make_unmasked_batch(c["B"], tokens=c["T"], regions=c["R"], feat_dim=c["F"], n_classes=5, vocab=VOCAB,
                                 seed=c["data_seed"], n_box=c["n_box"])
    feat = f16_values(raw["image_feat"].shape, c["data_seed"] + 100)
    raw["image_feat"] = widen(feat)
    return raw, feat


def mask_case_flags(raw):
    c = MASK_CASE
    return mr.mask_arrays(raw["input_ids"], raw["input_mask"], raw["image_mask"], raw["overlaps"], c["seed"], VOCAB, MASK_ID,
                          c["p"])["zero_row"]
