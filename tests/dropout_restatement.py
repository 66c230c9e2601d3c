"""A restatement of the dropout mask of every kernel (`csrc/rng.h`) in numpy, and of the element index each site feeds it
(`include/vilbert_hip.h`). Test infrastructure: tests/test_dropout_mask.py pins it bit for bit against the header itself
(compiled for the host, tests/rng_driver.cpp); tests/test_dropout_mask_gpu.py then holds every kernel that draws a mask to it, so
no GPU test has to read the mask off the kernel it is checking.

    hash(seed, i) = upper 32 bits of the splitmix64 finaliser of seed + i * 0x9E3779B97F4A7C15     (uint64, wrapping)
    u             = float32(hash >> 8) * float32(2^-24)                                            (exact: 24 bits)
    keep(seed, i, p) = u >= float32(p)                  survivors are multiplied by float32(1) / (float32(1) - float32(p))
    a registered device step counter e turns the launch seed into seed + e * 0xD1B54A32D192ED03    (uint64, wrapping)

Element index i of a site:
    vb_dropout                          the flat element index
    linear epilogues (fp32, bf16, fp8)  row * N + col, N = ALL output columns of the launch (nseg * seg_n)
    LayerNorm backward twin             row * n_cols + col (= the index of the linear in front of the LayerNorm)
    attention                           ((b * heads + h) * n_q + q) * n_k + key, n_k = the key count OF THE LAUNCH (a key chunk of
                                        a longer sequence counts its own keys from 0 and has its own seed, ops._chunk_seed)
"""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)        # stride of the element index inside the hash
EPOCH_STRIDE = 0xD1B54A32D192ED03             # stride of the device step counter inside the seed
MASK64 = 0xFFFFFFFFFFFFFFFF


def _u64(x):
    """Python ints (any size below 2^64), numpy integers or arrays of either -> uint64 array (no sign trouble for the top bit)."""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64, copy=False)
    if isinstance(x, (list, tuple)):
        return np.array([int(v) & MASK64 for v in x], dtype=np.uint64)
    return np.array(int(x) & MASK64, dtype=np.uint64)


def vb_hash(seed, idx):
    """uint32 array: rng.h vb_hash over broadcast (seed, idx)."""
    with np.errstate(over="ignore"):
        z = _u64(seed) + _u64(idx) * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def keep(seed, idx, p):
    """bool array: rng.h vb_keep - True where the element survives (probability 1 - p)."""
    u = (vb_hash(seed, idx) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.asarray(p, dtype=np.float32)


def drop_scale(p):
    """What a survivor is multiplied by, as the launchers compute it: fp32 1 / (1 - p)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def seed_with_epoch(seed, epoch):
    """rng.h vb_seed_with_epoch with a registered counter holding `epoch` (Python int in, Python int out)."""
    return (int(seed) + int(epoch) * EPOCH_STRIDE) & MASK64


# ---- element indices, one builder per convention (uint64 arrays shaped like the tensor the mask covers) -----------------------
def flat_index(n):
    return np.arange(n, dtype=np.uint64)


def linear_index(rows, n_total):
    """[rows, n_total]: row * N + col with N the launch's total output columns."""
    return np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(n_total) + np.arange(n_total, dtype=np.uint64)[None, :]


def layernorm_index(rows, n_cols):
    """[rows, n_cols]: row * n_cols + col."""
    return linear_index(rows, n_cols)


def attention_index(batch, heads, n_q, n_k):
    """[batch, heads, n_q, n_k]: ((b * heads + h) * n_q + q) * n_k + key."""
    return np.arange(batch * heads * n_q * n_k, dtype=np.uint64).reshape(batch, heads, n_q, n_k)
