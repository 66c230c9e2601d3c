"""The dropout mask function on the CPU: tests/dropout_restatement.py (what the GPU tests of tests/test_dropout_mask_gpu.py hold
every kernel to) against csrc/rng.h itself, its statistics, and the seeds the launchers derive.

  * bit for bit: the header compiles unchanged for the host (tests/rng_driver.cpp); hash, keep decision and the step-counter
    seed of ~4 x 10^5 (seed, index, p) triples - indices around 2^32 and 2^40, p at both ends of [0, 1), seeds with the top bit;
  * the kept fraction is 1 - p within 5 binomial standard deviations, over a flat range and per sample / head / row of an
    attention-shaped block (a hash that ignored part of the index, or a float step that lost bits, shows here);
  * seeds do not alias. rng.h hashes seed + index * G (G = 0x9E3779B97F4A7C15), so two launch seeds s1, s2 draw ONE mask shifted
    by m = (s2 - s1) / G mod 2^64 (signed) elements. The seed sources are additive - autograd_ops.next_seed per call,
    ops._chunk_seed per key chunk, vb_seed_with_epoch per graph replay - so m is a function of the three differences and the
    whole range |d call| <= 1024, |d epoch| <= 8192, |d chunk| <= 8 (one training step's sites, a graph replayed a few thousand
    times) is checked exhaustively: |m| >= 2^34, where the largest mask of the models covers < 2^27 elements (18432 x 3072 FFN
    outputs). _chunk_seed used to step by G itself: |m| = |d chunk| - the mask of chunk c was chunk 0's moved c keys along.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import dropout_restatement as DR

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "vilbert-multi-task_amd", "csrc")
DRIVER = os.path.join(TESTS, "rng_driver.cpp")

P_EDGES = (0.0, 2.0 ** -24, 0.1, 0.25, 0.5, 1.0 - 2.0 ** -24)
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
G_INV = pow(G, -1, 1 << 64)
MIN_SHIFT = 1 << 34


def host_compiler():
    return shutil.which("c++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")
                                        if os.path.exists(p)), None)


def _triples():
    rng = np.random.default_rng(20240607)
    seeds = rng.integers(0, 1 << 63, 4096, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 4096, dtype=np.uint64)
    seeds[::2] |= np.uint64(1 << 63)                                         # every second seed has the top bit set
    seeds[:4] = np.array([0, 1, M64, 1 << 63], dtype=np.uint64)
    near = np.arange(-64, 64, dtype=np.int64)
    idx = np.concatenate([np.arange(0, 4096, dtype=np.uint64),                # every lane of the first blocks
                          (np.int64(1 << 32) + near).astype(np.uint64), (np.int64(1 << 40) + near).astype(np.uint64),
                          (np.int64(1 << 31) + near).astype(np.uint64), np.uint64(M64) - np.arange(64, dtype=np.uint64),
                          rng.integers(0, 1 << 27, 8192, dtype=np.uint64),    # the range the models use
                          rng.integers(0, 1 << 63, 4096, dtype=np.uint64) * np.uint64(2) + np.uint64(1)])
    n = 1 << 16
    rec = np.zeros(n * len(P_EDGES), dtype=[("seed", "<u8"), ("idx", "<u8"), ("p", "<f4"), ("unused", "<u4")])
    rec["seed"] = np.tile(seeds[rng.integers(0, seeds.size, n)], len(P_EDGES))
    pick = rng.integers(0, idx.size, n)
    pick[:idx.size] = np.arange(idx.size)                                     # every listed index at least once
    rec["idx"] = np.tile(idx[pick], len(P_EDGES))
    rec["p"] = np.repeat(np.array(P_EDGES, dtype=np.float32), n)
    return rec


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    exe = os.path.join(str(tmp_path_factory.mktemp("rng")), "rng_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe], check=True)
    rec = _triples()
    out = subprocess.run([exe], input=rec.tobytes(), check=True, capture_output=True).stdout
    got = np.frombuffer(out, dtype=[("hash", "<u4"), ("keep", "<u4"), ("with_epoch", "<u8"), ("without_epoch", "<u8")])
    assert got.size == rec.size
    return rec, got


def test_triples_cover_the_edges():
    rec = _triples()
    assert rec.size == 6 << 16 and set(np.unique(rec["p"]).tolist()) == set(np.float32(p) for p in P_EDGES)
    assert np.float32(1.0 - 2.0 ** -24) < 1 and np.float32(2.0 ** -24) > 0
    idx, seed = rec["idx"], rec["seed"]
    for centre in (1 << 32, 1 << 40):
        assert ((idx >= centre - 64) & (idx < centre)).any() and ((idx >= centre) & (idx < centre + 64)).any()
    assert (seed >> np.uint64(63)).astype(bool).sum() > rec.size // 4 and (idx >> np.uint64(63)).astype(bool).any()


def test_restatement_equals_the_header_bit_for_bit(header):
    rec, got = header
    assert np.array_equal(DR.vb_hash(rec["seed"], rec["idx"]), got["hash"])
    keep = DR.keep(rec["seed"], rec["idx"], rec["p"])
    assert np.array_equal(keep, got["keep"].astype(bool))
    # the ends of p: nothing dropped at 0; at 2^-24 exactly the elements whose 24 hash bits are all zero; all but those whose 24
    # bits are all one at 1 - 2^-24
    h24 = got["hash"] >> np.uint32(8)
    for p, want in ((0.0, np.ones_like(keep)), (2.0 ** -24, h24 != 0), (1.0 - 2.0 ** -24, h24 == (1 << 24) - 1)):
        sel = rec["p"] == np.float32(p)
        assert sel.sum() == 1 << 16 and np.array_equal(keep[sel], want[sel])
    assert np.array_equal(got["without_epoch"], rec["seed"])
    with_epoch = np.array([DR.seed_with_epoch(int(s), int(e)) for s, e in zip(rec["seed"][:4096], rec["idx"][:4096])], dtype=np.uint64)
    assert np.array_equal(with_epoch, got["with_epoch"][:4096])
    with np.errstate(over="ignore"):
        assert np.array_equal(rec["seed"] + rec["idx"] * np.uint64(DR.EPOCH_STRIDE), got["with_epoch"])


def test_scalar_and_python_int_arguments():
    """The GPU tests pass Python ints above 2^63 as seeds: same values as the array form."""
    seed = 0xC0FFEE1234567891
    idx = DR.linear_index(3, 5)
    a = DR.keep(seed, idx, 0.5)
    b = DR.keep(np.full(idx.shape, seed, dtype=np.uint64), idx, np.full(idx.shape, 0.5, dtype=np.float32))
    assert a.shape == (3, 5) and np.array_equal(a, b)
    assert DR.seed_with_epoch(M64, 1) == (DR.EPOCH_STRIDE - 1) and DR.seed_with_epoch(5, 0) == 5
    assert DR.drop_scale(0.1).dtype == np.float32 and float(DR.drop_scale(0.5)) == 2.0
    assert float(DR.drop_scale(0.1)) == float(np.float32(1.0) / np.float32(0.9)) != 1.0 / 0.9
    assert DR.attention_index(2, 3, 4, 5)[1, 2, 3, 4] == ((1 * 3 + 2) * 4 + 3) * 5 + 4
    assert DR.layernorm_index(4, 7)[3, 6] == 3 * 7 + 6 and DR.flat_index(9)[8] == 8


def _within(kept_fraction, p, n):
    return abs(kept_fraction - (1.0 - p)) <= 5.0 * math.sqrt(p * (1.0 - p) / n)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_kept_fraction_matches_p(p):
    n = 999000
    kept = float(DR.keep(1234, DR.flat_index(n), p).mean())
    assert _within(kept, p, n), kept
    if p == 0.1:
        assert round(kept, 5) == 0.90028        # (the figure of tests/test_backward_gpu.py's 1000 x 999 launch)
    # attention-shaped block of ~10^6 elements: per sample, per head, per query row (n_k elements each), with the top seed bit set
    B, heads, n_q, n_k = 4, 8, 32, 977
    k = DR.keep(0xC0FFEE1234567891, DR.attention_index(B, heads, n_q, n_k), p)
    assert _within(float(k.mean()), p, k.size)
    for axes, n_group in (((1, 2, 3), heads * n_q * n_k), ((0, 2, 3), B * n_q * n_k), ((3,), n_k)):
        frac = k.mean(axis=axes)
        worst = float(np.abs(frac - (1.0 - p)).max())
        assert worst <= 5.0 * math.sqrt(p * (1.0 - p) / n_group), (axes, worst)


# ---- seeds -------------------------------------------------------------------------------------------------------------
def _shift(delta):
    """Signed element shift between the masks of two seeds `delta` apart."""
    m = (delta * G_INV) & M64
    return m - (1 << 64) if m >> 63 else m


def _seed_strides():
    """(per call, per chunk, per epoch) seed strides, read off the code under test; each source is checked to BE additive."""
    from vilbert import autograd_ops, ops
    calls = [autograd_ops.next_seed() for _ in range(6)]
    d_call = (calls[1] - calls[0]) & M64
    assert all((b - a) & M64 == d_call for a, b in zip(calls, calls[1:])) and d_call != 0
    bases = calls[:2] + [0xC0FFEE1234567891, 1]
    d_chunk = (ops._chunk_seed(bases[0], 1) - bases[0]) & M64
    for s in bases:
        assert ops._chunk_seed(s, 0) == s, "chunk 0 keeps the launch seed"
        assert all((ops._chunk_seed(s, c) - s) & M64 == (c * d_chunk) & M64 for c in range(9)), "_chunk_seed is not additive in c"
    assert ops._chunk_seed(0, 3) == 0, "seed 0 (dropout off) stays inert"
    d_epoch = (DR.seed_with_epoch(bases[0], 1) - bases[0]) & M64
    assert all(DR.seed_with_epoch(s, e) == (s + e * d_epoch) & M64 for s in bases for e in (0, 1, 5, 8192))
    return d_call, d_chunk, d_epoch


def _smallest_shift(d_call, d_chunk, d_epoch, chunk_range):
    """min |m| over |dcall| <= 1024, |depoch| <= 8192, dchunk in chunk_range, not all zero -> (|m|, dcall, depoch, dchunk).
    Per (dcall, dchunk) the nearest of the 16385 sorted epoch terms is looked up: exhaustive, ~35,000 binary searches."""
    u = np.uint64
    de = np.arange(-8192, 8193, dtype=np.int64)
    with np.errstate(over="ignore"):
        e_terms = de.astype(u) * u((d_epoch * G_INV) & M64)
    order = np.argsort(e_terms)
    e_sorted, de_sorted = e_terms[order], de[order]

    def circle(x):
        with np.errstate(over="ignore"):
            return np.minimum(x, ~x + u(1))
    dc = np.arange(-1024, 1025, dtype=np.int64)
    best = None
    for dk in chunk_range:
        with np.errstate(over="ignore"):
            q = dc.astype(u) * u((d_call * G_INV) & M64) + u((dk * d_chunk * G_INV) & M64)     # shift without the epoch term
            target = ~q + u(1)
            j = np.searchsorted(e_sorted, target)
            for jj in ((j - 1) % e_sorted.size, j % e_sorted.size, (j + 1) % e_sorted.size):
                dist = circle(e_sorted[jj] + q)
                dist[(dc == 0) & (de_sorted[jj] == 0) & (dk == 0)] = u(M64)
                i = int(np.argmin(dist))
                if best is None or int(dist[i]) < best[0]:
                    best = (int(dist[i]), int(dc[i]), int(de_sorted[jj][i]), dk)
    assert abs(_shift(best[1] * d_call + best[2] * d_epoch + best[3] * d_chunk)) == best[0]
    return best


def test_shift_between_two_seeds_is_what_the_mask_shows():
    """The premise of the aliasing condition, on the restatement: seeds d * G apart draw one mask shifted by d elements."""
    s1, i = 0xC0FFEE1234567891, DR.flat_index(4096)
    for d in (1, 7, -3):
        s2 = (s1 + d * G) & M64
        assert _shift((s2 - s1) & M64) == d
        a, b = DR.keep(s1, i + np.uint64(8), 0.5), DR.keep(s2, (i.astype(np.int64) + 8 - d).astype(np.uint64), 0.5)
        assert np.array_equal(a, b)


def test_calls_and_epochs_alone_do_not_alias():
    d_call, _, d_epoch = _seed_strides()
    m, dc, de, _ = _smallest_shift(d_call, 0, d_epoch, [0])
    print("smallest shift over calls x epochs: 2^%.2f elements at dcall %d depoch %d" % (math.log2(m), dc, de))
    assert m >= MIN_SHIFT, (m, dc, de)
    assert (abs(dc), abs(de)) == (890, 4326) and dc * de < 0 and 37.9 <= math.log2(m) < 38.0       # (known figure: pins the search)


def test_chunk_seeds_do_not_alias():
    d_call, d_chunk, d_epoch = _seed_strides()
    m, dc, de, dk = _smallest_shift(d_call, d_chunk, d_epoch, range(-8, 9))
    print("smallest shift over calls x epochs x chunks: 2^%.2f elements at dcall %d depoch %d dchunk %d" % (math.log2(m), dc, de, dk))
    assert m >= MIN_SHIFT, "two seeds %d calls, %d epochs, %d chunks apart draw one mask shifted by %d elements" % (dc, de, dk, m)


def test_the_search_finds_the_old_chunk_stride():
    """The chunk seeds used to step by the hash's own stride: the search must report a shift of one element."""
    d_call, _, d_epoch = _seed_strides()
    assert _smallest_shift(d_call, G, d_epoch, range(-8, 9))[0] == 1
