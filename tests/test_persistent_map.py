"""The block-to-tile map of every persistent kernel (csrc/persistent_map.h) on the CPU.

gemm_v4.h / gemm_v4w.h (fp32), gemm_bf16.hip (bf16 training) and mx8.hip (MX) deal their output tiles - or, for the bf16 weight
gradient, their (tile, contraction split) units - to a fixed set of resident blocks with tile_of / unit_of and place a tile
in the tile grid with tile_rc. A wrong map writes an output tile twice or never. The header is plain C++ for the host
compiler too, so tests/persistent_map_driver.cpp evaluates it over

    grid in GRIDS, every tile / unit count from 1 to 3 grid + 9, every round up to one past the last, every block
    tiles_n in 1 .. 32, tiles_m in 1 .. 80, every tile

and this file checks what the kernels rely on, and that the functions still compute what the three hand-copied versions
of the parent commit computed (restated below in numpy, line by line from mx8.hip's mx_tile_of / mx_origin and gemm_bf16.hip's
hw_unit_of as they stood before the extraction).
"""
import os
import subprocess

import numpy as np
import pytest

from test_gemm_plan import CSRC, TESTS, host_compiler

DRIVER = os.path.join(TESTS, "persistent_map_driver.cpp")
GRIDS = (8, 16, 64, 128, 160, 256, 512)


def ref_tile_of(b, it, grid, tiles):
    """mx_tile_of of the parent commit, for an array of blocks b."""
    base = it * grid
    n = min(grid, tiles - base)
    if n <= 0:
        return np.full_like(b, -1)
    if (n & 7) != 0:
        return np.where(b < n, base + b, -1)
    per, x, j = n >> 3, b & 7, b >> 3
    return np.where(j < per, base + x * per + j, -1)


def ref_unit_of(b, i, grid, units):
    """hw_unit_of of the parent commit, for an array of blocks b."""
    base = i * grid
    n = min(grid, units - base)
    if n <= 0:
        return np.full_like(b, -1)
    per, x, j = (n + 7) >> 3, b & 7, b >> 3
    idx = x * per + j
    return np.where((j < per) & (idx < n), base + idx, -1)


def ref_tile_rc(t, tiles, tiles_n):
    """The (r, c) part of mx_origin of the parent commit, for an array of tiles t."""
    tiles_m = tiles // tiles_n
    if (tiles_n & 7) == 0 and (tiles_m & 3) == 0:
        patch, w, pcols = t >> 5, t & 31, tiles_n >> 3
        return (patch // pcols) * 4 + (w >> 3), (patch % pcols) * 8 + (w & 7)
    return t // tiles_n, t % tiles_n


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    exe = os.path.join(str(tmp_path_factory.mktemp("pmap")), "persistent_map_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe], check=True)
    return np.frombuffer(subprocess.run([exe], check=True, capture_output=True).stdout, dtype=np.int32)


def rounds_of(grid, n):
    return (n + grid - 1) // grid + 1      # one past the last: it must hand out nothing


def deal_size():
    return sum(rounds_of(g, n) * g for g in GRIDS for n in range(1, 3 * g + 10))


def test_header_is_host_only(tmp_path):
    """persistent_map.h compiles alone with the host compiler: no HIP header."""
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    src = tmp_path / "only.cpp"
    src.write_text('#include "persistent_map.h"\n')
    subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(src)], check=True)
    assert "#include" not in open(os.path.join(CSRC, "persistent_map.h")).read()


@pytest.mark.parametrize("which", ["tile_of", "unit_of"])
def test_every_tile_is_dealt_exactly_once(driver_output, which):
    ref = ref_tile_of if which == "tile_of" else ref_unit_of
    pos = 0 if which == "tile_of" else deal_size()
    for grid in GRIDS:
        b = np.arange(grid, dtype=np.int32)
        for n in range(1, 3 * grid + 10):
            rounds = rounds_of(grid, n)
            got = driver_output[pos:pos + rounds * grid].reshape(rounds, grid)
            pos += rounds * grid
            where = "%s grid %d, %d tiles" % (which, grid, n)
            # the arithmetic is the parent commit's
            assert all(np.array_equal(got[it], ref(b, it, grid, n)) for it in range(rounds)), where
            # the union over blocks and rounds is {0 .. n - 1}, each once
            assert np.array_equal(np.sort(got[got >= 0]), np.arange(n)), where
            # a block's rounds are contiguous: after its first -1 it never gets a tile again (the kernels count their
            # rounds with `while (rounds * grid < tiles && tile_of(b, rounds, grid, tiles) >= 0) ++rounds`)
            live = got >= 0
            assert not (live[1:] & ~live[:-1]).any(), where
            assert not live[-1].any() and ((np.arange(rounds) * grid < n)[:, None] | ~live).all(), where
            # round `it` only hands out tiles of [it grid, (it + 1) grid)
            assert (np.where(live, got // grid, np.arange(rounds)[:, None]) == np.arange(rounds)[:, None]).all(), where


def test_tile_rc_is_a_bijection_onto_the_tile_grid(driver_output):
    pos = 2 * deal_size()
    n_patch = 0
    for tiles_n in range(1, 33):
        for tiles_m in range(1, 81):
            tiles = tiles_m * tiles_n
            r, c = driver_output[pos:pos + 2 * tiles].reshape(tiles, 2).T
            pos += 2 * tiles
            where = "%d x %d tiles" % (tiles_m, tiles_n)
            want_r, want_c = ref_tile_rc(np.arange(tiles, dtype=np.int32), tiles, tiles_n)
            assert np.array_equal(r, want_r) and np.array_equal(c, want_c), where
            assert (r >= 0).all() and (r < tiles_m).all() and (c >= 0).all() and (c < tiles_n).all(), where
            assert np.array_equal(np.sort(r * tiles_n + c), np.arange(tiles)), where
            if tiles_n % 8 == 0 and tiles_m % 4 == 0:
                # the patch case: 32 consecutive tiles (what an XCD works on at a time) span exactly 4 rows and 8 columns
                n_patch += 1
                for p in range(tiles // 32):
                    assert len(set(r[32 * p:32 * p + 32])) == 4 and len(set(c[32 * p:32 * p + 32])) == 8, where
                    assert r[32 * p:32 * p + 32].max() - r[32 * p] == 3 and c[32 * p:32 * p + 32].max() - c[32 * p] == 7, where
    assert pos == len(driver_output) and n_patch == 4 * 20
