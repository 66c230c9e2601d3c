"""Host side of the bf16 head kernels (csrc/heads16.hip, include/vilbert_hip_heads.h, prefix vbh_): the header, its ctypes
mirror (vilbert._native.HEADS_SIGNATURES) and the built library agree name by name and type by type; the entry points stay
out of the five pinned headers and the ABI version stays 18; every argument error comes back before anything is launched,
so without a GPU. No compute is launched here; the GPU side is tests/test_heads16_gpu.py."""
import ctypes
import os
import re
import subprocess

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
HEADER = os.path.join(ROOT, "include", "vilbert_hip_heads.h")
PINNED = ("vilbert_hip.h", "vilbert_hip_ext.h", "vilbert_hip_optim.h", "vilbert_hip_tasks.h", "vilbert_hip_pretrain.h")
ENTRY_POINTS = ["vbh_colsum_parts", "vbh_colsum_parts_count", "vbh_gather_rows_bf16", "vbh_invert_map", "vbh_kl_bwd_bf16",
                "vbh_mul_bf16", "vbh_padded", "vbh_relu_bwd_bf16",
                "vbh_scatter_rows_bf16", "vbh_weight_shadow_ragged", "vbh_xent_bwd_bf16"]
BADARG, ALIGN, RANGE = -1, -2, -3

_C_TYPES = {"void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "float": ctypes.c_float, "int": ctypes.c_int}


def _prototypes():
    """name -> (return ctype, [argument ctypes]) parsed from the header text; every pointer is a plain address."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(vbh_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(ctypes.c_void_p if "*" in a else _C_TYPES[a.replace("const ", "").split()[0]])
        out[name] = (_C_TYPES[ret], types)
    return out


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from vilbert import _native
    return _native


def test_header_declares_exactly_the_vbh_entry_points_and_stays_out_of_the_pinned_lists():
    assert sorted(_prototypes()) == ENTRY_POINTS
    for name in PINNED:
        assert "vbh_" not in open(os.path.join(ROOT, "include", name)).read(), name
    main = open(os.path.join(ROOT, "include", "vilbert_hip.h")).read()
    assert "#define VB_ABI_VERSION 18" in main
    make = open(os.path.join(ROOT, "vilbert-multi-task_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bheads16\.hip\b", make, flags=re.M) and re.search(r"^HDRS = .*vilbert_hip_heads\.h\b", make, flags=re.M)


def test_ctypes_mirror_and_library_agree_with_the_header(native):
    protos = _prototypes()
    assert sorted(native.HEADS_SIGNATURES) == sorted(protos)
    for name, (res, args) in protos.items():
        assert native.HEADS_SIGNATURES[name][0] is res, name
        assert native.HEADS_SIGNATURES[name][1] == args, name
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (vbh_[a-z0-9_]+)", nm))) == ENTRY_POINTS
    lib = native.lib()
    assert lib.vb_abi_version() == 18
    for name in ENTRY_POINTS:
        assert getattr(lib, name).argtypes == native.HEADS_SIGNATURES[name][1]
        assert getattr(lib, name).restype is native.HEADS_SIGNATURES[name][0]


def test_padded_is_the_next_multiple_of_256(native):
    pad = native.lib().vbh_padded
    assert [pad(n) for n in (-5, 0, 1, 255, 256, 257, 1601, 30522, 50265)] == [0, 0, 256, 256, 256, 512, 1792, 30720, 50432]


def _each(fn, good, cases, want):
    for pos, bad in cases:
        args = list(good)
        args[pos] = bad
        assert fn(*args) == want, (fn.__name__, pos, bad)


def test_argument_errors_do_not_need_a_gpu(native):
    lib = native.lib()
    a = ctypes.c_void_p(64)          # fake non-null, 16-byte aligned addresses: the argument checks come before any launch
    odd = ctypes.c_void_p(72)        # 8-byte aligned only
    big = 1 << 62

    # vbh_gather_rows_bf16(stream, rows, cols, src, lds, src_rows, map, out, ldo)
    good = [None, 4, 16, a, 16, 9, a, a, 24]
    _each(lib.vbh_gather_rows_bf16, good, [(3, None), (6, None), (7, None), (1, -1), (2, 0), (2, -8), (5, 0), (4, 8), (8, 8)],
          BADARG)
    _each(lib.vbh_gather_rows_bf16, good, [(3, odd), (7, odd), (4, 20), (8, 20)], ALIGN)
    assert lib.vbh_gather_rows_bf16(None, 4, 12, a, 16, 9, a, a, 24) == ALIGN          # cols % 8
    _each(lib.vbh_gather_rows_bf16, good, [(1, big), (5, big)], RANGE)
    assert lib.vbh_gather_rows_bf16(*[None, 0] + good[2:]) == 0                        # no rows: no launch

    # vbh_invert_map(stream, full_rows, rows, map, inv)
    inv = lib.vbh_invert_map
    assert inv(None, 8, 4, None, a) == BADARG and inv(None, 8, 4, a, None) == BADARG
    assert inv(None, -1, 4, a, a) == BADARG and inv(None, 8, -1, a, a) == BADARG
    assert inv(None, 1 << 31, 4, a, a) == RANGE and inv(None, 8, 1 << 31, a, a) == RANGE
    assert inv(None, 0, 4, a, a) == 0 and inv(None, 0, 0, None, a) == 0

    # vbh_scatter_rows_bf16(stream, full_rows, cols, compact, ldc, rows, inv, full, ldf)
    good = [None, 9, 16, a, 16, 4, a, a, 24]
    _each(lib.vbh_scatter_rows_bf16, good, [(3, None), (6, None), (7, None), (1, -1), (5, -1), (2, 0), (4, 8), (8, 8)], BADARG)
    _each(lib.vbh_scatter_rows_bf16, good, [(3, odd), (7, odd), (4, 20), (8, 20), (2, 12)], ALIGN)
    _each(lib.vbh_scatter_rows_bf16, good, [(1, big), (5, big)], RANGE)
    assert lib.vbh_scatter_rows_bf16(None, 0, 16, a, 16, 4, a, a, 24) == 0
    assert lib.vbh_scatter_rows_bf16(None, 0, 16, None, 16, 0, a, a, 24) == 0           # no compact rows: no buffer needed

    # vbh_weight_shadow_ragged(stream, n, K, w, ldw, bias, w16, wt16, bias_pad)
    good = [None, 211, 128, a, 128, a, a, a, a]
    _each(lib.vbh_weight_shadow_ragged, good, [(3, None), (1, 0), (1, -2), (2, 0), (4, 64)], BADARG)
    assert lib.vbh_weight_shadow_ragged(None, 211, 128, a, 128, a, None, None, a) == BADARG     # neither shadow wanted
    _each(lib.vbh_weight_shadow_ragged, good, [(2, 96), (4, 130), (3, odd), (6, odd), (7, odd)], ALIGN)
    _each(lib.vbh_weight_shadow_ragged, good, [(1, (1 << 21) + 1)], RANGE)

    # vbh_xent_bwd_bf16(stream, rows, n, logits, ld, labels, ignore_index, lse, grad_loss, count, G, ldg, GT, ldgt, colsum_part)
    good = [None, 5, 211, a, 211, a, -1, a, a, a, a, 256, a, 256, a]
    _each(lib.vbh_xent_bwd_bf16, good, [(3, None), (5, None), (7, None), (8, None), (9, None), (10, None), (1, -1), (2, 0),
                                        (4, 210), (11, 248), (13, 248)], BADARG)
    _each(lib.vbh_xent_bwd_bf16, good, [(10, odd), (12, odd), (11, 260), (13, 260)], ALIGN)
    _each(lib.vbh_xent_bwd_bf16, good, [(4, big), (11, big), (13, big)], RANGE)
    args = list(good)
    args[1], args[13] = (1 << 21) + 1, 1 << 22                                          # more rows than the grid serves
    assert lib.vbh_xent_bwd_bf16(*args) == RANGE
    args = list(good)
    args[2], args[4], args[11] = (1 << 21) + 1, 1 << 22, 1 << 22                        # wider than the grid serves
    assert lib.vbh_xent_bwd_bf16(*args) == RANGE
    assert lib.vbh_xent_bwd_bf16(*[None, 0] + good[2:]) == 0
    args = list(good)
    args[1], args[12], args[13], args[14] = 0, None, 0, None                            # GT and colsum_part are optional
    assert lib.vbh_xent_bwd_bf16(*args) == 0

    # vbh_colsum_parts(stream, parts, n, part, ldp, out)
    good = [None, 3, 211, a, 256, a]
    _each(lib.vbh_colsum_parts, good, [(3, None), (5, None), (1, -1), (2, 0), (4, 210)], BADARG)
    _each(lib.vbh_colsum_parts, good, [(1, big)], RANGE)
    assert lib.vbh_colsum_parts(None, 0, 211, a, 256, a) == 0
    cnt = lib.vbh_colsum_parts_count
    assert [cnt(r) for r in (-3, 0, 1, 64, 65, 2304)] == [0, 0, 1, 1, 2, 36]

    # vbh_kl_bwd_bf16(stream, rows, n, scores, ld, target, ldt, lse, tsum, grad_loss, divisor, divisor_dev, G, ldg)
    good = [None, 5, 1601, a, 1601, a, 1604, a, a, a, 5.0, None, a, 1792]
    _each(lib.vbh_kl_bwd_bf16, good, [(3, None), (5, None), (7, None), (8, None), (9, None), (12, None), (1, -1), (2, 0),
                                      (4, 1600), (6, 1600), (13, 1784)], BADARG)
    _each(lib.vbh_kl_bwd_bf16, good, [(12, odd), (13, 1796)], ALIGN)
    _each(lib.vbh_kl_bwd_bf16, good, [(4, big), (6, big), (13, big)], RANGE)
    assert lib.vbh_kl_bwd_bf16(*[None, 0] + good[2:]) == 0

    # vbh_relu_bwd_bf16(stream, rows, cols, dy, ldd, y, ldy, out, ldo)
    good = [None, 4, 16, a, 16, a, 20, a, 24]
    _each(lib.vbh_relu_bwd_bf16, good, [(3, None), (5, None), (7, None), (1, -1), (2, 0), (4, 12), (6, 12), (8, 8)], BADARG)
    _each(lib.vbh_relu_bwd_bf16, good, [(3, odd), (5, odd), (7, odd), (4, 18), (6, 18), (8, 20), (2, 12)], ALIGN)
    _each(lib.vbh_relu_bwd_bf16, good, [(4, big), (6, big), (8, big)], RANGE)
    assert lib.vbh_relu_bwd_bf16(*[None, 0] + good[2:]) == 0

    # vbh_mul_bf16(stream, rows, cols, a, lda, b, ldb, out, ldo)
    good = [None, 4, 16, a, 16, a, 24, a, 32]
    _each(lib.vbh_mul_bf16, good, [(3, None), (5, None), (7, None), (1, -1), (2, 0), (4, 8), (6, 8), (8, 8)], BADARG)
    _each(lib.vbh_mul_bf16, good, [(3, odd), (5, odd), (7, odd), (4, 20), (6, 20), (8, 20), (2, 12)], ALIGN)
    _each(lib.vbh_mul_bf16, good, [(4, big), (6, big), (8, big)], RANGE)
    assert lib.vbh_mul_bf16(*[None, 0] + good[2:]) == 0
