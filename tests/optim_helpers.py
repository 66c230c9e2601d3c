"""What the test modules of the native optimizers share (test_optim_clip*.py, test_radam*.py, test_lamb*.py): the parser of
the C prototypes of a header, the fixture that builds and loads the library, oddly offset device tensors, the comparison of
bits, and the fixture that frees the deterministic workspace's slices after a GPU test. A plain module the tests import."""
import ctypes
import re

import pytest
import torch

DEV = "cuda:0"
C_TYPES = {"void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
           "int": ctypes.c_int}


def header_text(header):
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)


def prototypes(header, prefix):
    """name -> (return ctype, [argument ctypes]) of the functions `prefix`* parsed from the header text; every pointer is a
    plain address."""
    out = {}
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(%s[a-z0-9_]+)\s*\(([^)]*)\)\s*;" % re.escape(prefix), header_text(header)):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(ctypes.c_void_p if "*" in a else C_TYPES[a.replace("const ", "").split()[0]])
        out[name] = (C_TYPES[ret], types)
    return out


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from vilbert import _native
    return _native


@pytest.fixture(autouse=True)
def leave_no_workspace_slices_behind():
    """The deterministic workspace hands its 8 slices to the first 8 streams that run a split launch and keeps that
    assignment for as long as the same buffer stays registered (csrc/det_workspace.hip) - a ninth stream falls back to
    atomics. The models, data-parallel wrappers and captured steps of the GPU modules bring streams of their own; switching
    the setting off and on again after each test re-registers the same buffer with an empty assignment, so that the
    tests that run later in the same process find the slices free. (No graph of those modules outlives its test.) Active in
    the modules that import it."""
    yield
    from vilbert import _native
    if _native.deterministic_enabled() and _native._DET["ws"]:
        torch.cuda.synchronize()
        _native.set_deterministic(False)
        _native.set_deterministic(True)


def odd(t):
    """A device copy of `t` one element into its storage: data_ptr % 16 == 4."""
    base = torch.empty(t.numel() + 1, device=DEV)
    view = base[1:]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def device_params(p0, odd_index):
    """Parameters on the device; tensor `odd_index` (None: no tensor) as an oddly offset view."""
    return [torch.nn.Parameter(odd(t) if i == odd_index else t.to(DEV)) for i, t in enumerate(p0)]


def device_grad(t, is_odd):
    if t is None:
        return None
    return odd(t) if is_odd else t.to(DEV)


def bits_equal(a, b):
    return torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))
