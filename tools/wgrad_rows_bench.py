"""Per-launch time of the weight-gradient GEMMs of the last layers: compact rows against their full-size siblings, planner's
choice (v4 mode 1) and the persistent v4w kernel forced wherever it is eligible (mode 2)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vilbert-multi-task_amd"), ROOT]
from vilbert import _native, ops  # noqa: E402

DEV = "cuda:0"
SHAPES = [(2304, 3072, 768), (9216, 3072, 768), (2304, 768, 3072), (9216, 768, 3072), (2304, 768, 768), (9216, 768, 768),
          (2368, 1024, 1024), (9472, 1024, 1024)]
_native.set_deterministic(True, device=DEV)
for mode in (1, 2):
    _native.set_gemm_v4(mode)
    for rows, n, k in SHAPES:
        g = torch.Generator().manual_seed(rows + n)
        dy = torch.randn(rows, n, generator=g).to(DEV)
        x = torch.randn(rows, k, generator=g).to(DEV)
        dw = torch.zeros(n, k, device=DEV)
        db = torch.zeros(n, device=DEV)
        for _ in range(3):
            ops.linear_bwd_weight(dy, x, 1, n, [True], dw_out=[dw], db_out=[db])
        torch.cuda.synchronize()
        ops.profile_linear(True)
        for _ in range(20):
            ops.linear_bwd_weight(dy, x, 1, n, [True], dw_out=[dw], db_out=[db])
        ms, fl, cnt = ops.profile_linear(False)
        print("v4_mode %d wgrad rows=%5d W[%4d,%4d]  %8.1f us  %6.1f TF" % (mode, rows, n, k, ms / cnt * 1e3, fl / (ms * 1e-3) / 1e12),
              flush=True)
_native.set_gemm_v4(1)
