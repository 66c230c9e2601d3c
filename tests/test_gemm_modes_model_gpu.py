"""The fp32-emulation GEMM modes at model level: every parameter gradient against autograd through the CPU
oracle (tests/test_backward_gpu.py _grad_parity, imported - dropout forced off as there), and the forward of "bf16x3" against
the reference's golden vectors.

"bf16x6" is held to the UNCHANGED criterion of the exact-fp32 mode: |got - ref| <= 2e-4 max|ref| + 2e-7 (largest gradient
entry of the model), ratio <= 1.0 - the README's claim that the mode passes the same parity tests. Configurations: the tiny
config for the pre-training and the task model, and bert_base_2layer_2conect.json at (4, 20, 37): the 768 / 1024 / 3072-wide
linears and the 30522-wide decoder with its ragged-contraction and split-K routes.

"bf16x3" drops the plane products of relative size 2^-16 and below and has a bound of its own, recorded here by the project's
rule for a measured bound: the worst ratio to that same criterion was measured on an MI355X (MEASURED below, the run is
deterministic by default), and the test asserts 1.5 x that ratio, never below 1.0; 1.5 is the project's plain margin and
covers machine-to-machine differences only. Measured: gradients 0.064 (tiny pre-training), 0.065 (tiny task model), 0.103
(base 2L/2C) of the criterion; golden forward cases 0.043 / 0.001 / 0.420 / 0.382 of the 1e-4 bar. Every one is below 1, so
the asserted bound is 1.0 everywhere: on these configurations bf16x3 meets the fp32 criterion too, with 2.4 x (forward) to
10 x (gradients) of headroom where bf16x6 has 17 x to 50 x.
"""
import pytest
import torch

import helpers
from helpers import cases
from oracle import synth
from test_backward_gpu import NO_DROPOUT, _grad_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GRAD_CONFIGS = {  # name -> (config, kind, batch, tokens, regions)
    "tiny_pretraining": (None, "pretraining", 4, 9, 8),
    "tiny_vltasks": (None, "vltasks", 4, 9, 8),
    "base_2l2c": ("bert_base_2layer_2conect.json", "pretraining", 4, 20, 37),
}
GOLDEN_CASES = ["tiny_vltasks", "tiny_pretraining_losses", "base_2l2c_b8", "base_6l6c_b2"]

# bf16x3, measured on one MI355X: worst |got - ref| / (2e-4 max|ref| + 2e-7 model max) over the parameter gradients, and worst
# |got - gold| / (1e-4 + 1e-4 |gold|) over the sampled outputs of the golden cases
# (bf16x6 on the same run, for comparison: gradients 0.004 / 0.008 / 0.019, golden cases 0.003 / 0.002 / 0.059 / 0.043)
MEASURED = {
    "tiny_pretraining": 0.0639, "tiny_vltasks": 0.0653, "base_2l2c": 0.1029,
    "golden/tiny_vltasks": 0.0426, "golden/tiny_pretraining_losses": 0.0009, "golden/base_2l2c_b8": 0.4196,
    "golden/base_6l6c_b2": 0.3818,
}
MARGIN = 1.5


def bound_of(key):
    return max(1.0, MARGIN * MEASURED[key])


@pytest.fixture
def mode(request):
    from vilbert import _native
    prev = _native.set_gemm_mode(request.param)
    yield request.param
    _native.set_gemm_mode(prev)


def grad_ratio(name, slack):
    """Worst gradient error of a configuration relative to the criterion, in the GEMM mode that is set."""
    import vilbert.vilbert as V
    cfgname, kind, batch, n_tok, n_reg = GRAD_CONFIGS[name]
    cfg = synth.tiny_config(**NO_DROPOUT) if cfgname is None else dict(synth.load_config(cfgname), **NO_DROPOUT)
    # the wrappers hard-code nn.Dropout(0.1) on the pooled output: every effective dropout probability is forced to 0
    orig, V._drop_p = V._drop_p, (lambda m: 0.0)
    try:
        return _grad_parity(cfg, kind, batch, n_tok, n_reg, slack=slack)
    finally:
        V._drop_p = orig


def golden_ratio(case):
    """Worst forward error of a golden case relative to helpers.assert_close's bound, in the GEMM mode that is set."""
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining, VILBertForVLTasks
    c = cases.CASES[case]
    cfg, sd, x = cases.case_inputs(case)
    conf = BertConfig.from_dict(cfg)
    m = VILBertForVLTasks(conf, num_labels=1) if c["kind"] == "vltasks" else BertForMultiModalPreTraining(conf)
    m.load_state_dict(sd)
    m = m.eval().to(DEV)
    with torch.no_grad():
        out = m(*helpers.to_device(cases.forward_args(case, x), DEV))
    gold = helpers.load_golden(case)
    worst = 0.0
    for i, n in enumerate(cases.output_names(case)):
        got = cases.sample(case, n, out[i]).detach().cpu().double()
        want = torch.as_tensor(gold[n]).double()
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), "%s/%s" % (case, n)
        worst = max(worst, float(((got - want).abs() / (helpers.ATOL + helpers.RTOL * want.abs())).max()))
    return worst


@pytest.mark.parametrize("mode", ["bf16x6"], indirect=True)
@pytest.mark.parametrize("name", list(GRAD_CONFIGS))
def test_bf16x6_model_gradients_match_oracle_autograd(mode, name):
    ratio = grad_ratio(name, 1.0)
    print("bf16x6, %s: worst gradient error %.3f of the fp32 criterion" % (name, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("mode", ["bf16x3"], indirect=True)
@pytest.mark.parametrize("name", list(GRAD_CONFIGS))
def test_bf16x3_model_gradients_stay_within_their_recorded_bound(mode, name):
    """Measured worst ratios to the fp32 criterion (2e-4 max|ref| + 2e-7 model max): see MEASURED; asserted: 1.5 x, >= 1."""
    ratio = grad_ratio(name, bound_of(name))
    print("bf16x3, %s: worst gradient error %.3f of the fp32 criterion (recorded %.3f, bound %.3f)" % (
        name, ratio, MEASURED[name], bound_of(name)))
    assert ratio <= bound_of(name)


@pytest.mark.parametrize("mode", ["bf16x3"], indirect=True)
@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_bf16x3_model_matches_reference_golden_within_its_recorded_bound(mode, case):
    """The bf16x3 twin of test_gemm_modes_gpu.py test_bf16x6_model_matches_reference_golden. Measured worst ratios to the
    1e-4 + 1e-4 |gold| bar: see MEASURED; asserted: 1.5 x, >= 1."""
    key = "golden/" + case
    ratio = golden_ratio(case)
    print("bf16x3, %s: worst output error %.3f of the 1e-4 bar (recorded %.3f, bound %.3f)" % (case, ratio, MEASURED[key], bound_of(key)))
    assert ratio <= bound_of(key)
