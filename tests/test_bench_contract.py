"""bench.py host-side pieces that can be checked without a GPU: the algorithmic FLOP formula the roofline
uses (15.247 GFLOP BertModel forward, 17.202 incl. VLTasks heads, 17.171 incl. the
pre-training heads, 32.993 for bert_large) and the synthetic batch conventions."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from vilbert.vilbert import BertConfig  # noqa: E402


def _cfg(name):
    return BertConfig.from_json_file(os.path.join(ROOT, "vilbert-multi-task_amd", "config", name)).to_dict()


def test_flop_formula_matches_the_survey_figures():
    base = _cfg("bert_base_6layer_6conect.json")
    bert, vl = bench.model_flops_per_sample(base, 36, 36, "vltasks")
    assert bert / 1e9 == pytest.approx(15.247, abs=2e-3)
    assert vl / 1e9 == pytest.approx(17.202, abs=2e-3)
    _, pre = bench.model_flops_per_sample(base, 36, 36, "pretraining")
    assert pre / 1e9 == pytest.approx(17.171, abs=2e-3)
    _, pre37 = bench.model_flops_per_sample(base, 36, 37, "pretraining")
    assert 3 * pre37 / 1e9 == pytest.approx(52.0, abs=0.05)           # fwd+bwd at the loader's R = 37
    large, _ = bench.model_flops_per_sample(_cfg("bert_large_6layer_6conect.json"), 36, 36, "vltasks")
    assert large / 1e9 == pytest.approx(32.993, abs=2e-3)


def test_synthetic_batch_follows_the_loader_conventions():
    cfg = _cfg("bert_base_6layer_6conect.json")
    x = bench.synthetic_batch(cfg, 4, 36, 37, 7, True)
    assert x["image_feat"].shape == (4, 37, 2048) and x["image_loc"].shape == (4, 37, 5)
    assert x["image_target"].shape == (4, 36, 1601) and x["image_label"].shape == (4, 36)
    assert torch.allclose(x["image_target"].sum(-1), torch.ones(4, 36), atol=1e-5)
    assert set(x["image_label"].unique().tolist()) <= {-1, 1} and (x["image_label"][:, 0] == 1).all()
    assert ((x["masked_lm_labels"] == -1) | (x["masked_lm_labels"] == x["input_ids"])).all()
    assert (x["image_loc"][:, 0] == torch.tensor([0.0, 0.0, 1.0, 1.0, 1.0])).all()
    y = bench.synthetic_batch(cfg, 4, 36, 37, 7, True)
    assert all(torch.equal(x[k], y[k]) for k in x)                      # seeded


def test_bench_starts_its_own_ranks_when_not_under_a_launcher():
    """`python bench.py --gpus 2` without RANK in the environment re-executes itself through torch.distributed.run
    (one process per GPU, rendezvous on 127.0.0.1). Without GPUs every rank stops at its device check - which proves
    that the ranks were started with the right environment."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, env=env)
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        assert r.returncode == 0, r.stderr[-2000:]
        return
    assert r.returncode != 0
    text = r.stdout + r.stderr
    assert "GPU(s) visible" in text, text[-2000:]


def test_dump_outputs_writes_float32_within_budget_and_samples_repeatably(tmp_path):
    """--dump-outputs: float32 files (float64 kept), arrays over their share of the budget replaced by the same seeded
    sample on every call, all files together under 64 MB."""
    import numpy as np
    g = torch.Generator().manual_seed(0)
    arrays = {"small": torch.randn(3, 5, generator=g), "wide": torch.randn(9000, 4000, generator=g),
              "half": torch.randn(7, generator=g).to(torch.bfloat16), "exact": torch.randn(4, dtype=torch.float64, generator=g)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in arrays}
    assert got["small"].dtype == np.float32 and np.array_equal(got["small"], arrays["small"].numpy())
    assert got["half"].dtype == np.float32 and np.array_equal(got["half"], arrays["half"].float().numpy())
    assert got["exact"].dtype == np.float64 and np.array_equal(got["exact"], arrays["exact"].numpy())
    assert got["wide"].dtype == np.float32 and got["wide"].ndim == 1 and 0 < got["wide"].size < 9000 * 4000
    assert np.isin(got["wide"], arrays["wide"].numpy()).all()
    assert np.array_equal(got["wide"], np.load(str(tmp_path / "b" / "wide.npy")))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64_000_000


def test_parameter_samples_follow_named_parameters():
    net = torch.nn.Sequential(torch.nn.Linear(300, 200), torch.nn.Linear(200, 2))
    net[0].weight.grad = torch.ones_like(net[0].weight)
    vals, grads = bench.parameter_samples(net, per_param=64)
    assert vals.shape == grads.shape == (64 + 64 + 64 + 2,)
    assert (grads[:64] == 1).all() and (grads[64:] == 0).all()
    assert torch.equal(vals, bench.parameter_samples(net, per_param=64)[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run times exactly --steps steps, prints the headline keys and none of the --full legs, and --dump-outputs
    leaves the last step's losses and the parameter / gradient samples as float32 .npy files."""
    import json
    import subprocess
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "16", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 2 and line["unit"] == "samples/s" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(16 * 1e3 / line["ms_per_step"], rel=1e-2)
    assert not {"roofline", "alt_gemm_modes", "cpu_baseline", "b64", "fwd_b512", "summary"} & set(line)
    names = {"masked_lm_loss", "masked_img_loss", "next_sentence_loss", "parameters_after_step_sample", "gradients_sample"}
    assert {p.stem for p in tmp_path.iterdir()} == names
    for n in names:
        a = np.load(str(tmp_path / (n + ".npy")))
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
    assert np.abs(np.load(str(tmp_path / "gradients_sample.npy"))).max() > 0
