"""bench.py's options and its --dump-outputs writer, checked without a GPU: a plain run is the headline only (--full is off by default), and the
writer stays under 64 MB in float32, samples an oversized array at the same seeded elements every time, and keeps small arrays whole."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_bench_for_test", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench)


def test_plain_run_is_the_default_and_steps_are_honoured():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def _outputs(seed, big):
    g = torch.Generator().manual_seed(seed)
    pd = {"buttons": torch.randn(4, 16, 1, 8641, generator=g), "camera": torch.randn(4, 16, 1, 121, generator=g).to(torch.bfloat16)}
    vpred = torch.randn(4, 16, 1, generator=g)
    state = [(None, (torch.randn(big, generator=g), torch.randn(big, generator=g))),
             (torch.rand(4, 1, 128, generator=g) < 0.5, (torch.randn(4, 128, 64, generator=g), torch.randn(4, 128, 64, generator=g)))]
    return pd, vpred, state


def test_dump_outputs_budget_sampling_and_repeatability(tmp_path):
    big = (8, 128, 1100)                       # 1.1 M elements: above the per-array share, written as a sample
    pd, vpred, state = _outputs(0, big)
    w1 = bench.dump_outputs(str(tmp_path / "a"), pd, vpred, state)
    w2 = bench.dump_outputs(str(tmp_path / "b"), *_outputs(0, big))
    assert w1 == w2
    assert set(w1) == {"buttons_logprob.npy", "camera_logprob.npy", "vpred.npy", "state_0_k_sample.npy", "state_0_v_sample.npy",
                       "state_1_mask.npy", "state_1_k.npy", "state_1_v.npy"}
    total = 0
    for name, shape in w1.items():
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and list(a.shape) == shape and np.array_equal(a, b), name
        total += os.path.getsize(tmp_path / "a" / name)
    assert total < 64 * 2**20
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "buttons_logprob.npy"), pd["buttons"].numpy())          # small arrays whole, shape kept
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "camera_logprob.npy"), pd["camera"].float().numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "state_1_mask.npy"), state[1][0].float().numpy())
    k = np.load(tmp_path / "a" / "state_0_k_sample.npy")
    flat = state[0][1][0].reshape(-1).numpy()
    assert k.ndim == 1 and len(k) <= 1 << 20 and np.isin(k, flat).all()      # elements of the array itself
    assert not np.array_equal(k, np.load(tmp_path / "a" / "state_0_v_sample.npy"))

