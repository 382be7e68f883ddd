"""tests/rollout_ref.py (the numpy twins of the two rollout kernels) against a naive per-episode loop on the scripted B = 3, T = 7 case, the record twin's
scatter, and the chunk index arithmetic of vpt_amd.rollout.  No GPU."""
import numpy as np
import pytest

import vpt_amd  # noqa: F401
from vpt_amd import rollout
from tests import rollout_ref as R


def _walk(reward, done, ret0, len0):
    b, t_len = reward.shape
    bufs = R.new_reward_bufs(b, t_len, ret0, len0)
    for t in range(t_len):
        R.reward_step(bufs, t, reward[:, t], done[:, t])
    return bufs


def test_scripted_case_holds_every_situation():
    reward, done, ret0, len0 = R.scripted_case()
    assert reward.shape == done.shape == (3, 7)
    assert done[:, 0].any() and done[:, -1].any()                       # an episode ends at step 0, one at the last step
    assert (done[:, 1:] & done[:, :-1]).any()                           # two on consecutive steps
    assert (~done.any(axis=1)).any()                                    # an environment that never finishes
    assert (ret0 != 0).any() and (len0 != 0).any()                      # an episode that continues from the previous rollout
    assert np.float32(reward[0, 1] + reward[0, 2]) + reward[0, 3] != reward[0, 1] + np.float32(reward[0, 2] + reward[0, 3])      # order of the adds matters


def test_reward_twin_equals_the_per_episode_loop():
    reward, done, ret0, len0 = R.scripted_case()
    bufs = _walk(reward, done, ret0, len0)
    finished, running = R.episodes_naive(reward, done, ret0, len0)
    want_ret, want_len = np.zeros_like(reward), np.zeros(reward.shape, np.int32)
    for i, eps in enumerate(finished):
        for t, total, n in eps:
            want_ret[i, t], want_len[i, t] = total, n
    assert np.array_equal(bufs["reward"], reward)
    assert bufs["done_return"].dtype == np.float32 and np.array_equal(bufs["done_return"].view(np.uint32), want_ret.view(np.uint32))
    assert np.array_equal(bufs["done_length"], want_len)
    assert np.array_equal(bufs["done_length"] > 0, done)
    assert np.array_equal(bufs["ep_return"].view(np.uint32), np.array([r for r, _ in running], np.float32).view(np.uint32))
    assert np.array_equal(bufs["ep_length"], np.array([n for _, n in running], np.int32))
    # the episode that came in with (2.5, 4) and ended at step 0 reports all of it; environment 1 has reported nothing and carries 7 steps
    assert bufs["done_return"][0, 0] == np.float32(3.5) and bufs["done_length"][0, 0] == 5
    assert not bufs["done_length"][1].any() and bufs["ep_length"][1] == 7
    assert bufs["done_return"][0, 3] == 0.0 and bufs["done_length"][0, 3] == 3          # (2^24 + 1) - 2^24 in float32, left to right


def test_reward_twin_across_two_rollouts_equals_one_long_rollout():
    reward, done, ret0, len0 = R.scripted_case()
    whole = _walk(np.concatenate([reward, reward], 1), np.concatenate([done, done], 1), ret0, len0)
    a = _walk(reward, done, ret0, len0)
    b = _walk(reward, done, a["ep_return"], a["ep_length"])
    for k in ("reward", "done_return", "done_length"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 1), whole[k]), k
    assert np.array_equal(b["ep_return"], whole["ep_return"]) and np.array_equal(b["ep_length"], whole["ep_length"])
    assert whole["done_length"][1].sum() == 0 and whole["ep_length"][1] == 14


def test_record_twin_is_a_scatter_into_column_t():
    rng = np.random.default_rng(0)
    b, t_len = 3, 5
    bufs = dict(img=np.full((b, t_len, 4, 4, 3), 0xA5, np.uint8), first=np.full((b, t_len), 0xA5, np.uint8), act_buttons=np.full((b, t_len), -7, np.int64),
                act_camera=np.full((b, t_len), -7, np.int64), old_log_prob=np.full((b, t_len), -7.0, np.float32), vpred=np.full((b, t_len), -7.0, np.float32),
                nan_flag=np.zeros(1, np.uint8))
    before = {k: v.copy() for k, v in bufs.items()}
    img = rng.integers(0, 256, (b, 4, 4, 3), dtype=np.uint8)
    lp = np.array([-1.0, -2.0, -3.0], np.float32)
    R.record(bufs, 2, img, [1, 0, 1], [5, 6, 7], [8, 9, 10], lp, [0.5, 1.5, 2.5])
    assert np.array_equal(bufs["img"][:, 2], img) and bufs["first"][:, 2].tolist() == [1, 0, 1] and bufs["act_camera"][:, 2].tolist() == [8, 9, 10]
    assert np.array_equal(bufs["old_log_prob"][:, 2], lp) and bufs["nan_flag"][0] == 0
    for k in before:
        if k != "nan_flag":
            keep = np.ones(t_len, bool)
            keep[2] = False
            assert np.array_equal(bufs[k][:, keep], before[k][:, keep]), k
    R.record(bufs, 0, img, [0, 0, 0], [5, 6, 7], [8, 9, 10], np.array([-1.0, np.nan, -3.0], np.float32), [0.5, 1.5, 2.5])
    assert bufs["nan_flag"][0] == 1
    R.record(bufs, 1, img, [0, 0, 0], [5, 6, 7], [8, 9, 10], lp, [0.5, 1.5, 2.5])
    assert bufs["nan_flag"][0] == 1                                    # sticky
    with pytest.raises(ValueError):
        R.record(bufs, t_len, img, [0, 0, 0], [5, 6, 7], [8, 9, 10], lp, [0.5, 1.5, 2.5])


@pytest.mark.parametrize("n_chunks", [1, 2, 7])
def test_chunk_index_arithmetic(n_chunks):
    for chunk_len in (1, 3):
        horizon = n_chunks * chunk_len
        bounds = R.chunk_bounds(horizon, chunk_len)
        assert bounds == rollout.chunk_bounds(horizon, chunk_len)
        assert len(bounds) == n_chunks and bounds[0][0] == 0 and bounds[-1][1] == horizon
        assert all(hi - lo == chunk_len for lo, hi in bounds) and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
        x = np.arange(2 * horizon).reshape(2, horizon)
        parts = [R.chunk(dict(x=x), k, chunk_len)["x"] for k in range(n_chunks)]
        assert np.array_equal(np.concatenate(parts, 1), x)
        assert all(np.array_equal(p, x[:, lo:hi]) for p, (lo, hi) in zip(parts, bounds))
    for bad in ((7, 2), (3, 6), (0, 1), (4, 0)):
        with pytest.raises(ValueError):
            rollout.chunk_bounds(*bad)
    with pytest.raises(ValueError):
        R.chunk_bounds(7, 2)


def test_chunk_keys_are_the_trainer_steps_argument_names():
    import inspect
    from vpt_amd.rl_training import PPOTrainer
    params = list(inspect.signature(PPOTrainer.step).parameters)
    assert list(rollout.CHUNK_KEYS) == params[1:1 + len(rollout.CHUNK_KEYS)]
