"""ops.rollout_record / ops.rollout_reward (csrc/vpt_rollout.hip) against their numpy twins (tests/rollout_ref.py), bit for bit.  Needs an MI355X.
Record: B in {1, 3}, T in {1, 5}, t in {0, middle, last}, every buffer pre-filled with a sentinel byte pattern -- column t equals the inputs, every other
byte is untouched; strided and contiguous scalar inputs give the same bytes; the NaN flag is sticky.  Reward: the scripted case of the CPU test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops  # noqa: E402
from tests import rollout_ref as R  # noqa: E402

DEV = "cuda"
SENTINEL = 0xA5
FRAME = (128, 128, 3)
DTYPES = dict(img=torch.uint8, first=torch.uint8, act_buttons=torch.int64, act_camera=torch.int64, old_log_prob=torch.float32, vpred=torch.float32)
NP_DTYPES = {torch.uint8: np.uint8, torch.int64: np.int64, torch.float32: np.float32}
ITEMSIZE = {torch.uint8: 1, torch.int64: 8, torch.float32: 4}


def _sentinel_bufs(b, t_len):
    """Every buffer filled with the byte 0xA5 (as bytes: the fp32 / int64 views show whatever that spells)."""
    shapes = dict(img=(b, t_len) + FRAME, first=(b, t_len), act_buttons=(b, t_len), act_camera=(b, t_len), old_log_prob=(b, t_len), vpred=(b, t_len))
    bufs = {}
    for k, shape in shapes.items():
        raw = torch.full((int(np.prod(shape)) * ITEMSIZE[DTYPES[k]],), SENTINEL, dtype=torch.uint8, device=DEV)
        bufs[k] = raw.view(DTYPES[k]).view(shape)
    bufs["nan_flag"] = torch.zeros(1, dtype=torch.uint8, device=DEV)
    return bufs


def _inputs(b, seed, nan_at=None):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (b,) + FRAME, generator=g, dtype=torch.uint8)
    first = torch.tensor([(i + seed) % 2 == 0 for i in range(b)])
    packed = torch.zeros(b, 4, dtype=torch.int64)                      # ops.act_epilogue's record: buttons, camera, (log_prob, -), (vpred, raw vpred)
    packed[:, 0], packed[:, 1] = torch.randint(0, 8641, (b,), generator=g), torch.randint(0, 121, (b,), generator=g)
    pf = packed.view(torch.float32)
    pf[:, 4], pf[:, 6], pf[:, 7] = -torch.rand(b, generator=g) * 9, torch.randn(b, generator=g) * 3, torch.randn(b, generator=g)
    if nan_at is not None:
        pf[nan_at, 4] = float("nan")
    return img.to(DEV), first.to(DEV), packed.to(DEV)


def _record(bufs, t, img, first, scalars):
    ab, ac, lp, vp = scalars
    ops.rollout_record(img, first, ab, ac, lp, vp, t, bufs["img"], bufs["first"], bufs["act_buttons"], bufs["act_camera"], bufs["old_log_prob"],
                       bufs["vpred"], bufs["nan_flag"])


def _bytes(x):
    return x.contiguous().view(-1).view(torch.uint8).cpu().numpy()


@pytest.mark.parametrize("b,t_len", [(1, 1), (1, 5), (3, 1), (3, 5)])
def test_record_writes_column_t_and_nothing_else(b, t_len):
    for t in sorted({0, t_len // 2, t_len - 1}):
        img, first, packed = _inputs(b, seed=10 * t_len + t)
        strided = ops.unpack_act_keep(packed)[:4]                       # views: stride 4 int64 / 8 floats
        assert strided[0].stride() == (4,) and strided[2].stride() == (8,)
        contiguous = tuple(x.contiguous() for x in strided)
        out = {}
        for name, scalars in (("strided", strided), ("contiguous", contiguous)):
            bufs = _sentinel_bufs(b, t_len)
            _record(bufs, t, img, first, scalars)
            out[name] = bufs
        torch.cuda.synchronize()
        ref = {k: np.full(v.numel() * v.element_size(), SENTINEL, np.uint8).view(NP_DTYPES[v.dtype]).reshape(tuple(v.shape))
               for k, v in out["strided"].items() if k != "nan_flag"}
        ref["nan_flag"] = np.zeros(1, np.uint8)
        R.record(ref, t, img.cpu().numpy(), first.cpu().numpy(), *(x.cpu().numpy() for x in contiguous))
        for k in ref:
            want = np.ascontiguousarray(ref[k]).view(np.uint8).reshape(-1)
            assert np.array_equal(_bytes(out["strided"][k]), want), (k, b, t_len, t)                 # column t bit for bit, every other byte the sentinel
            assert np.array_equal(_bytes(out["contiguous"][k]), want), (k, b, t_len, t)
        others = [c for c in range(t_len) if c != t]
        assert bool((out["strided"]["img"][:, others] == SENTINEL).all()) and torch.equal(out["strided"]["img"][:, t], img)


def test_record_addresses_a_column_past_two_gib():
    """B = 1, T = 43700, t = T - 1: column t of img_buf starts 2 147 893 248 bytes into the buffer, past 2^31 (a 32-bit byte or vector-times-16 offset
    would wrap into the front of the buffer).  Checked on the device: column t equals the frame, every byte before it is still the sentinel."""
    b, t_len = 1, 43700
    t = t_len - 1
    assert t * int(np.prod(FRAME)) > 2 ** 31
    bufs = _sentinel_bufs(b, t_len)
    img, first, packed = _inputs(b, seed=4)
    _record(bufs, t, img, first, ops.unpack_act_keep(packed)[:4])
    assert torch.equal(bufs["img"][:, t], img)
    assert bool((bufs["img"][:, :t] == SENTINEL).all())
    assert int(bufs["act_buttons"][0, t]) == int(packed[0, 0]) and bool((bufs["first"][:, :t] == SENTINEL).all())


def test_record_nan_flag_is_sticky():
    b, t_len = 3, 5
    bufs = _sentinel_bufs(b, t_len)
    img, first, packed = _inputs(b, seed=1)
    _record(bufs, 0, img, first, ops.unpack_act_keep(packed)[:4])
    assert int(bufs["nan_flag"]) == 0                                   # no NaN seen
    for env in range(b):                                                # a NaN in any one environment's log-prob sets it
        flag_bufs = _sentinel_bufs(b, t_len)
        img_n, first_n, packed_n = _inputs(b, seed=2 + env, nan_at=env)
        _record(flag_bufs, 1, img_n, first_n, ops.unpack_act_keep(packed_n)[:4])
        assert int(flag_bufs["nan_flag"]) == 1, env
        assert bool(torch.isnan(flag_bufs["old_log_prob"][env, 1]))
    img_n, first_n, packed_n = _inputs(b, seed=7, nan_at=2)
    _record(bufs, 1, img_n, first_n, ops.unpack_act_keep(packed_n)[:4])
    assert int(bufs["nan_flag"]) == 1
    _record(bufs, 2, img, first, ops.unpack_act_keep(packed)[:4])       # a later clean step does not clear it
    assert int(bufs["nan_flag"]) == 1


def test_reward_equals_the_numpy_twin_step_by_step():
    reward, done, ret0, len0 = R.scripted_case()
    b, t_len = reward.shape
    ref = R.new_reward_bufs(b, t_len, ret0, len0)
    dev = dict(reward=torch.full((b, t_len), -7.0, device=DEV), done_return=torch.full((b, t_len), -7.0, device=DEV),
               done_length=torch.full((b, t_len), -7, dtype=torch.int32, device=DEV), ep_return=torch.from_numpy(ret0.copy()).to(DEV),
               ep_length=torch.from_numpy(len0.copy()).to(DEV))
    for t in range(t_len):
        R.reward_step(ref, t, reward[:, t], done[:, t])
        ops.rollout_reward(torch.from_numpy(reward[:, t].copy()).to(DEV), torch.from_numpy(done[:, t].copy()).to(DEV), t, dev["reward"],
                           dev["done_return"], dev["done_length"], dev["ep_return"], dev["ep_length"])
        for k in ("ep_return", "ep_length"):                            # the accumulators after every step
            assert torch.equal(dev[k].cpu(), torch.from_numpy(ref[k])), (k, t)
        for k in ("reward", "done_return", "done_length"):              # columns <= t written, columns > t untouched
            assert torch.equal(dev[k][:, :t + 1].cpu(), torch.from_numpy(ref[k][:, :t + 1])), (k, t)
            assert bool((dev[k][:, t + 1:] == -7).all()), (k, t)
    for k in ref:
        assert torch.equal(dev[k].cpu(), torch.from_numpy(ref[k])), k
    assert float(dev["done_return"][0, 3]) == 0.0                       # (2^24 + 1) - 2^24 added left to right; any re-association gives 1


def test_bad_arguments_raise():
    b, t_len = 3, 5
    bufs = _sentinel_bufs(b, t_len)
    img, first, packed = _inputs(b, seed=3)
    scalars = ops.unpack_act_keep(packed)[:4]
    before = {k: v.clone() for k, v in bufs.items()}
    with pytest.raises(ValueError, match="horizon"):
        _record(bufs, t_len, img, first, scalars)
    with pytest.raises(ValueError, match="horizon"):
        _record(bufs, -1, img, first, scalars)
    with pytest.raises(TypeError, match="img"):
        _record(bufs, 0, img.float(), first, scalars)
    img2, first2, packed2 = _inputs(2, seed=3)
    with pytest.raises(ValueError):
        _record(bufs, 0, img2, first, scalars)                          # two frames for three environments
    with pytest.raises(ValueError):
        _record(bufs, 0, img, first2, scalars)
    with pytest.raises(ValueError):
        _record(bufs, 0, img, first, ops.unpack_act_keep(packed2)[:4])
    rbufs = [torch.zeros(b, t_len, device=DEV), torch.zeros(b, t_len, device=DEV), torch.zeros(b, t_len, dtype=torch.int32, device=DEV),
             torch.zeros(b, device=DEV), torch.zeros(b, dtype=torch.int32, device=DEV)]
    r, d = torch.zeros(b, device=DEV), torch.zeros(b, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match="horizon"):
        ops.rollout_reward(r, d, t_len, *rbufs)
    with pytest.raises(ValueError):
        ops.rollout_reward(r[:2].contiguous(), d, 0, *rbufs)
    with pytest.raises(TypeError):
        ops.rollout_reward(r.double(), d, 0, *rbufs)
    torch.cuda.synchronize()
    assert all(torch.equal(bufs[k], before[k]) for k in bufs)           # a refused call has written nothing
