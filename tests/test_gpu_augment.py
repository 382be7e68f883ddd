"""Sequence-consistent frame augmentation on the GPU (csrc/vpt_augment.hip, vpt_amd.augment): the kernel against the float32 numpy restatement
(tests/augment_ref.py) under torch.equal -- no tolerance anywhere -- at frame sizes that take the byte paths (5 x 7: frame 1 starts unaligned), several
vectors per thread (128 x 128) and the LDS limit (147 x 148); the Philox uniforms bit for bit; FrameAugmenter end to end, across a chunk edge; and one
IDMTrainer / BCTrainer step on an augmented chunk (wiring only).  No test feeds non-finite tables: tests/test_augment_host_cpu.py covers those on the
host.  Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import _native, ops  # noqa: E402
from vpt_amd.augment import FrameAugmenter, IDENTITY_TABLE  # noqa: E402
from tests import augment_ref as R  # noqa: E402

DEV = "cuda"
SHAPES = [(3, 5, 7), (3, 16, 16), (1, 33, 20), (6, 128, 128), (1, 147, 148)]          # (6, 128, 128) runs as B = 2 x T = 3


def _params(**kw):
    p = R.IDENTITY_PARAMS.copy()
    for k, v in kw.items():
        p[("hue", "sat", "bri", "con", "rot", "scl", "shr", "tx", "ty").index(k)] = v
    return p


def _tables(f, h, w):
    """name -> fp32 tables [f, 16] (numpy)."""
    rng = np.random.default_rng(1000 * h + w)
    one = lambda p: np.repeat(R.tables_ref(p, h, w).astype(np.float32), f, axis=0)
    cases = {
        "identity": np.repeat(R.IDENTITY_TABLE[None], f, axis=0),
        "translation": np.repeat(R.translation_table(2.0, -1.0)[None], f, axis=0),
        "default ranges": R.tables_ref(R.params_ref(rng.random((f, 9))), h, w).astype(np.float32),      # a different table per frame
        "rotation 180": one(_params(rot=180.0)),
        "scale 0.5": one(_params(scl=0.5, rot=1.0)),
        "scale 2": one(_params(scl=2.0, shr=3.0)),
        "both clamps": one(_params(bri=3.0, con=-1.0)),                    # o = 6 mu - 3 v: 255 for dark pixels, about 0 for v = 255
        "both clamps, steep": one(_params(bri=3.0, con=3.0, hue=0.1)),     # o = 9 v - 6 mu: below 0 for v < 85, above 255 for v > 113
        "all taps outside": one(_params(con=0.5, tx=1000.0)),
    }
    names = list(cases)
    cases["mixed"] = np.stack([cases[names[(i + 2) % len(names)]][i] for i in range(f)])                 # different kinds inside one launch
    return cases


_CACHE = {}


def _case(shape):
    """(img uint8 numpy [f, h, w, 3], {name: (tables, reference output)}), computed once per shape and left unchanged."""
    if shape not in _CACHE:
        f, h, w = shape
        img = np.random.default_rng(7 * h + w).integers(0, 256, (f, h, w, 3), dtype=np.uint8)
        _CACHE[shape] = (img, {name: (t, R.augment_frames_ref(img, t)) for name, t in _tables(f, h, w).items()})
    return _CACHE[shape]


def _run(img, tables, **kw):
    out = ops.augment_frames(img, torch.from_numpy(tables).to(DEV), **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_restatement(shape):
    f, h, w = shape
    img_np, cases = _case(shape)
    img = torch.from_numpy(img_np).to(DEV)
    if shape == (6, 128, 128):
        img = img.view(2, 3, h, w, 3)
    for name, (tables, want) in cases.items():
        got = _run(img, tables)
        assert got.shape == img.shape and got.dtype == torch.uint8
        assert torch.equal(got.cpu().view(f, h, w, 3), torch.from_numpy(want)), (shape, name)
    assert torch.equal(_run(img, cases["identity"][0]), img)
    want = cases["all taps outside"][1]
    assert all(len(np.unique(want[i])) == 1 for i in range(f))              # the constant rint(k mu) ...
    assert int(want.max()) > 0                                              # ... which is not the zero fill
    assert int(cases["both clamps"][1].max()) == 255
    assert int(cases["both clamps, steep"][1].max()) == 255 and int(cases["both clamps, steep"][1].min()) == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_in_place_repeat_stream_and_both_libraries(shape):
    f, h, w = shape
    img_np, cases = _case(shape)
    tables, want = cases["default ranges"]
    want = torch.from_numpy(want)
    img = torch.from_numpy(img_np).to(DEV)
    buf = img.clone()
    assert ops.augment_frames(buf, torch.from_numpy(tables).to(DEV), out=buf) is buf
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), want)                                     # out = img: the frame is whole in LDS before the first store
    assert torch.equal(_run(img, tables), _run(img, tables))
    assert torch.equal(img.cpu(), torch.from_numpy(img_np))                 # the input is left alone
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = ops.augment_frames(img, torch.from_numpy(tables).to(DEV))
    s.synchronize()
    assert torch.equal(got.cpu(), want)
    assert torch.equal(_run(img, tables, fmt="fp16").cpu(), want)
    for fmt in ("bf16", "fp16"):
        assert hasattr(_native.load(fmt), "vpt_augment_frames") and hasattr(_native.load(fmt), "vpt_augment_uniforms")


def test_argument_checks():
    t = torch.tensor(IDENTITY_TABLE, device=DEV)[None]
    with pytest.raises(ValueError):
        ops.augment_frames(torch.zeros(1, 148, 148, 3, dtype=torch.uint8, device=DEV), t)              # 65 712 bytes: over the LDS limit
    img = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.augment_frames(img, t)                                                                      # one table per frame
    with pytest.raises(TypeError):
        ops.augment_frames(img.float(), t.expand(2, 16).contiguous())
    with pytest.raises(ValueError):
        ops.augment_frames(img, t.expand(2, 16).contiguous(), out=torch.zeros(2, 16, 16, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError):
        ops.augment_frames(img.cpu(), t.expand(2, 16).contiguous())
    torch.cuda.synchronize()


def test_uniforms_equal_the_philox_restatement():
    keys = np.array([0, -1, 2 ** 31, 2 ** 40 + 3, 5, 5, 0, 123456789, -7], dtype=np.int64)
    seen = []
    for seed in (0, 0x1234567890ABCDEF):
        for epoch in (0, 7):
            want = R.uniforms_ref(keys, seed, epoch)
            for fmt in ("bf16", "fp16"):
                got = ops.augment_uniforms(torch.from_numpy(keys).to(DEV), seed, epoch, fmt=fmt)
                torch.cuda.synchronize()
                assert got.dtype == torch.float32 and tuple(got.shape) == (len(keys), 9)
                assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (seed, epoch, fmt)
            assert np.array_equal(want[4], want[5]) and np.array_equal(want[0], want[6]) and not np.array_equal(want[0], want[1])
            assert (want >= 0).all() and (want < 1).all()
            seen.append(want)
    assert all(not np.array_equal(a, b) for i, a in enumerate(seen) for b in seen[i + 1:])


def test_frame_augmenter_end_to_end():
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (2, 3, 128, 128, 3), generator=g, dtype=torch.uint8)
    ids = torch.tensor([[4, 4, 9], [7, 7, -1]], dtype=torch.int64)
    chunk = dict(img=img.to(DEV), episode_id=ids.to(DEV), first=torch.zeros(2, 3, dtype=torch.bool, device=DEV))
    aug = FrameAugmenter(seed=11)
    out = aug(chunk)
    torch.cuda.synchronize()
    assert out is not chunk and out["first"] is chunk["first"] and out["episode_id"] is chunk["episode_id"] and out["img"] is not chunk["img"]
    assert torch.equal(chunk["img"].cpu(), img)
    tables = aug.tables(chunk["episode_id"], 128, 128).cpu()
    assert torch.equal(tables[0], tables[1]) and torch.equal(tables[3], tables[4])                     # ids 4, 4 and 7, 7
    assert len({tuple(tables[i].tolist()) for i in (0, 2, 3, 5)}) == 4                                 # 4, 9, 7 and the padding: four tables
    assert torch.equal(tables[5], torch.tensor(IDENTITY_TABLE))
    assert torch.equal(out["img"][1, 2].cpu(), img[1, 2])                                              # the padding frame is unchanged
    assert not torch.equal(out["img"][0, 0].cpu(), img[0, 0])
    want = R.augment_frames_ref(img.numpy(), tables.numpy())
    assert torch.equal(out["img"].cpu(), torch.from_numpy(want))
    # a second chunk continues recording 9: the table recording 9 had (the chunk-edge case), by construction
    ids2 = torch.tensor([[9, 9, 12], [7, 3, 3]], dtype=torch.int64, device=DEV)
    tables2 = aug.tables(ids2, 128, 128).cpu()
    assert torch.equal(tables2[0], tables[2]) and torch.equal(tables2[1], tables[2]) and torch.equal(tables2[3], tables[3])
    out2 = aug(dict(img=chunk["img"], episode_id=ids2))["img"]
    assert torch.equal(out2[0, 0].cpu(), torch.from_numpy(R.augment_frame_ref(img[0, 0].numpy(), tables[2].numpy())))
    # keys per row, and keyless calls: a fresh key per row and call; a state_dict round trip reproduces the next call
    assert torch.equal(aug.apply(chunk["img"], torch.tensor([4, 7], device=DEV))[0].cpu(), torch.from_numpy(R.augment_frames_ref(img[0].numpy(), tables[:1].expand(3, 16).numpy())))
    a = aug.apply(chunk["img"])
    state = aug.state_dict()
    b = aug.apply(chunk["img"])
    assert state == dict(seed=11, epoch=0, calls=1) and not torch.equal(a, b)
    fresh = FrameAugmenter(seed=0)
    fresh.load_state_dict(state)
    assert torch.equal(fresh.apply(chunk["img"]), b)
    aug.epoch = 1                                                           # a new epoch redraws every recording
    assert not torch.equal(aug.tables(chunk["episode_id"], 128, 128).cpu()[0], tables[0])
    torch.cuda.synchronize()


def test_trainers_step_on_an_augmented_chunk():
    """Wiring only: the trainers take the augmenter's uint8 frames as they take any others."""
    from vpt_amd.idm_training import IDMTrainer
    from vpt_amd.lib.policy import InverseActionPolicy, MinecraftAgentPolicy
    from vpt_amd.lib.types import idm_action_space, minecraft_action_space
    from vpt_amd.training import BCTrainer
    from oracle import vpt_oracle as O
    from tests import labeler_ref as L
    from tests import parity as P
    b, t = 2, 4
    g = torch.Generator().manual_seed(31)
    chunk = dict(img=P.structured_frames(b, t, g).to(DEV), episode_id=torch.tensor([[1, 1, 1, 2], [3, 3, 3, 3]], device=DEV))
    img = FrameAugmenter(seed=2)(chunk)["img"]
    assert img.dtype == torch.uint8 and img.shape == chunk["img"].shape and not torch.equal(img, chunk["img"])

    kw, _, sd = L.tiny_idm()
    idm = InverseActionPolicy(idm_action_space(), pi_head_kwargs=dict(temperature=L.TEMPERATURE), idm_net_kwargs=kw, precision="bf16")
    idm.load_state_dict(sd, strict=False)
    loss = IDMTrainer(idm.to(DEV), lr=1e-4).step(img, torch.randint(0, 2, (b, t, 20), generator=g).to(DEV), torch.randint(0, 11, (b, t, 2), generator=g).to(DEV))
    assert np.isfinite(float(loss))

    pk = O.policy_kwargs_for("1x")
    cfg = O.config_from_policy_kwargs(pk, dict(temperature=2.0))
    pol = MinecraftAgentPolicy(minecraft_action_space(), pk, dict(temperature=2.0), precision="bf16")
    pol.load_state_dict(O.synthetic_state_dict(cfg, seed=0), strict=False)
    pol = pol.to(DEV)
    loss, _ = BCTrainer(pol, lr=1e-4).step(img, torch.zeros(b, t, dtype=torch.bool, device=DEV), pol.initial_state(b),
                                           torch.randint(0, 8641, (b, t), generator=g).to(DEV), torch.randint(0, 121, (b, t), generator=g).to(DEV))
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
