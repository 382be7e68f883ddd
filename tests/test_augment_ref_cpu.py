"""The frame augmentation's restatement (tests/augment_ref.py), its table builder (vpt_amd.augment) and the optional hooks, on the CPU.

The GPU tests hold the kernel to augment_ref bit for bit; here augment_ref itself is held to exact cases (identity, an integer translation) and
to an independent float64 route through torch's grid_sample, and the torch-op table builder to the float64 restatement of the formulas."""
import warnings

import numpy as np
import pytest
import torch

import vpt_amd  # noqa: F401
from vpt_amd.augment import FrameAugmenter, IDENTITY_TABLE, tables_from_params
from vpt_amd.labeler import labelled_chunks
from vpt_amd.sequence_batcher import SequenceBatcher
from tests import augment_ref as R
from tests.test_labelled_chunks_cpu import _video as labelled_video
from tests.test_sequence_batcher_cpu import _blank_processor, _loader, dataset, oracle_encoder  # noqa: F401  (dataset: a fixture)

SIZES = [(128, 128), (5, 7), (16, 16), (33, 20)]
# wide ranges: both clamps, large rotations, taps far outside
EXTREME_RANGES = ((-0.5, 0.5), (0.0, 2.0), (0.3, 3.0), (-1.0, 2.0), (-180.0, 180.0), (0.5, 2.0), (-30.0, 30.0), (-20.0, 20.0), (-20.0, 20.0))


def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("hw", SIZES)
def test_identity_table_returns_the_input(hw):
    img = _image(*hw, seed=1)
    assert np.array_equal(R.augment_frame_ref(img, R.IDENTITY_TABLE), img)
    # ... and identity PARAMETERS give that table exactly, from both builders
    assert np.array_equal(R.tables_ref(R.IDENTITY_PARAMS, *hw).astype(np.float32)[0], R.IDENTITY_TABLE)
    t = tables_from_params(torch.from_numpy(R.IDENTITY_PARAMS)[None], *hw)
    assert t.dtype == torch.float32 and t[0].tolist() == list(IDENTITY_TABLE)
    assert not np.signbit(t.numpy()).any()


@pytest.mark.parametrize("hw", SIZES)
def test_integer_translation_shifts_with_zero_fill(hw):
    h, w = hw
    img = _image(h, w, seed=2)
    want = np.zeros_like(img)
    want[:h - 1, 2:] = img[1:, :w - 2]                      # forward translation by (+2, -1): out(x, y) = src(x - 2, y + 1)
    assert np.array_equal(R.augment_frame_ref(img, R.translation_table(2.0, -1.0)), want)
    p = R.IDENTITY_PARAMS.copy()
    p[7], p[8] = 2.0, -1.0
    assert np.array_equal(R.tables_ref(p, h, w).astype(np.float32)[0], R.translation_table(2.0, -1.0))
    assert np.array_equal(tables_from_params(torch.from_numpy(p)[None], h, w)[0].numpy(), R.translation_table(2.0, -1.0))


def _route_differences(ranges, per_size, seed):
    rng = np.random.default_rng(seed)
    total = ones = worst = 0
    for h, w in SIZES:
        for _ in range(per_size):
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            table = R.tables_ref(R.params_ref(rng.random(9), ranges), h, w).astype(np.float32)[0]
            d = np.abs(R.augment_frame_ref(img, table).astype(np.int64) - R.grid_sample_route(img, table).astype(np.int64))
            total, ones, worst = total + d.size, ones + int((d == 1).sum()), max(worst, int(d.max()))
    return total, ones, worst


def test_restatement_agrees_with_an_independent_grid_sample_route():
    """float32 restatement against a float64 route through F.grid_sample(padding_mode="zeros", align_corners=False) plus the colour map: 40 seeded draws
    in the default ranges and 24 at extreme parameters (10 and 6 per size).  No element may differ by more than one level, and at most 1e-3 of the
    elements by one: the cap keeps a wrong formula from hiding behind rounding.
    Measured with these seeds: default ranges 105 of 520 050 elements differ by one (2.0e-4); extremes 58 of 312 030 (1.9e-4); none by two."""
    for name, ranges, per_size, seed in (("default", R.DEFAULT_RANGES, 10, 1234), ("extreme", EXTREME_RANGES, 6, 4321)):
        total, ones, worst = _route_differences(ranges, per_size, seed)
        print(f"augment routes [{name}]: {ones} of {total} elements differ by one ({ones / total:.2e}), largest difference {worst}")
        assert total == 52005 * per_size
        assert worst <= 1, (name, worst)
        assert ones <= 1e-3 * total, (name, ones, total)


def _ulp_ok(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_tables_match_the_float64_restatement():
    """augment.tables on CPU tensors (torch ops in float64, rounded to fp32) against tables_ref rounded to fp32: within 1 fp32 ulp per entry.
    Measured: 1536 of 1536 entries are bit-equal, in the default ranges and in the extreme ones."""
    keys = torch.arange(1, 97, dtype=torch.int64)
    for name, ranges in (("default", R.DEFAULT_RANGES), ("extreme", EXTREME_RANGES)):
        names = ("hue", "saturation", "brightness", "contrast", "rotation_deg", "scale", "shear_deg", "translate_px")
        aug = FrameAugmenter(seed=5, **dict(zip(names, ranges[:8])))
        aug.epoch = 2
        u = R.uniforms_ref(keys.numpy(), 5, 2)
        got = aug.tables(keys, 33, 20, uniforms=torch.from_numpy(u)).numpy()
        want = R.tables_ref(R.params_ref(u, ranges), 33, 20).astype(np.float32)
        assert got.dtype == np.float32 and got.shape == (96, 16)
        print(f"augment tables [{name}]: {int((got == want).sum())} of {got.size} entries bit-equal")
        assert _ulp_ok(got, want).all(), np.abs(got - want).max()


def test_tables_keys_epochs_and_seeds():
    keys = torch.tensor([3, -1, 7, 3, -5, 2 ** 40 + 3], dtype=torch.int64)

    def tables(seed, epoch):
        aug = FrameAugmenter(seed=seed)
        aug.epoch = epoch
        return aug.tables(keys, 16, 16, uniforms=torch.from_numpy(R.uniforms_ref(keys.numpy(), seed, epoch)))

    t = tables(0, 0)
    ident = torch.tensor(IDENTITY_TABLE)
    assert torch.equal(t[1], ident) and torch.equal(t[4], ident)            # negative keys: the identity row
    assert torch.equal(t[0], t[3])                                          # equal keys: equal rows
    assert not torch.equal(t[0], t[2]) and not torch.equal(t[0], t[5]) and not torch.equal(t[0], ident)
    for other in (tables(0, 1), tables(1, 0)):                             # another epoch, another seed: other rows; the identity rows stay
        assert not torch.equal(other[0], t[0]) and not torch.equal(other[2], t[2])
        assert torch.equal(other[1], ident)
    assert torch.equal(tables(0, 0), t)


def test_switched_off_terms_are_exact_identities():
    aug = FrameAugmenter(seed=0, hue=None, saturation=None, brightness=None, contrast=None, rotation_deg=None, scale=None, shear_deg=None, translate_px=None)
    keys = torch.arange(8, dtype=torch.int64)
    t = aug.tables(keys, 5, 7, uniforms=torch.from_numpy(R.uniforms_ref(keys.numpy(), 0, 0)))
    assert torch.equal(t, torch.tensor(IDENTITY_TABLE).expand(8, 16))
    with pytest.raises(ValueError):
        FrameAugmenter(scale=(0.0, 1.0))
    aug.epoch, aug.calls = 4, 9
    fresh = FrameAugmenter(seed=3)
    fresh.load_state_dict(aug.state_dict())
    assert (fresh.seed, fresh.epoch, fresh.calls) == (0, 4, 9)


def _stub(chunk):
    out = dict(chunk)
    out["img"] = 255 - chunk["img"]
    return out


def test_sequence_batcher_hook(dataset):  # noqa: F811
    root, lengths, videos = dataset

    def run(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return list(SequenceBatcher(_loader(root, videos, 2), 4, action_encoder=oracle_encoder, pad_last=True, **kw))

    today, off, stub = run(), run(augment=None), run(augment=_stub)
    assert len(today) == len(off) == len(stub) >= 2
    for a, b, c in zip(today, off, stub):
        assert a.keys() == b.keys() == c.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k                              # augment=None: what it produces today
            assert torch.equal(c[k], 255 - a[k] if k == "img" else a[k]), k
    assert any(int(c["img"].max()) > 0 for c in today)
    with pytest.raises(TypeError):
        SequenceBatcher(_loader(root, videos, 2, processor=_blank_processor), 4, oracle_encoder, True, _stub)      # keyword-only


def test_labelled_chunks_hook():
    vids = [labelled_video(9, 0), labelled_video(5, 1), labelled_video(7, 2)]
    today = list(labelled_chunks(vids, n_rows=2, seq_len=4, drop_null=False))
    off = list(labelled_chunks(vids, n_rows=2, seq_len=4, drop_null=False, augment=None))
    seen = []

    def stub(chunk):
        seen.append(chunk)
        return _stub(chunk)

    on = list(labelled_chunks(vids, n_rows=2, seq_len=4, drop_null=False, augment=stub))
    assert len(today) == len(off) == len(on) == len(seen) >= 2
    for a, b, c, s in zip(today, off, on, seen):
        assert a.keys() == b.keys() == c.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k
            assert torch.equal(c[k], 255 - a[k] if k == "img" else a[k]), k
            assert k == "img" or c[k] is s[k]                              # everything but img: the same objects
    with pytest.raises(TypeError):
        labelled_chunks(vids, 2, 4, False, _stub)                          # keyword-only
