"""The video labeller's kernels on the GPU: the indexed temporal conv against the plain one run on gathered windows, the row gather
against index_select, and the label decoder against CPU twins (torch.argmax on the CPU, oracle/action_codec.py, a sequential fp32 sum)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import ops, packing  # noqa: E402
from oracle import action_codec as A  # noqa: E402

DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


# ---- indexed temporal conv -----------------------------------------------------------------------------------------------------
def _slots(n_frames):
    """The slots of the (20, 8, 4) labelling plan plus hand-made ones: one frame wide ([lo, hi) = [src, src + 1): only the centre tap reads),
    bounds beyond the tap range (all five taps read), and bounds outside the video (clipped to it)."""
    plan = packing.idm_feature_plan(n_frames, 8, 4)
    extra = [(5, 5, 6), (0, 0, 1), (19, 19, 20), (7, 0, 20), (10, 3, 17), (0, -3, 2), (19, 15, 25), (1, -7, 40), (12, 11, 13), (12, 12, 14)]
    src = plan.src.tolist() + [e[0] for e in extra]
    lo = plan.lo.tolist() + [e[1] for e in extra]
    hi = plan.hi.tolist() + [e[2] for e in extra]
    return src, lo, hi


@pytest.mark.parametrize("cout", [32, 128])
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_indexed_conv_equals_plain_conv_on_gathered_windows(mode, cout):
    g = torch.Generator().manual_seed(3)
    n = 20
    img = torch.randint(0, 256, (n, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
    weight = (torch.randn(cout, 3, 5, 1, 1, generator=g) * 0.4).to(DEV)
    bias = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    wfrag, bpad = ops.pack_conv3d_t5(weight, bias, dtype=DTYPES[mode])
    src, lo, hi = _slots(n)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    stats = torch.zeros(len(src), 2, dtype=torch.float64, device=DEV)
    y = ops.conv3d_t5_indexed(img, i32(src), i32(lo), i32(hi), wfrag, bpad, cout, stats_out=stats)
    assert y.shape == (len(src), cout // 32, 128, 128, 32) and y.dtype == DTYPES[mode]
    # reference: the plain kernel on the pixels of the window each slot stands for -- the frames its taps may read, as one sequence
    windows = sorted({(max(l, 0, s - 2), min(h, n, s + 3)) for s, l, h in zip(src, lo, hi)})
    ref = {}
    for a, b in windows:
        st = torch.zeros(b - a, 2, dtype=torch.float64, device=DEV)
        ref[(a, b)] = (ops.conv3d_t5(img[a:b].contiguous(), wfrag, bpad, cout, b - a, stats_out=st), st)
    exact_stats = 0
    for j, (s, l, h) in enumerate(zip(src, lo, hi)):
        a, b = max(l, 0, s - 2), min(h, n, s + 3)
        yr, sr = ref[(a, b)]
        assert torch.equal(y[j], yr[s - a]), (j, s, l, h)                      # the same bytes through the same MFMA
        # fp64 sums of the workgroups' fp32 partial sums in arrival order
        assert torch.allclose(stats[j], sr[s - a], rtol=1e-12, atol=0.0), (j, stats[j], sr[s - a])
        exact_stats += int(torch.equal(stats[j], sr[s - a]))
    print(f"indexed conv [{mode}, cout {cout}]: {len(src)} slots, {len(windows)} windows, statistics bit-equal in {exact_stats} slots")
    # 64 workgroups' partials per frame, all positive and within a few binades of each other: their fp64 sum is exact (24 + 6 + a few bits
    # of 53), so the order of arrival cannot show
    assert exact_stats == len(src)
    # a slot whose taps see a frame differs from the slot that sees zeros there (the index is honoured, not just the centre)
    one_wide, full = src.index(5, len(src) - 10), None
    for j, (s, l, h) in enumerate(zip(src, lo, hi)):
        if (s, l, h) == (5, 3, 8):
            full = j
    assert full is not None and not torch.equal(y[one_wide], y[full])


def test_indexed_conv_checks_its_arguments():
    img = torch.zeros(4, 128, 128, 3, dtype=torch.uint8, device=DEV)
    wfrag, bpad = ops.pack_conv3d_t5(torch.zeros(32, 3, 5, 1, 1, device=DEV), torch.zeros(32, device=DEV))
    idx = torch.zeros(3, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.conv3d_t5_indexed(img, idx, idx[:2], idx, wfrag, bpad, 32)
    with pytest.raises(TypeError):
        ops.conv3d_t5_indexed(img, idx.long(), idx, idx, wfrag, bpad, 32)


# ---- row gather ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [512, 4096])
def test_gather_rows_equals_index_select(d):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, d, generator=g).to(DEV)
    index = torch.tensor([36, 0, 0, 17, 5, 36, 36, 1, 2, 3, 35, 18, 17, 0] + torch.randint(0, 37, (301,), generator=g).tolist(), dtype=torch.int32, device=DEV)
    y = ops.gather_rows(x, index)
    assert y.shape == (index.numel(), d) and torch.equal(y, x.index_select(0, index.long()))
    out = torch.full((index.numel(), d), 7.0, device=DEV)
    assert ops.gather_rows(x, index, out=out) is out and torch.equal(out, y)
    # an index outside the input is a row of zeros, never a read outside x
    bad = torch.tensor([3, -1, 37, 4], dtype=torch.int32, device=DEV)
    yb = ops.gather_rows(x, bad)
    assert torch.equal(yb[0], x[3]) and torch.equal(yb[3], x[4]) and not yb[1].any() and not yb[2].any()
    with pytest.raises(ValueError):
        ops.gather_rows(x[:, :6].contiguous(), index)


# ---- label decode ----------------------------------------------------------------------------------------------------------------
NEG_INF = float("-inf")


def _decode_inputs(n_bins=11):
    """64 constructed rows + 256 random ones -> (log-probs buttons [320, 20, 2], camera [320, 2, n_bins]) on the CPU."""
    g = torch.Generator().manual_seed(11)
    lb = torch.log_softmax(torch.randn(320, 20, 2, generator=g) * 1.5, -1)
    lc = torch.log_softmax(torch.randn(320, 2, n_bins, generator=g) * 1.5, -1)
    mid = n_bins // 2
    off, on = torch.tensor([-0.25, -1.5]), torch.tensor([-1.5, -0.25])

    def buttons(r, pressed):
        lb[r] = off
        for b in pressed:
            lb[r, b] = on

    def camera(r, c0, c1):
        lc[r] = -3.0
        lc[r, 0, c0] = -0.5
        lc[r, 1, c1] = -0.5

    for r in range(64):
        kind = r % 8
        if kind == 0:        # exact ties everywhere: the lowest index wins -> nothing pressed, camera bin 0 / the first of two maxima
            lb[r] = -0.6931472
            lc[r] = -2.3978953
            if r >= 32:
                lc[r, 0, [3, 7]] = -1.0
                lc[r, 1, [9, 10]] = -1.0
        elif kind == 1:      # all null: nothing pressed, camera at the centre
            buttons(r, [])
            camera(r, mid, mid)
        elif kind == 2:      # inventory together with other buttons: the joint index is "inventory", the joint camera the centre
            buttons(r, [A.IDX["inventory"], A.IDX["attack"], A.IDX["forward"], A.IDX["hotbar.3"]][: 1 + r // 8 % 4 + 1])
            camera(r, (r // 8) % n_bins, 2)
        elif kind == 3:      # forward + back (and left + right) pressed together cancel
            buttons(r, [A.IDX["forward"], A.IDX["back"]] + ([A.IDX["left"], A.IDX["right"], A.IDX["jump"]] if r >= 32 else []))
            camera(r, 4, 6)
        elif kind == 4:      # camera at the centre in ONE axis only: not null, camera meta action on
            buttons(r, [])
            camera(r, *((mid, (r // 8) % n_bins) if r < 32 else (r // 8 - 3, mid)))
        elif kind == 5:      # -inf among the losers, and a masked-out winner's neighbour (LOG0 = -100 in this project's heads)
            buttons(r, [A.IDX["use"], A.IDX["sneak"], A.IDX["sprint"]])
            lb[r, 0, 1] = NEG_INF
            lb[r, 1, 1] = -100.0
            camera(r, 1, 9)
            lc[r, 0, 2:] = NEG_INF
            lc[r, 1, :9] = -100.0
        elif kind == 6:      # a group that is -inf throughout: index 0, and the frame's log-prob is -inf
            buttons(r, [A.IDX["drop"]])
            lb[r, 5] = NEG_INF
            camera(r, mid, mid)
            if r >= 32:
                lc[r, 1] = NEG_INF
        else:                # several hotbar keys and sprint + sneak: the later button of a group wins
            buttons(r, [A.IDX["hotbar.2"], A.IDX["hotbar.7"], A.IDX["hotbar.9"], A.IDX["sprint"], A.IDX["sneak"]][r // 8 % 3:])
            camera(r, mid, mid)
    return lb.contiguous(), lc.contiguous()


def _decode_twin(lb, lc):
    """The CPU twin of vpt_idm_decode."""
    n, n_bins = lb.shape[0], lc.shape[2]
    buttons, camera = torch.argmax(lb, -1), torch.argmax(lc, -1)                     # CPU torch.argmax: the first maximum
    chosen = torch.cat([lb.gather(-1, buttons[..., None])[..., 0], lc.gather(-1, camera[..., None])[..., 0]], 1).numpy()      # [n, 22], buttons first
    lp = chosen[:, 0].astype(np.float32).copy()
    for k in range(1, 22):
        lp = (lp + chosen[:, k]).astype(np.float32)                                  # left to right, one fp32 rounding per addition
    jb, jc = A.from_factored(buttons.numpy(), camera.numpy(), n_bins)
    deg = A.undiscretize(camera.numpy())
    null = ((buttons.sum(1) == 0) & (camera == n_bins // 2).all(1)).to(torch.uint8)
    return dict(buttons=buttons, camera=camera, log_prob=torch.from_numpy(lp), joint_buttons=torch.from_numpy(jb), joint_camera=torch.from_numpy(jc),
                camera_deg=torch.from_numpy(deg), null=null)


def test_decode_bit_for_bit_with_the_cpu_twin():
    lb, lc = _decode_inputs()
    want = _decode_twin(lb, lc)
    got = {k: v.cpu() for k, v in ops.idm_decode(lb.to(DEV), lc.to(DEV)).items()}
    assert got["buttons"].dtype == torch.int64 and got["camera"].dtype == torch.int64 and got["log_prob"].dtype == torch.float32
    assert got["joint_buttons"].dtype == torch.int64 and got["camera_deg"].dtype == torch.float64 and got["null"].dtype == torch.uint8
    # the constructed rows do what they were constructed for
    assert int(want["null"][:64].sum()) == 8 and int((want["joint_buttons"][:64] == A.JOINT_INVENTORY).sum()) == 8
    assert bool(torch.isinf(want["log_prob"][:64]).any()) and not bool(torch.isnan(want["log_prob"]).any())
    d_deg = (got["camera_deg"] - want["camera_deg"]).abs().max().item()
    print(f"decode: camera_deg max|d| vs numpy {d_deg:.3e}; nulls {int(want['null'].sum())}, inventory rows {int((want['joint_buttons'] == A.JOINT_INVENTORY).sum())}")
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and g.dtype == w.dtype, k
        if g.dtype.is_floating_point:        # bit for bit: the same float, -inf included
            assert torch.equal(g.view(torch.int64 if g.dtype == torch.float64 else torch.int32), w.view(torch.int64 if w.dtype == torch.float64 else torch.int32)), k
        else:
            assert torch.equal(g, w), k
    # and the decoder is the codec: the stand-alone codec kernels give the same joint indices and angles from its labels
    jb, jc = ops.action_from_factored(got["buttons"].to(DEV), got["camera"].to(DEV), 11)
    assert torch.equal(jb.cpu(), got["joint_buttons"]) and torch.equal(jc.cpu(), got["joint_camera"])
    assert torch.equal(ops.camera_undiscretize(got["camera"].to(DEV), 10, 2, 10, True).cpu(), got["camera_deg"])


def test_decode_returns_the_reference_joint_indices_of_golden_actions():
    """Real pairs of the live reference (tests/golden/actions_seed0.npz): its factored actions as one-hot log-probs must come back as its
    joint indices.  Rows with a button value other than 0 / 1 are left out: a two-way head cannot express them."""
    G = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "actions_seed0.npz")))
    keep = (G["buttons"] <= 1).all(1)
    assert keep.sum() > 4000
    buttons, camera = torch.from_numpy(G["buttons"][keep]), torch.from_numpy(G["camera"][keep])
    lb = torch.full((buttons.shape[0], 20, 2), NEG_INF).scatter_(2, buttons[..., None], 0.0)
    lc = torch.full((buttons.shape[0], 2, 11), NEG_INF).scatter_(2, camera[..., None], 0.0)
    got = ops.idm_decode(lb.to(DEV), lc.to(DEV))
    assert torch.equal(got["buttons"].cpu(), buttons) and torch.equal(got["camera"].cpu(), camera)
    assert np.array_equal(got["joint_buttons"].cpu().numpy(), G["ff_buttons"][keep, 0])
    assert np.array_equal(got["joint_camera"].cpu().numpy(), G["ff_camera"][keep, 0])
    assert not got["log_prob"].cpu().any()                  # 22 times log 1


def test_decode_checks_its_arguments():
    with pytest.raises(ValueError):
        ops.idm_decode(torch.zeros(4, 20, 2, device=DEV), torch.zeros(4, 2, 10, device=DEV))
    with pytest.raises(ValueError):
        ops.idm_decode(torch.zeros(4, 19, 2, device=DEV), torch.zeros(4, 2, 11, device=DEV))
