"""Episode starts honoured at EVERY frame of a [B, T] chunk (episode_starts="frame"): the bounds kernel, the attention forward and backward
with qlo, the policy, the trainer and the loader -> SequenceBatcher -> BCTrainer path.  The semantics are the reference's own, stepped
one frame at a time with one hidden state per episode (behavioural_cloning.py:95-112 over lib/masked_attention.py:161-178); a chunk in
the new mode must equal that stepping.  The default ("chunk": first[:, 0] only) must not move.  Needs an MI355X."""
import gzip
import json
import os
import random
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd import clip, clip_loader, ops, packing  # noqa: E402
from vpt_amd.sequence_batcher import SequenceBatcher  # noqa: E402
from vpt_amd.training import BCTrainer  # noqa: E402
from vpt_amd.lib.policy import MinecraftAgentPolicy  # noqa: E402
from vpt_amd.lib.types import minecraft_action_space  # noqa: E402
from oracle import action_codec as A  # noqa: E402
from oracle import vpt_oracle as O  # noqa: E402
from tests import parity as P  # noqa: E402

DEV = "cuda"


def _l2(a, ref):
    return float((a - ref).norm() / ref.norm().clamp(min=1e-30))


def _first(b, t, where):
    f = torch.zeros(b, t, dtype=torch.bool)
    for row, ps in where.items():
        for p in ps:
            f[row, p] = True
    return f


# ---------------------------------------------------------------------------------------------------------
# 1. the bounds kernel
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bsz,t,maxlen", [(3, 1, 128), (3, 63, 128), (2, 64, 128), (2, 65, 16), (1, 200, 128)])
def test_episode_bounds_kernel_equals_the_host_twin(bsz, t, maxlen):
    g = torch.Generator().manual_seed(1000 * t + maxlen)
    patterns = [torch.rand(bsz, t, generator=g) < 0.1, torch.zeros(bsz, t, dtype=torch.bool), torch.ones(bsz, t, dtype=torch.bool),
                _first(bsz, t, {r: [t - 1] for r in range(bsz)}), _first(bsz, t, {0: [0], bsz - 1: [t // 2, t - 1]})]
    for first in patterns:
        state_mask = torch.rand(bsz, maxlen, generator=g) > 0.3
        want_q, want_m = packing.episode_bounds(first, state_mask, maxlen)
        qlo, m8 = ops.episode_bounds(first.to(DEV), state_mask.to(DEV), maxlen)
        assert qlo.dtype == torch.int32 and m8.dtype == torch.uint8
        assert torch.equal(qlo.cpu(), want_q) and torch.equal(m8.cpu().view(torch.bool), want_m)
        q_only, none = ops.episode_bounds(first.to(DEV), None, maxlen, want_mask=False)
        none2, m_only = ops.episode_bounds(first.to(DEV), state_mask.to(DEV), maxlen, want_qlo=False)
        assert none is None and none2 is None and torch.equal(q_only, qlo) and torch.equal(m_only, m8)
    with pytest.raises(RuntimeError, match="vpt_episode_bounds"):
        m = state_mask.to(DEV).view(torch.uint8)
        vpt_amd._native.call("vpt_episode_bounds", ops.ptr(first.to(DEV).view(torch.uint8)), ops.ptr(m), None, ops.ptr(m), bsz, t, maxlen, None)


# ---------------------------------------------------------------------------------------------------------
# 2. / 3. attention forward and backward with qlo against fp32 CPU attention with the explicit visibility
# ---------------------------------------------------------------------------------------------------------
ATT_CASES = [(2, 70, 128, {0: [31, 32, 33], 1: [0, 69]}),     # starts around a query-tile edge; at the first and the last frame
             (1, 200, 128, {0: [150]}),                        # queries beyond 128 reach the band's fifth key tile
             (2, 40, 16, {0: [5, 20], 1: [5, 20]})]            # maxlen below the tile
_ATT_CACHE = {}


def _attention_case(idx):
    """Inputs + the CPU reference (output and autograd gradients) of one case, computed once."""
    if idx in _ATT_CACHE:
        return _ATT_CACHE[idx]
    bsz, t, maxlen, where = ATT_CASES[idx]
    heads = 2
    g = torch.Generator().manual_seed(40 + idx)
    hid = heads * 128
    ld = 3 * hid + 10 * heads
    qkvr = torch.randn(bsz * t, ld, generator=g)
    qkvr[:, :hid] *= 2.0
    qkvr.requires_grad_(True)
    kmem = torch.randn(bsz, maxlen, hid, generator=g)
    vmem = torch.randn(bsz, maxlen, hid, generator=g)
    state_mask = torch.rand(bsz, maxlen, generator=g) > 0.3
    first = _first(bsz, t, where)
    b_nd = (0.5 * torch.randn(10, maxlen, generator=g)).requires_grad_(True)
    dout = torch.randn(bsz * t, hid, generator=g)
    qlo, _ = packing.episode_bounds(first, state_mask, maxlen)
    i = torch.arange(t).view(1, t, 1)
    j = torch.arange(t + maxlen).view(1, 1, t + maxlen)
    rows = torch.cat([state_mask, torch.ones(bsz, t, dtype=torch.bool)], 1)
    vis = (j >= i + 1) & (j <= i + maxlen) & (j >= qlo.view(bsz, t, 1).long()) & rows.view(bsz, 1, -1)
    q = qkvr[:, :hid].reshape(bsz, t, heads, 128).permute(0, 2, 1, 3)
    k_full = torch.cat([kmem, qkvr[:, hid:2 * hid].reshape(bsz, t, hid)], 1)
    v_full = torch.cat([vmem, qkvr[:, 2 * hid:3 * hid].reshape(bsz, t, hid)], 1)
    kh = k_full.reshape(bsz, -1, heads, 128).permute(0, 2, 1, 3)
    vh = v_full.reshape(bsz, -1, heads, 128).permute(0, 2, 1, 3)
    logits = q @ kh.transpose(-1, -2) / 128.0
    logits = logits + (~vis).float().unsqueeze(1) * O.NEG_MASK
    logits = logits + O.rel_pos_bias(qkvr[:, 3 * hid:].reshape(bsz, t, heads, 10), b_nd, t, maxlen)
    out = (torch.softmax(logits, -1) @ vh).permute(0, 2, 1, 3).reshape(bsz * t, hid)
    gq, gb = torch.autograd.grad((out * dout).sum(), [qkvr, b_nd])
    dev = lambda x: x.detach().to(DEV)
    case = dict(bsz=bsz, t=t, maxlen=maxlen, heads=heads, hid=hid, ld=ld, qkvr=dev(qkvr), kmem=dev(kmem), vmem=dev(vmem), b_nd=dev(b_nd), dout=dev(dout),
                mask8=dev(state_mask.to(torch.uint8)), qlo=dev(qlo), first=first, state_mask=state_mask, out=out.detach(), gq=gq, gb=gb)
    _ATT_CACHE[idx] = case
    return case


@pytest.mark.parametrize("idx", range(len(ATT_CASES)))
def test_attention_forward_with_episode_bounds(idx):
    c = _attention_case(idx)
    out = ops.masked_attention(c["qkvr"], c["kmem"], c["vmem"], c["mask8"], c["b_nd"], c["bsz"], c["t"], c["heads"], c["hid"], qlo=c["qlo"])
    torch.cuda.synchronize()
    err = (out.cpu().float() - c["out"]).abs().max().item()
    print(f"attention forward with qlo, case {ATT_CASES[idx][:3]}: max abs err {err:.3g}")
    assert err < 2e-2, f"attention abs err {err} (bf16 output of O(1) values)"
    # qlo = None and an all-zero qlo are today's kernel: bit-identical to the call with the equivalent memvalid
    first0 = torch.tensor([bool(c["first"][b, 0]) for b in range(c["bsz"])])
    memvalid = (c["state_mask"] & ~first0.view(-1, 1)).to(torch.uint8).to(DEV)
    base = ops.masked_attention(c["qkvr"], c["kmem"], c["vmem"], memvalid, c["b_nd"], c["bsz"], c["t"], c["heads"], c["hid"])
    zero = ops.masked_attention(c["qkvr"], c["kmem"], c["vmem"], memvalid, c["b_nd"], c["bsz"], c["t"], c["heads"], c["hid"], qlo=torch.zeros_like(c["qlo"]))
    assert torch.equal(base, zero)
    # ... and first at t = 0 alone, expressed through qlo with the plain state mask, is that same call again
    q0, _ = packing.episode_bounds(_first(c["bsz"], c["t"], {b: [0] for b in range(c["bsz"]) if first0[b]}), c["state_mask"], c["maxlen"])
    via_qlo = ops.masked_attention(c["qkvr"], c["kmem"], c["vmem"], c["mask8"], c["b_nd"], c["bsz"], c["t"], c["heads"], c["hid"], qlo=q0.to(DEV))
    assert torch.equal(base, via_qlo)


@pytest.mark.parametrize("idx", range(len(ATT_CASES)))
def test_attention_backward_with_episode_bounds(idx):
    c = _attention_case(idx)
    hid, ld = c["hid"], c["ld"]
    runs = []
    for _ in range(2):
        db = torch.zeros(10, c["maxlen"], device=DEV)
        dq = ops.masked_attention_backward(c["qkvr"], c["kmem"], c["vmem"], c["mask8"], c["b_nd"], c["dout"], db, c["bsz"], c["t"], c["heads"], hid, qlo=c["qlo"])
        runs.append((dq, db))
    torch.cuda.synchronize()
    dq, db = runs[0][0].cpu(), runs[0][1].cpu()
    for name, sl in [("dQ", slice(0, hid)), ("dK", slice(hid, 2 * hid)), ("dV", slice(2 * hid, 3 * hid)), ("dR", slice(3 * hid, ld))]:
        err = _l2(dq[:, sl], c["gq"][:, sl])
        print(f"attention backward with qlo, case {ATT_CASES[idx][:3]}: {name} rel L2 {err:.3g}")
        assert err < 1e-3, f"{name} rel L2 {err}"
    err = _l2(db, c["gb"])
    print(f"attention backward with qlo, case {ATT_CASES[idx][:3]}: db_nd rel L2 {err:.3g}")
    assert err < 1e-3, f"db_nd rel L2 {err}"
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_episode_entry_points_refuse_bad_arguments():
    """A qlo of the wrong size never reaches the kernel, and the *_episodes entry points need one (vpt_last_error says so)."""
    c = _attention_case(2)
    with pytest.raises((ValueError, TypeError)):
        ops.masked_attention(c["qkvr"], c["kmem"], c["vmem"], c["mask8"], c["b_nd"], c["bsz"], c["t"], c["heads"], c["hid"], qlo=c["qlo"][:, :-1].contiguous())
    with pytest.raises(RuntimeError, match="qlo"):
        vpt_amd._native.call("vpt_masked_attention_forward_episodes", ops.ptr(c["qkvr"]), ops.ptr(c["kmem"]), ops.ptr(c["vmem"]), ops.ptr(c["mask8"]),
                             ops.ptr(c["b_nd"]), ops.ptr(c["dout"]), None, c["bsz"], c["t"], c["heads"], c["hid"], c["ld"], c["maxlen"], None)


# ---------------------------------------------------------------------------------------------------------
# the policy
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["bf16", "fp16"])
def pol_1x(request):
    pk = O.policy_kwargs_for("1x")
    cfg = O.config_from_policy_kwargs(pk, dict(temperature=2.0))
    sd = O.synthetic_state_dict(cfg, seed=0)
    pol = MinecraftAgentPolicy(minecraft_action_space(), pk, dict(temperature=2.0), precision=request.param)
    pol.load_state_dict(sd, strict=False)
    pol = pol.to(DEV)
    yield pol, cfg, sd
    pol.set_episode_starts("chunk")


def _inputs(seed, b, t):
    return torch.randint(0, 256, (b, t, 128, 128, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _forward(pol, mode, img, first, state):
    pol.set_episode_starts(mode)
    try:
        with torch.no_grad():
            (pd, vpred, _), state_out = pol({"img": img.to(DEV)}, first.to(DEV), state)
        torch.cuda.synchronize()
    finally:
        pol.set_episode_starts("chunk")
    return pd["buttons"], pd["camera"], vpred, state_out


def _row(state, b):
    return [(m[b:b + 1], (k[b:b + 1].contiguous(), v[b:b + 1].contiguous())) for m, (k, v) in state]


def _state_to_dev(state):
    return [(None if m is None else m.to(DEV), (k.to(DEV), v.to(DEV))) for m, (k, v) in state]


def test_option_is_validated(pol_1x):
    pol, cfg, sd = pol_1x
    assert pol.episode_starts == "chunk"
    with pytest.raises(ValueError, match="episode_starts"):
        pol.set_episode_starts("episode")
    with pytest.raises(ValueError, match="episode_starts"):
        BCTrainer(pol, episode_starts="t0", optimizer_state=False)
    with pytest.raises(ValueError, match="episode_starts"):
        pol._ensure_packed()
        pol._engine.forward(_inputs(1, 1, 2).to(DEV), torch.zeros(1, 2, dtype=torch.bool, device=DEV), pol.initial_state(1), episode_starts="frames")
    assert pol.set_episode_starts("frame").episode_starts == "frame"
    pol.set_episode_starts("chunk")


def test_policy_frame_mode_equals_the_pieces_bit_for_bit(pol_1x):
    """Boundaries on multiples of the 32-query tile: a key's slot in a query tile depends on its offset to the query only, so one
    "frame"-mode call and the existing path run on the pieces add the same numbers in the same order -- torch.equal, no tolerance."""
    pol, cfg, sd = pol_1x
    b, t = 2, 96
    no_first = torch.zeros(b, 40, dtype=torch.bool)
    _, _, _, state = _forward(pol, "chunk", _inputs(21, b, 40), no_first, pol.initial_state(b))       # the state of a preceding 40-frame chunk
    img = _inputs(22, b, t)
    first = _first(b, t, {0: [32, 64]})
    lb, lc, v, st = _forward(pol, "frame", img, first, state)
    # row 0: three 32-frame calls, first[:, 0] on the second and third; row 1: one call.  The pieces run as calls of two rows as well (the
    # second row is company, its results are not looked at): the log-softmax of the heads picks its kernel by the number of rows of the call
    # (vpt_logsoftmax_launch: fewer than 64 rows of 8641 classes take the 16-wave kernel, which sums in another order), so a lone 32-frame row is
    # not bit-comparable with a row inside a larger call -- in either mode; that has nothing to do with episode starts
    s0, got0 = state, []
    for k in range(3):
        f = torch.zeros(b, 32, dtype=torch.bool)
        f[0, 0] = k > 0
        pb, pc, pv, s0 = _forward(pol, "chunk", img[:, 32 * k:32 * k + 32], f, s0)
        got0.append((pb, pc, pv))
    pb1, pc1, pv1, s1 = _forward(pol, "chunk", img, torch.zeros(b, t, dtype=torch.bool), state)
    for k, (pb, pc, pv) in enumerate(got0):
        sl = slice(32 * k, 32 * k + 32)
        for name, x, y in (("buttons", lb, pb), ("camera", lc, pc), ("vpred", v, pv)):
            assert torch.equal(x[0, sl], y[0]), f"row 0, piece {k}, {name}: max abs diff {float((x[0, sl] - y[0]).abs().max()):.3g}"
    for name, x, y in (("buttons", lb, pb1), ("camera", lc, pc1), ("vpred", v, pv1)):
        assert torch.equal(x[1], y[1]), f"row 1, {name}: max abs diff {float((x[1] - y[1]).abs().max()):.3g}"
    for l, (m, (kk, vv)) in enumerate(st):
        for row, piece in ((0, s0), (1, s1)):
            pm, (pk_, pv_) = piece[l]
            assert torch.equal(m[row], pm[row]) and torch.equal(kk[row], pk_[row]) and torch.equal(vv[row], pv_[row]), (l, row)
    assert st[0][0][0, 0].tolist() == [False] * 96 + [True] * 32          # row 0: only the frames since the last start are valid memory


_UNALIGNED = {}


def _unaligned_case(sd, cfg):
    """B = 2, T = 40, row 0 starts at {7, 33}, row 1 at {0, 39}, state from a preceding 5-frame chunk; expected values from the oracle run
    per row and per segment (first[:, 0] true on each later segment).  Computed once for both precisions."""
    if _UNALIGNED:
        return _UNALIGNED
    b, t = 2, 40
    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    pre = O.policy_forward(sd, cfg, _inputs(31, b, 5), torch.zeros(b, 5, dtype=torch.bool), O.initial_state(cfg, b))
    state = pre["state_out"]
    img = _inputs(32, b, t)
    first = _first(b, t, {0: [7, 33], 1: [0, 39]})
    outs = {k: [] for k in ("buttons", "camera", "vpred")}
    masks = []
    for row in range(b):
        cuts = sorted({0, t} | {p for p in range(t) if first[row, p]})
        st = [(m[row:row + 1], (k[row:row + 1], v[row:row + 1])) for m, (k, v) in state]
        parts = {k: [] for k in outs}
        for lo, hi in zip(cuts, cuts[1:]):
            f = torch.zeros(1, hi - lo, dtype=torch.bool)
            f[0, 0] = first[row, lo]
            r = O.policy_forward(sd, cfg, img[row:row + 1, lo:hi], f, st)
            st = r["state_out"]
            for k in parts:
                parts[k].append(r[k])
        for k in outs:
            outs[k].append(torch.cat(parts[k], 1))
        masks.append([m for m, _ in st])
    ref = {k: torch.cat(v, 0) for k, v in outs.items()}
    ref_masks = [torch.cat([masks[row][l] for row in range(b)], 0) for l in range(cfg["n_layers"])]
    _UNALIGNED.update(img=img, first=first, state=state, ref=ref, ref_masks=ref_masks)
    return _UNALIGNED


def test_policy_frame_mode_vs_the_oracle_per_segment(pol_1x):
    pol, cfg, sd = pol_1x
    c = _unaligned_case(sd, cfg)
    lb, lc, v, st = _forward(pol, "frame", c["img"], c["first"], _state_to_dev(c["state"]))
    m = P.policy_metrics(dict(buttons=lb, camera=lc, vpred=v), c["ref"])
    print(f"PARITY[{pol.precision}] frame mode vs the oracle per segment: {P.fmt(m)}")
    P.check(m, pol.precision, "episode_starts='frame', unaligned starts", model="1x")
    for l, (mk, _) in enumerate(st):
        assert mk.dtype == torch.bool and torch.equal(mk.cpu(), c["ref_masks"][l]), l


def test_frames_behind_an_episode_start_do_not_depend_on_what_came_before(pol_1x):
    pol, cfg, sd = pol_1x
    c = _unaligned_case(sd, cfg)
    state = _state_to_dev(c["state"])
    a = _forward(pol, "frame", c["img"], c["first"], state)
    img2 = c["img"].clone()
    img2[0, :33] = _inputs(33, 1, 33)[0]
    g = torch.Generator().manual_seed(34)
    state2 = []
    for mk, (k, v) in state:
        k2, v2, m2 = k.clone(), v.clone(), mk.clone()
        k2[0] = torch.randn(k[0].shape, generator=g).to(DEV)
        v2[0] = torch.randn(v[0].shape, generator=g).to(DEV)
        m2[0] = (torch.rand(m2[0].shape, generator=g) > 0.5).to(DEV)
        state2.append((m2, (k2, v2)))
    bb = _forward(pol, "frame", img2, c["first"], state2)
    for x, y in zip(a[:3], bb[:3]):
        assert torch.equal(x[0, 33:], y[0, 33:]) and torch.equal(x[1], y[1])
    assert not torch.equal(a[0][0, :33], bb[0][0, :33])
    # the default mode on the same inputs lets frame 33.. see the other episode: the very thing the option exists for
    ca = _forward(pol, "chunk", c["img"], c["first"], state)
    cb = _forward(pol, "chunk", img2, c["first"], state2)
    assert not torch.equal(ca[0][0, 33:], cb[0][0, 33:])


def test_default_mode_is_untouched(pol_1x):
    pol, cfg, sd = pol_1x
    b, t = 2, 12
    img = _inputs(41, b, t)
    _, _, _, state = _forward(pol, "chunk", _inputs(42, b, 5), torch.zeros(b, 5, dtype=torch.bool), pol.initial_state(b))
    first = _first(b, t, {1: [0]})
    fr, ch = _forward(pol, "frame", img, first, state), _forward(pol, "chunk", img, first, state)
    for x, y in zip(fr[:3], ch[:3]):
        assert torch.equal(x, y)
    for (m1, (k1, v1)), (m2, (k2, v2)) in zip(fr[3], ch[3]):
        assert torch.equal(m1, m2) and torch.equal(k1, k2) and torch.equal(v1, v2)
    g = torch.Generator().manual_seed(43)
    ab, ac = torch.randint(0, 8641, (b, t), generator=g).to(DEV), torch.randint(0, 121, (b, t), generator=g).to(DEV)
    res = {}
    for mode in ("chunk", "frame"):
        tr = BCTrainer(pol, train_cnn=True, optimizer_state=False, episode_starts=mode)
        res[mode] = tr.loss_and_grads(img.to(DEV), first.to(DEV), state, ab, ac)
    torch.cuda.synchronize()
    assert torch.equal(res["chunk"][0], res["frame"][0])
    assert set(res["chunk"][1]) == set(res["frame"][1]) and len(res["chunk"][1]) >= 120
    differing = [k for k in res["chunk"][1] if not torch.equal(res["chunk"][1][k], res["frame"][1][k])]
    assert not differing, differing[:8]
    # a mid-chunk first in the default mode is still ignored
    mid = first.clone()
    mid[0, 7] = True
    ig = _forward(pol, "chunk", img, mid, state)
    for x, y in zip(ig[:3], ch[:3]):
        assert torch.equal(x, y)
    for (m1, (k1, v1)), (m2, (k2, v2)) in zip(ig[3], ch[3]):
        assert torch.equal(m1, m2) and torch.equal(k1, k2) and torch.equal(v1, v2)
    assert not torch.equal(_forward(pol, "frame", img, mid, state)[0], ch[0])


_BC_ORACLE = {}


def test_bc_gradients_in_frame_mode_vs_the_oracle_per_segment(pol_1x):
    """B = 2, T = 6, row 0 starts at 3, row 1 at {0, 5}: the oracle's loss and gradients per row and per segment, weighted by
    (segment frames / 12), against BCTrainer(episode_starts="frame").loss_and_grads; the bounds of test_bc_gradients_vs_oracle."""
    pol, cfg, sd = pol_1x
    mode = pol.precision
    b, t = 2, 6
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (b, t, 128, 128, 3), generator=g, dtype=torch.uint8)
    ab = torch.randint(0, 8641, (b, t), generator=g)
    ac = torch.randint(0, 121, (b, t), generator=g)
    first = _first(b, t, {0: [3], 1: [0, 5]})
    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    if not _BC_ORACLE:
        state = O.policy_forward(sd, cfg, _inputs(51, b, 3), torch.zeros(b, 3, dtype=torch.bool), O.initial_state(cfg, b))["state_out"]
        loss_ref, grads_ref = 0.0, None
        for row in range(b):
            cuts = sorted({0, t} | {p for p in range(t) if first[row, p]})
            st = [(m[row:row + 1], (k[row:row + 1], v[row:row + 1])) for m, (k, v) in state]
            for lo, hi in zip(cuts, cuts[1:]):
                f = torch.zeros(1, hi - lo, dtype=torch.bool)
                f[0, 0] = first[row, lo]
                l_, g_, st = O.bc_loss_and_grads(sd, cfg, img[row:row + 1, lo:hi], f, st, ab[row:row + 1, lo:hi], ac[row:row + 1, lo:hi])
                wgt = (hi - lo) / float(b * t)
                loss_ref += wgt * l_
                grads_ref = {k: wgt * v for k, v in g_.items()} if grads_ref is None else {k: grads_ref[k] + wgt * g_[k] for k in grads_ref}
        _BC_ORACLE.update(state=state, loss=loss_ref, grads=grads_ref)
    loss_ref, grads_ref = _BC_ORACLE["loss"], _BC_ORACLE["grads"]
    tr = BCTrainer(pol, train_cnn=True, optimizer_state=False, episode_starts="frame")
    loss, grads, _ = tr.loss_and_grads(img.to(DEV), first.to(DEV), _state_to_dev(_BC_ORACLE["state"]), ab.to(DEV), ac.to(DEV))
    torch.cuda.synchronize()
    print(f"PARITY[{mode}] frame-mode BC loss {float(loss):.5f}, oracle per segment {loss_ref:.5f}")
    assert abs(float(loss) - loss_ref) < 2e-2, (float(loss), loss_ref)
    l2, cos = {}, {}
    for name in tr.trainable:
        ref = grads_ref[name]
        if float(ref.norm()) == 0.0:
            continue
        mine = grads[name].cpu().reshape(ref.shape)
        l2[name] = _l2(mine, ref)
        cos[name] = float((mine * ref).sum() / (mine.norm() * ref.norm()))
    mean_l2, mean_cos, min_cos = sum(l2.values()) / len(l2), sum(cos.values()) / len(cos), min(cos.values())
    print(f"PARITY[{mode}] frame-mode BC grads vs the fp32 oracle per segment over {len(l2)} tensors: mean rel-L2 {mean_l2:.3f}, "
          f"cosine mean {mean_cos:.4f}, worst {min_cos:.3f}")
    assert len(l2) >= 125
    GB = P.GRAD_BOUNDS[mode]
    assert mean_l2 < GB["l2_mean"] and mean_cos > GB["cos_mean"] and min_cos > GB["cos_min_small"], (mean_l2, mean_cos, min_cos)


# ---------------------------------------------------------------------------------------------------------
# 9. loader -> batcher -> trainer
# ---------------------------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(__file__), "golden")
H, W = 36, 64


def _video(name, n):
    base = sum(map(ord, name)) % 200
    return [np.full((H, W, 3), (base + 7 * i) % 256, np.uint8) + np.arange(3, dtype=np.uint8) for i in range(n)]


def test_trainer_from_the_batcher(pol_1x, tmp_path):
    pol, cfg, sd = pol_1x
    cursor = dict(np.load(os.path.join(GOLD, "clip_seed0.npz")))["cursor_bgra"]
    with gzip.open(os.path.join(GOLD, "clip_actions_seed0.json.gz"), "rt") as fh:
        recs = json.load(fh)
    videos = {}
    for k, (name, n) in enumerate({"a": 23, "b": 9, "c": 40, "d": 15, "e": 31}.items()):
        steps = recs[k % len(recs)]["steps"][:n]
        with open(tmp_path / f"{name}.jsonl", "w") as f:
            f.write("\n".join(json.dumps(s) for s in steps))
        (tmp_path / f"{name}.mp4").write_bytes(b"")
        videos[str(tmp_path / f"{name}.mp4")] = _video(name, n)
    random.seed(3)
    dl = clip_loader.DataLoader(str(tmp_path), n_workers=2, batch_size=2, n_epochs=2, device=DEV, decoder=lambda p: iter(videos[p]),
                                frame_processor=clip.ClipFrameProcessor(cursor, device=DEV), chunk_frames=16)
    sb = SequenceBatcher(dl, seq_len=8)
    tr = BCTrainer(pol, lr=1e-5, weight_decay=0.0, train_cnn=True, episode_starts="frame")
    state = pol.initial_state(2)
    losses, mid_chunk, expected, taken = [], False, {}, {}

    def oracle_indices(tid):
        """Joint action indices of every kept step of one recording, from the numpy oracle codec (agent.py's settings: maxval 10, binsize 2, mu-law mu 10)."""
        if tid not in expected:
            data = json.loads("[" + ",".join(open(dl.demonstration_tuples[tid][1]).readlines()) + "]")
            acts = clip.clip_steps(data, H).actions
            camera = np.stack([np.asarray(a["camera"], dtype=np.float64) for a in acts])
            buttons = np.array([[int(a.get(k, 0)) for k in A.BUTTONS_ALL] for a in acts], dtype=np.int64)
            expected[tid] = A.from_factored(buttons, A.discretize(camera, maxval=10, binsize=2, mu=10.0, mu_law=True))
        return expected[tid]

    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(3):
                c = next(sb)
                assert c["img"].is_cuda and c["img"].dtype == torch.uint8 and tuple(c["img"].shape) == (2, 8, 128, 128, 3)
                assert c["act_buttons"].is_cuda and c["act_buttons"].dtype == torch.int64 and tuple(c["act_camera"].shape) == (2, 8)
                mid_chunk |= bool(c["first"][:, 1:].any())
                # the default (device) encoder against the numpy oracle: a lane walks its recording in order, so the k-th item with a given
                # trajectory id is the recording's k-th kept step
                ids, gb, gc = c["episode_id"].cpu(), c["act_buttons"].cpu(), c["act_camera"].cpu()
                for row in range(2):
                    for k in range(8):
                        tid = int(ids[row, k])
                        n = taken.get(tid, 0)
                        taken[tid] = n + 1
                        wb, wc = oracle_indices(tid)
                        assert (int(gb[row, k]), int(gc[row, k])) == (int(wb[n]), int(wc[n])), (row, k, tid, n)
                loss, state = tr.step(c["img"], c["first"], state, c["act_buttons"], c["act_camera"])
                losses.append(loss)
        torch.cuda.synchronize()
    finally:
        pol.load_state_dict(sd, strict=False)
    print("BC losses over three chunks from the batcher:", [round(l, 3) for l in losses])
    assert len(losses) == 3 and all(np.isfinite(losses)) and pol.grad_overflows == 0 and tr.skipped_steps == 0
    assert mid_chunk                                  # a recording ended inside a chunk: the case the mode exists for
