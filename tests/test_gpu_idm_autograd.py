"""The autograd boundary of the inverse-dynamics model (lib/policy.py:_IDMForwardFn): a gradient-enabled InverseActionPolicy.forward joins the
autograd graph, and `loss.backward()` runs the hand-written HIP backward of IDMTrainer behind ops.grouped_logprob_backward.  Tiny IDM
(tests/labeler_ref.tiny_idm), temperature 2, both operand formats.  Needs an MI355X.

(a) the grad-enabled forward with the CNN frozen returns the no_grad forward's bits, attached to the graph;
(b) the mean NLL through the boundary gives IDMTrainer.loss_and_grads' gradients bit for bit (B x T = 16 frames: 1 / M and 1 / T are powers of two,
    so dz is the loss kernel's dz -- tests/test_gpu_grouped_logprob_backward.py -- and every reduction behind it has a fixed order), with the CNN
    frozen and with the whole network trained;
(c) a loss the trainer cannot express -- label-smoothed NLL with a coefficient per head minus an entropy bonus -- against fp64 autograd of
    tests/idm_trainer_ref.forward from the GPU's own dense output, with the assertions and constants of
    tests/test_gpu_idm_training.py::test_gradients_vs_the_fp64_reference;
(d) a loss that uses the camera head only: the button head's weight and bias gradients are EXACT ZEROS, not None (its block of dz is zero and
    backward_from runs the heads' GEMM over the whole [62, hid] matrix);
(e) obs["mask"] under autograd: an always-masked class has a bias (and weight-row) gradient of exactly 0, the other tensors meet (c)'s assertions
    against the reference run with the same mask;
(f) the reference-style loop: CNN frozen with requires_grad_(False), torch.optim.Adam, six steps on one batch;
(g) the fp16 failure paths, and the second backward."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vpt_amd  # noqa: E402,F401
from vpt_amd.idm_training import IDMTrainer  # noqa: E402
from vpt_amd.lib.policy import InverseActionPolicy  # noqa: E402
from vpt_amd.lib.types import idm_action_space  # noqa: E402
from tests import idm_trainer_ref as IR  # noqa: E402
from tests import labeler_ref as R  # noqa: E402
from tests import parity as P  # noqa: E402

DEV = "cuda"
CNN = ("net.conv3d_layer.", "net.img_process.cnn.")
LOG0 = -100.0


def _l2(a, ref):
    return float((a - ref).norm() / ref.norm().clamp(min=1e-30))


def _policy(precision):
    kw, cfg, sd = R.tiny_idm()
    pol = InverseActionPolicy(idm_action_space(), pi_head_kwargs=dict(temperature=R.TEMPERATURE), idm_net_kwargs=kw, precision=precision)
    missing, unexpected = pol.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    return pol.to(DEV), cfg, sd


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def idm(request):
    return _policy(request.param)


def _batch(b, t, seed=21):
    g = torch.Generator().manual_seed(seed)
    return P.structured_frames(b, t, g), torch.randint(0, 2, (b, t, 20), generator=g), torch.randint(0, 11, (b, t, 2), generator=g)


@pytest.fixture(scope="module")
def batch16():
    return _batch(2, 8)


@pytest.fixture(scope="module")
def batch24():
    return _batch(2, 12)


def _reset(pol, sd, train_cnn=False):
    """The fixture's policy as a test wants it: the synthetic weights, no gradients, the CNN frozen (or not), the default lift."""
    pol.load_state_dict(sd, strict=False)
    for n, p in pol.named_parameters():
        p.requires_grad_(train_cnn or not n.startswith(CNN))
        p.grad = None
    for eng in pol._grad_engines.values():
        eng.autograd_lift = 256.0


def _forward(pol, img, mask=None):
    obs = {"img": img} if mask is None else {"img": img, "mask": mask}
    (pd, v, _), state = pol(obs, None, pol.initial_state(img.shape[0]))
    assert v is None
    return pd


def _mean_nll(pol, pd, buttons, camera):
    return -pol.pi_head.logprob({"buttons": buttons, "camera": camera}, pd).mean()


def custom_loss(lp_b, lp_c, buttons, camera, eps=0.1, coef_b=1.0, coef_c=0.5, ent_coef=0.01):
    """Label-smoothed NLL with a coefficient per head, minus ent_coef x entropy, averaged over the frames.  lp_* [..., G, n], labels [..., G]."""
    def smoothed(lp, lab):
        pick = lp.gather(-1, lab.unsqueeze(-1)).squeeze(-1)
        return -((1.0 - eps) * pick + eps * lp.mean(-1)).sum(-1)
    ent = -(lp_b.exp() * lp_b).sum((-1, -2)) - (lp_c.exp() * lp_c).sum((-1, -2))
    return (coef_b * smoothed(lp_b, buttons) + coef_c * smoothed(lp_c, camera) - ent_coef * ent).mean()


def _reference_grads(sd, cfg, d, b, t, loss_fn, rnd=None, colmask=None):
    """fp64 autograd of loss_fn(lp_b [M, 20, 2], lp_c [M, 2, 11]) through tests/idm_trainer_ref.forward from the dense output d.  colmask
    ({"buttons": bool [40], "camera": bool [22]}, the same for every frame): a masked column's weight row is replaced by the constant 0 and its bias
    by the constant T x LOG0, which makes its scaled logit LOG0 at every frame -- obs["mask"] with a frame-independent mask -- and cuts it off
    from its parameters as the forward's overwrite does."""
    names = IR.trainable_names(sd, cfg)
    leaves = {k: (v.detach().double().clone().requires_grad_(True) if k in names else v.detach().double()) for k, v in sd.items()
              if v.dtype.is_floating_point}
    with torch.enable_grad():
        eff = dict(leaves)
        for h in ("buttons", "camera") if colmask is not None else ():
            keep = colmask[h]
            w_, b_ = leaves[f"pi_head.{h}.linear_layer.weight"], leaves[f"pi_head.{h}.linear_layer.bias"]
            eff[f"pi_head.{h}.linear_layer.weight"] = torch.where(keep[:, None], w_, torch.zeros_like(w_))
            eff[f"pi_head.{h}.linear_layer.bias"] = torch.where(keep, b_, torch.full_like(b_, cfg["temperature"] * LOG0))
        lp_b, lp_c = IR.forward(eff, cfg, d.detach().double(), b, t, rnd=rnd)
        loss = loss_fn(lp_b, lp_c)
        grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    return float(loss.detach()), {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, grads)}


def _assert_like_the_trainer(mode, what, trainable, loss, grads, ref, em):
    """tests/test_gpu_idm_training.py::test_gradients_vs_the_fp64_reference's assertions, constants included."""
    (loss_ref, grads_ref), (loss_em, grads_em) = ref, em
    print(f"PARITY[{mode}] {what} loss: GPU {float(loss):.5f}, fp64 reference {loss_ref:.5f}, {mode}-rounding reference {loss_em:.5f}")
    assert abs(float(loss) - loss_ref) < 2e-2 and abs(float(loss) - loss_em) < 1e-2, (float(loss), loss_ref, loss_em)
    assert set(grads) == set(trainable) == set(grads_ref)
    worst, cos_ref = {}, {}
    for name in trainable:
        r, e = grads_ref[name], grads_em[name]
        mine = grads[name].cpu().double().reshape(r.shape)
        if float(r.norm()) == 0.0:          # r_layer: unreached under mask "none"
            assert float(mine.abs().max()) == 0.0, name
            continue
        d_gpu, d_em = _l2(mine, r), _l2(e, r)
        worst[name] = (d_gpu, d_em)
        cos_ref[name] = float((mine * r).sum() / (mine.norm() * r.norm()))
        assert d_gpu < 1.5 * d_em + 0.1, (name, d_gpu, d_em)
        cos_em = float((e * r).sum() / (e.norm() * r.norm()))
        assert cos_ref[name] > min(0.93, cos_em - 0.15), (name, cos_ref[name], cos_em)
        ratio = float(mine.norm() / r.norm())
        assert 0.75 < ratio < 1.3, (name, ratio)
    assert len(worst) >= 35
    mean_gpu = sum(v[0] for v in worst.values()) / len(worst)
    mean_em = sum(v[1] for v in worst.values()) / len(worst)
    mean_cos = sum(cos_ref.values()) / len(cos_ref)
    print(f"PARITY[{mode}] {what} grads: mean rel-L2 to the fp64 reference over {len(worst)} tensors: GPU {mean_gpu:.4f}, {mode} rounding reference "
          f"{mean_em:.4f}; cosine: mean {mean_cos:.5f}, worst {min(cos_ref.values()):.4f}; largest", sorted(worst.items(), key=lambda kv: -kv[1][0])[:2])
    assert mean_gpu < 1.15 * mean_em + 0.02, (mean_gpu, mean_em)
    GB = P.GRAD_BOUNDS[mode]
    assert mean_gpu < GB["l2_mean"] and mean_cos > GB["cos_mean"] and min(cos_ref.values()) > GB["cos_min_small"], (mean_gpu, mean_cos, min(cos_ref.values()))


def _param_grads(pol):
    return {n: p.grad for n, p in pol.named_parameters() if p.grad is not None}


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------
def test_grad_enabled_forward_joins_the_graph_with_the_inference_bits(idm, batch16):
    pol, _, sd = idm
    _reset(pol, sd)
    img = batch16[0].to(DEV)
    with torch.no_grad():
        ref = _forward(pol, img)
    pd = _forward(pol, img)
    torch.cuda.synchronize()
    for h in ("buttons", "camera"):
        assert ref[h].grad_fn is None and not ref[h].requires_grad
        assert pd[h].grad_fn is not None and pd[h].requires_grad, h
        assert torch.equal(pd[h].detach(), ref[h]), h
    assert tuple(pd["buttons"].shape) == (2, 8, 20, 2) and tuple(pd["camera"].shape) == (2, 8, 2, 11)
    for p in pol.parameters():              # every parameter frozen: the inference engine again
        p.requires_grad_(False)
    assert _forward(pol, img)["buttons"].grad_fn is None


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train_cnn", [False, True])
def test_mean_nll_gives_the_trainers_gradients_bit_for_bit(idm, batch16, train_cnn):
    pol, _, sd = idm
    _reset(pol, sd, train_cnn=train_cnn)
    img, buttons, camera = (x.to(DEV) for x in batch16)
    tr = IDMTrainer(pol, optimizer_state=False, train_cnn=train_cnn)
    loss_tr, want = tr.loss_and_grads(img, buttons, camera)
    pd = _forward(pol, img)
    loss = _mean_nll(pol, pd, buttons, camera)
    loss.backward()
    torch.cuda.synchronize()
    got = _param_grads(pol)
    assert train_cnn in pol._grad_engines                   # the CNN is trained exactly when one of its parameters requires grad
    assert set(got) == set(want) == set(tr.trainable), set(got) ^ set(want)
    assert abs(float(loss.detach()) - float(loss_tr)) < 1e-3         # (the same log-probs summed in another association)
    differ = {n: _l2(got[n].reshape(want[n].shape).double(), want[n].double()) for n in want if not torch.equal(got[n].reshape(want[n].shape), want[n])}
    print(f"boundary vs IDMTrainer.loss_and_grads [{pol.precision}, train_cnn={train_cnn}]: {len(want)} tensors, {len(differ)} differ {differ}")
    assert not differ
    for n, p in pol.named_parameters():
        assert n not in got or got[n].shape == p.shape, n
        if n.startswith("net.lastlayer.") or n.endswith("b_nd") or (n.startswith(CNN) and not train_cnn):
            assert p.grad is None, n
        if ".r_layer." in n:
            assert float(p.grad.abs().max()) == 0.0, n
    assert pol.grad_overflows == 0


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------
def test_custom_loss_vs_the_fp64_reference(idm, batch24):
    pol, cfg, sd = idm
    _reset(pol, sd)
    mode = pol.precision
    img, buttons, camera = (x.to(DEV) for x in batch24)
    b, t = img.shape[:2]
    pd = _forward(pol, img)
    loss = custom_loss(pd["buttons"], pd["camera"], buttons, camera)
    loss.backward()
    torch.cuda.synchronize()
    eng = pol._grad_engines[False]
    d = eng.forward_saving(img)["d"].cpu()
    torch.set_num_threads(max(1, min(32, len(__import__("os").sched_getaffinity(0)))))
    fn = lambda lb, lc: custom_loss(lb, lc, batch24[1].reshape(b * t, 20), batch24[2].reshape(b * t, 2))
    ref, em = _reference_grads(sd, cfg, d, b, t, fn), _reference_grads(sd, cfg, d, b, t, fn, rnd=mode)
    _assert_like_the_trainer(mode, "IDM boundary, custom loss", eng.trainable, loss.detach(), _param_grads(pol), ref, em)
    assert pol.grad_overflows == 0


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------------
def test_a_loss_on_one_head_leaves_exact_zeros_in_the_other(idm, batch16):
    pol, _, sd = idm
    _reset(pol, sd)
    img, _, camera = (x.to(DEV) for x in batch16)
    pd = _forward(pol, img)
    loss = -pol.pi_head["camera"].logprob(camera, pd["camera"]).mean()
    loss.backward()
    torch.cuda.synchronize()
    gb_w, gb_b = pol.pi_head["buttons"].linear_layer.weight.grad, pol.pi_head["buttons"].linear_layer.bias.grad
    assert gb_w is not None and gb_b is not None                                  # exact zeros, not None
    assert float(gb_w.abs().max()) == 0.0 and float(gb_b.abs().max()) == 0.0
    gc_w = pol.pi_head["camera"].linear_layer.weight.grad
    assert float(gc_w.abs().max()) > 0.0 and bool(torch.isfinite(gc_w).all())
    assert float(pol.net.final_ln.weight.grad.abs().max()) > 0.0


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------------
def test_mask_under_autograd(idm, batch24):
    pol, cfg, sd = idm
    _reset(pol, sd)
    mode = pol.precision
    img = batch24[0].to(DEV)
    b, t = img.shape[:2]
    keep_b, keep_c = torch.ones(20, 2, dtype=torch.bool), torch.ones(2, 11, dtype=torch.bool)
    keep_b[3, 1] = keep_b[17, 0] = False
    keep_c[1, 0] = keep_c[1, 10] = keep_c[0, 5] = False
    buttons = torch.where(keep_b.gather(1, batch24[1].reshape(-1, 20).t()).t().reshape(b, t, 20), batch24[1], 1 - batch24[1])      # labels on available classes
    camera = batch24[2].clone()
    camera[..., 1] = camera[..., 1].clamp(1, 9)
    camera[..., 0] = torch.where(camera[..., 0] == 5, torch.full_like(camera[..., 0], 4), camera[..., 0])
    mask = {"buttons": keep_b.expand(b, t, 20, 2).contiguous().to(DEV), "camera": keep_c.expand(b, t, 2, 11).contiguous().to(DEV)}
    pd = _forward(pol, img, mask)
    with torch.no_grad():
        plain = _forward(pol, img, mask)
    assert torch.equal(pd["buttons"].detach(), plain["buttons"]) and torch.equal(pd["camera"].detach(), plain["camera"])
    assert float(pd["buttons"].detach()[..., 3, 1].max()) < -90.0 and float(pd["camera"].detach()[..., 1, 10].max()) < -90.0
    loss = custom_loss(pd["buttons"], pd["camera"], buttons.to(DEV), camera.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    gb_b, gc_b = pol.pi_head["buttons"].linear_layer.bias.grad.view(20, 2), pol.pi_head["camera"].linear_layer.bias.grad.view(2, 11)
    gb_w, gc_w = pol.pi_head["buttons"].linear_layer.weight.grad.view(20, 2, -1), pol.pi_head["camera"].linear_layer.weight.grad.view(2, 11, -1)
    assert float(gb_b[~keep_b.to(DEV)].abs().max()) == 0.0 and float(gc_b[~keep_c.to(DEV)].abs().max()) == 0.0
    assert float(gb_w[~keep_b.to(DEV)].abs().max()) == 0.0 and float(gc_w[~keep_c.to(DEV)].abs().max()) == 0.0
    assert float(gb_b[3, 0].abs()) > 0.0 and float(gc_b[1, 1].abs()) > 0.0
    eng = pol._grad_engines[False]
    d = eng.forward_saving(img)["d"].cpu()
    torch.set_num_threads(max(1, min(32, len(__import__("os").sched_getaffinity(0)))))
    fn = lambda lb, lc: custom_loss(lb, lc, buttons.reshape(b * t, 20), camera.reshape(b * t, 2))
    cm = {"buttons": keep_b.reshape(-1), "camera": keep_c.reshape(-1)}
    ref, em = _reference_grads(sd, cfg, d, b, t, fn, colmask=cm), _reference_grads(sd, cfg, d, b, t, fn, rnd=mode, colmask=cm)
    _assert_like_the_trainer(mode, "IDM boundary, masked", eng.trainable, loss.detach(), _param_grads(pol), ref, em)


# ---- (f) ------------------------------------------------------------------------------------------------------------------------------------
def test_reference_style_loop(idm, batch16):
    """Freeze the CNN, torch.optim.Adam(lr = 1e-4), six steps on one batch.  Every tensor that received a non-zero gradient moved; `r_layer.*`
    receives the exact zeros IDMTrainer produces (mask "none" does not reach it) and, without weight decay, Adam leaves it where it is."""
    pol, _, sd = idm
    _reset(pol, sd)
    img, buttons, camera = (x.to(DEV) for x in batch16)
    try:
        for n, p in pol.named_parameters():
            if n.startswith(CNN):
                p.requires_grad_(False)
        opt = torch.optim.Adam([p for p in pol.parameters() if p.requires_grad], lr=1e-4)
        before = {n: p.detach().clone() for n, p in pol.named_parameters()}
        _, _, out0 = pol.predict({"img": img})
        losses, got_grad = [], set()
        for _ in range(6):
            opt.zero_grad(set_to_none=True)
            (pd, _, _), _ = pol({"img": img}, None, pol.initial_state(2))
            loss = custom_loss(pd["buttons"], pd["camera"], buttons, camera)
            loss.backward()
            got_grad |= {n for n, p in pol.named_parameters() if p.grad is not None and float(p.grad.abs().max()) > 0.0}
            zero_grad = {n for n, p in pol.named_parameters() if p.grad is not None and float(p.grad.abs().max()) == 0.0}
            opt.step()
            losses.append(float(loss.detach()))
        _, _, out1 = pol.predict({"img": img})
        torch.cuda.synchronize()
        after = {n: p.detach().clone() for n, p in pol.named_parameters()}
    finally:
        _reset(pol, sd)
    print(f"IDM boundary + torch Adam on a fixed batch [{pol.precision}]:", [round(l, 4) for l in losses])
    assert losses[-1] < losses[0] and pol.grad_overflows == 0
    assert len(got_grad) >= 35 and all(".r_layer." in n for n in zero_grad) and len(zero_grad) == 2 * pol._cfg["n_layers"]
    for n in before:
        if n in got_grad:
            assert not torch.equal(before[n], after[n]), n
        else:
            assert torch.equal(before[n], after[n]), n
    assert not torch.equal(out0["pd"]["buttons"], out1["pd"]["buttons"]) and not torch.equal(out0["pd"]["camera"], out1["pd"]["camera"])


# ---- (g) ------------------------------------------------------------------------------------------------------------------------------------
def test_fp16_failure_paths_and_the_second_backward(batch16):
    pol, _, sd = _policy("fp16")
    _reset(pol, sd)
    img, buttons, camera = (x.to(DEV) for x in batch16)

    def backward_once(factor=1.0, **kw):
        pol.zero_grad(set_to_none=True)
        pd = _forward(pol, img)
        loss = _mean_nll(pol, pd, buttons, camera) * factor
        loss.backward(**kw)
        return loss

    backward_once()                                          # creates the gradient engine
    eng = pol._grad_engines[False]
    assert eng.autograd_overflows == 0 and eng.autograd_lift == 256.0 and len(_param_grads(pol)) >= 35
    with pytest.warns(RuntimeWarning, match="non-finite"):
        backward_once(float("inf"))
    assert eng.autograd_overflows == 1 and eng.autograd_lift == 256.0 and not _param_grads(pol)
    eng.autograd_lift = 2.0 ** 40
    with pytest.warns(RuntimeWarning, match="overflowed"):
        backward_once()
    assert eng.autograd_overflows == 2 and eng.autograd_lift == 2.0 ** 39 and not _param_grads(pol) and pol.grad_overflows == 2
    eng.autograd_lift = 256.0
    loss = backward_once(retain_graph=True)
    grads = _param_grads(pol)
    assert len(grads) >= 35 and all(bool(torch.isfinite(g_).all()) for g_ in grads.values())
    with pytest.raises(RuntimeError, match="already consumed"):
        loss.backward()
    # the same rule in bf16 (no lift there)
    pol.set_precision("bf16")
    assert pol._grad_engines == {}
    loss = backward_once(retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed"):
        loss.backward()
    torch.cuda.synchronize()
