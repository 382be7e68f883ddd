"""fp64 reference of vpt_grouped_lp_bwd_kernel (ops.grouped_logprob_backward), the error bound the kernel is held to, a float32 restatement of
the kernel's order of operations, three WRONG references for the tests' self-check, and the seeded inputs both test files use.  A plain helper (no
test, no fixture): torch / numpy on the CPU only, nothing of vpt_amd.

The heads are gb independent nb-way button groups and gc independent nc-way camera groups per frame (lib/action_head.py:136-184).  Per group, with
the forward's log-probs l_j (float32), the incoming gradients g_j = d loss / d log-prob (float32) and n classes:
    s    = ((g_0 + g_1) + ...) + g_{n-1}
    p_j  = exp(l_j)
    dz_j = ((g_j - p_j s) * inv_t) * grad_scale,        inv_t = the float32 quotient 1 / T (exact for the T in {1, 2} of the tests)
a masked element (its logit was the constant LOG0 in the forward) is 0 -- its g still counts in s --, a head without an incoming gradient is a block
of zeros, the columns behind the two blocks (buttons first, [group][class]) are zeros.  tests/test_grouped_logprob_ref_cpu.py proves on the CPU that
this is torch's fp64 gradient through log_softmax(where(mask, z, LOG0) / T); tests/test_gpu_grouped_logprob_backward.py holds the kernel to it.

Bound.  u = 2^-24; the kernel works in float32 without contraction, so every operation rounds once.  With G = sum_k |g_k| of the group,
d = g_j - p_j s and c = inv_t * grad_scale:
  s        (n - 1) additions, left to right:           |s^ - s| <= gamma G,  gamma = (n - 1) u / (1 - (n - 1) u)
  p        expf:                                        |p^ - p| <= E u p,  E = 2 x 1.345: twice the largest error of the device's expf this project
                                                        has measured (DESIGN.md section 14, 1.345 u); the 16-bit output cannot resolve expf itself
  p^ s^    the product:  exact value p s, error         e_ps = p gamma G + (E + 1) u p (|s| + gamma G)            (expf's E u |p s| and one rounding)
  d^       the subtraction rounds once:                 e_d  = e_ps + u (|d| + e_ps)
  scalings two multiplications, one rounding each:      e_x  = |c| e_d + 2 u (1 + u) (|x| + |c| e_d),   x = c d
  dz       one rounding to the operand format:          bound = ulp16(|x| + e_x) / 2 + e_x
(For powers of two T and grad_scale the scalings are exact and the bound is slightly generous.)  An element the definition makes exactly 0 --
masked, padding, a head without gradient -- has bound 0: it must BE 0.  A one-class group has p = 1, s = g_0 and d = 0 exactly in every
arithmetic, so its bound is that of x = 0: 0 as well."""
import numpy as np
import torch

from tests.cnn_backward_ref import U, ulp16

LOG0 = -100.0                     # lib/action_head.py:13
E_EXP = 2 * 1.345                 # see above
MUTATIONS = ("no_temp", "head_sum", "camera_shift")
# (M, gb, nb, gc, nc): one-class groups; the released heads (62 columns, 2 of padding); odd widths in a partly filled workgroup; 69 columns
# (ldz = 128: a lane owns two columns)
SHAPES = {"one": (1, 1, 1, 1, 1), "released": (3, 20, 2, 2, 11), "odd": (5, 3, 7, 2, 5), "wide": (2, 6, 11, 1, 3)}


def round_up(n, k=64):
    return (n + k - 1) // k * k


def make_case(m, gb, nb, gc, nc, temperature=2.0, seed=0, masks=True):
    """Seeded inputs: logits zb fp64 [m, gb, nb] / zc [m, gc, nc] of order 2, availability masks (about a quarter of the classes of a group with more
    than one class masked, never all of them; masks=False: none), the log-probs lb / lc = log_softmax(where(mask, z, LOG0) / T) rounded to float32 as
    the forward hands them over, and incoming gradients gb_in / gc_in float32 of order 1/2 (a tenth of them exact zeros, as a loss that ignores a
    class delivers)."""
    g = torch.Generator().manual_seed(seed + 1000 * m + 10 * nb + nc)
    out = dict(m=m, gb=gb, nb=nb, gc=gc, nc=nc, temperature=float(temperature))
    for h, (grp, n) in (("b", (gb, nb)), ("c", (gc, nc))):
        z = torch.randn(m, grp, n, generator=g, dtype=torch.float64) * 2
        avail = torch.ones(m, grp, n, dtype=torch.bool)
        if masks and n > 1:
            avail = torch.rand(m, grp, n, generator=g) > 0.25
            keep = torch.randint(0, n, (m, grp, 1), generator=g)
            avail.scatter_(-1, keep, True)
        lp = torch.log_softmax(torch.where(avail, z, torch.full_like(z, LOG0)) / temperature, -1).float()
        gin = (torch.randn(m, grp, n, generator=g) * 0.5).float()
        gin = torch.where(torch.rand(m, grp, n, generator=g) < 0.1, torch.zeros_like(gin), gin)
        out["z" + h], out["mask_" + h], out["l" + h], out["g" + h + "_in"] = z, (avail if masks else None), lp, gin
    return out


def reference(c, grad_scale=1.0, use_buttons=True, use_camera=True, mutate=None):
    """fp64 -> dict(dz [M, ldz], bound_abs [M, ldz]: the float32 part e_x of the bound), ldz = round_up(gb nb + gc nc, 64).  The log-probs and
    gradients are taken as given (float32 inputs are exact in fp64; fp64 inputs give the exact closed form for the autograd check).
    use_*: False = that head's incoming gradient is absent.  mutate (a WRONG reference): "no_temp" = 1 / T left out, "head_sum" = s taken over the
    whole head instead of per group, "camera_shift" = the camera block one column to the right."""
    m, gb, nb, gc, nc = c["m"], c["gb"], c["nb"], c["gc"], c["nc"]
    inv_t = 1.0 if mutate == "no_temp" else float(np.float32(1.0) / np.float32(c["temperature"]))
    cs = abs(inv_t * float(grad_scale))
    cols = gb * nb + gc * nc
    ldz = round_up(cols)
    dz, bnd = torch.zeros(m, ldz, dtype=torch.float64), torch.zeros(m, ldz, dtype=torch.float64)
    off = 0
    for h, n, grp, use in (("b", nb, gb, use_buttons), ("c", nc, gc, use_camera)):
        if use:
            l, g = c["l" + h].double(), c["g" + h + "_in"].double()
            p = torch.exp(l)
            if mutate == "head_sum":
                s = g.sum((-1, -2), keepdim=True).expand_as(g)
            else:
                s = g.sum(-1, keepdim=True).expand_as(g)
            G = g.abs().sum(-1, keepdim=True).expand_as(g)
            d = g - p * s
            x = d * inv_t * float(grad_scale)
            gam = (n - 1) * U / (1 - (n - 1) * U)
            e_ps = p * gam * G + (E_EXP + 1) * U * p * (s.abs() + gam * G)
            e_d = e_ps + U * (d.abs() + e_ps)
            e_x = cs * e_d + 2 * U * (1 + U) * (x.abs() + cs * e_d)
            if n == 1:                      # p = 1, s = g_0: d = 0 exactly, in every arithmetic
                x, e_x = torch.zeros_like(x), torch.zeros_like(x)
            mk = c["mask_" + h]
            if mk is not None:
                x, e_x = torch.where(mk, x, torch.zeros_like(x)), torch.where(mk, e_x, torch.zeros_like(x))
            dz[:, off:off + grp * n], bnd[:, off:off + grp * n] = x.reshape(m, grp * n), e_x.reshape(m, grp * n)
        off += grp * n
    if mutate == "camera_shift":
        nbt = gb * nb
        dz[:, nbt:] = torch.roll(dz[:, nbt:], 1, dims=1)
        bnd[:, nbt:] = torch.roll(bnd[:, nbt:], 1, dims=1)
    return dict(dz=dz, bound_abs=bnd, cols=cols, ldz=ldz)


def mutant_differs(mut, c):
    """Whether a mutated reference can be another reference at all on this shape: without a second class there is no gradient under any rule, at T = 1
    there is no 1 / T to leave out, with one group the head's sum is the group's, and a camera block of zeros moves nowhere."""
    many = c["nb"] > 1 or c["nc"] > 1
    if mut == "no_temp":
        return many and c["temperature"] != 1.0
    if mut == "head_sum":
        return c["gb"] > 1 or c["gc"] > 1
    if mut == "camera_shift":
        return c["nc"] > 1
    raise KeyError(mut)


def dz_bound(ref, fmt):
    """The full bound of a 16-bit dz; fmt None: the float32 part alone (for the restatement before its rounding)."""
    b = ref["bound_abs"]
    return b if fmt is None else 0.5 * ulp16(ref["dz"].abs() + b, fmt) * (b + ref["dz"].abs() > 0) + b


def ratio(dz, ref, fmt):
    """max err / bound over all [M, ldz] elements (an element with bound 0 must be exact: its ratio is 0 or inf)."""
    e = (dz.double().cpu() - ref["dz"]).abs()
    b = dz_bound(ref, fmt)
    q = torch.where(b > 0, e / b.clamp(min=1e-300), torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))))
    return float(q.max())


def restate_f32(c, grad_scale=1.0, use_buttons=True, use_camera=True):
    """float32 numpy in the kernel's order (numpy's own float32 exp) -> dz float32 [M, ldz] BEFORE the 16-bit rounding."""
    f = np.float32
    m, gb, nb, gc, nc = c["m"], c["gb"], c["nb"], c["gc"], c["nc"]
    inv_t, gs = f(1.0) / f(c["temperature"]), f(grad_scale)
    dz = np.zeros((m, round_up(gb * nb + gc * nc)), f)
    off = 0
    for h, n, grp, use in (("b", nb, gb, use_buttons), ("c", nc, gc, use_camera)):
        if use:
            l, g = c["l" + h].numpy().astype(f), c["g" + h + "_in"].numpy().astype(f)
            s = g[..., 0].copy()
            for k in range(1, n):
                s = (s + g[..., k]).astype(f)
            p = np.exp(l).astype(f)
            d = (g - (p * s[..., None]).astype(f)).astype(f)
            x = ((d * inv_t).astype(f) * gs).astype(f)
            if c["mask_" + h] is not None:
                x = np.where(c["mask_" + h].numpy(), x, f(0)).astype(f)
            dz[:, off:off + grp * n] = x.reshape(m, grp * n)
        off += grp * n
    return torch.from_numpy(dz)
