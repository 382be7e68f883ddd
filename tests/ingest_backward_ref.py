"""References for the BACKWARD of the ingest side: vpt_conv_first_bwd_kernel<false / true> (first conv + ReLU + 3x3/2 max-pool, weights and bias; <true> with the
GroupNorm `n` backward folded in), vpt_affine_bwd_reduce / apply / elem_kernel (frame_affine) and vpt_pool_bwd_kernel (max-pool).  Plain torch, fp64,
importable without a GPU.  The forward half is tests/ingest_ref.py, whose instruments (ulp16, ratio / failure, sum_bound, frame_sums) are used here;
the max-pool routing is tests/cnn_backward_ref.py's maxpool_backward_ref.  u = 2^-24 (unit roundoff of fp32) throughout.  Derived, not tuned:

1. conv_first backward.  The forward never stores its pre-pool tensor, so the routing cannot be pinned to a stored tensor.  Instead the operands are chosen so
   that the pre-pool tensor is known EXACTLY on the CPU (exact_operands):
       weight = 255 k 2^-12, integer |k| <= 255        ->  W16 = op16(fl32(weight / 255)) = k 2^-12 exactly (8 significant bits; normal in fp16)
       bias   = j 2^-14 - 2, integer |j| <= 4096       ->  bh + bl = bias exactly (at most 17 bits, split 8 + 8 resp. 11 + 5), bl != 0 for most j
   A byte times k 2^-12 is a multiple of 2^-12; every partial sum of the 29 terms, in any order, is a multiple of 2^-14 whose magnitude is at most the sum of
   the magnitudes (asserted < 2^24 units on the reference): exact in fp32.  So pre = op16(relu(sum)) is ONE deterministic rounding, and the pooled tensor and
   the arg-max routing -- ties included -- are determined exactly.
       G[p][o]   = d[pp][o] routed to the FIRST maximum of window pp in scan order; a window whose maximum is <= 0 routes nothing
       dW[o][t]  = sum_p G[p][o] byte[p + (kh, kw)][ch] / 255,  t = (kh 3 + kw) 3 + ch;         db[o] = sum_p G[p][o]
   The kernel (vpt_conv_first_bwd.hip): every routed gradient enters an fp32 MFMA accumulation un-merged (d times a byte is exact: 8 or 11 bits times 8), at
   most n = frames * PH * PW non-zero terms per output element over all workgroups (additions of zero are exact); the two waves of a channel block are added
   (1); dW is multiplied by fl32(1 / 255) (the constant: 1, the product: 1); the workgroups' slab rows are added by vpt_slab_sum (at most `rows` additions in a
   term's chain, rows = min(tiles, 2 CUs) slab rows of the launch); the result is ADDED to the destination (one rounding of the stored value).
       dW:  (n + rows + 3) u dW_abs + u |dW|            db:  (n + rows + 2) u db_abs + u |db|            (_abs: the same sums over magnitudes)
   `out=` accumulation rounds the stored total once: the u |value| term is taken at the total, plus u |value| of the launch's own sum (its accumulate onto the
   slab total happened before).
   Exact cases.  Integer gradients with sum |d| < 2^24 (asserted): every partial sum of db is an integer below 2^24, db is BIT EXACT in any order.  A one-tile
   launch (one workgroup, one slab row, accumulate onto zero) with integer gradients: S = sum d byte is an exact integer in fp32 and dW = fl32(S fl32(1/255))
   bit for bit.
   NFOLD.  dpooled holds g = d loss / d n(P); the kernel first forms, per pooled element, dP = op16(r (g gain - A - xhat B)), xhat = (P - m) r, (m, r) from
   pool_stats as frame_mean_rstd defines them, (A, B) = pool_ab / count, P the (exact) pooled value.  fp32 operations, in units of u, as ingest_ref counts
   frame_affine:
       r:      fl32(var), + eps, halved by the power -1/2 -> 1;  rsqrtf <= 1 ulp = 2                                       ->  3
       xhat:   fl32(m) is 1 RELATIVE TO |m| -- not to |P - m| -- so it enters as the separate term r |m|; the subtraction 1, r 3, the product 1    ->  5 |xhat| + r |m|
       g gain:          the product 1, the two subtractions 2, the outer product 1, r 3                                    ->  7
       A:               fl32(A) 1, subtractions 2, outer product 1, r 3                                                    ->  7
       xhat B:          xhat 5, fl32(B) 1, the product 1, the subtraction 1, outer product 1, r 3                          -> 12
   so |dP - dP64| <= ulp16(dP64) + C_AFFINE_BWD u r (|g gain| + |A| + (|xhat| + r |m|) |B|) with C_AFFINE_BWD = 12 + 1 (one more for the second-order terms,
   as ingest_ref's 7 -> 8).  This bound, routed like the gradient, adds sum bound_dP byte / 255 to the dW bound and sum bound_dP to the db bound.

2. frame_affine backward (vpt_cnn_backward.hip).  y = (x - m) r g + b with whole-frame statistics:
       ab = (sum dy g, sum dy g xhat) per frame;   dx = r (dy g - A - xhat B) [+ dx_add], (A, B) = ab / n;   dgain = sum dy xhat, dbias = sum dy
   pass 1 (reduce): a thread adds 16 pixels x 8 channels = 128 terms (s2 by fma), six shuffle levels, the four waves in two: N_ADD_AB = 128 + 6 + 2; across
   workgroups fp64 atomics (2^-53: not counted).  Per term: dy g one product (1), xhat as above:
       ab0:  (N_ADD_AB + 1) u sum |dy g|            ab1:  u sum |dy g| (6 |xhat| + r |m|) + N_ADD_AB u sum |dy g xhat|
   dgain / dbias per channel: 16 terms per thread (fma), four levels of sum_oct16, the four waves in two, then the slab rows (frames * ceil(HW / 1024))
   through vpt_slab_sum's tree (slab_chain: a quarter of a 256-row slice front to back, two levels; with more than one slice the same over the slices), and
   the accumulate onto the destination (u |total|):
       n_add = 16 + 4 + 2 + slab_chain(rows);   dgain: u sum |dy| (5 |xhat| + r |m|) + n_add u sum |dy xhat| + u |total|;   dbias: n_add u sum |dy| + u |total|
   per element (pass 3): a thread adds the frames of its slice (ceil(frames / slices); slices = 1, 8 from 16 frames, 32 from 512), then the slices as slab rows:
       n_add = ceil(frames / slices) + slab_chain(slices)
   dx (apply): the expression of section 1 with (A, B) from the kernel's own ab, so the ab bounds propagate through A and B; dx_add is one more fp32 addition
   (1 more on every term, and u |dx_add|):
       ulp16(dx64) + (C_AFFINE_BWD + [dx_add]) u r (|dy g| + |A| + (|xhat| + r |m|) |B|) + r (b_ab0 + |xhat| b_ab1) / n + u |dx_add|
   Exact cases: integer dy with sum |dy| < 2^24 -> dbias bit exact; gains that are powers of two as well (sum |dy g| / min g < 2^24) -> ab[:, 0] bit exact.

3. max-pool backward.  pool_backward_fp32 is the kernel's exact arithmetic: a pre-pool pixel takes its <= 4 windows in (py, px) ascending order -- which is
   window offset 3 dy + dx DESCENDING -- adds their routed gradients in fp32 from 0 and rounds to 16 bits once.  Bit for bit.
"""
import functools
import math

import torch
import torch.nn.functional as F

from tests.cnn_backward_ref import frame_mean_rstd, maxpool_backward_ref
from tests.ingest_ref import D, DT, U32, conv_first_operands, frame_sums, sum_bound, ulp16

C_AFFINE_BWD = 13
N_ADD_AB = 128 + 6 + 2
EXACT_LIMIT = 2.0 ** 24


def _gen(name):
    return torch.Generator().manual_seed(sum(map(ord, name)))


def op16(v, fmt):
    """fp64 -> the 16-bit format -> fp64.  One rounding wherever v is representable in fp32 (every use here)."""
    return v.to(DT[fmt]).to(D)


def slab_chain(rows):
    """Longest chain of additions of vpt_slab_sum over `rows` slab rows (vpt_reduce.hip: slices of 256 rows, four segments front to back, (s0 + s1) + (s2 + s3))."""
    slices = -(-rows // 256)
    first = -(-min(rows, 256) // 4) + 2
    return first + ((-(-slices // 4) + 2) if slices > 1 else 0)


def affine_elem_slices(frames):
    return 32 if frames >= 512 else (8 if frames >= 16 else 1)


# ---- conv_first ------------------------------------------------------------------------------------------------------------------------------------------
def exact_operands(cout, g):
    """-> fp32 (weight [cout, 3, 3, 3], bias [cout], k, j) with weight = 255 k 2^-12 and bias = j 2^-14 - 2."""
    k = torch.randint(-255, 256, (cout, 3, 3, 3), generator=g)
    j = torch.randint(-4096, 4097, (cout,), generator=g)
    return (255.0 * k.double() * 2.0 ** -12).float(), (j.double() * 2.0 ** -14 - 2.0).float(), k, j


def conv_first_pre(img_u8, w16, bh, bl, fmt):
    """-> (pre = op16(relu(conv + bh + bl)) fp64 [F, Cout, H, W], the largest sum of magnitudes in units of 2^-14)."""
    x = img_u8.permute(0, 3, 1, 2).to(D)
    s = F.conv2d(x, w16.to(D), padding=1) + (bh.to(D) + bl.to(D)).view(1, -1, 1, 1)
    mag = F.conv2d(x, w16.to(D).abs(), padding=1) + (bh.to(D).abs() + bl.to(D).abs()).view(1, -1, 1, 1)
    return op16(torch.relu(s), fmt), float(mag.max()) * 2.0 ** 14


def windows(pre):
    """[f, c, h, w] -> [f, c, 9, PH * PW]: the 3x3/2 windows with -inf outside the image, offset 3 dy + dx on axis 2."""
    f, c = pre.shape[:2]
    return F.unfold(F.pad(pre, (1, 1, 1, 1), value=-math.inf), 3, stride=2).view(f, c, 9, -1)


def window_argmax(pre, last=False):
    """-> int64 [f, c, 1, PH * PW]: offset of the first (last) maximum of every window in scan order."""
    win = windows(pre)
    if last:
        return 8 - win.flip(2).argmax(dim=2, keepdim=True)
    return win.argmax(dim=2, keepdim=True)


def route_parts(d, pre, last=False):
    """-> [f, c, 9, PH * PW]: d placed at its window's winning offset, zero elsewhere."""
    f, c = pre.shape[:2]
    idx = window_argmax(pre, last)
    return torch.zeros(f, c, 9, idx.shape[-1], dtype=D).scatter_(2, idx, d.reshape(f, c, 1, -1))


def fold_parts(parts, h, w):
    f, c = parts.shape[:2]
    return F.fold(parts.reshape(f, c * 9, -1), (h + 2, w + 2), 3, stride=2)[:, :, 1:-1, 1:-1].contiguous()


def _route(d, pre, mutate):
    if mutate not in ("last_max", "drop_offset_8"):
        return maxpool_backward_ref(d, pre)
    parts = route_parts(d, pre, last=mutate == "last_max")
    if mutate == "drop_offset_8":
        parts[:, :, 8] = 0
    return fold_parts(parts, *pre.shape[2:])


def _wgrad(gr, img_u8):
    """gr [F, Cout, H, W] fp64 -> (dW [Cout, 27] in (kh, kw, ch) order, db [Cout])."""
    h, w = gr.shape[2:]
    xp = F.pad(img_u8.permute(0, 3, 1, 2).to(D), (1, 1, 1, 1))
    taps = [torch.einsum("fohw,fchw->oc", gr, xp[:, :, kh:kh + h, kw:kw + w]) for kh in range(3) for kw in range(3)]
    return torch.stack(taps, 1).reshape(gr.shape[1], 27) / 255.0, gr.sum((0, 2, 3))


def swap_row_pairs(d):
    """The gradient with the two pooled-row pairs of every half tile exchanged: rows (0, 1) <-> (2, 3), (4, 5) <-> (6, 7) of every eight."""
    ph = d.shape[2]
    perm = torch.arange(ph) ^ 2
    return d[:, :, perm]


def nfold_dp_ref(pooled, g, gain, pool_stats, pool_ab, fmt, swap_ab=False):
    """The GroupNorm `n` backward per pooled element -> (dP64, bound)."""
    f, c, ph, pw = pooled.shape
    n = c * ph * pw
    m, r = frame_mean_rstd(pool_stats, n)
    m, r = m.view(f, 1, 1, 1), r.view(f, 1, 1, 1)
    a, b = (pool_ab[:, i].to(D).view(f, 1, 1, 1) / n for i in ((1, 0) if swap_ab else (0, 1)))
    gg = g * gain.to(D).view(1, c, 1, 1)
    xhat = (pooled - m) * r
    dp = r * (gg - a - xhat * b)
    mag = r * (gg.abs() + a.abs() + (xhat.abs() + r * m.abs()) * b.abs())
    return dp, ulp16(dp, fmt) + C_AFFINE_BWD * U32 * mag


def conv_first_backward_ref(img, w16, bh, bl, dpooled, fmt, nfold=None, mutate=None):
    """img uint8 [F, H, W, 3], dpooled fp64 [F, Cout, H/2, W/2] (16-bit values), nfold = (gain fp32 [Cout], pool_stats fp64 [F, 2], pool_ab fp64 [F, 2]) ->
    dict(dW, db, dW_abs, db_abs [, dW_extra, db_extra, dP, b_dP]).  mutate: one of the defects of MUTATIONS (for the tests that show a bound sees them)."""
    pre, _ = conv_first_pre(img, w16, bh, bl, fmt)
    pooled = F.max_pool2d(pre, 3, 2, 1)
    live = (pooled > 0).to(D) if mutate != "zero_max_passes" else torch.ones_like(pooled)
    out = {}
    d = dpooled
    if nfold is not None:
        d, b_dp = nfold_dp_ref(pooled, dpooled, *nfold, fmt, swap_ab=mutate == "swap_ab")
        out["dP"], out["b_dP"] = d, b_dp
        out["dW_extra"], out["db_extra"] = _wgrad(_route(b_dp * live, pre, None), img)
    if mutate == "row_pairs":
        d = swap_row_pairs(d)
    out["dW"], out["db"] = _wgrad(_route(d * live, pre, mutate), img)
    out["dW_abs"], out["db_abs"] = _wgrad(_route(d.abs() * live, pre, mutate), img)
    return out


MUTATIONS = ("last_max", "zero_max_passes", "drop_offset_8", "row_pairs")


def conv_first_backward_bounds(ref, n, rows, prior=None):
    """-> (bound dW, bound db) of a launch that summed n pooled pixels per element over `rows` slab rows; prior = (dW0, db0) fp64: what `out=` held before."""
    b_dw = (n + rows + 3) * U32 * ref["dW_abs"] + U32 * ref["dW"].abs()
    b_db = (n + rows + 2) * U32 * ref["db_abs"] + U32 * ref["db"].abs()
    if "dW_extra" in ref:
        b_dw, b_db = b_dw + ref["dW_extra"], b_db + ref["db_extra"]
    if prior is not None:
        b_dw, b_db = b_dw + U32 * (prior[0] + ref["dW"]).abs(), b_db + U32 * (prior[1] + ref["db"]).abs()
    return b_dw, b_db


def dw_exact_one_tile(ref):
    """fl32(S * fl32(1 / 255)), S the exact integer sum: what a one-tile launch with integer gradients stores."""
    s = (ref["dW"] * 255.0).round()
    assert bool(((s / 255.0 - ref["dW"]).abs() <= 1e-9 * ref["dW"].abs() + 1e-12).all()) and bool((ref["dW_abs"] * 255.0 < EXACT_LIMIT).all())
    return s.float() * torch.tensor(1.0, dtype=torch.float32).div(255.0)


def routing_shares(pre):
    """-> (live share of all windows, tied-and-live share of all windows, [9] share of the live windows each offset wins)."""
    win = windows(pre)
    mx = win.max(dim=2, keepdim=True).values
    live = mx > 0
    tied = (win == mx).sum(2, keepdim=True) > 1
    idx = win.argmax(dim=2, keepdim=True)
    wins = torch.stack([((idx == k) & live).sum() for k in range(9)]).double() / live.sum().clamp(min=1)
    return live.double().mean().item(), (live & tied).double().mean().item(), wins


# ---- frame_affine ----------------------------------------------------------------------------------------------------------------------------------------
def affine_backward_ref(x, dy, gain, stats_in, fmt, per_element, dx_add=None, prior=None, mutate=None):
    """x, dy [, dx_add] fp64 [F, C, H, W] (16-bit values); gain fp32 [C] or, per element, [C * H * W] in C,H,W order; prior = (dgain0, dbias0) fp64, what the
    destinations held before (same order as gain) -> dict(ab, b_ab [F, 2]; dx, b_dx; dgain, b_dgain, dbias, b_dbias (totals, prior included);
    abs_dyg [F], abs_dy: the sums of magnitudes the exact cases are conditioned on).
    mutate: "no_add" (dx_add dropped), "gain_octet" (the gain of the neighbouring channel octet), "swap_ab"."""
    f, c, h, w = x.shape
    n, hw = c * h * w, h * w
    m, r = frame_mean_rstd(stats_in, n)
    m, r = m.view(f, 1, 1, 1), r.view(f, 1, 1, 1)
    shape = (1, c, h, w) if per_element else (1, c, 1, 1)
    g = gain.to(D).view(shape)
    if mutate == "gain_octet":
        g = torch.roll(g, 8, 1)
    xhat = (x - m) * r
    xh_err = 5 * xhat.abs() + r * m.abs()                 # error of the fp32 xhat in units of u
    dyg = dy * g
    s = lambda t: t.reshape(f, -1).sum(1)                 # noqa: E731
    ab = torch.stack([s(dyg), s(dyg * xhat)], 1)
    b_ab = torch.stack([sum_bound(N_ADD_AB + 1, s(dyg.abs())),
                        U32 * s(dyg.abs() * (xhat.abs() + xh_err)) + sum_bound(N_ADD_AB, s((dyg * xhat).abs()))], 1)
    a_, b_ = (ab[:, i].view(f, 1, 1, 1) / n for i in ((1, 0) if mutate == "swap_ab" else (0, 1)))
    dx = r * (dyg - a_ - xhat * b_)
    add = dx_add is not None and mutate != "no_add"
    mag = r * (dyg.abs() + a_.abs() + (xhat.abs() + r * m.abs()) * b_.abs())
    fp32 = (C_AFFINE_BWD + (1 if add else 0)) * U32 * mag + r * (b_ab[:, 0].view(f, 1, 1, 1) + xhat.abs() * b_ab[:, 1].view(f, 1, 1, 1)) / n
    if add:
        dx = dx + dx_add
        fp32 = fp32 + U32 * dx_add.abs()
    over = (0,) if per_element else (0, 2, 3)
    dgain, dbias = (dy * xhat).sum(over).reshape(-1), dy.sum(over).reshape(-1)
    abs_dg, abs_db = (dy * xhat).abs().sum(over).reshape(-1), dy.abs().sum(over).reshape(-1)
    if per_element:
        slices = affine_elem_slices(f)
        n_add = -(-f // slices) + slab_chain(slices)
    else:
        n_add = 16 + 4 + 2 + slab_chain(f * (-(-hw // 1024)))
    if prior is not None:
        dgain, dbias = dgain + prior[0].to(D), dbias + prior[1].to(D)
    b_dgain = U32 * (dy.abs() * xh_err).sum(over).reshape(-1) + sum_bound(n_add, abs_dg) + U32 * dgain.abs()
    b_dbias = sum_bound(n_add, abs_db) + U32 * dbias.abs()
    return dict(ab=ab, b_ab=b_ab, dx=dx, b_dx=ulp16(dx, fmt) + fp32, dgain=dgain, b_dgain=b_dgain, dbias=dbias, b_dbias=b_dbias,
                abs_dyg=s(dyg.abs()), abs_dy=abs_db, n_add=n_add)


# ---- max-pool --------------------------------------------------------------------------------------------------------------------------------------------
def pool_backward_fp32(pre, pooled, dpooled, fmt):
    """vpt_pool_bwd_kernel's arithmetic -> the 16-bit tensor [F, C, H, W].  `pooled` must be the window maxima of `pre` (asserted)."""
    assert torch.equal(pooled, F.max_pool2d(pre, 3, 2, 1))
    f, c, h, w = pre.shape
    parts = route_parts(dpooled, pre)
    acc = torch.zeros(f, c, h, w, dtype=torch.float32)
    for k in range(8, -1, -1):                                  # (py, px) ascending = offset descending
        only = torch.zeros_like(parts)
        only[:, :, k] = parts[:, :, k]
        acc = acc + fold_parts(only, h, w).float()              # at most one window per pixel and offset: the conversion is of a single 16-bit value
    return acc.to(DT[fmt])


# ---- the cases (shared by tests/test_ingest_backward_ref_cpu.py and tests/test_gpu_ingest_backward_fp64.py; computed once, never modified) -----------------
#                         name           frames h   w   cout
CONV_FIRST_BWD_CASES = {"one_tile": (1, 16, 16, 128),      # one tile, all borders, one slab row: the bit-exact dW case
                        "nt2_partial": (3, 48, 80, 160),   # non-square, ty == 0 || tx == 0 mixed, two channel tiles with the second partial
                        "one_wave": (2, 16, 48, 32)}       # three of four channel-block waves have no valid channel
PERSISTENT_BWD_HW_COUT = (48, 80, 32)                      # 15 tiles per frame; the number of frames follows from the device (persistent_backward_frames)
STYLES = (("blocky", "int"), ("blocky", "real"), ("random", "real"))       # (image, gradient)


def persistent_backward_frames(cus):
    """-> (frames, T, grid): the fewest 48 x 80 frames (15 tiles each) with T > grid = 2 workgroups per CU."""
    grid = 2 * cus
    frames = grid // 15 + 1
    return frames, 15 * frames, grid


def slab_rows(frames, h, w, cus):
    return min(frames * (h // 16) * (w // 16), 2 * cus)


@functools.lru_cache(maxsize=None)
def conv_first_bwd_case(frames, h, w, cout, fmt, image, grad):
    """Exact operands, a blocky (one byte triple per 4 x 4 block) or random image, integer gradients in [-3, 3] or 16-bit real ones (x 1e-2 in fp16), the
    GroupNorm `n` operands of the NFOLD variant computed from the exact pooled tensor -> dict with the plain and the NFOLD reference."""
    g = _gen(f"{frames}x{h}x{w}x{cout}{image}{grad}")
    weight, bias, k, j = exact_operands(cout, g)
    w16, bh, bl = conv_first_operands(weight, bias, fmt)
    if image == "blocky":
        img = torch.randint(0, 256, (frames, h // 4, w // 4, 3), generator=g, dtype=torch.uint8).repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()
    else:
        img = torch.randint(0, 256, (frames, h, w, 3), generator=g, dtype=torch.uint8)
    ph, pw = h // 2, w // 2
    if grad == "int":
        d = torch.randint(-3, 4, (frames, cout, ph, pw), generator=g).to(D)
    else:
        d = op16(torch.randn(frames, cout, ph, pw, generator=g).to(D) * (1e-2 if fmt == "fp16" else 1.0), fmt)
    gain = 1 + 0.3 * torch.randn(cout, generator=g)
    pre, units = conv_first_pre(img, w16, bh, bl, fmt)
    pooled = F.max_pool2d(pre, 3, 2, 1)
    pool_stats, _ = frame_sums(pooled)
    m, r = frame_mean_rstd(pool_stats, cout * ph * pw)
    gg = d * gain.to(D).view(1, cout, 1, 1)
    xhat = (pooled - m.view(-1, 1, 1, 1)) * r.view(-1, 1, 1, 1)
    pool_ab = torch.stack([gg.reshape(frames, -1).sum(1), (gg * xhat).reshape(frames, -1).sum(1)], 1)
    nfold = (gain, pool_stats, pool_ab)
    return dict(frames=frames, h=h, w=w, cout=cout, weight=weight, bias=bias, k=k, j=j, w16=w16, bh=bh, bl=bl, img=img, d=d, pre=pre, pooled=pooled,
                units=units, nfold=nfold, n=frames * ph * pw,
                plain=conv_first_backward_ref(img, w16, bh, bl, d, fmt), folded=conv_first_backward_ref(img, w16, bh, bl, d, fmt, nfold=nfold))


#                     name          F    C   H   W   per_element
AFFINE_BWD_CASES = {"few_pixels": (2, 32, 4, 4, False),        # 16 pixels: most lanes never enter the loop
                    "clamped": (3, 96, 6, 10, False),          # 60 pixels: clamped duplicates and the `live` guard
                    "two_chunks": (2, 64, 40, 40, False),      # two pixel chunks, the second partial
                    "two_slices": (300, 32, 4, 4, False),      # 300 slab rows: two vpt_slab_sum slices, the second partial
                    "elem_small": (2, 64, 4, 4, True),
                    "elem_partial": (1, 160, 6, 10, True),
                    "elem_slices": (17, 32, 2, 4, True)}       # eight frame slices of three frames: the last two are empty


@functools.lru_cache(maxsize=None)
def affine_bwd_case(name, fmt, kind):
    """kind "real": real gradient and gain; "exact": integer dy in [-3, 3] and gains in {1/2, 1, 2}; "constant": frame 0 holds one value (variance 0)."""
    frames, c, h, w, per_element = AFFINE_BWD_CASES[name]
    g = _gen(name + kind)
    x = op16(torch.relu(torch.randn(frames, c, h, w, generator=g)).to(D), fmt)
    if kind == "constant":
        x[0] = 1.5
    n = c * h * w if per_element else c
    scale = 1e-2 if fmt == "fp16" else 1.0
    if kind == "exact":
        dy = torch.randint(-3, 4, (frames, c, h, w), generator=g).to(D)
        gain = torch.pow(2.0, torch.randint(-1, 2, (n,), generator=g).float())
    else:
        dy = op16(torch.randn(frames, c, h, w, generator=g).to(D) * scale, fmt)
        gain = 1 + 0.2 * torch.randn(n, generator=g)
    dx_add = op16(torch.randn(frames, c, h, w, generator=g).to(D) * scale, fmt)
    prior = (torch.randn(n, generator=g) * scale, torch.randn(n, generator=g) * scale)
    stats_in, _ = frame_sums(x)
    return dict(frames=frames, c=c, h=h, w=w, per_element=per_element, x=x, dy=dy, gain=gain, dx_add=dx_add, prior=prior, stats_in=stats_in,
                plain=affine_backward_ref(x, dy, gain, stats_in, fmt, per_element),
                added=affine_backward_ref(x, dy, gain, stats_in, fmt, per_element, dx_add=dx_add, prior=prior))


#              F  C   H   W
POOL_CASES = [(2, 32, 16, 16), (1, 96, 6, 10), (3, 32, 2, 2), (1, 64, 48, 16)]
POOL_LEVELS = (0.0, 0.125, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0)      # eight numbers both formats hold


@functools.lru_cache(maxsize=None)
def pool_case(i, fmt):
    """Post-ReLU values from eight levels (plateaus), whole 2 x 2 blocks zeroed with probability 0.4 (all-zero windows)."""
    f, c, h, w = POOL_CASES[i]
    g = _gen(f"pool{i}")
    pre = torch.tensor(POOL_LEVELS, dtype=D)[torch.randint(0, 8, (f, c, h, w), generator=g)]
    keep = (torch.rand(f, c, h // 2, w // 2, generator=g) > 0.4).to(D).repeat_interleave(2, 2).repeat_interleave(2, 3)
    pre = pre * keep
    pooled = F.max_pool2d(pre, 3, 2, 1)
    d = op16(torch.randn(f, c, h // 2, w // 2, generator=g).to(D) * (1e-2 if fmt == "fp16" else 1.0), fmt)
    return dict(f=f, c=c, h=h, w=w, pre=pre, pooled=pooled, d=d, dpre=pool_backward_fp32(pre, pooled, d, fmt), argmax=window_argmax(pre).view(f, c, h // 2, w // 2))
