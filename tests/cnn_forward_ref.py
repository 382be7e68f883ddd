"""References for the parts of the CNN forward that had none: vpt_conv3x3_small_kernel (the latency tiling of conv3x3), the frame statistics (stats_out) of every
conv3x3 forward mode, vpt_pool_kernel<ARGMAX>, vpt_channel_stats_kernel and vpt_nfold_coef_kernel (the GroupNorm-`n` fold).  Plain torch, fp64, importable
without a GPU.  ulp16, ratio / failure, frame_sums, sum_bound and unrounded_stats_bound are those of tests/ingest_ref.py, and so is the treatment of
frame_mean_rstd (u = 2^-24; rsqrtf is taken as <= 1 ulp = 2 u).  Every count below was made from the source line named beside it.

1. conv3x3, LATENCY TILING (vpt_conv3x3_small.hip).  The reference of tests/test_gpu_conv_mfma16.py on the same 16-bit operands, W' = op16(W * gain) and x as
   stored, (mean, rstd) = frame_mean_rstd64(stats_in): mean = fl32(s / n), rstd = 1 / sqrt(fl32(var) + eps) in fp64,
       y64 = relu(rstd * conv(W', x) + SA[e][o] - rstd * mean * SG[e][o]) (+ res),      bound = ulp16(y64) + (K + C_LATENCY) u P,   P = rstd * conv(|W'|, |x|), K = 9 Cin.
   The count of C_LATENCY, in units of u relative to the term named:
       acc        K products of two 16-bit operands (exact in fp32), K - 1 additions in the MFMA chain (channel block, kernel row, kernel column,
                  16-channel half: S_ITER / S_LOADG)                                                                                  K - 1   of P
       rstd       fl32(var) + 1e-5f rounds once, halved by the power -1/2; rsqrtf 2 (frame_mean_rstd, vpt_common.h)                    3       of P and of rstd |mean SG|
       kk         `kk[idx] = a.edge_sa[o] - rstd * mean * a.edge_sg[o]`: the product rstd * mean 1, the product with SG 1, the subtraction 1
                  (as an fma: one less)                                                          2 + 3 (rstd) + 1 = 6 of rstd |mean SG|,  1 of |SA|
       fma        `fmaxf(fmaf(rstd, acc, k4[j]), 0.f)`: one rounding of the sum                                                        1       of P + |SA| + rstd |mean SG|
       residual   `v[0] += ...`: one rounding                                                                                          1       of P + |SA| + rstd |mean SG| + |res|
   so  |v - y64| <= (K + 4) u P + 8 u (|SA| + rstd |mean SG| + |res|).  The bound has P alone, which the cases make legitimate: every case is generated so that
       |SA| + rstd |mean SG| + |res| <= P   at EVERY element (latency_case asserts it; the table terms are sums of W b and W' over the taps, P is the same
   sum of |W'| |x| with |x| several times |b|), and then the error is at most (K + 4) u P + 8 u P:                                   C_LATENCY = 12.
   (tests/test_gpu_conv_mfma16.py keeps its own `+ 8` for the throughput kernel; this is a count for this kernel's epilogue, not a copy.)

2. STATISTICS (stats_out).  Two references, because the two tilings sum different things -- a property of the code today:
   * the THROUGHPUT kernel (vpt_conv3x3_fwd.hip) sums the STORED 16-bit values (`s_sum2.x = dot2_op16(pk[h].x, OP16_ONE2, s_sum2.x)`), in the pool-fused modes
     4 / 7 the unscaled pooled values (`p_sum = dot2_op16(mv[k], OP16_ONE2, p_sum)` before out_gain is applied): the reference is the fp64 sum of the tensor the
     kernel itself returned (with out_gain: of the same call without the gain), the allowed error sum_bound(n_add, sum |y|) and sum_bound(n_add, sum y^2) --
     squares of 16-bit values are exact in fp32, their accumulation is not.  n_add = the longest fp32 chain before the fp64 atomic:
       modes 0, 1, 5, 16-row tiles and their halo-DMA instantiations (one epilogue, epilogue16): per lane and packed half (s_sum2.x / .y) 8 rows j x 2 blocks n2
           x 2 halves h = 32 dot2 of two values each, counted as two additions = 64; `s_sum2.x + s_sum2.y` 1; wave_sum 6; `(red[0] + red[1]) + (red[2] +
           red[3])` 2                                                                                                        N_ADD_FWD16 = 64 + 1 + 6 + 2 = 73
       32-row tiles (NWAVE == 8): `t1 += (red[4] + red[5]) + (red[6] + red[7])` one level more                               N_ADD_FWD32 = 74
       modes 4 / 7, in-tile pixels: 4 items x 4 dot2 x 2 values = 32, wave_sum 6, four waves 2                               N_ADD_POOL_TILE = 40
       modes 4 / 7, seam pixels (vpt_pool_seam_kernel, one workgroup per frame and channel block): a thread walks ceil(n_pix / 64) pixels of 8 values
           (`s_sum += vals[k]`), four shuffle levels (`off = 4; off < 64`), `(red[0] + red[1]) + (red[2] + red[3])` 2, the four octets `t += ...` 4
                                                                                                            n_add_pool_seam(h, w) = 8 ceil(n_pix / 64) + 10
           a frame's total is the fp64 sum of both kinds of partial sums, each within n u times ITS share of the magnitude: n_add = the larger of the two.
     The fp64 atomics add at most (partials) * 2^-53 relative, which the first (exact) addition 0 + v of every counted chain pays for ((n - 1) u would do).
   * the LATENCY kernel sums the UNROUNDED fp32 v (`s_sum += v[j]; s_sq = fmaf(v[j], v[j], s_sq)`): unrounded_stats_bound(y64, acc, n_add) with acc = (K + C_LATENCY)
     u P, and 16 values per lane, wave_sum 6, `((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + ...` 3                    N_ADD_LATENCY_STATS = 16 + 6 + 3 = 25

3. MAX POOL (vpt_pool_kernel, vpt_elementwise.hip).  The pooled value is exact: F.max_pool2d(x.float(), 3, 2, 1), compared on bits.  Arg-max = the FIRST maximum in
   scan order as torch's indices give it, mapped to k = 3 (iy - 2 py + 1) + (ix - 2 px + 1), and 15 for a window whose maximum is 0.  Statistics of the stored
   values: 4 items x 8 values per thread (`s_sum += vals[k]`), block_stats_atomic = wave_sum 6 + 2                            N_ADD_POOL_STATS = 32 + 6 + 2 = 40
   Inputs are post-ReLU values from a handful of levels with zeroed patches: ties, all-zero windows and maxima in row 0 / column 0 of the window are frequent
   (pool_shares; asserted in tests/test_cnn_forward_ref_cpu.py).  Negative inputs are outside the kernel's stated precondition.

4. CHANNEL_STATS (vpt_channel_stats_kernel).  Reference: per-channel fp64 (sum q, sum q^2) of the stored tensor.  A workgroup takes one split of per = ceil(HW /
   split) <= 1024 pixels, split = ceil(HW / 1024); a lane's serial run is every 64th pixel of it (`p += 256`, four loads 64 apart) = ceil(per / 64) <= 16 values per
   channel, then `off = 4; off < 64` 4 levels and `(red[0] + red[1]) + (red[2] + red[3])` 2; fp64 across splits.   n_add_channel_stats(hw) = ceil(per / 64) + 6 <= 22

5. NFOLD_COEF (vpt_nfold_coef_kernel).  The formulas of the comment above vpt_channel_stats_kernel in fp64 on the same tot, chs, gain, bias, sa, sg, tb, tg:
       mu_P = tot0 / n, r_P = (max(tot1 / n - mu_P^2, 0) + eps)^-1/2, kappa = r_P mu_P, b[c] = bias[c] - kappa gain[c],
       sum x = sum_c (r_P S1 + HW b), sum x^2 = sum_c (r_P^2 S2 + 2 r_P b S1 + HW b^2)  ->  mu_x, sigma_x^2, r_x = (sigma_x^2 + eps)^-1/2
       res_scale = r_P, res_bias = b, rs_frame = r_x r_P, kk_frame = sa + r_x tb - r_x kappa tg - r_x mu_x sg.
   The kernel evaluates the sums in fp64 from ITS r_P' = rsqrtf((float)var_P + 1e-5f) and m' = (float)mu_P.  Term by term, in u:
       r_P'    fl32(var_P) 1/2, the fp32 constant 1e-5f 1/2, the addition 1/2 (each halved by the power -1/2), rsqrtf 2                      E_RP = 3.5
       kappa'  = r_P' m':  E_RP + 1 (the rounding of mu_P)                                                                                   E_KAPPA = 4.5
       res_scale = (float)r_P' is exact: E_RP of r_P.      res_bias = (float)(bias - kappa' gain): E_KAPPA of |kappa gain| + 1 of |bias| + |kappa gain|.
       x' = bias + (r_P' / r_P) (z + r_P (mu_P - m') gain) with z = r_P (Q - mu_P gain) is what the kernel's sums are the exact moments of, so per element
           |x' - x| <= E_RP u |z| + r_P' |mu_P - m'| |gain|   ->   |mu_x' - mu_x| <= d_mu = E_RP u mean|z| + r_P' |mu_P - m'| mean|gain|  (mean|z| <= rms z, from chs, tot)
                                                          |sigma_x' - sigma_x| <= d_sigma = E_RP u rms z + r_P' |mu_P - m'| rms gain   (triangle inequality of the centred norm)
           with |mu_P - m'| <= u |mu_P| taken as what it IS for the given tot (a property of the input: 0 on the constant frame, whose mean 1.5 is an fp32 number)
           (relative errors of mu_x and sigma_x are NOT small numbers of u: r_P S1 and kappa gain HW cancel.  The absolute errors above are what is derived.)
       r_x'    (sigma_x + d_sigma) d_sigma / (sigma_x^2 + eps) from the variance, + 3.5 as r_P', + the fp64 evaluation of both sides: N_FP64 = 64 roundings of
               2^-53 relative to the all-magnitudes form of sum x^2 / n (per channel 12, the loop, shuffles and tree 10, mean and variance 3; twice: the kernel
               and this reference), halved by the power                                                                                       E_RX (per frame)
       rs_frame = fl32(r_x' r_P'):  E_RX + E_RP + 1.
       kk_frame = ((sa + c_b tb) + c_g tg) + c_s sg in fp32, c_b = r_x', c_g = -r_x' (float)kappa', c_s = -r_x' (float)mu_x': three multiply-adds, each one rounding
               relative to a partial sum that M = |sa| + |r_x tb| + |r_x kappa tg| + |r_x mu_x sg| bounds, + 1 on each product where the compiler does not fuse:
               |sa| 3;   |r_x tb| E_RX + 1 + 3;   |r_x kappa tg| E_RX + E_KAPPA + 1 ((float)) + 1 (c_g) + 1 + 3;
               |r_x mu_x sg| E_RX + 1 ((float)) + 1 (c_s) + 1 + 3, and r_x |sg| d_mu (with the fp64 evaluation's share) for the absolute error of mu_x.
   Second-order terms (u^2) are below the halves rounded up in these counts.  No tolerance here was chosen by trying values.
"""
import functools

import torch
import torch.nn.functional as F

from oracle.vpt_oracle import NORM_EPS
from tests.ingest_ref import D, DT, U32, failure, frame_sums, ratio, sum_bound, ulp16, unrounded_stats_bound  # noqa: F401  (one import site for the tests)
from vpt_amd import packing

FMTS = ["bf16", "fp16"]
U64 = 2.0 ** -53

C_LATENCY = 12
N_ADD_LATENCY_STATS = 16 + 6 + 3
N_ADD_FWD16 = 64 + 1 + 6 + 2
N_ADD_FWD32 = 64 + 1 + 6 + 3
N_ADD_POOL_TILE = 32 + 6 + 2
N_ADD_POOL_STATS = 32 + 6 + 2
E_RP, E_KAPPA, N_FP64 = 3.5, 4.5, 64


def n_add_pool_seam(h, w):
    """vpt_pool_seam_kernel: n_pix seam pixels per (frame, channel block), 64 pixel slots -> the chain length (0 with a single tile: no launch)."""
    ty, tx, ph, pw = h // 16, w // 16, h // 2, w // 2
    n_pix = (ty - 1) * pw + (tx - 1) * (ph - (ty - 1))
    return 8 * -(-n_pix // 64) + 4 + 2 + 4 if n_pix else 0


def n_add_pool_fused(h, w):
    return max(N_ADD_POOL_TILE, n_add_pool_seam(h, w))


def channel_stats_split(hw):
    """-> (split, pixels per split) of vpt_channel_stats_launch."""
    split = (hw + 1023) // 1024
    return split, (hw + split - 1) // split


def n_add_channel_stats(hw):
    return -(-channel_stats_split(hw)[1] // 64) + 4 + 2


def _gen(name):
    return torch.Generator().manual_seed(sum(map(ord, name)))


def edge_class(h, w):
    ey = torch.ones(h, dtype=torch.long); ey[0] = 0; ey[-1] = 2
    ex = torch.ones(w, dtype=torch.long); ex[0] = 0; ex[-1] = 2
    return ey.view(h, 1) * 3 + ex.view(1, w)          # [h, w]


def frame_mean_rstd64(stats_in, n):
    """(mean, rstd) [F, 1, 1, 1] in fp64 exactly as frame_mean_rstd forms them, but for its last step: mean = fl32(m), rstd = 1 / sqrt(fl32(var) + eps)."""
    m = stats_in[:, 0].to(D) / n
    var = (stats_in[:, 1].to(D) / n - m * m).clamp(min=0)
    mean = m.float().to(D)
    rstd = 1.0 / torch.sqrt(var.float().to(D) + NORM_EPS)
    return mean.view(-1, 1, 1, 1), rstd.view(-1, 1, 1, 1)


def stats_failure(got, want, allowed, what):
    """fp64 sums [.., 2] from a kernel against reference sums -> (worst err / allowed, None or a message)."""
    got = got.to(D).cpu()
    err = (got - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / allowed)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    worst = r.max().item()
    if bool((r <= 1.0).all()):
        return worst, None
    idx = tuple((~(r <= 1.0)).nonzero()[0].tolist())
    return worst, f"{what}: worst err / allowed {worst:.3f}; first at {idx}: got {got[idx].item()!r}, fp64 {want[idx].item()!r}, allowed {allowed[idx].item():.3e}"


def stored_stats_ref(y, n_add):
    """The throughput kernel's statistics: y [F, ...] = the STORED tensor the kernel returned -> (fp64 sums [F, 2], allowed error [F, 2])."""
    sums, mags = frame_sums(y)
    return sums, sum_bound(n_add, mags)


# ---- conv3x3, latency tiling ---------------------------------------------------------------------------------------------------------------------------
#                  name          frames h   w   cin  cout
LATENCY_CASES = {"one_block": (1, 16, 16, 32, 32),        # one channel block: no second stage issued, one workgroup, all nine edge classes
                 "two_blocks": (2, 32, 16, 64, 96),       # two blocks, more_ never true; a row seam; two frames; three output blocks
                 "three_blocks": (1, 16, 48, 96, 160),    # more_ true once, the last loop pass runs a single S_ITER; column seams; the second 128-channel tile, CoutPad 256
                 "ring_wraps": (1, 16, 16, 128, 32),      # four blocks: the stage ring wraps
                 "five_blocks": (1, 48, 48, 160, 64),     # five blocks; one interior tile
                 "k3456": (1, 16, 16, 384, 32)}           # twelve blocks: the 3x model's deepest K


@functools.lru_cache(maxsize=None)
def latency_case(name, fmt):
    """Operands (CPU) and the fp64 pieces of a latency case, computed once and never modified.  y64 / bound / acc are indexed by use_res."""
    frames, h, w, cin, cout = LATENCY_CASES[name]
    dt = DT[fmt]
    g = _gen(name)
    W = torch.randn(cout, cin, 3, 3, generator=g) * (1.6 / (cin * 9) ** 0.5)
    gain = 1 + 0.2 * torch.randn(cin, generator=g)
    bias = 0.1 * torch.randn(cin, generator=g)
    x = (torch.relu(torch.randn(frames, cin, h, w, generator=g)) + 0.2 * torch.randn(frames, cin, h, w, generator=g)).to(dt)
    res = torch.randn(frames, cout, h, w, generator=g).to(dt)
    wpk, sa, sg = packing.pack_conv3x3(W, gain, bias, dtype=dt)
    w16 = (W * gain.view(1, -1, 1, 1)).to(dt)                      # W' = op16(W * gain): what the packed image holds
    x64 = x.to(D)
    stats_in, _ = frame_sums(x)
    mean, rstd = frame_mean_rstd64(stats_in, cin * h * w)
    conv = F.conv2d(x64, w16.to(D), padding=1)
    p_abs = rstd * F.conv2d(x64.abs(), w16.to(D).abs(), padding=1)
    e = edge_class(h, w)
    sa_e = sa.to(D)[:, :cout][e].permute(2, 0, 1).unsqueeze(0)      # [1, cout, h, w]
    sg_e = sg.to(D)[:, :cout][e].permute(2, 0, 1).unsqueeze(0)
    pre = torch.relu(rstd * conv + sa_e - rstd * mean * sg_e)
    acc = (9 * cin + C_LATENCY) * U32 * p_abs
    y64 = {False: pre, True: pre + res.to(D)}
    bound = {r: ulp16(y64[r], fmt) + acc for r in (False, True)}
    dominated = ((sa_e.abs() + rstd * (mean * sg_e).abs() + res.to(D).abs()) / p_abs).max().item()      # the premise of C_LATENCY (docstring, 1.)
    assert dominated <= 1.0, (name, fmt, dominated)
    return dict(frames=frames, h=h, w=w, cin=cin, cout=cout, dt=dt, x=x, res=res, w16=w16, wpk=wpk, sa=sa, sg=sg, stats_in=stats_in, mean=mean, rstd=rstd,
                e=e, sa_e=sa_e, sg_e=sg_e, y64=y64, bound=bound, acc=acc, dominated=dominated)


def latency_stats_ref(c, use_res):
    """-> (fp64 sums [F, 2] of y64, allowed error [F, 2]) for the latency kernel's statistics of the UNROUNDED values."""
    sums, _ = frame_sums(c["y64"][use_res])
    return sums, unrounded_stats_bound(c["y64"][use_res], c["acc"], N_ADD_LATENCY_STATS)


# ---- max pool ------------------------------------------------------------------------------------------------------------------------------------------
#              name         F  C   H   W
POOL_CASES = {"one_window": (1, 32, 2, 2),       # one window per octet; every load clamped
              "partial": (3, 32, 6, 10),         # 60 items: a partial block; odd pooled sizes; three frames
              "first_item": (2, 32, 16, 16),     # 256 items: only the first of the thread's four items is live
              "crosses_cb": (2, 96, 16, 24),     # 1152 items: the second block is partial and crosses a channel-block edge
              "two_blocks": (1, 64, 32, 32)}     # the shape of tests/test_gpu_kernels.py: two full blocks
POOL_LEVELS = (0.0, 0.25, 0.5, 1.0, 1.5, 3.0)    # exact in both formats


def pool_windows(x):
    """x [F, C, H, W] >= 0 -> [F, C, 9, PH, PW]: window position k = 3 (dy + 1) + (dx + 1) of every pooled pixel, -1 outside the image."""
    h, w = x.shape[2:]
    p = F.pad(x, (1, 1, 1, 1), value=-1.0)
    return torch.stack([p[..., k // 3:k // 3 + h:2, k % 3:k % 3 + w:2] for k in range(9)], 2)


def pool_ref(x):
    """x [F, C, H, W] 16-bit, >= +0 -> (pooled in x's dtype, arg-max uint8): torch's max_pool2d and its indices (first maximum in scan order), 15 where the maximum is 0."""
    f, c, h, w = x.shape
    pooled, idx = F.max_pool2d(x.float(), 3, 2, 1, return_indices=True)
    py = torch.arange(h // 2).view(1, 1, -1, 1)
    px = torch.arange(w // 2).view(1, 1, 1, -1)
    k = (idx // w - 2 * py + 1) * 3 + (idx % w - 2 * px + 1)
    assert bool(((k >= 0) & (k < 9)).all())
    k = torch.where(pooled == 0, torch.full_like(k, 15), k)
    return pooled.to(x.dtype), k.to(torch.uint8)


def pool_shares(x):
    """Shares of the pooled elements whose window has: its maximum more than once; only zeros; its first maximum in window row 0; in window column 0."""
    win = pool_windows(x.float())
    mx = win.max(2).values
    _, am = pool_ref(x)
    live = mx > 0
    tie = ((win == mx.unsqueeze(2)).sum(2) > 1) & live
    mean = lambda m: float(m.double().mean())
    return dict(ties=mean(tie), zero=mean(~live), row0=mean(am < 3), col0=mean((am % 3 == 0) & (am < 9)))


@functools.lru_cache(maxsize=None)
def pool_case(name, fmt):
    f, c, h, w = POOL_CASES[name]
    g = _gen(name)
    levels = torch.tensor(POOL_LEVELS)
    x = levels[torch.randint(0, len(levels), (f, c, h, w), generator=g)]
    patch = torch.rand(f, c, -(-h // 4), -(-w // 4), generator=g) < 0.35                 # zeroed 4 x 4 patches: all-zero windows
    x = torch.where(patch.repeat_interleave(4, 2).repeat_interleave(4, 3)[:, :, :h, :w], torch.zeros_like(x), x).to(DT[fmt])
    assert not bool(torch.signbit(x.float()).any())
    pooled, am = pool_ref(x)
    sums, mags = frame_sums(pooled)
    return dict(f=f, c=c, h=h, w=w, x=x, pooled=pooled, argmax=am, sums=sums, allowed=sum_bound(N_ADD_POOL_STATS, mags), shares=pool_shares(x))


# ---- channel_stats -------------------------------------------------------------------------------------------------------------------------------------
#                       name       F  C   H   W
CHANNEL_STATS_CASES = {"hw64": (2, 32, 8, 8),
                       "hw320": (1, 64, 16, 20),       # a partial group of the four loads
                       "hw1024": (2, 32, 32, 32),      # exactly one split
                       "hw1040": (1, 32, 26, 40),      # two splits of 520
                       "hw2304": (1, 96, 48, 48)}


def channel_sums(q):
    """q [F, C, H, W] -> fp64 [F, C, 2] (sum, sum of squares) and the magnitudes [F, C, 2] (sum |q|, sum q^2)."""
    s = q.to(D).reshape(q.shape[0], q.shape[1], -1)
    sq = (s * s).sum(2)
    return torch.stack([s.sum(2), sq], 2), torch.stack([s.abs().sum(2), sq], 2)


@functools.lru_cache(maxsize=None)
def channel_stats_case(name, fmt):
    f, c, h, w = CHANNEL_STATS_CASES[name]
    g = _gen(name)
    gain = 1 + 0.3 * torch.randn(c, generator=g)
    gain[1] = -0.5
    q = (torch.relu(torch.randn(f, c, h, w, generator=g) * 1.3 + 0.4) * gain.view(1, -1, 1, 1)).to(DT[fmt])      # Q = gain * P, as a producer stores it
    sums, mags = channel_sums(q)
    return dict(f=f, c=c, h=h, w=w, q=q, sums=sums, allowed=sum_bound(n_add_channel_stats(h * w), mags))


# ---- nfold_coef ----------------------------------------------------------------------------------------------------------------------------------------
#               name             F  C    H  W
NFOLD_CASES = {"c32": (1, 32, 8, 8),
               "c96_frames3": (3, 96, 8, 8),
               "c288": (3, 288, 4, 4),                 # C > 256: a second trip of the channel loop
               "constant": (3, 96, 8, 8)}              # frame 1 is constant: var_P = 0, r_P = eps^-1/2


@functools.lru_cache(maxsize=None)
def nfold_case(name, fmt):
    """Inputs of vpt_nfold_coef as the engine makes them (tot = the fp64 statistics of P, chs = the per-channel fp64 sums of the stored Q = op16(gain P)),
    random tables [9, CoutPad], and the fp64 reference with its bounds."""
    f, c, h, w = NFOLD_CASES[name]
    dt = DT[fmt]
    g = _gen(name)
    p = torch.relu(torch.randn(f, c, h, w, generator=g) * 1.3 + 0.4).to(dt)
    if name == "constant":
        p[1] = 1.5
    gain = 1 + 0.2 * torch.randn(c, generator=g)
    gain[3] = -0.7                                                  # a negative gain
    bias = 0.1 * torch.randn(c, generator=g)
    q = (p.float() * gain.view(1, -1, 1, 1)).to(dt)
    pad = (c + 127) // 128 * 128
    sa, sg, tb, tg = (torch.randn(9, pad, generator=g) * s for s in (0.3, 1.0, 0.3, 1.0))
    tot, _ = frame_sums(p)
    chs, _ = channel_sums(q)
    out = dict(f=f, c=c, hw=h * w, pad=pad, p=p, q=q, gain=gain, bias=bias, sa=sa, sg=sg, tb=tb, tg=tg, tot=tot, chs=chs)
    out.update(nfold_ref(tot, chs, gain, bias, sa, sg, tb, tg, h * w))
    if name == "constant":
        assert out["var_p"][1].item() == 0.0
    return out


def nfold_ref(tot, chs, gain, bias, sa, sg, tb, tg, hw):
    """-> dict: the four outputs in fp64 (kk [F, 9, CoutPad], rs [F], res_scale [F], res_bias [F, C]), their bounds (b_kk, b_rs, b_res_scale, b_res_bias) and the
    intermediates (mu_p, var_p, r_p, kappa, mu_x, var_x, r_x)."""
    f, c, _ = chs.shape
    n = float(c * hw)
    gn, bs = gain.to(D).view(1, c), bias.to(D).view(1, c)
    mu_p = tot[:, 0].to(D) / n
    var_p = (tot[:, 1].to(D) / n - mu_p * mu_p).clamp(min=0)
    r_p = 1.0 / torch.sqrt(var_p + NORM_EPS)
    kappa = r_p * mu_p
    q1, q2 = chs[:, :, 0].to(D), chs[:, :, 1].to(D)
    rp, kp = r_p.view(f, 1), kappa.view(f, 1)
    b = bs - kp * gn                                                                         # [F, C]
    sx = (rp * q1 + hw * b).sum(1)
    sxx = (rp * rp * q2 + 2.0 * rp * b * q1 + hw * b * b).sum(1)
    mu_x = sx / n
    var_x = (sxx / n - mu_x * mu_x).clamp(min=0)
    r_x = 1.0 / torch.sqrt(var_x + NORM_EPS)
    rx, mx = r_x.view(f, 1, 1), mu_x.view(f, 1, 1)
    t_sa, t_tb, t_tg, t_sg = sa.to(D).unsqueeze(0), rx * tb.to(D).unsqueeze(0), rx * kappa.view(f, 1, 1) * tg.to(D).unsqueeze(0), rx * mx * sg.to(D).unsqueeze(0)
    kk = t_sa + t_tb - t_tg - t_sg
    # ---- bounds (docstring, 5.)
    b_abs = bs.abs() + (kp * gn).abs()
    mean_z2 = (rp * rp * (q2 - 2.0 * mu_p.view(f, 1) * gn * q1 + hw * (mu_p.view(f, 1) * gn) ** 2)).sum(1).clamp(min=0) / n      # mean of z^2, z = r_P (Q - mu_P gain)
    rms_z = torch.sqrt(mean_z2)
    mag_x = (rp * q1.abs() + hw * b_abs).sum(1) / n                                          # all-magnitudes forms of sum x / n and sum x^2 / n
    mag_xx = (rp * rp * q2 + 2.0 * rp * b_abs * q1.abs() + hw * b_abs * b_abs).sum(1) / n
    d_m = (mu_p - mu_p.float().to(D)).abs()                                                  # |mu_P - m'|: a property of the input, at most u |mu_P|
    d_mu = U32 * E_RP * rms_z + (1 + U32 * E_RP) * r_p * d_m * gn.abs().mean() + N_FP64 * U64 * mag_x
    d_sigma = U32 * E_RP * rms_z + (1 + U32 * E_RP) * r_p * d_m * torch.sqrt((gn * gn).mean())
    sigma = torch.sqrt(var_x)
    e_rx = (sigma + d_sigma) * d_sigma / (var_x + NORM_EPS) + 3.5 * U32 + 0.5 * N_FP64 * U64 * (mag_xx + mag_x * mag_x) / (var_x + NORM_EPS)      # relative error of r_x'
    erx = e_rx.view(f, 1, 1)
    big_m = t_sa.abs() + t_tb.abs() + t_tg.abs() + t_sg.abs()
    b_kk = (3 * U32 * big_m + t_tb.abs() * (erx + U32) + t_tg.abs() * (erx + (E_KAPPA + 3) * U32) + t_sg.abs() * (erx + 3 * U32)
            + rx * sg.to(D).abs().unsqueeze(0) * d_mu.view(f, 1, 1))
    return dict(kk=kk, rs=r_x * r_p, res_scale=r_p, res_bias=b, b_kk=b_kk, b_rs=(r_x * r_p) * (e_rx + (E_RP + 1) * U32), b_res_scale=r_p * E_RP * U32,
                b_res_bias=U32 * (E_KAPPA * (kp * gn).abs() + b_abs), mu_p=mu_p, var_p=var_p, r_p=r_p, kappa=kappa, mu_x=mu_x, var_x=var_x, r_x=r_x, e_rx=e_rx)


# ---- throughput statistics: the cases of tests/test_gpu_conv_mfma16.py plus pool32 of tests/test_gpu_conv_fwd_bitwise.py --------------------------------
#                    name        frames h   w   cin cout
THROUGHPUT_CASES = {"one_block": (1, 16, 16, 32, 96),
                    "two_blocks": (1, 48, 16, 64, 160),
                    "loop_once": (1, 16, 80, 96, 128),
                    "interior": (2, 64, 64, 64, 128),
                    "pool32": (1, 32, 32, 64, 160)}


@functools.lru_cache(maxsize=None)
def throughput_case(name, fmt):
    """CPU operands of a throughput case (the statistics' reference is the kernel's own output: nothing in fp64 here but stats_in)."""
    frames, h, w, cin, cout = THROUGHPUT_CASES[name]
    dt = DT[fmt]
    g = _gen(name)
    W = torch.randn(cout, cin, 3, 3, generator=g) * (1.6 / (cin * 9) ** 0.5)
    gain = 1 + 0.2 * torch.randn(cin, generator=g)
    bias = 0.1 * torch.randn(cin, generator=g)
    x = (torch.relu(torch.randn(frames, cin, h, w, generator=g)) + 0.2 * torch.randn(frames, cin, h, w, generator=g)).to(dt)
    res = torch.randn(frames, cout, h, w, generator=g).to(dt)
    wpk, sa, sg = packing.pack_conv3x3(W, gain, bias, dtype=dt)
    stats_in, _ = frame_sums(x)
    kk = 0.3 * torch.randn(frames, 9, sa.shape[1], generator=g)
    rs = 0.5 + torch.rand(frames, generator=g)
    rsc = 0.5 + torch.rand(frames, generator=g)
    rb = 0.3 * torch.randn(frames, cout, generator=g)
    out_gain = 1 + 0.3 * torch.randn(cout, generator=g)
    out_gain[1] = -0.5
    return dict(frames=frames, h=h, w=w, cin=cin, cout=cout, dt=dt, x=x, res=res, wpk=wpk, sa=sa, sg=sg, stats_in=stats_in, kk=kk, rs=rs, rsc=rsc, rb=rb,
                out_gain=out_gain)
