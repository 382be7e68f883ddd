"""References for the kernels every frame passes through first: vpt_conv_first_kernel (uint8 ingest + first conv + ReLU + 3x3/2 max-pool),
vpt_conv3d_t5_kernel and its indexed twin (the IDM's temporal conv) and vpt_affine_kernel (GroupNorm `n`, the 65536-wide LayerNorm).
Plain torch, fp64, importable without a GPU.

Every reference is an fp64 evaluation over the SAME operands the kernel multiplies (the 16-bit-rounded weights as the pack kernels make them, the raw
bytes, the stored 16-bit activations), so only the kernel's own arithmetic is judged.  Every bound has the form of tests/test_gpu_conv_mfma16.py,

    |y - y64| <= ulp16(y64) + (K + 8) * 2^-24 * A                                  (u = 2^-24: unit roundoff of fp32)

one unit in the last place of the stored format at y64 (twice the half ulp a rounding to nearest may cost: room for a y that rounds across a binade edge) plus
the fp32 error of the kernel's K-term sum relative to A, the same expression as y64 with every term replaced by its absolute value.  Derived, not tuned:

1. conv_first.  Operands W16 = op16(fl32(W / 255)) (vpt_pack_conv_first_kernel: __fdiv_rn, then one rounding), bh = op16(b), bl = op16(b - bh), raw bytes.
       pre64 = conv2d(img, W16, padding 1) + bh + bl,      y64 = max_pool2d(relu(pre64), 3, 2, 1)
       K = 29 (27 taps and the two bias slots of the MFMA's 32),      A = max_pool2d(conv2d(img, |W16|) + |bh| + |bl|)
   A byte times an 8- or 11-bit significand is exact in fp32, so only the 28 additions of the accumulation round, each by at most u relative to a partial sum
   that A bounds: (K - 1) u A, taken as (K + 8) u A like everywhere else in this suite.  ReLU and the window maximum are 1-Lipschitz and monotone: the pooled error
   is at most the largest per-pixel error in the window, and the window maximum of the per-pixel bound is that.  The rounding to 16 bits comes after the maximum
   (rounding is monotone: the kernel rounds the maximum once).

2. conv3d_t5, plain and indexed.  Operands W16 = op16(W), bytes; the bias stays in fp32.
       y64 = relu(sum_{dt, c} W16[o][c][dt] * byte[f + dt - 2][p][c] / 255 + b[o]),  taps outside the slot's window are zero
       K = 15,      A = sum |W16| * byte / 255 + |b|
   14 additions in the MFMA; the `+ 8` covers fl32(1 / 255) (u), the product with it and the addition of the bias (one fma: u on each term).

3. frame_affine.  From stats_in = (s, ss) exactly as frame_mean_rstd defines it: m = s / n, var = max(ss / n - m^2, 0), r = 1 / sqrt(var + eps),
       y64 = (x - m) * r * g + b,      A = (|x| + |m|) * r * |g| + |b|,      constant 8 (no K: nothing is summed)
   The kernel evaluates fma(fma(x, rstd, shift), g, b) with mean = fl32(m), rstd = rsqrtf(fl32(var) + eps), shift = fl32(-mean * rstd).  In units of u:
       rstd:   fl32(var) and the addition of eps one each, halved by the power -1/2 -> 1;  rsqrtf <= 1 ulp = 2  ->  3
       mean:   1
       shift:  3 (rstd) + 1 (mean) + 1 (the product)                                                  ->  5
       term x * r * g:   3 (rstd) + 1 (inner fma) + 1 (outer fma)                                     ->  5
       term m * r * g:   5 (shift) + 1 (inner fma) + 1 (outer fma)                                    ->  7
       term b:           1 (outer fma)                                                                ->  1
   each relative to its own term of A, so 8 u A holds with room for the second-order terms.

STATISTICS.  `sum_bound(n_add, mag)` = n_add * u * mag bounds an fp32 sum whose longest chain of additions is n_add, mag = the sum of the magnitudes.  The counts:

   conv_first stats_out    sums of the STORED (rounded, unscaled) values; the squares of 16-bit values are exact in fp32.  Per lane and half-tile 16 values are added
                           in fp32 (eight two-element dot products); everything after that (across half-tiles, tiles, lanes, waves) is fp64.        n_add = 16
   conv_first chs_out      sums of the stored (rounded, scaled) values.  A lane adds the 2 half-tiles of every tile of a GROUP of tiles in fp32 (group = 16 when
                           the frame's tile count is a multiple of 16, else the whole frame), then five shuffle levels combine the 32 pixels of a half-wave;
                           fp64 across groups.                                                                                    n_add = 2 * group + 5
   conv3d_t5 stats_out     sums of the UNROUNDED fp32 values v: a thread adds up to 128 values (2 pixels x 4 channel blocks x 16), six shuffle levels, the four waves
                           in two more.  |sum v - sum y64| <= sum e + n_add u sum(|y64| + e) with e the per-element accumulation bound (no ulp16: nothing was
                           rounded to 16 bits); for the squares |v^2 - y64^2| <= e (2 |y64| + e) and each fma of the chain rounds once.      n_add = 128 + 6 + 2
   frame_affine stats_out  as conv3d_t5 with 32 values per thread (4 items x 8).                                                    n_add = 32 + 6 + 2
"""
import functools

import torch
import torch.nn.functional as F

from oracle.vpt_oracle import NORM_EPS

D = torch.float64
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {"bf16": 7, "fp16": 10}
EMIN = {"bf16": -126, "fp16": -14}
U32 = 2.0 ** -24          # unit roundoff of fp32

K_CONV_FIRST, K_CONV3D, C_AFFINE = 29, 15, 8
N_ADD_CONV_FIRST_STATS = 16
N_ADD_CONV3D_STATS = 128 + 6 + 2
N_ADD_AFFINE_STATS = 32 + 6 + 2


def ulp16(v, fmt):
    """One unit in the last place of the 16-bit format at |v| (the form of tests/test_gpu_conv_mfma16.py)."""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** EMIN[fmt]))).clamp(min=EMIN[fmt])
    return torch.pow(torch.tensor(2.0, dtype=D), e - MANT[fmt])


def ratio(y, y64, bound):
    """err / bound per element with 0 / 0 = 0 (an exact zero under a zero bound is no error); a non-finite y counts as infinitely wrong."""
    err = (y.to(D) - y64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isfinite(y.to(D)), r, torch.full_like(r, float("inf")))


def failure(y, y64, bound, what):
    """-> (worst err / bound over ALL elements, None or a message with the count and the first failing index)."""
    r = ratio(y, y64, bound)
    worst = r.max().item()
    bad = ~(r <= 1.0)
    if not bool(bad.any()):
        return worst, None
    idx = tuple(bad.nonzero()[0].tolist())
    return worst, (f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound (worst err / bound {worst:.3f}); first at {idx}: "
                   f"got {y[idx].item()}, fp64 {y64[idx].item()}, bound {bound[idx].item():.3e}")


def frame_sums(y):
    """[F, ...] -> fp64 [F, 2] (sum, sum of squares) and [F, 2] (sum of magnitudes, sum of squares)."""
    flat = y.to(D).reshape(y.shape[0], -1)
    sq = (flat * flat).sum(1)
    return torch.stack([flat.sum(1), sq], 1), torch.stack([flat.abs().sum(1), sq], 1)


def sum_bound(n_add, mag):
    return n_add * U32 * mag


# ---- conv_first ----------------------------------------------------------------------------------------------------------------------------------
def conv_first_operands(weight, bias, fmt):
    """fp32 weight [Cout, 3, 3, 3], bias [Cout] -> (W16, bh, bl) in the 16-bit format, as vpt_pack_conv_first_kernel / packing.pack_conv_first make them."""
    dt = DT[fmt]
    w16 = (weight.float() / 255.0).to(dt)
    bh = bias.float().to(dt)
    bl = (bias.float() - bh.float()).to(dt)
    return w16, bh, bl


def conv_first_ref(img_u8, w16, bh, bl, fmt):
    """img_u8 [F, H, W, 3] uint8 -> (y64, bound) [F, Cout, H/2, W/2]."""
    x = img_u8.permute(0, 3, 1, 2).to(D)
    w = w16.to(D)
    bias = (bh.to(D) + bl.to(D)).view(1, -1, 1, 1)
    bias_abs = (bh.to(D).abs() + bl.to(D).abs()).view(1, -1, 1, 1)
    y64 = F.max_pool2d(torch.relu(F.conv2d(x, w, padding=1) + bias), 3, 2, 1)
    mag = F.max_pool2d(F.conv2d(x, w.abs(), padding=1) + bias_abs, 3, 2, 1)
    return y64, ulp16(y64, fmt) + (K_CONV_FIRST + 8) * U32 * mag


def conv_first_chs_group(h, w, cout):
    """-> (group, groups per frame): the tiles whose per-channel sums share an fp32 accumulator in vpt_conv_first_kernel<CHS> (one channel tile: cout <= 128)."""
    tiles = (h // 16) * (w // 16) * ((cout + 127) // 128)
    group = 16 if tiles % 16 == 0 else tiles
    return group, tiles // group


# ---- conv3d_t5 -----------------------------------------------------------------------------------------------------------------------------------
def conv3d_windows(frames, t):
    """(src, lo, hi) of the plain kernel: slot f is frame f, its taps stay inside its own sequence [f - f % t, + t)."""
    src = torch.arange(frames)
    lo = src - src % t
    return src, lo, lo + t


def conv3d_taps(img_u8, src, lo, hi):
    """img_u8 [N, H, W, 3], int [S] each -> fp64 [S, 5, H, W, 3]: tap dt of slot j is img[src[j] + dt - 2] inside [max(lo, 0), min(hi, N)), else zero."""
    n = img_u8.shape[0]
    x = img_u8.to(D)
    taps = torch.zeros((len(src), 5) + tuple(img_u8.shape[1:]), dtype=D)
    for j, (s, a, b) in enumerate(zip(src.tolist(), lo.tolist(), hi.tolist())):
        for dt in range(5):
            ft = s + dt - 2
            if max(a, 0) <= ft < min(b, n):
                taps[j, dt] = x[ft]
    return taps


def conv3d_ref(taps, w16, bias, fmt):
    """taps [S, 5, H, W, 3] (conv3d_taps), w16 [O, 3, 5, 1, 1] in the 16-bit format, bias fp32 [O] -> (y64, bound16, acc_bound) [S, O, H, W];
    acc_bound = the accumulation part alone, what the kernel's UNROUNDED values (its statistics) are held to."""
    w = w16.to(D).reshape(-1, 3, 5)
    b = bias.to(D).view(1, -1, 1, 1)
    y64 = torch.relu(torch.einsum("ocd,sdhwc->sohw", w, taps) / 255.0 + b)
    mag = torch.einsum("ocd,sdhwc->sohw", w.abs(), taps) / 255.0 + b.abs()
    acc = (K_CONV3D + 8) * U32 * mag
    return y64, ulp16(y64, fmt) + acc, acc


def unrounded_stats_bound(y64, acc, n_add):
    """Allowed error [F, 2] of (sum v, sum v^2) over fp32 values v with |v - y64| <= acc, summed in fp32 with chains of n_add additions."""
    f = y64.shape[0]
    a, e = y64.abs().reshape(f, -1), acc.reshape(f, -1)
    b_sum = e.sum(1) + sum_bound(n_add, (a + e).sum(1))
    b_sq = (e * (2 * a + e)).sum(1) + sum_bound(n_add, ((a + e) ** 2).sum(1))
    return torch.stack([b_sum, b_sq], 1)


# ---- frame_affine --------------------------------------------------------------------------------------------------------------------------------
def affine_ref(x, stats_in, gain, bias, fmt, per_element=False):
    """x [F, C, H, W] (16-bit values), stats_in fp64 [F, 2], gain / bias [C] or, per element, [C*H*W] in C,H,W order -> (y64, bound16, acc_bound)."""
    f, c, h, w = x.shape
    n = c * h * w
    m = stats_in[:, 0].to(D) / n
    var = (stats_in[:, 1].to(D) / n - m * m).clamp(min=0)
    r = (1.0 / torch.sqrt(var + NORM_EPS)).view(f, 1, 1, 1)
    m = m.view(f, 1, 1, 1)
    shape = (1, c, h, w) if per_element else (1, c, 1, 1)
    g, b = gain.to(D).view(shape), bias.to(D).view(shape)
    x = x.to(D)
    y64 = (x - m) * r * g + b
    acc = C_AFFINE * U32 * ((x.abs() + m.abs()) * r * g.abs() + b.abs())
    return y64, ulp16(y64, fmt) + acc, acc


# ---- the cases (shared by tests/test_ingest_ref_cpu.py and tests/test_gpu_ingest_fp64.py; computed once, never modified) -------------------------------
#                     name           frames h   w   cout
CONV_FIRST_CASES = {"all_borders": (2, 16, 16, 128),     # one tile with all four borders: top / left zero records, the clamped first and last records
                    "nt2_partial": (3, 48, 80, 160),     # seams both ways, non-square, two channel tiles with one valid wave in the second
                    "one_wave": (2, 16, 48, 32)}         # one valid wave, column seams only
PERSISTENT_HW_COUT = (48, 80, 128)                       # 15 tiles per frame; the number of frames follows from the device (persistent_frames)

#                 name        B  T  H   W   cout
CONV3D_CASES = {"t1": (1, 1, 16, 16, 32),                # window shorter than the five taps on both sides; one chunk; three of four channel blocks skipped
                "t2_nt2": (2, 2, 16, 16, 160),           # two sequences; two channel tiles, the second partial
                "t4_chunks": (3, 4, 16, 32, 128),        # two chunks per frame
                "t5": (1, 5, 16, 16, 32),                # exactly the five taps
                "t7_nt2": (1, 7, 16, 16, 160)}           # interior frames with all five taps
# The indexed kernel's slots over CONV3D_INDEXED_IMG image frames: (src, lo, hi).  src is not monotonic and repeats 2.
CONV3D_INDEXED_IMG = 12
CONV3D_INDEXED_SLOTS = [(5, 3, 8),       # all five taps
                        (2, 2, 7),       # clipped on the left only
                        (9, 5, 10),      # clipped on the right only
                        (4, 4, 5),       # both: hi - lo = 1, the centre tap alone
                        (1, -3, 6),      # lo < 0: clamped to 0
                        (11, 7, 15),     # hi > n_img: clamped to n_img
                        (6, 0, 12),      # a window wider than five frames
                        (2, 0, 3),       # src repeated, another window
                        (0, 0, 12)]
CONV3D_INDEXED_COUT = (32, 160)

#                 name          frames C   H  W   per_element
AFFINE_CASES = {"partial": (2, 96, 8, 8, False),         # 768 16-byte items: one partial block
                "full_partial": (3, 160, 6, 10, False),  # 1200 items: a full block and a partial one, non-square
                "elem_small": (2, 64, 4, 4, True),       # 128 items per element
                "elem_partial": (1, 160, 6, 10, True)}   # 1200 items per element


def _gen(name):
    return torch.Generator().manual_seed(sum(map(ord, name)))


def persistent_frames(cus):
    """-> (frames, T, cap): the fewest 48 x 80 frames (15 tiles each) with 3 cap < T <= 4 cap, cap = 4 workgroups per CU."""
    cap = 4 * cus
    frames = (3 * cap) // 15 + 1
    return frames, 15 * frames, cap


@functools.lru_cache(maxsize=None)
def conv_first_case(frames, h, w, cout, fmt, name="conv_first"):
    g = _gen(name)
    weight = torch.randn(cout, 3, 3, 3, generator=g) * 0.3
    bias = 0.1 * torch.randn(cout, generator=g)
    gain = 1 + 0.3 * torch.randn(cout, generator=g)
    img = torch.randint(0, 256, (frames, h, w, 3), generator=g, dtype=torch.uint8)
    w16, bh, bl = conv_first_operands(weight, bias, fmt)
    y64, bound = conv_first_ref(img, w16, bh, bl, fmt)
    return dict(frames=frames, h=h, w=w, cout=cout, weight=weight, bias=bias, gain=gain, img=img, w16=w16, bh=bh, bl=bl, y64=y64, bound=bound)


@functools.lru_cache(maxsize=None)
def conv3d_case(name, fmt):
    bsz, t, h, w, cout = CONV3D_CASES[name]
    g = _gen(name)
    weight = torch.randn(cout, 3, 5, 1, 1, generator=g) * 0.4
    bias = 0.1 * torch.randn(cout, generator=g)
    img = torch.randint(0, 256, (bsz * t, h, w, 3), generator=g, dtype=torch.uint8)
    w16 = weight.to(DT[fmt])
    y64, bound, acc = conv3d_ref(conv3d_taps(img, *conv3d_windows(bsz * t, t)), w16, bias, fmt)
    return dict(frames=bsz * t, t=t, h=h, w=w, cout=cout, weight=weight, bias=bias, img=img, w16=w16, y64=y64, bound=bound, acc=acc)


@functools.lru_cache(maxsize=None)
def conv3d_indexed_case(cout, fmt):
    g = _gen(f"indexed{cout}")
    weight = torch.randn(cout, 3, 5, 1, 1, generator=g) * 0.4
    bias = 0.1 * torch.randn(cout, generator=g)
    img = torch.randint(0, 256, (CONV3D_INDEXED_IMG, 16, 16, 3), generator=g, dtype=torch.uint8)
    src, lo, hi = (torch.tensor(v, dtype=torch.int32) for v in zip(*CONV3D_INDEXED_SLOTS))
    w16 = weight.to(DT[fmt])
    y64, bound, acc = conv3d_ref(conv3d_taps(img, src, lo, hi), w16, bias, fmt)
    return dict(cout=cout, weight=weight, bias=bias, img=img, src=src, lo=lo, hi=hi, w16=w16, y64=y64, bound=bound, acc=acc)


@functools.lru_cache(maxsize=None)
def affine_case(name, fmt):
    frames, c, h, w, per_element = AFFINE_CASES[name]
    g = _gen(name)
    x = torch.relu(torch.randn(frames, c, h, w, generator=g)).to(DT[fmt])          # post-ReLU data, as stored
    n = c * h * w if per_element else c
    gain = 1 + 0.2 * torch.randn(n, generator=g)
    bias = 0.1 * torch.randn(n, generator=g)
    stats_in, _ = frame_sums(x)                                                    # the exact fp64 sums of the stored values
    y64, bound, acc = affine_ref(x, stats_in, gain, bias, fmt, per_element)
    return dict(frames=frames, c=c, h=h, w=w, per_element=per_element, x=x, gain=gain, bias=bias, stats_in=stats_in, y64=y64, bound=bound, acc=acc)
