"""tests/cnn_forward_ref.py on the CPU, before a GPU sees any of it (tests/test_gpu_cnn_forward_fp64.py is the GPU half): an fp32 emulation of each kernel's
arithmetic in the kernel's order meets every bound at every shape, and the bounds see the defects they are there for.

a. Emulations.  conv3x3 latency: the K order (channel block, kernel row, kernel column, 16-channel half: one fp32 addition per MFMA) through a three-slot stage
   ring, then kk = sa - rstd mean sg, fma, ReLU, residual; its statistics in the lane / wave_sum / eight-wave order of the unrounded values.  The throughput
   kernel's statistics in the lane order of epilogue16 (pairs by dot2), wave_sum and the wave tree, for 16- and 32-row tiles; the pool-fused modes' in-tile
   items plus the seam kernel's walk.  Max pool: the kernel's clamped loads, row / column masks and strict `>` scan.  channel_stats: the lane's serial run, four
   shuffle levels, the waves.  nfold_coef: the fp64 sums from the fp32 r_P' and m', rsqrtf as a correctly rounded fp32 value, the three multiply-adds.
b. Mutations of the emulations, each of which must leave the bound (ratio > 1) on the cases it touches; the one rounding-only mutation must stay inside.  A lost
   lane or wave partial is lost in every workgroup, as a defect of the program would be.  The lost lane (four values) is asserted on the sums of STORED values
   (throughput kernel, max pool, channel_stats); on the latency kernel's sums of unrounded values it is printed only: their allowed error carries every element's
   accumulation bound, which four values of a tile's 8192 do not exceed (ratio 0.02 - 1.1), while a wave's partial does.
c. Nothing is excluded silently: the max-pool comparison covers every element (15 where the window's maximum is 0) and the share of such windows, of ties and of
   maxima in row 0 / column 0 of the window is asserted here."""
import pytest
import torch
import torch.nn.functional as F

import vpt_amd  # noqa: F401
from oracle.vpt_oracle import NORM_EPS
from tests import cnn_forward_ref as R

D = torch.float64
F32 = torch.float32
LANE = torch.arange(64)


# ---- summation trees ---------------------------------------------------------------------------------------------------------------------------------------
def _serial(v, square=False):
    """v fp32 [..., n] -> [...]: s += v[i] (square: s = fmaf(v[i], v[i], s), one rounding) in order."""
    s = torch.zeros(v.shape[:-1], dtype=F32)
    for i in range(v.shape[-1]):
        s = (s.double() + v[..., i].double() ** 2).float() if square else s + v[..., i]
    return s


def _butterfly(s, offsets):
    """s fp32 [..., 64]: v += __shfl_xor(v, o) for o in offsets."""
    for o in offsets:
        s = s + s[..., LANE ^ o]
    return s


def _wave_tree(s):
    """s fp32 [..., waves] -> [...]: (r0 + r1) + (r2 + r3) [+ ((r4 + r5) + (r6 + r7))]."""
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def _block_sums(v, offsets=(32, 16, 8, 4, 2, 1), drop_lane=None, drop_wave=None):
    """v fp32 [F, groups, waves, 64, n] -> fp64 [F, 2]: per group (a workgroup) the lanes' serial sums, the butterfly, the wave tree in fp32; fp64 across groups.
    drop_lane = (wave, lane, i0, i1): that lane's values i0:i1 are left out; drop_wave = wave: that wave's partial is -- in EVERY workgroup, as a defect of the
    program would show (every workgroup runs the same program)."""
    if drop_lane is not None:
        w, l, i0, i1 = drop_lane
        v = v.clone()
        v[:, :, w, l, i0:i1] = 0
    out = []
    for square in (False, True):
        s = _butterfly(_serial(v, square), offsets)[..., 0]          # [F, groups, waves]
        if drop_wave is not None:
            s = s.clone()
            s[:, :, drop_wave] = 0
        out.append(_wave_tree(s).double().sum(1))
    return torch.stack(out, 1)


def _sums_ratio(got, want, allowed):
    err = (got - want).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / allowed).max().item()


# ---- conv3x3, latency tiling -------------------------------------------------------------------------------------------------------------------------------
def _rstd32(stats_in, n):
    m = stats_in[:, 0] / n
    var = (stats_in[:, 1] / n - m * m).clamp(min=0)
    rstd = (1.0 / torch.sqrt((var.float() + torch.tensor(NORM_EPS, dtype=F32)).double())).float()      # rsqrtf as the correctly rounded value
    return m.float().view(-1, 1, 1, 1), rstd.view(-1, 1, 1, 1)


def emu_latency(c, use_res, mut=None):
    """-> (v fp32 unrounded [F, cout, h, w], y in the 16-bit format).  mut: None | "tap" | "halo" | "stage"."""
    frames, h, w, cin, cout = c["frames"], c["h"], c["w"], c["cin"], c["cout"]
    ncb = cin // 32
    x, w16 = c["x"].float(), c["w16"].float()

    def halo(cb):      # the channel block's image with its zeroed border, as S_WRITE_A leaves it in a stage
        a = F.pad(x[:, cb * 32:(cb + 1) * 32], (1, 1, 1, 1))
        if mut == "halo":      # the column right of the image keeps what its lanes loaded: a_gbyte = 0, the block's pixel (0, 0)
            a[:, :, 1:h + 1, w + 1] = x[:, cb * 32:(cb + 1) * 32, 0, 0].unsqueeze(2)
        return a
    slots = [halo(0), None, None]
    acc = torch.zeros(frames, cout, h, w, dtype=F32)
    for cb in range(ncb):
        a = slots[cb % 3]
        if a is None:      # a stage nothing was written to
            a = torch.zeros(frames, 32, h + 2, w + 2, dtype=F32)
        for tap in range(9):
            dy, dx = tap // 3, tap % 3
            for half in range(2):
                part = torch.einsum("oc,fchw->fohw", w16[:, cb * 32 + half * 16:cb * 32 + half * 16 + 16, dy, dx], a[:, half * 16:half * 16 + 16, dy:dy + h, dx:dx + w])
                if mut == "tap" and cb == ncb - 1 and tap == 0:
                    part[:, :, h - 1, w - 1] = 0
                acc = acc + part
        if cb + 1 < ncb:
            slots[(cb if mut == "stage" else cb + 1) % 3] = halo(cb + 1)
    mean, rstd = _rstd32(c["stats_in"], cin * h * w)
    kk = c["sa"][:, :cout][c["e"]].permute(2, 0, 1).unsqueeze(0) - (rstd * mean) * c["sg"][:, :cout][c["e"]].permute(2, 0, 1).unsqueeze(0)
    v = torch.relu(rstd * acc + kk)
    if use_res:
        v = v + c["res"].float()
    return v, v.to(c["dt"])


def _latency_lanes(v):
    """v fp32 [F, cout, h, w] -> [F, workgroups, 8 waves, 64 lanes, 16]: wave = pixel rows 2w, 2w + 1; lane (hi, l31): pixel (sub_row(l31), l31 & 15), channels
    4 hi + 8 g + j in the order (g, j)."""
    f, cout, h, w = v.shape
    t = v.view(f, cout // 32, 4, 2, 4, h // 16, 8, 2, w // 16, 16)        # f, cbo, g, hi, j, ty, wave, r, tx, col
    t = t.permute(0, 1, 5, 8, 6, 3, 7, 9, 2, 4)                            # f, cbo, ty, tx, wave, hi, r, col, g, j
    t = t.reshape(f, -1, 8, 2, 32, 16)                                    # l = r * 16 + col
    l31 = torch.arange(32)
    r = ((l31 >> 4) ^ (l31 >> 2) ^ (l31 >> 3)) & 1                         # sub_row
    return t[:, :, :, :, r * 16 + (l31 & 15)].reshape(f, -1, 8, 64, 16)


@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.LATENCY_CASES))
def test_latency_emulation_inside_the_bound(name, fmt, use_res):
    c = R.latency_case(name, fmt)
    v, y = emu_latency(c, use_res)
    worst, msg = R.failure(y, c["y64"][use_res], c["bound"][use_res], f"latency {name} {fmt} res={use_res}")
    want, allowed = R.latency_stats_ref(c, use_res)
    lanes = _latency_lanes(v)
    r_st = _sums_ratio(_block_sums(lanes), want, allowed)
    print(f"latency {name} {fmt} res={use_res}: worst err / bound {worst:.4f}, stats_out {r_st:.4f}, table and residual terms / P {c['dominated']:.3f}")
    assert msg is None, msg
    assert r_st <= 1.0
    r_wave = _sums_ratio(_block_sums(lanes, drop_wave=7), want, allowed)
    r_lane = _sums_ratio(_block_sums(lanes, drop_lane=(0, 0, 0, 4)), want, allowed)
    print(f"latency {name} {fmt} res={use_res}: statistics without one wave partial {r_wave:.3g}; without one lane's four values {r_lane:.3g} (not asserted: the "
          f"bound of the UNROUNDED sums carries every element's accumulation error, which four values need not exceed)")
    assert r_wave > 1.0


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.LATENCY_CASES))
def test_latency_mutations_fall_outside(name, fmt):
    c = R.latency_case(name, fmt)
    ncb = c["cin"] // 32
    for mut in ("tap", "halo", "stage"):
        if mut == "stage" and ncb == 1:      # one channel block: no second stage is ever written
            continue
        _, y = emu_latency(c, False, mut)
        r = R.ratio(y, c["y64"][False], c["bound"][False])
        print(f"latency {name} {fmt} mutation {mut}: worst err / bound {r.max().item():.3g}, {int((r > 1).sum())} elements outside")
        assert bool((r > 1.0).any()), mut
        if mut == "tap":      # nothing but the bottom-right pixel moves
            r[:, :, c["h"] - 1, c["w"] - 1] = 0
            assert bool((r <= 1.0).all())


# ---- statistics of the throughput kernel -------------------------------------------------------------------------------------------------------------------
def _emu_throughput_pre(c, res=False):
    """A stored tensor of the throughput kernel's kind: an fp32 convolution of the case's x with weights of its own (the statistics' reference is whatever
    tensor was stored: any 16-bit tensor of this shape and sparsity serves), scaled, shifted, ReLU (+ residual), rounded."""
    _, rstd = _rstd32(c["stats_in"], c["cin"] * c["h"] * c["w"])
    g = torch.Generator().manual_seed(3)
    wgt = torch.randn(c["cout"], c["cin"], 3, 3, generator=g) * (1.6 / (c["cin"] * 9) ** 0.5)
    v = torch.relu(rstd * F.conv2d(c["x"].float(), wgt.to(c["dt"]).float(), padding=1) - 0.3)
    if res:
        v = v + c["res"].float()
    return v.to(c["dt"])


def _fwd_lanes(y, rows):
    """y 16-bit [F, cout, h, w] -> fp32 [F, tiles, rows / 4 waves, 64, 128]: epilogue16's order.  Wave (wm, wn) = rows 8 wm .. + 7, channels 64 wn .. + 63; lane
    (q16, c16) = pixel column pcol(c16), channels 8 q16 .. + 7 of each 32-block; serial over (j, n2, h) with the packed halves .x (values 0, 1) and .y (2, 3),
    returned as [.., 2 halves, 64] flattened so that _serial over the first 64 and the last 64 gives s_sum2.x and s_sum2.y."""
    f, cout, h, w = y.shape
    nt = (cout + 127) // 128
    v = torch.zeros(f, nt * 128, h, w, dtype=F32)
    v[:, :cout] = y.float()
    wm_n = rows // 8
    c16 = torch.arange(16)
    pcol = torch.where(c16 < 4, 2 * c16, torch.where(c16 < 12, 2 * (c16 - 4) + 1, 2 * (c16 - 8)))
    t = v.view(f, nt, 2, 2, 4, 2, 2, 2, h // rows, wm_n, 8, w // 16, 16)      # f, nt, wn, n2, q16, hh, xy, e, ty, wm, j, tx, col
    t = t[..., pcol]                                                         # col -> c16
    t = t.permute(0, 8, 11, 1, 9, 2, 4, 12, 6, 10, 3, 5, 7)                   # f, ty, tx, nt, wm, wn, q16, c16, xy, j, n2, hh, e
    return t.reshape(f, -1, wm_n * 2, 64, 128)


def _fwd_block_sums(lanes, **kw):
    """s_sum2.x and s_sum2.y run apart and are added before wave_sum: emulated as two serial runs whose sum enters the tree."""
    f, g, wv, _, _ = lanes.shape
    halves = lanes.view(f, g, wv, 64, 2, 64)
    if kw.get("drop_lane") is not None:
        w_, l_, i0, i1 = kw.pop("drop_lane")
        halves = halves.clone()
        halves[:, :, w_, l_, :, i0:i1] = 0
    out = []
    for square in (False, True):
        s = _serial(halves[..., 0, :], square) + _serial(halves[..., 1, :], square)
        s = _butterfly(s, (32, 16, 8, 4, 2, 1))[..., 0]
        if kw.get("drop_wave") is not None:
            s = s.clone()
            s[:, :, kw["drop_wave"]] = 0
        out.append(_wave_tree(s).double().sum(1))
    return torch.stack(out, 1)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.THROUGHPUT_CASES))
def test_throughput_stats_emulation_and_mutations(name, fmt, res):
    c = R.throughput_case(name, fmt)
    y = _emu_throughput_pre(c, res)
    for rows, n_add in ((16, R.N_ADD_FWD16), (32, R.N_ADD_FWD32)):
        if c["h"] % rows:
            continue
        want, allowed = R.stored_stats_ref(y, n_add)
        lanes = _fwd_lanes(y, rows)
        r0 = _sums_ratio(_fwd_block_sums(lanes), want, allowed)
        # the first (j, n2, h) group of a lane in the image's interior whose four values are not all zero: two values of each packed half
        v = lanes.view(*lanes.shape[:4], 2, 64)
        live = (v[0, 0, 0, :, :, 0:2].abs().sum((1, 2)) > 0).nonzero()
        lane = int(live[0]) if len(live) else 0
        r_lane = _sums_ratio(_fwd_block_sums(lanes, drop_lane=(0, lane, 0, 2)), want, allowed)
        r_wave = _sums_ratio(_fwd_block_sums(lanes, drop_wave=1), want, allowed)
        print(f"throughput stats {name} {fmt} res={res} rows {rows}: emulation {r0:.4f}; without one lane's four values {r_lane:.3g}; without one wave partial {r_wave:.3g}")
        assert r0 <= 1.0 and r_lane > 1.0 and r_wave > 1.0


def _pool_fused_sums(pre, seam_twice=False):
    """pre 16-bit [F, cout, h, w] >= 0 (the pre-pool tensor) -> fp64 [F, 2]: the pool-fused modes' statistics.  In-tile items (thread tid: pooled row 2 it + (tid
    >> 7), column (tid >> 4) & 7, octet tid & 15, complete pixels only) + vpt_pool_seam_kernel's walk over the pixels of a tile's first pooled row / column."""
    f, cout, h, w = pre.shape
    nt, ty_n, tx_n, ph, pw = (cout + 127) // 128, h // 16, w // 16, h // 2, w // 2
    x = torch.zeros(f, nt * 128, h, w, dtype=F32)
    x[:, :cout] = pre.float()
    tiles = x.view(f, nt * 128, ty_n, 16, tx_n, 16).permute(0, 2, 4, 1, 3, 5).reshape(-1, nt * 128, 16, 16)
    part = F.max_pool2d(tiles, 3, 2, 1).view(f, ty_n, tx_n, nt, 16, 8, 4, 2, 8)      # f, ty, tx, nt, oct, k, it, tb, pi   (the in-tile part of every maximum)
    complete = torch.ones(ty_n, tx_n, 8, 8, dtype=torch.bool)                        # ty, tx, pj, pi
    complete[1:, :, 0, :] = False
    complete[:, 1:, :, 0] = False
    if not seam_twice:
        part = part * complete.view(1, ty_n, tx_n, 1, 1, 1, 4, 2, 8)
    lanes = part.permute(0, 1, 2, 3, 7, 8, 4, 6, 5).reshape(f, -1, 4, 64, 32)         # tid = tb 128 + pi 16 + oct -> (wave, lane); serial (it, k)
    total = _block_sums(lanes)
    # seam pixels, in the kernel's order
    pooled = F.max_pool2d(x, 3, 2, 1)
    pix = [((p // pw + 1) * 8, p % pw) for p in range((ty_n - 1) * pw)]
    col_len = ph - (ty_n - 1)
    for t in range(tx_n - 1):
        for k in range(col_len):
            pix.append((0 if k == 0 else (k - 1) // 7 * 8 + (k - 1) % 7 + 1, (t + 1) * 8))
    if pix:
        m = -(-len(pix) // 64)
        jj = torch.tensor([p[0] for p in pix]); ii = torch.tensor([p[1] for p in pix])
        vals = torch.zeros(f, nt * 128, m * 64, dtype=F32)
        vals[:, :, :len(pix)] = pooled[:, :, jj, ii]
        vals = vals.view(f, nt * 4, 4, 8, m, 4, 16)                                   # f, cb, oct, k, m, wave, slot
        s = []
        for square in (False, True):
            t_ = _serial(vals.permute(0, 1, 5, 6, 2, 4, 3).reshape(f, nt * 4, 4, 16, 4, m * 8), square)      # f, cb, wave, slot, oct
            for o in (1, 2, 4, 8):                                                    # off = 4 .. 32 of tid = slot 4 + oct: the slot's four bits
                t_ = t_ + t_[:, :, :, torch.arange(16) ^ o]
            t_ = _wave_tree(t_[:, :, :, 0].permute(0, 1, 3, 2))                       # f, cb, oct
            s.append(_serial(t_).double().sum(1))                                    # `t += ...` over the four octets, fp64 across workgroups
        total = total + torch.stack(s, 1)
    return total


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.THROUGHPUT_CASES))
def test_pool_fused_stats_emulation_and_seam_mutation(name, fmt):
    c = R.throughput_case(name, fmt)
    pre = _emu_throughput_pre(c)
    pooled = F.max_pool2d(pre.float(), 3, 2, 1).to(c["dt"])
    want, allowed = R.stored_stats_ref(pooled, R.n_add_pool_fused(c["h"], c["w"]))
    r0 = _sums_ratio(_pool_fused_sums(pre), want, allowed)
    r_twice = _sums_ratio(_pool_fused_sums(pre, seam_twice=True), want, allowed)
    seams = c["h"] > 16 or c["w"] > 16
    print(f"pool-fused stats {name} {fmt}: emulation {r0:.4f}; seam pixels counted twice {r_twice:.3g}" + ("" if seams else " (one tile: no seam, nothing changes)"))
    assert r0 <= 1.0
    assert r_twice > 1.0 if seams else r_twice == r0


# ---- max pool ----------------------------------------------------------------------------------------------------------------------------------------------
def emu_pool(x, last=False, unmasked_row0=False):
    """vpt_pool_kernel's scan on the bit patterns' order (values >= +0 order like their patterns): clamped loads, the row / column masks, strict `>`."""
    f, c, h, w = x.shape
    ph, pw = h // 2, w // 2
    xf = x.float()
    py, px = torch.arange(ph), torch.arange(pw)
    yy = [(2 * py - 1).clamp(min=0), 2 * py, 2 * py + 1]
    xx = [(2 * px - 1).clamp(min=0), 2 * px, 2 * px + 1]
    m = torch.zeros(f, c, ph, pw)
    am = torch.full((f, c, ph, pw), 15, dtype=torch.uint8)
    for q in range(9):
        v = xf[:, :, yy[q // 3]][:, :, :, xx[q % 3]]
        if q < 3 and not unmasked_row0:
            v = v * (py > 0).view(1, 1, -1, 1)
        if q % 3 == 0:
            v = v * (px > 0).view(1, 1, 1, -1)
        take = (v >= m) & (v > 0) if last else v > m
        am = torch.where(take, torch.full_like(am, q), am)
        m = torch.maximum(m, v)
    return m.to(x.dtype), am


def _pool_lanes(pooled):
    """pooled 16-bit [F, C, PH, PW] -> fp32 [F, blocks, 4, 64, 32]: item = ((cb PH + py) PW + px) 4 + oct, thread t of a block takes items t + 256 it."""
    f, c, ph, pw = pooled.shape
    items = pooled.float().view(f, c // 32, 4, 8, ph, pw).permute(0, 1, 4, 5, 2, 3).reshape(f, -1, 8)
    blocks = -(-items.shape[1] // 1024)
    pad = torch.zeros(f, blocks * 1024, 8)
    pad[:, :items.shape[1]] = items
    return pad.view(f, blocks, 4, 4, 64, 8).permute(0, 1, 3, 4, 2, 5).reshape(f, blocks, 4, 64, 32)


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.POOL_CASES))
def test_pool_emulation_shares_and_mutations(name, fmt):
    c = R.pool_case(name, fmt)
    sh = c["shares"]
    print(f"maxpool {name} {fmt}: windows with a tie {sh['ties']:.1%}, all zero {sh['zero']:.1%} (arg-max 15, compared like every other), first maximum in "
          f"window row 0 {sh['row0']:.1%}, column 0 {sh['col0']:.1%}")
    assert 0.02 < sh["zero"] < 1.0 / 3.0 and sh["ties"] > 0.1
    if c["h"] > 2:      # (the 2 x 2 frame has one window, whose row 0 and column 0 are padding)
        assert sh["row0"] > 0.1 and sh["col0"] > 0.1
    m, am = emu_pool(c["x"])
    assert torch.equal(m.view(torch.int16), c["pooled"].view(torch.int16)) and torch.equal(am, c["argmax"])
    r_st = _sums_ratio(_block_sums(_pool_lanes(m)), c["sums"], c["allowed"])
    lanes = _pool_lanes(m)
    live = (lanes[0, 0, 0, :, 0:4].abs().sum(1) > 0).nonzero()
    r_lane = _sums_ratio(_block_sums(lanes, drop_lane=(0, int(live[0]), 0, 4)), c["sums"], c["allowed"])
    print(f"maxpool {name} {fmt}: statistics emulation {r_st:.4f}; without one lane's four values {r_lane:.3g}")
    assert r_st <= 1.0 and r_lane > 1.0
    _, am_last = emu_pool(c["x"], last=True)
    n_last = int((am_last != c["argmax"]).sum())
    _, am_row = emu_pool(c["x"], unmasked_row0=True)
    wrong = am_row != c["argmax"]
    print(f"maxpool {name} {fmt}: last maximum instead of first: {n_last} arg-max bytes differ; row-0 clamp unmasked: {int(wrong.sum())} differ")
    assert n_last > 0 and bool(wrong.any())
    assert bool((wrong[:, :, 1:] == 0).all()) and bool((am_row[wrong] == c["argmax"][wrong] - 3).all())      # 0 where 3 belongs (1 / 4, 2 / 5), in pooled row 0 only


# ---- channel_stats -----------------------------------------------------------------------------------------------------------------------------------------
def emu_channel_stats(q, drop_lane=False):
    """q 16-bit [F, C, H, W] -> fp64 [F, C, 2]: per (channel block, split) a workgroup; thread (pixel slot tid >> 2, octet tid & 3) walks every 64th pixel."""
    f, c, h, w = q.shape
    hw = h * w
    split, per = R.channel_stats_split(hw)
    n = -(-per // 64)
    x = torch.zeros(f, c, split, n * 64, dtype=F32)
    flat = q.float().reshape(f, c, hw)
    for sp in range(split):
        seg = flat[:, :, sp * per:min((sp + 1) * per, hw)]
        x[:, :, sp, :seg.shape[2]] = seg
    x = x.view(f, c, split, n, 4, 16)                      # pixel = i 64 + wave 16 + slot
    if drop_lane:
        x = x.clone()
        x[:, 0, 0, :4, 0, 0] = 0
    out = []
    for square in (False, True):
        s = _serial(x.permute(0, 1, 2, 4, 5, 3), square)   # f, c, split, wave, slot
        for o in (1, 2, 4, 8):
            s = s + s[..., torch.arange(16) ^ o]
        out.append(_wave_tree(s[..., 0]).double().sum(2))
    return torch.stack(out, 2)


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.CHANNEL_STATS_CASES))
def test_channel_stats_emulation_and_lost_lane(name, fmt):
    c = R.channel_stats_case(name, fmt)
    r0 = _sums_ratio(emu_channel_stats(c["q"]), c["sums"], c["allowed"])
    r_lane = _sums_ratio(emu_channel_stats(c["q"], drop_lane=True), c["sums"], c["allowed"])
    print(f"channel_stats {name} {fmt}: n_add {R.n_add_channel_stats(c['h'] * c['w'])}, emulation {r0:.4f}; without one lane's (up to) four values {r_lane:.3g}")
    assert r0 <= 1.0 and r_lane > 1.0


# ---- nfold_coef --------------------------------------------------------------------------------------------------------------------------------------------
def emu_nfold(c, mut=None):
    """vpt_nfold_coef_kernel: fp64 sums from r_P' = rsqrtf((float)var_P + eps) and m' = (float)mu_P, fp32 coefficients and multiply-adds.
    mut: "stats_of_p" (mu_P, r_P where mu_x, r_x belong) | "kappa_unrounded" (kappa from the fp64 mu_P)."""
    f, ch, hw = c["f"], c["c"], c["hw"]
    n = float(ch * hw)
    eps = torch.tensor(NORM_EPS, dtype=F32)
    rsqrtf = lambda v: (1.0 / torch.sqrt((v.float() + eps).double())).float()
    mu_p = c["tot"][:, 0] / n
    var_p = (c["tot"][:, 1] / n - mu_p * mu_p).clamp(min=0)
    r_p = rsqrtf(var_p).double()
    kappa = r_p * (mu_p if mut == "kappa_unrounded" else mu_p.float().double())
    q1, q2 = c["chs"][:, :, 0], c["chs"][:, :, 1]
    b = c["bias"].double().view(1, ch) - kappa.view(f, 1) * c["gain"].double().view(1, ch)
    rp = r_p.view(f, 1)
    sx = (rp * q1 + hw * b).sum(1)
    sxx = (rp * rp * q2 + 2.0 * rp * b * q1 + hw * b * b).sum(1)
    mu_x = sx / n
    var_x = (sxx / n - mu_x * mu_x).clamp(min=0)
    r_x = rsqrtf(var_x)
    if mut == "stats_of_p":
        mu_x, r_x = mu_p, r_p.float()
    c_b, c_g, c_s = r_x, -r_x * kappa.float(), -r_x * mu_x.float()
    v3 = lambda t: t.view(f, 1, 1)
    kk = ((c["sa"].unsqueeze(0) + v3(c_b) * c["tb"].unsqueeze(0)) + v3(c_g) * c["tg"].unsqueeze(0)) + v3(c_s) * c["sg"].unsqueeze(0)
    return dict(kk=kk, rs=r_x * r_p.float(), res_scale=r_p.float(), res_bias=b.float())


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.NFOLD_CASES))
def test_nfold_emulation_and_mutations(name, fmt):
    c = R.nfold_case(name, fmt)
    got = {m: emu_nfold(c, m) for m in (None, "stats_of_p", "kappa_unrounded")}
    worst = {m: {k: R.ratio(got[m][k].double(), c[k], c["b_" + k]).max().item() for k in ("kk", "rs", "res_scale", "res_bias")} for m in got}
    print(f"nfold_coef {name} {fmt}: emulation " + ", ".join(f"{k} {v:.4f}" for k, v in worst[None].items()))
    print(f"nfold_coef {name} {fmt}: statistics of P for those of x: kk {worst['stats_of_p']['kk']:.3g}, rs {worst['stats_of_p']['rs']:.3g}; "
          f"kappa from the unrounded mu_P: kk {worst['kappa_unrounded']['kk']:.4f}, res_bias {worst['kappa_unrounded']['res_bias']:.4f}")
    assert max(worst[None].values()) <= 1.0
    assert worst["stats_of_p"]["kk"] > 1.0
    assert max(worst["kappa_unrounded"].values()) <= 1.0      # a rounding difference, not an error: the bound is not vacuous the other way round


def test_nfold_reference_is_group_norm_of_the_pooled_tensor():
    """The formulas are the operation: with the r_x, mu_x of the reference, x = r_P Q + b has the statistics the reference derives from the per-channel sums."""
    c = R.nfold_case("c96_frames3", "fp16")
    x = c["r_p"].view(-1, 1, 1, 1) * c["q"].double() + c["res_bias"].view(c["f"], c["c"], 1, 1)
    flat = x.reshape(c["f"], -1)
    assert torch.allclose(flat.mean(1), c["mu_x"], rtol=0, atol=1e-12) and torch.allclose(flat.var(1, unbiased=False), c["var_x"], rtol=1e-10)
    assert torch.allclose(c["rs"], c["r_p"] / torch.sqrt(flat.var(1, unbiased=False) + NORM_EPS), rtol=1e-10)


def test_counted_chain_lengths():
    assert (R.N_ADD_FWD16, R.N_ADD_FWD32, R.N_ADD_POOL_TILE, R.N_ADD_POOL_STATS, R.N_ADD_LATENCY_STATS) == (73, 74, 40, 40, 25)
    assert R.n_add_pool_seam(16, 16) == 0 and R.n_add_pool_seam(32, 32) == 8 * 1 + 10 and R.n_add_pool_seam(64, 64) == 8 * 3 + 10      # 0, 31 and 183 seam pixels
    assert [R.n_add_channel_stats(hw) for hw in (64, 320, 1024, 1040, 2304)] == [7, 11, 22, 15, 18]
    assert R.channel_stats_split(1040) == (2, 520) and R.channel_stats_split(2304) == (3, 768)
