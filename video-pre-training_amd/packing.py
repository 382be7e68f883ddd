"""Host-side weight re-packing into the layouts the gfx950 kernels stream (see DESIGN.md §Data layout).

All functions take fp32 torch tensors with the reference's shapes (the `.weights` state_dict,
SURVEY.md §8b) and return new tensors on the same device; the fp32 masters are left untouched.
"""
import collections
import math

import torch


def _ceil_div(a, b):
    return (a + b - 1) // b


def pack_conv3x3(weight, gain, bias, tables=True, dtype=torch.bfloat16):
    """Conv2d weight [Cout,Cin,3,3] with the preceding GroupNorm(1,Cin) affine (gain, bias [Cin]) folded.

    Returns (wpk bf16 [NT][Cin/32][9][128][32], edge_sa fp32 [9][NT*128], edge_sg fp32 [9][NT*128]).
    wpk holds bf16(W * gain), each 64-byte row (one cout, 32 cin) stored with its four 16-byte chunks
    XOR-swizzled by ((cout >> 2) & 3): the tile is DMA'd to LDS verbatim and read conflict-free; edge_sg[e][o] = sum over the taps valid for edge class e and over Cin of that
    rounded value; edge_sa[e][o] = same sum of W * bias (fp32).  e = 3*ey + ex with ey/ex in
    {0: first row/col, 1: interior, 2: last row/col} (vpt_conv3x3.hip epilogue)."""
    cout, cin = weight.shape[:2]
    assert cin % 32 == 0 and cout % 32 == 0
    nt = _ceil_div(cout, 128)
    cp = nt * 128
    wg = (weight * gain.view(1, -1, 1, 1)).to(dtype)
    wp = torch.zeros(cp, cin, 3, 3, dtype=dtype, device=weight.device)
    wp[:cout] = wg
    wpk = wp.view(nt, 128, cin // 32, 32, 9).permute(0, 2, 4, 1, 3).contiguous()
    wpk = swizzle_rows64(wpk)
    if not tables:
        return wpk, None, None
    sg_tap = torch.zeros(cp, 9, dtype=torch.float64, device=weight.device)
    sa_tap = torch.zeros(cp, 9, dtype=torch.float64, device=weight.device)
    sg_tap[:cout] = wg.double().sum(dim=1).view(cout, 9)
    sa_tap[:cout] = (weight.double() * bias.double().view(1, -1, 1, 1)).sum(dim=1).view(cout, 9)
    m = edge_tap_matrix(weight.device)                    # [9 edge classes, 9 taps]
    return wpk, (m @ sa_tap.t()).float().contiguous(), (m @ sg_tap.t()).float().contiguous()


_EDGE_TAP = {}


def edge_tap_matrix(device, dtype=torch.float64):
    """0/1 matrix [9 edge classes e = 3*ey + ex, 9 taps kh*3 + kw]: the tap reads inside the image for pixels of that class."""
    key = (str(device), dtype)
    if key not in _EDGE_TAP:
        valid = {0: [1, 2], 1: [0, 1, 2], 2: [0, 1]}
        m = torch.zeros(9, 9, dtype=dtype)
        for ey in range(3):
            for ex in range(3):
                for kh in valid[ey]:
                    for kw in valid[ex]:
                        m[ey * 3 + ex, kh * 3 + kw] = 1
        _EDGE_TAP[key] = m.to(device)
    return _EDGE_TAP[key]


def pack_conv3x3_dgrad(weight, gain, dtype=torch.bfloat16):
    """Weights of the input-gradient convolution of a normed conv layer: Wd[c, o, kh, kw] = op16(W * gain)[o, c, 2-kh, 2-kw]
    in the same packed format (a conv with Cin' = Cout, Cout' = Cin, no further gain)."""
    wg = (weight * gain.view(1, -1, 1, 1)).to(dtype).float()
    wd = wg.permute(1, 0, 2, 3).flip(2, 3).contiguous()
    wpk, _, _ = pack_conv3x3(wd, torch.ones(wd.shape[1], device=weight.device), None, tables=False, dtype=dtype)
    return wpk


def swizzle_rows64(t):
    """[..., rows, 32] bf16 -> same shape with chunk c (8 elements) of row r stored at chunk c ^ ((r >> 2) & 3).
    The permutation is an involution, so applying it twice restores the logical order."""
    rows = t.shape[-2]
    v = t.reshape(*t.shape[:-1], 4, 8)
    r = torch.arange(rows, device=t.device)
    idx = (torch.arange(4, device=t.device).view(1, 4) ^ ((r >> 2) & 3).view(rows, 1))  # [rows, 4]: source chunk per slot
    idx = idx.view(*([1] * (v.dim() - 3)), rows, 4, 1).expand(*v.shape)
    return torch.gather(v, -2, idx).reshape(t.shape).contiguous()


# K slot -> k of the first conv's two MFMA k-steps (vpt_conv_first_tile.h): values 0..7 of kernel row 0, 1, 2 (each one 16-byte
# read of the 16-bit input tile), then the ninth value of the three rows, the two bias slots and three zero slots.
CONV_FIRST_SLOT_K = [9 * (s >> 3) + (s & 7) for s in range(24)] + [8, 17, 26, 27, 28, 29, 30, 31]


def pack_conv_first(weight, bias, dtype=torch.bfloat16):
    """Stack-0 firstconv weight [Cout,3,3,3] + bias [Cout] -> MFMA A-operand fragments
    bf16 [NT][4][2][64][8] (vpt_conv_first.hip).  k = (kh*3+kw)*3 + ch for k < 27 holds W / 255 (the pixel operand is
    the raw byte 0..255); k = 27 / 28 carry the hi / lo bf16 halves of the bias (the pixel operand holds 1.0 there);
    the 32 values of a row are stored in the slot order CONV_FIRST_SLOT_K."""
    cout = weight.shape[0]
    assert weight.shape[1:] == (3, 3, 3) and cout % 32 == 0
    nt = _ceil_div(cout, 128)
    cp = nt * 128
    wk = torch.zeros(cp, 32, dtype=torch.float32, device=weight.device)
    wk[:cout, :27] = weight.permute(0, 2, 3, 1).reshape(cout, 27) / 255.0
    hi = bias.to(dtype).float()
    lo = (bias - hi).to(dtype).float()
    wk[:cout, 27] = hi
    wk[:cout, 28] = lo
    wk = wk[:, torch.tensor(CONV_FIRST_SLOT_K, device=wk.device)].contiguous()
    # [nt][cs][l31][ks][hi][e] -> [nt][cs][ks][hi][l31][e]
    frag = wk.view(nt, 4, 32, 2, 2, 8).permute(0, 1, 3, 4, 2, 5).contiguous().view(nt, 4, 2, 64, 8)
    return frag.to(dtype).contiguous()


def pack_conv3d_t5(weight, bias, dtype=torch.bfloat16):
    """IDM Conv3d weight [O,3,5,1,1] + bias [O] -> (MFMA A-operand fragments bf16 [NT][4][64][8], bias fp32 [NT*128]).
    k = dt*3 + ch for k < 15 (dt = temporal tap 0..4), k = 15 is zero padding (vpt_conv3d.hip)."""
    o = weight.shape[0]
    assert tuple(weight.shape[1:]) == (3, 5, 1, 1) and o % 32 == 0
    nt = _ceil_div(o, 128)
    cp = nt * 128
    wk = torch.zeros(cp, 16, dtype=torch.float32, device=weight.device)
    wk[:o, :15] = weight.reshape(o, 3, 5).permute(0, 2, 1).reshape(o, 15)
    frag = wk.view(nt, 4, 32, 2, 8).permute(0, 1, 3, 2, 4).contiguous().view(nt, 4, 64, 8)
    bp = torch.zeros(cp, dtype=torch.float32, device=weight.device)
    bp[:o] = bias
    return frag.to(dtype).contiguous(), bp


def pack_linear(weight, dtype=torch.bfloat16):
    """nn.Linear weight [N,K] -> bf16 [ceil(N/128)][K/32][128][32] (vpt_gemm.hip B operand)."""
    n, k = weight.shape
    assert k % 64 == 0
    nt = _ceil_div(n, 128)
    wp = torch.zeros(nt * 128, k, dtype=dtype, device=weight.device)
    wp[:n] = weight.to(dtype)
    return wp.view(nt, 128, k // 32, 32).permute(0, 2, 1, 3).contiguous()


def chw_to_blocked_columns(weight, c, h, w):
    """Permute the K axis of a [N, c*h*w] matrix from the reference's C,H,W flatten order
    (lib/impala_cnn.py:192-193) to the blocked activation order [c/32][h][w][32]."""
    n = weight.shape[0]
    return weight.view(n, c // 32, 32, h, w).permute(0, 1, 3, 4, 2).reshape(n, c * h * w).contiguous()


def chw_to_blocked_vector(v, c, h, w):
    return v.view(c // 32, 32, h, w).permute(0, 2, 3, 1).reshape(-1).contiguous()


def blocked_to_nchw(x_blocked, c, h, w):
    """bf16 [F][c/32][h][w][32] -> fp32 [F][c][h][w] (tests / debugging only)."""
    f = x_blocked.shape[0]
    return x_blocked.view(f, c // 32, h, w, 32).permute(0, 1, 4, 2, 3).reshape(f, c, h, w).float()


def nchw_to_blocked(x, dtype=torch.bfloat16):
    f, c, h, w = x.shape
    return x.view(f, c // 32, 32, h, w).permute(0, 1, 3, 4, 2).contiguous().to(dtype)


def episode_bounds(first, state_mask, maxlen):
    """Episode boundaries of a [B, t] chunk in the row coordinates of [memory (maxlen rows) ; chunk (t rows)] -- the host twin of
    vpt_episode_bounds_kernel (ops.episode_bounds), for the attention mode that honours `first` at EVERY frame (what stepping the
    reference one frame at a time computes, behavioural_cloning.py:95-112 over lib/masked_attention.py:161-178).
    first bool [B, t]; state_mask bool [B, maxlen] (or [B, 1, maxlen], or None = nothing valid).  Returns
      qlo int32 [B, t]: the lowest row query frame i may see = maxlen + (latest p <= i with first[b, p]), 0 when there is none;
      next mask bool [B, maxlen]: kept row j = t + r is valid iff j >= qlo[b, t-1] and (j >= maxlen or state_mask[b, j])."""
    bsz, t = first.shape
    dev = first.device
    first = first.to(torch.bool)
    if state_mask is None:
        state_mask = torch.zeros(bsz, maxlen, dtype=torch.bool, device=dev)
    state_mask = state_mask.reshape(bsz, maxlen).to(torch.bool)
    idx = torch.arange(t, device=dev).view(1, t).expand(bsz, t)
    start = torch.where(first, idx, torch.full_like(idx, -1)).cummax(dim=1).values          # s(i), -1 = none
    qlo = torch.where(start >= 0, start + maxlen, torch.zeros_like(start)).to(torch.int32)
    rows = torch.cat([state_mask, torch.ones(bsz, t, dtype=torch.bool, device=dev)], dim=1)   # validity of every row of [memory ; chunk]
    j = t + torch.arange(maxlen, device=dev).view(1, maxlen)
    return qlo, rows[:, t:] & (j >= qlo[:, -1:])


MAX_LABEL_WINDOW = 160     # the mask="none" attention kernel's longest chunk (IDMEngine.forward)

LabelWindows = collections.namedtuple("LabelWindows", "starts length owner")
IDMFeaturePlan = collections.namedtuple("IDMFeaturePlan", "n_frames window stride starts length owner src lo hi win_rows sel_rows")


def label_windows(n_frames: int, window: int, stride: int) -> LabelWindows:
    """The overlapping windows a video of n_frames is labelled in, and the window each frame takes its label from (host integers).
    Windows start at 0, stride, 2 stride, ... while start + window <= n_frames, plus one at n_frames - window if the last of those does
    not end the video; a video shorter than `window` is one window of its own length.  Frame f belongs to the window in which it is most
    central -- the smallest |2 (f - start) - (length - 1)|, the earlier window on ties -- so at window 128, stride 64 an interior window
    labels its offsets 32..95, and only the first and the last window label frames near their own edges.
    -> (starts int32 [W], length, owner int32 [n_frames])."""
    n, L, S = int(n_frames), int(window), int(stride)
    if n < 1:
        raise ValueError("label_windows: n_frames must be at least 1")
    if not (1 <= S <= L <= MAX_LABEL_WINDOW):
        raise ValueError(f"label_windows: need 1 <= stride <= window <= {MAX_LABEL_WINDOW}, got window {L}, stride {S}")
    if n < L:
        starts, L = [0], n
    else:
        starts = list(range(0, n - L + 1, S))
        if starts[-1] != n - L:
            starts.append(n - L)
    st = torch.tensor(starts, dtype=torch.int64)
    f = torch.arange(n, dtype=torch.int64).view(n, 1)
    off = f - st.view(1, -1)
    cost = (2 * off - (L - 1)).abs()
    cost = torch.where((off >= 0) & (off < L), cost, torch.full_like(cost, 4 * MAX_LABEL_WINDOW))
    # the FIRST minimum (ties go to the lower window): the smallest of cost * W + k
    owner = (cost * len(starts) + torch.arange(len(starts)).view(1, -1)).min(dim=1).values % len(starts)
    return LabelWindows(st.to(torch.int32), L, owner.to(torch.int32))


def idm_feature_plan(n_frames: int, window: int, stride: int) -> IDMFeaturePlan:
    """Which per-frame IDM features a labelling pass must compute, once each.  Everything in front of the transformer blocks is per-frame work
    except the temporal Conv3d(5,1,1), which zero-pads at the edges of ITS window (lib/policy.py:394-403): row (window k, offset o), frame
    f = s_k + o, sees the frames [max(s_k, f - 2), min(s_k + L, f + 3)) and nothing else of the window.  Rows with the same key
    (f, that lower bound, that upper bound) have identical features -- all but the two rows at either end of a window share the interior
    key (f, f - 2, f + 3) with every other window that holds f.  The distinct keys, sorted, are the slots: at most n_frames + 4 W of them,
    against W L window rows.
    -> label_windows' fields plus src, lo, hi int32 [n_slots] (ops.conv3d_t5_indexed), win_rows int32 [W L] (the slot of every window row)
    and sel_rows int32 [n_frames] (the window row k L + o that labels each frame).  CPU tensors."""
    starts, L, owner = label_windows(n_frames, window, stride)
    n, W = int(n_frames), starts.numel()
    s = starts.to(torch.int64).view(W, 1)
    f = s + torch.arange(L, dtype=torch.int64).view(1, L)                     # [W, L]
    lo = torch.maximum(s.expand(W, L), f - 2)
    hi = torch.minimum((s + L).expand(W, L), f + 3)
    # one sortable integer per key: the bounds as their offsets from f (2 - (f - lo) in 0..2, hi - f - 1 in 0..2)
    key = (f * 3 + (lo - f + 2)) * 3 + (hi - f - 1)
    uniq, inverse = torch.unique(key.reshape(-1), sorted=True, return_inverse=True)
    src = uniq // 9
    slot_lo = src + (uniq // 3) % 3 - 2
    slot_hi = src + uniq % 3 + 1
    assert uniq.numel() <= n + 4 * W
    own = owner.to(torch.int64)
    sel = own * L + (torch.arange(n, dtype=torch.int64) - starts.to(torch.int64)[own])
    i32 = lambda t: t.to(torch.int32).contiguous()
    return IDMFeaturePlan(n, int(window), int(stride), starts, L, owner, i32(src), i32(slot_lo), i32(slot_hi), i32(inverse), i32(sel))


def bc_loss_metrics(lp_buttons, lp_camera, act_buttons, act_camera, weight=None):
    """Per-frame records and totals of the weighted BC loss -- the host twin of vpt_bc_loss_kernel (ops.bc_loss), in fp64 torch; the
    formulas of lib/action_head.py:176-193 (logprob of the label, entropy) and behavioural_cloning.py:107 (their negated sum is the loss).
    lp_* [M, n] log-probs; act_* int [M]; weight [M] or None (all ones).  Returns
      frame_out fp64 [M, 8]: nll_b, nll_c, ent_b, ent_c, hit_b, hit_c, w, 0 -- the frame's own (unweighted) values; an entropy term with
                 p == 0 counts 0, a hit is `arg-max (lowest index on ties) == label`, a label outside [0, n) picks nothing (nll 0, no hit);
      totals fp64 [8]: sum_rows w * frame_out[row, :6], sum w, number of rows with w > 0; a row with w == 0 adds exact zeros whatever it holds."""
    m = lp_buttons.shape[0]
    dev = lp_buttons.device
    w = torch.ones(m, dtype=torch.float64, device=dev) if weight is None else weight.reshape(m).to(torch.float64)
    cols = []
    for lp, act in ((lp_buttons, act_buttons), (lp_camera, act_camera)):
        lp = lp.to(torch.float64)
        act = act.reshape(m, 1).to(torch.int64)
        onehot = torch.arange(lp.shape[1], device=dev).view(1, -1) == act
        nll = -torch.where(onehot, lp, torch.zeros_like(lp)).sum(-1)
        p = lp.exp()
        ent = -torch.where(p == 0, torch.zeros_like(lp), p * lp).sum(-1)
        hit = (lp.argmax(-1, keepdim=True) == act).reshape(m).to(torch.float64)
        cols.append((nll, ent, hit))
    frame_out = torch.stack([cols[0][0], cols[1][0], cols[0][1], cols[1][1], cols[0][2], cols[1][2], w, torch.zeros_like(w)], dim=1)
    live = (w != 0).view(m, 1)
    rec = torch.where(live, w.view(m, 1) * frame_out[:, :6], torch.zeros_like(frame_out[:, :6]))
    totals = torch.cat([rec.sum(0), torch.where(live.view(m), w, torch.zeros_like(w)).sum().view(1), (w > 0).sum().to(torch.float64).view(1)])
    return frame_out, totals


def idm_loss_metrics(lp_buttons, lp_camera, act_buttons, act_camera, weight=None):
    """Per-frame records and totals of the IDM's weighted loss -- the host twin of vpt_idm_loss_kernel (ops.idm_loss), in fp64 torch.  The IDM's heads
    are independent categorical groups (lib/action_head.py:176-184: logprob = the groups' gathers, summed): lp_buttons [M, G_b, n_b],
    lp_camera [M, G_c, n_c] log-probs; act_* int [M, G]; weight [M] or None (all ones).  Returns
      frame_out fp64 [M, 8]: nll_b, nll_c, ent_b, ent_c -- sums over the head's groups; an entropy term with p == 0 counts 0 --, hit_b, hit_c -- the
                 fraction of the head's groups whose arg-max (lowest index on ties) is the label; a label outside [0, n) picks nothing --, w, 0;
      totals fp64 [8]: sum_rows w * frame_out[row, :6], sum w, number of rows with w > 0; a row with w == 0 adds exact zeros whatever it holds."""
    m = lp_buttons.shape[0]
    dev = lp_buttons.device
    w = torch.ones(m, dtype=torch.float64, device=dev) if weight is None else weight.reshape(m).to(torch.float64)
    cols = []
    for lp, act in ((lp_buttons, act_buttons), (lp_camera, act_camera)):
        lp = lp.to(torch.float64)
        groups, n = lp.shape[1:]
        act = act.reshape(m, groups, 1).to(torch.int64)
        onehot = torch.arange(n, device=dev).view(1, 1, n) == act
        nll = -torch.where(onehot, lp, torch.zeros_like(lp)).sum(dim=(1, 2))
        p = lp.exp()
        ent = -torch.where(p == 0, torch.zeros_like(lp), p * lp).sum(dim=(1, 2))
        hit = (lp.argmax(-1, keepdim=True) == act).reshape(m, groups).to(torch.float64).mean(1)
        cols.append((nll, ent, hit))
    frame_out = torch.stack([cols[0][0], cols[1][0], cols[0][1], cols[1][1], cols[0][2], cols[1][2], w, torch.zeros_like(w)], dim=1)
    live = (w != 0).view(m, 1)
    rec = torch.where(live, w.view(m, 1) * frame_out[:, :6], torch.zeros_like(frame_out[:, :6]))
    totals = torch.cat([rec.sum(0), torch.where(live.view(m), w, torch.zeros_like(w)).sum().view(1), (w > 0).sum().to(torch.float64).view(1)])
    return frame_out, totals


def idm_loss_grad(lp_buttons, lp_camera, act_buttons, act_camera, scale, weight=None):
    """The host twin of ops.idm_loss's dz, unrounded and unpadded: fp64 [M, G_b n_b + G_c n_c] = scale * w_r * (exp(lp) - onehot), buttons first."""
    m = lp_buttons.shape[0]
    w = torch.ones(m, dtype=torch.float64, device=lp_buttons.device) if weight is None else weight.reshape(m).to(torch.float64)
    parts = []
    for lp, act in ((lp_buttons, act_buttons), (lp_camera, act_camera)):
        lp = lp.to(torch.float64)
        groups, n = lp.shape[1:]
        onehot = torch.arange(n, device=lp.device).view(1, 1, n) == act.reshape(m, groups, 1).to(torch.int64)
        g = (lp.exp() - onehot.to(torch.float64)) * (scale * w).view(m, 1, 1)
        parts.append(torch.where((w != 0).view(m, 1, 1), g, torch.zeros_like(g)).reshape(m, groups * n))
    return torch.cat(parts, 1)
