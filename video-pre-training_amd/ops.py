"""Torch-tensor front ends of the C-ABI entry points (one function per symbol of include/vpt_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; all arithmetic happens in
libvpt_hip.so.  Every function requires CUDA(HIP) tensors and raises if the native library is absent.

Argument and return types come from the header (_native.py binds every declaration of it), and so do the VPT_WS_* workspace
numbers below; a wrapper here only has to pass its arguments in the header's order.  The header is therefore read when this module is
imported: an unreadable include/vpt_hip.h raises NativeLibraryError at import, not at the first call.
"""
import ctypes
import os

import torch

from . import _native
from ._native import ptr


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class KernelTimer:
    """Optional per-entry-point HIP-event timing (bench.py / profiling only).  Events are recorded on the
    current torch stream, which is the stream every kernel is launched on."""

    def __init__(self):
        self.enabled = False
        self.records = []  # (name, start_event, stop_event, meta)

    def reset(self):
        self.records = []

    def _accumulate(self, key_of):
        """Sum the records under key_of(name, meta) (None: skip the record)."""
        torch.cuda.synchronize()
        out = {}
        for name, a, b, meta in self.records:
            key = key_of(name, meta)
            if key is None:
                continue
            d = out.setdefault(key, dict(ms=0.0, calls=0, flops=0.0, bytes=0.0))
            d["ms"] += a.elapsed_time(b)
            d["calls"] += 1
            d["flops"] += meta.get("flops", 0.0)
            d["bytes"] += meta.get("bytes", 0.0)
        return out

    def summary(self):
        return self._accumulate(lambda name, meta: name)

    def by_shape(self, prefix="vpt_conv3x3"):
        """Per (label, work size): the same records split by their FLOP / byte count, i.e. by layer shape (profiling: which shapes lose)."""
        return self._accumulate(lambda name, meta: (name, meta.get("flops", 0.0) or meta.get("bytes", 0.0)) if name.startswith(prefix) else None)


TIMER = KernelTimer()


POISON_LDS = os.environ.get("VPT_POISON_LDS", "0") == "1"    # diagnostics: NaN-fill every CU's LDS before each launch (vpt_debug_poison_lds)


def _call(name, meta, *args, fmt="bf16", label=None):
    if POISON_LDS:
        _native.call("vpt_debug_poison_lds", _stream(), fmt=fmt)
    if TIMER.enabled:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _native.call(name, *args, fmt=fmt)
        b.record()
        TIMER.records.append((label or name, a, b, meta or {}))
    else:
        _native.call(name, *args, fmt=fmt)


_WS = _native.header().workspace_ops      # include/vpt_hip.h's VPT_WS_* enum, as parsed: the numbers live in the header only
WS_CONV3X3_WGRAD = _WS["VPT_WS_CONV3X3_WGRAD"]
WS_CONV_BACKWARD_PREPARE = _WS["VPT_WS_CONV_BACKWARD_PREPARE"]
WS_LINEAR_SPLITK = _WS["VPT_WS_LINEAR_SPLITK"]
WS_LAYERNORM_BACKWARD = _WS["VPT_WS_LAYERNORM_BACKWARD"]
WS_COLUMN_SUM = _WS["VPT_WS_COLUMN_SUM"]
WS_ATTENTION_BACKWARD_DKV = _WS["VPT_WS_ATTENTION_BACKWARD_DKV"]
WS_ATTENTION_BACKWARD_DBND = _WS["VPT_WS_ATTENTION_BACKWARD_DBND"]
WS_FRAME_AFFINE_BACKWARD = _WS["VPT_WS_FRAME_AFFINE_BACKWARD"]
WS_CONV_FIRST_BACKWARD = _WS["VPT_WS_CONV_FIRST_BACKWARD"]
WS_BC_LOSS = _WS["VPT_WS_BC_LOSS"]
WS_FULL_ATTENTION_BACKWARD = _WS["VPT_WS_FULL_ATTENTION_BACKWARD"]
WS_CONV3D_T5_BACKWARD = _WS["VPT_WS_CONV3D_T5_BACKWARD"]
WS_RL_LOSS = _WS["VPT_WS_RL_LOSS"]
WS_PPG_AUX_LOSS = _WS["VPT_WS_PPG_AUX_LOSS"]
FULL_ATTENTION_MAX_T = 160      # the mask="none" attention kernels' longest window (forward and backward)


def _workspace(op, a=0, b=0, c=0, d=0, e=0, device=None, fmt="bf16"):
    """fp32 scratch of vpt_workspace_bytes(op, ...) bytes (caller-owned: the library never allocates); None when the entry point needs none."""
    nbytes = int(_native.load(fmt).vpt_workspace_bytes(int(op), int(a), int(b), int(c), int(d), int(e)))
    if nbytes < 0:
        raise RuntimeError(f"vpt_workspace_bytes({op}, {a}, {b}, {c}, {d}, {e}) failed")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None


# The 16-bit operand format of a call (bf16: libvpt_hip.so, fp16: libvpt_hip_f16.so, see include/vpt_hip.h
# vpt_operand_format) is the dtype of its 16-bit tensors; every 16-bit tensor of one call must agree.
OP16 = "op16"
_FMT = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def _fmt(*tensors, dtype=None):
    """-> (torch dtype, library format) of the 16-bit tensors among `tensors` (or of `dtype` when there are none)."""
    dt = dtype
    for t in tensors:
        if t is not None and t.dtype in _FMT:
            if dt is not None and t.dtype != dt:
                raise TypeError(f"mixed 16-bit operand formats in one call: {dt} and {t.dtype}")
            dt = t.dtype
    if dt is None:
        dt = torch.bfloat16
    if dt not in _FMT:
        raise TypeError(f"16-bit operand dtype must be bfloat16 or float16, got {dt}")
    return dt, _FMT[dt]


def _chk(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if dtype is OP16:
        if t.dtype not in _FMT:
            raise TypeError(f"{name}: expected a 16-bit operand tensor (bfloat16 / float16), got {t.dtype}")
    elif t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")


def pack_conv3x3(weight, gain, bias=None, tables=True, dtype=torch.bfloat16):
    """Device re-pack of a GN -> conv3x3 layer (vpt_pack_conv3x3): -> (wpk, edge_sa, edge_sg) exactly as packing.pack_conv3x3."""
    _chk(weight, torch.float32, "weight"); _chk(gain, torch.float32, "gain"); _chk(bias, torch.float32, "bias")
    cout, cin = weight.shape[:2]
    dt, fmt = _fmt(dtype=dtype)
    lib = _native.load(fmt)
    nt = (cout + 127) // 128
    wpk = torch.empty(nt, cin // 32, 9, 128, 32, dtype=dt, device=weight.device)
    assert wpk.numel() == lib.vpt_conv3x3_packed_elems(cout, cin)
    sa = sg = None
    if tables:
        sa = torch.empty(9, nt * 128, dtype=torch.float32, device=weight.device)
        sg = torch.empty(9, nt * 128, dtype=torch.float32, device=weight.device)
    _call("vpt_pack_conv3x3", None, ptr(weight), ptr(gain), ptr(bias), ptr(wpk), ptr(sa), ptr(sg), cout, cin, _stream(), fmt=fmt)
    return wpk, sa, sg


def pack_linear(weight, dtype=torch.bfloat16, transposed=False, k_pad=None):
    """Device re-pack of an nn.Linear weight [N, K] (vpt_pack_linear) -> [ceil(N/128)][K/32][128][32].
    transposed=True: the packed matrix is weight^T, i.e. [K rows][N reduction] with the reduction dimension zero-padded to
    k_pad (a multiple of 64) -- the operand of the input-gradient GEMM dx = dy W (training.linear_backward)."""
    _chk(weight, torch.float32, "weight")
    dt, fmt = _fmt(dtype=dtype)
    rows, cols = weight.shape
    if transposed:
        n_out, k_red, src_rows = cols, (k_pad or rows), rows
    else:
        n_out, k_red, src_rows = rows, cols, rows
    out = torch.empty((n_out + 127) // 128, k_red // 32, 128, 32, dtype=dt, device=weight.device)
    _call("vpt_pack_linear", None, ptr(weight), ptr(out), n_out, k_red, 1 if transposed else 0, cols, src_rows, _stream(), fmt=fmt)
    return out


def pack_conv_first(weight, bias, dtype=torch.bfloat16):
    """Device re-pack of the stack-0 firstconv (vpt_pack_conv_first) -> fragments [NT][4][2][64][8], exactly as packing.pack_conv_first."""
    _chk(weight, torch.float32, "weight"); _chk(bias, torch.float32, "bias")
    cout = weight.shape[0]
    if tuple(weight.shape[1:]) != (3, 3, 3):
        raise ValueError(f"pack_conv_first: weight must be [Cout, 3, 3, 3], got {tuple(weight.shape)}")
    dt, fmt = _fmt(dtype=dtype)
    out = torch.empty((cout + 127) // 128, 4, 2, 64, 8, dtype=dt, device=weight.device)
    assert out.numel() == _native.load(fmt).vpt_conv_first_packed_elems(cout)
    _call("vpt_pack_conv_first", None, ptr(weight), ptr(bias), ptr(out), cout, _stream(), fmt=fmt)
    return out


def pack_conv3d_t5(weight, bias, dtype=torch.bfloat16):
    """Device re-pack of the IDM's temporal conv (vpt_pack_conv3d_t5) -> (fragments [NT][4][64][8], bias fp32 [NT*128])."""
    _chk(weight, torch.float32, "weight"); _chk(bias, torch.float32, "bias")
    o = weight.shape[0]
    if tuple(weight.shape[1:]) != (3, 5, 1, 1):
        raise ValueError(f"pack_conv3d_t5: weight must be [O, 3, 5, 1, 1], got {tuple(weight.shape)}")
    dt, fmt = _fmt(dtype=dtype)
    nt = (o + 127) // 128
    out = torch.empty(nt, 4, 64, 8, dtype=dt, device=weight.device)
    bp = torch.empty(nt * 128, dtype=torch.float32, device=weight.device)
    _call("vpt_pack_conv3d_t5", None, ptr(weight), ptr(bias), ptr(out), ptr(bp), o, _stream(), fmt=fmt)
    return out, bp


def chw_to_blocked(x, c, h, w):
    """fp32 [rows, c*h*w] (or [c*h*w]) in C,H,W flatten order -> the same shape in blocked activation order (vpt_chw_to_blocked)."""
    _chk(x, torch.float32, "x")
    rows = 1 if x.dim() == 1 else x.shape[0]
    if x.numel() != rows * c * h * w:
        raise ValueError(f"chw_to_blocked: {tuple(x.shape)} is not [rows, {c}*{h}*{w}]")
    out = torch.empty_like(x)
    _call("vpt_chw_to_blocked", None, ptr(x), ptr(out), ctypes.c_int64(rows), c, h, w, _stream())
    return out


def conv_first(img_u8, wfrag, cout, stats_out=None, out_gain=None, chs_out=None):
    """img_u8 [F,H,W,3] uint8 -> pooled blocked bf16 [F, cout/32, H/2, W/2, 32].  out_gain fp32 [cout]: stored times it per channel
    (GroupNorm `n`'s gain when the norm is folded into the first block); stats_out are the statistics of the unscaled tensor.
    chs_out fp64 [F, cout, 2] (zeroed; cout <= 128): receives the per-channel sums of the stored tensor (what channel_stats() computes)."""
    _chk(img_u8, torch.uint8, "img"); _chk(wfrag, OP16, "wfrag"); _chk(stats_out, torch.float64, "stats_out"); _chk(out_gain, torch.float32, "out_gain")
    _chk(chs_out, torch.float64, "chs_out")
    f, h, w, _ = img_u8.shape
    dt, fmt = _fmt(wfrag)
    y = torch.empty(f, cout // 32, h // 2, w // 2, 32, dtype=dt, device=img_u8.device)
    _call("vpt_conv_first_forward", dict(flops=2.0 * f * h * w * cout * 27, bytes=f * (h * w * 3 + h * w * cout // 2)), ptr(img_u8), ptr(wfrag), ptr(y), ptr(stats_out), ptr(out_gain), ptr(chs_out), f, h, w, cout, _stream(), fmt=fmt)
    return y


CONV_TILING = {"throughput": 1, "latency": 2, "throughput32": 3}   # throughput32: 32-row / eight-wave tiles where H % 32 == 0 (measured at parity; A/B)


def conv3x3(x, wpk, edge_sa, edge_sg, stats_in, cout, res=None, stats_out=None, out=None, tiling="throughput"):
    """x blocked bf16 [F,Cin/32,H,W,32] -> blocked bf16 [F,cout/32,H,W,32] (GN fold + ReLU [+res]).
    tiling: "throughput" (default: a frame's result must not depend on how many frames share the launch -- chunking, sharding
    over ranks and the batch size are free choices of the caller; the two tilings sum a tile's statistics in different orders),
    or "latency" (the acting step asks for it explicitly) -- vpt_conv3x3_forward_tiled; the library never picks by grid size."""
    _chk(x, OP16, "x"); _chk(wpk, OP16, "wpk"); _chk(edge_sa, torch.float32, "edge_sa")
    _chk(edge_sg, torch.float32, "edge_sg"); _chk(stats_in, torch.float64, "stats_in")
    _chk(res, OP16, "res"); _chk(stats_out, torch.float64, "stats_out")
    f, cb, h, w, _ = x.shape
    dt, fmt = _fmt(x, wpk, res, out)
    if out is None:
        out = torch.empty(f, cout // 32, h, w, 32, dtype=dt, device=x.device)
    meta = dict(flops=2.0 * f * h * w * cout * 9 * cb * 32, bytes=2.0 * f * h * w * (cb * 32 + cout * (2 if res is not None else 1)))
    if tiling not in CONV_TILING:
        raise ValueError(f"conv3x3: tiling must be one of {sorted(CONV_TILING)}, got {tiling!r}")
    _call("vpt_conv3x3_forward_tiled", meta, ptr(x), ptr(wpk), ptr(edge_sa), ptr(edge_sg), ptr(stats_in), ptr(res),
          ptr(out), ptr(stats_out), f, h, w, cb * 32, cout, CONV_TILING[tiling], _stream(), fmt=fmt,
          label="vpt_conv3x3_forward_latency" if tiling == "latency" else "vpt_conv3x3_forward")
    return out


def conv3x3_pool(x, wpk, edge_sa, edge_sg, stats_in, cout, stats_out=None, out=None, out_gain=None, chs_out=None):
    """GN fold + conv3x3 + ReLU + max_pool2d(3, 2, 1) in one pass (vpt_conv3x3_pool_forward): x blocked [F,Cin/32,H,W,32] -> pooled
    [F,cout/32,H/2,W/2,32] (+ its frame statistics into stats_out) -- what conv3x3() followed by maxpool() returns, bit for bit, without
    the pre-pool tensor's round trip through HBM.  Inference path of the stacks' firstconv (the BC step keeps the pre-pool tensor)."""
    _chk(x, OP16, "x"); _chk(wpk, OP16, "wpk"); _chk(edge_sa, torch.float32, "edge_sa"); _chk(edge_sg, torch.float32, "edge_sg")
    _chk(stats_in, torch.float64, "stats_in"); _chk(stats_out, torch.float64, "stats_out"); _chk(out, OP16, "out"); _chk(out_gain, torch.float32, "out_gain"); _chk(chs_out, torch.float64, "chs_out")
    f, cb, h, w, _ = x.shape
    dt, fmt = _fmt(x, wpk, out)
    if out is not None and (tuple(out.shape) != (f, cout // 32, h // 2, w // 2, 32) or not out.is_contiguous()):
        raise ValueError("conv3x3_pool: out must be a contiguous [F, cout/32, H/2, W/2, 32] tensor")
    y = out if out is not None else torch.empty(f, cout // 32, h // 2, w // 2, 32, dtype=dt, device=x.device)
    seam = torch.empty(_native.load(fmt).vpt_conv3x3_pool_seam_elems(f, h, w, cout), dtype=dt, device=x.device)
    meta = dict(flops=2.0 * f * h * w * cout * 9 * cb * 32, bytes=2.0 * f * h * w * (cb * 32 + cout * 0.25))
    args = (ptr(x), ptr(wpk), ptr(edge_sa), ptr(edge_sg), ptr(stats_in), ptr(y), ptr(seam), ptr(stats_out), ptr(out_gain), ptr(chs_out), f, h, w, cb * 32, cout)
    if TIMER.enabled:    # the two launches timed apart: the convolution is the roofline kernel (vpt_conv3x3_kernel, pool-fused mode: same FLOPs)
        _call("vpt_conv3x3_pool_forward", meta, *args, 1, _stream(), fmt=fmt, label="vpt_conv3x3_pool_forward")
        _call("vpt_conv3x3_pool_forward", dict(bytes=2.0 * y.numel() * 0.4), *args, 2, _stream(), fmt=fmt, label="vpt_pool_seam")
    else:
        _call("vpt_conv3x3_pool_forward", meta, *args, 3, _stream(), fmt=fmt)
    return y


def conv3x3_pool_argmax(x, wpk, edge_sa, edge_sg, stats_in, cout, stats_out=None):
    """conv3x3_pool() for the TRAINING forward (vpt_conv3x3_pool_argmax_forward): -> (pooled [F,cout/32,H/2,W/2,32], mask int16 of the same shape).
    mask: per pooled value the 9-bit "window position differs from the maximum" word (bit 8 - k for scan position k; outside the image: 1) --
    conv_backward_prepare_pooled() routes the pooled gradient to the first zero bit; the pre-pool tensor never exists."""
    _chk(x, OP16, "x"); _chk(wpk, OP16, "wpk"); _chk(edge_sa, torch.float32, "edge_sa"); _chk(edge_sg, torch.float32, "edge_sg")
    _chk(stats_in, torch.float64, "stats_in"); _chk(stats_out, torch.float64, "stats_out")
    f, cb, h, w, _ = x.shape
    dt, fmt = _fmt(x, wpk)
    y = torch.empty(f, cout // 32, h // 2, w // 2, 32, dtype=dt, device=x.device)
    mask = torch.empty(f, cout // 32, h // 2, w // 2, 32, dtype=torch.int16, device=x.device)
    seam = torch.empty(_native.load(fmt).vpt_conv3x3_pool_seam_elems(f, h, w, cout), dtype=dt, device=x.device)
    meta = dict(flops=2.0 * f * h * w * cout * 9 * cb * 32, bytes=2.0 * f * h * w * (cb * 32 + cout * 0.5))
    args = (ptr(x), ptr(wpk), ptr(edge_sa), ptr(edge_sg), ptr(stats_in), ptr(y), ptr(mask), ptr(seam), ptr(stats_out), f, h, w, cb * 32, cout)
    if TIMER.enabled:    # the two launches timed apart, as in conv3x3_pool()
        _call("vpt_conv3x3_pool_argmax_forward", meta, *args, 1, _stream(), fmt=fmt, label="vpt_conv3x3_pool_forward")
        _call("vpt_conv3x3_pool_argmax_forward", dict(bytes=2.0 * y.numel() * 0.8), *args, 2, _stream(), fmt=fmt, label="vpt_pool_seam")
    else:
        _call("vpt_conv3x3_pool_argmax_forward", meta, *args, 3, _stream(), fmt=fmt)
    return y, mask


def conv_backward_prepare_pooled(dpooled, pooled, mask, stats_in, edge_sa, edge_sg, cin, d_sa=None, d_sg=None, want_t12=False, nfold=None):
    """conv_backward_prepare() for the layer in front of the max-pool when its forward was conv3x3_pool_argmax(): (dpooled, pooled, mask) at the
    pooled resolution -> (dacc blocked [F,Cout/32,2h,2w,32], coef, d_sa, d_sg[, t12]) (vpt_conv_backward_prepare_pooled).
    nfold = (n_gain fp32 [Cout], pool_stats fp64 [F,2], ab fp64 [F,2] from frame_affine_backward_reduce): `dpooled` is the gradient w.r.t.
    n(pooled) and the GroupNorm `n` backward is applied on the fly (no second affine-backward pass)."""
    ng, pst, pab = nfold if nfold is not None else (None, None, None)
    _chk(ng, torch.float32, "n_gain"); _chk(pst, torch.float64, "pool_stats"); _chk(pab, torch.float64, "pool_ab")
    _chk(dpooled, OP16, "dpooled"); _chk(pooled, OP16, "pooled"); _chk(mask, torch.int16, "mask")
    _chk(stats_in, torch.float64, "stats_in"); _chk(edge_sa, torch.float32, "edge_sa"); _chk(edge_sg, torch.float32, "edge_sg")
    _chk(d_sa, torch.float32, "d_sa"); _chk(d_sg, torch.float32, "d_sg")
    if dpooled.shape != pooled.shape or mask.shape != pooled.shape:
        raise ValueError("conv_backward_prepare_pooled: dpooled, pooled and mask must have one shape")
    f, cb, ph, pw, _ = pooled.shape
    h, w = 2 * ph, 2 * pw
    dev = pooled.device
    dt, fmt = _fmt(dpooled, pooled)
    dacc = torch.empty(f, cb, h, w, 32, dtype=dt, device=dev)
    coef = torch.empty(f, 2, dtype=torch.float32, device=dev)
    t12 = torch.empty(f, 2, dtype=torch.float64, device=dev) if want_t12 else None
    if d_sa is None:
        d_sa, d_sg = torch.zeros_like(edge_sa), torch.zeros_like(edge_sg)
    scratch = _workspace(WS_CONV_BACKWARD_PREPARE, f, 0, 0, 0, cb * 32, device=dev)
    _call("vpt_conv_backward_prepare_pooled", dict(bytes=2.0 * dacc.numel() + 6.0 * pooled.numel()), ptr(dpooled), ptr(pooled), ptr(mask), ptr(stats_in), ptr(edge_sa), ptr(edge_sg),
          ptr(dacc), ptr(t12), ptr(coef), ptr(d_sa), ptr(d_sg), ptr(scratch), ptr(ng), ptr(pst), ptr(pab), f, h, w, cin, cb * 32, _stream(), fmt=fmt, label="vpt_conv_backward_prepare")
    return (dacc, coef, d_sa, d_sg, t12) if want_t12 else (dacc, coef, d_sa, d_sg)


def conv3x3_folded(x, wpk, edge_sa, edge_sg, stats_in, cout, kk_frame=None, rs_frame=None, res=None, res_scale=None, res_bias=None, stats_out=None, out=None):
    """conv3x3() with the GroupNorm `n` of the stack folded in (vpt_conv3x3_forward_folded): (kk_frame [F,9,CoutPad], rs_frame [F]) from
    nfold_coef() replace edge_sa and the statistics of x (conv0 on the gain-scaled pooled tensor Q); (res_scale [F], res_bias [F,cout])
    make the residual res_scale * res + res_bias (conv1 with res = Q)."""
    _chk(x, OP16, "x"); _chk(wpk, OP16, "wpk"); _chk(edge_sa, torch.float32, "edge_sa"); _chk(edge_sg, torch.float32, "edge_sg")
    _chk(stats_in, torch.float64, "stats_in"); _chk(kk_frame, torch.float32, "kk_frame"); _chk(rs_frame, torch.float32, "rs_frame")
    _chk(res, OP16, "res"); _chk(res_scale, torch.float32, "res_scale"); _chk(res_bias, torch.float32, "res_bias"); _chk(stats_out, torch.float64, "stats_out")
    f, cb, h, w, _ = x.shape
    dt, fmt = _fmt(x, wpk, res)
    if kk_frame is not None and tuple(kk_frame.shape) != (f, 9, edge_sg.shape[1]):
        raise ValueError(f"conv3x3_folded: kk_frame must be [F, 9, {edge_sg.shape[1]}], got {tuple(kk_frame.shape)}")
    if res_bias is not None and tuple(res_bias.shape) != (f, cout):
        raise ValueError(f"conv3x3_folded: res_bias must be [F, {cout}], got {tuple(res_bias.shape)}")
    if out is None:
        out = torch.empty(f, cout // 32, h, w, 32, dtype=dt, device=x.device)
    meta = dict(flops=2.0 * f * h * w * cout * 9 * cb * 32, bytes=2.0 * f * h * w * (cb * 32 + cout * (2 if res is not None else 1)))
    _call("vpt_conv3x3_forward_folded", meta, ptr(x), ptr(wpk), ptr(edge_sa), ptr(edge_sg), ptr(stats_in), ptr(kk_frame), ptr(rs_frame), ptr(res),
          ptr(res_scale), ptr(res_bias), ptr(out), ptr(stats_out), f, h, w, cb * 32, cout, _stream(), fmt=fmt, label="vpt_conv3x3_forward")
    return out


def channel_stats(x, out=None):
    """Blocked [F,C/32,H,W,32] -> fp64 [F, C, 2] per-frame, per-channel (sum, sum of squares) (vpt_channel_stats)."""
    _chk(x, OP16, "x"); _chk(out, torch.float64, "out")
    f, cb, h, w, _ = x.shape
    chs = out if out is not None else torch.zeros(f, cb * 32, 2, dtype=torch.float64, device=x.device)
    _call("vpt_channel_stats", dict(bytes=2.0 * x.numel()), ptr(x), ptr(chs), f, cb * 32, h * w, _stream(), fmt=_fmt(x)[1])
    return chs


def nfold_coef(tot, chs, gain, bias, sa, sg, tb, tg, hw, cout):
    """Per-frame coefficients of the folded GroupNorm `n` (vpt_nfold_coef) -> (kk_frame [F,9,CoutPad], rs_frame [F], res_scale [F], res_bias [F,C])."""
    _chk(tot, torch.float64, "tot"); _chk(chs, torch.float64, "chs")
    for t_, nme in ((gain, "gain"), (bias, "bias"), (sa, "sa"), (sg, "sg"), (tb, "tb"), (tg, "tg")):
        _chk(t_, torch.float32, nme)
    f, c, _ = chs.shape
    dev = chs.device
    kk = torch.empty(f, 9, sa.shape[1], dtype=torch.float32, device=dev)
    rs = torch.empty(f, dtype=torch.float32, device=dev)
    rsc = torch.empty(f, dtype=torch.float32, device=dev)
    rb = torch.empty(f, c, dtype=torch.float32, device=dev)
    _call("vpt_nfold_coef", dict(bytes=4.0 * kk.numel()), ptr(tot), ptr(chs), ptr(gain), ptr(bias), ptr(sa), ptr(sg), ptr(tb), ptr(tg),
          ptr(kk), ptr(rs), ptr(rsc), ptr(rb), f, c, int(hw), int(cout), _stream())
    return kk, rs, rsc, rb


def maxpool(x, stats_out=None, want_argmax=False, out=None):
    """-> pooled, or (pooled, argmax uint8) with want_argmax (training: vpt_conv_backward_prepare routes through it).
    out: pooled tensor to fill (e.g. a slice of a larger batch's)."""
    _chk(x, OP16, "x"); _chk(stats_out, torch.float64, "stats_out"); _chk(out, OP16, "out")
    f, cb, h, w, _ = x.shape
    dt, fmt = _fmt(x, out)
    if out is not None and (tuple(out.shape) != (f, cb, h // 2, w // 2, 32) or not out.is_contiguous()):
        raise ValueError("maxpool: out must be a contiguous [F, C/32, H/2, W/2, 32] tensor")
    y = out if out is not None else torch.empty(f, cb, h // 2, w // 2, 32, dtype=dt, device=x.device)
    am = torch.empty(f, cb, h // 2, w // 2, 32, dtype=torch.uint8, device=x.device) if want_argmax else None
    _call("vpt_maxpool_forward", dict(bytes=2.0 * f * cb * 32 * h * w * 1.25), ptr(x), ptr(y), ptr(stats_out), ptr(am), f, cb * 32, h, w, _stream(), fmt=fmt)
    return (y, am) if want_argmax else y


def frame_affine(x, gain, bias, stats_in, stats_out=None, per_element=False, out=None):
    _chk(x, OP16, "x"); _chk(gain, torch.float32, "gain"); _chk(bias, torch.float32, "bias")
    _chk(stats_in, torch.float64, "stats_in"); _chk(stats_out, torch.float64, "stats_out")
    f, cb, h, w, _ = x.shape
    if out is None:
        out = torch.empty_like(x)
    _call("vpt_frame_affine_forward", dict(bytes=4.0 * f * cb * 32 * h * w), ptr(x), ptr(out), ptr(gain), ptr(bias), ptr(stats_in), ptr(stats_out),
                 f, cb * 32, h * w, 1 if per_element else 0, _stream(), fmt=_fmt(x, out)[1])
    return out


def dense_fold_epilogue(part, stats, count, sg, sb):
    """Split-K partial slices [S, M, N] of x @ op16(W gain)^T + the frame statistics of x -> LayerNorm(x) @ W^T [M, N] (vpt_dense_fold_epilogue)."""
    _chk(part, torch.float32, "part"); _chk(stats, torch.float64, "stats"); _chk(sg, torch.float32, "sg"); _chk(sb, torch.float32, "sb")
    s_, m, n = part.shape
    out = torch.empty(m, n, dtype=torch.float32, device=part.device)
    _call("vpt_dense_fold_epilogue", dict(bytes=4.0 * (s_ + 1) * m * n), ptr(part), s_, ptr(stats), int(count), ptr(sg), ptr(sb), ptr(out), m, n, _stream())
    return out


_GEMM256 = os.environ.get("VPT_LINEAR_256", "0") == "1"      # A/B switch: "throughput" takes the 256 x 256 kernel (bit-identical results either way)
LINEAR_TILING = {"auto": 0, "throughput": 1, "latency": 2, "throughput256": 4}   # throughput256: vpt_gemm256_kernel where its grid fills the chip (measured neutral in the engine: not the default)


def nk_splitk(n: int, k: int) -> int:
    """The split-K factor of a mid-size-M linear as a function of the LAYER (N, K) alone: enough K slices that one row tile's N/128 column tiles
    fill the chip.  Named by the caller (`splitk="nk"`: IDMEngine, whose workload is one <= 160-frame window), never derived from M."""
    tiles = (n + 127) // 128
    if k < 2048 or tiles >= 128:
        return 1
    return max(1, min(16, k // 512, 256 // tiles))


def _every_split_has_k_steps(k: int, sk: int) -> bool:
    """vpt_gemm_kernel cuts the K / 64 steps into `sk` runs of ceil(steps / sk): when the last run is not empty every [M, N] slice of the partial buffer
    is written in full and needs no zero-fill (the dense layer: 1024 steps in 32 runs)."""
    steps = k // 64
    return sk >= 1 and (sk - 1) * ((steps + sk - 1) // sk) < steps


def linear(a_bf16, wpk, n, bias=None, res=None, relu=False, out_f32=True, out_bf16=False, splitk=1, mask=None,
           out_bf16_ld=None, splitk_raw=False, tiling="auto", out=None, partials_extra=None):
    """a [M,K] bf16 (row stride = K) x packed weight -> ([M,n] fp32 or None, [M,ld] bf16 or None).
    mask: optional bf16 [M, >=n] gate (output zeroed where mask <= 0).  out_bf16_ld: row stride of the bf16
    output (>= n, extra columns zero) so it can feed the next GEMM as an A operand with K padded to 64.
    tiling: "throughput" = the MFMA GEMM whatever M (the inference engine's batch path: a row's result must not depend on how many rows
    share the call), "latency" = the weight-streaming kernel (M <= 8: the acting step), "auto" = by M (vpt_linear_forward).
    splitk: an int (the caller's explicit factor: the dense layer), or "nk" = nk_splitk(n, k) finished by the epilogue kernel.  Under the
    named tilings ("throughput", "latency") the summation order over K is a function of (tiling, splitk, N, K) ONLY -- never of M:
    the M-based automatic split below applies to tiling="auto" alone (the BC step's small test shapes).
    out: an fp32 [M, n] buffer the unsplit product's fp32 result lands in (one slice of a partial-sum buffer).  partials_extra: linear_partials'
    exit -- the kernel and the K split are decided HERE, for both."""
    _chk(a_bf16, OP16, "A"); _chk(wpk, OP16, "wpk"); _chk(bias, torch.float32, "bias")
    _chk(res, torch.float32, "res"); _chk(mask, OP16, "mask")
    m, k = a_bf16.shape
    dev = a_bf16.device
    dt, fmt = _fmt(a_bf16, wpk, mask)
    ld16 = (out_bf16_ld or n) if out_bf16 else n
    if tiling == "throughput" and _GEMM256:
        tiling = "throughput256"
    tl = LINEAR_TILING[tiling]
    auto_sk = 1
    if splitk == "nk":
        splitk = 1
        if tl != 2:
            auto_sk = nk_splitk(n, k)
    elif splitk == 1 and tl == 0 and 8 < m <= 512 and k >= 2048:
        # tiling "auto" only.  Mid-size M: the 256 x 128 tiling alone gives N/128 workgroups for 256 CUs, so cut K as well and finish
        # with the epilogue kernel (fixed summation order: deterministic)
        tiles = ((m + 255) // 256) * ((n + 127) // 128)
        if tiles < 128:
            auto_sk = max(1, min(16, k // 512, 256 // tiles))
    if out is not None:      # the fp32 result lands in the caller's [M, n] buffer (one slice of a partial-sum buffer: DESIGN.md section 20)
        _chk(out, torch.float32, "out")
        if tuple(out.shape) != (m, n) or not out_f32 or splitk != 1 or auto_sk != 1:
            raise ValueError(f"linear(out=): an fp32 [{m}, {n}] buffer for an unsplit product with an fp32 result, got {tuple(out.shape)} (splitk {splitk}, automatic {auto_sk})")
    # the MFMA GEMM cuts K so that _every_split_has_k_steps tells whether every partial slice is written in full; the weight-streaming kernel cuts K its
    # own way (and a split without k-steps writes nothing): keep its zero-fill
    gemm = tl in (1, 4) or (tl == 0 and m > 8)
    if partials_extra is not None:      # the raw slices of this call's own kernel and split, with room for the caller's: no epilogue stage runs
        sk = max(int(splitk), auto_sk)
        part = (torch.empty if gemm and _every_split_has_k_steps(k, sk) else torch.zeros)(sk + int(partials_extra), m, n, dtype=torch.float32, device=dev)
        _call("vpt_linear_forward_tiled", dict(flops=2.0 * m * n * k, bytes=2.0 * (m * k + n * k) + 4.0 * m * n), ptr(a_bf16), ptr(wpk), None, None, ptr(part), None,
              m, n, k, k, n, n, n, 0, sk, None, 0, tl, _stream(), fmt=fmt, label="vpt_linear_forward")
        return part, sk
    partials = lambda sk: (torch.empty if gemm and _every_split_has_k_steps(k, sk) else torch.zeros)(sk, m, n, dtype=torch.float32, device=dev)
    o16 = None
    if out_bf16:
        o16 = torch.zeros(m, ld16, dtype=dt, device=dev) if ld16 > n else torch.empty(m, n, dtype=dt, device=dev)
    if auto_sk > 1:
        part = partials(auto_sk)
        _call("vpt_linear_forward_tiled", dict(flops=2.0 * m * n * k, bytes=2.0 * (m * k + n * k) + 4.0 * m * n), ptr(a_bf16), ptr(wpk), None, None, ptr(part), None,
              m, n, k, k, n, n, n, 0, auto_sk, None, 0, tl, _stream(), fmt=fmt, label="vpt_linear_forward")
        o32 = torch.empty(m, n, dtype=torch.float32, device=dev) if out_f32 else None
        _call("vpt_linear_splitk_epilogue", dict(bytes=4.0 * (auto_sk + 1) * m * n), ptr(part), auto_sk, ptr(bias), ptr(res), ptr(o32), ptr(o16),
              m, n, n, n, ld16, 1 if relu else 0, ptr(mask), mask.shape[1] if mask is not None else 0, _stream(), fmt=fmt)
        return o32, o16
    o32 = None
    if out_f32:   # split-K: one [m, n] slice per split, summed below
        o32 = partials(splitk) if splitk > 1 else (out if out is not None else torch.empty(m, n, dtype=torch.float32, device=dev))
    _call("vpt_linear_forward_tiled", dict(flops=2.0 * m * n * k, bytes=2.0 * (m * k + n * k) + 4.0 * m * n), ptr(a_bf16), ptr(wpk), ptr(bias), ptr(res), ptr(o32), ptr(o16),
          m, n, k, k, n, n, ld16, 1 if relu else 0, splitk, ptr(mask), mask.shape[1] if mask is not None else 0, tl, _stream(), fmt=fmt, label="vpt_linear_forward")
    if splitk > 1 and o32 is not None and not splitk_raw:
        o32 = o32.sum(0)           # fixed summation order: the result does not depend on scheduling
    return o32, o16                # (splitk_raw: the [splitk, M, n] partial slices, for an epilogue of the caller's)


def linear_partials(a_bf16, wpk, n, extra=1, splitk=1, tiling="auto"):
    """The raw fp32 partial slices of a [M, K] x packed weight, by the kernel and the K split ops.linear(a, wpk, n, splitk=, tiling=) takes for
    the same arguments, in a buffer with room for `extra` more slices -> (part fp32 [S + extra, M, n], S).  Slices S .. are the caller's to fill
    (ops.linear(out=part[S])); splitk_epilogue(part, ...) then sums all of them in order and applies the GEMM's epilogue.  With one extra slice
    of exact zeros the result is ops.linear's own, bit for bit: the same accumulators, 0 + acc (+ 0), the same epilogue arithmetic."""
    return linear(a_bf16, wpk, n, splitk=splitk, tiling=tiling, partials_extra=int(extra))


def splitk_epilogue(part, bias=None, res=None, relu=False, out_f32=True, out_bf16=False, mask=None, out_bf16_ld=None, dtype=torch.bfloat16):
    """part fp32 [S, M, n] -> epilogue(sum_s part[s]) (vpt_linear_splitk_epilogue): the slices summed in order from 0.f, then bias -> ReLU ->
    gate `mask` -> + res, exactly ops.linear's options and outputs ([M, n] fp32 or None, [M, ld] 16-bit or None)."""
    _chk(part, torch.float32, "part"); _chk(bias, torch.float32, "bias"); _chk(res, torch.float32, "res"); _chk(mask, OP16, "mask")
    s_, m, n = part.shape
    dt, fmt = _fmt(mask, dtype=None if mask is not None else dtype)
    ld16 = (out_bf16_ld or n) if out_bf16 else n
    o32 = torch.empty(m, n, dtype=torch.float32, device=part.device) if out_f32 else None
    o16 = None
    if out_bf16:
        o16 = torch.zeros(m, ld16, dtype=dt, device=part.device) if ld16 > n else torch.empty(m, n, dtype=dt, device=part.device)
    _call("vpt_linear_splitk_epilogue", dict(bytes=4.0 * (s_ + 1) * m * n), ptr(part), s_, ptr(bias), ptr(res), ptr(o32), ptr(o16),
          m, n, n, n, ld16, 1 if relu else 0, ptr(mask), mask.shape[1] if mask is not None else 0, _stream(), fmt=fmt)
    return o32, o16


LOWRANK_MAX_RANK = 64


def lowrank_merge(weight, a, b, s, out=None):
    """out = weight + s * (b @ a) in fp32 with the rank index ascending and no contraction (vpt_lowrank_merge): weight fp32 [n, K], a fp32 [r, K],
    b fp32 [n, r], 1 <= r <= 64; `out` may be `weight` (in place).  A float32 numpy restatement equals it bit for bit."""
    _chk(weight, torch.float32, "weight"); _chk(a, torch.float32, "a"); _chk(b, torch.float32, "b"); _chk(out, torch.float32, "out")
    n, k = weight.shape
    r = a.shape[0]
    if not 1 <= r <= LOWRANK_MAX_RANK or tuple(a.shape) != (r, k) or tuple(b.shape) != (n, r):
        raise ValueError(f"lowrank_merge: weight [{n}, {k}] needs a [r, {k}] and b [{n}, r] with 1 <= r <= {LOWRANK_MAX_RANK}, got {tuple(a.shape)} and {tuple(b.shape)}")
    if out is None:
        out = torch.empty_like(weight)
    elif tuple(out.shape) != (n, k):
        raise ValueError(f"lowrank_merge: out must be [{n}, {k}], got {tuple(out.shape)}")
    _call("vpt_lowrank_merge", dict(flops=2.0 * n * k * r, bytes=8.0 * n * k), ptr(weight), ptr(a), ptr(b), ptr(out), n, k, r, ctypes.c_float(float(s)), _stream())
    return out


def linear_wgrad(dy16, x16, n, out=None):
    """dW [n, K] fp32 = dy16[:, :n]^T @ x16 (sum over the M rows), straight from the row-major activations; added to `out` when given."""
    _chk(dy16, OP16, "dy"); _chk(x16, OP16, "x"); _chk(out, torch.float32, "out")
    m, k = x16.shape
    assert dy16.shape[0] == m and n % 8 == 0 and k % 8 == 0
    dw = out if out is not None else torch.empty(n, k, dtype=torch.float32, device=x16.device)
    _call("vpt_linear_wgrad", dict(flops=2.0 * m * n * k), ptr(dy16), ptr(x16), ptr(dw), m, n, k, dy16.shape[1], k, k, 1 if out is not None else 0, _stream(), fmt=_fmt(dy16, x16)[1])
    return dw


def layernorm(x, gain, bias, relu_in=False, out_f32=False, out_bf16=True, dtype=torch.bfloat16):
    """dtype: format of the 16-bit output (the A operand of the next GEMM)."""
    _chk(x, torch.float32, "x"); _chk(gain, torch.float32, "gain"); _chk(bias, torch.float32, "bias")
    m, d = x.shape
    o32 = torch.empty_like(x) if out_f32 else None
    dt, fmt = _fmt(dtype=dtype)
    o16 = torch.empty(m, d, dtype=dt, device=x.device) if out_bf16 else None
    _call("vpt_layernorm_forward", dict(bytes=6.0 * m * d), ptr(x), ptr(gain), ptr(bias), ptr(o32), ptr(o16), m, d, 1 if relu_in else 0, _stream(), fmt=fmt)
    return o32, o16


LN_LINEAR_MAX_ROWS, LN_LINEAR_MAX_K = 8, 3072


def layernorm_linear(x, gain, ln_bias, wpk, n, bias=None, res=None, relu=False, relu_in=False, ln_out_f32=False, out_f32=True, out_bf16=False,
                     dtype=torch.bfloat16):
    """LayerNorm (optionally of relu(x)) fused into the linear layer it feeds, for the acting path (M <= 8 rows, K <= 3072):
    (normalised rows fp32 or None, [M,n] fp32 or None, [M,n] 16-bit or None) -- bit-identical to layernorm() + linear()."""
    _chk(x, torch.float32, "x"); _chk(gain, torch.float32, "gain"); _chk(ln_bias, torch.float32, "ln_bias"); _chk(wpk, OP16, "wpk")
    _chk(bias, torch.float32, "bias"); _chk(res, torch.float32, "res")
    m, k = x.shape
    if m > LN_LINEAR_MAX_ROWS or k > LN_LINEAR_MAX_K:
        raise ValueError(f"layernorm_linear: M <= {LN_LINEAR_MAX_ROWS}, K <= {LN_LINEAR_MAX_K} (got {m} x {k}); call layernorm() and linear()")
    dt, fmt = _fmt(wpk, dtype=dtype)
    ln32 = torch.empty_like(x) if ln_out_f32 else None
    o32 = torch.empty(m, n, dtype=torch.float32, device=x.device) if out_f32 else None
    o16 = torch.empty(m, n, dtype=dt, device=x.device) if out_bf16 else None
    _call("vpt_layernorm_linear_forward", dict(flops=2.0 * m * n * k, bytes=2.0 * n * k + 4.0 * m * (n + 2 * k)), ptr(x), ptr(gain), ptr(ln_bias), 1 if relu_in else 0, ptr(ln32),
          ptr(wpk), ptr(bias), ptr(res), ptr(o32), ptr(o16), m, n, k, n, n, n, 1 if relu else 0, _stream(), fmt=fmt)
    return ln32, o32, o16


def conv3d_t5(img_u8, wfrag, bias, cout, t, stats_out=None):
    """img_u8 [F = B*t, H, W, 3] uint8 -> blocked bf16 [F, cout/32, H, W, 32] (IDM temporal conv + ReLU)."""
    _chk(img_u8, torch.uint8, "img"); _chk(wfrag, OP16, "wfrag"); _chk(bias, torch.float32, "bias")
    _chk(stats_out, torch.float64, "stats_out")
    f, h, w, _ = img_u8.shape
    dt, fmt = _fmt(wfrag)
    y = torch.empty(f, cout // 32, h, w, 32, dtype=dt, device=img_u8.device)
    _call("vpt_conv3d_t5_forward", dict(flops=2.0 * f * h * w * cout * 15, bytes=f * h * w * (3 + 2 * cout)),
          ptr(img_u8), ptr(wfrag), ptr(bias), ptr(y), ptr(stats_out), f, t, h, w, cout, _stream(), fmt=fmt)
    return y


def conv3d_t5_backward(img_u8, y, dy, t, out=None):
    """Weight and bias gradient of conv3d_t5: img_u8 [F = B*t, H, W, 3] uint8, y the forward's stored output (its ReLU gate is [y > 0]) and dy the
    gradient w.r.t. it, both blocked [F, cout/32, H, W, 32] -> (dW fp32 [cout, 3, 5, 1, 1], db fp32 [cout]); accumulated into out=(dW, db) when given.
    A tap never crosses the edge of a frame's own window of t frames.  Bit-reproducible (fixed-order sums, no atomics)."""
    _chk(img_u8, torch.uint8, "img"); _chk(y, OP16, "y"); _chk(dy, OP16, "dy")
    f, h, w, c3 = img_u8.shape
    if c3 != 3 or y.dim() != 5 or y.shape[0] != f or tuple(y.shape[2:]) != (h, w, 32) or dy.shape != y.shape:
        raise ValueError(f"conv3d_t5_backward: img {tuple(img_u8.shape)}, y {tuple(y.shape)} and dy {tuple(dy.shape)} do not belong together")
    cout = y.shape[1] * 32
    if t <= 0 or f % t or (h * w) % 256 or cout > 128:
        raise ValueError(f"conv3d_t5_backward: needs frames % t == 0, H * W % 256 == 0 and cout <= 128, got frames {f}, t {t}, {h} x {w}, cout {cout}")
    fmt = _fmt(y, dy)[1]
    if out is None:
        out = (torch.zeros(cout, 3, 5, 1, 1, dtype=torch.float32, device=y.device), torch.zeros(cout, dtype=torch.float32, device=y.device))
    dw, db = out
    _chk(dw, torch.float32, "dw"); _chk(db, torch.float32, "db")
    if dw.numel() != cout * 15 or db.numel() != cout:
        raise ValueError(f"conv3d_t5_backward: out must be ([{cout}, 3, 5, 1, 1], [{cout}]), got {tuple(dw.shape)}, {tuple(db.shape)}")
    part = _workspace(WS_CONV3D_T5_BACKWARD, f, h, w, 0, cout, device=y.device, fmt=fmt)
    _call("vpt_conv3d_t5_backward", dict(flops=2.0 * f * h * w * cout * 16, bytes=f * h * w * (15 + 4 * cout)),
          ptr(img_u8), ptr(y), ptr(dy), ptr(dw), ptr(db), ptr(part), f, t, h, w, cout, _stream(), fmt=fmt)
    return dw, db


def conv3d_t5_indexed(img_u8, src, lo, hi, wfrag, bias, cout, stats_out=None):
    """The temporal conv with indexed output frames: img_u8 [F, H, W, 3] uint8, src / lo / hi int32 [S] -> blocked [S, cout/32, H, W, 32].
    Slot j is centred on img_u8[src[j]]; tap dt reads img_u8[src[j] + dt - 2] iff lo[j] <= src[j] + dt - 2 < hi[j], zeros otherwise
    (packing.idm_feature_plan: a window's zero padding without a copy of its pixels)."""
    _chk(img_u8, torch.uint8, "img"); _chk(wfrag, OP16, "wfrag"); _chk(bias, torch.float32, "bias")
    _chk(stats_out, torch.float64, "stats_out")
    for name, t in (("src", src), ("lo", lo), ("hi", hi)):
        _chk(t, torch.int32, name)
        if t.dim() != 1 or t.numel() != src.numel():
            raise ValueError(f"conv3d_t5_indexed: {name} must be int32 [{src.numel()}], got {tuple(t.shape)}")
    f, h, w, _ = img_u8.shape
    s = src.numel()
    if stats_out is not None and stats_out.numel() != 2 * s:
        raise ValueError(f"conv3d_t5_indexed: stats_out must hold [{s}, 2] values, got {tuple(stats_out.shape)}")
    dt, fmt = _fmt(wfrag)
    y = torch.empty(s, cout // 32, h, w, 32, dtype=dt, device=img_u8.device)
    if s:
        _call("vpt_conv3d_t5_forward_indexed", dict(flops=2.0 * s * h * w * cout * 15, bytes=s * h * w * (15 + 2 * cout)),
              ptr(img_u8), ptr(src), ptr(lo), ptr(hi), ptr(wfrag), ptr(bias), ptr(y), ptr(stats_out), s, f, h, w, cout, _stream(), fmt=fmt)
    return y


def gather_rows(x, index, out=None):
    """y[i] = x[index[i]]: x fp32 [R, D] (D % 4 == 0), index int32 [n] -> fp32 [n, D]; an index outside [0, R) gives a row of zeros."""
    _chk(x, torch.float32, "x"); _chk(index, torch.int32, "index"); _chk(out, torch.float32, "out")
    if x.dim() != 2 or index.dim() != 1:
        raise ValueError("gather_rows: x must be [R, D] and index [n]")
    r, d = x.shape
    n = index.numel()
    if d % 4 or r == 0:
        raise ValueError(f"gather_rows: needs D % 4 == 0 and at least one input row, got x {tuple(x.shape)}")
    if out is None:
        out = torch.empty(n, d, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (n, d) or out.device != x.device:
        raise ValueError(f"gather_rows: out must be fp32 [{n}, {d}] on {x.device}")
    if n:
        _call("vpt_gather_rows", dict(bytes=8.0 * n * d), ptr(x), ptr(index), ptr(out), r, n, d, _stream())
    return out


def idm_decode(lp_buttons, lp_camera, maxval=10, binsize=2, mu=10, mu_law=True):
    """IDM log-probs (buttons fp32 [N, 20, 2], camera fp32 [N, 2, n_bins]) -> dict of labels, one launch: buttons int64 [N, 20], camera int64
    [N, 2] (arg-max, lowest index on ties), log_prob fp32 [N] (the 22 chosen log-probs added left to right), joint_buttons / joint_camera
    int64 [N] (action_from_factored of them), camera_deg fp64 [N, 2] (camera_undiscretize), null uint8 [N] (nothing pressed, camera centred)."""
    _chk(lp_buttons, torch.float32, "lp_buttons"); _chk(lp_camera, torch.float32, "lp_camera")
    n = lp_buttons.shape[0]
    if tuple(lp_buttons.shape) != (n, 20, 2) or lp_camera.dim() != 3 or tuple(lp_camera.shape[:2]) != (n, 2) or not lp_camera.shape[2] & 1:
        raise ValueError(f"idm_decode: expected log-probs [N, 20, 2] and [N, 2, odd n_bins], got {tuple(lp_buttons.shape)} and {tuple(lp_camera.shape)}")
    dev = lp_buttons.device
    out = dict(buttons=torch.empty(n, 20, dtype=torch.int64, device=dev), camera=torch.empty(n, 2, dtype=torch.int64, device=dev),
               log_prob=torch.empty(n, dtype=torch.float32, device=dev), joint_buttons=torch.empty(n, dtype=torch.int64, device=dev),
               joint_camera=torch.empty(n, dtype=torch.int64, device=dev), camera_deg=torch.empty(n, 2, dtype=torch.float64, device=dev),
               null=torch.empty(n, dtype=torch.uint8, device=dev))
    if n:
        _call("vpt_idm_decode", dict(bytes=float(n) * (160 + 8 * lp_camera.shape[2] + 250)), ptr(lp_buttons), ptr(lp_camera), ptr(out["buttons"]),
              ptr(out["camera"]), ptr(out["log_prob"]), ptr(out["joint_buttons"]), ptr(out["joint_camera"]), ptr(out["camera_deg"]), ptr(out["null"]),
              n, int(lp_camera.shape[2]), float(maxval), float(binsize), float(mu), int(bool(mu_law)), _stream())
    return out


def full_attention(qkv, batch, t, heads, hid, dtype=torch.bfloat16):
    """Mask "none", no memory (IDM): every query attends to all t rows of its chunk.  qkv [B*t, 3*hid] fp32."""
    _chk(qkv, torch.float32, "qkv")
    dt, fmt = _fmt(dtype=dtype)
    out = torch.empty(batch * t, hid, dtype=dt, device=qkv.device)
    _call("vpt_masked_attention_forward", dict(flops=4.0 * batch * t * t * hid), ptr(qkv), None, None, None, None, ptr(out),
          batch, t, heads, hid, qkv.shape[1], 0, 0, _stream(), fmt=fmt)
    return out


def _chk_qlo(qlo, batch, t):
    _chk(qlo, torch.int32, "qlo")
    if qlo.numel() != batch * t:
        raise ValueError(f"qlo must hold one int32 per frame ([{batch}, {t}]), got {tuple(qlo.shape)}")


def episode_bounds(first, state_mask, maxlen, want_qlo=True, want_mask=True):
    """Episode starts honoured at every frame (packing.episode_bounds on the device, vpt_episode_bounds_kernel).
    first bool/uint8 [batch, t]; state_mask bool/uint8 [batch, maxlen] (needed for the mask only).
    -> (qlo int32 [batch, t] | None, next state mask uint8 [batch, maxlen] | None)."""
    if first.dtype == torch.bool:
        first = first.view(torch.uint8)
    _chk(first, torch.uint8, "first")
    if first.dim() != 2 or first.shape[1] < 1:
        raise ValueError(f"episode_bounds: first must be [batch, t >= 1], got {tuple(first.shape)}")
    batch, t = first.shape
    qlo = mout = None
    if want_mask:
        if state_mask is None:
            raise ValueError("episode_bounds: the next mask needs state_mask")
        if state_mask.dtype == torch.bool:
            state_mask = state_mask.view(torch.uint8)
        _chk(state_mask, torch.uint8, "state_mask")
        if tuple(state_mask.shape) != (batch, maxlen):
            raise ValueError(f"episode_bounds: state_mask must be [{batch}, {maxlen}], got {tuple(state_mask.shape)}")
        mout = torch.empty_like(state_mask)
    if want_qlo:
        qlo = torch.empty(batch, t, dtype=torch.int32, device=first.device)
    if batch and (want_qlo or want_mask):
        _call("vpt_episode_bounds", dict(bytes=5.0 * batch * t + 2.0 * batch * maxlen), ptr(first), ptr(state_mask) if want_mask else None, ptr(qlo), ptr(mout),
              batch, t, int(maxlen), _stream())
    return qlo, mout


def masked_attention(qkvr, kmem, vmem, memvalid, b_nd, batch, t, heads, hid, dtype=torch.bfloat16, qlo=None):
    """qlo (int32 [batch, t], ops.episode_bounds): episode starts at any frame -- query i sees rows >= qlo[i] of [memory ; chunk] only."""
    _chk(qkvr, torch.float32, "qkvr"); _chk(kmem, torch.float32, "kmem"); _chk(vmem, torch.float32, "vmem")
    _chk(memvalid, torch.uint8, "memvalid"); _chk(b_nd, torch.float32, "b_nd")
    maxlen = kmem.shape[1]
    dt, fmt = _fmt(dtype=dtype)
    out = torch.empty(batch * t, hid, dtype=dt, device=qkvr.device)
    if qlo is not None:
        _chk_qlo(qlo, batch, t)
        _call("vpt_masked_attention_forward_episodes", dict(flops=4.0 * batch * t * (t + maxlen) * hid), ptr(qkvr), ptr(kmem), ptr(vmem), ptr(memvalid), ptr(b_nd),
              ptr(out), ptr(qlo), batch, t, heads, hid, qkvr.shape[1], maxlen, _stream(), fmt=fmt)
        return out
    _call("vpt_masked_attention_forward", dict(flops=4.0 * batch * t * (t + maxlen) * hid), ptr(qkvr), ptr(kmem), ptr(vmem), ptr(memvalid), ptr(b_nd), ptr(out),
                 batch, t, heads, hid, qkvr.shape[1], maxlen, 1, _stream(), fmt=fmt)
    return out


def kv_memory_update(qkvr, kmem, vmem, batch, t, hid):
    _chk(qkvr, torch.float32, "qkvr"); _chk(kmem, torch.float32, "kmem"); _chk(vmem, torch.float32, "vmem")
    kout, vout = torch.empty_like(kmem), torch.empty_like(vmem)
    _call("vpt_kv_memory_update", dict(bytes=16.0 * batch * kmem.shape[1] * hid), ptr(qkvr), ptr(kmem), ptr(vmem), ptr(kout), ptr(vout),
                 batch, t, hid, qkvr.shape[1], kmem.shape[1], _stream())
    return kout, vout


ATTENTION_STEP_MAXLEN = 128


def masked_attention_step(qkvr, kmem, vmem, state_mask, first, b_nd, batch, heads, hid, dtype=torch.bfloat16, inplace=False, done=None):
    """Acting step (t = 1): masked_attention(), kv_memory_update() and the state-mask bookkeeping in one launch.
    state_mask bool/uint8 [batch, maxlen], first bool/uint8 [batch] -> (out 16-bit [batch, hid], kout, vout, new mask uint8 [batch, maxlen]).
    inplace: kout / vout ARE kmem / vmem (updated in place: the captured acting graph's static state; a workgroup owns its head's
    columns and holds the rows in registers across a barrier).  The mask is a new tensor unless `done` (int32 [>= batch], zero; the
    kernel leaves it zero) is given with inplace: then the workgroup that arrives last writes it over state_mask."""
    _chk(qkvr, torch.float32, "qkvr"); _chk(kmem, torch.float32, "kmem"); _chk(vmem, torch.float32, "vmem"); _chk(b_nd, torch.float32, "b_nd")
    if state_mask.dtype == torch.bool:
        state_mask = state_mask.view(torch.uint8)
    if first.dtype == torch.bool:
        first = first.view(torch.uint8)
    _chk(state_mask, torch.uint8, "state_mask"); _chk(first, torch.uint8, "first")
    maxlen = kmem.shape[1]
    if qkvr.shape[0] != batch or maxlen > ATTENTION_STEP_MAXLEN or tuple(state_mask.shape) != (batch, maxlen) or first.numel() != batch:
        raise ValueError(f"masked_attention_step: one token per sequence, maxlen <= {ATTENTION_STEP_MAXLEN}, state_mask [batch, maxlen], first [batch] "
                         f"(got {qkvr.shape[0]} rows for batch {batch}, maxlen {maxlen}, mask {tuple(state_mask.shape)})")
    dt, fmt = _fmt(dtype=dtype)
    out = torch.empty(batch, hid, dtype=dt, device=qkvr.device)
    meta = dict(flops=4.0 * batch * maxlen * hid, bytes=16.0 * batch * maxlen * hid)
    if done is not None:
        if not inplace:
            raise ValueError("masked_attention_step: `done` is the in-place variant's counter")
        if done.dtype != torch.int32 or done.numel() < batch or not done.is_contiguous():
            raise ValueError("masked_attention_step: done must be a contiguous int32 tensor of at least `batch` zeros")
        _call("vpt_masked_attention_step_inplace", meta, ptr(qkvr), ptr(kmem), ptr(vmem), ptr(state_mask), ptr(first), ptr(b_nd), ptr(out), ptr(done),
              batch, heads, hid, qkvr.shape[1], maxlen, _stream(), fmt=fmt, label="vpt_masked_attention_step")
        return out, kmem, vmem, state_mask
    mout = torch.empty_like(state_mask)
    kout, vout = (kmem, vmem) if inplace else (torch.empty_like(kmem), torch.empty_like(vmem))
    _call("vpt_masked_attention_step", meta, ptr(qkvr), ptr(kmem), ptr(vmem), ptr(state_mask), ptr(first),
          ptr(b_nd), ptr(out), ptr(kout), ptr(vout), ptr(mout), batch, heads, hid, qkvr.shape[1], maxlen, _stream(), fmt=fmt)
    return out, kout, vout, mout


def new_rng_state(device, seed=None):
    """Device-resident state of the in-kernel generator: int64 [2] = {seed, step}.  The seed comes from torch's default CPU generator
    unless given, so torch.manual_seed() makes a run's sampled actions reproducible, as it does for the reference's th.rand_like."""
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return torch.tensor([int(seed), 0], dtype=torch.int64, device=device)


def _chk_rng(rng_state):
    if rng_state is not None and (rng_state.dtype != torch.int64 or rng_state.numel() != 2 or not rng_state.is_cuda or not rng_state.is_contiguous()):
        raise ValueError("rng_state must be a contiguous int64 [2] GPU tensor {seed, step} (ops.new_rng_state)")


def uniform_noise(rng_state, rng_stream, m, n):
    """fp32 [m, n]: exactly the uniforms log_softmax_cols(..., rng=(rng_state, rng_stream)) draws (vpt_uniform_noise); state not advanced."""
    _chk_rng(rng_state)
    out = torch.empty(m, n, dtype=torch.float32, device=rng_state.device)
    _call("vpt_uniform_noise", dict(bytes=4.0 * m * n), ptr(rng_state), ctypes.c_uint32(rng_stream), ptr(out), m, n, _stream())
    return out


def act_epilogue(action_buttons, action_camera, logp_buttons, logp_camera, logits, value_col, scale, shift, rng_state=None):
    """Tail of MinecraftAgentPolicy.act on the acting path in one launch (include/vpt_hip.h: vpt_act_epilogue) ->
    (keep int64 [M, 4], nan_flag uint8 [1]); see unpack_act_keep().  rng_state: the generator state whose step counter this launch
    advances (the stochastic heads of the step drew from it)."""
    _chk_rng(rng_state)
    _chk(action_buttons, torch.int64, "action_buttons"); _chk(action_camera, torch.int64, "action_camera")
    _chk(logp_buttons, torch.float32, "logp_buttons"); _chk(logp_camera, torch.float32, "logp_camera"); _chk(logits, torch.float32, "logits")
    m = logits.shape[0]
    if m > 64 or action_buttons.numel() != m or action_camera.numel() != m or logp_buttons.numel() != m or logp_camera.numel() != m:
        raise ValueError("act_epilogue: one action / log-prob per row of logits, at most 64 rows")
    keep = torch.empty(m, 4, dtype=torch.int64, device=logits.device)
    flag = torch.empty(1, dtype=torch.uint8, device=logits.device)
    _call("vpt_act_epilogue", dict(bytes=64.0 * m), ptr(action_buttons), ptr(action_camera), ptr(logp_buttons), ptr(logp_camera), ptr(logits),
          logits.shape[1], int(value_col), ctypes.c_float(scale), ctypes.c_float(shift), ptr(keep), ptr(flag), ptr(rng_state), m, _stream())
    return keep, flag


def unpack_act_keep(keep):
    """Views (no kernels) of act_epilogue's packed record: (buttons int64 [M], camera int64 [M], log_prob fp32 [M], vpred de-normalised
    fp32 [M], raw vpred fp32 [M])."""
    kf = keep.view(torch.float32)       # [M, 8]
    return keep[:, 0], keep[:, 1], kf[:, 4], kf[:, 6], kf[:, 7]


def log_softmax_cols(logits, col0, n, temperature, mask=None, noise=None, want_action=False, rng=None):
    """log_softmax(logits[:, col0:col0+n] / T) -> fp32 [M, n]; mask uint8 [M, n] (0 -> LOG0).  want_action: also
    CategoricalActionHead.sample + logprob in the same kernel -> (lp, action int64 [M], action_logp fp32 [M]).  Stochastic
    (Gumbel-max) when uniforms are given -- noise fp32 [M, n], or rng = (rng_state, stream id): drawn inside the kernel from the
    device-resident generator state (new_rng_state; the caller advances its step) --, deterministic arg-max otherwise."""
    _chk(logits, torch.float32, "logits"); _chk(mask, torch.uint8, "mask"); _chk(noise, torch.float32, "noise")
    rng_state, rng_stream = rng if rng is not None else (None, 0)
    _chk_rng(rng_state)
    if noise is not None and rng_state is not None:
        raise ValueError("log_softmax_cols: give noise or rng, not both")
    m = logits.shape[0]
    out = torch.empty(m, n, dtype=torch.float32, device=logits.device)
    if mask is None and not want_action:
        _call("vpt_log_softmax_forward", dict(bytes=8.0 * m * n), ptr(logits), ptr(out), m, logits.shape[1], col0, n,
              ctypes.c_float(temperature), _stream())
        return out
    action = torch.empty(m, dtype=torch.int64, device=logits.device) if want_action else None
    alp = torch.empty(m, dtype=torch.float32, device=logits.device) if want_action else None
    _call("vpt_action_head_forward", dict(bytes=8.0 * m * n), ptr(logits), ptr(mask), ptr(noise), ptr(rng_state), ctypes.c_uint32(rng_stream),
          ptr(out), ptr(action), ptr(alp), m, logits.shape[1], col0, n, ctypes.c_float(temperature), _stream())
    return (out, action, alp) if want_action else out


def adam_step_(param, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    """In-place fused Adam on flat fp32 tensors (torch.optim.Adam semantics, L2 weight decay)."""
    for t, nme in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, torch.float32, nme)
    n = param.numel()
    assert grad.numel() == n and exp_avg.numel() == n and exp_avg_sq.numel() == n
    _call("vpt_adam_step", dict(bytes=28.0 * n), ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), ctypes.c_uint64(n), int(step),
          ctypes.c_float(lr), ctypes.c_float(beta1), ctypes.c_float(beta2), ctypes.c_float(eps), ctypes.c_float(weight_decay),
          ctypes.c_float(grad_scale), _stream())


def _adam_table(grads, params=None, exp_avgs=None, exp_avg_sqs=None):
    """The device table of VptAdamTensor descriptors (include/vpt_hip.h: vpt_adam_step_multi) the multi-tensor launches share -> (table uint8
    tensor, total 1024-element blocks, total elements).  With `grads` alone the other three pointers are null (the launches that only read gradients)."""
    import numpy as np
    rec = np.zeros(len(grads), dtype=[("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<u8"), ("fb", "<i8")])
    blk = numel = 0
    for i, g in enumerate(grads):
        _chk(g, torch.float32, "grad")
        n = g.numel()
        if params is None:
            assert g.is_contiguous()
            rec[i] = (0, g.data_ptr(), 0, 0, n, blk)
        else:
            p, m, v = params[i], exp_avgs[i], exp_avg_sqs[i]
            for t, nme in ((p, "param"), (g, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
                _chk(t, torch.float32, nme)
                assert t.is_contiguous()
            assert p.numel() == n and m.numel() == n and v.numel() == n
            rec[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, blk)
        blk += (n + 1023) // 1024
        numel += n
    table = torch.from_numpy(rec.view(np.uint8)).to(grads[0].device, non_blocking=False)
    return table, blk, numel


def _grad_norm_workspace(n_t, blk, device):
    """vpt_grad_norm_multi's scratch: vpt_grad_norm_workspace_bytes(n_t, blk) bytes, 8-byte aligned (fp64 sums in front of an fp32 array whose length may
    be odd: the byte count is rounded UP to whole doubles)."""
    nbytes = int(_native.load("bf16").vpt_grad_norm_workspace_bytes(n_t, blk))
    if nbytes < 0:
        raise RuntimeError(f"vpt_grad_norm_workspace_bytes({n_t}, {blk}) failed")
    return torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.float64, device=device)


def _grad_norm_launch(table, n_t, blk, numel, scale, max_norm, norm_out, per_tensor, flag):
    """vpt_grad_norm_multi over a table already on the device (norm kernel + the two fp64 finish launches); max_norm None: the norm only."""
    ws = _grad_norm_workspace(n_t, blk, table.device)
    _call("vpt_grad_norm_multi", dict(bytes=4.0 * numel + 8.0 * blk), ptr(table), n_t, blk, ctypes.c_float(scale),
          ctypes.c_float(0.0 if max_norm is None else max_norm), ptr(ws), ptr(norm_out), ptr(per_tensor), ptr(flag), _stream())
    return ws


def grad_norm(grads, scale=1.0, max_norm=None, per_tensor=False, flag=None):
    """fp32 [4] device tensor (norm, clip coefficient, non-finite, 0) of the fp32 tensors in `grads` -- the global l2 norm of grads * scale and
    torch.nn.utils.clip_grad_norm_'s clip_coef_clamped for `max_norm` (None: 1.0, the norm only; behavioural_cloning.py:121) -- and, with
    per_tensor=True, a second fp32 [len(grads)] tensor of each tensor's own norm.  Three dependent launches (vpt_grad_norm_multi), fixed summation
    order, no host synchronisation: for callers of loss_and_grads who bring their own optimiser.  flag: optional int32 [1] device tensor, SET (never
    cleared: the caller zeroes it) when the squared sum is not finite or any gradient is inf / nan; the coefficient is then 0."""
    grads = [g if g.is_contiguous() else g.contiguous() for g in grads if g is not None]
    if not grads:
        raise ValueError("grad_norm: no gradient tensors")
    _chk(flag, torch.int32, "flag")
    table, blk, numel = _adam_table(grads)
    norm_out = torch.empty(4, dtype=torch.float32, device=grads[0].device)
    per = torch.empty(len(grads), dtype=torch.float32, device=grads[0].device) if per_tensor else None
    _grad_norm_launch(table, len(grads), blk, numel, scale, max_norm, norm_out, per, flag)
    return (norm_out, per) if per_tensor else norm_out


def adam_step_multi_(params, grads, exp_avgs, exp_avg_sqs, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0,
                     found_inf=None, max_grad_norm=None, norm_out=None, per_tensor_norms=None):
    """The Adam update of adam_step_ for a list of tensors in ONE launch (flat fp32 views; same arithmetic per element).
    found_inf: optional int32 [1] device tensor (loss-scaled fp16 step).  It is zeroed, set by vpt_grads_nonfinite_multi when any
    gradient is inf / nan, and read by the Adam launch, which then leaves every tensor untouched -- no host round trip.
    max_grad_norm (None: off, exactly the launches above): global-norm clipping of grads * grad_scale (clip_grad_norm_ + Adam.step(),
    behavioural_cloning.py:121-122).  vpt_grad_norm_multi runs over the same table -- with found_inf as its flag it REPLACES the non-finite launch --
    and the Adam launch multiplies by the coefficient it left on the device (vpt_adam_step_multi_clip); float("inf") measures and never clips.
    A non-finite norm sets found_inf (pass one: without it the update would carry the non-finite gradients on).  norm_out (fp32 [4]) and
    per_tensor_norms (fp32 [len(params)]) receive ops.grad_norm's results; pass norm_out to read them (a scratch one is used otherwise).
    Returns the table (keep it alive until the launch has been enqueued; the caller may drop it afterwards: stream-ordered free)."""
    n_t = len(params)
    if n_t == 0:
        return
    _chk(found_inf, torch.int32, "found_inf")
    table, blk, numel = _adam_table(grads, params, exp_avgs, exp_avg_sqs)
    hyper = (int(step), ctypes.c_float(lr), ctypes.c_float(beta1), ctypes.c_float(beta2), ctypes.c_float(eps), ctypes.c_float(weight_decay),
             ctypes.c_float(grad_scale), ptr(found_inf))
    if found_inf is not None:
        found_inf.zero_()
    if max_grad_norm is None:
        if found_inf is not None:
            _call("vpt_grads_nonfinite_multi", dict(bytes=4.0 * numel), ptr(table), n_t, blk, ptr(found_inf), _stream())
        _call("vpt_adam_step_multi", dict(bytes=28.0 * numel), ptr(table), n_t, blk, *hyper, _stream())
        return table   # keep alive until the launch has been enqueued (the caller may drop it afterwards: stream-ordered free)
    if norm_out is None:
        norm_out = torch.empty(4, dtype=torch.float32, device=table.device)
    _chk(norm_out, torch.float32, "norm_out")
    _chk(per_tensor_norms, torch.float32, "per_tensor_norms")
    assert norm_out.numel() >= 4 and norm_out.is_contiguous() and (per_tensor_norms is None or per_tensor_norms.numel() >= n_t)
    _grad_norm_launch(table, n_t, blk, numel, grad_scale, max_grad_norm, norm_out, per_tensor_norms, found_inf)
    _call("vpt_adam_step_multi_clip", dict(bytes=28.0 * numel), ptr(table), n_t, blk, *hyper, ptr(norm_out[1:]), _stream())
    return table   # (norm_out too outlives the enqueue: the Adam launch reads norm_out[1] on the device; a scratch one is freed in stream order)


def adam_step_groups_(params, grads, exp_avgs, exp_avg_sqs, step, lrs, weight_decays, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0,
                      decoupled=False, found_inf=None, max_grad_norm=None, norm_out=None, per_tensor_norms=None):
    """adam_step_multi_ with ONE (lr, weight_decay) PER TENSOR, still one launch (vpt_adam_step_groups): torch.optim.Adam over parameter groups,
    and with decoupled=True torch.optim.AdamW's decay, p *= 1 - lr * wd before a coupled update with weight_decay = 0.
    lrs, weight_decays: sequences of len(params) floats (rounded to fp32 as a launch argument would be); they travel as a device array next to
    the table.  A tensor whose (lr, wd) are adam_step_multi_'s launch-wide values gets that launch's bits (the step size is the same double
    expression on the fp32 lr, formed in the kernel).  found_inf / max_grad_norm / norm_out / per_tensor_norms: as adam_step_multi_, with the same
    launches in front (vpt_grads_nonfinite_multi, or vpt_grad_norm_multi which replaces it); the norm is ONE global norm over all groups.
    ValueError on a length mismatch and on tensors that are not contiguous fp32.  Returns (table, hyper array): keep them until the launch is enqueued."""
    import numpy as np
    lists = [list(params), list(grads), list(exp_avgs), list(exp_avg_sqs), list(lrs), list(weight_decays)]
    n_t = len(lists[0])
    if any(len(x) != n_t for x in lists[1:]):
        raise ValueError(f"adam_step_groups_: one entry per tensor everywhere, got lengths {[len(x) for x in lists]} "
                         "(params, grads, exp_avgs, exp_avg_sqs, lrs, weight_decays)")
    params, grads, exp_avgs, exp_avg_sqs, lrs, weight_decays = lists
    for i in range(n_t):
        for t, nme in ((params[i], "param"), (grads[i], "grad"), (exp_avgs[i], "exp_avg"), (exp_avg_sqs[i], "exp_avg_sq")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"adam_step_groups_: {nme} {i} must be a contiguous fp32 tensor")
            if t.numel() != params[i].numel():
                raise ValueError(f"adam_step_groups_: {nme} {i} has {t.numel()} elements, its parameter {params[i].numel()}")
    if n_t == 0:
        return None
    _chk(found_inf, torch.int32, "found_inf")
    table, blk, numel = _adam_table(grads, params, exp_avgs, exp_avg_sqs)
    rec = np.zeros(n_t, dtype=[("lr", "<f4"), ("wd", "<f4")])      # VptAdamGroup, record i for table entry i
    rec["lr"], rec["wd"] = np.asarray(lrs, dtype=np.float64), np.asarray(weight_decays, dtype=np.float64)
    hyper = torch.from_numpy(rec.view(np.uint8)).to(table.device, non_blocking=False)
    clip_coef = None
    if found_inf is not None:
        found_inf.zero_()
    if max_grad_norm is None:
        if found_inf is not None:
            _call("vpt_grads_nonfinite_multi", dict(bytes=4.0 * numel), ptr(table), n_t, blk, ptr(found_inf), _stream())
    else:
        if norm_out is None:
            norm_out = torch.empty(4, dtype=torch.float32, device=table.device)
        _chk(norm_out, torch.float32, "norm_out")
        _chk(per_tensor_norms, torch.float32, "per_tensor_norms")
        assert norm_out.numel() >= 4 and norm_out.is_contiguous() and (per_tensor_norms is None or per_tensor_norms.numel() >= n_t)
        _grad_norm_launch(table, n_t, blk, numel, grad_scale, max_grad_norm, norm_out, per_tensor_norms, found_inf)
        clip_coef = norm_out[1:]
    _call("vpt_adam_step_groups", dict(bytes=28.0 * numel), ptr(table), ptr(hyper), n_t, blk, int(step), ctypes.c_float(beta1), ctypes.c_float(beta2),
          ctypes.c_float(eps), ctypes.c_float(grad_scale), 1 if decoupled else 0, ptr(found_inf), ptr(clip_coef), _stream())
    return table, hyper


def grad_accumulate_(accs, grads):
    """accs[i] += grads[i] for lists of contiguous fp32 tensors in ONE launch (vpt_grad_accumulate_multi): one fp32 add per element in the table
    and block mapping of adam_step_multi_, no reductions, no atomics -- torch's `acc + g`, bit for bit.  inf / nan go through the sum.
    ValueError on a length or size mismatch and when an accumulator shares storage with its addend.  Returns the table (keep it alive until the
    launch has been enqueued; stream-ordered free afterwards)."""
    accs, grads = list(accs), list(grads)
    if len(accs) != len(grads):
        raise ValueError(f"grad_accumulate_: {len(accs)} accumulators but {len(grads)} addends")
    for i, (a, g) in enumerate(zip(accs, grads)):
        if a.numel() != g.numel():
            raise ValueError(f"grad_accumulate_: tensor {i} has {a.numel()} accumulator elements but {g.numel()} addend elements")
        if a.dtype != torch.float32 or g.dtype != torch.float32 or not a.is_contiguous() or not g.is_contiguous():
            raise ValueError(f"grad_accumulate_: tensor {i} must be contiguous fp32 on both sides")
        if a.numel() and a.data_ptr() < g.data_ptr() + 4 * g.numel() and g.data_ptr() < a.data_ptr() + 4 * a.numel():
            raise ValueError(f"grad_accumulate_: accumulator {i} shares storage with its addend (their elements overlap)")
    if not accs:
        return None
    table, blk, numel = _adam_table(grads, accs, grads, grads)      # m, v: ignored by the kernel (any fp32 tensor of the size passes the table's checks)
    _call("vpt_grad_accumulate_multi", dict(bytes=12.0 * numel), ptr(table), len(accs), blk, _stream())
    return table


def grads_nonfinite(grads):
    """int32 [1] device flag: 1 if any element of the fp32 tensors in `grads` is inf / nan (vpt_grads_nonfinite_multi, one launch; what
    torch.cuda.amp.GradScaler.unscale_ computes).  No host synchronisation here: the caller reads the flag when it needs it."""
    grads = [g if g.is_contiguous() else g.contiguous() for g in grads if g is not None and g.numel()]
    if not grads:
        raise ValueError("grads_nonfinite: no gradient tensors to check")
    flag = torch.zeros(1, dtype=torch.int32, device=grads[0].device)
    table, blk, numel = _adam_table(grads)
    _call("vpt_grads_nonfinite_multi", dict(bytes=4.0 * numel), ptr(table), len(grads), blk, ptr(flag), _stream())
    return flag


# ---- backward (behavioural-cloning step) ---------------------------------------------------------------
def nll_backward(lp_buttons, lp_camera, act_buttons, act_camera, ldz, scale, dtype=torch.bfloat16):
    """16-bit [M, ldz] gradient of the BC loss w.r.t. the fused head logits (value column and padding zero).  `scale` carries
    1 / (frames x temperature) and, in the fp16 mode, the loss scale (training.BCTrainer)."""
    _chk(lp_buttons, torch.float32, "lp_buttons"); _chk(lp_camera, torch.float32, "lp_camera")
    _chk(act_buttons, torch.int64, "act_buttons"); _chk(act_camera, torch.int64, "act_camera")
    m, nb = lp_buttons.shape
    nc = lp_camera.shape[1]
    dt, fmt = _fmt(dtype=dtype)
    dz = torch.empty(m, ldz, dtype=dt, device=lp_buttons.device)
    _call("vpt_bc_nll_backward", dict(bytes=6.0 * m * ldz), ptr(lp_buttons), ptr(lp_camera), ptr(act_buttons), ptr(act_camera),
          ptr(dz), m, nb, nc, ldz, ctypes.c_float(scale), _stream(), fmt=fmt)
    return dz


def bc_loss(lp_buttons, lp_camera, act_buttons, act_camera, ldz, scale, weight=None, dtype=torch.bfloat16, want_dz=True, want_frames=True,
            want_totals=True):
    """The weighted BC loss in one sweep over the log-probs (vpt_bc_loss) -> (dz | None, frame_out | None, totals | None).
    dz: 16-bit [M, ldz], nll_backward's values with row r at scale * weight[r] (a zero-weight row: exact zeros); frame_out fp32 [M, 8] =
    nll_b, nll_c, ent_b, ent_c, hit_b, hit_c, w, 0 per frame (unweighted); totals fp32 [8] = sum_r w frame_out[r, :6], sum w, rows with w > 0.
    weight: fp32 [M] or None (all ones).  packing.bc_loss_metrics is the host twin of frame_out / totals."""
    _chk(lp_buttons, torch.float32, "lp_buttons"); _chk(lp_camera, torch.float32, "lp_camera")
    _chk(act_buttons, torch.int64, "act_buttons"); _chk(act_camera, torch.int64, "act_camera"); _chk(weight, torch.float32, "weight")
    m, nb = lp_buttons.shape
    nc = lp_camera.shape[1]
    if lp_camera.shape[0] != m or act_buttons.numel() != m or act_camera.numel() != m or (weight is not None and weight.numel() != m):
        raise ValueError(f"bc_loss: every per-frame tensor must have {m} rows")
    dt, fmt = _fmt(dtype=dtype)
    dev = lp_buttons.device
    dz = torch.empty(m, ldz, dtype=dt, device=dev) if want_dz else None
    frame_out = torch.empty(m, 8, dtype=torch.float32, device=dev) if want_frames else None
    totals = torch.empty(8, dtype=torch.float32, device=dev) if want_totals else None
    ws = _workspace(WS_BC_LOSS, m, device=dev, fmt=fmt) if want_totals else None
    _call("vpt_bc_loss", dict(bytes=(4.0 * (nb + nc) + (2.0 * ldz if want_dz else 0.0)) * m), ptr(lp_buttons), ptr(lp_camera), ptr(act_buttons),
          ptr(act_camera), ptr(weight), ptr(dz), ptr(frame_out), ptr(totals), ptr(ws), m, nb, nc, ldz, ctypes.c_float(scale), _stream(), fmt=fmt)
    return dz, frame_out, totals


def heads_logprob_backward(lp_buttons, lp_camera, g_buttons, g_camera, g_value, ldz, temperature, mask_buttons=None, mask_camera=None,
                           dtype=torch.bfloat16, grad_scale=1.0):
    """16-bit [M, ldz] gradient w.r.t. the fused head logits for arbitrary incoming gradients of the two log-prob tensors and of the
    raw value output (any of them None = zero).  The autograd boundary of lib/policy.py uses this; the BC fast path uses nll_backward."""
    _chk(lp_buttons, torch.float32, "lp_buttons"); _chk(lp_camera, torch.float32, "lp_camera")
    _chk(g_buttons, torch.float32, "g_buttons"); _chk(g_camera, torch.float32, "g_camera"); _chk(g_value, torch.float32, "g_value")
    _chk(mask_buttons, torch.uint8, "mask_buttons"); _chk(mask_camera, torch.uint8, "mask_camera")
    m, nb = lp_buttons.shape
    nc = lp_camera.shape[1]
    dt, fmt = _fmt(dtype=dtype)
    dz = torch.empty(m, ldz, dtype=dt, device=lp_buttons.device)
    # grad_scale (fp16 loss scaling): d/dz is linear in the incoming gradients and they enter as g / temperature
    _call("vpt_heads_logprob_backward", dict(bytes=10.0 * m * ldz), ptr(lp_buttons), ptr(lp_camera), ptr(g_buttons), ptr(g_camera), ptr(g_value),
          ptr(mask_buttons), ptr(mask_camera), ptr(dz), m, nb, nc, ldz, ctypes.c_float(temperature), ctypes.c_float(grad_scale), _stream(), fmt=fmt)
    return dz


def layernorm_backward(x, gain, dy, dgain, dbias, relu_in=False, dx_add=None):
    for t, nme in ((x, "x"), (gain, "gain"), (dy, "dy"), (dgain, "dgain"), (dbias, "dbias"), (dx_add, "dx_add")):
        _chk(t, torch.float32, nme)
    m, d = x.shape
    dx = torch.empty_like(x)
    part = _workspace(WS_LAYERNORM_BACKWARD, m, d, device=x.device)
    _call("vpt_layernorm_backward", dict(bytes=20.0 * m * d), ptr(x), ptr(gain), ptr(dy), ptr(dx_add), ptr(dx), ptr(dgain), ptr(dbias), ptr(part),
          m, d, 1 if relu_in else 0, _stream())
    return dx


def gate_cast(x, ldo, mask=None, dtype=torch.bfloat16):
    """fp32 [M, N] -> 16-bit [M, ldo] (zero padded), zeroed where mask <= 0."""
    _chk(x, torch.float32, "x"); _chk(mask, OP16, "mask")
    m, n = x.shape
    dt, fmt = _fmt(mask, dtype=dtype if mask is None else None)
    out = torch.empty(m, ldo, dtype=dt, device=x.device)
    _call("vpt_gate_cast", dict(bytes=6.0 * m * ldo), ptr(x), ptr(mask), ptr(out), m, n, n, mask.shape[1] if mask is not None else 0, ldo, _stream(), fmt=fmt)
    return out


def column_sum_(out, x_bf16, n):
    _chk(x_bf16, OP16, "x"); _chk(out, torch.float32, "out")
    part = _workspace(WS_COLUMN_SUM, x_bf16.shape[0], n, device=out.device)
    _call("vpt_column_sum", dict(bytes=2.0 * x_bf16.numel()), ptr(x_bf16), ptr(out), ptr(part), x_bf16.shape[0], n, x_bf16.shape[1], _stream(), fmt=_fmt(x_bf16)[1])


def masked_attention_backward(qkvr, kmem, vmem, memvalid, b_nd, dout, db_nd, batch, t, heads, hid, qlo=None):
    for tt, nme in ((qkvr, "qkvr"), (kmem, "kmem"), (vmem, "vmem"), (b_nd, "b_nd"), (dout, "dout"), (db_nd, "db_nd")):
        _chk(tt, torch.float32, nme)
    _chk(memvalid, torch.uint8, "memvalid")
    dqkvr = torch.empty_like(qkvr) if qkvr.shape[1] == 3 * hid + 10 * heads else torch.zeros_like(qkvr)     # (every projection column is written)
    dkv = _workspace(WS_ATTENTION_BACKWARD_DKV, batch, t, hid, device=qkvr.device)
    dbnd = _workspace(WS_ATTENTION_BACKWARD_DBND, batch, t, heads, kmem.shape[1], device=qkvr.device)
    if qlo is not None:     # the forward's episode bounds (ops.episode_bounds)
        _chk_qlo(qlo, batch, t)
        _call("vpt_masked_attention_backward_episodes", dict(flops=10.0 * batch * t * (t + kmem.shape[1]) * hid), ptr(qkvr), ptr(kmem), ptr(vmem),
              ptr(memvalid), ptr(b_nd), ptr(dout), ptr(dqkvr), ptr(db_nd), ptr(dkv), ptr(dbnd), ptr(qlo), batch, t, heads, hid, qkvr.shape[1], kmem.shape[1], _stream())
        return dqkvr
    _call("vpt_masked_attention_backward", dict(flops=10.0 * batch * t * (t + kmem.shape[1]) * hid), ptr(qkvr), ptr(kmem), ptr(vmem),
          ptr(memvalid), ptr(b_nd), ptr(dout), ptr(dqkvr), ptr(db_nd), ptr(dkv), ptr(dbnd), batch, t, heads, hid, qkvr.shape[1], kmem.shape[1], _stream())
    return dqkvr


def full_attention_backward(qkv, dout, batch, t, heads, hid):
    """Backward of full_attention (mask "none", no memory): qkv fp32 [B*t, ld], dout fp32 [B*t, hid] -> dqkv fp32 [B*t, ld] (dQ | dK | dV, zeros in
    the columns >= 3 hid; every element written).  Bit-reproducible; a window's rows do not depend on the other windows of the call."""
    _chk(qkv, torch.float32, "qkv"); _chk(dout, torch.float32, "dout")
    if t > FULL_ATTENTION_MAX_T:
        raise NotImplementedError(f"the mask='none' attention backward handles windows of at most {FULL_ATTENTION_MAX_T} frames, got {t}")
    if qkv.dim() != 2 or qkv.shape[0] != batch * t or tuple(dout.shape) != (batch * t, hid):
        raise ValueError(f"full_attention_backward: qkv must be [{batch * t}, ld] and dout [{batch * t}, {hid}], got {tuple(qkv.shape)} and {tuple(dout.shape)}")
    dqkv = torch.empty_like(qkv)
    slab = _workspace(WS_FULL_ATTENTION_BACKWARD, batch, t, hid, device=qkv.device)
    _call("vpt_full_attention_backward", dict(flops=10.0 * batch * t * t * hid), ptr(qkv), ptr(dout), ptr(dqkv), ptr(slab),
          batch, t, heads, hid, qkv.shape[1], _stream())
    return dqkv


def idm_loss(lp_buttons, lp_camera, act_buttons, act_camera, scale, weight=None, dtype=torch.bfloat16, want_dz=True, want_frames=True,
             want_totals=True):
    """The IDM's weighted loss in one sweep over the two heads' log-probs (vpt_idm_loss) -> (dz | None, frame_out | None, totals | None).
    lp_buttons fp32 [M, G_b, n_b], lp_camera fp32 [M, G_c, n_c]; act_* int64 [M, G]; weight fp32 [M] or None (all ones).
    dz: 16-bit [M, round_up(G_b n_b + G_c n_c, 64)] = scale * w_r * (exp(lp) - onehot), buttons first (padding and zero-weight rows: exact zeros);
    frame_out fp32 [M, 8] = nll_b, nll_c, ent_b, ent_c (sums over the groups), hit_b, hit_c (fraction of groups), w, 0; totals fp32 [8] =
    sum_r w frame_out[r, :6], sum w, rows with w > 0.  packing.idm_loss_metrics is the host twin."""
    _chk(lp_buttons, torch.float32, "lp_buttons"); _chk(lp_camera, torch.float32, "lp_camera")
    _chk(act_buttons, torch.int64, "act_buttons"); _chk(act_camera, torch.int64, "act_camera"); _chk(weight, torch.float32, "weight")
    if lp_buttons.dim() != 3 or lp_camera.dim() != 3:
        raise ValueError("idm_loss: log-probs must be [M, groups, classes]")
    m, gb, nb = lp_buttons.shape
    gc, nc = lp_camera.shape[1:]
    if lp_camera.shape[0] != m or tuple(act_buttons.shape) != (m, gb) or tuple(act_camera.shape) != (m, gc) or (weight is not None and weight.numel() != m):
        raise ValueError(f"idm_loss: labels must be [{m}, {gb}] / [{m}, {gc}] and weight [{m}]")
    dt, fmt = _fmt(dtype=dtype)
    dev = lp_buttons.device
    ldz = (gb * nb + gc * nc + 63) // 64 * 64
    dz = torch.empty(m, ldz, dtype=dt, device=dev) if want_dz else None
    frame_out = torch.empty(m, 8, dtype=torch.float32, device=dev) if want_frames else None
    totals = torch.empty(8, dtype=torch.float32, device=dev) if want_totals else None
    ws = _workspace(WS_BC_LOSS, m, device=dev, fmt=fmt) if want_totals else None
    _call("vpt_idm_loss", dict(bytes=(8.0 * (gb * nb + gc * nc) + (2.0 * ldz if want_dz else 0.0)) * m), ptr(lp_buttons), ptr(lp_camera), ptr(act_buttons),
          ptr(act_camera), ptr(weight), ptr(dz), ptr(frame_out), ptr(totals), ptr(ws), m, gb, nb, gc, nc, ldz, ctypes.c_float(scale), _stream(), fmt=fmt)
    return dz, frame_out, totals


def grouped_logprob_backward(lp_buttons, lp_camera, g_buttons, g_camera, temperature, mask_buttons=None, mask_camera=None, dtype=torch.bfloat16,
                             grad_scale=1.0):
    """Backward of the IDM's grouped log-softmax heads for arbitrary incoming gradients (vpt_grouped_logprob_backward) -> dz, 16-bit
    [M, round_up(G_b n_b + G_c n_c, 64)] = d loss / d (the two heads' logits, [group][class], buttons first; padding: exact zeros).
    lp_buttons fp32 [M, G_b, n_b], lp_camera fp32 [M, G_c, n_c]; g_* fp32 of the same shapes = d loss / d log-prob, or None (zeros: that head's block
    of dz is zero); mask_* uint8 of the same shapes or None: the forward's availability masks (a masked element gets 0).  Per group
    dz_j = ((g_j - exp(lp_j) sum_k g_k) / temperature) * grad_scale, rounded once.  The autograd boundary of lib/policy.py:_IDMForwardFn uses this; the
    trainer's fast path is idm_loss."""
    _chk(lp_buttons, torch.float32, "lp_buttons"); _chk(lp_camera, torch.float32, "lp_camera")
    _chk(g_buttons, torch.float32, "g_buttons"); _chk(g_camera, torch.float32, "g_camera")
    _chk(mask_buttons, torch.uint8, "mask_buttons"); _chk(mask_camera, torch.uint8, "mask_camera")
    if lp_buttons.dim() != 3 or lp_camera.dim() != 3:
        raise ValueError("grouped_logprob_backward: log-probs must be [M, groups, classes]")
    m, gb, nb = lp_buttons.shape
    gc, nc = lp_camera.shape[1:]
    if lp_camera.shape[0] != m:
        raise ValueError(f"grouped_logprob_backward: lp_camera must have {m} rows")
    for t, ref, nme in ((g_buttons, lp_buttons, "g_buttons"), (mask_buttons, lp_buttons, "mask_buttons"), (g_camera, lp_camera, "g_camera"),
                        (mask_camera, lp_camera, "mask_camera")):
        if t is not None and tuple(t.shape) != tuple(ref.shape):
            raise ValueError(f"grouped_logprob_backward: {nme} must be {tuple(ref.shape)}, got {tuple(t.shape)}")
    dt, fmt = _fmt(dtype=dtype)
    ldz = (gb * nb + gc * nc + 63) // 64 * 64
    dz = torch.empty(m, ldz, dtype=dt, device=lp_buttons.device)
    _call("vpt_grouped_logprob_backward", dict(bytes=(12.0 * (gb * nb + gc * nc) + 2.0 * ldz) * m), ptr(lp_buttons), ptr(lp_camera), ptr(g_buttons),
          ptr(g_camera), ptr(mask_buttons), ptr(mask_camera), ptr(dz), m, gb, nb, gc, nc, ldz, ctypes.c_float(temperature), ctypes.c_float(grad_scale),
          _stream(), fmt=fmt)
    return dz


def rl_loss(lp_buttons, lp_camera, act_buttons, act_camera, old_log_prob, advantage, ldz, scale, *, prior_buttons=None, prior_camera=None,
            value=None, value_target=None, vnorm=None, weight=None, clip=0.2, kl_coef=0.0, entropy_coef=0.0, value_coef=0.5, temperature=1.0,
            dtype=torch.bfloat16, want_dz=True, want_frames=True, want_totals=True):
    """The fine-tuning loss in one launch (vpt_rl_loss) -> (dz | None, frame_out | None, totals | None): clipped policy gradient + kl_coef x
    KL(pi || prior) - entropy_coef x entropy + value_coef x (v - normalised target)^2, per frame, weighted mean over the frames.
    lp_* / prior_* fp32 [M, n] log-probs (the priors both or neither); act_* int64 [M]; old_log_prob, advantage fp32 [M]; value: fp32 [M] VIEW of the raw
    value output (any positive stride -- S["logits"][:, nb + nc]) with value_target fp32 [M] (denormalised) and vnorm fp32 [2] = (mean, std) on the
    device, or None (no value term); weight fp32 [M] or None (all ones).
    dz: 16-bit [M, ldz], ldz >= nb + nc + 1 (a zero-weight row: exact zeros); frame_out fp32 [M, 16] = surrogate, K_b, K_c, H_b, H_c, (v - t^)^2, rho,
    clipped, lp, old_lp - lp, w, w > 0, 0 x 4 (unweighted); totals fp32 [16] = sum_r w frame_out[r, :10], sum w, rows with w > 0, 0 x 4.  `scale`
    carries 1 / sum w (and the fp16 loss scale); the temperature is applied by the kernel.  tests/rl_loss_ref.py is the fp64 host reference."""
    for t, nme in ((lp_buttons, "lp_buttons"), (lp_camera, "lp_camera"), (prior_buttons, "prior_buttons"), (prior_camera, "prior_camera"),
                   (old_log_prob, "old_log_prob"), (advantage, "advantage"), (value_target, "value_target"), (vnorm, "vnorm"), (weight, "weight")):
        _chk(t, torch.float32, nme)
    _chk(act_buttons, torch.int64, "act_buttons"); _chk(act_camera, torch.int64, "act_camera")
    if lp_buttons.dim() != 2 or lp_camera.dim() != 2:
        raise ValueError("rl_loss: log-probs must be [M, classes]")
    m, nb = lp_buttons.shape
    nc = lp_camera.shape[1]
    per_frame = [act_buttons, act_camera, old_log_prob, advantage] + [t for t in (weight, value, value_target) if t is not None]
    if lp_camera.shape[0] != m or any(t.numel() != m for t in per_frame):
        raise ValueError(f"rl_loss: every per-frame tensor must have {m} rows")
    if (prior_buttons is None) != (prior_camera is None):
        raise ValueError("rl_loss: give both prior_buttons and prior_camera or neither")
    if prior_buttons is not None and (prior_buttons.shape != lp_buttons.shape or prior_camera.shape != lp_camera.shape):
        raise ValueError("rl_loss: the prior's log-probs must have the policy's shapes")
    stride = 0
    if value is not None:
        if not value.is_cuda or value.dtype != torch.float32 or value.dim() != 1 or (m > 1 and value.stride(0) < 1):
            raise ValueError("rl_loss: value must be a 1-D fp32 GPU tensor (or view) with a positive stride")
        if value_target is None or vnorm is None or vnorm.numel() != 2:
            raise ValueError("rl_loss: the value term needs value_target [M] and vnorm [2] = (mean, std) on the device")
        stride = value.stride(0) if m > 1 else 1
    if not temperature > 0:
        raise ValueError("rl_loss: temperature must be positive")
    dt, fmt = _fmt(dtype=dtype)
    dev = lp_buttons.device
    dz = torch.empty(m, ldz, dtype=dt, device=dev) if want_dz else None
    frame_out = torch.empty(m, 16, dtype=torch.float32, device=dev) if want_frames else None
    totals = torch.empty(16, dtype=torch.float32, device=dev) if want_totals else None
    ws = _workspace(WS_RL_LOSS, m, device=dev, fmt=fmt) if want_totals else None
    reads = (2 if want_dz else 1) * 4.0 * (nb + nc) * (2 if prior_buttons is not None else 1)
    f = ctypes.c_float
    _call("vpt_rl_loss", dict(bytes=(reads + (2.0 * ldz if want_dz else 0.0)) * m), ptr(lp_buttons), ptr(lp_camera), ptr(prior_buttons), ptr(prior_camera),
          ptr(act_buttons), ptr(act_camera), ptr(old_log_prob), ptr(advantage), ptr(value), ctypes.c_int64(stride), ptr(value_target), ptr(vnorm),
          ptr(weight), ptr(dz), ptr(frame_out), ptr(totals), ptr(ws), m, nb, nc, ldz, f(clip), f(kl_coef), f(entropy_coef), f(value_coef),
          f(temperature), f(scale), _stream(), fmt=fmt)
    return dz, frame_out, totals


def ppg_aux_loss(lp_buttons, lp_camera, old_buttons, old_camera, ldz, scale, *, value=None, value_target=None, vnorm=None, weight=None,
                 clone_coef=1.0, value_coef=0.5, temperature=1.0, dtype=torch.bfloat16, want_dz=True, want_frames=True, want_totals=True):
    """The loss of PPG's auxiliary phase in one sweep (vpt_ppg_aux_loss) -> (dz | None, frame_out | None, totals | None): clone_coef x
    KL(pi_old || pi) + value_coef x (v - normalised target)^2, per frame, weighted mean over the frames.  The KL's expectation runs over the stored
    snapshot old_* (the opposite direction of rl_loss's KL(pi || prior)).
    lp_* / old_* fp32 [M, n] log-probs (both old rows are required); value, value_target, vnorm, weight as rl_loss takes them (value = None: no value
    term).  dz: 16-bit [M, ldz], ldz >= nb + nc + 1 = clone_coef (p - o) scale w / temperature per head -- the gradient for a teacher of mass exactly
    1; the exact one is p S - o -- then 2 value_coef (v - t^) scale w, then zeros (a zero-weight row: exact zeros); frame_out fp32 [M, 8] = D_b, D_c,
    (v - t^)^2, S_b, S_c, w, w > 0, 0 (unweighted; S = sum exp(old), the teacher's mass); totals fp32 [8] = sum_r w frame_out[r, :5], sum w, rows
    with w > 0, 0.  `scale` carries 1 / sum w (and the fp16 loss scale); the temperature is applied by the kernel.  At most 65536 rows with totals.
    tests/ppg_loss_ref.py is the fp64 host reference."""
    for t, nme in ((lp_buttons, "lp_buttons"), (lp_camera, "lp_camera"), (old_buttons, "old_buttons"), (old_camera, "old_camera"),
                   (value_target, "value_target"), (vnorm, "vnorm"), (weight, "weight")):
        _chk(t, torch.float32, nme)
    if old_buttons is None or old_camera is None:
        raise ValueError("ppg_aux_loss: both old_buttons and old_camera (the snapshot's log-probs) are required")
    if lp_buttons.dim() != 2 or lp_camera.dim() != 2:
        raise ValueError("ppg_aux_loss: log-probs must be [M, classes]")
    m, nb = lp_buttons.shape
    nc = lp_camera.shape[1]
    if lp_camera.shape[0] != m or any(t.numel() != m for t in (weight, value, value_target) if t is not None):
        raise ValueError(f"ppg_aux_loss: every per-frame tensor must have {m} rows")
    if old_buttons.shape != lp_buttons.shape or old_camera.shape != lp_camera.shape:
        raise ValueError("ppg_aux_loss: the snapshot's log-probs must have the policy's shapes")
    stride = 0
    if value is not None:
        if not value.is_cuda or value.dtype != torch.float32 or value.dim() != 1 or (m > 1 and value.stride(0) < 1):
            raise ValueError("ppg_aux_loss: value must be a 1-D fp32 GPU tensor (or view) with a positive stride")
        if value_target is None or vnorm is None or vnorm.numel() != 2:
            raise ValueError("ppg_aux_loss: the value term needs value_target [M] and vnorm [2] = (mean, std) on the device")
        stride = value.stride(0) if m > 1 else 1
    if not temperature > 0:
        raise ValueError("ppg_aux_loss: temperature must be positive")
    dt, fmt = _fmt(dtype=dtype)
    dev = lp_buttons.device
    dz = torch.empty(m, ldz, dtype=dt, device=dev) if want_dz else None
    frame_out = torch.empty(m, 8, dtype=torch.float32, device=dev) if want_frames else None
    totals = torch.empty(8, dtype=torch.float32, device=dev) if want_totals else None
    ws = _workspace(WS_PPG_AUX_LOSS, m, device=dev, fmt=fmt) if want_totals else None
    f = ctypes.c_float
    _call("vpt_ppg_aux_loss", dict(bytes=(8.0 * (nb + nc) + (2.0 * ldz if want_dz else 0.0)) * m), ptr(lp_buttons), ptr(lp_camera), ptr(old_buttons),
          ptr(old_camera), ptr(value), ctypes.c_int64(stride), ptr(value_target), ptr(vnorm), ptr(weight), ptr(dz), ptr(frame_out), ptr(totals), ptr(ws),
          m, nb, nc, ldz, f(clone_coef), f(value_coef), f(temperature), f(scale), _stream(), fmt=fmt)
    return dz, frame_out, totals


def gae(reward, value, first, last_value, next_first, gamma=0.999, lam=0.95):
    """Generalised advantage estimation (vpt_gae) -> (adv, ret) fp32 [B, T].  reward, value fp32 [B, T] (value denormalised); first bool / uint8 [B, T]
    (frame t starts an episode); last_value fp32 [B], next_first bool / uint8 [B]: the frame after the rollout.  tests/gae_ref.py is the float32 host
    twin (bit for bit)."""
    _chk(reward, torch.float32, "reward"); _chk(value, torch.float32, "value"); _chk(last_value, torch.float32, "last_value")
    if reward.dim() != 2 or value.shape != reward.shape or first.shape != reward.shape:
        raise ValueError(f"gae: reward, value and first must share one [B, T] shape, got {tuple(reward.shape)}, {tuple(value.shape)}, {tuple(first.shape)}")
    b, t = reward.shape
    if last_value.numel() != b or next_first.numel() != b:
        raise ValueError(f"gae: last_value and next_first must hold {b} elements")
    first8 = (first.view(torch.uint8) if first.dtype == torch.bool else first).contiguous()
    next8 = (next_first.view(torch.uint8) if next_first.dtype == torch.bool else next_first).contiguous()
    _chk(first8, torch.uint8, "first"); _chk(next8, torch.uint8, "next_first")
    adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    _call("vpt_gae", dict(bytes=17.0 * b * t), ptr(reward), ptr(value), ptr(first8), ptr(last_value), ptr(next8), ptr(adv), ptr(ret), b, t,
          ctypes.c_float(gamma), ctypes.c_float(lam), _stream())
    return adv, ret


def _chk_strided(x, dtype, b, name):
    """A per-environment scalar input of rollout_record: `b` elements along ONE axis with a non-negative element stride (a contiguous [B] / [B, 1] tensor
    or a column view of a packed record) -> its element stride."""
    if not x.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if x.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {x.dtype}")
    if x.numel() != b:
        raise ValueError(f"{name}: expected one value per environment ({b}), got {tuple(x.shape)}")
    strides = [s for n, s in zip(x.shape, x.stride()) if n != 1]
    if len(strides) > 1 or any(s < 0 for s in strides):
        raise ValueError(f"{name}: the {b} values must lie along one axis, got shape {tuple(x.shape)} with strides {x.stride()}")
    return strides[0] if strides else 1


def rollout_record(img, first, act_buttons, act_camera, log_prob, vpred, t, img_buf, first_buf, act_buttons_buf, act_camera_buf, old_log_prob_buf,
                   vpred_buf, nan_flag):
    """One acting step of B environments into column t of the [B, T] rollout buffers, in place, one launch (vpt_rollout_record).  img uint8 [B, ...] ->
    img_buf uint8 [B, T, ...]; first bool / uint8 [B] -> first_buf (bool / uint8 [B, T]); act_buttons, act_camera int64, log_prob, vpred fp32, one value
    per environment each, contiguous or strided along one axis (the views of unpack_act_keep go in as they are) -> act_*_buf int64, old_log_prob_buf,
    vpred_buf fp32 [B, T].  nan_flag uint8 [1]: set to 1 by a NaN log-prob, never cleared here.  tests/rollout_ref.py is the numpy twin."""
    _chk(img, torch.uint8, "img"); _chk(img_buf, torch.uint8, "img_buf")
    _chk(act_buttons_buf, torch.int64, "act_buttons_buf"); _chk(act_camera_buf, torch.int64, "act_camera_buf")
    _chk(old_log_prob_buf, torch.float32, "old_log_prob_buf"); _chk(vpred_buf, torch.float32, "vpred_buf"); _chk(nan_flag, torch.uint8, "nan_flag")
    if img_buf.dim() < 3 or img.dim() != img_buf.dim() - 1:
        raise ValueError(f"rollout_record: img must be [B, ...] and img_buf [B, T, ...], got {tuple(img.shape)} and {tuple(img_buf.shape)}")
    b, t_len = img_buf.shape[:2]
    if img.shape[0] != b or img.shape[1:] != img_buf.shape[2:]:
        raise ValueError(f"rollout_record: img {tuple(img.shape)} does not hold {b} frames of img_buf {tuple(img_buf.shape)}")
    t = int(t)
    if not 0 <= t < t_len:
        raise ValueError(f"rollout_record: t = {t} is outside the horizon [0, {t_len})")
    frame_bytes = img[0].numel()
    if frame_bytes % 16 or img.data_ptr() % 16 or img_buf.data_ptr() % 16:
        raise ValueError("rollout_record: frames must be a multiple of 16 bytes and 16-byte aligned")
    first8 = first.view(torch.uint8) if first.dtype == torch.bool else first
    fbuf8 = first_buf.view(torch.uint8) if first_buf.dtype == torch.bool else first_buf
    _chk(first8, torch.uint8, "first"); _chk(fbuf8, torch.uint8, "first_buf")
    if first8.numel() != b:
        raise ValueError(f"rollout_record: first must hold {b} flags, got {tuple(first.shape)}")
    for x, name in ((fbuf8, "first_buf"), (act_buttons_buf, "act_buttons_buf"), (act_camera_buf, "act_camera_buf"), (old_log_prob_buf, "old_log_prob_buf"),
                    (vpred_buf, "vpred_buf")):
        if tuple(x.shape) != (b, t_len):
            raise ValueError(f"rollout_record: {name} must be [{b}, {t_len}], got {tuple(x.shape)}")
    if nan_flag.numel() != 1:
        raise ValueError("rollout_record: nan_flag must hold one byte")
    sb, sc = _chk_strided(act_buttons, torch.int64, b, "act_buttons"), _chk_strided(act_camera, torch.int64, b, "act_camera")
    sl, sv = _chk_strided(log_prob, torch.float32, b, "log_prob"), _chk_strided(vpred, torch.float32, b, "vpred")
    i64 = ctypes.c_int64
    _call("vpt_rollout_record", dict(bytes=2.0 * b * frame_bytes), ptr(img), ptr(first8), ptr(act_buttons), ptr(act_camera), ptr(log_prob), ptr(vpred),
          i64(sb), i64(sc), i64(sl), i64(sv), ptr(img_buf), ptr(fbuf8), ptr(act_buttons_buf), ptr(act_camera_buf), ptr(old_log_prob_buf), ptr(vpred_buf),
          ptr(nan_flag), b, t_len, t, i64(frame_bytes), _stream())


def rollout_reward(reward, done, t, reward_buf, done_return, done_length, ep_return, ep_length):
    """The environment's answer to step t into column t, in place, one launch (vpt_rollout_reward).  reward fp32 [B]; done bool / uint8 [B]: the NEXT frame
    starts an episode; reward_buf, done_return fp32 [B, T], done_length int32 [B, T]; ep_return fp32 [B], ep_length int32 [B]: the running totals of the
    episodes in progress, advanced here and reset where done.  tests/rollout_ref.py is the float32 numpy twin (bit for bit)."""
    _chk(reward, torch.float32, "reward"); _chk(reward_buf, torch.float32, "reward_buf"); _chk(done_return, torch.float32, "done_return")
    _chk(done_length, torch.int32, "done_length"); _chk(ep_return, torch.float32, "ep_return"); _chk(ep_length, torch.int32, "ep_length")
    if reward_buf.dim() != 2 or done_return.shape != reward_buf.shape or done_length.shape != reward_buf.shape:
        raise ValueError(f"rollout_reward: reward_buf, done_return and done_length must share one [B, T] shape, got {tuple(reward_buf.shape)}, "
                         f"{tuple(done_return.shape)}, {tuple(done_length.shape)}")
    b, t_len = reward_buf.shape
    t = int(t)
    if not 0 <= t < t_len:
        raise ValueError(f"rollout_reward: t = {t} is outside the horizon [0, {t_len})")
    done8 = done.view(torch.uint8) if done.dtype == torch.bool else done
    _chk(done8, torch.uint8, "done")
    if reward.numel() != b or done8.numel() != b or ep_return.numel() != b or ep_length.numel() != b:
        raise ValueError(f"rollout_reward: reward, done, ep_return and ep_length must hold {b} elements")
    _call("vpt_rollout_reward", dict(bytes=22.0 * b), ptr(reward), ptr(done8), ptr(reward_buf), ptr(done_return), ptr(done_length), ptr(ep_return),
          ptr(ep_length), b, t_len, t, _stream())


def conv_backward_prepare(dy, y, res, stats_in, edge_sa, edge_sg, cin, dpooled=None, argmax=None, d_sa=None, d_sg=None, want_t12=False):
    """-> (dacc bf16 blocked, coef fp32 [F,2], d_sa fp32 [9,CoutPad], d_sg fp32 [9,CoutPad][, t12 double [F,2]]).
    coef = (c0, c1) of the statistics terms conv3x3_dgrad adds (dx += c0 + c1 x).  d_sa / d_sg are accumulated into when
    given.  dy=None with (dpooled, argmax): the layer feeds a max-pool whose backward is applied on the fly."""
    for t, nme in ((dy, "dy"), (y, "y"), (res, "res"), (dpooled, "dpooled")):
        _chk(t, OP16, nme)
    _chk(argmax, torch.uint8, "argmax")
    _chk(stats_in, torch.float64, "stats_in"); _chk(edge_sa, torch.float32, "edge_sa"); _chk(edge_sg, torch.float32, "edge_sg")
    _chk(d_sa, torch.float32, "d_sa"); _chk(d_sg, torch.float32, "d_sg")
    if (dy is None) == (dpooled is None or argmax is None):
        raise ValueError("conv_backward_prepare: give either dy or (dpooled, argmax)")
    f, cb, h, w, _ = y.shape
    dev = y.device
    dacc = torch.empty_like(y)
    coef = torch.empty(f, 2, dtype=torch.float32, device=dev)
    t12 = torch.empty(f, 2, dtype=torch.float64, device=dev) if want_t12 else None
    if d_sa is None:
        d_sa, d_sg = torch.zeros_like(edge_sa), torch.zeros_like(edge_sg)
    scratch = _workspace(WS_CONV_BACKWARD_PREPARE, f, 0, 0, 0, cb * 32, device=dev)
    _call("vpt_conv_backward_prepare", dict(bytes=(6.0 if dy is not None else 4.75) * y.numel() + (2.0 * y.numel() if res is not None else 0)),
          ptr(dy), ptr(dpooled), ptr(argmax), ptr(y), ptr(res), ptr(stats_in), ptr(edge_sa), ptr(edge_sg),
          ptr(dacc), ptr(t12), ptr(coef), ptr(d_sa), ptr(d_sg), ptr(scratch), f, h, w, cin, cb * 32, _stream(), fmt=_fmt(dy, y, res, dpooled)[1])
    return (dacc, coef, d_sa, d_sg, t12) if want_t12 else (dacc, coef, d_sa, d_sg)


def conv3x3_dgrad(dacc, wpk_t, cin, skip=None, xin=None, coef=None):
    """dacc blocked [F,Cout/32,H,W,32] -> dx blocked [F,cin/32,H,W,32] (transposed conv + skip + c0 + c1*xin)."""
    _chk(dacc, OP16, "dacc"); _chk(wpk_t, OP16, "wpk_t"); _chk(skip, OP16, "skip")
    _chk(xin, OP16, "xin"); _chk(coef, torch.float32, "coef")
    f, cb, h, w, _ = dacc.shape
    dt, fmt = _fmt(dacc, wpk_t, skip, xin)
    dx = torch.empty(f, cin // 32, h, w, 32, dtype=dt, device=dacc.device)
    _call("vpt_conv3x3_dgrad", dict(flops=2.0 * f * h * w * cin * 9 * cb * 32), ptr(dacc), ptr(wpk_t), ptr(skip), ptr(xin), ptr(coef), ptr(dx),
          f, h, w, cb * 32, cin, _stream(), fmt=fmt)
    return dx


def conv3x3_dgrad_gated(dacc, wpk_t, cin, xin, coef, gate_stats, gate_cin):
    """A block's conv1 -> conv0 backward in one epilogue (vpt_conv3x3_dgrad_gated): the transposed convolution of `dacc` (conv1's operand) whose
    output is conv0's OPERAND  rstd0 * (conv^T + c0 + c1 xin) * [xin > 0]  (xin = conv0's output, gate_stats = the frame statistics of conv0's
    input over gate_cin * H * W elements) instead of the plain gradient.  -> (dacc0 blocked [F, cin/32, H, W, 32], gate_u fp64 [F])."""
    _chk(dacc, OP16, "dacc"); _chk(wpk_t, OP16, "wpk_t"); _chk(xin, OP16, "xin"); _chk(coef, torch.float32, "coef"); _chk(gate_stats, torch.float64, "gate_stats")
    f, cb, h, w, _ = dacc.shape
    dt, fmt = _fmt(dacc, wpk_t, xin)
    out = torch.empty(f, cin // 32, h, w, 32, dtype=dt, device=dacc.device)
    gate_u = torch.zeros(f, dtype=torch.float64, device=dacc.device)
    _call("vpt_conv3x3_dgrad_gated", dict(flops=2.0 * f * h * w * cin * 9 * cb * 32), ptr(dacc), ptr(wpk_t), ptr(xin), ptr(coef), ptr(gate_stats), int(gate_cin),
          ptr(out), ptr(gate_u), f, h, w, cb * 32, cin, _stream(), fmt=fmt, label="vpt_conv3x3_dgrad")
    return out, gate_u


def conv_backward_reduce(dacc, gate_u, stats_in, edge_sa, edge_sg, cin, d_sa=None, d_sg=None, want_t12=False):
    """What conv_backward_prepare returns besides dacc, for an operand that conv3x3_dgrad_gated already wrote: (coef fp32 [F,2], d_sa, d_sg[, t12])
    from one read of dacc (vpt_conv_backward_reduce).  stats_in: the layer's input statistics (cin * H * W elements)."""
    _chk(dacc, OP16, "dacc"); _chk(gate_u, torch.float64, "gate_u"); _chk(stats_in, torch.float64, "stats_in")
    _chk(edge_sa, torch.float32, "edge_sa"); _chk(edge_sg, torch.float32, "edge_sg"); _chk(d_sa, torch.float32, "d_sa"); _chk(d_sg, torch.float32, "d_sg")
    f, cb, h, w, _ = dacc.shape
    dev = dacc.device
    coef = torch.empty(f, 2, dtype=torch.float32, device=dev)
    t12 = torch.empty(f, 2, dtype=torch.float64, device=dev) if want_t12 else None
    if d_sa is None:
        d_sa, d_sg = torch.zeros_like(edge_sa), torch.zeros_like(edge_sg)
    scratch = _workspace(WS_CONV_BACKWARD_PREPARE, f, 0, 0, 0, cb * 32, device=dev)
    _call("vpt_conv_backward_reduce", dict(bytes=2.0 * dacc.numel()), ptr(dacc), ptr(gate_u), ptr(stats_in), ptr(edge_sa), ptr(edge_sg),
          ptr(t12), ptr(coef), ptr(d_sa), ptr(d_sg), ptr(scratch), f, h, w, cin, cb * 32, _stream(), fmt=_fmt(dacc)[1], label="vpt_conv_backward_prepare")
    return (coef, d_sa, d_sg, t12) if want_t12 else (coef, d_sa, d_sg)


def maxpool_backward(pre, pooled, dpooled):
    for t, nme in ((pre, "pre"), (pooled, "pooled"), (dpooled, "dpooled")):
        _chk(t, OP16, nme)
    f, cb, h, w, _ = pre.shape
    dpre = torch.empty_like(pre)
    _call("vpt_maxpool_backward", dict(bytes=5.0 * pre.numel()), ptr(pre), ptr(pooled), ptr(dpooled), ptr(dpre), f, cb * 32, h, w, _stream(), fmt=_fmt(pre, pooled, dpooled)[1])
    return dpre


def frame_affine_backward_reduce(x, dy, gain, stats_in, dgain, dbias):
    """Pass 1 of frame_affine_backward alone (per-channel gain): dgain / dbias accumulated in place, returns ab fp64 [F,2] = (sum dy g, sum dy g xhat)
    for a consumer that applies dx = rstd (dy g - ab0/n - xhat ab1/n) itself (conv_backward_prepare_pooled(nfold=...))."""
    _chk(x, OP16, "x"); _chk(dy, OP16, "dy"); _chk(gain, torch.float32, "gain"); _chk(stats_in, torch.float64, "stats_in")
    _chk(dgain, torch.float32, "dgain"); _chk(dbias, torch.float32, "dbias")
    f, cb, h, w, _ = x.shape
    ab = torch.zeros(f, 2, dtype=torch.float64, device=x.device)
    part = _workspace(WS_FRAME_AFFINE_BACKWARD, f, h * w, 0, 1, cb * 32, device=x.device)
    _call("vpt_frame_affine_backward", dict(bytes=4.0 * x.numel()), ptr(x), ptr(dy), None, None, ptr(gain), ptr(stats_in), ptr(ab), ptr(dgain), ptr(dbias), ptr(part),
          f, cb * 32, h * w, 0, 1, _stream(), fmt=_fmt(x, dy)[1])
    return ab


def frame_affine_backward(x, dy, gain, stats_in, dgain, dbias, per_element=False, dx_add=None):
    """Backward of frame_affine: returns dx (bf16 blocked); dgain / dbias accumulated in place."""
    _chk(x, OP16, "x"); _chk(dy, OP16, "dy"); _chk(dx_add, OP16, "dx_add")
    _chk(gain, torch.float32, "gain"); _chk(stats_in, torch.float64, "stats_in"); _chk(dgain, torch.float32, "dgain"); _chk(dbias, torch.float32, "dbias")
    f, cb, h, w, _ = x.shape
    ab = torch.zeros(f, 2, dtype=torch.float64, device=x.device)
    dx = torch.empty_like(x)
    pe = 1 if per_element else 0
    head = (ptr(x), ptr(dy), ptr(dx_add), ptr(dx), ptr(gain), ptr(stats_in), ptr(ab), ptr(dgain), ptr(dbias))
    tail = (f, cb * 32, h * w, pe)
    fmt = _fmt(x, dy, dx_add)[1]
    part1 = _workspace(WS_FRAME_AFFINE_BACKWARD, f, h * w, pe, 1, cb * 32, device=x.device)      # (None for the per-element variant: pass 3 reduces)
    _call("vpt_frame_affine_backward", dict(bytes=4.0 * x.numel()), *head, ptr(part1), *tail, 1, _stream(), fmt=fmt)
    _call("vpt_frame_affine_backward", dict(bytes=6.0 * x.numel()), *head, None, *tail, 2, _stream(), fmt=fmt)
    if per_element:
        part3 = _workspace(WS_FRAME_AFFINE_BACKWARD, f, h * w, pe, 3, cb * 32, device=x.device)
        _call("vpt_frame_affine_backward", dict(bytes=4.0 * x.numel()), *head, ptr(part3), *tail, 3, _stream(), fmt=fmt)
    return dx


def conv3x3_wgrad(dacc, x, out=None):
    """-> fp32 [Cout, 9, Cin]: sum over frames and pixels of dacc (x) shifted x (added to `out` when given)."""
    _chk(dacc, OP16, "dacc"); _chk(x, OP16, "x"); _chk(out, torch.float32, "out")
    f, cbo, h, w, _ = dacc.shape
    cbi = x.shape[1]
    dw = out if out is not None else torch.zeros(cbo * 32, 9, cbi * 32, dtype=torch.float32, device=x.device)
    fmt = _fmt(dacc, x)[1]
    scratch = torch.empty(_native.load(fmt).vpt_conv3x3_wgrad_scratch_floats(f, cbi * 32, cbo * 32), dtype=torch.float32, device=x.device)
    _call("vpt_conv3x3_wgrad", dict(flops=2.0 * f * h * w * cbo * 32 * 9 * cbi * 32), ptr(dacc), ptr(x), ptr(dw), ptr(scratch), f, h, w, cbi * 32, cbo * 32, _stream(), fmt=fmt)
    return dw


def conv_first_backward(img_u8, wfrag, dpooled, cout, out=None, nfold=None):
    """-> (dW fp32 [cout, 27] in (kh, kw, ch) tap order, db fp32 [cout]); accumulated into out=(dW, db) when given.
    conv_first_grad_to_reference() maps dW to the reference's [cout, 3, 3, 3] (o, ch, kh, kw).
    nfold = (n_gain fp32 [cout], pool_stats fp64 [F,2], ab fp64 [F,2] from frame_affine_backward_reduce): `dpooled` is the gradient w.r.t. n(pooled) and the
    GroupNorm `n` backward is applied on the fly (vpt_conv_first_backward_nfold: no second affine-backward pass over stack 0)."""
    _chk(img_u8, torch.uint8, "img"); _chk(wfrag, OP16, "wfrag"); _chk(dpooled, OP16, "dpooled")
    f, h, w, _ = img_u8.shape
    if out is None:
        out = (torch.zeros(cout, 27, dtype=torch.float32, device=img_u8.device), torch.zeros(cout, dtype=torch.float32, device=img_u8.device))
    dw, db = out
    _chk(dw, torch.float32, "dw"); _chk(db, torch.float32, "db")
    part = _workspace(WS_CONV_FIRST_BACKWARD, f, h, w, 0, cout, device=img_u8.device)
    if nfold is not None:
        ng, pst, pab = nfold
        _chk(ng, torch.float32, "n_gain"); _chk(pst, torch.float64, "pool_stats"); _chk(pab, torch.float64, "pool_ab")
        _call("vpt_conv_first_backward_nfold", dict(flops=2.0 * f * (h // 2) * (w // 2) * cout * 27), ptr(img_u8), ptr(wfrag), ptr(dpooled), ptr(ng), ptr(pst), ptr(pab),
              ptr(dw), ptr(db), ptr(part), f, h, w, cout, _stream(), fmt=_fmt(wfrag, dpooled)[1], label="vpt_conv_first_backward")
        return dw, db
    _call("vpt_conv_first_backward", dict(flops=2.0 * f * (h // 2) * (w // 2) * cout * 27), ptr(img_u8), ptr(wfrag), ptr(dpooled), ptr(dw), ptr(db), ptr(part),
          f, h, w, cout, _stream(), fmt=_fmt(wfrag, dpooled)[1])
    return dw, db


def conv_first_grad_to_reference(dw):
    cout = dw.shape[0]
    return dw.view(cout, 3, 3, 3).permute(0, 3, 1, 2).contiguous()


# ---- action codec (lib/actions.py, lib/action_mapping.py on the device) ----------------------------------------
def camera_discretize(xy, maxval, binsize, mu, mu_law):
    """fp64 tensor (any shape) -> int64 bins of the same shape."""
    _chk(xy, torch.float64, "xy")
    out = torch.empty(xy.shape, dtype=torch.int64, device=xy.device)
    if xy.numel():
        _call("vpt_camera_discretize", dict(bytes=16.0 * xy.numel()), ptr(xy), ptr(out), xy.numel(), float(maxval), float(binsize), float(mu), int(bool(mu_law)), _stream())
    return out


def camera_undiscretize(bins, maxval, binsize, mu, mu_law):
    """int64 bins -> fp64 camera angles."""
    _chk(bins, torch.int64, "bins")
    out = torch.empty(bins.shape, dtype=torch.float64, device=bins.device)
    if bins.numel():
        _call("vpt_camera_undiscretize", dict(bytes=16.0 * bins.numel()), ptr(bins), ptr(out), bins.numel(), float(maxval), float(binsize), float(mu), int(bool(mu_law)), _stream())
    return out


def action_from_factored(buttons, camera, n_camera_bins=11):
    """buttons int64 [N,20], camera int64 [N,2] -> (joint buttons int64 [N], joint camera int64 [N])."""
    _chk(buttons, torch.int64, "buttons"); _chk(camera, torch.int64, "camera")
    n = buttons.shape[0]
    jb = torch.empty(n, dtype=torch.int64, device=buttons.device)
    jc = torch.empty(n, dtype=torch.int64, device=buttons.device)
    if n:
        # camera bins outside 0..n_bins-1 are a KeyError in the reference's table lookup (buttons are truthy flags there: any value)
        if int(camera.min()) < 0 or int(camera.max()) >= n_camera_bins:
            raise IndexError(f"factored action out of range: camera bins must lie in 0..{n_camera_bins - 1}")
        _call("vpt_action_from_factored", dict(bytes=192.0 * n), ptr(buttons), ptr(camera), ptr(jb), ptr(jc), n, int(n_camera_bins), _stream())
    return jb, jc


def action_to_factored(joint_buttons, joint_camera, n_camera_bins=11):
    """joint indices int64 [N] -> (buttons int64 [N,20], camera int64 [N,2])."""
    _chk(joint_buttons, torch.int64, "joint_buttons"); _chk(joint_camera, torch.int64, "joint_camera")
    n = joint_buttons.shape[0]
    b = torch.empty(n, 20, dtype=torch.int64, device=joint_buttons.device)
    c = torch.empty(n, 2, dtype=torch.int64, device=joint_buttons.device)
    if n:
        # the kernel decodes blindly; the reference raises IndexError / KeyError on indices outside its tables
        lo_b, hi_b = int(joint_buttons.min()), int(joint_buttons.max())
        lo_c, hi_c = int(joint_camera.min()), int(joint_camera.max())
        if lo_b < 0 or hi_b > 8640 or lo_c < 0 or hi_c >= n_camera_bins * n_camera_bins:
            raise IndexError(f"joint action index out of range: buttons [{lo_b}, {hi_b}] (0..8640), camera [{lo_c}, {hi_c}] (0..{n_camera_bins * n_camera_bins - 1})")
        _call("vpt_action_to_factored", dict(bytes=192.0 * n), ptr(joint_buttons), ptr(joint_camera), ptr(b), ptr(c), n, int(n_camera_bins), _stream())
    return b, c


# ---- clip data path (data_loader.py:113-122 on the device) --------------------------------------------------------
def clip_frames(frames_bgr, cursor_state=None, cursor_bgr=None, cursor_alpha=None, out_hw=(128, 128), out=None):
    """uint8 BGR [F,H,W,3] (+ int32 [F,3] (gui open, x, y), uint8 cursor [h,w,3] BGR, fp64 alpha [h,w]) -> uint8 RGB [F,oh,ow,3]:
    cursor compositing, BGR->RGB and the cv2.INTER_LINEAR resize in one launch.  The compositing is bit-identical to the live
    reference's function (golden vectors); the resize restates OpenCV's 8-bit fixed-point algorithm and is bit-identical to
    oracle/clip_oracle.py, which is NOT pinned against real cv2 (absent from this image)."""
    _chk(frames_bgr, torch.uint8, "frames_bgr")
    if frames_bgr.dim() != 4 or frames_bgr.shape[3] != 3:
        raise ValueError("frames_bgr must be [F, H, W, 3]")
    f, h, w, _ = frames_bgr.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if out is None:
        out = torch.empty(f, oh, ow, 3, dtype=torch.uint8, device=frames_bgr.device)
    else:
        _chk(out, torch.uint8, "out")
        if tuple(out.shape) != (f, oh, ow, 3) or out.device != frames_bgr.device:
            raise ValueError(f"clip_frames: out must be uint8 [{f}, {oh}, {ow}, 3] on {frames_bgr.device}, got {tuple(out.shape)} on {out.device}")
    ch = cw = 0
    if cursor_state is not None:
        if cursor_bgr is None or cursor_alpha is None:
            raise ValueError("cursor_state needs cursor_bgr and cursor_alpha")
        _chk(cursor_state, torch.int32, "cursor_state"); _chk(cursor_bgr, torch.uint8, "cursor_bgr"); _chk(cursor_alpha, torch.float64, "cursor_alpha")
        if tuple(cursor_state.shape) != (f, 3) or cursor_bgr.dim() != 3 or cursor_bgr.shape[2] != 3 or tuple(cursor_alpha.shape) != tuple(cursor_bgr.shape[:2]):
            raise ValueError("cursor_state must be [F, 3], cursor_bgr [h, w, 3], cursor_alpha [h, w]")
        ch, cw = int(cursor_bgr.shape[0]), int(cursor_bgr.shape[1])
    if f:
        _call("vpt_clip_frames", dict(bytes=float(f) * (h * w * 3 + oh * ow * 3)), ptr(frames_bgr), f, h, w, ptr(cursor_state), ptr(cursor_bgr), ptr(cursor_alpha),
              ch, cw, ptr(out), oh, ow, _stream())
    return out


AUGMENT_MAX_FRAME_BYTES = 65536      # vpt_augment_frames stages a frame whole in LDS (csrc/vpt_augment_pixel.h: VPT_AUG_MAX_FRAME_BYTES)


def augment_uniforms(keys, seed, epoch, fmt="bf16"):
    """int64 keys [...] -> fp32 [keys.numel(), 9]: the nine uniforms in [0, 1) of every frame (vpt_augment_uniforms): Philox4x32-10, key = seed, counter =
    (draw >> 2, key lo, key hi, epoch).  A pure function of (seed, epoch, key): equal keys give equal rows in whichever call they appear."""
    _chk(keys, torch.int64, "keys")
    n = keys.numel()
    out = torch.empty(n, 9, dtype=torch.float32, device=keys.device)
    if n:
        _call("vpt_augment_uniforms", dict(bytes=44.0 * n), ptr(keys), ptr(out), n, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
              ctypes.c_uint32(int(epoch) & 0xFFFFFFFF), _stream(), fmt=fmt)
    return out


def augment_frames(img, tables, out=None, fmt="bf16"):
    """uint8 frames [F,H,W,3] or [B,T,H,W,3] under fp32 tables [F,16] (colour matrix 3x3 row-major, mean gain, inverse affine map 2x3: include/vpt_hip.h)
    -> uint8 frames of the same shape, one launch (vpt_augment_frames).  Fixed fp32 arithmetic: tests/augment_ref.py restates it bit for bit.
    H * W * 3 <= 65536 (a frame is staged in LDS).  `out` may be `img` itself (in place); any other overlap is not supported."""
    _chk(img, torch.uint8, "img"); _chk(tables, torch.float32, "tables")
    if img.dim() not in (4, 5) or img.shape[-1] != 3:
        raise ValueError("img must be [F, H, W, 3] or [B, T, H, W, 3]")
    h, w = int(img.shape[-3]), int(img.shape[-2])
    f = img.numel() // (h * w * 3) if h * w else 0
    if h < 1 or w < 1:
        raise ValueError("augment_frames: empty frames")
    if h * w * 3 > AUGMENT_MAX_FRAME_BYTES:
        raise ValueError(f"augment_frames: a frame of {h} x {w} x 3 bytes does not fit the LDS staging (H * W * 3 <= {AUGMENT_MAX_FRAME_BYTES})")
    if tuple(tables.shape) != (f, 16) or tables.device != img.device:
        raise ValueError(f"augment_frames: tables must be fp32 [{f}, 16] on {img.device}, got {tuple(tables.shape)} on {tables.device}")
    if out is None:
        out = torch.empty_like(img)
    else:
        _chk(out, torch.uint8, "out")
        if tuple(out.shape) != tuple(img.shape) or out.device != img.device:
            raise ValueError(f"augment_frames: out must be uint8 {tuple(img.shape)} on {img.device}, got {tuple(out.shape)} on {out.device}")
    if f:
        _call("vpt_augment_frames", dict(bytes=float(f) * (2 * h * w * 3 + 64)), ptr(img), ptr(tables), ptr(out), f, h, w, _stream(), fmt=fmt)
    return out
