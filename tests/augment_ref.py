"""Restatement of the frame augmentation  --  TEST INFRASTRUCTURE.

  * augment_frames_ref: the per-pixel arithmetic of csrc/vpt_augment_pixel.h in float32 numpy, element-wise.  numpy never fuses a multiply into an add and
    np.rint rounds half to even, so this equals the kernel (built with fp contraction off) bit for bit.
  * tables_ref: the tables from the parameters, literally as the formulas are written, in float64 (numpy.linalg.inv for Y^-1 and A^-1).
  * uniforms_ref: the nine uniforms per key via oracle.philox.philox4x32_10 with the kernel's counter layout.
  * grid_sample_route: an INDEPENDENT float64 route through torch.nn.functional.grid_sample (zeros padding, align_corners=False) plus the colour map, for
    the CPU test that keeps the restatement itself honest."""
import math

import numpy as np

from oracle.philox import philox4x32_10

YIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]], dtype=np.float64)
LUMA = np.array([77.0, 150.0, 29.0], dtype=np.float64) / 256.0
IDENTITY_PARAMS = np.array([0.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0], dtype=np.float64)
IDENTITY_TABLE = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0], dtype=np.float32)
DEFAULT_RANGES = ((-0.02, 0.02), (0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-2.0, 2.0), (0.98, 1.02), (-2.0, 2.0), (-2.0, 2.0), (-2.0, 2.0))


def uniforms_ref(keys, seed: int, epoch: int) -> np.ndarray:
    """int64 keys [F] -> fp32 [F, 9]: key (seed lo, seed hi), counter (draw >> 2, key lo, key hi, epoch), word draw & 3, u = (word >> 8) * 2^-24."""
    k = np.asarray(keys, dtype=np.int64).reshape(-1).view(np.uint64)
    n = k.shape[0]
    ctr = np.zeros((n, 3, 4), dtype=np.uint32)
    ctr[:, :, 0] = np.arange(3, dtype=np.uint32)[None, :]
    ctr[:, :, 1] = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    ctr[:, :, 2] = (k >> np.uint64(32)).astype(np.uint32)[:, None]
    ctr[:, :, 3] = np.uint32(epoch & 0xFFFFFFFF)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    words = philox4x32_10(ctr, key).reshape(n, 12)[:, :9]
    return ((words >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def params_ref(u, ranges=DEFAULT_RANGES) -> np.ndarray:
    """value = lo + (hi - lo) u in float64; a range of None is the term's identity value."""
    u = np.asarray(u, dtype=np.float64)
    lo = np.array([IDENTITY_PARAMS[i] if r is None else r[0] for i, r in enumerate(ranges)], dtype=np.float64)
    hi = np.array([IDENTITY_PARAMS[i] if r is None else r[1] for i, r in enumerate(ranges)], dtype=np.float64)
    return lo + (hi - lo) * u


def tables_ref(params, H: int, W: int) -> np.ndarray:
    """float64 parameters [F, 9] (hue, saturation, brightness, contrast, rotation deg, scale, shear deg, tx, ty) -> float64 tables [F, 16]."""
    params = np.asarray(params, dtype=np.float64).reshape(-1, 9)
    yinv = np.linalg.inv(YIQ)
    out = np.zeros((params.shape[0], 16), dtype=np.float64)
    for f, (h, s, b, c, rot, scl, shr, tx, ty) in enumerate(params):
        a = 2.0 * math.pi * h
        rot_m = np.array([[0.0, 0.0, 0.0], [0.0, math.cos(a) - 1.0, -math.sin(a)], [0.0, math.sin(a), math.cos(a) - 1.0]])
        hue_m = np.eye(3) + yinv @ rot_m @ YIQ                       # = Y^-1 Rot_IQ Y, exactly I at h = 0
        sat_m = s * np.eye(3) + (1.0 - s) * np.outer(np.ones(3), LUMA)
        out[f, :9] = (b * c * (hue_m @ sat_m)).reshape(9)
        out[f, 9] = b * (1.0 - c)
        th, phi = math.radians(rot), math.radians(shr)
        r_m = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        a_m = scl * (r_m @ np.array([[1.0, math.tan(phi)], [0.0, 1.0]]))
        ainv = np.linalg.inv(a_m)
        ctr = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
        g = ctr - ainv @ (ctr + np.array([tx, ty]))
        out[f, 10:13] = ainv[0, 0], ainv[0, 1], g[0]
        out[f, 13:16] = ainv[1, 0], ainv[1, 1], g[1]
    return out + 0.0


def translation_table(tx: float, ty: float) -> np.ndarray:
    """The table of a pure translation by (tx, ty) pixels: out(x, y) = src(x - tx, y - ty)."""
    t = IDENTITY_TABLE.copy()
    t[12], t[15] = -tx, -ty
    return t


def mean_luma_sum(frame: np.ndarray) -> int:
    f = frame.astype(np.int64)
    return int((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2]).sum())


def _tap(src, H, W, yf, xf):
    with np.errstate(invalid="ignore"):
        ok = (yf >= 0) & (yf < np.float32(H)) & (xf >= 0) & (xf < np.float32(W))          # on the float coordinate; NaN compares false
    yi = np.where(ok, yf, np.float32(0)).astype(np.int64)
    xi = np.where(ok, xf, np.float32(0)).astype(np.int64)
    return np.where(ok[..., None], src[yi, xi, :].astype(np.float32), np.float32(0))


def augment_frame_ref(src: np.ndarray, table: np.ndarray) -> np.ndarray:
    """One frame uint8 [H, W, 3] under one fp32 table [16] -> uint8 [H, W, 3]; float32 throughout, every operation rounded on its own."""
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    H, W = src.shape[:2]
    tb = np.asarray(table, dtype=np.float32)
    inv = np.float32(1.0 / (256.0 * H * W))
    mu = np.float32(mean_luma_sum(src)) * inv
    with np.errstate(all="ignore"):
        off = tb[9] * mu
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        sx = (tb[10] * xx + tb[11] * yy) + tb[12]
        sy = (tb[13] * xx + tb[14] * yy) + tb[15]
        xl, yl = np.floor(sx), np.floor(sy)
        fx, fy = sx - xl, sy - yl
        xh, yh = xl + np.float32(1), yl + np.float32(1)
        gy, gx = np.float32(1) - fy, np.float32(1) - fx
        w00, w01, w10, w11 = (gy * gx)[..., None], (gy * fx)[..., None], (fy * gx)[..., None], (fy * fx)[..., None]
        t00, t01, t10, t11 = _tap(src, H, W, yl, xl), _tap(src, H, W, yl, xh), _tap(src, H, W, yh, xl), _tap(src, H, W, yh, xh)
        v = (w00 * t00 + w01 * t01) + (w10 * t10 + w11 * t11)
        assert v.dtype == np.float32
        out = np.empty((H, W, 3), dtype=np.uint8)
        for c in range(3):
            o = ((tb[3 * c] * v[..., 0] + tb[3 * c + 1] * v[..., 1]) + tb[3 * c + 2] * v[..., 2]) + off
            m = np.where(o > 0, o, np.float32(0))                   # NaN -> 0
            m = np.where(m < 255, m, np.float32(255))
            assert m.dtype == np.float32
            out[..., c] = np.rint(m).astype(np.uint8)
    return out


def augment_frames_ref(img: np.ndarray, tables: np.ndarray) -> np.ndarray:
    """uint8 [F, H, W, 3] (or [B, T, H, W, 3]) under fp32 tables [F, 16]."""
    shape = img.shape
    img = img.reshape((-1,) + shape[-3:])
    tables = np.asarray(tables, dtype=np.float32).reshape(-1, 16)
    assert tables.shape[0] == img.shape[0]
    return np.stack([augment_frame_ref(img[f], tables[f]) for f in range(img.shape[0])]).reshape(shape)


def grid_sample_route(src: np.ndarray, table: np.ndarray) -> np.ndarray:
    """The same frame under the same table by an independent float64 route: F.grid_sample(bilinear, zeros, align_corners=False) on the normalised
    coordinates of the table's source positions, then the colour map; clamp, round half to even."""
    import torch
    import torch.nn.functional as F
    H, W = src.shape[:2]
    tb = torch.from_numpy(np.asarray(table, dtype=np.float32)).to(torch.float64)
    x = torch.from_numpy(src.astype(np.float64)).permute(2, 0, 1)[None]
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    sx = tb[10] * xx + tb[11] * yy + tb[12]
    sy = tb[13] * xx + tb[14] * yy + tb[15]
    grid = torch.stack([(2.0 * sx + 1.0) / W - 1.0, (2.0 * sy + 1.0) / H - 1.0], dim=-1)[None]
    v = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0]          # [3, H, W]
    mu = mean_luma_sum(src) / (256.0 * H * W)
    o = torch.einsum("cd,dhw->chw", tb[:9].view(3, 3), v) + tb[9] * mu
    return torch.round(o.clamp(0.0, 255.0)).permute(1, 2, 0).to(torch.uint8).numpy()
