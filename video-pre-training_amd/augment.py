"""Sequence-consistent image augmentation on the device  (`from vpt_amd.augment import FrameAugmenter`).

The VPT recipe trains its inverse-dynamics model and its foundation model on augmented frames: the colour is perturbed (hue, saturation,
brightness, contrast) and the frame gets a small affine warp (rotation, scale, shear, translation), with ONE draw for all frames of a
sequence -- the IDM reads the motion between neighbouring frames, which a per-frame draw would destroy.  Horizontal flips are deliberately
absent: the actions are not flip-invariant.

    aug = FrameAugmenter(seed=0)
    chunk2 = aug(chunk)                  # a SequenceBatcher / labelled_chunks dict: img replaced, keyed by chunk["episode_id"]
    img2 = aug.apply(img, keys)          # uint8 [B,T,H,W,3]; keys int64 [B,T] or [B]; None: a fresh key per row and call
    tables = aug.tables(keys, H, W)      # fp32 [F,16]: what the kernel is given

The transform of a frame is a pure function of (seed, epoch, key): nine Philox uniforms (ops.augment_uniforms) -> nine parameters -> a
16-float table (colour matrix, mean gain, inverse affine map).  Frames with the same key -- a recording's id -- get the same table in
whichever chunk they appear, so a recording keeps its transform across chunk edges without any bookkeeping; a new `epoch` redraws every
recording.  A negative key (the padding frames of `pad_last` / `labelled_chunks` carry episode_id = -1) gets the identity table.

The tables are built with torch ops in float64 and rounded to fp32 at the end (device-agnostic: the same function runs on CPU tensors
in the tests); one launch (ops.augment_frames, csrc/vpt_augment.hip) then turns the uint8 frames into augmented uint8 frames: no host
round trip, no fp32 image in memory.

THE DEFAULT RANGES ARE UNVERIFIED AGAINST THE PAPER: they are a recollection of its appendix (the paper is not available to this
repository) and plain constructor arguments; set your own.  `None` switches a term off."""
import math
from typing import Optional, Tuple

import torch

# RGB -> YIQ (rows) and its inverse (numpy.linalg.inv of the matrix below in float64, written out so that no device needs a solver)
_YIQ = ((0.299, 0.587, 0.114), (0.596, -0.274, -0.322), (0.211, -0.523, 0.312))
_LUMA = (77.0 / 256.0, 150.0 / 256.0, 29.0 / 256.0)
IDENTITY_PARAMS = (0.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0)      # hue, saturation, brightness, contrast, rotation, scale, shear, tx, ty
PARAM_NAMES = ("hue", "saturation", "brightness", "contrast", "rotation_deg", "scale", "shear_deg", "translate_x", "translate_y")
IDENTITY_TABLE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _yiq_inverse():
    (a, b, c), (d, e, f), (g, h, i) = _YIQ
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    return (((e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det),
            ((f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det),
            ((d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det))


def tables_from_params(params: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """float64 parameters [F, 9] (PARAM_NAMES order; hue in turns, angles in degrees, translation in pixels) -> fp32 tables [F, 16].

    Colour:   C = b c (Hue(h) Sat(s)),  k = b (1 - c);  Sat(s) = s I + (1 - s) 1 w^T with w = (77, 150, 29) / 256;
              Hue(h) = Y^-1 Rot_IQ(2 pi h) Y, computed as I + Y^-1 (Rot_IQ - I) Y so that h = 0 gives I exactly.
    Geometry: forward map about ctr = ((W-1)/2, (H-1)/2):  dst = A (src - ctr) + ctr + t,  A = scale R(theta) [[1, tan phi], [0, 1]];
              the table holds the inverse, from an output pixel index to a source pixel index:  G = [A^-1 | ctr - A^-1 (ctr + t)].
    Identity parameters give the identity table bit for bit."""
    if params.dim() != 2 or params.shape[1] != 9:
        raise ValueError(f"params must be [F, 9], got {tuple(params.shape)}")
    p = params.to(torch.float64)
    dev, n = p.device, p.shape[0]
    hue, sat, bri, con, rot, scl, shr, tx, ty = p.unbind(1)
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    y = torch.tensor(_YIQ, dtype=torch.float64, device=dev)
    yinv = torch.tensor(_yiq_inverse(), dtype=torch.float64, device=dev)
    ang = (2.0 * math.pi) * hue
    cs, sn = torch.cos(ang), torch.sin(ang)
    rot_m = torch.zeros(n, 3, 3, dtype=torch.float64, device=dev)          # Rot_IQ - I
    rot_m[:, 1, 1] = cs - 1.0
    rot_m[:, 1, 2] = -sn
    rot_m[:, 2, 1] = sn
    rot_m[:, 2, 2] = cs - 1.0
    hue_m = eye + yinv @ rot_m @ y
    w = torch.tensor(_LUMA, dtype=torch.float64, device=dev)
    sat_m = sat[:, None, None] * eye + (1.0 - sat)[:, None, None] * w.expand(3, 3)
    c_m = (bri * con)[:, None, None] * (hue_m @ sat_m)
    k = bri * (1.0 - con)

    th, phi = torch.deg2rad(rot), torch.deg2rad(shr)
    ct, st, tp = torch.cos(th), torch.sin(th), torch.tan(phi)
    a00, a01, a10, a11 = scl * ct, scl * (ct * tp - st), scl * st, scl * (st * tp + ct)
    det = a00 * a11 - a01 * a10
    i00, i01, i10, i11 = a11 / det, -a01 / det, -a10 / det, a00 / det
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    ux, uy = cx + tx, cy + ty
    g02 = cx - (i00 * ux + i01 * uy)
    g12 = cy - (i10 * ux + i11 * uy)
    g = torch.stack([i00, i01, g02, i10, i11, g12], dim=1) + 0.0        # + 0.0: no negative zeros in the table
    return torch.cat([c_m.reshape(n, 9), k[:, None], g], dim=1).to(torch.float32)


def _range(r, ident, name) -> Tuple[float, float]:
    if r is None:
        return (ident, ident)
    lo, hi = float(r[0]), float(r[1])
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"FrameAugmenter: {name} must be a finite (lo, hi) with lo <= hi, or None; got {r}")
    return (lo, hi)


class FrameAugmenter:
    """Colour and affine augmentation of uint8 frame chunks with one draw per recording (module docstring).

    hue in turns of the IQ plane; saturation, brightness, contrast and scale as factors (contrast about the frame's mean luma); rotation and shear
    in degrees; translate_px in pixels, drawn separately for x and y.  Each range is (lo, hi), drawn uniformly; None switches the term off.
    DEFAULTS UNVERIFIED AGAINST THE PAPER.

    `epoch` is a plain attribute: a new epoch redraws every recording.  state_dict() / load_state_dict() carry seed, epoch and the counter of
    keyless calls; the ranges are configuration, not state."""

    def __init__(self, seed: int = 0, hue=(-0.02, 0.02), saturation=(0.8, 1.2), brightness=(0.8, 1.2), contrast=(0.8, 1.2),
                 rotation_deg=(-2, 2), scale=(0.98, 1.02), shear_deg=(-2, 2), translate_px=(-2, 2)):
        self.seed = int(seed)
        self.epoch = 0
        self.calls = 0
        given = (hue, saturation, brightness, contrast, rotation_deg, scale, shear_deg, translate_px, translate_px)
        self.ranges = tuple(_range(r, ident, name) for r, ident, name in zip(given, IDENTITY_PARAMS, PARAM_NAMES))
        if self.ranges[5][0] <= 0.0:
            raise ValueError("FrameAugmenter: scale must be positive")

    # ---- the transform of a key ----
    def params(self, uniforms: torch.Tensor) -> torch.Tensor:
        """uniforms [F, 9] in [0, 1) -> float64 parameters [F, 9]: value = lo + (hi - lo) u."""
        u = uniforms.to(torch.float64)
        lo = torch.tensor([r[0] for r in self.ranges], dtype=torch.float64, device=u.device)
        hi = torch.tensor([r[1] for r in self.ranges], dtype=torch.float64, device=u.device)
        return lo + (hi - lo) * u

    def tables(self, keys: torch.Tensor, H: int, W: int, uniforms: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int64 keys [...] -> fp32 tables [keys.numel(), 16] for frames of H x W.  `uniforms` fp32 [F, 9]: the draws, when the caller has them
        (then nothing here needs a GPU); default: ops.augment_uniforms(keys, seed, epoch) on the keys' device.  Negative keys get the identity."""
        if keys.dtype != torch.int64:
            raise TypeError(f"keys: expected int64, got {keys.dtype}")
        keys = keys.reshape(-1).contiguous()
        if uniforms is None:
            from . import ops
            uniforms = ops.augment_uniforms(keys, self.seed, self.epoch)
        if tuple(uniforms.shape) != (keys.numel(), 9) or uniforms.device != keys.device:
            raise ValueError(f"uniforms must be [{keys.numel()}, 9] on {keys.device}, got {tuple(uniforms.shape)} on {uniforms.device}")
        t = tables_from_params(self.params(uniforms), int(H), int(W))
        ident = torch.tensor(IDENTITY_TABLE, dtype=torch.float32, device=t.device)
        return torch.where((keys < 0)[:, None], ident, t).contiguous()

    # ---- frames ----
    def apply(self, img: torch.Tensor, keys: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [B,T,H,W,3] on the GPU -> augmented uint8 [B,T,H,W,3].  keys int64 [B,T] (one per frame) or [B] (one per row); None: row b of this
        call gets the fresh key calls * B + b, and the call counter advances.  `out` may be `img` (in place)."""
        from . import ops
        if img.dim() != 5 or img.shape[-1] != 3:
            raise ValueError(f"img must be uint8 [B, T, H, W, 3], got {tuple(img.shape)}")
        b, t, h, w, _ = img.shape
        if keys is None:
            keys = torch.arange(self.calls * b, (self.calls + 1) * b, dtype=torch.int64, device=img.device)
            self.calls += 1
        if keys.dtype != torch.int64:
            raise TypeError(f"keys: expected int64, got {keys.dtype}")
        if tuple(keys.shape) == (b,):
            keys = keys[:, None].expand(b, t)
        if tuple(keys.shape) != (b, t):
            raise ValueError(f"keys must be int64 [{b}, {t}] or [{b}], got {tuple(keys.shape)}")
        keys = keys.to(img.device)
        return ops.augment_frames(img, self.tables(keys, h, w), out=out)

    def __call__(self, chunk: dict) -> dict:
        """A chunk dict of SequenceBatcher / labelled_chunks -> a new dict whose `img` is augmented, keyed by chunk["episode_id"]; every other entry is
        the same object."""
        out = dict(chunk)
        out["img"] = self.apply(chunk["img"], chunk["episode_id"])
        return out

    # ---- state ----
    def state_dict(self) -> dict:
        return dict(seed=self.seed, epoch=int(self.epoch), calls=self.calls)

    def load_state_dict(self, state: dict) -> None:
        self.seed, self.epoch, self.calls = int(state["seed"]), int(state["epoch"]), int(state["calls"])
