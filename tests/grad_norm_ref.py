"""Host twin of csrc/vpt_grad_norm.hip: the kernels restated operation for operation in numpy, the fp64 reference, and the derived error bound.

The summation tree, per tensor and per 1024-element table block (elements past the tensor's end are exact zeros):
  x = g * scale, q = x * x                                  fp32, two roundings per factor, no fma
  thread t (256 per block) owns elements 4t .. 4t + 3:       ((q0 + q1) + q2) + q3
  wave (64 threads): xor butterfly, offsets 32, 16, .. 1     v += v[lane ^ o]   (every lane ends with the same bits)
  block: the four waves                                      (w0 + w1) + (w2 + w3)         -> one fp32 partial
  tensor (fp64): thread i adds partials i, i + 256, ...      sequentially, then the same butterfly and cross-wave tree over the 256 threads
  total (fp64): thread i adds tensor sums i, i + 256, ...    the same
  norm = fp32(sqrt_f64(total));  coef = min((1 / (norm + 1e-6)) * max_norm, 1) in fp32 -- the operations of torch's clip_coef_clamped
  (`max_norm / tensor` is tensor.reciprocal() * max_norm in torch, two roundings, not one division); 1 when max_norm is None or <= 0, 0 when the total
  is not finite.

The bound (first order, u = 2^-24): each square carries 3u (one rounding of g * scale, doubled by the square, one of the product); a block partial adds
3 + 6 + 2 = 11 fp32 additions of non-negative terms, u each; the fp64 finish adds at most (256 + 8) + (256 + 8) additions of 2^-53 (the longest chain:
65 536 blocks in one tensor, 65 536 tensors), below 1e-13.  So |sum - exact| <= 14u sum, the square root halves it, the final rounding to fp32 adds u:
8u on the norm.  Measured over the sizes, magnitudes and scales of tests/test_grad_norm_ref_cpu.py: at most 0.7u (errors add like sqrt(n), the bound like n).
`scale` is taken as the fp32 value the C entry point receives, in the twin and in the reference alike: its own rounding is the caller's."""
import numpy as np

U = 2.0 ** -24
BOUND_ULPS = 8.0
BOUND = BOUND_ULPS * U + 600 * 2.0 ** -53          # relative, on the norm

_F = np.float32


def _butterfly(v):
    """[..., 64] -> [...]: the xor butterfly of wave_sum; lane 0's value (all lanes agree)."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def _block_tree(v, cross_wave=True):
    """[..., 256] per-thread values -> [...]: butterfly per wave, then (w0 + w1) + (w2 + w3).  cross_wave=False: a MUTATION (wave 0 only)."""
    w = _butterfly(v.reshape(v.shape[:-1] + (4, 64)))
    if not cross_wave:
        return w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _strided_f64(x):
    """fp64 [n] -> fp64 scalar: thread i adds x[i], x[i + 256], ... in order, then the block tree (stages one and two of the finish)."""
    n = x.shape[0]
    rows = max((n + 255) // 256, 1)
    pad = np.zeros(rows * 256, dtype=np.float64)
    pad[:n] = x
    acc = np.zeros(256, dtype=np.float64)
    for r in pad.reshape(rows, 256):
        acc = acc + r
    return _block_tree(acc)


def block_partials(g, scale, drop_tail=False, use_scale=True, cross_wave=True):
    """fp32 [ceil(n / 1024)] block partials of one tensor.  The keyword arguments are the test's MUTATIONS (drop_tail: the tensor's last partial
    group of four is lost; use_scale=False: grad_scale ignored; cross_wave=False: only wave 0 of every block counts)."""
    g = np.ascontiguousarray(g, dtype=_F).reshape(-1)
    n = g.shape[0]
    nb = (n + 1023) // 1024
    pad = np.zeros(nb * 1024, dtype=_F)
    pad[:n] = g
    if drop_tail and n % 4:
        pad[n - n % 4:n] = 0
    with np.errstate(over="ignore", invalid="ignore"):
        x = pad * _F(scale) if use_scale else pad
        q = (x * x).reshape(nb, 256, 4)
        t = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
        return _block_tree(t, cross_wave=cross_wave).astype(_F)


def coef_f32(norm, max_norm):
    """The fp32 clip coefficient from the fp32 norm, as the finish kernel (and torch's clip_grad_norm_) computes it."""
    if max_norm is None or not max_norm > 0:
        return _F(1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return np.fmin((_F(1.0) / (_F(norm) + _F(1e-6))) * _F(max_norm), _F(1.0))


def restate_f32(grads, scale=1.0, max_norm=None, **mutation):
    """The kernels' result for a list of arrays -> dict(partials [list of fp32 arrays], tensor_sums fp64 [T], total fp64, norm fp32, coef fp32,
    nonfinite bool, per_tensor fp32 [T], out fp32 [4] = norm_out)."""
    partials = [block_partials(g, scale, **mutation) for g in grads]
    with np.errstate(over="ignore", invalid="ignore"):
        tsum = np.array([_strided_f64(p.astype(np.float64)) for p in partials], dtype=np.float64)
        total = _strided_f64(tsum)
        finite = bool(np.isfinite(total))
        norm = _F(np.sqrt(total))
        per = np.sqrt(tsum).astype(_F)
    coef = coef_f32(norm, max_norm) if finite else _F(0.0)
    out = np.array([norm, coef, 0.0 if finite else 1.0, 0.0], dtype=_F)
    return dict(partials=partials, tensor_sums=tsum, total=total, norm=norm, coef=coef, nonfinite=not finite, per_tensor=per, out=out)


def norm_f64(grads, scale=1.0):
    """The reference: l2 norm of grads * scale with every operation in fp64 (scale as the fp32 value the kernel receives), pairwise sums."""
    s = np.float64(_F(scale))
    tot = 0.0
    for g in grads:
        x = np.asarray(g, dtype=np.float64).reshape(-1) * s
        tot += float(np.sum(x * x))
    return float(np.sqrt(tot))
