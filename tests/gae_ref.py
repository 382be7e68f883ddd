"""Generalised advantage estimation on the host: the float32 twin of vpt_gae_kernel (ops.gae) -- the same fp32 operations in the same order, so
the GPU result equals it bit for bit -- and the fp64 textbook recursion run per episode segment, with the bound between the two.  A plain helper
(no test, no fixture): numpy only, nothing of vpt_amd.

    nt = !first[t+1] (t = T-1: !next_first),  delta = r + (nt ? gamma V_{t+1} : 0) - V,  A = delta + (nt ? (gamma lambda) A_{t+1} : 0),  ret = A + V"""
import numpy as np

U = 2.0 ** -24
CASES = [(1, 1), (3, 7), (2, 64), (5, 130)]


def make_case(b, t, seed=0):
    """Rewards and values of mixed sign; `first` flags at t = 0, mid-row and t = T - 1 (and a few at random); next_first both ways."""
    rng = np.random.default_rng(seed + 100 * b + t)
    r, v = rng.standard_normal((b, t)).astype(np.float32), (3 * rng.standard_normal((b, t))).astype(np.float32)
    first = rng.random((b, t)) < 0.08
    first[0, 0] = True
    first[b - 1, t // 2] = True
    first[b // 2, t - 1] = True
    next_first = (np.arange(b) % 2 == 0)
    last = (3 * rng.standard_normal(b)).astype(np.float32)
    return r, v, first, last, next_first


def gae_f32(reward, value, first, last_value, next_first, gamma, lam):
    """float32 [B, T] twin -> (adv, ret).  Every intermediate is rounded to float32 exactly where the kernel rounds (no fused multiply-add)."""
    f = np.float32
    r, v = np.asarray(reward, f), np.asarray(value, f)
    first, next_first = np.asarray(first).astype(bool), np.asarray(next_first).astype(bool)
    b, t_ = r.shape
    g = f(gamma)
    gl = f(g * f(lam))
    adv, ret = np.zeros((b, t_), f), np.zeros((b, t_), f)
    vnext, anext, nt = np.asarray(last_value, f).reshape(b).copy(), np.zeros(b, f), ~next_first.reshape(b)
    with np.errstate(all="ignore"):
        for t in range(t_ - 1, -1, -1):
            boot = np.where(nt, (g * vnext).astype(f), f(0)).astype(f)
            delta = ((r[:, t] + boot).astype(f) - v[:, t]).astype(f)
            a = (delta + np.where(nt, (gl * anext).astype(f), f(0)).astype(f)).astype(f)
            adv[:, t], ret[:, t] = a, (a + v[:, t]).astype(f)
            vnext, anext, nt = v[:, t], a, ~first[:, t]
    return adv, ret


def gae_f64_segments(reward, value, first, last_value, next_first, gamma, lam):
    """The textbook definition in fp64, episode segment by segment: a segment is a maximal run of frames with no episode start after its first
    frame; inside it A_t = sum_k (gamma lambda)^k delta_{t+k}, the last delta bootstrapping from the next value unless the next frame starts an
    episode.  -> (adv, ret, bound): bound is the float32 recurrence's propagated rounding, T 4u sum |terms| over the segment's tail."""
    r, v = np.asarray(reward, np.float64), np.asarray(value, np.float64)
    first, next_first = np.asarray(first).astype(bool), np.asarray(next_first).astype(bool).reshape(-1)
    last_value = np.asarray(last_value, np.float64).reshape(-1)
    g, gl = float(np.float32(gamma)), float(np.float32(np.float32(gamma) * np.float32(lam)))
    b, t_ = r.shape
    adv, bound = np.zeros((b, t_)), np.zeros((b, t_))
    for i in range(b):
        ends = [t for t in range(t_) if (next_first[i] if t == t_ - 1 else first[i, t + 1])] + ([t_ - 1] if not next_first[i] else [])
        start = 0
        for e in sorted(set(ends)):
            terminal = next_first[i] if e == t_ - 1 else True
            for t in range(start, e + 1):
                a = mag = 0.0
                for k in range(e - t + 1):
                    s = t + k
                    vn = 0.0 if (s == e and terminal) else (last_value[i] if s == t_ - 1 else v[i, s + 1])
                    a += gl ** k * (r[i, s] + g * vn - v[i, s])
                    mag += gl ** k * (abs(r[i, s]) + abs(g * vn) + abs(v[i, s]))
                adv[i, t], bound[i, t] = a, t_ * 4 * U * (mag + abs(v[i, t]))
            start = e + 1
    return adv, adv + v, bound
