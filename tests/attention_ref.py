"""References for the attention kernels (vpt_attn_kernel, vpt_attn_step_kernel, vpt_attn_bwd_kernel, vpt_full_attn_bwd_kernel and the two finish
kernels): plain torch, importable without a GPU.  compute() evaluates forward and closed-form backward in ONE dtype: float64 is the reference
(tests/test_attention_ref_cpu.py pins it to fp64 autograd), float32 is the emulation of the kernels' arithmetic that the CPU tests mutate.

Layout (ops.masked_attention): qkvr [B*t, ld] = Q | K | V (hid columns each) | R (10 per head) | padding;  kmem / vmem [B, maxlen, hid];  row j of
[memory ; chunk] is visible to query i when  i + 1 <= j <= i + maxlen  (band offset off = maxlen + i - j: 0 = the query itself, maxlen - 1 = the oldest
key),  memvalid[j] for a memory row,  j >= qlo[i].  logit = q.k / 128 + sum_n R[i][n] b_nd[n][off];  P = softmax over the visible keys;  out = P V.
Mask "none" (ops.full_attention): maxlen = 0, no memory, no bias, every query sees the t rows of its window.

Two instruments, as in tests/linear_ref.py.

A. EXACT VALUES (index mapping and masking) -- exact_case().  k_j = 128 e_code(j), code(j) = (j + 37 head) mod 128, q_i = 128 * (sum of e_code over
   the query's targets and its decoy), V / dOut / b_nd small nonzero integers, R = 0.  A matching key has logit 128 * 128 / 128 = 128, every other 0;
   fp32 expf(-128) underflows to exactly 0 (e^-128 < 2^-150), so P is exactly one-hot ("onehot") or (1/2, 1/2) ("tie"), and every later value is a
   dyadic number of a few bits: out = V[target] resp. the mean of two rows, dV = the sums of the dOut rows routed to a key, dS = 0 resp.
   +-(dP1 - dP2) / 4, so dQ, dK, dR are exact (zero in "onehot").  Family "bias" puts the logits through R . b_nd alone (q = 0, R = 128 e_n, two columns
   of row n of b_nd set to 1): offset indexing of the bias, and a nonzero exact db_nd.  Stages of the kernels on these inputs, read in the source:
   the dot products add exact products (16384 or integers) -- exact; `dot * (1.0f / 128)` a power of two -- exact; `expf(s - m)` with s - m in
   {0, -128, -256, ...}: expf(0) = 1 exactly (|error| <= 2 ulp of a result that is representable: any correctly bounded implementation returns 1.0
   for x = 0; the CPU test checks torch's, the GPU test the device's through every "onehot" output) and 0 below; tot in {1, 2}: `1.0f / tot` exact;
   fma chains over values with < 24 significant bits -- exact.  No stage had to be excepted.  Decoys: an invalid memory row holds k = 128 * (1, ..., 1)
   (logit 128 with EVERY query); the row just below qlo[i] has its code added to q_i; rows j - 128 and j + 128 carry the target's own code by
   construction of code().  Admitting any of them changes the answer outright (a three-way tie or a moved row).  Zeros are compared by value
   (-0.0 == 0.0: a product p * (dP - D) with p = 0 may carry either sign), everything else is then bit-equal.

B. REAL VALUES UNDER A DERIVED BOUND (rounding points) -- real_case().  randn inputs (q scaled by 2, b_nd by 0.5: today's tests), fp64 over the same
   fp32 operands.  u = 2^-24.  Each constant is an operation count of the kernel:
     logit      |s - s64| <= D = 129 u (sum_d |q||k| / 128 + sum_n |R||b_nd|)        a term of the 128-term MFMA chain passes its product's rounding and at most
                127 additions (tile 4: four 32-term chains + 2 additions: fewer); the scale is exact; the bias is 10 fma (< 128); + 1 for the final addition.
                D_q = max over the visible keys.
     expf       relative 4 u.  The ROCm math documentation is not among the files of this installation (no accuracy table under the ROCm tree), so
                2 ulp = 2 * 2^-23 are allowed, as the issue provides; plus |s - m| u from the rounding of its argument.
     P          p^ = p (1 + eta),  |eta| <= 2 D_q + (C_P + |s_k - m| + A_q) u,  A_q = sum_k p_k |s_k - m|:
                C_P = 4 (own expf) + 4 (the expf errors inside the normaliser, a p-weighted mean) + 8 (wave_sum: 2 additions + 6 butterfly levels on
                positive terms) + 1 (the correctly rounded 1.0f / tot) [+ 1 for e * inv in the backward kernels] = 17 [18].
     out        |out - out64| <= ulp16(out64) + (2 D_q + (C_F + A_q) u) sum_k p_k |v_kd| + u sum_k p_k |s_k - m| |v_kd|,
                C_F = 17 + 160 (the 160-term P V chain) + 1 (o * Sc) = 178.  The step kernel's chains are shorter (2 x 64 fma + 1).
     dP         129 u sum_d |dO||V|                                                  128-term chain + 1
     D_i        sum_k p (eta |dP| + E_dP) + 9 u sum_k p |dP|                         fma chain of 3 + 6 butterfly levels
     dS         E_dS = p (eta |dP - D_i| + E_dP + E_Di + 2 u (|dP| + |D_i|))         the subtraction and the product
     dQ         (E_dS |K| + 161 u |dS||K|) / 128                                     160-term chain + the scale's product
     dK, dV     (E_dS^T |Q| + 38 u |dS|^T|Q|) / 128,   (p eta)^T |dO| + 38 u p^T |dO|   32-term chain per slab + its product + 5 slabs summed
     dR         E_dS |b| + (maxlen + 1) u |dS||b|                                    one fma per band offset
     db_nd      E_dS^T |R| + (32 + rows) u |dS|^T|R|                                 32 fma per query tile, `rows` = B * heads * tiles slab rows summed
   Every bound is multiplied by 1 + 2^-10 for the products of two first-order terms (each far below 2^-10).  No element is left out; padding columns of
   dqkvr have bound 0 (exact zeros).  fp16 output: the same with that format's ulp."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests import linear_ref as L

D = torch.float64
U = 2.0 ** -24
DH, QT, NK = 128, 32, 160
C_LOGIT, C_EXP, C_TOT, C_DIV = DH + 1, 4, 8, 1
C_P = 2 * C_EXP + C_TOT + C_DIV            # 17
C_F = C_P + NK + 1                         # 178
C_DP, C_DI, C_DQ, C_SLAB = DH + 1, 9, NK + 1, QT + 1 + 5
SECOND = 1.0 + 2.0 ** -10
FLUSH = -104.0                             # fp32 expf(x) == 0 for x < -103.98 (e^x < 2^-150)
ulp16, DT = L.ulp16, L.DT

MUTATIONS = ["band+1", "band-1", "drop_oldest", "bias_off+1", "bias_missing", "scale127", "no_memvalid", "qlo+1", "norm_missing", "drop_slab",
             "no_Di_row", "dbnd_missing_tile"]
NONE_MUTATIONS = ["scale127", "norm_missing", "drop_slab", "no_Di_row"]     # the ones that exist for mask "none"


def qlo_of(first, maxlen):
    """first bool [B, t] -> int32 [B, t]: maxlen + the latest episode start at or before the frame, 0 without one (packing.episode_bounds)."""
    b, t = first.shape
    q = torch.zeros(b, t, dtype=torch.int32)
    for r in range(b):
        last = -1
        for p in range(t):
            if bool(first[r, p]):
                last = p
            q[r, p] = maxlen + last if last >= 0 else 0
    return q


def _heads(z, b, n, h):
    return z.reshape(b, n, h, DH).permute(0, 2, 1, 3)                        # [B, H, n, 128]


def _rows(z, b, t):
    return z.permute(0, 2, 1, 3).reshape(b * t, -1)                          # [B, H, t, c] -> [B*t, H*c]


def compute(c, dt=D, mut=None, flush=False, backward=True):
    """Forward and closed-form backward of one case in dtype `dt`.  dt = float64 and mut = None: the reference, with the magnitudes and bounds
    (fields b_*; b_out WITHOUT the 16-bit ulp, see out_bound).  flush: P = 0 where s - m < -104, what fp32 expf gives (instrument A's expected values).
    mut: one of MUTATIONS, a subtly wrong kernel."""
    B, t, H, ml, hid = c.B, c.t, c.heads, c.maxlen, c.hid
    ref = dt == D and mut is None
    x = c.qkvr.to(dt)
    q, kc, vc = _heads(x[:, :hid], B, t, H), _heads(x[:, hid:2 * hid], B, t, H), _heads(x[:, 2 * hid:3 * hid], B, t, H)
    ii = torch.arange(t).view(t, 1)
    if c.causal:
        k = torch.cat([_heads(c.kmem.to(dt), B, ml, H), kc], 2)
        v = torch.cat([_heads(c.vmem.to(dt), B, ml, H), vc], 2)
        r = x[:, 3 * hid:3 * hid + 10 * H].reshape(B, t, H, 10).permute(0, 2, 1, 3)       # [B, H, t, 10]
        bnd = c.b_nd.to(dt)
        J = ml + t
        jj = torch.arange(J).view(1, J)
        sh = {"band+1": 1, "band-1": -1}.get(mut, 0)
        band = (jj >= ii + 1 + sh + (1 if mut == "drop_oldest" else 0)) & (jj <= ii + ml + sh)
        mv = torch.ones(B, ml, dtype=torch.bool) if mut == "no_memvalid" else c.memvalid.bool()
        vis = band.view(1, t, J) & torch.cat([mv, torch.ones(B, t, dtype=torch.bool)], 1).view(B, 1, J)
        if c.qlo is not None:
            ql = c.qlo.long()
            if mut == "qlo+1":
                ql = torch.where(ql > 0, ql + 1, ql)
            vis = vis & (jj.view(1, 1, J) >= ql.view(B, t, 1))
        vis = vis.unsqueeze(1).expand(B, H, t, J)
        off = ml + ii - jj                                                               # [t, J]
        inband = (off >= 0) & (off < ml)
        offc = (off + (1 if mut == "bias_off+1" else 0)).clamp(0, ml - 1)
        bm = bnd[:, offc]                                                                # [10, t, J]: the b_nd column a (query, key) pair reads
        if mut == "bias_missing":
            bm = bm * (off != 0).to(dt)
        bias = torch.einsum("bhin,nij->bhij", r, bm)
    else:
        k, v, J = kc, vc, t
        vis = torch.ones(B, H, t, J, dtype=torch.bool)
        bias = torch.zeros((), dtype=dt)
    scale = 1.0 / 127 if mut == "scale127" else 1.0 / DH
    s = (q @ k.transpose(-1, -2)) * scale + bias
    zero = torch.zeros((), dtype=dt)
    m = torch.where(vis, s, torch.full((), -math.inf, dtype=dt)).amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, zero)
    xa = torch.where(vis, s - m, zero)
    e = torch.where(vis, torch.exp(xa), zero)
    if flush:
        e = torch.where(xa < FLUSH, zero, e)
    et = e
    if mut == "norm_missing":                                                            # the normaliser loses the first visible key's term
        et = e.clone()
        et.scatter_(-1, vis.to(torch.uint8).argmax(-1, keepdim=True), 0.0)
    tot = et.sum(-1, keepdim=True)
    p = e * torch.where(tot > 0, 1.0 / tot, zero)
    o = SimpleNamespace(p=p, vis=vis, s=s, out=_rows(p @ v, B, t))
    if ref:
        mag_s = (q.abs() @ k.abs().transpose(-1, -2)) / DH
        if c.causal:
            mag_s = mag_s + torch.einsum("bhin,nij->bhij", r.abs(), bm.abs())
        dq_ = torch.where(vis, C_LOGIT * U * mag_s, zero).amax(-1, keepdim=True)        # D_q
        xabs = xa.abs()
        aq = (p * xabs).sum(-1, keepdim=True)                                           # A_q
        o.mag_s, o.Dq, o.mag_o = mag_s, dq_, _rows(p @ v.abs(), B, t)          # per logit; per query; sum_k p_k |v_kd| per output
        o.b_out = SECOND * _rows((2 * dq_ + (C_F + aq) * U) * (p @ v.abs()) + U * ((p * xabs) @ v.abs()), B, t)
    if not backward:
        return o
    do = _heads(c.dout.to(dt), B, t, H)
    dP = do @ v.transpose(-1, -2)
    Di = (p * dP).sum(-1, keepdim=True)
    Dm = Di
    irow = min(QT - 1, t - 1)                                                            # the last row of query tile 0
    if mut == "no_Di_row":
        Dm = Di.clone()
        Dm[:, :, irow] = 0
    dS = p * (dP - Dm)
    w = torch.ones(t, J, dtype=dt)
    if mut == "drop_slab":                                                               # one of a key's partial dK / dV contributions (slab slot 1, or 0)
        slot = 1 if t > QT else 0
        w = (((ii >> 5) - ((torch.arange(J).view(1, J) - (J - t)) >> 5)) != slot).to(dt)
    dQ = (dS @ k) * scale
    dK = (((dS * w).transpose(-1, -2) @ q) * scale)[:, :, J - t:]
    dV = ((p * w).transpose(-1, -2) @ do)[:, :, J - t:]
    g = torch.zeros(B * t, c.ld, dtype=dt)
    g[:, :hid], g[:, hid:2 * hid], g[:, 2 * hid:3 * hid] = _rows(dQ, B, t), _rows(dK, B, t), _rows(dV, B, t)

    def per_offset(z):                                                                   # [10, t, J] -> [10, maxlen]: summed over the pairs of an offset
        out = torch.zeros(10, ml, dtype=z.dtype)
        return out.index_add_(1, (ml + ii - jj).clamp(0, ml - 1).reshape(-1), (z * inband.to(z.dtype)).reshape(10, -1))

    if c.causal:
        g[:, 3 * hid:3 * hid + 10 * H] = _rows(torch.einsum("bhij,nij->bhin", dS, bm), B, t)
        dS2 = dS
        if mut == "dbnd_missing_tile":
            dS2 = dS.clone()
            dS2[0, 0, :QT] = 0
        o.db = per_offset(torch.einsum("bhij,bhin->nij", dS2, r))
    o.dqkvr = g
    if ref:
        eta = 2 * dq_ + (C_P + 1 + xabs + aq) * U
        e_dp = C_DP * U * (do.abs() @ v.abs().transpose(-1, -2))
        e_di = (p * (eta * dP.abs() + e_dp)).sum(-1, keepdim=True) + C_DI * U * (p * dP.abs()).sum(-1, keepdim=True)
        e_ds = p * (eta * (dP - Di).abs() + e_dp + e_di + 2 * U * (dP.abs() + Di.abs()))
        a_s = dS.abs()
        bg = torch.zeros(B * t, c.ld, dtype=D)
        bg[:, :hid] = _rows((e_ds @ k.abs() + C_DQ * U * (a_s @ k.abs())) / DH, B, t)
        bg[:, hid:2 * hid] = _rows(((e_ds.transpose(-1, -2) @ q.abs() + C_SLAB * U * (a_s.transpose(-1, -2) @ q.abs())) / DH)[:, :, J - t:], B, t)
        bg[:, 2 * hid:3 * hid] = _rows(((p * eta).transpose(-1, -2) @ do.abs() + C_SLAB * U * (p.transpose(-1, -2) @ do.abs()))[:, :, J - t:], B, t)
        if c.causal:
            bg[:, 3 * hid:3 * hid + 10 * H] = _rows(torch.einsum("bhij,nij->bhin", e_ds, bm.abs()) + (ml + 1) * U * torch.einsum("bhij,nij->bhin", a_s, bm.abs()), B, t)
            rows = B * H * ((t + QT - 1) // QT)
            o.b_db = SECOND * (per_offset(torch.einsum("bhij,bhin->nij", e_ds, r.abs())) + (QT + rows) * U * per_offset(torch.einsum("bhij,bhin->nij", a_s, r.abs())))
        o.b_dqkvr = SECOND * bg
    return o


def out_bound(o, fmt):
    """The forward bound of a 16-bit output: one ulp of the format at the reference value + the fp32 part."""
    return ulp16(o.out, fmt) + o.b_out


def step_ref(c, first):
    """The t = 1 step (ops.masked_attention_step) on a case whose memvalid holds the STATE mask: -> (compute() of the case with memvalid = state_mask &
    ~first, next kmem, next vmem, next mask uint8 [B, maxlen]) -- the memory shifted one row up with the new K / V row appended, bit for bit."""
    mv = (c.memvalid.bool() & ~first.bool().view(-1, 1)).to(torch.uint8)
    o = compute(SimpleNamespace(**{**vars(c), "memvalid": mv, "qlo": None}), backward=False)
    hid = c.hid
    kout = torch.cat([c.kmem[:, 1:], c.qkvr[:, hid:2 * hid].view(c.B, 1, hid)], 1)
    vout = torch.cat([c.vmem[:, 1:], c.qkvr[:, 2 * hid:3 * hid].view(c.B, 1, hid)], 1)
    mout = torch.cat([mv[:, 1:], torch.ones(c.B, 1, dtype=torch.uint8)], 1)
    return o, kout, vout, mout


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------------
def ld_of(heads):
    """3 hid + 10 heads rounded up to a multiple of 4 (the banded backward's requirement): heads = 1 and 3 get padding columns."""
    return (3 * heads * DH + 10 * heads + 3) // 4 * 4


def _first(b, t, where):
    f = torch.zeros(b, t, dtype=torch.bool)
    for row, ps in (where or {}).items():
        for pp in ps:
            f[row, pp] = True
    return f


def _shell(B, t, maxlen, heads, where, causal=True):
    hid = heads * DH
    c = SimpleNamespace(B=B, t=t, maxlen=maxlen, heads=heads, hid=hid, ld=ld_of(heads) if causal else 3 * hid, causal=causal, qlo=None, where=where)
    if where:
        c.first = _first(B, t, where)
        c.qlo = qlo_of(c.first, maxlen)
    return c


def real_case(B, t, maxlen, heads, where=None, seed=0, causal=True):
    """Instrument B's inputs: today's tests' distributions; the padding columns of qkvr hold nonzero values."""
    g = torch.Generator().manual_seed(1000 + seed)
    c = _shell(B, t, maxlen, heads, where, causal)
    c.qkvr = torch.randn(B * t, c.ld, generator=g)
    c.qkvr[:, :c.hid] *= 2.0
    c.dout = torch.randn(B * t, c.hid, generator=g)
    if causal:
        c.kmem, c.vmem = torch.randn(B, maxlen, c.hid, generator=g), torch.randn(B, maxlen, c.hid, generator=g)
        c.memvalid = (torch.rand(B, maxlen, generator=g) > 0.3).to(torch.uint8)
        c.b_nd = 0.5 * torch.randn(10, maxlen, generator=g)
    return c


RULES = ["oldest", "self", "lastmem", "firstchunk", "slot127", "slot128", "slot159", "random"]
PAIRS = [("oldest", "self"), ("lastmem", "firstchunk"), ("slot127", "slot128"), ("slot159", "random"), ("random", "random")]
EXACT_RUNS = [("onehot", i) for i in range(len(RULES))] + [("tie", i) for i in range(len(PAIRS))] + [("bias", 0)]


def _code(j, h):
    return (j + 37 * h) % DH


def exact_case(B, t, maxlen, heads, where=None, family="onehot", rule=0, seed=0, causal=True):
    """Instrument A's inputs (module docstring).  rule: index into RULES ("onehot": every query aims at that key of its band where it is visible, else at a
    random visible key) or PAIRS ("tie").  c.targets[b][h][i] lists the key rows that hold the weight."""
    g = torch.Generator().manual_seed(2000 + seed)
    rng = np.random.RandomState(seed + 17 * rule)
    c = _shell(B, t, maxlen, heads, where, causal)
    hid, ml = c.hid, maxlen
    c.qkvr = L.ints(g, B * t, c.ld)                     # V, and nonzero padding
    c.dout = L.ints(g, B * t, hid)
    J = ml + t if causal else t
    if causal:
        c.vmem = L.ints(g, B, ml, hid)
        c.memvalid = (torch.rand(B, ml, generator=g) > 0.3).to(torch.uint8)
        c.memvalid[:, -1] = 1                           # the last memory row is one of the targets
        c.b_nd = L.ints(g, 10, ml)
    c.qkvr[:, :hid] = 0
    c.qkvr[:, 3 * hid:3 * hid + 10 * heads] = 0
    if family == "bias":
        assert causal
        c.kmem = L.ints(g, B, ml, hid)
        c.b_nd = torch.zeros(10, ml)
        others = [ml - 1, 1, 127, 2, ml - 2, 64, 63, 3, 31, 32]
        for n in range(10):
            c.b_nd[n, 0] = 1.0
            if 0 < others[n] < ml:
                c.b_nd[n, others[n]] = 1.0
        for h in range(heads):
            for i in range(t):
                c.qkvr[i::t, 3 * hid + 10 * h + (i + h) % 10] = 128.0
        return c
    kfull = torch.zeros(B, J, heads, DH)
    for h in range(heads):
        kfull[:, torch.arange(J), h, _code(torch.arange(J), h)] = 128.0
    if causal:
        kfull[:, :ml][c.memvalid == 0] = 128.0          # an invalid memory row matches EVERY query
        c.kmem = kfull[:, :ml].reshape(B, ml, hid).contiguous()
    c.qkvr[:, hid:2 * hid] = kfull[:, J - t:].reshape(B * t, hid)
    names = (RULES[rule],) if family == "onehot" else PAIRS[rule]
    c.targets = [[[None] * t for _ in range(heads)] for _ in range(B)]
    for b in range(B):
        for i in range(t):
            if causal:
                lo = max(i + 1, int(c.qlo[b, i]) if c.qlo is not None else 0)
                visible = [j for j in range(lo, i + ml + 1) if j >= ml or c.memvalid[b, j]]
                q0 = i & ~(QT - 1)
                cand = dict(oldest=i + 1, self=i + ml, lastmem=ml - 1, firstchunk=ml, slot127=q0 + 128, slot128=q0 + 129, slot159=q0 + 160)
                decoy = lo - 1 if lo - 1 >= i + 1 else None          # the row just below qlo[i], inside the band
            else:
                visible = list(range(t))
                cand = dict(oldest=0, self=i, lastmem=t - 1, firstchunk=(i + 1) % t, slot127=127, slot128=128, slot159=159)
                decoy = None
            for h in range(heads):
                tg = []
                for nm in names:
                    j = cand.get(nm)
                    if j is None or j not in visible or j in tg:
                        rest = [jv for jv in visible if jv not in tg]
                        j = rest[rng.randint(len(rest))] if rest else None
                    if j is not None:
                        tg.append(j)
                pick = lambda cs_: [j for j in visible if _code(j, h) in cs_]
                codes = {_code(j, h) for j in tg}
                cs = codes | ({_code(decoy, h)} if decoy is not None else set())
                if len(pick(cs)) not in (1, 2):                      # the decoy's code is also a visible row's (maxlen = 129): no decoy
                    cs = codes
                if len(pick(cs)) not in (1, 2):                      # rows 128 apart share a code: fall back to the query's own key (+ its twin)
                    cs = {_code(visible[-1], h)}
                tg = pick(cs)
                for cd in cs:
                    c.qkvr[b * t + i, h * DH + cd] = 128.0
                c.targets[b][h][i] = tg
    return c


# ---- comparison helpers -------------------------------------------------------------------------------------------------------------------------------------
def describe(c, kind, idx):
    """Names an element of "out" ([B*t, hid]), "dqkvr" ([B*t, ld]: dQ | dK | dV | dR | padding) or "db" (db_nd [10, maxlen])."""
    if kind == "db":
        return f"b_nd row n = {idx[0]}, band offset {idx[1]} (0 = the query itself, {c.maxlen - 1} = the oldest key)"
    row, col = idx
    b, i = row // c.t, row % c.t
    hid = c.hid
    if kind == "out":
        blk, cc = "out", col
    else:
        blk, cc = ("dQ", col) if col < hid else ("dK", col - hid) if col < 2 * hid else ("dV", col - 2 * hid) if col < 3 * hid else ("dR", col - 3 * hid)
    if blk == "dR":
        where = f"head {cc // 10}, n = {cc % 10}" if cc < 10 * c.heads else f"padding column {col}"
    else:
        where = f"head {cc // DH}, d = {cc % DH}"
    pos = f"row {i} (tile {i // QT}, position {i % QT} in tile)"
    if blk in ("dK", "dV"):
        extra = f" = row {c.maxlen + i} of [memory ; chunk], at band offset o for query {i} + o" if c.causal else ""
        return f"sequence {b}, {blk}, key {pos}{extra}, {where}"
    aims = ""
    if hasattr(c, "targets") and cc < c.heads * (10 if blk == "dR" else DH):          # an exact case: where this query's weight sits
        tg = c.targets[b][cc // (10 if blk == "dR" else DH)][i]
        aims = f"; its weight is on rows {tg} of [memory ; chunk]" + (f" = band offsets {[c.maxlen + i - j for j in tg]}" if c.causal else "")
    return f"sequence {b}, {blk}, query {pos}, {where}{aims}"


def blocks(c):
    """[(name, column slice)] of dqkvr."""
    hid = c.hid
    res = [("dQ", slice(0, hid)), ("dK", slice(hid, 2 * hid)), ("dV", slice(2 * hid, 3 * hid))]
    return res + ([("dR", slice(3 * hid, c.ld))] if c.ld > 3 * hid else [])


def worst(got, want, bnd):
    """-> (worst err / bound over ALL elements, index of the worst, number beyond the bound).  err = 0 counts as ratio 0 also under a zero bound."""
    err = (got.to(D) - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    ratio = torch.where(torch.isfinite(got.to(D)), ratio, torch.full_like(ratio, math.inf))
    flat = int(ratio.argmax())
    idx = tuple(int(v) for v in np.unravel_index(flat, tuple(ratio.shape)))
    return float(ratio.reshape(-1)[flat]), idx, int((~(ratio <= 1.0)).sum())


def check(c, name, kind, got, want, bnd):
    """-> (worst ratio, None or a message naming the worst element)."""
    if tuple(got.shape) != tuple(want.shape):
        return math.inf, f"{name}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    w, idx, n = worst(got, want, bnd)
    if w <= 1.0:
        return w, None
    return w, (f"{name}: {n} of {got.numel()} elements beyond the bound, worst err / bound = {w:.3f} at {idx}: {describe(c, kind, idx)}; "
               f"got {float(got[idx])!r}, fp64 {float(want[idx])!r}, bound {float(bnd[idx]):.3e}")


def check_exact(c, name, kind, got, want):
    """None when `got` equals the exact values rounded ONCE to got's dtype, element for element (by value: -0.0 == 0.0), else a message."""
    if tuple(got.shape) != tuple(want.shape):
        return f"{name}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    bad = ~(got.to(D) == want.to(got.dtype).to(D))
    if not bool(bad.any()):
        return None
    idx = tuple(int(v) for v in bad.nonzero()[0])
    return (f"{name}: {int(bad.sum())} of {got.numel()} elements differ from the exact values, first at {idx}: {describe(c, kind, idx)}; "
            f"got {float(got[idx])!r}, exact {float(want[idx])!r}")


# ---- the shapes both test modules use -----------------------------------------------------------------------------------------------------------------------
#         B  t    maxlen heads  episode starts of the "with qlo" variant
SHAPES = [(1, 1, 1, 1, {0: [0]}),
          (1, 32, 128, 1, {0: [13]}),
          (2, 33, 129, 2, {0: [16], 1: [0, 32]}),                # the band fills all 160 staged key slots, b_nd all 10 * 129 floats of LDS
          (2, 70, 128, 2, {0: [31, 32, 33], 1: [0, 69]}),        # starts around a query-tile edge, at the first and at the last frame
          (1, 200, 128, 2, {0: [150]}),                          # fifth key tile, five slabs per key
          (2, 40, 16, 2, {0: [5, 20], 1: [5, 20]}),
          (1, 40, 128, 3, {0: [7, 33]})]                         # ld = 1182 padded to 1184
STEP_MAXLENS = [1, 2, 37, 63, 64, 65, 128]
NONE_TS = [1, 12, 33, 160]


def ratios(c, o, out16, dqkvr, db, fmt):
    """{output: worst err / bound} and the failure messages of one run against the reference o (any of the three may be None)."""
    res, msgs = {}, []
    if out16 is not None:
        res["out"], m = check(c, f"out ({fmt})", "out", out16, o.out, out_bound(o, fmt))
        msgs += [m] if m else []
    if dqkvr is not None:
        _, m = check(c, "dqkvr", "dqkvr", dqkvr, o.dqkvr, o.b_dqkvr)
        msgs += [m] if m else []
        for nm, sl in blocks(c):
            res[nm] = worst(dqkvr[:, sl], o.dqkvr[:, sl], o.b_dqkvr[:, sl])[0]
    if db is not None:
        res["db_nd"], m = check(c, "db_nd", "db", db, o.db, o.b_db)
        msgs += [m] if m else []
    return res, msgs


def exact_failures(c, o, out16, dqkvr, db):
    """Messages of instrument A for one run against o = compute(c, flush=True)."""
    msgs = []
    for nm, kind, got, want in (("out", "out", out16, o.out), ("dqkvr", "dqkvr", dqkvr, getattr(o, "dqkvr", None)), ("db_nd", "db", db, getattr(o, "db", None))):
        if got is not None:
            m = check_exact(c, nm, kind, got, want)
            msgs += [m] if m else []
    return msgs
