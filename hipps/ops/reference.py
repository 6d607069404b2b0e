"""Pure-PyTorch reference implementations of every hipps kernel.

Two roles:
  * the CPU backend (gloo plumbing tests, BASELINE config 1 "MLP sync PS on CPU");
  * the numerics oracle the GPU kernel tests compare against (fp32 torch math; fp64 for
    attention, with a mode that rounds to bf16 where csrc/attn.hip does).

Semantics mirror the HIP kernels exactly (rank-ordered sums, reference SGD/Adam formulas from
/root/reference/ps.py:197-261, 256-element int8 blocks, exact top-k with lowest-index tie
break, ascending index order).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

QBLOCK = 256


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.float()


def aggregate(slots: Sequence[torch.Tensor], acc: torch.Tensor, gscale: float = 1.0, accumulate: bool = False):
    if accumulate:  # each message added on its own (batch-invariant; csrc/flat.hip k_aggregate)
        for s in slots:
            acc.add_(_f32(s) * gscale if gscale != 1.0 else _f32(s))
        return
    d = _f32(slots[0]).clone()
    for s in slots[1:]:  # rank order (ps.py:176 `sum(grads)`)
        d += _f32(s)
    if gscale != 1.0:
        d *= gscale
    if accumulate:
        acc += d
    else:
        acc.copy_(d)


def convert(src: torch.Tensor, dst: torch.Tensor, scale: float = 1.0):
    x = _f32(src)
    if scale != 1.0:
        x = x * scale
    dst.copy_(x.to(dst.dtype))


def _elem_mask(mask, n):
    """Chunk mask (one byte per 16 elements) -> per-element bool."""
    return mask.bool().repeat_interleave(16)[:n]


def _masked(mask, n, fn, *bufs):
    """Run ``fn`` and restore the elements of ``bufs`` whose chunk mask byte is 0."""
    if mask is None:
        return fn()
    keep = ~_elem_mask(mask, n)
    saved = [b[keep].clone() if b is not None else None for b in bufs]
    fn()
    for b, s in zip(bufs, saved):
        if b is not None:
            b[keep] = s


def _chunk_groups(mask, csteps, key):
    """Split the chunks this step updates (mask byte != 0, or all) by ``key(count)`` -> list of
    (key value, chunk mask) so each group runs the scalar-hyper-parameter formula."""
    live = torch.ones_like(csteps, dtype=torch.bool) if mask is None else mask[: csteps.numel()].to(torch.bool)
    keys = key(csteps)
    out = []
    for kv in sorted(set(keys[live].tolist())):
        out.append((kv, (live & (keys == kv)).to(torch.uint8)))
    return live, out


def sgd_step(grads, p, buf=None, pub=None, zero_src=False, gscale=1.0, lr=0.0, weight_decay=0.0, momentum=0.0,
             dampening=0.0, nesterov=False, first=False, mask=None, csteps=None, lookahead=0.0):
    """Reference SGD (ps.py:197-214) on flat fp32 buffers; masked chunks are left untouched.
    ``csteps``: per-chunk update counts -- first step (buf = d_p) where the count is 0.
    ``lookahead`` c: the published copy is ``p - c * buf``."""
    if lookahead:
        sgd_step(grads, p, buf, None, zero_src, gscale, lr, weight_decay, momentum, dampening, nesterov, first, mask,
                 csteps)
        if pub is not None:
            pub.copy_(p.add(buf, alpha=-lookahead).to(pub.dtype))
        return
    if csteps is not None:
        live, groups = _chunk_groups(mask, csteps, lambda c: (c == 0).to(torch.int32))
        for is_first, m in groups:
            sgd_step(grads, p, buf, None, False, gscale, lr, weight_decay, momentum, dampening, nesterov,
                     bool(is_first), m)
        csteps[live] += 1
        if zero_src:
            grads[0].zero_()
        if pub is not None:
            pub.copy_(p.to(pub.dtype))
        return
    if mask is not None:
        _masked(mask, p.numel(), lambda: sgd_step(grads, p, buf, None, zero_src, gscale, lr, weight_decay, momentum,
                                                  dampening, nesterov, first), p, buf)
        if pub is not None:
            pub.copy_(p.to(pub.dtype))
        return
    d = _f32(grads[0]).clone()
    for g in grads[1:]:
        d += _f32(g)
    if gscale != 1.0:
        d *= gscale
    if zero_src:
        grads[0].zero_()
    if weight_decay != 0:
        d = d.add(p, alpha=weight_decay)
    if momentum != 0:
        if first:
            buf.copy_(d)
        else:
            buf.mul_(momentum).add_(d, alpha=1 - dampening)
        d = d.add(buf, alpha=momentum) if nesterov else buf
    p.add_(d, alpha=-lr)
    if pub is not None:
        pub.copy_(p.to(pub.dtype))


def adam_step(grads, p, exp_avg, exp_avg_sq, max_exp_avg_sq=None, pub=None, zero_src=False, gscale=1.0, lr=1e-3,
              betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1, amsgrad=False, torch_mode=False, mask=None,
              csteps=None):
    """Reference Adam (ps.py:217-261): denom = sqrt(v) + eps; step = lr*sqrt(bc2)/bc1.
    ``csteps``: per-chunk update counts -- each chunk is corrected for its own t = count + 1."""
    if csteps is not None:
        live, groups = _chunk_groups(mask, csteps, lambda c: c + 1)
        for t, m in groups:
            adam_step(grads, p, exp_avg, exp_avg_sq, max_exp_avg_sq, None, False, gscale, lr, betas, eps,
                      weight_decay, int(t), amsgrad, torch_mode, m)
        csteps[live] += 1
        if zero_src:
            grads[0].zero_()
        if pub is not None:
            pub.copy_(p.to(pub.dtype))
        return
    if mask is not None:
        _masked(mask, p.numel(), lambda: adam_step(grads, p, exp_avg, exp_avg_sq, max_exp_avg_sq, None, zero_src,
                                                   gscale, lr, betas, eps, weight_decay, step, amsgrad, torch_mode),
                p, exp_avg, exp_avg_sq, max_exp_avg_sq)
        if pub is not None:
            pub.copy_(p.to(pub.dtype))
        return
    g = _f32(grads[0]).clone()
    for x in grads[1:]:
        g += _f32(x)
    if gscale != 1.0:
        g *= gscale
    if zero_src:
        grads[0].zero_()
    b1, b2 = betas
    if weight_decay != 0:
        g = g.add(p, alpha=weight_decay)
    exp_avg.mul_(b1).add_(g, alpha=1 - b1)
    exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
    v = exp_avg_sq
    if amsgrad:
        torch.maximum(max_exp_avg_sq, exp_avg_sq, out=max_exp_avg_sq)
        v = max_exp_avg_sq
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    if torch_mode:
        denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
        step_size = lr / bc1
    else:
        denom = v.sqrt().add_(eps)
        step_size = lr * math.sqrt(bc2) / bc1
    p.addcdiv_(exp_avg, denom, value=-step_size)
    if pub is not None:
        pub.copy_(p.to(pub.dtype))


# ---- counter-based RNG identical to common.h uniform01 ------------------------------------
_M64 = (1 << 64) - 1


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def uniform01(seed: int, idx: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        h = _splitmix64(np.uint64(seed & _M64) ^ (idx.astype(np.uint64) * np.uint64(0xD1B54A32D192ED03)))
    return (h >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


# ---- dropout mask identical to common.h dropout_keep ---------------------------------------
DROP_STREAM_ATTN = 1  # attention probabilities (other dropout sites take other stream ids)


def dropout_params(p: float):
    """(threshold, p_eff) of drop probability ``p``: the mask compares 8-bit hash fields with
    threshold = round(256 p) (at most 255), so the probability in effect is p_eff = threshold /
    256 -- kernels, oracle and tests scale by 1 / (1 - p_eff).  Threshold 0: no dropout."""
    p = float(p)
    if not 0.0 <= p < 1.0:  # (NaN fails both comparisons)
        raise ValueError(f"dropout probability must be in [0, 1), got {p}")
    thr = min(255, int(math.floor(p * 256.0 + 0.5)))
    return thr, thr / 256.0


def dropout_keep(seed: int, p: float, b, h, i, j, stream: int = DROP_STREAM_ATTN) -> np.ndarray:
    """keep(seed, b, h, i, j) -> bool, broadcast over integer arrays: element (i, j) of head ``h``
    of batch row ``b`` survives dropout at probability ``p``.  A pure function of its arguments.
    One hash covers a block of 2 rows x 4 columns as eight 8-bit fields:

        head = splitmix64(splitmix64(seed) ^ (stream << 56 | b << 24 | h))
        word = splitmix64(head ^ ((i >> 1) << 32 | (j >> 2)))
        keep = ((word >> (32 (i & 1) + 8 (j & 3))) & 255) >= threshold

    (b < 2^32, h < 2^24, stream < 2^8, i, j < 2^25: disjoint bits, so no two elements share a
    field.)  common.h dropout_keep is the device twin, bit for bit."""
    thr, _ = dropout_params(p)
    b, h, i, j = (np.asarray(t).astype(np.uint64) for t in (b, h, i, j))
    u = np.uint64
    with np.errstate(over="ignore"):
        s0 = _splitmix64(np.array(int(seed) & _M64, dtype=np.uint64))
        head = _splitmix64(s0 ^ ((u(stream) << u(56)) | (b << u(24)) | h))
        word = _splitmix64(head ^ (((i >> u(1)) << u(32)) | (j >> u(2))))
        field = (word >> (u(32) * (i & u(1)) + u(8) * (j & u(3)))) & u(255)
    return field >= u(thr)


def dropout_keep_mask(seed: int, p: float, B: int, H: int, Sq: int, Sk: int) -> torch.Tensor:
    """bool [B, H, Sq, Sk] of :func:`dropout_keep` over a whole attention problem."""
    b, h, i, j = np.ogrid[:B, :H, :Sq, :Sk]
    return torch.from_numpy(np.array(np.broadcast_to(dropout_keep(seed, p, b, h, i, j), (B, H, Sq, Sk))))


def q8_encode(x, resid, q, scales, stochastic=False, seed=0):
    v = _f32(x).clone()
    if resid is not None:
        v += resid
    n = v.numel()
    nb = (n + QBLOCK - 1) // QBLOCK
    pad = nb * QBLOCK - n
    vb = torch.cat([v, v.new_zeros(pad)]).view(nb, QBLOCK)
    amax = vb.abs().amax(dim=1)
    scale = amax / 127.0
    inv = torch.where(amax > 0, 127.0 / amax, torch.zeros_like(amax))
    y = vb * inv[:, None]
    if stochastic:
        u = torch.from_numpy(uniform01(seed, np.arange(nb * QBLOCK, dtype=np.int64))).view(nb, QBLOCK)
        y = torch.floor(y + u)
    else:
        y = torch.round(y)  # rintf: round-half-even, same as torch.round
    y = y.clamp_(-127, 127).to(torch.int8)
    q.copy_(y.view(-1)[:n])
    scales.copy_(scale)
    if resid is not None:
        resid.copy_(v - y.view(-1)[:n].float() * scale.repeat_interleave(QBLOCK)[:n])


def q8_dequant(q, scales):
    n = q.numel()
    return q.float() * scales.float().repeat_interleave(QBLOCK)[:n]


def q8_aggregate(qs, ss, acc, gscale=1.0, accumulate=False):
    if accumulate:  # each message added on its own (batch-invariant; csrc/quant.hip k_q8_aggregate)
        for q, s in zip(qs, ss):
            acc.add_(q8_dequant(q, s) * gscale)
        return
    d = q8_dequant(qs[0], ss[0])
    for q, s in zip(qs[1:], ss[1:]):
        d += q8_dequant(q, s)
    if gscale != 1.0:
        d *= gscale
    if accumulate:
        acc += d
    else:
        acc.copy_(d)


# ---- MXFP4 (OCP MX: e2m1 elements, one E8M0 scale byte per 32) ---------------------------------
# This twin DEFINES the mx4 wire format; csrc/mx4.hip matches it bit for bit.
MXBLOCK = 32
MX4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mx4_encode(x, resid, q, scales):
    """scales[ceil(n/32)] (uint8, e + 127) and q[ceil(n/2)] (uint8, element 2j in the low nibble) of
    v = x (+ resid); resid <- v - deq.  Per 32-block, a = max|v| (zeros pad the last block):
    any non-finite element -> byte 255, codes 0, residual 0; a < 2^-100 -> byte 0, codes 0,
    residual v; else the smallest e <= 125 with 6 * 2^e >= a and round-to-nearest codes, ties to
    the even code.  The |v| bit patterns order like the magnitudes with Inf / NaN on top, so the
    three cases and e are read from their integer maximum."""
    v = _f32(x).clone()
    if resid is not None:
        v += resid
    n = v.numel()
    nb = (n + MXBLOCK - 1) // MXBLOCK
    vb = torch.cat([v, v.new_zeros(nb * MXBLOCK - n)]).view(nb, MXBLOCK)
    bits = vb.view(torch.int32)
    amax = (bits & 0x7FFFFFFF).amax(dim=1)
    nonfinite = amax >= 0x7F800000
    tiny = amax < (27 << 23)  # 2^-100
    normal = ~(nonfinite | tiny)
    # a = m * 2^k, m in [1, 2): e = k - 2 if m <= 1.5 else k - 1, capped so 6 * 2^e stays finite
    e = ((amax >> 23) - 127 - 2 + ((amax & 0x7FFFFF) > 0x400000).int()).clamp(max=125)
    e = torch.where(normal, e, torch.zeros_like(e))
    y = torch.ldexp(vb.abs(), -e[:, None])
    mag = ((y > 0.25).int() + (y >= 0.75).int() + (y > 1.25).int() + (y >= 1.75).int() + (y > 2.5).int()
           + (y >= 3.5).int() + (y > 5.0).int())
    sign = (bits >> 31) & 1
    code = torch.where(normal[:, None], (sign << 3) | mag, torch.zeros_like(mag))
    grid = torch.tensor(MX4_GRID, dtype=torch.float32)
    deq = torch.ldexp(torch.where(sign.bool(), -grid[mag], grid[mag]), e[:, None])  # exact
    new = torch.where(normal[:, None], vb - deq, torch.where(tiny[:, None], vb, torch.zeros_like(vb)))
    c = torch.cat([code.view(-1)[:n], code.new_zeros(n & 1)]).view(-1, 2)
    q.copy_((c[:, 0] | (c[:, 1] << 4)).to(torch.uint8))
    byte = torch.where(nonfinite, torch.full_like(e, 255), torch.where(tiny, torch.zeros_like(e), e + 127))
    scales.copy_(byte.to(torch.uint8))
    if resid is not None:
        resid.copy_(new.view(-1)[:n])


def mx4_dequant(q, scales, n):
    """fp32[n] of one message: +-GRID[code & 7] * 2^(byte - 127); byte 255 -> NaN for the block."""
    c = torch.stack([q & 15, q >> 4], dim=1).view(-1)[:n].long()
    grid = torch.tensor(MX4_GRID, dtype=torch.float32)
    val = torch.where((c & 8) != 0, -grid[c & 7], grid[c & 7])
    b = scales.to(torch.int32).repeat_interleave(MXBLOCK)[:n]
    d = torch.ldexp(val, b - 127)
    return torch.where(b == 255, torch.full_like(d, float("nan")), d)


def mx4_aggregate(qs, ss, acc, gscale=1.0, accumulate=False):
    n = acc.numel()
    g = torch.tensor(gscale, dtype=torch.float32)
    if accumulate:  # each message added on its own (batch-invariant; csrc/mx4.hip k_mx4_aggregate)
        for q, s in zip(qs, ss):
            acc.add_(mx4_dequant(q, s, n) * g)
        return
    d = mx4_dequant(qs[0], ss[0], n)
    for q, s in zip(qs[1:], ss[1:]):
        d += mx4_dequant(q, s, n)
    acc.copy_(d * g)


def topk_select(x: torch.Tensor, k: int):
    """Exact top-k by |x| with lowest-index tie break; returns ascending indices."""
    key = x.float().abs()
    # sort by (-|x|, index): stable sort on -key keeps lowest index first among equals
    order = torch.sort(-key, stable=True).indices[:k]
    return torch.sort(order).values


def topk_encode(g, resid, k, idx, val, workspace=None):
    x = _f32(g).clone()
    if resid is not None:
        x += resid
    sel = topk_select(x, k)
    idx.copy_(sel.to(torch.int32))
    v = x[sel]
    val.copy_(v.to(val.dtype))
    if resid is not None:
        resid.copy_(x)
        resid[sel] = v - val.float()


def topk_accumulate(idx, val, acc, gscale=1.0):
    acc.index_add_(0, idx.long(), val.float() * gscale)


def topk_q8_accumulate(idx, q, scales, acc, gscale=1.0):
    acc.index_add_(0, idx.long(), q8_dequant(q, scales) * gscale)


def topk_q8_residual(idx, v, q, scales, resid):
    resid.index_add_(0, idx.long(), v.float() - q8_dequant(q, scales))


def topk_workspace_bytes(n: int, k: int = 0) -> int:
    return 16


def thresh_encode(g, resid, tau, count, idx, val, workspace=None):
    """Every |x| > tau in ascending index order, at most idx.numel() of them (count in count[0])."""
    x = _f32(g).clone()
    if resid is not None:
        x += resid
    cap = idx.numel()
    sel = torch.nonzero(x.abs() > abs(tau)).view(-1)[:cap]
    count[0] = sel.numel()
    idx[: sel.numel()] = sel.to(torch.int32)
    v = x[sel]
    val[: sel.numel()] = v.to(val.dtype)
    if resid is not None:
        resid.copy_(x)
        resid[sel] = v - val[: sel.numel()].float()


def thresh_accumulate(count, idx, val, acc, gscale=1.0):
    k = min(int(count[0]), idx.numel())
    acc.index_add_(0, idx[:k].long(), val[:k].float() * gscale)


# ---- attention (csrc/attn.hip) -------------------------------------------------------------
def _bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float64)


def attention(q, k, v, dout, causal=False, kv_len=None, scale=None, emulate_bf16=False, doc_ids=None, window=None,
              dropout_p=0.0, dropout_seed=None):
    """fp64 oracle of csrc/attn.hip, forward and an explicit (no autograd) backward.

    q / dout [B, Sq, Hq, D], k / v [B, Sk, Hkv, D] (GQA by repetition: query head h reads kv head
    h // (Hq / Hkv)); ``causal`` masks key > query row, ``kv_len`` [B] masks key >= kv_len[b]
    (values above Sk behave as Sk).  Self-attention only: ``doc_ids`` [B, S] masks every key outside
    the query's document (a maximal run of equal consecutive values), ``window`` every key with
    |query - key| >= window.  Returns fp64 (o [B, Sq, Hq, D], lse [B, Hq, Sq], dq, dk, dv).
    A row with every key masked has o = 0, lse = +inf and contributes no gradient.

    ``dropout_p`` > 0 (with an integer ``dropout_seed``): dropout of the attention probabilities by
    the mask of :func:`dropout_keep`, P_drop = keep * P / (1 - p_eff) with p_eff of
    :func:`dropout_params`; o = P_drop v, lse is that of P, and with dP = dO v^T
    dS = P (keep * dP / (1 - p_eff) - delta), delta = rowsum(dO * o), dV = P_drop^T dO.  A p whose
    threshold is 0 (and the default) is the function without dropout.

    ``emulate_bf16`` rounds to bf16 where the kernels do and nowhere else: exp(s - rowmax) before
    P V (the row sum stays unrounded); exp(s - lse) before P^T dO; dS = P (dP - delta) before the
    dQ and dK products; delta from the rounded o; o / dq / dk / dv themselves (lse to fp32).  With
    dropout the same list holds, on keep * exp(s - rowmax) and keep * exp(s - lse): the kernels zero
    the dropped elements before they round, and apply 1 / (1 - p_eff) in fp32 -- to the P V and the
    P^T dO accumulators after the products, to dP before delta is subtracted -- so the scale adds no
    rounding; a one-key row's dS is then not forced to 0 (delta comes from the rounded o = v /
    (1 - p_eff), as in the kernels).  Its distance from the unrounded mode is the error a correct bf16 implementation of
    this algorithm has on the given inputs."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    sc = float(scale) if scale is not None else 1.0 / math.sqrt(D)
    rnd = _bf16_round if emulate_bf16 else (lambda t: t)
    keep, rinv = None, 1.0
    if dropout_params(dropout_p)[0] > 0:
        if dropout_seed is None:
            raise ValueError("attention: dropout_p > 0 needs a dropout_seed")
        keep = dropout_keep_mask(int(dropout_seed), dropout_p, B, Hq, Sq, Sk).to(q.device)
        rinv = 1.0 / (1.0 - dropout_params(dropout_p)[1])
    qd, dod = (t.to(torch.float64).transpose(1, 2) for t in (q, dout))                    # [B, Hq, Sq, D]
    kd, vd = (t.to(torch.float64).transpose(1, 2).repeat_interleave(G, 1) for t in (k, v))  # [B, Hq, Sk, D]
    keys = torch.arange(Sk, device=q.device)
    mask = torch.ones(B, 1, Sq, Sk, dtype=torch.bool, device=q.device)
    if causal:
        mask = mask & (keys[None, :] <= torch.arange(Sq, device=q.device)[:, None])
    if kv_len is not None:
        kl = torch.as_tensor(kv_len, device=q.device).view(B, 1, 1, 1)
        mask = mask & (keys < kl)
    if doc_ids is not None or window is not None:
        assert Sq == Sk, "doc_ids / window: self-attention only"
    if doc_ids is not None:
        d = torch.as_tensor(doc_ids, device=q.device).view(B, Sk)
        doc = torch.zeros_like(d)  # the index of each token's run
        for j in range(1, Sk):
            doc[:, j] = doc[:, j - 1] + (d[:, j] != d[:, j - 1]).to(doc.dtype)
        mask = mask & (doc[:, None, :, None] == doc[:, None, None, :])
    if window is not None:
        mask = mask & ((keys[:, None] - keys[None, :]).abs() < int(window))
    mask = mask.expand(B, Hq, Sq, Sk)
    s = (qd @ kd.transpose(-1, -2)) * sc
    live = mask.any(-1, keepdim=True)
    m = torch.where(live, s.masked_fill(~mask, -math.inf).amax(-1, keepdim=True), torch.zeros_like(s[..., :1]))
    e = torch.where(mask, torch.exp(s - m), torch.zeros_like(s))
    l = e.sum(-1, keepdim=True)
    if keep is None:
        o = torch.where(live, (rnd(e) @ vd) / l.clamp_min(1e-300), torch.zeros_like(qd))
    else:
        ed = torch.where(keep, e, torch.zeros_like(e))
        o = torch.where(live, (rnd(ed) @ vd) * rinv / l.clamp_min(1e-300), torch.zeros_like(qd))
    lse = torch.where(live, m + torch.log(l.clamp_min(1e-300)), torch.full_like(m, math.inf))
    o = rnd(o)
    if emulate_bf16:
        lse = lse.float().to(torch.float64)
    # backward: the kernels recompute P from the stored lse
    p = torch.where(mask, torch.exp(s - lse), torch.zeros_like(s))
    delta = (dod * o).sum(-1, keepdim=True)
    if keep is None:
        ds = p * (dod @ vd.transpose(-1, -2) - delta)
    else:
        dpd = torch.where(keep, (dod @ vd.transpose(-1, -2)) * rinv, torch.zeros_like(p))
        ds = p * (dpd - delta)
    # a one-key softmax is constant: dS is exactly zero there, not the rounding residue of dP - delta
    # (with dropout, kept or dropped: delta = dO . o carries the same factor as dP.  The emulation
    # keeps what it computed there: the key dropped gives exactly 0, the key kept the residue of
    # rounding o = v / (1 - p_eff) to bf16, which the kernels' delta has too)
    if keep is None or not emulate_bf16:
        ds = torch.where(mask.sum(-1, keepdim=True) == 1, torch.zeros_like(ds), ds)
    ds = rnd(ds)
    dq = (ds @ kd) * sc
    dk = (ds.transpose(-1, -2) @ qd) * sc
    if keep is None:
        dv = rnd(p).transpose(-1, -2) @ dod
    else:
        dv = (rnd(torch.where(keep, p, torch.zeros_like(p))).transpose(-1, -2) @ dod) * rinv
    dk, dv = (t.view(B, Hkv, G, Sk, D).sum(2) for t in (dk, dv))
    return (o.transpose(1, 2), lse.squeeze(-1), rnd(dq).transpose(1, 2), rnd(dk).transpose(1, 2),
            rnd(dv).transpose(1, 2))


def attention_row_error(got: torch.Tensor, want: torch.Tensor) -> float:
    """Largest per-row error of a [B, S, H, D] attention tensor, relative to the typical row:
    max_row ||got - want||_2 / RMS_row ||want||_2 with the RMS over the rows where ``want`` is not
    zero.  One wrong row shows at full size however many rows there are; rows whose own norm is
    tiny from cancellation do not inflate it.  Needs a non-zero ``want``."""
    g, w = got.to(torch.float64), want.to(torch.float64).to(got.device)
    norms = w.norm(dim=-1)
    nz = norms[norms > 0]
    assert nz.numel() > 0, "attention_row_error: the reference is identically zero"
    return ((g - w).norm(dim=-1).max() / nz.pow(2).mean().sqrt()).item()
