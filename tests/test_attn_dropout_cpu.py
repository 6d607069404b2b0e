"""Attention dropout without a GPU: the numpy twin of the mask function (hipps.ops.reference.
dropout_keep), the fp64 oracle's dropout forward / backward, the ``hipps.ops.nn`` arguments on CPU
tensors (the SDPA route) and the two models' ``attn_dropout``.

Statistical bounds are binomial, not measured: a fraction f estimated from n independent draws has
standard deviation sqrt(f (1 - f) / n); every check allows 5 of them (two-sided chance ~6e-7 per
check) with fixed seeds, so the file is deterministic.  Two independent masks with keep rate
k = 1 - p_eff agree on a fraction k^2 + p_eff^2 of their elements.  Every comparison pairs each
element at most once (even against odd indices, the upper against the lower triangle), so the
agreement indicators are independent draws under the hypothesis.
"""
import math

import numpy as np
import pytest
import torch

from hipps.ops import nn as hnn
from hipps.ops import reference as ref

SEED = 0x1234_5678_9ABC_DEF0
B, H, S = 2, 4, 368  # B * H * S * S = 1,083,392 draws
TOP = (1 << 24) - 1


def _mask(seed, p, B_=B, H_=H, Sq=S, Sk=S):
    return ref.dropout_keep_mask(seed, p, B_, H_, Sq, Sk).numpy()


def _agree_ok(a, b, p_eff):
    f = (1 - p_eff) ** 2 + p_eff ** 2
    n = a.size
    got = float((a == b).mean())
    assert abs(got - f) <= 5 * math.sqrt(f * (1 - f) / n), (got, f, n)


def test_dropout_params():
    assert ref.dropout_params(0.0) == (0, 0.0)
    assert ref.dropout_params(0.1) == (26, 26 / 256)
    assert ref.dropout_params(0.5) == (128, 0.5)
    assert ref.dropout_params(0.001) == (0, 0.0)  # rounds to threshold 0: no dropout
    assert ref.dropout_params(0.9999) == (255, 255 / 256)
    for bad in (-0.1, 1.0, 1.5, math.nan):
        with pytest.raises(ValueError):
            ref.dropout_params(bad)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p):
    _, pe = ref.dropout_params(p)
    m = _mask(SEED, p)
    n = m.size
    assert n >= 10 ** 6
    assert abs(float(m.mean()) - (1 - pe)) <= 5 * math.sqrt(pe * (1 - pe) / n)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_independence(p):
    _, pe = ref.dropout_params(p)
    m = _mask(SEED, p)
    _agree_ok(m[:, 0::2], m[:, 1::2], pe)              # adjacent heads (0, 1), (2, 3)
    _agree_ok(m[:, 1:3:2], m[:, 2::2], pe)             # ... and (1, 2)
    _agree_ok(m[0], m[1], pe)                          # two batch rows
    _agree_ok(m[:, :, 0::2], m[:, :, 1::2], pe)        # adjacent query rows: the two rows of one hash block
    _agree_ok(m[:, :, 1:-1:2], m[:, :, 2::2], pe)      # ... and across two blocks
    _agree_ok(m[..., 0::2], m[..., 1::2], pe)          # adjacent keys inside a block
    _agree_ok(m[..., 3:-1:4], m[..., 4::4], pe)        # ... and across two blocks
    _agree_ok(m, _mask(SEED + 1, p), pe)        # seeds that differ by 1
    other = ref.dropout_keep(SEED, p, *np.ogrid[:B, :H, :S, :S], stream=ref.DROP_STREAM_ATTN + 1)
    _agree_ok(m, np.broadcast_to(other, m.shape), pe)  # another stream id


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_no_aliasing(p):
    _, pe = ref.dropout_params(p)
    m = _mask(SEED, p)
    iu = np.triu_indices(S, 1)
    _agree_ok(m[:, :, iu[0], iu[1]], m[:, :, iu[1], iu[0]], pe)   # (i, j) and (j, i), i < j
    _agree_ok(m[:, :, 0::2, 1:], m[:, :, 1::2, :-1], pe)          # (i, j) and (i + 1, j - 1), i even
    _agree_ok(m[:, :, 1:-1:2, 1:], m[:, :, 2::2, :-1], pe)        # ... i odd
    # a window that ends at 2^24 - 1 in both indices, against the same window at the origin and
    # against itself transposed; b and h at large values against small ones
    n = 600
    i = (TOP - n + 1 + np.arange(n, dtype=np.int64))[:, None]
    j = (TOP - n + 1 + np.arange(n, dtype=np.int64))[None, :]
    b, h = np.arange(2)[:, None, None, None], np.arange(3)[None, :, None, None]
    top = ref.dropout_keep(SEED, p, b, h, i[None, None], j[None, None])
    low = ref.dropout_keep(SEED, p, b, h, i[None, None] - (TOP - n + 1), j[None, None] - (TOP - n + 1))
    assert top.shape == (2, 3, n, n)
    rate = float(top.mean())
    assert abs(rate - (1 - pe)) <= 5 * math.sqrt(pe * (1 - pe) / top.size)
    _agree_ok(top, low, pe)
    iu = np.triu_indices(n, 1)
    _agree_ok(top[:, :, iu[0], iu[1]], top[:, :, iu[1], iu[0]], pe)
    _agree_ok(top[:, :, 0::2, 1:], top[:, :, 1::2, :-1], pe)
    far = ref.dropout_keep(SEED, p, b + (1 << 31), h + (1 << 23), i[None, None], j[None, None])
    _agree_ok(top, far, pe)
    # b << 24 must not run into h, nor i into j: (b, h) = (1, 0) vs (0, 2^24 - 1) + ... are distinct inputs
    x = ref.dropout_keep(SEED, p, 1, 0, i, j)
    y = ref.dropout_keep(SEED, p, 0, TOP, i, j)
    _agree_ok(x, y, pe)


def test_twin_is_a_pure_function_of_its_arguments():
    """A value at (b, h, i, j) does not depend on the extent of the problem it is evaluated in."""
    big = _mask(SEED, 0.1, 2, 3, 70, 90)
    small = _mask(SEED, 0.1, 1, 2, 33, 41)
    assert np.array_equal(big[:1, :2, :33, :41], small)
    one = ref.dropout_keep(SEED, 0.1, 1, 2, 69, 89)
    assert bool(one) == bool(big[1, 2, 69, 89])


# ------------------------------------------------------------------------------------ oracle
def _inputs(Bq, Sq, Sk, Hq, Hkv, D, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(Bq, Sq, Hq, D, generator=g, dtype=torch.float64)
    k, v = (torch.randn(Bq, Sk, Hkv, D, generator=g, dtype=torch.float64) for _ in range(2))
    dout = torch.randn(Bq, Sq, Hq, D, generator=g, dtype=torch.float64)
    return q, k, v, dout


def _dense(q, k, v, dout, p, seed, causal=False, kv_len=None, doc_ids=None):
    """softmax(s) * keep / (1 - p_eff) @ v by dense fp64 ops, gradients by torch autograd."""
    Bq, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    _, pe = ref.dropout_params(p)
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    qt = q.transpose(1, 2)
    kt, vt = (t.transpose(1, 2).repeat_interleave(G, 1) for t in (k, v))
    s = qt @ kt.transpose(-1, -2) / math.sqrt(D)
    mask = torch.ones(Bq, 1, Sq, Sk, dtype=torch.bool)
    keys = torch.arange(Sk)
    if causal:
        mask = mask & (keys[None, :] <= torch.arange(Sq)[:, None])
    if kv_len is not None:
        mask = mask & (keys < torch.as_tensor(kv_len).view(Bq, 1, 1, 1))
    if doc_ids is not None:
        d = torch.as_tensor(doc_ids)
        run = torch.cat([torch.zeros_like(d[:, :1]), (d[:, 1:] != d[:, :-1]).long()], 1).cumsum(1)
        mask = mask & (run[:, None, :, None] == run[:, None, None, :])
    live = mask.any(-1, keepdim=True)
    P = torch.softmax(s.masked_fill(~(mask | ~live), -math.inf), -1)
    P = torch.where(mask, P, torch.zeros_like(P))
    keep = ref.dropout_keep_mask(seed, p, Bq, Hq, Sq, Sk)
    o = (P * keep / (1 - pe)) @ vt
    o = o.transpose(1, 2)
    o.backward(dout)
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("case", ["plain", "causal", "kv_len", "doc_ids", "gqa", "causal_gqa_kvlen"])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_oracle_backward_matches_autograd(case, p):
    Hq, Hkv = (6, 2) if "gqa" in case else (2, 2)
    Sq = Sk = 37
    if case == "plain":
        Sq, Sk = 29, 45
    kw = {}
    if "causal" in case:
        kw["causal"] = True
    if "kv_len" in case or "kvlen" in case:
        kw["kv_len"] = torch.tensor([20, 37])
    if case == "doc_ids":
        kw["doc_ids"] = torch.tensor([[0] * 10 + [1] * 27, [5] * 30 + [6] * 7])
    t = _inputs(2, Sq, Sk, Hq, Hkv, 16, seed=11)
    o, lse, dq, dk, dv = ref.attention(*t, dropout_p=p, dropout_seed=SEED, **kw)
    wo, wq, wk, wv = _dense(*t, p, SEED, **kw)
    for got, want in ((o, wo), (dq, wq), (dk, wk), (dv, wv)):
        torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)
    # lse is that of the undropped P
    lse0 = ref.attention(*t, **kw)[1]
    assert torch.equal(lse, lse0)
    assert not torch.equal(o, ref.attention(*t, **kw)[0])


def test_oracle_one_key_row_has_zero_ds():
    """A one-key row (causal row 0): dS is exactly 0 whether the key is kept or dropped."""
    t = _inputs(2, 9, 9, 2, 2, 16, seed=3)
    keep = ref.dropout_keep_mask(SEED, 0.5, 2, 2, 9, 9)
    assert keep[:, :, 0, 0].any() and not keep[:, :, 0, 0].all()  # both kinds of row 0 occur
    o, lse, dq, dk, dv = ref.attention(*t, causal=True, dropout_p=0.5, dropout_seed=SEED)
    assert torch.count_nonzero(dq[:, 0]) == 0
    wo, wq, wk, wv = _dense(*t, 0.5, SEED, causal=True)
    torch.testing.assert_close(dq, wq, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("emulate", [False, True])
def test_oracle_defaults(emulate):
    t = [x.to(torch.bfloat16) for x in _inputs(2, 33, 33, 4, 2, 16, seed=5)]
    base = ref.attention(*t, causal=True, emulate_bf16=emulate)
    for kw in ({"dropout_p": 0.0}, {"dropout_p": 0.0, "dropout_seed": 7}, {"dropout_p": 0.001, "dropout_seed": 7}):
        got = ref.attention(*t, causal=True, emulate_bf16=emulate, **kw)
        for a, b in zip(got, base):
            assert torch.equal(a, b)
    with pytest.raises(ValueError):
        ref.attention(*t, dropout_p=0.1)  # p > 0 needs a seed


# ------------------------------------------------------------------------ hipps.ops.nn on the CPU
def test_hnn_on_cpu_tensors():
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(2, 24, 4, 16, generator=g) for _ in range(3))
    base = hnn.attention(q, k, v, causal=True)
    assert torch.equal(hnn.attention(q, k, v, causal=True, dropout_p=0.0), base)
    assert torch.equal(hnn.attention(q, k, v, causal=True, dropout_p=0.0, dropout_seed=3), base)
    torch.manual_seed(5)
    a = hnn.attention(q, k, v, causal=True, dropout_p=0.3)
    assert not torch.equal(a, base)
    torch.manual_seed(5)
    assert torch.equal(hnn.attention(q, k, v, causal=True, dropout_p=0.3), a)
    qkv = torch.stack((q, k, v), dim=2)
    assert torch.equal(hnn.attention_qkv(qkv, causal=True, dropout_p=0.0), hnn.attention_qkv(qkv, causal=True))
    torch.manual_seed(5)
    assert torch.equal(hnn.attention_qkv(qkv, causal=True, dropout_p=0.3), a)
    bounds = hnn.attention_bounds(24, window=5, causal=True)
    wb = hnn.attention(q, k, v, causal=True, bounds=bounds)
    assert torch.equal(hnn.attention(q, k, v, causal=True, bounds=bounds, dropout_p=0.0), wb)
    assert not torch.equal(hnn.attention(q, k, v, causal=True, bounds=bounds, dropout_p=0.3), wb)
    for bad in (-0.1, 1.0, 2.0, math.nan):
        with pytest.raises(ValueError):
            hnn.attention(q, k, v, dropout_p=bad)
        with pytest.raises(ValueError):
            hnn.attention_qkv(qkv, dropout_p=bad)


def test_dropout_rng_state_round_trip():
    saved = hnn.dropout_rng_state()
    try:
        hnn.manual_dropout_seed(123)
        a = [hnn.next_dropout_seed() for _ in range(3)]
        assert len(set(a)) == 3 and all(0 <= s < (1 << 64) for s in a)
        hnn.manual_dropout_seed(123)
        assert [hnn.next_dropout_seed() for _ in range(3)] == a
        hnn.manual_dropout_seed(124)
        assert hnn.next_dropout_seed() != a[0]
        st = hnn.dropout_rng_state()
        b = [hnn.next_dropout_seed() for _ in range(2)]
        assert hnn.dropout_rng_state() != st
        hnn.set_dropout_rng_state(st)
        assert hnn.dropout_rng_state() == st
        assert [hnn.next_dropout_seed() for _ in range(2)] == b
    finally:
        hnn.set_dropout_rng_state(saved)


def test_ranks_seeded_alike_differ(monkeypatch):
    saved = hnn.dropout_rng_state()
    try:
        seeds = []
        for rank in ("0", "1"):
            monkeypatch.setenv("RANK", rank)
            hnn.manual_dropout_seed(99)
            seeds.append(hnn.next_dropout_seed())
        assert seeds[0] != seeds[1]
    finally:
        hnn.set_dropout_rng_state(saved)


# ------------------------------------------------------------------------------------- models
def _tiny(name, **kw):
    from hipps.models import transformer as tf

    torch.manual_seed(0)
    return tf.build(name, **kw)


@pytest.mark.parametrize("name", ["bert-tiny", "llama-tiny"])
def test_tiny_models(name):
    m0, m1 = _tiny(name), _tiny(name, attn_dropout=0.1)
    m1.load_state_dict(m0.state_dict())
    assert m1.c.attn_dropout == 0.1 and m0.c.attn_dropout == 0.0
    ids = torch.randint(0, 512, (2, 32), generator=torch.Generator().manual_seed(1))
    m0.eval(), m1.eval()
    with torch.no_grad():
        assert torch.equal(m1(ids), m0(ids))
    m1.train()
    saved, tstate = hnn.dropout_rng_state(), torch.get_rng_state()
    with torch.no_grad():
        a, b = m1(ids), m1(ids)
        assert not torch.equal(a, b)
        assert not torch.equal(a, m0(ids))
        hnn.set_dropout_rng_state(saved)
        torch.set_rng_state(tstate)  # (CPU tensors take the SDPA route: torch's generator draws the mask)
        assert torch.equal(m1(ids), a)
