"""Packed-document / sliding-window attention masks without a GPU: the row ranges of
``hnn.attention_bounds`` against the dense mask of the definition, the fp64 oracle's ``doc_ids`` /
``window`` against per-document runs, the SDPA fallback of ``hnn.attention`` against the oracle,
and the models' ``doc_ids`` argument.

Definition (self-attention of S tokens): query i sees key j iff both lie in the same document (a
maximal run of equal consecutive ``doc_ids``), |i - j| < window, j <= i under causal, and
j < kv_len[b]."""
import math

import pytest
import torch

from hipps.models import transformer as tf
from hipps.ops import nn as hnn
from hipps.ops import reference as ref


def _random_doc_ids(B, S, g, max_run):
    """[B, S] ids from random run lengths in 1 .. max_run; values neither sorted nor unique."""
    rows = []
    for _ in range(B):
        row = []
        while len(row) < S:
            n = int(torch.randint(1, max_run + 1, (1,), generator=g))
            val = int(torch.randint(0, 5, (1,), generator=g))
            if row and row[-1] == val:
                val += 7  # (a new run needs a new value)
            row += [val] * n
        rows.append(row[:S])
    return torch.tensor(rows)


def _dense(doc_ids, S, window, causal):
    """bool [B, S, S] straight from the definition: the run of every token counted one token at a
    time, then the three conditions on all (i, j)."""
    B = 1 if doc_ids is None else doc_ids.shape[0]
    runs = torch.zeros(B, S, dtype=torch.long)
    for b in range(B):
        ids = [0] * S if doc_ids is None else doc_ids[b].tolist()
        for j in range(1, S):
            runs[b, j] = runs[b, j - 1] + (ids[j] != ids[j - 1])
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    m = runs[:, :, None] == runs[:, None, :]
    if window is not None:
        m = m & ((i - j).abs() < window)
    if causal:
        m = m & (j <= i)
    return m


# ------------------------------------------------------------------ 1. ranges vs the dense mask
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S", [1, 5, 64, 130])
def test_ranges_equal_the_dense_mask(S, causal):
    g = torch.Generator().manual_seed(100 + S + causal)
    j = torch.arange(S)
    cases = [(None, w) for w in (1, 2, 7, S, 3 * S)]
    for max_run in (1, 3, max(1, S // 3), S):
        d = _random_doc_ids(3, S, g, max_run)
        cases += [(d, w) for w in (None, 1, 2, 7, S, 3 * S)]
    for doc_ids, window in cases:
        bd = hnn.attention_bounds(S, doc_ids=doc_ids, window=window, causal=causal)
        want = _dense(doc_ids, S, window, causal)
        B = want.shape[0]
        for t in bd[:4]:
            assert t.dtype == torch.int32 and t.shape == (B, S) and t.stride(1) == 1
            assert (t[:, 1:] >= t[:, :-1]).all(), "not non-decreasing"
        from_k = (j[None, None, :] >= bd.klo[:, :, None]) & (j[None, None, :] < bd.khi[:, :, None])
        from_q = (j[None, :, None] >= bd.qlo[:, None, :]) & (j[None, :, None] < bd.qhi[:, None, :])
        assert torch.equal(from_k, want), (window, "klo / khi")
        assert torch.equal(from_q, want), (window, "qlo / qhi")
        assert torch.equal(bd.dense_mask(), want), (window, "dense_mask")
        assert bd.causal == causal and bd.window == window


# ------------------------------------------------- 2. oracle with doc_ids vs per-document runs
@pytest.mark.parametrize("causal", [False, True])
def test_oracle_documents_equal_separate_runs(causal):
    g = torch.Generator().manual_seed(7 + causal)
    B, S, Hq, Hkv, D = 2, 40, 4, 2, 16
    lens = [[1, 17, 22], [13, 8, 19]]
    doc_ids = torch.tensor([sum(([i % 2] * n for i, n in enumerate(row)), []) for row in lens])  # 0 1 0: any change
    q, dout = (torch.randn(B, S, Hq, D, generator=g, dtype=torch.float64) for _ in range(2))
    k, v = (torch.randn(B, S, Hkv, D, generator=g, dtype=torch.float64) for _ in range(2))
    full = ref.attention(q, k, v, dout, causal, doc_ids=doc_ids)
    for b in range(B):
        a = 0
        for n in lens[b]:
            sl = slice(a, a + n)
            one = ref.attention(q[b:b + 1, sl], k[b:b + 1, sl], v[b:b + 1, sl], dout[b:b + 1, sl], causal)
            for name, x, y in zip(("o", "lse", "dq", "dk", "dv"), full, one):
                x = x[b:b + 1, :, sl] if name == "lse" else x[b:b + 1, sl]
                torch.testing.assert_close(x, y, rtol=0, atol=1e-12, msg=lambda m, nm=name: nm + ": " + m)
            a += n


# ----------------------------------------------------------------- 3. fallback vs the oracle
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("window,docs,kv_len", [(None, True, None), (5, False, None), (9, True, None),
                                                (None, True, [37, 20]), (6, True, [30, 37])])
def test_fallback_matches_the_oracle(window, docs, kv_len, causal):
    g = torch.Generator().manual_seed(11)
    B, S, Hq, Hkv, D = 2, 37, 4, 2, 16
    doc_ids = torch.tensor([[0] * 10 + [1] * 20 + [2] * 7, [3] * 1 + [4] * 21 + [3] * 15]) if docs else None
    q, k, v, dout = (torch.randn(B, S, h, D, generator=g) for h in (Hq, Hkv, Hkv, Hq))
    bd = hnn.attention_bounds(S, doc_ids=doc_ids, window=window, causal=causal)
    assert not hnn.attention_ok(q, k, v, causal, bd)  # fp32 host tensors: the SDPA route
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32)
    o = hnn.attention(qa, ka, va, causal=causal, kv_len=kl, bounds=bd)
    o.backward(dout)
    want = ref.attention(q, k, v, dout, causal, kl, doc_ids=doc_ids, window=window)
    if kv_len is not None and not causal:
        assert (want[1] == math.inf).any()  # (rows with no key: a document wholly in the padding)
    for name, x, y in zip(("o", "dq", "dk", "dv"), (o, qa.grad, ka.grad, va.grad), (want[0],) + want[2:]):
        torch.testing.assert_close(x, y.float(), rtol=1e-5, atol=1e-5, msg=lambda m, nm=name: nm + ": " + m)


# ------------------------------------------------------------------------------- 4. models
def _two_docs(S=48, cut=20):
    return torch.tensor([[0] * cut + [1] * (S - cut)] * 2), cut


def test_llama_documents_are_isolated():
    torch.manual_seed(0)
    m = tf.Llama(tf.LlamaConfig(vocab=512, dim=64, layers=2, heads=4, kv_heads=2, ffn=128, max_seq=128)).eval()
    doc_ids, cut = _two_docs()
    ids = torch.randint(0, 512, (2, 48))
    ids2 = ids.clone()
    ids2[:, :cut] = torch.randint(0, 512, (2, cut))
    assert not torch.equal(ids, ids2)
    with torch.no_grad():
        a, b = m(ids, doc_ids=doc_ids), m(ids2, doc_ids=doc_ids)
        c, d = m(ids), m(ids2)
    assert (a[:, cut:] - b[:, cut:]).abs().max() <= 1e-5
    assert (a[:, :cut] - b[:, :cut]).abs().max() > 1e-3
    assert (c[:, cut:] - d[:, cut:]).abs().max() > 1e-3
    assert (a[:, cut:] - c[:, cut:]).abs().max() > 1e-3  # (the mask matters)


def test_llama_window_limits_the_reach():
    torch.manual_seed(0)
    kw = dict(vocab=512, dim=64, layers=2, heads=4, kv_heads=2, ffn=128, max_seq=128)
    m = tf.Llama(tf.LlamaConfig(window=4, **kw)).eval()
    ids = torch.randint(0, 512, (2, 48))
    ids2 = ids.clone()
    ids2[:, :10] = torch.randint(0, 512, (2, 10))
    with torch.no_grad():
        a, b = m(ids), m(ids2)
    # 2 layers of window 4 reach 6 tokens back: position 9 is out of sight from 16 on
    assert (a[:, 16:] - b[:, 16:]).abs().max() <= 1e-5
    assert (a[:, 10:16] - b[:, 10:16]).abs().max() > 1e-3


def test_bert_documents_are_isolated():
    torch.manual_seed(0)
    m = tf.Bert(tf.BertConfig(vocab=512, hidden=64, layers=2, heads=4, ffn=128, max_pos=64)).eval()
    doc_ids, cut = _two_docs()
    ids = torch.randint(0, 512, (2, 48))
    ids2 = ids.clone()
    ids2[:, :cut] = torch.randint(0, 512, (2, cut))
    with torch.no_grad():
        a, b = m(ids, doc_ids=doc_ids), m(ids2, doc_ids=doc_ids)
        c, d = m(ids), m(ids2)
        e = m(ids, kv_len=torch.tensor([48, 40]), doc_ids=doc_ids)
    assert (a[:, cut:] - b[:, cut:]).abs().max() <= 1e-5
    assert (a[:, :cut] - b[:, :cut]).abs().max() > 1e-3
    assert (c[:, cut:] - d[:, cut:]).abs().max() > 1e-3
    assert torch.isfinite(e).all() and torch.equal(e[0], a[0]) and not torch.equal(e[1], a[1])


# ----------------------------------------------------------------------------- 5. defaults
def test_defaults_and_argument_errors():
    assert hnn.attention_bounds(16) is None
    assert hnn.attention_bounds(16, causal=True, batch=2) is None
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, 16, 2, 8, generator=g) for _ in range(3))
    bd = hnn.attention_bounds(16, window=4, causal=True)
    assert bd.klo.shape == (1, 16)  # a window alone: one row for every batch
    with pytest.raises(ValueError, match="causal"):
        hnn.attention(q, k, v, causal=False, bounds=bd)
    with pytest.raises(ValueError, match="causal"):
        hnn.attention_qkv(torch.stack((q, k, v), 2), causal=False, bounds=bd)
    with pytest.raises(ValueError, match="causal"):
        hnn.rope_attention_packed(torch.cat((q, k, v), 2).flatten(2), None, None, 2, 2, causal=False, bounds=bd)
    with pytest.raises(ValueError, match="window"):
        hnn.attention_bounds(16, window=0)
    with pytest.raises(ValueError, match="doc_ids"):
        hnn.attention_bounds(16, doc_ids=torch.zeros(2, 15, dtype=torch.long))
    with pytest.raises(ValueError, match="bounds"):
        hnn.attention(q[:, :8], k[:, :8], v[:, :8], causal=True, bounds=bd)  # 16-token bounds, 8 tokens
    with pytest.raises(AttributeError):
        bd.window = 5  # immutable
    # bounds are self-attention only: the gate rejects Sq != Sk
    assert not hnn.attention_ok(q[:, :8], k, v, False, hnn.attention_bounds(16, window=4))
    # without bounds nothing changes: the same call, the same bits
    assert torch.equal(hnn.attention(q, k, v, causal=True), hnn.attention(q, k, v, causal=True, bounds=None))
    assert torch.equal(hnn.attention(q, k, v, causal=True, bounds=hnn.attention_bounds(16, window=16, causal=True)),
                       hnn.attention(q, k, v, causal=True, bounds=hnn.attention_bounds(16, window=99, causal=True)))
