"""CPU tests of the reference op semantics (the oracle the GPU kernels are checked against).

SGD/Adam are checked against independent re-statements of the reference formulas
(/root/reference/ps.py:197-214, 217-261) written out step by step here.
"""
import math

import numpy as np
import pytest
import torch

from hipps import ops
from hipps.ops import reference as ref


def _ref_sgd_loop(p, grads_seq, lr, wd, mom, damp, nesterov):
    """Literal transcription of ps.py SGD.optim_step (per-parameter state dict)."""
    state = {}
    p = p.clone()
    for d_p in grads_seq:
        d_p = d_p.clone()
        if wd != 0:
            d_p.add_(p, alpha=wd)
        if mom != 0:
            if "momentum_buffer" not in state:
                buf = state["momentum_buffer"] = torch.zeros_like(p)
                buf.mul_(mom).add_(d_p)
            else:
                buf = state["momentum_buffer"]
                buf.mul_(mom).add_(d_p, alpha=1 - damp)
            if nesterov:
                d_p = d_p.add(buf, alpha=mom)
            else:
                d_p = buf
        p.add_(d_p, alpha=-lr)
    return p


@pytest.mark.parametrize("mom,damp,nesterov,wd", [(0, 0, False, 0), (0.9, 0, False, 1e-4), (0.9, 0.1, False, 0),
                                                  (0.9, 0, True, 5e-4)])
def test_sgd_reference_matches_ps_py(mom, damp, nesterov, wd):
    torch.manual_seed(0)
    n = 1000
    p0 = torch.randn(n)
    seq = [torch.randn(n) for _ in range(4)]
    want = _ref_sgd_loop(p0, seq, 0.1, wd, mom, damp, nesterov)
    p = p0.clone()
    buf = torch.zeros(n)
    for t, g in enumerate(seq):
        ops.sgd_step([g], p, buf if mom else None, lr=0.1, weight_decay=wd, momentum=mom, dampening=damp,
                     nesterov=nesterov, first=(t == 0))
    torch.testing.assert_close(p, want, rtol=0, atol=0)


def _ref_adam_loop(p, seq, lr, betas, eps, wd, amsgrad):
    """Literal transcription of ps.py Adam.optim_step."""
    p = p.clone()
    st = {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p),
          "max_exp_avg_sq": torch.zeros_like(p)}
    for grad in seq:
        b1, b2 = betas
        st["step"] += 1
        if wd != 0:
            grad = grad.add(p, alpha=wd)
        st["exp_avg"].mul_(b1).add_(grad, alpha=1 - b1)
        st["exp_avg_sq"].mul_(b2).addcmul_(grad, grad, value=1 - b2)
        if amsgrad:
            torch.max(st["max_exp_avg_sq"], st["exp_avg_sq"], out=st["max_exp_avg_sq"])
            denom = st["max_exp_avg_sq"].sqrt().add_(eps)
        else:
            denom = st["exp_avg_sq"].sqrt().add_(eps)
        bc1 = 1 - b1 ** st["step"]
        bc2 = 1 - b2 ** st["step"]
        step_size = lr * math.sqrt(bc2) / bc1
        p.addcdiv_(st["exp_avg"], denom, value=-step_size)
    return p


@pytest.mark.parametrize("amsgrad,wd", [(False, 0.0), (True, 1e-2)])
def test_adam_reference_matches_ps_py(amsgrad, wd):
    torch.manual_seed(1)
    n = 777
    p0 = torch.randn(n)
    seq = [torch.randn(n) for _ in range(5)]
    want = _ref_adam_loop(p0, seq, 1e-2, (0.9, 0.999), 1e-8, wd, amsgrad)
    p, m, v, vm = p0.clone(), torch.zeros(n), torch.zeros(n), torch.zeros(n)
    for t, g in enumerate(seq, 1):
        ops.adam_step([g], p, m, v, vm if amsgrad else None, lr=1e-2, betas=(0.9, 0.999), eps=1e-8,
                      weight_decay=wd, step=t, amsgrad=amsgrad)
    torch.testing.assert_close(p, want, rtol=0, atol=0)


def test_adam_torch_mode_matches_torch_optim():
    torch.manual_seed(2)
    n = 300
    p0 = torch.randn(n)
    seq = [torch.randn(n) for _ in range(3)]
    tp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([tp], lr=1e-2)
    for g in seq:
        tp.grad = g.clone()
        opt.step()
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    for t, g in enumerate(seq, 1):
        ops.adam_step([g], p, m, v, lr=1e-2, step=t, torch_mode=True)
    torch.testing.assert_close(p, tp.detach(), rtol=1e-6, atol=1e-7)


def test_aggregate_rank_order_and_bf16():
    torch.manual_seed(3)
    slots = [torch.randn(100).to(torch.bfloat16) for _ in range(3)]
    acc = torch.zeros(100)
    ops.aggregate(slots, acc, 0.5)
    want = (slots[0].float() + slots[1].float() + slots[2].float()) * 0.5
    torch.testing.assert_close(acc, want)
    ops.aggregate(slots[:1], acc, 1.0, accumulate=True)
    torch.testing.assert_close(acc, want + slots[0].float())


def test_q8_roundtrip_and_error_feedback():
    torch.manual_seed(4)
    n = 1000  # not a multiple of the 256 block
    x = torch.randn(n)
    q = torch.empty(n, dtype=torch.int8)
    s = torch.empty((n + 255) // 256)
    r = torch.zeros(n)
    ops.q8_encode(x, r, q, s)
    deq = ref.q8_dequant(q, s)
    # error feedback invariant: x == deq + r exactly in the math (fp32 rounding only)
    torch.testing.assert_close(deq + r, x, rtol=0, atol=1e-6)
    assert (deq - x).abs().max() <= s.max() / 2 + 1e-6
    assert q.abs().max() <= 127


def test_q8_stochastic_rounding_unbiased():
    x = torch.full((256 * 64,), 0.3)
    x[0] = 1.0  # pins the block scale
    q = torch.empty_like(x, dtype=torch.int8)
    s = torch.empty(64)
    ops.q8_encode(x, None, q, s, stochastic=True, seed=123)
    deq = ref.q8_dequant(q, s)
    assert abs(deq[1:256].mean().item() - 0.3) < 0.02


def test_topk_reference_ties_and_order():
    x = torch.tensor([0.5, -3.0, 2.0, -2.0, 2.0, 0.1, 3.0])
    sel = ref.topk_select(x, 4)
    # |x|: 3.0 at 1 and 6, 2.0 at 2,3,4 -> lowest-index tie break takes 2,3
    assert sel.tolist() == [1, 2, 3, 6]
    idx = torch.empty(4, dtype=torch.int32)
    val = torch.empty(4)
    r = torch.zeros(7)
    ops.topk_encode(x, r, 4, idx, val)
    assert idx.tolist() == [1, 2, 3, 6]
    assert val.tolist() == [-3.0, 2.0, -2.0, 3.0]
    # EF residual keeps exactly the untransmitted mass
    torch.testing.assert_close(r, torch.tensor([0.5, 0, 0, 0, 2.0, 0.1, 0]))
    acc = torch.zeros(7)
    ops.topk_accumulate(idx, val, acc)
    torch.testing.assert_close(acc + r, x)


def test_uniform01_matches_splitmix_definition():
    u = ref.uniform01(7, np.arange(4, dtype=np.int64))
    assert u.dtype == np.float32 and ((u >= 0) & (u < 1)).all()
    assert len(set(u.tolist())) == 4


def test_threshold_codec_variable_size_and_ef():
    from hipps.codecs import Threshold

    x = torch.tensor([0.5, -3.0, 0.01, 2.0, -0.2, 0.0, 1.0])
    c = Threshold(tau=0.3, max_ratio=0.5)  # capacity 4
    lay = c.layout(7)
    buf = torch.zeros(lay.nbytes, dtype=torch.uint8)
    v = lay.views(buf)
    st = c.init_state(7, "cpu")
    c.encode_into(x, v, st)
    assert int(v["count"][0]) == 4 and v["idx"].tolist() == [0, 1, 3, 6]
    acc = torch.zeros(7)
    c.accumulate([v], acc)
    torch.testing.assert_close(acc + st["resid"], x)
    # capacity clamps: a second, denser message keeps the overflow in the residual
    c2 = Threshold(tau=0.0, max_ratio=2 / 7, error_feedback=False)
    lay2 = c2.layout(7)
    v2 = lay2.views(torch.zeros(lay2.nbytes, dtype=torch.uint8))
    c2.encode_into(x, v2, c2.init_state(7, "cpu"))
    assert int(v2["count"][0]) == 2 and v2["idx"].tolist() == [0, 1]


# ---- attention oracle (reference.attention) --------------------------------------------------
def _attn_inputs(B, Sq, Sk, Hq, Hkv, D, seed):
    """The sharp inputs of tests/test_attn_edges_gpu.py: bf16 randn with q scaled by 4, so the
    scores have standard deviation ~4 and a few keys dominate each row."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Sq, Hq, D, generator=g) * 4).to(torch.bfloat16)
    k, v = (torch.randn(B, Sk, Hkv, D, generator=g).to(torch.bfloat16) for _ in range(2))
    dout = torch.randn(B, Sq, Hq, D, generator=g).to(torch.bfloat16)
    return q, k, v, dout


def _attn_autograd(q, k, v, dout, causal, kv_len, scale):
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    G = q.shape[2] // k.shape[2]
    s = (qd.transpose(1, 2) @ kd.transpose(1, 2).repeat_interleave(G, 1).transpose(-1, -2)) * scale
    Sq, Sk = s.shape[-2:]
    bias = torch.zeros(q.shape[0], 1, Sq, Sk, dtype=torch.float64)
    if causal:
        bias = bias.masked_fill(~torch.ones(Sq, Sk, dtype=torch.bool).tril(), -math.inf)
    if kv_len is not None:
        bias = bias.masked_fill((torch.arange(Sk)[None, :] >= torch.tensor(kv_len)[:, None])[:, None, None, :],
                                -math.inf)
    s = s + bias
    o = (torch.softmax(s, -1) @ vd.transpose(1, 2).repeat_interleave(G, 1)).transpose(1, 2)
    lse = torch.logsumexp(s, -1)
    o.backward(dout.double())
    return o.detach(), lse.detach(), qd.grad, kd.grad, vd.grad


ATTN_ORACLE_CASES = [
    # B, Sq, Sk, Hq, Hkv, D, causal, kv_len, scale
    (2, 17, 17, 2, 2, 64, False, None, None),
    (2, 70, 70, 2, 2, 64, True, None, 0.37),
    (3, 40, 40, 2, 2, 32, False, [1, 33, 47], None),   # one key, a partial row, above Sk
    (2, 40, 40, 2, 2, 32, True, [9, 40], None),
    (2, 33, 33, 6, 2, 16, True, None, None),            # GQA
    (1, 33, 33, 3, 1, 16, False, [20], 0.2),
    (2, 50, 21, 4, 2, 32, False, None, None),           # Sq != Sk
    (2, 5, 61, 2, 1, 32, False, [61, 7], None),
]


@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,D,causal,kv_len,scale", ATTN_ORACLE_CASES)
def test_attention_oracle_matches_fp64_autograd(B, Sq, Sk, Hq, Hkv, D, causal, kv_len, scale):
    q, k, v, dout = _attn_inputs(B, Sq, Sk, Hq, Hkv, D, seed=Sq + Sk + Hq)
    sc = scale if scale is not None else D ** -0.5
    got = ref.attention(q, k, v, dout, causal, None if kv_len is None else torch.tensor(kv_len), scale)
    want = _attn_autograd(q, k, v, dout, causal, kv_len, sc)
    for g, w, name in zip(got, want, ("o", "lse", "dq", "dk", "dv")):
        assert g.dtype == torch.float64 and g.shape == w.shape, name
        torch.testing.assert_close(g, w, rtol=1e-10, atol=1e-10, msg=lambda m, n=name: "%s: %s" % (n, m))


@pytest.mark.parametrize("emulate", [False, True])
def test_attention_oracle_fully_masked_rows(emulate):
    """kv_len = 0: o = 0, lse = +inf, no gradient from or to that batch row; the others are what
    they are without it."""
    q, k, v, dout = _attn_inputs(3, 9, 12, 4, 2, 16, seed=3)
    o, lse, dq, dk, dv = ref.attention(q, k, v, dout, False, torch.tensor([5, 0, 12]), None, emulate)
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t).all() and torch.count_nonzero(t[1]) == 0
    assert (lse[1] == math.inf).all() and torch.isfinite(lse[[0, 2]]).all()
    assert torch.count_nonzero(dk[0, 5:]) == 0 and torch.count_nonzero(dv[0, 5:]) == 0
    rest = ref.attention(q[[0, 2]], k[[0, 2]], v[[0, 2]], dout[[0, 2]], False, torch.tensor([5, 12]), None, emulate)
    for t, r in zip((o, lse, dq, dk, dv), rest):
        assert torch.equal(t[[0, 2]], r)


def test_attention_oracle_one_key_rows_have_exactly_zero_score_gradient():
    """A softmax over one key is constant: dq and dk are exactly zero, dv is the sum of dout."""
    q, k, v, dout = _attn_inputs(2, 7, 1, 2, 1, 16, seed=4)
    for emulate in (False, True):
        o, lse, dq, dk, dv = ref.attention(q, k, v, dout, False, None, None, emulate)
        assert torch.equal(o, v.double().expand(2, 7, 2, 16))
        assert torch.count_nonzero(dq) == 0 and torch.count_nonzero(dk) == 0
        if not emulate:
            torch.testing.assert_close(dv, dout.double().sum((1, 2), keepdim=True), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,D,causal,kv_len,scale", [
    (2, 17, 17, 2, 2, 64, True, None, None),
    (2, 200, 200, 2, 2, 64, False, None, None),
    (1, 130, 75, 4, 2, 128, False, [60], 0.37),
])
def test_attention_oracle_emulated_error_is_a_yardstick(B, Sq, Sk, Hq, Hkv, D, causal, kv_len, scale):
    """The bf16-emulating mode differs from the exact one (it rounds) by a few per cent at the
    most in the per-row metric (it rounds nothing else), and its outputs are bf16 values."""
    q, k, v, dout = _attn_inputs(B, Sq, Sk, Hq, Hkv, D, seed=Sq)
    kl = None if kv_len is None else torch.tensor(kv_len)
    exact = ref.attention(q, k, v, dout, causal, kl, scale)
    emu = ref.attention(q, k, v, dout, causal, kl, scale, emulate_bf16=True)
    for e, x, name in zip(emu, exact, ("o", "lse", "dq", "dk", "dv")):
        if name == "lse":
            torch.testing.assert_close(e, x, rtol=1e-6, atol=1e-6)
            continue
        assert torch.equal(e, e.to(torch.bfloat16).double()), name
        err = ref.attention_row_error(e, x)
        assert 0.0 < err < 0.05, (name, err)


def test_attention_row_error_sees_one_wrong_row():
    want = torch.randn(2, 300, 4, 64, dtype=torch.float64)
    got = want.clone()
    got[1, 177, 2] = 0.0
    assert 0.8 < ref.attention_row_error(got, want) < 1.3
    assert ref.attention_row_error(want, want) == 0.0
