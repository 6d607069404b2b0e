"""hipps flash attention (csrc/attn.hip) at its tile edges, against the fp64 oracle
``hipps.ops.reference.attention``.

tests/test_attn_gpu.py bounds a whole-tensor Frobenius ratio on near-uniform softmax rows; one
row that gains or loses a key does not move it.  Here

  * q is scaled by 4 (score standard deviation ~4: a few keys dominate each row, so a wrongly
    masked key changes the row at full size);
  * the metric is per row: E = max_row ||got - ref64|| / RMS_row ||ref64|| (reference.
    attention_row_error), for each of o, dq, dk, dv;
  * the bound is E_kernel <= 2 * E_emulated, where E_emulated is the same metric of the oracle's
    bf16-emulating mode (it rounds where the kernels round and nowhere else) on the same inputs.
    Kernel and emulation make the same roundings, so their errors are two draws of one
    distribution; 2 covers the maximum of two such draws.  The kernels' fp32 online-softmax
    rescale and exp2 approximation (~2^-20) are negligible against the 2^-9 roundings;
  * a reference that is identically zero (dq and dk with a single key: a one-key softmax is
    constant) has no relative error; the kernel's value there is the fp32 residue of
    dP - delta, bounded in _check_one_key;
  * lse: rtol 1e-3 / atol 2e-3 on finite entries, fully masked rows exactly +inf;
  * mask invariants (causality, padding never read, batch / head independence, the 3-stage
    kernels) are exact: torch.equal.

Tile constants: 128 query rows (forward / dQ) or keys (dK/dV) per workgroup, 32 per wave, 64-row
streamed tiles.

Measured E_kernel / E_emulated on an MI355X, smallest .. largest over the cases of each group
(the bound is 2; E_emulated itself is 0.2 % - 5.6 %; cases where both errors are exactly 0, S = 1,
are left out):

  group                        o             dq            dk            dv
  self-attention edges         1.00 .. 1.00  0.88 .. 1.05  0.92 .. 1.07  1.00 .. 1.03
  cross-attention              1.00 .. 1.00  1.00 .. 1.28  0.73 .. 1.01  1.00 .. 1.00
  key padding (both sets)      1.00 .. 1.00  1.00 .. 1.00  0.98 .. 1.01  1.00 .. 1.00
  key padding, packed qkv      1.00 .. 1.00  1.00 .. 1.00  0.98 .. 1.01  1.00 .. 1.00
  GQA group sizes              1.00 .. 1.00  1.00 .. 1.00  0.98 .. 1.02  1.00 .. 1.00
  padding fills (zeros run)    1.00 .. 1.00  1.00 .. 1.00  1.00 .. 1.00  1.00 .. 1.00
  batch / head independence    1.00 .. 1.00  1.00 .. 1.03  1.00 .. 1.01  1.00 .. 1.00

(1.28 and 0.73 are both (Sq, Sk) = (1, 200), D = 64: four query rows.)  With Sk = 1 the kernels'
dq / dk are 3e-7 .. 5e-5 in row norm where the reference is exactly zero.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from hipps.ops import reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("o", "lse", "dq", "dk", "dv")


def _inputs(B, Sq, Sk, Hq, Hkv, D, seed):
    """bf16 randn q (x4 before rounding), k, v, dout on the device; generated on the host so the
    values do not depend on the device's generator."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Sq, Hq, D, generator=g) * 4).to(torch.bfloat16)
    k, v = (torch.randn(B, Sk, Hkv, D, generator=g).to(torch.bfloat16) for _ in range(2))
    dout = torch.randn(B, Sq, Hq, D, generator=g).to(torch.bfloat16)
    return tuple(t.cuda() for t in (q, k, v, dout))


def _kvlen(kv_len):
    return None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device="cuda")


def _kernel(q, k, v, dout, causal=False, kv_len=None, scale=None, packed=False):
    """(o, lse, dq, dk, dv) of hnn.attention (or attention_qkv) forward + backward."""
    from hipps.ops import nn as hnn

    kl = _kvlen(kv_len)
    assert hnn.attention_ok(q, k, v, causal)
    if packed:
        x = torch.stack((q, k, v), dim=2).requires_grad_(True)
        o = hnn.attention_qkv(x, causal=causal, scale=scale, kv_len=kl)
        o.backward(dout)
        dq, dk, dv = x.grad.unbind(2)
    else:
        qa, ka, va = (t.detach().requires_grad_(True) for t in (q, k, v))
        o = hnn.attention(qa, ka, va, causal=causal, scale=scale, kv_len=kl)
        o.backward(dout)
        dq, dk, dv = qa.grad, ka.grad, va.grad
    sc = float(scale) if scale is not None else q.shape[-1] ** -0.5
    _, lse = hnn.native().attn_forward(q, k, v, causal, sc, kl)
    for t in (o, dq, dk, dv):
        assert t.dtype == torch.bfloat16
    assert o.shape == q.shape and dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    return o.detach(), lse, dq, dk, dv


def _oracle(q, k, v, dout, causal, kv_len, scale):
    """(exact, bf16-emulated) oracle outputs, fp64 on the host."""
    args = [t.cpu() for t in (q, k, v, dout)] + [causal, None if kv_len is None else torch.tensor(kv_len), scale]
    return ref.attention(*args), ref.attention(*args, emulate_bf16=True)


def _check_one_key(got, q, k, v, dout, scale):
    """Sk == 1: dq and dk are exactly zero in exact arithmetic.  The kernels form dS = p (dP -
    delta) from two fp32 sums of the same D products dO_d v_d (o = v exactly), each within
    D 2^-24 sum|dO_d v_d| <= D 2^-24 ||dO|| ||v|| of the true value, so |dS| <= 2 D 2^-24 ||dO||
    ||v|| (p <= 1 up to the fp32 error of s - lse, and the bf16 roundings: 5 % slack), dq_i =
    scale dS_i k and dk = scale sum_i dS_i q_i over the Sq rows of the G query heads."""
    o, lse, dq, dk, dv = got
    D, G = q.shape[-1], q.shape[2] // k.shape[2]
    sc = float(scale) if scale is not None else D ** -0.5
    nrm = lambda t: t.double().norm(dim=-1).max().item()
    eps = 1.05 * 2 * D * 2.0 ** -24 * nrm(dout) * nrm(v) * sc
    e_dq, e_dk = nrm(dq), nrm(dk)
    print("ATTN_EDGE_ZERO dq %.3e <= %.3e  dk %.3e <= %.3e" % (e_dq, eps * nrm(k), e_dk, eps * nrm(q) * q.shape[1] * G))
    assert e_dq <= eps * nrm(k), ("dq", e_dq)
    assert e_dk <= eps * nrm(q) * q.shape[1] * G, ("dk", e_dk)


def _check(got, q, k, v, dout, causal=False, kv_len=None, scale=None, group="", only=NAMES):
    """The per-row bound of every tensor in ``only`` and the lse tolerance, against the oracle."""
    exact, emu = _oracle(q, k, v, dout, causal, kv_len, scale)
    fails = []
    for name, g, x, e in zip(NAMES, got, exact, emu):
        if name not in only:
            continue
        g = g.detach().cpu()
        if name == "lse":
            fin = torch.isfinite(x)
            assert torch.isfinite(g[fin]).all(), name
            assert torch.equal(g[~fin], torch.full_like(g[~fin], math.inf)), "lse of fully masked rows"
            torch.testing.assert_close(g[fin].double(), x[fin], rtol=1e-3, atol=2e-3)
            continue
        assert torch.isfinite(g.float()).all(), name
        if torch.count_nonzero(x) == 0:
            assert k.shape[1] == 1 and name in ("dq", "dk"), name
            continue
        ek, ee = ref.attention_row_error(g, x), ref.attention_row_error(e, x)
        print("ATTN_EDGE %s %s E_kernel %.5f E_emulated %.5f ratio %.3f" % (group, name, ek, ee, ek / ee if ee else 0.0))
        if not ek <= 2 * ee:
            err = (g.double() - x).norm(dim=-1)
            b, s, h = (int(i) for i in (err == err.max()).nonzero()[0])
            fails.append("%s: E_kernel %.5f > 2 * E_emulated %.5f, worst row (b %d, s %d, h %d): block %d, wave %d, "
                         "row %d of the wave" % (name, ek, ee, b, s, h, s // 128, s % 128 // 32, s % 32))
    if k.shape[1] == 1 and ("dq" in only or "dk" in only):
        _check_one_key(got, q, k, v, dout, scale)
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------ case groups
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 33, 64, 65, 129, 193, 257])
def test_self_attention_edges(S, D, causal):
    scale = 0.37 if S in (65, 193) else None  # (not 1/sqrt(D))
    t = _inputs(2, S, S, 2, 2, D, seed=1000 + S + D + causal)
    _check(_kernel(*t, causal, None, scale), *t, causal, None, scale, group="self")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk", [(1, 200), (200, 1), (65, 129), (129, 65), (257, 63)])
def test_cross_attention(Sq, Sk, D):
    scale = 0.21 if (Sq, Sk) == (129, 65) else None
    t = _inputs(2, Sq, Sk, 2, 2, D, seed=2000 + Sq + 3 * Sk + D)
    _check(_kernel(*t, False, None, scale), *t, False, None, scale, group="cross")


PAD_SETS = {"first": [0, 1, 64, 197], "second": [63, 65, 128, 192]}  # Sk = 192; 197 behaves as 192


def _padding_case(which, D, causal, packed):
    kv_len = PAD_SETS[which]
    t = _inputs(4, 192, 192, 2, 2, D, seed=3000 + D + causal)
    got = _kernel(*t, causal, kv_len, None, packed=packed)
    _check(got, *t, causal, kv_len, None, group="packed" if packed else "padding")
    o, lse, dq, dk, dv = got
    for b, n in enumerate(kv_len):
        assert torch.count_nonzero(dk[b, n:]) == 0 and torch.count_nonzero(dv[b, n:]) == 0, b
        if n == 0:  # a fully padded batch row
            for x in (o, dq, dk, dv):
                assert torch.isfinite(x[b].float()).all() and torch.count_nonzero(x[b]) == 0
            assert (lse[b] == math.inf).all()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("which", ["first", "second"])
def test_key_padding_boundaries(which, D, causal):
    _padding_case(which, D, causal, packed=False)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_key_padding_boundaries_packed_qkv(D, causal):
    _padding_case("first", D, causal, packed=True)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Hq,Hkv", [(2, 1), (3, 1), (6, 1), (8, 1), (6, 2)])
def test_gqa_group_sizes(Hq, Hkv, causal):
    """Groups of 2, 3, 6 and 8 query heads: the dK/dV group split takes 2, 1 (odd: no split), 2
    and 8 slices here, (6, 2) a group of 3 per kv head."""
    scale = 0.37 if (Hq, Hkv) == (6, 1) else None
    t = _inputs(2, 129, 129, Hq, Hkv, 128, seed=4000 + 10 * Hq + Hkv + causal)
    _check(_kernel(*t, causal, None, scale), *t, causal, None, scale, group="gqa")


# ------------------------------------------------------------------------- exact invariants
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("j", [1, 64, 97])
def test_causal_rows_never_see_later_keys(j, D):
    """Under the causal mask, other K / V rows at and after j leave o, lse and dq of the query
    rows before j unchanged bit for bit (no upstream gradient on the rows from j on, in both
    runs).  j = 1, 64, 97: the first row, a tile boundary, inside the fourth wave's rows."""
    q, k, v, dout = _inputs(2, 193, 193, 2, 2, D, seed=5000 + D)
    dout[:, j:] = 0
    k2, v2 = k.clone(), v.clone()
    g = torch.Generator().manual_seed(j)
    k2[:, j:] = torch.randn(k[:, j:].shape, generator=g).to(torch.bfloat16).cuda()
    v2[:, j:] = torch.randn(v[:, j:].shape, generator=g).to(torch.bfloat16).cuda()
    assert not torch.equal(k2, k)
    o1, lse1, dq1, _, _ = _kernel(q, k, v, dout, True)
    o2, lse2, dq2, _, _ = _kernel(q, k2, v2, dout, True)
    assert torch.equal(o1[:, :j], o2[:, :j])
    assert torch.equal(lse1[..., :j], lse2[..., :j])
    assert torch.equal(dq1[:, :j], dq2[:, :j])
    assert not torch.equal(o1[:, j:], o2[:, j:])  # (the perturbation is visible where it may be)


@pytest.mark.parametrize("D,causal,Hq,Hkv", [(64, False, 2, 2), (128, True, 2, 2), (64, True, 4, 1),
                                             (128, False, 4, 1)])
def test_padded_keys_are_never_read_into_a_result(D, causal, Hq, Hkv):
    """Whatever the K / V rows at and above kv_len hold -- Inf and NaN included, as after
    torch.empty -- every output is finite, the padded keys' dk / dv are exactly zero and all five
    outputs equal those of zero padding bit for bit.  (Hq, Hkv) = (4, 1) takes the split-group
    dK/dV path with fp32 partials.)"""
    kv_len = [70, 33]
    q, k, v, dout = _inputs(2, 129, 129, Hq, Hkv, D, seed=6000 + D + Hq)
    g = torch.Generator().manual_seed(1)
    fills = {"zeros": 0.0, "randn": None, "3e38": 3e38, "inf": math.inf, "nan": math.nan}
    base = None
    for name, val in fills.items():
        k2, v2 = k.clone(), v.clone()
        for b, n in enumerate(kv_len):
            for t in (k2, v2):
                if val is None:
                    t[b, n:] = torch.randn(t[b, n:].shape, generator=g).to(torch.bfloat16).cuda()
                else:
                    t[b, n:] = val
        got = _kernel(q, k2, v2, dout, causal, kv_len)
        for x, nm in zip(got, NAMES):
            assert torch.isfinite(x.float()).all(), (name, nm)
        for b, n in enumerate(kv_len):
            assert torch.count_nonzero(got[3][b, n:]) == 0 and torch.count_nonzero(got[4][b, n:]) == 0, name
        if base is None:
            base = got
            _check(got, q, k2, v2, dout, causal, kv_len, group="poison")
        for x, y, nm in zip(got, base, NAMES):
            assert torch.equal(x, y), (name, nm)


@pytest.mark.parametrize("causal", [False, True])
def test_batch_and_head_independence(causal):
    """A batch row, and a kv group with its two query heads, computed alone give the same o, lse
    and dq bit for bit (with distinct key lengths per row); dk / dv meet the oracle bound either
    way (the group split depends on the grid, so their summation order may differ)."""
    kv_len = [129, 40, 97]
    q, k, v, dout = _inputs(3, 129, 129, 4, 2, 64, seed=7000 + causal)
    full = _kernel(q, k, v, dout, causal, kv_len)
    _check(full, q, k, v, dout, causal, kv_len, group="indep")
    for b in range(3):
        sl = [t[b:b + 1] for t in (q, k, v, dout)]
        one = _kernel(*sl, causal, kv_len[b:b + 1])
        for i in (0, 1, 2):
            assert torch.equal(one[i], full[i][b:b + 1]), (b, NAMES[i])
        _check(one, *sl, causal, kv_len[b:b + 1], group="indep", only=("dk", "dv"))
    for hk in range(2):
        hs = slice(2 * hk, 2 * hk + 2)
        sl = [q[:, :, hs], k[:, :, hk:hk + 1], v[:, :, hk:hk + 1], dout[:, :, hs]]
        one = _kernel(*sl, causal, kv_len)
        assert torch.equal(one[0], full[0][:, :, hs]), hk
        assert torch.equal(one[1], full[1][:, hs]), hk
        assert torch.equal(one[2], full[2][:, :, hs]), hk
        _check(one, *sl, causal, kv_len, group="indep", only=("dk", "dv"))


_STAGES_CHILD = """
import sys
import torch
from hipps.ops import nn as hnn
cases = torch.load(sys.argv[1])
outs = []
for q, k, v, dout, causal in cases:
    q, k, v, dout = (t.cuda() for t in (q, k, v, dout))
    qa, ka, va = (t.detach().requires_grad_(True) for t in (q, k, v))
    o = hnn.attention(qa, ka, va, causal=causal)
    o.backward(dout)
    _, lse = hnn.native().attn_forward(q, k, v, causal, q.shape[-1] ** -0.5, None)
    outs.append([t.detach().cpu() for t in (o, lse, qa.grad, ka.grad, va.grad)])
torch.cuda.synchronize()
torch.save(outs, sys.argv[2])
"""


def test_three_stage_kernels_match_two_stage(tmp_path):
    """HIPPS_ATTN_STAGES=3 (read once per process, so a fresh child process) selects the 3-stage
    forward / dQ / dK/dV kernels: the same arithmetic in the same order, so the same bits."""
    assert os.environ.get("HIPPS_ATTN_STAGES", "") != "3"
    cases = []
    for D in (64, 128):
        for causal in (False, True):
            q, k, v, dout = _inputs(2, 257, 257, 4, 2, D, seed=8000 + D + causal)
            cases.append((q, k, v, dout, causal))
    mine = [[t.cpu() for t in _kernel(q, k, v, dout, causal)] for q, k, v, dout, causal in cases]
    fin, fout = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save([tuple(t.cpu() for t in c[:4]) + (c[4],) for c in cases], fin)
    env = dict(os.environ, HIPPS_ATTN_STAGES="3")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _STAGES_CHILD, fin, fout], env=env, cwd=ROOT, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    theirs = torch.load(fout)
    assert len(theirs) == len(mine)
    for c, a, b in zip(cases, mine, theirs):
        for x, y, nm in zip(a, b, NAMES):
            assert torch.equal(x, y), (c[0].shape[-1], c[4], nm)


# --------------------------------------------------------------------------------------- gate
def _gate_cases():
    q, k, v, _ = _inputs(2, 40, 40, 2, 2, 96, seed=9001)
    yield "D=96", q, k, v, False
    q, k, v, _ = _inputs(2, 40, 40, 2, 2, 64, seed=9002)
    yield "fp16", q.half(), k.half(), v.half(), False
    q, k, v, _ = _inputs(2, 40, 72, 2, 2, 64, seed=9003)
    yield "causal Sq != Sk", q, k, v, True
    q, k, v, _ = _inputs(2, 40, 40, 2, 2, 64, seed=9004)
    n = q.numel()
    buf = torch.zeros(3 * (n + 8) + 8, dtype=torch.bfloat16, device="cuda")
    off = (16 - buf.data_ptr() % 16) % 16 // 2 + 4  # 8 bytes past a 16-byte boundary
    views = []
    for i, t in enumerate((q, k, v)):
        w = buf[off + i * (n + 8): off + i * (n + 8) + n].view(t.shape)
        w.copy_(t)
        assert w.data_ptr() % 16 == 8
        views.append(w)
    yield "misaligned", views[0], views[1], views[2], False


def test_gate_keeps_unsupported_operands_off_the_kernels(monkeypatch):
    """Head dim 96, fp16, causal cross-attention and rows off 16-byte alignment do not reach the
    kernels: attention_ok is false, _FlashAttention.forward is not called and hnn.attention
    returns the SDPA result."""
    from hipps.ops import nn as hnn

    calls = []

    def counted(ctx, *a, _fwd=hnn._FlashAttention.forward):
        calls.append(1)
        return _fwd(ctx, *a)

    monkeypatch.setattr(hnn._FlashAttention, "forward", staticmethod(counted))
    q, k, v, _ = _inputs(1, 40, 40, 2, 2, 64, seed=9000)
    hnn.attention(q, k, v)
    assert len(calls) == 1  # (the counter sees the kernel route)
    for name, q, k, v, causal in _gate_cases():
        calls.clear()
        assert not hnn.attention_ok(q, k, v, causal), name
        o = hnn.attention(q, k, v, causal=causal)
        assert not calls, name
        assert o.shape == q.shape and o.dtype == q.dtype, name
        want = ref.attention(q.cpu(), k.cpu(), v.cpu(), torch.zeros_like(q).cpu(), causal)[0]
        torch.testing.assert_close(o.float().cpu(), want.float(), rtol=2e-2, atol=2e-2, msg=lambda m, n=name: n + ": " + m)


def test_native_entry_points_reject_what_the_gate_rejects():
    """Past the Python gate the extension's own checks raise (a RuntimeError, no launch)."""
    from hipps.ops import nn as hnn

    q, k, v, _ = _inputs(2, 40, 40, 2, 2, 32, seed=9100)
    with pytest.raises(RuntimeError, match="head dim"):
        hnn.native().attn_forward(q, k, v, False, 32 ** -0.5, None)
    q, k, v, _ = _inputs(2, 40, 40, 2, 2, 64, seed=9101)
    with pytest.raises(RuntimeError, match="kv_len"):
        hnn.native().attn_forward(q, k, v, False, 0.125, torch.tensor([40, 20], device="cuda"))
    with pytest.raises(RuntimeError, match="causal"):
        hnn.native().attn_forward(q, k[:, :33], v[:, :33], True, 0.125, None)


def test_bert_takes_int64_key_lengths():
    """Bert(ids, kv_len=...) with the int64 lengths torch.tensor([...]) makes (on the host, even)
    is the int32 call, bit for bit -- not a 1-D SDPA attn_mask."""
    from hipps.models import transformer as tf

    torch.manual_seed(0)
    m = tf.Bert(tf.BertConfig(vocab=512, hidden=128, layers=2, heads=2, ffn=256, max_pos=128)).cuda()
    ids = torch.randint(0, 512, (2, 96), device="cuda")
    outs = []
    for kv_len in (torch.tensor([96, 50], dtype=torch.int32, device="cuda"), torch.tensor([96, 50])):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            outs.append(m(ids, kv_len=kv_len))
    assert outs[1].dtype == outs[0].dtype and torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert not torch.equal(m(ids), outs[0])  # (the lengths matter)
