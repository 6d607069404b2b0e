"""Packed-document and sliding-window masks of the hipps flash-attention kernels (csrc/attn.hip,
the BND instantiations), against the fp64 oracle ``hipps.ops.reference.attention(doc_ids=,
window=)`` -- which builds its mask from the definition, not from the row ranges the kernels read.

The method is that of tests/test_attn_edges_gpu.py: inputs built on the host with q x 4 (sharp
rows: a wrongly masked key moves its row at full size); per tensor o / dq / dk / dv the per-row
error E = reference.attention_row_error against the exact oracle; the bound E_kernel <= 2 *
E_emulated, the same metric of the oracle's bf16-emulating mode on the same inputs (kernel and
emulation round in the same places: two draws of one distribution, 2 covers the larger); lse at
rtol 1e-3 / atol 2e-3 on finite rows and exactly +inf on rows with no key.  With a one-key
softmax on every row (window 1) dq and dk are exactly zero in the reference: only o, lse and dv
are bounded there.  The rope-packed route's q and k are rotated on the host for the oracle and
its dq / dk rotated back (the emulation rounds them once more, as the kernels' in-place rotation
does).

Exact invariants (torch.equal): one document / window >= S are the unbounded kernels; documents
cut at multiples of 128 equal each document run alone; other documents' rows never reach a
result; the 3-stage kernels equal the 2-stage ones.

Isolation is a statement about FINITE values.  A document that shares a 64-row tile with another
is multiplied by probability 0 inside the MFMA, and 0 x NaN (or 0 x Inf) is NaN: non-finite K / V
rows of a neighbouring document are outside the contract, exactly as non-finite rows above the
diagonal are under the causal mask today.  (Rows at and above ``kv_len`` stay covered: they are
staged as zeros.)

Tile constants: 128 query rows (forward / dQ) or keys (dK/dV) per workgroup, 32 per wave, 64-row
streamed tiles.

Measured E_kernel / E_emulated on an MI355X, smallest .. largest over the cases of each group
(the bound is 2):

  group                        o             dq            dk            dv
  document edges               1.00 .. 1.00  1.00 .. 1.00  1.00 .. 1.00  1.00 .. 1.00
  windows 2 .. 200             1.00 .. 1.00  1.00 .. 1.05  0.97 .. 1.14  1.00 .. 1.00
  window 1                     (o and dv equal the reference bit for bit: both errors are 0)
  documents + window + kv_len  1.00 .. 1.00  1.00 .. 1.01  0.99 .. 1.00  1.00 .. 1.00
  GQA with documents           1.00 .. 1.00  1.00 .. 1.00  1.00 .. 1.02  0.95 .. 1.00
  packed qkv route             1.00 .. 1.00  0.96 .. 1.00  0.98 .. 1.00  0.98 .. 1.00
  rope-packed route            1.00 .. 1.00  0.98 .. 1.00  1.00 .. 1.00  1.00 .. 1.00

(E_emulated itself is 0.2 % - 2.8 %.)
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


def _inputs(B, S, Hq, Hkv, D, seed):
    """bf16 randn q (x4 before rounding), k, v, dout on the device; generated on the host so the
    values do not depend on the device's generator."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, S, Hq, D, generator=g) * 4).to(torch.bfloat16)
    k, v = (torch.randn(B, S, Hkv, D, generator=g).to(torch.bfloat16) for _ in range(2))
    dout = torch.randn(B, S, Hq, D, generator=g).to(torch.bfloat16)
    return tuple(t.cuda() for t in (q, k, v, dout))


def _docs(*rows):
    """[B, S] doc ids from run lengths per batch row; the values alternate 0 1 0 .. (any change
    starts a new document: ids need be neither sorted nor unique)."""
    return torch.tensor([sum(([i % 2] * n for i, n in enumerate(r)), []) for r in rows])


def _bounds(S, doc_ids, window, causal):
    from hipps.ops import nn as hnn

    return hnn.attention_bounds(S, doc_ids=doc_ids, window=window, causal=causal, device="cuda")


def _kernel(q, k, v, dout, causal=False, kv_len=None, bounds=None, packed=False):
    """(o, lse, dq, dk, dv) of hnn.attention (or attention_qkv) forward + backward."""
    from hipps.ops import nn as hnn

    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device="cuda")
    assert hnn.attention_ok(q, k, v, causal, bounds)
    if packed:
        x = torch.stack((q, k, v), dim=2).requires_grad_(True)
        o = hnn.attention_qkv(x, causal=causal, kv_len=kl, bounds=bounds)
        o.backward(dout)
        dq, dk, dv = x.grad.unbind(2)
    else:
        qa, ka, va = (t.detach().requires_grad_(True) for t in (q, k, v))
        o = hnn.attention(qa, ka, va, causal=causal, kv_len=kl, bounds=bounds)
        o.backward(dout)
        dq, dk, dv = qa.grad, ka.grad, va.grad
    r = (None, None) if bounds is None else (bounds.klo, bounds.khi)
    _, lse = hnn.native().attn_forward(q, k, v, causal, q.shape[-1] ** -0.5, kl, *r)
    for t in (o, dq, dk, dv):
        assert t.dtype == torch.bfloat16
    return o.detach(), lse, dq, dk, dv


def _compare(got, exact, emu, group, only=NAMES):
    """The per-row bound of every tensor in ``only`` and the lse tolerance."""
    fails = []
    for name, g, x, e in zip(NAMES, got, exact, emu):
        if name not in only:
            continue
        g = g.detach().cpu()
        if name == "lse":
            fin = torch.isfinite(x)
            assert torch.isfinite(g[fin]).all(), name
            assert torch.equal(g[~fin], torch.full_like(g[~fin], math.inf)), "lse of rows with no key"
            torch.testing.assert_close(g[fin].double(), x[fin], rtol=1e-3, atol=2e-3)
            continue
        assert torch.isfinite(g.float()).all(), name
        ek, ee = ref.attention_row_error(g, x), ref.attention_row_error(e, x)
        print("ATTN_DOC %s %s E_kernel %.5f E_emulated %.5f ratio %.3f" % (group, name, ek, ee, ek / ee if ee else 0.0))
        if not ek <= 2 * ee:
            err = (g.double() - x).norm(dim=-1)
            b, s, h = (int(i) for i in (err == err.max()).nonzero()[0])
            fails.append("%s: E_kernel %.5f > 2 * E_emulated %.5f, worst row (b %d, s %d, h %d): block %d, wave %d, "
                         "row %d of the wave" % (name, ek, ee, b, s, h, s // 128, s % 128 // 32, s % 32))
    assert not fails, "; ".join(fails)


def _check(got, q, k, v, dout, causal, kv_len, doc_ids, window, group, only=NAMES):
    args = [t.cpu() for t in (q, k, v, dout)] + [causal, None if kv_len is None else torch.tensor(kv_len)]
    kw = dict(doc_ids=doc_ids, window=window)
    _compare(got, ref.attention(*args, **kw), ref.attention(*args, emulate_bf16=True, **kw), group, only)


def _run(B, S, Hq, Hkv, D, seed, causal, kv_len, doc_ids, window, group, packed=False, only=NAMES):
    t = _inputs(B, S, Hq, Hkv, D, seed)
    bd = _bounds(S, doc_ids, window, causal)
    got = _kernel(*t, causal, kv_len, bd, packed=packed)
    _check(got, *t, causal, kv_len, doc_ids, window, group, only)
    return t, got


# -------------------------------------------------------------------- oracle-bounded groups
EDGE_DOCS = _docs([1, 63, 64, 65, 127], [31, 33, 64, 1, 128, 63])  # S = 320: on and beside 32 / 64 / 128


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_document_edges(D, causal):
    (q, k, v, dout), got = _run(2, 320, 2, 2, D, 100 + D + causal, causal, None, EDGE_DOCS, None, "docs")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("W", [2, 32, 64, 65, 128, 200])
def test_windows(W, D, causal):
    _run(2, 257, 2, 2, D, 200 + W + D + causal, causal, None, None, W, "window")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_window_of_one_key(D, causal):
    """|i - j| < 1: every row sees itself alone.  o = v, lse = the score; dq and dk are exactly
    zero in the reference (a one-key softmax is constant), so o, lse and dv are bounded."""
    (q, k, v, dout), got = _run(2, 257, 2, 2, D, 300 + D + causal, causal, None, None, 1, "window1",
                                only=("o", "lse", "dv"))
    assert torch.equal(got[0], v)  # (p = 1 exactly)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_documents_window_and_key_padding_together(D, causal):
    kv_len = [320, 190]
    (q, k, v, dout), got = _run(2, 320, 2, 2, D, 400 + D + causal, causal, kv_len, EDGE_DOCS, 65, "docs+win+pad")
    o, lse, dq, dk, dv = got
    assert torch.count_nonzero(dk[1, 190:]) == 0 and torch.count_nonzero(dv[1, 190:]) == 0
    if not causal:  # row 1's last document (257 ..) lies wholly in the padding: rows with no key
        assert (lse[1, :, 257:] == math.inf).all() and torch.count_nonzero(o[1, 257:]) == 0
        assert torch.count_nonzero(dq[1, 257:]) == 0


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (6, 2)])
def test_gqa_with_documents(Hq, Hkv, D, causal):
    """(4, 1) splits the dK/dV group over workgroups (fp32 partials); (6, 2) is a group of 3."""
    _run(2, 257, Hq, Hkv, D, 500 + Hq + D + causal, causal, None, _docs([100, 57, 100], [64, 129, 64]), None, "gqa")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_packed_qkv_route(D, causal):
    _run(2, 320, 2, 2, D, 600 + D + causal, causal, [300, 320], EDGE_DOCS, 130, "packed qkv", packed=True)


def _rope64(x, cos, sin, sign=1.0):
    """Rotary embedding of interleaved pairs in fp64 on the host (sign -1: the inverse rotation)."""
    c, s = cos[None, :, None, :].double(), sign * sin[None, :, None, :].double()
    x1, x2 = x.double()[..., ::2], x.double()[..., 1::2]
    return torch.stack((x1 * c - x2 * s, x1 * s + x2 * c), dim=-1).flatten(-2)


@pytest.mark.parametrize("D", [64, 128])
def test_rope_packed_route(D):
    """y [B, S, (hq + 2 hkv) D] -> RoPE -> bounded causal GQA attention -> packed gradient rotated
    back.  The oracle gets q and k rotated on the host (fp64, rounded to bf16 as the RoPE kernel
    writes them); its dq / dk are rotated back on the host."""
    from hipps.ops import nn as hnn

    B, S, hq, hkv = 2, 257, 4, 2
    doc_ids = _docs([100, 57, 100], [64, 129, 64])
    q, k, v, dout = _inputs(B, S, hq, hkv, D, 700 + D)
    inv = 1.0 / (5e5 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    f = torch.outer(torch.arange(S, dtype=torch.float32), inv)
    cos, sin = f.cos().contiguous(), f.sin().contiguous()
    y = torch.cat([t.flatten(2) for t in (q, k, v)], dim=2).contiguous().requires_grad_(True)
    bd = _bounds(S, doc_ids, 90, True)
    assert hnn.rope_attention_packed_ok(y, cos.cuda(), hq, hkv)
    o = hnn.rope_attention_packed(y, cos.cuda(), sin.cuda(), hq, hkv, bounds=bd)
    o.backward(dout)
    dq, dk, dv = (t.reshape(B, S, -1, D) for t in y.grad.split([hq * D, hkv * D, hkv * D], dim=-1))
    qr, kr = (_rope64(t.cpu(), cos, sin).to(torch.bfloat16) for t in (q, k))
    _, lse = hnn.native().attn_forward(qr.cuda(), kr.cuda(), v, True, D ** -0.5, None, bd.klo, bd.khi)
    outs = []
    for emulate in (False, True):
        eo, el, edq, edk, edv = ref.attention(qr, kr, v.cpu(), dout.cpu(), True, doc_ids=doc_ids, window=90,
                                              emulate_bf16=emulate)
        edq, edk = _rope64(edq, cos, sin, -1.0), _rope64(edk, cos, sin, -1.0)
        if emulate:
            edq, edk = (t.to(torch.bfloat16).double() for t in (edq, edk))
        outs.append((eo, el, edq, edk, edv))
    _compare((o.detach(), lse, dq, dk, dv), outs[0], outs[1], "rope packed")


# ------------------------------------------------------------------------- exact invariants
def _assert_equal(a, b, what):
    for x, y, nm in zip(a, b, NAMES):
        assert torch.equal(x, y), (what, nm)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_one_document_and_wide_windows_are_the_unbounded_kernels(D, causal):
    """doc_ids all equal, window >= S, or both: the same tiles in the same order, the same bits."""
    S = 257
    t = _inputs(2, S, 4, 2, D, 800 + D + causal)
    plain = _kernel(*t, causal)
    one_doc = torch.zeros(2, S, dtype=torch.long)
    for doc_ids, window in ((one_doc, None), (None, S), (None, 3 * S), (one_doc, S + 1)):
        bd = _bounds(S, doc_ids, window, causal)
        assert bd is not None
        _assert_equal(_kernel(*t, causal, None, bd), plain, (doc_ids is not None, window))
    _assert_equal(_kernel(*t, causal, [257, 100], _bounds(S, one_doc, None, causal)), _kernel(*t, causal, [257, 100]),
                  "with kv_len")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_documents_cut_at_128_equal_separate_runs(D, causal):
    """Boundaries on multiples of the 128-row workgroup and Hq == Hkv (no dK/dV group split):
    every document's slice is that document run alone through the unbounded kernels."""
    S, lens = 512, ([128, 256, 128], [256, 128, 128])
    q, k, v, dout = _inputs(2, S, 2, 2, D, 900 + D + causal)
    got = _kernel(q, k, v, dout, causal, None, _bounds(S, _docs(*lens), None, causal))
    for b in range(2):
        a = 0
        for n in lens[b]:
            one = _kernel(*(t[b:b + 1, a:a + n] for t in (q, k, v, dout)), causal)
            for x, y, nm in zip(got, one, NAMES):
                x = x[b:b + 1, :, a:a + n] if nm == "lse" else x[b:b + 1, a:a + n]
                assert torch.equal(x, y), (b, a, nm)
            a += n


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_other_documents_never_reach_a_result(D, causal):
    """Boundaries at 1, 64 and 97 (the first row, a tile edge, inside the fourth wave's rows) of
    193 tokens.  Other finite q / k / v / dout rows in one document leave every output row of the
    other documents unchanged bit for bit, and change its own.  Finite values only: see the
    module docstring."""
    S, cuts = 193, [0, 1, 64, 97, 193]
    doc_ids = _docs([1, 63, 33, 96], [1, 63, 33, 96])
    bd = _bounds(S, doc_ids, None, causal)
    base_in = _inputs(2, S, 4, 2, D, 1000 + D + causal)
    base = _kernel(*base_in, causal, None, bd)
    for d in range(4):
        a, e = cuts[d], cuts[d + 1]
        g = torch.Generator().manual_seed(d)
        ins = [t.clone() for t in base_in]
        for t in ins:
            t[:, a:e] = torch.randn(t[:, a:e].shape, generator=g).to(torch.bfloat16).cuda()
        got = _kernel(*ins, causal, None, bd)
        for x, y, nm in zip(got, base, NAMES):
            if nm == "lse":
                x, y = x.transpose(1, 2), y.transpose(1, 2)  # [B, S, H]
            assert torch.equal(x[:, :a], y[:, :a]) and torch.equal(x[:, e:], y[:, e:]), (d, nm)
        assert not torch.equal(got[0][:, a:e], base[0][:, a:e]), d  # (its own rows do change)


_STAGES_CHILD = """
import sys
import torch
from hipps.ops import nn as hnn
cases = torch.load(sys.argv[1])
outs = []
for q, k, v, dout, causal, doc_ids, window in cases:
    q, k, v, dout = (t.cuda() for t in (q, k, v, dout))
    bd = hnn.attention_bounds(q.shape[1], doc_ids=doc_ids, window=window, causal=causal, device="cuda")
    qa, ka, va = (t.detach().requires_grad_(True) for t in (q, k, v))
    o = hnn.attention(qa, ka, va, causal=causal, bounds=bd)
    o.backward(dout)
    _, lse = hnn.native().attn_forward(q, k, v, causal, q.shape[-1] ** -0.5, None, bd.klo, bd.khi)
    outs.append([t.detach().cpu() for t in (o, lse, qa.grad, ka.grad, va.grad)])
torch.cuda.synchronize()
torch.save(outs, sys.argv[2])
"""


def test_three_stage_bounded_kernels_match_two_stage(tmp_path):
    """HIPPS_ATTN_STAGES=3 (read once per process, so a fresh child process) selects the 3-stage
    BND kernels: the same arithmetic in the same order, so the same bits."""
    assert os.environ.get("HIPPS_ATTN_STAGES", "") != "3"
    cases = []
    for D in (64, 128):
        for causal in (False, True):
            q, k, v, dout = _inputs(2, 320, 4, 2, D, 1100 + D + causal)
            cases.append((q, k, v, dout, causal, EDGE_DOCS, 100))
    mine = [[t.cpu() for t in _kernel(q, k, v, dout, causal, None, _bounds(320, d, w, causal))]
            for q, k, v, dout, causal, d, w in cases]
    fin, fout = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save([tuple(t.cpu() for t in c[:4]) + c[4:] for c in cases], fin)
    env = dict(os.environ, HIPPS_ATTN_STAGES="3")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _STAGES_CHILD, fin, fout], env=env, cwd=ROOT, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    theirs = torch.load(fout)
    assert len(theirs) == len(mine)
    for c, a, b in zip(cases, mine, theirs):
        _assert_equal(a, b, (c[0].shape[-1], c[4]))


# --------------------------------------------------------------------------------------- gate
def test_gate_keeps_cross_attention_bounds_off_the_kernels(monkeypatch):
    """Bounds are for self-attention: with Sq != Sk attention_ok is false, no kernel is launched
    and the fallback (which has no mask to build for two different lengths) raises ValueError."""
    from hipps.ops import nn as hnn

    calls = []

    def counted(ctx, *a, _fwd=hnn._FlashAttention.forward):
        calls.append(1)
        return _fwd(ctx, *a)

    monkeypatch.setattr(hnn._FlashAttention, "forward", staticmethod(counted))
    q, k, v, _ = _inputs(2, 72, 2, 2, 64, 1200)
    bd = _bounds(72, None, 8, False)
    hnn.attention(q, k, v, bounds=bd)
    assert len(calls) == 1  # (the counter sees the kernel route)
    calls.clear()
    assert hnn.attention_ok(q[:, :40], k, v) and not hnn.attention_ok(q[:, :40], k, v, False, bd)
    with pytest.raises(ValueError, match="self-attention"):
        hnn.attention(q[:, :40], k, v, bounds=bd)
    assert not calls


def test_native_entry_points_reject_bad_bounds():
    """Past the Python gate the extension's own checks raise (a RuntimeError, no launch)."""
    from hipps.ops import nn as hnn

    C = hnn.native()
    q, k, v, dout = _inputs(2, 40, 2, 2, 64, 1300)
    bd = _bounds(40, _docs([10, 30], [25, 15]), None, False)
    o, lse = C.attn_forward(q, k, v, False, 0.125, None, bd.klo, bd.khi)  # (these are accepted)
    C.attn_backward(dout, q, k, v, o, lse, False, 0.125, None, None, None, None, *bd[:4])
    bad = {"int64": bd.klo.long(), "host": bd.klo.cpu(), "shape": bd.klo[:, :39].contiguous(),
           "batch": torch.cat([bd.klo, bd.klo[:1]]), "1-D": bd.klo[0], "strided": bd.klo.repeat(1, 2)[:, ::2]}
    for name, t in bad.items():
        with pytest.raises(RuntimeError, match="klo"):
            C.attn_forward(q, k, v, False, 0.125, None, t, bd.khi)
        with pytest.raises(RuntimeError, match="qhi"):
            C.attn_backward(dout, q, k, v, o, lse, False, 0.125, None, None, None, None, bd.klo, bd.khi, bd.qlo, t)
    with pytest.raises(RuntimeError, match="together"):
        C.attn_forward(q, k, v, False, 0.125, None, bd.klo, None)
    with pytest.raises(RuntimeError, match="together"):
        C.attn_backward(dout, q, k, v, o, lse, False, 0.125, None, None, None, None, bd.klo, bd.khi)
    with pytest.raises(RuntimeError, match="Sq == Sk"):
        C.attn_forward(q[:, :33], k, v, False, 0.125, None, bd.klo, bd.khi)
    with pytest.raises(RuntimeError, match="share"):  # [1, S] next to [B, S]
        C.attn_forward(q, k, v, False, 0.125, None, bd.klo, bd.khi[:1])
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------- model
def test_llama_documents_are_isolated_bit_for_bit():
    """Head dim 64 Llama under bf16 autocast, two documents of 128 tokens: other tokens in document
    0 leave document 1's logits bit-identical with doc_ids, and do not without."""
    from hipps.models import transformer as tf

    torch.manual_seed(0)
    m = tf.Llama(tf.LlamaConfig(vocab=512, dim=128, layers=2, heads=2, kv_heads=1, ffn=256, max_seq=256)).cuda()
    ids = torch.randint(0, 512, (2, 256), device="cuda")
    ids2 = ids.clone()
    ids2[:, :128] = torch.randint(0, 512, (2, 128), device="cuda")
    doc_ids = _docs([128, 128], [128, 128]).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        a, b = m(ids, doc_ids=doc_ids), m(ids2, doc_ids=doc_ids)
        c, d = m(ids), m(ids2)
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a[:, 128:], b[:, 128:])
    assert not torch.equal(a[:, :128], b[:, :128])
    assert not torch.equal(c[:, 128:], d[:, 128:])
