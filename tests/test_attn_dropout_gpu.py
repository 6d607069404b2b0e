"""Attention-probability dropout inside the flash attention kernels (csrc/attn.hip, the DROP
instantiations) against the numpy twin of the mask (hipps.ops.reference.dropout_keep) and the fp64
oracle ``reference.attention(..., dropout_p, dropout_seed)``.

  * The mask is read out of the forward kernel bit for bit: with q = k = 0 P is uniform over the
    visible keys, and with v[j] = e_(j - off) for keys off <= j < off + D the output o[b, i, hq, d]
    is non-zero exactly where key off + d is visible to and kept for query i.
  * ``attn_dropout_keep`` evaluates the device function at arbitrary indices (up to 2^24 - 1).
  * Numerics, as tests/test_attn_edges_gpu.py: q x 4, per-row error E = max_row ||got - ref64|| /
    RMS_row ||ref64|| (reference.attention_row_error) of o / dq / dk / dv, bound E_kernel <= 2 *
    E_emulated with E_emulated that of the oracle's bf16-emulating mode with the same mask (kernel
    and emulation round in the same places: two draws of one distribution, 2 covers the larger);
    lse rtol 1e-3 / atol 2e-3, exactly +inf on rows with no key.
  * Sk = 1: dq and dk are exactly zero in the reference (a one-key softmax is constant, kept or
    dropped).  The kernels form dS = p (rinv dP - delta) with delta = dO . o from the bf16 o =
    round(rinv v): |dS| <= ||dO|| (2^-9 rinv ||v|| + 2 D 2^-24 rinv ||v||) -- the rounding of o
    (exact at p = 0.5, rinv = 2) plus the two fp32 sums -- bounded in _check_one_key.
  * Routes, determinism, independence of the problem's extent, p = 0: torch.equal.

Tile constants: 128 query rows (forward / dQ) or keys (dK/dV) per workgroup, 32 per wave, 64-row
streamed tiles; the mask's hash block is 2 queries x 4 keys.

Measured E_kernel / E_emulated on an MI355X, smallest .. largest over the cases of each group (the
bound is 2; cases where both errors are exactly 0 are left out):

  group                        o             dq            dk            dv
  self-attention edges         1.00 .. 1.00  0.99 .. 1.12  0.98 .. 1.06  1.00 .. 1.00
  cross-attention              1.00 .. 1.00  1.00 .. 1.00  1.00 .. 1.02  1.00 .. 1.00
  causal                       1.00 .. 1.00  1.00 .. 1.11  1.00 .. 1.06  1.00 .. 1.00
  key padding                  0.97 .. 1.00  1.00 .. 1.00  1.00 .. 1.00  1.00 .. 1.00
  documents + window           1.00 .. 1.00  1.00 .. 1.00  1.00 .. 1.00  1.00 .. 1.00
  GQA groups 1 / 3 / 4         1.00 .. 1.00  1.00 .. 1.00  0.96 .. 1.02  1.00 .. 1.00
  S = 1000                     1.00 .. 1.00  1.00 .. 1.00  1.00 .. 1.00  1.00 .. 1.00

(E_emulated itself is 0.2 % - 5.0 %.)  With S = 1 the kernels' dq / dk row norms are 2.0e-2 / 8.0e-2
at p = 0.1 (the rounding of o = v / (1 - p_eff); bounds 0.18 / 0.83 and 0.35 / 1.4 for D = 64 / 128)
and 2e-6 .. 1.6e-5 at p = 0.5, where the reference is exactly zero.
"""
import math

import numpy as np
import pytest
import torch

from hipps.ops import reference as ref

pytestmark = pytest.mark.gpu

NAMES = ("o", "lse", "dq", "dk", "dv")
SEED = 0x0123_4567_89AB_CDEF
PS = (0.1, 0.5)


def _hnn():
    from hipps.ops import nn as hnn
    return hnn


def _inputs(B, Sq, Sk, Hq, Hkv, D, seed):
    """bf16 randn q (x4 before rounding), k, v, dout on the device, generated on the host."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Sq, Hq, D, generator=g) * 4).to(torch.bfloat16)
    k, v = (torch.randn(B, Sk, Hkv, D, generator=g).to(torch.bfloat16) for _ in range(2))
    dout = torch.randn(B, Sq, Hq, D, generator=g).to(torch.bfloat16)
    return tuple(t.cuda() for t in (q, k, v, dout))


def _kvlen(kv_len):
    return None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device="cuda")


def _bounds(S, doc_ids, window, causal):
    hnn = _hnn()
    d = None if doc_ids is None else doc_ids.cuda()
    return hnn.attention_bounds(S, doc_ids=d, window=window, causal=causal, device="cuda")


def _kernel(q, k, v, dout, p, seed, causal=False, kv_len=None, bounds=None, packed=False):
    """(o, lse, dq, dk, dv) of hnn.attention (or attention_qkv) forward + backward with dropout."""
    hnn = _hnn()
    kl = _kvlen(kv_len)
    assert hnn.attention_ok(q, k, v, causal, bounds)
    kw = dict(causal=causal, kv_len=kl, bounds=bounds, dropout_p=p, dropout_seed=seed)
    if packed:
        x = torch.stack((q, k, v), dim=2).requires_grad_(True)
        o = hnn.attention_qkv(x, **kw)
        o.backward(dout)
        dq, dk, dv = x.grad.unbind(2)
    else:
        qa, ka, va = (t.detach().requires_grad_(True) for t in (q, k, v))
        o = hnn.attention(qa, ka, va, **kw)
        o.backward(dout)
        dq, dk, dv = qa.grad, ka.grad, va.grad
    r = (None, None) if bounds is None else (bounds.klo, bounds.khi)
    o2, lse = hnn.native().attn_forward(q, k, v, causal, q.shape[-1] ** -0.5, kl, r[0], r[1], p, seed)
    assert torch.equal(o2, o.detach())
    for t in (o, dq, dk, dv):
        assert t.dtype == torch.bfloat16
    assert o.shape == q.shape and dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    return o.detach(), lse, dq, dk, dv


def _check_one_key(got, q, k, v, dout, p):
    o, lse, dq, dk, dv = got
    D, G = q.shape[-1], q.shape[2] // k.shape[2]
    sc = D ** -0.5
    rinv = 1.0 / (1.0 - ref.dropout_params(p)[1])
    nrm = lambda t: t.double().norm(dim=-1).max().item()
    eps = 1.05 * (2.0 ** -9 + 2 * D * 2.0 ** -24) * rinv * nrm(dout) * nrm(v) * sc
    e_dq, e_dk = nrm(dq), nrm(dk)
    print("ATTN_DROP_ZERO dq %.3e <= %.3e  dk %.3e <= %.3e" % (e_dq, eps * nrm(k), e_dk, eps * nrm(q) * q.shape[1] * G))
    assert e_dq <= eps * nrm(k), ("dq", e_dq)
    assert e_dk <= eps * nrm(q) * q.shape[1] * G, ("dk", e_dk)


def _check(got, q, k, v, dout, p, seed, causal=False, kv_len=None, doc_ids=None, window=None, group=""):
    """The per-row bound of o / dq / dk / dv and the lse tolerance, against the oracle."""
    args = [t.cpu() for t in (q, k, v, dout)] + [causal, None if kv_len is None else torch.tensor(kv_len), None]
    kw = dict(doc_ids=doc_ids, window=window, dropout_p=p, dropout_seed=seed)
    exact, emu = ref.attention(*args, **kw), ref.attention(*args, emulate_bf16=True, **kw)
    fails = []
    for name, g, x, e in zip(NAMES, got, exact, emu):
        g = g.detach().cpu()
        if name == "lse":
            fin = torch.isfinite(x)
            assert torch.isfinite(g[fin]).all(), name
            assert torch.equal(g[~fin], torch.full_like(g[~fin], math.inf)), "lse of rows with no key"
            torch.testing.assert_close(g[fin].double(), x[fin], rtol=1e-3, atol=2e-3)
            continue
        assert torch.isfinite(g.float()).all(), name
        if torch.count_nonzero(x) == 0:
            assert k.shape[1] == 1 and name in ("dq", "dk"), name
            continue
        ek, ee = ref.attention_row_error(g, x), ref.attention_row_error(e, x)
        print("ATTN_DROP %s p=%.1f %s E_kernel %.5f E_emulated %.5f ratio %.3f" % (group, p, name, ek, ee, ek / ee if ee else 0.0))
        if not ek <= 2 * ee:
            err = (g.double() - x).norm(dim=-1)
            b, s, h = (int(i) for i in (err == err.max()).nonzero()[0])
            fails.append("%s: E_kernel %.5f > 2 * E_emulated %.5f, worst row (b %d, s %d, h %d)" % (name, ek, ee, b, s, h))
    if k.shape[1] == 1:
        _check_one_key(got, q, k, v, dout, p)
    assert not fails, "; ".join(fails)


def _seed_with_a_kept_row(p, B, H, Sq, Sk, start=SEED):
    """The first seed from ``start`` at which some element is kept (a non-zero reference) and, where
    there are at least two elements, some element is dropped too (tiny problems only)."""
    for s in range(start, start + 1000):
        m = ref.dropout_keep_mask(s, p, B, H, Sq, Sk)
        if m.flatten(2).any(-1).any() and (m.numel() < 2 or not m.all()):
            return s
    raise AssertionError("no such seed")


# -------------------------------------------------------------- the mask, out of the forward
def _read_mask(B, Sq, Sk, Hq, Hkv, D, p, seed, causal=False, kv_len=None, bounds=None):
    """bool [B, Hq, Sq, Sk]: where the forward kernel kept a visible key (see the module docstring)."""
    hnn = _hnn()
    q = torch.zeros(B, Sq, Hq, D, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(B, Sk, Hkv, D, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(B, Hq, Sq, Sk, dtype=torch.bool, device="cuda")
    r = (None, None) if bounds is None else (bounds.klo, bounds.khi)
    for off in range(0, Sk, D):
        n = min(D, Sk - off)
        v = torch.zeros(B, Sk, Hkv, D, dtype=torch.bfloat16, device="cuda")
        v[:, off + torch.arange(n), :, torch.arange(n)] = 1
        o, _ = hnn.native().attn_forward(q, k, v, causal, D ** -0.5, _kvlen(kv_len), r[0], r[1], p, seed)
        assert torch.count_nonzero(o[..., n:]) == 0
        out[..., off:off + n] = (o[..., :n] != 0).permute(0, 2, 1, 3)
    return out.cpu()


def _visible(B, Sq, Sk, causal=False, kv_len=None, dense=None):
    m = torch.ones(B, 1, Sq, Sk, dtype=torch.bool)
    keys = torch.arange(Sk)
    if causal:
        m = m & (keys[None, :] <= torch.arange(Sq)[:, None])
    if kv_len is not None:
        m = m & (keys < torch.tensor(kv_len).view(B, 1, 1, 1))
    if dense is not None:
        m = m & dense.cpu()[:, None]
    return m


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk", [(1, 1), (33, 65), (130, 257)])
def test_mask_read_out_of_the_forward(Sq, Sk, D, p):
    B, Hq = 2, 3
    want = ref.dropout_keep_mask(SEED, p, B, Hq, Sq, Sk)
    assert torch.equal(_read_mask(B, Sq, Sk, Hq, 3, D, p, SEED), want)
    if (Sq, Sk) == (33, 65):  # grouped heads: the hash takes the query head
        assert torch.equal(_read_mask(B, Sq, Sk, Hq, 1, D, p, SEED), want)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("mode", ["causal", "kv_len", "documents"])
def test_mask_read_out_under_masks(mode, D, p):
    """Causal (tiles above the diagonal are skipped), a key length inside a tile, and a two-document
    row range: the kept set is the twin's mask ANDed with the visibility, whatever was skipped."""
    B, Hq, S = 2, 3, 130
    keep = ref.dropout_keep_mask(SEED + 1, p, B, Hq, S, S if mode != "kv_len" else 257)
    if mode == "causal":
        got = _read_mask(B, S, S, Hq, 3, D, p, SEED + 1, causal=True)
        vis = _visible(B, S, S, causal=True)
    elif mode == "kv_len":
        kv_len = [70, 200]
        got = _read_mask(B, S, 257, Hq, 1, D, p, SEED + 1, kv_len=kv_len)
        vis = _visible(B, S, 257, kv_len=kv_len)
    else:
        doc_ids = torch.tensor([[0] * 50 + [1] * 80, [3] * 97 + [4] * 33])
        bd = _bounds(S, doc_ids, None, False)
        got = _read_mask(B, S, S, Hq, 3, D, p, SEED + 1, bounds=bd)
        vis = _visible(B, S, S, dense=bd.dense_mask())
    assert torch.equal(got, keep & vis)


@pytest.mark.parametrize("p", PS)
def test_device_twin_at_arbitrary_indices(p):
    hnn = _hnn()
    rng = np.random.default_rng(7)
    n, top = 100_000, (1 << 24) - 1
    b = rng.integers(0, 1 << 16, n)
    h = rng.integers(0, 1 << 10, n)
    i = rng.integers(0, top + 1, n)
    j = rng.integers(0, top + 1, n)
    corners = [(0, 0, 0, 0), (0, 0, top, top), (0, 0, top, 0), (0, 0, 0, top), (0, 0, top - 1, top - 1),
               ((1 << 32) - 1, top, top, top), (1, 0, 5, 7), (0, top, 5, 7), (0, 1, 5, 7), (1 << 8, 0, 5, 7)]
    for c in corners:
        b, h, i, j = (np.append(a, x) for a, x in zip((b, h, i, j), c))
    for seed in (0, SEED, (1 << 64) - 1):
        want = ref.dropout_keep(seed, p, b, h, i, j)
        got = hnn.native().attn_dropout_keep(seed, p, *(torch.from_numpy(a.astype(np.int64)).cuda() for a in (b, h, i, j)))
        assert got.dtype == torch.uint8 and got.shape == (n + len(corners),)
        assert np.array_equal(got.cpu().numpy().astype(bool), want)


# --------------------------------------------------------------------------------- numerics
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 31, 33, 64, 65, 127, 129, 257])
def test_self_attention(S, D, p):
    seed = _seed_with_a_kept_row(p, 2, 2, S, S) if S == 1 else SEED + S
    t = _inputs(2, S, S, 2, 2, D, seed=100 + S + D)
    _check(_kernel(*t, p, seed), *t, p, seed, group="self")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk", [(70, 200), (200, 70)])
def test_cross_attention(Sq, Sk, D, p):
    t = _inputs(2, Sq, Sk, 2, 2, D, seed=200 + Sq + D)
    _check(_kernel(*t, p, SEED), *t, p, SEED, group="cross")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [65, 129, 257])
def test_causal(S, D, p):
    t = _inputs(2, S, S, 2, 2, D, seed=300 + S + D)
    _check(_kernel(*t, p, SEED + 3, causal=True), *t, p, SEED + 3, causal=True, group="causal")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kv_len,causal", [([0, 63], False), ([1, 65], False), ([200, 64], False), ([1, 65], True)])
def test_key_padding(kv_len, causal, D, p):
    """Key lengths 0 / 1 / 63 / 65 / above Sk (= 129): a fully padded batch row gives zeros and
    lse = +inf; padded keys get exactly zero dk / dv."""
    t = _inputs(2, 129, 129, 2, 2, D, seed=400 + D + kv_len[0])
    got = _kernel(*t, p, SEED + 4, causal=causal, kv_len=kv_len)
    _check(got, *t, p, SEED + 4, causal=causal, kv_len=kv_len, group="padding")
    o, lse, dq, dk, dv = got
    for b, n in enumerate(kv_len):
        assert torch.count_nonzero(dk[b, n:]) == 0 and torch.count_nonzero(dv[b, n:]) == 0, b
        if n == 0:
            for x in (o, dq, dk, dv):
                assert torch.count_nonzero(x[b]) == 0
            assert (lse[b] == math.inf).all()


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_documents_and_window(causal, D, p):
    """Documents cut at 32 / 64 / 100 with a window of 40: the row-range (BND) DROP kernels."""
    S = 129
    doc_ids = torch.tensor([[0] * 32 + [1] * 32 + [2] * 36 + [3] * 29, [0] * 64 + [1] * 36 + [2] * 29])
    bd = _bounds(S, doc_ids, 40, causal)
    t = _inputs(2, S, S, 2, 2, D, seed=500 + D + causal)
    got = _kernel(*t, p, SEED + 5, causal=causal, bounds=bd)
    _check(got, *t, p, SEED + 5, causal=causal, doc_ids=doc_ids, window=40, group="documents")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (3, 1), (4, 1)])
def test_gqa_groups(Hq, Hkv, D, p):
    """Groups of 1, 3 (odd: the unsplit dK/dV loop runs over three query heads) and 4 (the small
    grid splits the group: fp32 partials and k_attn_gsum)."""
    t = _inputs(2, 129, 129, Hq, Hkv, D, seed=600 + 10 * Hq + D)
    causal = Hq == 4
    _check(_kernel(*t, p, SEED + 6, causal=causal), *t, p, SEED + 6, causal=causal, group="gqa")


def test_long_sequence():
    t = _inputs(2, 1000, 1000, 2, 1, 64, seed=700)
    _check(_kernel(*t, 0.1, SEED + 7, causal=True), *t, 0.1, SEED + 7, causal=True, group="S=1000")


# ------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("D,causal", [(64, False), (128, True)])
def test_packed_qkv_route_is_the_same_function(D, causal):
    t = _inputs(2, 130, 130, 2, 2, D, seed=800 + D)
    a = _kernel(*t, 0.1, SEED + 8, causal=causal, kv_len=[130, 77])
    b = _kernel(*t, 0.1, SEED + 8, causal=causal, kv_len=[130, 77], packed=True)
    for x, y, nm in zip(a, b, NAMES):
        assert torch.equal(x, y), nm


@pytest.mark.parametrize("D", [64, 128])
def test_rope_packed_route_is_the_same_function(D):
    """rope_attention_packed against RoPE (the same kernel, into separate tensors) followed by
    hnn.attention and the inverse rotation of dq / dk: equal bits with one explicit seed."""
    hnn = _hnn()
    C = hnn.native()
    B, S, hq, hkv = 2, 130, 4, 2
    q, k, v, dout = _inputs(B, S, S, hq, hkv, D, seed=900 + D)
    inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    f = torch.outer(torch.arange(S, dtype=torch.float32), inv)
    cos, sin = f.cos().contiguous().cuda(), f.sin().contiguous().cuda()
    y = torch.cat([t.flatten(2) for t in (q, k, v)], dim=2).contiguous().requires_grad_(True)
    assert hnn.rope_attention_packed_ok(y, cos, hq, hkv)
    o = hnn.rope_attention_packed(y, cos, sin, hq, hkv, dropout_p=0.1, dropout_seed=SEED + 9)
    o.backward(dout)
    dq, dk, dv = (t.reshape(B, S, -1, D) for t in y.grad.split([hq * D, hkv * D, hkv * D], dim=-1))
    qr, kr = torch.empty_like(q), torch.empty_like(k)
    C.rope_apply(q.view(B * S, hq * D), qr.view(B * S, hq * D), cos, sin, S, D, 1.0)
    C.rope_apply(k.view(B * S, hkv * D), kr.view(B * S, hkv * D), cos, sin, S, D, 1.0)
    qa, ka, va = (t.detach().requires_grad_(True) for t in (qr, kr, v))
    o2 = hnn.attention(qa, ka, va, causal=True, dropout_p=0.1, dropout_seed=SEED + 9)
    o2.backward(dout)
    gq, gk = qa.grad.contiguous(), ka.grad.contiguous()
    C.rope_apply(gq.view(B * S, hq * D), gq.view(B * S, hq * D), cos, sin, S, D, -1.0)
    C.rope_apply(gk.view(B * S, hkv * D), gk.view(B * S, hkv * D), cos, sin, S, D, -1.0)
    assert torch.equal(o.detach(), o2.detach())
    assert not torch.equal(o.detach(), hnn.rope_attention_packed(y, cos, sin, hq, hkv).detach())
    for x, w, nm in ((dq, gq, "dq"), (dk, gk, "dk"), (dv, va.grad, "dv")):
        assert torch.equal(x, w), nm


# ------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("D,causal", [(64, True), (128, False)])
def test_determinism_and_extent(D, causal):
    """The same seed twice: equal bits; another seed: another result.  Batch row 0 and query heads
    0 .. 1 (kv head 0) of a larger problem with equal leading data: all five outputs equal bits
    (the GQA group of 2 is split in two slices at every extent here, so dk / dv sum alike)."""
    q, k, v, dout = _inputs(2, 193, 193, 4, 2, D, seed=1000 + D)
    a = _kernel(q, k, v, dout, 0.1, SEED, causal=causal)
    b = _kernel(q, k, v, dout, 0.1, SEED, causal=causal)
    for x, y, nm in zip(a, b, NAMES):
        assert torch.equal(x, y), nm
    c = _kernel(q, k, v, dout, 0.1, SEED + 1, causal=causal)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[2], c[2]) and not torch.equal(a[4], c[4])
    assert torch.equal(a[1], c[1])  # lse is that of the undropped P
    one = _kernel(q[:1], k[:1], v[:1], dout[:1], 0.1, SEED, causal=causal)
    for i, nm in enumerate(NAMES):
        assert torch.equal(one[i], a[i][:1]), nm
    heads = _kernel(q[:, :, :2], k[:, :, :1], v[:, :, :1], dout[:, :, :2], 0.1, SEED, causal=causal)
    assert torch.equal(heads[0], a[0][:, :, :2])
    assert torch.equal(heads[1], a[1][:, :2])
    assert torch.equal(heads[2], a[2][:, :, :2])
    assert torch.equal(heads[3], a[3][:, :, :1]) and torch.equal(heads[4], a[4][:, :, :1])


@pytest.mark.parametrize("D,causal", [(64, False), (128, True)])
def test_p_zero_is_the_plain_call(D, causal):
    hnn = _hnn()
    q, k, v, dout = _inputs(2, 129, 129, 4, 2, D, seed=1100 + D)

    def run(**kw):
        qa, ka, va = (t.detach().requires_grad_(True) for t in (q, k, v))
        o = hnn.attention(qa, ka, va, causal=causal, **kw)
        o.backward(dout)
        return o.detach(), qa.grad, ka.grad, va.grad

    base = run()
    for kw in ({"dropout_p": 0.0}, {"dropout_p": 0.0, "dropout_seed": 5}, {"dropout_p": 0.001, "dropout_seed": 5}):
        for x, y in zip(run(**kw), base):
            assert torch.equal(x, y), kw
    sc = D ** -0.5
    o0, lse0 = hnn.native().attn_forward(q, k, v, causal, sc, None)
    o1, lse1 = hnn.native().attn_forward(q, k, v, causal, sc, None, None, None, 0.001, 99)  # threshold 0
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)
    g0 = hnn.native().attn_backward(dout, q, k, v, o0, lse0, causal, sc, None)
    g1 = hnn.native().attn_backward(dout, q, k, v, o0, lse0, causal, sc, None, None, None, None, None, None, None,
                                    None, 0.001, 99)
    for x, y in zip(g0, g1):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------ models
def _no_sdpa(*a, **k):
    raise AssertionError("F.scaled_dot_product_attention called: not the kernel route")


def _model_checks(m0, m1, ids, monkeypatch):
    import torch.nn.functional as F
    hnn = _hnn()
    monkeypatch.setattr(F, "scaled_dot_product_attention", _no_sdpa)
    m1.load_state_dict(m0.state_dict())
    labels = ids.clone()

    def fwd(m, with_loss=False):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return m(ids, labels) if with_loss else m(ids)

    m0.eval(), m1.eval()
    with torch.no_grad():
        e0, e1 = fwd(m0), fwd(m1)
    assert torch.equal(e0, e1)
    m1.train()
    state = hnn.dropout_rng_state()
    with torch.no_grad():
        a, b = fwd(m1), fwd(m1)
    assert not torch.equal(a, b) and not torch.equal(a, e1)
    hnn.set_dropout_rng_state(state)
    with torch.no_grad():
        assert torch.equal(fwd(m1), a)
    hnn.set_dropout_rng_state(state)
    loss = fwd(m1, with_loss=True)
    loss.backward()
    torch.cuda.synchronize()
    g1 = {n: p.grad.clone() for n, p in m1.named_parameters() if p.grad is not None}
    m0.train()
    fwd(m0, with_loss=True).backward()  # every parameter the loss reaches (not Bert's pooler) has a gradient
    assert set(g1) == {n for n, p in m0.named_parameters() if p.grad is not None} and len(g1) > 10
    for n, g in g1.items():
        assert torch.isfinite(g.float()).all(), n
    m1.zero_grad(set_to_none=True)
    hnn.set_dropout_rng_state(state)
    loss2 = fwd(m1, with_loss=True)
    loss2.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2)
    for n, g in g1.items():
        assert torch.equal(m1.get_parameter(n).grad, g), n


def test_bert_with_attention_dropout(monkeypatch):
    from hipps.models import transformer as tf

    cfg = dict(vocab=512, hidden=128, layers=2, heads=2, ffn=256, max_pos=128)
    torch.manual_seed(0)
    m0 = tf.Bert(tf.BertConfig(**cfg)).cuda()
    m1 = tf.Bert(tf.BertConfig(attn_dropout=0.1, **cfg)).cuda()
    ids = torch.randint(0, 512, (2, 96), device="cuda")
    _model_checks(m0, m1, ids, monkeypatch)


def test_llama_with_attention_dropout(monkeypatch):
    from hipps.models import transformer as tf
    hnn = _hnn()

    cfg = dict(vocab=512, dim=256, layers=2, heads=4, kv_heads=2, ffn=512, max_seq=128)
    torch.manual_seed(0)
    m0 = tf.Llama(tf.LlamaConfig(**cfg)).cuda()
    m1 = tf.Llama(tf.LlamaConfig(attn_dropout=0.1, **cfg)).cuda()
    ids = torch.randint(0, 512, (2, 96), device="cuda")
    calls = []
    packed = hnn.rope_attention_packed
    monkeypatch.setattr(hnn, "rope_attention_packed", lambda *a, **k: (calls.append(k.get("dropout_p")), packed(*a, **k))[1])
    _model_checks(m0, m1, ids, monkeypatch)
    assert 0.1 in calls and 0.0 in calls  # the RoPE-packed route, with and without dropout


# -------------------------------------------------------------------------------- rejections
@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, math.nan])
def test_rejections(bad):
    hnn = _hnn()
    q, k, v, dout = _inputs(1, 40, 40, 2, 2, 64, seed=1200)
    with pytest.raises(ValueError):
        hnn.attention(q, k, v, dropout_p=bad)
    with pytest.raises(ValueError):
        hnn.attention_qkv(torch.stack((q, k, v), dim=2), dropout_p=bad)
    with pytest.raises(RuntimeError, match="dropout_p"):
        hnn.native().attn_forward(q, k, v, False, 0.125, None, None, None, bad, 1)
    o, lse = hnn.native().attn_forward(q, k, v, False, 0.125, None)
    with pytest.raises(RuntimeError, match="dropout_p"):
        hnn.native().attn_backward(dout, q, k, v, o, lse, False, 0.125, None, None, None, None, None, None, None,
                                   None, bad, 1)
    idx = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="dropout_p"):
        hnn.native().attn_dropout_keep(1, bad, idx, idx, idx, idx)
