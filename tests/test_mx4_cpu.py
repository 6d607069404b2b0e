"""The mx4 codec (OCP MXFP4: e2m1 codes, one E8M0 scale byte per 32 elements) on CPU: the twin in
hipps/ops/reference.py defines the wire format, these tests pin it -- sizes, the rounding ladder,
the scale rule, non-finite blocks, idempotence, the per-element error bound, error-feedback
conservation -- and run it through the sync engines, the async PS and a checkpoint."""
import math

import numpy as np
import pytest
import torch

from dist_util import run_world
from test_dist_cpu import _data, _mlp, _train

from hipps import get_codec
from hipps.ops import reference as ref

GRID = np.array(ref.MX4_GRID, dtype=np.float64)
FLT_MAX = float(np.finfo(np.float32).max)


def heavy(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.exp(2 * torch.randn(n, generator=g))


def encode(x, resid=None):
    n = x.numel()
    q = torch.empty((n + 1) // 2, dtype=torch.uint8)
    s = torch.empty((n + 31) // 32, dtype=torch.uint8)
    ref.mx4_encode(x, resid, q, s)
    return q, s


def _near(t):
    t = np.float32(t)
    return [np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(np.inf))]


def crafted():
    """Every ladder tie and both neighbours in both signs under a block maximum of 6 * 2^e, block
    maxima of exactly 1.5 * 2^k and one ulp above, and the special blocks; 32-element blocks plus a
    5-element tail."""
    rng = np.random.default_rng(7)
    blocks = []
    for e in (-20, 0, 20):
        vals = [np.float32(v) for t in (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0) for v in _near(t)]
        vals = vals + [-v for v in vals] + [np.float32(0.0), np.float32(-0.0), np.float32(-0.1), np.float32(0.1)]
        vals = [np.float32(6.0)] + vals[:31] + [np.float32(-6.0)] + vals[31:]
        vals += [np.float32(0.0)] * (-len(vals) % 32)
        blocks.append(np.ldexp(np.array(vals, dtype=np.float32), e))
    for k in (-3, 0, 5):
        for top in (np.float32(1.5), np.nextafter(np.float32(1.5), np.float32(2))):
            b = (rng.standard_normal(32) * 0.3).astype(np.float32)
            b[int(rng.integers(32))] = -top if k == 0 else top
            blocks.append(np.ldexp(b, k))
    z = np.zeros(32, dtype=np.float32)
    small = np.ldexp(rng.standard_normal(32).astype(np.float32), -102)
    small[:4] = [2.0 ** -101, -(2.0 ** -110), 2.0 ** -126, 1e-40]
    assert np.abs(small).max() < 2.0 ** -100
    edge = small.copy()  # the smallest scale the encoder emits: amax exactly 2^-100, e = -102
    edge[11] = -(2.0 ** -100)
    blocks.append(edge)
    inf, ninf, nan, big = (rng.standard_normal(32).astype(np.float32) for _ in range(4))
    inf[5], ninf[31], nan[0], nan[17] = np.inf, -np.inf, np.nan, np.inf
    big *= np.float32(1e37)
    big[3], big[4], big[9] = FLT_MAX, -FLT_MAX, 2.0 ** 125
    blocks += [z, small, inf, rng.standard_normal(32).astype(np.float32), ninf, nan, big,
               rng.standard_normal(5).astype(np.float32)]
    return torch.from_numpy(np.concatenate(blocks))


def test_layout_size():
    c = get_codec("mx4")
    assert type(get_codec("mxfp4")) is type(c) and c.name == "mx4" and c.error_feedback
    a16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    for n in (1, 2, 31, 32, 33, 511, 4099, 25557032):
        assert c.nbytes(n) == a16(math.ceil(n / 32)) + a16(math.ceil(n / 2))
        lay = c.layout(n)
        assert [(f.name, f.dtype, f.numel) for f in lay.fields] == [("scales", torch.uint8, math.ceil(n / 32)),
                                                                    ("q", torch.uint8, math.ceil(n / 2))]


def test_ladder_is_nearest_even():
    """Under a block maximum of 6 (e = 0) the code of y is the nearest grid point, ties to the even
    code: a brute-force search in fp64 over 240 001 points plus every tie and its neighbours."""
    y = np.linspace(0.0, 6.0, 240001).astype(np.float32)
    y = np.concatenate([y, np.array([v for t in (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0) for v in _near(t)], np.float32)])
    y = np.concatenate([y, np.zeros(-len(y) % 31, np.float32)]).reshape(-1, 31)
    x = np.concatenate([np.full((len(y), 1), 6.0, np.float32), y], axis=1)
    q, s = encode(torch.from_numpy(x.reshape(-1)))
    assert (s == 127).all()
    got = torch.stack([q & 15, q >> 4], dim=1).view(-1).numpy()
    d = np.abs(x.reshape(-1).astype(np.float64)[:, None] - GRID[None, :])
    best = d.min(axis=1, keepdims=True)
    cand = d == best  # one or two codes
    want = np.where(cand.sum(axis=1) == 1, cand.argmax(axis=1),
                    np.where(cand[:, ::2].any(axis=1), 2 * cand[:, ::2].argmax(axis=1), -1))
    assert (want >= 0).all() and np.array_equal(got, want)


@pytest.mark.parametrize("amax,byte,code,deq", [
    (1.0, 125, 6, 1.0), (1.5, 125, 7, 1.5), (float(np.nextafter(np.float32(1.5), np.float32(2))), 126, 5, 1.5),
    (6.0, 127, 7, 6.0), (2.0 ** -100, 25, 6, 2.0 ** -100),
    (float(np.nextafter(np.float32(2.0 ** -100), np.float32(0))), 0, 0, 0.0), (FLT_MAX, 252, 7, 6 * 2.0 ** 125)])
def test_scale_rule(amax, byte, code, deq):
    x = torch.zeros(32)
    x[3] = -amax
    r = torch.zeros(32)
    q, s = encode(x, r)
    assert int(s[0]) == byte
    assert int(q[1]) == ((8 | code) << 4 if byte else 0)
    d = ref.mx4_dequant(q, s, 32)
    assert torch.isfinite(d).all() and d[3].item() == -deq and d.abs().sum().item() == deq
    assert torch.equal(r, x - d)  # byte 0: the whole block stays in the residual


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_nonfinite_block(bad):
    x = heavy(96, 3)
    clean_q, clean_s = encode(x)
    x[40] = bad
    r = torch.full((96,), 0.0)
    q, s = encode(x, r)
    assert int(s[1]) == 255 and (q[16:32] == 0).all() and (r[32:64] == 0).all()
    d = ref.mx4_dequant(q, s, 96)
    assert torch.isnan(d[32:64]).all() and torch.isfinite(d[:32]).all() and torch.isfinite(d[64:]).all()
    for sl, bl in ((slice(0, 16), 0), (slice(32, 48), 2)):  # the neighbouring blocks are untouched
        assert torch.equal(q[sl], clean_q[sl]) and s[bl] == clean_s[bl]


def test_decode_encode_decode_is_identity():
    for x in (heavy(4099, 1), crafted()):
        n = x.numel()
        d = ref.mx4_dequant(*encode(x), n)
        d2 = ref.mx4_dequant(*encode(d), n)
        assert torch.equal(torch.isnan(d), torch.isnan(d2))
        assert torch.equal(d.nan_to_num(7.0).view(torch.int32), d2.nan_to_num(7.0).view(torch.int32))


@pytest.mark.parametrize("kind", ["normal", "heavy"])
def test_per_element_error_bound(kind):
    """|v - deq| <= max(|v|, 2^e) / 4: the grid spacing is 2^e / 2 below 2^(e+1) and at most half
    the value's binade above, and nothing saturates.  Every element, nothing excluded."""
    n = 1 << 16
    x = torch.randn(n, generator=torch.Generator().manual_seed(5)) if kind == "normal" else heavy(n, 5)
    q, s = encode(x)
    assert ((s >= 25) & (s <= 252)).all()
    d = ref.mx4_dequant(q, s, n).double()
    unit = torch.ldexp(torch.ones(n, dtype=torch.float64), s.int().repeat_interleave(32)[:n] - 127)
    assert ((x.double() - d).abs() <= torch.maximum(x.double().abs(), unit) / 4).all()


def test_error_feedback_conserves_the_sum():
    """sum g - sum deq - r over T steps: two fp32 roundings per step (v = g + r, r = v - deq)."""
    n, T = 4099, 50
    r = torch.zeros(n)
    sg, sd = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    vmax = 0.0
    for t in range(T):
        g = heavy(n, 100 + t)
        vmax = max(vmax, (g + r).abs().max().item())
        q, s = encode(g, r)
        sg += g.double()
        sd += ref.mx4_dequant(q, s, n).double()
    assert ((sg - sd - r.double()).abs() <= T * 2.0 ** -23 * vmax).all()
    assert r.abs().max() > 0


def test_aggregate_modes_and_object_api():
    n = 257
    msgs = [encode(heavy(n, 20 + w)) for w in range(3)]
    deq = [ref.mx4_dequant(q, s, n) for q, s in msgs]
    g = torch.tensor(1 / 3, dtype=torch.float32)
    acc = torch.full((n,), 9.0)
    ref.mx4_aggregate([m[0] for m in msgs], [m[1] for m in msgs], acc, 1 / 3, False)
    assert torch.equal(acc, ((deq[0] + deq[1]) + deq[2]) * g)
    acc = torch.full((n,), 9.0)
    ref.mx4_aggregate([m[0] for m in msgs], [m[1] for m in msgs], acc, 1 / 3, True)
    assert torch.equal(acc, ((9.0 + deq[0] * g) + deq[1] * g) + deq[2] * g)
    c = get_codec("mx4")
    x = heavy(300, 2).view(3, 100)
    assert torch.equal(c.decode(c.encode(x)), ref.mx4_dequant(*encode(x.reshape(-1)), 300).view(3, 100))


def test_allgather_two_ranks_replicas_identical():
    out = run_world(_train, 2, "allgather", "mx4", 3, "sgd")
    for a, b in zip(out[0][0], out[1][0]):
        assert torch.equal(a, b)
    assert out[0][1]["grad_bytes_sent"] > 0


def _async_train(rank, world, steps):
    import hipps

    def mean_loss(m):
        with torch.no_grad():
            return sum(torch.nn.functional.cross_entropy(m(x), y).item() for x, y in (_data(0, b) for b in range(4))) / 4

    m = _mlp()
    first = mean_loss(m)
    opt = hipps.SGD(m.named_parameters(), lr=0.05, momentum=0.9, mode="ps_async", code="mx4", max_delay=0)
    for s in range(steps):
        x, y = _data(0, s % 4)
        opt.zero_grad()
        torch.nn.functional.cross_entropy(m(x), y).backward()
        opt.step()
    opt.close()
    return first, mean_loss(m)


def test_ps_async_trains():
    first, last = run_world(_async_train, 1, 40)[0]
    print("mean loss over the four batches: step 0 %.4g, after 40 steps %.4g" % (first, last))
    assert last < 0.1 * first


def _ckpt(rank, world, path):
    import hipps
    from hipps.utils import checkpoint

    def make():
        m = _mlp()
        return m, hipps.SGD(m.named_parameters(), lr=0.05, momentum=0.9, mode="ps_async", code="mx4", max_delay=0,
                            bucket_mb=0.0005)

    m, opt = make()
    for s in range(3):
        x, y = _data(0, s)
        opt.zero_grad()
        torch.nn.functional.cross_entropy(m(x), y).backward()
        opt.step()
    saved = [st["resid"].clone() for st in opt.engine.codec_state]
    checkpoint.save(opt, path, m)
    opt.close()
    m, opt = make()
    fresh = [st["resid"].clone() for st in opt.engine.codec_state]
    checkpoint.load(opt, path, m)
    loaded = [st["resid"].clone() for st in opt.engine.codec_state]
    opt.close()
    return saved, fresh, loaded


def test_checkpoint_restores_the_residual(tmp_path):
    saved, fresh, loaded = run_world(_ckpt, 1, str(tmp_path / "ck"))[0]
    assert len(saved) > 1 and all(s.abs().max() > 0 for s in saved) and all(f.abs().max() == 0 for f in fresh)
    for a, b in zip(saved, loaded):
        assert torch.equal(a, b)
