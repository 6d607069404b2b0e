"""bn3 + residual + ReLU fused into the next block's conv1 GEMM (hipps/csrc/bnconv.hip) against the
two kernels it replaces: the BN apply pass (norm.hip) and the 1x1 GEMM with the statistics
epilogue (gemm2.hip / gemm.hip) at the same 128-row tile.  Everything must be bit-identical: the
block output, its ReLU bits, the conv output and its statistics partials.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
# (imgs, h, K, N): M = 98 < one tile; M = 243: a tail tile, bits end in a partial wave (3888 bytes);
# eight K tiles; four column tiles (out written once)
SHAPES = [(2, 7, 256, 64), (3, 9, 128, 128), (2, 14, 512, 128), (2, 7, 2048, 512)]
CASES = [(s, False) for s in SHAPES] + [(s, True) for s in SHAPES[:2]]


def C():
    from hipps.ops._native import native

    return native()


def _act(n, c, h, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, c, h, h, generator=g).to(DEV).to(torch.bfloat16).contiguous(memory_format=CL)


def _partials(x):
    """[2, C, 1] statistics partials of x (one row block)."""
    xf = x.float()
    return torch.stack([xf.sum((0, 2, 3)), (xf * xf).sum((0, 2, 3))]).unsqueeze(2).contiguous()


def _bn_params(c, seed):
    """BN weights of both signs and biases around zero (about half of relu's inputs clamp);
    channels 0..7: weight = bias = 0, so the BN term is exactly 0 there."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = torch.randn(c, generator=g)
    b = torch.randn(c, generator=g) * 0.3
    w[:8] = 0
    b[:8] = 0
    return w.to(DEV), b.to(DEV)


@pytest.mark.parametrize("shape,dual", CASES)
def test_bnconv_bitwise_against_apply_then_gemm(shape, dual):
    n, h, K, N = shape
    M = n * h * h
    x3, res = _act(n, K, h, 1), _act(n, K, h, 2)
    # rows whose residual is zero: with the zeroed channels, v is exactly 0 there
    r2 = res.permute(0, 2, 3, 1).reshape(M, K)
    for row in (0, 5, M - 1):
        r2[row].zero_()
    w = (torch.randn(N, K, device=DEV) / K ** 0.5).to(torch.bfloat16)
    w3, b3 = _bn_params(K, 3)
    wd, bd = _bn_params(K, 4)
    f32 = dict(dtype=torch.float32, device=DEV)
    v3 = [torch.empty(K, **f32) for _ in range(4)]  # mean, invstd, scale, shift
    vd = [torch.empty(K, **f32) for _ in range(4)]
    rm, rv = torch.zeros(K, **f32), torch.ones(K, **f32)
    out_ref = torch.empty_like(x3)
    bits_ref = torch.empty(M * K // 8, dtype=torch.uint8, device=DEV)
    p3 = _partials(x3)
    if dual:
        C().bn_dual_forward(p3, 1, _partials(res), 1, x3, res, out_ref, bits_ref, w3, b3, rm, rv, *v3, wd, bd,
                            rm.clone(), rv.clone(), *vd, K, 1e-5, 0.1, 1e-5, 0.1)
        rsc, rsh = vd[2], vd[3]
    else:
        C().bn_forward_partials(p3, 1, x3, res, out_ref, w3, b3, rm, rv, *v3, K, 1e-5, 0.1, True, bits_ref)
        rsc = rsh = None
    y_ref = torch.empty(n, N, h, h, device=DEV, dtype=torch.bfloat16).contiguous(memory_format=CL)
    p_ref = torch.empty(2, N, C().gemm2_mtiles(M, N, K, 128), device=DEV)
    C().gemm2_conv(out_ref, w, y_ref, p_ref, None, None, h, h, 1, 1, 1, 0, 128, 128 if N % 128 == 0 else 64)

    out = torch.full_like(x3, 7.0)
    bits = torch.full_like(bits_ref, 0xA5)
    y = torch.full_like(y_ref, 7.0)
    part = torch.full((2, N, C().bnconv_mtiles(M)), 7.0, device=DEV)
    C().bnconv_forward(x3, res, v3[2], v3[3], rsc, rsh, w, out, bits, y, part)
    torch.cuda.synchronize()

    of = out_ref.float()
    frac = (of == 0).float().mean().item()
    assert 0.25 < frac < 0.75, frac  # the inputs do clamp about half of the elements
    assert (of.permute(0, 2, 3, 1).reshape(M, K)[0, :8] == 0).all()
    assert torch.equal(out, out_ref)
    assert torch.equal(bits, bits_ref)
    assert torch.equal(y, y_ref)
    assert part.shape == p_ref.shape and torch.equal(part, p_ref)
    if N % 128 == 0:  # the first core's 128-wide tile splits its rows the same way
        y1 = torch.empty_like(y_ref)
        p1 = torch.empty(2, N, C().conv1x1_mtiles(M), device=DEV)
        C().conv1x1_forward(out_ref, w, y1, p1, h, h, 1)
        assert torch.equal(y, y1) and torch.equal(part, p1)
    ref = out.float().permute(0, 2, 3, 1).reshape(M, K) @ w.float().t()
    torch.testing.assert_close(y.float().permute(0, 2, 3, 1).reshape(M, N), ref, rtol=2e-2, atol=2e-2)
    # the apply pass alone (what a deferred output without a conv1 consumer runs)
    out2, bits2 = torch.full_like(x3, 7.0), torch.full_like(bits_ref, 0xA5)
    C().bn_apply_bits(x3, res, out2, bits2, v3[2], v3[3], rsc, rsh, K)
    assert torch.equal(out2, out_ref) and torch.equal(bits2, bits_ref)


def _run_blocks(blocks0, x0, wsum, fused, routes, monkeypatch):
    import hipps.ops.nn as hnn

    monkeypatch.setattr(hnn, "_FUSED_BNCONV", fused)
    del routes[:]
    blocks = copy.deepcopy(blocks0)
    x = x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = x
        for b in blocks:  # every block defers: the last one's output is flushed before the pool
            y = b(y, defer_out=True)
        pending = getattr(y, "_hipps_pending", None) is not None
        out = hnn.global_avg_pool(hnn.materialize(y))
    (out.float() * wsum).sum().backward()
    torch.cuda.synchronize()
    grads, stats = {}, {}
    for i, b in enumerate(blocks):
        grads.update({f"{i}.{n}": p.grad.clone() for n, p in b.named_parameters()})
        stats.update({f"{i}.{n}": v.clone() for n, v in b.named_buffers() if "running" in n})
    return out.detach().clone(), x.grad.clone(), grads, stats, list(routes), pending


def test_blocks_fused_boundary_bitwise(monkeypatch):
    """Two identity blocks and a downsample pair, imgs 2, 8x8: HIPPS_FUSED_BNCONV on (every eligible
    boundary on the fused kernel) against off, same tuner picks: the output, every gradient and
    the BN running statistics are bit-identical; the last output is flushed by the plain kernel."""
    import hipps.ops.nn as hnn
    from hipps.models.resnet import Bottleneck

    torch.manual_seed(0)
    blocks = [Bottleneck(256, 64), Bottleneck(256, 64), Bottleneck(256, 128, stride=2, downsample=True),
              Bottleneck(512, 128)]
    for b in blocks:
        b.to(DEV).train()
        for m in b.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                torch.nn.init.normal_(m.weight)
                torch.nn.init.normal_(m.bias, std=0.3)
    x0 = _act(2, 256, 8, 11)
    wsum = torch.randn(2, 512, device=DEV)
    cache0 = dict(hnn.TUNER.cache)
    routes = []
    pick0 = hnn.TUNER.pick

    def pick(key, names, run, timed=None):
        if key[0] == "bnconv":  # both routes give the same bits: take the one under test
            routes.append(key)
            return "fused"
        got = pick0(key, names, run, timed)
        if key[0] == "1x1" and not got.startswith("g2_128x"):  # the fused kernel's row tile
            got = hnn.TUNER.cache[key] = [n for n in names if n.startswith("g2_128x")][0]
        return got

    monkeypatch.setattr(hnn.TUNER, "pick", pick)
    # (MIOpen's default algorithms for the 3x3 convolutions are not repeatable run to run)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    try:
        off0 = _run_blocks(blocks, x0, wsum, False, routes, monkeypatch)  # (measures the plain picks)
        off = _run_blocks(blocks, x0, wsum, False, routes, monkeypatch)
        on = _run_blocks(blocks, x0, wsum, True, routes, monkeypatch)
    finally:
        hnn.TUNER.cache.clear()
        hnn.TUNER.cache.update(cache0)
    assert not off[4] and not off[5]
    for k in off[2]:  # the step itself repeats bit for bit
        assert torch.equal(off0[2][k], off[2][k]), k
    # three boundaries took the fused kernel (two plain residuals, one downsample form); the last
    # block's output was still pending at the pool
    assert sorted(k[4] for k in on[4]) == [False, False, True] and on[5]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    for k in off[2]:
        assert torch.equal(on[2][k], off[2][k]), k
    for k in off[3]:
        assert torch.equal(on[3][k], off[3][k]), k
