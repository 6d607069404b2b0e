"""bn3's backward apply pass fused into conv3's input-gradient GEMM (hipps/csrc/bnconv.hip
bnconv_backward) against the two kernels it replaces: the BN backward finalize + apply (norm.hip)
and the 1x1 GEMM with bn2's backward reduction in its epilogue (gemm2.hip, 128-row tile).
Everything must be bit-identical: bn3's input gradient, conv3's input gradient, bn2's reduction
partials and bn3's dgamma / dbeta.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
MASK_BITS = 3
# (imgs, h, K, N): M = 98 < one tile; M = 243: a tail tile, the bits end in a partial wave; several
# row tiles; two column tiles (dx3 written once, A rebuilt)
SHAPES = [(2, 7, 256, 64), (3, 9, 512, 128), (2, 14, 256, 64), (2, 7, 1024, 256)]
CASES = [(s, bn) for s in SHAPES for bn in (64, 128) if s[3] % bn == 0]


def C():
    from hipps.ops._native import native

    return native()


def _act(n, c, h, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, c, h, h, generator=g).to(DEV).to(torch.bfloat16).contiguous(memory_format=CL)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _stats(x):
    xf = _rows(x).float()
    mean = xf.mean(0)
    invstd = (xf.var(0, unbiased=False) + 1e-5).rsqrt()
    return mean.contiguous(), invstd.contiguous()


def _bn_weight(c, seed):
    """BN weights of both signs; channels 0..7: weight = 0."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = torch.randn(c, generator=g)
    w[:8] = 0
    return w.to(DEV)


def _unpack(bits, M, K):
    b = (bits.view(-1, 1) >> torch.arange(8, device=bits.device, dtype=torch.uint8)) & 1
    return b.view(M, K).float()


@pytest.mark.parametrize("shape,bn", CASES)
def test_bnbwd_bitwise_against_apply_then_gemm(shape, bn):
    n, h, K, N = shape
    M = n * h * h
    f32 = dict(dtype=torch.float32, device=DEV)
    dy, x3 = _act(n, K, h, 1), _act(n, K, h, 2)
    g = torch.Generator(device="cpu").manual_seed(3)
    bits = torch.randint(0, 256, (M * K // 8,), generator=g, dtype=torch.uint8).to(DEV)
    b2 = bits.view(M, K // 8)
    b2[0].zero_()       # rows whose ReLU bits are all 0 ...
    b2[M - 1].zero_()
    b2[5].fill_(0xFF)   # ... and all 1
    b2[M - 2].fill_(0xFF)
    w3 = _bn_weight(K, 4)
    mean3, invstd3 = _stats(x3)
    sc3, sh3 = (w3 * invstd3).contiguous(), torch.zeros(K, **f32)  # (unused by the MASK_BITS kernels)
    # bn3's backward partials, as its consumer's epilogue would have left them (one row block)
    dz = _rows(dy).float() * _unpack(bits, M, K)
    xh = (_rows(x3).float() - mean3) * invstd3
    part3 = torch.stack([dz.sum(0), (dz * xh).sum(0)]).unsqueeze(2).contiguous()
    # bn2: input x2, weights of both signs, biases around zero (about half of the mask clamps)
    x2 = _act(n, N, h, 5)
    mean2, invstd2 = _stats(x2)
    w2 = _bn_weight(N, 6)
    sc2 = (w2 * invstd2).contiguous()
    b2n = torch.randn(N, generator=torch.Generator(device="cpu").manual_seed(7)).to(DEV) * 0.3
    sh2 = (b2n - mean2 * sc2).contiguous()
    on = (_rows(x2).float() * sc2 + sh2 > 0).float().mean().item()
    assert 0.25 < on < 0.75, on
    wt = (torch.randn(N, K, device=DEV) / K ** 0.5).to(torch.bfloat16)

    # the two kernels
    dx_ref = torch.full_like(x3, 7.0)
    dgw_ref, dgb_ref = torch.full((K,), 7.0, **f32), torch.full((K,), 7.0, **f32)
    C().bn_backward_partials(part3, 1, dy, x3, MASK_BITS, w3, mean3, invstd3, sc3, sh3, dx_ref, None, dgw_ref, dgb_ref,
                             K, bits)
    dbn_ref = torch.full_like(x2, 7.0)
    p_ref = torch.full((2, N, C().gemm2_mtiles(M, N, K, 128)), 7.0, **f32)
    C().gemm2_conv(dx_ref, wt, dbn_ref, p_ref, None, None, h, h, 1, 1, 1, 0, 128, bn, x2, None, mean2, invstd2, sc2,
                   sh2)

    # finalize only, then the fused kernel
    dgw, dgb = torch.full((K,), 7.0, **f32), torch.full((K,), 7.0, **f32)
    coef = torch.full((3, K), 7.0, **f32)
    C().bn_finalize_bwd_partials(part3, 1, M, w3, mean3, invstd3, dgw, dgb, coef)
    dx = torch.full_like(x3, 7.0)
    dbn = torch.full_like(x2, 7.0)
    part = torch.full((2, N, C().bnconv_mtiles(M)), 7.0, **f32)
    C().bnconv_backward(dy, x3, bits, coef, wt, dx, dbn, part, x2, mean2, invstd2, sc2, sh2, bn)
    torch.cuda.synchronize()

    assert torch.equal(dgw, dgw_ref) and torch.equal(dgb, dgb_ref)
    assert torch.equal(dx, dx_ref)
    assert torch.equal(dbn, dbn_ref)
    assert part.shape == p_ref.shape and torch.equal(part, p_ref)
    # the first core's kernel at this column tile reduces in the same order (its default tile)
    if bn == (128 if N % 128 == 0 else 64):
        y1 = torch.full_like(x2, 7.0)
        p1 = torch.full((2, N, C().conv1x1_mtiles(M)), 7.0, **f32)
        C().conv1x1_forward(dx_ref, wt, y1, p1, h, h, 1, None, None, x2, None, mean2, invstd2, sc2, sh2)
        assert torch.equal(dbn, y1) and torch.equal(part, p1)
    ref = _rows(dx).float() @ wt.float().t()
    torch.testing.assert_close(_rows(dbn).float(), ref, rtol=2e-2, atol=2e-2)
    # the apply pass alone (what a gradient that came round the link runs)
    dx2 = torch.full_like(x3, 7.0)
    C().bn_backward_apply(dy, x3, MASK_BITS, sc3, sh3, coef, dx2, K, bits)
    assert torch.equal(dx2, dx_ref)


def _count(monkeypatch, name, calls):
    fn = getattr(C(), name)

    def wrapped(*a, **k):
        calls.append(name)
        return fn(*a, **k)

    monkeypatch.setattr(C(), name, wrapped)


def _run_blocks(blocks0, x0, wsum, on, monkeypatch):
    import hipps.ops.nn as hnn

    monkeypatch.setattr(hnn, "_FUSED_BNBWD", on)
    blocks = copy.deepcopy(blocks0)
    x = x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = x
        for b in blocks:
            y = b(y)
        out = hnn.global_avg_pool(y)
    (out.float() * wsum).sum().backward()
    torch.cuda.synchronize()
    grads = {f"{i}.{n}": p.grad.clone() for i, b in enumerate(blocks) for n, p in b.named_parameters()}
    return out.detach().clone(), x.grad.clone(), grads


def test_blocks_fused_backward_bitwise(monkeypatch):
    """Two identity blocks of width 64 at 2 x 256 x 8 x 8, wired as in layer 1 (bn2 inside conv3's
    prologue; the second block's conv1 reduces the first one's bn3 backward statistics, so the
    first block's bn3 hands its apply pass over): the route off against on with the fused kernel
    forced, same tuner picks: the input gradient and every parameter gradient are bit-identical,
    and each case repeats bit for bit."""
    import hipps.ops.nn as hnn
    from hipps.models.resnet import Bottleneck

    torch.manual_seed(0)
    blocks = [Bottleneck(256, 64), Bottleneck(256, 64)]
    for b in blocks:
        b.to(DEV).to(memory_format=CL).train()  # (the 3x3 GEMM core reads channels-last weights)
        for m in b.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                torch.nn.init.normal_(m.weight)
                torch.nn.init.normal_(m.bias, std=0.3)
    x0 = _act(2, 256, 8, 11)
    wsum = torch.randn(2, 256, device=DEV)
    cache0 = dict(hnn.TUNER.cache)
    calls = []
    _count(monkeypatch, "bnconv_backward", calls)
    # (MIOpen's default algorithms for the 3x3 convolutions are not repeatable run to run)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    try:
        # conv2 on the GEMM core (MIOpen's forward leaves no bn2 statistics for conv3's prologue route)
        hnn.TUNER.cache[("kxk", 2, 64, 8, 8, 64, 3, 1, 1, (True, None))] = "g2_128x64"
        hnn.TUNER.cache[("bnpro", 2, 64, 8, 8, 256)] = "pro"
        # conv3's input-gradient pick: a 128-row tile, the same in every run
        hnn.TUNER.cache[("1x1", 128, 256, 64, 1, 8, 8, (True, False, False, False, True, False))] = "g2_128x64"
        hnn.TUNER.cache[("bnbwd", 128, 256, 64)] = "fused"
        off0 = _run_blocks(blocks, x0, wsum, False, monkeypatch)  # (measures the other picks)
        off = _run_blocks(blocks, x0, wsum, False, monkeypatch)
        assert not calls
        on0 = _run_blocks(blocks, x0, wsum, True, monkeypatch)
        on = _run_blocks(blocks, x0, wsum, True, monkeypatch)
    finally:
        hnn.TUNER.cache.clear()
        hnn.TUNER.cache.update(cache0)
    assert len(calls) == 2  # the first block's conv3, once per run
    for a, b in ((off0, off), (on0, on), (off, on)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for k in a[2]:
            assert torch.equal(a[2][k], b[2][k]), k


def _run_link(mods, x2_0, idt, wsum, part3, on, hook, monkeypatch):
    import hipps.ops.nn as hnn

    monkeypatch.setattr(hnn, "_FUSED_BNBWD", on)
    bn2, conv3, bn3 = copy.deepcopy(mods)
    x2 = x2_0.clone().requires_grad_(True)
    xf = x2_0.float()
    p2 = torch.stack([xf.sum((0, 2, 3)), (xf * xf).sum((0, 2, 3))]).unsqueeze(2).contiguous()
    tap = hnn.ResidualTap()
    tap.armed = True  # (the residual's gradient goes to a tap, as in an identity block)
    link = hnn.BNBwdLink()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        x3, p3 = hnn.bn_relu_conv(bn2, conv3, x2, p2, link)
        if hook:
            x3.register_hook(lambda g: g.clone())
        out = bn3(x3, idt, stats=p3, res_tap=tap, bwd_link=link)
    out._hipps_bngrad.part = part3  # bn3's backward reduction, as a consuming conv1 leaves it
    (out.float() * wsum).sum().backward()
    torch.cuda.synchronize()
    grads = {f"{i}.{n}": p.grad.clone() for i, m in enumerate((bn2, conv3, bn3)) for n, p in m.named_parameters()}
    return x2.grad.clone(), grads, link


def test_gradient_round_the_link_materializes(monkeypatch):
    """A hook on x3 that returns a clone takes bn3's gradient round the link: conv3's backward gets
    another buffer, writes bn3's own with the plain apply kernel and uses that; same bits as the
    route off, and as the fused kernel when nothing is in the way."""
    import hipps.ops.nn as hnn
    from hipps.models.resnet import _bn, _conv

    torch.manual_seed(1)
    mods = (_bn(64, relu=True), _conv(64, 256, 1), _bn(256, relu=True))
    for m in mods:
        m.to(DEV).train()
        if isinstance(m, torch.nn.BatchNorm2d):
            torch.nn.init.normal_(m.weight)
            torch.nn.init.normal_(m.bias, std=0.3)
    x2, idt = _act(2, 64, 8, 21), _act(2, 256, 8, 22)
    wsum = torch.randn(2, 256, 8, 8, device=DEV).contiguous(memory_format=CL)
    part3 = torch.randn(2, 256, 1, device=DEV)
    cache0 = dict(hnn.TUNER.cache)
    calls = []
    _count(monkeypatch, "bnconv_backward", calls)
    _count(monkeypatch, "bn_backward_apply", calls)
    try:
        hnn.TUNER.cache[("1x1", 128, 256, 64, 1, 8, 8, (True, False, False, False, True, False))] = "g2_128x64"
        hnn.TUNER.cache[("bnbwd", 128, 256, 64)] = "fused"
        off = _run_link(mods, x2, idt, wsum, part3, False, False, monkeypatch)
        assert not calls and not off[2].armed
        hooked = _run_link(mods, x2, idt, wsum, part3, True, True, monkeypatch)
        assert calls == ["bn_backward_apply"] and hooked[2].armed and hooked[2].pend is None
        del calls[:]
        fused = _run_link(mods, x2, idt, wsum, part3, True, False, monkeypatch)
        assert calls == ["bnconv_backward"]
    finally:
        hnn.TUNER.cache.clear()
        hnn.TUNER.cache.update(cache0)
    for got in (hooked, fused):
        assert torch.equal(got[0], off[0])
        for k in off[1]:
            assert torch.equal(got[1][k], off[1][k]), k
