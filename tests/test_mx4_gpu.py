"""The mx4 kernels (csrc/mx4.hip) against the CPU twin (hipps/ops/reference.py), bit for bit, and
the codec through the async PS: native loop against Python loop, one rank and three, SGD and Adam,
and the GPU job against the same job on CPU."""
import pytest
import torch

from dist_util import run_world
from test_dist_cpu import _data, _mlp
from test_mx4_cpu import crafted, encode, heavy
from test_native_ps_gpu import _run

from hipps import ops
from hipps.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 0xA5
# one grid-wide pass of k_mx4_encode: kMaxGrid (2048) workgroups x 4 waves x 512 elements
PASS = 2048 * 4 * 512
SIZES = [1, 2, 7, 8, 9, 31, 32, 33, 63, 65, 255, 257, 511, 513, 4099, (1 << 20) + 5, PASS + 1037]


def _a16(v):
    return (v + 15) // 16 * 16


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _gpu_encode(x, resid):
    """Encode on the GPU into fields that sit in 0xA5 guard bytes; returns (q, scales, resid) on
    CPU after checking that no guard byte (or guard float around the residual) changed."""
    n = x.numel()
    ns, nq = (n + 31) // 32, (n + 1) // 2
    off_q = 64 + _a16(ns) + 64
    buf = torch.full((off_q + _a16(nq) + 64,), GUARD, dtype=torch.uint8, device=DEV)
    s, q = buf[64:64 + ns], buf[off_q:off_q + nq]
    rbuf = rd = None
    if resid is not None:
        rbuf = torch.full((n + 16,), 12345.0, device=DEV)
        rd = rbuf[8:8 + n]
        rd.copy_(resid)
    ops.mx4_encode(x.to(DEV), rd, q, s)
    torch.cuda.synchronize()
    out = buf.cpu()
    inside = torch.zeros_like(out, dtype=torch.bool)
    inside[64:64 + ns] = True
    inside[off_q:off_q + nq] = True
    assert (out[~inside] == GUARD).all(), "a guard byte around scales / q was written"
    if rbuf is not None:
        assert (rbuf[:8] == 12345.0).all() and (rbuf[8 + n:] == 12345.0).all(), "a guard float around resid was written"
    return out[off_q:off_q + nq].clone(), out[64:64 + ns].clone(), None if rd is None else rd.cpu()


def _check_encode(x, ef, seed=11):
    n = x.numel()
    r0 = heavy(n, seed) * 0.01 if ef == "random" else torch.zeros(n) if ef else None
    want_r = None if r0 is None else r0.clone()
    want_q, want_s = encode(x, want_r)
    q, s, r = _gpu_encode(x, r0)
    assert torch.equal(s, want_s), "scales"
    assert torch.equal(q, want_q), "codes"
    if n & 1:
        assert int(q[-1]) >> 4 == 0
    if ef:
        assert torch.equal(_bits(r), _bits(want_r)), "residual"
    q2, s2, r2 = _gpu_encode(x, r0)  # a second run: the same bits
    assert torch.equal(q, q2) and torch.equal(s, s2) and (not ef or torch.equal(_bits(r), _bits(r2)))


@pytest.mark.parametrize("ef", [False, "random"])
@pytest.mark.parametrize("n", SIZES)
def test_encode_matches_twin(n, ef):
    _check_encode(heavy(n, n % 1000), ef)


@pytest.mark.parametrize("ef", [False, True])
def test_encode_crafted_matches_twin(ef):
    x = crafted()
    _check_encode(x, ef)
    _check_encode(x[:x.numel() - 6], ef)  # the FLT_MAX block as a 31-element tail


# ---- aggregate --------------------------------------------------------------------------------
_MSGS = {}


def _messages(n):
    """16 CPU-encoded messages of n elements (3 at the largest size); message 1 has a NaN block."""
    if n not in _MSGS:
        out = []
        for w in range(16 if n < (1 << 20) else 3):
            x = heavy(n, 50 + w)
            if w == 1:
                x[n // 2] = float("inf")
            out.append(encode(x))
        _MSGS[n] = out
    return _MSGS[n]


def _same(got, want):
    got = got.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(_bits(got.nan_to_num(3.0)), _bits(want.nan_to_num(3.0)))


def _agg(msgs, acc, g, accumulate, acquire=False):
    ops.mx4_aggregate([m[0].to(DEV) for m in msgs], [m[1].to(DEV) for m in msgs], acc, g, accumulate, acquire)


@pytest.mark.parametrize("gscale", [1.0, 0.25, 1 / 3])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("W", [1, 3, 16])
def test_aggregate_matches_twin(W, accumulate, gscale):
    for n in (1, 7, 33, 257, 4099, (1 << 20) + 5):
        msgs = _messages(n)[:W]
        if len(msgs) < W:
            continue
        a0 = heavy(n, 9)
        want = a0.clone()
        ref.mx4_aggregate([m[0] for m in msgs], [m[1] for m in msgs], want, gscale, accumulate)
        for acquire in (False, True):
            acc = a0.to(DEV)
            _agg(msgs, acc, gscale, accumulate, acquire)
            _same(acc, want)


def test_aggregate_crafted_message():
    x = crafted()
    n = x.numel()
    msg = encode(x)
    for accumulate in (False, True):
        want = torch.ones(n)
        ref.mx4_aggregate([msg[0]], [msg[1]], want, 1.0, accumulate)
        acc = torch.ones(n, device=DEV)
        _agg([msg], acc, 1.0, accumulate)
        _same(acc, want)


def test_aggregate_rejects_17_sources():
    msgs = _messages(257)
    acc = torch.zeros(257, device=DEV)
    with pytest.raises(RuntimeError):
        _agg(msgs + msgs[:1], acc, 1.0, True)


def test_aggregate_batch_invariant():
    n = 4099
    msgs = _messages(n)[2:7]
    one = heavy(n, 9).to(DEV)
    each = one.clone()
    _agg(msgs, one, 1 / 3, True)
    for m in msgs:
        _agg([m], each, 1 / 3, True)
    assert torch.equal(_bits(one), _bits(each))


# ---- through the engines ----------------------------------------------------------------------
def _cpu_job(rank, world, steps):
    """test_native_ps_gpu._run's job (SGD) on CPU."""
    import hipps

    m = _mlp()
    opt = hipps.SGD(m.named_parameters(), mode="ps_async", code="mx4", bucket_mb=0.0005, max_delay=0, accumulate=world,
                    ps_granularity="bucket", lr=0.05, momentum=0.9, weight_decay=1e-4)
    for s in range(steps):
        if s == steps // 2:
            for g in opt.param_groups:
                g["lr"] *= 0.5
        x, y = _data(0, s % 4)
        opt.zero_grad()
        torch.nn.functional.cross_entropy(m(x), y).backward()
        opt.step()
    opt.close()
    return [p.detach().clone() for p in m.parameters()]


def test_native_loop_single_rank_bitwise():
    a = run_world(_run, 1, True, 6, "mx4")[0]
    b = run_world(_run, 1, False, 6, "mx4")[0]
    assert a["stats"]["native_loop"] == 1 and b["stats"]["native_loop"] == 0
    assert a["stats"]["accumulated"] == b["stats"]["accumulated"] == 6
    assert a["stats"]["bucket_updates"] == b["stats"]["bucket_updates"] == 6 * a["nb"] and a["nb"] >= 3
    for x, y in zip(a["params"], b["params"]):
        torch.testing.assert_close(x, y, rtol=0, atol=0)


def test_gpu_job_matches_cpu_job():
    a = run_world(_run, 1, True, 6, "mx4")[0]
    c = run_world(_cpu_job, 1, 6)[0]
    print("GPU vs CPU job, max |diff| per tensor:", [(x - z).abs().max().item() for x, z in zip(a["params"], c)])
    for x, z in zip(a["params"], c):
        torch.testing.assert_close(x, z, rtol=1e-3, atol=5e-5)


def test_native_loop_three_ranks_bitwise():
    a = run_world(_run, 3, True, 6, "mx4", timeout=300)
    b = run_world(_run, 3, False, 6, "mx4", timeout=300)
    assert a[0]["stats"]["native_loop"] == 1
    assert a[0]["stats"]["accumulated"] == 18 and a[0]["stats"]["version"] == 6
    for r in range(3):
        for x, y in zip(a[r]["params"], b[r]["params"]):
            torch.testing.assert_close(x, y, rtol=0, atol=0)


def test_native_loop_adam_bitwise():
    a = run_world(_run, 1, True, 6, "mx4", "adam")[0]
    b = run_world(_run, 1, False, 6, "mx4", "adam")[0]
    assert a["stats"]["native_loop"] == 1 and b["stats"]["native_loop"] == 0
    for x, y in zip(a["params"], b["params"]):
        torch.testing.assert_close(x, y, rtol=0, atol=0)
    for k in b["state"]:
        torch.testing.assert_close(a["state"][k], b["state"][k], rtol=0, atol=0)
