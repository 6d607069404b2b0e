"""Time hipps flash attention (csrc/attn.hip) against PyTorch SDPA (aotriton on ROCm) on the
transformer configs' attention shapes, forward and backward, same process, interleaved.

    python tools/diag/attn_time.py [--json out.json]

With ``--docs N`` (N equal documents per row) and / or ``--window W`` it times the row-range
(BND) kernels with that mask against the unbounded kernels instead, and prints next to each time
the (wave, 64-row tile) pairs the mask leaves the kernels to visit -- forward / dQ: per 32 query
rows the key tiles that meet the union of their key ranges; dK/dV: per 32 keys the query tiles
likewise -- so the time ratio can be held against the tile ratio.  ``--docs 1`` is one document:
every tile of the unbounded kernels, plus the loads of the bounds.

    python tools/diag/attn_time.py --docs 8 [--window 512] [--json out.json]

With ``--dropout P`` it times the DROP kernels (attention dropout at probability P, the mask
generated in the kernels) against the plain ones, per shape: plain, dropout, plain again.

    python tools/diag/attn_time.py --dropout 0.1 --iters 200 [--json out.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import hipps.ops.nn as hnn  # noqa: E402

SHAPES = {
    # name: B, S, Hq, Hkv, D, causal
    "bert-base b32": (32, 512, 12, 12, 64, False),
    "bert-base b256": (256, 512, 12, 12, 64, False),
    "llama3-1b b4": (4, 2048, 32, 8, 64, True),
    "llama3-8b b1": (1, 2048, 32, 8, 128, True),
}


ITERS = 10


def _time(fn, n=None):
    n = n or ITERS
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[n // 2]


def _tiles(lo, hi):
    """(wave, tile) pairs over a [B or 1, S] pair of range arrays: per run of 32 rows the 64-row
    tiles that meet [lo[first], hi[last]) (what the kernels' wave-uniform skip leaves)."""
    S = lo.shape[1]
    first = torch.arange(0, S, 32)
    last = (first + 31).clamp(max=S - 1)
    a, b = lo[:, first].long(), hi[:, last].long()
    return int(((b + 63) // 64 - a // 64).clamp(min=0)[b > a].sum()) / lo.shape[0]


def _mask_tiles(bd):
    """Visited tiles per (batch row, head) of the forward (= dQ) and the dK/dV kernels."""
    bd = bd.to("cpu")
    return _tiles(bd.klo, bd.khi), _tiles(bd.qlo, bd.qhi)


def _masked(a):
    """--docs / --window: the bounded kernels against the unbounded ones, with tile counts."""
    out = {}
    for name, (B, S, Hq, Hkv, D, causal) in SHAPES.items():
        if a.only and a.only not in name:
            continue
        torch.manual_seed(0)
        q = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        k = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        v = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        g = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16)
        doc_ids = None
        if a.docs:
            doc_ids = (torch.arange(S, device="cuda") * a.docs // S)[None].expand(B, S).contiguous()
        bd = hnn.attention_bounds(S, doc_ids=doc_ids, window=a.window or None, causal=causal, device="cuda")
        full = hnn.attention_bounds(S, window=S, causal=causal)  # the ranges of the unbounded kernels
        row = {}
        for tag, b in (("unbounded", None), ("masked", bd)):
            f = lambda b=b: hnn.attention(q, k, v, causal=causal, bounds=b)  # noqa: E731
            with torch.no_grad():
                tf = _time(f)
            o = f()
            tb = _time(lambda: torch.autograd.grad(o, (q, k, v), g, retain_graph=True))
            tq, tk = _mask_tiles(full if b is None else b)
            row[tag] = {"fwd_ms": round(tf, 4), "bwd_ms": round(tb, 4), "fwd_tiles": tq, "bwd_tiles": tq + tk}
        m, u = row["masked"], row["unbounded"]
        row["ratio"] = {x: round(m[x] / u[x], 4) for x in ("fwd_ms", "fwd_tiles", "bwd_ms", "bwd_tiles")}
        out[name] = row
        r = row["ratio"]
        print(f"{name:16s} fwd {u['fwd_ms']:.3f} -> {m['fwd_ms']:.3f} ms (x{r['fwd_ms']:.3f}; tiles "
              f"{u['fwd_tiles']:.0f} -> {m['fwd_tiles']:.0f}, x{r['fwd_tiles']:.3f}) | bwd {u['bwd_ms']:.3f} -> "
              f"{m['bwd_ms']:.3f} ms (x{r['bwd_ms']:.3f}; tiles {u['bwd_tiles']:.0f} -> {m['bwd_tiles']:.0f}, "
              f"x{r['bwd_tiles']:.3f})", flush=True)
        del q, k, v, g
        torch.cuda.empty_cache()
    return out


def _dropout(a):
    """--dropout P: the DROP kernels (in-kernel mask at probability P) against the plain ones, each
    shape's four figures from one process, interleaved."""
    out = {}
    for name, (B, S, Hq, Hkv, D, causal) in SHAPES.items():
        if a.only and a.only not in name:
            continue
        torch.manual_seed(0)
        q = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        k = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        v = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        g = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16)
        row = {}
        for tag, p in (("plain", 0.0), ("dropout", a.dropout), ("plain_again", 0.0)):
            f = lambda p=p: hnn.attention(q, k, v, causal=causal, dropout_p=p, dropout_seed=1234)  # noqa: E731
            with torch.no_grad():
                tf = _time(f)
            o = f()
            tb = _time(lambda: torch.autograd.grad(o, (q, k, v), g, retain_graph=True))
            row[tag] = {"fwd_ms": round(tf, 4), "bwd_ms": round(tb, 4)}
        d, u = row["dropout"], row["plain"]
        row["ratio"] = {x: round(d[x] / u[x], 4) for x in ("fwd_ms", "bwd_ms")}
        out[name] = row
        print(f"{name:16s} fwd {u['fwd_ms']:.3f} -> {d['fwd_ms']:.3f} ms (x{row['ratio']['fwd_ms']:.3f}) | bwd "
              f"{u['bwd_ms']:.3f} -> {d['bwd_ms']:.3f} ms (x{row['ratio']['bwd_ms']:.3f}) | plain again fwd "
              f"{row['plain_again']['fwd_ms']:.3f} bwd {row['plain_again']['bwd_ms']:.3f}", flush=True)
        del q, k, v, g
        torch.cuda.empty_cache()
    return out


def main():
    global ITERS
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--docs", type=int, default=0, help="N equal documents per row (row-range kernels)")
    ap.add_argument("--window", type=int, default=0, help="sliding window of W keys (row-range kernels)")
    ap.add_argument("--iters", type=int, default=ITERS, help="timed calls per figure (the median is kept)")
    ap.add_argument("--dropout", type=float, default=0.0, help="attention dropout P: DROP kernels vs the plain ones")
    a = ap.parse_args()
    ITERS = a.iters
    if a.dropout:
        out = _dropout(a)
        if a.json:
            os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
            with open(a.json, "w") as f:
                json.dump({"dropout_p": a.dropout, "iters": ITERS, "shapes": out}, f, indent=1)
        return
    if a.docs or a.window:
        out = _masked(a)
        if a.json:
            os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
            with open(a.json, "w") as f:
                json.dump({"docs": a.docs, "window": a.window, "shapes": out}, f, indent=1)
        return
    out = {}
    for name, (B, S, Hq, Hkv, D, causal) in SHAPES.items():
        if a.only and a.only not in name:
            continue
        torch.manual_seed(0)
        q = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        k = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        v = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        g = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16)
        flops_f = 4.0 * B * Hq * S * S * D * (0.5 if causal else 1.0)
        flops_b = 2.5 * flops_f

        def ours_f():
            return hnn.attention(q, k, v, causal=causal)

        def sdpa_f():
            return F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                                  is_causal=causal, enable_gqa=Hq != Hkv).transpose(1, 2)

        row = {}
        for tag, f in (("hipps", ours_f), ("sdpa", sdpa_f)):
            with torch.no_grad():
                tf = _time(f)
            o = f()
            tb = _time(lambda: torch.autograd.grad(o, (q, k, v), g, retain_graph=True))
            row[tag] = {"fwd_ms": round(tf, 4), "bwd_ms": round(tb, 4),
                        "fwd_tflops": round(flops_f / tf / 1e9, 1), "bwd_tflops": round(flops_b / tb / 1e9, 1)}
        out[name] = row
        print(f"{name:16s} fwd hipps {row['hipps']['fwd_ms']:.3f} ms ({row['hipps']['fwd_tflops']} TF) "
              f"sdpa {row['sdpa']['fwd_ms']:.3f} ({row['sdpa']['fwd_tflops']}) | bwd hipps "
              f"{row['hipps']['bwd_ms']:.3f} ({row['hipps']['bwd_tflops']}) sdpa {row['sdpa']['bwd_ms']:.3f} "
              f"({row['sdpa']['bwd_tflops']})", flush=True)
        del q, k, v, g
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
