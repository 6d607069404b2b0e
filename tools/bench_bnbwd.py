"""Microbenchmark of the ResNet-50 identity block's bn3 -> conv3 backward (bs 256, channels-last
bf16): bn3's backward apply pass and conv3's input-gradient GEMM, as two kernels and as one.

  apply   norm.hip k_bn_apply_bwd<MASK_BITS>: reads dy, x3 and the bits, writes dx3   (bytes: 3 M K 2 + M K / 8)
  dgrad   the tuned 1x1 GEMM with bn2's backward reduction in its epilogue: reads dx3
          and x2, writes dbn                                                          (bytes: M K 2 + 2 M N 2)
  fused   bnconv.hip bnconv_backward: reads dy, x3, the bits and x2, writes dx3 + dbn  (bytes: apply + 2 M N 2)

bn3's finalize precedes both routes and is not timed.  Every call starts cold (a 512 MB fill
flushes the caches); the median of ``--iters`` calls.

    python tools/bench_bnbwd.py [--out file.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipps.ops import nn as hnn  # noqa: E402
from hipps.ops._native import native  # noqa: E402

SHAPES = [(56, 256, 64), (28, 512, 128), (14, 1024, 256), (7, 2048, 512)]  # (H, K = 4w, N = w): layers 1-4


def cold_us(fn, flush, iters):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        flush.zero_()
        s, e = torch.cuda.Event(True), torch.cuda.Event(True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=15)
    a = ap.parse_args()
    C = native()
    cl = torch.channels_last
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    rows = []
    for h, K, N in SHAPES:
        M = 256 * h * h
        dy = torch.randn(256, K, h, h, device="cuda").to(torch.bfloat16).contiguous(memory_format=cl)
        x3 = torch.randn_like(dy)
        dx3 = torch.empty_like(dy)
        bits = torch.randint(0, 256, (M * K // 8,), dtype=torch.uint8, device="cuda")
        coef = torch.randn(3, K, device="cuda")
        sc3 = torch.randn(K, device="cuda")
        wt = (torch.randn(N, K, device="cuda") / K ** 0.5).to(torch.bfloat16)
        x2 = torch.randn(256, N, h, h, device="cuda").to(torch.bfloat16).contiguous(memory_format=cl)
        dbn = torch.empty_like(x2)
        mean, invstd = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
        scale, shift = torch.randn(N, device="cuda"), torch.randn(N, device="cuda") * 0.3
        bg = hnn.BNGradTap(x2, None, mean, invstd, scale, shift)
        part = torch.empty(2, N, C.bnconv_mtiles(M), device="cuda")
        hnn._conv1x1_gemm(dx3, wt, dbn, h, h, 1, True, None, None, bg)  # (measures the pick if it is not recorded)
        pick = hnn.TUNER.cache.get(("1x1", M, K, N, 1, h, h, (True, False, False, False, True, False)), "g1")
        bn = hnn._bnbwd_tile(pick, N)
        t_a = cold_us(lambda: C.bn_backward_apply(dy, x3, hnn.MASK_BITS, sc3, sc3, coef, dx3, K, bits), flush, a.iters)
        t_g = cold_us(lambda: hnn._conv1x1_gemm(dx3, wt, dbn, h, h, 1, True, None, None, bg), flush, a.iters)
        t_f = cold_us(lambda: C.bnconv_backward(dy, x3, bits, coef, wt, dx3, dbn, part, x2, mean, invstd, scale,
                                                shift, bn), flush, a.iters)
        b_a = 3 * M * K * 2 + M * K // 8
        b_g = M * K * 2 + 2 * M * N * 2
        b_f = b_a + 2 * M * N * 2
        rows.append({"M": M, "K": K, "N": N, "dgrad_pick": pick, "fused_bn": bn or (128 if N % 128 == 0 else 64),
                     "same_bits_as_pick": bool(bn),
                     "apply_us": round(t_a, 1), "apply_TBps": round(b_a / t_a / 1e6, 2),
                     "dgrad_us": round(t_g, 1), "dgrad_TBps": round(b_g / t_g / 1e6, 2),
                     "fused_us": round(t_f, 1), "fused_TBps": round(b_f / t_f / 1e6, 2),
                     "fused_minus_separate_us": round(t_f - t_a - t_g, 1)})
        print(json.dumps(rows[-1]), flush=True)
        del dy, x3, dx3, x2, dbn
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
