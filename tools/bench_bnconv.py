"""Microbenchmark of the ResNet-50 block boundary (bs 256, channels-last bf16): bn3's apply pass
(+ residual + ReLU + bits) and the next block's conv1, as two kernels and as one.

  apply   norm.hip k_bn_apply_fwd: reads x3 and res, writes out + bits           (bytes: 3 M K 2 + M K / 8)
  conv1   the tuned 1x1 GEMM with the statistics epilogue: reads out, writes y1   (bytes: M K 2 + M N 2)
  fused   bnconv.hip: reads x3 and res, writes out + bits + y1                    (bytes: apply + M N 2)

Every call starts cold (a 512 MB fill flushes the caches); the median of ``--iters`` calls.

    python tools/bench_bnconv.py [--out file.json] [--dual]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipps.ops import nn as hnn  # noqa: E402
from hipps.ops._native import native  # noqa: E402

SHAPES = [(56, 256, 64), (56, 256, 128), (28, 512, 128), (28, 512, 256), (14, 1024, 256), (14, 1024, 512),
          (7, 2048, 512)]  # (H, K, N): the 7 distinct producer -> conv1 pairs


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
    ap.add_argument("--dual", action="store_true", help="the downsample form (the residual has its own scale / shift)")
    a = ap.parse_args()
    C = native()
    cl = torch.channels_last
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    rows = []
    for h, K, N in SHAPES:
        M = 256 * h * h
        x3 = torch.randn(256, K, h, h, device="cuda").to(torch.bfloat16).contiguous(memory_format=cl)
        res = torch.randn_like(x3)
        out = torch.empty_like(x3)
        bits = torch.empty(M * K // 8, dtype=torch.uint8, device="cuda")
        w = (torch.randn(N, K, device="cuda") / K ** 0.5).to(torch.bfloat16)
        y = torch.empty(256, N, h, h, dtype=torch.bfloat16, device="cuda").contiguous(memory_format=cl)
        sc, sh = torch.randn(K, device="cuda"), torch.randn(K, device="cuda") * 0.3
        rsc, rsh = (torch.randn(K, device="cuda"), torch.randn(K, device="cuda") * 0.3) if a.dual else (None, None)
        part = torch.empty(2, N, C.bnconv_mtiles(M), device="cuda")
        hnn._conv1x1_gemm(out, w, y, h, h, 1, True)  # (measures this shape's pick if it is not recorded)
        pick = hnn.TUNER.cache.get(("1x1", M, K, N, 1, h, h, (True, False, False, False, False, False)), "g1")
        t_a = cold_us(lambda: C.bn_apply_bits(x3, res, out, bits, sc, sh, rsc, rsh, K), flush, a.iters)
        t_c = cold_us(lambda: hnn._conv1x1_gemm(out, w, y, h, h, 1, True), flush, a.iters)
        t_f = cold_us(lambda: C.bnconv_forward(x3, res, sc, sh, rsc, rsh, w, out, bits, y, part), flush, a.iters)
        b_a = 3 * M * K * 2 + M * K // 8
        b_c = M * K * 2 + M * N * 2
        b_f = b_a + M * N * 2
        rows.append({"M": M, "K": K, "N": N, "conv1_pick": pick,
                     "apply_us": round(t_a, 1), "apply_TBps": round(b_a / t_a / 1e6, 2),
                     "conv1_us": round(t_c, 1), "conv1_TBps": round(b_c / t_c / 1e6, 2),
                     "fused_us": round(t_f, 1), "fused_TBps": round(b_f / t_f / 1e6, 2),
                     "fused_minus_separate_us": round(t_f - t_a - t_c, 1)})
        print(json.dumps(rows[-1]), flush=True)
        del x3, res, out, y
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"dual": a.dual, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
