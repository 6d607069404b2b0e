// hipps — MXFP4 block-scaled gradient codec (encode on the worker, fused decode-accumulate on PS).
//
// OCP MXFP4: 4-bit e2m1 elements {0, .5, 1, 1.5, 2, 3, 4, 6} with a sign bit, one E8M0
// power-of-two scale byte per 32-element block.  Wire payload per message:
//   scales : uint8[ceil(n / 32)]      (e + 127; 0 = all-zero block, 255 = NaN block)
//   q      : uint8[ceil(n / 2)]       (element 2j in the low nibble of byte j)
// = 0.53125 B/elem.  hipps/ops/reference.py (mx4_encode / mx4_dequant / mx4_aggregate) is the
// normative definition; both kernels match it bit for bit.
//
// A lane owns 8 consecutive elements (two 16-byte loads, one dword of codes), so a DPP quad is
// exactly one 32-element block and a wave covers 16 blocks (512 elements) per iteration.  The block
// maximum is two quad-permute DPP steps on the |v| BIT PATTERNS: as unsigned integers they order
// like the magnitudes, and Inf / NaN sort above every finite value, so one integer maximum gives
// the scale exponent, the below-2^-100 test and the non-finite test.  No LDS, no log2.
#include "common.h"

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

// The format is defined with separate roundings, and the aggregate is batch-invariant only with
// them.  hipcc contracts a * b + c into an fma by default, and __fmul_rn / __fadd_rn do not stop it
// (they are plain operators compiled under the header's contraction mode), so this file turns
// contraction off and does its arithmetic through the helpers below.
#pragma clang fp contract(off)

namespace hipps {

__device__ __forceinline__ float mx_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float mx_add(float a, float b) { return a + b; }
__device__ __forceinline__ float mx_sub(float a, float b) { return a - b; }

constexpr int kMxBlock = 32;
constexpr int kMxLane = 8;             // elements per lane
constexpr int kMxWave = 64 * kMxLane;  // elements per wave per iteration (16 blocks)

template <int kCtrl> __device__ __forceinline__ uint32_t mx_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, false);
}

// Element conversions are the hardware's: v_cvt_scalef32_pk_fp4_f32 (f32 / scale -> e2m1, round to
// nearest even, the sign kept on zero codes) and v_cvt_scalef32_pk_f32_fp4 (e2m1 * scale, a NaN
// scale giving NaN for every code).  On the MI355X both agree with the twin's compare ladder and
// GRID[code] * 2^e on every tie, both neighbours of every tie, signed zeros and scales from 2^-102
// to 2^125 (tests/test_mx4_gpu.py).  Each call converts two elements; the byte index is an immediate.
__device__ __forceinline__ uint32_t mx4_codes(const float (&v)[kMxLane], float sc) {
  uint32_t word = 0;
  word = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(word, v[0], v[1], sc, 0);
  word = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(word, v[2], v[3], sc, 1);
  word = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(word, v[4], v[5], sc, 2);
  word = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(word, v[6], v[7], sc, 3);
  return word;
}

__device__ __forceinline__ void mx4_decode(uint32_t word, float sc, float (&d)[kMxLane]) {
  const auto d0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, sc, 0);
  const auto d1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, sc, 1);
  const auto d2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, sc, 2);
  const auto d3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, sc, 3);
  d[0] = d0[0]; d[1] = d0[1]; d[2] = d1[0]; d[3] = d1[1];
  d[4] = d2[0]; d[5] = d2[1]; d[6] = d3[0]; d[7] = d3[1];
}

__global__ __launch_bounds__(kBlock) void k_mx4_encode(const float* __restrict__ x, float* __restrict__ resid,
                                                       uint8_t* __restrict__ q, uint8_t* __restrict__ scales,
                                                       int64_t n) {
  const int lane = threadIdx.x & 63;
  const int64_t nunits = (n + kMxWave - 1) / kMxWave, nblocks = (n + kMxBlock - 1) / kMxBlock;
  const int64_t wstride = (int64_t)gridDim.x * (blockDim.x >> 6);
  auto load = [&](const float* src, int64_t u, float (&v)[kMxLane]) {
    const int64_t i = u * kMxWave + lane * kMxLane;
    if (i + kMxLane <= n) {
      const float4 a = *reinterpret_cast<const float4*>(src + i), b = *reinterpret_cast<const float4*>(src + i + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
      v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {  // the bucket's last lanes: zeros past n count for the block maximum only
#pragma unroll
      for (int j = 0; j < kMxLane; ++j) v[j] = i + j < n ? src[i + j] : 0.f;
    }
  };
  int64_t u = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // wave-uniform
  float xv[kMxLane], rv[kMxLane];
  if (u < nunits) {
    load(x, u, xv);
    if (resid) load(resid, u, rv);
  }
  while (u < nunits) {
    const int64_t un = u + wstride;
    float v[kMxLane];
#pragma unroll
    for (int j = 0; j < kMxLane; ++j) v[j] = resid ? mx_add(xv[j], rv[j]) : xv[j];
    if (un < nunits) {  // the next iteration's operands in flight during this one's work
      load(x, un, xv);
      if (resid) load(resid, un, rv);
    }
    uint32_t am = 0;
#pragma unroll
    for (int j = 0; j < kMxLane; ++j) am = max(am, __float_as_uint(v[j]) & 0x7fffffffu);
    // quad xor 1, quad xor 2: every lane of the wave is active here (wave-uniform loop)
    am = max(am, mx_dpp<0xB1>(am));
    am = max(am, mx_dpp<0x4E>(am));
    const bool nonfinite = am >= 0x7f800000u, tiny = am < (27u << 23), normal = !(nonfinite || tiny);
    // a = m * 2^k: e = k - 2 (m <= 1.5) or k - 1, capped at 125; the byte is e + 127
    const uint32_t sb = normal ? min((am >> 23) - 2u + (uint32_t)((am & 0x7fffffu) > 0x400000u), 252u) : 127u;
    const float sc = __uint_as_float(sb << 23);
    const uint32_t word = normal ? mx4_codes(v, sc) : 0u;
    float r[kMxLane];
    mx4_decode(word, sc, r);
#pragma unroll
    for (int j = 0; j < kMxLane; ++j) r[j] = normal ? mx_sub(v[j], r[j]) : tiny ? v[j] : 0.f;  // deq is exact
    const int64_t i = u * kMxWave + lane * kMxLane;
    if (i + kMxLane <= n) {
      *reinterpret_cast<uint32_t*>(q + (i >> 1)) = word;
      if (resid) {
        *reinterpret_cast<float4*>(resid + i) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<float4*>(resid + i + 4) = make_float4(r[4], r[5], r[6], r[7]);
      }
    } else {  // never past ceil(n/2) code bytes: the next field starts right after them
#pragma unroll
      for (int j = 0; j < kMxLane; ++j)
        if (i + j < n) {
          if (!(j & 1)) q[(i + j) >> 1] = (uint8_t)(word >> (4 * j));  // a padded high nibble is code 0
          if (resid) resid[i + j] = r[j];
        }
    }
    // the four scale bytes of a 16-lane row in one dword store: each quad shifts its byte into
    // place, half-row mirror + row mirror OR them together in every lane of the row
    const uint32_t sbyte = nonfinite ? 255u : tiny ? 0u : sb;
    uint32_t sw = sbyte << (8 * ((lane >> 2) & 3));
    sw |= mx_dpp<0x141>(sw);
    sw |= mx_dpp<0x140>(sw);
    if ((lane & 15) == 0) {
      const int64_t b = u * (kMxWave / kMxBlock) + (lane >> 4) * 4;
      if (b + 4 <= nblocks) {
        *reinterpret_cast<uint32_t*>(scales + b) = sw;
      } else {  // never past ceil(n/32) scale bytes
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (b + k < nblocks) scales[b + k] = (uint8_t)(sw >> (8 * k));
      }
    }
    u = un;
  }
}

// block scale of byte b: 2^(b - 127), NaN for 255
__device__ __forceinline__ float mx4_scale(uint32_t b) {
  return __uint_as_float(b == 255u ? 0x7fc00000u : b ? b << 23 : 0x00400000u);
}

// acc = gscale * (deq_0 + deq_1 + ...) (rank order, 8 elements per lane), or with ``accumulate``
// acc = ((acc + g*deq_0) + g*deq_1) + ... -- each message on its own, no contraction: batch-
// invariant, as quant.hip k_q8_aggregate
__global__ __launch_bounds__(kBlock) void k_mx4_aggregate(SlotPtrs qs, SlotPtrs ss, int W, float gscale,
                                                          float* __restrict__ acc, int64_t n, int accumulate,
                                                          int acquire) {
  if (acquire) acquire_remote_block();  // a source slot was written by another GPU (common.h)
  const int64_t nv = (n + kMxLane - 1) / kMxLane, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
    const int64_t i = v * kMxLane;
    const bool full = i + kMxLane <= n;
    float a[kMxLane];
    if (accumulate) {
      if (full) {
        const float4 lo = *reinterpret_cast<const float4*>(acc + i), hi = *reinterpret_cast<const float4*>(acc + i + 4);
        a[0] = lo.x; a[1] = lo.y; a[2] = lo.z; a[3] = lo.w;
        a[4] = hi.x; a[5] = hi.y; a[6] = hi.z; a[7] = hi.w;
      } else {
#pragma unroll
        for (int j = 0; j < kMxLane; ++j) a[j] = i + j < n ? acc[i + j] : 0.f;
      }
    }
    for (int w = 0; w < W; ++w) {
      const uint8_t* q = reinterpret_cast<const uint8_t*>(qs.p[w]);
      const float sc = mx4_scale(reinterpret_cast<const uint8_t*>(ss.p[w])[i / kMxBlock]);
      uint32_t word = 0;
      if (full) {
        word = *reinterpret_cast<const uint32_t*>(q + (i >> 1));
      } else {  // never past ceil(n/2) code bytes
#pragma unroll
        for (int j = 0; j < kMxLane; j += 2)
          if (i + j < n) word |= (uint32_t)q[(i + j) >> 1] << (4 * j);
      }
      float d[kMxLane];
      mx4_decode(word, sc, d);
#pragma unroll
      for (int j = 0; j < kMxLane; ++j) {
        if (accumulate)
          a[j] = mx_add(a[j], mx_mul(d[j], gscale));
        else
          a[j] = w == 0 ? d[j] : mx_add(a[j], d[j]);
      }
    }
    if (!accumulate) {
#pragma unroll
      for (int j = 0; j < kMxLane; ++j) a[j] = mx_mul(a[j], gscale);
    }
    if (full) {
      *reinterpret_cast<float4*>(acc + i) = make_float4(a[0], a[1], a[2], a[3]);
      *reinterpret_cast<float4*>(acc + i + 4) = make_float4(a[4], a[5], a[6], a[7]);
    } else {
#pragma unroll
      for (int j = 0; j < kMxLane; ++j)
        if (i + j < n) acc[i + j] = a[j];
    }
  }
}

// ------------------------------------------------------------------------------------------
void mx4_encode(at::Tensor x, c10::optional<at::Tensor> resid, at::Tensor q, at::Tensor scales) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.scalar_type() == at::kFloat, "x: contiguous f32 device tensor");
  const int64_t n = x.numel();
  TORCH_CHECK(q.numel() == (n + 1) / 2 && q.scalar_type() == at::kByte && q.is_contiguous(), "q must be uint8[ceil(n/2)]");
  TORCH_CHECK(scales.numel() == (n + kMxBlock - 1) / kMxBlock && scales.scalar_type() == at::kByte &&
                  scales.is_contiguous(),
              "scales must be uint8[ceil(n/32)]");
  TORCH_CHECK(q.is_cuda() && scales.is_cuda(), "q, scales: device tensors");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(q.data_ptr()) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(scales.data_ptr()) % 4 == 0,
              "x must be 16-byte, q and scales 4-byte aligned");
  float* rp = nullptr;
  if (resid.has_value() && resid->defined()) {
    TORCH_CHECK(resid->is_cuda() && resid->numel() == n && resid->scalar_type() == at::kFloat && resid->is_contiguous(),
                "residual");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(resid->data_ptr()) % 16 == 0, "residual must be 16-byte aligned");
    rp = resid->data_ptr<float>();
  }
  const int grid = grid_for((n + kMxWave - 1) / kMxWave * 64);
  hipLaunchKernelGGL(k_mx4_encode, grid, kBlock, 0, c10::hip::getCurrentHIPStream(), x.data_ptr<float>(), rp,
                     q.data_ptr<uint8_t>(), scales.data_ptr<uint8_t>(), n);
}

void mx4_aggregate(const std::vector<at::Tensor>& qs, const std::vector<at::Tensor>& ss, at::Tensor acc, double gscale,
                   bool accumulate, bool acquire) {
  TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == at::kFloat && acc.is_contiguous(), "acc: f32 device tensor");
  TORCH_CHECK(!qs.empty() && qs.size() == ss.size() && (int)qs.size() <= kMaxSlots, "1..16 (q, scale) pairs");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(acc.data_ptr()) % 16 == 0, "acc must be 16-byte aligned");
  const int64_t n = acc.numel();
  SlotPtrs qp{}, sp{};
  for (size_t w = 0; w < qs.size(); ++w) {
    TORCH_CHECK(qs[w].is_cuda() && qs[w].numel() == (n + 1) / 2 && qs[w].scalar_type() == at::kByte &&
                    qs[w].is_contiguous(),
                "q size/dtype");
    TORCH_CHECK(ss[w].is_cuda() && ss[w].numel() == (n + kMxBlock - 1) / kMxBlock && ss[w].scalar_type() == at::kByte &&
                    ss[w].is_contiguous(),
                "scale size/dtype");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(qs[w].data_ptr()) % 4 == 0, "q must be 4-byte aligned");
    qp.p[w] = qs[w].data_ptr();
    sp.p[w] = ss[w].data_ptr();
  }
  const int grid = grid_for((n + kMxLane - 1) / kMxLane);
  hipLaunchKernelGGL(k_mx4_aggregate, grid, kBlock, 0, c10::hip::getCurrentHIPStream(), qp, sp, (int)qs.size(), (float)gscale,
                     acc.data_ptr<float>(), n, (int)accumulate, (int)acquire);
}

}  // namespace hipps
