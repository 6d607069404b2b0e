// hipps — 1x1-convolution GEMM whose A operand is produced inside the kernel and also stored.
//
//   A[M, K]  = bf16(max(x3 * scale + shift + r, 0))     r = res, or res * rscale + rshift
//   Y[M, N]  = A · W[N, K]^T                            + the BN statistics partials of Y
//
// A is the output of a ResNet bottleneck block (bn3 + residual + ReLU, norm.hip k_bn_apply_fwd)
// and Y the next block's conv1 (gemm.hip k_conv1x1_nt / gemm2.hip k_gemm with the kStats
// epilogue).  Run as two kernels, the widest tensor of the block is written by the first and read
// straight back by the second; here the thread that computes a 16-byte chunk of A stores it to
// ``out`` (with its ReLU bits) and puts it into the GEMM's LDS stage, so A is never re-read.
//
// The kernel is a streaming pass that contains a small matmul, so it is built like the first core
// (register-staged A): the global loads of the x3 / res chunks of K-tile k+1 are issued before the
// MFMAs of tile k, transformed in registers after them, and leave as one 16-byte ``out`` store and
// one ds_write per chunk -- no transform in LDS behind a DMA.  Tiles are 128 x BN x 64 (BN = 64 or
// 128) on 4 waves as 2 x 2 sub-tiles of 64 rows, the row split of gemm2's 128-row tiles, so Y and
// its statistics partials are bitwise those of gemm2_conv (bm = 128) / conv1x1_forward (N % 128
// == 0) on A.  64 KB (BN = 128) or 48 KB (BN = 64) of LDS and <= 128 registers keep two or three
// blocks per CU, whose loads cover one another's latency as the apply kernel's waves do.
// With several column tiles (N > BN) every column tile builds A from x3 / res -- the re-reads hit
// the L2 of the XCD the block order keeps them on -- and only column tile 0 stores out / bits.
//
// The A producer is a struct with two members, fetch / emit; two of them feed the same main loop:
//
//   BnResRelu    the forward above
//   BnBwdApply   the backward twin: A = bn3's input gradient, bf16(a * dz + k1 * x3 + k0) with dz =
//                dy where bn3's ReLU bit is set (norm.hip k_bn_apply_bwd<MASK_BITS>), stored once
//                to dx3 (conv3's weight gradient reads it there), and Y = A . Wt^T is conv3's input
//                gradient, the gradient of bn2's output, with bn2's backward reduction in the
//                epilogue (gemm2.hip kBst: relu' recomputed from x2 * scale2 + shift2): bitwise
//                gemm2_conv(bm = 128, bn = BN) with its bn_x arguments on the applied dx3.
#include "common.h"

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

namespace hipps {
namespace bnconv {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BK = 64;
constexpr int A_CH = BM * BK / 8 / 256;  // 16-byte A chunks per thread per K-tile

template <int BN>
constexpr int lds_elems() {
  constexpr int stage = 2 * (BM + BN) * BK;
  constexpr int epi = BM * (BN + 8);
  return (stage > epi ? stage : epi) + 2 * 2 * 2 * BN;  // + stats scratch [2 row halves][BN][2] floats
}

struct Args {
  const uint16_t *x3, *res, *W;
  uint16_t *out, *Y;
  uint8_t* bits;
  float *pa, *pb;
  const float *sc, *sh, *rsc, *rsh;
  int M, N, K, mtiles, ntiles;
  // backward (BnBwdApply + the BST epilogue): x3 / out / bits / W / Y / pa / pb as above (out = dx3,
  // bits read), dy the gradient of bn3's output, a / k1 / k0 bn3's input-gradient coefficients [K],
  // bx the input of the BN whose output gradient Y is, with that BN's mean / invstd / scale / shift [N]
  const uint16_t *dy, *bx;
  const float *ca, *ck1, *ck0, *bmean, *binvstd, *bscale, *bshift;
};

__device__ __forceinline__ void load8f(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// A producer: relu(bn3(x3) + residual), element for element norm.hip k_bn_apply_fwd.
//   fetch(off, c)   issue the loads of one 16-byte chunk (element offset off) per slot, and of the
//                   per-channel constants of channels c .. c+7
//   emit(i, ...)    the bf16 A chunk of slot i; with ``store`` also written to out, and its ReLU
//                   bits (one byte; the 8 lanes of a row's K-tile pack theirs into one 8-byte store)
template <bool DUAL>
struct BnResRelu {
  u32x4 xv[A_CH], rv[A_CH];
  float s[8], h[8], rs[DUAL ? 8 : 1], rh[DUAL ? 8 : 1];

  __device__ __forceinline__ void fetch(const Args& g, const int64_t (&off)[A_CH], int k0, int c) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      xv[i] = *reinterpret_cast<const u32x4*>(g.x3 + off[i] + k0);
      rv[i] = *reinterpret_cast<const u32x4*>(g.res + off[i] + k0);
    }
    load8f(g.sc + c, s);
    load8f(g.sh + c, h);
    if constexpr (DUAL) {
      load8f(g.rsc + c, rs);
      load8f(g.rsh + c, rh);
    }
  }

  __device__ __forceinline__ u32x4 emit(const Args& g, int i, bool ok, bool store, int64_t o, int lane) const {
    const uint32_t xw[4] = {xv[i].x, xv[i].y, xv[i].z, xv[i].w};
    const uint32_t rw[4] = {rv[i].x, rv[i].y, rv[i].z, rv[i].w};
    uint32_t ow[4];
    uint32_t b = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t xu = xw[j >> 1], ru = rw[j >> 1];
      float v = fmaf(__uint_as_float(j & 1 ? xu & 0xffff0000u : xu << 16), s[j], h[j]);
      float r = __uint_as_float(j & 1 ? ru & 0xffff0000u : ru << 16);
      if constexpr (DUAL) r = fmaf(r, rs[j], rh[j]);
      v += r;
      v = fmaxf(v, 0.f);
      b |= (v > 0.f ? 1u : 0u) << j;
      const uint32_t hb = f32_to_bf16(v);
      if (j & 1) ow[j >> 1] |= hb << 16;
      else ow[j >> 1] = hb;
    }
    const u32x4 a = ok ? u32x4{ow[0], ow[1], ow[2], ow[3]} : u32x4{0u, 0u, 0u, 0u};
    // the 8 bytes of lanes 8q .. 8q+7 (one row's 64 channels) gathered into lane 8q
    const uint32_t b2 = b | (__shfl_down(b, 1, 64) << 8);
    const uint32_t b4 = b2 | (__shfl_down(b2, 2, 64) << 16);
    const uint32_t b8 = __shfl_down(b4, 4, 64);
    if (store && ok) {
      *reinterpret_cast<u32x4*>(g.out + o) = a;
      if ((lane & 7) == 0) *reinterpret_cast<uint2*>(g.bits + (o >> 3)) = make_uint2(b4, b8);
    }
    return a;
  }
};

// A producer: bn3's input gradient, element for element norm.hip k_bn_apply_bwd<MASK_BITS> without
// a residual gradient output (same fetch / emit shape; the ReLU bits are read here, one byte per chunk)
struct BnBwdApply {
  u32x4 dv[A_CH], xv[A_CH];
  uint32_t mb[A_CH];
  float a[8], k1[8], k0[8];

  __device__ __forceinline__ void fetch(const Args& g, const int64_t (&off)[A_CH], int kk, int c) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      dv[i] = *reinterpret_cast<const u32x4*>(g.dy + off[i] + kk);
      xv[i] = *reinterpret_cast<const u32x4*>(g.x3 + off[i] + kk);
      mb[i] = g.bits[(off[i] + kk) >> 3];
    }
    load8f(g.ca + c, a);
    load8f(g.ck1 + c, k1);
    load8f(g.ck0 + c, k0);
  }

  __device__ __forceinline__ u32x4 emit(const Args& g, int i, bool ok, bool store, int64_t o, int) const {
    const uint32_t dw[4] = {dv[i].x, dv[i].y, dv[i].z, dv[i].w};
    const uint32_t xw[4] = {xv[i].x, xv[i].y, xv[i].z, xv[i].w};
    uint32_t ow[4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t du = dw[j >> 1], xu = xw[j >> 1];
      const float d = __uint_as_float(j & 1 ? du & 0xffff0000u : du << 16);
      const float x = __uint_as_float(j & 1 ? xu & 0xffff0000u : xu << 16);
      const float dz = ((mb[i] >> j) & 1u) ? d : 0.f;
      const uint32_t hb = f32_to_bf16(fmaf(a[j], dz, fmaf(k1[j], x, k0[j])));
      if (j & 1) ow[j >> 1] |= hb << 16;
      else ow[j >> 1] = hb;
    }
    const u32x4 v = ok ? u32x4{ow[0], ow[1], ow[2], ow[3]} : u32x4{0u, 0u, 0u, 0u};
    if (store && ok) *reinterpret_cast<u32x4*>(g.out + o) = v;
    return v;
  }
};

// BST: the epilogue is gemm2's kBst (the backward reduction of the BN whose output gradient Y is)
// instead of the forward statistics of Y
template <int BN, class Prod, bool BST>
__global__ __launch_bounds__(256, 2) void k_bnconv(Args g) {
  constexpr int WM = 2, WN = 2;
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int FM = TM / 16, FN = TN / 16;
  constexpr int B_CH = BN * BK / 8 / 256;
  constexpr int STAGE = (BM + BN) * BK;  // elements
  constexpr int EP = BN + 8;             // epilogue row pitch (elements)
  __shared__ __attribute__((aligned(16))) uint16_t lds[lds_elems<BN>()];

  // bijective XCD-aware block order (gemm2.hip): each XCD gets a contiguous run of tiles, so the
  // column tiles of one row tile share an L2
  const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int mt = bid / g.ntiles, nt = bid - mt * g.ntiles;
  const int m0 = mt * BM, n0 = nt * BN;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wm = w / WN, wn = w % WN;
  const int cchunk = t & 7;  // the 16-byte chunk (k / 8) of a K-tile row this thread stages, fixed
  const bool store = nt == 0;
  const int K = g.K;

  // per-thread A rows (fixed over the K loop); rows past M read row M - 1 and stage zeros
  int64_t a_off[A_CH];
  bool a_ok[A_CH];
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    const int m = m0 + (t >> 3) + 32 * i;
    a_ok[i] = m < g.M;
    a_off[i] = (int64_t)(a_ok[i] ? m : g.M - 1) * K + cchunk * 8;
  }
  int64_t b_off[B_CH];
#pragma unroll
  for (int i = 0; i < B_CH; ++i) b_off[i] = (int64_t)(n0 + (t >> 3) + 32 * i) * K + cchunk * 8;

  Prod prod;
  u32x4 rb[B_CH];
  // (macros, not lambdas: by-reference captures of register arrays end up in scratch)
#define HIPPS_BC_LOAD(kt_)                                                                  \
  {                                                                                         \
    const int k0_ = (kt_) * BK;                                                             \
    prod.fetch(g, a_off, k0_, k0_ + cchunk * 8);                                            \
    _Pragma("unroll") for (int i = 0; i < B_CH; ++i) rb[i] =                                \
        *reinterpret_cast<const u32x4*>(g.W + b_off[i] + k0_);                              \
  }
#define HIPPS_BC_STAGE(kt_, s_)                                                             \
  {                                                                                         \
    uint16_t* base_ = lds + (s_) * STAGE;                                                   \
    const int k0_ = (kt_) * BK;                                                             \
    _Pragma("unroll") for (int i = 0; i < A_CH; ++i) {                                      \
      const int row_ = (t >> 3) + 32 * i;                                                   \
      const u32x4 v_ = prod.emit(g, i, a_ok[i], store, a_off[i] + k0_, lane);               \
      *reinterpret_cast<u32x4*>(base_ + row_ * BK + ((cchunk ^ (row_ & 7)) << 3)) = v_;     \
    }                                                                                       \
    _Pragma("unroll") for (int i = 0; i < B_CH; ++i) {                                      \
      const int row_ = (t >> 3) + 32 * i;                                                   \
      *reinterpret_cast<u32x4*>(base_ + BM * BK + row_ * BK + ((cchunk ^ (row_ & 7)) << 3)) = rb[i]; \
    }                                                                                       \
  }

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int KT = K / BK;
  HIPPS_BC_LOAD(0);
  HIPPS_BC_STAGE(0, 0);
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) HIPPS_BC_LOAD(kt + 1);
    const uint16_t* As = lds + cur * STAGE;
    const uint16_t* Bs = As + BM * BK;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      const int c = ks * 4 + (lane >> 4);
      bf16x8 a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int row = wm * TM + i * 16 + (lane & 15);
        a[i] = *reinterpret_cast<const bf16x8*>(As + row * BK + ((c ^ (row & 7)) << 3));
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int row = wn * TN + j * 16 + (lane & 15);
        b[j] = *reinterpret_cast<const bf16x8*>(Bs + row * BK + ((c ^ (row & 7)) << 3));
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < KT) HIPPS_BC_STAGE(kt + 1, cur ^ 1);
    __syncthreads();
  }
#undef HIPPS_BC_LOAD
#undef HIPPS_BC_STAGE

  // C/D map (16x16x32): column = lane & 15, row = (lane >> 4) * 4 + r.  Rows past M hold zeros.
  constexpr int RCH = BN / 8;            // 16-byte chunks per output row
  constexpr int NOUT = BM * RCH / 256;   // output chunks per thread
  if constexpr (BST) {
    // ---- epilogue (gemm2.hip kBst, element for element): bf16 tile -> LDS, 16-byte row stores, and
    // on the stored bf16 values dz = dy * relu'(x * scale + shift), sum dz and sum dz * x-hat per
    // channel: the thread's NOUT rows in order, then its 256 / RCH row lanes through LDS in order ----
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int col = wn * TN + j * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wm * TM + i * 16 + (lane >> 4) * 4 + r;
          lds[row * EP + col] = f32_to_bf16(acc[i][j][r]);
        }
      }
    }
    __syncthreads();
    const int cc = (t % RCH) * 8;  // this thread's 8 channels are fixed (256 % RCH == 0)
    float bmu[8], bis[8], bsc[8], bsh[8], bsa[8], bsb[8];
    load8f(g.bmean + n0 + cc, bmu);
    load8f(g.binvstd + n0 + cc, bis);
    load8f(g.bscale + n0 + cc, bsc);
    load8f(g.bshift + n0 + cc, bsh);
    u32x4 lx[NOUT];  // (the accumulators are retired: all of the BN input chunks in flight together)
#pragma unroll
    for (int i = 0; i < NOUT; ++i) {
      const int row = (t + 256 * i) / RCH;
      lx[i] = *reinterpret_cast<const u32x4*>(g.bx + (int64_t)(m0 + row < g.M ? m0 + row : m0) * g.N + n0 + cc);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) bsa[j] = bsb[j] = 0.f;
#pragma unroll
    for (int i = 0; i < NOUT; ++i) {
      const int row = (t + 256 * i) / RCH;
      if (m0 + row < g.M) {
        const uint4 v = *reinterpret_cast<const uint4*>(lds + row * EP + cc);
        *reinterpret_cast<uint4*>(g.Y + (int64_t)(m0 + row) * g.N + n0 + cc) = v;
        const uint32_t dv[4] = {v.x, v.y, v.z, v.w};
        const uint32_t xw[4] = {lx[i].x, lx[i].y, lx[i].z, lx[i].w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = __uint_as_float(j & 1 ? dv[j >> 1] & 0xffff0000u : dv[j >> 1] << 16);
          const float xv = __uint_as_float(j & 1 ? xw[j >> 1] & 0xffff0000u : xw[j >> 1] << 16);
          const float dz = fmaf(xv, bsc[j], bsh[j]) > 0.f ? d : 0.f;
          bsa[j] += dz;
          bsb[j] = fmaf(dz, (xv - bmu[j]) * bis[j], bsb[j]);
        }
      }
    }
    constexpr int RL = 256 / RCH;
    static_assert(2 * RL * BN * 2 <= 2 * STAGE, "BST scratch");
    float* red = reinterpret_cast<float*>(lds);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[(t / RCH) * BN + cc + j] = bsa[j];
      red[RL * BN + (t / RCH) * BN + cc + j] = bsb[j];
    }
    __syncthreads();
    if (t < BN) {
      float sa = 0.f, sb = 0.f;
      for (int r = 0; r < RL; ++r) {
        sa += red[r * BN + t];
        sb += red[RL * BN + r * BN + t];
      }
      g.pa[(int64_t)(n0 + t) * g.mtiles + mt] = sa;
      g.pb[(int64_t)(n0 + t) * g.mtiles + mt] = sb;
    }
    return;
  }
  // ---- epilogue (the kStats epilogue of the GEMM cores): bf16 tile -> LDS (padded rows), per-
  // channel sum / sum of squares of the stored bf16 values, 16-byte row stores ----
  float* st = reinterpret_cast<float*>(lds + (2 * STAGE > BM * EP ? 2 * STAGE : BM * EP));
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int col = wn * TN + j * 16 + (lane & 15);
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * TM + i * 16 + (lane >> 4) * 4 + r;
        const uint16_t hb = f32_to_bf16(acc[i][j][r]);
        lds[row * EP + col] = hb;
        const float v = bf16_to_f32(hb);
        s += v;
        q = fmaf(v, v, q);
      }
    }
    s += __shfl_xor(s, 16, 64);
    q += __shfl_xor(q, 16, 64);
    s += __shfl_xor(s, 32, 64);
    q += __shfl_xor(q, 32, 64);
    if (lane < 16) {
      st[(wm * BN + col) * 2] = s;
      st[(wm * BN + col) * 2 + 1] = q;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NOUT; ++i) {
    const int id = t + 256 * i;
    const int row = id / RCH, c = id - row * RCH;
    if (m0 + row < g.M)
      *reinterpret_cast<uint4*>(g.Y + (int64_t)(m0 + row) * g.N + n0 + c * 8) =
          *reinterpret_cast<const uint4*>(lds + row * EP + c * 8);
  }
  if (t < BN) {
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      s += st[(i * BN + t) * 2];
      q += st[(i * BN + t) * 2 + 1];
    }
    g.pa[(int64_t)(n0 + t) * g.mtiles + mt] = s;
    g.pb[(int64_t)(n0 + t) * g.mtiles + mt] = q;
  }
}

}  // namespace bnconv

int64_t bnconv_mtiles(int64_t M) { return (M + bnconv::BM - 1) / bnconv::BM; }

// out = relu(x3 * scale + shift + r) with its ReLU bits, y = out . w^T and the BN statistics
// partials of y, in one kernel.  x3 / res / out: bf16 [M, K] (channels-last storage); w: bf16
// [N, K]; y: bf16 [M, N]; bits: uint8 [M * K / 8]; part: f32 [2, N, bnconv_mtiles(M)]; scale /
// shift (and rscale / rshift, the residual's own BN in a downsample block): f32 [K].
void bnconv_forward(at::Tensor x3, at::Tensor res, at::Tensor scale, at::Tensor shift,
                    c10::optional<at::Tensor> rscale, c10::optional<at::Tensor> rshift, at::Tensor w, at::Tensor out,
                    at::Tensor bits, at::Tensor y, at::Tensor part) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 && w.is_contiguous(), "bnconv: w must be bf16 [N, K]");
  const int64_t N = w.size(0), K = w.numel() / N;
  TORCH_CHECK(K % 64 == 0 && N % 64 == 0, "bnconv: needs K % 64 == 0 and N % 64 == 0");
  const int64_t M = x3.numel() / K;
  TORCH_CHECK(M > 0 && M * K == x3.numel() && M < (int64_t(1) << 31), "bnconv: x3 size");
  for (const at::Tensor* t : {&x3, &res, &out}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16 && t->numel() == M * K &&
                    (t->is_contiguous(at::MemoryFormat::ChannelsLast) || (t->dim() != 4 && t->is_contiguous())),
                "bnconv: x3 / res / out must be channels-last bf16 tensors of one size");
  }
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kBFloat16 && y.numel() == M * N &&
                  (y.is_contiguous(at::MemoryFormat::ChannelsLast) || (y.dim() != 4 && y.is_contiguous())),
              "bnconv: y must be a channels-last bf16 [M, N] tensor");
  for (const at::Tensor* t : {&x3, &res, &out, &y, &w, &bits})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "bnconv: 16-byte aligned tensors");
  TORCH_CHECK(bits.is_cuda() && bits.scalar_type() == at::kByte && bits.is_contiguous() && bits.numel() == M * K / 8,
              "bnconv: bits must be uint8[M*K/8]");
  const int64_t mtiles = bnconv_mtiles(M);
  TORCH_CHECK(part.is_cuda() && part.scalar_type() == at::kFloat && part.is_contiguous() &&
                  part.numel() == 2 * N * mtiles, "bnconv: part must be f32 [2, N, mtiles]");
  const bool dual = rscale.has_value() && rscale->defined();
  TORCH_CHECK(dual == (rshift.has_value() && rshift->defined()), "bnconv: rscale and rshift come together");
  auto vec = [&](const at::Tensor& v) {
    TORCH_CHECK(v.is_cuda() && v.scalar_type() == at::kFloat && v.is_contiguous() && v.numel() == K &&
                    reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0, "bnconv: per-channel vectors must be f32 [K]");
  };
  vec(scale);
  vec(shift);
  if (dual) {
    vec(*rscale);
    vec(*rshift);
  }
  const bool bn128 = N % 128 == 0;
  const int64_t ntiles = N / (bn128 ? 128 : 64);
  const int64_t nblk = mtiles * ntiles;
  TORCH_CHECK(nblk < (int64_t(1) << 31), "bnconv: grid");
  bnconv::Args g{};
  g.x3 = (const uint16_t*)x3.data_ptr();
  g.res = (const uint16_t*)res.data_ptr();
  g.W = (const uint16_t*)w.data_ptr();
  g.out = (uint16_t*)out.data_ptr();
  g.Y = (uint16_t*)y.data_ptr();
  g.bits = (uint8_t*)bits.data_ptr();
  g.pa = part.data_ptr<float>();
  g.pb = g.pa + N * mtiles;
  g.sc = scale.data_ptr<float>();
  g.sh = shift.data_ptr<float>();
  g.rsc = dual ? rscale->data_ptr<float>() : nullptr;
  g.rsh = dual ? rshift->data_ptr<float>() : nullptr;
  g.M = (int)M;
  g.N = (int)N;
  g.K = (int)K;
  g.mtiles = (int)mtiles;
  g.ntiles = (int)ntiles;
  auto stream = c10::hip::getCurrentHIPStream();
#define HIPPS_BC(BNv, DUALv) \
  hipLaunchKernelGGL((bnconv::k_bnconv<BNv, bnconv::BnResRelu<DUALv>, false>), (int)nblk, 256, 0, stream, g)
  if (bn128) {
    if (dual) HIPPS_BC(128, true); else HIPPS_BC(128, false);
  } else {
    if (dual) HIPPS_BC(64, true); else HIPPS_BC(64, false);
  }
#undef HIPPS_BC
}

// dx3 = a * dz + k1 * x3 + k0 (dz = dy where bn3's ReLU bit is set: bn3's input gradient), dbn =
// dx3 . wt^T (conv3's input gradient, the gradient of bn2's output) and bn2's backward reduction
// partials of dbn, in one kernel.  dy / x3 / dx3: bf16 [M, K] (channels-last storage); bits: uint8
// [M * K / 8]; coef: f32 [3, K] = (a, k1, k0) (bn_finalize_bwd_partials); wt: bf16 [N, K]; dbn /
// bn_x: bf16 [M, N]; part: f32 [2, N, bnconv_mtiles(M)]; bn_mean / bn_invstd / bn_scale / bn_shift:
// f32 [N].  bn: the column tile, 64 or 128 (0: 128 if it divides N) -- dbn and part are bitwise
// those of gemm2_conv(bm = 128, bn) with the bn_x arguments on the applied dx3.
void bnconv_backward(at::Tensor dy, at::Tensor x3, at::Tensor bits, at::Tensor coef, at::Tensor wt, at::Tensor dx3,
                     at::Tensor dbn, at::Tensor part, at::Tensor bn_x, at::Tensor bn_mean, at::Tensor bn_invstd,
                     at::Tensor bn_scale, at::Tensor bn_shift, int64_t bn) {
  TORCH_CHECK(wt.is_cuda() && wt.scalar_type() == at::kBFloat16 && wt.is_contiguous(), "bnconv: wt must be bf16 [N, K]");
  const int64_t N = wt.size(0), K = wt.numel() / N;
  TORCH_CHECK(K % 64 == 0 && N % 64 == 0, "bnconv: needs K % 64 == 0 and N % 64 == 0");
  if (bn == 0) bn = N % 128 == 0 ? 128 : 64;
  TORCH_CHECK((bn == 64 || bn == 128) && N % bn == 0, "bnconv: bn must be 64 or 128 and divide N");
  const int64_t M = x3.numel() / K;
  TORCH_CHECK(M > 0 && M * K == x3.numel() && M < (int64_t(1) << 31), "bnconv: x3 size");
  for (const at::Tensor* t : {&dy, &x3, &dx3}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16 && t->numel() == M * K &&
                    (t->is_contiguous(at::MemoryFormat::ChannelsLast) || (t->dim() != 4 && t->is_contiguous())),
                "bnconv: dy / x3 / dx3 must be channels-last bf16 tensors of one size");
  }
  for (const at::Tensor* t : {&dbn, &bn_x}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16 && t->numel() == M * N &&
                    (t->is_contiguous(at::MemoryFormat::ChannelsLast) || (t->dim() != 4 && t->is_contiguous())),
                "bnconv: dbn / bn_x must be channels-last bf16 [M, N] tensors");
  }
  for (const at::Tensor* t : {&dy, &x3, &dx3, &dbn, &bn_x, &wt, &bits, &coef})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "bnconv: 16-byte aligned tensors");
  TORCH_CHECK(bits.is_cuda() && bits.scalar_type() == at::kByte && bits.is_contiguous() && bits.numel() == M * K / 8,
              "bnconv: bits must be uint8[M*K/8]");
  TORCH_CHECK(coef.is_cuda() && coef.scalar_type() == at::kFloat && coef.is_contiguous() && coef.numel() == 3 * K,
              "bnconv: coef must be f32 [3, K]");
  const int64_t mtiles = bnconv_mtiles(M);
  TORCH_CHECK(part.is_cuda() && part.scalar_type() == at::kFloat && part.is_contiguous() &&
                  part.numel() == 2 * N * mtiles, "bnconv: part must be f32 [2, N, mtiles]");
  for (const at::Tensor* v : {&bn_mean, &bn_invstd, &bn_scale, &bn_shift})
    TORCH_CHECK(v->is_cuda() && v->scalar_type() == at::kFloat && v->is_contiguous() && v->numel() == N &&
                    reinterpret_cast<uintptr_t>(v->data_ptr()) % 16 == 0, "bnconv: per-channel vectors must be f32 [N]");
  const int64_t ntiles = N / bn;
  const int64_t nblk = mtiles * ntiles;
  TORCH_CHECK(nblk < (int64_t(1) << 31), "bnconv: grid");
  bnconv::Args g{};
  g.dy = (const uint16_t*)dy.data_ptr();
  g.x3 = (const uint16_t*)x3.data_ptr();
  g.bits = (uint8_t*)bits.data_ptr();
  g.ca = coef.data_ptr<float>();
  g.ck1 = g.ca + K;
  g.ck0 = g.ca + 2 * K;
  g.W = (const uint16_t*)wt.data_ptr();
  g.out = (uint16_t*)dx3.data_ptr();
  g.Y = (uint16_t*)dbn.data_ptr();
  g.pa = part.data_ptr<float>();
  g.pb = g.pa + N * mtiles;
  g.bx = (const uint16_t*)bn_x.data_ptr();
  g.bmean = bn_mean.data_ptr<float>();
  g.binvstd = bn_invstd.data_ptr<float>();
  g.bscale = bn_scale.data_ptr<float>();
  g.bshift = bn_shift.data_ptr<float>();
  g.M = (int)M;
  g.N = (int)N;
  g.K = (int)K;
  g.mtiles = (int)mtiles;
  g.ntiles = (int)ntiles;
  auto stream = c10::hip::getCurrentHIPStream();
  if (bn == 128)
    hipLaunchKernelGGL((bnconv::k_bnconv<128, bnconv::BnBwdApply, true>), (int)nblk, 256, 0, stream, g);
  else
    hipLaunchKernelGGL((bnconv::k_bnconv<64, bnconv::BnBwdApply, true>), (int)nblk, 256, 0, stream, g);
}

}  // namespace hipps
