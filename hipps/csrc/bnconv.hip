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
// The A producer is a struct (BnResRelu): a second one of the same shape (fetch / emit) can feed
// the same main loop.
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

template <int BN, bool DUAL>
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

  BnResRelu<DUAL> prod;
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

  // ---- epilogue (the kStats epilogue of the GEMM cores): bf16 tile -> LDS (padded rows), per-
  // channel sum / sum of squares of the stored bf16 values, 16-byte row stores ----
  // C/D map (16x16x32): column = lane & 15, row = (lane >> 4) * 4 + r.  Rows past M hold zeros.
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
  constexpr int RCH = BN / 8;            // 16-byte chunks per output row
  constexpr int NOUT = BM * RCH / 256;   // output chunks per thread
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
  bnconv::Args g;
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
#define HIPPS_BC(BNv, DUALv) hipLaunchKernelGGL((bnconv::k_bnconv<BNv, DUALv>), (int)nblk, 256, 0, stream, g)
  if (bn128) {
    if (dual) HIPPS_BC(128, true); else HIPPS_BC(128, false);
  } else {
    if (dual) HIPPS_BC(64, true); else HIPPS_BC(64, false);
  }
#undef HIPPS_BC
}

}  // namespace hipps
