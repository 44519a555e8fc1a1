// Squeeze-excite and hardswish for gfx950 (MobileNetV3, EfficientNet): NHWC
// bf16/fp16 activations as rows [R = N*HW, C], fp32 weights and statistics.
//
//   y = a(x) * s[n, c],  s = gate(W2 . hid(W1 . mean_hw(a(x)) + b1) + b2)
//
// hid is ReLU or SiLU, gate is hardsigmoid or sigmoid (template parameters
// HID, GATE of the two MLP kernels): MobileNetV3 is ReLU + hardsigmoid,
// EfficientNet SiLU + sigmoid.
// a is the identity or hardswish (template parameter HSW): with HSW the
// input is the linear BN output and the activation is never written.  The
// op is pure HBM traffic around a tiny MLP, so the design is about touching
// the tensor the minimum number of times (3 passes forward, 4 backward) and
// filling the chip at small N * C:
//
//  * Tensor passes (se_squeeze, se_scale, se_bwd_reduce, se_bwd_apply) share
//    one geometry (se_geo): the C/8 16-byte packs of a row are cut into G
//    groups of PX <= 64 packs, a block of 256 threads is PX pack lanes x RS
//    row slots, and owns one image, one pack group and one run of rows.  A
//    lane keeps its pack for the whole run: the apply kernels read their
//    per-(image, pack) operands (s, dm) once, the reduce kernels accumulate
//    in registers and fold the RS slots through LDS in slot order.
//  * The reduce kernels write fp32 partials [N, S, C], S row splits chosen
//    on the host so that N * G * S blocks fill the chip; the MLP kernels
//    fold the S partials in order.  No atomics anywhere: every sum has a
//    fixed order, results are bitwise reproducible.
//  * The MLP kernels (se_excite, se_excite_bwd) run one block of 1024
//    threads per image with mean / h / dz in LDS.  W . v products take one
//    wave per output row (lanes stride over the row, coalesced, shuffle
//    tree); W^T . v products take one thread per output column and split the
//    rows over the thread groups that are left, folded through LDS in group
//    order.  Weights are read as fp32 straight from the parameters.
//  * se_wgrad: one launch, one thread per element of dW1, dW2, db1, db2,
//    n ascending.
//
// hardswish(x) = x * relu6(x + 3) / 6.  Derivative convention (that of
// torch's hardswish backward, checked on the CPU in tests/test_mobilenetv3.py):
//   x <= -3: 0;  -3 < x < 3: x / 3 + 1 / 2;  x >= 3: 1
// so the kinks belong to the flat pieces: exactly 0 at x = -3 and exactly 1
// at x = 3, on bf16 inputs that land there as on any other.
// The hardsigmoid gate's derivative is 1/6 strictly inside (0 < s < 1) and
// 0 where it saturates, torch's convention again.
//
// The sigmoid gate's slope s (1 - s) comes from the saved s.  A SiLU hidden
// unit's slope sg (1 + z1 (1 - sg)), sg = sigmoid(z1), cannot be had from
// h = z1 sg (h is not monotone in z1), so the forward keeps the
// pre-activation as well: under SiLU se_excite returns z1 [N, Cs] as a
// fourth tensor and se_excite_bwd takes it where ReLU passes h.  A second
// [N, Cs] fp32 tensor (48 KiB at N = 256, Cs = 48) rather than z1 alone with
// h recomputed in se_wgrad: there every thread of a dW2 row would redo the
// same N sigmoids, C times over, to save a tensor a thousandth of x's size.
// sigmoid(z) = 1 / (1 + 2^fl(-z log2 e)) on v_exp_f32 and v_rcp_f32 (1 ulp
// each; batchnorm_anyc.h has the error account): z far negative gives
// 2^.. = inf, s = 0 and slope 0, never NaN.
#include "common.h"

// No packed-fp32 selection (v_pk_*_f32) for the code of this file (see
// lars.hip): a device target feature, switched off per function.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int SE_TPB = 256;       // tensor passes
constexpr int SE_MLP_TPB = 1024;  // one block per image
constexpr int SE_ROWS_PER_SLOT = 8;  // apply kernels: rows per lane and block

// __syncthreads(), spelled out: the header's function lacks this file's
// target attribute and would stay a call
__device__ __forceinline__ void se_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float hsw(float x) {
  return x * (fminf(fmaxf(x + 3.f, 0.f), 6.f) * (1.f / 6.f));
}

__device__ __forceinline__ float hsw_grad(float x) {
  const float mid = __builtin_fmaf(x, 1.f / 3.f, 0.5f);
  return x <= -3.f ? 0.f : (x >= 3.f ? 1.f : mid);
}

constexpr int SE_HID_RELU = 0, SE_HID_SILU = 1;
constexpr int SE_GATE_HSIG = 0, SE_GATE_SIGMOID = 1;

__device__ __forceinline__ float se_sigmoid(float z) {
  const float e = __builtin_amdgcn_exp2f(z * -1.44269504088896341f);
  return __builtin_amdgcn_rcpf(1.f + e);
}

template <bool HSW> __device__ __forceinline__ float se_act(float x) {
  return HSW ? hsw(x) : x;
}

// block (n, pack group) from blockIdx.x, lane (pack, row slot) from the
// thread index; ok: the lane has a pack and a slot
struct SeLane {
  long n;
  int c0, px, rs;
  bool ok;
};

__device__ __forceinline__ SeLane se_lane(int C, int G, int PX, int RS) {
  SeLane l;
  const int g = blockIdx.x % G;
  l.n = blockIdx.x / G;
  l.px = threadIdx.x % PX;
  l.rs = threadIdx.x / PX;
  l.c0 = (g * PX + l.px) * 8;
  l.ok = l.rs < RS && l.c0 < C;
  return l;
}

// part[n, split, c] = sum over the split's pixels of a(x) (DY: of dy * a(x))
template <typename T, bool HSW, bool DY>
__global__ void __launch_bounds__(SE_TPB)
se_reduce_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                 float* __restrict__ part, int HW, int C, int G, int PX,
                 int RS, int S) {
  __shared__ float red[SE_TPB * 8];  // [RS][PX * 8]
  const SeLane l = se_lane(C, G, PX, RS);
  const int split = blockIdx.y;
  const int chunk = (HW + S - 1) / S;
  const int lo = split * chunk, hi = min(HW, lo + chunk);
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  if (l.ok) {
    const long base = l.n * HW * (long)C + l.c0;
#pragma unroll 4
    for (int r = lo + l.rs; r < hi; r += RS) {
      const long off = base + (long)r * C;
      const Pack<T, 8> xv = *(const Pack<T, 8>*)(x + off);
      if (DY) {
        const Pack<T, 8> gv = *(const Pack<T, 8>*)(dy + off);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          acc[k] += to_f32(gv.v[k]) * se_act<HSW>(to_f32(xv.v[k]));
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += se_act<HSW>(to_f32(xv.v[k]));
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) red[(l.rs * PX + l.px) * 8 + k] = acc[k];
  }
  se_barrier();
  // fold the row slots in slot order; thread t owns channel t of the group
  const int t = threadIdx.x;
  for (int col = t; col < PX * 8; col += SE_TPB) {
    const int c = (blockIdx.x % G) * PX * 8 + col;
    if (c < C) {
      float s = 0.f;
      for (int rs = 0; rs < RS; ++rs) s += red[rs * PX * 8 + col];
      part[(l.n * S + split) * C + c] = s;
    }
  }
}

// y = a(x) * s  (BWD: dx = (dy * s + dm) * a'(x))
template <typename T, bool HSW, bool BWD>
__global__ void __launch_bounds__(SE_TPB)
se_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                const float* __restrict__ s, const float* __restrict__ dm,
                T* __restrict__ out, int HW, int C, int G, int PX, int RS) {
  const SeLane l = se_lane(C, G, PX, RS);
  if (!l.ok) return;
  const int chunk = RS * SE_ROWS_PER_SLOT;
  const int lo = blockIdx.y * chunk, hi = min(HW, lo + chunk);
  float sv[8], dv[8];
  {
    const float4* sp = (const float4*)(s + l.n * C + l.c0);
    const float4 a = sp[0], b = sp[1];
    sv[0] = a.x; sv[1] = a.y; sv[2] = a.z; sv[3] = a.w;
    sv[4] = b.x; sv[5] = b.y; sv[6] = b.z; sv[7] = b.w;
  }
  if (BWD) {
    const float4* dp = (const float4*)(dm + l.n * C + l.c0);
    const float4 a = dp[0], b = dp[1];
    dv[0] = a.x; dv[1] = a.y; dv[2] = a.z; dv[3] = a.w;
    dv[4] = b.x; dv[5] = b.y; dv[6] = b.z; dv[7] = b.w;
  }
  const long base = l.n * HW * (long)C + l.c0;
#pragma unroll 4
  for (int r = lo + l.rs; r < hi; r += RS) {
    const long off = base + (long)r * C;
    Pack<T, 8> o;
    if (BWD) {
      const Pack<T, 8> gv = *(const Pack<T, 8>*)(dy + off);
      if (HSW) {
        const Pack<T, 8> xv = *(const Pack<T, 8>*)(x + off);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          o.v[k] = from_f32<T>(
              __builtin_fmaf(to_f32(gv.v[k]), sv[k], dv[k]) *
              hsw_grad(to_f32(xv.v[k])));
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          o.v[k] = from_f32<T>(__builtin_fmaf(to_f32(gv.v[k]), sv[k], dv[k]));
      }
    } else {
      const Pack<T, 8> xv = *(const Pack<T, 8>*)(x + off);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        o.v[k] = from_f32<T>(se_act<HSW>(to_f32(xv.v[k])) * sv[k]);
    }
    *(Pack<T, 8>*)(out + off) = o;
  }
}

// out[i] = post(sum_k M[i * K + k] * v[k]) for i < n_out: one wave per row,
// lanes stride over k (coalesced), fixed shuffle tree; a wave keeps four
// rows in flight to hide the load and shuffle latencies.  v in LDS.
template <typename Post>
__device__ __forceinline__ void se_matvec(const float* __restrict__ M,
                                          const float* v, int n_out, int K,
                                          Post post) {
  const int lane = threadIdx.x % AMD_WAVE, wave = threadIdx.x / AMD_WAVE;
  constexpr int NW = SE_MLP_TPB / AMD_WAVE;
  for (int i0 = wave; i0 < n_out; i0 += 4 * NW) {
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = lane; k < K; k += AMD_WAVE) {
      const float vk = v[k];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + q * NW;  // wave-uniform
        if (i < n_out) a[q] = __builtin_fmaf(M[(long)i * K + k], vk, a[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + q * NW;
      const float r = wave_reduce_sum(a[q]);
      if (lane == 0 && i < n_out) post(i, r);
    }
  }
}

// out[i] = post(sum_k M[k * n_out + i] * v[k]) for i < n_out: a thread per
// column i (coalesced over i), the K rows split over the KG thread groups
// that fit in the block, partials folded through red[SE_MLP_TPB] in group
// order.  v in LDS.  Ends with the block in step.
template <typename Post>
__device__ __forceinline__ void se_matTvec(const float* __restrict__ M,
                                           const float* v, int n_out, int K,
                                           float* red, Post post) {
  const int width = min(n_out, SE_MLP_TPB);
  const int KG = SE_MLP_TPB / width;
  const int kchunk = (K + KG - 1) / KG;
  const int ti = threadIdx.x % width, kg = threadIdx.x / width;
  for (int i0 = 0; i0 < n_out; i0 += width) {
    const int i = i0 + ti;
    if (kg < KG) {
      float a = 0.f;
      if (i < n_out) {
        const int k1 = min(K, (kg + 1) * kchunk);
#pragma unroll 8
        for (int k = kg * kchunk; k < k1; ++k)
          a = __builtin_fmaf(M[(long)k * n_out + i], v[k], a);
      }
      red[kg * width + ti] = a;
    }
    se_barrier();
    if (kg == 0 && i < n_out) {
      float a = 0.f;
      for (int q = 0; q < KG; ++q) a += red[q * width + ti];
      post(i, a);
    }
    se_barrier();
  }
}

// one block per image: mean, z1 = W1 mean + b1, h = hid(z1),
// s = gate(W2 h + b2); z1 is written under SiLU only
template <int HID, int GATE>
__global__ void __launch_bounds__(SE_MLP_TPB)
se_excite_kernel(const float* __restrict__ part, const float* __restrict__ w1,
                 const float* __restrict__ b1, const float* __restrict__ w2,
                 const float* __restrict__ b2, float* __restrict__ s_out,
                 float* __restrict__ mean_out, float* __restrict__ h_out,
                 float* __restrict__ z1_out, int S, int C, int Cs,
                 float inv_hw) {
  extern __shared__ float sm[];  // mean[C], h[Cs]
  float* mean = sm;
  float* h = sm + C;
  const long n = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += SE_MLP_TPB) {
    float a = 0.f;
    for (int sp = 0; sp < S; ++sp) a += part[(n * S + sp) * C + c];
    a *= inv_hw;
    mean[c] = a;
    mean_out[n * C + c] = a;
  }
  se_barrier();
  se_matvec(w1, mean, Cs, C, [&](int j, float a) {
    if (HID == SE_HID_SILU) {
      a += b1[j];
      z1_out[n * Cs + j] = a;
      a *= se_sigmoid(a);
    } else {
      a = fmaxf(a + b1[j], 0.f);
    }
    h[j] = a;
    h_out[n * Cs + j] = a;
  });
  se_barrier();
  se_matvec(w2, h, C, Cs, [&](int c, float a) {
    a += b2[c];
    s_out[n * C + c] = GATE == SE_GATE_SIGMOID
                           ? se_sigmoid(a)
                           : fminf(fmaxf(a + 3.f, 0.f), 6.f) * (1.f / 6.f);
  });
}

// one block per image: ds -> dz2 -> dz1 -> dm.  hz is h under ReLU (a
// mask) and z1 under SiLU (a slope).
template <int HID, int GATE>
__global__ void __launch_bounds__(SE_MLP_TPB)
se_excite_bwd_kernel(const float* __restrict__ ds_part,
                     const float* __restrict__ s, const float* __restrict__ hz,
                     const float* __restrict__ w1, const float* __restrict__ w2,
                     float* __restrict__ dz2_out, float* __restrict__ dz1_out,
                     float* __restrict__ dm_out, int S, int C, int Cs,
                     float inv_hw) {
  extern __shared__ float sm[];  // dz2[C], dz1[Cs], red[SE_MLP_TPB]
  float* dz2 = sm;
  float* dz1 = sm + C;
  float* red = dz1 + Cs;
  const long n = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += SE_MLP_TPB) {
    float a = 0.f;
    for (int sp = 0; sp < S; ++sp) a += ds_part[(n * S + sp) * C + c];
    const float sv = s[n * C + c];
    if (GATE == SE_GATE_SIGMOID)
      a *= sv * (1.f - sv);
    else
      a = (sv > 0.f && sv < 1.f) ? a * (1.f / 6.f) : 0.f;
    dz2[c] = a;
    dz2_out[n * C + c] = a;
  }
  se_barrier();
  // dz1 = (W2^T dz2) times hid'(z1): the mask h > 0, or SiLU's slope;
  // W2 is [C][Cs]
  se_matTvec(w2, dz2, Cs, C, red, [&](int j, float a) {
    const float q = hz[n * Cs + j];
    if (HID == SE_HID_SILU) {
      const float sg = se_sigmoid(q);
      a *= sg * __builtin_fmaf(q, 1.f - sg, 1.f);
    } else {
      a = q > 0.f ? a : 0.f;
    }
    dz1[j] = a;
    dz1_out[n * Cs + j] = a;
  });
  // dm = (W1^T dz1) / HW;  W1 is [Cs][C]
  se_matTvec(w1, dz1, C, Cs, red,
             [&](int c, float a) { dm_out[n * C + c] = a * inv_hw; });
}

// dW1[j, c] = sum_n dz1[n, j] mean[n, c];  dW2[c, j] = sum_n dz2[n, c] h[n, j]
// db1 = sum_n dz1;  db2 = sum_n dz2.  One thread per element, n ascending.
__global__ void __launch_bounds__(SE_TPB)
se_wgrad_kernel(const float* __restrict__ dz2, const float* __restrict__ dz1,
                const float* __restrict__ mean, const float* __restrict__ h,
                float* __restrict__ dw1, float* __restrict__ db1,
                float* __restrict__ dw2, float* __restrict__ db2, int N, int C,
                int Cs) {
  const long W = (long)C * Cs;
  const long total = 2 * W + Cs + C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    float a = 0.f;
    if (i < W) {
      const int j = (int)(i / C), c = (int)(i % C);
#pragma unroll 8
      for (long n = 0; n < N; ++n)
        a = __builtin_fmaf(dz1[n * Cs + j], mean[n * C + c], a);
      dw1[i] = a;
    } else if (i < 2 * W) {
      const long e = i - W;
      const int c = (int)(e / Cs), j = (int)(e % Cs);
#pragma unroll 8
      for (long n = 0; n < N; ++n)
        a = __builtin_fmaf(dz2[n * C + c], h[n * Cs + j], a);
      dw2[e] = a;
    } else if (i < 2 * W + Cs) {
      const int j = (int)(i - 2 * W);
#pragma unroll 8
      for (long n = 0; n < N; ++n) a += dz1[n * Cs + j];
      db1[j] = a;
    } else {
      const int c = (int)(i - 2 * W - Cs);
#pragma unroll 8
      for (long n = 0; n < N; ++n) a += dz2[n * C + c];
      db2[c] = a;
    }
  }
}

// flat hardswish: 16-byte packs, then a scalar tail of numel % VEC elements
template <typename T, int VEC, bool BWD>
__global__ void __launch_bounds__(AMD_TPB)
hardswish_kernel(const T* __restrict__ x, const T* __restrict__ gy,
                 T* __restrict__ out, long numel) {
  const long npack = numel / VEC;
  const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long step = (long)gridDim.x * blockDim.x;
  for (long i = t0; i < npack; i += step) {
    const Pack<T, VEC> xv = ((const Pack<T, VEC>*)x)[i];
    Pack<T, VEC> o;
    if (BWD) {
      const Pack<T, VEC> gv = ((const Pack<T, VEC>*)gy)[i];
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        o.v[k] = from_f32<T>(to_f32(gv.v[k]) * hsw_grad(to_f32(xv.v[k])));
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) o.v[k] = from_f32<T>(hsw(to_f32(xv.v[k])));
    }
    ((Pack<T, VEC>*)out)[i] = o;
  }
  for (long i = npack * VEC + t0; i < numel; i += step) {
    const float xv = to_f32(x[i]);
    out[i] = from_f32<T>(BWD ? to_f32(gy[i]) * hsw_grad(xv) : hsw(xv));
  }
}

}  // namespace

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

namespace {

struct SeGeo {
  int G, PX, RS;
};

// C/8 packs in G groups of PX <= 64 pack lanes; RS row slots fill the block
static SeGeo se_geo(long C) {
  const int P = (int)(C / 8);
  SeGeo g;
  g.G = (P + 63) / 64;
  g.PX = (P + g.G - 1) / g.G;
  g.RS = SE_TPB / g.PX;
  return g;
}

static bool is_act(const at::Tensor& t) {
  return t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf;
}

// rows [N*HW, C] of a 16-bit activation, inside the channel contract
static void se_check_rows(const char* op, const at::Tensor& x, long N,
                          long HW) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(), op,
              ": expected dense CUDA rows [N*HW, C]");
  TORCH_CHECK(is_act(x), op, ": activations must be bf16 or fp16, got ",
              x.scalar_type());
  const long C = x.size(1);
  TORCH_CHECK(C > 0 && C % 8 == 0 && C <= 4096, op,
              ": C must be a multiple of 8, at most 4096 (C = ", C, ")");
  TORCH_CHECK(N >= 0 && HW >= 1 && x.size(0) == N * HW, op, ": ", x.size(0),
              " rows for N = ", N, ", HW = ", HW);
  TORCH_CHECK(N * (long)se_geo(C).G < (1L << 31) && HW < (1L << 30), op,
              ": too many images or pixels");
  TORCH_CHECK((uintptr_t)x.const_data_ptr() % 16 == 0, op,
              ": rows must be 16-byte aligned");
}

static void se_check_same(const char* op, const at::Tensor& a,
                          const at::Tensor& x) {
  TORCH_CHECK(a.is_cuda() && a.is_contiguous() && a.sizes() == x.sizes() &&
                  a.scalar_type() == x.scalar_type() &&
                  a.device() == x.device() &&
                  (uintptr_t)a.const_data_ptr() % 16 == 0,
              op, ": dy and x must be dense rows of one shape and dtype");
}

// fp32 [d0, d1] on x's device
static void se_check_f32(const char* op, const char* name, const at::Tensor& t,
                         long d0, long d1, const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev &&
                  t.scalar_type() == at::kFloat && t.is_contiguous() &&
                  t.numel() == d0 * d1,
              op, ": ", name, " must be dense fp32 with ", d0, " x ", d1,
              " elements on ", dev);
}

static void se_check_cs(const char* op, long Cs) {
  TORCH_CHECK(Cs >= 1 && Cs <= 1024, op,
              ": squeeze width must be in [1, 1024] (Cs = ", Cs, ")");
}

// hidden_act: 0 ReLU, 1 SiLU;  gate: 0 hardsigmoid, 1 sigmoid
static void se_check_acts(const char* op, long hidden_act, long gate) {
  TORCH_CHECK((hidden_act == SE_HID_RELU || hidden_act == SE_HID_SILU) &&
                  (gate == SE_GATE_HSIG || gate == SE_GATE_SIGMOID),
              op, ": hidden_act and gate must be 0 or 1, got ", hidden_act,
              ", ", gate);
}

// calls fn with (HID, GATE) as integral constants
template <typename F>
static void se_by_acts(long hidden_act, long gate, F fn) {
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  if (hidden_act == SE_HID_SILU) {
    if (gate == SE_GATE_SIGMOID) fn(I1{}, I1{});
    else fn(I1{}, I0{});
  } else {
    if (gate == SE_GATE_SIGMOID) fn(I0{}, I1{});
    else fn(I0{}, I0{});
  }
}

// row splits of the reduce kernels: enough blocks to fill the chip, at
// least two rows per slot and split
static int se_splits(long N, long HW, const SeGeo& g, long splits) {
  if (splits > 0) {
    TORCH_CHECK(splits <= HW && splits <= 64,
                "se: splits must be at most min(HW, 64)");
    return (int)splits;
  }
  const long blocks = std::max<long>(1, N * g.G);
  const long want = (1024 + blocks - 1) / blocks;
  const long room = std::max<long>(1, HW / (2 * g.RS));
  return (int)std::min<long>(std::min(want, room), 32);
}

template <bool DY>
static at::Tensor se_reduce(const char* op, const at::Tensor& x,
                            const at::Tensor* dy, long N, long HW, bool hswish,
                            long splits) {
  se_check_rows(op, x, N, HW);
  if (DY) se_check_same(op, *dy, x);
  const long C = x.size(1);
  const SeGeo g = se_geo(C);
  const int S = se_splits(N, HW, g, splits);
  auto part = at::empty({N, (long)S, C}, x.options().dtype(at::kFloat));
  if (N == 0) return part;
  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 grid((unsigned)(N * g.G), (unsigned)S);
  auto launch = [&](auto tag, auto hs) {
    using T = decltype(tag);
    se_reduce_kernel<T, decltype(hs)::value, DY>
        <<<grid, SE_TPB, 0, stream>>>(
            (const T*)x.const_data_ptr(),
            DY ? (const T*)dy->const_data_ptr() : nullptr,
            part.data_ptr<float>(), (int)HW, (int)C, g.G, g.PX, g.RS, S);
  };
  auto by_act = [&](auto tag) {
    if (hswish)
      launch(tag, std::true_type{});
    else
      launch(tag, std::false_type{});
  };
  if (x.scalar_type() == at::kBFloat16)
    by_act(__hip_bfloat16{});
  else
    by_act(__half{});
  CHECK_CUDA_OK();
  return part;
}

template <bool BWD>
static at::Tensor se_apply(const char* op, const at::Tensor& x,
                           const at::Tensor* dy, const at::Tensor& s,
                           const at::Tensor* dm, long N, long HW,
                           bool hswish) {
  se_check_rows(op, x, N, HW);
  const long C = x.size(1);
  se_check_f32(op, "s", s, N, C, x.device());
  if (BWD) {
    se_check_same(op, *dy, x);
    se_check_f32(op, "dm", *dm, N, C, x.device());
  }
  auto out = at::empty_like(x);
  if (N == 0) return out;
  const SeGeo g = se_geo(C);
  const long chunk = (long)g.RS * SE_ROWS_PER_SLOT;
  const dim3 grid((unsigned)(N * g.G), (unsigned)((HW + chunk - 1) / chunk));
  TORCH_CHECK(grid.y <= 65535, op, ": HW too large");
  auto stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&](auto tag, auto hs) {
    using T = decltype(tag);
    se_apply_kernel<T, decltype(hs)::value, BWD>
        <<<grid, SE_TPB, 0, stream>>>(
            (const T*)x.const_data_ptr(),
            BWD ? (const T*)dy->const_data_ptr() : nullptr,
            s.data_ptr<float>(),
            BWD ? dm->data_ptr<float>() : nullptr,
            (T*)out.data_ptr(), (int)HW, (int)C, g.G, g.PX, g.RS);
  };
  auto by_act = [&](auto tag) {
    if (hswish)
      launch(tag, std::true_type{});
    else
      launch(tag, std::false_type{});
  };
  if (x.scalar_type() == at::kBFloat16)
    by_act(__hip_bfloat16{});
  else
    by_act(__half{});
  CHECK_CUDA_OK();
  return out;
}

}  // namespace

// fp32 partials [N, S, C] of sum_hw a(x); splits = 0 picks S
at::Tensor se_squeeze(at::Tensor x2d, long N, long HW, bool hswish,
                      long splits) {
  return se_reduce<false>("se_squeeze", x2d, nullptr, N, HW, hswish, splits);
}

// fp32 partials [N, S, C] of sum_hw dy * a(x)
at::Tensor se_bwd_reduce(at::Tensor dy2d, at::Tensor x2d, long N, long HW,
                         bool hswish, long splits) {
  return se_reduce<true>("se_bwd_reduce", x2d, &dy2d, N, HW, hswish, splits);
}

// {s [N, C], mean [N, C], h [N, Cs]} from the squeeze partials, and
// z1 [N, Cs] as a fourth under a SiLU hidden layer
std::vector<at::Tensor> se_excite(at::Tensor part, long HW, at::Tensor w1,
                                  at::Tensor b1, at::Tensor w2, at::Tensor b2,
                                  long hidden_act, long gate) {
  se_check_acts("se_excite", hidden_act, gate);
  TORCH_CHECK(part.is_cuda() && part.dim() == 3 && part.is_contiguous() &&
                  part.scalar_type() == at::kFloat,
              "se_excite: partials must be dense fp32 [N, S, C]");
  const long N = part.size(0), S = part.size(1), C = part.size(2);
  TORCH_CHECK(C > 0 && C % 8 == 0 && C <= 4096 && S >= 1 && HW >= 1,
              "se_excite: C must be a multiple of 8, at most 4096");
  const long Cs = w1.numel() / C;
  se_check_cs("se_excite", Cs);
  const auto dev = part.device();
  se_check_f32("se_excite", "w1", w1, Cs, C, dev);
  se_check_f32("se_excite", "b1", b1, Cs, 1, dev);
  se_check_f32("se_excite", "w2", w2, C, Cs, dev);
  se_check_f32("se_excite", "b2", b2, C, 1, dev);
  auto s = at::empty({N, C}, part.options());
  auto mean = at::empty({N, C}, part.options());
  auto h = at::empty({N, Cs}, part.options());
  const bool silu = hidden_act == SE_HID_SILU;
  at::Tensor z1;
  if (silu) z1 = at::empty({N, Cs}, part.options());
  std::vector<at::Tensor> out = {s, mean, h};
  if (silu) out.push_back(z1);
  if (N == 0) return out;
  auto stream = at::cuda::getCurrentCUDAStream();
  se_by_acts(hidden_act, gate, [&](auto hid, auto gt) {
    se_excite_kernel<decltype(hid)::value, decltype(gt)::value>
        <<<(unsigned)N, SE_MLP_TPB, (C + Cs) * sizeof(float), stream>>>(
            part.data_ptr<float>(), w1.data_ptr<float>(),
            b1.data_ptr<float>(), w2.data_ptr<float>(),
            b2.data_ptr<float>(), s.data_ptr<float>(),
            mean.data_ptr<float>(), h.data_ptr<float>(),
            silu ? z1.data_ptr<float>() : nullptr, (int)S, (int)C, (int)Cs,
            1.f / (float)HW);
  });
  CHECK_CUDA_OK();
  return out;
}

at::Tensor se_scale(at::Tensor x2d, at::Tensor s, long N, long HW,
                    bool hswish) {
  return se_apply<false>("se_scale", x2d, nullptr, s, nullptr, N, HW, hswish);
}

// {dz2 [N, C], dz1 [N, Cs], dm [N, C] (already / HW)}; h is the forward's
// h under ReLU and its z1 under SiLU
std::vector<at::Tensor> se_excite_bwd(at::Tensor ds_part, at::Tensor s,
                                      at::Tensor h, at::Tensor w1,
                                      at::Tensor w2, long HW,
                                      long hidden_act, long gate) {
  se_check_acts("se_excite_bwd", hidden_act, gate);
  TORCH_CHECK(ds_part.is_cuda() && ds_part.dim() == 3 &&
                  ds_part.is_contiguous() &&
                  ds_part.scalar_type() == at::kFloat,
              "se_excite_bwd: partials must be dense fp32 [N, S, C]");
  const long N = ds_part.size(0), S = ds_part.size(1), C = ds_part.size(2);
  TORCH_CHECK(C > 0 && C % 8 == 0 && C <= 4096 && S >= 1 && HW >= 1,
              "se_excite_bwd: C must be a multiple of 8, at most 4096");
  const long Cs = w1.numel() / C;
  se_check_cs("se_excite_bwd", Cs);
  const auto dev = ds_part.device();
  se_check_f32("se_excite_bwd", "s", s, N, C, dev);
  se_check_f32("se_excite_bwd", "h", h, N, Cs, dev);
  se_check_f32("se_excite_bwd", "w1", w1, Cs, C, dev);
  se_check_f32("se_excite_bwd", "w2", w2, C, Cs, dev);
  auto dz2 = at::empty({N, C}, ds_part.options());
  auto dz1 = at::empty({N, Cs}, ds_part.options());
  auto dm = at::empty({N, C}, ds_part.options());
  if (N == 0) return {dz2, dz1, dm};
  auto stream = at::cuda::getCurrentCUDAStream();
  se_by_acts(hidden_act, gate, [&](auto hid, auto gt) {
    se_excite_bwd_kernel<decltype(hid)::value, decltype(gt)::value>
        <<<(unsigned)N, SE_MLP_TPB, (C + Cs + SE_MLP_TPB) * sizeof(float),
           stream>>>(
            ds_part.data_ptr<float>(), s.data_ptr<float>(),
            h.data_ptr<float>(), w1.data_ptr<float>(),
            w2.data_ptr<float>(), dz2.data_ptr<float>(),
            dz1.data_ptr<float>(), dm.data_ptr<float>(), (int)S, (int)C,
            (int)Cs, 1.f / (float)HW);
  });
  CHECK_CUDA_OK();
  return {dz2, dz1, dm};
}

// {dW1 [Cs, C], db1 [Cs], dW2 [C, Cs], db2 [C]}; zeros for an empty batch
std::vector<at::Tensor> se_wgrad(at::Tensor dz2, at::Tensor dz1,
                                 at::Tensor mean, at::Tensor h) {
  TORCH_CHECK(dz2.is_cuda() && dz2.dim() == 2 && dz1.dim() == 2,
              "se_wgrad: expected dz2 [N, C], dz1 [N, Cs]");
  const long N = dz2.size(0), C = dz2.size(1), Cs = dz1.size(1);
  TORCH_CHECK(C > 0 && C % 8 == 0 && C <= 4096 && N < (1L << 31),
              "se_wgrad: C must be a multiple of 8, at most 4096");
  se_check_cs("se_wgrad", Cs);
  const auto dev = dz2.device();
  se_check_f32("se_wgrad", "dz2", dz2, N, C, dev);
  se_check_f32("se_wgrad", "dz1", dz1, N, Cs, dev);
  se_check_f32("se_wgrad", "mean", mean, N, C, dev);
  se_check_f32("se_wgrad", "h", h, N, Cs, dev);
  auto dw1 = at::zeros({Cs, C}, dz2.options());
  auto db1 = at::zeros({Cs}, dz2.options());
  auto dw2 = at::zeros({C, Cs}, dz2.options());
  auto db2 = at::zeros({C}, dz2.options());
  if (N == 0) return {dw1, db1, dw2, db2};
  auto stream = at::cuda::getCurrentCUDAStream();
  const int blocks = amd_grid(2 * C * Cs + Cs + C, SE_TPB, 65536);
  se_wgrad_kernel<<<blocks, SE_TPB, 0, stream>>>(
      dz2.data_ptr<float>(), dz1.data_ptr<float>(),
      mean.data_ptr<float>(), h.data_ptr<float>(),
      dw1.data_ptr<float>(), db1.data_ptr<float>(), dw2.data_ptr<float>(),
      db2.data_ptr<float>(), (int)N, (int)C, (int)Cs);
  CHECK_CUDA_OK();
  return {dw1, db1, dw2, db2};
}

at::Tensor se_bwd_apply(at::Tensor dy2d, at::Tensor x2d, at::Tensor s,
                        at::Tensor dm, long N, long HW, bool hswish) {
  return se_apply<true>("se_bwd_apply", x2d, &dy2d, s, &dm, N, HW, hswish);
}

namespace {

template <bool BWD>
static at::Tensor hardswish_run(const char* op, const at::Tensor& x,
                                const at::Tensor* gy) {
  TORCH_CHECK(x.is_cuda() && is_act(x), op,
              ": expected a bf16 or fp16 CUDA tensor");
  TORCH_CHECK(x.numel() == 0 || x.is_non_overlapping_and_dense(), op,
              ": x must be dense");
  if (BWD)
    TORCH_CHECK(gy->is_cuda() && gy->device() == x.device() &&
                    gy->scalar_type() == x.scalar_type() &&
                    gy->sizes() == x.sizes() && gy->strides() == x.strides() &&
                    (uintptr_t)gy->const_data_ptr() % 16 == 0,
                op, ": grad must share x's shape, dtype and memory order");
  TORCH_CHECK((uintptr_t)x.const_data_ptr() % 16 == 0, op,
              ": x must be 16-byte aligned");
  auto out = at::empty_like(x);  // same strides: the kernel walks memory flat
  const long numel = x.numel();
  if (numel == 0) return out;
  TORCH_CHECK(out.strides() == x.strides(), op, ": layout not preserved");
  auto stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&](auto tag) {
    using T = decltype(tag);
    hardswish_kernel<T, 8, BWD>
        <<<amd_grid((numel + 7) / 8), AMD_TPB, 0, stream>>>(
            (const T*)x.const_data_ptr(),
            BWD ? (const T*)gy->const_data_ptr() : nullptr,
            (T*)out.data_ptr(), numel);
  };
  if (x.scalar_type() == at::kBFloat16)
    launch(__hip_bfloat16{});
  else
    launch(__half{});
  CHECK_CUDA_OK();
  return out;
}

}  // namespace

at::Tensor hardswish_fwd(at::Tensor x) {
  return hardswish_run<false>("hardswish_fwd", x, nullptr);
}

at::Tensor hardswish_bwd(at::Tensor grad_y, at::Tensor x) {
  return hardswish_run<true>("hardswish_bwd", x, &grad_y);
}
