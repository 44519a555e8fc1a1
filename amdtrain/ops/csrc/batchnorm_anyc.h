// BatchNorm(+ReLU / ReLU6) kernels for any channel count (gfx950).
//
// batchnorm.hip's kernels take power-of-two C only: their channel-group
// decompose is a mask.  MobileNetV2's widths (24, 96, 144, 160, 192, 320,
// 384, 576, 960, 1280) are not, and a 64-bit % per 16-byte pack costs ~25
// VALU cycles.  This family takes any C with C % VEC == 0 and
// gpr = C / VEC <= 256 and pays no divide in a loop:
//
//   blockDim = gpr * floor(256 / gpr)       (gpr 3 -> 255, 18 -> 252,
//                                            72 -> 216, 120 -> 240, 160 -> 160)
//
// The block size, and with it the grid stride, is a multiple of gpr, so a
// thread's channel group is threadIdx.x % gpr — one 32-bit modulo before the
// loop — and never changes.  Its coefficients live in registers, as in the
// REGC variants.  The idle lanes of the last wave (at most 96 of 256, at
// gpr 160) are the price.
//
// Same stages as the power-of-two family, and the same collapse / finalize
// kernels behind them:
//   reduce:     rows split across blocks, blockDim / gpr phases per block
//               folded through LDS in ascending order, per-block partials
//               [nparts][2C].  No atomics; two runs give the same bits.
//   apply:      y = act(scale*x + shift (+ z)), two 16-byte streams in
//               flight per thread.
//   bwd reduce: sum(ghat), sum(ghat*xhat) with ghat = go masked by the
//               activation, recomputed from the forward's scale / shift
//               (the MASK 2 idea: no y read, no mask tensor).
//   bwd apply:  gx = A*ghat + B*x + D with the same recomputed mask.
//
// ReLU6 passes the gradient where 0 < v < 6.  Every kernel here forms the
// pre-activation v through bn_anyc_v, a single explicit FMA: were it left
// to the compiler's contraction, the forward, the backward reduce and the
// backward apply could round v differently and disagree about an element
// at a clamp boundary.
#pragma once

#include "common.h"

constexpr int BN_ACT_NONE = 0, BN_ACT_RELU = 1, BN_ACT_RELU6 = 2;

__device__ __forceinline__ float bn_anyc_v(float sc, float xe, float sh) {
  return __builtin_fmaf(sc, xe, sh);
}

// does the activation pass the gradient at pre-activation v?
template <int ACT>
__device__ __forceinline__ bool bn_anyc_pass(float v) {
  if (ACT == BN_ACT_RELU) return v > 0.f;
  if (ACT == BN_ACT_RELU6) return v > 0.f && v < 6.f;
  return true;
}

template <int ACT>
__device__ __forceinline__ float bn_anyc_act(float v) {
  if (ACT == BN_ACT_RELU) return fmaxf(v, 0.f);
  if (ACT == BN_ACT_RELU6) return fminf(fmaxf(v, 0.f), 6.f);
  return v;
}

// threads per block: the largest multiple of gpr that fits AMD_TPB
static inline int bn_anyc_block(int gpr) { return gpr * (AMD_TPB / gpr); }

// ---- reduce: per-channel (a, b) sums over rows ----------------------------
// fwd (BWD=false): a = x, b = x^2
// bwd (BWD=true):  a = ghat, b = ghat * xhat,
//                  ghat = go where the activation passes, else 0
// Two rows in flight per thread; they are accumulated in row order, so the
// sums are those of the one-row-at-a-time loop.
template <typename T, int VEC, bool BWD, int ACT>
__global__ void __launch_bounds__(AMD_TPB)
bn_anyc_reduce_kernel(const T* __restrict__ x, const T* __restrict__ go,
                      const float* __restrict__ mean,
                      const float* __restrict__ invstd,
                      const float* __restrict__ scale,
                      const float* __restrict__ shift,
                      float* __restrict__ out, long R, int C) {
  static_assert(BWD || ACT == BN_ACT_NONE, "the forward sums take no mask");
  const int t = threadIdx.x;
  const int gpr = C / VEC;             // channel groups per row
  const int rstep = blockDim.x / gpr;  // phases: rows a block takes at once
  const int phase = t / gpr;           // decoded once
  const int gc = t - phase * gpr;
  const int c0 = gc * VEC;
  const long rows_per_block = (R + gridDim.x - 1) / gridDim.x;
  const long r0 = blockIdx.x * rows_per_block;
  const long r1 = min(r0 + rows_per_block, R);

  float sa[VEC], sb[VEC], mk[VEC], ik[VEC], sck[VEC], shk[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    sa[k] = sb[k] = 0.f;
    if (BWD) {
      mk[k] = mean[c0 + k];
      ik[k] = invstd[c0 + k];
      if (ACT != BN_ACT_NONE) {
        sck[k] = scale[c0 + k];
        shk[k] = shift[c0 + k];
      }
    }
  }
  auto accumulate = [&](const Pack<T, VEC>& xv, const Pack<T, VEC>& gv) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float xe = to_f32(xv.v[k]);
      if (BWD) {
        float ge = to_f32(gv.v[k]);
        if (ACT != BN_ACT_NONE &&
            !bn_anyc_pass<ACT>(bn_anyc_v(sck[k], xe, shk[k])))
          ge = 0.f;
        sa[k] += ge;
        sb[k] += ge * (xe - mk[k]) * ik[k];
      } else {
        sa[k] += xe;
        sb[k] += xe * xe;
      }
    }
  };
  const long rstep2 = 2L * rstep;
  for (long r = r0 + phase; r < r1; r += rstep2) {
    const bool has2 = r + rstep < r1;
    const long rr = has2 ? r + rstep : r;  // clamp: loads stay in bounds
    const long base = r * C + c0, base2 = rr * C + c0;
    Pack<T, VEC> xv = *(const Pack<T, VEC>*)(x + base);
    Pack<T, VEC> xv2 = *(const Pack<T, VEC>*)(x + base2);
    Pack<T, VEC> gv, gv2;
    if (BWD) {
      gv = *(const Pack<T, VEC>*)(go + base);
      gv2 = *(const Pack<T, VEC>*)(go + base2);
    }
    accumulate(xv, gv);
    if (has2) accumulate(xv2, gv2);
  }
  // LDS fold across phases into phase 0, ascending, one array at a time
  __shared__ float lds[AMD_TPB * VEC];
  auto fold = [&](float(&s)[VEC]) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) lds[t * VEC + k] = s[k];
    __syncthreads();
    if (phase == 0) {
      for (int ph = 1; ph < rstep; ++ph)
#pragma unroll
        for (int k = 0; k < VEC; ++k) s[k] += lds[(ph * gpr + gc) * VEC + k];
    }
    __syncthreads();
  };
  fold(sa);
  fold(sb);
  if (phase == 0) {
    float* part = out + (long)blockIdx.x * 2 * C;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      part[c0 + k] = sa[k];
      part[C + c0 + k] = sb[k];
    }
  }
}

// ---- apply: y = act(scale*x + shift (+ z)) --------------------------------
template <typename T, int VEC, int ACT, bool HAS_ADD>
__global__ void __launch_bounds__(AMD_TPB)
bn_anyc_apply_kernel(const T* __restrict__ x, const T* __restrict__ z,
                     T* __restrict__ y, const float* __restrict__ scale,
                     const float* __restrict__ shift, long total_vec, int C) {
  const int gpr = C / VEC;
  // blockDim is a multiple of gpr, so is the grid stride: i % gpr is
  // threadIdx.x % gpr for every i this thread visits
  const int c0 = (int)(threadIdx.x % (unsigned)gpr) * VEC;
  const long stride = (long)gridDim.x * blockDim.x;
  float rs[VEC], rb[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    rs[k] = scale[c0 + k];
    rb[k] = shift[c0 + k];
  }
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total_vec;
       i += 2 * stride) {
    const bool has2 = i + stride < total_vec;
    const long i2 = has2 ? i + stride : i;  // clamp: loads stay in bounds
    Pack<T, VEC> xv = *(const Pack<T, VEC>*)(x + i * VEC);
    Pack<T, VEC> xv2 = *(const Pack<T, VEC>*)(x + i2 * VEC);
    Pack<T, VEC> zv, zv2;
    if (HAS_ADD) {
      zv = *(const Pack<T, VEC>*)(z + i * VEC);
      zv2 = *(const Pack<T, VEC>*)(z + i2 * VEC);
    }
    Pack<T, VEC> yv, yv2;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float v = bn_anyc_v(rs[k], to_f32(xv.v[k]), rb[k]);
      float v2 = bn_anyc_v(rs[k], to_f32(xv2.v[k]), rb[k]);
      if (HAS_ADD) {
        v += to_f32(zv.v[k]);
        v2 += to_f32(zv2.v[k]);
      }
      yv.v[k] = from_f32<T>(bn_anyc_act<ACT>(v));
      yv2.v[k] = from_f32<T>(bn_anyc_act<ACT>(v2));
    }
    *(Pack<T, VEC>*)(y + i * VEC) = yv;
    if (has2) *(Pack<T, VEC>*)(y + i2 * VEC) = yv2;
  }
}

// ---- bwd apply: gx = A*ghat + B*x + D -------------------------------------
// ghat is go under the activation's mask, recomputed exactly as the reduce
// did (bn_anyc_v); the contraction of the gx expression is spelled out so
// that it does not depend on the variant either.
template <typename T, int VEC, int ACT>
__global__ void __launch_bounds__(AMD_TPB)
bn_anyc_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ go,
                         T* __restrict__ gx, const float* __restrict__ A,
                         const float* __restrict__ Bc,
                         const float* __restrict__ Dc,
                         const float* __restrict__ scale,
                         const float* __restrict__ shift, long total_vec,
                         int C) {
  const int gpr = C / VEC;
  const int c0 = (int)(threadIdx.x % (unsigned)gpr) * VEC;
  const long stride = (long)gridDim.x * blockDim.x;
  float ra[VEC], rb[VEC], rd[VEC], rsc[VEC], rsh[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    ra[k] = A[c0 + k];
    rb[k] = Bc[c0 + k];
    rd[k] = Dc[c0 + k];
    if (ACT != BN_ACT_NONE) {
      rsc[k] = scale[c0 + k];
      rsh[k] = shift[c0 + k];
    }
  }
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total_vec;
       i += 2 * stride) {
    const bool has2 = i + stride < total_vec;
    const long i2 = has2 ? i + stride : i;  // clamp: loads stay in bounds
    Pack<T, VEC> xv = *(const Pack<T, VEC>*)(x + i * VEC);
    Pack<T, VEC> gv = *(const Pack<T, VEC>*)(go + i * VEC);
    Pack<T, VEC> xv2 = *(const Pack<T, VEC>*)(x + i2 * VEC);
    Pack<T, VEC> gv2 = *(const Pack<T, VEC>*)(go + i2 * VEC);
    Pack<T, VEC> out, out2;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float xe = to_f32(xv.v[k]), xe2 = to_f32(xv2.v[k]);
      float ge = to_f32(gv.v[k]), ge2 = to_f32(gv2.v[k]);
      if (ACT != BN_ACT_NONE) {
        if (!bn_anyc_pass<ACT>(bn_anyc_v(rsc[k], xe, rsh[k]))) ge = 0.f;
        if (!bn_anyc_pass<ACT>(bn_anyc_v(rsc[k], xe2, rsh[k]))) ge2 = 0.f;
      }
      out.v[k] = from_f32<T>(__builtin_fmaf(ra[k], ge, rb[k] * xe) + rd[k]);
      out2.v[k] =
          from_f32<T>(__builtin_fmaf(ra[k], ge2, rb[k] * xe2) + rd[k]);
    }
    *(Pack<T, VEC>*)(gx + i * VEC) = out;
    if (has2) *(Pack<T, VEC>*)(gx + i2 * VEC) = out2;
  }
}
