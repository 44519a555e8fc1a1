// Fused NHWC BatchNorm(+residual add)(+ReLU) forward/backward for gfx950.
//
// The reference runs conv -> BN -> ReLU as separate cuDNN/elementwise
// launches (53 BN layers in ResNet-50; SURVEY §2c "fuse into conv epilogue").
// On MI355X the BN+add+ReLU tail is pure HBM traffic, so it runs as:
//   fwd train: [reduce: per-channel sum/sumsq, fp32]  ->
//              [finalize: mean/invstd + running-stat update + scale/shift] ->
//              [apply: y = scale*x + shift (+z), relu — one pass]
//   bwd:       [reduce: per-channel sum(ghat), sum(ghat*xhat)] ->
//              [finalize: grad_w/grad_b + per-channel A,B,D coefficients] ->
//              [apply: gx = A*ghat + B*x + D (+ optional ghat out)]
//
// Reduction strategy (CDNA4): rows R = N*H*W of C contiguous channels;
// 16 B/lane vector loads; each thread owns a FIXED channel-group so partial
// sums live in registers (no LDS atomics in the hot loop), then one LDS
// phase-reduction per block and one global atomicAdd per channel per block.
// All ResNet channel counts (64..2048) hit this register path.
#include "common.h"

namespace {

// ---- reduction: per-channel (a, b) sums over rows -------------------------
// fwd (BWD=false): a = x, b = x^2
// bwd (BWD=true):  a = ghat, b = ghat * xhat, where
//   MASK 0: ghat = go (no relu / pre-masked input)
//   MASK 1: ghat = go * (y > 0)                  (block-tail BN: y has addend)
//   MASK 2: ghat = go * (scale*x + shift > 0)    (inner BN: skip the y read)
//   MASK 3: ghat = go * fwd-bitmask              (block-tail: 1/16 the bytes
//                                                 of the y read; y = the
//                                                 mask byte stream here)
// WG: additionally materialize ghat (consumed by the mask-free bwd apply and
// as the residual addend gradient) — turns reduce into 3r+1w so apply drops
// to 2r+1w (guide: every pass here is an HBM-bound R x C stream).
// GO2: go is the SUM of two operands (goB = the rerouted residual
// shortcut gradient, see ResidualGradTap) — added in fp32 here so the
// eager CUDAFunctor_add pass disappears; the sum is baked into ghat_out.
// DUAL (downsample block tail): the shortcut is a second BN over x_d whose
// grad_out IS ghat, so its two sums ride in the same row loop.  They are
// taken over the ROUNDED ghat (what the separate pass read back from
// memory), hence four sums per channel: with GO2 the fp32 go+go2 and its
// rounding differ.  Same grid / row partition / fold order as two passes.
template <typename T>
struct BNDualSide {
  const T* x = nullptr;
  const float* mean = nullptr;
  const float* invstd = nullptr;
  float* out = nullptr;
};

template <typename T, int VEC, bool BWD, int MASK, bool WG, bool GO2,
          bool DUAL = false>
__global__ void __launch_bounds__(AMD_TPB)
bn_reduce_kernel(const T* __restrict__ x, const T* __restrict__ go,
                 const T* __restrict__ goB, const T* __restrict__ y,
                 const float* __restrict__ mean,
                 const float* __restrict__ invstd,
                 const float* __restrict__ scale,
                 const float* __restrict__ shift, T* __restrict__ ghat_out,
                 float* __restrict__ out, long R, int C,
                 BNDualSide<T> ds = {}) {
  static_assert(!DUAL || (BWD && WG), "DUAL rides the ghat-writing bwd pass");
  const int t = threadIdx.x;
  const int gpr = C / VEC;  // channel-groups per row
  // rows are split across blocks
  const long rows_per_block = (R + gridDim.x - 1) / gridDim.x;
  const long r0 = blockIdx.x * rows_per_block;
  const long r1 = min(r0 + rows_per_block, R);

  if (gpr <= AMD_TPB) {
    // thread's channel group is fixed: gc = t % gpr; phase = t / gpr
    const int gc = t % gpr;
    const int phase = t / gpr;
    const int rstep = AMD_TPB / gpr;
    const int c0 = gc * VEC;
    float sa[VEC], sb[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) sa[k] = sb[k] = 0.f;
    float mk[VEC], ik[VEC], sck[VEC], shk[VEC];
    float sda[VEC], sdb[VEC], mdk[VEC], idk[VEC];  // DUAL: downsample BN
    if (BWD) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        mk[k] = mean[c0 + k];
        ik[k] = invstd[c0 + k];
        if (MASK == 2) {
          sck[k] = scale[c0 + k];
          shk[k] = shift[c0 + k];
        }
        if (DUAL) {
          sda[k] = sdb[k] = 0.f;
          mdk[k] = ds.mean[c0 + k];
          idk[k] = ds.invstd[c0 + k];
        }
      }
    }
    for (long r = r0 + phase; r < r1; r += rstep) {
      const long base = r * C + c0;
      Pack<T, VEC> xv = *(const Pack<T, VEC>*)(x + base);
      Pack<T, VEC> gv, gv2, yv, gh, dv;
      unsigned int mbits = 0;
      if (BWD) {
        gv = *(const Pack<T, VEC>*)(go + base);
        if (DUAL) dv = *(const Pack<T, VEC>*)(ds.x + base);
        if (GO2) gv2 = *(const Pack<T, VEC>*)(goB + base);
        if (MASK == 1) yv = *(const Pack<T, VEC>*)(y + base);
        if (MASK == 3)
          mbits = ((const unsigned char*)y)[base / VEC];
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float xe = to_f32(xv.v[k]);
        if (BWD) {
          float ge = to_f32(gv.v[k]);
          if (GO2) ge += to_f32(gv2.v[k]);
          if (MASK == 1 && to_f32(yv.v[k]) <= 0.f) ge = 0.f;
          if (MASK == 2 && sck[k] * xe + shk[k] <= 0.f) ge = 0.f;
          if (MASK == 3 && !(mbits & (1u << k))) ge = 0.f;
          sa[k] += ge;
          sb[k] += ge * (xe - mk[k]) * ik[k];
          if (WG) gh.v[k] = from_f32<T>(ge);
          if (DUAL) {
            const float gr = to_f32(gh.v[k]);
            sda[k] += gr;
            sdb[k] += gr * (to_f32(dv.v[k]) - mdk[k]) * idk[k];
          }
        } else {
          sa[k] += xe;
          sb[k] += xe * xe;
        }
      }
      if (BWD && WG) *(Pack<T, VEC>*)(ghat_out + base) = gh;
    }
    // LDS reduce across phases into phase 0, one sum array at a time
    __shared__ float lds[AMD_TPB * VEC];
    auto fold = [&](float(&s)[VEC]) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) lds[t * VEC + k] = s[k];
      __syncthreads();
      if (phase == 0) {
        for (int ph = 1; ph < rstep; ++ph)
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            s[k] += lds[(ph * gpr + gc) * VEC + k];
      }
      __syncthreads();
    };
    fold(sa);
    fold(sb);
    if (DUAL) {
      fold(sda);
      fold(sdb);
    }
    if (phase == 0) {
      // per-block partials (no global atomics: 1024-way same-line atomic
      // contention was ~24 ms/step — two-stage instead)
      float* part = out + (long)blockIdx.x * 2 * C;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        part[c0 + k] = sa[k];
        part[C + c0 + k] = sb[k];
      }
      if (DUAL) {
        float* partd = ds.out + (long)blockIdx.x * 2 * C;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          partd[c0 + k] = sda[k];
          partd[C + c0 + k] = sdb[k];
        }
      }
    }
  } else {
    // wide-C: each thread owns up to 2 channel-groups, no cross-thread reduce
    // (DUAL is register-path only; the host entry rejects wide-C)
    const int cpt = gpr / AMD_TPB;  // host guarantees <= 2 and divisible
    float sa[2][VEC], sb[2][VEC];
    float mk[2][VEC], ik[2][VEC], sck[2][VEC], shk[2][VEC];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        sa[j][k] = sb[j][k] = 0.f;
        if (BWD && j < cpt) {
          mk[j][k] = mean[(t + j * AMD_TPB) * VEC + k];
          ik[j][k] = invstd[(t + j * AMD_TPB) * VEC + k];
          if (MASK == 2) {
            sck[j][k] = scale[(t + j * AMD_TPB) * VEC + k];
            shk[j][k] = shift[(t + j * AMD_TPB) * VEC + k];
          }
        }
      }
    for (long r = r0; r < r1; ++r) {
      for (int j = 0; j < cpt; ++j) {
        const int c0 = (t + j * AMD_TPB) * VEC;
        const long base = r * C + c0;
        Pack<T, VEC> xv = *(const Pack<T, VEC>*)(x + base);
        Pack<T, VEC> gv, gv2, yv, gh;
        unsigned int mbits = 0;
        if (BWD) {
          gv = *(const Pack<T, VEC>*)(go + base);
          if (GO2) gv2 = *(const Pack<T, VEC>*)(goB + base);
          if (MASK == 1) yv = *(const Pack<T, VEC>*)(y + base);
          if (MASK == 3)
            mbits = ((const unsigned char*)y)[base / VEC];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          float xe = to_f32(xv.v[k]);
          if (BWD) {
            float ge = to_f32(gv.v[k]);
            if (GO2) ge += to_f32(gv2.v[k]);
            if (MASK == 1 && to_f32(yv.v[k]) <= 0.f) ge = 0.f;
            if (MASK == 2 && sck[j][k] * xe + shk[j][k] <= 0.f) ge = 0.f;
            if (MASK == 3 && !(mbits & (1u << k))) ge = 0.f;
            sa[j][k] += ge;
            sb[j][k] += ge * (xe - mk[j][k]) * ik[j][k];
            if (WG) gh.v[k] = from_f32<T>(ge);
          } else {
            sa[j][k] += xe;
            sb[j][k] += xe * xe;
          }
        }
        if (BWD && WG) *(Pack<T, VEC>*)(ghat_out + base) = gh;
      }
    }
    float* part = out + (long)blockIdx.x * 2 * C;
    for (int j = 0; j < cpt; ++j) {
      const int c0 = (t + j * AMD_TPB) * VEC;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        part[c0 + k] = sa[j][k];
        part[C + c0 + k] = sb[j][k];
      }
    }
  }
}

// collapse [nparts][2C] partials to [NCOLLAPSE][2C] (coalesced, parallel) —
// the finalize kernels then loop only NCOLLAPSE rows (a single small block
// looping 512 strided rows measured 125 us; this two-level scheme is ~2 us)
constexpr int BN_COLLAPSE = 32;

static inline int bn_collapse_slots(int nparts) {
  // more fold-slots for large partial sets (conv-stats partials reach
  // ~12k rows at layer1 b512; 32 slots left the collapse latency-bound)
  return nparts >= 2048 ? 4 * BN_COLLAPSE : BN_COLLAPSE;
}

__global__ void bn_collapse_partials_kernel(const float* __restrict__ in,
                                            float* __restrict__ out,
                                            int nparts, int twoC, int slots) {
  // grid: slots x ceil(twoC/256); block b sums rows [b].. step slots
  const int slot = blockIdx.x % slots;
  const int cblk = blockIdx.x / slots;
  const int c = cblk * AMD_TPB + threadIdx.x;
  if (c >= twoC) return;
  float acc = 0.f;
  for (int p = slot; p < nparts; p += slots)
    acc += in[(long)p * twoC + c];
  out[(long)slot * twoC + c] = acc;
}

// ---- finalize (train): stats + running update + scale/shift ---------------
// 4 slot-threads per channel (the single-thread row loop over up to 128
// collapse slots was ~20 us latency-bound x 106 calls/step)
__global__ void bn_finalize_train_kernel(
    const float* __restrict__ partials, int nparts,
    const float* __restrict__ w,
    const float* __restrict__ b, float* __restrict__ rm,
    float* __restrict__ rv, float* __restrict__ mean,
    float* __restrict__ invstd, float* __restrict__ scale,
    float* __restrict__ shift, long R, int C, float momentum, float eps) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int sl = threadIdx.x >> 6;  // 0..3
  float s1 = 0.f, s2 = 0.f;
  if (c < C)
    for (int p = sl; p < nparts; p += 4) {
      s1 += partials[(long)p * 2 * C + c];
      s2 += partials[(long)p * 2 * C + C + c];
    }
  __shared__ float red[2][4][64];
  red[0][sl][threadIdx.x & 63] = s1;
  red[1][sl][threadIdx.x & 63] = s2;
  __syncthreads();
  if (sl != 0 || c >= C) return;
  s1 += red[0][1][threadIdx.x] + red[0][2][threadIdx.x] +
        red[0][3][threadIdx.x];
  s2 += red[1][1][threadIdx.x] + red[1][2][threadIdx.x] +
        red[1][3][threadIdx.x];
  float m = s1 / R;
  float var = fmaxf(s2 / R - m * m, 0.f);
  float is = rsqrtf(var + eps);
  mean[c] = m;
  invstd[c] = is;
  // torch semantics: running_var uses the unbiased estimator
  float unbiased = R > 1 ? var * (float)R / (float)(R - 1) : var;
  rm[c] = (1.f - momentum) * rm[c] + momentum * m;
  rv[c] = (1.f - momentum) * rv[c] + momentum * unbiased;
  float sc = w[c] * is;
  scale[c] = sc;
  shift[c] = b[c] - m * sc;
}

__global__ void bn_finalize_eval_kernel(
    const float* __restrict__ w, const float* __restrict__ b,
    const float* __restrict__ rm, const float* __restrict__ rv,
    float* __restrict__ scale, float* __restrict__ shift, int C, float eps) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float is = rsqrtf(rv[c] + eps);
  float sc = w[c] * is;
  scale[c] = sc;
  shift[c] = b[c] - rm[c] * sc;
}

// ---- apply: y = scale*x + shift (+z), relu --------------------------------
// 2-way unrolled (two independent 16 B streams in flight per thread) with a
// pow2 fast path for the channel-group decompose (all ResNet C are pow2;
// the 64-bit % was ~25 VALU cycles per 16 B).
// DUAL (downsample block tail): z is the RAW downsample-conv output and the
// addend is its own BN, T(scale_d*z + shift_d) — rounded through the
// activation dtype exactly as the materialized intermediate was, so the
// separate downsample apply (1r+1w) disappears without changing a bit.
// Its four coefficient sets stay in registers (measured +0.7% end to end
// over [4][C] in LDS).
template <typename T, int VEC, bool RELU, bool HAS_ADD, bool POW2,
          bool DUAL = false>
__global__ void __launch_bounds__(AMD_TPB)
bn_apply_kernel(const T* __restrict__ x, const T* __restrict__ z,
                T* __restrict__ y, unsigned char* __restrict__ mask,
                const float* __restrict__ scale,
                const float* __restrict__ shift, long total_vec, int C,
                const float* __restrict__ scale_d = nullptr,
                const float* __restrict__ shift_d = nullptr) {
  static_assert(!DUAL || (HAS_ADD && POW2), "DUAL normalizes the addend");
  extern __shared__ float sm[];  // [2][C] (unused by DUAL)
  const int gpr = C / VEC;
  const long stride = (long)gridDim.x * blockDim.x;
  // DUAL: the host admits only pow2 C/VEC <= blockDim, so the grid stride
  // is a multiple of C/VEC and a thread keeps ONE channel group for the
  // whole loop — its four coefficient sets live in registers, not LDS.
  float rs[VEC], rb[VEC], rsd[VEC], rbd[VEC];
  if (DUAL) {
    const int cf =
        (int)(((long)blockIdx.x * blockDim.x + threadIdx.x) & (gpr - 1)) * VEC;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      rs[k] = scale[cf + k];
      rb[k] = shift[cf + k];
      rsd[k] = scale_d[cf + k];
      rbd[k] = shift_d[cf + k];
    }
  } else {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      sm[c] = scale[c];
      sm[C + c] = shift[c];
    }
    __syncthreads();
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
    const int c0 = (int)(POW2 ? (i & (gpr - 1)) : (i % gpr)) * VEC;
    const int c02 = (int)(POW2 ? (i2 & (gpr - 1)) : (i2 % gpr)) * VEC;
    Pack<T, VEC> yv, yv2;
    unsigned int mb = 0, mb2 = 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float v = DUAL ? rs[k] * to_f32(xv.v[k]) + rb[k]
                     : sm[c0 + k] * to_f32(xv.v[k]) + sm[C + c0 + k];
      if (HAS_ADD) {
        float ze = to_f32(zv.v[k]);
        if (DUAL) ze = to_f32(from_f32<T>(rsd[k] * ze + rbd[k]));
        v += ze;
      }
      if (RELU) {
        if (mask != nullptr && v > 0.f) mb |= 1u << k;
        v = fmaxf(v, 0.f);
      }
      yv.v[k] = from_f32<T>(v);
      float v2 = DUAL ? rs[k] * to_f32(xv2.v[k]) + rb[k]
                      : sm[c02 + k] * to_f32(xv2.v[k]) + sm[C + c02 + k];
      if (HAS_ADD) {
        float ze2 = to_f32(zv2.v[k]);
        if (DUAL) ze2 = to_f32(from_f32<T>(rsd[k] * ze2 + rbd[k]));
        v2 += ze2;
      }
      if (RELU) {
        if (mask != nullptr && v2 > 0.f) mb2 |= 1u << k;
        v2 = fmaxf(v2, 0.f);
      }
      yv2.v[k] = from_f32<T>(v2);
    }
    *(Pack<T, VEC>*)(y + i * VEC) = yv;
    if (has2) *(Pack<T, VEC>*)(y + i2 * VEC) = yv2;
    if (RELU && mask != nullptr) {
      mask[i] = (unsigned char)mb;  // one byte per VEC-pack
      if (has2) mask[i2] = (unsigned char)mb2;
    }
  }
}

// ---- bwd finalize: grad_w/grad_b + A,B,D coefficients ---------------------
__global__ void bn_bwd_finalize_kernel(
    const float* __restrict__ partials, int nparts,
    const float* __restrict__ w, const float* __restrict__ mean,
    const float* __restrict__ invstd, float* __restrict__ gw,
    float* __restrict__ gb, float* __restrict__ A, float* __restrict__ Bc,
    float* __restrict__ Dc, long R, int C) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int sl = threadIdx.x >> 6;
  float sg = 0.f, sgx = 0.f;
  if (c < C)
    for (int p = sl; p < nparts; p += 4) {
      sg += partials[(long)p * 2 * C + c];
      sgx += partials[(long)p * 2 * C + C + c];
    }
  __shared__ float red[2][4][64];
  red[0][sl][threadIdx.x & 63] = sg;
  red[1][sl][threadIdx.x & 63] = sgx;
  __syncthreads();
  if (sl != 0 || c >= C) return;
  sg += red[0][1][threadIdx.x] + red[0][2][threadIdx.x] +
        red[0][3][threadIdx.x];
  sgx += red[1][1][threadIdx.x] + red[1][2][threadIdx.x] +
         red[1][3][threadIdx.x];
  gb[c] = sg;
  gw[c] = sgx;
  float a = w[c] * invstd[c];
  float bcoef = -a * invstd[c] * sgx / R;
  A[c] = a;
  Bc[c] = bcoef;
  Dc[c] = -a * sg / R - bcoef * mean[c];
}

// ---- bwd apply: gx = A*ghat + B*x + D -------------------------------------
// 2-way unrolled + pow2 fast path (see bn_apply_kernel).  MASK 0: go is
// already masked (the reduce pass wrote ghat, or no relu) — no y read at
// all; MASK 2: relu mask recomputed from the forward's scale/shift
// (y = relu(scale*x+shift) so y>0 <=> scale*x+shift>0) — also no y read.
// DUAL (downsample block tail): the shortcut BN shares ghat, so one pass
// reads x, x_d, ghat and writes gx and gx_d, each with its own A/B/D —
// the downsample BN's separate apply no longer re-reads ghat.
template <typename T>
struct BNDualBwdSide {
  const T* x = nullptr;
  T* gx = nullptr;
  const float* A = nullptr;
  const float* Bc = nullptr;
  const float* Dc = nullptr;
};

template <typename T, int VEC, int MASK, bool WRITE_GHAT, bool POW2,
          bool DUAL = false>
__global__ void __launch_bounds__(AMD_TPB)
bn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ go,
                    T* __restrict__ gx,
                    T* __restrict__ ghat_out, const float* __restrict__ A,
                    const float* __restrict__ Bc, const float* __restrict__ Dc,
                    const float* __restrict__ scale,
                    const float* __restrict__ shift, long total_vec, int C,
                    BNDualBwdSide<T> ds = {}) {
  static_assert(!DUAL || (MASK == 0 && POW2 && !WRITE_GHAT),
                "DUAL consumes the materialized ghat");
  const int gpr = C / VEC;
  const long stride = (long)gridDim.x * blockDim.x;
  if (DUAL) {
    // The host admits only pow2 C/VEC <= blockDim here, so the grid stride
    // is a multiple of C/VEC and a thread keeps ONE channel group for the
    // whole loop: all six coefficient sets live in registers (six [C]
    // arrays in LDS would be 48 KB/block at C=2048 — 3 blocks/CU).
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c0 = (int)(i0 & (gpr - 1)) * VEC;
    float a3[VEC], b3[VEC], d3[VEC], ad[VEC], bd[VEC], dd[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      a3[k] = A[c0 + k];
      b3[k] = Bc[c0 + k];
      d3[k] = Dc[c0 + k];
      ad[k] = ds.A[c0 + k];
      bd[k] = ds.Bc[c0 + k];
      dd[k] = ds.Dc[c0 + k];
    }
    for (long i = i0; i < total_vec; i += 2 * stride) {
      const bool has2 = i + stride < total_vec;
      const long i2 = has2 ? i + stride : i;  // clamp: loads stay in bounds
      Pack<T, VEC> xv = *(const Pack<T, VEC>*)(x + i * VEC);
      Pack<T, VEC> dv = *(const Pack<T, VEC>*)(ds.x + i * VEC);
      Pack<T, VEC> gv = *(const Pack<T, VEC>*)(go + i * VEC);
      Pack<T, VEC> xv2 = *(const Pack<T, VEC>*)(x + i2 * VEC);
      Pack<T, VEC> dv2 = *(const Pack<T, VEC>*)(ds.x + i2 * VEC);
      Pack<T, VEC> gv2 = *(const Pack<T, VEC>*)(go + i2 * VEC);
      Pack<T, VEC> out, dout, out2, dout2;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float ge = to_f32(gv.v[k]);
        float v = a3[k] * ge + b3[k] * to_f32(xv.v[k]) + d3[k];
        out.v[k] = from_f32<T>(v);
        float w = ad[k] * ge + bd[k] * to_f32(dv.v[k]) + dd[k];
        dout.v[k] = from_f32<T>(w);
        float ge2 = to_f32(gv2.v[k]);
        float v2 = a3[k] * ge2 + b3[k] * to_f32(xv2.v[k]) + d3[k];
        out2.v[k] = from_f32<T>(v2);
        float w2 = ad[k] * ge2 + bd[k] * to_f32(dv2.v[k]) + dd[k];
        dout2.v[k] = from_f32<T>(w2);
      }
      *(Pack<T, VEC>*)(gx + i * VEC) = out;
      *(Pack<T, VEC>*)(ds.gx + i * VEC) = dout;
      if (has2) {
        *(Pack<T, VEC>*)(gx + i2 * VEC) = out2;
        *(Pack<T, VEC>*)(ds.gx + i2 * VEC) = dout2;
      }
    }
    return;
  }
  extern __shared__ float sm[];  // [3][C] (+[2][C] for MASK 2)
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    sm[c] = A[c];
    sm[C + c] = Bc[c];
    sm[2 * C + c] = Dc[c];
    if (MASK == 2) {
      sm[3 * C + c] = scale[c];
      sm[4 * C + c] = shift[c];
    }
  }
  __syncthreads();
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total_vec;
       i += 2 * stride) {
    const bool has2 = i + stride < total_vec;
    const long i2 = has2 ? i + stride : i;  // clamp: loads stay in bounds
    Pack<T, VEC> xv = *(const Pack<T, VEC>*)(x + i * VEC);
    Pack<T, VEC> gv = *(const Pack<T, VEC>*)(go + i * VEC);
    Pack<T, VEC> xv2 = *(const Pack<T, VEC>*)(x + i2 * VEC);
    Pack<T, VEC> gv2 = *(const Pack<T, VEC>*)(go + i2 * VEC);
    const int c0 = (int)(POW2 ? (i & (gpr - 1)) : (i % gpr)) * VEC;
    const int c02 = (int)(POW2 ? (i2 & (gpr - 1)) : (i2 % gpr)) * VEC;
    Pack<T, VEC> out, gh, out2, gh2;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float xe = to_f32(xv.v[k]);
      float ge = to_f32(gv.v[k]);
      if (MASK == 2 && sm[3 * C + c0 + k] * xe + sm[4 * C + c0 + k] <= 0.f)
        ge = 0.f;
      float v = sm[c0 + k] * ge + sm[C + c0 + k] * xe + sm[2 * C + c0 + k];
      out.v[k] = from_f32<T>(v);
      if (WRITE_GHAT) gh.v[k] = from_f32<T>(ge);
      float xe2 = to_f32(xv2.v[k]);
      float ge2 = to_f32(gv2.v[k]);
      if (MASK == 2 && sm[3 * C + c02 + k] * xe2 + sm[4 * C + c02 + k] <= 0.f)
        ge2 = 0.f;
      float v2 = sm[c02 + k] * ge2 + sm[C + c02 + k] * xe2 +
                 sm[2 * C + c02 + k];
      out2.v[k] = from_f32<T>(v2);
      if (WRITE_GHAT) gh2.v[k] = from_f32<T>(ge2);
    }
    *(Pack<T, VEC>*)(gx + i * VEC) = out;
    if (WRITE_GHAT) *(Pack<T, VEC>*)(ghat_out + i * VEC) = gh;
    if (has2) {
      *(Pack<T, VEC>*)(gx + i2 * VEC) = out2;
      if (WRITE_GHAT) *(Pack<T, VEC>*)(ghat_out + i2 * VEC) = gh2;
    }
  }
}

// ---- host helpers ---------------------------------------------------------

static void check_nhwc(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "expected 4D CUDA tensor");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "expected channels_last (NHWC) tensor");
}

template <typename F>
static void dispatch_vec(const at::Tensor& x, F fn) {
  int C = (int)x.size(1);
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, x.scalar_type(), "bn",
      [&] {
        using devT = typename DevT<scalar_t>::type;
        constexpr int VEC = 16 / sizeof(devT);
        TORCH_CHECK(C % VEC == 0, "C must be a multiple of ", VEC);
        TORCH_CHECK((C & (C - 1)) == 0,
                    "C must be a power of two (apply-kernel fast path): ", C);
        TORCH_CHECK(C / VEC <= 2 * AMD_TPB, "C too large: ", C);
        fn((devT*)nullptr, std::integral_constant<int, VEC>{});
      });
}

static int bn_reduce_grid(long R, int C) {
  // enough blocks to saturate HBM reads (1536 = 6 blocks/CU keeps 12
  // waves/SIMD in flight over the 3-stream bwd reduce; 512 measured ~56%
  // of achievable BW); partial-buffer cost is grid*2C f32, folded by
  // bn_collapse_partials
  long rows_per_block = std::max<long>(1, R / 1536);
  return (int)std::min<long>((R + rows_per_block - 1) / rows_per_block, 1536);
}

// collapse [nparts][2C] per-block partials to the few slots the finalize
// kernels loop over
static at::Tensor bn_collapse(const at::Tensor& parts, long C,
                              hipStream_t stream) {
  const int nparts = (int)parts.size(0);
  const int slots = bn_collapse_slots(nparts);
  auto sums2 = at::empty({slots, 2 * C}, parts.options());
  int cgrid = slots * (int)((2 * C + AMD_TPB - 1) / AMD_TPB);
  bn_collapse_partials_kernel<<<cgrid, AMD_TPB, 0, stream>>>(
      parts.data_ptr<float>(), sums2.data_ptr<float>(), nparts, (int)(2 * C),
      slots);
  CHECK_CUDA_OK();
  return sums2;
}

struct BNTrainStats {
  at::Tensor mean, invstd, scale, shift;
};

// training-mode statistics stage shared by every forward entry:
// [reduce over x unless the producing conv's epilogue already left
// partials] -> collapse -> finalize (+ running-stat update)
static BNTrainStats bn_train_stats(const at::Tensor& x,
                                   const std::optional<at::Tensor>& parts,
                                   const at::Tensor& weight,
                                   const at::Tensor& bias,
                                   at::Tensor& running_mean,
                                   at::Tensor& running_var, double momentum,
                                   double eps) {
  const long C = x.size(1);
  const long R = x.numel() / C;
  auto opts = x.options().dtype(at::kFloat);
  auto stream = at::cuda::getCurrentCUDAStream();
  at::Tensor sums;
  if (parts) {
    TORCH_CHECK(parts->size(1) == 2 * C, "parts must be [nparts][2C]");
    sums = *parts;
  } else {
    const int rgrid = bn_reduce_grid(R, C);
    sums = at::empty({rgrid, 2 * C}, opts);
    dispatch_vec(x, [&](auto* tp, auto vec) {
      using devT = std::remove_pointer_t<decltype(tp)>;
      constexpr int VEC = decltype(vec)::value;
      bn_reduce_kernel<devT, VEC, false, 0, false, false>
          <<<rgrid, AMD_TPB, 0, stream>>>((const devT*)x.const_data_ptr(),
                                          nullptr, nullptr, nullptr, nullptr,
                                          nullptr, nullptr, nullptr, nullptr,
                                          sums.data_ptr<float>(), R, (int)C);
      CHECK_CUDA_OK();
    });
  }
  auto sums2 = bn_collapse(sums, C, stream);
  BNTrainStats s{at::empty({C}, opts), at::empty({C}, opts),
                 at::empty({C}, opts), at::empty({C}, opts)};
  int fgrid = (int)((C + 63) / 64);
  bn_finalize_train_kernel<<<fgrid, AMD_TPB, 0, stream>>>(
      sums2.data_ptr<float>(), (int)sums2.size(0), weight.data_ptr<float>(),
      bias.data_ptr<float>(), running_mean.data_ptr<float>(),
      running_var.data_ptr<float>(), s.mean.data_ptr<float>(),
      s.invstd.data_ptr<float>(), s.scale.data_ptr<float>(),
      s.shift.data_ptr<float>(), R, (int)C, (float)momentum, (float)eps);
  CHECK_CUDA_OK();
  return s;
}

struct BNBwdCoeffs {
  at::Tensor gw, gb, A, Bc, Dc;
};

// backward collapse -> finalize: grad_w/grad_b + the apply's A,B,D
static BNBwdCoeffs bn_bwd_coeffs(const at::Tensor& sums,
                                 const at::Tensor& weight,
                                 const at::Tensor& mean,
                                 const at::Tensor& invstd, long R, long C) {
  auto stream = at::cuda::getCurrentCUDAStream();
  auto opts = sums.options();
  auto sums2 = bn_collapse(sums, C, stream);
  BNBwdCoeffs k{at::empty({C}, opts), at::empty({C}, opts),
                at::empty({C}, opts), at::empty({C}, opts),
                at::empty({C}, opts)};
  int fgrid = (int)((C + 63) / 64);
  bn_bwd_finalize_kernel<<<fgrid, AMD_TPB, 0, stream>>>(
      sums2.data_ptr<float>(), (int)sums2.size(0), weight.data_ptr<float>(),
      mean.data_ptr<float>(), invstd.data_ptr<float>(),
      k.gw.data_ptr<float>(), k.gb.data_ptr<float>(), k.A.data_ptr<float>(),
      k.Bc.data_ptr<float>(), k.Dc.data_ptr<float>(), R, (int)C);
  CHECK_CUDA_OK();
  return k;
}

// the dual-BN tail is register-path only: same C on both sides and
// C/VEC within one block (wide-C would need its own masked branch)
static void check_dual(const at::Tensor& x3, const at::Tensor& x_d) {
  check_nhwc(x3);
  check_nhwc(x_d);
  TORCH_CHECK(x3.sizes() == x_d.sizes() &&
                  x3.scalar_type() == x_d.scalar_type(),
              "dual BN tail: x3 and x_d must match in shape and dtype");
  TORCH_CHECK(x3.size(1) * (long)x3.element_size() / 16 <= AMD_TPB,
              "dual BN tail: C too wide for the register path: ", x3.size(1));
}

}  // namespace

// statistics stage alone (mean, invstd, scale, shift + running update) for
// consumers that apply scale/shift inside their own kernel (stem max pool)
std::vector<at::Tensor> batch_norm_train_stats(
    at::Tensor x, std::optional<at::Tensor> parts, at::Tensor weight,
    at::Tensor bias, at::Tensor running_mean, at::Tensor running_var,
    double momentum, double eps) {
  check_nhwc(x);
  auto s = bn_train_stats(x, parts, weight, bias, running_mean, running_var,
                          momentum, eps);
  return {s.mean, s.invstd, s.scale, s.shift};
}

std::vector<at::Tensor> batch_norm_fwd_train(
    at::Tensor x, at::Tensor weight, at::Tensor bias, at::Tensor running_mean,
    at::Tensor running_var, double momentum, double eps, bool relu,
    std::optional<at::Tensor> addend) {
  check_nhwc(x);
  const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const long R = N * H * W;
  auto y = at::empty_like(x);
  // block-tail BNs (relu+addend) also emit a 1-bit relu mask (1/16 the
  // bytes of y) so the bwd reduce skips the y read entirely
  at::Tensor mask;
  if (relu && addend)  // one byte per VEC-pack; VEC is 4 for fp32 (16B/4B)
    mask = at::empty({R * C / 4}, x.options().dtype(at::kByte));
  auto stream = at::cuda::getCurrentCUDAStream();
  auto st = bn_train_stats(x, std::nullopt, weight, bias, running_mean,
                           running_var, momentum, eps);
  auto &mean = st.mean, &invstd = st.invstd, &scale = st.scale,
       &shift = st.shift;

  dispatch_vec(x, [&](auto* tp, auto vec) {
    using devT = std::remove_pointer_t<decltype(tp)>;
    constexpr int VEC = decltype(vec)::value;
    long total_vec = R * C / VEC;
    int agrid = amd_grid(total_vec);
    size_t smem = 2 * C * sizeof(float);
    const devT* zp =
        addend ? (const devT*)addend->const_data_ptr() : nullptr;
#define APPLY(RELU_, ADD_)                                                  \
  bn_apply_kernel<devT, VEC, RELU_, ADD_, true>                             \
      <<<agrid, AMD_TPB, smem, stream>>>(                                   \
          (const devT*)x.const_data_ptr(), zp, (devT*)y.data_ptr(),         \
          mask.defined() ? mask.data_ptr<unsigned char>() : nullptr,        \
          scale.data_ptr<float>(), shift.data_ptr<float>(),     \
          total_vec, (int)C)
    if (relu && addend) APPLY(true, true);
    else if (relu) APPLY(true, false);
    else if (addend) APPLY(false, true);
    else APPLY(false, false);
#undef APPLY
    CHECK_CUDA_OK();
  });
  if (!mask.defined()) mask = at::empty({0}, x.options().dtype(at::kByte));
  return {y, mean, invstd, scale, shift, mask};
}

// forward-train using per-block statistics partials produced by the conv
// epilogue (conv fused BN-stats: the separate reduce pass over x is skipped)
std::vector<at::Tensor> batch_norm_fwd_train_from_parts(
    at::Tensor x, at::Tensor parts, at::Tensor weight, at::Tensor bias,
    at::Tensor running_mean, at::Tensor running_var, double momentum,
    double eps, bool relu, std::optional<at::Tensor> addend) {
  check_nhwc(x);
  const long C = x.size(1);
  const long R = x.numel() / C;
  auto y = at::empty_like(x);
  at::Tensor mask;
  if (relu && addend)  // one byte per VEC-pack; VEC is 4 for fp32 (16B/4B)
    mask = at::empty({R * C / 4}, x.options().dtype(at::kByte));
  auto stream = at::cuda::getCurrentCUDAStream();
  auto st = bn_train_stats(x, parts, weight, bias, running_mean, running_var,
                           momentum, eps);
  auto &mean = st.mean, &invstd = st.invstd, &scale = st.scale,
       &shift = st.shift;
  dispatch_vec(x, [&](auto* tp, auto vec) {
    using devT = std::remove_pointer_t<decltype(tp)>;
    constexpr int VEC = decltype(vec)::value;
    long total_vec = R * C / VEC;
    int agrid = amd_grid(total_vec);
    size_t smem = 2 * C * sizeof(float);
    const devT* zp =
        addend ? (const devT*)addend->const_data_ptr() : nullptr;
#define APPLY2(RELU_, ADD_)                                                 \
  bn_apply_kernel<devT, VEC, RELU_, ADD_, true>                             \
      <<<agrid, AMD_TPB, smem, stream>>>(                                   \
          (const devT*)x.const_data_ptr(), zp, (devT*)y.data_ptr(),         \
          mask.defined() ? mask.data_ptr<unsigned char>() : nullptr,        \
          scale.data_ptr<float>(), shift.data_ptr<float>(),                 \
          total_vec, (int)C)
    if (relu && addend) APPLY2(true, true);
    else if (relu) APPLY2(true, false);
    else if (addend) APPLY2(false, true);
    else APPLY2(false, false);
#undef APPLY2
    CHECK_CUDA_OK();
  });
  if (!mask.defined()) mask = at::empty({0}, x.options().dtype(at::kByte));
  return {y, mean, invstd, scale, shift, mask};
}

// Downsample block tail, forward: y = relu(bn3(x3) + T(bn_d(x_d))) with the
// downsample BN's output never materialized.  Each side takes its
// statistics from conv-epilogue partials when it has them, else from the
// reduce pass (the strided downsample convs emit none).
// Returns {y, mean3, invstd3, mean_d, invstd_d, mask}.
std::vector<at::Tensor> batch_norm_dual_fwd_train(
    at::Tensor x3, at::Tensor x_d, std::optional<at::Tensor> parts3,
    std::optional<at::Tensor> parts_d, at::Tensor weight3, at::Tensor bias3,
    at::Tensor running_mean3, at::Tensor running_var3, double momentum3,
    double eps3, at::Tensor weight_d, at::Tensor bias_d,
    at::Tensor running_mean_d, at::Tensor running_var_d, double momentum_d,
    double eps_d) {
  check_dual(x3, x_d);
  const long C = x3.size(1);
  const long R = x3.numel() / C;
  auto sd = bn_train_stats(x_d, parts_d, weight_d, bias_d, running_mean_d,
                           running_var_d, momentum_d, eps_d);
  auto s3 = bn_train_stats(x3, parts3, weight3, bias3, running_mean3,
                           running_var3, momentum3, eps3);
  auto y = at::empty_like(x3);
  // one byte per VEC-pack; VEC is 4 for fp32 (16B/4B)
  auto mask = at::empty({R * C / 4}, x3.options().dtype(at::kByte));
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_vec(x3, [&](auto* tp, auto vec) {
    using devT = std::remove_pointer_t<decltype(tp)>;
    constexpr int VEC = decltype(vec)::value;
    long total_vec = R * C / VEC;
    int agrid = amd_grid(total_vec);
    bn_apply_kernel<devT, VEC, true, true, true, true>
        <<<agrid, AMD_TPB, 0, stream>>>(
            (const devT*)x3.const_data_ptr(),
            (const devT*)x_d.const_data_ptr(), (devT*)y.data_ptr(),
            mask.data_ptr<unsigned char>(), s3.scale.data_ptr<float>(),
            s3.shift.data_ptr<float>(), total_vec, (int)C,
            sd.scale.data_ptr<float>(), sd.shift.data_ptr<float>());
    CHECK_CUDA_OK();
  });
  return {y, s3.mean, s3.invstd, sd.mean, sd.invstd, mask};
}

// Downsample block tail, backward: one reduce (x3, x_d, go[, go2], mask ->
// ghat + both BNs' sums) and one apply (x3, x_d, ghat -> gx3, gx_d).
// Returns {gx3, gw3, gb3, gx_d, gw_d, gb_d}.
std::vector<at::Tensor> batch_norm_dual_bwd(
    at::Tensor x3, at::Tensor x_d, at::Tensor grad_out,
    std::optional<at::Tensor> grad_out2, at::Tensor relu_mask,
    at::Tensor weight3, at::Tensor mean3, at::Tensor invstd3,
    at::Tensor weight_d, at::Tensor mean_d, at::Tensor invstd_d) {
  check_dual(x3, x_d);
  check_nhwc(grad_out);
  const long C = x3.size(1);
  const long R = x3.numel() / C;
  TORCH_CHECK(relu_mask.numel() == R * C / 4, "relu_mask size mismatch");
  auto opts = x3.options().dtype(at::kFloat);
  const int rgrid = bn_reduce_grid(R, C);
  auto sums3 = at::empty({rgrid, 2 * C}, opts);
  auto sums_d = at::empty({rgrid, 2 * C}, opts);
  auto ghat = at::empty_like(grad_out);
  auto gx3 = at::empty_like(x3);
  auto gx_d = at::empty_like(x_d);
  BNBwdCoeffs k3, kd;
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_vec(x3, [&](auto* tp, auto vec) {
    using devT = std::remove_pointer_t<decltype(tp)>;
    constexpr int VEC = decltype(vec)::value;
    const devT* go2p = grad_out2
        ? (const devT*)grad_out2->const_data_ptr() : nullptr;
    BNDualSide<devT> rs{(const devT*)x_d.const_data_ptr(),
                        mean_d.data_ptr<float>(), invstd_d.data_ptr<float>(),
                        sums_d.data_ptr<float>()};
#define REDUCE_DUAL(GO2_)                                                   \
  bn_reduce_kernel<devT, VEC, true, 3, true, GO2_, true>                    \
      <<<rgrid, AMD_TPB, 0, stream>>>(                                      \
          (const devT*)x3.const_data_ptr(),                                 \
          (const devT*)grad_out.const_data_ptr(), go2p,                     \
          (const devT*)relu_mask.const_data_ptr(), mean3.data_ptr<float>(), \
          invstd3.data_ptr<float>(), nullptr, nullptr,                      \
          (devT*)ghat.data_ptr(), sums3.data_ptr<float>(), R, (int)C, rs)
    if (go2p) REDUCE_DUAL(true);
    else REDUCE_DUAL(false);
#undef REDUCE_DUAL
    CHECK_CUDA_OK();
    k3 = bn_bwd_coeffs(sums3, weight3, mean3, invstd3, R, C);
    kd = bn_bwd_coeffs(sums_d, weight_d, mean_d, invstd_d, R, C);
    long total_vec = R * C / VEC;
    int agrid = amd_grid(total_vec);
    BNDualBwdSide<devT> as{(const devT*)x_d.const_data_ptr(),
                           (devT*)gx_d.data_ptr(), kd.A.data_ptr<float>(),
                           kd.Bc.data_ptr<float>(), kd.Dc.data_ptr<float>()};
    bn_bwd_apply_kernel<devT, VEC, 0, false, true, true>
        <<<agrid, AMD_TPB, 0, stream>>>(
            (const devT*)x3.const_data_ptr(),
            (const devT*)ghat.const_data_ptr(), (devT*)gx3.data_ptr(),
            nullptr, k3.A.data_ptr<float>(), k3.Bc.data_ptr<float>(),
            k3.Dc.data_ptr<float>(), nullptr, nullptr, total_vec, (int)C, as);
    CHECK_CUDA_OK();
  });
  return {gx3, k3.gw, k3.gb, gx_d, kd.gw, kd.gb};
}

at::Tensor batch_norm_fwd_eval(at::Tensor x, at::Tensor weight,
                               at::Tensor bias, at::Tensor running_mean,
                               at::Tensor running_var, double eps, bool relu,
                               std::optional<at::Tensor> addend) {
  check_nhwc(x);
  const long C = x.size(1);
  const long R = x.numel() / C;
  auto opts = x.options().dtype(at::kFloat);
  auto scale = at::empty({C}, opts);
  auto shift = at::empty({C}, opts);
  auto y = at::empty_like(x);
  at::Tensor mask;  // eval: no mask output
  auto stream = at::cuda::getCurrentCUDAStream();
  int fgrid = (int)((C + AMD_TPB - 1) / AMD_TPB);
  bn_finalize_eval_kernel<<<fgrid, AMD_TPB, 0, stream>>>(
      weight.data_ptr<float>(), bias.data_ptr<float>(),
      running_mean.data_ptr<float>(), running_var.data_ptr<float>(),
      scale.data_ptr<float>(), shift.data_ptr<float>(), (int)C, (float)eps);
  CHECK_CUDA_OK();
  dispatch_vec(x, [&](auto* tp, auto vec) {
    using devT = std::remove_pointer_t<decltype(tp)>;
    constexpr int VEC = decltype(vec)::value;
    long total_vec = R * C / VEC;
    int agrid = amd_grid(total_vec);
    size_t smem = 2 * C * sizeof(float);
    const devT* zp =
        addend ? (const devT*)addend->const_data_ptr() : nullptr;
#define APPLY(RELU_, ADD_)                                                  \
  bn_apply_kernel<devT, VEC, RELU_, ADD_, true>                             \
      <<<agrid, AMD_TPB, smem, stream>>>(                                   \
          (const devT*)x.const_data_ptr(), zp, (devT*)y.data_ptr(),         \
          mask.defined() ? mask.data_ptr<unsigned char>() : nullptr,        \
          scale.data_ptr<float>(), shift.data_ptr<float>(),     \
          total_vec, (int)C)
    if (relu && addend) APPLY(true, true);
    else if (relu) APPLY(true, false);
    else if (addend) APPLY(false, true);
    else APPLY(false, false);
#undef APPLY
    CHECK_CUDA_OK();
  });
  return y;
}

std::vector<at::Tensor> batch_norm_bwd(at::Tensor x, at::Tensor grad_out,
                                       std::optional<at::Tensor> y,
                                       at::Tensor weight,
                                       at::Tensor mean, at::Tensor invstd,
                                       bool relu, bool need_ghat,
                                       std::optional<at::Tensor> scale,
                                       std::optional<at::Tensor> shift,
                                       std::optional<at::Tensor> grad_out2,
                                       std::optional<at::Tensor> relu_mask) {
  // Pass structure (every kernel is an HBM-bound R x C stream, so passes
  // are the whole cost):
  //  * no relu:                reduce(x,go) -> apply(x,go -> gx)
  //  * relu + addend (bn3):    reduce(x,go,y -> ghat) [mask from y]
  //                            -> apply(x,ghat -> gx); ghat returned as the
  //                            residual addend gradient (1 pass saved vs
  //                            masking again + writing ghat in apply)
  //  * relu, no addend (bn1/2) with fwd scale/shift: mask recomputed as
  //                            scale*x+shift>0 in BOTH passes — the y read
  //                            disappears entirely (2 passes saved)
  check_nhwc(x);
  check_nhwc(grad_out);
  const long C = x.size(1);
  const long R = x.numel() / C;
  auto opts = x.options().dtype(at::kFloat);
  const int rgrid = bn_reduce_grid(R, C);
  auto sums = at::empty({rgrid, 2 * C}, opts);
  BNBwdCoeffs k;
  auto gx = at::empty_like(x);
  const bool affine_mask = relu && !need_ghat && scale && shift;
  // grad_out2 (rerouted residual gradient) forces the ghat-writing path so
  // the fp32 sum is materialized once
  const bool mask_y = relu && (!affine_mask || grad_out2.has_value());
  at::Tensor ghat;
  if (mask_y || grad_out2) ghat = at::empty_like(grad_out);
  auto stream = at::cuda::getCurrentCUDAStream();

  dispatch_vec(x, [&](auto* tp, auto vec) {
    using devT = std::remove_pointer_t<decltype(tp)>;
    constexpr int VEC = decltype(vec)::value;
    const float* scp = affine_mask ? scale->data_ptr<float>() : nullptr;
    const float* shp = affine_mask ? shift->data_ptr<float>() : nullptr;
    const devT* go2p = grad_out2
        ? (const devT*)grad_out2->const_data_ptr() : nullptr;
#define REDUCE(MASK_, WG_, GO2_)                                            \
  bn_reduce_kernel<devT, VEC, true, MASK_, WG_, GO2_>                       \
      <<<rgrid, AMD_TPB, 0, stream>>>(                                      \
          (const devT*)x.const_data_ptr(),                                  \
          (const devT*)grad_out.const_data_ptr(), go2p,                     \
          yp, mean.data_ptr<float>(),                                       \
          invstd.data_ptr<float>(), scp, shp,                               \
          WG_ ? (devT*)ghat.data_ptr() : nullptr,                           \
          sums.data_ptr<float>(), R, (int)C)
// MASK 3: the fwd bitmask rides in the y operand slot
#define REDUCE3(GO2_)                                                       \
  bn_reduce_kernel<devT, VEC, true, 3, true, GO2_>                          \
      <<<rgrid, AMD_TPB, 0, stream>>>(                                      \
          (const devT*)x.const_data_ptr(),                                  \
          (const devT*)grad_out.const_data_ptr(), go2p,                     \
          (const devT*)mkp, mean.data_ptr<float>(),                         \
          invstd.data_ptr<float>(), scp, shp,                               \
          (devT*)ghat.data_ptr(),                                           \
          sums.data_ptr<float>(), R, (int)C)
    const unsigned char* mkp = (relu_mask && relu_mask->numel())
        ? relu_mask->data_ptr<unsigned char>() : nullptr;
    // only the MASK 1 reduce dereferences y (the affine-mask and bitmask
    // forms never do, so their callers need not keep y alive)
    TORCH_CHECK(y.has_value() || !mask_y || mkp,
                "batch_norm_bwd: y is required to mask a relu+addend BN "
                "that saved no relu_mask");
    const devT* yp = y ? (const devT*)y->const_data_ptr() : nullptr;
    if (mask_y && mkp && go2p) REDUCE3(true);
    else if (mask_y && mkp) REDUCE3(false);
    else if (mask_y && go2p) REDUCE(1, true, true);
    else if (mask_y) REDUCE(1, true, false);
    else if (affine_mask) REDUCE(2, false, false);
    else if (go2p) REDUCE(0, true, true);
    else REDUCE(0, false, false);
#undef REDUCE
#undef REDUCE3
    CHECK_CUDA_OK();
    k = bn_bwd_coeffs(sums, weight, mean, invstd, R, C);
    long total_vec = R * C / VEC;
    int agrid = amd_grid(total_vec);
    size_t smem = (affine_mask ? 5 : 3) * C * sizeof(float);
    // use the materialized ghat whenever the reduce produced it (mask or
    // summed grad_out2); otherwise the raw grad_out
    const devT* go_in = ghat.defined()
                            ? (const devT*)ghat.const_data_ptr()
                            : (const devT*)grad_out.const_data_ptr();
#define BAPPLY(MASK_)                                                       \
  bn_bwd_apply_kernel<devT, VEC, MASK_, false, true>                        \
      <<<agrid, AMD_TPB, smem, stream>>>(                                   \
          (const devT*)x.const_data_ptr(), go_in, (devT*)gx.data_ptr(),     \
          nullptr, k.A.data_ptr<float>(), k.Bc.data_ptr<float>(),           \
          k.Dc.data_ptr<float>(), scp, shp, total_vec, (int)C)
    if (affine_mask) BAPPLY(2);
    else BAPPLY(0);
#undef BAPPLY
    CHECK_CUDA_OK();
  });
  if (!ghat.defined()) ghat = grad_out;  // placeholder (no addend path)
  return {gx, k.gw, k.gb, ghat};
}
