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
// phase-reduction per block into per-block partials that a second stage
// sums in a fixed order (no global atomics).
// All ResNet channel counts (64..2048) hit this register path.
//
// These kernels take power-of-two C only.  Any other C with whole 16-byte
// packs and at most 256 of them per row, and every ReLU6, runs on the
// kernels of batchnorm_anyc.h, behind the same entries and the same
// collapse / finalize stages.
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "batchnorm_anyc.h"

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

// Gradient operands that are a pure gather of a smaller tensor are formed
// in the consuming BN kernel instead of being written out and read back:
//  GSRC_POOL:    go is the stem max pool's input gradient — per element the
//                fp32 sum, in (ho, wo) order, of the <= 4 pool-output
//                gradients whose argmax code selects it, rounded through T
//                like the tensor maxpool_bwd_kernel wrote.  With gy2 (the
//                pool output's second consumer) each window contributes
//                T(gy + gy2), the value the eager add produced.
//  GSRC_COMPACT: goB is the [N,Hs,Ws,C] dgrad of a stride-2 1x1 conv; row
//                (n,h,w) reads (n,h/2,w/2) when h and w are even, else 0 —
//                the tensor scatter_rows_x2 wrote.
constexpr int GSRC_NONE = 0, GSRC_POOL = 1, GSRC_COMPACT = 2;

template <typename T>
struct BNGradSrc {
  const T* gy = nullptr;
  const T* gy2 = nullptr;
  const unsigned char* idx = nullptr;
  int H = 0, W = 0, Hs = 0, Ws = 0;
};

// (n,h,w) of a row, decoded once per thread and advanced incrementally
// (H, W are not powers of two: no 64-bit divide per row)
struct RowPos {
  int n, h, w;
};

__device__ __forceinline__ RowPos row_decode(long r, int H, int W) {
  RowPos p;
  p.w = (int)(r % W);
  r /= W;
  p.h = (int)(r % H);
  p.n = (int)(r / H);
  return p;
}

// p += d for d.w < W, d.h < H (one carry each)
__device__ __forceinline__ void row_advance(RowPos& p, const RowPos& d, int H,
                                            int W) {
  p.w += d.w;
  int c = p.w >= W;
  if (c) p.w -= W;
  p.h += d.h + c;
  c = p.h >= H;
  if (c) p.h -= H;
  p.n += d.n + c;
}

template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> pool_grad_gather(
    const BNGradSrc<T>& s, const RowPos& p, int C, int c0) {
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  // windows (ho,wo) containing (h,w): ho in {h/2, (h+1)/2}, ascending,
  // exactly the loop maxpool_bwd_kernel runs
  const int nh = ((p.h & 1) && (p.h + 1) / 2 < s.Hs) ? 2 : 1;
  const int nw = ((p.w & 1) && (p.w + 1) / 2 < s.Ws) ? 2 : 1;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    if (a >= nh) continue;
    const int ho = p.h / 2 + a;
    const int kh = p.h - (ho * 2 - 1);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (b >= nw) continue;
      const int wo = p.w / 2 + b;
      const int kw = p.w - (wo * 2 - 1);
      const unsigned char code = (unsigned char)(kh * 3 + kw);
      const long obase = (((long)p.n * s.Hs + ho) * s.Ws + wo) * C + c0;
      Pack<unsigned char, VEC> iv =
          *(const Pack<unsigned char, VEC>*)(s.idx + obase);
      Pack<T, VEC> gv = *(const Pack<T, VEC>*)(s.gy + obase);
      if (s.gy2 != nullptr) {
        Pack<T, VEC> g2 = *(const Pack<T, VEC>*)(s.gy2 + obase);
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          gv.v[k] = from_f32<T>(to_f32(gv.v[k]) + to_f32(g2.v[k]));
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        if (iv.v[k] == code) acc[k] += to_f32(gv.v[k]);
    }
  }
  Pack<T, VEC> out;
#pragma unroll
  for (int k = 0; k < VEC; ++k) out.v[k] = from_f32<T>(acc[k]);
  return out;
}

template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> compact_grad_gather(
    const BNGradSrc<T>& s, const RowPos& p, int C, int c0) {
  if (((p.h | p.w) & 1) == 0)
    return *(const Pack<T, VEC>*)(
        s.gy + (((long)p.n * s.Hs + p.h / 2) * s.Ws + p.w / 2) * C + c0);
  Pack<T, VEC> z;
#pragma unroll
  for (int k = 0; k < VEC; ++k) z.v[k] = from_f32<T>(0.f);
  return z;
}

template <typename T, int VEC, bool BWD, int MASK, bool WG, bool GO2,
          bool DUAL = false, int GSRC = GSRC_NONE>
__global__ void __launch_bounds__(AMD_TPB)
bn_reduce_kernel(const T* __restrict__ x, const T* __restrict__ go,
                 const T* __restrict__ goB, const T* __restrict__ y,
                 const float* __restrict__ mean,
                 const float* __restrict__ invstd,
                 const float* __restrict__ scale,
                 const float* __restrict__ shift, T* __restrict__ ghat_out,
                 float* __restrict__ out, long R, int C,
                 BNDualSide<T> ds = {}, BNGradSrc<T> gs = {}) {
  static_assert(!DUAL || (BWD && WG), "DUAL rides the ghat-writing bwd pass");
  static_assert(GSRC == GSRC_NONE || BWD, "gather operands are gradients");
  static_assert(GSRC != GSRC_COMPACT || GO2, "the compact operand is go2");
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
    RowPos pos{0, 0, 0};
    if (GSRC != GSRC_NONE && r0 + phase < r1)
      pos = row_decode(r0 + phase, gs.H, gs.W);
    for (long r = r0 + phase; r < r1; r += rstep) {
      const long base = r * C + c0;
      Pack<T, VEC> xv = *(const Pack<T, VEC>*)(x + base);
      Pack<T, VEC> gv, gv2, yv, gh, dv;
      unsigned int mbits = 0;
      if (BWD) {
        if (GSRC == GSRC_POOL) gv = pool_grad_gather<T, VEC>(gs, pos, C, c0);
        else gv = *(const Pack<T, VEC>*)(go + base);
        if (DUAL) dv = *(const Pack<T, VEC>*)(ds.x + base);
        if (GSRC == GSRC_COMPACT)
          gv2 = compact_grad_gather<T, VEC>(gs, pos, C, c0);
        else if (GO2) gv2 = *(const Pack<T, VEC>*)(goB + base);
        if (GSRC != GSRC_NONE) {  // rstep may exceed W at small shapes
          pos.w += rstep;
          while (pos.w >= gs.W) {
            pos.w -= gs.W;
            if (++pos.h == gs.H) {
              pos.h = 0;
              ++pos.n;
            }
          }
        }
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

// The same fold, streaming: one thread owns VEC adjacent columns of one slot
// (VEC = 4: 16 B loads; VEC = 1 serves twoC % 4 != 0 or a misaligned base),
// work items are laid slot-major over the whole grid so every thread of a
// block has one (twoC = 128: a 256-thread block covers 8 slots), and the
// row loads of a batch of BN_COLLAPSE_U rows are all issued before the
// first add.  The adds then run in the kernel above's order — acc = 0.f,
// rows slot, slot + slots, ... one by one — so every output bit is the same.
constexpr int BN_COLLAPSE_U = 8;

template <int VEC>
__global__ void bn_collapse_partials_stream_kernel(
    const float* __restrict__ in, float* __restrict__ out, int nparts,
    int twoC, int slots) {
  using Vec = Pack<float, VEC>;
  const int cols = twoC / VEC;  // column groups per row
  const long item = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= (long)slots * cols) return;
  const int slot = (int)(item / cols);
  const int c = (int)(item % cols) * VEC;
  const float* src = in + (long)slot * twoC + c;
  const long step = (long)slots * twoC;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  int p = slot;
  // full batches: U independent loads in flight, then U ordered adds
  for (; p + (BN_COLLAPSE_U - 1) * slots < nparts;
       p += BN_COLLAPSE_U * slots, src += BN_COLLAPSE_U * step) {
    Vec v[BN_COLLAPSE_U];
#pragma unroll
    for (int u = 0; u < BN_COLLAPSE_U; ++u)
      v[u] = *(const Vec*)(src + u * step);
#pragma unroll
    for (int u = 0; u < BN_COLLAPSE_U; ++u)
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] += v[u].v[k];
  }
  if (p < nparts) {
    // last, partial batch, still branch-free: a row past the end reads row
    // 0 instead and adds +0.f, which changes no bit (acc starts at +0.f and
    // a sum of round-to-nearest adds from +0.f is never -0.f)
    Vec v[BN_COLLAPSE_U];
#pragma unroll
    for (int u = 0; u < BN_COLLAPSE_U; ++u)
      v[u] = *(const Vec*)(p + u * slots < nparts ? src + u * step : in + c);
#pragma unroll
    for (int u = 0; u < BN_COLLAPSE_U; ++u)
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        acc[k] += p + u * slots < nparts ? v[u].v[k] : 0.f;
  }
  Vec o;
#pragma unroll
  for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
  *(Vec*)(out + (long)slot * twoC + c) = o;
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
          bool DUAL = false, bool REGC = DUAL>
__global__ void __launch_bounds__(AMD_TPB)
bn_apply_kernel(const T* __restrict__ x, const T* __restrict__ z,
                T* __restrict__ y, unsigned char* __restrict__ mask,
                const float* __restrict__ scale,
                const float* __restrict__ shift, long total_vec, int C,
                const float* __restrict__ scale_d = nullptr,
                const float* __restrict__ shift_d = nullptr) {
  static_assert(!DUAL || (HAS_ADD && POW2), "DUAL normalizes the addend");
  static_assert(!DUAL || REGC, "DUAL keeps its coefficients in registers");
  static_assert(!REGC || POW2, "REGC needs a pow2 channel-group count");
  extern __shared__ float sm[];  // [2][C] (unused by REGC)
  const int gpr = C / VEC;
  const long stride = (long)gridDim.x * blockDim.x;
  // REGC: the host admits only pow2 C/VEC <= blockDim, so the grid stride
  // is a multiple of C/VEC and a thread keeps ONE channel group for the
  // whole loop — its two (DUAL: four) coefficient sets live in registers,
  // not LDS.
  float rs[VEC], rb[VEC], rsd[VEC], rbd[VEC];
  if (REGC) {
    const int cf =
        (int)(((long)blockIdx.x * blockDim.x + threadIdx.x) & (gpr - 1)) * VEC;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      rs[k] = scale[cf + k];
      rb[k] = shift[cf + k];
      if (DUAL) {
        rsd[k] = scale_d[cf + k];
        rbd[k] = shift_d[cf + k];
      }
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
      float v = REGC ? rs[k] * to_f32(xv.v[k]) + rb[k]
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
      float v2 = REGC ? rs[k] * to_f32(xv2.v[k]) + rb[k]
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

// The LDS path's gx arithmetic with its contraction spelled out.  The
// compiler is free to fuse either product of A*ghat + B*x + D into the FMA,
// and it picks differently per kernel variant (MASK 0 fuses A*ghat, MASK 2
// fuses B*x; with the coefficients in registers it flipped MASK 0), which
// moves the last bit.  The register path pins the LDS path's choice.
template <int MASK>
__device__ __forceinline__ float bn_bwd_gx(float a, float b, float d,
                                           float ge, float xe) {
#pragma clang fp contract(off)
  if (MASK == 2) return __builtin_fmaf(b, xe, a * ge) + d;
  return __builtin_fmaf(a, ge, b * xe) + d;
}

// REGC (single BN, pow2 C/VEC <= blockDim): the same one-channel-group-per-
// thread property lets the 3 (MASK 2: 5) coefficient sets live in registers
// instead of LDS; the arithmetic is the LDS path's, so are the bits.
// POOLGO (stem, REGC only): go is gathered from the max pool's gradient
// (pool_grad_gather) instead of read from a materialized tensor.
template <typename T, int VEC, int MASK, bool WRITE_GHAT, bool POW2,
          bool DUAL = false, bool REGC = false, bool POOLGO = false>
__global__ void __launch_bounds__(AMD_TPB)
bn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ go,
                    T* __restrict__ gx,
                    T* __restrict__ ghat_out, const float* __restrict__ A,
                    const float* __restrict__ Bc, const float* __restrict__ Dc,
                    const float* __restrict__ scale,
                    const float* __restrict__ shift, long total_vec, int C,
                    BNDualBwdSide<T> ds = {}, BNGradSrc<T> gs = {}) {
  static_assert(!DUAL || (MASK == 0 && POW2 && !WRITE_GHAT),
                "DUAL consumes the materialized ghat");
  static_assert(!REGC || (POW2 && !DUAL), "REGC is the single-BN form");
  static_assert(!POOLGO || REGC, "POOLGO rides the register path");
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
  if (REGC) {
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c0 = (int)(i0 & (gpr - 1)) * VEC;
    float ra[VEC], rb[VEC], rd[VEC], rsc[VEC], rsh[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      ra[k] = A[c0 + k];
      rb[k] = Bc[c0 + k];
      rd[k] = Dc[c0 + k];
      if (MASK == 2) {
        rsc[k] = scale[c0 + k];
        rsh[k] = shift[c0 + k];
      }
    }
    // POOLGO: both streams' (n,h,w), advanced by two grid strides of rows
    RowPos p1{0, 0, 0}, p2{0, 0, 0}, dstep{0, 0, 0};
    if (POOLGO) {
      const int lg = __builtin_ctz(gpr);
      const long rstride = stride >> lg;  // stride is a multiple of gpr
      if (i0 < total_vec) p1 = row_decode(i0 >> lg, gs.H, gs.W);
      p2 = p1;
      row_advance(p2, row_decode(rstride, gs.H, gs.W), gs.H, gs.W);
      dstep = row_decode(2 * rstride, gs.H, gs.W);
    }
    for (long i = i0; i < total_vec; i += 2 * stride) {
      const bool has2 = i + stride < total_vec;
      const long i2 = has2 ? i + stride : i;  // clamp: loads stay in bounds
      Pack<T, VEC> xv = *(const Pack<T, VEC>*)(x + i * VEC);
      Pack<T, VEC> xv2 = *(const Pack<T, VEC>*)(x + i2 * VEC);
      Pack<T, VEC> gv, gv2;
      if (POOLGO) {
        gv = pool_grad_gather<T, VEC>(gs, p1, C, c0);
        gv2 = pool_grad_gather<T, VEC>(gs, has2 ? p2 : p1, C, c0);
        row_advance(p1, dstep, gs.H, gs.W);
        row_advance(p2, dstep, gs.H, gs.W);
      } else {
        gv = *(const Pack<T, VEC>*)(go + i * VEC);
        gv2 = *(const Pack<T, VEC>*)(go + i2 * VEC);
      }
      Pack<T, VEC> out, gh, out2, gh2;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float xe = to_f32(xv.v[k]);
        float ge = to_f32(gv.v[k]);
        if (MASK == 2 && rsc[k] * xe + rsh[k] <= 0.f) ge = 0.f;
        float v = bn_bwd_gx<MASK>(ra[k], rb[k], rd[k], ge, xe);
        out.v[k] = from_f32<T>(v);
        if (WRITE_GHAT) gh.v[k] = from_f32<T>(ge);
        float xe2 = to_f32(xv2.v[k]);
        float ge2 = to_f32(gv2.v[k]);
        if (MASK == 2 && rsc[k] * xe2 + rsh[k] <= 0.f) ge2 = 0.f;
        float v2 = bn_bwd_gx<MASK>(ra[k], rb[k], rd[k], ge2, xe2);
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

static bool bn_pow2(long C) { return (C & (C - 1)) == 0; }

// the forward / backward activation selector of the entries' two flags
static int bn_act(bool relu, bool relu6) {
  TORCH_CHECK(!(relu && relu6), "batch_norm: relu and relu6 are exclusive");
  return relu6 ? BN_ACT_RELU6 : relu ? BN_ACT_RELU : BN_ACT_NONE;
}

// which family serves (C, act): the power-of-two kernels keep every shape
// they served before ReLU6 existed
static bool bn_use_anyc(long C, int act) {
  return !bn_pow2(C) || act == BN_ACT_RELU6;
}

// the any-C contract: whole 16-byte packs, one channel group per thread
static void bn_check_anyc_channels(const at::Tensor& x) {
  const long C = x.size(1);
  const long vec = 16 / (long)x.element_size();
  TORCH_CHECK(C > 0 && C % vec == 0 && C / vec <= AMD_TPB,
              "batch_norm: C must be a multiple of ", vec, " and at most ",
              vec * AMD_TPB, " for this dtype, got ", C);
}

// forward entries: refuse what the any-C family does not build before any
// kernel runs (the statistics stage updates the running stats in place)
static void bn_check_fwd_form(const at::Tensor& x, int act,
                              const std::optional<at::Tensor>& addend) {
  const long C = x.size(1);
  if (!bn_use_anyc(C, act)) return;
  bn_check_anyc_channels(x);
  TORCH_CHECK(!(addend && act != BN_ACT_NONE), "batch_norm: an addend under ",
              act == BN_ACT_RELU6 ? "ReLU6" : "ReLU",
              " is not built for this channel count: C = ", C);
}

template <typename F>
static void dispatch_vec_anyc(const at::Tensor& x, F fn) {
  bn_check_anyc_channels(x);
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, x.scalar_type(),
      "bn_anyc", [&] {
        using devT = typename DevT<scalar_t>::type;
        constexpr int VEC = 16 / sizeof(devT);
        fn((devT*)nullptr, std::integral_constant<int, VEC>{});
      });
}

// AMDTRAIN_BN_REGCOEF=0 keeps the single-BN applies on the LDS coefficient
// path (A/B switch; read per call so one process can compare both)
static bool bn_regcoef_enabled() {
  const char* v = std::getenv("AMDTRAIN_BN_REGCOEF");
  return v == nullptr || std::strcmp(v, "1") == 0;
}

// forward apply shared by the train / from-parts / eval entries
static void bn_apply_launch(const at::Tensor& x,
                            const std::optional<at::Tensor>& addend,
                            at::Tensor& y, const at::Tensor& mask,
                            const at::Tensor& scale, const at::Tensor& shift,
                            int act) {
  const long C = x.size(1);
  const long R = x.numel() / C;
  auto stream = at::cuda::getCurrentCUDAStream();
  if (bn_use_anyc(C, act)) {
    if (addend) {
      check_nhwc(*addend);
      TORCH_CHECK(addend->sizes() == x.sizes() &&
                      addend->scalar_type() == x.scalar_type(),
                  "batch_norm: addend must match x in shape and dtype");
    }
    // (bn_check_fwd_form has refused an addend under an activation)
    dispatch_vec_anyc(x, [&](auto* tp, auto vec) {
      using devT = std::remove_pointer_t<decltype(tp)>;
      constexpr int VEC = decltype(vec)::value;
      const long total_vec = R * C / VEC;
      const int nt = bn_anyc_block((int)(C / VEC));
      const int agrid = amd_grid(total_vec, nt);
      const devT* zp =
          addend ? (const devT*)addend->const_data_ptr() : nullptr;
#define APPLY_ANYC(ACT_, ADD_)                                              \
  bn_anyc_apply_kernel<devT, VEC, ACT_, ADD_><<<agrid, nt, 0, stream>>>(    \
      (const devT*)x.const_data_ptr(), zp, (devT*)y.data_ptr(),             \
      scale.data_ptr<float>(), shift.data_ptr<float>(), total_vec, (int)C)
      if (addend) APPLY_ANYC(BN_ACT_NONE, true);
      else if (act == BN_ACT_RELU6) APPLY_ANYC(BN_ACT_RELU6, false);
      else if (act == BN_ACT_RELU) APPLY_ANYC(BN_ACT_RELU, false);
      else APPLY_ANYC(BN_ACT_NONE, false);
#undef APPLY_ANYC
      CHECK_CUDA_OK();
    });
    return;
  }
  const bool relu = act == BN_ACT_RELU;
  dispatch_vec(x, [&](auto* tp, auto vec) {
    using devT = std::remove_pointer_t<decltype(tp)>;
    constexpr int VEC = decltype(vec)::value;
    long total_vec = R * C / VEC;
    int agrid = amd_grid(total_vec);
    // one channel group per thread needs C/VEC (pow2) to divide the block
    const bool regc = bn_regcoef_enabled() && C / VEC <= AMD_TPB;
    size_t smem = regc ? 0 : 2 * C * sizeof(float);
    const devT* zp =
        addend ? (const devT*)addend->const_data_ptr() : nullptr;
#define APPLY(RELU_, ADD_, REGC_)                                           \
  bn_apply_kernel<devT, VEC, RELU_, ADD_, true, false, REGC_>               \
      <<<agrid, AMD_TPB, smem, stream>>>(                                   \
          (const devT*)x.const_data_ptr(), zp, (devT*)y.data_ptr(),         \
          mask.defined() ? mask.data_ptr<unsigned char>() : nullptr,        \
          scale.data_ptr<float>(), shift.data_ptr<float>(), total_vec,      \
          (int)C)
#define APPLY_RC(RELU_, ADD_)                                               \
  do {                                                                      \
    if (regc) APPLY(RELU_, ADD_, true);                                     \
    else APPLY(RELU_, ADD_, false);                                         \
  } while (0)
    if (relu && addend) APPLY_RC(true, true);
    else if (relu) APPLY_RC(true, false);
    else if (addend) APPLY_RC(false, true);
    else APPLY_RC(false, false);
#undef APPLY_RC
#undef APPLY
    CHECK_CUDA_OK();
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
// kernels loop over.  impl: 1 the streaming kernel, 0 the one-column-per-
// thread kernel it replaced (AMDTRAIN_BN_COLLAPSE=0), negative = the
// environment, else 1; both give the same bits.
static at::Tensor bn_collapse(const at::Tensor& parts, long C,
                              hipStream_t stream, long impl = -1) {
  static const int env = []() {
    const char* e = std::getenv("AMDTRAIN_BN_COLLAPSE");
    return e ? (e[0] == '0' ? 0 : 1) : -1;
  }();
  if (impl < 0) impl = env >= 0 ? env : 1;
  const int nparts = (int)parts.size(0);
  const int slots = bn_collapse_slots(nparts);
  const int twoC = (int)(2 * C);
  auto sums2 = at::empty({slots, 2 * C}, parts.options());
  const float* in = parts.data_ptr<float>();
  float* out = sums2.data_ptr<float>();
  if (impl == 0) {
    int cgrid = slots * (int)((2 * C + AMD_TPB - 1) / AMD_TPB);
    bn_collapse_partials_kernel<<<cgrid, AMD_TPB, 0, stream>>>(
        in, out, nparts, twoC, slots);
  } else {
    const bool vec = twoC % 4 == 0 && (uintptr_t)in % 16 == 0 &&
                     (uintptr_t)out % 16 == 0;
    const long items = (long)slots * (vec ? twoC / 4 : twoC);
    const int cgrid = (int)((items + AMD_TPB - 1) / AMD_TPB);
    if (vec)
      bn_collapse_partials_stream_kernel<4><<<cgrid, AMD_TPB, 0, stream>>>(
          in, out, nparts, twoC, slots);
    else
      bn_collapse_partials_stream_kernel<1><<<cgrid, AMD_TPB, 0, stream>>>(
          in, out, nparts, twoC, slots);
  }
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
    if (!bn_pow2(C))
      dispatch_vec_anyc(x, [&](auto* tp, auto vec) {
        using devT = std::remove_pointer_t<decltype(tp)>;
        constexpr int VEC = decltype(vec)::value;
        bn_anyc_reduce_kernel<devT, VEC, false, BN_ACT_NONE>
            <<<rgrid, bn_anyc_block((int)(C / VEC)), 0, stream>>>(
                (const devT*)x.const_data_ptr(), nullptr, nullptr, nullptr,
                nullptr, nullptr, sums.data_ptr<float>(), R, (int)C);
        CHECK_CUDA_OK();
      });
    else dispatch_vec(x, [&](auto* tp, auto vec) {
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

// single-BN backward apply: the affine-mask form (MASK 2) when the forward's
// scale/shift are given, else MASK 0.  pool != nullptr gathers go from the
// stem pool gradient (register path only; the caller has checked C).
template <typename devT, int VEC>
static void bn_bwd_apply_launch(const devT* x, const devT* go, devT* gx,
                                const BNBwdCoeffs& k, const float* scp,
                                const float* shp, long R, long C,
                                const BNGradSrc<devT>* pool) {
  auto stream = at::cuda::getCurrentCUDAStream();
  const long total_vec = R * C / VEC;
  const int agrid = amd_grid(total_vec);
  const bool affine = scp != nullptr;
  const bool fits = C / VEC <= AMD_TPB;  // one channel group per thread
#define BAPPLY(MASK_, REGC_, POOL_, SMEM_, GS_)                             \
  bn_bwd_apply_kernel<devT, VEC, MASK_, false, true, false, REGC_, POOL_>   \
      <<<agrid, AMD_TPB, SMEM_, stream>>>(                                  \
          x, go, gx, nullptr, k.A.data_ptr<float>(),                        \
          k.Bc.data_ptr<float>(), k.Dc.data_ptr<float>(), scp, shp,         \
          total_vec, (int)C, BNDualBwdSide<devT>{}, GS_)
  if (pool != nullptr) {
    TORCH_CHECK(affine && fits, "pool-gather bwd apply: unsupported form");
    BAPPLY(2, true, true, 0, *pool);
  } else if (bn_regcoef_enabled() && fits) {
    if (affine) BAPPLY(2, true, false, 0, BNGradSrc<devT>{});
    else BAPPLY(0, true, false, 0, BNGradSrc<devT>{});
  } else {
    const size_t smem = (affine ? 5 : 3) * C * sizeof(float);
    if (affine) BAPPLY(2, false, false, smem, BNGradSrc<devT>{});
    else BAPPLY(0, false, false, smem, BNGradSrc<devT>{});
  }
#undef BAPPLY
  CHECK_CUDA_OK();
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

// the fold on its own (tests, tools): parts [nparts][2C] fp32 -> [slots][2C]
at::Tensor bn_collapse_partials(at::Tensor parts, long impl) {
  TORCH_CHECK(parts.is_cuda() && parts.dim() == 2 &&
              parts.scalar_type() == at::kFloat && parts.size(0) >= 1 &&
              parts.size(1) % 2 == 0, "parts must be fp32 [nparts][2C]");
  TORCH_CHECK(parts.stride(1) == 1 && parts.stride(0) == parts.size(1),
              "parts must be dense (a storage offset is fine)");
  return bn_collapse(parts, parts.size(1) / 2,
                     at::cuda::getCurrentCUDAStream(), impl);
}

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
    std::optional<at::Tensor> addend, bool relu6) {
  check_nhwc(x);
  const int act = bn_act(relu, relu6);
  bn_check_fwd_form(x, act, addend);
  const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const long R = N * H * W;
  auto y = at::empty_like(x);
  // block-tail BNs (relu+addend) also emit a 1-bit relu mask (1/16 the
  // bytes of y) so the bwd reduce skips the y read entirely
  at::Tensor mask;
  // one byte per VEC-pack; VEC is 4 for fp32 (16B/4B)
  if (relu && addend && !bn_use_anyc(C, act))
    mask = at::empty({R * C / 4}, x.options().dtype(at::kByte));
  auto st = bn_train_stats(x, std::nullopt, weight, bias, running_mean,
                           running_var, momentum, eps);
  auto &mean = st.mean, &invstd = st.invstd, &scale = st.scale,
       &shift = st.shift;
  bn_apply_launch(x, addend, y, mask, scale, shift, act);
  if (!mask.defined()) mask = at::empty({0}, x.options().dtype(at::kByte));
  return {y, mean, invstd, scale, shift, mask};
}

// forward-train using per-block statistics partials produced by the conv
// epilogue (conv fused BN-stats: the separate reduce pass over x is skipped)
std::vector<at::Tensor> batch_norm_fwd_train_from_parts(
    at::Tensor x, at::Tensor parts, at::Tensor weight, at::Tensor bias,
    at::Tensor running_mean, at::Tensor running_var, double momentum,
    double eps, bool relu, std::optional<at::Tensor> addend, bool relu6) {
  check_nhwc(x);
  const int act = bn_act(relu, relu6);
  bn_check_fwd_form(x, act, addend);
  const long C = x.size(1);
  const long R = x.numel() / C;
  auto y = at::empty_like(x);
  at::Tensor mask;
  // one byte per VEC-pack; VEC is 4 for fp32 (16B/4B)
  if (relu && addend && !bn_use_anyc(C, act))
    mask = at::empty({R * C / 4}, x.options().dtype(at::kByte));
  auto st = bn_train_stats(x, parts, weight, bias, running_mean, running_var,
                           momentum, eps);
  auto &mean = st.mean, &invstd = st.invstd, &scale = st.scale,
       &shift = st.shift;
  bn_apply_launch(x, addend, y, mask, scale, shift, act);
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
                               std::optional<at::Tensor> addend, bool relu6) {
  check_nhwc(x);
  const int act = bn_act(relu, relu6);
  bn_check_fwd_form(x, act, addend);
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
  bn_apply_launch(x, addend, y, mask, scale, shift, act);
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
                                       std::optional<at::Tensor> relu_mask,
                                       bool grad_out2_compact, bool relu6) {
  // relu6, or a C that is not a power of two: the any-C kernels (below).
  // grad_out2_compact: grad_out2 is the [N*Hs*Ws, C] dgrad of a stride-2
  // 1x1 conv (Hs = ceil(H/2), Ws = ceil(W/2)); the reduce reads it at the
  // even positions and adds 0 elsewhere, which is the tensor
  // scatter_rows_x2 would have written.  Register path only.
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
  const int act = bn_act(relu, relu6);
  const long C = x.size(1);
  const long R = x.numel() / C;
  auto opts = x.options().dtype(at::kFloat);
  const int rgrid = bn_reduce_grid(R, C);
  auto sums = at::empty({rgrid, 2 * C}, opts);
  BNBwdCoeffs k;
  auto gx = at::empty_like(x);
  if (bn_use_anyc(C, act)) {
    TORCH_CHECK(grad_out.sizes() == x.sizes() &&
                    grad_out.scalar_type() == x.scalar_type(),
                "batch_norm_bwd: grad_out must match x in shape and dtype");
    // Two passes, neither reads y: reduce(x, go) -> apply(x, go -> gx),
    // each masking go by the activation recomputed from scale / shift.
    // With an addend (no activation) its gradient is grad_out itself.
    TORCH_CHECK(!grad_out2.has_value(),
                "batch_norm_bwd: grad_out2 (the block-tail mailbox) is "
                "power-of-two C and ReLU only: C = ", C);
    TORCH_CHECK(!(need_ghat && act != BN_ACT_NONE),
                "batch_norm_bwd: an addend under an activation is not built "
                "for this channel count: C = ", C);
    TORCH_CHECK(act == BN_ACT_NONE || (scale && shift),
                "batch_norm_bwd: the activation mask needs the forward's "
                "scale and shift");
    dispatch_vec_anyc(x, [&](auto* tp, auto vec) {
      using devT = std::remove_pointer_t<decltype(tp)>;
      constexpr int VEC = decltype(vec)::value;
      auto stream = at::cuda::getCurrentCUDAStream();
      const float* scp = act != BN_ACT_NONE ? scale->data_ptr<float>()
                                            : nullptr;
      const float* shp = act != BN_ACT_NONE ? shift->data_ptr<float>()
                                            : nullptr;
      const devT* xp = (const devT*)x.const_data_ptr();
      const devT* gop = (const devT*)grad_out.const_data_ptr();
      const int nt = bn_anyc_block((int)(C / VEC));
      const long total_vec = R * C / VEC;
      const int agrid = amd_grid(total_vec, nt);
#define BWD_ANYC(ACT_)                                                      \
  do {                                                                      \
    bn_anyc_reduce_kernel<devT, VEC, true, ACT_><<<rgrid, nt, 0, stream>>>( \
        xp, gop, mean.data_ptr<float>(), invstd.data_ptr<float>(), scp,     \
        shp, sums.data_ptr<float>(), R, (int)C);                            \
    CHECK_CUDA_OK();                                                        \
    k = bn_bwd_coeffs(sums, weight, mean, invstd, R, C);                    \
    bn_anyc_bwd_apply_kernel<devT, VEC, ACT_><<<agrid, nt, 0, stream>>>(    \
        xp, gop, (devT*)gx.data_ptr(), k.A.data_ptr<float>(),               \
        k.Bc.data_ptr<float>(), k.Dc.data_ptr<float>(), scp, shp,           \
        total_vec, (int)C);                                                 \
    CHECK_CUDA_OK();                                                        \
  } while (0)
      if (act == BN_ACT_RELU6) BWD_ANYC(BN_ACT_RELU6);
      else if (act == BN_ACT_RELU) BWD_ANYC(BN_ACT_RELU);
      else BWD_ANYC(BN_ACT_NONE);
#undef BWD_ANYC
    });
    return {gx, k.gw, k.gb, grad_out};
  }
  const bool affine_mask = relu && !need_ghat && scale && shift;
  // grad_out2 (rerouted residual gradient) forces the ghat-writing path so
  // the fp32 sum is materialized once
  const bool mask_y = relu && (!affine_mask || grad_out2.has_value());
  at::Tensor ghat;
  if (mask_y || grad_out2) ghat = at::empty_like(grad_out);
  auto stream = at::cuda::getCurrentCUDAStream();
  const long H = x.size(2), W = x.size(3);
  const long Hs = (H + 1) / 2, Ws = (W + 1) / 2;
  if (grad_out2_compact) {
    TORCH_CHECK(grad_out2.has_value() && grad_out2->is_cuda() &&
                    grad_out2->dim() == 2 && grad_out2->is_contiguous() &&
                    grad_out2->scalar_type() == x.scalar_type() &&
                    grad_out2->size(0) == x.size(0) * Hs * Ws &&
                    grad_out2->size(1) == C,
                "batch_norm_bwd: compact grad_out2 must be a contiguous "
                "[N*ceil(H/2)*ceil(W/2), C] tensor of x's dtype");
    TORCH_CHECK(C * (long)x.element_size() / 16 <= AMD_TPB,
                "batch_norm_bwd: C too wide for a compact grad_out2: ", C);
  } else if (grad_out2) {
    check_nhwc(*grad_out2);
    TORCH_CHECK(grad_out2->sizes() == x.sizes(),
                "batch_norm_bwd: grad_out2 shape mismatch");
  }

  dispatch_vec(x, [&](auto* tp, auto vec) {
    using devT = std::remove_pointer_t<decltype(tp)>;
    constexpr int VEC = decltype(vec)::value;
    const float* scp = affine_mask ? scale->data_ptr<float>() : nullptr;
    const float* shp = affine_mask ? shift->data_ptr<float>() : nullptr;
    const devT* go2p = grad_out2
        ? (const devT*)grad_out2->const_data_ptr() : nullptr;
    BNGradSrc<devT> gs;
    if (grad_out2_compact) {
      gs.gy = go2p;
      gs.H = (int)H, gs.W = (int)W, gs.Hs = (int)Hs, gs.Ws = (int)Ws;
    }
#define REDUCE_G(MASK_, WG_, GO2_, GSRC_)                                   \
  bn_reduce_kernel<devT, VEC, true, MASK_, WG_, GO2_, false, GSRC_>         \
      <<<rgrid, AMD_TPB, 0, stream>>>(                                      \
          (const devT*)x.const_data_ptr(),                                  \
          (const devT*)grad_out.const_data_ptr(), go2p,                     \
          yp, mean.data_ptr<float>(),                                       \
          invstd.data_ptr<float>(), scp, shp,                               \
          WG_ ? (devT*)ghat.data_ptr() : nullptr,                           \
          sums.data_ptr<float>(), R, (int)C, BNDualSide<devT>{}, gs)
#define REDUCE(MASK_, WG_, GO2_) REDUCE_G(MASK_, WG_, GO2_, GSRC_NONE)
// MASK 3: the fwd bitmask rides in the y operand slot
#define REDUCE3_G(GO2_, GSRC_)                                              \
  bn_reduce_kernel<devT, VEC, true, 3, true, GO2_, false, GSRC_>            \
      <<<rgrid, AMD_TPB, 0, stream>>>(                                      \
          (const devT*)x.const_data_ptr(),                                  \
          (const devT*)grad_out.const_data_ptr(), go2p,                     \
          (const devT*)mkp, mean.data_ptr<float>(),                         \
          invstd.data_ptr<float>(), scp, shp,                               \
          (devT*)ghat.data_ptr(),                                           \
          sums.data_ptr<float>(), R, (int)C, BNDualSide<devT>{}, gs)
#define REDUCE3(GO2_) REDUCE3_G(GO2_, GSRC_NONE)
    const unsigned char* mkp = (relu_mask && relu_mask->numel())
        ? relu_mask->data_ptr<unsigned char>() : nullptr;
    // only the MASK 1 reduce dereferences y (the affine-mask and bitmask
    // forms never do, so their callers need not keep y alive)
    TORCH_CHECK(y.has_value() || !mask_y || mkp,
                "batch_norm_bwd: y is required to mask a relu+addend BN "
                "that saved no relu_mask");
    const devT* yp = y ? (const devT*)y->const_data_ptr() : nullptr;
    if (grad_out2_compact) {
      if (mask_y && mkp) REDUCE3_G(true, GSRC_COMPACT);
      else if (mask_y) REDUCE_G(1, true, true, GSRC_COMPACT);
      else REDUCE_G(0, true, true, GSRC_COMPACT);
    } else if (mask_y && mkp && go2p) REDUCE3(true);
    else if (mask_y && mkp) REDUCE3(false);
    else if (mask_y && go2p) REDUCE(1, true, true);
    else if (mask_y) REDUCE(1, true, false);
    else if (affine_mask) REDUCE(2, false, false);
    else if (go2p) REDUCE(0, true, true);
    else REDUCE(0, false, false);
#undef REDUCE
#undef REDUCE3
#undef REDUCE_G
#undef REDUCE3_G
    CHECK_CUDA_OK();
    k = bn_bwd_coeffs(sums, weight, mean, invstd, R, C);
    // use the materialized ghat whenever the reduce produced it (mask or
    // summed grad_out2); otherwise the raw grad_out
    const devT* go_in = ghat.defined()
                            ? (const devT*)ghat.const_data_ptr()
                            : (const devT*)grad_out.const_data_ptr();
    bn_bwd_apply_launch<devT, VEC>((const devT*)x.const_data_ptr(), go_in,
                                   (devT*)gx.data_ptr(), k, scp, shp, R, C,
                                   nullptr);
  });
  if (!ghat.defined()) ghat = grad_out;  // placeholder (no addend path)
  return {gx, k.gw, k.gb, ghat};
}

// Stem BN backward with the max pool's backward folded in: grad_out of the
// BN is never materialized — the reduce and the affine-mask apply gather
// it from the pool-output gradient(s) and the argmax codes.  grad_pool2 is
// the gradient from the pool output's second consumer (GradCell), summed
// per window as T(gy + gy2).  Returns {gx, gw, gb}.
std::vector<at::Tensor> batch_norm_bwd_pool(
    at::Tensor x, at::Tensor grad_pool, std::optional<at::Tensor> grad_pool2,
    at::Tensor idx, at::Tensor weight, at::Tensor mean, at::Tensor invstd,
    at::Tensor scale, at::Tensor shift) {
  check_nhwc(x);
  check_nhwc(grad_pool);
  const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const long Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long R = N * H * W;
  const std::vector<int64_t> pool_shape{N, C, Ho, Wo};
  TORCH_CHECK(grad_pool.sizes() == pool_shape &&
                  grad_pool.scalar_type() == x.scalar_type(),
              "batch_norm_bwd_pool: grad_pool must be [N,C,Ho,Wo] of x's "
              "dtype");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kByte &&
                  idx.sizes() == pool_shape &&
                  idx.is_contiguous(at::MemoryFormat::ChannelsLast),
              "batch_norm_bwd_pool: idx must be NHWC u8 [N,C,Ho,Wo]");
  if (grad_pool2) {
    check_nhwc(*grad_pool2);
    TORCH_CHECK(grad_pool2->sizes() == pool_shape &&
                    grad_pool2->scalar_type() == x.scalar_type(),
                "batch_norm_bwd_pool: grad_pool2 shape/dtype mismatch");
  }
  TORCH_CHECK(C * (long)x.element_size() / 16 <= AMD_TPB,
              "batch_norm_bwd_pool: C too wide for the register path: ", C);
  TORCH_CHECK(R < (1L << 31), "batch_norm_bwd_pool: too many rows");
  auto opts = x.options().dtype(at::kFloat);
  const int rgrid = bn_reduce_grid(R, C);
  auto sums = at::empty({rgrid, 2 * C}, opts);
  BNBwdCoeffs k;
  auto gx = at::empty_like(x);
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_vec(x, [&](auto* tp, auto vec) {
    using devT = std::remove_pointer_t<decltype(tp)>;
    constexpr int VEC = decltype(vec)::value;
    const float* scp = scale.data_ptr<float>();
    const float* shp = shift.data_ptr<float>();
    BNGradSrc<devT> gs;
    gs.gy = (const devT*)grad_pool.const_data_ptr();
    gs.gy2 = grad_pool2 ? (const devT*)grad_pool2->const_data_ptr() : nullptr;
    gs.idx = idx.data_ptr<unsigned char>();
    gs.H = (int)H, gs.W = (int)W, gs.Hs = (int)Ho, gs.Ws = (int)Wo;
    bn_reduce_kernel<devT, VEC, true, 2, false, false, false, GSRC_POOL>
        <<<rgrid, AMD_TPB, 0, stream>>>(
            (const devT*)x.const_data_ptr(), nullptr, nullptr, nullptr,
            mean.data_ptr<float>(), invstd.data_ptr<float>(), scp, shp,
            nullptr, sums.data_ptr<float>(), R, (int)C, BNDualSide<devT>{},
            gs);
    CHECK_CUDA_OK();
    k = bn_bwd_coeffs(sums, weight, mean, invstd, R, C);
    bn_bwd_apply_launch<devT, VEC>((const devT*)x.const_data_ptr(), nullptr,
                                   (devT*)gx.data_ptr(), k, scp, shp, R, C,
                                   &gs);
  });
  return {gx, k.gw, k.gb};
}
