// Generic implicit-GEMM convolution for gfx950 — covers the ResNet stem
// (7x7 stride-2 pad-3, Cin=3) and any other odd configuration.
//
// Motivation (measured): torch-ROCm's MIOpen path for the stem wgrad
// nondeterministically selects `naive_conv_..._wrw` at ~1.2 s/call
// (profiles/rocprof_kernel_stats_allcustom.txt) — the hot path must not
// depend on MIOpen find.  Here the im2col K dimension (KH*KW*Cin, e.g. 147)
// is padded to a multiple of 32 and A-tiles are staged by per-element
// gather (scalar loads + LDS writes; the data is tiny — Cin=3 — so staging
// amplification is ~940 MB/step at b256, ~0.15 ms of HBM time), then the
// same 128x128 MFMA block structure as gemm.hip runs the math.
//
// The channel-padded (3 -> 8) 49-tap stem runs the C8 staging on a 64-wide
// n-tile.  Opt-in (AMDTRAIN_STEM_S2D=1; faster, but not bit-compatible with
// the 49-tap path) the stem runs in a width space-to-depth form
// (conv.py stem_s2d_weight): channels 3 -> 4, two neighbouring pixels form
// one 8-channel row, and the conv becomes 7 x 4 taps of 8 channels with
// stride (2, 1) — K = 224 = 7 K-steps, one per kernel row (ROW4 staging),
// on a 64-wide n-tile, with the BN-statistics partials in the epilogue.
//
//   fwd:   Y[m, cout] = sum_col im2col[m, col] * W2[cout, col]
//   wgrad: the tap-gather form of tn2_wgrad (wgrad.hip)
//   dgrad: dX[m=(n,h,w), ci] = sum_col2 im2colT[m, col2] * W2p[ci, col2]
//          with col2 = tap*Cout + cout, im2colT gathering dY through the
//          transposed-conv map ho = (h + pad - kh) / stride (exact
//          divisions only), W2p = weight permuted to [Cin, KH*KW*Cout].
//          (The stem itself never needs it — x is data — but any other
//          odd-shaped conv does)
#include "common.h"

namespace {

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int GEMM_TPB = 256;
constexpr int BK = 32;

__device__ __forceinline__ int xcd_swz(int bid, int nwg) {
  constexpr int NXCD = 8;
  if (nwg < NXCD) return bid;
  int xcd = bid % NXCD, idx = bid / NXCD;
  int q = nwg / NXCD, r = nwg % NXCD;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

struct StemGeom {
  int H, W, Hout, Wout;    // input / output spatial
  int KH, KW, Cin;         // filter
  int stride, pad;         // along h (and along w for dgrad)
  int sw, pw;              // forward stride / left padding along w
  int Kpad;                // padded im2col K (multiple of 32)
};

// per-row (m) decode, hoisted out of the per-element gather: output pixel ->
// input-space base coordinates
struct StemCoord {
  long n_off;
  int hb, wb;
};

template <bool DGRAD = false>
__device__ __forceinline__ StemCoord stem_decode(long m, const StemGeom& g) {
  StemCoord u;
  long t = m;
  if (DGRAD) {  // m ranges over INPUT pixels; gather reads dY [Hout,Wout]
    const int w = (int)(t % g.W); t /= g.W;
    const int h = (int)(t % g.H); t /= g.H;
    u.n_off = t * (long)g.Hout * g.Wout;
    u.hb = h + g.pad;
    u.wb = w + g.pad;
    return u;
  }
  const int wo = (int)(t % g.Wout); t /= g.Wout;
  const int ho = (int)(t % g.Hout); t /= g.Hout;
  u.n_off = t * (long)g.H * g.W;
  u.hb = ho * g.stride - g.pad;
  u.wb = wo * g.sw - g.pw;
  return u;
}

// per-column decode via reciprocal multiply (integer div is ~20 cyc and was
// executed per element per K-step before)
__device__ __forceinline__ void col_decode(int col, const StemGeom& g,
                                           float inv_cin, float inv_kw,
                                           int& kh, int& kw, int& ci) {
  const int tap = (int)((float)col * inv_cin + 1e-4f);
  ci = col - tap * g.Cin;
  kh = (int)((float)tap * inv_kw + 1e-4f);
  kw = tap - kh * g.KW;
}

// element gather using hoisted row coords (DGRAD: g.Cin holds the conv's
// Cout — the channel count of the gathered dY rows)
template <bool DGRAD = false>
__device__ __forceinline__ long stem_elem(const StemCoord& u, int col,
                                          const StemGeom& g, float inv_cin,
                                          float inv_kw) {
  if (col >= g.KH * g.KW * g.Cin) return -1;  // K padding
  int kh, kw, ci;
  col_decode(col, g, inv_cin, inv_kw, kh, kw, ci);
  if (DGRAD) {
    int ho2 = u.hb - kh, wo2 = u.wb - kw;
    if (g.stride > 1) {
      if (ho2 % g.stride || wo2 % g.stride) return -1;
      ho2 /= g.stride;
      wo2 /= g.stride;
    }
    if (ho2 < 0 || ho2 >= g.Hout || wo2 < 0 || wo2 >= g.Wout) return -1;
    return (u.n_off + (long)ho2 * g.Wout + wo2) * g.Cin + ci;
  }
  const int h = u.hb + kh, w = u.wb + kw;
  if (h < 0 || h >= g.H || w < 0 || w >= g.W) return -1;
  return (u.n_off + (long)h * g.W + w) * g.Cin + ci;
}

// stage a [128 m][32 col] im2col tile into LDS (per-element gather with
// hoisted per-row decode — uc[] is precomputed once per kernel)
template <bool DGRAD = false>
__device__ __forceinline__ void stage_im2col(
    const bf16* __restrict__ x, const StemCoord* uc, const bool* valid,
    int c0, const StemGeom& g, float inv_cin, float inv_kw, bf16* lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int rnd = 0; rnd < 2; ++rnd) {
    const int unit = rnd * GEMM_TPB + t;  // 4 units of 8 cols per m-row
    const int cc0 = c0 + (unit & 3) * 8;
    bf16 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      long idx = valid[rnd]
                     ? stem_elem<DGRAD>(uc[rnd], cc0 + j, g, inv_cin, inv_kw)
                     : -1;
      v[j] = idx < 0 ? bf16(0.f) : x[idx];
    }
    *(Pack<bf16, 8>*)(lds + unit * 8) = *(Pack<bf16, 8>*)v;
  }
}

template <int ROWS = 128>
__device__ __forceinline__ void stage_rows(
    const bf16* __restrict__ gsrc, long ld, long row0, long rows, long koff,
    bf16* lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int rnd = 0; rnd < ROWS / 64; ++rnd) {
    int unit = rnd * GEMM_TPB + t;
    long row = row0 + (unit >> 2);
    if (row >= rows) row = rows - 1;
    const bf16* src = gsrc + row * ld + koff + (unit & 3) * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(lds + unit * 8), 16,
        0, 0);
  }
}


// Cin==8 fast path (the channel-padded stem): one 16 B unit == one tap's
// 8 channels, so the A tile stages via global_load_lds with a per-unit
// tap-gathered source row — same structure as conv3x3.hip's stage, no
// per-element scalar gather (the r1 elem-gather fwd measured 1.2 ms/step
// at b512, VALU-bound).
__device__ __forceinline__ void stage_im2col8(
    const bf16* __restrict__ x, const StemCoord* uc, const bool* valid,
    int c0, const StemGeom& g, const bf16* __restrict__ zp, bf16* lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int rnd = 0; rnd < 2; ++rnd) {
    const int unit = rnd * GEMM_TPB + t;  // 4 units (taps) per m-row
    const int tap = (c0 >> 3) + (unit & 3);
    const bf16* src = zp;
    if (valid[rnd] && tap < g.KH * g.KW) {
      const int kh = tap / g.KW, kw = tap - (tap / g.KW) * g.KW;
      const int h = uc[rnd].hb + kh, w = uc[rnd].wb + kw;
      if (h >= 0 && h < g.H && w >= 0 && w < g.W)
        src = x + (uc[rnd].n_off + (long)h * g.W + w) * 8;
    }
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(lds + unit * 8), 16,
        0, 0);
  }
}

// ROW4 staging (Cin == 8, KW == 4, Kpad == KH*32 — the width
// space-to-depth stem): K-step ks is exactly kernel row ks, and its 4
// units are the 4 consecutive 16 B pixel groups wb..wb+3 of input row
// hb + ks, i.e. 64 contiguous bytes.  A unit's column is fixed for the
// whole K loop, so its address base and its left/right bounds test are
// decoded once (StemRow) and the loop only steps the row: no division.
struct StemRow {
  long base;  // element-row index of (n, hb, wb + unit) — may be off-image
  int hb;
  bool wok;   // row valid and column inside [0, W)
};

__device__ __forceinline__ void stage_row4(
    const bf16* __restrict__ x, const StemRow* ur, int ks, const StemGeom& g,
    const bf16* __restrict__ zp, bf16* lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int rnd = 0; rnd < 2; ++rnd) {
    const int unit = rnd * GEMM_TPB + t;
    const int h = ur[rnd].hb + ks;
    const bf16* src = zp;
    if (ur[rnd].wok && h >= 0 && h < g.H)
      src = x + (ur[rnd].base + (long)ks * g.W) * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(lds + unit * 8), 16,
        0, 0);
  }
}

// DGRAD instantiation computes dX[m, cin] from gathered dY rows and the
// permuted weight; operand roles mirror fwd exactly.
// NT: output-tile width — 64 (Cout <= 64) runs a 2m x 2n wave grid of 4x2
// fragments over [128m x 64n] with a half-size B stage, like conv3x3's.
// stats != nullptr: also emit the BN-statistics partials [nbm][2*Cout]
// from the fp32 accumulator (conv_epilogue_stats).
// DB: double-buffered K-loop (gemm.hip pattern — stage ks+1's tiles while
// ks computes, one barrier per chunk), AMDTRAIN_STEM_DB=0 reverts.
// WIDE: the wide-store C epilogue and its B-row map (common.h); epi is the
// runtime mode of the narrow one (AMDTRAIN_EPILOGUE 0 / 1).
template <bool DGRAD = false, bool C8 = false, bool DB = false, int NT = 128,
          bool ROW4 = false, bool WIDE = false>
__global__ void __launch_bounds__(GEMM_TPB, 2)
conv_generic_fwd_kernel(const bf16* __restrict__ x,
                        const bf16* __restrict__ W2, bf16* __restrict__ Y,
                        long M, int Cout, StemGeom g, int nbm, int nbn,
                        const bf16* __restrict__ zp,
                        float* __restrict__ stats, int epi) {
  static_assert(!ROW4 || (C8 && !DGRAD), "ROW4 is a C8 forward staging");
  constexpr int STG = (128 + NT) * BK;  // one A+B stage
  constexpr int NFR = NT / 32;          // n fragments per wave
  __shared__ bf16 SMEM[(DB ? 2 : 1) * STG];
  const int bid = xcd_swz(blockIdx.x, nbm * nbn);
  const int bm = bid / nbn, bn = bid % nbn;
  const long m0 = (long)bm * 128, n0 = (long)bn * NT;
  const int t = threadIdx.x;
  const int wave = t / AMD_WAVE, lane = t % AMD_WAVE;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * (NT / 2);
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[4][NFR];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NFR; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const float inv_cin = 1.f / g.Cin, inv_kw = 1.f / g.KW;
  StemCoord uc[2];
  bool valid[2];
#pragma unroll
  for (int rnd = 0; rnd < 2; ++rnd) {
    long m = m0 + (((rnd * GEMM_TPB) + t) >> 2);
    valid[rnd] = m < M;
    uc[rnd] = stem_decode<DGRAD>(valid[rnd] ? m : M - 1, g);
  }
  StemRow ur[2];
  if (ROW4) {
#pragma unroll
    for (int rnd = 0; rnd < 2; ++rnd) {
      const int w = uc[rnd].wb + (t & 3);  // unit & 3 == t & 3
      ur[rnd].hb = uc[rnd].hb;
      ur[rnd].wok = valid[rnd] && w >= 0 && w < g.W;
      ur[rnd].base = uc[rnd].n_off + (long)uc[rnd].hb * g.W + w;
    }
  }

  const int ksteps = g.Kpad / BK;
  auto stage = [&](int ks, bf16* as) {
    if (ROW4)
      stage_row4(x, ur, ks, g, zp, as);
    else if (C8)
      stage_im2col8(x, uc, valid, ks * BK, g, zp, as);
    else
      stage_im2col<DGRAD>(x, uc, valid, ks * BK, g, inv_cin, inv_kw, as);
    stage_rows<NT>(W2, g.Kpad, n0, Cout, ks * BK, as + 128 * BK);
  };
  auto compute = [&](const bf16* as) {
    const bf16* bs = as + 128 * BK;
    bf16x8 a[4], b[NFR];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      a[i] = *(const bf16x8*)&as[(wm + i * 16 + fr) * BK + fq * 8];
#pragma unroll
    for (int j = 0; j < NFR; ++j)
      b[j] = *(const bf16x8*)
          &bs[(wn + epi_col<WIDE>(j, fr)) * BK + fq * 8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NFR; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[i], b[j], acc[i][j], 0, 0, 0);
  };
  if (DB) {
    constexpr int HB = STG;
    if (ksteps > 0) stage(0, SMEM);
    for (int ks = 0; ks < ksteps; ++ks) {
      bf16* const as = SMEM + (ks & 1) * HB;
      __syncthreads();  // implicit vmcnt(0) drains this chunk's DMA
      if (ks + 1 < ksteps) stage(ks + 1, SMEM + ((ks + 1) & 1) * HB);
      compute(as);
    }
  } else {
    for (int ks = 0; ks < ksteps; ++ks) {
      __syncthreads();
      stage(ks, SMEM);
      __syncthreads();
      compute(SMEM);
    }
  }
  epi_store_bf16<NFR, NFR, WIDE>(Y, Cout, m0, M, n0, Cout, wm, wn, fr, fq,
                                 &acc[0][0], epi);
  if (stats != nullptr)
    conv_epilogue_stats<NT, WIDE>(stats, (const float*)acc, m0, M, n0, Cout,
                                  bm, wm, wn, fr, fq, SMEM);
}

// stride_w == 0 / pad_w < 0 / Hout, Wout == 0: same as along h / symmetric
// padding.  Explicit output dims serve asymmetric padding (only the top /
// left amounts enter the gather; the bottom / right are implied).
static StemGeom make_geom(long H, long W, long KH, long KW, long Cin,
                          long stride, long pad, long stride_w = 0,
                          long pad_w = -1, long Hout = 0, long Wout = 0) {
  StemGeom g;
  g.H = (int)H; g.W = (int)W;
  g.sw = (int)(stride_w > 0 ? stride_w : stride);
  g.pw = (int)(pad_w >= 0 ? pad_w : pad);
  g.Hout = (int)(Hout > 0 ? Hout : (H + 2 * pad - KH) / stride + 1);
  g.Wout = (int)(Wout > 0 ? Wout : (W + 2 * g.pw - KW) / g.sw + 1);
  g.KH = (int)KH; g.KW = (int)KW; g.Cin = (int)Cin;
  g.stride = (int)stride; g.pad = (int)pad;
  int K = (int)(KH * KW * Cin);
  g.Kpad = (K + 31) / 32 * 32;
  return g;
}

// the double-buffered C8 forward variants (the stem) also exist with the
// wide-store epilogue (wide: AMDTRAIN_EPILOGUE=2 and Cout % 8 == 0)
template <bool DGRAD, bool C8, bool DBUF, int NT = 128, bool ROW4 = false>
static void stem_launch(int grid, hipStream_t stream, const bf16* x,
                        const bf16* w2, bf16* y, long M, int Cout,
                        const StemGeom& g, int nbm, int nbn, const bf16* zp,
                        float* stats, bool wide, int epi) {
  if constexpr (C8 && DBUF && !DGRAD) {
    if (wide) {
      conv_generic_fwd_kernel<DGRAD, C8, DBUF, NT, ROW4, true>
          <<<grid, GEMM_TPB, 0, stream>>>(x, w2, y, M, Cout, g, nbm, nbn, zp,
                                          stats, epi);
      return;
    }
  }
  conv_generic_fwd_kernel<DGRAD, C8, DBUF, NT, ROW4, false>
      <<<grid, GEMM_TPB, 0, stream>>>(x, w2, y, M, Cout, g, nbm, nbn, zp,
                                      stats, epi);
}

static at::Tensor stem_zero_page(const at::Tensor& like) {
  static thread_local at::Tensor zp;
  if (!zp.defined() || zp.device() != like.device())
    zp = at::zeros({16}, like.options().dtype(at::kBFloat16));
  return zp;
}

}  // namespace


// AMDTRAIN_STEM_DB=0 reverts to the single-buffer K-loop
static bool stem_db_enabled() {
  static const bool v = []() {
    const char* e = std::getenv("AMDTRAIN_STEM_DB");
    return !(e && e[0] == '0');
  }();
  return v;
}

// x2d: [N*H*W, Cin] bf16 NHWC rows; w2: [Cout, Kpad] (host-padded).
// Cin == 8 (channel-padded stem) takes the vectorized tap-gather staging;
// with KW == 4 and no K padding on top (the width space-to-depth stem) the
// division-free row staging.  tile64 runs either Cin == 8 staging on the
// 64-wide n-tile when Cout <= 64 (per-element K order unchanged, so y is
// identical to the 128-wide tile's).  want_stats adds the BN-statistics
// partials [nbm][2*Cout].
static std::vector<at::Tensor> conv_generic_fwd_impl(
    at::Tensor x2d, long Nn, long H, long W, long KH, long KW, long stride,
    long pad, at::Tensor w2, long stride_w, long pad_w, long Hout, long Wout,
    bool want_stats, bool tile64, long epi) {
  TORCH_CHECK(x2d.is_cuda() && x2d.scalar_type() == at::kBFloat16);
  TORCH_CHECK(x2d.is_contiguous() && w2.is_contiguous());
  long Cin = x2d.size(1), Cout = w2.size(0);
  TORCH_CHECK(x2d.size(0) == Nn * H * W);
  auto g = make_geom(H, W, KH, KW, Cin, stride, pad, stride_w, pad_w, Hout,
                     Wout);
  TORCH_CHECK(w2.size(1) == g.Kpad, "weight must be K-padded to ", g.Kpad);
  long M = Nn * g.Hout * g.Wout;
  auto y = at::empty({M, Cout}, x2d.options());
  int nbm = (int)((M + 127) / 128), nbn = (int)((Cout + 127) / 128);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto zp = stem_zero_page(x2d);
  const bool db = stem_db_enabled();
  const bool c8 = Cin == 8 && g.Kpad == (KH * KW * 8 + 31) / 32 * 32;
  const bool row4 = c8 && KW == 4 && g.Kpad == KH * 32;
  const bool t64 = tile64 && Cout <= 64;
  TORCH_CHECK(!want_stats || c8, "conv_generic stats need the C8 kernel");
  at::Tensor stats;
  float* sp = nullptr;
  if (want_stats) {
    stats = at::empty({nbm, 2 * Cout}, x2d.options().dtype(at::kFloat));
    sp = stats.data_ptr<float>();
  }
  const bf16* xp = (const bf16*)x2d.const_data_ptr();
  const bf16* wp = (const bf16*)w2.const_data_ptr();
  const bf16* zpp = (const bf16*)zp.const_data_ptr();
  bf16* yp = (bf16*)y.data_ptr();
  const int grid = nbm * nbn, co = (int)Cout, ep = epi_mode(epi, 2);
  const bool wide = ep >= 2 && Cout % 8 == 0;
  if (c8 && row4 && t64 && db)
    stem_launch<false, true, true, 64, true>(grid, stream, xp, wp, yp, M, co,
                                             g, nbm, nbn, zpp, sp, wide, ep);
  else if (c8 && row4 && t64)
    stem_launch<false, true, false, 64, true>(grid, stream, xp, wp, yp, M, co,
                                              g, nbm, nbn, zpp, sp, wide, ep);
  else if (c8 && t64 && db)  // 49-tap stem: same K order, half the MFMAs
    stem_launch<false, true, true, 64>(grid, stream, xp, wp, yp, M, co, g,
                                       nbm, nbn, zpp, sp, wide, ep);
  else if (c8 && t64)
    stem_launch<false, true, false, 64>(grid, stream, xp, wp, yp, M, co, g,
                                        nbm, nbn, zpp, sp, wide, ep);
  else if (c8 && db)
    stem_launch<false, true, true>(grid, stream, xp, wp, yp, M, co, g, nbm,
                                   nbn, zpp, sp, wide, ep);
  else if (c8)
    stem_launch<false, true, false>(grid, stream, xp, wp, yp, M, co, g, nbm,
                                    nbn, zpp, sp, wide, ep);
  else if (db)
    stem_launch<false, false, true>(grid, stream, xp, wp, yp, M, co, g, nbm,
                                    nbn, zpp, sp, wide, ep);
  else
    stem_launch<false, false, false>(grid, stream, xp, wp, yp, M, co, g, nbm,
                                     nbn, zpp, sp, wide, ep);
  CHECK_CUDA_OK();
  if (want_stats) return {y, stats};
  return {y};
}

at::Tensor conv_generic_fwd(at::Tensor x2d, long Nn, long H, long W,
                            long KH, long KW, long stride, long pad,
                            at::Tensor w2, long stride_w, long pad_w,
                            long Hout, long Wout, bool tile64, long epi) {
  return conv_generic_fwd_impl(x2d, Nn, H, W, KH, KW, stride, pad, w2,
                               stride_w, pad_w, Hout, Wout, false, tile64,
                               epi)[0];
}

std::vector<at::Tensor> conv_generic_fwd_stats(
    at::Tensor x2d, long Nn, long H, long W, long KH, long KW, long stride,
    long pad, at::Tensor w2, long stride_w, long pad_w, long Hout, long Wout,
    bool tile64, long epi) {
  return conv_generic_fwd_impl(x2d, Nn, H, W, KH, KW, stride, pad, w2,
                               stride_w, pad_w, Hout, Wout, true, tile64,
                               epi);
}

// dy2d: [N*Hout*Wout, Cout]; w2p: [Cin, pad32(KH*KW*Cout)] (weight permuted
// to cin-major, host-padded).  Returns dx2d [N*H*W, Cin].
at::Tensor conv_generic_dgrad(at::Tensor dy2d, at::Tensor w2p, long Nn,
                              long H, long W, long KH, long KW, long stride,
                              long pad) {
  TORCH_CHECK(dy2d.is_cuda() && dy2d.scalar_type() == at::kBFloat16);
  long Cout = dy2d.size(1), Cin = w2p.size(0);
  // geometry carries the FORWARD conv dims; g.Cin = Cout (gathered rows)
  auto g = make_geom(H, W, KH, KW, Cout, stride, pad);
  TORCH_CHECK(w2p.size(1) == g.Kpad, "w2p must be K-padded to ", g.Kpad);
  TORCH_CHECK(dy2d.size(0) == Nn * g.Hout * g.Wout);
  long M = Nn * H * W;
  auto dx = at::empty({M, Cin}, dy2d.options());
  int nbm = (int)((M + 127) / 128), nbn = (int)((Cin + 127) / 128);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto zp = stem_zero_page(dy2d);
  if (stem_db_enabled())
    conv_generic_fwd_kernel<true, false, true>
        <<<nbm * nbn, GEMM_TPB, 0, stream>>>(
            (const bf16*)dy2d.const_data_ptr(),
            (const bf16*)w2p.const_data_ptr(), (bf16*)dx.data_ptr(), M,
            (int)Cin, g, nbm, nbn, (const bf16*)zp.const_data_ptr(),
            nullptr, 0);
  else
    conv_generic_fwd_kernel<true><<<nbm * nbn, GEMM_TPB, 0, stream>>>(
        (const bf16*)dy2d.const_data_ptr(),
        (const bf16*)w2p.const_data_ptr(), (bf16*)dx.data_ptr(), M,
        (int)Cin, g, nbm, nbn, (const bf16*)zp.const_data_ptr(), nullptr,
        0);
  CHECK_CUDA_OK();
  return dx;
}
