// Per-group MFMA kernel for grouped 3x3 convolutions (NHWC bf16, pad 1,
// stride 1/2, Cin == Cout == C, S = C / groups in {4, 8, 16, 32}) for gfx950:
// forward (with the BN-statistics partials) and input gradient.
//
// The dense conv3x3 kernels serve a grouped conv "banded": a 64-wide output
// tile walks a 64-channel K window of which only S channels carry weight.
// Here the MFMA tile sits on a channel WINDOW of CW = 16 (S <= 16) or 32
// (S = 32) channels, whose outputs depend on the same CW inputs only:
//
//   Y[pixel, window] = sum_{tap, c in window} X[pixel + tap, c] * Wd[n, tap, c]
//
// one GEMM per window with N = CW and K = 9 * CW, (tap, channel) ordered, Wd
// block-diagonal over the CW / S groups of the window.
//
//  * Block = 4 waves = one tile of TH x 16 output pixels of one image x a
//    slab of 64 channels.  The input halo tile of the slab is staged once in
//    LDS, out-of-image pixels as zeros: that is all the padding handling.
//  * mfma_f32_16x16x32_bf16: lane (fq = lane>>4, fr = lane&15) supplies 8
//    consecutive k of row fr.  An m-fragment is 16 consecutive output
//    columns of one row.  CW = 16: a K-step is two taps x 16 channels, the
//    lane's operand is ONE 16-byte LDS read — pixel(fr) shifted by tap
//    2t + (fq>>1), channel half fq&1 of the window; five K-steps, the tenth
//    tap is fed as zeros (and its packed weight is zero).  CW = 32: a K-step
//    is one tap, nine steps, the A fragment serves two n-fragments.
//  * Weights sit in VGPRs for the whole block (20 / 72 per lane), loaded as
//    16-byte runs from a buffer packed once per call by gconv_pack_kernel:
//    [window][kstep][n-fragment][lane][8].
//  * CW = 16: wave = window, all TH m-fragments.  CW = 32: two waves share a
//    window and split the m-fragments.
//  * LDS pixel pitch 144 B (128 + 16): the sixteen 16-byte reads of a
//    fragment row at stride 1 start 9 sixteen-byte units apart, 9 odd, so
//    they cover all 64 banks once.
//  * Epilogue: quad transpose (common.h) of pairs of fragments -> 8-byte
//    writes into the (now dead) LDS tile as [pixel][64 ch], then 16-byte
//    global stores, 128 contiguous bytes per pixel.
//  * dgrad = the same kernel over dY with the dgrad-packed weight and the
//    mirrored gather (ho = h + 1 - kh).  At stride 2 the dY tile an input
//    tile reaches is staged and taps of the wrong parity are fed zeros.
//  * Statistics: per-channel (sum, sum of squares) of the fp32 accumulators
//    over the block's valid pixels, reduced in registers over (fragment, r),
//    then over the four fq lane groups; row = pixel tile, [nb][2*C].  No
//    atomics, one writer per element, fixed order.
#include "common.h"

// the compiler's packed fp32 forms are kept out of this file's kernels
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) short;

constexpr int GC_TPB = 256;
constexpr int GC_SLAB = 64;    // channels per block
constexpr int GC_TW = 16;      // tile width = one m-fragment
constexpr int GC_PITCH = 144;  // LDS bytes per pixel

enum { GC_FWD1 = 0, GC_FWD2 = 1, GC_DG1 = 2, GC_DG2 = 3 };

// TH x 16 written pixels; LH x LW staged pixels of the tensor read
template <int MODE> struct GcTile {
  static constexpr int TH = MODE == GC_FWD2 ? 4 : 8;
  static constexpr int LH = MODE == GC_FWD2  ? 2 * TH + 1
                            : MODE == GC_DG2 ? TH / 2 + 1
                                             : TH + 2;
  static constexpr int LW = MODE == GC_FWD2  ? 2 * GC_TW + 1
                            : MODE == GC_DG2 ? GC_TW / 2 + 1
                                             : GC_TW + 2;
};

struct GcGeom {
  int C;
  int SH, SW;  // tensor read (x, or dY for dgrad)
  int OH, OW;  // tensor written
  int tilesH, tilesW, nslab;
};

// staged-tile pixel that output pixel (row i, column fr) of the tile reads
// for tap (kh, kw); ok = false: the tap does not reach it (feed zeros)
template <int MODE>
__device__ __forceinline__ int gc_pixel(int i, int fr, int kh, int kw,
                                        bool& ok) {
  int lr, lc;
  ok = true;
  if (MODE == GC_FWD1) {
    lr = i + kh;
    lc = fr + kw;
  } else if (MODE == GC_FWD2) {
    lr = 2 * i + kh;
    lc = 2 * fr + kw;
  } else if (MODE == GC_DG1) {
    lr = i + 2 - kh;
    lc = fr + 2 - kw;
  } else {  // tile origin is even: parity of h + 1 - kh is that of i + 1 - kh
    const int er = i + 1 - kh, ec = fr + 1 - kw;
    ok = !((er | ec) & 1);
    lr = max(er, 0) >> 1;
    lc = max(ec, 0) >> 1;
  }
  return lr * GcTile<MODE>::LW + lc;
}

template <int CW, int MODE>
__global__ void __launch_bounds__(GC_TPB, 2)
gconv3x3_kernel(const bf16* __restrict__ src, const bf16* __restrict__ packed,
                bf16* __restrict__ dst, float* __restrict__ stats, GcGeom g) {
  using T = GcTile<MODE>;
  constexpr int TH = T::TH, LH = T::LH, LW = T::LW;
  constexpr int KS = CW == 16 ? 5 : 9, NJ = CW / 16;
  constexpr int NFRAG = CW == 16 ? TH : TH / 2;  // m-fragments per wave
  constexpr int NACC = NFRAG * NJ;
  constexpr int NPIX = LH * LW, OPIX = TH * GC_TW;
  __shared__ __attribute__((aligned(16))) char lds[(NPIX > OPIX ? NPIX : OPIX) *
                                                   GC_PITCH];
  __shared__ float red[CW == 32 ? 2 * GC_SLAB : 1];

  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int fr = lane & 15, fq = lane >> 4;
  int bid = blockIdx.x;
  const int slab = bid % g.nslab;
  bid /= g.nslab;
  const int tile = bid;  // statistics row
  const int tw = bid % g.tilesW;
  bid /= g.tilesW;
  const int th = bid % g.tilesH, n = bid / g.tilesH;
  const int c0 = slab * GC_SLAB, h0 = th * TH, w0 = tw * GC_TW;
  // the wave's window: first channel inside the slab, first m-fragment
  const int wch = CW == 16 ? wave * 16 : (wave >> 1) * 32;
  const int i0 = CW == 16 ? 0 : (wave & 1) * NFRAG;
  const bool active = c0 + wch < g.C;  // last slab may be part full

  bf16x8 bw[KS][NJ];
  if (active) {
    const bf16x8* wp = (const bf16x8*)packed +
                       (long)((c0 + wch) / CW) * (KS * NJ * 64) + lane;
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int j = 0; j < NJ; ++j) bw[k][j] = wp[(k * NJ + j) * 64];
  }

  // ---- stage the halo tile: 8 threads x 16 B per pixel --------------------
  {
    const int sr0 = MODE == GC_FWD2 ? 2 * h0 - 1
                    : MODE == GC_DG2 ? h0 / 2
                                     : h0 - 1;
    const int sc0 = MODE == GC_FWD2 ? 2 * w0 - 1
                    : MODE == GC_DG2 ? w0 / 2
                                     : w0 - 1;
    const int cu = t & 7;
    const bool cok = c0 + cu * 8 < g.C;
    const bf16* sbase = src + (long)n * g.SH * g.SW * g.C + c0 + cu * 8;
    constexpr int NLD = (NPIX + 31) / 32;
    uint4 v[NLD];
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int p = (t >> 3) + k * 32;
      const int sr = sr0 + p / LW, sc = sc0 + p % LW;
      const bool ok = p < NPIX && cok && sr >= 0 && sr < g.SH && sc >= 0 &&
                      sc < g.SW;
      v[k] = make_uint4(0, 0, 0, 0);
      if (ok) v[k] = *(const uint4*)(sbase + ((long)sr * g.SW + sc) * g.C);
    }
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int p = (t >> 3) + k * 32;
      if (p < NPIX) *(uint4*)(lds + p * GC_PITCH + cu * 16) = v[k];
    }
  }
  __syncthreads();

  // ---- K loop: everything unrolled, A straight from the halo tile ---------
  epi_f32x4 acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; ++a) acc[a] = {0.f, 0.f, 0.f, 0.f};
  if (active) {
    const char* abase = lds + (wch + (CW == 16 ? (fq & 1) * 8 : fq * 8)) * 2;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int tap = CW == 16 ? 2 * k + (fq >> 1) : k;
      const bool tap_ok = tap < 9;
      const int tp = tap_ok ? tap : 8;
      const int kh = tp / 3, kw = tp - 3 * kh;
#pragma unroll
      for (int ii = 0; ii < NFRAG; ++ii) {
        bool ok;
        const int pix = gc_pixel<MODE>(i0 + ii, fr, kh, kw, ok);
        bf16x8 a = *(const bf16x8*)(abase + pix * GC_PITCH);
        if (!(ok && tap_ok)) a = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[ii * NJ + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, bw[k][j], acc[ii * NJ + j], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // the halo tile is dead: reuse it as [pixel][64 ch]

  float s1[NJ] = {}, s2[NJ] = {};
  if (active) {
    // accumulator a = fragment (i0 + a / NJ), channels wch + (a % NJ)*16 + fr;
    // after the transpose a lane holds pixel fq*4 + (fr&3), 4 channels
#pragma unroll
    for (int p = 0; p < NACC / 2; ++p) {
      uint4 run[1];
      epi_quad_transpose<2>(acc + 2 * p, run, fr);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int a = 2 * p + q;
        const int pixel = (i0 + a / NJ) * 16 + fq * 4 + (fr & 3);
        const int ch = wch + (a % NJ) * 16 + (fr >> 2) * 4;
        *(uint2*)(lds + pixel * GC_PITCH + ch * 2) =
            q ? make_uint2(run[0].z, run[0].w) : make_uint2(run[0].x, run[0].y);
      }
    }
    if (stats != nullptr) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        s1[j] = 0.f;
        s2[j] = 0.f;
#pragma unroll
        for (int ii = 0; ii < NFRAG; ++ii)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool ok = h0 + i0 + ii < g.OH && w0 + fq * 4 + r < g.OW;
            const float x = ok ? acc[ii * NJ + j][r] : 0.f;
            s1[j] += x;
            s2[j] += x * x;
          }
#pragma unroll
        for (int off = 32; off >= 16; off >>= 1) {
          s1[j] += __shfl_down(s1[j], off, AMD_WAVE);
          s2[j] += __shfl_down(s2[j], off, AMD_WAVE);
        }
        if (CW == 32 && (wave & 1) && fq == 0) {
          red[(wch + j * 16 + fr) * 2] = s1[j];
          red[(wch + j * 16 + fr) * 2 + 1] = s2[j];
        }
      }
    }
  }
  __syncthreads();

  if (stats != nullptr && active && fq == 0 && (CW == 16 || !(wave & 1))) {
    float* srow = stats + (long)tile * 2 * g.C + c0 + wch + fr;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float a1 = s1[j], a2 = s2[j];
      if (CW == 32) {  // fragments of the even wave first, then the odd one's
        a1 += red[(wch + j * 16 + fr) * 2];
        a2 += red[(wch + j * 16 + fr) * 2 + 1];
      }
      srow[j * 16] = a1;
      srow[g.C + j * 16] = a2;
    }
  }

  // ---- 16-byte stores, 128 contiguous bytes per pixel ----------------------
  bf16* dbase = dst + (long)n * g.OH * g.OW * g.C + c0;
#pragma unroll
  for (int k = 0; k < OPIX * 8 / GC_TPB; ++k) {
    const int u = t + k * GC_TPB, p = u >> 3, cu = u & 7;
    const int h = h0 + (p >> 4), w = w0 + (p & 15);
    if (h < g.OH && w < g.OW && c0 + cu * 8 < g.C)
      *(uint4*)(dbase + ((long)h * g.OW + w) * g.C + cu * 8) =
          *(const uint4*)(lds + p * GC_PITCH + cu * 16);
  }
}

// packed[window][kstep][n-fragment][lane][8] from the grouped weight
// w[C][S][3][3] (any strides).  Entry (n, tap, k), n / k the window's output /
// reduction channel: forward W[n][k % S][tap]; dgrad (n = input channel,
// k = output channel) W[k][n % S][tap], tap index kept — the dgrad gather
// already encodes the rotation.  Zero across groups and for the tenth tap.
template <int CW>
__global__ void __launch_bounds__(AMD_TPB)
gconv_pack_kernel(const bf16* __restrict__ w, bf16* __restrict__ out, int C,
                  int S, long s0, long s1, long s2, long s3, bool dgrad) {
  constexpr int KS = CW == 16 ? 5 : 9, NJ = CW / 16;
  const long total = (long)(C / CW) * KS * NJ * 64 * 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long r = i;
    const int e = (int)(r % 8); r /= 8;
    const int lane = (int)(r % 64); r /= 64;
    const int j = (int)(r % NJ); r /= NJ;
    const int ks = (int)(r % KS); r /= KS;
    const int win = (int)r;
    const int fr = lane & 15, fq = lane >> 4;
    const int tap = CW == 16 ? 2 * ks + (fq >> 1) : ks;
    const int nc = win * CW + j * 16 + fr;
    const int kc = win * CW + (CW == 16 ? (fq & 1) * 8 : fq * 8) + e;
    bf16 val = __float2bfloat16(0.f);
    if (tap < 9 && nc / S == kc / S) {
      const int co = dgrad ? kc : nc, ci = (dgrad ? nc : kc) % S;
      val = w[co * s0 + ci * s1 + (tap / 3) * s2 + (tap % 3) * s3];
    }
    out[i] = val;
  }
}

}  // namespace

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// contract shared by the entry points here and in gconv_wgrad.hip:
// C % 32 == 0, S in {4,8,16,32}
int gconv_window(long C, long groups, const char* op) {
  TORCH_CHECK(groups > 0 && C % 32 == 0 && C % groups == 0, op,
              ": C must be a multiple of 32 and of groups, got C = ", C,
              ", groups = ", groups);
  const long S = C / groups;
  TORCH_CHECK(S == 4 || S == 8 || S == 16 || S == 32, op,
              ": channels per group must be 4, 8, 16 or 32, got ", S);
  return S == 32 ? 32 : 16;
}

static long gconv_packed_numel(long C, int cw) {
  return (C / cw) * (cw == 16 ? 5 : 9) * (cw / 16) * 64 * 8;
}

at::Tensor gconv3x3_pack(at::Tensor weight, long groups, bool dgrad) {
  TORCH_CHECK(weight.is_cuda() && weight.scalar_type() == at::kBFloat16 &&
                  weight.dim() == 4 && weight.size(2) == 3 &&
                  weight.size(3) == 3,
              "gconv3x3_pack: weight must be a CUDA bf16 [C, S, 3, 3] tensor");
  const long C = weight.size(0);
  const int cw = gconv_window(C, groups, "gconv3x3_pack");
  TORCH_CHECK(weight.size(1) * groups == C,
              "gconv3x3_pack: weight is [", C, ", ", weight.size(1),
              ", 3, 3] but C / groups = ", C / groups);
  const long total = gconv_packed_numel(C, cw);
  auto out = at::empty({total}, weight.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* wp = (const bf16*)weight.const_data_ptr();
  bf16* op = (bf16*)out.data_ptr();
  const int S = (int)(C / groups);
  if (cw == 16)
    gconv_pack_kernel<16><<<amd_grid(total), AMD_TPB, 0, stream>>>(
        wp, op, (int)C, S, weight.stride(0), weight.stride(1),
        weight.stride(2), weight.stride(3), dgrad);
  else
    gconv_pack_kernel<32><<<amd_grid(total), AMD_TPB, 0, stream>>>(
        wp, op, (int)C, S, weight.stride(0), weight.stride(1),
        weight.stride(2), weight.stride(3), dgrad);
  CHECK_CUDA_OK();
  return out;
}

template <int MODE>
static void gconv_launch(int cw, const at::Tensor& src,
                         const at::Tensor& packed, at::Tensor& dst,
                         float* stats, long Nn, GcGeom g) {
  const long grid = Nn * g.tilesH * g.tilesW * g.nslab;
  TORCH_CHECK(grid < (1L << 31), "gconv3x3: too many tiles (", grid, ")");
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* sp = (const bf16*)src.const_data_ptr();
  const bf16* pp = (const bf16*)packed.const_data_ptr();
  bf16* dp = (bf16*)dst.data_ptr();
  if (cw == 16)
    gconv3x3_kernel<16, MODE><<<(int)grid, GC_TPB, 0, stream>>>(sp, pp, dp,
                                                                 stats, g);
  else
    gconv3x3_kernel<32, MODE><<<(int)grid, GC_TPB, 0, stream>>>(sp, pp, dp,
                                                                 stats, g);
  CHECK_CUDA_OK();
}

// src2d: rows of the tensor read ([Nn*SH*SW, C]); returns the geometry after
// every host check of the contract
static GcGeom gconv_check(const char* op, const at::Tensor& src2d, long Nn,
                          long SH, long SW, long OH, long OW, long stride,
                          const at::Tensor& packed, long groups, int th,
                          int* cw) {
  TORCH_CHECK(src2d.is_cuda() && src2d.scalar_type() == at::kBFloat16 &&
                  src2d.dim() == 2 && src2d.is_contiguous(),
              op, ": rows must be a contiguous CUDA bf16 [R, C] tensor");
  TORCH_CHECK(stride == 1 || stride == 2, op, ": stride must be 1 or 2, got ",
              stride);
  const long C = src2d.size(1);
  *cw = gconv_window(C, groups, op);
  TORCH_CHECK(Nn > 0 && SH > 0 && SW > 0 && src2d.size(0) == Nn * SH * SW, op,
              ": ", src2d.size(0), " rows, expected ", Nn, " x ", SH, " x ",
              SW);
  TORCH_CHECK(packed.is_cuda() && packed.device() == src2d.device() &&
                  packed.scalar_type() == at::kBFloat16 &&
                  packed.is_contiguous() &&
                  packed.numel() == gconv_packed_numel(C, *cw),
              op, ": packed weight does not match C = ", C, ", groups = ",
              groups, " (use gconv3x3_pack)");
  GcGeom g;
  g.C = (int)C;
  g.SH = (int)SH;
  g.SW = (int)SW;
  g.OH = (int)OH;
  g.OW = (int)OW;
  g.tilesH = (int)((OH + th - 1) / th);
  g.tilesW = (int)((OW + GC_TW - 1) / GC_TW);
  g.nslab = (int)((C + GC_SLAB - 1) / GC_SLAB);
  return g;
}

std::vector<at::Tensor> gconv3x3_fwd(at::Tensor x2d, long Nn, long H, long W,
                                     long stride, at::Tensor packed,
                                     long groups, bool want_stats) {
  const long Hout = (H + 2 - 3) / stride + 1, Wout = (W + 2 - 3) / stride + 1;
  int cw;
  GcGeom g = gconv_check("gconv3x3_fwd", x2d, Nn, H, W, Hout, Wout, stride,
                         packed, groups,
                         stride == 2 ? GcTile<GC_FWD2>::TH
                                     : GcTile<GC_FWD1>::TH,
                         &cw);
  auto y = at::empty({Nn * Hout * Wout, (long)g.C}, x2d.options());
  const long nb = Nn * g.tilesH * g.tilesW;
  auto stats = at::empty({want_stats ? nb : 0, 2L * g.C},
                         x2d.options().dtype(at::kFloat));
  float* sp = want_stats ? stats.data_ptr<float>() : nullptr;
  if (stride == 1)
    gconv_launch<GC_FWD1>(cw, x2d, packed, y, sp, Nn, g);
  else
    gconv_launch<GC_FWD2>(cw, x2d, packed, y, sp, Nn, g);
  if (!want_stats) stats = at::empty({0}, stats.options());
  return {y, stats};
}

at::Tensor gconv3x3_dgrad(at::Tensor dy2d, long Nn, long H, long W,
                          long stride, at::Tensor packed, long groups) {
  // H, W: the INPUT's; dy2d is [Nn*Hout*Wout, C]; returns dx2d [Nn*H*W, C]
  const long Hout = (H + 2 - 3) / stride + 1, Wout = (W + 2 - 3) / stride + 1;
  int cw;
  GcGeom g = gconv_check("gconv3x3_dgrad", dy2d, Nn, Hout, Wout, H, W, stride,
                         packed, groups, GcTile<GC_DG1>::TH, &cw);
  auto dx = at::empty({Nn * H * W, (long)g.C}, dy2d.options());
  if (stride == 1)
    gconv_launch<GC_DG1>(cw, dy2d, packed, dx, nullptr, Nn, g);
  else
    gconv_launch<GC_DG2>(cw, dy2d, packed, dx, nullptr, Nn, g);
  return dx;
}
