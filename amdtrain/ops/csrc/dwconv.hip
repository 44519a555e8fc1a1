// Depthwise 3x3 pad-1 convolution (stride 1/2), NHWC bf16, for gfx950.
//
// A depthwise 3x3 is 9 multiply-adds per output element: no inner dot
// product, nothing for the matrix cores, purely HBM-bound.  The kernels are
// vectorised stencils:
//
//  * a lane owns one 16-byte pack of 8 channels and a strip of DW_TW
//    columns of one row; consecutive lanes take consecutive channel packs
//    first, then consecutive strips, so a wave's loads are contiguous runs
//    of the NHWC row
//  * the strip's input window ((DW_TW-1)*S + 3 columns per input row) is
//    loaded once and reused by the three horizontal taps in registers
//  * the 9 x 8 weights of the lane's pack sit in registers as fp32; the
//    weight comes in tap-major [9, C] so one tap is one 16-byte load
//  * fp32 accumulation, one rounding to bf16
//  * padding by predicate: a tap outside the image is never loaded
//
// dgrad is a gather as well: stride 1 is the forward stencil with the taps
// mirrored, stride 2 sums for every input pixel only the taps whose parity
// matches (1, 2 or 4 of them).  wgrad is a two-level reduction in a fixed
// order, like the batch-norm statistics: blocks reduce fixed chunks of
// output rows into fp32 partials [P, 9, C], a second kernel collapses the
// partials in a fixed order.  P is a function of the shape alone, so the
// result is bitwise reproducible.  No atomics anywhere.
#include "common.h"

namespace {

constexpr int DW_TW = 4;      // columns per lane strip
constexpr int DW_L2E = 32;    // elements per block of the wgrad collapse
constexpr int DW_L2G = 8;     // ... and partial groups per element

using bf16 = __hip_bfloat16;
using Pk8 = Pack<bf16, 8>;

__device__ __forceinline__ void load8(const bf16* p, float f[8]) {
  Pk8 v = *reinterpret_cast<const Pk8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = to_f32<bf16>(v.v[j]);
}

__device__ __forceinline__ void load8_pred(const bf16* p, bool ok,
                                           float f[8]) {
  if (ok) {
    load8(p, f);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = 0.f;
  }
}

__device__ __forceinline__ void store8(bf16* p, const float f[8]) {
  Pk8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v.v[j] = from_f32<bf16>(f[j]);
  *reinterpret_cast<Pk8*>(p) = v;
}

// y(ho, wo) = sum_{kh,kw} x(ho*S - 1 + kh, wo*S - 1 + kw) * w[kh][kw].
// MIRROR reads tap (2-kh, 2-kw) instead: with x = dy and S = 1 that is the
// stride-1 input gradient.  One work item per lane: (row = n*Ho + ho,
// strip, pack), pack fastest.
template <int S, bool MIRROR>
__global__ __launch_bounds__(AMD_TPB) void dwconv3x3_stencil_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ w9,
    bf16* __restrict__ y, int H, int W, int Ho, int Wo, int C, int CP,
    int nstrips, long total) {
  const long idx = (long)blockIdx.x * AMD_TPB + threadIdx.x;
  if (idx >= total) return;
  const int cp = (int)(idx % CP);
  const long r = idx / CP;
  const int strip = (int)(r % nstrips);
  const long row = r / nstrips;
  const int ho = (int)(row % Ho);
  const long n = row / Ho;
  const int c0 = cp * 8;

  float wr[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t)
    load8(w9 + (long)(MIRROR ? 8 - t : t) * C + c0, wr[t]);

  float acc[DW_TW][8];
#pragma unroll
  for (int o = 0; o < DW_TW; ++o)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[o][j] = 0.f;

  constexpr int NC = (DW_TW - 1) * S + 3;  // window columns
  const int wo0 = strip * DW_TW;
  const int wi0 = wo0 * S - 1;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int hi = ho * S - 1 + kh;
    if (hi < 0 || hi >= H) continue;
    const bf16* xr = x + ((n * H + hi) * W) * C + c0;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int wi = wi0 + j;
      float xf[8];
      load8_pred(xr + (long)wi * C, wi >= 0 && wi < W, xf);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        // window column j is tap kw of output o = (j - kw) / S
        if (j - kw >= 0 && (j - kw) % S == 0 && (j - kw) / S < DW_TW) {
          const int o = (j - kw) / S;
#pragma unroll
          for (int q = 0; q < 8; ++q)
            acc[o][q] = fmaf(xf[q], wr[kh * 3 + kw][q], acc[o][q]);
        }
      }
    }
  }
  bf16* yr = y + (row * Wo) * C + c0;
#pragma unroll
  for (int o = 0; o < DW_TW; ++o)
    if (wo0 + o < Wo) store8(yr + (long)(wo0 + o) * C, acc[o]);
}

// Stride-2 input gradient: dx(h, w) = sum over the taps (kh, kw) with
// (h + 1 - kh) and (w + 1 - kw) even and the halves inside [0, Ho) x
// [0, Wo), of dy((h+1-kh)/2, (w+1-kw)/2) * w[kh][kw].  A strip starts at an
// even column w0 = 4*strip, q = w0/2:
//   w0   : kw 1 <- dy[q]          w0+1 : kw 0 <- dy[q+1], kw 2 <- dy[q]
//   w0+2 : kw 1 <- dy[q+1]        w0+3 : kw 0 <- dy[q+2], kw 2 <- dy[q+1]
// so three dy packs per matching dy row serve the four pixels.
__global__ __launch_bounds__(AMD_TPB) void dwconv3x3_dgrad_s2_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ w9,
    bf16* __restrict__ dx, int H, int W, int Ho, int Wo, int C, int CP,
    int nstrips, long total) {
  static_assert(DW_TW == 4, "tap table below is written for 4 columns");
  const long idx = (long)blockIdx.x * AMD_TPB + threadIdx.x;
  if (idx >= total) return;
  const int cp = (int)(idx % CP);
  const long r = idx / CP;
  const int strip = (int)(r % nstrips);
  const long row = r / nstrips;  // n*H + h
  const int h = (int)(row % H);
  const long n = row / H;
  const int c0 = cp * 8;

  float wr[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t) load8(w9 + (long)t * C + c0, wr[t]);

  float acc[DW_TW][8];
#pragma unroll
  for (int o = 0; o < DW_TW; ++o)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[o][j] = 0.f;

  const int w0 = strip * DW_TW;
  const int q = w0 >> 1;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int t = h + 1 - kh;
    if (t < 0 || (t & 1)) continue;
    const int ho = t >> 1;
    if (ho >= Ho) continue;
    const bf16* gr = dy + ((n * Ho + ho) * Wo) * C + c0;
    float d0[8], d1[8], d2[8];
    load8_pred(gr + (long)q * C, q < Wo, d0);
    load8_pred(gr + (long)(q + 1) * C, q + 1 < Wo, d1);
    load8_pred(gr + (long)(q + 2) * C, q + 2 < Wo, d2);
    const float* k0 = wr[kh * 3 + 0];
    const float* k1 = wr[kh * 3 + 1];
    const float* k2 = wr[kh * 3 + 2];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[0][j] = fmaf(d0[j], k1[j], acc[0][j]);
      acc[1][j] = fmaf(d1[j], k0[j], acc[1][j]);
      acc[1][j] = fmaf(d0[j], k2[j], acc[1][j]);
      acc[2][j] = fmaf(d1[j], k1[j], acc[2][j]);
      acc[3][j] = fmaf(d2[j], k0[j], acc[3][j]);
      acc[3][j] = fmaf(d1[j], k2[j], acc[3][j]);
    }
  }
  bf16* xr = dx + (row * W) * C + c0;
#pragma unroll
  for (int o = 0; o < DW_TW; ++o)
    if (w0 + o < W) store8(xr + (long)(w0 + o) * C, acc[o]);
}

// Weight gradient, level 1.  dw[kh][kw][c] = sum over (n, ho, wo) of
// dy(n, ho, wo, c) * x(n, ho*S-1+kh, wo*S-1+kw, c).
// Block (chunk = blockIdx.x, pack group = blockIdx.y): threads are
// (slot, pack) with pack fastest, CPB packs and nslots = 256 / CPB slots.
// The chunk is RC consecutive output rows (n*Ho + ho); slot s walks its
// strips s, s + nslots, ... in order with 9 x 8 fp32 accumulators, then the
// slots of a pack are summed in slot order through LDS, one tap at a time.
template <int S>
__global__ __launch_bounds__(AMD_TPB) void dwconv3x3_wgrad_part_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ x,
    float* __restrict__ part, int H, int W, int Ho, int Wo, int C, int CP,
    int CPB, int nslots, int nstrips, int RC, long NR) {
  __shared__ float red[AMD_TPB * 8];
  const int t = threadIdx.x;
  const int cpl = t % CPB;
  const int slot = t / CPB;
  const int cp0 = blockIdx.y * CPB;
  const int cp = cp0 + cpl;
  const int c0 = cp * 8;
  const bool active = slot < nslots && cp < CP;

  float acc[9][8];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;

  if (active) {
    constexpr int NC = (DW_TW - 1) * S + 3;
    const long row0 = (long)blockIdx.x * RC;
    const long rows = (NR - row0 < RC) ? (NR - row0) : (long)RC;
    const long items = rows * nstrips;
    for (long it = slot; it < items; it += nslots) {
      const long row = row0 + it / nstrips;
      const int strip = (int)(it % nstrips);
      const int ho = (int)(row % Ho);
      const long n = row / Ho;
      const int wo0 = strip * DW_TW;
      const int wi0 = wo0 * S - 1;
      float g[DW_TW][8];
      const bf16* gr = dy + (row * Wo) * C + c0;
#pragma unroll
      for (int o = 0; o < DW_TW; ++o)
        load8_pred(gr + (long)(wo0 + o) * C, wo0 + o < Wo, g[o]);
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int hi = ho * S - 1 + kh;
        if (hi < 0 || hi >= H) continue;
        const bf16* xr = x + ((n * H + hi) * W) * C + c0;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          const int wi = wi0 + j;
          float xf[8];
          load8_pred(xr + (long)wi * C, wi >= 0 && wi < W, xf);
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            if (j - kw >= 0 && (j - kw) % S == 0 && (j - kw) / S < DW_TW) {
              const int o = (j - kw) / S;
#pragma unroll
              for (int q = 0; q < 8; ++q)
                acc[kh * 3 + kw][q] =
                    fmaf(g[o][q], xf[q], acc[kh * 3 + kw][q]);
            }
          }
        }
      }
    }
  }

  // slot*CPB + cpl == t < 256, so every thread has its own 8 floats
  const int ncol = CPB * 8;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[t * 8 + j] = acc[k][j];
    __syncthreads();
    for (int col = t; col < ncol; col += AMD_TPB) {
      float s = 0.f;
      for (int sl = 0; sl < nslots; ++sl) s += red[sl * ncol + col];
      const int c = cp0 * 8 + col;
      if (c < C) part[((long)blockIdx.x * 9 + k) * C + c] = s;
    }
    __syncthreads();
  }
}

// Weight gradient, level 2: out[e] = sum_p part[p][e], e over 9*C.  A block
// takes DW_L2E elements; each of its DW_L2G thread groups sums the partials
// p = g, g + DW_L2G, ... in order (four loads in flight, added in p order;
// a slot past P adds 0.f, which changes nothing), then the groups are added
// in group order.
__global__ __launch_bounds__(AMD_TPB) void dwconv3x3_wgrad_collapse_kernel(
    const float* __restrict__ part, float* __restrict__ out, int P, int E) {
  static_assert(AMD_TPB == DW_L2E * DW_L2G, "elements x groups");
  __shared__ float red[AMD_TPB];
  const int lane = threadIdx.x % DW_L2E;
  const int g = threadIdx.x / DW_L2E;
  const int e = blockIdx.x * DW_L2E + lane;
  float s = 0.f;
  if (e < E) {
    for (int p = g; p < P; p += 4 * DW_L2G) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pu = p + u * DW_L2G;
        v[u] = pu < P ? part[(long)pu * E + e] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) s += v[u];
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (g == 0 && e < E) {
    float tot = red[lane];
#pragma unroll
    for (int k = 1; k < DW_L2G; ++k) tot += red[k * DW_L2E + lane];
    out[e] = tot;
  }
}

struct DwGeom {
  long C, CP, Ho, Wo;
};

// Shared host-side contract of the three entry points.
DwGeom dw_check(const at::Tensor& a2d, const char* what, long Nn, long H,
                long W, long stride, long rows_h, long rows_w) {
  TORCH_CHECK(a2d.is_cuda() && a2d.scalar_type() == at::kBFloat16 &&
                  a2d.dim() == 2 && a2d.is_contiguous(),
              what, " must be a contiguous 2-D bf16 GPU tensor");
  TORCH_CHECK(stride == 1 || stride == 2, "dwconv3x3: stride must be 1 or 2");
  TORCH_CHECK(Nn >= 0 && H >= 1 && W >= 1, "dwconv3x3: bad geometry");
  TORCH_CHECK(H < (1 << 24) && W < (1 << 24), "dwconv3x3: image too large");
  const long C = a2d.size(1);
  TORCH_CHECK(C >= 8 && C % 8 == 0,
              "dwconv3x3: C must be a positive multiple of 8, got ", C);
  TORCH_CHECK(C < (1 << 24), "dwconv3x3: C too large");
  const long Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
  const long eh = rows_h ? Ho : H, ew = rows_w ? Wo : W;
  TORCH_CHECK(a2d.size(0) == Nn * eh * ew, what, " has ", a2d.size(0),
              " rows, geometry needs ", Nn * eh * ew);
  return {C, C / 8, Ho, Wo};
}

void dw_check_w9(const at::Tensor& w9, const at::Tensor& like, long C) {
  TORCH_CHECK(w9.is_cuda() && w9.scalar_type() == at::kBFloat16 &&
                  w9.dim() == 2 && w9.is_contiguous() && w9.size(0) == 9 &&
                  w9.size(1) == C && w9.device() == like.device(),
              "w9 must be a contiguous [9, C] bf16 tensor on the same GPU");
}

long dw_blocks(long total) {
  const long nb = (total + AMD_TPB - 1) / AMD_TPB;
  TORCH_CHECK(nb < (1L << 31), "dwconv3x3: too many blocks");
  return nb;
}

}  // namespace

at::Tensor dwconv3x3_fwd(at::Tensor x2d, long Nn, long H, long W, long stride,
                         at::Tensor w9) {
  const DwGeom g = dw_check(x2d, "x2d", Nn, H, W, stride, 0, 0);
  dw_check_w9(w9, x2d, g.C);
  auto y = at::empty({Nn * g.Ho * g.Wo, g.C}, x2d.options());
  const long nstrips = (g.Wo + DW_TW - 1) / DW_TW;
  const long total = Nn * g.Ho * nstrips * g.CP;
  if (total == 0) return y;  // empty batch
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* xp = (const bf16*)x2d.const_data_ptr();
  const bf16* wp = (const bf16*)w9.const_data_ptr();
  bf16* yp = (bf16*)y.data_ptr();
  const dim3 grid((unsigned)dw_blocks(total));
  if (stride == 1)
    dwconv3x3_stencil_kernel<1, false><<<grid, AMD_TPB, 0, stream>>>(
        xp, wp, yp, (int)H, (int)W, (int)g.Ho, (int)g.Wo, (int)g.C,
        (int)g.CP, (int)nstrips, total);
  else
    dwconv3x3_stencil_kernel<2, false><<<grid, AMD_TPB, 0, stream>>>(
        xp, wp, yp, (int)H, (int)W, (int)g.Ho, (int)g.Wo, (int)g.C,
        (int)g.CP, (int)nstrips, total);
  CHECK_CUDA_OK();
  return y;
}

at::Tensor dwconv3x3_dgrad(at::Tensor dy2d, long Nn, long H, long W,
                           long stride, at::Tensor w9) {
  const DwGeom g = dw_check(dy2d, "dy2d", Nn, H, W, stride, 1, 1);
  dw_check_w9(w9, dy2d, g.C);
  auto dx = at::empty({Nn * H * W, g.C}, dy2d.options());
  const long nstrips = (W + DW_TW - 1) / DW_TW;
  const long total = Nn * H * nstrips * g.CP;
  if (total == 0) return dx;  // empty batch
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* gp = (const bf16*)dy2d.const_data_ptr();
  const bf16* wp = (const bf16*)w9.const_data_ptr();
  bf16* xp = (bf16*)dx.data_ptr();
  const dim3 grid((unsigned)dw_blocks(total));
  if (stride == 1)
    // Ho == H, Wo == W: the forward stencil over dy with mirrored taps
    dwconv3x3_stencil_kernel<1, true><<<grid, AMD_TPB, 0, stream>>>(
        gp, wp, xp, (int)H, (int)W, (int)H, (int)W, (int)g.C, (int)g.CP,
        (int)nstrips, total);
  else
    dwconv3x3_dgrad_s2_kernel<<<grid, AMD_TPB, 0, stream>>>(
        gp, wp, xp, (int)H, (int)W, (int)g.Ho, (int)g.Wo, (int)g.C,
        (int)g.CP, (int)nstrips, total);
  CHECK_CUDA_OK();
  return dx;
}

at::Tensor dwconv3x3_wgrad(at::Tensor dy2d, at::Tensor x2d, long Nn, long H,
                           long W, long stride) {
  const DwGeom g = dw_check(dy2d, "dy2d", Nn, H, W, stride, 1, 1);
  dw_check(x2d, "x2d", Nn, H, W, stride, 0, 0);
  TORCH_CHECK(x2d.size(1) == g.C && x2d.device() == dy2d.device(),
              "dwconv3x3_wgrad: x2d and dy2d disagree");
  // geometry of the partial reduction: a function of the shape alone
  const long CPB = std::min<long>(g.CP, AMD_TPB);
  const long nslots = AMD_TPB / CPB;
  const long npg = (g.CP + CPB - 1) / CPB;
  const long nstrips = (g.Wo + DW_TW - 1) / DW_TW;
  const long NR = Nn * g.Ho;
  if (NR == 0)  // empty batch
    return at::zeros({9, g.C}, dy2d.options().dtype(at::kFloat));
  // about 4 strips per slot, so that the late-stage shapes (few rows, many
  // channels) still fill the device, and no more than 512 chunks, which
  // bounds the partials that the collapse has to read
  long RC = std::max<long>(1, nslots * 4 / nstrips);
  RC = std::max<long>(RC, (NR + 511) / 512);
  const long P = (NR + RC - 1) / RC;
  TORCH_CHECK(RC < (1L << 31) && npg < 65536, "dwconv3x3_wgrad: shape");
  auto fopt = dy2d.options().dtype(at::kFloat);
  auto part = at::empty({P, 9, g.C}, fopt);
  auto dw9 = at::empty({9, g.C}, fopt);
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* gp = (const bf16*)dy2d.const_data_ptr();
  const bf16* xp = (const bf16*)x2d.const_data_ptr();
  const dim3 grid((unsigned)P, (unsigned)npg);
  if (stride == 1)
    dwconv3x3_wgrad_part_kernel<1><<<grid, AMD_TPB, 0, stream>>>(
        gp, xp, part.data_ptr<float>(), (int)H, (int)W, (int)g.Ho, (int)g.Wo,
        (int)g.C, (int)g.CP, (int)CPB, (int)nslots, (int)nstrips, (int)RC,
        NR);
  else
    dwconv3x3_wgrad_part_kernel<2><<<grid, AMD_TPB, 0, stream>>>(
        gp, xp, part.data_ptr<float>(), (int)H, (int)W, (int)g.Ho, (int)g.Wo,
        (int)g.C, (int)g.CP, (int)CPB, (int)nslots, (int)nstrips, (int)RC,
        NR);
  CHECK_CUDA_OK();
  const long E = 9 * g.C;
  dwconv3x3_wgrad_collapse_kernel<<<(unsigned)((E + DW_L2E - 1) / DW_L2E), AMD_TPB, 0,
                                    stream>>>(
      part.data_ptr<float>(), dw9.data_ptr<float>(), (int)P, (int)E);
  CHECK_CUDA_OK();
  return dw9;
}
