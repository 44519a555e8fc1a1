// Depthwise 5x5 pad-2 convolution (stride 1/2), NHWC bf16, for gfx950.
//
// 25 multiply-adds per output element and a 5x5 window: the 3x3 design
// (all taps' weights in registers, window re-read from global memory by
// every lane) does not carry over.  25 x 8 fp32 weights are 200 VGPRs, and
// every input element would be fetched 25 times.  Here the window goes
// through LDS and a lane never holds more than one kernel row of weights:
//
//  * forward and stride-1 dgrad (dw5_halo_kernel): a 256-thread block owns
//    TH x TWB output pixels x CPB channel packs of one image.  It stages the
//    input halo ((TH-1)*S + 5) x ((TWB-1)*S + 5) pixels x CPB packs, zeros
//    where the image ends, and its 25 x CPB weight packs into LDS with
//    16-byte loads, pack index fastest across lanes.  A lane then owns one
//    pack and strips of 4 output columns of one row: per kernel row it reads
//    the strip's window of (4-1)*S + 5 packs from LDS once, feeds the five
//    horizontal taps from registers and keeps that row's 5 x 8 weights live.
//    The compute loop has no predicates.  dgrad at stride 1 is the same
//    kernel over dy with the taps staged mirrored (24 - t).
//  * stride-2 dgrad (dw5_dgrad_s2_kernel): a parity gather.  dx(h, w) sums
//    the taps with (h + 2 - kh) and (w + 2 - kw) even: 3 or 2 kernel rows
//    times 3 or 2 columns, never 25.  The block stages the
//    (TH/2 + 2) x (TWB/2 + 2) dy pixels its dx tile needs, on the same
//    scheme.
//  * wgrad (dw5_wgrad_part_kernel + the shared collapse): a thread is
//    (slot, kh, pack) with 5 x 8 fp32 accumulators for one kernel row; the
//    five kh lanes of a (slot, pack) read the same dy strip and each its own
//    x row.  Slots are summed in slot order through LDS into part[P, 25, C];
//    P depends on the shape alone; the collapse runs over E = 25*C.
//
// fp32 accumulation with fmaf over exact bf16 products, one rounding to
// bf16, fixed summation order, no atomics: bitwise reproducible.  Row
// offsets into the tensors are 64-bit.
#include "common.h"

// No packed-fp32 selection (v_pk_*_f32) for the code of this file (see
// lars.hip): a device target feature, switched off per function.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "dwconv_common.h"

namespace {

constexpr int DW5_LDS = 64 * 1024;  // per block: two blocks and more per CU
constexpr int DW5_WG_CPB = 16;      // wgrad: packs per block, at most
constexpr int DW5_WG_P = 512;       // wgrad: partials, at most

// 8 bf16 in a uint4 -> 8 fp32 (exact)
__device__ __forceinline__ void cvt8(const uint4& v, float f[8]) {
  const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float(u[j] << 16);
    f[2 * j + 1] = __uint_as_float(u[j] & 0xffff0000u);
  }
}

// Tile of a block, chosen on the host from the shape alone.
struct Dw5Tile {
  int TH, nstr;       // tile rows, strips of 4 columns per tile row
  int nth, ntw;       // tiles per image
  int CPB, npg;       // packs per block, pack groups
  int lds_bytes;
  long blocks;
};

// block -> (pack group, tile column, tile row, image), pack group fastest
struct Dw5Block {
  int pg, tw, th;
  long n;
};
__device__ __forceinline__ Dw5Block dw5_block(int npg, int ntw, int nth) {
  long b = blockIdx.x;
  Dw5Block r;
  r.pg = (int)(b % npg);
  b /= npg;
  r.tw = (int)(b % ntw);
  b /= ntw;
  r.th = (int)(b % nth);
  r.n = b / nth;
  return r;
}

// y(ho, wo) = sum_{kh,kw} x(ho*S - 2 + kh, wo*S - 2 + kw) * w[kh][kw];
// `mirror` stages tap 24 - t in place of t.
// LDS: wl[25][CPB] weight packs, then hl[HH][HW][CPB] input packs.
template <int S>
__global__ __launch_bounds__(AMD_TPB) void dw5_halo_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ w25,
    bf16* __restrict__ y, int H, int W, int Ho, int Wo, int C, int CP,
    int CPB, int npg, int TH, int nstr, int ntw, int nth, int mirror) {
  extern __shared__ uint4 dw5_lds[];
  const int t = threadIdx.x;
  const int cpl = t % CPB, sp = t / CPB, nsp = AMD_TPB / CPB;
  const Dw5Block bk = dw5_block(npg, ntw, nth);
  const int cp = bk.pg * CPB + cpl;
  const bool lane_ok = sp < nsp && cp < CP;
  const int TWB = nstr * DW_TW;
  const int HH = (TH - 1) * S + 5, HW = (TWB - 1) * S + 5;
  const int ho0 = bk.th * TH, wo0 = bk.tw * TWB;
  const int hi0 = ho0 * S - 2, wi0 = wo0 * S - 2;
  uint4* wl = dw5_lds;
  uint4* hl = dw5_lds + 25 * CPB;
  if (lane_ok) {
    for (int tap = sp; tap < 25; tap += nsp)
      wl[tap * CPB + cpl] = *reinterpret_cast<const uint4*>(
          w25 + (long)(mirror ? 24 - tap : tap) * C + cp * 8);
    const bf16* xc = x + (long)cp * 8;
    for (int p = sp; p < HH * HW; p += nsp) {
      const int r = p / HW, col = p - r * HW;
      const int hi = hi0 + r, wi = wi0 + col;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (hi >= 0 && hi < H && wi >= 0 && wi < W)
        v = *reinterpret_cast<const uint4*>(
            xc + ((bk.n * H + hi) * W + wi) * C);
      hl[p * CPB + cpl] = v;
    }
  }
  __syncthreads();
  if (!lane_ok) return;

  constexpr int NC = (DW_TW - 1) * S + 5;  // window columns
  const int items = TH * nstr;
  for (int it = sp; it < items; it += nsp) {
    const int orow = it / nstr, strip = it - orow * nstr;
    const int ho = ho0 + orow, wo = wo0 + strip * DW_TW;
    if (ho >= Ho || wo >= Wo) continue;
    float acc[DW_TW][8];
#pragma unroll
    for (int o = 0; o < DW_TW; ++o)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[o][q] = 0.f;
    // a real loop: unrolled, the compiler hoists every row's LDS reads and
    // all 25 taps' weights become live at once
#pragma unroll 1
    for (int kh = 0; kh < 5; ++kh) {
      float wr[5][8];
#pragma unroll
      for (int kw = 0; kw < 5; ++kw) cvt8(wl[(kh * 5 + kw) * CPB + cpl], wr[kw]);
      const uint4* row =
          hl + ((orow * S + kh) * HW + strip * DW_TW * S) * CPB + cpl;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        float xf[8];
        cvt8(row[j * CPB], xf);
#pragma unroll
        for (int kw = 0; kw < 5; ++kw) {
          // window column j is tap kw of output o = (j - kw) / S
          if (j - kw >= 0 && (j - kw) % S == 0 && (j - kw) / S < DW_TW) {
            const int o = (j - kw) / S;
#pragma unroll
            for (int q = 0; q < 8; ++q)
              acc[o][q] = fmaf(xf[q], wr[kw][q], acc[o][q]);
          }
        }
      }
    }
    bf16* yr = y + ((bk.n * Ho + ho) * Wo) * C + cp * 8;
#pragma unroll
    for (int o = 0; o < DW_TW; ++o)
      if (wo + o < Wo) store8(yr + (long)(wo + o) * C, acc[o]);
  }
}

// Stride-2 input gradient: dx(h, w) = sum over the taps (kh, kw) with
// (h + 2 - kh) and (w + 2 - kw) even and the halves inside [0, Ho) x
// [0, Wo), of dy((h+2-kh)/2, (w+2-kw)/2) * w[kh][kw].  A strip starts at an
// even column w = 2q and reads the dy packs d0..d3 = dy[q-1 .. q+2]:
//   w   : kw 0 <- d2, kw 2 <- d1, kw 4 <- d0     w+1 : kw 1 <- d2, kw 3 <- d1
//   w+2 : kw 0 <- d3, kw 2 <- d2, kw 4 <- d1     w+3 : kw 1 <- d3, kw 3 <- d2
// Rows alike: even h takes kh 0, 2, 4 from dy rows h/2 + 1, h/2, h/2 - 1,
// odd h takes kh 1, 3 from (h+1)/2, (h-1)/2.  The tile is TH (even) x
// nstr*4 dx pixels; LDS holds wl[25][CPB], then gl[DH][DW][CPB] with
// DH = TH/2 + 2, DW = 2*nstr + 2, first dy row and column h0/2 - 1,
// w0/2 - 1, zeros outside dy.
__global__ __launch_bounds__(AMD_TPB) void dw5_dgrad_s2_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ w25,
    bf16* __restrict__ dx, int H, int W, int Ho, int Wo, int C, int CP,
    int CPB, int npg, int TH, int nstr, int ntw, int nth) {
  static_assert(DW_TW == 4, "tap table below is written for 4 columns");
  extern __shared__ uint4 dw5_lds[];
  const int t = threadIdx.x;
  const int cpl = t % CPB, sp = t / CPB, nsp = AMD_TPB / CPB;
  const Dw5Block bk = dw5_block(npg, ntw, nth);
  const int cp = bk.pg * CPB + cpl;
  const bool lane_ok = sp < nsp && cp < CP;
  const int DH = TH / 2 + 2, DW = 2 * nstr + 2;
  const int h0 = bk.th * TH, w0 = bk.tw * nstr * DW_TW;
  const int r0 = h0 / 2 - 1, q0 = w0 / 2 - 1;
  uint4* wl = dw5_lds;
  uint4* gl = dw5_lds + 25 * CPB;
  if (lane_ok) {
    for (int tap = sp; tap < 25; tap += nsp)
      wl[tap * CPB + cpl] = *reinterpret_cast<const uint4*>(
          w25 + (long)tap * C + cp * 8);
    const bf16* gc = dy + (long)cp * 8;
    for (int p = sp; p < DH * DW; p += nsp) {
      const int r = p / DW, col = p - r * DW;
      const int ho = r0 + r, wo = q0 + col;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (ho >= 0 && ho < Ho && wo >= 0 && wo < Wo)
        v = *reinterpret_cast<const uint4*>(
            gc + ((bk.n * Ho + ho) * Wo + wo) * C);
      gl[p * CPB + cpl] = v;
    }
  }
  __syncthreads();
  if (!lane_ok) return;

  const int items = TH * nstr;
  for (int it = sp; it < items; it += nsp) {
    const int irow = it / nstr, strip = it - irow * nstr;
    const int h = h0 + irow, w = w0 + strip * DW_TW;
    if (h >= H || w >= W) continue;
    float acc[DW_TW][8];
#pragma unroll
    for (int o = 0; o < DW_TW; ++o)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[o][q] = 0.f;
    // kh = (h & 1), +2, +4 while <= 4; dy row (h + 2 - kh) / 2
    for (int kh = h & 1; kh < 5; kh += 2) {
      const int r = ((h + 2 - kh) >> 1) - r0;  // 0 <= r < DH
      float k[5][8], d[4][8];
#pragma unroll
      for (int kw = 0; kw < 5; ++kw) cvt8(wl[(kh * 5 + kw) * CPB + cpl], k[kw]);
      const uint4* row = gl + (r * DW + 2 * strip) * CPB + cpl;
#pragma unroll
      for (int j = 0; j < 4; ++j) cvt8(row[j * CPB], d[j]);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        acc[0][q] = fmaf(d[2][q], k[0][q], acc[0][q]);
        acc[0][q] = fmaf(d[1][q], k[2][q], acc[0][q]);
        acc[0][q] = fmaf(d[0][q], k[4][q], acc[0][q]);
        acc[1][q] = fmaf(d[2][q], k[1][q], acc[1][q]);
        acc[1][q] = fmaf(d[1][q], k[3][q], acc[1][q]);
        acc[2][q] = fmaf(d[3][q], k[0][q], acc[2][q]);
        acc[2][q] = fmaf(d[2][q], k[2][q], acc[2][q]);
        acc[2][q] = fmaf(d[1][q], k[4][q], acc[2][q]);
        acc[3][q] = fmaf(d[3][q], k[1][q], acc[3][q]);
        acc[3][q] = fmaf(d[2][q], k[3][q], acc[3][q]);
      }
    }
    bf16* xr = dx + ((bk.n * H + h) * W) * C + cp * 8;
#pragma unroll
    for (int o = 0; o < DW_TW; ++o)
      if (w + o < W) store8(xr + (long)(w + o) * C, acc[o]);
  }
}

// Weight gradient, level 1.  dw[kh][kw][c] = sum over (n, ho, wo) of
// dy(n, ho, wo, c) * x(n, ho*S-2+kh, wo*S-2+kw, c).
// Block (chunk = blockIdx.x, pack group = blockIdx.y): thread
// t = (slot*5 + kh)*CPB + pack, pack fastest, nslots = 256 / (5*CPB).  The
// chunk is RC consecutive output rows (n*Ho + ho); slot s walks its strips
// s, s + nslots, ... in order, its kh lane with 5 x 8 fp32 accumulators for
// the taps (kh, 0..4).  Then the slots of a (kh, pack) are summed in slot
// order through LDS, one kw at a time.
template <int S>
__global__ __launch_bounds__(AMD_TPB) void dw5_wgrad_part_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ x,
    float* __restrict__ part, int H, int W, int Ho, int Wo, int C, int CP,
    int CPB, int nslots, int nstrips, int RC, long NR) {
  __shared__ float red[AMD_TPB * 8];
  const int t = threadIdx.x;
  const int cpl = t % CPB;
  const int kh = (t / CPB) % 5;
  const int slot = t / (5 * CPB);
  const int cp0 = blockIdx.y * CPB;
  const int cp = cp0 + cpl;
  const bool active = slot < nslots && cp < CP;

  float acc[5][8];
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[k][q] = 0.f;

  if (active) {
    constexpr int NC = (DW_TW - 1) * S + 5;
    const int c0 = cp * 8;
    const long row0 = (long)blockIdx.x * RC;
    const long rows = (NR - row0 < RC) ? (NR - row0) : (long)RC;
    const long items = rows * nstrips;
    for (long it = slot; it < items; it += nslots) {
      const long row = row0 + it / nstrips;
      const int strip = (int)(it % nstrips);
      const int ho = (int)(row % Ho);
      const long n = row / Ho;
      const int hi = ho * S - 2 + kh;
      if (hi < 0 || hi >= H) continue;
      const int wo0 = strip * DW_TW;
      const int wi0 = wo0 * S - 2;
      float g[DW_TW][8];
      const bf16* gr = dy + (row * Wo) * C + c0;
#pragma unroll
      for (int o = 0; o < DW_TW; ++o)
        load8_pred(gr + (long)(wo0 + o) * C, wo0 + o < Wo, g[o]);
      const bf16* xr = x + ((n * H + hi) * W) * C + c0;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int wi = wi0 + j;
        float xf[8];
        load8_pred(xr + (long)wi * C, wi >= 0 && wi < W, xf);
#pragma unroll
        for (int kw = 0; kw < 5; ++kw) {
          if (j - kw >= 0 && (j - kw) % S == 0 && (j - kw) / S < DW_TW) {
            const int o = (j - kw) / S;
#pragma unroll
            for (int q = 0; q < 8; ++q)
              acc[kw][q] = fmaf(g[o][q], xf[q], acc[kw][q]);
          }
        }
      }
    }
  }

  // red[t*8 + q], t < 256: column (kh*CPB + pack)*8 + q of row `slot`
  const int ncol = 5 * CPB * 8;
#pragma unroll
  for (int kw = 0; kw < 5; ++kw) {
#pragma unroll
    for (int q = 0; q < 8; ++q) red[t * 8 + q] = acc[kw][q];
    __syncthreads();
    for (int col = t; col < ncol; col += AMD_TPB) {
      float s = 0.f;
      for (int sl = 0; sl < nslots; ++sl) s += red[sl * ncol + col];
      const int khc = col / (CPB * 8);
      const int c = cp0 * 8 + col - khc * CPB * 8;
      if (c < C) part[((long)blockIdx.x * 25 + khc * 5 + kw) * C + c] = s;
    }
    __syncthreads();
  }
}

DwGeom dw5_check(const at::Tensor& a2d, const char* what, long Nn, long H,
                 long W, long stride, long rows_h, long rows_w) {
  return dw_check("dwconv5x5", 5, a2d, what, Nn, H, W, stride, rows_h,
                  rows_w);
}

long dw5_ceil(long a, long b) { return (a + b - 1) / b; }

// Tile of the LDS kernels for an image of rows x cols result pixels.
// `halo(TH, TWB)` is the number of staged pixels.  At most 8 x 16 pixels,
// split evenly over the image; as many packs per block as keep every lane
// on an item (8 at least: 128-byte global runs; 32 at most).  A block over
// DW5_LDS gives up packs down to 8, then rows, then packs again.
template <typename Halo>
Dw5Tile dw5_tile(long Nn, long rows, long cols, long CP, bool even_rows,
                 Halo halo) {
  Dw5Tile tl;
  const long nstrips = dw5_ceil(cols, DW_TW);
  tl.ntw = (int)dw5_ceil(nstrips, 4);
  tl.nstr = (int)dw5_ceil(nstrips, tl.ntw);
  long TH = dw5_ceil(rows, dw5_ceil(rows, 8));
  if (even_rows) TH += TH & 1;
  const long cap =
      std::min<long>(32, std::max<long>(8, AMD_TPB / (TH * tl.nstr)));
  tl.npg = (int)dw5_ceil(CP, cap);
  tl.CPB = (int)dw5_ceil(CP, tl.npg);
  const long step = even_rows ? 2 : 1;
  auto bytes = [&](long th) {
    return 16 * tl.CPB * (25 + halo(th, (long)tl.nstr * DW_TW));
  };
  while (bytes(TH) > DW5_LDS) {
    if (tl.CPB > 8 || TH <= step) {
      ++tl.npg;
      tl.CPB = (int)dw5_ceil(CP, tl.npg);
    } else {
      TH -= step;
    }
  }
  tl.TH = (int)TH;
  tl.nth = (int)dw5_ceil(rows, TH);
  tl.lds_bytes = (int)bytes(TH);
  tl.blocks = Nn * tl.nth * tl.ntw * tl.npg;
  TORCH_CHECK(tl.blocks < (1L << 31), "dwconv5x5: too many blocks");
  return tl;
}

// forward of `in` [Nn*H*W, C] to `out` [Nn*Ho*Wo, C]
void dw5_launch_halo(const at::Tensor& in, const at::Tensor& w25,
                     at::Tensor& out, long Nn, long H, long W, long Ho,
                     long Wo, long stride, const DwGeom& g, bool mirror) {
  const long S = stride;
  const Dw5Tile tl =
      dw5_tile(Nn, Ho, Wo, g.CP, false, [S](long th, long twb) {
        return ((th - 1) * S + 5) * ((twb - 1) * S + 5);
      });
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* ip = (const bf16*)in.const_data_ptr();
  const bf16* wp = (const bf16*)w25.const_data_ptr();
  bf16* op = (bf16*)out.data_ptr();
  const dim3 grid((unsigned)tl.blocks);
  if (stride == 1)
    dw5_halo_kernel<1><<<grid, AMD_TPB, tl.lds_bytes, stream>>>(
        ip, wp, op, (int)H, (int)W, (int)Ho, (int)Wo, (int)g.C, (int)g.CP,
        tl.CPB, tl.npg, tl.TH, tl.nstr, tl.ntw, tl.nth, (int)mirror);
  else
    dw5_halo_kernel<2><<<grid, AMD_TPB, tl.lds_bytes, stream>>>(
        ip, wp, op, (int)H, (int)W, (int)Ho, (int)Wo, (int)g.C, (int)g.CP,
        tl.CPB, tl.npg, tl.TH, tl.nstr, tl.ntw, tl.nth, (int)mirror);
  CHECK_CUDA_OK();
}

}  // namespace

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

at::Tensor dwconv5x5_fwd(at::Tensor x2d, long Nn, long H, long W, long stride,
                         at::Tensor w25) {
  const DwGeom g = dw5_check(x2d, "x2d", Nn, H, W, stride, 0, 0);
  dw_check_w("w25", 25, w25, x2d, g.C);
  auto y = at::empty({Nn * g.Ho * g.Wo, g.C}, x2d.options());
  if (Nn == 0) return y;  // empty batch
  dw5_launch_halo(x2d, w25, y, Nn, H, W, g.Ho, g.Wo, stride, g, false);
  return y;
}

at::Tensor dwconv5x5_dgrad(at::Tensor dy2d, long Nn, long H, long W,
                           long stride, at::Tensor w25) {
  const DwGeom g = dw5_check(dy2d, "dy2d", Nn, H, W, stride, 1, 1);
  dw_check_w("w25", 25, w25, dy2d, g.C);
  auto dx = at::empty({Nn * H * W, g.C}, dy2d.options());
  if (Nn == 0) return dx;  // empty batch
  if (stride == 1) {
    // Ho == H, Wo == W: the forward kernel over dy with mirrored taps
    dw5_launch_halo(dy2d, w25, dx, Nn, H, W, H, W, 1, g, true);
    return dx;
  }
  const Dw5Tile tl = dw5_tile(Nn, H, W, g.CP, true, [](long th, long twb) {
    return (th / 2 + 2) * (twb / 2 + 2);
  });
  auto stream = at::cuda::getCurrentCUDAStream();
  dw5_dgrad_s2_kernel<<<dim3((unsigned)tl.blocks), AMD_TPB, tl.lds_bytes,
                        stream>>>(
      (const bf16*)dy2d.const_data_ptr(), (const bf16*)w25.const_data_ptr(),
      (bf16*)dx.data_ptr(), (int)H, (int)W, (int)g.Ho, (int)g.Wo, (int)g.C,
      (int)g.CP, tl.CPB, tl.npg, tl.TH, tl.nstr, tl.ntw, tl.nth);
  CHECK_CUDA_OK();
  return dx;
}

at::Tensor dwconv5x5_wgrad(at::Tensor dy2d, at::Tensor x2d, long Nn, long H,
                           long W, long stride) {
  const DwGeom g = dw5_check(dy2d, "dy2d", Nn, H, W, stride, 1, 1);
  dw5_check(x2d, "x2d", Nn, H, W, stride, 0, 0);
  TORCH_CHECK(x2d.size(1) == g.C && x2d.device() == dy2d.device(),
              "dwconv5x5_wgrad: x2d and dy2d disagree");
  auto fopt = dy2d.options().dtype(at::kFloat);
  const long NR = Nn * g.Ho;
  if (NR == 0) return at::zeros({25, g.C}, fopt);  // empty batch
  // geometry of the partial reduction: a function of the shape alone.
  // About 640 blocks over all pack groups (a few per CU), at most DW5_WG_P
  // chunks, which bounds the partials that the collapse has to read.
  const long npg = dw5_ceil(g.CP, DW5_WG_CPB);
  const long CPB = dw5_ceil(g.CP, npg);
  const long nslots = AMD_TPB / (5 * CPB);
  const long nstrips = dw5_ceil(g.Wo, DW_TW);
  const long Pt = std::max<long>(1, std::min<long>(DW5_WG_P, 640 / npg));
  const long RC = dw5_ceil(NR, Pt);
  const long P = dw5_ceil(NR, RC);
  TORCH_CHECK(RC < (1L << 31) && npg < 65536, "dwconv5x5_wgrad: shape");
  auto part = at::empty({P, 25, g.C}, fopt);
  auto dw25 = at::empty({25, g.C}, fopt);
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* gp = (const bf16*)dy2d.const_data_ptr();
  const bf16* xp = (const bf16*)x2d.const_data_ptr();
  const dim3 grid((unsigned)P, (unsigned)npg);
  if (stride == 1)
    dw5_wgrad_part_kernel<1><<<grid, AMD_TPB, 0, stream>>>(
        gp, xp, part.data_ptr<float>(), (int)H, (int)W, (int)g.Ho, (int)g.Wo,
        (int)g.C, (int)g.CP, (int)CPB, (int)nslots, (int)nstrips, (int)RC,
        NR);
  else
    dw5_wgrad_part_kernel<2><<<grid, AMD_TPB, 0, stream>>>(
        gp, xp, part.data_ptr<float>(), (int)H, (int)W, (int)g.Ho, (int)g.Wo,
        (int)g.C, (int)g.CP, (int)CPB, (int)nslots, (int)nstrips, (int)RC,
        NR);
  CHECK_CUDA_OK();
  dw_collapse(part, dw25, P, 25 * g.C, stream);
  return dw25;
}
