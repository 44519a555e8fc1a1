// Per-group MFMA weight gradient of grouped 3x3 convolutions (NHWC bf16, pad
// 1, stride 1/2, Cin == Cout == C, S = C / groups in {4, 8, 16, 32}) for
// gfx950: the third pass of the layer gconv.hip serves.
//
// Per channel WINDOW of CW = 16 (S <= 16) or 32 (S = 32) channels the
// gradient is one TN GEMM whose reduction dimension is the pixel:
//
//   dWwin[n, tap, c] = sum_{img, ho, wo} dY[img, ho, wo, n]
//                                        * X[img, ho*s + kh - 1, wo*s + kw - 1, c]
//
// of which only the S x S blocks with n / S == c / S are kept.
//
//  * Block = 4 waves = a slab of 64 channels x a contiguous range of the
//    forward kernel's pixel tiles (TH x 16 output pixels of one image, TH = 8
//    at stride 1, 4 at stride 2).  All tiles of the range accumulate in
//    registers; the block stores once.  Grid = P x nslab, block p takes tiles
//    [p*T/P, (p+1)*T/P).
//  * Per tile the X halo (out-of-image pixels as zeros: all the padding
//    handling) and the dY tile (overhanging pixels as zeros: they add exactly
//    0) are staged with 16-byte loads into 16-channel planes
//    [window quarter][pixel][16 ch], 32 B per pixel, X pixels first, then dY.
//    The NEXT tile's global loads are issued into registers before the
//    current tile's MFMAs and written to LDS after them: one LDS buffer,
//    loads in flight under the compute.
//  * Both MFMA operands need k = pixel while memory is channel-contiguous.
//    16 consecutive pixels of a plane are 512 contiguous bytes, and one
//    ds_read_b64_tr_b16 at base + lane*8 hands lane (fq, fr) channel fr,
//    pixels fq*4 + j — the form tests/test_gpu_wgrad2.py pins.  A K-step is
//    32 pixels = two tile rows x 16 columns = two such reads per operand; the
//    k -> pixel map (read, fq, j) is the same for A and B.
//  * A (dY^T) is read once per K-step and kept for all nine taps.  B for tap
//    (kh, kw) is the same halo plane at pixel offset (i + kh)*LW + kw: X is
//    staged once and read nine times, no im2col, no gather addressing.
//  * Stride 2: a halo row is stored with its columns split by parity (17
//    even-offset columns, then 16 odd-offset ones), so consecutive wo are
//    consecutive pixels again: kw = 0 / 2 read the first sub-plane at wo /
//    wo + 1, kw = 1 the second at wo; halo row 2*i + kh.
//  * CW = 16: wave = window, 9 accumulator fragments.  CW = 32: two waves
//    share a window and split the output-channel halves, 18 fragments each.
//    Either way wave w owns dY quarter w.
//  * Epilogue: a lane keeps the elements on the group diagonal and stores
//    them to partials [P][C][9][S] fp32 (P = 1: straight to the output);
//    gconv_wgrad_collapse sums p = 0..P-1 in a fixed order.  No atomics, one
//    writer per element, bitwise repeatable for a fixed P.
#include "common.h"

// the compiler's packed fp32 forms are kept out of this file's kernels
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) short;
using s16x4 = __attribute__((ext_vector_type(4))) short;

constexpr int GW_TPB = 256;
constexpr int GW_SLAB = 64;  // channels per block
constexpr int GW_TW = 16;    // tile width = pixels of one transpose read
constexpr int GW_PIX = 32;   // LDS bytes per pixel of a 16-channel plane
constexpr int GW_CP = 16;    // collapse: partial lanes x float4 columns / block

template <int STRIDE> struct GwTile {
  static constexpr int TH = STRIDE == 2 ? 4 : 8;
  static constexpr int LH = STRIDE == 2 ? 2 * TH + 1 : TH + 2;
  static constexpr int LW = STRIDE == 2 ? 2 * GW_TW + 1 : GW_TW + 2;
  static constexpr int NPX = LH * LW;         // staged X pixels
  static constexpr int NPIX = NPX + TH * GW_TW;  // ... then the dY tile
  static constexpr int PLANE = NPIX * GW_PIX;
};

struct GwGeom {
  int C, lgS;
  int H, W;    // x
  int OH, OW;  // dY
  int tilesH, tilesW, nslab;
  int T, P;    // pixel tiles, blocks per slab
};

// first pixel of the 16-pixel run of halo row that output row i reads for
// tap (kh, kw)
template <int STRIDE>
__device__ __forceinline__ constexpr int gw_xoff(int i, int kh, int kw) {
  return STRIDE == 1 ? (i + kh) * GwTile<1>::LW + kw
                     : (2 * i + kh) * GwTile<2>::LW +
                           (kw == 1 ? GW_TW + 1 : kw >> 1);
}

// two transpose reads (tile rows i, i + 1) -> one bf16x8 MFMA operand;
// p0 / p1 = plane + first pixel * 32 + lane * 8
__device__ __forceinline__ bf16x8 gw_frag(const char* p0, const char* p1) {
  typedef __attribute__((address_space(3))) s16x4* lds_ptr;
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p0);
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p1);
  return bf16x8{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}

// 3 (CW = 16) / 2 (CW = 32) blocks per CU: the register budget at which the
// accumulators, the prefetched tile and the fragments stay out of scratch
template <int CW, int STRIDE>
__global__ void __launch_bounds__(GW_TPB, CW == 16 ? 3 : 2)
gconv3x3_wgrad_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                      float* __restrict__ out, GwGeom g) {
  using T = GwTile<STRIDE>;
  constexpr int TH = T::TH, LW = T::LW, NPX = T::NPX, NPIX = T::NPIX;
  constexpr int PLANE = T::PLANE;
  constexpr int NLD = (NPIX + 31) / 32;  // 16-byte units per thread and tile
  constexpr int NB = CW / 16;            // X quarter planes per wave
  __shared__ __attribute__((aligned(16))) char lds[4 * PLANE];

  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int fr = lane & 15, fq = lane >> 4;
  const int slab = blockIdx.x % g.nslab, part = blockIdx.x / g.nslab;
  const int c0 = slab * GW_SLAB;
  const bool active = c0 + wave * 16 < g.C;  // last slab may be part full
  const int tile0 = (int)((long)part * g.T / g.P);
  const int tile1 = (int)((long)(part + 1) * g.T / g.P);

  // ---- staging: 8 threads x 16 B per pixel, unit k = pixel (t>>3) + 32k ----
  const int cu = t & 7;
  const bool cok = c0 + cu * 8 < g.C;
  char* const sdst = lds + (cu >> 1) * PLANE + (cu & 1) * 16;
  // (row, column) of the unit's pixel relative to the tile's first one, in
  // the tensor it is read from; the same for every tile
  int rc[NLD];
#pragma unroll
  for (int k = 0; k < NLD; ++k) {
    const int p = (t >> 3) + k * 32;
    int dr, dc;
    if (p < NPX) {
      const int e = p % LW;
      dr = p / LW - 1;
      dc = (STRIDE == 1 ? e : e <= GW_TW ? 2 * e : 2 * (e - GW_TW - 1) + 1) - 1;
    } else {
      dr = (p - NPX) >> 4;
      dc = (p - NPX) & 15;
    }
    rc[k] = dr * 65536 + (dc & 0xffff);
  }
  uint4 v[NLD];
  auto load_tile = [&](int tile) {
    const int tw = tile % g.tilesW, rest = tile / g.tilesW;
    const int th = rest % g.tilesH, n = rest / g.tilesH;
    const int h0 = th * TH, w0 = tw * GW_TW;
    const bf16* xb = x + (long)n * g.H * g.W * g.C + c0 + cu * 8;
    const bf16* yb = dy + (long)n * g.OH * g.OW * g.C + c0 + cu * 8;
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int p = (t >> 3) + k * 32;
      const int dr = rc[k] >> 16, dc = (short)(rc[k] & 0xffff);
      const bool isx = p < NPX;
      const int r = (isx ? h0 * STRIDE : h0) + dr;
      const int c = (isx ? w0 * STRIDE : w0) + dc;
      const int nr = isx ? g.H : g.OH, nc = isx ? g.W : g.OW;
      const bool ok = p < NPIX && cok && r >= 0 && r < nr && c >= 0 && c < nc;
      v[k] = make_uint4(0, 0, 0, 0);
      if (ok) v[k] = *(const uint4*)((isx ? xb : yb) + ((long)r * nc + c) * g.C);
    }
  };

  constexpr int NACC = 9 * NB;
  epi_f32x4 acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; ++a) acc[a] = {0.f, 0.f, 0.f, 0.f};
  // the wave's planes: dY quarter `wave`; X quarter `wave` (CW = 16) or both
  // quarters of window wave >> 1 (CW = 32)
  const char* const ybase = lds + wave * PLANE + NPX * GW_PIX + lane * 8;
  const char* const xbase =
      lds + (CW == 16 ? wave : (wave >> 1) * 2) * PLANE + lane * 8;

  if (tile0 < tile1) load_tile(tile0);
  for (int tile = tile0; tile < tile1; ++tile) {
    __syncthreads();  // the previous tile's reads are done
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int p = (t >> 3) + k * 32;
      if (p < NPIX) *(uint4*)(sdst + p * GW_PIX) = v[k];
    }
    __syncthreads();
    if (tile + 1 < tile1) load_tile(tile + 1);  // in flight under the MFMAs
    if (active) {
      // (K-step, tap) flattened; step s + 1's fragments are read before step
      // s's MFMAs issue, and the fences keep it at that: two sets of B
      // fragments live, not a K-step's worth
      constexpr int NSTEP = TH / 2 * 9;
      auto read_a = [&](int ks) {
        return gw_frag(ybase + 2 * ks * GW_TW * GW_PIX,
                       ybase + (2 * ks + 1) * GW_TW * GW_PIX);
      };
      auto read_x = [&](int s, bf16x8* f) {
        const int i = s / 9 * 2, kh = s % 9 / 3, kw = s % 3;
#pragma unroll
        for (int b = 0; b < NB; ++b)
          f[b] = gw_frag(
              xbase + b * PLANE + gw_xoff<STRIDE>(i, kh, kw) * GW_PIX,
              xbase + b * PLANE + gw_xoff<STRIDE>(i + 1, kh, kw) * GW_PIX);
      };
      bf16x8 a = read_a(0), an = a, xf[2][NB];
      read_x(0, xf[0]);
#pragma unroll
      for (int s = 0; s < NSTEP; ++s) {
        if (s % 9 == 0) a = an;
        if (s + 1 < NSTEP) {
          read_x(s + 1, xf[(s + 1) & 1]);
          if ((s + 1) % 9 == 0) an = read_a((s + 1) / 9);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < NB; ++b)
          acc[s % 9 * NB + b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, xf[s & 1][b], acc[s % 9 * NB + b], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // ---- the group diagonal: fragment (tap, b) holds dY channel
  // wave*16 + fq*4 + r against X channel xq*16 + fr of the slab --------------
  if (!active) return;
  float* const obase = out + (long)part * g.C * (9 << g.lgS);
  const int smask = (1 << g.lgS) - 1;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int cx = (CW == 16 ? wave : (wave >> 1) * 2 + b) * 16 + fr;
    if ((cx >> g.lgS) != ((wave * 16 + fq * 4) >> g.lgS)) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* orow = obase + (long)(c0 + wave * 16 + fq * 4 + r) * (9 << g.lgS) +
                    (cx & smask);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        orow[tap << g.lgS] = acc[tap * NB + b][r];
    }
  }
}

// out[i] = parts[0][i] + ... + parts[P-1][i] in a fixed order: GW_CP lanes
// take p = lane, lane + GW_CP, ... of one float4 column, then lane 0 adds the
// GW_CP sums in lane order
__global__ void __launch_bounds__(GW_CP * GW_CP)
gconv_wgrad_collapse(const float* __restrict__ parts, float* __restrict__ out,
                     int P, long nk4) {
  __shared__ float4 red[GW_CP][GW_CP];
  const int col = threadIdx.x % GW_CP, pl = threadIdx.x / GW_CP;
  const long i = (long)blockIdx.x * GW_CP + col;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < nk4)
    for (int p = pl; p < P; p += GW_CP) {
      const float4 u = ((const float4*)parts)[(long)p * nk4 + i];
      s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
    }
  red[pl][col] = s;
  __syncthreads();
  if (pl == 0 && i < nk4) {
    for (int q = 1; q < GW_CP; ++q) {
      const float4 u = red[q][col];
      s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
    }
    ((float4*)out)[i] = s;
  }
}

}  // namespace

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

int gconv_window(long C, long groups, const char* op);  // gconv.hip

// Blocks per slab.  The kernel streams its input once, so it wants every CU
// busy, but each block also writes a [64][9][S] partial that the collapse
// reads back.  GW_TARGET = 512 blocks in all (two per CU) measured fastest on
// all five resnext50_32x4d shapes swept at batch 256, against 256, 1024 and
// 2048 (docs/KERNELS.md); at least GW_MIN_TILES tiles per block keep the
// partials small beside the input on tiny problems.
constexpr long GW_TARGET = 512, GW_MIN_TILES = 4;

static long gconv_wgrad_split(long T, long nslab) {
  const long want = (GW_TARGET + nslab - 1) / nslab;
  return std::max<long>(1, std::min<long>(want, T / GW_MIN_TILES));
}

at::Tensor gconv3x3_wgrad(at::Tensor dy2d, at::Tensor x2d, long Nn, long H,
                          long W, long stride, long groups, long nsplit) {
  // H, W: the INPUT's; x2d is [Nn*H*W, C], dy2d [Nn*Hout*Wout, C]; returns
  // dW [C, S, 3, 3] fp32 in channels_last memory ([C][3][3][S])
  const char* op = "gconv3x3_wgrad";
  for (const at::Tensor* r : {&x2d, &dy2d})
    TORCH_CHECK(r->is_cuda() && r->scalar_type() == at::kBFloat16 &&
                    r->dim() == 2 && r->is_contiguous(),
                op, ": rows must be a contiguous CUDA bf16 [R, C] tensor");
  TORCH_CHECK(dy2d.device() == x2d.device(), op, ": dY is on ", dy2d.device(),
              ", X on ", x2d.device());
  TORCH_CHECK(stride == 1 || stride == 2, op, ": stride must be 1 or 2, got ",
              stride);
  const long C = x2d.size(1);
  TORCH_CHECK(dy2d.size(1) == C, op, ": dY has ", dy2d.size(1),
              " channels, X has ", C, " (Cin must equal Cout)");
  const int cw = gconv_window(C, groups, op);
  const long S = C / groups;
  const long Hout = (H + 2 - 3) / stride + 1, Wout = (W + 2 - 3) / stride + 1;
  TORCH_CHECK(Nn > 0 && H > 0 && W > 0 && x2d.size(0) == Nn * H * W, op,
              ": X has ", x2d.size(0), " rows, expected ", Nn, " x ", H, " x ",
              W);
  TORCH_CHECK(dy2d.size(0) == Nn * Hout * Wout, op, ": dY has ", dy2d.size(0),
              " rows, expected ", Nn, " x ", Hout, " x ", Wout);
  TORCH_CHECK(nsplit >= 0, op, ": nsplit must be >= 0, got ", nsplit);

  const int th = stride == 2 ? GwTile<2>::TH : GwTile<1>::TH;
  GwGeom g;
  g.C = (int)C;
  g.lgS = S == 4 ? 2 : S == 8 ? 3 : S == 16 ? 4 : 5;
  g.H = (int)H;
  g.W = (int)W;
  g.OH = (int)Hout;
  g.OW = (int)Wout;
  g.tilesH = (int)((Hout + th - 1) / th);
  g.tilesW = (int)((Wout + GW_TW - 1) / GW_TW);
  g.nslab = (int)((C + GW_SLAB - 1) / GW_SLAB);
  const long T = Nn * g.tilesH * g.tilesW;
  TORCH_CHECK(T < (1L << 31), op, ": too many tiles (", T, ")");
  const long P = nsplit > 0 ? std::min(nsplit, T)
                            : gconv_wgrad_split(T, g.nslab);
  TORCH_CHECK(P * g.nslab < (1L << 31), op, ": too many blocks (",
              P * g.nslab, ")");
  g.T = (int)T;
  g.P = (int)P;

  auto fopt = x2d.options().dtype(at::kFloat);
  auto out = at::empty({C, S, 3, 3}, fopt, at::MemoryFormat::ChannelsLast);
  const long nk = C * 9 * S;
  at::Tensor parts;
  if (P > 1) parts = at::empty({P, nk}, fopt);
  float* dst = P > 1 ? parts.data_ptr<float>() : out.data_ptr<float>();
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* yp = (const bf16*)dy2d.const_data_ptr();
  const bf16* xp = (const bf16*)x2d.const_data_ptr();
  const int grid = (int)(P * g.nslab);
  if (cw == 16 && stride == 1)
    gconv3x3_wgrad_kernel<16, 1><<<grid, GW_TPB, 0, stream>>>(yp, xp, dst, g);
  else if (cw == 16)
    gconv3x3_wgrad_kernel<16, 2><<<grid, GW_TPB, 0, stream>>>(yp, xp, dst, g);
  else if (stride == 1)
    gconv3x3_wgrad_kernel<32, 1><<<grid, GW_TPB, 0, stream>>>(yp, xp, dst, g);
  else
    gconv3x3_wgrad_kernel<32, 2><<<grid, GW_TPB, 0, stream>>>(yp, xp, dst, g);
  CHECK_CUDA_OK();
  if (P > 1) {
    const long nk4 = nk / 4;
    gconv_wgrad_collapse<<<(int)((nk4 + GW_CP - 1) / GW_CP), GW_CP * GW_CP, 0,
                           stream>>>(dst, out.data_ptr<float>(), (int)P, nk4);
    CHECK_CUDA_OK();
  }
  return out;
}
