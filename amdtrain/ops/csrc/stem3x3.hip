// Direct 3x3 stride-2 pad-1 conv of a 3-channel (RGB) image for gfx950: the
// stem of every mobile-class net.  bf16 in, fp32 accumulation, the raw
// channels-last input [N,H,W,3] at 6 bytes per pixel, never a channel-padded
// copy.  Cout is any multiple of 8 from 8 to 64.
//
// The whole reduction is K = 3*3*3 = 27 <= 32: one v_mfma_f32_16x16x32_bf16
// step per 16 pixels x 16 output channels.  The layer is memory-bound, so the
// kernels are built around moving x once and y (or dY) once.
//
//  * Geometry (forward and weight gradient): a block of 256 threads owns a
//    rectangle of S3_TH x S3_TW = 8 x 32 output pixels of one image and
//    stages its input halo, 17 rows x 65 pixels x 3 channels, into LDS once.
//    The pad-1 border and everything outside the image are zeros there, so
//    the MFMA loops carry no bounds tests on x.
//  * Halo row in LDS: 5 lead elements, then halo pixel 0 (input pixel
//    2*wo0 - 1), then 64 body pixels; 200 bf16 = 400 B per row.  The lead puts
//    the body at a 16-byte offset.  When W % 8 == 0 and x is 16-byte aligned,
//    the body of every row starts 16-byte aligned in memory as well (a row is
//    6*W bytes, a tile 384 B), and a 16-byte unit lies wholly inside or
//    outside its image row: the fast route moves the body as 24 uint4 per
//    row and the 3 elements of halo pixel 0 on their own.  Every other shape
//    takes the element route, one bounds-tested bf16 at a time.
//  * k = (kh*3 + kw)*3 + c: the nine (kw, c) values of kernel row kh are nine
//    consecutive bf16 of halo row 2*ho + kh, from element 6*wo of the row.
//    A lane's 8 consecutive k are 8 two-byte LDS reads at offsets fixed per
//    lane before the loop; k = 27..31 are masked to zero in registers.
//  * Forward: the weight is the A operand (16 channels x 32 k), the pixels
//    the B operand (16 pixels of one output row x 32 k), so the accumulator
//    gives a lane 4 channels of ONE pixel.  Two 16-channel tiles form a
//    32-channel pair whose A rows are permuted, row i of tile j holding
//    channel (i>>2)*8 + j*4 + (i&3): lane (fr, fq) then owns channels
//    fq*8 .. fq*8+7 of pixel fr, one 16-byte store, and the 16 lanes x 4
//    quads of a wave instruction write 16 consecutive rows of y.  A Cout
//    that is not a multiple of 32 masks the quads at or beyond Cout.  The
//    weight, K-padded to 32 on the host, stays in registers: 2 fragments per
//    32 channels.  A wave owns 2 output rows of the tile, 4 MFMA tiles.
//  * Statistics (STATS): per-block (sum, sumsq) of the fp32 accumulators,
//    pixels outside the image masked to zero: per lane over its tiles, a
//    16-lane butterfly over the pixels, the 4 waves added in wave order.
//    Row `block` of [blocks][2*Cout], the layout of pw_gemm's partials.
//  * Weight gradient: dW[co][k] = sum over pixels of dY[pixel][co] *
//    xcol[pixel][k].  The dY tile goes through LDS ([pixel][Cout + 8]), rows
//    outside the image as zeros, which is what masks ragged tiles.  One
//    output row of the tile is 32 pixels = one MFMA K: A = dY^T (16 channels
//    x 32 pixels), B = xcol (32 pixels x 16 taps, two tap tiles for the 27).
//    Fragments are plain two-byte LDS reads (pixel stride).  A block walks a
//    fixed contiguous run of tiles with its accumulators in registers, adds
//    its 4 waves in wave order and writes one [Cout][32] fp32 partial;
//    s3_fold_kernel adds the partials, 8 contiguous groups in ascending block
//    order, then the 8 group sums in ascending order.
//  * No atomics; grids and summation orders depend on the shape only, so two
//    calls give the same bits.  All offsets into x, y and dY are 64-bit.
#include <climits>

#include "common.h"

namespace {

using bf16 = __hip_bfloat16;
using u16 = unsigned short;
using bf16x8 = __attribute__((ext_vector_type(8))) short;  // MFMA A/B frag

constexpr int S3_TH = 8, S3_TW = 32;    // output pixels per block
constexpr int S3_HR = 2 * S3_TH + 1;    // halo rows
constexpr int S3_HE = (2 * S3_TW + 1) * 3;  // halo elements per row
constexpr int S3_LEAD = 5;              // body at element 8 = byte 16
constexpr int S3_PITCH = S3_LEAD + S3_HE;   // 200 bf16
constexpr int S3_BODY_UNITS = 2 * S3_TW * 3 / 8;  // 16-byte units per row
constexpr int S3_WGRAD_BLOCKS = 1024;   // cap of the wgrad grid
static_assert(S3_PITCH % 8 == 0, "halo rows keep 16-byte alignment");
static_assert(S3_TH == 2 * (AMD_TPB / AMD_WAVE), "a wave owns 2 tile rows");
static_assert(S3_TW == 32, "one tile row is one MFMA K of the wgrad");

__device__ __forceinline__ bf16x8 s3_frag(unsigned a, unsigned b, unsigned c,
                                          unsigned d) {
  union { uint4 u; bf16x8 v; } f;
  f.u = make_uint4(a, b, c, d);
  return f.v;
}

// Stage the halo of tile (ho0, wo0) of image n: zeros outside the image.
__device__ __forceinline__ void s3_stage_halo(u16* __restrict__ hal,
                                              const u16* __restrict__ x,
                                              long n, int H, int W, int ho0,
                                              int wo0, bool fast) {
  const int t = threadIdx.x;
  const int hi0 = 2 * ho0 - 1;
  const long rowlen = 3L * W;
  if (fast) {
    const long e0 = 6L * wo0;  // element of the body's first pixel in a row
    for (int idx = t; idx < S3_HR * S3_BODY_UNITS; idx += AMD_TPB) {
      const int r = idx / S3_BODY_UNITS, u = idx - r * S3_BODY_UNITS;
      const int hi = hi0 + r;
      const long e = e0 + u * 8;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (hi >= 0 && hi < H && e < rowlen)
        v = *(const uint4*)(x + (n * H + hi) * rowlen + e);
      *(uint4*)&hal[r * S3_PITCH + S3_LEAD + 3 + u * 8] = v;
    }
    for (int idx = t; idx < S3_HR * 3; idx += AMD_TPB) {
      const int r = idx / 3, c = idx - r * 3;
      const int hi = hi0 + r;
      u16 v = 0;
      if (hi >= 0 && hi < H && wo0 > 0)
        v = x[(n * H + hi) * rowlen + e0 - 3 + c];
      hal[r * S3_PITCH + S3_LEAD + c] = v;
    }
    return;
  }
  const long e0 = 6L * wo0 - 3;  // element of halo pixel 0 in a row
  for (int idx = t; idx < S3_HR * S3_HE; idx += AMD_TPB) {
    const int r = idx / S3_HE, c = idx - r * S3_HE;
    const int hi = hi0 + r;
    const long e = e0 + c;
    u16 v = 0;
    if (hi >= 0 && hi < H && e >= 0 && e < rowlen)
      v = x[(n * H + hi) * rowlen + e];
    hal[r * S3_PITCH + S3_LEAD + c] = v;
  }
}

// halo offset of reduction index k (clamped to the 27 real ones) relative to
// element 6*wo of halo row 2*ho
__device__ __forceinline__ int s3_koff(int k) {
  const int kc = min(k, 26);
  const int kh = kc / 9;
  return kh * S3_PITCH + (kc - 9 * kh);
}

template <int NP, bool STATS>
__global__ void __launch_bounds__(AMD_TPB)
s3_fwd_kernel(const u16* __restrict__ x, const bf16* __restrict__ w32,
              bf16* __restrict__ y, float* __restrict__ stats, int H, int W,
              int Ho, int Wo, int Cout, int tH, int tW, int fast) {
  __shared__ __attribute__((aligned(16))) u16 hal[S3_HR * S3_PITCH];
  __shared__ float red[STATS ? 4 * 128 : 1];

  const int t = threadIdx.x;
  const int wave = t / AMD_WAVE, lane = t % AMD_WAVE;
  const int fr = lane & 15, fq = lane >> 4;
  const int blk = blockIdx.x;
  const int tw = blk % tW, th = (blk / tW) % tH;
  const long n = blk / (tW * tH);
  const int ho0 = th * S3_TH, wo0 = tw * S3_TW;

  // A fragments: the weight, rows permuted inside each 32-channel pair
  bf16x8 wf[NP][2];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ch = p * 32 + (fr >> 2) * 8 + j * 4 + (fr & 3);
      wf[p][j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (ch < Cout) wf[p][j] = *(const bf16x8*)(w32 + ch * 32 + fq * 8);
    }

  int off[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) off[i] = s3_koff(fq * 8 + i);
  // k = 27..31 (elements 3..7 of quad 3) are zeros
  const unsigned m1 = fq == 3 ? 0x0000FFFFu : 0xFFFFFFFFu;
  const unsigned m23 = fq == 3 ? 0u : 0xFFFFFFFFu;

  s3_stage_halo(hal, x, n, H, W, ho0, wo0, fast != 0);
  __syncthreads();

  float s1[NP][8], s2[NP][8];
  if constexpr (STATS) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int c = 0; c < 8; ++c) s1[p][c] = s2[p][c] = 0.f;
  }

#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int hl = wave * 2 + rr, ho = ho0 + hl;
    if (ho >= Ho) continue;  // wave-uniform
#pragma unroll
    for (int seg = 0; seg < 2; ++seg) {
      if (wo0 + seg * 16 >= Wo) continue;  // wave-uniform
      const int wl = seg * 16 + fr, wo = wo0 + wl;
      const u16* b = hal + 2 * hl * S3_PITCH + S3_LEAD + 6 * wl;
      const bf16x8 pix = s3_frag(
          (unsigned)b[off[0]] | ((unsigned)b[off[1]] << 16),
          ((unsigned)b[off[2]] | ((unsigned)b[off[3]] << 16)) & m1,
          ((unsigned)b[off[4]] | ((unsigned)b[off[5]] << 16)) & m23,
          ((unsigned)b[off[6]] | ((unsigned)b[off[7]] << 16)) & m23);
      const bool live = wo < Wo;
      bf16* yrow = y + ((n * Ho + ho) * Wo + wo) * Cout;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        epi_f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[p][0], pix, a0, 0, 0,
                                                     0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[p][1], pix, a1, 0, 0,
                                                     0);
        const int ch0 = p * 32 + fq * 8;
        if (live && ch0 < Cout)
          *(uint4*)(yrow + ch0) = make_uint4(
              epi_pack_bf16(a0[0], a0[1]), epi_pack_bf16(a0[2], a0[3]),
              epi_pack_bf16(a1[0], a1[1]), epi_pack_bf16(a1[2], a1[3]));
        if constexpr (STATS) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v0 = live ? a0[r] : 0.f, v1 = live ? a1[r] : 0.f;
            s1[p][r] += v0;
            s2[p][r] += v0 * v0;
            s1[p][4 + r] += v1;
            s2[p][4 + r] += v1 * v1;
          }
        }
      }
    }
  }

  if constexpr (STATS) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float a = s1[p][c], b = s2[p][c];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
          a += __shfl_xor(a, m, AMD_WAVE);
          b += __shfl_xor(b, m, AMD_WAVE);
        }
        if (fr == 0) {
          red[wave * 128 + p * 32 + fq * 8 + c] = a;
          red[wave * 128 + 64 + p * 32 + fq * 8 + c] = b;
        }
      }
    __syncthreads();
    if (t < 2 * Cout) {
      const int c = t < Cout ? t : 64 + (t - Cout);
      const float s = ((red[c] + red[128 + c]) + red[256 + c]) + red[384 + c];
      stats[(long)blk * 2 * Cout + t] = s;
    }
  }
}

template <int NCT>
__global__ void __launch_bounds__(AMD_TPB)
s3_wgrad_kernel(const u16* __restrict__ x, const u16* __restrict__ dy,
                float* __restrict__ part, int H, int W, int Ho, int Wo,
                int Cout, int tH, int tW, long tiles, int per, int fast) {
  extern __shared__ uint4 s3_smem[];
  u16* hal = (u16*)s3_smem;
  u16* dyt = hal + S3_HR * S3_PITCH;  // [256 pixels][Cout + 8]
  static_assert(S3_HR * S3_PITCH % 8 == 0, "dY tile is 16-byte aligned");
  const int CP = Cout + 8, units = CP / 8;

  const int t = threadIdx.x;
  const int wave = t / AMD_WAVE, lane = t % AMD_WAVE;
  const int fr = lane & 15, fq = lane >> 4;

  // B fragment of tap tile tt: lane = tap tt*16 + fr, pixels fq*8 .. +7
  int offb[2];
  unsigned kmask[2];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    offb[tt] = s3_koff(tt * 16 + fr) + S3_LEAD + 6 * (fq * 8);
    kmask[tt] = tt * 16 + fr < 27 ? 0xFFFFFFFFu : 0u;
  }

  epi_f32x4 acc[NCT][2];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) acc[ct][tt] = {0.f, 0.f, 0.f, 0.f};

  const long t0 = (long)blockIdx.x * per;
  const long t1 = t0 + per < tiles ? t0 + per : tiles;
  for (long tix = t0; tix < t1; ++tix) {
    const int tw = (int)(tix % tW), th = (int)((tix / tW) % tH);
    const long n = tix / ((long)tW * tH);
    const int ho0 = th * S3_TH, wo0 = tw * S3_TW;
    __syncthreads();  // every wave is past its reads of the previous tile
    s3_stage_halo(hal, x, n, H, W, ho0, wo0, fast != 0);
    for (int idx = t; idx < S3_TH * S3_TW * units; idx += AMD_TPB) {
      const int px = idx / units, u = idx - px * units;
      const int ho = ho0 + px / S3_TW, wo = wo0 + px % S3_TW;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (u * 8 < Cout && ho < Ho && wo < Wo)
        v = *(const uint4*)(dy + ((n * Ho + ho) * Wo + wo) * Cout + u * 8);
      *(uint4*)&dyt[px * CP + u * 8] = v;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int hl = wave * 2 + rr;
      if (ho0 + hl >= Ho) continue;  // wave-uniform: the dY rows are zeros
      bf16x8 bfrag[2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const u16* b = hal + 2 * hl * S3_PITCH + offb[tt];
        const unsigned m = kmask[tt];
        bfrag[tt] = s3_frag(
            ((unsigned)b[0] | ((unsigned)b[6] << 16)) & m,
            ((unsigned)b[12] | ((unsigned)b[18] << 16)) & m,
            ((unsigned)b[24] | ((unsigned)b[30] << 16)) & m,
            ((unsigned)b[36] | ((unsigned)b[42] << 16)) & m);
      }
      const u16* a = dyt + (hl * S3_TW + fq * 8) * CP + fr;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const u16* ac = a + ct * 16;
        const bf16x8 afrag = s3_frag(
            (unsigned)ac[0] | ((unsigned)ac[CP] << 16),
            (unsigned)ac[2 * CP] | ((unsigned)ac[3 * CP] << 16),
            (unsigned)ac[4 * CP] | ((unsigned)ac[5 * CP] << 16),
            (unsigned)ac[6 * CP] | ((unsigned)ac[7 * CP] << 16));
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
          acc[ct][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag, bfrag[tt], acc[ct][tt], 0, 0, 0);
      }
    }
  }

  // the 4 waves in wave order, through the dY tile's LDS
  __syncthreads();
  float* red = (float*)dyt;  // [4][NCT * 16][32]
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        red[((wave * NCT + ct) * 16 + fq * 4 + r) * 32 + tt * 16 + fr] =
            acc[ct][tt][r];
  __syncthreads();
  constexpr int WS = NCT * 16 * 32;  // one wave's floats
  for (int idx = t; idx < Cout * 32; idx += AMD_TPB)
    part[(long)blockIdx.x * Cout * 32 + idx] =
        ((red[idx] + red[WS + idx]) + red[2 * WS + idx]) + red[3 * WS + idx];
}

// dW[co][0..26] = the partials of row co: 8 contiguous groups of blocks, each
// in ascending block order, then the group sums in ascending order
__global__ void __launch_bounds__(AMD_TPB)
s3_fold_kernel(const float* __restrict__ part, float* __restrict__ dW,
               int nblk, int Cout) {
  __shared__ float grp[8][32];
  const int co = blockIdx.x, t = threadIdx.x;
  const int k = t & 31, g = t >> 5;
  const int chunk = (nblk + 7) / 8;
  const int lo = g * chunk, hi = min(nblk, lo + chunk);
  float s = 0.f;
  for (int b = lo; b < hi; ++b) s += part[((long)b * Cout + co) * 32 + k];
  grp[g][k] = s;
  __syncthreads();
  if (t < 27) {
    float tot = grp[0][t];
#pragma unroll
    for (int i = 1; i < 8; ++i) tot += grp[i][t];
    dW[co * 27 + t] = tot;
  }
}

struct S3Geom {
  long N, H, W, Ho, Wo, tH, tW, tiles;
  bool fast;
};

// shared host contract of both entry points
S3Geom s3_check(const char* op, const at::Tensor& x, long Cout) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, op,
              " needs a 4-d GPU tensor x [N,H,W,3]");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, op, " needs bf16 x, got ",
              x.scalar_type());
  TORCH_CHECK(x.is_contiguous(), op, " needs a contiguous x [N,H,W,3]");
  TORCH_CHECK(x.size(3) == 3, op, " needs Cin == 3, got ", x.size(3));
  TORCH_CHECK(Cout % 8 == 0, op, " needs Cout % 8 == 0, got ", Cout);
  TORCH_CHECK(Cout >= 8 && Cout <= 64, op, " needs 8 <= Cout <= 64, got ",
              Cout);
  S3Geom g;
  g.N = x.size(0), g.H = x.size(1), g.W = x.size(2);
  TORCH_CHECK(g.N == 0 || (g.H >= 1 && g.W >= 1), op, " needs H, W >= 1");
  TORCH_CHECK(g.H < (1 << 24) && g.W < (1 << 24), op, ": H or W too large");
  g.Ho = (g.H - 1) / 2 + 1, g.Wo = (g.W - 1) / 2 + 1;
  g.tH = (g.Ho + S3_TH - 1) / S3_TH, g.tW = (g.Wo + S3_TW - 1) / S3_TW;
  g.tiles = g.N * g.tH * g.tW;
  TORCH_CHECK(g.tiles <= INT_MAX, op, ": ", g.tiles, " tiles");
  g.fast = g.W % 8 == 0 && (uintptr_t)x.const_data_ptr() % 16 == 0;
  return g;
}

}  // namespace

// y [N*Ho*Wo, Cout] bf16 = conv3x3 s2 p1 of x [N,H,W,3] with w [Cout,3,3,3]
// (any strides); with want_stats also the per-block (sum, sumsq) partials
// [blocks][2*Cout] that batch_norm_fwd_train_from_parts takes.
std::vector<at::Tensor> stem3x3_fwd(at::Tensor x, at::Tensor w,
                                    bool want_stats) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 4, "stem3x3_fwd needs a 4-d GPU "
              "weight [Cout,3,3,3]");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16, "stem3x3_fwd needs a bf16 "
              "weight, got ", w.scalar_type());
  TORCH_CHECK(w.size(1) == 3, "stem3x3_fwd needs Cin == 3, got a weight "
              "with ", w.size(1), " input channels");
  TORCH_CHECK(w.size(2) == 3 && w.size(3) == 3,
              "stem3x3_fwd needs a 3x3 kernel");
  const long Cout = w.size(0);
  const S3Geom g = s3_check("stem3x3_fwd", x, Cout);
  auto fopt = x.options().dtype(at::kFloat);
  if (g.N == 0)
    return {at::empty({0, Cout}, x.options()),
            want_stats ? at::empty({0, 2 * Cout}, fopt)
                       : at::empty({0}, fopt)};
  // k = (kh*3 + kw)*3 + c, padded to 32
  auto w32 = at::constant_pad_nd(
      w.permute({0, 2, 3, 1}).reshape({Cout, 27}), {0, 5}).contiguous();
  auto y = at::empty({g.N * g.Ho * g.Wo, Cout}, x.options());
  auto stats = want_stats ? at::empty({g.tiles, 2 * Cout}, fopt)
                          : at::empty({0}, fopt);
  auto stream = at::cuda::getCurrentCUDAStream();
  const u16* xp = (const u16*)x.const_data_ptr();
  const bf16* wp = (const bf16*)w32.const_data_ptr();
  bf16* yp = (bf16*)y.data_ptr();
  float* sp = want_stats ? stats.data_ptr<float>() : nullptr;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)g.tiles), dim3(AMD_TPB), 0,
                       stream, xp, wp, yp, sp, (int)g.H, (int)g.W, (int)g.Ho,
                       (int)g.Wo, (int)Cout, (int)g.tH, (int)g.tW,
                       (int)g.fast);
  };
  if (Cout <= 32) {
    if (want_stats) launch(s3_fwd_kernel<1, true>);
    else launch(s3_fwd_kernel<1, false>);
  } else {
    if (want_stats) launch(s3_fwd_kernel<2, true>);
    else launch(s3_fwd_kernel<2, false>);
  }
  CHECK_CUDA_OK();
  return {y, stats};
}

// dW [Cout, 27] fp32 (k = (kh*3 + kw)*3 + c) from dy [N*Ho*Wo, Cout] and
// x [N,H,W,3]
at::Tensor stem3x3_wgrad(at::Tensor dy, at::Tensor x) {
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 2, "stem3x3_wgrad needs a 2-d GPU "
              "tensor dy [N*Ho*Wo, Cout]");
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16, "stem3x3_wgrad needs bf16 "
              "dy, got ", dy.scalar_type());
  TORCH_CHECK(dy.is_contiguous(), "stem3x3_wgrad needs a contiguous dy");
  const long Cout = dy.size(1);
  const S3Geom g = s3_check("stem3x3_wgrad", x, Cout);
  TORCH_CHECK(dy.size(0) == g.N * g.Ho * g.Wo, "stem3x3_wgrad: dy has ",
              dy.size(0), " rows, x gives ", g.N * g.Ho * g.Wo);
  auto fopt = x.options().dtype(at::kFloat);
  if (g.N == 0) return at::zeros({Cout, 27}, fopt);
  TORCH_CHECK((uintptr_t)dy.const_data_ptr() % 16 == 0,
              "stem3x3_wgrad needs a 16-byte aligned dy");
  const long per = (g.tiles + S3_WGRAD_BLOCKS - 1) / S3_WGRAD_BLOCKS;
  const long nblk = (g.tiles + per - 1) / per;
  auto part = at::empty({nblk, Cout, 32}, fopt);
  auto dW = at::empty({Cout, 27}, fopt);
  auto stream = at::cuda::getCurrentCUDAStream();
  const size_t lds =
      (S3_HR * S3_PITCH + S3_TH * S3_TW * (Cout + 8)) * sizeof(u16);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(AMD_TPB), lds,
                       stream, (const u16*)x.const_data_ptr(),
                       (const u16*)dy.const_data_ptr(),
                       part.data_ptr<float>(), (int)g.H, (int)g.W, (int)g.Ho,
                       (int)g.Wo, (int)Cout, (int)g.tH, (int)g.tW, g.tiles,
                       (int)per, (int)g.fast);
  };
  switch ((Cout + 15) / 16) {
    case 1: launch(s3_wgrad_kernel<1>); break;
    case 2: launch(s3_wgrad_kernel<2>); break;
    case 3: launch(s3_wgrad_kernel<3>); break;
    default: launch(s3_wgrad_kernel<4>); break;
  }
  CHECK_CUDA_OK();
  hipLaunchKernelGGL(s3_fold_kernel, dim3((unsigned)Cout), dim3(AMD_TPB), 0,
                     stream, part.data_ptr<float>(), dW.data_ptr<float>(),
                     (int)nblk, (int)Cout);
  CHECK_CUDA_OK();
  return dW;
}
