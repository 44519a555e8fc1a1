// Implicit-GEMM 3x3 convolution (NHWC, pad 1, stride 1/2) for gfx950 —
// forward and dgrad (SURVEY §2c "Conv2d 3x3 ... 16 call sites/fwd"); the
// weight gradient is the 9-tap gather form of tn2_wgrad (wgrad.hip).
//
// GEMM view over rows m = (n, ho, wo):
//   fwd:   Y[m, cout] = sum_{tap, cin} X[gather(m, tap), cin] * W[cout, tap, cin]
//   dgrad: dX[m, cin] = sum_{tap, cout} dY[gather'(m, tap), cout] * W'[cin, tap, cout]
//          (W' is the 180-degree-rotated, [Cin, 9*Cout]-permuted weight)
//
// Same block structure as gemm.hip (128x128 tile, BK=32 within one tap —
// all ResNet channel counts are multiples of 32 — 4 waves of 4x4
// mfma_f32_16x16x32_bf16 fragments, global_load_lds staging).  Padding is
// handled with a 16 B zero page: out-of-bounds gather rows load from it, so
// no LDS pre-zeroing pass and no boundary branches in the MFMA loop.
//
// Two variants avoid MFMA work on operands that are zero by construction:
// outputs of <= 64 channels run a 64-wide n-tile (NT = 64), and the
// stride-2 dgrad tiles each (h&1, w&1) parity class on its own and walks
// only that class's taps (PAR).  Both reproduce the 128-wide all-taps
// loop value for value.
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

struct ConvGeom {
  int H, W, Hout, Wout, stride;  // input / output spatial dims
};

// dgrad gather: input row m=(n,h,w), tap (kh,kw) -> dY row or -1
// (H,W = input dims; Hout,Wout = dY dims)
__device__ __forceinline__ long dgrad_gather(long m, int kh, int kw,
                                             const ConvGeom& g) {
  long t = m;
  const int w = (int)(t % g.W); t /= g.W;
  const int h = (int)(t % g.H); t /= g.H;
  const int ho2 = h + 1 - kh, wo2 = w + 1 - kw;
  if (g.stride == 1) {
    if (ho2 < 0 || ho2 >= g.Hout || wo2 < 0 || wo2 >= g.Wout) return -1;
    return (t * g.Hout + ho2) * g.Wout + wo2;
  }
  if ((ho2 & 1) || (wo2 & 1)) return -1;
  const int ho = ho2 >> 1, wo = wo2 >> 1;
  if (ho < 0 || ho >= g.Hout || wo < 0 || wo >= g.Wout) return -1;
  return (t * g.Hout + ho) * g.Wout + wo;
}

// per-unit precomputed pixel coordinates: the output-row decode (div/mod
// chains) is tap-invariant, so it is hoisted out of the K-loop entirely
struct UnitCoord {
  long n_off;  // n * H * W (input-row base for this image)
  int hb, wb;  // tap-0 pixel coords (may be negative / out of range)
};

// PAR (stride-2 dgrad, even H and W): m is a row of parity class
// cls = (h&1)*2 + (w&1), ordered (n, h>>1, w>>1) within the class
template <bool DGRAD, bool PAR = false>
__device__ __forceinline__ UnitCoord decode_unit(long m, const ConvGeom& g,
                                                 int cls = 0) {
  UnitCoord u;
  long t = m;
  if (PAR) {
    const int W2 = g.W >> 1, H2 = g.H >> 1;
    const int w2 = (int)(t % W2); t /= W2;
    const int h2 = (int)(t % H2); t /= H2;
    u.n_off = t * (long)g.Hout * g.Wout;
    u.hb = 2 * h2 + (cls >> 1) + 1;
    u.wb = 2 * w2 + (cls & 1) + 1;
  } else if (DGRAD) {  // m ranges over INPUT pixels; gather reads dY [Hout,Wout]
    const int w = (int)(t % g.W); t /= g.W;
    const int h = (int)(t % g.H); t /= g.H;
    u.n_off = t * (long)g.Hout * g.Wout;
    u.hb = h + 1;  // minus kh per tap
    u.wb = w + 1;
  } else {      // m ranges over OUTPUT pixels; gather reads X [H,W]
    const int wo = (int)(t % g.Wout); t /= g.Wout;
    const int ho = (int)(t % g.Hout); t /= g.Hout;
    u.n_off = t * (long)g.H * g.W;
    u.hb = ho * g.stride - 1;  // plus kh per tap
    u.wb = wo * g.stride - 1;
  }
  return u;
}

template <bool DGRAD, bool PAR = false>
__device__ __forceinline__ long unit_row(const UnitCoord& u, int kh, int kw,
                                         const ConvGeom& g) {
  if (DGRAD) {
    int ho2 = u.hb - kh, wo2 = u.wb - kw;
    if (PAR) {  // the block only walks taps of its class's parity
      ho2 >>= 1;
      wo2 >>= 1;
    } else if (g.stride == 2) {
      if ((ho2 | wo2) & 1) return -1;
      ho2 >>= 1;
      wo2 >>= 1;
    }
    if (ho2 < 0 || ho2 >= g.Hout || wo2 < 0 || wo2 >= g.Wout) return -1;
    return u.n_off + (long)ho2 * g.Wout + wo2;
  }
  const int h = u.hb + kh, w = u.wb + kw;
  if (h < 0 || h >= g.H || w < 0 || w >= g.W) return -1;
  return u.n_off + (long)h * g.W + w;
}

// BKT = K-step depth (32 or 64): BKT/8 16-B units per m-row, BKT/16 rounds
template <bool DGRAD, int BKT, bool PAR = false>
__device__ __forceinline__ void stage_gathered(
    const bf16* __restrict__ src, int ld, const UnitCoord* uc, int c0, int kh,
    int kw, const ConvGeom& g, const bf16* __restrict__ zero_page,
    bf16* lds) {
  const int t = threadIdx.x;
  constexpr int UPR = BKT / 8;
#pragma unroll
  for (int rnd = 0; rnd < BKT / 16; ++rnd) {
    int unit = rnd * GEMM_TPB + t;
    long row = unit_row<DGRAD, PAR>(uc[rnd], kh, kw, g);
    const bf16* p = row < 0 ? zero_page
                            : src + row * (long)ld + c0 +
                                  (unit % UPR) * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)p,
        (__attribute__((address_space(3))) unsigned int*)(lds + unit * 8), 16,
        0, 0);
  }
}

// stage a [128 rows][32 cols] tile of a plain [Rows x ld] matrix at column
// offset koff (weights)
// stage ROWS x BKT (ROWS=64 for the NT=64 tile: half the units)
template <int BKT, int ROWS>
__device__ __forceinline__ void stage_plain_rows(
    const bf16* __restrict__ gsrc, long ld, long row0, long rows, long koff,
    bf16* lds) {
  const int t = threadIdx.x;
  constexpr int UPR = BKT / 8;
  constexpr int UNITS = ROWS * UPR;
#pragma unroll
  for (int rnd = 0; rnd < UNITS / GEMM_TPB; ++rnd) {
    int unit = rnd * GEMM_TPB + t;
    long row = row0 + unit / UPR;
    if (row >= rows) row = rows - 1;
    const bf16* src = gsrc + row * ld + koff + (unit % UPR) * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(lds + unit * 8), 16,
        0, 0);
  }
}

template <int BKT>
__device__ __forceinline__ void stage_plain(
    const bf16* __restrict__ gsrc, long ld, long row0, long rows, long koff,
    bf16* lds) {
  const int t = threadIdx.x;
  constexpr int UPR = BKT / 8;
#pragma unroll
  for (int rnd = 0; rnd < BKT / 16; ++rnd) {
    int unit = rnd * GEMM_TPB + t;
    long row = row0 + unit / UPR;
    if (row >= rows) row = rows - 1;
    const bf16* src = gsrc + row * ld + koff + (unit % UPR) * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(lds + unit * 8), 16,
        0, 0);
  }
}

// fwd / dgrad main kernel.  DGRAD only changes the gather map; operand roles:
//   fwd:   A = x rows (AC channels), B = w [NC, 9*AC], C = y [M, NC]
//   dgrad: A = dy rows (AC = Cout), B = w' [NC = Cin, 9*Cout], C = dx
// BAND: block-diagonal weight (grouped conv via the dense path, Cin==NC,
// both % 128): only the K-steps whose NT-channel window matches this
// n-tile's group window are nonzero — skip the rest.
// NT: output-tile width (128 default; 64 halves the band window and thus
// the off-diagonal waste for grouped convs — wave grid becomes 2m x 2n
// over [128m x 64n], 4x2 fragments per wave).
// DB: double-buffered (tap, ks) pipeline — stage iteration it+1's A/B
// tiles while the MFMAs consume iteration it's (one barrier per iteration
// instead of two; the barrier's implicit vmcnt(0) drains the DMA queue),
// mirroring the gemm.hip DB loop.
// PAR (stride-2 dgrad, even H and W): the M rows are ordered class-major
// over the four (h&1, w&1) parity classes and each class is tiled on its
// own, so a block's class is uniform and it walks only the taps whose
// parity reaches its pixels — kh = 1 for even h, {0, 2} for odd h, same
// for kw: 1, 2, 2 or 4 taps instead of 9, the other taps are all-zero
// gathers.  Taps stay in ascending order with the same ks order inside,
// so every output accumulates exactly the nonzero terms of the all-taps
// loop in the same order.  M is the TOTAL row count (4 classes of M/4),
// nbm = 4 * tiles-per-class; the class is the fastest block index so the
// 1/2/2/4-tap blocks interleave evenly over the XCDs.
// WIDE: the wide-store C epilogue and its B-row map (common.h); epi is the
// runtime mode of the narrow one (AMDTRAIN_EPILOGUE 0 / 1; PAR rows are
// not affine in the tile row, so the narrow PAR store has one form only).
template <bool DGRAD, int BKT = BK, bool BAND = false, int NT = 128,
          bool DB = false, bool PAR = false, bool WIDE = false>
__global__ void __launch_bounds__(GEMM_TPB, 2)
conv3x3_kernel(const bf16* __restrict__ A, const bf16* __restrict__ Bw,
               bf16* __restrict__ C, long M, int AC, int NC, ConvGeom g,
               int nbm, int nbn, const bf16* __restrict__ zero_page,
               float* __restrict__ stats, int epi) {
  static_assert(!PAR || (DGRAD && !BAND), "PAR is a dense-dgrad variant");
  constexpr int STG = (128 + NT) * BKT;  // one A+B stage
  __shared__ bf16 SMEM[(DB ? 2 : 1) * STG];
  bf16* const As = SMEM;

  const int bid = xcd_swz(blockIdx.x, nbm * nbn);
  const int bm = bid / nbn, bn = bid % nbn;
  const int cls = PAR ? (bm & 3) : 0;  // (h&1)*2 + (w&1)
  const long Mr = PAR ? (M >> 2) : M;  // rows in this block's tile space
  const long m0 = (long)(PAR ? (bm >> 2) : bm) * 128, n0 = (long)bn * NT;
  constexpr int NFR = NT / 32;  // n fragments per wave (4 at NT=128)

  const int t = threadIdx.x;
  const int wave = t / AMD_WAVE, lane = t % AMD_WAVE;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * (NT / 2);
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[4][NFR];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NFR; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // hoist the per-unit coordinate decode out of the K-loop
  UnitCoord uc[BKT / 16];
#pragma unroll
  for (int rnd = 0; rnd < BKT / 16; ++rnd) {
    long m = m0 + (rnd * GEMM_TPB + t) / (BKT / 8);
    if (m >= Mr) m = Mr - 1;
    uc[rnd] = decode_unit<DGRAD, PAR>(m, g, cls);
  }

  const int ks_lo = BAND ? (int)(n0 / BKT) : 0;
  const int ks_hi = BAND ? ks_lo + NT / BKT : AC / BKT;
  const int nks = ks_hi - ks_lo;
  // PAR: odd rows/cols take taps {0, 2}, even ones tap {1}
  const int par_h = cls >> 1, par_w = cls & 1;
  const int total = (PAR ? (1 + par_h) * (1 + par_w) : 9) * nks;
  auto stage_it = [&](int it, bf16* as) {
    int tap = it / nks;
    const int ks = ks_lo + it % nks;
    if (PAR) {  // tap index within the class -> (kh, kw), ascending
      const int khi = par_w ? (tap >> 1) : tap, kwi = par_w ? (tap & 1) : 0;
      tap = (par_h ? 2 * khi : 1) * 3 + (par_w ? 2 * kwi : 1);
    }
    const int kh = tap / 3, kw = tap % 3, c0 = ks * BKT;
    stage_gathered<DGRAD, BKT, PAR>(A, AC, uc, c0, kh, kw, g, zero_page,
                                    as);
    if (NT == 128)
      stage_plain<BKT>(Bw, (long)9 * AC, n0, NC, (long)tap * AC + c0,
                       as + 128 * BKT);
    else  // 64-row B tile: half the staging rounds
      stage_plain_rows<BKT, 64>(Bw, (long)9 * AC, n0, NC,
                                (long)tap * AC + c0, as + 128 * BKT);
  };
  auto compute_it = [&](const bf16* as) {
    const bf16* bs = as + 128 * BKT;
#pragma unroll
    for (int kk = 0; kk < BKT / 32; ++kk) {
      bf16x8 a[4], b[NFR];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a[i] = *(const bf16x8*)
            &as[(wm + i * 16 + fr) * BKT + kk * 32 + fq * 8];
#pragma unroll
      for (int j = 0; j < NFR; ++j)
        b[j] = *(const bf16x8*)
            &bs[(wn + epi_col<WIDE>(j, fr)) * BKT + kk * 32 + fq * 8];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NFR; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[i], b[j], acc[i][j], 0, 0, 0);
    }
  };
  if (DB) {
    constexpr int HB = STG;
    if (total > 0) stage_it(0, SMEM);
    for (int it = 0; it < total; ++it) {
      bf16* const as = SMEM + (it & 1) * HB;
      __syncthreads();  // implicit vmcnt(0) drains this iter's DMA; all
                        // waves are past reading the other buffer
      if (it + 1 < total) stage_it(it + 1, SMEM + ((it + 1) & 1) * HB);
      compute_it(as);
    }
  } else {
    for (int it = 0; it < total; ++it) {
      __syncthreads();
      stage_it(it, SMEM);
      __syncthreads();
      compute_it(SMEM);
    }
  }

  if (PAR && WIDE) {
    // after the quad transpose a lane holds ONE class row per m-fragment:
    // decode it to the true input row and store its 16 B runs
    const unsigned W2 = g.W >> 1, H2 = g.H >> 1;
    const long lcol = n0 + wn + (fr >> 2) * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint4 run[NFR / 2];
      epi_quad_transpose<NFR>(&acc[i][0], run, fr);
      const unsigned mr = (unsigned)m0 + wm + i * 16 + fq * 4 + (fr & 3);
      if ((long)mr < Mr) {
        const unsigned w2 = mr % W2, t2 = mr / W2;
        const unsigned h2 = t2 % H2, n = t2 / H2;
        const long row = ((long)n * g.H + 2 * h2 + par_h) * g.W + 2 * w2 +
                         par_w;
#pragma unroll
        for (int h = 0; h < NFR / 2; ++h)
          if (lcol + h * 32 + 8 <= NC)
            *(uint4*)(C + row * NC + lcol + h * 32) = run[h];
      }
    }
    return;
  }
  if (PAR) {
    // class row -> true input row; one decode per 4-row fragment group,
    // then step (w2, h2, n) with carries (host guarantees M < 2^31)
    const unsigned W2 = g.W >> 1, H2 = g.H >> 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned mr = (unsigned)m0 + wm + i * 16 + fq * 4;
      unsigned w2 = mr % W2, t2 = mr / W2;
      unsigned h2 = t2 % H2, n = t2 / H2;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if ((long)mr + r < Mr) {
          const long row = ((long)n * g.H + 2 * h2 + par_h) * g.W +
                           2 * w2 + par_w;
#pragma unroll
          for (int j = 0; j < NFR; ++j) {
            long col = n0 + wn + j * 16 + fr;
            if (col < NC)
              C[row * NC + col] = __float2bfloat16(acc[i][j][r]);
          }
        }
        if (++w2 == W2) {
          w2 = 0;
          if (++h2 == H2) {
            h2 = 0;
            ++n;
          }
        }
      }
    }
    return;
  }
  epi_store_bf16<NFR, NFR, WIDE>(C, NC, m0, M, n0, NC, wm, wn, fr, fq,
                                 &acc[0][0], epi);
  if (stats != nullptr)
    conv_epilogue_stats<NT, WIDE>(stats, (const float*)acc, m0, M, n0, NC,
                                  bm, wm, wn, fr, fq, As);
}

// permute weight [Cout, 9, Cin] -> [Cin, 9, Cout] for dgrad.
// NO 180-degree rotation here: the dgrad gather (ho = h+1-kh) already
// encodes it, so tap k pairs with W[., k, .] directly.
__global__ void __launch_bounds__(AMD_TPB)
rotate_weight_kernel(const bf16* __restrict__ w, bf16* __restrict__ out,
                     int Cout, int Cin) {
  long total = (long)Cout * 9 * Cin;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long t = i;
    const int cin = (int)(t % Cin); t /= Cin;
    const int tap = (int)(t % 9); t /= 9;
    const int cout = (int)t;
    out[((long)cin * 9 + tap) * Cout + cout] =
        w[((long)cout * 9 + tap) * Cin + cin];
  }
}

}  // namespace

// AMDTRAIN_CONV3X3_DB=0 forces the single-buffer (tap, ks) loop; default
// is the double-buffered pipeline (see kernel comment / gemm.hip).
static bool conv3x3_db_enabled() {
  static const bool v = []() {
    const char* e = std::getenv("AMDTRAIN_CONV3X3_DB");
    return !(e && e[0] == '0');
  }();
  return v;
}

// host-side 16B zero page (device memory), one per device, created lazily
static at::Tensor zero_page_for(const at::Tensor& like) {
  static thread_local at::Tensor zp;
  if (!zp.defined() || zp.device() != like.device())
    zp = at::zeros({16}, like.options().dtype(at::kBFloat16));
  return zp;
}

// one conv3x3_kernel launch; the double-buffered dense variants also exist
// with the wide-store epilogue (wide: AMDTRAIN_EPILOGUE=2 and NC % 8 == 0)
template <bool DGRAD, int BKT, bool BAND, int NT, bool DB, bool PAR = false>
static void launch_c3(bool wide, int grid, hipStream_t stream, const bf16* A,
                      const bf16* Bw, bf16* C, long M, int AC, int NC,
                      const ConvGeom& g, int nbm, int nbn, const bf16* zp,
                      float* stats, int epi) {
  if constexpr (DB && !BAND) {
    if (wide) {
      conv3x3_kernel<DGRAD, BKT, BAND, NT, DB, PAR, true>
          <<<grid, GEMM_TPB, 0, stream>>>(A, Bw, C, M, AC, NC, g, nbm, nbn,
                                          zp, stats, epi);
      return;
    }
  }
  conv3x3_kernel<DGRAD, BKT, BAND, NT, DB, PAR, false>
      <<<grid, GEMM_TPB, 0, stream>>>(A, Bw, C, M, AC, NC, g, nbm, nbn, zp,
                                      stats, epi);
}

std::vector<at::Tensor> conv3x3_fwd_stats_impl(at::Tensor x2d, long Nn,
                                                long H, long W, long stride,
                                                at::Tensor w2d,
                                                bool want_stats,
                                                bool banded = false,
                                                bool nt64 = true,
                                                long epi = -1) {
  // x2d: [Nn*H*W, Cin] bf16 NHWC rows; w2d: [Cout, 9*Cin]
  TORCH_CHECK(x2d.is_cuda() && x2d.scalar_type() == at::kBFloat16);
  long Cin = x2d.size(1), Cout = w2d.size(0);
  TORCH_CHECK(w2d.size(1) == 9 * Cin);
  TORCH_CHECK(Cin % BK == 0, "Cin must be multiple of 32");
  long Hout = (H + 2 - 3) / stride + 1, Wout = (W + 2 - 3) / stride + 1;
  long M = Nn * Hout * Wout;
  auto y = at::empty({M, Cout}, x2d.options());
  ConvGeom g{(int)H, (int)W, (int)Hout, (int)Wout, (int)stride};
  int nbm = (int)((M + 127) / 128), nbn = (int)((Cout + 127) / 128);
  auto zp = zero_page_for(x2d);
  at::Tensor stats;
  float* sp = nullptr;
  if (want_stats) {
    stats = at::empty({nbm, 2 * Cout}, x2d.options().dtype(at::kFloat));
    sp = stats.data_ptr<float>();
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  static const bool bk64 = []() {
    const char* v = std::getenv("AMDTRAIN_CONV3X3_BK64");
    return !(v && v[0] == '0');
  }();
  const bf16* xp = (const bf16*)x2d.const_data_ptr();
  const bf16* wp = (const bf16*)w2d.const_data_ptr();
  const bf16* zpp = (const bf16*)zp.const_data_ptr();
  bf16* yp = (bf16*)y.data_ptr();
  const int ci = (int)Cin, co = (int)Cout, ep = epi_mode(epi, 2);
  const bool wide = ep >= 2 && Cout % 8 == 0;
  const bool db = conv3x3_db_enabled();
  // A/B (tools/bench_conv3x3.py + in-context traces): BK64 fwd +17% at
  // layer2 (Cin=128, M=400k); layer1 (Cin=64) and layer3/4 (small M)
  // measured WORSE in-context -> Cin>=128 && large-M only
  if (banded) {  // requires Cin == Cout, both % 128 (host-checked)
    // NT=64 tile halves the group-band window (and the off-diag waste)
    int nbn64 = (int)((Cout + 63) / 64);
    if (db)
      launch_c3<false, BK, true, 64, true>(wide, nbm * nbn64, stream, xp, wp,
                                           yp, M, ci, co, g, nbm, nbn64, zpp,
                                           sp, ep);
    else
      launch_c3<false, BK, true, 64, false>(wide, nbm * nbn64, stream, xp,
                                            wp, yp, M, ci, co, g, nbm, nbn64,
                                            zpp, sp, ep);
  } else if (nt64 && Cout <= 64 && db) {
    // narrow output (layer 1): the 64-wide n-tile issues no MFMAs on the
    // clamped B rows 64..127 of the 128-wide tile; per-element K order
    // and per-block row sets are unchanged, so y and the stats partials
    // equal the 128-wide tile's
    launch_c3<false, BK, false, 64, true>(wide, nbm, stream, xp, wp, yp, M,
                                          ci, co, g, nbm, 1, zpp, sp, ep);
  } else if (bk64 && Cin % 64 == 0 && Cin >= 128 && M >= 200000) {
    if (db)
      launch_c3<false, 64, false, 128, true>(wide, nbm * nbn, stream, xp, wp,
                                             yp, M, ci, co, g, nbm, nbn, zpp,
                                             sp, ep);
    else
      launch_c3<false, 64, false, 128, false>(wide, nbm * nbn, stream, xp,
                                              wp, yp, M, ci, co, g, nbm, nbn,
                                              zpp, sp, ep);
  } else if (db)
    launch_c3<false, BK, false, 128, true>(wide, nbm * nbn, stream, xp, wp,
                                           yp, M, ci, co, g, nbm, nbn, zpp,
                                           sp, ep);
  else
    launch_c3<false, BK, false, 128, false>(wide, nbm * nbn, stream, xp, wp,
                                            yp, M, ci, co, g, nbm, nbn, zpp,
                                            sp, ep);
  CHECK_CUDA_OK();
  if (want_stats) return {y, stats};
  return {y};
}

at::Tensor conv3x3_fwd(at::Tensor x2d, long Nn, long H, long W, long stride,
                       at::Tensor w2d, bool nt64, long epi) {
  return conv3x3_fwd_stats_impl(x2d, Nn, H, W, stride, w2d, false, false,
                                nt64, epi)[0];
}

std::vector<at::Tensor> conv3x3_fwd_stats(at::Tensor x2d, long Nn, long H,
                                          long W, long stride,
                                          at::Tensor w2d, bool banded,
                                          bool nt64, long epi) {
  TORCH_CHECK(!banded || (x2d.size(1) == w2d.size(0) &&
                          x2d.size(1) % 128 == 0),
              "banded conv3x3 needs Cin == Cout, both % 128");
  return conv3x3_fwd_stats_impl(x2d, Nn, H, W, stride, w2d, true, banded,
                                nt64, epi);
}

// s2parity: stride-2 calls with even H and W run the parity-class tiling
// (conv3x3_kernel PAR); nt64: Cin <= 64 runs the 64-wide n-tile.  Both are
// value-for-value equal to the all-taps 128-wide loop and need the
// double-buffered pipeline (AMDTRAIN_CONV3X3_DB=0 keeps the old loop).
at::Tensor conv3x3_dgrad(at::Tensor dy2d, long Nn, long H, long W,
                         long stride, at::Tensor w2d, bool banded,
                         bool s2parity, bool nt64, long epi) {
  // dy2d: [Nn*Hout*Wout, Cout]; returns dx2d [Nn*H*W, Cin]
  long Cout = dy2d.size(1), Cin = w2d.size(1) / 9;
  TORCH_CHECK(w2d.size(0) == Cout && w2d.size(1) == 9 * Cin);
  TORCH_CHECK(Cout % BK == 0);
  long Hout = (H + 2 - 3) / stride + 1, Wout = (W + 2 - 3) / stride + 1;
  long M = Nn * H * W;
  auto stream = at::cuda::getCurrentCUDAStream();
  // build rotated-permuted weight W' [Cin, 9*Cout]
  auto wrot = at::empty({Cin, 9 * Cout}, w2d.options());
  rotate_weight_kernel<<<amd_grid(Cout * 9 * Cin), AMD_TPB, 0, stream>>>(
      (const bf16*)w2d.const_data_ptr(), (bf16*)wrot.data_ptr(), (int)Cout,
      (int)Cin);
  CHECK_CUDA_OK();
  auto dx = at::empty({M, Cin}, dy2d.options());
  ConvGeom g{(int)H, (int)W, (int)Hout, (int)Wout, (int)stride};
  int nbm = (int)((M + 127) / 128), nbn = (int)((Cin + 127) / 128);
  auto zp = zero_page_for(dy2d);
  const bf16* yp = (const bf16*)dy2d.const_data_ptr();
  const bf16* wp = (const bf16*)wrot.const_data_ptr();
  const bf16* zpp = (const bf16*)zp.const_data_ptr();
  bf16* xp = (bf16*)dx.data_ptr();
  const int ci = (int)Cin, co = (int)Cout, ep = epi_mode(epi, 2);
  const bool wide = ep >= 2 && Cin % 8 == 0;
  const bool db = conv3x3_db_enabled();
  if (banded) {
    TORCH_CHECK(Cin == Cout && Cin % 128 == 0);
    // NT=64 tile: the group-diagonal K window shrinks to 64 channels,
    // halving the off-diagonal waste vs the 128-wide tile
    int nbn64 = (int)(Cin / 64);
    if (db)
      launch_c3<true, BK, true, 64, true>(wide, nbm * nbn64, stream, yp, wp,
                                          xp, M, co, ci, g, nbm, nbn64, zpp,
                                          nullptr, ep);
    else
      launch_c3<true, BK, true, 64, false>(wide, nbm * nbn64, stream, yp, wp,
                                           xp, M, co, ci, g, nbm, nbn64, zpp,
                                           nullptr, ep);
    CHECK_CUDA_OK();
    return dx;
  }
  static const bool bk64d = []() {  // measured negative for dgrad: off
    const char* v = std::getenv("AMDTRAIN_CONV3X3_BK64D");
    return v && v[0] == '1';
  }();
  const bool par = s2parity && stride == 2 && H % 2 == 0 && W % 2 == 0 &&
                   M < (1L << 31) && db;
  const bool n64 = nt64 && Cin <= 64 && db;
  if (par) {
    // four parity classes of M/4 rows, each tiled on its own
    const int nbmp = 4 * (int)((M / 4 + 127) / 128);
    if (n64)
      launch_c3<true, BK, false, 64, true, true>(wide, nbmp, stream, yp, wp,
                                                 xp, M, co, ci, g, nbmp, 1,
                                                 zpp, nullptr, ep);
    else
      launch_c3<true, BK, false, 128, true, true>(wide, nbmp * nbn, stream,
                                                  yp, wp, xp, M, co, ci, g,
                                                  nbmp, nbn, zpp, nullptr,
                                                  ep);
  } else if (n64)
    launch_c3<true, BK, false, 64, true>(wide, nbm, stream, yp, wp, xp, M,
                                         co, ci, g, nbm, 1, zpp, nullptr,
                                         ep);
  else if (bk64d && Cout % 64 == 0)
    launch_c3<true, 64, false, 128, false>(wide, nbm * nbn, stream, yp, wp,
                                           xp, M, co, ci, g, nbm, nbn, zpp,
                                           nullptr, ep);
  else if (db)
    launch_c3<true, BK, false, 128, true>(wide, nbm * nbn, stream, yp, wp,
                                          xp, M, co, ci, g, nbm, nbn, zpp,
                                          nullptr, ep);
  else
    launch_c3<true, BK, false, 128, false>(wide, nbm * nbn, stream, yp, wp,
                                           xp, M, co, ci, g, nbm, nbn, zpp,
                                           nullptr, ep);
  CHECK_CUDA_OK();
  return dx;
}
