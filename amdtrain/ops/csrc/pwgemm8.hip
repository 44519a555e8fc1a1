// Pointwise (1x1 conv) MFMA GEMM for gfx950 on any channel counts that are
// multiples of 8: C[M,N] (bf16) = A[M,K] x B[N,K]^T, bf16 operands, fp32
// accumulation, K % 8 == 0 and N % 8 == 0, K and N up to a few thousand.
//
// It serves the stride-1 1x1 convs that neither gemm_bt (K % 32 == 0, and
// its input gradient N % 32 == 0) nor pw_gemm (the whole zero-padded weight
// in 16 KiB of LDS) takes: the mobile-class widths 48, 72, 88, 120, 136,
// 224, 240, 288, 528, 816 ... of MobileNetV2 at width multipliers other
// than 1.0 and of its relatives, forward (A = activation rows, B = weight)
// and input gradient (A = dY rows, B = the transposed weight).
//
//  * Block = 256 threads = 4 waves in a 2 (m) x 2 (n) grid over a
//    128 x NT tile, NT = 128 or 64; a wave owns 64 rows by NT/2 columns as
//    4 x NT/32 fragments of v_mfma_f32_16x16x32_bf16.  Two instances, not a
//    ladder: N <= 64 runs on 64 (one n-tile, no idle wave column), every
//    other N on 128, which measured ahead of 64 on most of them although it
//    pads more (docs/KERNELS.md): fewer blocks re-read the A panel.
//  * Grid = m-tiles x n-tiles, n fastest, through the XCD swizzle of
//    gemm.hip: the n-tiles of one row panel run next to each other on one
//    XCD and re-read the panel from its L2, not from memory.
//  * K loop in steps of 32 over ceil(K / 32).  A and B tiles go global ->
//    registers -> LDS, 16 B per lane and unit: a unit whose row is >= M
//    (A) or >= N (B), or whose k-pack is >= K / 8, is an exact zero made in
//    registers and never read.  Nothing is over-read, so what lies behind
//    a row (the next row, or the end of the tensor) cannot reach C.
//    The register stage is what double-buffers the loop: the loads of step
//    kt + 1 are issued before the MFMAs of step kt and written to the other
//    LDS buffer after them; one barrier per step.
//  * LDS rows are 32 + 8 bf16 (80 B) apart, the 16 B of row padding that
//    pwconv.hip uses against bank conflicts of the 16-byte fragment reads.
//  * A wave skips the MFMAs of a 32-column group that starts at or beyond N
//    (a wave-uniform branch), so the arithmetic follows ceil32(N), not NT.
//  * Epilogue: the WIDE column map and epi_store_bf16 of common.h: 16-byte
//    runs, predicated whole (N % 8 == 0: a run never straddles N) on edge
//    tiles.  Rows >= M and columns >= N are never stored.
//  * Statistics (STATS): per-block column (sum, sumsq) of the fp32
//    accumulators through conv_epilogue_stats of common.h into row bm of
//    [m-tiles][2N], each n-tile its own columns.  Tail rows and columns hold
//    exact zeros.  No atomics; grid and reduction order depend on the shape
//    and on constants only, so two calls give the same bits.
//
// All row and byte offsets are 64-bit.
#include <climits>

#include "common.h"

// the compiler's packed fp32 forms are kept out of this file's kernels
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) short;  // MFMA A/B frag

constexpr int P8_BM = 128, P8_BK = 32;
constexpr int P8_LD = P8_BK + 8;  // LDS row pitch in bf16

// gemm.hip's bijective XCD swizzle: contiguous chunks of the grid share an
// XCD, and with it an L2
__device__ __forceinline__ int p8_xcd_swizzle(int bid, int nwg) {
  constexpr int NXCD = 8;
  if (nwg < NXCD) return bid;
  const int xcd = bid % NXCD, idx = bid / NXCD;
  const int q = nwg / NXCD, r = nwg % NXCD;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

template <int NT, bool STATS>
__global__ void __launch_bounds__(AMD_TPB, 2)
pw8_gemm_kernel(const bf16* __restrict__ A, const bf16* __restrict__ B,
                bf16* __restrict__ C, long M, int K, int N, int nbm, int nbn,
                float* __restrict__ stats) {
  constexpr int NF = NT / 32;             // n-fragments per wave
  constexpr int UA = P8_BM * 4 / AMD_TPB;  // 16 B units per thread, A tile
  constexpr int UB = NT * 4 / AMD_TPB;     // and B tile
  constexpr int HB = (P8_BM + NT) * P8_LD;  // one buffer: A rows | B rows
  __shared__ __attribute__((aligned(16))) bf16 SMEM[2 * HB];
  static_assert(2 * HB * sizeof(bf16) >= 4 * NT * sizeof(float),
                "the statistics scratch reuses the staging buffers");

  const int bid = p8_xcd_swizzle(blockIdx.x, nbm * nbn);
  const int bm = bid / nbn, bn = bid % nbn;
  const long m0 = (long)bm * P8_BM;
  const int n0 = bn * NT;

  const int t = threadIdx.x;
  const int wave = t / AMD_WAVE, lane = t % AMD_WAVE;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * (NT / 2);
  const int fr = lane & 15, fq = lane >> 4;
  const int kpacks = K / 8, ksteps = (K + P8_BK - 1) / P8_BK;
  // 32-column groups of this wave that start inside N
  const int ngrp = min(NF / 2, max(0, (N - n0 - wn + 31) / 32));

  // a thread's units: rows t/4 (+64 per round), k-pack t%4 of the step
  const int urow = t >> 2, uq = t & 3;
  const bf16* ap[UA];
  const bf16* bp[UB];
#pragma unroll
  for (int u = 0; u < UA; ++u) {
    const long row = m0 + urow + u * 64;
    ap[u] = row < M ? A + row * K + uq * 8 : nullptr;
  }
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    const int row = n0 + urow + u * 64;
    bp[u] = row < N ? B + (long)row * K + uq * 8 : nullptr;
  }

  uint4 ra[UA], rb[UB];
  auto gload = [&](int kt) {
    const bool kin = kt * 4 + uq < kpacks;
#pragma unroll
    for (int u = 0; u < UA; ++u) {
      ra[u] = make_uint4(0, 0, 0, 0);
      if (kin && ap[u] != nullptr) ra[u] = *(const uint4*)(ap[u] + kt * P8_BK);
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      rb[u] = make_uint4(0, 0, 0, 0);
      if (kin && bp[u] != nullptr) rb[u] = *(const uint4*)(bp[u] + kt * P8_BK);
    }
  };
  auto lstore = [&](bf16* buf) {
#pragma unroll
    for (int u = 0; u < UA; ++u)
      *(uint4*)&buf[(urow + u * 64) * P8_LD + uq * 8] = ra[u];
#pragma unroll
    for (int u = 0; u < UB; ++u)
      *(uint4*)&buf[(P8_BM + urow + u * 64) * P8_LD + uq * 8] = rb[u];
  };

  epi_f32x4 acc[4][NF];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  auto compute = [&](const bf16* buf) {
    const bf16* bs = buf + P8_BM * P8_LD;
    bf16x8 a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      a[i] = *(const bf16x8*)&buf[(wm + i * 16 + fr) * P8_LD + fq * 8];
#pragma unroll
    for (int h = 0; h < NF / 2; ++h) {
      if (h >= ngrp) continue;  // wave-uniform
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int j = 2 * h + jj;
        const bf16x8 b = *(const bf16x8*)
            &bs[(wn + epi_col<true>(j, fr)) * P8_LD + fq * 8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[i], b, acc[i][j], 0, 0, 0);
      }
    }
  };

  gload(0);
  lstore(SMEM);
  for (int kt = 0; kt < ksteps; ++kt) {
    // the writes of buffer kt & 1 are visible, and every wave is past its
    // reads of the other buffer, which this step overwrites below
    __syncthreads();
    const bool more = kt + 1 < ksteps;
    if (more) gload(kt + 1);
    compute(SMEM + (kt & 1) * HB);
    if (more) lstore(SMEM + ((kt + 1) & 1) * HB);
  }

  epi_store_bf16<NF, NF, true>(C, N, m0, M, n0, N, wm, wn, fr, fq,
                               &acc[0][0], 2);
  if constexpr (STATS)
    conv_epilogue_stats<NT, true>(stats, (const float*)acc, m0, M, n0, N, bm,
                                  wm, wn, fr, fq, SMEM);
}

template <int NT>
void pw8_launch(bool want_stats, int nbm, int nbn, hipStream_t stream,
                const bf16* A, const bf16* B, bf16* C, long M, int K, int N,
                float* stats) {
  if (want_stats)
    hipLaunchKernelGGL((pw8_gemm_kernel<NT, true>), dim3(nbm * nbn),
                       dim3(AMD_TPB), 0, stream, A, B, C, M, K, N, nbm, nbn,
                       stats);
  else
    hipLaunchKernelGGL((pw8_gemm_kernel<NT, false>), dim3(nbm * nbn),
                       dim3(AMD_TPB), 0, stream, A, B, C, M, K, N, nbm, nbn,
                       stats);
}

}  // namespace

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// C = A x B^T (bf16, fp32 accumulation) for any K, N >= 8 that are multiples
// of 8; with want_stats also the per-block column (sum, sumsq) partials
// [ceil(M / 128)][2N] that batch_norm_fwd_train_from_parts takes.  n_tile:
// 64 or 128 forces that instance (tools/bench_pwwide.py, tests), anything
// else takes 64 for N <= 64 and 128 above.  Both give the same bits.
std::vector<at::Tensor> pw8_gemm(at::Tensor A, at::Tensor B, bool want_stats,
                                 long n_tile) {
  TORCH_CHECK(A.is_cuda() && B.is_cuda() && A.dim() == 2 && B.dim() == 2,
              "pw8_gemm needs 2-d GPU tensors A [M,K] and B [N,K]");
  TORCH_CHECK(A.scalar_type() == at::kBFloat16 &&
                  B.scalar_type() == at::kBFloat16,
              "pw8_gemm needs bf16 A and B, got ", A.scalar_type(), " and ",
              B.scalar_type());
  const long M = A.size(0), K = A.size(1), N = B.size(0);
  TORCH_CHECK(B.size(1) == K, "pw8_gemm: A has K = ", K, " columns, B has ",
              B.size(1));
  TORCH_CHECK(K >= 8 && N >= 8 && K % 8 == 0 && N % 8 == 0,
              "pw8_gemm needs K and N that are multiples of 8 and >= 8, got "
              "K = ", K, ", N = ", N);
  TORCH_CHECK(K <= (1 << 20) && N <= (1 << 20),
              "pw8_gemm: K = ", K, " or N = ", N, " is too large");
  auto fopt = A.options().dtype(at::kFloat);
  if (M == 0)
    return {at::empty({0, N}, A.options()),
            want_stats ? at::empty({0, 2 * N}, fopt) : at::empty({0}, fopt)};
  auto Ac = A.contiguous();
  auto Bc = B.contiguous();
  TORCH_CHECK((uintptr_t)Ac.const_data_ptr() % 16 == 0 &&
                  (uintptr_t)Bc.const_data_ptr() % 16 == 0,
              "pw8_gemm needs 16-byte aligned A and B");
  const int nt = (n_tile == 64 || n_tile == 128) ? (int)n_tile
                                                 : (N <= 64 ? 64 : 128);
  const long nbm = (M + P8_BM - 1) / P8_BM, nbn = (N + nt - 1) / nt;
  TORCH_CHECK(nbm * nbn <= INT_MAX, "pw8_gemm: M = ", M, " needs ",
              nbm * nbn, " blocks");
  auto C = at::empty({M, N}, Ac.options());
  auto stats = want_stats ? at::empty({nbm, 2 * N}, fopt)
                          : at::empty({0}, fopt);
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* Ap = (const bf16*)Ac.const_data_ptr();
  const bf16* Bp = (const bf16*)Bc.const_data_ptr();
  bf16* Cp = (bf16*)C.data_ptr();
  float* Sp = want_stats ? stats.data_ptr<float>() : nullptr;
  if (nt == 64)
    pw8_launch<64>(want_stats, (int)nbm, (int)nbn, stream, Ap, Bp, Cp, M,
                   (int)K, (int)N, Sp);
  else
    pw8_launch<128>(want_stats, (int)nbm, (int)nbn, stream, Ap, Bp, Cp, M,
                    (int)K, (int)N, Sp);
  CHECK_CUDA_OK();
  return {C, stats};
}
