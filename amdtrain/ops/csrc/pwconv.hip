// Thin pointwise (1x1 conv) GEMM for gfx950: C[M,N] = A[M,K] x B[N,K]^T with
// min(K, N) small — the mobilenet_v2 1x1 layers whose channel counts are
// not multiples of 32 (32->16, 16->96, 96->24, 24->144, 144->24, 144->32)
// and their input gradients, which are the same product with K and N
// swapped.
//
// These are skinny, purely memory-bound GEMMs: every A row is read once,
// the weight is a few KiB and constant, the cost is the A read plus the C
// write.  The 128x128 tile of gemm.hip would spend 4-8x of its MFMA, LDS
// and epilogue on columns that do not exist, so this kernel is shaped the
// other way round:
//
//  * 256 threads; a wave owns 16*MI rows by ALL of N, a block 64*MI rows.
//    Blocks grid-stride over row tiles with a grid of min(tiles, PW_GRID),
//    so the weight is staged once per block (zero-padded to
//    [ceil32(N)][ceil32(K)] in LDS) and the BN-statistics partials are one
//    row per block, not one per 128 rows.
//  * A fragments go straight from global memory into the
//    v_mfma_f32_16x16x32_bf16 A layout: lane (fr, fq) holds the 16 B of row
//    r0 + fr, k-pack ks*4 + fq.  There is no re-use across n-tiles to stage
//    for.  A pack >= K/8 or a row >= M is a zero fragment made in
//    registers: the K tail needs no zero page, and tail rows contribute
//    exact zeros to C (never stored) and to the statistics.
//  * The next tile's fragments are loaded before the current tile's MFMAs.
//  * C is stored in 16-byte runs through the WIDE column map and
//    epi_quad_transpose of common.h (N % 8 == 0: a run never straddles N).
//    The statistics then cost 2 registers per 16 columns; the
//    operand-swapped product (W x X^T, 4 adjacent channels per lane) would
//    carry 8 per 16 columns across the tile loop.
//  * Statistics: per-column (sum, sumsq) of the fp32 accumulators, carried
//    in registers over the block's tiles, folded once at the end in a
//    fixed order (fq lanes, then waves 0..3) into row blockIdx of
//    [nblk][2N].  No atomics; the grid depends on M and constants only, so
//    the result is bitwise repeatable.
//
// All row and byte offsets are 64-bit.
#include "common.h"

namespace {

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) short;  // MFMA A/B frag

constexpr int PW_GRID = 1024;  // 256 CUs x 4 resident blocks

// m-fragments per wave: as many as keep acc (8*NG*MI) plus the current and
// prefetched A fragments (8*KS*MI) near 64 VGPRs
constexpr int pw_mi(int KS, int NG) {
  return KS + NG <= 2 ? 4 : (KS + NG <= 4 ? 2 : 1);
}

// KS = ceil32(K)/32 k-steps, NG = ceil32(N)/32 column groups
template <int KS, int NG, bool STATS>
__global__ void __launch_bounds__(AMD_TPB)
pw_gemm_kernel(const bf16* __restrict__ A, const bf16* __restrict__ B,
               bf16* __restrict__ C, long M, int K, int N, long tiles,
               float* __restrict__ stats) {
  constexpr int MI = pw_mi(KS, NG);
  constexpr int KP = KS * 32, NP = NG * 32, NF = 2 * NG;
  constexpr int LDW = KP + 8;  // +16 B per row: conflict-free 16 B reads
  __shared__ __attribute__((aligned(16))) bf16 Ws[NP * LDW];
  __shared__ float red[STATS ? 4 * 2 * NP : 1];

  const int t = threadIdx.x;
  const int wave = t / AMD_WAVE, lane = t % AMD_WAVE;
  const int fr = lane & 15, fq = lane >> 4;
  const int kpacks = K / 8;

  // the whole weight, zero-padded, once per block
  for (int u = t; u < NP * (KP / 8); u += AMD_TPB) {
    const int n = u / (KP / 8), p = u % (KP / 8);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (n < N && p < kpacks) v = *(const uint4*)(B + (long)n * K + p * 8);
    *(uint4*)&Ws[n * LDW + p * 8] = v;
  }
  __syncthreads();

  auto load = [&](long tile, bf16x8 (&f)[MI][KS]) {
    const long rbase = tile * (64 * MI) + wave * (16 * MI) + fr;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const long row = rbase + i * 16;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int p = ks * 4 + fq;
        bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < M && p < kpacks)
          v = *(const bf16x8*)(A + row * K + p * 8);
        f[i][ks] = v;
      }
    }
  };

  float s1[NF], s2[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) s1[j] = s2[j] = 0.f;

  bf16x8 cur[MI][KS], nxt[MI][KS];
  load(blockIdx.x, cur);
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // a tile past the end is all rows >= M: zero fragments, no read
    load(tile + gridDim.x, nxt);

    epi_f32x4 acc[MI][NF];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const bf16x8 b = *(const bf16x8*)
            &Ws[epi_col<true>(j, fr) * LDW + ks * 32 + fq * 8];
#pragma unroll
        for (int i = 0; i < MI; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              cur[i][ks], b, acc[i][j], 0, 0, 0);
      }

    if constexpr (STATS) {
      // rows >= M are exact zeros (zero A fragments): no mask needed
#pragma unroll
      for (int j = 0; j < NF; ++j)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = acc[i][j][r];
            s1[j] += v;
            s2[j] += v * v;
          }
    }

    // after the quad transpose lane (fr, fq) holds row fq*4 + (fr&3),
    // columns h*32 + (fr>>2)*8 .. +7
    const long r0 = tile * (64 * MI) + wave * (16 * MI) + fq * 4 + (fr & 3);
    const int c0 = (fr >> 2) * 8;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      uint4 run[NG];
      epi_quad_transpose<NF>(acc[i], run, fr);
      const long row = r0 + i * 16;
      if (row < M) {
        bf16* const crow = C + row * N + c0;
#pragma unroll
        for (int h = 0; h < NG; ++h)
          if (c0 + h * 32 + 8 <= N) *(uint4*)(crow + h * 32) = run[h];
      }
    }

#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) cur[i][ks] = nxt[i][ks];
  }

  if constexpr (STATS) {
    // the 4 fq lanes of a column (16 apart), then the 4 waves in order
#pragma unroll
    for (int j = 0; j < NF; ++j) {
#pragma unroll
      for (int off = 32; off >= 16; off >>= 1) {
        s1[j] += __shfl_down(s1[j], off, AMD_WAVE);
        s2[j] += __shfl_down(s2[j], off, AMD_WAVE);
      }
    }
    if (fq == 0) {
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int col = epi_col<true>(j, fr);
        red[wave * 2 * NP + col] = s1[j];
        red[wave * 2 * NP + NP + col] = s2[j];
      }
    }
    __syncthreads();
    float* const srow = stats + (long)blockIdx.x * 2 * N;
    for (int col = t; col < N; col += AMD_TPB) {
      srow[col] = ((red[col] + red[2 * NP + col]) + red[4 * NP + col]) +
                  red[6 * NP + col];
      srow[N + col] = ((red[NP + col] + red[3 * NP + col]) +
                       red[5 * NP + col]) + red[7 * NP + col];
    }
  }
}

template <int KS, int NG>
void pw_launch(bool want_stats, int grid, hipStream_t stream, const bf16* A,
               const bf16* B, bf16* C, long M, int K, int N, long tiles,
               float* stats) {
  if (want_stats)
    hipLaunchKernelGGL((pw_gemm_kernel<KS, NG, true>), dim3(grid),
                       dim3(AMD_TPB), 0, stream, A, B, C, M, K, N, tiles,
                       stats);
  else
    hipLaunchKernelGGL((pw_gemm_kernel<KS, NG, false>), dim3(grid),
                       dim3(AMD_TPB), 0, stream, A, B, C, M, K, N, tiles,
                       stats);
}

}  // namespace

// C = A x B^T (bf16, fp32 accumulation) for thin K / N; with want_stats also
// the per-block column (sum, sumsq) partials [nblk][2N] that
// batch_norm_fwd_train_from_parts takes.  The grid is min(row tiles,
// PW_GRID); max_blocks >= 1 replaces PW_GRID.
std::vector<at::Tensor> pw_gemm(at::Tensor A, at::Tensor B, bool want_stats,
                                long max_blocks) {
  TORCH_CHECK(A.is_cuda() && B.is_cuda() && A.dim() == 2 && B.dim() == 2,
              "pw_gemm needs 2-d GPU tensors A [M,K] and B [N,K]");
  TORCH_CHECK(A.scalar_type() == at::kBFloat16 &&
                  B.scalar_type() == at::kBFloat16,
              "pw_gemm needs bf16 A and B, got ", A.scalar_type(), " and ",
              B.scalar_type());
  const long M = A.size(0), K = A.size(1), N = B.size(0);
  TORCH_CHECK(B.size(1) == K, "pw_gemm: A has K = ", K, " columns, B has ",
              B.size(1));
  TORCH_CHECK(K >= 8 && N >= 8 && K % 8 == 0 && N % 8 == 0,
              "pw_gemm needs K and N that are multiples of 8 and >= 8, got "
              "K = ", K, ", N = ", N);
  const long KS = (K + 31) / 32, NG = (N + 31) / 32;
  TORCH_CHECK(KS * NG <= 8,
              "pw_gemm needs ceil32(K) * ceil32(N) <= 8192 (the zero-padded "
              "weight in 16 KiB of LDS), got K = ", K, ", N = ", N);
  TORCH_CHECK(max_blocks != 0, "pw_gemm: max_blocks must be >= 1 or negative");
  auto fopt = A.options().dtype(at::kFloat);
  if (M == 0)
    return {at::empty({0, N}, A.options()),
            want_stats ? at::empty({0, 2 * N}, fopt) : at::empty({0}, fopt)};
  auto Ac = A.contiguous();
  auto Bc = B.contiguous();
  TORCH_CHECK((uintptr_t)Ac.const_data_ptr() % 16 == 0 &&
                  (uintptr_t)Bc.const_data_ptr() % 16 == 0,
              "pw_gemm needs 16-byte aligned A and B");
  const int mi = pw_mi((int)KS, (int)NG);
  const long tiles = (M + 64 * mi - 1) / (64 * mi);
  // max_blocks stands in for PW_GRID (tests: few blocks, many tiles each;
  // tools/bench_pwconv.py: the sweep behind PW_GRID)
  const long grid = std::min<long>(tiles, max_blocks > 0 ? max_blocks
                                                         : PW_GRID);
  auto C = at::empty({M, N}, Ac.options());
  auto stats = want_stats ? at::empty({grid, 2 * N}, fopt)
                          : at::empty({0}, fopt);
  auto stream = at::cuda::getCurrentCUDAStream();
  const bf16* Ap = (const bf16*)Ac.const_data_ptr();
  const bf16* Bp = (const bf16*)Bc.const_data_ptr();
  bf16* Cp = (bf16*)C.data_ptr();
  float* Sp = want_stats ? stats.data_ptr<float>() : nullptr;
#define PW_CASE(ks, ng)                                                     \
  case ks * 16 + ng:                                                        \
    pw_launch<ks, ng>(want_stats, (int)grid, stream, Ap, Bp, Cp, M, (int)K, \
                      (int)N, tiles, Sp);                                   \
    break;
  switch (KS * 16 + NG) {
    PW_CASE(1, 1) PW_CASE(1, 2) PW_CASE(1, 3) PW_CASE(1, 4)
    PW_CASE(1, 5) PW_CASE(1, 6) PW_CASE(1, 7) PW_CASE(1, 8)
    PW_CASE(2, 1) PW_CASE(2, 2) PW_CASE(2, 3) PW_CASE(2, 4)
    PW_CASE(3, 1) PW_CASE(3, 2)
    PW_CASE(4, 1) PW_CASE(4, 2)
    PW_CASE(5, 1) PW_CASE(6, 1) PW_CASE(7, 1) PW_CASE(8, 1)
    default:
      TORCH_CHECK(false, "pw_gemm: no kernel for K = ", K, ", N = ", N);
  }
#undef PW_CASE
  CHECK_CUDA_OK();
  return {C, stats};
}
