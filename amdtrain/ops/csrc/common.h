// Shared helpers for the amdtrain gfx950 (CDNA4) HIP kernels.
//
// Conventions (per the CDNA4 programming model):
//  * wavefront = 64 lanes (hard-coded; NOT 32)
//  * block size = 256 (4 waves) unless stated otherwise
//  * memory-bound kernels vectorize loads/stores to 16 B per lane
//    (Pack<T,N>), grid-stride, grid capped ~2048 blocks
//  * NHWC ("channels_last") layout: a logical [N,C,H,W] tensor is stored as
//    rows of C contiguous channels, R = N*H*W rows
#pragma once

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#define AMD_WAVE 64
#define AMD_TPB 256
#define AMD_MAX_BLOCKS 2048

#define CHECK_CUDA_OK()                                                     \
  do {                                                                      \
    hipError_t e = hipGetLastError();                                       \
    TORCH_CHECK(e == hipSuccess, "HIP kernel launch failed: ",              \
                hipGetErrorString(e));                                      \
  } while (0)

static inline int amd_grid(long total, int tpb = AMD_TPB,
                           int cap = AMD_MAX_BLOCKS) {
  long g = (total + tpb - 1) / tpb;
  return (int)std::min<long>(g, cap);
}

// ---- device dtype mapping: at:: scalar types -> HIP device types ----------

template <typename scalar_t> struct DevT { using type = scalar_t; };
template <> struct DevT<at::BFloat16> { using type = __hip_bfloat16; };
template <> struct DevT<at::Half> { using type = __half; };

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<__hip_bfloat16>(__hip_bfloat16 v) {
  return __bfloat162float(v);
}
template <> __device__ __forceinline__ float to_f32<__half>(__half v) {
  return __half2float(v);
}
template <> __device__ __forceinline__ float to_f32<double>(double v) {
  return (float)v;  // double path exists only to satisfy AT_DISPATCH
}

template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ __hip_bfloat16 from_f32<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}
template <> __device__ __forceinline__ __half from_f32<__half>(float v) {
  return __float2half(v);
}
template <> __device__ __forceinline__ double from_f32<double>(float v) {
  return (double)v;
}

// 16-byte packed vector for coalesced loads (8x bf16/fp16 or 4x fp32)
template <typename T, int N> struct alignas(sizeof(T) * N) Pack {
  T v[N];
};
template <typename T> struct VecWidth {
  static constexpr int value = 16 / sizeof(T);
};

// ---- wave / block reductions ----------------------------------------------

__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = AMD_WAVE / 2; off > 0; off >>= 1)
    v += __shfl_down(v, off, AMD_WAVE);
  return v;  // valid in lane 0
}

__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int off = AMD_WAVE / 2; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_down(v, off, AMD_WAVE));
  return v;
}

// ---- bf16 C-tile store epilogue of the MFMA kernels -------------------------
// (shared by gemm.hip, conv3x3.hip and conv_stem.hip)
//
// A wave owns a [64 rows][NF*16 cols] sub-tile as 4 x NF fragments of
// mfma_f32_16x16x32_bf16: lane (fq = lane>>4, fr = lane&15) holds rows
// fq*4 + r (r = 0..3) of ONE column per fragment.  Which column fragment j
// of lane fr holds is free — it is the LDS B row that lane read — and two
// maps are in use (epi_col):
//   narrow: col = j*16 + fr.  One 2-byte store per element.
//   WIDE:   col = (j>>1)*32 + (fr>>2)*8 + (j&1)*4 + (fr&3).  The 4 lanes of
//           a quad hold 4 adjacent columns, so a 4x4 transpose inside the
//           quad (two DPP quad_perm butterfly stages on packed bf16 pairs)
//           leaves lane fr with row fq*4 + (fr&3), columns
//           (fr>>2)*8 .. +7 of every 32-column group: one 16 B store per
//           m-fragment and group, 64 contiguous bytes per row and wave
//           instruction.  Every element is still produced by the same MFMA
//           sequence in the same k order; only its column label moves.
//
// epi (runtime, AMDTRAIN_EPILOGUE): 0 = per-element predicate and 64-bit
// row*ld+col address for every store; >= 1 = a wave whose sub-tile lies
// fully inside [M, N] stores unpredicated through a block-uniform base and
// 32-bit tile-local offsets (128 rows x ld x 2 B fits easily).  WIDE is a
// compile-time variant of the kernel (it changes the K-loop's B rows),
// needs ld % 8 == 0, and always uses the lean addressing; edge waves
// predicate whole 16 B runs (a run never straddles N when N % 8 == 0).
//
// Host side every entry point takes the mode as a trailing `epi` argument;
// a negative value selects the kernel's measured default (epi_mode).
static inline int epi_mode(long epi, int kernel_default) {
  return epi < 0 ? kernel_default : (int)epi;
}
typedef float epi_f32x4 __attribute__((ext_vector_type(4)));
typedef float epi_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 epi_bf16x2 __attribute__((ext_vector_type(2)));

template <bool WIDE>
__device__ __forceinline__ constexpr int epi_col(int j, int fr) {
  return WIDE ? (j >> 1) * 32 + (fr >> 2) * 8 + (j & 1) * 4 + (fr & 3)
              : j * 16 + fr;
}

// two fp32 -> one dword of two bf16 (lo in the low half): the same
// round-to-nearest-even conversion as __float2bfloat16, on a real pair
__device__ __forceinline__ unsigned epi_pack_bf16(float lo, float hi) {
  epi_f32x2 f = {lo, hi};
  epi_bf16x2 b = __builtin_convertvector(f, epi_bf16x2);
  unsigned u;
  __builtin_memcpy(&u, &b, 4);
  return u;
}

// One m-fragment of a WIDE wave tile: a[j][r] = (row fq*4 + r, column
// epi_col<true>(j, fr)) -> run[h] = the 8 bf16 of row fq*4 + (fr&3),
// columns h*32 + (fr>>2)*8 .. +7.
template <int NF>
__device__ __forceinline__ void epi_quad_transpose(const epi_f32x4* a,
                                                   uint4* run, int fr) {
  const bool odd = fr & 1, low = !(fr & 2);
  // v_perm_b32 pool: bytes 0-3 = own dword, 4-7 = the xor-1 neighbour's
  const unsigned sel = odd ? 0x03020706u : 0x05040100u;
  unsigned d[NF][2];
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    // rows (0,1) and (2,3) of this lane's column, packed
    const unsigned p01 = epi_pack_bf16(a[j][0], a[j][1]);
    const unsigned p23 = epi_pack_bf16(a[j][2], a[j][3]);
    // stage 1, quad_perm [1,0,3,2]: even lanes collect the even row of
    // both columns of the pair, odd lanes the odd row
    const unsigned x01 = __builtin_amdgcn_update_dpp(0, (int)p01, 0xB1, 0xF,
                                                     0xF, true);
    const unsigned x23 = __builtin_amdgcn_update_dpp(0, (int)p23, 0xB1, 0xF,
                                                     0xF, true);
    const unsigned q01 = __builtin_amdgcn_perm(x01, p01, sel);
    const unsigned q23 = __builtin_amdgcn_perm(x23, p23, sel);
    // stage 2, quad_perm [2,3,0,1]: lanes 0,1 keep rows 0,1 and receive
    // columns 2,3; lanes 2,3 keep rows 2,3 and receive columns 0,1
    const unsigned send = low ? q23 : q01;
    const unsigned recv = __builtin_amdgcn_update_dpp(0, (int)send, 0x4E,
                                                      0xF, 0xF, true);
    d[j][0] = low ? q01 : recv;
    d[j][1] = low ? recv : q23;
  }
#pragma unroll
  for (int h = 0; h < NF / 2; ++h)
    run[h] = make_uint4(d[2 * h][0], d[2 * h][1], d[2 * h + 1][0],
                        d[2 * h + 1][1]);
}

// Store the wave's [64][NF*16] bf16 sub-tile at rows m0 + wm.., columns
// n0 + wn.. of C[M][N] (row pitch ld == N).  acc[i * ACCLD + j] is
// fragment (i, j); m0 / n0 are block-uniform, wm / wn the wave's offsets.
template <int NF, int ACCLD, bool WIDE>
__device__ __forceinline__ void epi_store_bf16(
    __hip_bfloat16* __restrict__ C, long ld, long m0, long M, long n0,
    long N, int wm, int wn, int fr, int fq, const epi_f32x4* acc, int epi) {
  const bool inside = __builtin_amdgcn_readfirstlane(
      (int)(m0 + wm + 64 <= M && n0 + wn + NF * 16 <= N));
  char* const blk = (char*)(C + m0 * ld + n0);
  const unsigned ld2 = (unsigned)ld * 2;  // row pitch in bytes
  if constexpr (WIDE) {
    const unsigned lrow = wm + fq * 4 + (fr & 3), lcol = wn + (fr >> 2) * 8;
    const unsigned off = lrow * ld2 + lcol * 2;
    auto rows = [&](auto pred) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint4 run[NF / 2];
        epi_quad_transpose<NF>(acc + i * ACCLD, run, fr);
        if (!pred.value || m0 + lrow + i * 16 < M) {
#pragma unroll
          for (int h = 0; h < NF / 2; ++h)
            if (!pred.value || n0 + lcol + h * 32 + 8 <= N)
              *(uint4*)(blk + (off + i * 16 * ld2 + h * 64)) = run[h];
        }
      }
    };
    if (inside)
      rows(std::false_type{});
    else
      rows(std::true_type{});
    return;
  }
  if (inside && epi >= 1) {
    const unsigned off = (wm + fq * 4) * ld2 + (wn + fr) * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned roff = off + (i * 16 + r) * ld2;
#pragma unroll
        for (int j = 0; j < NF; ++j)
          *(__hip_bfloat16*)(blk + (roff + j * 32)) =
              __float2bfloat16(acc[i * ACCLD + j][r]);
      }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        long row = m0 + wm + i * 16 + fq * 4 + r;
        long col = n0 + wn + j * 16 + fr;
        if (row < M && col < N)
          C[row * ld + col] = __float2bfloat16(acc[i * ACCLD + j][r]);
      }
}

// ---- implicit-GEMM conv epilogue: BN-statistics partials --------------------
// (shared by conv3x3.hip and conv_stem.hip)
// per-block column (sum, sumsq) of the fp32 accumulator tile (see
// gemm.hip) of a 128-row block whose 4 waves form a 2m x 2n grid of
// 4 x (NTE/32) 16x16 fragments; NTE = n-tile width (128 or 64).  Writes row
// bm of stats [nbm][2*N]; lds_scratch needs 4*NTE floats.
// WIDE: the kernel's column map (epi_col) — only the column label moves.
template <int NTE = 128, bool WIDE = false>
__device__ __forceinline__ void conv_epilogue_stats(
    float* __restrict__ stats, const float* acc_flat, long m0, long M,
    long n0, long N, int bm, int wm, int wn, int fr, int fq,
    void* lds_scratch) {
  constexpr int NF = NTE / 32;  // n fragments per wave
  float* srow = stats + (long)bm * 2 * N;
  float s1[NF], s2[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    s1[j] = 0.f;
    s2[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        long row = m0 + wm + i * 16 + fq * 4 + r;
        float v = (row < M) ? acc_flat[(i * NF + j) * 4 + r] : 0.f;
        s1[j] += v;
        s2[j] += v * v;
      }
  }
#pragma unroll
  for (int j = 0; j < NF; ++j) {
#pragma unroll
    for (int off = 32; off >= 16; off >>= 1) {
      s1[j] += __shfl_down(s1[j], off, AMD_WAVE);
      s2[j] += __shfl_down(s2[j], off, AMD_WAVE);
    }
  }
  float* red = (float*)lds_scratch;
  __syncthreads();
  if (fq == 0) {
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      int col = wn + epi_col<WIDE>(j, fr);
      red[(wm ? 1 : 0) * (2 * NTE) + col * 2 + 0] = s1[j];
      red[(wm ? 1 : 0) * (2 * NTE) + col * 2 + 1] = s2[j];
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  for (int col = t; col < NTE; col += AMD_TPB) {
    long n = n0 + col;
    if (n < N) {
      srow[n] = red[col * 2] + red[2 * NTE + col * 2];
      srow[N + n] = red[col * 2 + 1] + red[2 * NTE + col * 2 + 1];
    }
  }
}

// ---- multi-tensor-apply metadata (apex amp_C style, struct by value) -------

constexpr int MT_TENSORS = 24;
constexpr int MT_BLOCKS = 320;
constexpr long MT_CHUNK = 1 << 16;  // elements per block-chunk

struct MTMeta {
  const void* a[MT_TENSORS];
  void* b[MT_TENSORS];
  void* c[MT_TENSORS];
  long sizes[MT_TENSORS];
  short t_for_block[MT_BLOCKS];
  short chunk_for_block[MT_BLOCKS];
};

// Layout contract of the multi-tensor ops.  The kernels walk every tensor of
// a slot (param / grad / momentum, or src / dst) as ONE flat run of numel()
// elements from data_ptr(), so element i of each must be the same logical
// element.  That holds iff the tensors have equal sizes, each is
// non-overlapping and dense, and their strides agree on every dim of size
// != 1 (a size-1 dim's stride addresses nothing: a channels_last [O,I,1,1]
// weight and its row-major gradient share one memory order; this is the
// rule of torch's gradient layout contract).  Anything else would be
// updated silently permuted or out of bounds, so it is refused here, on the
// host, before any launch.
static inline void mt_check_tensor(const char* op, const char* list, size_t i,
                                   const at::Tensor& t,
                                   const at::Device& device) {
  TORCH_CHECK(t.is_cuda() && t.device() == device, op, ": ", list, "[", i,
              "] is on ", t.device(), ", expected ", device);
  TORCH_CHECK(t.numel() == 0 || t.is_non_overlapping_and_dense(), op, ": ",
              list, "[", i, "] is not dense (sizes ", t.sizes(), ", strides ",
              t.strides(), ")");
  // chunk_for_block is a short
  TORCH_CHECK(t.numel() <= 32767 * MT_CHUNK, op, ": ", list, "[", i,
              "] has too many elements (", t.numel(), ")");
}

// `t` must share the memory order of `ref` (both already mt_check_tensor'ed)
static inline void mt_check_same_layout(const char* op, size_t i,
                                        const char* ref_list,
                                        const at::Tensor& ref,
                                        const char* list,
                                        const at::Tensor& t) {
  TORCH_CHECK(t.sizes() == ref.sizes(), op, ": ", list, "[", i, "] has sizes ",
              t.sizes(), " but ", ref_list, "[", i, "] has ", ref.sizes());
  if (t.numel() == 0) return;
  for (int64_t d = 0; d < t.dim(); ++d)
    TORCH_CHECK(t.size(d) == 1 || t.stride(d) == ref.stride(d), op, ": ", list,
                "[", i, "] has strides ", t.strides(), " but ", ref_list, "[",
                i, "] has ", ref.strides(), " (sizes ", t.sizes(),
                "): the tensors of one slot must share a memory order");
}

// Host-side chunking driver: fills MTMeta over (up to) three parallel tensor
// lists and invokes `launch(meta, nblocks, ntensors)` for each full batch.
// Callers validate the lists first (mt_check_tensor / mt_check_same_layout).
template <typename LaunchFn>
static void mt_apply(const std::vector<at::Tensor>& A,
                     const std::vector<at::Tensor>* B,
                     const std::vector<at::Tensor>* C, LaunchFn launch) {
  MTMeta meta;
  int t = 0, blk = 0;
  for (size_t i = 0; i < A.size(); ++i) {
    long n = A[i].numel();
    meta.a[t] = A[i].const_data_ptr();
    meta.b[t] = B ? (*B)[i].data_ptr() : nullptr;
    meta.c[t] = C ? (*C)[i].data_ptr() : nullptr;
    meta.sizes[t] = n;
    long nchunks = (n + MT_CHUNK - 1) / MT_CHUNK;
    for (long ch = 0; ch < nchunks; ++ch) {
      meta.t_for_block[blk] = (short)t;
      meta.chunk_for_block[blk] = (short)ch;
      ++blk;
      if (blk == MT_BLOCKS) {
        launch(meta, blk, t + 1);
        // re-seed current tensor into slot 0 for remaining chunks
        meta.a[0] = meta.a[t];
        meta.b[0] = meta.b[t];
        meta.c[0] = meta.c[t];
        meta.sizes[0] = meta.sizes[t];
        t = 0;
        blk = 0;
      }
    }
    ++t;
    if (t == MT_TENSORS && i + 1 < A.size()) {
      if (blk) launch(meta, blk, t);
      t = 0;
      blk = 0;
    }
  }
  if (blk) launch(meta, blk, t);
}
