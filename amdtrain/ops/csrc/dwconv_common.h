// What the depthwise stencil families (dwconv.hip 3x3, dwconv5x5.hip 5x5)
// share: the 16-byte pack helpers, the fixed-order collapse of the weight
// gradient partials and the host-side geometry contract.  Everything has
// internal linkage; each .hip file gets its own copy.
#pragma once

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

// Weight gradient, level 2: out[e] = sum_p part[p][e], e over taps*C.  A
// block takes DW_L2E elements; each of its DW_L2G thread groups sums the
// partials p = g, g + DW_L2G, ... in order (four loads in flight, added in p
// order; a slot past P adds 0.f, which changes nothing), then the groups are
// added in group order.
__global__ __launch_bounds__(AMD_TPB) void dw_wgrad_collapse_kernel(
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

// Shared host-side contract of the entry points of a K x K, pad K/2 family;
// `op` names it in the messages.
DwGeom dw_check(const char* op, long K, const at::Tensor& a2d,
                const char* what, long Nn, long H, long W, long stride,
                long rows_h, long rows_w) {
  TORCH_CHECK(a2d.is_cuda() && a2d.scalar_type() == at::kBFloat16 &&
                  a2d.dim() == 2 && a2d.is_contiguous(),
              what, " must be a contiguous 2-D bf16 GPU tensor");
  TORCH_CHECK(stride == 1 || stride == 2, op, ": stride must be 1 or 2");
  TORCH_CHECK(Nn >= 0 && H >= 1 && W >= 1, op, ": bad geometry");
  TORCH_CHECK(H < (1 << 24) && W < (1 << 24), op, ": image too large");
  const long C = a2d.size(1);
  TORCH_CHECK(C >= 8 && C % 8 == 0, op,
              ": C must be a positive multiple of 8, got ", C);
  TORCH_CHECK(C < (1 << 24), op, ": C too large");
  const long pad = K / 2;
  const long Ho = (H + 2 * pad - K) / stride + 1;
  const long Wo = (W + 2 * pad - K) / stride + 1;
  const long eh = rows_h ? Ho : H, ew = rows_w ? Wo : W;
  TORCH_CHECK(a2d.size(0) == Nn * eh * ew, what, " has ", a2d.size(0),
              " rows, geometry needs ", Nn * eh * ew);
  return {C, C / 8, Ho, Wo};
}

// tap-major weight [K*K, C] bf16 on the GPU of `like`
void dw_check_w(const char* name, long taps, const at::Tensor& w,
                const at::Tensor& like, long C) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 &&
                  w.dim() == 2 && w.is_contiguous() && w.size(0) == taps &&
                  w.size(1) == C && w.device() == like.device(),
              name, " must be a contiguous [", taps,
              ", C] bf16 tensor on the same GPU");
}

void dw_collapse(const at::Tensor& part, at::Tensor& out, long P, long E,
                 hipStream_t stream) {
  dw_wgrad_collapse_kernel<<<(unsigned)((E + DW_L2E - 1) / DW_L2E), AMD_TPB,
                             0, stream>>>(
      part.data_ptr<float>(), out.data_ptr<float>(), (int)P, (int)E);
  CHECK_CUDA_OK();
}

}  // namespace
