// Fused multi-tensor LARS (layer-wise adaptive rate scaling, You et al. 2017)
// for gfx950: momentum SGD whose update of every tensor is scaled by a trust
// ratio built from that tensor's own parameter and gradient norms.
//
//   r  = eta * |p| / (|g| + wd * |p| + eps)   if adapt and |p| > 0 and |g| > 0
//   r  = 1                                    otherwise
//   u  = r * (g + wd_t * p)                   wd_t = 0 for tensors without decay
//   b  = u (first step)  |  mu * b + u
//   p -= lr * (nesterov ? u + mu * b : b);    g = 0 when zero_grad
//
// Two phases over the chunk lists of mt_apply (common.h), launched back to
// back on one stream; no atomics, no host synchronisation, no copies:
//
//  1. lars_norm_kernel: one block per 64Ki-element chunk sums p^2 and g^2 of
//     its chunk in fp32 and writes the pair to partials[row], row =
//     (prefix sum of the chunk counts of the tensors before it in the list)
//     + chunk.  The row depends on the list position and the chunk alone,
//     never on how mt_apply cut the list into launches.  Blocks of tensors
//     without adaptation exit at once: their r is 1 by definition.
//  2. lars_apply_kernel: one block per chunk again.  Every block first
//     collapses ALL partial rows of its tensor (the biggest registry tensor
//     has under 40), so every block of a tensor holds the same r without a
//     third kernel or a grid-wide barrier, then applies the update with
//     the aligned 16 B / unaligned scalar / tail structure of
//     mt_sgd_kernel.  The block of chunk 0 stores r for logging.
//
// Summation order (fixed, hence bitwise reproducible): a thread owns
// elements base + 4*tid + 1024*k of the chunk and keeps one accumulator per
// component of its 16 B packs, folded as (0 + 1) + (2 + 3); the unaligned path keeps
// one accumulator over base + tid + 256*k.  64 lanes fold by the
// shfl_down halving tree of wave_reduce_sum, the 4 waves as
// (w0 + w1) + (w2 + w3) through LDS.  The collapse gives thread i the rows
// i, i + 256, ... in ascending order and folds the 256 threads by the same
// tree, so its order is a function of the chunk count alone.
//
// Bit parity with mt_sgd_kernel: with r == 1 the element update below is the
// SGD kernel's, written with explicit fmaf where that kernel's expressions
// contract (g + wd*p, mu*b + u, u + mu*b, p - lr*u), and 1.0f * x is exact.
#include "common.h"

// No packed-fp32 selection (v_pk_*_f32) for the code of this file: a device
// target feature, switched off per function (the host pass does not know
// it).  A callee without the attribute is inlined only when it is
// always_inline, hence the spelled-out barrier in block_sum2.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

struct LarsArgs {
  float lr, momentum, weight_decay, eta, eps;
  bool nesterov, first, zero_grad;
};

// per-launch side data of MTMeta's slots (MTMeta itself is shared with the
// other multi-tensor ops and stays as it is)
struct LarsMeta {
  int part_row[MT_TENSORS];  // first partials row of the slot's tensor
  int index[MT_TENSORS];     // the tensor's position in the caller's lists
  unsigned adapt, decay;     // bit s: slot s adapts / decays
};

// (a, b) summed over the block in a fixed order; every thread gets the result
using F2 = Pack<float, 2>;
using F4 = Pack<float, 4>;  // one 16 B load / store per lane

__device__ __forceinline__ F2 block_sum2(float a, float b, float* red) {
  a = wave_reduce_sum(a);
  b = wave_reduce_sum(b);
  const int wave = threadIdx.x / AMD_WAVE;
  if (threadIdx.x % AMD_WAVE == 0) {
    red[2 * wave] = a;
    red[2 * wave + 1] = b;
  }
  // __syncthreads()
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return F2{{(red[0] + red[2]) + (red[4] + red[6]),
             (red[1] + red[3]) + (red[5] + red[7])}};
}

__global__ void __launch_bounds__(AMD_TPB)
lars_norm_kernel(MTMeta meta, LarsMeta lm, F2* __restrict__ partials) {
  __shared__ float red[2 * AMD_TPB / AMD_WAVE];
  const int t = meta.t_for_block[blockIdx.x];
  if (!((lm.adapt >> t) & 1)) return;  // block-uniform
  const int chunk = meta.chunk_for_block[blockIdx.x];
  const long base = (long)chunk * MT_CHUNK;
  const long end = min(base + MT_CHUNK, meta.sizes[t]);
  const float* __restrict__ p = (const float*)meta.b[t];
  const float* __restrict__ g = (const float*)meta.c[t];

  float sp, sg;
  if ((((uintptr_t)p | (uintptr_t)g) & 15) != 0) {
    sp = sg = 0.f;
    for (long i = base + threadIdx.x; i < end; i += blockDim.x) {
      const float pe = p[i], ge = g[i];
      sp = fmaf(pe, pe, sp);
      sg = fmaf(ge, ge, sg);
    }
  } else {
    F4 ap = {{0.f, 0.f, 0.f, 0.f}}, ag = ap;
    for (long i = base + threadIdx.x * 4; i + 3 < end;
         i += (long)blockDim.x * 4) {
      const F4 pv = *(const F4*)(p + i);
      const F4 gv = *(const F4*)(g + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ap.v[k] = fmaf(pv.v[k], pv.v[k], ap.v[k]);
        ag.v[k] = fmaf(gv.v[k], gv.v[k], ag.v[k]);
      }
    }
    // scalar tail (at most 3 elements, threads 0..2, component 0)
    const long tail = base + ((end - base) / 4) * 4 + threadIdx.x;
    if (tail < end) {
      ap.v[0] = fmaf(p[tail], p[tail], ap.v[0]);
      ag.v[0] = fmaf(g[tail], g[tail], ag.v[0]);
    }
    sp = (ap.v[0] + ap.v[1]) + (ap.v[2] + ap.v[3]);
    sg = (ag.v[0] + ag.v[1]) + (ag.v[2] + ag.v[3]);
  }
  const F2 s = block_sum2(sp, sg, red);
  if (threadIdx.x == 0) partials[lm.part_row[t] + chunk] = s;
}

template <bool HAS_MU>
__device__ __forceinline__ float lars_element(float pe, float ge, float& me,
                                              float r, float wd,
                                              const LarsArgs& a) {
  float u = r * fmaf(wd, pe, ge);
  if (HAS_MU) {
    me = a.first ? u : fmaf(a.momentum, me, u);
    u = a.nesterov ? fmaf(a.momentum, me, u) : me;
  }
  return fmaf(-a.lr, u, pe);
}

template <bool HAS_MU>
__global__ void __launch_bounds__(AMD_TPB)
lars_apply_kernel(MTMeta meta, LarsMeta lm, LarsArgs args,
                  const F2* __restrict__ partials,
                  float* __restrict__ ratios) {
  __shared__ float red[2 * AMD_TPB / AMD_WAVE];
  const int t = meta.t_for_block[blockIdx.x];
  const int chunk = meta.chunk_for_block[blockIdx.x];
  const long base = (long)chunk * MT_CHUNK;
  const long n = meta.sizes[t];
  const long end = min(base + MT_CHUNK, n);
  float* __restrict__ p = (float*)meta.b[t];
  float* __restrict__ g = (float*)meta.c[t];
  float* __restrict__ m = (float*)const_cast<void*>(meta.a[t]);
  const float wd = ((lm.decay >> t) & 1) ? args.weight_decay : 0.f;

  float r = 1.f;
  if ((lm.adapt >> t) & 1) {  // block-uniform
    const int nchunks = (int)((n + MT_CHUNK - 1) / MT_CHUNK);
    const F2* __restrict__ rows = partials + lm.part_row[t];
    float sp = 0.f, sg = 0.f;
    for (int c = threadIdx.x; c < nchunks; c += blockDim.x) {
      const F2 v = rows[c];
      sp += v.v[0];
      sg += v.v[1];
    }
    const F2 s = block_sum2(sp, sg, red);
    const float pn = sqrtf(s.v[0]), gn = sqrtf(s.v[1]);
    if (pn > 0.f && gn > 0.f)
      r = args.eta * pn / (gn + args.weight_decay * pn + args.eps);
  }
  if (chunk == 0 && threadIdx.x == 0) ratios[lm.index[t]] = r;

  // grads can be views into bucket flats at arbitrary offsets: vectorize
  // only when all three pointers are 16B-aligned (uniform branch per block)
  const bool vec_ok = ((((uintptr_t)p | (uintptr_t)g |
                         (uintptr_t)(HAS_MU ? m : p)) & 15) == 0);
  float me = 0.f;
  if (!vec_ok) {
    for (long i = base + threadIdx.x; i < end; i += blockDim.x) {
      if (HAS_MU) me = m[i];
      p[i] = lars_element<HAS_MU>(p[i], g[i], me, r, wd, args);
      if (HAS_MU) m[i] = me;
      if (args.zero_grad) g[i] = 0.f;
    }
    return;
  }

  // 16 B main body over the 16B-aligned interior of the chunk
  for (long i = base + threadIdx.x * 4; i + 3 < end;
       i += (long)blockDim.x * 4) {
    F4 pv = *(const F4*)(p + i);
    const F4 gv = *(const F4*)(g + i);
    F4 mv = {{0.f, 0.f, 0.f, 0.f}};
    if (HAS_MU) mv = *(const F4*)(m + i);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      pv.v[k] = lars_element<HAS_MU>(pv.v[k], gv.v[k], mv.v[k], r, wd, args);
    *(F4*)(p + i) = pv;
    if (HAS_MU) *(F4*)(m + i) = mv;
    if (args.zero_grad) *(F4*)(g + i) = F4{{0.f, 0.f, 0.f, 0.f}};
  }
  // scalar tail (chunk length not a multiple of 4)
  const long tail = base + ((end - base) / 4) * 4 + threadIdx.x;
  if (tail < end) {
    if (HAS_MU) me = m[tail];
    p[tail] = lars_element<HAS_MU>(p[tail], g[tail], me, r, wd, args);
    if (HAS_MU) m[tail] = me;
    if (args.zero_grad) g[tail] = 0.f;
  }
}

}  // namespace

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

at::Tensor multi_tensor_lars(std::vector<at::Tensor> params,
                             std::vector<at::Tensor> grads,
                             std::vector<at::Tensor> momenta,
                             std::vector<bool> adapt_mask,
                             std::vector<bool> decay_mask, double lr,
                             double momentum, double weight_decay, double eta,
                             double eps, bool nesterov, bool first,
                             bool zero_grad) {
  const char* op = "multi_tensor_lars";
  const size_t count = params.size();
  TORCH_CHECK(count == grads.size() && count == momenta.size() &&
                  count == adapt_mask.size() && count == decay_mask.size(),
              op, ": the five lists must have one entry per tensor");
  if (params.empty()) return at::empty({0}, at::kFloat);
  // every list is checked before the first launch: the kernels read element
  // i of param, grad and momentum from the same flat offset
  const at::Device device = params[0].device();
  for (size_t i = 0; i < count; ++i) {
    const at::Tensor* slot[3] = {&params[i], &grads[i], &momenta[i]};
    const char* names[3] = {"params", "grads", "momenta"};
    for (int k = 0; k < 3; ++k) {
      TORCH_CHECK(slot[k]->scalar_type() == at::kFloat, op, ": ", names[k],
                  "[", i, "] is ", slot[k]->scalar_type(),
                  ", expected fp32 CUDA tensors");
      mt_check_tensor(op, names[k], i, *slot[k], device);
      if (k) mt_check_same_layout(op, i, names[0], params[i], names[k],
                                  *slot[k]);
    }
  }

  // partials rows: host-side prefix sum of the chunk counts, in list order
  std::vector<int> part_row(count);
  long rows = 0;
  bool any_adapt = false, any_empty = false;
  for (size_t i = 0; i < count; ++i) {
    part_row[i] = (int)rows;
    rows += (params[i].numel() + MT_CHUNK - 1) / MT_CHUNK;
    any_adapt |= adapt_mask[i];
    any_empty |= params[i].numel() == 0;
  }
  TORCH_CHECK(rows <= INT_MAX, op, ": too many chunks (", rows, ")");
  const auto f32 = params[0].options().dtype(at::kFloat);
  at::Tensor partials = at::empty({rows, 2}, f32);
  // an empty tensor has no chunk 0 block to store its ratio
  at::Tensor ratios = any_empty ? at::ones({(long)count}, f32)
                                : at::empty({(long)count}, f32);
  F2* part = (F2*)partials.data_ptr<float>();

  auto side = [&](int tensors, size_t list_first) {
    LarsMeta lm;
    lm.adapt = lm.decay = 0;
    for (int s = 0; s < tensors; ++s) {
      lm.part_row[s] = part_row[list_first + s];
      lm.index[s] = (int)(list_first + s);
      lm.adapt |= (unsigned)adapt_mask[list_first + s] << s;
      lm.decay |= (unsigned)decay_mask[list_first + s] << s;
    }
    return lm;
  };
  LarsArgs args{(float)lr, (float)momentum, (float)weight_decay, (float)eta,
                (float)eps, nesterov, first, zero_grad};
  auto stream = at::cuda::getCurrentCUDAStream();
  if (any_adapt)
    mt_apply(momenta, &params, &grads,
             [&](const MTMeta& meta, int blocks, int tensors, size_t lf) {
               const LarsMeta lm = side(tensors, lf);
               if (!lm.adapt) return;
               lars_norm_kernel<<<blocks, AMD_TPB, 0, stream>>>(meta, lm,
                                                                 part);
               CHECK_CUDA_OK();
             });
  const bool has_mu = momentum != 0.0;
  float* rat = ratios.data_ptr<float>();
  mt_apply(momenta, &params, &grads,
           [&](const MTMeta& meta, int blocks, int tensors, size_t lf) {
             const LarsMeta lm = side(tensors, lf);
             if (has_mu)
               lars_apply_kernel<true><<<blocks, AMD_TPB, 0, stream>>>(
                   meta, lm, args, part, rat);
             else
               lars_apply_kernel<false><<<blocks, AMD_TPB, 0, stream>>>(
                   meta, lm, args, part, rat);
             CHECK_CUDA_OK();
           });
  return ratios;
}
