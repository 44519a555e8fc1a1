// TN ("wgrad") GEMM core v2 for gfx950 — dW[N, K] += sum_m dY[m,n] * Xg[m,k]
// covering conv1x1 wgrad (K = Cin), strided-1x1 wgrad (gathered X rows) and
// conv3x3 wgrad (K = 9*Cin, im2col column gather) in ONE kernel family
// (SURVEY §2c rows "Linear/GEMM (cuBLAS)" wgrad + "Conv2d 3x3" wgrad;
// reference hot path /root/reference/distributed.py:268 loss.backward()).
//
// Why v2 (round-1 profile: conv3x3 wgrad 19 ms/step + 1x1 wgrad 10 ms/step;
// those kernels are gone, docs/KERNELS.md keeps the record):
//  * the round-1 TN kernels transposed through REGISTERS with per-element
//    swizzled ds_write_b16 (32 x 2B writes per thread per 32-m chunk) and
//    drained two barriers per chunk for only 16 MFMA/wave;
//  * conv3x3 wgrad launched 9 separate kernels re-reading dY and X per tap;
//  * split-M accumulated through fp32 atomic adds — heavily contended on
//    the small early-layer dW tiles.
// v2 fixes all three:
//  * staging is __builtin_amdgcn_global_load_lds DIRECT into a subtiled
//    layout consumed by ds_read_b64_tr_b16 (gfx950 hardware transpose read,
//    guide T10): no register round-trip, vectorized 16 B stores, and the
//    9 taps are just columns of one [N, 9*Cin] output (dY staged ONCE per
//    m-chunk instead of 9 times);
//  * 2-phase double-buffer (guide §5.5 minimum-2-phase recipe): stage the
//    next m-chunk while MFMAs consume the current one, one vmcnt(0)+barrier
//    per chunk, 32 MFMA/wave between barriers (MC=64);
//  * split-M partial outputs go to a [msplit, N*K] fp32 buffer with plain
//    stores + a vectorized collapse kernel — no atomics, and the reduction
//    order is FIXED, so wgrad v2 is bitwise deterministic by construction.
//
// LDS layout ("tr-subtile", derived from the guide's m156 mapping): the
// [MC x NCOLS] operand tile is stored as 256-element (512 B) groups
// G = ((m>>5)*NCOLS/16 + (c>>4))*2 + ((m>>2)&1), element (m,c) at byte
//   G*512 + ((m>>3)&3)*128 + (m&3)*32 + (c&15)*2 .
// A group's four 128 B windows are exactly what one ds_read_b64_tr_b16
// returns per 16-lane quarter (lane l, elem j <- window byte
// (l&15)*2 + j*32), so two tr-reads (r = 0/1 groups, +512 B apart)
// assemble the full bf16x8 MFMA operand
//   frag[jj] = T[m = 8*(l>>4) + jj][c = l&15],   jj = 0..7.
// Bank behavior: a staging wave's 64 concurrent 16 B stores land on the 8
// 16 B positions of the 128 B bank cycle exactly 8x each (position =
// (2*(m&3) + ((c>>3)&1)) mod 8) — evenly distributed, i.e. the 8-cycle
// floor for 1 KiB of LDS writes with no aliasing penalty; each tr-read
// window is 128 B contiguous, so reads are conflict-free too.
#include "common.h"

namespace {

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;

constexpr int TN2_TPB = 256;  // 4 waves
constexpr int GROUP_BYTES = 512;

__device__ __forceinline__ int xcd_swz_tn2(int bid, int nwg) {
  constexpr int NXCD = 8;
  if (nwg < NXCD) return bid;
  int xcd = bid % NXCD, idx = bid / NXCD;
  int q = nwg / NXCD, r = nwg % NXCD;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

struct TnGeom {
  int H, W, Hout, Wout, stride;  // stride / pad: along h
  int kh, kw, pad;  // filter geometry (3,3,1 for the bottleneck 3x3 convs)
  int sw, pw;       // stride / left padding along w
};

// generic conv forward gather, split in two so the (n, ho, wo) decode of a
// staged row — two 64-bit div/mod pairs — runs once per row, not once per
// 16 B unit: output row m -> tap-0 input coordinates ...
struct TnRow {
  long n_off;  // n * H * W
  int hb, wb;  // may be negative / off-image
};

__device__ __forceinline__ TnRow tn2_decode_row(long m, const TnGeom& g) {
  TnRow r;
  long t = m;
  const int wo = (int)(t % g.Wout); t /= g.Wout;
  const int ho = (int)(t % g.Hout); t /= g.Hout;
  r.n_off = t * (long)g.H * g.W;
  r.hb = ho * g.stride - g.pad;
  r.wb = wo * g.sw - g.pw;
  return r;
}

// ... + tap -> X row or -1
__device__ __forceinline__ long tn2_gather_tap(const TnRow& r, int tap,
                                               const TnGeom& g) {
  // 3- and 4-wide filters (every 3x3 conv, the space-to-depth stem) divide
  // by a constant
  const int kh = g.kw == 3 ? tap / 3 : g.kw == 4 ? tap >> 2 : tap / g.kw;
  const int h = r.hb + kh;
  const int w = r.wb + tap - kh * g.kw;
  if (h < 0 || h >= g.H || w < 0 || w >= g.W) return -1;
  return r.n_off + (long)h * g.W + w;
}

// strided-1x1 gather: compact output row m=(n,ho,wo) -> input row
__device__ __forceinline__ long tn2_gather_stride(long m, const TnGeom& g) {
  long t = m;
  const int wo = (int)(t % g.Wout); t /= g.Wout;
  const int ho = (int)(t % g.Hout); t /= g.Hout;
  return (t * g.H + (long)ho * g.stride) * g.W + (long)wo * g.stride;
}

// byte offset of element (m, c) of a [MC x NCOLS] tile in tr-subtile layout
template <int NCOLS>
__device__ __forceinline__ int st_byte(int m, int c) {
  const int sub = (m >> 5) * (NCOLS / 16) + (c >> 4);
  const int G = sub * 2 + ((m >> 2) & 1);
  return G * GROUP_BYTES + ((m >> 3) & 3) * 128 + (m & 3) * 32 + (c & 15) * 2;
}

template <int NCOLS, int MC>
constexpr int tile_bytes() {
  return (MC / 32) * (NCOLS / 16) * 2 * GROUP_BYTES;
}

// Stage one [MC x NCOLS] operand tile into tr-subtile LDS via
// global_load_lds.  MODE 0: rows are m (plain; also the dY operand),
// MODE 1: strided-1x1 gather, MODE 2: conv3x3 tap gather (cols span taps).
// Out-of-range rows/cols pull from the 16 B zero page.
//
// global_load_lds is a WAVE-UNIFORM-BASE DMA: the hardware writes lane i's
// 16 B at base + i*16 regardless of per-lane LDS addresses (guide: "CDNA's
// is wave-uniform-base not per-lane scatter").  So each WAVE stages one
// complete 1 KiB subtile (32 m x 16 c), whose tr-layout bytes are exactly
// subtile_base + lane*16 under the lane -> (m, c) decode
//   m' = 8*((lane>>3)&3) + 4*(lane>>5) + ((lane>>1)&3),
//   c  = (lane&1)*8 .. +8
// (inverse of st_byte: lane*16 = r*512 + q*128 + j*32 + c_half*2).
template <int MODE, int NCOLS, int MC, int NWAVES = 4, bool CUT = false>
__device__ __forceinline__ void stage_tn2(
    const bf16* __restrict__ g, int ld, long m0, long M, int col0,
    int total_cols, int cin, const TnGeom& geo, const bf16* __restrict__ zp,
    bf16* lds, int ncut = 0) {
  const int t = threadIdx.x;
  const int wave = t / AMD_WAVE, lane = t % AMD_WAVE;
  constexpr int SUBTILES = (MC / 32) * (NCOLS / 16);
  const int r = lane >> 5, q = (lane >> 3) & 3, j = (lane >> 1) & 3;
  const int c_half = (lane & 1) * 8;
  const int mfrag = q * 8 + r * 4 + j;  // m offset within the 32-row block
  // a thread's rows differ only by the 32-row block: decode each once
  TnRow rows[MC / 32];
  if (MODE == 2) {
#pragma unroll
    for (int mb = 0; mb < MC / 32; ++mb) {
      const long m = m0 + mb * 32 + mfrag;
      rows[mb] = tn2_decode_row(m < M ? m : M - 1, geo);
    }
  }
#pragma unroll
  for (int ss = 0; ss < SUBTILES / NWAVES; ++ss) {
    const int s = ss * NWAVES + wave;
    // 32-row block: a compile-time constant per unrolled ss (a wave round
    // never straddles two blocks), so rows[] stays in registers
    static_assert((NCOLS / 16) % NWAVES == 0, "wave round spans m-blocks");
    const int mb = (ss * NWAVES) / (NCOLS / 16);
    const int cs = (s % (NCOLS / 16)) * 16;  // subtile column base
    // subtiles wholly past ncut are never read (tn2_kernel, nlive): no DMA
    if (CUT && col0 + cs >= ncut) continue;
    const int mloc = mb * 32 + mfrag;
    const long m = m0 + mloc;
    const int col = col0 + cs + c_half;
    const bf16* src = zp;
    if (m < M && col + 8 <= total_cols) {
      if (MODE == 0) {
        src = g + m * (long)ld + col;
      } else if (MODE == 1) {
        src = g + tn2_gather_stride(m, geo) * (long)ld + col;
      } else {
        // unit never spans taps (cin % 8 == 0); power-of-two channel
        // counts (all of ResNet's, and the stem's 8) shift instead
        const int tap = (cin & (cin - 1)) == 0 ? col >> (__ffs(cin) - 1)
                                               : col / cin;
        const long row = tn2_gather_tap(rows[mb], tap, geo);
        if (row >= 0) src = g + row * (long)ld + (col - tap * cin);
      }
    }
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(
            (char*)lds + s * 1024 + lane * 16),
        16, 0, 0);
  }
}

// ---- incremental gather addressing (AMDTRAIN_TN2_ADDR, default on) --------
// stage_tn2 above re-derives every gathered address from m for every 16 B
// unit of every chunk: two 64-bit div/mod pairs per row, tap and kh
// divisions, four bounds tests and a 64-bit multiply per unit, all under
// divergent branches — several times the issue slots of the chunk's 32
// MFMAs.  But a block's chunks are consecutive, so a thread's rows only
// ever advance by MC, and its columns never change.  TnWalk keeps
//   per row slot (MC/32):  the tap-0 input pixel (hb, wb) and its byte
//     address, stepped by MC rows per chunk with two carries (the
//     row_advance idea of batchnorm.hip), and from (hb, wb) a validity mask:
//     bit kh set where row hb+kh is inside the image, bit 16+kw likewise;
//   per column slot (loop-invariant): the tap's byte offset
//     ((kh*W + kw)*ld + channel)*2 and the two mask bits it needs.
// A unit is then one AND + compare, one 64-bit add and a select against the
// zero page.  The bytes staged are exactly stage_tn2's.

// what MC output rows are in input bytes; filled on the host (tn2_make_step)
struct TnStep {
  int step;          // (dn*H*W + dh*stride*W + dw*sw) * ld * 2, no carry
  int cw, ch;        // extra bytes when wo / ho wraps
  int dhb, dwb;      // dh*stride, dw*sw
  int hhi, whi;      // first hb / wb past the last output row / column
  int hspan, wspan;  // Hout*stride, Wout*sw
  int nlive;         // dY columns >= nlive are padding (AMDTRAIN_TN2_NSKIP)
};

// bits t of [0, k) with 0 <= b + t < size  (b >= -15, k <= 15)
__device__ __forceinline__ unsigned tn2_range_mask(int b, int size, int k) {
  const int lo = max(-b, 0);
  const int hi = max(min(size - b, k), lo);
  return (1u << hi) - (1u << lo);
}

template <int MODE, int NCOLS, int MC, int NWAVES>
struct TnWalk {
  static_assert(MODE == 1 || MODE == 2, "gather modes only");
  static_assert((NCOLS / 16) % NWAVES == 0, "wave round spans m-blocks");
  static constexpr int NRS = MC / 32;                // row slots
  static constexpr int NCS = (NCOLS / 16) / NWAVES;  // column slots
  static constexpr unsigned NEVER = 0x80000000u;     // bit no row mask has

  unsigned long long base[NRS];  // byte address of the tap-0 pixel's row
  int hb[NRS], wb[NRS];          // its coordinates, may be off-image
  long mrow;                     // output row of slot 0 (slot mb: + 32*mb)
  unsigned toff[NCS], sel[NCS];

  __device__ __forceinline__ void init(const bf16* g, int ld, long m0,
                                       int col0, int total_cols, int cin,
                                       const TnGeom& geo) {
    const int lane = threadIdx.x % AMD_WAVE, wave = threadIdx.x / AMD_WAVE;
    const int r = lane >> 5, q = (lane >> 3) & 3, j = (lane >> 1) & 3;
    mrow = m0 + q * 8 + r * 4 + j;
    const bool narrow = m0 + MC <= 0x7fffffffL;  // block-uniform
#pragma unroll
    for (int mb = 0; mb < NRS; ++mb) {
      long n;
      int ho, wo;
      if (narrow) {
        const unsigned m = (unsigned)(mrow + mb * 32);
        const unsigned t = m / (unsigned)geo.Wout;
        wo = (int)(m - t * geo.Wout);
        const unsigned nn = t / (unsigned)geo.Hout;
        ho = (int)(t - nn * geo.Hout);
        n = nn;
      } else {
        long t = mrow + mb * 32;
        wo = (int)(t % geo.Wout); t /= geo.Wout;
        ho = (int)(t % geo.Hout);
        n = t / geo.Hout;
      }
      hb[mb] = ho * geo.stride - geo.pad;
      wb[mb] = wo * geo.sw - geo.pw;
      base[mb] = (unsigned long long)g +
                 ((n * geo.H + hb[mb]) * geo.W + wb[mb]) * (long)ld * 2;
    }
#pragma unroll
    for (int c = 0; c < NCS; ++c) {
      const int col = col0 + (c * NWAVES + wave) * 16 + (lane & 1) * 8;
      const bool in = col + 8 <= total_cols;
      if (MODE == 1) {
        toff[c] = col * 2;
        sel[c] = in ? 1u : NEVER;
      } else {
        // a unit never spans taps (cin % 8 == 0)
        const int tap = col / cin;
        const int kh = tap / geo.kw, kw = tap - kh * geo.kw;
        toff[c] = ((kh * geo.W + kw) * ld + (col - tap * cin)) * 2;
        sel[c] = in ? (1u << (kh & 15)) | (0x10000u << (kw & 15)) : NEVER;
      }
    }
  }

  // stage the current chunk (same bytes, same LDS slots as stage_tn2), then
  // step to the next
  __device__ __forceinline__ void stage(long M, const TnGeom& geo,
                                        const TnStep& st,
                                        const bf16* __restrict__ zp,
                                        bf16* lds) {
    const int lane = threadIdx.x % AMD_WAVE, wave = threadIdx.x / AMD_WAVE;
    unsigned rmask[NRS];
#pragma unroll
    for (int mb = 0; mb < NRS; ++mb) {
      const unsigned in =
          MODE == 1 ? 1u
                    : tn2_range_mask(hb[mb], geo.H, geo.kh) |
                          tn2_range_mask(wb[mb], geo.W, geo.kw) << 16;
      rmask[mb] = mrow + mb * 32 < M ? in : 0u;
    }
#pragma unroll
    for (int ss = 0; ss < NRS * NCS; ++ss) {
      const int mb = ss / NCS, c = ss % NCS;
      const int s = ss * NWAVES + wave;
      const unsigned long long a = base[mb] + toff[c];
      const unsigned long long src =
          (rmask[mb] & sel[c]) == sel[c] ? a : (unsigned long long)zp;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)(
              (char*)lds + s * 1024 + lane * 16),
          16, 0, 0);
    }
    mrow += MC;
#pragma unroll
    for (int mb = 0; mb < NRS; ++mb) {
      wb[mb] += st.dwb;
      const bool c1 = wb[mb] >= st.whi;
      wb[mb] -= c1 ? st.wspan : 0;
      hb[mb] += st.dhb + (c1 ? geo.stride : 0);
      const bool c2 = hb[mb] >= st.hhi;
      hb[mb] -= c2 ? st.hspan : 0;
      base[mb] += (long)(st.step + (c1 ? st.cw : 0) + (c2 ? st.ch : 0));
    }
  }
};

template <int N>
__device__ __forceinline__ void vmcnt_wait() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 10)
    asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  else if constexpr (N == 12)
    asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if constexpr (N == 16)
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else static_assert(N == 0, "unsupported vmcnt");
}

// Two hardware transpose reads -> one bf16x8 MFMA operand.
// addr = LDS tile base + lane*8 + (runtime wave column offset); OFF is the
// compile-time byte offset of the (sub, r=0) group; r=1 is the next group.
template <int OFF>
__device__ __forceinline__ bf16x8 tr_frag(unsigned addr) {
  u32x2 v0, v1;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2 offset:%3\n\t"
      "ds_read_b64_tr_b16 %1, %2 offset:%4"
      : "=&v"(v0), "=&v"(v1)
      : "v"(addr), "i"(OFF), "i"(OFF + GROUP_BYTES));
  union {
    unsigned int u[4];
    bf16x8 f;
  } pack;
  pack.u[0] = v0.x;
  pack.u[1] = v0.y;
  pack.u[2] = v1.x;
  pack.u[3] = v1.y;
  return pack.f;
}

// NW x KW = wave grid over the (n, k) output tile (NW*KW == 4); per-wave
// sub-tile is 64x64 (4x4 fragments).  MC = m rows staged per chunk.
// NBUF = LDS pipeline depth: 2 = classic double buffer with a full
// vmcnt(0) drain per chunk; 3 = stage TWO chunks ahead and only wait for
// the NEWEST chunk's loads at each barrier (counted vmcnt, guide T4) —
// each wave drains to <= its own newest-chunk loads before the barrier,
// so the chunk consumed next iteration is complete for every wave.
// BAND: group-diagonal wgrad (grouped conv, Cin == N, both % 128): each
// n-tile needs only ONE k-tile per tap (its own 128-channel window), so
// tiles = nbn*9 and the output is the COMPACT [N, 9*NCX] band.
// WALK (gather modes only): X addresses from TnWalk instead of stage_tn2.
template <int GMODE, int NW, int KW, int MC, int NBUF = 2, bool BAND = false,
          bool WALK = false>
__global__ void __launch_bounds__(
    NW * KW * 64,
    // the walk's state must not cost (1,4,32) its fourth block per CU
    // (40 KB LDS): hold it to the 128 VGPRs stage_tn2's version has
    (WALK && MC == 32 && NBUF == 2 ? 4 : NW * KW == 4 ? 2 : 1))
tn2_kernel(const bf16* __restrict__ dY, const bf16* __restrict__ X,
           float* __restrict__ parts, long M, int N, int K9, int Cin,
           TnGeom geo, int nbn, int nbk, int msplit,
           const bf16* __restrict__ zp, TnStep step) {
  static_assert(!WALK || GMODE != 0, "plain rows have nothing to walk");
  constexpr int NWAVES = NW * KW;  // 4 (256 thr, 2 blk/CU) or 8 (512, 1)
  constexpr int NCY = NW * 64;   // dY tile cols
  constexpr int NCX = KW * 64;   // X tile cols
  constexpr int KSTEPS = MC / 32;
  // counted vmcnt (NBUF 3) needs every wave to issue every load
  constexpr bool NSKIP = WALK && NBUF == 2 && NW == 2 && KW == 2;
  // per-thread global_load_lds issues per chunk (both operands):
  // subtiles = (MC/32)*(cols/16) per operand, one wave-round each
  constexpr int LC = (MC / 32) * (NCY / 16 + NCX / 16) * 64 / (NW * KW * 64);
  __shared__ __align__(16) char Ys[NBUF][tile_bytes<NCY, MC>()];
  __shared__ __align__(16) char Xs[NBUF][tile_bytes<NCX, MC>()];

  const int tiles = nbn * nbk;
  const int bid = xcd_swz_tn2(blockIdx.x, tiles * msplit);
  const int tile = bid % tiles;
  const int mpart = bid / tiles;
  const int bn = tile / nbk, bk = tile % nbk;
  const int n0 = bn * NCY;
  // BAND: bk is the TAP index; the k window is this n-tile's own channels
  const int k0 = BAND ? bk * Cin + n0 : bk * NCX;

  const long mchunks = (M + MC - 1) / MC;
  const long cpp = (mchunks + msplit - 1) / msplit;
  const long mc0 = (long)mpart * cpp;
  const long mc1 = min(mc0 + cpp, mchunks);

  const int t = threadIdx.x;
  const int wave = t / AMD_WAVE, lane = t % AMD_WAVE;
  const int wn = (wave / KW) * 64;  // n offset of this wave's sub-tile
  const int wk = (wave % KW) * 64;  // k offset
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  if (mc0 < mc1) {
    // per-wave LDS base addresses (bytes; +lane*8 is the tr-read's own slot)
    const unsigned ybase0 =
        (unsigned)(unsigned long long)(&Ys[0][0]) + lane * 8 +
        (wn / 16) * 2 * GROUP_BYTES;
    const unsigned xbase0 =
        (unsigned)(unsigned long long)(&Xs[0][0]) + lane * 8 +
        (wk / 16) * 2 * GROUP_BYTES;
    constexpr unsigned YB = tile_bytes<NCY, MC>();
    constexpr unsigned XB = tile_bytes<NCX, MC>();

    // X chunks are staged in order mc0, mc0 + 1, ...: the walk starts at
    // mc0 and every stage_x call moves it one chunk on
    TnWalk<WALK ? GMODE : 1, NCX, MC, NWAVES> xw;
    if constexpr (WALK) xw.init(X, Cin, mc0 * MC, k0, K9, Cin, geo);
    auto stage_x = [&](long mch, char* dst) {
      if constexpr (WALK)
        xw.stage(M, geo, step, zp, (bf16*)dst);
      else
        stage_tn2<GMODE, NCX, MC, NWAVES>(X, Cin, mch * MC, M, k0, K9, Cin,
                                          geo, zp, (bf16*)dst);
    };

    // NSKIP: where N <= 64 leaves the upper half of the 128-wide dY tile
    // padding, its subtiles are not staged and the waves that own it (their
    // results are never stored) skip their tr-reads and MFMAs
    auto stage_y = [&](long mch, char* dst) {
      stage_tn2<0, NCY, MC, NWAVES, NSKIP>(dY, N, mch * MC, M, n0, N, Cin, geo,
                                           zp, (bf16*)dst, step.nlive);
    };
    const bool live =
        !NSKIP || __builtin_amdgcn_readfirstlane(n0 + wn) < step.nlive;

    stage_y(mc0, Ys[0]);
    stage_x(mc0, Xs[0]);
    if (NBUF >= 3 && mc0 + 1 < mc1) {
      stage_y(mc0 + 1, Ys[1]);
      stage_x(mc0 + 1, Xs[1]);
      vmcnt_wait<LC>();  // chunk 0 complete; chunk 1 may stay in flight
    } else {
      vmcnt_wait<0>();
    }
    __builtin_amdgcn_s_barrier();

    for (long mc = mc0; mc < mc1; ++mc) {
      const int cur = (int)((mc - mc0) % NBUF);
      const long pre = NBUF >= 3 ? mc + 2 : mc + 1;
      if (pre < mc1) {
        const int nxt = (int)((pre - mc0) % NBUF);
        stage_y(pre, Ys[nxt]);
        stage_x(pre, Xs[nxt]);
      }
      const unsigned yb = ybase0 + cur * YB;
      const unsigned xb = xbase0 + cur * XB;
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        if (!live) break;  // wave-uniform
        bf16x8 a[4], b[4];
        // each 16-col subtile is 2 groups; the m-half (ks) advances by a
        // full row of subtiles
#pragma unroll
        for (int i = 0; i < 4; ++i)
          a[i] = tr_frag<0>(yb + (ks * (NCY / 16) + i) * 2 * GROUP_BYTES);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          b[j] = tr_frag<0>(xb + (ks * (NCX / 16) + j) * 2 * GROUP_BYTES);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[i], b[j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
      if (NBUF >= 3 && mc + 2 < mc1)
        vmcnt_wait<LC>();  // only the newest chunk's loads may remain
      else
        vmcnt_wait<0>();
      __builtin_amdgcn_s_barrier();
    }
  }

  // plain (non-atomic) per-mpart partial tile; BAND writes the compact
  // [N, 9*NCX] layout (col = tap*NCX + in-window offset)
  const int kout_cols = BAND ? 9 * NCX : K9;
  float* out = parts + (long)mpart * N * (long)kout_cols;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + i * 16 + fq * 4 + r;
        const int klocal = wk + j * 16 + fr;
        const int k = BAND ? bk * NCX + klocal : k0 + klocal;
        if (n < N && (BAND || k < K9))
          out[(long)n * kout_cols + k] = acc[i][j][r];
      }
}

// out[i] = sum over p in {slot, slot+step, ...} of parts[p][i] — fixed-order,
// vectorized.  Used two-stage for large msplit (a single-stage collapse of
// e.g. 170 partials x 36 K elems leaves only ~36 blocks = latency-bound;
// stage 1 folds to TN2_FOLD rows in parallel, stage 2 sums those).
constexpr int TN2_FOLD = 16;

__global__ void __launch_bounds__(AMD_TPB)
tn2_collapse_kernel(const float* __restrict__ parts, float* __restrict__ out,
                    int nparts, int step, long NK) {
  const long nv = NK / 4;
  const int slot = blockIdx.x % step;
  for (long i = (long)(blockIdx.x / step) * blockDim.x + threadIdx.x; i < nv;
       i += (long)(gridDim.x / step) * blockDim.x) {
    f32x4 s = ((const f32x4*)(parts + (long)slot * NK))[i];
    for (int p = slot + step; p < nparts; p += step) {
      f32x4 v = ((const f32x4*)(parts + (long)p * NK))[i];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    ((f32x4*)(out + (long)slot * NK))[i] = s;
  }
}

// semantics probe for ds_read_b64_tr_b16 (GPU test asserts the m156
// mapping: lane l, elem j  <-  lds[(l&15) + j*16 + (l>>4)*64])
__global__ void tr16_probe_kernel(const short* __restrict__ in,
                                  short* __restrict__ out) {
  __shared__ short lds[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) lds[i] = in[i];
  __syncthreads();
  if (threadIdx.x < 64) {
    const unsigned addr =
        (unsigned)(unsigned long long)(&lds[0]) + threadIdx.x * 8;
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:0"
                 : "=&v"(v) : "v"(addr));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    short4 s;
    __builtin_memcpy(&s, &v, 8);
    out[threadIdx.x * 4 + 0] = s.x;
    out[threadIdx.x * 4 + 1] = s.y;
    out[threadIdx.x * 4 + 2] = s.z;
    out[threadIdx.x * 4 + 3] = s.w;
  }
}

// Sum the msplit partials [msplit, NK] into out [NK] in a fixed order: one
// pass, or for large msplit a fold to TN2_FOLD rows and a pass over those.
static void tn2_collapse(const at::Tensor& parts, at::Tensor& out, int msplit,
                         long NK, hipStream_t stream) {
  TORCH_CHECK(NK % 4 == 0);
  const int nkgrid = amd_grid(NK / 4);
  if (msplit > 2 * TN2_FOLD) {
    auto folded = at::empty({TN2_FOLD, NK}, out.options());
    tn2_collapse_kernel<<<nkgrid * TN2_FOLD, AMD_TPB, 0, stream>>>(
        (const float*)parts.const_data_ptr(), folded.data_ptr<float>(),
        msplit, TN2_FOLD, NK);
    CHECK_CUDA_OK();
    tn2_collapse_kernel<<<nkgrid, AMD_TPB, 0, stream>>>(
        (const float*)folded.const_data_ptr(), out.data_ptr<float>(),
        TN2_FOLD, 1, NK);
    CHECK_CUDA_OK();
  } else {
    tn2_collapse_kernel<<<nkgrid, AMD_TPB, 0, stream>>>(
        (const float*)parts.const_data_ptr(), out.data_ptr<float>(), msplit,
        1, NK);
    CHECK_CUDA_OK();
  }
}

static at::Tensor tn2_zero_page(const at::Tensor& like) {
  static thread_local at::Tensor zp;
  if (!zp.defined() || zp.device() != like.device())
    zp = at::zeros({16}, like.options().dtype(at::kBFloat16));
  return zp;
}

// AMDTRAIN_TN2_ADDR=0: the gather modes derive every address from m again
// (stage_tn2) — the reference of the equality tests and the A/B.  Read per
// call, like AMDTRAIN_TN2_BLOCKS.
static bool tn2_walk_enabled() {
  const char* v = std::getenv("AMDTRAIN_TN2_ADDR");
  return !(v && v[0] == '0');
}

// AMDTRAIN_TN2_NSKIP=0: stage and multiply the padded half of the dY tile
// where N <= 64, as before (A/B; the outputs are the same either way)
static bool tn2_nskip_enabled() {
  const char* v = std::getenv("AMDTRAIN_TN2_NSKIP");
  return !(v && v[0] == '0');
}

// The steps of TnWalk for chunks of MC rows over rows of ld elements.
// Returns false where the walk's 32-bit offsets or 15-bit masks do not hold
// the geometry (no conv here comes near); stage_tn2 then serves it.
static bool tn2_make_step(const TnGeom& g, int MC, int ld, int N,
                          TnStep* st) {
  const long hw = (long)g.Hout * g.Wout;
  const long dn = MC / hw, rem = MC % hw;
  const long dh = rem / g.Wout, dw = rem % g.Wout;
  const long step =
      (dn * g.H * g.W + dh * g.stride * g.W + dw * g.sw) * ld * 2;
  const long cw = ((long)g.stride * g.W - (long)g.Wout * g.sw) * ld * 2;
  const long ch = ((long)g.H * g.W - (long)g.Hout * g.stride * g.W) * ld * 2;
  const long tap = ((long)g.kh * g.W + g.kw + 1) * ld * 2;
  const long lim = 1L << 29;  // step + cw + ch and base + tap stay in range
  if (std::abs(step) >= lim || std::abs(cw) >= lim || std::abs(ch) >= lim ||
      tap >= lim || g.kh > 15 || g.kw > 15 || g.pad > 15 || g.pw > 15 ||
      g.pad < 0 || g.pw < 0)
    return false;
  *st = TnStep{(int)step, (int)cw, (int)ch,
               (int)(dh * g.stride), (int)(dw * g.sw),
               g.Hout * g.stride - g.pad, g.Wout * g.sw - g.pw,
               g.Hout * g.stride, g.Wout * g.sw,
               tn2_nskip_enabled() ? N : 0x7fffffff};
  return true;
}

template <int GMODE, int NW, int KW, int MC, int NBUF = 2>
void tn2_launch(const at::Tensor& dY, const at::Tensor& X, at::Tensor& out,
                long M, int N, int K9, int Cin, TnGeom geo, int target_blocks,
                hipStream_t stream) {
  const int nbn = (N + NW * 64 - 1) / (NW * 64);
  const int nbk = (K9 + KW * 64 - 1) / (KW * 64);
  const long tiles = (long)nbn * nbk;
  const long mchunks = (M + MC - 1) / MC;
  int msplit = (int)std::max<long>(
      1, std::min<long>(mchunks, target_blocks / tiles));
  auto zp = tn2_zero_page(dY);
  at::Tensor parts = out;
  if (msplit > 1)
    parts = at::empty({msplit, (long)N * K9}, out.options());
  TnStep st{};
  bool walk = false;
  if constexpr (GMODE != 0)
    walk = tn2_walk_enabled() && tn2_make_step(geo, MC, Cin, N, &st);
  auto launch = [&](auto kernel) {
    kernel<<<(int)(tiles * msplit), NW * KW * 64, 0, stream>>>(
        (const bf16*)dY.const_data_ptr(), (const bf16*)X.const_data_ptr(),
        parts.data_ptr<float>(), M, N, K9, Cin, geo, nbn, nbk, msplit,
        (const bf16*)zp.const_data_ptr(), st);
  };
  if constexpr (GMODE != 0) {
    if (walk)
      launch(tn2_kernel<GMODE, NW, KW, MC, NBUF, false, true>);
    else
      launch(tn2_kernel<GMODE, NW, KW, MC, NBUF>);
  } else {
    launch(tn2_kernel<GMODE, NW, KW, MC, NBUF>);
  }
  CHECK_CUDA_OK();
  if (msplit > 1) tn2_collapse(parts, out, msplit, (long)N * K9, stream);
}

}  // namespace

// Unified TN wgrad v2.  gmode: 0 = plain rows (1x1 s1 / linear), 1 =
// strided-1x1 row gather, 2 = conv tap gather (taps*Cin columns; kh x kw
// filter, stride / pad along h, stride_w / pad_w along w).
// Returns fp32 [N, taps*Cin]; bitwise deterministic (fixed split + ordered
// collapse).
at::Tensor tn2_wgrad(at::Tensor dY, at::Tensor X, long taps, long Nn, long H,
                     long W, long stride, long gmode, long kh, long kw,
                     long pad, long stride_w, long pad_w, long Hout,
                     long Wout) {
  TORCH_CHECK(dY.is_cuda() && dY.scalar_type() == at::kBFloat16 &&
              X.scalar_type() == at::kBFloat16);
  auto Yc = dY.contiguous();
  auto Xc = X.contiguous();
  const long M = Yc.size(0);
  const int N = (int)Yc.size(1);
  const int Cin = (int)Xc.size(1);
  const int K9 = (int)(taps * Cin);
  TORCH_CHECK(Cin % 8 == 0 && N % 8 == 0,
              "tn2_wgrad needs dY columns (Cout) and X columns (Cin) that are "
              "multiples of 8, got Cout = ", N, ", Cin = ", Cin);
  TnGeom geo{0, 0, 0, 0, 1, 3, 3, 1, 1, 1};
  if (gmode == 1) {
    long Hout = (H + stride - 1) / stride, Wout = (W + stride - 1) / stride;
    TORCH_CHECK(M == Nn * Hout * Wout);
    geo = TnGeom{(int)H, (int)W, (int)Hout, (int)Wout, (int)stride, 1, 1, 0,
                 (int)stride, 0};
  } else if (gmode == 2) {
    // stride_w == 0 / pad_w < 0 / Hout, Wout == 0: same as along h,
    // symmetric padding (explicit output dims serve asymmetric padding)
    const long sw = stride_w > 0 ? stride_w : stride;
    const long pw = pad_w >= 0 ? pad_w : pad;
    if (Hout <= 0) Hout = (H + 2 * pad - kh) / stride + 1;
    if (Wout <= 0) Wout = (W + 2 * pw - kw) / sw + 1;
    TORCH_CHECK(M == Nn * Hout * Wout && taps == kh * kw);
    TORCH_CHECK(Xc.size(0) == Nn * H * W);
    geo = TnGeom{(int)H, (int)W, (int)Hout, (int)Wout, (int)stride,
                 (int)kh, (int)kw, (int)pad, (int)sw, (int)pw};
  } else {
    TORCH_CHECK(M == Xc.size(0));
  }
  auto out = at::empty({(long)N, (long)K9}, Yc.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  const char* tb = std::getenv("AMDTRAIN_TN2_BLOCKS");
  const int target = tb ? atoi(tb) : 512;

  // config: (2,2) 128x128 tile MC=64 default; skinny-N with wide K -> (1,4);
  // skinny-K with tall N -> (4,1) (both MC=32 to keep 2 blocks/CU in LDS)
  // thin-channel tap gather (the stem, Cin = 8): also below K9 = 256, where
  // the 256-wide k-tile of (1,4,32) holds all of K9 and dY is staged once
  if (N < 128 && (K9 >= 256 || (gmode == 2 && Cin < 32))) {
    // skinny-N conv wgrad: the (2,2,64) tile zero-pads the N half but its
    // MC=64 pipeline beats the fully-dense (1,4,32) config (which is
    // issue-bound at 16 MFMA/barrier) for layer-1-class shapes; the
    // channel-padded STEM (Cin=8) measured the other way (1.55 vs 1.78 ms
    // at b512) — its 16x-redundant tap gather prefers the narrower k-tile.
    // A/B via AMDTRAIN_TN2_14.  The space-to-depth stem (28 taps, K9 = 224)
    // fits the 256-wide k-tile of (1,4,32) whole, so dY is staged once:
    // 0.63 ms against 0.82 ms on (2,2,64) and 1.45 ms for the 49-tap form
    // (b512, tools/bench_wgrad.py --stem; AMDTRAIN_TN2_STEM22 forces (2,2,64))
    // Those figures predate TnWalk.  On the walk (bench_wgrad.py --configs):
    // layer-1 3x3 254 us here against 253 us on (1,4,32), a tie; the stems
    // 625 / 352 us on (1,4,32) against 760 / 396 us on (2,2,64).
    if (gmode == 2 && Cin >= 32 && std::getenv("AMDTRAIN_TN2_14") == nullptr)
      tn2_launch<2, 2, 2, 64>(Yc, Xc, out, M, N, K9, Cin, geo, target, stream);
    else if (gmode == 2 && std::getenv("AMDTRAIN_TN2_STEM22") != nullptr)
      tn2_launch<2, 2, 2, 64>(Yc, Xc, out, M, N, K9, Cin, geo, target, stream);
    else if (gmode == 2)
      tn2_launch<2, 1, 4, 32>(Yc, Xc, out, M, N, K9, Cin, geo, target, stream);
    else if (gmode == 1)
      tn2_launch<1, 2, 2, 64>(Yc, Xc, out, M, N, K9, Cin, geo, target, stream);
    else
      tn2_launch<0, 1, 4, 32>(Yc, Xc, out, M, N, K9, Cin, geo, target, stream);
  } else if (K9 < 128 && N >= 256 && gmode == 0) {
    tn2_launch<0, 4, 1, 32>(Yc, Xc, out, M, N, K9, Cin, geo, target, stream);
  } else {
    static const bool pipe3 = []() {
      const char* v = std::getenv("AMDTRAIN_TN2_PIPE3");
      return v && v[0] == '1';
    }();
    static const int w8 = []() {  // A/B override: 1 always, 0 never
      const char* v = std::getenv("AMDTRAIN_TN2_W8");
      return v && v[0] == '1' ? 1 : v && v[0] == '0' ? 0 : -1;
    }();
    const bool wide8 = w8 == 1;
    // 8-wave (2m x 4k) block halves dY re-reads (two k-tiles per staged
    // chunk); measured +11% at deep-K (K9=4608 layer4 3x3), flat at
    // smaller K (L3 already absorbs those re-reads) -> auto for K>=4096
    if ((wide8 || (w8 != 0 && gmode == 2 && K9 >= 4096)) && K9 % 256 == 0
        && gmode != 1) {
      if (gmode == 2)
        tn2_launch<2, 2, 4, 64>(Yc, Xc, out, M, N, K9, Cin, geo, target,
                                stream);
      else
        tn2_launch<0, 2, 4, 64>(Yc, Xc, out, M, N, K9, Cin, geo, target,
                                stream);
    } else if (pipe3) {
      // A/B: 3-buffer counted-vmcnt pipeline at MC=32 (48 KB LDS -> 3
      // blocks/CU).  MEASURED -10..-15% vs the MC=64 double buffer
      // (docs/KERNELS.md negative-results) — kept off-by-default
      if (gmode == 2)
        tn2_launch<2, 2, 2, 32, 3>(Yc, Xc, out, M, N, K9, Cin, geo, target,
                                   stream);
      else if (gmode == 1)
        tn2_launch<1, 2, 2, 32, 3>(Yc, Xc, out, M, N, K9, Cin, geo, target,
                                   stream);
      else
        tn2_launch<0, 2, 2, 32, 3>(Yc, Xc, out, M, N, K9, Cin, geo, target,
                                   stream);
    } else if (gmode == 2) {
      tn2_launch<2, 2, 2, 64>(Yc, Xc, out, M, N, K9, Cin, geo, target, stream);
    } else if (gmode == 1) {
      tn2_launch<1, 2, 2, 64>(Yc, Xc, out, M, N, K9, Cin, geo, target, stream);
    } else {
      tn2_launch<0, 2, 2, 64>(Yc, Xc, out, M, N, K9, Cin, geo, target, stream);
    }
  }
  return out;
}

// Group-diagonal conv3x3 wgrad: returns the COMPACT band [Cout, 9*128]
// (column = tap*128 + channel offset within the cout-row's own 128-wide
// group window).  Requires Cin == Cout, both % 128.
at::Tensor tn2_wgrad_banded(at::Tensor dY, at::Tensor X, long Nn, long H,
                            long W, long stride) {
  TORCH_CHECK(dY.is_cuda() && dY.scalar_type() == at::kBFloat16 &&
              X.scalar_type() == at::kBFloat16);
  auto Yc = dY.contiguous();
  auto Xc = X.contiguous();
  const long M = Yc.size(0);
  const int N = (int)Yc.size(1);
  const int Cin = (int)Xc.size(1);
  TORCH_CHECK(N == Cin && N % 128 == 0);
  long Hout = (H + 2 - 3) / stride + 1, Wout = (W + 2 - 3) / stride + 1;
  TORCH_CHECK(M == Nn * Hout * Wout);
  TnGeom geo{(int)H, (int)W, (int)Hout, (int)Wout, (int)stride, 3, 3, 1,
             (int)stride, 1};
  auto out = at::empty({(long)N, (long)9 * 128},
                       Yc.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  const char* tb = std::getenv("AMDTRAIN_TN2_BLOCKS");
  const int target = tb ? atoi(tb) : 512;
  const int nbn = N / 128, nbk = 9;
  const long tiles = (long)nbn * nbk;
  const long mchunks = (M + 63) / 64;
  int msplit = (int)std::max<long>(
      1, std::min<long>(mchunks, target / tiles));
  auto zp = tn2_zero_page(Yc);
  at::Tensor parts = out;
  if (msplit > 1)
    parts = at::empty({msplit, (long)N * 9 * 128}, out.options());
  TnStep st{};
  const bool walk = tn2_walk_enabled() && tn2_make_step(geo, 64, Cin, N, &st);
  auto launch = [&](auto kernel) {
    kernel<<<(int)(tiles * msplit), TN2_TPB, 0, stream>>>(
        (const bf16*)Yc.const_data_ptr(), (const bf16*)Xc.const_data_ptr(),
        parts.data_ptr<float>(), M, N, 9 * Cin, Cin, geo, nbn, nbk, msplit,
        (const bf16*)zp.const_data_ptr(), st);
  };
  if (walk)
    launch(tn2_kernel<2, 2, 2, 64, 2, true, true>);
  else
    launch(tn2_kernel<2, 2, 2, 64, 2, true>);
  CHECK_CUDA_OK();
  if (msplit > 1)
    tn2_collapse(parts, out, msplit, (long)N * 9 * 128, stream);
  return out;
}

at::Tensor tr16_probe(at::Tensor in) {
  TORCH_CHECK(in.is_cuda() && in.scalar_type() == at::kShort &&
              in.numel() == 256);
  auto inc = in.contiguous();
  auto out = at::zeros({64, 4}, inc.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  tr16_probe_kernel<<<1, 64, 0, stream>>>(
      (const short*)inc.const_data_ptr(), out.data_ptr<short>());
  CHECK_CUDA_OK();
  return out;
}
