// Weight-only OCP MX e4m3 GEMVs of the KV-cached decode step for gfx950 (MI355X): svla_mx_scales_rowmajor,
// svla_gemv_mxfp8 and svla_head_gemv_mxfp8, and their forms under unmerged LoRA adapters, svla_lora_gemv_mxfp8 and
// svla_lora_head_gemv_mxfp8 (include/svla.h).
//
// A decode step streams every Gemma2 projection weight and lm_head once from HBM; with the weights kept as the e4m3
// values of svla_quant_mx_rows (one E8M0 exponent per 32 consecutive k) a token moves half the bytes.  Activations stay
// bf16 and the accumulation fp32: a lane converts the 16 e4m3 bytes of one 16-B load to fp32 in registers
// (v_cvt_pk_f32_fp8), sums their products with x in k order and adds the sum times the block's 2^X to its accumulator
// -- 16 consecutive k never straddle a 32-k block, so every load needs one exponent byte.  The exponents are read from
// a row-major [N][K/32] repack (svla_mx_scales_rowmajor), contiguous beside the row the lane streams; the tile-major
// layout of the MFMA GEMMs would cost a lane one cache line per 128 k.
//   mxg_kernel         one wave per two output rows (STORE) or per gate|up row pair (GEGLU); lane l owns
//                      k = 16 l + 1024 i, all chunks of both rows in flight before the first FMA (K <= 4096), then the
//                      wave butterfly;
//   mxg_norm2_kernel   the same with the Gemma2 norm pair of svla_gemv_rmsnorm2 in its prologue (gemm.hip
//                      gemv_norm2_kernel's chunk map and reduction order: h and x are svla_add_rmsnorm2_fwd's bits);
//   mxg_splitk_kernel  long K (the down projection, K = 9216): the four waves of a block split one row's K range and
//                      their partial sums are added through LDS in wave order;
//   mxh_kernel         the decode head: a block owns 128 consecutive vocabulary rows (one statistics group of
//                      svla_softcap_ce_rows), each wave walks its rows with mxg_kernel's per-row dot product (the next
//                      row in flight while this one is summed) and leaves the raw bf16 logit in LDS; 16 lanes per
//                      token row then run svla_softcap_ce_rows' per-element unit and group combine.
// Under unmerged adapters (the AD instances of mxg_kernel, mxg_splitk_kernel and mxh_kernel) the frozen base weight is
// the e4m3 copy and the rank-r term is added in bf16 inside the same pass, as lora_decode.hip does over bf16 weights:
// lane j < r holds B[n, j] and T[m, j] (lora_adapter.h), one product per lane and a wave butterfly, then
// y = bf16(bf16(base) + bf16(s l)).  The base sum is the AD = false instance's, bit for bit; the adapter operands are
// loaded ahead of the weight stream, and the M = 1 instances keep the occupancy of their parents within one wave.
// fp32 accumulation in a fixed order (fmaf only, so the contraction mode cannot change it), 16-B non-temporal weight
// reads, no atomics, no block waits for another block, no allocation and no host synchronisation (graph-capturable).
#include "softcap_tab.h"
#include "lora_adapter.h"

namespace {

constexpr int MXG_MAXM = 8;
constexpr int MXG_MAXSEG = 3;
constexpr int MXG_NORM_MAX_K = 2560;
constexpr int MXG_GN_MAXC = 2;  // norm chunks per thread (256 threads x 8 elements x 2 >= 2560)
constexpr int MXH_COLS = 128;
constexpr int MXH_MAX_K = 4096;

struct MxRows {  // svla_mxfp8_rows with typed pointers
  const uint8_t *q0, *q1, *q2;  // scalar fields: the struct stays in kernel-argument registers
  const uint8_t *s0, *s1, *s2;
  int64_t st1, st2;
  int64_t ldq, lds;
  int nseg;
};
struct MxNorm2 {  // svla_lora_norm2 with typed pointers
  const bf16_t* res;
  const bf16_t* y;
  const bf16_t* w1;
  const bf16_t* w2;
  bf16_t* h_out;
  int64_t ld;
  float eps1, eps2;
};
struct MxOut {
  bf16_t* c;
  bf16_t* g;
  bf16_t* u;
  int64_t ldc, ldg, ldu;
};
struct MxAd {  // the unmerged adapters of svla_lora_gemv_mxfp8: T [M][ldt], the B segments, the scaling
  const bf16_t* T;
  int64_t ldt;
  Segs S;
  float sc;
};
struct MxHeadAd {  // the lm_head adapter of svla_lora_head_gemv_mxfp8
  const bf16_t* T;
  const bf16_t* B;
  int64_t ldt, ldb;
  int r;
  float sc;
};

// e4m3 row n and its exponent row of a weight of up to three row segments (q|k|v)
__device__ __forceinline__ void mx_row(const MxRows& W, int64_t n, const uint8_t*& q, const uint8_t*& s) {
  // The fields are pinned in scalar registers first.  With ROCm 7.2 (AMD clang 22) a select between loads of
  // kernel-argument fields is folded into one load from a selected address, which puts a 96-B copy of the struct in
  // scratch in every STORE instance (hipcc -Rpass-analysis=kernel-resource-usage: "ScratchSize [bytes/lane]" 96
  // without the asm, 0 with it -- the figure to check when the compiler changes).  The fields are kernel arguments,
  // hence uniform, which is what the "s" constraint asks for; the asm emits no instruction.
  const uint8_t *q0 = W.q0, *q1 = W.q1, *q2 = W.q2, *s0 = W.s0, *s1 = W.s1, *s2 = W.s2;
  int64_t st1 = W.st1, st2 = W.st2;
  asm volatile("" : "+s"(q0), "+s"(q1), "+s"(q2), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(st1), "+s"(st2));
  const int sg = (int)(W.nseg > 1 && n >= st1) + (int)(W.nseg > 2 && n >= st2);
  const uint8_t* qb = sg == 0 ? q0 : (sg == 1 ? q1 : q2);
  const uint8_t* sb = sg == 0 ? s0 : (sg == 1 ? s1 : s2);
  const int64_t r = n - (sg == 0 ? 0 : (sg == 1 ? st1 : st2));
  q = qb + r * W.ldq;
  s = sb + r * W.lds;
}

// 2^(b - 127) of an E8M0 byte: 0xFF is the quantiser's NaN block, 0 (X = -127) is below the normal range
__device__ __forceinline__ float e8m0(uint32_t b) {
  return b == 0xffu ? __uint_as_float(0x7fc00000u)
                    : (b == 0u ? __uint_as_float(0x00400000u) : __uint_as_float(b << 23));
}

// 16 e4m3 bytes (k order) -> fp32
__device__ __forceinline__ void cvt16(const u32x4 w, float* f) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], true);
    f[4 * d] = lo[0];
    f[4 * d + 1] = lo[1];
    f[4 * d + 2] = hi[0];
    f[4 * d + 3] = hi[1];
  }
}

// One 16-k chunk of NR weight rows against the M rows of x (xk = x + k, row stride ldx):
// acc[r][m] = fma(2^X_r, sum_{j < 16, in order} x[m][k + j] q_r[k + j], acc[r][m]) -- the only arithmetic of the dot
// products, shared by every kernel so the same K gives the same bits in all of them.
template <int NR, int MR>
__device__ __forceinline__ void mx_fma(const u32x4 (&w)[NR], const uint32_t (&sb)[NR], int M, const bf16_t* xk,
                                       int64_t ldx, float (&acc)[NR][MR]) {
  float wf[NR][16], sc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    cvt16(w[r], wf[r]);
    sc[r] = e8m0(sb[r]);
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    if (m < M) {
      float xf[16];
      unpack8(*reinterpret_cast<const u32x4*>(xk + m * ldx), xf);
      unpack8(*reinterpret_cast<const u32x4*>(xk + m * ldx + 8), xf + 8);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) p = fmaf(wf[r][j], xf[j], p);
        acc[r][m] = fmaf(sc[r], p, acc[r][m]);
      }
    }
  }
}

__device__ __forceinline__ u32x4 mx_ld16(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

// STORE / GEGLU stores of one output row n (STORE: v[0]; GEGLU: v = {g, u} of SVLA_EPI_GEGLU's element formula)
template <bool GEGLU>
__device__ __forceinline__ void mx_store(const MxOut& O, int m, int64_t n, float v0, float v1) {
  if constexpr (GEGLU) {
    const float g = round_bf(v0), u = round_bf(v1);
    O.c[m * O.ldc + n] = f2bf(gelu_bf16(g) * u);
    O.g[m * O.ldg + n] = f2bf(g);
    O.u[m * O.ldu + n] = f2bf(u);
  } else {
    O.c[m * O.ldc + n] = f2bf(v0);
  }
}

// ------------------------------------------------------------------------------------------------ mxg_kernel
// KCH > 0: K <= 1024 KCH, every chunk of the wave's two rows loaded before the first FMA; KCH == 0: a runtime loop
// (the same per-lane order).  rows: output rows (GEGLU: I, the wave's two weight rows are gate row n and up row n).
// AD (svla_lora_gemv_mxfp8): each of the wave's two rows also carries its adapter operands (lora_adapter.h), loaded
// ahead of the weight stream, and its sum goes through ad_finish; the base sum is the AD = false instance's.
template <int KCH, bool GEGLU, int MR, bool AD>
__global__ __launch_bounds__(256) void mxg_kernel(int M, int64_t rows, int64_t K, const bf16_t* __restrict__ x,
                                                  int64_t ldx, MxRows W, MxOut O, MxAd A) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t r0 = GEGLU ? wave : wave * 2;
  if (r0 >= rows) return;
  AdRow<MR> ad[2];
  if constexpr (AD) {
    if constexpr (GEGLU) {
      ad_load(ad[0], A.S, 0, r0, A.T, A.ldt, M, lane);
      ad_load(ad[1], A.S, 1, r0, A.T, A.ldt, M, lane);
    } else {
      const int64_t r1 = r0 + 1 < rows ? r0 + 1 : rows - 1;
      const int s0 = seg_of(A.S, r0), s1 = seg_of(A.S, r1);
      ad_load(ad[0], A.S, s0, r0 - seg_st(A.S, s0), A.T, A.ldt, M, lane);
      ad_load(ad[1], A.S, s1, r1 - seg_st(A.S, s1), A.T, A.ldt, M, lane);
    }
  }
  const uint8_t *qp[2], *sp[2];
  if constexpr (GEGLU) {
    qp[0] = W.q0 + r0 * W.ldq;
    sp[0] = W.s0 + r0 * W.lds;
    qp[1] = W.q1 + r0 * W.ldq;
    sp[1] = W.s1 + r0 * W.lds;
  } else {
    mx_row(W, r0, qp[0], sp[0]);
    mx_row(W, r0 + 1 < rows ? r0 + 1 : rows - 1, qp[1], sp[1]);
  }
  float acc[2][MR];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[r][m] = 0.f;
  if constexpr (KCH > 0) {
    u32x4 wq[KCH][2];
    uint32_t sb[KCH][2];
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int64_t k = (int64_t)lane * 16 + i * 1024;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        wq[i][r] = u32x4{0u, 0u, 0u, 0u};
        sb[i][r] = 0u;
        if (k < K) {
          wq[i][r] = mx_ld16(qp[r] + k);
          sb[i][r] = sp[r][k >> 5];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int64_t k = (int64_t)lane * 16 + i * 1024;
      if (k < K) mx_fma<2, MR>(wq[i], sb[i], M, x + k, ldx, acc);
    }
  } else {
#pragma unroll 2
    for (int64_t k = (int64_t)lane * 16; k < K; k += 1024) {
      u32x4 wq[2];
      uint32_t sb[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        wq[r] = mx_ld16(qp[r] + k);
        sb[r] = sp[r][k >> 5];
      }
      mx_fma<2, MR>(wq, sb, M, x + k, ldx, acc);
    }
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    if (m < M) {
      float v0 = wave_sum(acc[0][m]), v1 = wave_sum(acc[1][m]);
      if constexpr (AD) {
        v0 = ad_finish(ad[0], m, v0, A.sc);
        v1 = ad_finish(ad[1], m, v1, A.sc);
      }
      if (lane == 0) {
        if constexpr (GEGLU) {
          mx_store<true>(O, m, r0, v0, v1);
        } else {
          mx_store<false>(O, m, r0, v0, 0.f);
          if (r0 + 1 < rows) mx_store<false>(O, m, r0 + 1, v1, 0.f);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ mxg_norm2_kernel
// The norm pair in the prologue (gemm.hip gemv_norm2_kernel: rms_add_norm2_kernel's chunk map and reduction order, so h
// and x are bitwise svla_add_rmsnorm2_fwd's outputs), computed per block into LDS, h also stored by block 0; every
// thread issues its norm-input loads before its weight loads and the norm's block reductions use raw barriers, so the
// weight stream is in flight while the norms run.  Then mxg_kernel's dot products on the LDS x.
template <int KCH, bool GEGLU, int MR>
__global__ __launch_bounds__(256) void mxg_norm2_kernel(int M, int64_t rows, int64_t K, MxNorm2 Nn, MxRows W, MxOut O) {
  extern __shared__ __attribute__((aligned(16))) char mxg_smem[];  // [M][K] bf16 x, then the reduction slots
  bf16_t* const xs = reinterpret_cast<bf16_t*>(mxg_smem);
  float (*red)[4] = reinterpret_cast<float (*)[4]>(mxg_smem + (size_t)M * K * 2);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int nch = (int)(K >> 3);
  const int64_t ldn = Nn.ld;
  u32x4 yv[MR][MXG_GN_MAXC], rv[MR][MXG_GN_MAXC], w1v[MXG_GN_MAXC], w2v[MXG_GN_MAXC];
#pragma unroll
  for (int cI = 0; cI < MXG_GN_MAXC; ++cI) {
    const int ch = t + cI * 256;
    w1v[cI] = w2v[cI] = u32x4{0u, 0u, 0u, 0u};
    if (ch < nch) {
      w1v[cI] = *reinterpret_cast<const u32x4*>(Nn.w1 + ch * 8);
      w2v[cI] = *reinterpret_cast<const u32x4*>(Nn.w2 + ch * 8);
    }
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      yv[m][cI] = rv[m][cI] = u32x4{0u, 0u, 0u, 0u};
      if (m < M && ch < nch) {
        yv[m][cI] = *reinterpret_cast<const u32x4*>(Nn.y + m * ldn + ch * 8);
        rv[m][cI] = *reinterpret_cast<const u32x4*>(Nn.res + m * ldn + ch * 8);
      }
    }
  }
  // weight stream (as mxg_kernel)
  const int64_t wave = (int64_t)blockIdx.x * 4 + wv;
  const int64_t r0 = GEGLU ? wave : wave * 2;
  const int64_t rc = r0 < rows ? r0 : rows - 1;
  const uint8_t *qp[2], *sp[2];
  if constexpr (GEGLU) {
    qp[0] = W.q0 + rc * W.ldq;
    sp[0] = W.s0 + rc * W.lds;
    qp[1] = W.q1 + rc * W.ldq;
    sp[1] = W.s1 + rc * W.lds;
  } else {
    mx_row(W, rc, qp[0], sp[0]);
    mx_row(W, rc + 1 < rows ? rc + 1 : rows - 1, qp[1], sp[1]);
  }
  u32x4 wq[KCH][2];
  uint32_t sb[KCH][2];
#pragma unroll
  for (int i = 0; i < KCH; ++i) {
    const int64_t k = (int64_t)lane * 16 + i * 1024;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      wq[i][r] = u32x4{0u, 0u, 0u, 0u};
      sb[i][r] = 0u;
      if (k < K) {
        wq[i][r] = mx_ld16(qp[r] + k);
        sb[i][r] = sp[r][k >> 5];
      }
    }
  }
  // the norms, one row at a time (block_sum's order: wave butterfly, then the four waves in order)
  auto bsum = [&](float v, int slot) {
    v = wave_sum(v);
    if (lane == 0) red[slot][wv] = v;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    return ((red[slot][0] + red[slot][1]) + red[slot][2]) + red[slot][3];
  };
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    if (m < M) {
      float v[MXG_GN_MAXC][8];
      float ss = 0.f;
#pragma unroll
      for (int cI = 0; cI < MXG_GN_MAXC; ++cI)
        if (t + cI * 256 < nch) {
          unpack8(yv[m][cI], v[cI]);
#pragma unroll
          for (int j = 0; j < 8; ++j) ss += v[cI][j] * v[cI][j];
        }
      const float rstd1 = rsqrtf(bsum(ss, 0) / (float)K + Nn.eps1);
      float ss2 = 0.f;
#pragma unroll
      for (int cI = 0; cI < MXG_GN_MAXC; ++cI) {
        const int ch = t + cI * 256;
        if (ch < nch) {
          float wf[8], r[8];
          unpack8(w1v[cI], wf);
          unpack8(rv[m][cI], r);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            v[cI][j] = round_bf(r[j] + round_bf((v[cI][j] * rstd1) * (1.0f + wf[j])));
            ss2 += v[cI][j] * v[cI][j];
          }
          if (blockIdx.x == 0) *reinterpret_cast<u32x4*>(Nn.h_out + m * ldn + ch * 8) = pack8(v[cI]);
        }
      }
      const float rstd2 = rsqrtf(bsum(ss2, 1) / (float)K + Nn.eps2);
#pragma unroll
      for (int cI = 0; cI < MXG_GN_MAXC; ++cI) {
        const int ch = t + cI * 256;
        if (ch < nch) {
          float wf[8], o[8];
          unpack8(w2v[cI], wf);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (v[cI][j] * rstd2) * (1.0f + wf[j]);
          *reinterpret_cast<u32x4*>(xs + m * K + ch * 8) = pack8(o);
        }
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (r0 >= rows) return;
  float acc[2][MR];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[r][m] = 0.f;
#pragma unroll
  for (int i = 0; i < KCH; ++i) {
    const int64_t k = (int64_t)lane * 16 + i * 1024;
    if (k < K) mx_fma<2, MR>(wq[i], sb[i], M, xs + k, K, acc);
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    if (m < M) {
      const float v0 = wave_sum(acc[0][m]), v1 = wave_sum(acc[1][m]);
      if (lane == 0) {
        if constexpr (GEGLU) {
          mx_store<true>(O, m, r0, v0, v1);
        } else {
          mx_store<false>(O, m, r0, v0, 0.f);
          if (r0 + 1 < rows) mx_store<false>(O, m, r0 + 1, v1, 0.f);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ mxg_splitk_kernel
// One block per output row: thread t owns k = 16 t + 4096 i (K <= 12288: all three chunks in flight at once), the four
// waves' partial sums are added in wave order.  AD: wave 0 also carries the row's adapter term (lora_decode.hip's
// lg_split_kernel), left in part[4].
template <int MR, bool AD>
__global__ __launch_bounds__(256) void mxg_splitk_kernel(int M, int64_t rows, int64_t K, const bf16_t* __restrict__ x,
                                                         int64_t ldx, MxRows W, bf16_t* __restrict__ c, int64_t ldc,
                                                         MxAd A) {
  __shared__ float part[AD ? 5 : 4][MXG_MAXM];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t n = blockIdx.x;
  AdRow<MR> ad;
  if constexpr (AD) {
    if (w == 0) {  // wave-uniform
      const int s = seg_of(A.S, n);
      ad_load(ad, A.S, s, n - seg_st(A.S, s), A.T, A.ldt, M, lane);
    }
  }
  const uint8_t *qp, *sp;
  mx_row(W, n, qp, sp);
  float acc[1][MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[0][m] = 0.f;
  if (K <= 3 * 4096) {
    constexpr int KCH = 3;
    u32x4 wq[KCH][1];
    uint32_t sb[KCH][1];
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int64_t k = (int64_t)threadIdx.x * 16 + i * 4096;
      wq[i][0] = u32x4{0u, 0u, 0u, 0u};
      sb[i][0] = 0u;
      if (k < K) {
        wq[i][0] = mx_ld16(qp + k);
        sb[i][0] = sp[k >> 5];
      }
    }
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int64_t k = (int64_t)threadIdx.x * 16 + i * 4096;
      if (k < K) mx_fma<1, MR>(wq[i], sb[i], M, x + k, ldx, acc);
    }
  } else {
#pragma unroll 2
    for (int64_t k = (int64_t)threadIdx.x * 16; k < K; k += 4096) {
      u32x4 wq[1] = {mx_ld16(qp + k)};
      uint32_t sb[1] = {sp[k >> 5]};
      mx_fma<1, MR>(wq, sb, M, x + k, ldx, acc);
    }
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    if (m < M) {
      const float v = wave_sum(acc[0][m]);
      if (lane == 0) part[w][m] = v;
      if constexpr (AD) {
        if (w == 0) {  // wave-uniform
          const float l = wave_sum(ad.b * ad.t[m]);
          if (lane == 0) part[4][m] = l;
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < M) {
    const int m = threadIdx.x;
    const float base = ((part[0][m] + part[1][m]) + part[2][m]) + part[3][m];
    if constexpr (AD) c[m * ldc + n] = f2bf(round_bf(round_bf(base) + round_bf(A.sc * part[4][m])));  // ad_finish
    else c[m * ldc + n] = f2bf(base);
  }
}

// ------------------------------------------------------------------------------------------------ mxh_kernel
template <int CTRL>
__device__ __forceinline__ int mxh_dpp(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float mxh_dppf(float x) {
  return __int_as_float(mxh_dpp<CTRL>(__float_as_int(x)));
}
constexpr int MXH_X1 = 0xb1, MXH_X2 = 0x4e, MXH_HALF_MIRROR = 0x141, MXH_MIRROR = 0x140;  // softcap.hip's butterfly

// AD (svla_lora_head_gemv_mxfp8): lane j < r also holds T[m, j] and, with each weight row, B[n, j]; the raw logit is
// lora_decode.hip lh_kernel's y = bf16(bf16(base) + bf16(s T B)).
template <int KCH, int MR, bool AD>
__global__ __launch_bounds__(256) void mxh_kernel(int M, int64_t N, int64_t K, const bf16_t* __restrict__ x, int64_t ldx,
                                                  const uint8_t* __restrict__ Q, int64_t ldq,
                                                  const uint8_t* __restrict__ S, int64_t lds, float cap,
                                                  bf16_t* __restrict__ lg, int64_t ld, float* __restrict__ row_stats,
                                                  MxHeadAd A) {
  __shared__ __attribute__((aligned(16))) unsigned short tab[TANH_TAB_BYTES / 2 + 8];
  __shared__ __attribute__((aligned(16))) bf16_t ys[MXG_MAXM][MXH_COLS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < TANH_TAB_BYTES / 16)
    reinterpret_cast<u32x4*>(tab)[tid] = reinterpret_cast<const u32x4*>(svla_tanh_bf16_tab)[tid];
  const int64_t n0 = (int64_t)blockIdx.x * MXH_COLS;
  const int nrow = (int)(N - n0 < MXH_COLS ? N - n0 : MXH_COLS);
  const bool on = AD && lane < A.r;
  float tv[MR];
  if constexpr (AD) {
#pragma unroll
    for (int m = 0; m < MR; ++m) tv[m] = (on && m < M) ? bf2f(A.T[m * A.ldt + lane]) : 0.f;
  }
  auto load_row = [&](int64_t n, u32x4 (&w)[KCH][1], uint32_t (&sb)[KCH][1], float& b) {
    const uint8_t* qr = Q + n * ldq;
    const uint8_t* sr = S + n * lds;
    if constexpr (AD) b = on ? bf2f(A.B[n * A.ldb + lane]) : 0.f;
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int64_t k = (int64_t)lane * 16 + i * 1024;
      w[i][0] = u32x4{0u, 0u, 0u, 0u};
      sb[i][0] = 0u;
      if (k < K) {
        w[i][0] = mx_ld16(qr + k);
        sb[i][0] = sr[k >> 5];
      }
    }
  };
  u32x4 wc[KCH][1], wn[KCH][1];
  uint32_t sc[KCH][1], sn[KCH][1];
#pragma unroll
  for (int i = 0; i < KCH; ++i) {
    wc[i][0] = wn[i][0] = u32x4{0u, 0u, 0u, 0u};
    sc[i][0] = sn[i][0] = 0u;
  }
  float bc = 0.f, bn = 0.f;
  if (wv < nrow) load_row(n0 + wv, wc, sc, bc);
  for (int i = wv; i < nrow; i += 4) {  // wave-uniform
    if (i + 4 < nrow) load_row(n0 + i + 4, wn, sn, bn);
    float acc[1][MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[0][m] = 0.f;
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
      const int64_t k = (int64_t)lane * 16 + c * 1024;
      if (k < K) mx_fma<1, MR>(wc[c], sc[c], M, x + k, ldx, acc);
    }
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      if (m < M) {
        float y = wave_sum(acc[0][m]);
        if constexpr (AD) y = round_bf(round_bf(y) + round_bf(A.sc * wave_sum(bc * tv[m])));  // ad_finish
        if (lane == 0) ys[m][i] = f2bf(y);
      }
    }
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
      wc[c][0] = wn[c][0];
      sc[c][0] = sn[c][0];
    }
    bc = bn;
  }
  __syncthreads();
  if (tid >= 16 * MXG_MAXM) return;  // whole waves leave
  // softcap + statistics: token row m = tid / 16, columns n .. n + 7 of the block's group (softcap.hip's partition)
  const float icap = 1.0f / cap;
  const int m = tid >> 4, l16 = tid & 15;
  const int64_t n = n0 + 8 * l16;
  const int64_t nv = m < M ? N - n : 0;  // >= 8 whole chunk, 1..7 ragged row end, <= 0 none
  float mx = -INFINITY, se = 0.f;
  int am = 0x7fffffff;
  if (nv > 0) {
    bf16_t* p = lg + m * ld + n;
    float v[8];
    if (nv >= 8) {
      unpack8(*reinterpret_cast<const u32x4*>(&ys[m][8 * l16]), v);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = i < nv ? bf2f(ys[m][8 * l16 + i]) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = softcap_bf16_tab<const unsigned short*, true>(v[i], cap, icap, tab);
      if (i < nv && v[i] > mx) { mx = v[i]; am = (int)(n + i); }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < nv) se += __expf(v[i] - mx);
    if (nv >= 8) {
      *reinterpret_cast<u32x4*>(p) = pack8(v);
    } else {
      for (int i = 0; i < nv; ++i) p[i] = f2bf(v[i]);
    }
    if (mx == -INFINITY) se = 0.f;
  }
  float gm = mx;
  gm = fmaxf(gm, mxh_dppf<MXH_X1>(gm));
  gm = fmaxf(gm, mxh_dppf<MXH_X2>(gm));
  gm = fmaxf(gm, mxh_dppf<MXH_HALF_MIRROR>(gm));
  gm = fmaxf(gm, mxh_dppf<MXH_MIRROR>(gm));
  se = (mx == -INFINITY) ? 0.f : se * __expf(mx - gm);
  am = (mx == gm) ? am : 0x7fffffff;
  se += mxh_dppf<MXH_X1>(se);
  am = min(am, mxh_dpp<MXH_X1>(am));
  se += mxh_dppf<MXH_X2>(se);
  am = min(am, mxh_dpp<MXH_X2>(am));
  se += mxh_dppf<MXH_HALF_MIRROR>(se);
  am = min(am, mxh_dpp<MXH_HALF_MIRROR>(am));
  se += mxh_dppf<MXH_MIRROR>(se);
  am = min(am, mxh_dpp<MXH_MIRROR>(am));
  if (l16 == 0 && nv > 0) {
    float* rs = row_stats + (m * ((N + 127) / 128) + n / 128) * 3;
    rs[0] = gm;
    rs[1] = se;
    rs[2] = __int_as_float(am);
  }
}

// ------------------------------------------------------------------------------------------------ scale repack
// out[r][4 t .. 4 t + 3] = the four E8M0 bytes of row r in 128-k tile t (svla_quant_mx_rows: scales[t sld + 4 r])
__global__ void mx_scales_rowmajor_kernel(int64_t rows, int64_t ntile, const uint32_t* __restrict__ in, int64_t sld4,
                                          uint32_t* __restrict__ out, int64_t ldo4) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * ntile) return;
  const int64_t r = idx / ntile, t = idx % ntile;
  out[r * ldo4 + t] = in[t * sld4 + r];
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int svla_mx_scales_rowmajor(int64_t rows, int64_t K, const void* scales, int64_t sld, void* out, int64_t ldo,
                                       void* stream) {
  SVLA_CHECK_ARG(rows >= 1 && K >= 128 && K % 128 == 0, "mx_scales_rowmajor: rows >= 1 and K a positive multiple of "
                 "128 (rows %lld, K %lld)", (long long)rows, (long long)K);
  SVLA_CHECK_ARG(scales && out && ((uintptr_t)scales & 3) == 0 && ((uintptr_t)out & 3) == 0,
                 "mx_scales_rowmajor: scales / out NULL or not 4-B aligned");
  SVLA_CHECK_ARG(sld % 4 == 0 && sld >= 4 * rows && ldo % 4 == 0 && ldo >= K / 32,
                 "mx_scales_rowmajor: sld a multiple of 4 >= 4 rows, ldo a multiple of 4 >= K / 32");
  const int64_t ntile = K / 128, work = rows * ntile;
  hipLaunchKernelGGL(mx_scales_rowmajor_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     rows, ntile, (const uint32_t*)scales, sld / 4, (uint32_t*)out, ldo / 4);
  return svla::check_launch("mx_scales_rowmajor");
}

namespace {

// svla_gemv_mxfp8 (ad == nullptr) and svla_lora_gemv_mxfp8 (ad: T, ldt, the scaling and the validated B segments)
template <bool AD>
int mx_gemv(int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx, const svla_lora_norm2* norm,
            const svla_mxfp8_rows* W, void* c, int64_t ldc, const svla_epilogue* epi, const MxAd& A, void* stream) {
  SVLA_CHECK_ARG(M >= 1 && M <= MXG_MAXM && N >= 1 && K >= 128 && K % 128 == 0,
                 "gemv_mxfp8: M in [1, %d], N >= 1, K a positive multiple of 128 (M %lld, N %lld, K %lld)", MXG_MAXM,
                 (long long)M, (long long)N, (long long)K);
  SVLA_CHECK_ARG(W && c && epi && al16(c), "gemv_mxfp8: NULL argument, or c not 16-B aligned");
  SVLA_CHECK_ARG(ldc % 8 == 0, "gemv_mxfp8: ldc must be a multiple of 8");
  const bool geglu = epi->kind == SVLA_EPI_GEGLU;
  SVLA_CHECK_ARG(geglu || (epi->kind == SVLA_EPI_STORE && !epi->accumulate && epi->alpha == 1.0f),
                 "gemv_mxfp8: epilogue STORE (plain) or GEGLU");
  SVLA_CHECK_ARG(!epi->mx_q, "gemv_mxfp8: the MX copy of C (epi->mx_q) is an fp8-GEMM output only");
  SVLA_CHECK_ARG(W->nseg >= 1 && W->nseg <= MXG_MAXSEG && W->ldq % 16 == 0 && W->ldq >= K && W->lds >= K / 32,
                 "gemv_mxfp8: 1..3 weight segments, ldq a multiple of 16 >= K, lds >= K / 32");
  SVLA_CHECK_ARG(W->start[0] == 0 && W->start[W->nseg] == N, "gemv_mxfp8: segment starts must run from 0 to N");
  MxRows R = {};
  const uint8_t* rq[MXG_MAXSEG] = {nullptr, nullptr, nullptr};
  const uint8_t* rs[MXG_MAXSEG] = {nullptr, nullptr, nullptr};
  int64_t rst[MXG_MAXSEG] = {0, 0, 0};
  for (int i = 0; i < W->nseg; ++i) {
    SVLA_CHECK_ARG(W->q[i] && W->x[i] && al16(W->q[i]), "gemv_mxfp8: segment %d q / exponents NULL or q not 16-B aligned",
                   i);
    SVLA_CHECK_ARG(W->start[i + 1] > W->start[i], "gemv_mxfp8: segment starts must ascend");
    rq[i] = (const uint8_t*)W->q[i];
    rs[i] = (const uint8_t*)W->x[i];
    rst[i] = W->start[i];
  }
  R.q0 = rq[0], R.q1 = rq[1], R.q2 = rq[2];
  R.s0 = rs[0], R.s1 = rs[1], R.s2 = rs[2];
  R.st1 = rst[1], R.st2 = rst[2];
  R.ldq = W->ldq;
  R.lds = W->lds;
  R.nseg = W->nseg;
  MxOut O = {(bf16_t*)c, nullptr, nullptr, ldc, 0, 0};
  if (geglu) {
    SVLA_CHECK_ARG(N % 2 == 0 && W->nseg == 2 && W->start[1] * 2 == N && epi->out1 && epi->out2 &&
                       epi->ld_out1 % 8 == 0 && epi->ld_out2 % 8 == 0,
                   "gemv_mxfp8: GEGLU needs two weight segments of N/2 rows (gate, up) and out1/out2");
    O.g = (bf16_t*)epi->out1;
    O.u = (bf16_t*)epi->out2;
    O.ldg = epi->ld_out1;
    O.ldu = epi->ld_out2;
  }
  const int64_t rows = geglu ? N / 2 : N;
  const int64_t waves = geglu ? rows : (rows + 1) / 2;
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  const int kch = (int)((K + 1023) / 1024);
  hipStream_t s = (hipStream_t)stream;
  if (!AD && norm) {
    SVLA_CHECK_ARG(K <= MXG_NORM_MAX_K, "gemv_mxfp8: the norm prologue holds rows of K <= %d, got %lld", MXG_NORM_MAX_K,
                   (long long)K);
    SVLA_CHECK_ARG(norm->res && norm->y && norm->w1 && norm->w2 && norm->h_out && al16(norm->res) && al16(norm->y) &&
                       al16(norm->w1) && al16(norm->w2) && al16(norm->h_out),
                   "gemv_mxfp8: norm operands NULL or not 16-B aligned");
    SVLA_CHECK_ARG(norm->ld % 8 == 0 && norm->ld >= K, "gemv_mxfp8: the norm rows' ld must be a multiple of 8 >= K");
    MxNorm2 Nn = {(const bf16_t*)norm->res, (const bf16_t*)norm->y, (const bf16_t*)norm->w1, (const bf16_t*)norm->w2,
                  (bf16_t*)norm->h_out, norm->ld, norm->eps1, norm->eps2};
    const size_t lds = (size_t)M * K * 2 + 2 * 4 * sizeof(float);
#define SVLA_MXN1(KC, GG, MR_) \
  hipLaunchKernelGGL((mxg_norm2_kernel<KC, GG, MR_>), grid, block, lds, s, (int)M, rows, K, Nn, R, O)
#define SVLA_MXN(KC)                              \
  do {                                            \
    if (geglu) {                                  \
      if (M == 1) SVLA_MXN1(KC, true, 1);         \
      else SVLA_MXN1(KC, true, MXG_MAXM);         \
    } else {                                      \
      if (M == 1) SVLA_MXN1(KC, false, 1);        \
      else SVLA_MXN1(KC, false, MXG_MAXM);        \
    }                                             \
  } while (0)
    if (kch == 1) SVLA_MXN(1);
    else if (kch == 2) SVLA_MXN(2);
    else SVLA_MXN(3);
#undef SVLA_MXN
#undef SVLA_MXN1
    return svla::check_launch("gemv_mxfp8 (norm prologue)");
  }
  SVLA_CHECK_ARG(x && al16(x) && ldx % 8 == 0 && ldx >= K, "gemv_mxfp8: x NULL or not 16-B aligned, or ldx not a "
                 "multiple of 8 >= K");
  if (!geglu && K > 4096) {  // long K (the down projection): the block-per-row split-K form
    if (M == 1)
      hipLaunchKernelGGL((mxg_splitk_kernel<1, AD>), dim3((unsigned)rows), block, 0, s, (int)M, rows, K,
                         (const bf16_t*)x, ldx, R, (bf16_t*)c, ldc, A);
    else
      hipLaunchKernelGGL((mxg_splitk_kernel<MXG_MAXM, AD>), dim3((unsigned)rows), block, 0, s, (int)M, rows, K,
                         (const bf16_t*)x, ldx, R, (bf16_t*)c, ldc, A);
    return svla::check_launch(AD ? "lora_gemv_mxfp8 (split-K)" : "gemv_mxfp8 (split-K)");
  }
#define SVLA_MXG1(KC, GG, MR_) \
  hipLaunchKernelGGL((mxg_kernel<KC, GG, MR_, AD>), grid, block, 0, s, (int)M, rows, K, (const bf16_t*)x, ldx, R, O, A)
#define SVLA_MXG(KC)                              \
  do {                                            \
    if (geglu) {                                  \
      if (M == 1) SVLA_MXG1(KC, true, 1);         \
      else SVLA_MXG1(KC, true, MXG_MAXM);         \
    } else {                                      \
      if (M == 1) SVLA_MXG1(KC, false, 1);        \
      else SVLA_MXG1(KC, false, MXG_MAXM);        \
    }                                             \
  } while (0)
  if (kch == 1) SVLA_MXG(1);
  else if (kch == 2) SVLA_MXG(2);
  else if (kch == 3) SVLA_MXG(3);
  else if (kch == 4) SVLA_MXG(4);
  else SVLA_MXG(0);
#undef SVLA_MXG
#undef SVLA_MXG1
  return svla::check_launch(AD ? "lora_gemv_mxfp8" : "gemv_mxfp8");
}

}  // namespace

extern "C" int svla_gemv_mxfp8(int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx, const svla_lora_norm2* norm,
                               const svla_mxfp8_rows* W, void* c, int64_t ldc, const svla_epilogue* epi, void* stream) {
  return mx_gemv<false>(M, N, K, x, ldx, norm, W, c, ldc, epi, MxAd{}, stream);
}

extern "C" int svla_lora_gemv_mxfp8(int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx,
                                    const svla_mxfp8_rows* W, const void* t, int64_t ldt, const svla_lora_segs* bsegs,
                                    float scaling, void* c, int64_t ldc, const svla_epilogue* epi, void* stream) {
  SVLA_CHECK_ARG(N >= 16, "lora_gemv_mxfp8: N >= 16, got %lld", (long long)N);
  SVLA_CHECK_ARG(t && al16(t), "lora_gemv_mxfp8: t NULL or not 16-B aligned");
  MxAd A = {(const bf16_t*)t, ldt, {}, scaling};
  const int rc = make_segs("lora_gemv_mxfp8", bsegs, A.S, true, N);
  if (rc != SVLA_OK) return rc;
  SVLA_CHECK_ARG(A.S.ld >= A.S.r, "lora_gemv_mxfp8: the B matrices' ld is below r");
  SVLA_CHECK_ARG(ldt >= (int64_t)(A.S.nseg - 1) * A.S.R + A.S.r,
                 "lora_gemv_mxfp8: ldt must cover (nseg - 1) * R + r columns, got %lld", (long long)ldt);
  SVLA_CHECK_ARG(W && W->nseg == A.S.nseg, "lora_gemv_mxfp8: one B segment per weight segment");
  for (int i = 0; i <= A.S.nseg; ++i)
    SVLA_CHECK_ARG(W->start[i] == A.S.st[i], "lora_gemv_mxfp8: the weight and the B segments must start at the same rows");
  return mx_gemv<true>(M, N, K, x, ldx, nullptr, W, c, ldc, epi, A, stream);
}

namespace {

template <bool AD>
int mx_head(int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx, const void* q, int64_t ldq, const void* xs,
            int64_t lds, float cap, void* logits, int64_t ld, float* row_stats, const MxHeadAd& A, void* stream) {
  SVLA_CHECK_ARG(M >= 1 && M <= MXG_MAXM && N >= 1 && N < (1ll << 31) && K >= 128 && K % 128 == 0 && K <= MXH_MAX_K,
                 "head_gemv_mxfp8: M in [1, %d], N >= 1, K a multiple of 128 in [128, %d] (M %lld, N %lld, K %lld)",
                 MXG_MAXM, MXH_MAX_K, (long long)M, (long long)N, (long long)K);
  SVLA_CHECK_ARG(x && q && xs && logits && row_stats, "head_gemv_mxfp8: NULL argument");
  SVLA_CHECK_ARG(al16(x) && al16(q) && al16(logits), "head_gemv_mxfp8: x / q / logits not 16-B aligned");
  SVLA_CHECK_ARG(ldx % 8 == 0 && ldx >= K && ldq % 16 == 0 && ldq >= K && lds >= K / 32,
                 "head_gemv_mxfp8: ldx a multiple of 8 >= K, ldq a multiple of 16 >= K, lds >= K / 32");
  SVLA_CHECK_ARG(ld % 8 == 0 && ld >= N && cap > 0.f, "head_gemv_mxfp8: ld (multiple of 8 >= N), cap > 0");
  const int kch = (int)((K + 1023) / 1024);
  const dim3 grid((unsigned)((N + MXH_COLS - 1) / MXH_COLS)), block(256);
#define SVLA_MXH1(KC, MR_)                                                                                           \
  hipLaunchKernelGGL((mxh_kernel<KC, MR_, AD>), grid, block, 0, (hipStream_t)stream, (int)M, N, K, (const bf16_t*)x, \
                     ldx, (const uint8_t*)q, ldq, (const uint8_t*)xs, lds, cap, (bf16_t*)logits, ld, row_stats, A)
#define SVLA_MXH(KC)                  \
  do {                                \
    if (M == 1) SVLA_MXH1(KC, 1);     \
    else SVLA_MXH1(KC, MXG_MAXM);     \
  } while (0)
  if (kch <= 1) SVLA_MXH(1);
  else if (kch <= 3) SVLA_MXH(3);
  else SVLA_MXH(4);
#undef SVLA_MXH
#undef SVLA_MXH1
  return svla::check_launch(AD ? "lora_head_gemv_mxfp8" : "head_gemv_mxfp8");
}

}  // namespace

extern "C" int svla_head_gemv_mxfp8(int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx, const void* q,
                                    int64_t ldq, const void* xs, int64_t lds, float cap, void* logits, int64_t ld,
                                    float* row_stats, void* stream) {
  return mx_head<false>(M, N, K, x, ldx, q, ldq, xs, lds, cap, logits, ld, row_stats, MxHeadAd{}, stream);
}

extern "C" int svla_lora_head_gemv_mxfp8(int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx, const void* q,
                                         int64_t ldq, const void* xs, int64_t lds, const void* t, int64_t ldt,
                                         const void* B, int64_t ldb, int32_t r, float scaling, float cap, void* logits,
                                         int64_t ld, float* row_stats, void* stream) {
  SVLA_CHECK_ARG(t && B && al16(t) && al16(B), "lora_head_gemv_mxfp8: t / B NULL or not 16-B aligned");
  SVLA_CHECK_ARG(r >= 8 && r <= MAX_R && r % 8 == 0,
                 "lora_head_gemv_mxfp8: rank must be a multiple of 8 in [8, 64], got %d", (int)r);
  SVLA_CHECK_ARG(ldb % 8 == 0 && ldb >= r && ldt % 8 == 0 && ldt >= r,
                 "lora_head_gemv_mxfp8: ldb, ldt multiples of 8 >= r");
  const MxHeadAd A = {(const bf16_t*)t, (const bf16_t*)B, ldt, ldb, (int)r, scaling};
  return mx_head<true>(M, N, K, x, ldx, q, ldq, xs, lds, cap, logits, ld, row_stats, A, stream);
}
