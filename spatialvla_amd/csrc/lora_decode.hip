// Decode-step (M <= 8 token rows) projections with unmerged LoRA adapters for gfx950 (MI355X): svla_lora_gemv_down,
// svla_lora_gemv and svla_lora_head_gemv (include/svla.h).
//
// A decode step is bound by launch latency, not bytes (a layer streams ~200 MB of base weights next to ~3 MB of
// adapters), so the adapter arithmetic rides inside the GEMVs that stream the base weights instead of the training
// path's projection + svla_lora_down + svla_lora_up triple:
//   svla_lora_gemv_down  T = bf16(x A_s^T) for up to 3 adapters that share x, one wave per rank row (the four waves of
//                        a block split a row at long K), optionally with the Gemma2 norm pair of svla_gemv_rmsnorm2
//                        in its prologue (h and x are then stored for the projection that follows);
//   svla_lora_gemv       y = bf16(bf16(x W^T) + bf16(s T B_s^T)), one wave per output row (or gate|up row pair): the
//                        wave's B row (<= 128 B) and the M r values of T are loaded with its weight prefetch, the
//                        rank-r dot product is one value per lane and a butterfly;
//   svla_lora_head_gemv  the lm_head form of svla_lora_gemv: a block owns 128 consecutive vocabulary rows, keeps their
//                        raw logits in LDS and finishes them with svla_softcap_ce_rows' per-lane unit (softcap, store,
//                        the group's max / sum exp / first argmax), so a decode step's head is T, this, finalize.
// The base dot products keep the chunk map and summation order of gemm.hip's GEMVs (gemv_kernel / gemv_pf_kernel /
// gemv_splitk_kernel / gemv_norm2_kernel) for the same K, so with B = 0 the outputs are those kernels' bits, and the
// rounding points are svla_gemm_bf16 (plain store) followed by svla_lora_up (SLICED).
// fp32 accumulation in a fixed order, 16-B non-temporal weight reads issued before the first FMA, no atomics, no
// block waits for another block, no allocation and no host synchronisation (graph-capturable).
#include "softcap_tab.h"
#include "lora_adapter.h"

namespace {

constexpr int LG_MAXM = 8;
constexpr int GN_MAXC = 2;     // norm chunks per thread (256 threads x 8 elements x 2 >= 2560)
constexpr int NORM_MAX_K = 2560;

struct Norm2 {  // svla_lora_norm2 with typed pointers
  const bf16_t* res;
  const bf16_t* y;
  const bf16_t* w1;
  const bf16_t* w2;
  bf16_t* h_out;
  int64_t ld;
  float eps1, eps2;
};

// weight row n of a W operand with up to 4 outer segments (gemm.hip gemv_row)
__device__ __forceinline__ const bf16_t* w_row(const svla_operand& W, int64_t n) {
  int s = 0;
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (i < W.nseg && n >= W.seg_start[i]) s = i;
  return (const bf16_t*)W.ptr[s] + (n - W.seg_start[s]) * W.ld;
}

// ------------------------------------------------------------------------------------------------ lora_gemv_down
// K <= 2560: one wave per column c = s R + j of T (rank row j of adapter s; columns r..R-1 are written as zero), the
// lane's whole K range of the A row loaded up front.  NORM: the norm pair of gemv_norm2_kernel (rms_add_norm2_kernel's
// chunk map and reduction order, so h and x are bitwise svla_add_rmsnorm2_fwd) computed per block into LDS -- the
// norm inputs are loaded before the A row, the block reductions use raw barriers, so the A stream is in flight while
// the norms run; block 0 also stores h and x.
template <bool NORM, int MR>
__global__ __launch_bounds__(256) void lgd_kernel(int M, int64_t K, bf16_t* __restrict__ x, int64_t ldx, Norm2 Nn,
                                                  Segs S, bf16_t* __restrict__ T, int64_t ldt) {
  constexpr int KCH = NORM_MAX_K / 512;
  constexpr int NR = NORM ? MR : 1;
  extern __shared__ __attribute__((aligned(16))) char lgd_smem[];  // NORM: [M][K] bf16 x, then the reduction slots
  bf16_t* const xs = reinterpret_cast<bf16_t*>(lgd_smem);
  float (*red)[4] = reinterpret_cast<float (*)[4]>(lgd_smem + (size_t)M * K * 2);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int nch = (int)(K >> 3);
  u32x4 yv[NR][GN_MAXC], rv[NR][GN_MAXC], w1v[GN_MAXC], w2v[GN_MAXC];
  if constexpr (NORM) {
#pragma unroll
    for (int cI = 0; cI < GN_MAXC; ++cI) {
      const int ch = t + cI * 256;
      w1v[cI] = w2v[cI] = u32x4{0u, 0u, 0u, 0u};
      if (ch < nch) {
        w1v[cI] = *reinterpret_cast<const u32x4*>(Nn.w1 + ch * 8);
        w2v[cI] = *reinterpret_cast<const u32x4*>(Nn.w2 + ch * 8);
      }
#pragma unroll
      for (int m = 0; m < NR; ++m) {
        yv[m][cI] = rv[m][cI] = u32x4{0u, 0u, 0u, 0u};
        if (m < M && ch < nch) {
          yv[m][cI] = *reinterpret_cast<const u32x4*>(Nn.y + m * Nn.ld + ch * 8);
          rv[m][cI] = *reinterpret_cast<const u32x4*>(Nn.res + m * Nn.ld + ch * 8);
        }
      }
    }
  }
  // the A row of this wave's column
  const int ncol = S.nseg * S.R;
  const int c = blockIdx.x * 4 + wv;
  const int cc = c < ncol ? c : ncol - 1;
  const int s = cc / S.R, j = cc - s * S.R;
  const bool live = c < ncol && j < S.r;
  const bf16_t* ar = seg_p(S, s) + (int64_t)(live ? j : 0) * S.ld;
  u32x4 wt[KCH];
#pragma unroll
  for (int i = 0; i < KCH; ++i) {
    const int64_t k = (int64_t)lane * 8 + i * 512;
    wt[i] = (live && k < K) ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ar + k)) : u32x4{0, 0, 0, 0};
  }
  if constexpr (NORM) {
    auto bsum = [&](float v, int slot) {
      v = wave_sum(v);
      if (lane == 0) red[slot][wv] = v;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      return ((red[slot][0] + red[slot][1]) + red[slot][2]) + red[slot][3];
    };
#pragma unroll
    for (int m = 0; m < NR; ++m) {
      if (m < M) {
        float v[GN_MAXC][8];
        float ss = 0.f;
#pragma unroll
        for (int cI = 0; cI < GN_MAXC; ++cI)
          if (t + cI * 256 < nch) {
            unpack8(yv[m][cI], v[cI]);
#pragma unroll
            for (int q = 0; q < 8; ++q) ss += v[cI][q] * v[cI][q];
          }
        const float rstd1 = rsqrtf(bsum(ss, 0) / (float)K + Nn.eps1);
        float ss2 = 0.f;
#pragma unroll
        for (int cI = 0; cI < GN_MAXC; ++cI) {
          const int ch = t + cI * 256;
          if (ch < nch) {
            float wf[8], r[8];
            unpack8(w1v[cI], wf);
            unpack8(rv[m][cI], r);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              v[cI][q] = round_bf(r[q] + round_bf((v[cI][q] * rstd1) * (1.0f + wf[q])));
              ss2 += v[cI][q] * v[cI][q];
            }
            if (blockIdx.x == 0) *reinterpret_cast<u32x4*>(Nn.h_out + m * Nn.ld + ch * 8) = pack8(v[cI]);
          }
        }
        const float rstd2 = rsqrtf(bsum(ss2, 1) / (float)K + Nn.eps2);
#pragma unroll
        for (int cI = 0; cI < GN_MAXC; ++cI) {
          const int ch = t + cI * 256;
          if (ch < nch) {
            float wf[8], o[8];
            unpack8(w2v[cI], wf);
#pragma unroll
            for (int q = 0; q < 8; ++q) o[q] = (v[cI][q] * rstd2) * (1.0f + wf[q]);
            const u32x4 ov = pack8(o);
            *reinterpret_cast<u32x4*>(xs + m * K + ch * 8) = ov;
            if (blockIdx.x == 0) *reinterpret_cast<u32x4*>(x + m * ldx + ch * 8) = ov;
          }
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  if (c >= ncol) return;
  float acc[LG_MAXM];
#pragma unroll
  for (int m = 0; m < LG_MAXM; ++m) acc[m] = 0.f;
  if (live) {
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int64_t k = (int64_t)lane * 8 + i * 512;
      if (k < K) {
        float wf[8];
        unpack8(wt[i], wf);
#pragma unroll
        for (int m = 0; m < LG_MAXM; ++m) {
          if (m < M) {
            float xf[8];
            if constexpr (NORM) unpack8(*reinterpret_cast<const u32x4*>(xs + m * K + k), xf);
            else unpack8(*reinterpret_cast<const u32x4*>(x + m * ldx + k), xf);
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[m] = fmaf(wf[q], xf[q], acc[m]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < LG_MAXM; ++m) {
    if (m < M) {
      const float v = wave_sum(acc[m]);
      if (lane == 0) T[m * ldt + c] = live ? f2bf(v) : (bf16_t)0;
    }
  }
}

// Long K (the down projection's adapter, K = 9216): one block per column of T, its four waves split the row's K range
// as gemv_splitk_kernel does, partial dots summed through LDS in wave order.
__global__ __launch_bounds__(256) void lgd_split_kernel(int M, int64_t K, const bf16_t* __restrict__ x, int64_t ldx,
                                                        Segs S, bf16_t* __restrict__ T, int64_t ldt) {
  __shared__ float part[4][LG_MAXM];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x;  // grid = nseg R exactly
  const int s = c / S.R, j = c - s * S.R;
  if (j >= S.r) {  // block-uniform
    if (threadIdx.x < M) T[threadIdx.x * ldt + c] = 0;
    return;
  }
  const bf16_t* ar = seg_p(S, s) + (int64_t)j * S.ld;
  float acc[LG_MAXM];
#pragma unroll
  for (int m = 0; m < LG_MAXM; ++m) acc[m] = 0.f;
  if (K <= 5 * 2048) {
    constexpr int KCH = 5;
    u32x4 wv[KCH];
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int64_t k = (int64_t)threadIdx.x * 8 + i * 2048;
      wv[i] = k < K ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ar + k)) : u32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int64_t k = (int64_t)threadIdx.x * 8 + i * 2048;
      if (k < K) {
        float wf[8];
        unpack8(wv[i], wf);
#pragma unroll
        for (int m = 0; m < LG_MAXM; ++m) {
          if (m < M) {
            float xf[8];
            unpack8(*reinterpret_cast<const u32x4*>(x + m * ldx + k), xf);
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[m] = fmaf(wf[q], xf[q], acc[m]);
          }
        }
      }
    }
  } else {
#pragma unroll 4
    for (int64_t k = (int64_t)threadIdx.x * 8; k < K; k += 2048) {
      float wf[8];
      unpack8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ar + k)), wf);
#pragma unroll
      for (int m = 0; m < LG_MAXM; ++m) {
        if (m < M) {
          float xf[8];
          unpack8(*reinterpret_cast<const u32x4*>(x + m * ldx + k), xf);
#pragma unroll
          for (int q = 0; q < 8; ++q) acc[m] = fmaf(wf[q], xf[q], acc[m]);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < LG_MAXM; ++m) {
    if (m < M) {
      const float v = wave_sum(acc[m]);
      if (lane == 0) part[w][m] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < M) {
    const int m = threadIdx.x;
    T[m * ldt + c] = f2bf(((part[0][m] + part[1][m]) + part[2][m]) + part[3][m]);
  }
}

// ------------------------------------------------------------------------------------------------ lora_gemv
// The adapter operands of one output row (AdRow, ad_load, ad_finish) are lora_adapter.h's.
struct LgOut {
  bf16_t* c;
  bf16_t* g;
  bf16_t* u;
  int64_t ldc, ldg, ldu;
};

// One wave per output row (GEGLU: per gate|up row pair).  KCH > 0: the lane's whole K range (K <= KCH * 512) loaded
// before the first FMA (gemv_pf_kernel); KCH == 0: the runtime loop of gemv_kernel for every other K.  MR: token rows
// held in registers (1 for the batch-1 decode step: fewer registers, more waves streaming weights per CU).
template <int KCH, bool GEGLU, int MR>
__global__ __launch_bounds__(256) void lg_kernel(int M, int64_t rows, int64_t K, const bf16_t* __restrict__ x,
                                                 int64_t ldx, svla_operand W, const bf16_t* __restrict__ T, int64_t ldt,
                                                 Segs S, float sc, LgOut O) {
  constexpr int NW = GEGLU ? 2 : 1;
  constexpr int NCH = KCH > 0 ? KCH : 1;
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= rows) return;
  AdRow<MR> ad[NW];
  const bf16_t* wr[NW];
  if constexpr (GEGLU) {
    ad_load(ad[0], S, 0, n, T, ldt, M, lane);
    ad_load(ad[NW - 1], S, 1, n, T, ldt, M, lane);
    wr[0] = (const bf16_t*)W.ptr[0] + n * W.ld;
    wr[NW - 1] = (const bf16_t*)W.ptr[1] + n * W.ld;
  } else {
    const int s = seg_of(S, n);
    ad_load(ad[0], S, s, n - seg_st(S, s), T, ldt, M, lane);
    wr[0] = w_row(W, n);
  }
  float acc[NW][MR];
#pragma unroll
  for (int q = 0; q < NW; ++q)
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[q][m] = 0.f;
  if constexpr (KCH > 0) {
    u32x4 wv[NW][NCH];
#pragma unroll
    for (int q = 0; q < NW; ++q)
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int64_t k = (int64_t)lane * 8 + i * 512;
        wv[q][i] = k < K ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wr[q] + k)) : u32x4{0, 0, 0, 0};
      }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int64_t k = (int64_t)lane * 8 + i * 512;
      if (k < K) {
        float wf[NW][8];
#pragma unroll
        for (int q = 0; q < NW; ++q) unpack8(wv[q][i], wf[q]);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          if (m < M) {
            float xf[8];
            unpack8(*reinterpret_cast<const u32x4*>(x + m * ldx + k), xf);
#pragma unroll
            for (int q = 0; q < NW; ++q)
#pragma unroll
              for (int e = 0; e < 8; ++e) acc[q][m] = fmaf(wf[q][e], xf[e], acc[q][m]);
          }
        }
      }
    }
  } else {
#pragma unroll 4
    for (int64_t k = (int64_t)lane * 8; k < K; k += 512) {
      float wf[NW][8];
#pragma unroll
      for (int q = 0; q < NW; ++q) unpack8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wr[q] + k)), wf[q]);
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        if (m < M) {
          float xf[8];
          unpack8(*reinterpret_cast<const u32x4*>(x + m * ldx + k), xf);
#pragma unroll
          for (int q = 0; q < NW; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[q][m] = fmaf(wf[q][e], xf[e], acc[q][m]);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    if (m < M) {
      float v[NW];
#pragma unroll
      for (int q = 0; q < NW; ++q) v[q] = ad_finish(ad[q], m, wave_sum(acc[q][m]), sc);
      if (lane == 0) {
        if constexpr (GEGLU) {  // SVLA_EPI_GEGLU's element formula on the adapted g, u
          O.c[m * O.ldc + n] = f2bf(gelu_bf16(v[0]) * v[1]);
          O.g[m * O.ldg + n] = f2bf(v[0]);
          O.u[m * O.ldu + n] = f2bf(v[NW - 1]);
        } else {
          O.c[m * O.ldc + n] = f2bf(v[0]);
        }
      }
    }
  }
}

// Long-K STORE form (K > 4096: the down projection): one block per output row, its four waves split the K range
// (gemv_splitk_kernel's chunk map and LDS sum order); wave 0 also carries the adapter term.
__global__ __launch_bounds__(256) void lg_split_kernel(int M, int64_t rows, int64_t K, const bf16_t* __restrict__ x,
                                                       int64_t ldx, svla_operand W, const bf16_t* __restrict__ T,
                                                       int64_t ldt, Segs S, float sc, LgOut O) {
  __shared__ float part[4][LG_MAXM];
  __shared__ float lpart[LG_MAXM];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t n = blockIdx.x;  // grid = rows exactly
  AdRow<LG_MAXM> ad;
  if (w == 0) {
    const int s = seg_of(S, n);
    ad_load(ad, S, s, n - seg_st(S, s), T, ldt, M, lane);
  }
  const bf16_t* wr = w_row(W, n);
  float acc[LG_MAXM];
#pragma unroll
  for (int m = 0; m < LG_MAXM; ++m) acc[m] = 0.f;
  if (K <= 5 * 2048) {
    constexpr int KCH = 5;
    u32x4 wv[KCH];
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int64_t k = (int64_t)threadIdx.x * 8 + i * 2048;
      wv[i] = k < K ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wr + k)) : u32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int64_t k = (int64_t)threadIdx.x * 8 + i * 2048;
      if (k < K) {
        float wf[8];
        unpack8(wv[i], wf);
#pragma unroll
        for (int m = 0; m < LG_MAXM; ++m) {
          if (m < M) {
            float xf[8];
            unpack8(*reinterpret_cast<const u32x4*>(x + m * ldx + k), xf);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[m] = fmaf(wf[e], xf[e], acc[m]);
          }
        }
      }
    }
  } else {
#pragma unroll 4
    for (int64_t k = (int64_t)threadIdx.x * 8; k < K; k += 2048) {
      float wf[8];
      unpack8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wr + k)), wf);
#pragma unroll
      for (int m = 0; m < LG_MAXM; ++m) {
        if (m < M) {
          float xf[8];
          unpack8(*reinterpret_cast<const u32x4*>(x + m * ldx + k), xf);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[m] = fmaf(wf[e], xf[e], acc[m]);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < LG_MAXM; ++m) {
    if (m < M) {
      const float v = wave_sum(acc[m]);
      if (lane == 0) part[w][m] = v;
      if (w == 0) {  // wave-uniform
        const float l = wave_sum(ad.b * ad.t[m]);
        if (lane == 0) lpart[m] = l;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < M) {
    const int m = threadIdx.x;
    const float base = ((part[0][m] + part[1][m]) + part[2][m]) + part[3][m];
    O.c[m * O.ldc + n] = f2bf(round_bf(round_bf(base) + round_bf(sc * lpart[m])));
  }
}

// ------------------------------------------------------------------------------------------------ lora_head_gemv
// A block owns LH_COLS = 128 consecutive output rows n (vocabulary entries): one statistics group of
// svla_softcap_ce_rows.  Wave w walks rows w, w + 4, ... of the block with lg_kernel's per-row dot product (the lane's
// chunks k = 8 lane + 512 i in order, then the wave butterfly; KCH covers K, chunks at or beyond K are skipped, so the
// order is that of lg_kernel's KCH = 4 / 5 / loop forms for the same K), the next row's weights and B row in flight
// while this one is summed; lane 0 leaves y = bf16(bf16(base) + bf16(s T B)) in LDS.  Then 16 lanes per token row run
// the per-element unit of softcap.hip (8 columns per lane in scan order, the 16-lane DPP butterfly of its group
// combine) on the block's [M][128] raw values: logits and statistics are svla_softcap_ce_rows' bits on y.
constexpr int LH_COLS = 128;
constexpr int LH_MAX_K = 4096;

template <int CTRL>
__device__ __forceinline__ int lh_dpp(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float lh_dppf(float x) {
  return __int_as_float(lh_dpp<CTRL>(__float_as_int(x)));
}
constexpr int LH_X1 = 0xb1, LH_X2 = 0x4e, LH_HALF_MIRROR = 0x141, LH_MIRROR = 0x140;  // softcap.hip's group butterfly

template <int KCH, int MR>
__global__ __launch_bounds__(256) void lh_kernel(int M, int64_t N, int64_t K, const bf16_t* __restrict__ x, int64_t ldx,
                                                 const bf16_t* __restrict__ W, int64_t ldw,
                                                 const bf16_t* __restrict__ T, int64_t ldt,
                                                 const bf16_t* __restrict__ B, int64_t ldb, int r, float sc, float cap,
                                                 bf16_t* __restrict__ lg, int64_t ld, float* __restrict__ row_stats) {
  __shared__ __attribute__((aligned(16))) unsigned short tab[TANH_TAB_BYTES / 2 + 8];
  __shared__ __attribute__((aligned(16))) bf16_t ys[LG_MAXM][LH_COLS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < TANH_TAB_BYTES / 16)
    reinterpret_cast<u32x4*>(tab)[tid] = reinterpret_cast<const u32x4*>(svla_tanh_bf16_tab)[tid];
  const int64_t n0 = (int64_t)blockIdx.x * LH_COLS;
  const int nrow = (int)(N - n0 < LH_COLS ? N - n0 : LH_COLS);
  const bool on = lane < r;
  float tv[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) tv[m] = (on && m < M) ? bf2f(T[m * ldt + lane]) : 0.f;
  auto load_row = [&](int64_t n, u32x4 (&w)[KCH], float& b) {
    const bf16_t* wr = W + n * ldw;
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int64_t k = (int64_t)lane * 8 + i * 512;
      w[i] = k < K ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wr + k)) : u32x4{0, 0, 0, 0};
    }
    b = on ? bf2f(B[n * ldb + lane]) : 0.f;
  };
  u32x4 wc[KCH], wn[KCH];
  float bc = 0.f, bn = 0.f;
  if (wv < nrow) load_row(n0 + wv, wc, bc);
  for (int i = wv; i < nrow; i += 4) {  // wave-uniform
    if (i + 4 < nrow) load_row(n0 + i + 4, wn, bn);
    float acc[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[m] = 0.f;
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
      const int64_t k = (int64_t)lane * 8 + c * 512;
      if (k < K) {
        float wf[8];
        unpack8(wc[c], wf);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          if (m < M) {
            float xf[8];
            unpack8(*reinterpret_cast<const u32x4*>(x + m * ldx + k), xf);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[m] = fmaf(wf[e], xf[e], acc[m]);
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      if (m < M) {
        const float base = wave_sum(acc[m]);
        const float l = wave_sum(bc * tv[m]);
        const float y = round_bf(round_bf(base) + round_bf(sc * l));  // ad_finish
        if (lane == 0) ys[m][i] = f2bf(y);
      }
    }
#pragma unroll
    for (int c = 0; c < KCH; ++c) wc[c] = wn[c];
    bc = bn;
  }
  __syncthreads();
  if (tid >= 16 * LG_MAXM) return;  // whole waves leave
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
  gm = fmaxf(gm, lh_dppf<LH_X1>(gm));
  gm = fmaxf(gm, lh_dppf<LH_X2>(gm));
  gm = fmaxf(gm, lh_dppf<LH_HALF_MIRROR>(gm));
  gm = fmaxf(gm, lh_dppf<LH_MIRROR>(gm));
  se = (mx == -INFINITY) ? 0.f : se * __expf(mx - gm);
  am = (mx == gm) ? am : 0x7fffffff;
  se += lh_dppf<LH_X1>(se);
  am = min(am, lh_dpp<LH_X1>(am));
  se += lh_dppf<LH_X2>(se);
  am = min(am, lh_dpp<LH_X2>(am));
  se += lh_dppf<LH_HALF_MIRROR>(se);
  am = min(am, lh_dpp<LH_HALF_MIRROR>(am));
  se += lh_dppf<LH_MIRROR>(se);
  am = min(am, lh_dpp<LH_MIRROR>(am));
  if (l16 == 0 && nv > 0) {
    float* rs = row_stats + (m * ((N + 127) / 128) + n / 128) * 3;
    rs[0] = gm;
    rs[1] = se;
    rs[2] = __int_as_float(am);
  }
}

}  // namespace

extern "C" int svla_lora_gemv_down(int64_t M, int64_t K, void* x, int64_t ldx, const svla_lora_norm2* norm,
                                   const svla_lora_segs* segs, void* t, int64_t ldt, void* stream) {
  SVLA_CHECK_ARG(M >= 1 && M <= LG_MAXM && K >= 8 && K % 8 == 0,
                 "lora_gemv_down: M in [1, %d] and K a positive multiple of 8 (M %lld, K %lld)", LG_MAXM, (long long)M,
                 (long long)K);
  SVLA_CHECK_ARG(x && t && aligned16(x) && aligned16(t), "lora_gemv_down: x / t NULL or not 16-B aligned");
  SVLA_CHECK_ARG(ldx % 8 == 0 && ldx >= K, "lora_gemv_down: ldx must be a multiple of 8 and >= K, got %lld",
                 (long long)ldx);
  Segs S;
  const int rc = make_segs("lora_gemv_down", segs, S, false, 0);
  if (rc != SVLA_OK) return rc;
  SVLA_CHECK_ARG(S.ld >= K, "lora_gemv_down: the A matrices' ld is below K");
  SVLA_CHECK_ARG(ldt % 8 == 0 && ldt >= (int64_t)S.nseg * S.R,
                 "lora_gemv_down: ldt must be a multiple of 8 and >= nseg * R = %d", S.nseg * S.R);
  hipStream_t s = (hipStream_t)stream;
  const int ncol = S.nseg * S.R;
  Norm2 Nn = {};
  if (norm) {
    SVLA_CHECK_ARG(K <= NORM_MAX_K, "lora_gemv_down: the norm prologue holds rows of K <= %d, got %lld", NORM_MAX_K,
                   (long long)K);
    SVLA_CHECK_ARG(norm->res && norm->y && norm->w1 && norm->w2 && norm->h_out && aligned16(norm->res) &&
                       aligned16(norm->y) && aligned16(norm->w1) && aligned16(norm->w2) && aligned16(norm->h_out),
                   "lora_gemv_down: norm operands NULL or not 16-B aligned");
    SVLA_CHECK_ARG(norm->ld % 8 == 0 && norm->ld >= K, "lora_gemv_down: the norm rows' ld must be a multiple of 8 >= K");
    Nn.res = (const bf16_t*)norm->res;
    Nn.y = (const bf16_t*)norm->y;
    Nn.w1 = (const bf16_t*)norm->w1;
    Nn.w2 = (const bf16_t*)norm->w2;
    Nn.h_out = (bf16_t*)norm->h_out;
    Nn.ld = norm->ld;
    Nn.eps1 = norm->eps1;
    Nn.eps2 = norm->eps2;
    const size_t lds = (size_t)M * K * 2 + 2 * 4 * sizeof(float);
    const dim3 grid((unsigned)((ncol + 3) / 4)), block(256);
    if (M == 1)
      hipLaunchKernelGGL((lgd_kernel<true, 1>), grid, block, lds, s, (int)M, K, (bf16_t*)x, ldx, Nn, S, (bf16_t*)t, ldt);
    else
      hipLaunchKernelGGL((lgd_kernel<true, LG_MAXM>), grid, block, lds, s, (int)M, K, (bf16_t*)x, ldx, Nn, S,
                         (bf16_t*)t, ldt);
  } else if (K <= NORM_MAX_K) {
    hipLaunchKernelGGL((lgd_kernel<false, 1>), dim3((unsigned)((ncol + 3) / 4)), dim3(256), 0, s, (int)M, K, (bf16_t*)x,
                       ldx, Nn, S, (bf16_t*)t, ldt);
  } else {
    hipLaunchKernelGGL(lgd_split_kernel, dim3((unsigned)ncol), dim3(256), 0, s, (int)M, K, (const bf16_t*)x, ldx, S,
                       (bf16_t*)t, ldt);
  }
  return svla::check_launch("lora_gemv_down");
}

extern "C" int svla_lora_gemv(int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx, const svla_operand* W,
                              const void* t, int64_t ldt, const svla_lora_segs* bsegs, float scaling, void* c,
                              int64_t ldc, const svla_epilogue* epi, void* stream) {
  SVLA_CHECK_ARG(M >= 1 && M <= LG_MAXM && N >= 16 && K >= 8 && K % 8 == 0,
                 "lora_gemv: M in [1, %d], N >= 16, K a positive multiple of 8 (M %lld, N %lld, K %lld)", LG_MAXM,
                 (long long)M, (long long)N, (long long)K);
  SVLA_CHECK_ARG(x && t && c && W && epi, "lora_gemv: NULL argument");
  SVLA_CHECK_ARG(aligned16(x) && aligned16(t) && aligned16(c), "lora_gemv: x / t / c not 16-B aligned");
  SVLA_CHECK_ARG(ldx % 8 == 0 && ldx >= K && ldc % 8 == 0, "lora_gemv: ldx >= K and ldc multiples of 8");
  const bool geglu = epi->kind == SVLA_EPI_GEGLU;
  SVLA_CHECK_ARG(geglu || (epi->kind == SVLA_EPI_STORE && !epi->accumulate && epi->alpha == 1.0f),
                 "lora_gemv: epilogue STORE (plain) or GEGLU");
  SVLA_CHECK_ARG(!epi->mx_q, "lora_gemv: the MX copy of C (epi->mx_q) is an fp8-GEMM output only");
  SVLA_CHECK_ARG(W->layout == SVLA_LAYOUT_KC && W->ld % 8 == 0 && W->ld >= K && W->nseg >= 1 && W->nseg <= 4,
                 "lora_gemv: W must be KC with ld % 8 == 0, ld >= K and 1..4 segments");
  for (int i = 0; i < W->nseg; ++i) {
    SVLA_CHECK_ARG(W->ptr[i] && aligned16(W->ptr[i]), "lora_gemv: W segment %d NULL or not 16-B aligned", i);
    SVLA_CHECK_ARG(i == 0 ? W->seg_start[0] == 0 : (W->seg_start[i] > W->seg_start[i - 1] && W->seg_start[i] < N),
                   "lora_gemv: W segment starts must ascend from 0 below N");
  }
  Segs S;
  const int rc = make_segs("lora_gemv", bsegs, S, true, N);
  if (rc != SVLA_OK) return rc;
  SVLA_CHECK_ARG(S.ld >= S.r, "lora_gemv: the B matrices' ld is below r");
  SVLA_CHECK_ARG(ldt >= (int64_t)(S.nseg - 1) * S.R + S.r, "lora_gemv: ldt must cover (nseg - 1) * R + r columns, got %lld",
                 (long long)ldt);
  LgOut O = {(bf16_t*)c, nullptr, nullptr, ldc, 0, 0};
  if (geglu) {
    SVLA_CHECK_ARG(N % 2 == 0 && W->nseg == 2 && W->seg_dim == SVLA_SEG_GEGLU && W->seg_start[1] * 2 == N &&
                       S.nseg == 2 && S.st[1] * 2 == N && epi->out1 && epi->out2 && epi->ld_out1 % 8 == 0 &&
                       epi->ld_out2 % 8 == 0,
                   "lora_gemv: GEGLU needs two W and two B segments of N/2 rows and out1/out2");
    O.g = (bf16_t*)epi->out1;
    O.u = (bf16_t*)epi->out2;
    O.ldg = epi->ld_out1;
    O.ldu = epi->ld_out2;
  } else {
    SVLA_CHECK_ARG(W->nseg == 1 || W->seg_dim == SVLA_SEG_OUTER, "lora_gemv: STORE takes outer W segments");
  }
  const int64_t rows = geglu ? N / 2 : N;
  const int kch = (int)((K + 511) / 512);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define SVLA_LG1(KC, GG, MR_)                                                                                        \
  hipLaunchKernelGGL((lg_kernel<KC, GG, MR_>), grid, block, 0, s, (int)M, rows, K, (const bf16_t*)x, ldx, *W,        \
                     (const bf16_t*)t, ldt, S, scaling, O)
#define SVLA_LG(KC, GG)                  \
  do {                                   \
    if (M == 1) SVLA_LG1(KC, GG, 1);     \
    else SVLA_LG1(KC, GG, LG_MAXM);      \
  } while (0)
  // the K ranges of gemm.hip's small-M dispatch (the same summation order for the same K)
  if (geglu) {
    if (kch == 4) SVLA_LG(4, true);
    else if (kch == 5) SVLA_LG(5, true);
    else SVLA_LG(0, true);
  } else if (kch == 4) {
    SVLA_LG(4, false);
  } else if (kch == 5) {
    SVLA_LG(5, false);
  } else if (K > 4096) {
    hipLaunchKernelGGL(lg_split_kernel, dim3((unsigned)rows), block, 0, s, (int)M, rows, K, (const bf16_t*)x, ldx, *W,
                       (const bf16_t*)t, ldt, S, scaling, O);
  } else {
    SVLA_LG(0, false);
  }
#undef SVLA_LG
#undef SVLA_LG1
  return svla::check_launch("lora_gemv");
}

extern "C" int svla_lora_head_gemv(int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx, const void* W,
                                   int64_t ldw, const void* t, int64_t ldt, const void* B, int64_t ldb, int32_t r,
                                   float scaling, float cap, void* logits, int64_t ld, float* row_stats, void* stream) {
  SVLA_CHECK_ARG(M >= 1 && M <= LG_MAXM && N >= 1 && N < (1ll << 31) && K >= 8 && K % 8 == 0 && K <= LH_MAX_K,
                 "lora_head_gemv: M in [1, %d], N >= 1, K a multiple of 8 in [8, %d] (M %lld, N %lld, K %lld)", LG_MAXM,
                 LH_MAX_K, (long long)M, (long long)N, (long long)K);
  SVLA_CHECK_ARG(x && W && t && B && logits && row_stats, "lora_head_gemv: NULL argument");
  SVLA_CHECK_ARG(aligned16(x) && aligned16(W) && aligned16(t) && aligned16(B) && aligned16(logits),
                 "lora_head_gemv: x / W / t / B / logits not 16-B aligned");
  SVLA_CHECK_ARG(r >= 8 && r <= MAX_R && r % 8 == 0, "lora_head_gemv: rank must be a multiple of 8 in [8, 64], got %d",
                 (int)r);
  SVLA_CHECK_ARG(ldx % 8 == 0 && ldx >= K && ldw % 8 == 0 && ldw >= K, "lora_head_gemv: ldx, ldw multiples of 8 >= K");
  SVLA_CHECK_ARG(ldb % 8 == 0 && ldb >= r && ldt % 8 == 0 && ldt >= r, "lora_head_gemv: ldb, ldt multiples of 8 >= r");
  SVLA_CHECK_ARG(ld % 8 == 0 && ld >= N && cap > 0.f, "lora_head_gemv: ld (multiple of 8 >= N), cap > 0");
  const int kch = (int)((K + 511) / 512);
  const dim3 grid((unsigned)((N + LH_COLS - 1) / LH_COLS)), block(256);
#define SVLA_LH1(KC, MR_)                                                                                             \
  hipLaunchKernelGGL((lh_kernel<KC, MR_>), grid, block, 0, (hipStream_t)stream, (int)M, N, K, (const bf16_t*)x, ldx,  \
                     (const bf16_t*)W, ldw, (const bf16_t*)t, ldt, (const bf16_t*)B, ldb, (int)r, scaling, cap,       \
                     (bf16_t*)logits, ld, row_stats)
#define SVLA_LH(KC)                  \
  do {                               \
    if (M == 1) SVLA_LH1(KC, 1);     \
    else SVLA_LH1(KC, LG_MAXM);      \
  } while (0)
  if (kch <= 1) SVLA_LH(1);
  else if (kch <= 5) SVLA_LH(5);
  else SVLA_LH(8);
#undef SVLA_LH
#undef SVLA_LH1
  return svla::check_launch("lora_head_gemv");
}
