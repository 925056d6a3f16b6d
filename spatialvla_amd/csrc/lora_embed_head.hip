// LoRA adapters on both ends of the action-token path, gfx950 (MI355X): the peft Embedding adapter on
// spatial_embed_tokens and the peft Linear adapter on lm_head of the reference's lora_target = "linear+emb" /
// "linear+emb+h" (train/spatialvla_finetune.py:272-286) -- svla_lora_embed_fwd, svla_lora_embed_decode,
// svla_lora_embed_bwd, svla_lora_softcap_ce_rows (include/svla.h).  fp32 accumulation in a fixed order, no atomics, no block waits on
// another, no allocation or host sync, bitwise stable run to run.
//
// The embedding kernels touch the few hundred action-token rows of a batch only (one block per row / per table id);
// they are latency bound and kept plain.  The head pass is the hot one: it streams the raw logits [M][ld] once.  A
// block owns one 512-column chunk and keeps that chunk's B rows in LDS as bf16 pairs along j (lora_softcap_rows_kernel
// documents the layout); its four waves then walk rows of the chunk, T[m, :] wave-uniform, the term as packed bf16 dot
// products (v_dot2c_f32_bf16).  B (17 MB at V = 265347, r = 32) is read once per row slice of the grid, never copied or
// padded.
#include "softcap_tab.h"

#include <algorithm>

namespace {

constexpr int EH_MAXR = 64;

// ------------------------------------------------------------------ embedding forward
__global__ __launch_bounds__(256) void lora_embed_fwd_kernel(int64_t H, const int64_t* __restrict__ ids,
                                                             const int32_t* __restrict__ img_index,
                                                             const bf16_t* __restrict__ embed,
                                                             const bf16_t* __restrict__ spatial, int64_t a0, int64_t na,
                                                             const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
                                                             int r, float s, float normalizer, bf16_t* __restrict__ out) {
  const int64_t row = blockIdx.x;
  const int64_t id = ids[row];
  if (id < a0 || id >= a0 + na) return;  // block-uniform
  if (img_index && img_index[row] >= 0) return;
  const int64_t sid = id - a0;
  __shared__ float a[EH_MAXR];
  if ((int)threadIdx.x < r) a[threadIdx.x] = bf2f(A[(int64_t)threadIdx.x * na + sid]);
  __syncthreads();
  for (int64_t ch = threadIdx.x; ch < (H >> 3); ch += blockDim.x) {
    float e[8], v[8];
    unpack8(*reinterpret_cast<const u32x4*>(embed + id * H + ch * 8), e);
    unpack8(*reinterpret_cast<const u32x4*>(spatial + sid * H + ch * 8), v);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bf16_t* brow = B + (ch * 8 + i) * r;  // r % 8 == 0: 16-B pieces
      float acc = 0.f;
      for (int j0 = 0; j0 < r; j0 += 8) {
        float b[8];
        unpack8(*reinterpret_cast<const u32x4*>(brow + j0), b);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += a[j0 + j] * b[j];
      }
      const float base = round_bf(round_bf(e[i] * 0.0f) + v[i]);  // svla_embed_merge's value of the row
      v[i] = round_bf(base + round_bf(s * acc)) * normalizer;
    }
    *reinterpret_cast<u32x4*>(out + row * H + ch * 8) = pack8(v);
  }
}

// ------------------------------------------------------------------ embedding forward, decode step
// svla_embed_merge (no image slot) and lora_embed_fwd_kernel in one launch for the few token rows of a decode step:
// a text id takes the merge kernel's expression, an action-token id the kernel's above, operand for operand, so the
// row is bitwise what the two launches leave.
__global__ __launch_bounds__(256) void lora_embed_decode_kernel(int64_t H, const int64_t* __restrict__ ids,
                                                                const bf16_t* __restrict__ embed,
                                                                const bf16_t* __restrict__ spatial, int64_t a0,
                                                                int64_t na, const bf16_t* __restrict__ A,
                                                                const bf16_t* __restrict__ B, int r, float s,
                                                                float normalizer, bf16_t* __restrict__ out) {
  const int64_t row = blockIdx.x;
  const int64_t id = ids[row];
  if (id < a0 || id >= a0 + na) {  // block-uniform: embed_merge_kernel's text row
    for (int64_t ch = threadIdx.x; ch < (H >> 3); ch += blockDim.x) {
      float v[8];
      unpack8(*reinterpret_cast<const u32x4*>(embed + id * H + ch * 8), v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = round_bf(v[j]) * normalizer;
      *reinterpret_cast<u32x4*>(out + row * H + ch * 8) = pack8(v);
    }
    return;
  }
  const int64_t sid = id - a0;
  __shared__ float a[EH_MAXR];
  if ((int)threadIdx.x < r) a[threadIdx.x] = bf2f(A[(int64_t)threadIdx.x * na + sid]);
  __syncthreads();
  for (int64_t ch = threadIdx.x; ch < (H >> 3); ch += blockDim.x) {
    float e[8], v[8];
    unpack8(*reinterpret_cast<const u32x4*>(embed + id * H + ch * 8), e);
    unpack8(*reinterpret_cast<const u32x4*>(spatial + sid * H + ch * 8), v);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bf16_t* brow = B + (ch * 8 + i) * r;
      float acc = 0.f;
      for (int j0 = 0; j0 < r; j0 += 8) {
        float b[8];
        unpack8(*reinterpret_cast<const u32x4*>(brow + j0), b);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += a[j0 + j] * b[j];
      }
      const float base = round_bf(round_bf(e[i] * 0.0f) + v[i]);
      v[i] = round_bf(base + round_bf(s * acc)) * normalizer;
    }
    *reinterpret_cast<u32x4*>(out + row * H + ch * 8) = pack8(v);
  }
}

// ------------------------------------------------------------------ embedding backward
// dA[:, id]: one block per table id.  Thread t < nsl * r owns (j = t % r, slice = t / r) and sums G[h] B[h, j] over
// h = slice, slice + nsl, ... with G[h] = sum over the id's rows (CSR order) of g[row, h]; the slices are summed in
// slice order by the first r threads.
__global__ __launch_bounds__(256) void lora_embed_da_kernel(int64_t H, int64_t na, const int32_t* __restrict__ sorted_rows,
                                                            const int32_t* __restrict__ offsets,
                                                            const bf16_t* __restrict__ dout, float normalizer,
                                                            const bf16_t* __restrict__ B, int r, float s,
                                                            bf16_t* __restrict__ dA, int accumulate) {
  const int64_t sid = blockIdx.x;
  const int b = offsets[sid], e = offsets[sid + 1];
  const int t = threadIdx.x;
  if (b >= e) {  // block-uniform: the id does not occur
    if (t < r && !accumulate) dA[(int64_t)t * na + sid] = 0;
    return;
  }
  __shared__ float red[256];
  const int nsl = 256 / r;
  float acc = 0.f;
  if (t < nsl * r) {
    const int j = t % r, sl = t / r;
    for (int64_t h = sl; h < H; h += nsl) {
      float G = 0.f;
      for (int i = b; i < e; ++i) G += round_bf(bf2f(dout[(int64_t)sorted_rows[i] * H + h]) * normalizer);
      acc += G * bf2f(B[h * r + j]);
    }
  }
  red[t] = acc;
  __syncthreads();
  if (t < r) {
    float sum = 0.f;
    for (int sl = 0; sl < nsl; ++sl) sum += red[sl * r + t];
    const int64_t o = (int64_t)t * na + sid;
    const float val = s * sum;
    dA[o] = f2bf(accumulate ? bf2f(dA[o]) + round_bf(val) : val);
  }
}

// dB[h, :]: a block owns 64 consecutive h; wave w owns j = w, w + 4, ...  The spatial rows are walked in CSR order in
// pieces of EB_CH whose row numbers and A columns are staged in LDS first.
constexpr int EB_CH = 128;
__global__ __launch_bounds__(256) void lora_embed_db_kernel(int64_t H, int64_t na, int64_t a0,
                                                            const int64_t* __restrict__ ids,
                                                            const int32_t* __restrict__ sorted_rows,
                                                            const int32_t* __restrict__ offsets,
                                                            const bf16_t* __restrict__ dout, float normalizer,
                                                            const bf16_t* __restrict__ A, int r, float s,
                                                            bf16_t* __restrict__ dB, int accumulate) {
  __shared__ int rowS[EB_CH];
  __shared__ int idS[EB_CH];
  __shared__ float As[EB_CH][EH_MAXR];
  const int t = threadIdx.x, hl = t & 63, jg = t >> 6;
  const int64_t h = (int64_t)blockIdx.x * 64 + hl;
  const int n0 = offsets[0], n1 = offsets[na];
  float acc[EH_MAXR / 4];
#pragma unroll
  for (int k = 0; k < EH_MAXR / 4; ++k) acc[k] = 0.f;
  for (int base = n0; base < n1; base += EB_CH) {
    const int cnt = min(EB_CH, n1 - base);
    __syncthreads();
    if (t < cnt) {
      const int row = sorted_rows[base + t];
      rowS[t] = row;
      idS[t] = (int)(ids[row] - a0);
    }
    __syncthreads();
    for (int idx = t; idx < cnt * r; idx += 256) {
      const int i = idx / r, j = idx - i * r;
      As[i][j] = bf2f(A[(int64_t)j * na + idS[i]]);
    }
    __syncthreads();
    if (h < H) {
#pragma unroll 4
      for (int i = 0; i < cnt; ++i) {
        const float g = round_bf(bf2f(dout[(int64_t)rowS[i] * H + h]) * normalizer);
#pragma unroll
        for (int k = 0; k < EH_MAXR / 4; ++k)
          if (jg + 4 * k < r) acc[k] += g * As[i][jg + 4 * k];
      }
    }
  }
  if (h < H) {
#pragma unroll
    for (int k = 0; k < EH_MAXR / 4; ++k) {
      const int j = jg + 4 * k;
      if (j < r) {
        const int64_t o = h * r + j;
        const float val = s * acc[k];
        dB[o] = f2bf(accumulate ? bf2f(dB[o]) + round_bf(val) : val);
      }
    }
  }
}

// ------------------------------------------------------------------ lm_head: adapter term + softcap + statistics
// lane value from the DPP partner, the 16-lane butterfly of softcap.hip's pass (xor 1, xor 2, half-row mirror, row
// mirror), operand for operand: the group statistics are that pass's bits
template <int CTRL>
__device__ __forceinline__ int eh_dpp(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float eh_dppf(float x) {
  return __int_as_float(eh_dpp<CTRL>(__float_as_int(x)));
}
constexpr int EH_X1 = 0xb1, EH_X2 = 0x4e, EH_HALF_MIRROR = 0x141, EH_MIRROR = 0x140;
constexpr int EH_COLS = 512;  // columns of a block's chunk: 8 per lane

typedef __bf16 eh_bf2 __attribute__((ext_vector_type(2)));
// acc + a.lo b.lo + a.hi b.hi on packed bf16 pairs, fp32 accumulate (v_dot2c_f32_bf16)
__device__ __forceinline__ float eh_dot2(uint32_t a, uint32_t b, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(eh_bf2, a), __builtin_bit_cast(eh_bf2, b), acc, false);
}

// B's rows in LDS as Bs[j / 2][slot]: one dword = the bf16 pair (B[n][j], B[n][j + 1]), as it lies in global memory, so a
// lane's term is r / 2 packed dot products per column with the T pair (wave-uniform) and no unpacking.  Column c of
// the chunk sits at dword (c & 4 ? 256 : 0) + (c >> 3) * 4 + (c & 3): a lane's columns 8l .. 8l+3 and 8l+4 .. 8l+7 are
// two 16-B slots l and 64 + l, so both ds_read_b128 of a wave walk consecutive slots (no bank conflict) while the lane
// keeps the eight consecutive columns svla_softcap_ce_rows' statistics partition gives it.
template <int RMAX>
__global__ __launch_bounds__(256) void lora_softcap_rows_kernel(int64_t M, int64_t N, bf16_t* __restrict__ lg, int64_t ld,
                                                                const bf16_t* __restrict__ T, int64_t ldt,
                                                                const bf16_t* __restrict__ B, int r, float s, float cap,
                                                                float* __restrict__ row_stats) {
  __shared__ __attribute__((aligned(16))) unsigned short tab[TANH_TAB_BYTES / 2 + 8];
  __shared__ __attribute__((aligned(16))) uint32_t Bs[RMAX / 2][EH_COLS];
  const int tid = threadIdx.x;
  if (tid < TANH_TAB_BYTES / 16)
    reinterpret_cast<u32x4*>(tab)[tid] = reinterpret_cast<const u32x4*>(svla_tanh_bf16_tab)[tid];
  const int64_t c0 = (int64_t)blockIdx.x * EH_COLS;
  // B rows [c0, c0 + 512); rows at or beyond N read as zero
  for (int idx = tid; idx < EH_COLS * (r >> 3); idx += 256) {
    const int col = idx % EH_COLS, j0 = (idx / EH_COLS) << 3;
    u32x4 w = {0u, 0u, 0u, 0u};
    if (c0 + col < N) w = *reinterpret_cast<const u32x4*>(B + (c0 + col) * r + j0);
    const int pos = ((col & 4) ? EH_COLS / 2 : 0) + (col >> 3) * 4 + (col & 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) Bs[(j0 >> 1) + i][pos] = w[i];
  }
  __syncthreads();
  const float icap = 1.0f / cap;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ntn = (N + 127) / 128;
  const int64_t n = c0 + 8 * lane;
  const int64_t nv = N - n;  // valid columns of this lane: >= 8 whole chunk, 1..7 ragged row end, <= 0 none
  const int64_t mstep = (int64_t)gridDim.y * 4;
  int64_t m = (int64_t)blockIdx.y * 4 + wave;
  u32x4 wcur = {0u, 0u, 0u, 0u};
  if (m < M && nv >= 8) wcur = *reinterpret_cast<const u32x4*>(lg + m * ld + n);
  for (; m < M; m += mstep) {
    bf16_t* p = lg + m * ld + n;
    u32x4 wnext = {0u, 0u, 0u, 0u};  // the next row's chunk is in flight while this one is computed
    if (m + mstep < M && nv >= 8) wnext = *reinterpret_cast<const u32x4*>(p + mstep * ld);
    const u32x4* tp = reinterpret_cast<const u32x4*>(T + m * ldt);  // wave-uniform
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < RMAX / 8; ++q) {
      if (q * 8 < r) {
        const u32x4 tq = tp[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const u32x4 b0 = *reinterpret_cast<const u32x4*>(&Bs[q * 4 + i][4 * lane]);
          const u32x4 b1 = *reinterpret_cast<const u32x4*>(&Bs[q * 4 + i][EH_COLS / 2 + 4 * lane]);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            acc[k] = eh_dot2(b0[k], tq[i], acc[k]);
            acc[4 + k] = eh_dot2(b1[k], tq[i], acc[4 + k]);
          }
        }
      }
    }
    float v[8];
    if (nv >= 8) {
      unpack8(wcur, v);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = i < nv ? bf2f(p[i]) : 0.f;
    }
    float mx = -INFINITY, se = 0.f;
    int am = 0x7fffffff;
    if (nv > 0) {
      // the in-order scan of svla_softcap_ce_rows' per-element unit, on the adapted logit
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float term = round_bf(s * acc[i]);
        if (term != 0.f) v[i] = round_bf(v[i] + term);  // a zero term keeps the raw bits (-0 included)
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
    gm = fmaxf(gm, eh_dppf<EH_X1>(gm));
    gm = fmaxf(gm, eh_dppf<EH_X2>(gm));
    gm = fmaxf(gm, eh_dppf<EH_HALF_MIRROR>(gm));
    gm = fmaxf(gm, eh_dppf<EH_MIRROR>(gm));
    se = (mx == -INFINITY) ? 0.f : se * __expf(mx - gm);
    am = (mx == gm) ? am : 0x7fffffff;
    se += eh_dppf<EH_X1>(se);
    am = min(am, eh_dpp<EH_X1>(am));
    se += eh_dppf<EH_X2>(se);
    am = min(am, eh_dpp<EH_X2>(am));
    se += eh_dppf<EH_HALF_MIRROR>(se);
    am = min(am, eh_dpp<EH_HALF_MIRROR>(am));
    se += eh_dppf<EH_MIRROR>(se);
    am = min(am, eh_dpp<EH_MIRROR>(am));
    if ((lane & 15) == 0 && nv > 0) {
      float* rs = row_stats + (m * ntn + n / 128) * 3;
      rs[0] = gm;
      rs[1] = se;
      rs[2] = __int_as_float(am);
    }
    wcur = wnext;
  }
}

bool rank_ok(int r) { return r >= 8 && r <= EH_MAXR && r % 8 == 0; }
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int svla_lora_embed_fwd(int64_t rows, int64_t H, const int64_t* ids, const int32_t* img_index,
                                   const void* embed, const void* spatial, int64_t a0, int64_t na, const void* A,
                                   const void* B, int32_t r, float scaling, float normalizer, void* out, void* stream) {
  SVLA_CHECK_ARG(rows > 0 && rows < (1ll << 31) && H > 0 && H % 8 == 0 && na > 0, "lora_embed_fwd: rows, H %% 8, na");
  SVLA_CHECK_ARG(rank_ok(r), "lora_embed_fwd: r must be a multiple of 8 in [8, 64], got %d", (int)r);
  SVLA_CHECK_ARG(ids && embed && spatial && A && B && out, "lora_embed_fwd: null pointer");
  SVLA_CHECK_ARG(al16(embed) && al16(spatial) && al16(B) && al16(out), "lora_embed_fwd: 16-B aligned tables");
  hipLaunchKernelGGL(lora_embed_fwd_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, H, ids, img_index,
                     (const bf16_t*)embed, (const bf16_t*)spatial, a0, na, (const bf16_t*)A, (const bf16_t*)B, (int)r,
                     scaling, normalizer, (bf16_t*)out);
  return svla::check_launch("lora_embed_fwd");
}

extern "C" int svla_lora_embed_decode(int64_t rows, int64_t H, const int64_t* ids, const void* embed, const void* spatial,
                                      int64_t a0, int64_t na, const void* A, const void* B, int32_t r, float scaling,
                                      float normalizer, void* out, void* stream) {
  SVLA_CHECK_ARG(rows >= 1 && rows <= 8 && H > 0 && H % 8 == 0 && na > 0, "lora_embed_decode: rows in [1, 8], H %% 8, na");
  SVLA_CHECK_ARG(rank_ok(r), "lora_embed_decode: r must be a multiple of 8 in [8, 64], got %d", (int)r);
  SVLA_CHECK_ARG(ids && embed && spatial && A && B && out, "lora_embed_decode: null pointer");
  SVLA_CHECK_ARG(al16(embed) && al16(spatial) && al16(B) && al16(out), "lora_embed_decode: 16-B aligned tables");
  hipLaunchKernelGGL(lora_embed_decode_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, H, ids,
                     (const bf16_t*)embed, (const bf16_t*)spatial, a0, na, (const bf16_t*)A, (const bf16_t*)B, (int)r,
                     scaling, normalizer, (bf16_t*)out);
  return svla::check_launch("lora_embed_decode");
}

extern "C" int svla_lora_embed_bwd(int64_t rows, int64_t H, const int64_t* ids, const int32_t* spatial_sorted_rows,
                                   const int32_t* spatial_offsets, int64_t a0, int64_t na, const void* dout,
                                   float normalizer, const void* A, const void* B, int32_t r, float scaling, void* dA,
                                   void* dB, int32_t accumulate, void* stream) {
  SVLA_CHECK_ARG(rows > 0 && rows < (1ll << 31) && H > 0 && H % 8 == 0 && na > 0 && na < (1ll << 31),
                 "lora_embed_bwd: rows, H %% 8, na");
  SVLA_CHECK_ARG(rank_ok(r), "lora_embed_bwd: r must be a multiple of 8 in [8, 64], got %d", (int)r);
  SVLA_CHECK_ARG(ids && spatial_sorted_rows && spatial_offsets && dout && A && B, "lora_embed_bwd: null pointer");
  if (dA)
    hipLaunchKernelGGL(lora_embed_da_kernel, dim3((unsigned)na), dim3(256), 0, (hipStream_t)stream, H, na,
                       spatial_sorted_rows, spatial_offsets, (const bf16_t*)dout, normalizer, (const bf16_t*)B, (int)r,
                       scaling, (bf16_t*)dA, (int)accumulate);
  if (dB)
    hipLaunchKernelGGL(lora_embed_db_kernel, dim3((unsigned)((H + 63) / 64)), dim3(256), 0, (hipStream_t)stream, H, na,
                       a0, ids, spatial_sorted_rows, spatial_offsets, (const bf16_t*)dout, normalizer, (const bf16_t*)A,
                       (int)r, scaling, (bf16_t*)dB, (int)accumulate);
  return svla::check_launch("lora_embed_bwd");
}

extern "C" int svla_lora_softcap_ce_rows(int64_t M, int64_t N, void* logits, int64_t ld, const void* t, int64_t ldt,
                                         const void* B, int32_t r, float scaling, float cap, float* row_stats,
                                         void* stream) {
  SVLA_CHECK_ARG(M > 0 && N > 0 && ld >= N && ld % 8 == 0 && cap > 0.f, "lora_softcap_ce_rows: M, N, ld (multiple of 8 "
                 ">= N), cap > 0");
  SVLA_CHECK_ARG(rank_ok(r) && ldt >= r && ldt % 8 == 0, "lora_softcap_ce_rows: r a multiple of 8 in [8, 64], ldt "
                 "(multiple of 8) >= r");
  SVLA_CHECK_ARG(logits && row_stats && t && B && al16(logits) && al16(B) && al16(t), "lora_softcap_ce_rows: logits, "
                 "T and B 16-B aligned");
  const int64_t chunks = (N + EH_COLS - 1) / EH_COLS;
  // row slices: enough blocks for ~4 per CU, each wave of a block keeping at least 8 rows (the B chunk is staged once
  // per block)
  int64_t ys = std::max<int64_t>(1, ((int64_t)svla::num_cus() * 4 + chunks - 1) / chunks);
  ys = std::min<int64_t>(ys, std::max<int64_t>(1, M / 32));
  ys = std::min<int64_t>(ys, 65535);
  const dim3 grid((unsigned)chunks, (unsigned)ys);
  if (r <= 32)
    hipLaunchKernelGGL(lora_softcap_rows_kernel<32>, grid, dim3(256), 0, (hipStream_t)stream, M, N, (bf16_t*)logits, ld,
                       (const bf16_t*)t, ldt, (const bf16_t*)B, (int)r, scaling, cap, row_stats);
  else
    hipLaunchKernelGGL(lora_softcap_rows_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, M, N, (bf16_t*)logits, ld,
                       (const bf16_t*)t, ldt, (const bf16_t*)B, (int)r, scaling, cap, row_stats);
  return svla::check_launch("lora_softcap_ce_rows");
}
