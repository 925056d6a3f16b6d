// Rank-r (LoRA) products for gfx950 (MI355X): svla_lora_down, svla_lora_up, svla_lora_wgrad (include/svla.h).
//
// A LoRA adapter adds s * B (A x) to a frozen projection W x (reference train/spatialvla_finetune.py:262-300).  Its
// three products are tall and skinny -- [M, K] x [K, r], [M, r] x [r, N] added into an existing matrix, and an M-long
// reduction to [r, K] / [N, r] with r <= 64 -- so they are bound by the one pass over the large matrix, and the
// 256 x 256 / 64 x 64 LDS-staged tiles of gemm.hip are the wrong tool.  Here every product is
// v_mfma_f32_16x16x32_bf16 with both fragments loaded straight from global memory (a fragment is 8 consecutive k of
// one row: one 16-B load where the reduction index is contiguous, 8 two-byte loads down a column where it is not; the
// small matrices stay in L2), no LDS operand image.  The operands are swapped (C^T is accumulated) wherever that makes
// a lane own consecutive columns of one output row.
//   MFMA maps: D[i][j] = sum_k A[i][k] B[k][j]; lane l holds A[i = l & 15][k = 8 (l >> 4) + e] and
//   B[k = 8 (l >> 4) + e][j = l & 15] (e = 0..7) and D[i = 4 (l >> 4) + reg][j = l & 15].
// Nothing here uses atomics: reductions over workgroups go through fp32 partials summed in a fixed order.
#include "svla_common.h"

namespace {

constexpr int MAX_SEG = 3;
constexpr int MAX_R = 64;                 // rank-space slice width R = round_up(r, 32) <= 64: at most 4 16-column tiles
constexpr int TPS = MAX_R / 16;           // accumulator tiles reserved per segment

struct Segs {
  const bf16_t* p[MAX_SEG];
  int64_t st[MAX_SEG + 1];
  int64_t ld;
  int nseg, r, R;
};

__device__ __forceinline__ const bf16_t* seg_p(const Segs& S, int s) {
  return s == 0 ? S.p[0] : (s == 1 ? S.p[1] : S.p[2]);
}
// segment of column n (starts ascending, st[0] == 0)
__device__ __forceinline__ int seg_of(const Segs& S, int64_t n) {
  return (int)(S.nseg > 1 && n >= S.st[1]) + (int)(S.nseg > 2 && n >= S.st[2]);
}
__device__ __forceinline__ int64_t seg_st(const Segs& S, int s) { return s == 0 ? 0 : (s == 1 ? S.st[1] : S.st[2]); }

// fragment of 8 consecutive elements (one 16-B load), zeros when !ok
__device__ __forceinline__ bf16x8 ld8(const bf16_t* p, bool ok) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (ok) v = *reinterpret_cast<const u32x4*>(p);
  return __builtin_bit_cast(bf16x8, v);
}
// fragment of 8 elements `stride` apart (down a column of a row-major matrix); elements >= nvalid read as zero
__device__ __forceinline__ bf16x8 ld8s(const bf16_t* p, int64_t stride, int nvalid) {
  u32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t lo = 2 * i < nvalid ? (uint32_t)p[(2 * i) * stride] : 0u;
    const uint32_t hi = 2 * i + 1 < nvalid ? (uint32_t)p[(2 * i + 1) * stride] : 0u;
    v[i] = lo | (hi << 16);
  }
  return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ void unpack4(u32x2 v, float* f) {
  f[0] = __uint_as_float(v[0] << 16);
  f[1] = __uint_as_float(v[0] & 0xffff0000u);
  f[2] = __uint_as_float(v[1] << 16);
  f[3] = __uint_as_float(v[1] & 0xffff0000u);
}
__device__ __forceinline__ u32x2 pack4(const float* f) { return u32x2{pack2(f[0], f[1]), pack2(f[2], f[3])}; }

// ------------------------------------------------------------------------------------------------ lora_down
// One workgroup = 16 rows of X; its 8 waves split the reduction.  Shared mode: a wave takes 64 consecutive k per
// round (two k-steps: 128 contiguous bytes of every row, both loads in flight).  Sliced mode: the fragment of S runs
// down a column, so a wave reads its 32-row block of S (contiguous in memory) with 16-B loads and transposes it
// through its own LDS image; the fragment is then one 16-B LDS read (the first version gathered it with eight 2-byte
// global loads and lost to the GEMM composition at 18432 columns).  The fp32 partial tiles meet in LDS (the same
// bytes as the images, after a barrier): waves 4..7 are folded into waves 0..3, then those four are summed, always
// in the same order.  C^T is accumulated: first
// operand = the small matrix (rank index on the rows), second = X, so a lane holds row m = l & 15 and rank columns
// 4 (l >> 4) .. +3 of a tile.
constexpr int DOWN_NW = 8;
constexpr int DOWN_RB = 2;  // shared mode: row blocks per wave (q|k|v forward 51.7 us at 1, 48.2 us at 2)
constexpr int DOWN_SLD = 40;  // sliced mode: a wave's transposed image of a 32-row block of S, [rank j][32 rows + 8 pad]
constexpr int DOWN_LD = MAX_SEG * MAX_R + 4;

template <bool SLICED>
__global__ __launch_bounds__(64 * DOWN_NW) void lora_down_kernel(int64_t M, int64_t K, const bf16_t* __restrict__ X, int64_t ldx,
                                                        Segs S, float alpha, bf16_t* __restrict__ T, int64_t ldt) {
  constexpr int RB = SLICED ? 1 : DOWN_RB;  // row blocks per wave: they share the wave's fragments of the small matrix
  __shared__ __attribute__((aligned(16))) float red[4][16][DOWN_LD];
  static_assert(sizeof(bf16_t) * DOWN_NW * MAX_R * DOWN_SLD <= sizeof(float) * 4 * 16 * DOWN_LD, "images alias red");
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, mi = l & 15, g = l >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * (16 * RB);
  const int tps = S.R >> 4;
  bool mok[RB];
  const bf16_t* xr[RB];
#pragma unroll
  for (int b = 0; b < RB; ++b) {
    const int64_t m = m0 + 16 * b + mi;
    mok[b] = m < M;
    xr[b] = X + (mok[b] ? m : 0) * ldx;
  }
  f32x4 acc[RB][MAX_SEG][TPS];
#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int s = 0; s < MAX_SEG; ++s)
#pragma unroll
      for (int t = 0; t < TPS; ++t) acc[b][s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (!SLICED) {
    // T[m, sR + j] = sum_k X[m, k] S_s[j, k]   (S_s [r][K], k contiguous)
    for (int64_t kk = (int64_t)w * 64; kk < K; kk += 64 * DOWN_NW) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int64_t k = kk + 32 * u + 8 * g;
        const bool kok = k < K;
        bf16x8 xf[RB];
#pragma unroll
        for (int b = 0; b < RB; ++b) xf[b] = ld8(xr[b] + k, mok[b] && kok);
#pragma unroll
        for (int s = 0; s < MAX_SEG; ++s) {
          if (s >= S.nseg) continue;
#pragma unroll
          for (int t = 0; t < TPS; ++t) {
            if (t >= tps) continue;
            const int j = t * 16 + mi;
            const bf16x8 sf = ld8(S.p[s] + (int64_t)j * S.ld + k, kok && j < S.r);
#pragma unroll
            for (int b = 0; b < RB; ++b) acc[b][s][t] = mfma(sf, xf[b], acc[b][s][t]);
          }
        }
      }
    }
  } else {
    // T[m, sR + j] = sum_c X[m, st_s + c] S_s[c, j]   (S_s [N_s][r], j contiguous: the fragment runs down a column)
#pragma unroll
    for (int s = 0; s < MAX_SEG; ++s) {
      if (s >= S.nseg) continue;
      const int64_t beg = S.st[s], len = S.st[s + 1] - S.st[s];
      bf16_t(*St)[DOWN_SLD] = reinterpret_cast<bf16_t(*)[DOWN_SLD]>(&red[0][0][0]) + w * MAX_R;
      const int rc = S.r >> 3;  // 16-B chunks per row of S
      for (int64_t kk = (int64_t)w * 32; kk < len; kk += 32 * DOWN_NW) {
        const int64_t c = kk + 8 * g;
        const bool cok = c < len;  // len % 8 == 0: a chunk is whole or absent
        bf16x8 xf[RB];
#pragma unroll
        for (int b = 0; b < RB; ++b) xf[b] = ld8(xr[b] + beg + c, mok[b] && cok);
        // rows kk .. kk+31 of S_s ([32][r], contiguous when ld == r) -> St[j][row]
        u32x4 sv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int idx = l + 64 * i, row = idx / rc, ch = idx - row * rc;
          sv[i] = u32x4{0u, 0u, 0u, 0u};
          if (idx < 32 * rc && kk + row < len) sv[i] = *reinterpret_cast<const u32x4*>(S.p[s] + (kk + row) * S.ld + 8 * ch);
        }
        __builtin_amdgcn_wave_barrier();  // the previous round's fragment reads precede these writes (one wave, in order)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int idx = l + 64 * i, row = idx / rc, ch = idx - row * rc;
          if (idx < 32 * rc) {
#pragma unroll
            for (int e = 0; e < 8; ++e) St[8 * ch + e][row] = (bf16_t)(sv[i][e >> 1] >> (16 * (e & 1)));
          }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < TPS; ++t) {
          if (t >= tps) continue;
          const int j = t * 16 + mi;
          u32x4 fv = *reinterpret_cast<const u32x4*>(&St[j < S.r ? j : 0][8 * g]);
          if (j >= S.r) fv = u32x4{0u, 0u, 0u, 0u};
          const bf16x8 sf = __builtin_bit_cast(bf16x8, fv);
#pragma unroll
          for (int b = 0; b < RB; ++b) acc[b][s][t] = mfma(sf, xf[b], acc[b][s][t]);
        }
      }
    }
  }
  const int cps = S.R >> 3;  // 8-column chunks per segment slice
  const int cpr = S.nseg * cps;
#pragma unroll
  for (int b = 0; b < RB; ++b) {
    for (int q = 1; q < DOWN_NW / 4; ++q) {  // fold waves 4q .. 4q+3 into waves 0..3
      __syncthreads();
      if ((w >> 2) == q) {
#pragma unroll
        for (int s = 0; s < MAX_SEG; ++s)
#pragma unroll
          for (int t = 0; t < TPS; ++t)
            *reinterpret_cast<f32x4*>(&red[w & 3][mi][s * MAX_R + t * 16 + 4 * g]) = acc[b][s][t];
      }
      __syncthreads();
      if (w < 4) {
#pragma unroll
        for (int s = 0; s < MAX_SEG; ++s)
#pragma unroll
          for (int t = 0; t < TPS; ++t)
            acc[b][s][t] += *reinterpret_cast<const f32x4*>(&red[w][mi][s * MAX_R + t * 16 + 4 * g]);
      }
    }
    __syncthreads();
    if (w < 4) {
#pragma unroll
      for (int s = 0; s < MAX_SEG; ++s)
#pragma unroll
        for (int t = 0; t < TPS; ++t)
          *reinterpret_cast<f32x4*>(&red[w][mi][s * MAX_R + t * 16 + 4 * g]) = acc[b][s][t];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 16 * cpr; idx += 64 * DOWN_NW) {
      const int row = idx / cpr, ch = idx % cpr, s = ch / cps, cc = ch % cps;
      const int64_t m = m0 + 16 * b + row;
      if (m >= M) continue;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = s * MAX_R + cc * 8 + e;
        v[e] = alpha * (((red[0][row][col] + red[1][row][col]) + red[2][row][col]) + red[3][row][col]);
      }
      *reinterpret_cast<u32x4*>(T + m * ldt + s * S.R + cc * 8) = pack8(v);
    }
  }
}

// ------------------------------------------------------------------------------------------------ lora_up
// One wave = a pair of 16-column tiles of C (ROPE: column d and d + D/2 of a head; GEGLU: gate column n and up column
// I + n; else two neighbours) whose fragments of the small matrices stay in registers while it walks down the rows,
// 16 at a time, the next row block's T and C loads issued before the current MFMAs.  C^T is accumulated (first
// operand = the small matrix, column index on the rows), so a lane owns 4 consecutive columns of row m = l & 15 of
// each tile: it reads them, adds, applies the epilogue and writes them back -- no element is touched by two lanes.
// GELU / RESID / SCALE (the vision-side linears: SigLIP fc1, out_proj | fc2 | Ego3D head.3, the projector) work on the
// adapted bf16 value of each of the lane's columns on its own, so both tiles of a unit take the same path and the
// last unit of an N with N % 32 == 16 (SigLIP I = 4304) simply has no b tile (b_ok false: nothing loaded or stored).
enum { UP_NONE = 0, UP_ROPE = 1, UP_GEGLU = 2, UP_GELU = 3, UP_RESID = 4, UP_SCALE = 5 };
struct UpEpi {
  const bf16_t* cos;
  const bf16_t* sin;
  int64_t rope_ld, rope_cols;
  bf16_t* h;
  int64_t ldh;
  int rope_L, rope_D;
  const bf16_t* res;  // RESID: added after the adapter term, row stride ldres (never aliases C)
  int64_t ldres;
  float post;         // SCALE
};
constexpr int UP_F = MAX_SEG * 2;  // k-steps of 32 a tile can need (summed: 3 segments x R / 32)

template <bool SUMMED, int EPI>
__global__ __launch_bounds__(256) void lora_up_kernel(int64_t M, int64_t N, bf16_t* __restrict__ C, int64_t ldc,
                                                      const bf16_t* __restrict__ T, int64_t ldt, Segs S, float alpha,
                                                      UpEpi E, int64_t nunits) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, mi = l & 15, g = l >> 4;
  // GELU: the bf16 gelu table in LDS, copied once per workgroup before any wave leaves (svla_gelu_rows does the same:
  // from global memory every lookup is a scattered 2-B load)
  __shared__ __attribute__((aligned(16))) unsigned short ltab[EPI == UP_GELU ? 2 * SVLA_GELU_TAB_N : 8];
  if constexpr (EPI == UP_GELU) {
    constexpr int NCH = (int)(sizeof(svla_gelu_bf16_tab) / 16);
    for (int i = threadIdx.x; i < NCH; i += 256)
      reinterpret_cast<u32x4*>(ltab)[i] = reinterpret_cast<const u32x4*>(svla_gelu_bf16_tab)[i];
    __syncthreads();
  }
  const int64_t u = (int64_t)blockIdx.x * 4 + w;
  if (u >= nunits) return;
  int64_t na, nb, lim_a = N;
  bool rot = false;
  int dd = 0;
  if constexpr (EPI == UP_GEGLU) {
    na = 16 * u;
    nb = (N >> 1) + na;
    lim_a = N >> 1;
  } else if constexpr (EPI == UP_ROPE) {
    const int half = E.rope_D >> 1, tph = half >> 4;
    const int64_t nrot = (E.rope_cols / E.rope_D) * tph;
    if (u < nrot) {
      rot = true;
      dd = (int)(u % tph) * 16;
      na = (u / tph) * E.rope_D + dd;
      nb = na + half;
    } else {
      na = E.rope_cols + 32 * (u - nrot);
      nb = na + 16;
    }
  } else {
    na = 32 * u;
    nb = na + 16;
  }
  const bool a_ok = na + 4 * g < lim_a, b_ok = nb + 4 * g < N;  // this lane's 4 columns exist (N, N/2 multiples of 4)
  const int sa = SUMMED ? 0 : seg_of(S, na), sb = SUMMED ? 0 : seg_of(S, nb < N ? nb : na);
  const int ksteps = S.R >> 5;

  // fragments of the small matrices, loaded once
  bf16x8 fa[UP_F], fb[UP_F];
  if constexpr (!SUMMED) {
    // column n of segment s uses S_s[n - st_s, j]  (S_s [N_s][r], j contiguous)
    const int64_t ra = na + mi, rb = nb + mi;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = 32 * q + 8 * g;
      fa[q] = ld8(seg_p(S, sa) + (ra - seg_st(S, sa)) * S.ld + j, ra < lim_a && j < S.r);
      fb[q] = ld8(seg_p(S, sb) + (rb - seg_st(S, sb)) * S.ld + j, rb < N && j < S.r);
    }
  } else {
    // every column sums over all segments: S_s[j, n]  (S_s [r][N], n contiguous: the fragment runs down a column)
#pragma unroll
    for (int s = 0; s < MAX_SEG; ++s)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int j = 32 * q + 8 * g;
        const bool on = s < S.nseg && q < ksteps && j < S.r;
        const int64_t ra = na + mi, rb = nb + mi;
        fa[2 * s + q] = ld8s(S.p[s] + (int64_t)j * S.ld + ra, S.ld, on && ra < N ? 8 : 0);
        fb[2 * s + q] = ld8s(S.p[s] + (int64_t)j * S.ld + rb, S.ld, on && rb < N ? 8 : 0);
      }
  }

  const int64_t nrb = (M + 15) / 16;
  bf16x8 ta[UP_F], tb[2], ta_n[UP_F], tb_n[2];
  u32x2 ca = {0u, 0u}, cb = {0u, 0u}, ca_n = {0u, 0u}, cb_n = {0u, 0u};
  u32x2 ea = {0u, 0u}, eb = {0u, 0u}, ea_n = {0u, 0u}, eb_n = {0u, 0u};  // RESID: the lane's columns of res
  auto load_rows = [&](int64_t rb, bf16x8(&xa)[UP_F], bf16x8(&xb)[2], u32x2& ya, u32x2& yb, u32x2& za, u32x2& zb) {
    const int64_t m = rb * 16 + mi;
    const bool mok = m < M;
    const bf16_t* tr = T + (mok ? m : 0) * ldt;
    if constexpr (!SUMMED) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int j = 32 * q + 8 * g;
        xa[q] = ld8(tr + sa * S.R + j, mok && j < S.r);
        xb[q] = ld8(tr + sb * S.R + j, mok && j < S.r);
      }
    } else {
#pragma unroll
      for (int s = 0; s < MAX_SEG; ++s)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int j = 32 * q + 8 * g;
          xa[2 * s + q] = ld8(tr + s * S.R + j, mok && s < S.nseg && j < S.r);
        }
    }
    bf16_t* cr = C + (mok ? m : 0) * ldc;
    ya = u32x2{0u, 0u};
    yb = u32x2{0u, 0u};
    if (mok && a_ok) ya = *reinterpret_cast<const u32x2*>(cr + na + 4 * g);
    if (mok && b_ok) yb = *reinterpret_cast<const u32x2*>(cr + nb + 4 * g);
    if constexpr (EPI == UP_RESID) {
      const bf16_t* rr = E.res + (mok ? m : 0) * E.ldres;
      za = u32x2{0u, 0u};
      zb = u32x2{0u, 0u};
      if (mok && a_ok) za = *reinterpret_cast<const u32x2*>(rr + na + 4 * g);
      if (mok && b_ok) zb = *reinterpret_cast<const u32x2*>(rr + nb + 4 * g);
    }
  };

  int64_t rb = blockIdx.y;
  if (rb < nrb) load_rows(rb, ta_n, tb_n, ca_n, cb_n, ea_n, eb_n);
  for (; rb < nrb; rb += gridDim.y) {
#pragma unroll
    for (int i = 0; i < UP_F; ++i) ta[i] = ta_n[i];
    tb[0] = tb_n[0];
    tb[1] = tb_n[1];
    ca = ca_n;
    cb = cb_n;
    ea = ea_n;
    eb = eb_n;
    if (rb + gridDim.y < nrb) load_rows(rb + gridDim.y, ta_n, tb_n, ca_n, cb_n, ea_n, eb_n);
    f32x4 da = {0.f, 0.f, 0.f, 0.f}, db = {0.f, 0.f, 0.f, 0.f};
    if constexpr (!SUMMED) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (q >= ksteps) continue;
        da = mfma(fa[q], ta[q], da);
        db = mfma(fb[q], tb[q], db);
      }
    } else {
#pragma unroll
      for (int s = 0; s < MAX_SEG; ++s)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          if (s >= S.nseg || q >= ksteps) continue;
          da = mfma(fa[2 * s + q], ta[2 * s + q], da);
          db = mfma(fb[2 * s + q], ta[2 * s + q], db);
        }
    }
    const int64_t m = rb * 16 + mi;
    if (m >= M) continue;
    float a[4], b[4];
    unpack4(ca, a);
    unpack4(cb, b);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // the bf16 chain of the reference: u rounded, then the sum rounded
      a[i] = round_bf(a[i] + round_bf(alpha * da[i]));
      b[i] = round_bf(b[i] + round_bf(alpha * db[i]));
    }
    bf16_t* cr = C + m * ldc;
    if constexpr (EPI == UP_ROPE) {
      if (rot) {  // a = columns d.., b = their partners D/2 away: out = bf16(bf16(x cos) + bf16(rotate_half(x) sin))
        const int64_t pos = m % E.rope_L;
        float cs[4], sn[4], ol[4], oh[4];
        unpack4(*reinterpret_cast<const u32x2*>(E.cos + pos * E.rope_ld + dd + 4 * g), cs);
        unpack4(*reinterpret_cast<const u32x2*>(E.sin + pos * E.rope_ld + dd + 4 * g), sn);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          ol[i] = round_bf(a[i] * cs[i]) + round_bf(-b[i] * sn[i]);
          oh[i] = round_bf(b[i] * cs[i]) + round_bf(a[i] * sn[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { a[i] = ol[i]; b[i] = oh[i]; }
      }
    }
    if constexpr (EPI == UP_GEGLU) {
      if (a_ok) {  // a = g, b = u (bf16 values): h = bf16(bf16(gelu_tanh(g)) * u), the GeGLU GEMM epilogue's formula
        float h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = gelu_bf16(a[i]) * b[i];
        *reinterpret_cast<u32x2*>(E.h + m * E.ldh + na + 4 * g) = pack4(h);
      }
    }
    if constexpr (EPI == UP_GELU) {  // C keeps the pre-activation; h = bf16(gelu_tanh(v)): svla_gelu_rows' element formula
      float ha[4], hb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ha[i] = gelu_bf16_lut(__float_as_uint(a[i]) >> 16, a[i], ltab);
        hb[i] = gelu_bf16_lut(__float_as_uint(b[i]) >> 16, b[i], ltab);
      }
      bf16_t* hr = E.h + m * E.ldh;
      if (a_ok) *reinterpret_cast<u32x2*>(hr + na + 4 * g) = pack4(ha);
      if (b_ok) *reinterpret_cast<u32x2*>(hr + nb + 4 * g) = pack4(hb);
    }
    if constexpr (EPI == UP_RESID) {  // bf16(v + res): SVLA_EPI_BIAS_RESID's last rounding after a plain adapter add
      float x[4], y[4];
      unpack4(ea, x);
      unpack4(eb, y);
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] += x[i]; b[i] += y[i]; }
    }
    if constexpr (EPI == UP_SCALE) {  // bf16(v post): SVLA_EPI_BIAS's alpha after its bf16(acc + bias)
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] *= E.post; b[i] *= E.post; }
    }
    if (a_ok) *reinterpret_cast<u32x2*>(cr + na + 4 * g) = pack4(a);
    if (b_ok) *reinterpret_cast<u32x2*>(cr + nb + 4 * g) = pack4(b);
  }
}

// GEGLU with the OCP MX e4m3 copy of h (the fp8 down projection's operand) out of the same pass.  One wave = the 32
// gate columns of one MX block and their 32 up columns, two 16-column MFMA tiles each.  The tiles' rows are assigned so
// that a lane owns 8 consecutive columns of row m = l & 15: MFMA row i of tile t is column 8 (i >> 2) + 4 t + (i & 3),
// so lane group g = l >> 4 holds columns 8 g .. + 3 from tile 0 and 8 g + 4 .. + 7 from tile 1 (a dot product does not
// depend on where its column sits in a tile: g | u and h are the bits of lora_up_kernel).  The four lanes l & 15,
// + 16, + 32, + 48 hold one row's block, so its maximum is two xor shuffles on the h values still in registers;
// the e4m3 bytes leave as one 8-B store a lane, the E8M0 byte from the block's first lane (svla_quant_mx_rows' layout
// and element formula, fp8.hip).  N/2 % 128 == 0: every wave of the grid has all its columns, only rows are ragged.
__global__ __launch_bounds__(256) void lora_up_geglu_mx_kernel(int64_t M, int64_t N, bf16_t* __restrict__ C, int64_t ldc,
                                                               const bf16_t* __restrict__ T, int64_t ldt, Segs S,
                                                               float alpha, bf16_t* __restrict__ H, int64_t ldh,
                                                               uint8_t* __restrict__ Q, int64_t ldq,
                                                               uint8_t* __restrict__ SC, int64_t sld) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, mi = l & 15, g = l >> 4;
  const int64_t I = N >> 1;
  const int64_t n0 = ((int64_t)blockIdx.x * 4 + w) * 32;  // the wave's MX block: gate columns n0 .., up columns I + n0 ..
  const int ksteps = S.R >> 5;
  bf16x8 fa[2][2], fb[2][2];  // [tile][k-step]: rows of B_gate / B_up, loaded once
#pragma unroll
  for (int tl = 0; tl < 2; ++tl) {
    const int64_t col = n0 + 8 * (mi >> 2) + 4 * tl + (mi & 3);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = 32 * q + 8 * g;
      fa[tl][q] = ld8(S.p[0] + col * S.ld + j, j < S.r);
      fb[tl][q] = ld8(S.p[1] + col * S.ld + j, j < S.r);
    }
  }
  const int64_t nrb = (M + 15) / 16;
  bf16x8 ta[2], tb[2], ta_n[2], tb_n[2];
  u32x4 ca, cb, ca_n = {0u, 0u, 0u, 0u}, cb_n = {0u, 0u, 0u, 0u};
  auto load_rows = [&](int64_t rb, bf16x8(&xa)[2], bf16x8(&xb)[2], u32x4& ya, u32x4& yb) {
    const int64_t m = rb * 16 + mi;
    const bool mok = m < M;
    const bf16_t* tr = T + (mok ? m : 0) * ldt;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = 32 * q + 8 * g;
      xa[q] = ld8(tr + j, mok && j < S.r);
      xb[q] = ld8(tr + S.R + j, mok && j < S.r);
    }
    const bf16_t* cr = C + (mok ? m : 0) * ldc + n0 + 8 * g;
    ya = u32x4{0u, 0u, 0u, 0u};
    yb = u32x4{0u, 0u, 0u, 0u};
    if (mok) {
      ya = *reinterpret_cast<const u32x4*>(cr);
      yb = *reinterpret_cast<const u32x4*>(cr + I);
    }
  };
  int64_t rb = blockIdx.y;
  if (rb < nrb) load_rows(rb, ta_n, tb_n, ca_n, cb_n);
  for (; rb < nrb; rb += gridDim.y) {
    ta[0] = ta_n[0]; ta[1] = ta_n[1];
    tb[0] = tb_n[0]; tb[1] = tb_n[1];
    ca = ca_n;
    cb = cb_n;
    if (rb + gridDim.y < nrb) load_rows(rb + gridDim.y, ta_n, tb_n, ca_n, cb_n);
    f32x4 da[2], db[2];
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) {
      da[tl] = f32x4{0.f, 0.f, 0.f, 0.f};
      db[tl] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (q >= ksteps) continue;
        da[tl] = mfma(fa[tl][q], ta[q], da[tl]);
        db[tl] = mfma(fb[tl][q], tb[q], db[tl]);
      }
    }
    // rows >= M went in as zeros and stay finite zeros: their lanes take part in the shuffles and store nothing
    const int64_t m = rb * 16 + mi;
    const bool mok = m < M;
    float a[8], b[8], h[8];
    unpack8(ca, a);
    unpack8(cb, b);
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // lora_up_kernel's bf16 chain and GeGLU formula
      a[i] = round_bf(a[i] + round_bf(alpha * da[i >> 2][i & 3]));
      b[i] = round_bf(b[i] + round_bf(alpha * db[i >> 2][i & 3]));
      h[i] = gelu_bf16(a[i]) * b[i];
    }
    const u32x4 hv = pack8(h);
    unpack8(hv, h);  // the bf16 h this launch stores: what the MX copy is made from
    uint32_t byte;
    const u32x2 qv = mx_block8<16, 32>(h, byte);  // the block's lanes are l & 15, + 16, + 32, + 48
    if (mok) {
      bf16_t* cr = C + m * ldc + n0 + 8 * g;
      *reinterpret_cast<u32x4*>(H + m * ldh + n0 + 8 * g) = hv;
      *reinterpret_cast<u32x4*>(cr) = pack8(a);
      *reinterpret_cast<u32x4*>(cr + I) = pack8(b);
      *reinterpret_cast<u32x2*>(Q + m * ldq + n0 + 8 * g) = qv;
      if (g == 0) SC[(n0 >> 7) * sld + m * 4 + ((n0 & 127) >> 5)] = (uint8_t)byte;
    }
  }
}

// ------------------------------------------------------------------------------------------------ lora_wgrad
// Both adapter gradients reduce over the rows m, which is the strided index of both operands, so both fragments run
// down columns: each k-block of 32 rows is read with coalesced 16-B row loads (the next one in flight during the
// MFMAs) and transposed through LDS.  A workgroup owns 128 columns of Y (2 tiles per wave) and one slice of the rows;
// it writes its fp32 partial tiles to the workspace and a second launch sums the slices in order (no counters, no block waits).
//   shared: dA_s[j, c] = sum_m T[m, sR + j] Y[m, c]           partials [split][nseg R][Wp]
//   sliced: dB_s[c, j] = alpha sum_m Y[m, st_s + c] T[m, sR + j]   partials [split][Wp][R]
constexpr int WG_CT = 2;
constexpr int WG_COLS = 4 * WG_CT * 16;

// LDS images of one k-block (32 rows) of the strip, transposed: [column][row], 32 rows + 8 pad per column (80-B rows,
// 16-B aligned), so that an MFMA fragment -- 8 consecutive rows m of one column -- is one 16-B LDS read.
constexpr int WG_TLD = 40;
constexpr int WG_TMAX = MAX_SEG * MAX_R;

template <bool SLICED>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(int64_t M, int64_t W, const bf16_t* __restrict__ Y, int64_t ldy,
                                                         const bf16_t* __restrict__ T, int64_t ldt, Segs S,
                                                         float* __restrict__ P, int64_t Wp, int64_t per) {
  __shared__ __attribute__((aligned(16))) bf16_t Yt[WG_COLS][WG_TLD];
  __shared__ __attribute__((aligned(16))) bf16_t Tt[WG_TMAX][WG_TLD];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, mi = l & 15, g = l >> 4;
  const int64_t cblk = (int64_t)blockIdx.x * WG_COLS;
  const int64_t c0 = cblk + w * (WG_CT * 16);
  const bool wave_on = c0 < W;
  const int tps = S.R >> 4;
  const int tc = (S.nseg * S.R) >> 3;  // 16-B chunks per row of T
  const int64_t nkb = (M + 31) / 32;
  const int64_t kb0 = (int64_t)blockIdx.y * per, kb1 = kb0 + per < nkb ? kb0 + per : nkb;
  f32x4 acc[WG_CT][MAX_SEG * TPS];
#pragma unroll
  for (int ct = 0; ct < WG_CT; ++ct)
#pragma unroll
    for (int i = 0; i < MAX_SEG * TPS; ++i) acc[ct][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  int sct[WG_CT];
#pragma unroll
  for (int ct = 0; ct < WG_CT; ++ct) sct[ct] = SLICED ? seg_of(S, c0 + ct * 16 < W ? c0 + ct * 16 : 0) : 0;

  // one k-block of the strip in registers: 16-B row chunks, coalesced (Y: 32 x 16 chunks, T: 32 x tc <= 768 chunks)
  u32x4 yr[2], tr[3];
  auto load_kb = [&](int64_t kb) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i, m = idx >> 4, ch = idx & 15;
      const int64_t mm = kb * 32 + m, c = cblk + 8 * ch;
      yr[i] = u32x4{0u, 0u, 0u, 0u};
      if (mm < M && c < W) yr[i] = *reinterpret_cast<const u32x4*>(Y + mm * ldy + c);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int idx = tid + 256 * i, m = idx / tc, ch = idx - m * tc;
      const int64_t mm = kb * 32 + m;
      tr[i] = u32x4{0u, 0u, 0u, 0u};
      if (idx < 32 * tc && mm < M && ((8 * ch) & (S.R - 1)) < S.r)  // columns r..R-1 of a slice are never read
        tr[i] = *reinterpret_cast<const u32x4*>(T + mm * ldt + 8 * ch);
    }
  };
  auto store_kb = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i, m = idx >> 4, ch = idx & 15;
#pragma unroll
      for (int e = 0; e < 8; ++e) Yt[8 * ch + e][m] = (bf16_t)(yr[i][e >> 1] >> (16 * (e & 1)));
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int idx = tid + 256 * i, m = idx / tc, ch = idx - m * tc;
      if (idx < 32 * tc) {
#pragma unroll
        for (int e = 0; e < 8; ++e) Tt[8 * ch + e][m] = (bf16_t)(tr[i][e >> 1] >> (16 * (e & 1)));
      }
    }
  };

  if (kb0 < kb1) load_kb(kb0);
  for (int64_t kb = kb0; kb < kb1; ++kb) {
    __syncthreads();  // the previous k-block's fragments are read
    store_kb();
    __syncthreads();
    if (kb + 1 < kb1) load_kb(kb + 1);  // in flight while this k-block's MFMAs run
    if (!wave_on) continue;
    bf16x8 yf[WG_CT];
#pragma unroll
    for (int ct = 0; ct < WG_CT; ++ct)
      yf[ct] = *reinterpret_cast<const bf16x8*>(&Yt[w * (WG_CT * 16) + ct * 16 + mi][8 * g]);
    if constexpr (!SLICED) {
#pragma unroll
      for (int s = 0; s < MAX_SEG; ++s) {
        if (s >= S.nseg) continue;
#pragma unroll
        for (int t = 0; t < TPS; ++t) {
          if (t >= tps) continue;
          const bf16x8 tf = *reinterpret_cast<const bf16x8*>(&Tt[s * S.R + t * 16 + mi][8 * g]);
#pragma unroll
          for (int ct = 0; ct < WG_CT; ++ct) acc[ct][s * TPS + t] = mfma(yf[ct], tf, acc[ct][s * TPS + t]);
        }
      }
    } else {
#pragma unroll
      for (int ct = 0; ct < WG_CT; ++ct)
#pragma unroll
        for (int t = 0; t < TPS; ++t) {
          if (t >= tps) continue;
          const bf16x8 tf = *reinterpret_cast<const bf16x8*>(&Tt[sct[ct] * S.R + t * 16 + mi][8 * g]);
          acc[ct][t] = mfma(tf, yf[ct], acc[ct][t]);
        }
    }
  }
  if (!wave_on) return;
  if constexpr (!SLICED) {
    float* Pp = P + (int64_t)blockIdx.y * (S.nseg * S.R) * Wp;
#pragma unroll
    for (int s = 0; s < MAX_SEG; ++s) {
      if (s >= S.nseg) continue;
#pragma unroll
      for (int t = 0; t < TPS; ++t) {
        if (t >= tps) continue;
#pragma unroll
        for (int ct = 0; ct < WG_CT; ++ct)  // lane: rank row j = t 16 + mi, columns c0 + ct 16 + 4 g .. + 3 (< Wp)
          *reinterpret_cast<f32x4*>(Pp + (int64_t)(s * S.R + t * 16 + mi) * Wp + c0 + ct * 16 + 4 * g) =
              acc[ct][s * TPS + t];
      }
    }
  } else {
    float* Pp = P + (int64_t)blockIdx.y * Wp * S.R;
#pragma unroll
    for (int ct = 0; ct < WG_CT; ++ct)
#pragma unroll
      for (int t = 0; t < TPS; ++t) {
        if (t >= tps) continue;  // lane: column row c0 + ct 16 + mi (< Wp), rank columns t 16 + 4 g .. + 3
        *reinterpret_cast<f32x4*>(Pp + (c0 + ct * 16 + mi) * S.R + t * 16 + 4 * g) = acc[ct][t];
      }
  }
}

// out = bf16([out +] alpha * sum over the row slices, in slice order); one thread = 8 consecutive output elements
template <bool SLICED>
__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(int64_t W, int64_t Wp, Segs S, int split,
                                                                const float* __restrict__ P, float alpha,
                                                                int accumulate) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float* src;
  bf16_t* dst;
  int64_t pstride;
  if constexpr (!SLICED) {
    const int64_t w8 = W >> 3;
    if (idx >= (int64_t)S.nseg * S.r * w8) return;
    const int s = (int)(idx / (S.r * w8));
    const int64_t rem = idx % (S.r * w8), j = rem / w8, c = (rem % w8) * 8;
    src = P + ((int64_t)s * S.R + j) * Wp + c;
    dst = const_cast<bf16_t*>(seg_p(S, s)) + j * W + c;
    pstride = (int64_t)S.nseg * S.R * Wp;
  } else {
    const int r8 = S.r >> 3;
    if (idx >= W * r8) return;
    const int64_t c = idx / r8;
    const int j = (int)(idx % r8) * 8;
    const int s = seg_of(S, c);
    src = P + c * S.R + j;
    dst = const_cast<bf16_t*>(seg_p(S, s)) + (c - seg_st(S, s)) * S.r + j;
    pstride = Wp * S.R;
  }
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = 0.f;
  for (int p = 0; p < split; ++p) {
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(src + p * pstride);
    const f32x4 x1 = *reinterpret_cast<const f32x4*>(src + p * pstride + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] += x0[e]; v[4 + e] += x1[e]; }
  }
  float o[8];
  if (accumulate) unpack8(*reinterpret_cast<const u32x4*>(dst), o);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = alpha * v[e] + (accumulate ? o[e] : 0.f);
  *reinterpret_cast<u32x4*>(dst) = pack8(v);
}

// ------------------------------------------------------------------------------------------------ host side
int64_t round_up64(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// byte ranges [a, a + na) and [b, b + nb) share a byte
bool overlaps(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

// checks shared by the three entry points; fills S (every pointer 16-B aligned: fragments are 16-B loads)
int make_segs(const char* what, const svla_lora_segs* in, Segs& S, bool need_starts, int64_t extent, int64_t start_mult) {
  SVLA_CHECK_ARG(in != nullptr, "%s: segment list is NULL", what);
  SVLA_CHECK_ARG(in->nseg >= 1 && in->nseg <= MAX_SEG, "%s: 1..3 segments, got %d", what, in->nseg);
  SVLA_CHECK_ARG(in->r >= 8 && in->r <= MAX_R && in->r % 8 == 0, "%s: rank must be a multiple of 8 in [8, 64], got %d",
                 what, in->r);
  SVLA_CHECK_ARG(in->ld > 0 && in->ld % 8 == 0, "%s: the small matrices' ld must be a positive multiple of 8, got %lld",
                 what, (long long)in->ld);
  S.nseg = in->nseg;
  S.r = in->r;
  S.R = (int)round_up64(in->r, 32);
  S.ld = in->ld;
  for (int s = 0; s < MAX_SEG; ++s) {
    S.p[s] = s < in->nseg ? (const bf16_t*)in->ptr[s] : nullptr;
    SVLA_CHECK_ARG(s >= in->nseg || (S.p[s] != nullptr && aligned16(S.p[s])), "%s: segment %d pointer NULL or not 16-B aligned",
                   what, s);
  }
  for (int s = 0; s <= MAX_SEG; ++s) S.st[s] = 0;
  if (need_starts) {
    SVLA_CHECK_ARG(in->start[0] == 0 && in->start[in->nseg] == extent,
                   "%s: segment starts must run from 0 to %lld", what, (long long)extent);
    for (int s = 0; s < in->nseg; ++s)
      SVLA_CHECK_ARG(in->start[s + 1] > in->start[s] && in->start[s] % start_mult == 0,
                     "%s: segment starts must ascend and be multiples of %lld", what, (long long)start_mult);
    for (int s = 0; s <= in->nseg; ++s) S.st[s] = in->start[s];
  }
  return SVLA_OK;
}

// Row slices of svla_lora_wgrad: enough workgroups for ~8 per CU (a wave's k-steps are serial load -> MFMA rounds, so
// the loads in flight come from resident waves), at most 64 slices, and at most 32 MiB of fp32 partials (they are
// written and read once: traffic beside the one pass over Y).  A function of the shapes only: the sum order is fixed.
int64_t wgrad_split(int64_t M, int64_t W, int64_t out_rows_x_cols, int64_t* per_out) {
  const int64_t strips = (W + WG_COLS - 1) / WG_COLS, nkb = (M + 31) / 32;
  int64_t split = 2048 / strips;
  const int64_t cap = (32ll << 20) / (out_rows_x_cols * 4);
  if (split > cap) split = cap;
  split = split < 1 ? 1 : (split > 64 ? 64 : split);
  if (split > nkb) split = nkb;
  const int64_t per = (nkb + split - 1) / split;
  if (per_out) *per_out = per;
  return (nkb + per - 1) / per;
}

}  // namespace

extern "C" int svla_lora_down(int64_t M, int64_t K, const void* x, int64_t ldx, const svla_lora_segs* segs, int32_t mode,
                              float alpha, void* t, int64_t ldt, void* stream) {
  SVLA_CHECK_ARG(mode == SVLA_LORA_SHARED || mode == SVLA_LORA_SLICED, "lora_down: mode must be SHARED or SLICED");
  SVLA_CHECK_ARG(M >= 1 && K >= 8 && K % 8 == 0, "lora_down: M >= 1 and K a positive multiple of 8 (M %lld, K %lld)",
                 (long long)M, (long long)K);
  SVLA_CHECK_ARG(x && t && aligned16(x) && aligned16(t), "lora_down: x / t NULL or not 16-B aligned");
  SVLA_CHECK_ARG(ldx % 8 == 0 && ldx >= K, "lora_down: ldx must be a multiple of 8 and >= K, got %lld", (long long)ldx);
  Segs S;
  const int rc = make_segs("lora_down", segs, S, mode == SVLA_LORA_SLICED, K, 8);
  if (rc != SVLA_OK) return rc;
  SVLA_CHECK_ARG(ldt % 8 == 0 && ldt >= (int64_t)S.nseg * S.R, "lora_down: ldt must be a multiple of 8 and >= nseg * R = %d",
                 S.nseg * S.R);
  SVLA_CHECK_ARG(mode == SVLA_LORA_SLICED ? S.ld >= S.r : S.ld >= K, "lora_down: the small matrices' ld is below their width");
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(64 * DOWN_NW);
  if (mode == SVLA_LORA_SHARED)
    hipLaunchKernelGGL(lora_down_kernel<false>, dim3((unsigned)((M + 16 * DOWN_RB - 1) / (16 * DOWN_RB))), block, 0, s, M,
                       K, (const bf16_t*)x, ldx, S, alpha, (bf16_t*)t, ldt);
  else
    hipLaunchKernelGGL(lora_down_kernel<true>, dim3((unsigned)((M + 15) / 16)), block, 0, s, M, K, (const bf16_t*)x, ldx,
                       S, alpha, (bf16_t*)t, ldt);
  return svla::check_launch("lora_down");
}

extern "C" int svla_lora_up(int64_t M, int64_t N, void* c, int64_t ldc, const void* t, int64_t ldt,
                            const svla_lora_segs* segs, int32_t mode, float alpha, const svla_lora_epilogue* epi,
                            void* stream) {
  SVLA_CHECK_ARG(mode == SVLA_LORA_SLICED || mode == SVLA_LORA_SUMMED, "lora_up: mode must be SLICED or SUMMED");
  SVLA_CHECK_ARG(M >= 1 && N >= 8 && N % 8 == 0, "lora_up: M >= 1 and N a positive multiple of 8 (M %lld, N %lld)",
                 (long long)M, (long long)N);
  SVLA_CHECK_ARG(c && t && aligned16(c) && aligned16(t), "lora_up: c / t NULL or not 16-B aligned");
  SVLA_CHECK_ARG(ldc % 8 == 0 && ldc >= N, "lora_up: ldc must be a multiple of 8 and >= N, got %lld", (long long)ldc);
  Segs S;
  const int rc = make_segs("lora_up", segs, S, mode == SVLA_LORA_SLICED, N, 16);
  if (rc != SVLA_OK) return rc;
  SVLA_CHECK_ARG(ldt % 8 == 0 && ldt >= (int64_t)(S.nseg - 1) * S.R + S.r,
                 "lora_up: ldt must be a multiple of 8 and cover (nseg - 1) * R + r columns, got %lld", (long long)ldt);
  SVLA_CHECK_ARG(mode == SVLA_LORA_SLICED ? S.ld >= S.r : S.ld >= N, "lora_up: the small matrices' ld is below their width");
  const int kind = epi ? epi->kind : SVLA_LORA_EPI_NONE;
  SVLA_CHECK_ARG(mode == SVLA_LORA_SLICED || kind == SVLA_LORA_EPI_NONE,
                 "lora_up: the epilogues belong to the sliced (forward) mode");
  UpEpi E = {};
  int64_t nunits = (N + 31) / 32;
  if (kind == SVLA_LORA_EPI_ROPE) {
    SVLA_CHECK_ARG(epi->rope_cos && epi->rope_sin && epi->rope_L > 0 && epi->rope_D >= 32 && epi->rope_D % 32 == 0 &&
                       epi->rope_ld % 8 == 0 && epi->rope_ld >= epi->rope_D / 2 && epi->rope_cols >= 0 &&
                       epi->rope_cols % epi->rope_D == 0 && epi->rope_cols <= N && aligned16(epi->rope_cos) &&
                       aligned16(epi->rope_sin),
                   "lora_up: ROPE needs 16-B aligned cos/sin tables, rope_L, rope_D a multiple of 32, rope_cols a multiple of D");
    E.cos = (const bf16_t*)epi->rope_cos;
    E.sin = (const bf16_t*)epi->rope_sin;
    E.rope_ld = epi->rope_ld;
    E.rope_cols = epi->rope_cols;
    E.rope_L = epi->rope_L;
    E.rope_D = epi->rope_D;
    nunits = (epi->rope_cols / epi->rope_D) * (epi->rope_D / 32) + (N - epi->rope_cols + 31) / 32;
  } else if (kind == SVLA_LORA_EPI_GEGLU) {
    SVLA_CHECK_ARG(mode == SVLA_LORA_SLICED && S.nseg == 2 && S.st[1] == N / 2 && epi->h && aligned16(epi->h) &&
                       epi->ldh % 8 == 0 && epi->ldh >= N / 2,
                   "lora_up: GEGLU needs sliced mode with the gate | up segments of N/2 columns and an h output");
    E.h = (bf16_t*)epi->h;
    E.ldh = epi->ldh;
    nunits = (N / 2 + 15) / 16;
    if (epi->mx_q) {  // + the MX e4m3 copy of h: a wave takes a whole 32-column block
      SVLA_CHECK_ARG(epi->mx_scales && (N / 2) % 128 == 0 && epi->mx_ldq >= N / 2 && epi->mx_ldq % 8 == 0 &&
                         ((uintptr_t)epi->mx_q & 7) == 0 && ((uintptr_t)epi->mx_scales & 3) == 0 &&
                         epi->mx_sld >= 4 * M && epi->mx_sld % 4 == 0,
                     "lora_up: GEGLU MX copy of h: N/2 % 128 == 0, mx_ldq >= N/2 (8-B rows), mx_sld >= 4 M");
      // the kernel's pointers are __restrict__: the copy and its scales may share no byte with g | u, h or each other
      const int64_t cb = ((M - 1) * ldc + N) * 2, hb = ((M - 1) * epi->ldh + N / 2) * 2;
      const int64_t qb = (M - 1) * epi->mx_ldq + N / 2, sb = (N / 256) * epi->mx_sld;
      SVLA_CHECK_ARG(!overlaps(epi->mx_q, qb, c, cb) && !overlaps(epi->mx_q, qb, epi->h, hb) &&
                         !overlaps(epi->mx_scales, sb, c, cb) && !overlaps(epi->mx_scales, sb, epi->h, hb) &&
                         !overlaps(epi->mx_q, qb, epi->mx_scales, sb),
                     "lora_up: mx_q / mx_scales overlap c, h or each other");
      nunits = N / 64;
    }
  } else if (kind == SVLA_LORA_EPI_GELU) {
    // the kernel's pointers are __restrict__ and a lane stores h beside C: h may share no byte with C
    SVLA_CHECK_ARG(S.nseg == 1 && epi->h && aligned16(epi->h) && epi->ldh % 8 == 0 && epi->ldh >= N,
                   "lora_up: GELU needs one segment and a 16-B aligned h output with ldh % 8 == 0, ldh >= N");
    SVLA_CHECK_ARG(!overlaps(epi->h, ((M - 1) * epi->ldh + N) * 2, c, ((M - 1) * ldc + N) * 2),
                   "lora_up: GELU: h overlaps c");
    E.h = (bf16_t*)epi->h;
    E.ldh = epi->ldh;
  } else if (kind == SVLA_LORA_EPI_RESID) {
    SVLA_CHECK_ARG(epi->res && aligned16(epi->res) && epi->ldres % 8 == 0 && epi->ldres >= N,
                   "lora_up: RESID needs a 16-B aligned res with ldres % 8 == 0, ldres >= N");
    SVLA_CHECK_ARG(!overlaps(epi->res, ((M - 1) * epi->ldres + N) * 2, c, ((M - 1) * ldc + N) * 2),
                   "lora_up: RESID: res overlaps c");
    E.res = (const bf16_t*)epi->res;
    E.ldres = epi->ldres;
  } else if (kind == SVLA_LORA_EPI_SCALE) {
    E.post = epi->post;
  } else {
    SVLA_CHECK_ARG(kind == SVLA_LORA_EPI_NONE, "lora_up: unknown epilogue %d", kind);
  }
  SVLA_CHECK_ARG(kind == SVLA_LORA_EPI_GEGLU || !epi || !epi->mx_q, "lora_up: the MX copy (epi->mx_q) is a GEGLU output");
  hipStream_t s = (hipStream_t)stream;
  const int64_t gx = (nunits + 3) / 4, nrb = (M + 15) / 16;
  int64_t gy = (8 * (int64_t)svla::num_cus() + gx - 1) / gx;
  gy = gy < 1 ? 1 : (gy > nrb ? nrb : gy);
  const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
  if (kind == SVLA_LORA_EPI_GEGLU && epi->mx_q) {
    hipLaunchKernelGGL(lora_up_geglu_mx_kernel, grid, block, 0, s, M, N, (bf16_t*)c, ldc, (const bf16_t*)t, ldt, S, alpha,
                       E.h, E.ldh, (uint8_t*)epi->mx_q, epi->mx_ldq, (uint8_t*)epi->mx_scales, epi->mx_sld);
    return svla::check_launch("lora_up");
  }
#define SVLA_UP(SUMMED_, EPI_)                                                                                       \
  hipLaunchKernelGGL((lora_up_kernel<SUMMED_, EPI_>), grid, block, 0, s, M, N, (bf16_t*)c, ldc, (const bf16_t*)t, ldt, S, \
                     alpha, E, nunits)
  if (mode == SVLA_LORA_SUMMED) {
    SVLA_UP(true, UP_NONE);
  } else {
    if (kind == SVLA_LORA_EPI_ROPE) SVLA_UP(false, UP_ROPE);
    else if (kind == SVLA_LORA_EPI_GEGLU) SVLA_UP(false, UP_GEGLU);
    else if (kind == SVLA_LORA_EPI_GELU) SVLA_UP(false, UP_GELU);
    else if (kind == SVLA_LORA_EPI_RESID) SVLA_UP(false, UP_RESID);
    else if (kind == SVLA_LORA_EPI_SCALE) SVLA_UP(false, UP_SCALE);
    else SVLA_UP(false, UP_NONE);
  }
#undef SVLA_UP
  return svla::check_launch("lora_up");
}

extern "C" size_t svla_lora_wgrad_workspace_bytes(int64_t M, int64_t W, int32_t mode, int32_t nseg, int32_t r) {
  if (M < 1 || W < 1 || nseg < 1 || nseg > MAX_SEG || r < 8 || r > MAX_R) return 0;
  const int64_t Wp = round_up64(W, WG_COLS), R = round_up64(r, 32);
  const int64_t elems = Wp * R * (mode == SVLA_LORA_SLICED ? 1 : nseg);
  return (size_t)(wgrad_split(M, W, elems, nullptr) * elems) * sizeof(float);
}

extern "C" int svla_lora_wgrad(int64_t M, int64_t W, const void* y, int64_t ldy, const void* t, int64_t ldt, int32_t mode,
                               const svla_lora_segs* outs, float alpha, int32_t accumulate, void* workspace,
                               size_t ws_bytes, void* stream) {
  SVLA_CHECK_ARG(mode == SVLA_LORA_SHARED || mode == SVLA_LORA_SLICED, "lora_wgrad: mode must be SHARED or SLICED");
  SVLA_CHECK_ARG(M >= 1 && W >= 8 && W % 8 == 0, "lora_wgrad: M >= 1 and W a positive multiple of 8 (M %lld, W %lld)",
                 (long long)M, (long long)W);
  SVLA_CHECK_ARG(y && t && aligned16(y) && aligned16(t), "lora_wgrad: y / t NULL or not 16-B aligned");
  SVLA_CHECK_ARG(ldy % 8 == 0 && ldy >= W, "lora_wgrad: ldy must be a multiple of 8 and >= W, got %lld", (long long)ldy);
  Segs S;
  const int rc = make_segs("lora_wgrad", outs, S, mode == SVLA_LORA_SLICED, W, 16);
  if (rc != SVLA_OK) return rc;
  SVLA_CHECK_ARG(mode == SVLA_LORA_SLICED ? S.ld == S.r : S.ld == W,
                 "lora_wgrad: the outputs are dense ([r][W] shared, [W_s][r] sliced); ld %lld", (long long)S.ld);
  SVLA_CHECK_ARG(ldt % 8 == 0 && ldt >= (int64_t)S.nseg * S.R, "lora_wgrad: ldt must be a multiple of 8 and >= nseg * R = %d",
                 S.nseg * S.R);
  const size_t need = svla_lora_wgrad_workspace_bytes(M, W, mode, S.nseg, S.r);
  SVLA_CHECK_ARG(workspace && aligned16(workspace) && ws_bytes >= need,
                 "lora_wgrad: workspace NULL, misaligned or below svla_lora_wgrad_workspace_bytes() = %zu", need);
  int64_t per = 0;
  const int64_t Wp = round_up64(W, WG_COLS);
  const int64_t split = wgrad_split(M, W, Wp * S.R * (mode == SVLA_LORA_SLICED ? 1 : S.nseg), &per);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(Wp / WG_COLS), (unsigned)split), block(256);
  float* P = (float*)workspace;
  if (mode == SVLA_LORA_SHARED) {
    hipLaunchKernelGGL(lora_wgrad_kernel<false>, grid, block, 0, s, M, W, (const bf16_t*)y, ldy, (const bf16_t*)t, ldt, S,
                       P, Wp, per);
    const int64_t n = (int64_t)S.nseg * S.r * (W / 8);
    hipLaunchKernelGGL(lora_wgrad_reduce_kernel<false>, dim3((unsigned)((n + 255) / 256)), block, 0, s, W, Wp, S,
                       (int)split, (const float*)P, alpha, (int)accumulate);
  } else {
    hipLaunchKernelGGL(lora_wgrad_kernel<true>, grid, block, 0, s, M, W, (const bf16_t*)y, ldy, (const bf16_t*)t, ldt, S,
                       P, Wp, per);
    const int64_t n = W * (S.r / 8);
    hipLaunchKernelGGL(lora_wgrad_reduce_kernel<true>, dim3((unsigned)((n + 255) / 256)), block, 0, s, W, Wp, S,
                       (int)split, (const float*)P, alpha, (int)accumulate);
  }
  return svla::check_launch("lora_wgrad");
}
