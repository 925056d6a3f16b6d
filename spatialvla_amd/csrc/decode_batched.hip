// Batched decode projections for gfx950 (MI355X): svla_gemm_skinny (include/svla.h), y[M, N] = x[M, K] W^T for
// 1 <= M <= 64 token rows in bf16 with fp32 accumulation on v_mfma_f32_16x16x32_bf16.
//
// The GEMVs of the decode step (gemm.hip gemv_pf_kernel and its siblings) spend M N K fp32 FMAs on the VALU and stop
// at 8 rows; the tiled GEMMs zero-fill three quarters of a 64-row tile at 16 rows and reach the CUs of the narrow
// projections only through cross-block split-K slabs.  Here the weight stream feeds the MFMA directly:
//   - the first MFMA operand is a 16-row block of W.  Lane l holds W[n0 + (l & 15)][k0 + 8 (l >> 4) .. + 7], which is
//     one 16-B piece of row-major W: a 16-B non-temporal load lands in the fragment registers, no LDS image of W, and
//     every weight byte is read exactly once per launch;
//   - the second operand is x: lane l holds x[16 t + (l & 15)][the same k] for each of the ceil(M / 16) row tiles t,
//     read in the same fragment shape from L2 (x is at most 64 rows and is re-read by every block; it is not staged
//     through LDS).  C^T is accumulated, so a lane owns token row (l & 15) and the four consecutive output columns
//     4 (l >> 4) .. + 3;
//   - a wave walks its k-steps in ranges (sk_range) whose issue order is pinned: the x fragments of the range, every
//     weight load of the range, then the MFMAs.  The range is as deep as the registers allow, 32 / (row tiles + 1)
//     k-steps rounded down to a power of two (16 at <= 16 rows, 8 at <= 48, 4 at 64; half that in the 16-wave form);
//   - a workgroup owns one 16-column block of y and its waves split K into contiguous runs of k-steps; the partial
//     tiles meet in LDS and are added in wave order.  Weights with fewer 16-row blocks than CUs (o: 144) use 16 waves a
//     workgroup instead of 4, so the reduction never leaves the workgroup: no workspace, no tickets, no block waits
//     for another.
// Batch invariance: the column blocks, the wave count and each wave's k range depend on (N, K) only, and a token row
// is one column of the MFMA's second operand, which no other column touches -- row m of y has the same bits for every
// M and every position of that row in the batch.  M only decides how many row tiles are computed and how the k-steps
// are grouped into ranges, not their order.
// Built for, and measured on, the small latency-bound projections of the step (q|k|v, o).  On the large ones (gate|up,
// down, lm_head) an earlier form with a GEGLU epilogue lost to the tiled GEMM at every row count
// (profiles/batched_decode_ab.txt), so there is no GEGLU form and the model does not route them.
// fp32 in a fixed order, no atomics, no allocation, no host synchronisation (graph-capturable).
#include "svla_common.h"

namespace {

constexpr int SK_MAXM = 64;
constexpr int SK_MAXSEG = 3;
constexpr int SK_NW_WIDE = 4;     // waves per workgroup where the column blocks alone fill the CUs
constexpr int SK_NW_NARROW = 16;  // ... and where they do not (o: 144 blocks)

struct SkRows {  // svla_bf16_rows with typed pointers
  const bf16_t *w0, *w1, *w2;
  int64_t st1, st2;
  int64_t ldw;
  int nseg;
};

__device__ __forceinline__ f32x4 sk_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 sk_ldw(const bf16_t* p) {
  return __builtin_bit_cast(bf16x8, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)));
}
__device__ __forceinline__ bf16x8 sk_ldx(const bf16_t* p) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(p));
}
// row n of a weight of up to three row segments (q|k|v); n differs from lane to lane
__device__ __forceinline__ const bf16_t* sk_row(const SkRows& W, int64_t n) {
  const int sg = (int)(W.nseg > 1 && n >= W.st1) + (int)(W.nseg > 2 && n >= W.st2);
  const bf16_t* b = sg == 0 ? W.w0 : (sg == 1 ? W.w1 : W.w2);
  const int64_t r = n - (sg == 0 ? 0 : (sg == 1 ? W.st1 : W.st2));
  return b + r * W.ldw;
}

constexpr int sk_pow2_floor(int v) { return v >= 16 ? 16 : (v >= 8 ? 8 : (v >= 4 ? 4 : 2)); }

// UU k-steps from step s on.  The issue order is pinned (sched_barrier: nothing moves across): first the x fragments
// of the whole range (L2 hits, back first -- vmcnt counts returns in issue order, so an x load issued behind the weight
// loads would make the first MFMA wait for all of them), then every weight load of the range, then the MFMAs, each
// waiting only for its own weight fragment.  Left to itself the scheduler sinks the weight loads between the MFMAs
// and a wave has a few of them in flight instead of UU.
template <int UU, int MT>
__device__ __forceinline__ void sk_range(const bf16_t* wp, const bf16_t* const (&xp)[MT], int64_t s, f32x4 (&acc)[MT]) {
  bf16x8 xf[UU][MT], wf[UU];
#pragma unroll
  for (int j = 0; j < UU; ++j)
#pragma unroll
    for (int m = 0; m < MT; ++m) xf[j][m] = sk_ldx(xp[m] + (s + j) * 32);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < UU; ++j) wf[j] = sk_ldw(wp + (s + j) * 32);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < UU; ++j)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = sk_mfma(wf[j], xf[j][m], acc[m]);
  __builtin_amdgcn_sched_barrier(0);
}

// NWV waves; MT row tiles of 16 token rows
template <int NWV, int MT>
__global__ __launch_bounds__(64 * NWV) void sk_kernel(int M, int64_t N, int64_t K, const bf16_t* __restrict__ x,
                                                      int64_t ldx, SkRows W, bf16_t* __restrict__ y, int64_t ldy) {
  // k-steps per range: the x and weight fragments of a range are all live at once, UU (MT + 1) x 4 VGPRs, held to
  // 128 (64 in the 1024-thread form, whose lanes have 128 VGPRs in all)
  constexpr int MAXU = sk_pow2_floor((NWV > SK_NW_WIDE ? 16 : 32) / (MT + 1));
  __shared__ __attribute__((aligned(16))) f32x4 red[NWV][MT][64];  // the waves' partial tiles: at most 64 KB
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * 16;
  // this wave's contiguous run of k-steps: a function of K and NWV only
  const int64_t T = K >> 5, q = T / NWV, r = T % NWV;
  const int64_t ns = q + (w < r ? 1 : 0), s0 = w * q + (w < r ? w : r);
  const int64_t nr = n0 + i < N ? n0 + i : N - 1;  // clamped: the stores are masked
  const bf16_t* wp = sk_row(W, nr) + s0 * 32 + g * 8;
  const bf16_t* xp[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mr = m * 16 + i < M ? m * 16 + i : M - 1;  // clamped: a column of the second operand feeds only itself
    xp[m] = x + (int64_t)mr * ldx + s0 * 32 + g * 8;
  }
  f32x4 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  int64_t s = 0;
  for (; s + MAXU <= ns; s += MAXU) sk_range<MAXU, MT>(wp, xp, s, acc);
  if constexpr (MAXU > 8) {
    if (ns - s >= 8) { sk_range<8, MT>(wp, xp, s, acc); s += 8; }
  }
  if constexpr (MAXU > 4) {
    if (ns - s >= 4) { sk_range<4, MT>(wp, xp, s, acc); s += 4; }
  }
  if constexpr (MAXU > 2) {
    if (ns - s >= 2) { sk_range<2, MT>(wp, xp, s, acc); s += 2; }
  }
  if (ns - s >= 1) { sk_range<1, MT>(wp, xp, s, acc); s += 1; }
#pragma unroll
  for (int m = 0; m < MT; ++m) red[w][m][lane] = acc[m];
  __syncthreads();
  if (w >= MT) return;  // wave w finishes row tile w (NWV >= 4 >= MT)
  f32x4 v = red[0][w][lane];
#pragma unroll
  for (int ww = 1; ww < NWV; ++ww) v += red[ww][w][lane];
  const int m = w * 16 + i;
  const int64_t n = n0 + 4 * g;
  if (m >= M || n >= N) return;
  bf16_t* p = y + (int64_t)m * ldy + n;  // 8-B aligned: y 16-B aligned, ldy % 8 == 0, n % 4 == 0
  if (N - n >= 4) {
    *reinterpret_cast<u32x2*>(p) = u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])};
  } else {
    for (int e = 0; e < (int)(N - n); ++e) p[e] = f2bf(v[e]);
  }
}

bool sk_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int NWV>
void sk_launch(int mt, unsigned blocks, hipStream_t s, int M, int64_t N, int64_t K, const bf16_t* x, int64_t ldx,
               const SkRows& R, bf16_t* y, int64_t ldy) {
  const dim3 grid(blocks), block(64 * NWV);
  if (mt == 1) hipLaunchKernelGGL((sk_kernel<NWV, 1>), grid, block, 0, s, M, N, K, x, ldx, R, y, ldy);
  else if (mt == 2) hipLaunchKernelGGL((sk_kernel<NWV, 2>), grid, block, 0, s, M, N, K, x, ldx, R, y, ldy);
  else if (mt == 3) hipLaunchKernelGGL((sk_kernel<NWV, 3>), grid, block, 0, s, M, N, K, x, ldx, R, y, ldy);
  else hipLaunchKernelGGL((sk_kernel<NWV, 4>), grid, block, 0, s, M, N, K, x, ldx, R, y, ldy);
}

}  // namespace

extern "C" int svla_gemm_skinny(int64_t M, int64_t N, int64_t K, const void* x, int64_t ldx, const svla_bf16_rows* W,
                                void* y, int64_t ldy, void* stream) {
  SVLA_CHECK_ARG(M >= 1 && M <= SK_MAXM && N >= 1 && K >= 32 && K % 32 == 0,
                 "gemm_skinny: M in [1, %d], N >= 1, K a positive multiple of 32 (M %lld, N %lld, K %lld)", SK_MAXM,
                 (long long)M, (long long)N, (long long)K);
  SVLA_CHECK_ARG(x && W && y && sk_al16(x) && sk_al16(y), "gemm_skinny: NULL argument, or x / y not 16-B aligned");
  SVLA_CHECK_ARG(ldx % 8 == 0 && ldx >= K && ldy % 8 == 0 && ldy >= N,
                 "gemm_skinny: ldx a multiple of 8 >= K, ldy a multiple of 8 >= N");
  SVLA_CHECK_ARG(W->nseg >= 1 && W->nseg <= SK_MAXSEG && W->ldw % 8 == 0 && W->ldw >= K,
                 "gemm_skinny: 1..3 weight segments, ldw a multiple of 8 >= K");
  SVLA_CHECK_ARG(W->start[0] == 0 && W->start[W->nseg] == N, "gemm_skinny: segment starts must run from 0 to N");
  const bf16_t* rw[SK_MAXSEG] = {nullptr, nullptr, nullptr};
  int64_t rst[SK_MAXSEG] = {0, 0, 0};
  for (int s = 0; s < W->nseg; ++s) {
    SVLA_CHECK_ARG(W->w[s] && sk_al16(W->w[s]), "gemm_skinny: segment %d NULL or not 16-B aligned", s);
    SVLA_CHECK_ARG(W->start[s + 1] > W->start[s], "gemm_skinny: segment starts must ascend");
    rw[s] = (const bf16_t*)W->w[s];
    rst[s] = W->start[s];
  }
  const SkRows R = {rw[0], rw[1], rw[2], rst[1], rst[2], W->ldw, W->nseg};
  const int64_t blocks = (N + 15) / 16;
  SVLA_CHECK_ARG(blocks < (1ll << 31), "gemm_skinny: N too large");
  const int mt = (int)((M + 15) / 16);
  // the wave count is a function of N (the 16-row weight blocks against the CUs), never of M
  if (blocks >= svla::num_cus())
    sk_launch<SK_NW_WIDE>(mt, (unsigned)blocks, (hipStream_t)stream, (int)M, N, K, (const bf16_t*)x, ldx, R, (bf16_t*)y,
                          ldy);
  else
    sk_launch<SK_NW_NARROW>(mt, (unsigned)blocks, (hipStream_t)stream, (int)M, N, K, (const bf16_t*)x, ldx, R,
                            (bf16_t*)y, ldy);
  return svla::check_launch("gemm_skinny");
}
