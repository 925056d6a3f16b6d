// svla_sample_rows: one token per row of softcapped bf16 logits, drawn by Gumbel-max under an allowed column range,
// temperature, top-k and top-p, with the token's log-probabilities (include/svla.h states the semantics; the numpy
// restatement is tests/sample_ref.py).
//
// One workgroup of 512 threads per row.  Nothing of a row's result depends on another row, on M or on the grid:
//  * the kept set comes from integer counts per distinct bf16 value (a 32768-bin LDS histogram per sign half of the
//    ordered 16-bit key, integer LDS atomics) and from masses count * round(2^40 exp((v - vmax)/T)) in uint64 --
//    integer sums, so their order does not matter;
//  * the draw is a maximum over packed (score, column) keys -- order-free as well;
//  * the two float sums (the raw log-sum-exp over all N columns, and the kept mass when nothing is filtered) are taken
//    per thread over a fixed column assignment in double and combined in a fixed order.
// No float atomics, no workspace, no cross-workgroup traffic.
#include <math.h>

#include "svla_common.h"

namespace {

constexpr int SR_THREADS = 512;   // 117 VGPRs, no scratch (1024 threads cap at 128 and spill)
constexpr int SR_WAVES = SR_THREADS / 64;
constexpr int SR_BINS = 32768;                     // keys of one sign half
constexpr int SR_PER = SR_BINS / SR_THREADS;       // bins a thread scans (64, contiguous, descending)
constexpr int SR_HIST = SR_BINS + SR_THREADS;     // one pad dword per thread's run of bins: the scan's strided reads spread over the banks
constexpr int SR_LDS = SR_HIST * 4;                // 133120 B of dynamic LDS
constexpr double SR_FIX = 1099511627776.0;         // 2^40: fixed-point scale of the masses
constexpr int64_t SR_MAX_N = (int64_t)1 << 22;     // N * 2^40 < 2^63

// ordered 16-bit key of a bf16: a larger value has a larger key; -0 < +0; NaNs sit beyond the infinities
__device__ __forceinline__ uint32_t okey(uint32_t b) { return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u); }
__device__ __forceinline__ float key_value(uint32_t k) {
  const uint32_t b = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
  return __uint_as_float(b << 16);
}
__device__ __forceinline__ bool bf_isnan(uint32_t b) { return (b & 0x7fffu) > 0x7f80u; }
__device__ __forceinline__ int hphys(int j) { return j + j / SR_PER; }

// Philox4x32-10 (Salmon et al., SC'11; Random123's constants)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// Gumbel noise of one 32-bit word: u = ((w >> 8) + 0.5) 2^-24, g = -log(-log u).  Both logs are libm's (logf /
// log1pf, ~1 ulp): the winners have u near 1, where -log u ~ 6e-8 and a fast log's absolute error would move g by
// O(1).  Above 1/2, u = 1 - d with d = (2^24 - (w >> 8) - 0.5) 2^-24 exact in fp32 (u itself is not), so -log u is
// taken as -log1p(-d).
__device__ __forceinline__ float gumbel(uint32_t w) {
  const uint32_t i = w >> 8;
  float a;
  if (i < (1u << 23)) {
    a = -logf(((float)i + 0.5f) * 0x1p-24f);
  } else {
    a = -log1pf(-(((float)((1u << 24) - i) - 0.5f) * 0x1p-24f));
  }
  return -logf(a);
}

// the weight of a key under the temperature, in 2^-40 units (the maximum's weight is exactly 2^40)
__device__ __forceinline__ uint64_t key_mass(uint32_t key, uint32_t kmax, float vmax, float invT) {
  if (key == kmax) return (uint64_t)SR_FIX;
  const float w = expf((key_value(key) - vmax) * invT);
  return (uint64_t)((double)w * SR_FIX + 0.5);
}

// 8 consecutive bf16 of a row starting at column c0 (a multiple of 8): one 16-B load when all 8 are below N, else
// the valid ones alone (columns >= N are never read).  Returns the raw bits; invalid slots hold 0.
__device__ __forceinline__ void load8(const bf16_t* row, int64_t c0, int64_t N, uint32_t* b) {
  if (c0 + 8 <= N) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(row + c0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      b[2 * i] = v[i] & 0xffffu;
      b[2 * i + 1] = v[i] >> 16;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = (c0 + i < N) ? (uint32_t)row[c0 + i] : 0u;
  }
}

struct SrShared {
  double wsum[SR_WAVES];
  float wmax[SR_WAVES];
  uint64_t wmass[SR_WAVES];
  uint32_t wcnt[SR_WAVES];
  unsigned long long best;   // packed (ordered score << 32 | ~column) maximum of the draw
  uint64_t f_mass;           // scan result: cumulative mass down to and including the found key's class
  uint32_t f_cnt, f_key, f_found;
  uint32_t kmax, kmin;       // ordered keys of the allowed maximum / minimum
  int nan_col;
};

// exclusive block prefix (in thread order) of an integer pair; `tot*` receive the block totals
__device__ __forceinline__ void block_prefix(uint32_t c, uint64_t m, SrShared& sh, uint32_t& cb, uint64_t& mb,
                                             uint32_t& totc, uint64_t& totm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t ci = c;
  uint64_t mi = m;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t cu = __shfl_up(ci, o, 64);
    const uint64_t mu = __shfl_up((unsigned long long)mi, o, 64);
    if (lane >= o) ci += cu, mi += mu;
  }
  __syncthreads();
  if (lane == 63) sh.wcnt[wave] = ci, sh.wmass[wave] = mi;
  __syncthreads();
  cb = ci - c, mb = mi - m;
  totc = 0, totm = 0;
  for (int w = 0; w < SR_WAVES; ++w) {
    if (w < wave) cb += sh.wcnt[w], mb += sh.wmass[w];
    totc += sh.wcnt[w], totm += sh.wmass[w];
  }
}

__global__ __launch_bounds__(SR_THREADS) void sample_rows_kernel(
    int64_t N, const bf16_t* __restrict__ logits, int64_t ld, const svla_sample_params* __restrict__ params,
    const int32_t* __restrict__ row_ids, uint32_t position, const int32_t* __restrict__ ranges, int32_t max_ranges,
    const int64_t* __restrict__ step, int64_t* __restrict__ token, float* __restrict__ logprob,
    float* __restrict__ logprob_raw, float* __restrict__ aux) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
  __shared__ SrShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = blockIdx.x;
  const bf16_t* row = logits + m * ld;

  const float T = params->temperature, top_p = params->top_p;
  const int64_t top_k = params->top_k;
  const uint64_t seed = params->seed, draw = params->draw;
  const uint32_t rid = row_ids ? (uint32_t)row_ids[m] : (uint32_t)m;
  const bool greedy = !(T > 0.f);
  const float invT = greedy ? 1.f : 1.f / T;

  // 1. allowed columns [lo, hi), clamped to [0, N); an empty range falls back to every column
  int64_t lo = 0, hi = N;
  const int64_t nranges = ranges != nullptr ? min(params->nranges, max_ranges) : 0;  // the table's entries in use
  if (nranges > 0) {
    const int64_t s = step ? step[0] : 0;
    const int64_t r = ((s % nranges) + nranges) % nranges;
    const int64_t a = max((int64_t)ranges[2 * r], (int64_t)0), b = min((int64_t)ranges[2 * r + 1], N);
    if (a < b) lo = a, hi = b;
  }
  const int64_t nallowed = hi - lo;

  if (tid == 0) {
    sh.best = 0ull;
    sh.kmax = 0u;
    sh.kmin = 0xffffu;
    sh.nan_col = 0x7fffffff;
    sh.f_found = 0u;
  }
  __syncthreads();

  // 2. pass A over all N columns: the raw log-sum-exp (online, per thread in double over a fixed column assignment),
  // and over the allowed ones the maximum / minimum key and the first NaN
  float rmax = -INFINITY;
  double rsum = 0.0;
  {
    uint32_t kmx = 0u, kmn = 0xffffu;
    int nanc = 0x7fffffff;
    const int64_t groups = (N + 7) / 8;
    for (int64_t g = tid; g < groups; g += SR_THREADS) {
      uint32_t b[8];
      load8(row, g * 8, N, b);
      float v[8], gm = -INFINITY;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t c = g * 8 + i;
        v[i] = (c < N) ? __uint_as_float(b[i] << 16) : -INFINITY;
        gm = fmaxf(gm, v[i]);
        if (c >= lo && c < hi) {
          if (bf_isnan(b[i])) {
            nanc = min(nanc, (int)c);
          } else {
            const uint32_t k = okey(b[i]);
            kmx = max(kmx, k);
            kmn = min(kmn, k);
          }
        }
      }
      if (gm > rmax) {
        rsum *= (double)expf(rmax - gm);  // rmax = -inf: rsum is 0 and stays 0
        rmax = gm;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t c = g * 8 + i;
        if (c < N) rsum += (v[i] == rmax) ? 1.0 : (double)expf(v[i] - rmax);  // NaN: propagates
      }
    }
    atomicMax(&sh.kmax, kmx);
    atomicMin(&sh.kmin, kmn);
    if (nanc != 0x7fffffff) atomicMin(&sh.nan_col, nanc);
    // fixed-order combine: the block maximum, then each thread's sum rescaled to it, xor butterfly, waves in order
    float wm = wave_max(rmax);
    if (lane == 0) sh.wmax[wave] = wm;
    __syncthreads();
    float bm = sh.wmax[0];
    for (int w = 1; w < SR_WAVES; ++w) bm = fmaxf(bm, sh.wmax[w]);
    double s = (rmax == -INFINITY) ? 0.0 : (rmax == bm ? rsum : rsum * (double)expf(rmax - bm));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) sh.wsum[wave] = s;
    __syncthreads();
    rsum = 0.0;
    for (int w = 0; w < SR_WAVES; ++w) rsum += sh.wsum[w];
    rmax = bm;
  }
  const double raw_lse = (double)rmax + log(rsum);
  const int nan_col = sh.nan_col;
  const uint32_t kmax = sh.kmax, kmin = sh.kmin;
  if (nan_col != 0x7fffffff) {  // rule 6: a NaN among the allowed columns
    if (tid == 0) {
      token[m] = nan_col;
      logprob[m] = NAN;
      logprob_raw[m] = NAN;
      if (aux) aux[2 * m] = NAN, aux[2 * m + 1] = 0.f;
    }
    return;
  }
  const float vmax = key_value(kmax);

  // 3. the kept set {key >= tstar}: top-k then top-p over the per-value histogram, one sign half at a time from the top
  const int64_t keff = (top_k > 0 && top_k < nallowed) ? top_k : nallowed;
  const bool filtering = !greedy && (keff < nallowed || top_p < 1.f);
  uint32_t tstar = kmin;
  uint64_t zkept = 0;     // mass of the kept set, 2^-40 units (filtering only)
  uint32_t nkept = (uint32_t)nallowed;
  if (filtering) {
    const int64_t g0 = lo / 8, g1 = (hi + 7) / 8;
    int held = -1;  // the half the histogram holds
    auto build = [&](int half) {
      for (int j = tid; j < SR_HIST; j += SR_THREADS) hist[j] = 0u;
      __syncthreads();
      for (int64_t g = g0 + tid; g < g1; g += SR_THREADS) {
        uint32_t b[8];
        load8(row, g * 8, N, b);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int64_t c = g * 8 + i;
          const uint32_t k = okey(b[i]);
          if (c >= lo && c < hi && (int)(k >> 15) == half) atomicAdd(&hist[hphys((int)(k & 0x7fffu))], 1u);
        }
      }
      __syncthreads();
      held = half;
    };
    // Descending scan of the held half for the first key >= floor_key whose cumulative (count, mass), carries
    // included, satisfies: by_count ? count >= need_c : (double)mass >= need_m.  Leaves sh.f_*; adds the half's
    // totals (over keys >= floor_key) to the carries.
    auto scan = [&](bool by_count, uint32_t need_c, double need_m, uint32_t floor_key, uint32_t& carry_c,
                    uint64_t& carry_m) {
      const uint32_t base = (uint32_t)held << 15;
      const int jtop = SR_BINS - 1 - tid * SR_PER;
      uint32_t c = 0;
      uint64_t ms = 0;
      for (int i = 0; i < SR_PER; ++i) {
        const int j = jtop - i;
        const uint32_t key = base | (uint32_t)j, n = hist[hphys(j)];
        if (n && key >= floor_key) c += n, ms += (uint64_t)n * key_mass(key, kmax, vmax, invT);
      }
      uint32_t cb, totc;
      uint64_t mb, totm;
      block_prefix(c, ms, sh, cb, mb, totc, totm);
      cb += carry_c, mb += carry_m;
      const bool before = by_count ? cb >= need_c : (double)mb >= need_m;
      const bool after = by_count ? cb + c >= need_c : (double)(mb + ms) >= need_m;
      if (!before && after) {  // integer prefixes are monotonic: exactly one thread
        for (int i = 0; i < SR_PER; ++i) {
          const int j = jtop - i;
          const uint32_t key = base | (uint32_t)j, n = hist[hphys(j)];
          if (n && key >= floor_key) {
            cb += n, mb += (uint64_t)n * key_mass(key, kmax, vmax, invT);
            if (by_count ? cb >= need_c : (double)mb >= need_m) {
              sh.f_key = key, sh.f_cnt = cb, sh.f_mass = mb, sh.f_found = 1u;
              break;
            }
          }
        }
      }
      carry_c += totc, carry_m += totm;
      __syncthreads();
    };

    // top-k: the k-th largest allowed value's key tk, Z = mass of {key >= tk}, ties at tk included
    uint32_t cc = 0;
    uint64_t cm = 0;
    uint32_t tk = kmin;
    for (int half = 1; half >= 0; --half) {
      if ((int)(kmax >> 15) < half) continue;  // no allowed value in this half
      build(half);
      scan(true, (uint32_t)keff, 0.0, 0u, cc, cm);
      if (sh.f_found) break;
    }
    // every allowed column was counted and keff <= nallowed, so the scan found its key
    const bool got = sh.f_found != 0u;
    tk = got ? sh.f_key : kmin;
    const uint64_t Z = got ? sh.f_mass : cm;
    tstar = tk, zkept = Z, nkept = got ? sh.f_cnt : cc;
    __syncthreads();
    if (top_p < 1.f) {  // top-p: the largest t with mass{key >= t} >= top_p Z, searched among keys >= tk
      if (tid == 0) sh.f_found = 0u;
      __syncthreads();
      const double need = fmax((double)top_p * (double)Z, 1.0);  // top_p <= 0: the top value class alone
      cc = 0, cm = 0;
      for (int half = 1; half >= (int)(tk >> 15); --half) {
        if ((int)(kmax >> 15) < half) continue;
        if (held != half) build(half);
        scan(false, 0u, need, tk, cc, cm);
        if (sh.f_found) break;
      }
      if (sh.f_found) tstar = sh.f_key, zkept = sh.f_mass, nkept = sh.f_cnt;
    }
  }

  // 4. the draw over the kept set: argmax of v / T + g, first column on an exact tie (greedy: no noise); without a
  // filter the kept mass is summed here (per thread in double, fixed order)
  {
    const int64_t g0 = lo / 8, g1 = (hi + 7) / 8;
    unsigned long long best = 0ull;
    double zs = 0.0;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), dr = (uint32_t)draw;
    for (int64_t g = g0 + tid; g < g1; g += SR_THREADS) {
      uint32_t b[8];
      load8(row, g * 8, N, b);
      bool any = false;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t c = g * 8 + i;
        any |= c >= lo && c < hi && okey(b[i]) >= tstar;
      }
      if (!any) continue;
      uint32_t rnd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (!greedy) {
        philox4x32_10((uint32_t)(g * 2), position, rid, dr, k0, k1, rnd);
        philox4x32_10((uint32_t)(g * 2 + 1), position, rid, dr, k0, k1, rnd + 4);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t c = g * 8 + i;
        const uint32_t k = okey(b[i]);
        if (!(c >= lo && c < hi && k >= tstar)) continue;
        const float v = __uint_as_float(b[i] << 16);
        if (!filtering) zs += (k == kmax) ? 1.0 : (double)expf((v - vmax) * invT);
        const float s = greedy ? v : v * invT + gumbel(rnd[i]);
        uint32_t sb = __float_as_uint(s);
        sb = (sb & 0x80000000u) ? ~sb : (sb | 0x80000000u);  // ordered: -inf scores still beat the empty 0
        const unsigned long long p = ((unsigned long long)sb << 32) | (uint32_t)(~(uint32_t)c);
        best = p > best ? p : best;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(best, o, 64);
      best = other > best ? other : best;
      zs += __shfl_xor(zs, o, 64);
    }
    __syncthreads();
    if (lane == 0) {
      atomicMax(&sh.best, best);
      sh.wsum[wave] = zs;
    }
    __syncthreads();
    if (tid == 0) {
      // a kept set is never empty (the maximum is always kept); the guard keeps the read below inside the row
      const uint32_t col = sh.best ? ~(uint32_t)(sh.best & 0xffffffffull) : (uint32_t)lo;
      const float vt = __uint_as_float((uint32_t)row[col] << 16);
      double logz;
      if (filtering) {
        logz = log((double)zkept / SR_FIX);
      } else {
        double z = 0.0;
        for (int w = 0; w < SR_WAVES; ++w) z += sh.wsum[w];
        logz = log(z);
      }
      token[m] = (int64_t)col;
      logprob[m] = (float)(((double)vt - (double)vmax) * (double)invT - logz);
      logprob_raw[m] = (float)((double)vt - raw_lse);
      if (aux) aux[2 * m] = key_value(tstar), aux[2 * m + 1] = (float)nkept;
    }
  }
}

}  // namespace

extern "C" int svla_sample_rows(int64_t M, int64_t N, const void* logits, int64_t ld,
                                const svla_sample_params* params, const int32_t* row_ids, int64_t position,
                                const int32_t* ranges, int32_t max_ranges, const int64_t* step, int64_t* token,
                                float* logprob, float* logprob_raw, float* aux, void* stream) {
  SVLA_CHECK_ARG(M > 0 && M <= 0x7fffffff && N > 0 && N <= SR_MAX_N && ld >= N && ld % 8 == 0,
                 "sample_rows: M >= 1, 1 <= N <= 2^22, ld a multiple of 8 >= N");
  SVLA_CHECK_ARG(logits && ((uintptr_t)logits & 15) == 0 && params && token && logprob && logprob_raw,
                 "sample_rows: logits (16-B aligned), params, token, logprob, logprob_raw must be set");
  SVLA_CHECK_ARG(max_ranges >= 0 && (ranges != nullptr || max_ranges == 0), "sample_rows: max_ranges without a range table");
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)sample_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SR_LDS);
    attr = true;
  }
  hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)M), dim3(SR_THREADS), SR_LDS, (hipStream_t)stream, N,
                     (const bf16_t*)logits, ld, params, row_ids, (uint32_t)position, ranges, max_ranges, step, token,
                     logprob, logprob_raw, aux);
  return svla::check_launch("sample_rows");
}
