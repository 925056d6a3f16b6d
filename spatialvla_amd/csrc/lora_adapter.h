// The adapter operands of the decode-step GEMVs with unmerged LoRA adapters, shared by lora_decode.hip (bf16 base
// weights) and fp8_decode.hip (e4m3 base weights): the segment list with typed pointers, one output row's B row and T
// values (one value per lane: r <= 64) and the two roundings of svla_gemm_bf16's plain store followed by svla_lora_up.
#pragma once
#include "svla_common.h"

namespace {

constexpr int MAX_SEG = 3;
constexpr int MAX_R = 64;

struct Segs {
  const bf16_t* p[MAX_SEG];
  int64_t st[MAX_SEG + 1];
  int64_t ld;
  int nseg, r, R;
};

__device__ __forceinline__ const bf16_t* seg_p(const Segs& S, int s) {
  return s == 0 ? S.p[0] : (s == 1 ? S.p[1] : S.p[2]);
}
__device__ __forceinline__ int seg_of(const Segs& S, int64_t n) {
  return (int)(S.nseg > 1 && n >= S.st[1]) + (int)(S.nseg > 2 && n >= S.st[2]);
}
__device__ __forceinline__ int64_t seg_st(const Segs& S, int s) { return s == 0 ? 0 : (s == 1 ? S.st[1] : S.st[2]); }

// The adapter operands of one output row: lane j < r holds B_s[row, j] and T[m, s R + j] (one value per lane: r <= 64).
template <int MR>
struct AdRow {
  float b;
  float t[MR];
};
template <int MR>
__device__ __forceinline__ void ad_load(AdRow<MR>& a, const Segs& S, int s, int64_t row, const bf16_t* __restrict__ T,
                                        int64_t ldt, int M, int lane) {
  const bool on = lane < S.r;
  a.b = on ? bf2f(seg_p(S, s)[row * S.ld + lane]) : 0.f;
#pragma unroll
  for (int m = 0; m < MR; ++m) a.t[m] = (on && m < M) ? bf2f(T[m * ldt + s * S.R + lane]) : 0.f;
}
// bf16(bf16(base) + bf16(s * sum_j T B)): svla_gemm_bf16's plain store followed by svla_lora_up
template <int MR>
__device__ __forceinline__ float ad_finish(const AdRow<MR>& a, int m, float base, float sc) {
  const float l = wave_sum(a.b * a.t[m]);
  return round_bf(round_bf(base) + round_bf(sc * l));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int make_segs(const char* what, const svla_lora_segs* in, Segs& S, bool need_starts, int64_t extent) {
  SVLA_CHECK_ARG(in != nullptr, "%s: segment list is NULL", what);
  SVLA_CHECK_ARG(in->nseg >= 1 && in->nseg <= MAX_SEG, "%s: 1..3 segments, got %d", what, in->nseg);
  SVLA_CHECK_ARG(in->r >= 8 && in->r <= MAX_R && in->r % 8 == 0, "%s: rank must be a multiple of 8 in [8, 64], got %d",
                 what, in->r);
  SVLA_CHECK_ARG(in->ld > 0 && in->ld % 8 == 0, "%s: the small matrices' ld must be a positive multiple of 8, got %lld",
                 what, (long long)in->ld);
  S.nseg = in->nseg;
  S.r = in->r;
  S.R = (in->r + 31) / 32 * 32;
  S.ld = in->ld;
  for (int s = 0; s < MAX_SEG; ++s) {
    S.p[s] = s < in->nseg ? (const bf16_t*)in->ptr[s] : nullptr;
    SVLA_CHECK_ARG(s >= in->nseg || (S.p[s] != nullptr && aligned16(S.p[s])),
                   "%s: segment %d pointer NULL or not 16-B aligned", what, s);
  }
  for (int s = 0; s <= MAX_SEG; ++s) S.st[s] = 0;
  if (need_starts) {
    SVLA_CHECK_ARG(in->start[0] == 0 && in->start[in->nseg] == extent, "%s: segment starts must run from 0 to %lld",
                   what, (long long)extent);
    for (int s = 0; s < in->nseg; ++s)
      SVLA_CHECK_ARG(in->start[s + 1] > in->start[s] && in->start[s] % 16 == 0,
                     "%s: segment starts must ascend and be multiples of 16", what);
    for (int s = 0; s <= in->nseg; ++s) S.st[s] = in->start[s];
  }
  return SVLA_OK;
}

}  // namespace
