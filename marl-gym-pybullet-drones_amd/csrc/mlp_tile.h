// mlp_tile.h — one layer's product of the planners' f32-MFMA tanh MLPs, shared by
// the value tail (planner_value.hip) and the policy prior (planner_prior.hip).
// HIP; the constants (workgroup, MFMA shape, K-chunk, LDS padding) are
// value_sizes.h's.
#pragma once

#include <hip/hip_runtime.h>

#include "value_sizes.h"

namespace qs {

typedef float value_f4 __attribute__((ext_vector_type(4)));

// out = clip((x − mean) / sqrt(var + eps), ±clip) in float64, rounded to float32:
// rms_norm1 of normalizer.hip.
__device__ __forceinline__ float norm1(float xv, double m, double sd, double clip) {
  double y = ((double)xv - m) / sd;
  y = y < -clip ? -clip : (y > clip ? clip : y);
  return (float)y;
}

// One layer's product for a workgroup's rows: acc[mt][nt] += A · Wᵀ over K, with W
// [N][K] row-major in global memory streamed through sW in chunks of kValueChunk
// columns (zero beyond K).  FIRST: A is the input, staged a chunk at a time into
// sX from `in`: in.stage<XR>(r0, k, kv, out) fills out[i] with column k of row
// r0 + 8 · i as the net takes it (normalised; 0 where !kv, i.e. k >= K, or past
// the last row), and is asked once for every (row, k) of the tile; otherwise A
// is sH, resident, and `in` is not used.  Wave w owns the column tiles w · NT ..
// w · NT + NT - 1 of all MT row tiles.  The next chunk's global loads are issued
// before the current chunk's MFMAs and land in LDS after them.
template <int N, int MT, bool FIRST, class Input>
__device__ __forceinline__ void layer_product(const Input& in, const float* __restrict__ W, int K, size_t row0, float* sH,
                                              float* sW, float* sX, value_f4 (&acc)[MT][N / 64]) {
  constexpr int NT = N / 64, TM = MT * kValueMfmaM, CP = kValueChunk + kValuePad, HP = N + kValuePad;
  constexpr int WR = N / 8, XR = TM / 8;   // rows of W / X a thread stages per chunk (32 columns x 8 rows a pass)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & 31, rsub = tid >> 5;   // this thread's column of a chunk, and its first row
  const int l15 = lane & 15, lq = lane >> 4;
  float wreg[WR], xreg[FIRST ? XR : 1];
  const int chunks = (K + kValueChunk - 1) / kValueChunk;

  auto load = [&](int ch) {
    const int k = ch * kValueChunk + col;
    const bool kv = k < K;
#pragma unroll
    for (int i = 0; i < WR; ++i) wreg[i] = kv ? W[(size_t)(rsub + 8 * i) * K + k] : 0.0f;
    if constexpr (FIRST) in.template stage<XR>(row0 + (size_t)rsub, k, kv, xreg);
  };

  load(0);
  for (int ch = 0; ch < chunks; ++ch) {
#pragma unroll
    for (int i = 0; i < WR; ++i) sW[(rsub + 8 * i) * CP + col] = wreg[i];
    if constexpr (FIRST) {
#pragma unroll
      for (int i = 0; i < XR; ++i) sX[(rsub + 8 * i) * CP + col] = xreg[i];
    }
    __syncthreads();
    if (ch + 1 < chunks) load(ch + 1);
    const int left = K - ch * kValueChunk;
    const int ksteps = left >= kValueChunk ? kValueChunk / kValueMfmaK : (left + kValueMfmaK - 1) / kValueMfmaK;
    const float* A = FIRST ? sX : sH + ch * kValueChunk;
    constexpr int AP = FIRST ? CP : HP;
    for (int ks = 0; ks < ksteps; ++ks) {
      const int kk = ks * kValueMfmaK + lq;
      float a[MT], b[NT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = A[(mt * kValueMfmaM + l15) * AP + kk];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) b[nt] = sW[((wave * NT + nt) * kValueMfmaM + l15) * CP + kk];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    }
    __syncthreads();   // sW / sX are rewritten by the next trip (and sH by the caller)
  }
}

// The hidden layers of a workgroup's TM = MT · 16 rows: H1 = tanh(X · W1ᵀ + b1),
// then H2 = tanh(H1 · W2ᵀ + b2) · scale2[column] (scale2 null: 1), left in sH
// [TM][N + kValuePad] behind a barrier.  The accumulators' (row, column) of
// register r: row = 4 · (lane >> 4) + r, column = lane & 15.
template <int N, int MT, class Input>
__device__ __forceinline__ void hidden_layers(const Input& in, int I, const float* w1, const float* b1, const float* w2,
                                              const float* b2, const float* scale2, size_t row0, float* sH, float* sW,
                                              float* sX) {
  constexpr int NT = N / 64, HP = N + kValuePad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  value_f4 acc[MT][NT];
  auto clear = [&]() {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = value_f4{0.0f, 0.0f, 0.0f, 0.0f};
  };

  clear();
  layer_product<N, MT, true>(in, w1, I, row0, sH, sW, sX, acc);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int nc = (wave * NT + nt) * kValueMfmaM + l15;
    const float bias = b1[nc];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) sH[(mt * kValueMfmaM + 4 * lq + r) * HP + nc] = tanhf(acc[mt][nt][r] + bias);
  }
  __syncthreads();

  clear();
  layer_product<N, MT, false>(in, w2, N, row0, sH, sW, sX, acc);   // (ends in a barrier: every wave is done with H1)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int nc = (wave * NT + nt) * kValueMfmaM + l15;
    const float bias = b2[nc], s2 = scale2 ? scale2[nc] : 1.0f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) sH[(mt * kValueMfmaM + 4 * lq + r) * HP + nc] = tanhf(acc[mt][nt][r] + bias) * s2;
  }
  __syncthreads();
}

}  // namespace qs
