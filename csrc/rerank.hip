// Cross-encoder score head, one kernel: CLS row -> pooler dense + tanh -> classifier -> score.
//   x   = hidden[cu[b]]                       (first row of sequence b; a zero vector if it is empty)
//   a_j = sum_k pool_w[j,k] * x_k + pool_b[j]
//   s   = sum_j tanhf(a_j) * cls_w[j] + cls_b
//   out[b] = activation ? 1 / (1 + expf(-s)) : s
// One 256-thread workgroup per sequence.  The CLS row, pool_b and cls_w are staged once into LDS
// as f32 (12 KB, no opt-in) and each lane keeps its own K slice of the CLS row in registers (the
// slice is the same for every output row).  Wave w takes the output rows j = w, w+4, ... and
// reads pool_w[j,:] with 16-byte loads along K, f32 accumulation.  A wave owns H/4 rows at one
// load per lane each, so what it waits for is latency, not bytes: it works on kRows rows at a
// time.  All their loads are issued first, then the kRows lane partials are reduced together by a
// transposing butterfly (17 shuffles instead of 6 per row) that leaves row r's sum in lanes
// 4r..4r+3, so sixteen lanes apply bias, tanhf and the classifier weight at once.  Per-lane
// partials -> wave_sum -> four wave partials added in a fixed order: no atomics, the same bits on
// every run.  (Measured and not kept: a second register buffer that prefetches the next kRows
// rows, 12.2 us against 11.9 us at H 384 -- docs/rerank.md.)
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kRerankMaxH = 1024;
constexpr int kRerankWaves = 4;
constexpr int kRows = 16;  // rows of pool_w a wave has in flight

// v[0..15]: this lane's partial of 16 rows -> returns the full 64-lane sum of row (lane >> 2) & 15.
// Each step folds the upper half of the rows onto the lanes whose bit is set: 8 + 4 + 2 + 1
// shuffles, then two plain butterfly steps over the lane's two low bits.
LK_DEVICE float reduce16_transposed(float (&v)[kRows], int lane) {
#pragma unroll
  for (int half = kRows / 2, off = 32; half >= 1; half >>= 1, off >>= 1) {
    // bitwise selects (one v_bfi each): written as `hi ? v[i + half] : v[i]` the compiler turns
    // the pair into a lane-indexed read of v[], a chain of 16 compares and selects per value
    const unsigned m = (lane & off) ? 0xffffffffu : 0u;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const unsigned lo = __float_as_uint(v[i]), up = __float_as_uint(v[i + half]);
      const float keep = __uint_as_float((up & m) | (lo & ~m));
      const float send = __uint_as_float((lo & m) | (up & ~m));
      v[i] = keep + __shfl_xor(send, off, 64);
    }
  }
  float s = v[0];
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 1, 64);
  return s;
}

// NV: 16-byte vectors of a row per lane (1: H <= 512, 2: H <= 1024)
template <int NV>
__global__ __launch_bounds__(256) void rerank_head_kernel(const bf16_t* __restrict__ hidden, long hs,
                                                          const int* __restrict__ cu, int H,
                                                          const bf16_t* __restrict__ pool_w,
                                                          const bf16_t* __restrict__ pool_b,
                                                          const bf16_t* __restrict__ cls_w,
                                                          const bf16_t* __restrict__ cls_b, int activation,
                                                          float* __restrict__ out) {
  __shared__ float xs[kRerankMaxH];
  // pool_b and cls_w as f32: read per row group from LDS (a global load there would sit, with its
  // full latency, between two groups, and waiting for it would also wait for the prefetched rows)
  __shared__ float pbs[kRerankMaxH], cws[kRerankMaxH];
  __shared__ float part[kRerankWaves];
  const int b = blockIdx.x;
  const int beg = cu[b], end = cu[b + 1];
  const int nvec = H >> 3;  // <= 64 * NV
  const int lane = threadIdx.x & 63;
  // (scalar: the row index, its bound check and the row's base address stay off the VALU)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if ((int)threadIdx.x < nvec) {
    float v[8];
    if (end > beg) {
      load8(hidden + (long)beg * hs + threadIdx.x * 8, v);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) xs[threadIdx.x * 8 + i] = v[i];
    float bv[8], cv[8];
    load8(cls_w + threadIdx.x * 8, cv);
    if (pool_b) {
      load8(pool_b + threadIdx.x * 8, bv);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) bv[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      pbs[threadIdx.x * 8 + i] = bv[i];
      cws[threadIdx.x * 8 + i] = cv[i];
    }
  }
  __syncthreads();
  lk_f2 xr[NV][4];  // pairs: the dot products run as packed fp32 FMAs
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int c = lane + u * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      xr[u][i] = c < nvec ? (lk_f2){xs[c * 8 + 2 * i], xs[c * 8 + 2 * i + 1]} : (lk_f2){0.f, 0.f};
  }
  float p = 0.f;
  // kRows rows of pool_w, this lane's K slice of each (rows past H: zeros, no load)
  auto load_rows = [&](int j0, short8 (&w)[kRows][NV]) {
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const int j = j0 + r * kRerankWaves;
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int c = lane + u * 64;
        w[r][u] = (j < H && c < nvec) ? *reinterpret_cast<const short8*>(pool_w + (long)j * H + c * 8) : (short8)(0);
      }
    }
  };
  auto score_rows = [&](int j0, const short8 (&w)[kRows][NV]) {
    float acc[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      lk_f2 a2 = {0.f, 0.f};
#pragma unroll
      for (int u = 0; u < NV; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const lk_f2 w2 = {bf2f((bf16_t)w[r][u][2 * i]), bf2f((bf16_t)w[r][u][2 * i + 1])};
          a2 = __builtin_elementwise_fma(w2, xr[u][i], a2);
        }
      acc[r] = a2.x + a2.y;
    }
    const float dot = reduce16_transposed(acc, lane);
    const int j = j0 + ((lane >> 2) & (kRows - 1)) * kRerankWaves;
    if ((lane & 3) == 0 && j < H) {
      p += tanhf(dot + pbs[j]) * cws[j];
    }
  };
  for (int j0 = wave; j0 < H; j0 += kRerankWaves * kRows) {
    short8 w[kRows][NV];
    load_rows(j0, w);
    score_rows(j0, w);
  }
  p = wave_sum(p);
  if (lane == 0) part[wave] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = ((part[0] + part[1]) + part[2]) + part[3];
    s += cls_b ? bf2f(cls_b[0]) : 0.f;
    out[b] = activation ? 1.f / (1.f + expf(-s)) : s;
  }
}

}  // namespace

int lk_rerank_head(const bf16_t* hidden, long hs, const int* cu, int B, int H, const bf16_t* pool_w,
                   const bf16_t* pool_b, const bf16_t* cls_w, const bf16_t* cls_b, int activation, float* out,
                   hipStream_t st) {
  if (B <= 0) return 0;
  if (H <= 0 || H % 8) return -1;
  if (H > kRerankMaxH) return -2;
  if (hs < H) return -3;
  if (H <= 512)
    rerank_head_kernel<1><<<B, 256, 0, st>>>(hidden, hs, cu, H, pool_w, pool_b, cls_w, cls_b, activation, out);
  else
    rerank_head_kernel<2><<<B, 256, 0, st>>>(hidden, hs, cu, H, pool_w, pool_b, cls_w, cls_b, activation, out);
  LK_CHECK_LAUNCH();
  return 0;
}
