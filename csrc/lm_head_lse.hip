// Fused LM-head log-softmax ("prompt logprobs"): lp[r] = logit[r, target[r]] - logsumexp_v logit[r, v]
// with logit = x . w^T, without a logit ever reaching memory.
//
// Work split: (row tile of 128 hidden rows) x (vocabulary slice).  A workgroup of 4 waves owns one
// row tile and one slice and walks the slice's 128-column tiles persistently; its waves form a
// 2 x 2 grid, each holding a 64-row x 64-column fp32 accumulator block (4 x 4 MFMA 16x16x32 tiles).
//   * K loop: BK = 64 per stage, both operands staged by 16-B global_load_lds (LDS-DMA) into a
//     4-stage ring, one s_barrier per stage, counted vmcnt.  The ring runs over the flattened
//     (column tile, K step) sequence, so the first stages of the next column tile are in flight while
//     the epilogue of the current one runs.  The (row >> 1) & 7 XOR chunk swizzle is applied on the
//     source address, so the ds_read_b128 fragment reads are bank-conflict free (as in skinny_gemm.hip).
//   * W is the MFMA's A operand: a lane ends with ONE hidden row (lane & 15 of each 16-row tile) and
//     16 vocabulary columns of its wave's block per column tile.  It keeps that row's running
//     (max, sum exp, target logit) over its own columns in registers across all column tiles; the
//     exponent is only taken of logit - running max.
//   * At the end of the slice the 4 lane groups of a row merge by shuffles, the two column waves merge
//     through LDS (left wave first), and one (max, sumexp, target-or--inf) triple per row goes to `ws`.
//   * A second small launch merges a row's triples in slice order 0, 1, 2, ...: no atomics, no
//     tickets, the same bits on every call.
// Rows >= R and columns >= V are masked in the epilogue (loads clamp to the last valid row), so
// neither operand is padded by the caller and the padding rows [V, Vpad) of w are never read.
#include "common.h"

#include <math.h>

namespace {

constexpr int BM = 128, BN = 128, BK = 64, NS = 4;
constexpr int XB = BM * 128, WB = BN * 128, SB = XB + WB;  // stage bytes (128 B of K per row)
constexpr int LX = BM / 32, LW = BN / 32, L = LX + LW;     // glds per wave per stage (8 rows each)
constexpr int kMaxSlices = 1024;

typedef __attribute__((address_space(3))) void* lds_ptr;
typedef const __attribute__((address_space(1))) void* gbl_ptr;

template <int N>
LK_DEVICE void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 0xF) | ((N >> 4) << 14) | (0x7 << 4) | (0xF << 8));
}
LK_DEVICE void wait_ahead(int ahead) {  // this wave's DMAs of all but the newest `ahead` stages landed
  if (ahead >= 2) wait_vm<2 * L>();
  else if (ahead == 1) wait_vm<L>();
  else wait_vm<0>();
}
LK_DEVICE int swz(int row) { return (row >> 1) & 7; }

// (m, s) <- (m, s) merged with (m2, s2): sums of exp relative to their maxima; -inf = empty
LK_DEVICE void lse_merge(float& m, float& s, float m2, float s2) {
  const float nm = fmaxf(m, m2);
  const float ref = nm == -INFINITY ? 0.f : nm;
  s = s * __expf(m - ref) + s2 * __expf(m2 - ref);
  m = nm;
}

int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      n = 0;
    return n > 0 ? n : 256;
  }();
  return cus;
}

// ws image: [row tile][slice][max | sumexp | target][BM rows]
__global__ __launch_bounds__(256, 1) void lm_head_lse_kernel(const bf16_t* __restrict__ X, long ldx,
                                                             const bf16_t* __restrict__ W, int R, int V, int H,
                                                             const int* __restrict__ targets, int S, int nct,
                                                             float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float xw[2][3][64];  // right column wave -> left column wave, per row half

  const int rt = blockIdx.x / S, s = blockIdx.x % S;
  const int c0 = (int)((long)s * nct / S), c1 = (int)((long)(s + 1) * nct / S);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int r = lane & 15, g = lane >> 4;
  const int nk = H / BK;
  const int Q = (c1 - c0) * nk;  // stages of this workgroup

  // sources of this wave's DMA instructions: 8 rows x 128 B each, chunk-swizzled per row
  const int lrow = lane >> 3, lch = lane & 7;
  const bf16_t* xsrc[LX];
  int wrow[LW], wch[LW];
#pragma unroll
  for (int i = 0; i < LX; ++i) {
    const int row = (w * LX + i) * 8 + lrow;
    xsrc[i] = X + (long)min(rt * BM + row, R - 1) * ldx + ((lch ^ swz(row)) * 8);
  }
#pragma unroll
  for (int i = 0; i < LW; ++i) {
    wrow[i] = (w * LW + i) * 8 + lrow;
    wch[i] = (lch ^ swz(wrow[i])) * 8;
  }
  int ict = c0, ik = 0, ist = 0;  // next stage to issue: column tile, K step, ring slot
  auto issue = [&]() {
    unsigned char* base = smem + ist * SB;
#pragma unroll
    for (int i = 0; i < LX; ++i)
      __builtin_amdgcn_global_load_lds((gbl_ptr)(xsrc[i] + ik * BK), (lds_ptr)(base + (w * LX + i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < LW; ++i) {
      // columns past V clamp to the last vocabulary row: never a padding row, never outside w
      const bf16_t* src = W + (long)min(ict * BN + wrow[i], V - 1) * H + ik * BK + wch[i];
      __builtin_amdgcn_global_load_lds((gbl_ptr)src, (lds_ptr)(base + XB + (w * LW + i) * 1024), 16, 0, 0);
    }
    if (++ik == nk) {
      ik = 0;
      ++ict;
    }
    ist = (ist + 1) & (NS - 1);
  };

  // per-lane running state of rows wm * 64 + 16 m + r over this lane's columns
  int tg[4];
  float rmax[4], rsum[4], tlog[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int row = rt * BM + wm * 64 + 16 * m + r;
    tg[m] = row < R ? targets[row] : -1;
    rmax[m] = -INFINITY;
    rsum[m] = 0.f;
    tlog[m] = -INFINITY;
  }
  // the target loads retire before the first DMA is issued: the counted vmcnt waits of the ring
  // below must count DMAs only
#pragma unroll
  for (int m = 0; m < 4; ++m) asm volatile("" : "+v"(tg[m]));
  __builtin_amdgcn_sched_barrier(0);

  floatx4 acc[4][4];
  auto zero = [&]() {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = floatx4{0.f, 0.f, 0.f, 0.f};
  };
  zero();

  auto compute = [&](int st) {
    const unsigned char* base = smem + st * SB;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = 4 * h + g;
      short8 a[4], b[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int row = wm * 64 + 16 * m + r;
        a[m] = *reinterpret_cast<const short8*>(base + row * 128 + ((c ^ swz(row)) << 4));
      }
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int row = wn * 64 + 16 * n + r;
        b[n] = *reinterpret_cast<const short8*>(base + XB + row * 128 + ((c ^ swz(row)) << 4));
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[n], a[m], acc[m][n], 0, 0, 0);
    }
  };

  // column tile ct done: fold the accumulators (hidden row 16 m + r, columns 16 n + 4 g + i of the
  // wave's block) into the lane's running state
  auto fold = [&](int ct) {
    const int cb = ct * BN + wn * 64 + 4 * g;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      float tmax = -INFINITY;
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int col = cb + 16 * n + i;
          const float v = col < V ? acc[m][n][i] : -INFINITY;
          acc[m][n][i] = v;
          tmax = fmaxf(tmax, v);
          if (col == tg[m]) tlog[m] = v;
        }
      const float nm = fmaxf(rmax[m], tmax);
      const float ref = nm == -INFINITY ? 0.f : nm;
      float sum = rsum[m] * __expf(rmax[m] - ref);
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) sum += __expf(acc[m][n][i] - ref);
      rsum[m] = sum;
      rmax[m] = nm;
    }
  };

#pragma unroll
  for (int p = 0; p < NS - 1; ++p)
    if (p < Q) issue();
  int ct = c0, kk = 0, st = 0;
  for (int q = 0; q < Q; ++q) {
    wait_ahead(min(NS - 2, Q - 1 - q));  // stage q landed (this wave's part)
    __builtin_amdgcn_s_barrier();        // ... for every wave; and ring slot (q - 1) % NS is free
    __builtin_amdgcn_sched_barrier(0);
    if (q + NS - 1 < Q) issue();
    __builtin_amdgcn_sched_barrier(0);
    compute(st);
    st = (st + 1) & (NS - 1);
    if (++kk == nk) {
      fold(ct);
      zero();
      kk = 0;
      ++ct;
    }
  }

  // slice done: lane groups of a row (lanes r, r + 16, r + 32, r + 48) in a fixed order
#pragma unroll
  for (int m = 0; m < 4; ++m) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float m2 = __shfl_xor(rmax[m], o, 64), s2 = __shfl_xor(rsum[m], o, 64);
      // both partners compute the same value: the lower lane's operand goes first on both
      float a = (lane & o) ? m2 : rmax[m], as = (lane & o) ? s2 : rsum[m];
      const float b = (lane & o) ? rmax[m] : m2, bs = (lane & o) ? rsum[m] : s2;
      lse_merge(a, as, b, bs);
      rmax[m] = a;
      rsum[m] = as;
      tlog[m] = fmaxf(tlog[m], __shfl_xor(tlog[m], o, 64));
    }
  }
  // the two column waves of a row half through LDS: left (wn 0) first
  if (wn == 1 && g == 0) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      xw[wm][0][16 * m + r] = rmax[m];
      xw[wm][1][16 * m + r] = rsum[m];
      xw[wm][2][16 * m + r] = tlog[m];
    }
  }
  __syncthreads();
  if (wn == 0 && g == 0) {
    float* dst = ws + ((long)rt * S + s) * 3 * BM + wm * 64;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int i = 16 * m + r;
      lse_merge(rmax[m], rsum[m], xw[wm][0][i], xw[wm][1][i]);
      dst[i] = rmax[m];
      dst[BM + i] = rsum[m];
      dst[2 * BM + i] = fmaxf(tlog[m], xw[wm][2][i]);
    }
  }
}

// one thread per row: the S triples in slice order
__global__ __launch_bounds__(BM) void lm_head_lse_merge_kernel(const float* __restrict__ ws, int R, int S,
                                                               float* __restrict__ lp, float* __restrict__ lse) {
  const int rt = blockIdx.x, i = threadIdx.x;
  const int row = rt * BM + i;
  if (row >= R) return;
  const float* src = ws + (long)rt * S * 3 * BM + i;
  float m = -INFINITY, sum = 0.f, t = -INFINITY;
  for (int s = 0; s < S; ++s, src += 3 * BM) {
    lse_merge(m, sum, src[0], src[BM]);
    t = fmaxf(t, src[2 * BM]);
  }
  const float l = logf(sum);
  lse[row] = m + l;
  lp[row] = t == -INFINITY ? -INFINITY : (t - m) - l;
}

}  // namespace

void lk_lm_head_logprobs_plan(int R, int V, int* row_tile, int* col_tile, int* slices) {
  const int nrt = R > 0 ? (R + BM - 1) / BM : 1;
  const int nct = V > 0 ? (V + BN - 1) / BN : 1;
  // enough workgroups for every CU, but at least two column tiles per slice (the ring's fill and
  // the slice's merge are paid once per workgroup)
  int s = (device_cus() + nrt - 1) / nrt;
  s = min(s, (nct + 1) / 2);
  s = max(1, min(s, kMaxSlices));
  *row_tile = BM;
  *col_tile = BN;
  *slices = s;
}

int lk_lm_head_logprobs_supported(int R, int V, int Vpad, int H) {
  if (R < 0 || R > (1 << 22)) return -1;
  if (V < 1 || V > (1 << 30) || Vpad < V) return -2;
  if (H < BK || H % BK != 0 || H > (1 << 16)) return -3;
  return 1;
}

long lk_lm_head_logprobs_ws_floats(int R, int V) {
  int bm, bn, s;
  lk_lm_head_logprobs_plan(R, V, &bm, &bn, &s);
  return (long)((R + BM - 1) / BM) * s * 3 * BM;
}

int lk_lm_head_logprobs(const bf16_t* x, long ldx, const bf16_t* w, int R, int V, int H, const int* targets,
                        float* ws, float* lp, float* lse, hipStream_t st) {
  const int ok = lk_lm_head_logprobs_supported(R, V, V, H);
  if (ok < 0) return ok;
  if (ldx < H || ldx % 8 != 0 || reinterpret_cast<uintptr_t>(x) % 16 != 0 || reinterpret_cast<uintptr_t>(w) % 16 != 0)
    return -4;
  if (R == 0) return 0;
  int bm, bn, S;
  lk_lm_head_logprobs_plan(R, V, &bm, &bn, &S);
  const int nrt = (R + BM - 1) / BM, nct = (V + BN - 1) / BN;
  constexpr int lds = NS * SB;
  LK_SET_MAX_LDS(lm_head_lse_kernel, lds);
  lm_head_lse_kernel<<<nrt * S, 256, lds, st>>>(x, ldx, w, R, V, H, targets, S, nct, ws);
  LK_CHECK_LAUNCH();
  lm_head_lse_merge_kernel<<<nrt, BM, 0, st>>>(ws, R, S, lp, lse);
  LK_CHECK_LAUNCH();
  return 0;
}
