// Decode-step GEMV for one or two rows over OCP MXFP4 weights: W is [N, K] e2m1, two weights per
// byte (weight 2 j in the low nibble of byte j of a row, weight 2 j + 1 in the high nibble), with one
// e8m0 scale byte per 32 consecutive weights of a row (wexp [N, K / 32], value 2^(E - 127)) and no
// other scale.  The contract is gemv_decode.hip's (modes 0 plain, 1 res +=, 2 SwiGLU, 3 RoPE +
// paged-KV write; optional RMSNorm prologue; the same pair rules and the same rounding points in
// every epilogue); the weight stream is 17/32 B per weight.
//
//   dot[m][row] = sum_k (e2m1(wq4[row][k]) * 2^(E[row][k / 32] - 127)) * x[m][k]
// The block scale is applied by the conversion instruction itself (v_cvt_scalef32_pk_f32_fp4: one
// byte -> two fp32 times a power-of-two scale operand, exact), the products and the sum are fp32.
//
// Lane -> k mapping.  A wave's load instruction covers one contiguous 1 KB of a W row, a CHUNK of
// 2,048 weights (K % 2048 == 0): in chunk c lane l owns the 32 weights
//   k = 2048 c + 32 l + (0 .. 31)          (one 16-B nontemporal load),
// which are exactly one MX block: one scale byte per lane-load, wexp[row][64 c + l], a byte load
// issued with the chunk's W load (a wave's 64 scale bytes of a chunk are contiguous).  The operand
// of the conversion is the f32 with that exponent field, E << 23; the quantiser never writes E = 0
// (whose f32 image is zero, not 2^-127) or 0xFF.
//
// X image in LDS.  A lane's 32 weights meet 64 B of X: four 16-B pieces ("quarters") that a plain
// X row would hold at a 64-B lane stride, a 4-way bank conflict.  The image is permuted while it is
// staged: within chunk c the 16-B piece 4 l + q of the row lands at piece 64 q + l of the chunk's
// image, so quarter q of a chunk is 64 consecutive pieces, one per lane: every X read is a 16-B
// read at a 16-B lane stride.  The LDS-DMA does the permutation: lane l of the instruction for
// (chunk c, quarter q) fetches global piece 4 l + q and the DMA writes the 64 pieces to consecutive
// LDS addresses.  gamma is staged in the same order, so the RMSNorm prologue (elementwise plus a sum
// of squares) runs on the permuted image unchanged.
//
// Conversion and FMAs.  Dword j of a lane's W load (8 weights) takes four conversions, one per
// byte; byte b gives weights 8 j + 2 b (low nibble, .x) and 8 j + 2 b + 1 (high nibble, .y), which
// meet dword b of X quarter j unpacked to its (lo, hi) fp32 pair; one packed FMA per (row, m) adds
// the pair into a two-wide accumulator.  Per 32 weights of one row: 16 conversions and 16 M packed
// FMAs, plus 32 M unpack ops shared by the 2 P rows of a wave.
//
// Loads in flight.  A W row is a quarter of the bf16 bytes (K 4,096 is 2 chunks per lane per row),
// so a wave owns P pairs of rows at a time and loads U chunks of each before it converts: 2 U P
// 16-B loads per lane (U P <= 8: 256 B, the bf16 kernel's depth).  The long-K projections keep the
// two-waves-per-pair K split (KW = 2); the chunks of a row need not divide evenly (K 14,336 is
// 4 + 3), a wave's last group of U is cut by a wave-uniform test.  pick_plan holds the defaults per
// (M, N, chunks per row); lk_gemv_w4_set_plan overrides P and the K split for measurements
// (benchmarks/gemv_w4_bench.py; docs/decode_mxfp4.md has the arms).
// All of it is plain fp32 in one fixed order: no atomics, the same bits on every run.
#include "common.h"
#include "kernels.h"

namespace {

struct GemvW4Args {
  const bf16_t* x = nullptr;  // [M, K] input rows (NORM: the residual rows to normalise)
  long ldx = 0;
  const bf16_t* gamma = nullptr;  // NORM weights [K]
  float eps = 0.f;
  const unsigned char* w = nullptr;  // [N, K / 2] row-major e2m1 pairs
  const unsigned char* e = nullptr;  // [N, K / 32] e8m0 block scales
  int M = 0, N = 0, K = 0;
  int npairs = 0;
  bf16_t* out = nullptr;  // modes 0 / 2 / 3
  long ldo = 0;
  bf16_t* res = nullptr;  // mode 1
  long ldr = 0;
  int I = 0;  // mode 2: gate rows [0, I), up rows [I, 2I)
  // mode 3
  const int* positions = nullptr;
  const float* cos_sin = nullptr;
  int Hq = 0, Hkv = 0, D = 0, BS = 0, neox = 0;
  bf16_t* kc = nullptr;
  bf16_t* vc = nullptr;
  const int* slots = nullptr;
};

typedef __attribute__((address_space(3))) void* w4_lptr;
typedef const __attribute__((address_space(1))) void* w4_gptr;

LK_DEVICE float rbf4(float x) { return bf2f(f2bf(x)); }
LK_DEVICE float silu4(float x) { return x / (1.f + __expf(-x)); }

// the (lo, hi) fp32 pairs of four dwords of bf16
LK_DEVICE void unpack_x4(const uint4_t xv, lk_f2* xf) {
#pragma unroll
  for (int j = 0; j < 4; ++j) xf[j] = (lk_f2){__uint_as_float(xv[j] << 16), __uint_as_float(xv[j] & 0xffff0000u)};
}

// 32 e2m1 (one 16-B lane-load, one MX block) times their block scale against the 32 X values
// xf[0..15] (quarter j: xf[4 j .. 4 j + 3])
LK_DEVICE void dot32(const uint4_t wv, float scale, const lk_f2* xf, lk_f2& acc) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc = __builtin_elementwise_fma(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wv[j], scale, 0), xf[4 * j], acc);
    acc = __builtin_elementwise_fma(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wv[j], scale, 1), xf[4 * j + 1], acc);
    acc = __builtin_elementwise_fma(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wv[j], scale, 2), xf[4 * j + 2], acc);
    acc = __builtin_elementwise_fma(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wv[j], scale, 3), xf[4 * j + 3], acc);
  }
}

// rows of pair p (the pair rules of gemv_decode.hip)
template <int MODE>
LK_DEVICE void pair_rows(const GemvW4Args& g, int p, long& ra, long& rb, int& hd, int& head, int& ip) {
  if constexpr (MODE == 2) {
    ra = p;
    rb = (long)g.I + p;
  } else if constexpr (MODE == 3) {
    hd = g.D >> 1;
    head = p / hd;
    ip = p - head * hd;
    if (g.neox && head < g.Hq + g.Hkv) {
      ra = (long)head * g.D + ip;
      rb = ra + hd;
    } else {
      ra = (long)head * g.D + 2 * ip;
      rb = ra + 1;
    }
  } else {
    ra = 2L * p;
    rb = ra + 1;
  }
}

// the epilogue of one pair's two finished dot products, row m: gemv_decode.hip's arithmetic
template <int MODE>
LK_DEVICE void epilogue(const GemvW4Args& g, int m, int p, long ra, long rb, int hd, int head, int ip, float da,
                        float db) {
  if constexpr (MODE == 0) {
    g.out[(long)m * g.ldo + ra] = f2bf(da);
    g.out[(long)m * g.ldo + rb] = f2bf(db);
  } else if constexpr (MODE == 1) {
    bf16_t* rr = g.res + (long)m * g.ldr;
    const unsigned old = *reinterpret_cast<const unsigned*>(rr + ra);  // (ra even: rb = ra + 1)
    const float va = rbf4(rbf4(da) + __uint_as_float(old << 16));
    const float vb = rbf4(rbf4(db) + __uint_as_float(old & 0xffff0000u));
    *reinterpret_cast<unsigned*>(rr + ra) = pack_bf2(va, vb);
  } else if constexpr (MODE == 2) {
    g.out[(long)m * g.ldo + p] = f2bf(rbf4(silu4(rbf4(da))) * rbf4(db));
  } else {
    bf16_t* orow = g.out + (long)m * g.ldo;
    const float x1 = rbf4(da), x2 = rbf4(db);
    const int slot = g.slots ? g.slots[m] : -1;
    const long blk = slot >= 0 ? slot / g.BS : 0;
    const int off = slot >= 0 ? slot % g.BS : 0;
    const int d0 = (int)(ra - (long)head * g.D), d1 = (int)(rb - (long)head * g.D);
    if (head >= g.Hq + g.Hkv) {  // V: copied (into the row and the cache)
      const int h = head - g.Hq - g.Hkv;
      orow[ra] = f2bf(x1);
      orow[rb] = f2bf(x2);
      if (g.vc && slot >= 0) {
        bf16_t* vd = g.vc + ((blk * g.Hkv + h) * g.BS + off) * g.D;
        vd[d0] = f2bf(x1);
        vd[d1] = f2bf(x2);
      }
    } else {
      const float* cs = g.cos_sin + (long)g.positions[m] * g.D;  // [cos(D/2) | sin(D/2)]
      const float c = cs[ip], s = cs[hd + ip];
      const float y1 = x1 * c - x2 * s, y2 = x2 * c + x1 * s;
      if (head < g.Hq) {
        orow[ra] = f2bf(y1);
        orow[rb] = f2bf(y2);
      } else {  // K: unrotated in the row, rotated in the cache
        orow[ra] = f2bf(x1);
        orow[rb] = f2bf(x2);
        if (g.kc && slot >= 0) {
          bf16_t* kd = g.kc + ((blk * g.Hkv + (head - g.Hq)) * g.BS + off) * g.D;
          kd[d0] = f2bf(y1);
          kd[d1] = f2bf(y2);
        }
      }
    }
  }
}

template <int MR, bool NORM, int MODE, int U, int KW, int P>
__global__ __launch_bounds__(256) void gemv_w4_kernel(GemvW4Args g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);  // [MR][K], permuted per 2,048-element chunk (header)
  __shared__ float red[4 * MR];
  const int K = g.K;
  const int nch = K >> 3;   // 16-B pieces of an X row
  const int nk = K >> 11;   // W chunks per lane per row
  const int nkb = K >> 5;   // scale bytes of a W row
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

  // ---- stage X (and gamma) into LDS by LDS-DMA, permuted: instruction gi = 4 c + q takes the 64
  // pieces 4 l + q of chunk c and lands them at pieces [64 gi, 64 gi + 64) of the row's image
  bf16_t* gs = xs + MR * K;  // NORM: gamma [K], the same order
  for (int gi = wv; gi < (nch >> 6); gi += 4) {
    const int src = (gi >> 2) * 2048 + (4 * lane + (gi & 3)) * 8;  // element of the row
#pragma unroll
    for (int m = 0; m < MR; ++m)
      __builtin_amdgcn_global_load_lds((w4_gptr)(g.x + (long)m * g.ldx + src), (w4_lptr)(xs + m * K + gi * 512), 16, 0,
                                       0);
    if constexpr (NORM)
      __builtin_amdgcn_global_load_lds((w4_gptr)(g.gamma + src), (w4_lptr)(gs + gi * 512), 16, 0, 0);
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) (lgkmcnt / expcnt untouched)
  __syncthreads();
  if constexpr (NORM) {
    // RMSNorm with rmsnorm_kernel's rounding: y = bf16(bf16(v * inv) * g), in place in LDS
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      float ss = 0.f;
      for (int c = threadIdx.x; c < nch; c += 256) {
        const uint4_t v = *reinterpret_cast<const uint4_t*>(xs + m * K + c * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float lo = __uint_as_float(v[j] << 16), hi = __uint_as_float(v[j] & 0xffff0000u);
          ss += lo * lo + hi * hi;
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) red[m * 4 + wv] = ss;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const float tot = red[m * 4] + red[m * 4 + 1] + red[m * 4 + 2] + red[m * 4 + 3];
      const float inv = rsqrtf(tot / (float)K + g.eps);
      for (int c = threadIdx.x; c < nch; c += 256) {
        const uint4_t v = *reinterpret_cast<const uint4_t*>(xs + m * K + c * 8);
        const uint4_t gv = *reinterpret_cast<const uint4_t*>(gs + c * 8);
        uint4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float y0 = rbf4(__uint_as_float(v[j] << 16) * inv) * __uint_as_float(gv[j] << 16);
          const float y1 = rbf4(__uint_as_float(v[j] & 0xffff0000u) * inv) * __uint_as_float(gv[j] & 0xffff0000u);
          o[j] = pack_bf2(y0, y1);
        }
        *reinterpret_cast<uint4_t*>(xs + m * K + c * 8) = o;
      }
    }
    __syncthreads();
  }

  // ---- stream W: P pairs of rows per KW waves at a time (KW = 2: wave 0 of a slot takes the first
  // ceil(nk / 2) chunks of K, wave 1 the rest, and their sums meet in LDS).  The round loop is
  // uniform over the workgroup (its barriers); a pair slot past the last pair idles.
  constexpr int PPW = 4 / KW * P;  // pairs per workgroup per round
  const int ps = wv / KW, kh = wv % KW;
  const int jb = kh ? (nk + 1) / 2 : 0;
  const int je = KW == 1 || kh ? nk : (nk + 1) / 2;
  __shared__ float red2[KW > 1 ? 4 / KW : 1][P][MR][2];
  const uint4_t* xl = reinterpret_cast<const uint4_t*>(xs) + lane;
  for (int pb = blockIdx.x * PPW; pb < g.npairs; pb += gridDim.x * PPW) {
    const int p0 = pb + ps * P;
    long ra[P], rb[P];
    int hd[P], head[P], ip[P];
    bool valid[P];
    const uint4_t *wa[P], *wb[P];
    const unsigned char *ea[P], *eb[P];
    lk_f2 acc_a[P][MR], acc_b[P][MR];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      valid[i] = p0 + i < g.npairs;
      ra[i] = rb[i] = 0;
      hd[i] = head[i] = ip[i] = 0;
      // (an idle slot streams the rows of the last pair again, L2 hits, and drops the sums: no
      // divergent copy of the load block)
      pair_rows<MODE>(g, valid[i] ? p0 + i : g.npairs - 1, ra[i], rb[i], hd[i], head[i], ip[i]);
      wa[i] = reinterpret_cast<const uint4_t*>(g.w + ra[i] * (K >> 1)) + lane;
      wb[i] = reinterpret_cast<const uint4_t*>(g.w + rb[i] * (K >> 1)) + lane;
      ea[i] = g.e + ra[i] * nkb + lane;
      eb[i] = g.e + rb[i] * nkb + lane;
#pragma unroll
      for (int m = 0; m < MR; ++m) acc_a[i][m] = acc_b[i][m] = (lk_f2){0.f, 0.f};
    }
    if (valid[0]) {  // (wave-uniform: a wave whose first slot is idle has nothing to stream)
      for (int j0 = jb; j0 < je; j0 += U) {
        uint4_t va[P][U], vb[P][U];
        unsigned sa8[P][U], sb8[P][U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (u && j0 + u >= je) break;  // (wave-uniform: the last group of a wave's chunks may be short)
#pragma unroll
          for (int i = 0; i < P; ++i) {
            va[i][u] = __builtin_nontemporal_load(wa[i] + (j0 + u) * 64);
            vb[i][u] = __builtin_nontemporal_load(wb[i] + (j0 + u) * 64);
            sa8[i][u] = ea[i][(j0 + u) * 64];
            sb8[i][u] = eb[i][(j0 + u) * 64];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (u && j0 + u >= je) break;
#pragma unroll
          for (int m = 0; m < MR; ++m) {
            lk_f2 xf[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) unpack_x4(xl[m * nch + (j0 + u) * 256 + q * 64], xf + 4 * q);
#pragma unroll
            for (int i = 0; i < P; ++i) {
              dot32(va[i][u], __uint_as_float(sa8[i][u] << 23), xf, acc_a[i][m]);
              dot32(vb[i][u], __uint_as_float(sb8[i][u] << 23), xf, acc_b[i][m]);
            }
          }
        }
      }
    }
    float sa[P][MR], sb[P][MR];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        sa[i][m] = wave_sum(acc_a[i][m].x + acc_a[i][m].y);
        sb[i][m] = wave_sum(acc_b[i][m].x + acc_b[i][m].y);
      }
    if constexpr (KW > 1) {
      static_assert(KW == 2, "two K parts");
      if (kh == 1 && lane == 0)
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
          for (int m = 0; m < MR; ++m) {
            red2[ps][i][m][0] = sa[i][m];
            red2[ps][i][m][1] = sb[i][m];
          }
      __syncthreads();
      if (kh == 0)
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
          for (int m = 0; m < MR; ++m) {
            sa[i][m] += red2[ps][i][m][0];
            sb[i][m] += red2[ps][i][m][1];
          }
      __syncthreads();  // (red2 is rewritten next round)
      if (kh != 0) continue;
    }
    if (lane != 0) continue;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      if (!valid[i]) continue;
#pragma unroll
      for (int m = 0; m < MR; ++m)
        epilogue<MODE>(g, m, p0 + i, ra[i], rb[i], hd[i], head[i], ip[i], sa[i][m], sb[i][m]);
    }
  }
}

constexpr int kW4MaxLds = 163840 - 1024;  // dynamic LDS opt-in (the static `red` stays below)
int g_w4_pairs = 0;    // pairs per wave (0: the plan's own)
int g_w4_ksplit = -1;  // two waves per pair (-1: the plan's own)

struct W4Plan {
  int U, KW, P;
};

// (U, KW, P) by M and chunks per row nk = K / 2048.  U is the largest of 4, 2, 1 that a wave's
// share of the chunks fills; M U P <= 8 (beyond it the W registers, the accumulators and the X
// pairs no longer fit in 256 VGPRs and the compiler parks values in AGPRs), P <= 4.  The defaults
// are the measured winners (benchmarks/gemv_w4_bench.py, docs/decode_mxfp4.md): the K split at one
// row of X from 4 chunks per row on, never at two rows; two pairs per wave (four never won), one
// where two would leave fewer than 512 workgroups (N 4,096 and 6,144: the grid, not the loads in
// flight, is what is short there).
W4Plan pick_plan(int M, int npairs, int K) {
  const int nk = K / 2048;
  const bool ks = nk >= 2 && (g_w4_ksplit >= 0 ? g_w4_ksplit != 0 : (M == 1 && nk >= 4));
  const int cw = ks ? (nk + 1) / 2 : nk;  // chunks of the busier wave
  const int U = cw >= 4 ? 4 : cw >= 2 ? 2 : 1;
  const int cap = 8 / (M * U) < 4 ? 8 / (M * U) : 4;
  int P = g_w4_pairs ? g_w4_pairs : (cap < 2 ? cap : 2);
  if (P > cap) P = cap;
  if (!g_w4_pairs && P == 2 && npairs / (4 / (ks ? 2 : 1) * 2) < 512) P = 1;
  return {U, ks ? 2 : 1, P};
}

template <int MR, bool NORM, int MODE>
int launch_plan(const GemvW4Args& a, hipStream_t st) {
  const W4Plan pl = pick_plan(MR, a.npairs, a.K);
  const size_t lds = (size_t)(MR + (NORM ? 1 : 0)) * a.K * 2;  // X rows (+ gamma)
  if (lds > kW4MaxLds) return -3;
  const int ppw = 4 / pl.KW * pl.P;
  int wgs = (a.npairs + ppw - 1) / ppw;
  const int target = 512 * pl.KW;
  if (wgs > target) wgs = target;
#define LK_W4_PLAN(UU, KK, PP)                                                     \
  if constexpr (MR * UU * PP <= 8)                                                 \
    if (pl.U == UU && pl.KW == KK && pl.P == PP) {                                 \
      LK_SET_MAX_LDS((gemv_w4_kernel<MR, NORM, MODE, UU, KK, PP>), kW4MaxLds);     \
      gemv_w4_kernel<MR, NORM, MODE, UU, KK, PP><<<wgs, 256, lds, st>>>(a);        \
      LK_CHECK_LAUNCH();                                                           \
      return 0;                                                                    \
    }
  LK_W4_PLAN(1, 1, 1) LK_W4_PLAN(1, 1, 2) LK_W4_PLAN(1, 1, 4) LK_W4_PLAN(2, 1, 1) LK_W4_PLAN(2, 1, 2)
  LK_W4_PLAN(2, 1, 4) LK_W4_PLAN(4, 1, 1) LK_W4_PLAN(4, 1, 2) LK_W4_PLAN(1, 2, 1) LK_W4_PLAN(1, 2, 2)
  LK_W4_PLAN(1, 2, 4) LK_W4_PLAN(2, 2, 1) LK_W4_PLAN(2, 2, 2) LK_W4_PLAN(2, 2, 4) LK_W4_PLAN(4, 2, 1)
  LK_W4_PLAN(4, 2, 2)
#undef LK_W4_PLAN
  return -4;
}

template <bool NORM, int MODE>
int launch_m(const GemvW4Args& a, hipStream_t st) {
  if (a.M == 1) return launch_plan<1, NORM, MODE>(a, st);
  if (a.M == 2) return launch_plan<2, NORM, MODE>(a, st);
  return -2;
}

}  // namespace

int lk_gemv_w4_supported(int M, int N, int K, int mode) {
  // (X rows and, for the RMSNorm prologue, gamma in LDS)
  if (M < 1 || M > 2 || K < 2048 || K % 2048 || (long)(M + 1) * K * 2 > kW4MaxLds) return 0;
  if (mode < 0 || mode > 3) return 0;
  return N >= 2 && N % 2 == 0;
}

void lk_gemv_w4_set_plan(int pairs, int ksplit) {
  g_w4_pairs = pairs == 1 || pairs == 2 || pairs == 4 ? pairs : 0;
  g_w4_ksplit = ksplit < 0 ? -1 : (ksplit ? 1 : 0);
}

// Return codes (all before any launch): -1 shape (M, K % 2048, odd N, LDS), -5 a null pointer,
// -6 a misaligned pointer or ldx % 8, -7 the mode's own arguments.
int lk_gemv_w4_decode(int mode, const bf16_t* x, long ldx, const bf16_t* gamma, float eps, const unsigned char* wq4,
                      const unsigned char* wexp, int M, int N, int K, bf16_t* out, long ldo, bf16_t* res, long ldr,
                      const int* positions, const float* cos_sin, int Hq, int Hkv, int D, bf16_t* kc, bf16_t* vc,
                      const int* slots, int BS, int neox, hipStream_t st) {
  if (!lk_gemv_w4_supported(M, N, K, mode)) return -1;
  if (!x || !wq4 || !wexp) return -5;
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(wq4) % 16 ||
      (gamma && reinterpret_cast<uintptr_t>(gamma) % 16) || ldx % 8 || ldx < K)
    return -6;
  GemvW4Args a;
  a.x = x;
  a.ldx = ldx;
  a.gamma = gamma;
  a.eps = eps;
  a.w = wq4;
  a.e = wexp;
  a.M = M;
  a.N = N;
  a.K = K;
  a.out = out;
  a.ldo = ldo;
  a.res = res;
  a.ldr = ldr;
  a.npairs = N / 2;
  switch (mode) {
    case 0:
      if (!out || ldo < N) return -7;
      break;
    case 1:
      if (!res || ldr % 2 || ldr < N || reinterpret_cast<uintptr_t>(res) % 4) return -7;
      break;
    case 2:
      if (!out || ldo < N / 2) return -7;
      a.I = N / 2;
      break;
    case 3:
      if (!out || ldo < N || !positions || !cos_sin || D % 2 || D <= 0 || N != (Hq + 2 * Hkv) * D || (kc && BS <= 0) ||
          (kc && !vc))
        return -7;
      a.positions = positions;
      a.cos_sin = cos_sin;
      a.Hq = Hq;
      a.Hkv = Hkv;
      a.D = D;
      a.BS = BS;
      a.neox = neox;
      a.kc = kc;
      a.vc = vc;
      a.slots = slots;
      break;
    default:
      return -1;
  }
  const bool norm = gamma != nullptr;
#define LK_W4_MODE(MD) \
  if (mode == MD) return norm ? launch_m<true, MD>(a, st) : launch_m<false, MD>(a, st);
  LK_W4_MODE(0) LK_W4_MODE(1) LK_W4_MODE(2) LK_W4_MODE(3)
#undef LK_W4_MODE
  return -1;
}
