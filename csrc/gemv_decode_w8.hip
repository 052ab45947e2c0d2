// Decode-step GEMV for one or two rows over FP8 weights: W is [N, K] OCP e4m3 (torch.float8_e4m3fn),
// one byte per weight, with one fp32 scale per output row.  The contract is gemv_decode.hip's (modes
// 0 plain, 1 res +=, 2 SwiGLU, 3 RoPE + paged-KV write; optional RMSNorm prologue; the same pair
// rules and the same rounding points in every epilogue); the weight stream is half the bytes.
//
//   dot[m][row] = wscale[row] * sum_k float(wq[row][k]) * x[m][k]
// The sum runs in fp32 over the raw e4m3 values (every product of an e4m3 and a bf16 value is exact
// in fp32); the row scale multiplies the finished sum once, in fp32, before the epilogue's first
// bf16 rounding.  It is never applied per element.
//
// Layout and lane -> k mapping.  A wave's load instruction still covers one contiguous 1 KB of a W
// row, which is now a BLOCK of 1,024 weights (K % 1024 == 0): in block c lane l owns the 16 weights
//   k = 1024 c + 16 l + (0 .. 15)          (one 16-B nontemporal load),
// which meet 32 B of X: the bf16 elements k .. k + 7 ("half 0") and k + 8 .. k + 15 ("half 1").
// Read from a plain X row those would be two 16-B LDS reads at a 32-B lane stride (a 2-way bank
// conflict each), so the X image in LDS is permuted while it is staged: block c of row m occupies
// elements [1024 c, 1024 c + 1024) of the row's image as
//   [ half 0 of lane 0, half 0 of lane 1, ... half 0 of lane 63 | half 1 of lane 0 ... lane 63 ]
// i.e. the 16-B piece j of the block (elements 8 j .. 8 j + 7) sits at piece (j & 1) * 64 + (j >> 1).
// Both X reads of a chunk are then 16-B reads at a 16-B lane stride: conflict-free.  The staging
// costs nothing: X (and gamma, in the same permuted order) come in by LDS-DMA, where lane l of the
// instruction for (block c, half h) reads global piece 2 l + h and the DMA writes the 64 pieces to
// consecutive LDS addresses.  The RMSNorm prologue is elementwise plus a sum of squares, so it runs
// on the permuted image as it is (x, gamma and the result share the order).
//
// Loads in flight.  A W row is half the bytes of the bf16 kernel's, so one pair of rows at U chunks
// keeps half the loads in flight per lane (K 4,096 has only 4 chunks per lane per row).  A wave
// therefore owns P pairs at a time (P = 2: 16 loads = 256 B per lane at U = 4, the bf16 kernel's
// depth), and the long-K projections keep the two-waves-per-pair K split (KW = 2: K 14,336 is 7
// chunks per lane per wave and row; K 8,192 is 4 with P = 2).  Plans (U, KW, P) by chunks per lane
// nk = K / 1024, at M = 1:  nk % 14 == 0: (7, 2, 1);  nk % 8 == 0: (4, 2, 2);  nk % 4 == 0: (4, 1, 2);
// nk % 7 == 0: (7, 1, 1);  else (1, 1, 2).  At M = 2 the measured winners are one pair per wave and
// no K split: nk % 4 == 0: (4, 1, 1);  nk % 7 == 0: (7, 1, 1).  lk_gemv_w8_set_plan overrides P and
// the K split for measurements (benchmarks/gemv_w8_bench.py; docs/decode_fp8.md has the arms).
//
// VALU.  v_cvt_pk_f32_fp8 turns two e4m3 bytes into two fp32 (a word select picks the half of the
// dword); the X dword unpacks to the matching (lo, hi) fp32 pair by a shift and a mask, and the
// pair is accumulated by one packed FMA (v_pk_fma_f32) into a two-wide accumulator per (row, m):
// per 16 weights of a pair of rows 16 conversions, 8 M unpack ops and 16 M packed FMAs.  All of it
// is plain IEEE fp32 in one fixed order: no atomics, the same bits on every run.
#include "common.h"
#include "kernels.h"

namespace {

struct GemvW8Args {
  const bf16_t* x = nullptr;  // [M, K] input rows (NORM: the residual rows to normalise)
  long ldx = 0;
  const bf16_t* gamma = nullptr;  // NORM weights [K]
  float eps = 0.f;
  const unsigned char* w = nullptr;  // [N, K] row-major e4m3
  const float* wscale = nullptr;     // [N]
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

typedef __attribute__((address_space(3))) void* w8_lptr;
typedef const __attribute__((address_space(1))) void* w8_gptr;

LK_DEVICE float rbf8(float x) { return bf2f(f2bf(x)); }
LK_DEVICE float silu8(float x) { return x / (1.f + __expf(-x)); }

// the (lo, hi) fp32 pairs of four dwords of bf16
LK_DEVICE void unpack_x(const uint4_t xv, lk_f2* xf) {
#pragma unroll
  for (int j = 0; j < 4; ++j) xf[j] = (lk_f2){__uint_as_float(xv[j] << 16), __uint_as_float(xv[j] & 0xffff0000u)};
}

// 16 e4m3 (one 16-B chunk) against the 16 X values xf[0..7] (half 0: xf[0..3], half 1: xf[4..7])
LK_DEVICE void dot16(const uint4_t wv, const lk_f2* xf, lk_f2& acc) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const lk_f2 w0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)wv[j], false);  // bytes 0, 1: k = 4 j, 4 j + 1
    const lk_f2 w1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)wv[j], true);   // bytes 2, 3
    acc = __builtin_elementwise_fma(w0, xf[2 * j], acc);
    acc = __builtin_elementwise_fma(w1, xf[2 * j + 1], acc);
  }
}

// rows of pair p (the pair rules of gemv_decode.hip)
template <int MODE>
LK_DEVICE void pair_rows(const GemvW8Args& g, int p, long& ra, long& rb, int& hd, int& head, int& ip) {
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

// the epilogue of one pair's two finished (scaled) dot products, row m: gemv_decode.hip's arithmetic
template <int MODE>
LK_DEVICE void epilogue(const GemvW8Args& g, int m, int p, long ra, long rb, int hd, int head, int ip, float da,
                        float db) {
  if constexpr (MODE == 0) {
    g.out[(long)m * g.ldo + ra] = f2bf(da);
    g.out[(long)m * g.ldo + rb] = f2bf(db);
  } else if constexpr (MODE == 1) {
    bf16_t* rr = g.res + (long)m * g.ldr;
    const unsigned old = *reinterpret_cast<const unsigned*>(rr + ra);  // (ra even: rb = ra + 1)
    const float va = rbf8(rbf8(da) + __uint_as_float(old << 16));
    const float vb = rbf8(rbf8(db) + __uint_as_float(old & 0xffff0000u));
    *reinterpret_cast<unsigned*>(rr + ra) = pack_bf2(va, vb);
  } else if constexpr (MODE == 2) {
    g.out[(long)m * g.ldo + p] = f2bf(rbf8(silu8(rbf8(da))) * rbf8(db));
  } else {
    bf16_t* orow = g.out + (long)m * g.ldo;
    const float x1 = rbf8(da), x2 = rbf8(db);
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
__global__ __launch_bounds__(256) void gemv_w8_kernel(GemvW8Args g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);  // [MR][K], permuted per 1,024-element block (header)
  __shared__ float red[4 * MR];
  const int K = g.K;
  const int nch = K >> 3;  // 16-B pieces of an X row
  const int nk = K >> 10;  // W chunks per lane per row
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

  // ---- stage X (and gamma) into LDS by LDS-DMA, permuted: instruction gi = 2 c + h takes the 64
  // pieces 2 l + h of block c and lands them at pieces [64 gi, 64 gi + 64) of the row's image
  bf16_t* gs = xs + MR * K;  // NORM: gamma [K], the same order
  for (int gi = wv; gi < (nch >> 6); gi += 4) {
    const int src = (gi >> 1) * 1024 + (2 * lane + (gi & 1)) * 8;  // element of the row
#pragma unroll
    for (int m = 0; m < MR; ++m)
      __builtin_amdgcn_global_load_lds((w8_gptr)(g.x + (long)m * g.ldx + src), (w8_lptr)(xs + m * K + gi * 512), 16, 0,
                                       0);
    if constexpr (NORM)
      __builtin_amdgcn_global_load_lds((w8_gptr)(g.gamma + src), (w8_lptr)(gs + gi * 512), 16, 0, 0);
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
          const float y0 = rbf8(__uint_as_float(v[j] << 16) * inv) * __uint_as_float(gv[j] << 16);
          const float y1 = rbf8(__uint_as_float(v[j] & 0xffff0000u) * inv) * __uint_as_float(gv[j] & 0xffff0000u);
          o[j] = pack_bf2(y0, y1);
        }
        *reinterpret_cast<uint4_t*>(xs + m * K + c * 8) = o;
      }
    }
    __syncthreads();
  }

  // ---- stream W: P pairs of rows per KW waves at a time (KW = 2: the two waves take one half of K
  // each and their sums meet in LDS).  The round loop is uniform over the workgroup (its barriers);
  // a pair slot past the last pair idles.
  constexpr int PPW = 4 / KW * P;  // pairs per workgroup per round
  const int ps = wv / KW, kh = wv % KW;
  const int kc_w = nk / KW;  // chunks per lane of this wave's part of K
  const int jb = kh * kc_w;
  __shared__ float red2[KW > 1 ? 4 / KW : 1][P][MR][2];
  const uint4_t* xl = reinterpret_cast<const uint4_t*>(xs) + lane;
  for (int pb = blockIdx.x * PPW; pb < g.npairs; pb += gridDim.x * PPW) {
    const int p0 = pb + ps * P;
    long ra[P], rb[P];
    int hd[P], head[P], ip[P];
    bool valid[P];
    const uint4_t *wa[P], *wb[P];
    lk_f2 acc_a[P][MR], acc_b[P][MR];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      valid[i] = p0 + i < g.npairs;
      ra[i] = rb[i] = 0;
      hd[i] = head[i] = ip[i] = 0;
      // (an idle slot streams the rows of the last pair again, L2 hits, and drops the sums: no
      // divergent copy of the load block)
      pair_rows<MODE>(g, valid[i] ? p0 + i : g.npairs - 1, ra[i], rb[i], hd[i], head[i], ip[i]);
      wa[i] = reinterpret_cast<const uint4_t*>(g.w + ra[i] * K) + lane;
      wb[i] = reinterpret_cast<const uint4_t*>(g.w + rb[i] * K) + lane;
#pragma unroll
      for (int m = 0; m < MR; ++m) acc_a[i][m] = acc_b[i][m] = (lk_f2){0.f, 0.f};
    }
    if (valid[0]) {  // (wave-uniform: a wave whose first slot is idle has nothing to stream)
      for (int j0 = jb; j0 < jb + kc_w; j0 += U) {
        uint4_t va[P][U], vb[P][U];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int i = 0; i < P; ++i) {
            va[i][u] = __builtin_nontemporal_load(wa[i] + (j0 + u) * 64);
            vb[i][u] = __builtin_nontemporal_load(wb[i] + (j0 + u) * 64);
          }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int m = 0; m < MR; ++m) {
            lk_f2 xf[8];
            unpack_x(xl[m * nch + (j0 + u) * 128], xf);
            unpack_x(xl[m * nch + (j0 + u) * 128 + 64], xf + 4);
#pragma unroll
            for (int i = 0; i < P; ++i) {
              dot16(va[i][u], xf, acc_a[i][m]);
              dot16(vb[i][u], xf, acc_b[i][m]);
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
      static_assert(KW == 2, "two K halves");
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
      const float sca = g.wscale[ra[i]], scb = g.wscale[rb[i]];
#pragma unroll
      for (int m = 0; m < MR; ++m)
        epilogue<MODE>(g, m, p0 + i, ra[i], rb[i], hd[i], head[i], ip[i], sa[i][m] * sca, sb[i][m] * scb);
    }
  }
}

constexpr int kW8MaxLds = 163840 - 1024;  // dynamic LDS opt-in (the static `red` stays below)
int g_w8_pairs = 0;    // pairs per wave (0: the plan's own), where that arm is built
int g_w8_ksplit = -1;  // two waves per pair on the long-K projections (-1: the plan's own)

struct W8Plan {
  int U, KW, P;
};

// Measured (benchmarks/gemv_w8_bench.py, docs/decode_fp8.md): one row of X streams fastest with two
// pairs per wave and the K split; two rows double the FMAs and the X registers per chunk, and one
// pair per wave without the K split wins there.
W8Plan pick_plan(int M, int K) {
  const int nk = K / 1024;
  const bool ks = g_w8_ksplit >= 0 ? g_w8_ksplit != 0 : M == 1;
  const int p4 = g_w8_pairs ? g_w8_pairs : (M == 1 ? 2 : 1);
  if (ks && nk % 14 == 0) return {7, 2, g_w8_pairs == 2 ? 2 : 1};
  if (ks && nk % 8 == 0) return {4, 2, 2};
  if (nk % 4 == 0) return {4, 1, p4};
  if (nk % 7 == 0) return {7, 1, 1};
  return {1, 1, 2};
}

template <int MR, bool NORM, int MODE>
int launch_plan(const GemvW8Args& a, hipStream_t st) {
  const W8Plan pl = pick_plan(MR, a.K);
  const size_t lds = (size_t)(MR + (NORM ? 1 : 0)) * a.K * 2;  // X rows (+ gamma)
  if (lds > kW8MaxLds) return -3;
  const int ppw = 4 / pl.KW * pl.P;
  int wgs = (a.npairs + ppw - 1) / ppw;
  const int target = 512 * pl.KW;
  if (wgs > target) wgs = target;
#define LK_W8_PLAN(UU, KK, PP)                                                     \
  if (pl.U == UU && pl.KW == KK && pl.P == PP) {                                   \
    LK_SET_MAX_LDS((gemv_w8_kernel<MR, NORM, MODE, UU, KK, PP>), kW8MaxLds);       \
    gemv_w8_kernel<MR, NORM, MODE, UU, KK, PP><<<wgs, 256, lds, st>>>(a);          \
  } else
  LK_W8_PLAN(4, 1, 2) LK_W8_PLAN(7, 2, 1) LK_W8_PLAN(4, 2, 2) LK_W8_PLAN(7, 1, 1) LK_W8_PLAN(1, 1, 2)
  LK_W8_PLAN(4, 1, 1) LK_W8_PLAN(7, 2, 2) return -4;
#undef LK_W8_PLAN
  LK_CHECK_LAUNCH();
  return 0;
}

template <bool NORM, int MODE>
int launch_m(const GemvW8Args& a, hipStream_t st) {
  if (a.M == 1) return launch_plan<1, NORM, MODE>(a, st);
  if (a.M == 2) return launch_plan<2, NORM, MODE>(a, st);
  return -2;
}

}  // namespace

int lk_gemv_w8_supported(int M, int N, int K, int mode) {
  // (X rows and, for the RMSNorm prologue, gamma in LDS)
  if (M < 1 || M > 2 || K < 1024 || K % 1024 || (long)(M + 1) * K * 2 > kW8MaxLds) return 0;
  if (mode < 0 || mode > 3) return 0;
  return N >= 2 && N % 2 == 0;
}

void lk_gemv_w8_set_plan(int pairs, int ksplit) {
  g_w8_pairs = pairs == 1 || pairs == 2 ? pairs : 0;
  g_w8_ksplit = ksplit < 0 ? -1 : (ksplit ? 1 : 0);
}

// Return codes (all before any launch): -1 shape (M, K % 1024, odd N, LDS), -5 a null pointer,
// -6 a misaligned pointer or ldx % 8, -7 the mode's own arguments.
int lk_gemv_w8_decode(int mode, const bf16_t* x, long ldx, const bf16_t* gamma, float eps, const unsigned char* wq,
                      const float* wscale, int M, int N, int K, bf16_t* out, long ldo, bf16_t* res, long ldr,
                      const int* positions, const float* cos_sin, int Hq, int Hkv, int D, bf16_t* kc, bf16_t* vc,
                      const int* slots, int BS, int neox, hipStream_t st) {
  if (!lk_gemv_w8_supported(M, N, K, mode)) return -1;
  if (!x || !wq || !wscale) return -5;
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(wq) % 16 ||
      reinterpret_cast<uintptr_t>(wscale) % 4 || (gamma && reinterpret_cast<uintptr_t>(gamma) % 16) || ldx % 8 ||
      ldx < K)
    return -6;
  GemvW8Args a;
  a.x = x;
  a.ldx = ldx;
  a.gamma = gamma;
  a.eps = eps;
  a.w = wq;
  a.wscale = wscale;
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
#define LK_W8_MODE(MD) \
  if (mode == MD) return norm ? launch_m<true, MD>(a, st) : launch_m<false, MD>(a, st);
  LK_W8_MODE(0) LK_W8_MODE(1) LK_W8_MODE(2) LK_W8_MODE(3)
#undef LK_W8_MODE
  return -1;
}
