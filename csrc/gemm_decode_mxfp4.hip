// Decode-step GEMM for 3 to 16 rows over OCP MXFP4 weights, on the matrix unit.  The contract is
// gemv_decode_mxfp4.hip's (modes 0 plain, 1 res +=, 2 SwiGLU, 3 RoPE + paged-KV write; optional
// RMSNorm prologue; the same pair rules, the same rounding points in every epilogue, the same
// operands: wq4 [N, K / 2] e2m1 pairs, low nibble first, wexp [N, K / 32] e8m0, E never 0 or 0xFF).
//
//   dot[m][row] = sum_k (e2m1(wq4[row][k]) * 2^(E[row][k / 32] - 127)) * x[m][k]
// Each e2m1 block is converted once to bf16 by v_cvt_scalef32_pk_bf16_fp4 (exact: e2m1 times a power
// of two is a bf16 value) and v_mfma_f32_16x16x32_bf16 serves up to 16 rows of X for the cost of one.
//
// Work split.  W is the MFMA's A operand (16 weight rows x 32 k), X its B operand (column j = X row
// j; lanes with j >= M read row M - 1 and never store).  A lane's four accumulators are the four
// consecutive weight rows 4 (l / 16) + r of X row l % 16, so the adjacent-row pairs of modes 0 / 1,
// of the interleaved RoPE and of the V heads sit in one lane and every store is 8 B.  A wave's unit
// of work is 32 weight rows, two A tiles, chosen so that both members of every pair meet in one
// lane with no shuffle:
//   modes 0 / 1, V heads, interleaved RoPE   rows 32 u .. 32 u + 15 and 32 u + 16 .. 32 u + 31
//   mode 2                                   gate rows 16 t ..  and up rows I + 16 t ..
//   mode 3, rotate-half Q / K heads          head D + 16 t ..  and head D + D / 2 + 16 t ..
// A wave owns P units at a time and reuses each B fragment across them.  The NW = 4 waves of a
// workgroup are NW / KW slots of KW waves; the waves of a slot split the K steps of the slot's units
// (KW 1 / 2 / 4) and their partial tiles are summed through LDS in wave order.  Nothing is split
// across workgroups: fp32 in one fixed order, no atomics, the same bits on every run.
//
// W path: HBM -> VGPR, no LDS.  A K step is 256 weights of a row, one 128-B line.  Lane
// (r = l % 16, g = l / 16) issues two 16-B nontemporal loads per tile and step c: MX blocks 8 c + g
// and 8 c + 4 + g of row r, each exactly one block with one scale.  The MFMA does not care which k
// a lane group holds as long as A and B agree, so one 16-B load feeds four MFMAs: dword s of the
// load is k = 32 blk + 8 s .. + 7, and the B fragment of that MFMA in the same lane is the 16 B of
// X at that k.  A step's eight scale bytes of a row are one aligned 8-B load per lane (the four
// lanes of a row share the address); lane group g takes byte g of each half, and the conversion's
// scale operand is the f32 E << 23.  Per dword four conversions (byte b gives elements 2 b, 2 b + 1
// of the fragment, low nibble first) make the 8-wide A fragment.
//
// X path.  NORM (QKV, gate_up): the M rows and gamma are staged whole by LDS-DMA at a row stride of
// 2 K + 16 B (the 16 rows of one k group fall in distinct 16-B bank groups), normalised in place
// with rmsnorm_kernel's rounding, and the B fragments are 16-B LDS reads.  Not NORM (O, down, LM
// head): the B fragments come from global memory (X is L2-resident), 16 B per lane, prefetched with
// the W loads, so K is not bounded by LDS.
//
// Loads in flight.  Two register sets ping-pong, U steps each: while one set's MFMAs run, the next
// U steps of all P units are in flight (P U 64 B of W per lane, plus 128 U B of X when not NORM).
// pick_plan holds the defaults; lk_gemm_w4_set_plan overrides them for measurements
// (benchmarks/gemm_w4_bench.py; docs/decode_mxfp4_rows.md has the arms).
#include "common.h"
#include "kernels.h"

namespace {

struct GemmW4Args {
  const bf16_t* x = nullptr;  // [M, K] input rows (NORM: the residual rows to normalise)
  long ldx = 0;
  const bf16_t* gamma = nullptr;  // NORM weights [K]
  float eps = 0.f;
  const unsigned char* w = nullptr;  // [N, K / 2] row-major e2m1 pairs
  const unsigned char* e = nullptr;  // [N, K / 32] e8m0 block scales
  int M = 0, N = 0, K = 0;
  int nunits = 0;
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

constexpr int kNW = 4;  // waves per workgroup
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int uint2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* g4_lptr;
typedef const __attribute__((address_space(1))) void* g4_gptr;

LK_DEVICE float rbf4(float x) { return bf2f(f2bf(x)); }
LK_DEVICE float silu4(float x) { return x / (1.f + __expf(-x)); }
LK_DEVICE float lo16(unsigned v) { return __uint_as_float(v << 16); }
LK_DEVICE float hi16(unsigned v) { return __uint_as_float(v & 0xffff0000u); }

// eight e2m1 of one dword times the block scale: the A fragment of one MFMA (element 2 b + h is
// nibble h of byte b)
LK_DEVICE bf16x8_t cvt8(unsigned d, float scale) {
  const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0);
  const bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1);
  const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2);
  const bf16x2_t e = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3);
  return (bf16x8_t){a.x, a.y, b.x, b.y, c.x, c.y, e.x, e.y};
}

// first weight rows of the two A tiles of unit u (header)
template <int MODE>
LK_DEVICE void unit_rows(const GemmW4Args& g, int u, long& r0, long& r1) {
  if constexpr (MODE == 2) {
    r0 = 16L * u;
    r1 = (long)g.I + 16L * u;
  } else if constexpr (MODE == 3) {
    const int uph = g.D >> 5;  // units per head
    const int head = u / uph, t = u - head * uph;
    if (g.neox && head < g.Hq + g.Hkv) {
      r0 = (long)head * g.D + 16 * t;
      r1 = r0 + (g.D >> 1);
    } else {
      r0 = (long)head * g.D + 32 * t;
      r1 = r0 + 16;
    }
  } else {
    r0 = 32L * u;
    r1 = r0 + 16;
  }
}

LK_DEVICE void store4(bf16_t* p, const float* v) {
  *reinterpret_cast<uint2_t*>(p) = (uint2_t){pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
}

// The epilogue of one unit in one lane: X row m, weight rows r0 + 4 g + (0 .. 3) in a[0] and
// r1 + 4 g + (0 .. 3) in a[1].  gemv_decode_mxfp4.hip's arithmetic, pair by pair.
template <int MODE>
LK_DEVICE void epilogue(const GemmW4Args& g, int m, int grp, long r0, long r1, const floatx4 (&a)[2]) {
  const long ra = r0 + 4 * grp, rb = r1 + 4 * grp;
  float va[4], vb[4];
  if constexpr (MODE == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) va[q] = a[0][q], vb[q] = a[1][q];
    store4(g.out + (long)m * g.ldo + ra, va);
    store4(g.out + (long)m * g.ldo + rb, vb);
  } else if constexpr (MODE == 1) {
    bf16_t* rr = g.res + (long)m * g.ldr;
    const uint2_t oa = *reinterpret_cast<const uint2_t*>(rr + ra), ob = *reinterpret_cast<const uint2_t*>(rr + rb);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      va[q] = rbf4(rbf4(a[0][q]) + (q & 1 ? hi16(oa[q >> 1]) : lo16(oa[q >> 1])));
      vb[q] = rbf4(rbf4(a[1][q]) + (q & 1 ? hi16(ob[q >> 1]) : lo16(ob[q >> 1])));
    }
    store4(rr + ra, va);
    store4(rr + rb, vb);
  } else if constexpr (MODE == 2) {
#pragma unroll
    for (int q = 0; q < 4; ++q) va[q] = rbf4(silu4(rbf4(a[0][q]))) * rbf4(a[1][q]);
    store4(g.out + (long)m * g.ldo + ra, va);  // (gate row = output column)
  } else {
    bf16_t* orow = g.out + (long)m * g.ldo;
    const int head = (int)(r0 / g.D), hd = g.D >> 1;
    const int da = (int)(ra - (long)head * g.D), db = (int)(rb - (long)head * g.D);
    const int slot = g.slots ? g.slots[m] : -1;
    const long blk = slot >= 0 ? slot / g.BS : 0;
    const int off = slot >= 0 ? slot % g.BS : 0;
    if (head >= g.Hq + g.Hkv) {  // V: copied (into the row and the cache)
#pragma unroll
      for (int q = 0; q < 4; ++q) va[q] = a[0][q], vb[q] = a[1][q];
      store4(orow + ra, va);
      store4(orow + rb, vb);
      if (g.vc && slot >= 0) {
        bf16_t* vd = g.vc + ((blk * g.Hkv + (head - g.Hq - g.Hkv)) * g.BS + off) * g.D;
        store4(vd + da, va);
        store4(vd + db, vb);
      }
      return;
    }
    const float* cs = g.cos_sin + (long)g.positions[m] * g.D;  // [cos(D/2) | sin(D/2)]
    float ya[4], yb[4];  // rotated
    if (g.neox) {  // pair q: rows ra + q and rb + q = ra + q + D / 2
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float x1 = rbf4(a[0][q]), x2 = rbf4(a[1][q]);
        const float c = cs[da + q], s = cs[hd + da + q];
        va[q] = x1, vb[q] = x2;
        ya[q] = x1 * c - x2 * s, yb[q] = x2 * c + x1 * s;
      }
    } else {  // pairs of adjacent rows within each tile
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float x1 = rbf4(a[0][2 * q]), x2 = rbf4(a[0][2 * q + 1]);
        const float c = cs[(da >> 1) + q], s = cs[hd + (da >> 1) + q];
        va[2 * q] = x1, va[2 * q + 1] = x2;
        ya[2 * q] = x1 * c - x2 * s, ya[2 * q + 1] = x2 * c + x1 * s;
        const float z1 = rbf4(a[1][2 * q]), z2 = rbf4(a[1][2 * q + 1]);
        const float c2 = cs[(db >> 1) + q], s2 = cs[hd + (db >> 1) + q];
        vb[2 * q] = z1, vb[2 * q + 1] = z2;
        yb[2 * q] = z1 * c2 - z2 * s2, yb[2 * q + 1] = z2 * c2 + z1 * s2;
      }
    }
    if (head < g.Hq) {
      store4(orow + ra, ya);
      store4(orow + rb, yb);
    } else {  // K: unrotated in the row, rotated in the cache
      store4(orow + ra, va);
      store4(orow + rb, vb);
      if (g.kc && slot >= 0) {
        bf16_t* kd = g.kc + ((blk * g.Hkv + (head - g.Hq)) * g.BS + off) * g.D;
        store4(kd + da, ya);
        store4(kd + db, yb);
      }
    }
  }
}

// one register set of the ping-pong: U steps of P units (two tiles, two blocks each), their scale
// bytes, and (not NORM) the X fragments of the steps
template <bool NORM, int P, int U>
struct W4Set {
  uint4_t w[U][P][2][2];
  uint2_t s[U][P][2];
  bf16x8_t x[NORM ? 1 : U][2][4];
};

template <bool NORM, int MODE, int KW, int P, int U>
__global__ __launch_bounds__(64 * kNW) void gemm_w4_kernel(GemmW4Args g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int K = g.K, M = g.M;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 15, grp = lane >> 4;
  const int xrow = r < M ? r : M - 1;
  const int lds_ld = K + 8;  // LDS row stride of the X image, elements
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);  // NORM: [M][K + 8], then gamma [K]
  floatx4* red = reinterpret_cast<floatx4*>(smem + (NORM ? ((size_t)M * lds_ld + K) * 2 : 0));

  if constexpr (NORM) {
    // ---- stage X and gamma by LDS-DMA: instruction gi lands pieces [64 gi, 64 gi + 64) of a row
    __shared__ float ssum[16 * kNW];
    bf16_t* gs = xs + M * lds_ld;
    const int nch = K >> 3;  // 16-B pieces of a row (a multiple of 32: the last instruction may be half)
    for (int gi = wv; gi < ((nch + 63) >> 6); gi += kNW) {
      const int pc = gi * 64 + lane;
      if (pc < nch) {
        for (int m = 0; m < M; ++m)
          __builtin_amdgcn_global_load_lds((g4_gptr)(g.x + (long)m * g.ldx + pc * 8),
                                           (g4_lptr)(xs + m * lds_ld + gi * 512), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((g4_gptr)(g.gamma + pc * 8), (g4_lptr)(gs + gi * 512), 16, 0, 0);
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) (lgkmcnt / expcnt untouched)
    __syncthreads();
    // RMSNorm with rmsnorm_kernel's rounding: y = bf16(bf16(v * inv) * g), in place in LDS
    for (int m = 0; m < M; ++m) {
      float ss = 0.f;
      for (int c = threadIdx.x; c < nch; c += 64 * kNW) {
        const uint4_t v = *reinterpret_cast<const uint4_t*>(xs + m * lds_ld + c * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) ss += lo16(v[j]) * lo16(v[j]) + hi16(v[j]) * hi16(v[j]);
      }
      ss = wave_sum(ss);
      if (lane == 0) ssum[m * kNW + wv] = ss;
    }
    __syncthreads();
    for (int m = 0; m < M; ++m) {
      const float tot = ssum[m * kNW] + ssum[m * kNW + 1] + ssum[m * kNW + 2] + ssum[m * kNW + 3];
      const float inv = rsqrtf(tot / (float)K + g.eps);
      for (int c = threadIdx.x; c < nch; c += 64 * kNW) {
        const uint4_t v = *reinterpret_cast<const uint4_t*>(xs + m * lds_ld + c * 8);
        const uint4_t gv = *reinterpret_cast<const uint4_t*>(gs + c * 8);
        uint4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = pack_bf2(rbf4(lo16(v[j]) * inv) * lo16(gv[j]), rbf4(hi16(v[j]) * inv) * hi16(gv[j]));
        *reinterpret_cast<uint4_t*>(xs + m * lds_ld + c * 8) = o;
      }
    }
    __syncthreads();
  }

  // ---- stream W.  Slot ps of the workgroup owns P units per round, wave kh of the slot the K
  // steps [sb, se).  The round loop is uniform over the workgroup (its barriers); a unit past the
  // last one streams the last unit again (L2 hits) and drops the sums.
  constexpr int SLOTS = kNW / KW, UPW = SLOTS * P;
  const int ps = wv / KW, kh = wv % KW;
  const int ns = K >> 8;
  const int per = (ns + KW - 1) / KW;
  const int sb = kh * per, se = sb + per < ns ? sb + per : ns;
  const long wrow = K >> 1;  // bytes of a W row
  const int erow = K >> 5;   // scale bytes of a W row
  const bf16_t* xg = NORM ? xs + xrow * lds_ld : g.x + (long)xrow * g.ldx;  // this lane's X row
  for (int ub = blockIdx.x * UPW; ub < g.nunits; ub += gridDim.x * UPW) {
    const int u0 = ub + ps * P;
    long r0[P], r1[P];
    const unsigned char* wp[P][2];
    const unsigned char* ep[P][2];
    floatx4 acc[P][2];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      unit_rows<MODE>(g, u0 + i < g.nunits ? u0 + i : g.nunits - 1, r0[i], r1[i]);
      wp[i][0] = g.w + (r0[i] + r) * wrow + grp * 16;
      wp[i][1] = g.w + (r1[i] + r) * wrow + grp * 16;
      ep[i][0] = g.e + (r0[i] + r) * erow;
      ep[i][1] = g.e + (r1[i] + r) * erow;
      acc[i][0] = acc[i][1] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    auto load = [&](W4Set<NORM, P, U>& b, int c0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u;
        if (c >= se) break;  // (wave-uniform)
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            b.w[u][i][t][0] = __builtin_nontemporal_load(reinterpret_cast<const uint4_t*>(wp[i][t] + c * 128));
            b.w[u][i][t][1] = __builtin_nontemporal_load(reinterpret_cast<const uint4_t*>(wp[i][t] + c * 128 + 64));
            b.s[u][i][t] = *reinterpret_cast<const uint2_t*>(ep[i][t] + c * 8);
          }
        if constexpr (!NORM) {
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < 4; ++s)
              b.x[u][h][s] = *reinterpret_cast<const bf16x8_t*>(xg + 32 * (8 * c + 4 * h + grp) + 8 * s);
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch issued ahead of the MFMAs below
    };
    auto compute = [&](W4Set<NORM, P, U>& b, int c0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u;
        if (c >= se) break;
        if constexpr (NORM) {
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < 4; ++s)
              b.x[0][h][s] = *reinterpret_cast<const bf16x8_t*>(xg + 32 * (8 * c + 4 * h + grp) + 8 * s);
        }
        const int xu = NORM ? 0 : u;
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const float scale = __uint_as_float(((b.s[u][i][t][h] >> (8 * grp)) & 0xffu) << 23);
#pragma unroll
              for (int s = 0; s < 4; ++s)
                acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8(b.w[u][i][t][h][s], scale), b.x[xu][h][s],
                                                                    acc[i][t], 0, 0, 0);
            }
      }
    };
    // ping-pong register sets, no copies: the next U steps are in flight under this set's MFMAs
    W4Set<NORM, P, U> sa, sc;
    load(sa, sb);
    for (int c = sb; c < se; c += 2 * U) {
      load(sc, c + U);
      compute(sa, c);
      load(sa, c + 2 * U);
      compute(sc, c + U);
    }
    if constexpr (KW > 1) {  // partial tiles of waves 1 .. KW - 1 of a slot, added in wave order
      if (kh > 0)
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
          for (int t = 0; t < 2; ++t) red[(((ps * (KW - 1) + kh - 1) * P + i) * 2 + t) * 64 + lane] = acc[i][t];
      __syncthreads();
      if (kh == 0)
#pragma unroll
        for (int k = 0; k < KW - 1; ++k)
#pragma unroll
          for (int i = 0; i < P; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[i][t] += red[(((ps * (KW - 1) + k) * P + i) * 2 + t) * 64 + lane];
      __syncthreads();  // (red is rewritten next round)
    }
    if (kh == 0 && r < M) {
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (u0 + i < g.nunits) epilogue<MODE>(g, r, grp, r0[i], r1[i], acc[i]);
    }
  }
}

constexpr int kG4MaxImage = 163840 - 1024;  // the NORM image: M (2 K + 16) + 2 K bytes
constexpr int kG4MaxLds = 163840 - 512;     // dynamic LDS opt-in (image + partial tiles; `ssum` stays below)
int g_plan_kw = 0, g_plan_p = 0, g_plan_u = 0;  // measurement overrides (0: the plan's own)

struct G4Plan {
  int KW, P, U;
};

size_t image_bytes(int M, int K) { return (size_t)M * (2 * K + 16) + 2 * (size_t)K; }
size_t red_bytes(const G4Plan& p) { return p.KW > 1 ? (size_t)(kNW / p.KW) * (p.KW - 1) * p.P * 2 * 1024 : 0; }

// (KW, P, U) by units, K steps and the X source.  Two units per wave where that still leaves a round
// for each of 256 workgroups; the K split that brings the rounds up to 256 (N 4,096: 128 units, KW 4,
// one unit per workgroup); two steps per register set under the NORM image, where one workgroup
// fills a CU and depth must come from the wave, one where the X fragments travel with W.
// docs/decode_mxfp4_rows.md has the measured arms.
G4Plan pick_plan(int M, int nunits, int K, bool norm) {
  const int ns = K / 256;
  G4Plan p;
  p.P = g_plan_p ? g_plan_p : (nunits >= 2 * kNW * 256 ? 2 : 1);
  if (g_plan_kw) {
    p.KW = g_plan_kw;
  } else {
    p.KW = 1;
    while (p.KW < 4 && nunits * p.KW / (kNW * p.P) < 256) p.KW *= 2;
  }
  while (p.KW > 1 && p.KW > ns) p.KW /= 2;
  const int steps = (ns + p.KW - 1) / p.KW;
  p.U = g_plan_u ? g_plan_u : (norm && steps >= 4 ? 2 : 1);
  if (p.U > 1 && steps < 2) p.U = 1;
  // (the partial tiles share LDS with the NORM image: no K split where they do not fit)
  if (norm && image_bytes(M, K) + red_bytes(p) > (size_t)kG4MaxLds) p.KW = 1;
  return p;
}

template <bool NORM, int MODE>
int launch_plan(const GemmW4Args& a, hipStream_t st) {
  const G4Plan pl = pick_plan(a.M, a.nunits, a.K, NORM);
  const size_t lds = (NORM ? image_bytes(a.M, a.K) : 0) + red_bytes(pl);
  if (lds > (size_t)kG4MaxLds) return -3;
  const int upw = kNW / pl.KW * pl.P;
  const int rounds = (a.nunits + upw - 1) / upw;
  // workgroups resident at once: by the LDS image under NORM, two per CU otherwise; every workgroup
  // takes the same number of rounds
  int per_cu = 2;
  if (NORM) per_cu = (int)(163840 / (lds + 512)) < 2 ? 1 : 2;
  const int cap = 256 * per_cu;
  const int rpw = (rounds + cap - 1) / cap;
  const int wgs = (rounds + rpw - 1) / rpw;
#define LK_G4_PLAN(KK, PP, UU)                                                  \
  if (pl.KW == KK && pl.P == PP && pl.U == UU) {                                \
    LK_SET_MAX_LDS((gemm_w4_kernel<NORM, MODE, KK, PP, UU>), kG4MaxLds);        \
    gemm_w4_kernel<NORM, MODE, KK, PP, UU><<<wgs, 64 * kNW, lds, st>>>(a);      \
    LK_CHECK_LAUNCH();                                                          \
    return 0;                                                                   \
  }
  LK_G4_PLAN(1, 1, 1) LK_G4_PLAN(1, 1, 2) LK_G4_PLAN(1, 2, 1) LK_G4_PLAN(1, 2, 2)
  LK_G4_PLAN(2, 1, 1) LK_G4_PLAN(2, 1, 2) LK_G4_PLAN(2, 2, 1) LK_G4_PLAN(2, 2, 2)
  LK_G4_PLAN(4, 1, 1) LK_G4_PLAN(4, 1, 2) LK_G4_PLAN(4, 2, 1) LK_G4_PLAN(4, 2, 2)
#undef LK_G4_PLAN
  return -4;
}

// what the kernel can run
bool shape_ok(int M, int N, int K, int mode, int norm) {
  if (M < 3 || M > 16 || K < 256 || K % 256 || N < 32 || N % 32) return false;
  if (mode < 0 || mode > 3) return false;
  return !norm || image_bytes(M, K) <= (size_t)kG4MaxImage;
}

// The (shape class, row bucket) pairs measured slower than, or within the spread of, the bf16 route
// (benchmarks/gemm_w4_bench.py; the table is in docs/decode_mxfp4_rows.md): they stay on bf16.
// Buckets are the decode graphs' 4 / 8 / 16.  A shape that was not measured is not routed back.
struct G4RoutedBack {
  int N, K, mlo, mhi;
};
constexpr G4RoutedBack kRoutedBack[] = {
    {6144, 4096, 3, 16},   // Llama-3-8B QKV: the 16-row X image per 32 weight rows costs more than the bytes saved
    {4096, 4096, 3, 4},    // O at bucket 4: faster in every round but one bf16 round widened the spread past the gain
    {4096, 14336, 9, 16},  // down at bucket 16: 26.7 against 26.1 us
};

bool routed(int M, int N, int K) {
  for (const G4RoutedBack& r : kRoutedBack)
    if (r.N == N && r.K == K && M >= r.mlo && M <= r.mhi) return false;
  return true;
}

}  // namespace

int lk_gemm_w4_supported(int M, int N, int K, int mode, int norm) {
  return shape_ok(M, N, K, mode, norm) && routed(M, N, K);
}

void lk_gemm_w4_set_plan(int kw, int units, int steps) {
  g_plan_kw = kw == 1 || kw == 2 || kw == 4 ? kw : 0;
  g_plan_p = units == 1 || units == 2 ? units : 0;
  g_plan_u = steps == 1 || steps == 2 ? steps : 0;
}

// Return codes (all before any launch): -1 shape (M, K % 256, N % 32, the NORM image), -5 a null
// pointer, -6 a misaligned pointer or row stride, -7 the mode's own arguments.
int lk_gemm_w4_decode(int mode, const bf16_t* x, long ldx, const bf16_t* gamma, float eps, const unsigned char* wq4,
                      const unsigned char* wexp, int M, int N, int K, bf16_t* out, long ldo, bf16_t* res, long ldr,
                      const int* positions, const float* cos_sin, int Hq, int Hkv, int D, bf16_t* kc, bf16_t* vc,
                      const int* slots, int BS, int neox, hipStream_t st) {
  if (!shape_ok(M, N, K, mode, gamma != nullptr)) return -1;
  if (!x || !wq4 || !wexp) return -5;
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(wq4) % 16 ||
      reinterpret_cast<uintptr_t>(wexp) % 8 || (gamma && reinterpret_cast<uintptr_t>(gamma) % 16) || ldx % 8 || ldx < K)
    return -6;
  // (every store is 8 B: four consecutive bf16 of a row)
  if ((out && (reinterpret_cast<uintptr_t>(out) % 8 || ldo % 4)) || (res && (reinterpret_cast<uintptr_t>(res) % 8 || ldr % 4)))
    return -6;
  GemmW4Args a;
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
  a.nunits = N / 32;
  switch (mode) {
    case 0:
      if (!out || ldo < N) return -7;
      break;
    case 1:
      if (!res || ldr < N) return -7;
      break;
    case 2:
      if (!out || ldo < N / 2 || (N / 2) % 16) return -7;
      a.I = N / 2;
      break;
    case 3:
      if (!out || ldo < N || !positions || !cos_sin || D <= 0 || D % 32 || N != (Hq + 2 * Hkv) * D || (kc && BS <= 0) ||
          (kc && !vc) || reinterpret_cast<uintptr_t>(kc) % 8 || reinterpret_cast<uintptr_t>(vc) % 8)
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
#define LK_G4_MODE(MD) \
  if (mode == MD) return norm ? launch_plan<true, MD>(a, st) : launch_plan<false, MD>(a, st);
  LK_G4_MODE(0) LK_G4_MODE(1) LK_G4_MODE(2) LK_G4_MODE(3)
#undef LK_G4_MODE
  return -1;
}
