// Decode-step GEMM for 3 to 16 rows over FP8 weights, on the matrix unit.  The contract is
// gemv_decode_w8.hip's (modes 0 plain, 1 res +=, 2 SwiGLU, 3 RoPE + paged-KV write; optional RMSNorm
// prologue; the same pair rules, the same rounding points in every epilogue, the same operands: wq
// [N, K] OCP e4m3, one byte per weight, wscale f32 [N]).
//
//   dot[m][row] = wscale[row] * sum_k float(wq[row][k]) * x[m][k]
// e4m3 to bf16 is exact (3 mantissa bits into 7, exponents far inside bf16's), so the raw bytes are
// converted in registers by v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 and v_mfma_f32_16x16x32_bf16 forms
// exact products, summed in fp32.  The row scale never enters the K loop: it multiplies the finished
// sum once, in fp32, before the epilogue's first bf16 rounding.
//
// Matrix unit.  W is the A operand (16 weight rows x 32 k), X the B operand (column j = X row j;
// lanes with j >= M read row M - 1 and never store).  Lane l = 16 g + r holds row r of A and column r
// of B at the lane group's 8 k, and its four accumulators are weight rows 4 g + (0 .. 3) of X row r:
// adjacent weight rows meet in one lane and every store is 8 B.  A wave's unit is 32 weight rows as
// two A tiles whose first rows r0 and r1 put both members of every epilogue pair into one lane:
//   modes 0 / 1, V heads, interleaved RoPE   r0 = 32 u, r1 = 32 u + 16
//   mode 2                                   r0 = 16 u (gate), r1 = I + 16 u (up)
//   mode 3, rotate-half Q / K heads          r0 = head D + 16 t, r1 = r0 + D / 2
//
// W path: HBM -> VGPR, no LDS.  One byte per weight: a K step is 128 weights of a row, one 128-B line.
// In step c lane (r, g) issues two 16-B nontemporal loads per tile, bytes 128 c + 64 h + 16 g .. + 15
// of row r (h = 0, 1): the four lane groups of a row cover 64 contiguous bytes per load and the two
// loads the whole line.  A load holds 16 k, that is two 8-wide A fragments (dwords 0 - 1 and 2 - 3),
// so it feeds two MFMAs, against the two 16-B pieces of X at the same k in the same lane: the MFMA
// does not care which k a lane group holds as long as A and B agree.  Byte b of a dword is element b
// of its fragment half (two conversions per dword: bytes 0 - 1 and bytes 2 - 3).
//
// X path.  NORM (QKV, gate_up): the M rows and gamma are staged whole by LDS-DMA at a row stride of
// 2 K + 16 B (the 16 lanes of a lane group read 16 rows at one k: distinct 16-B bank groups).  Each
// wave then owns whole rows of the image, rows wave, wave + NW, ...: it sums a row's squares and
// rescales it in place with rmsnorm_kernel's rounding, so no partial sums cross waves and one barrier
// ends the prologue.  gamma is dead after that, and the K split's partial tiles reuse its place.  The
// B fragments are 32 contiguous bytes per lane and load (two 16-B LDS reads).  Not NORM (O, down, LM
// head): the same 32 B come from global memory (X is L2-resident), prefetched with the W loads, so K
// is not bounded by LDS.
//
// Loads in flight.  Two register sets ping-pong; a set is 2 / P steps of P units (32 VGPRs of W per
// set whatever P is), and a B fragment is reused across the P units.  A workgroup is NW = 4 or 8
// waves (a plan parameter: under NORM every workgroup pays for the whole X image, and a wider
// workgroup spreads one image over more weight rows), split into NW / KW slots of KW waves; the waves
// of a slot split the K steps of the slot's units and their partial tiles are summed through LDS in
// wave order.  Nothing is split across workgroups: fp32 in one fixed order, no atomics, the same bits
// on every run.  Workgroups are persistent over equal numbers of rounds.  pick_plan holds the
// defaults; lk_gemm_w8_set_plan overrides them for measurements (benchmarks/gemm_w8_bench.py;
// docs/decode_fp8_rows.md has the arms).
#include "common.h"
#include "kernels.h"

namespace {

struct GemmW8Args {
  const bf16_t* x = nullptr;  // [M, K] input rows (NORM: the residual rows to normalise)
  long ldx = 0;
  const bf16_t* gamma = nullptr;  // NORM weights [K]
  float eps = 0.f;
  const unsigned char* w = nullptr;  // [N, K] row-major e4m3
  const float* wscale = nullptr;     // [N]
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

typedef __bf16 g8_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int g8_uint2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* g8_lptr;
typedef const __attribute__((address_space(1))) void* g8_gptr;

LK_DEVICE float g8_rbf(float x) { return bf2f(f2bf(x)); }
LK_DEVICE float g8_silu(float x) { return x / (1.f + __expf(-x)); }
LK_DEVICE float g8_lo(unsigned v) { return __uint_as_float(v << 16); }
LK_DEVICE float g8_hi(unsigned v) { return __uint_as_float(v & 0xffff0000u); }

// eight e4m3 (two dwords, k ascending with the byte address) as the 8-wide bf16 A fragment
LK_DEVICE g8_bf16x8 g8_cvt8(unsigned d0, unsigned d1) {
  const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, false);
  const bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, true);
  const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, false);
  const bf16x2_t e = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, true);
  return (g8_bf16x8){a.x, a.y, b.x, b.y, c.x, c.y, e.x, e.y};
}

// first weight rows of the two A tiles of unit u (header)
template <int MODE>
LK_DEVICE void g8_unit_rows(const GemmW8Args& g, int u, long& r0, long& r1) {
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

LK_DEVICE void g8_store4(bf16_t* p, const float* v) {
  *reinterpret_cast<g8_uint2*>(p) = (g8_uint2){pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
}

// The epilogue of one unit in one lane: X row m, weight rows ra + (0 .. 3) in a[0] and rb + (0 .. 3)
// in a[1], raw sums.  The row scale first, then gemv_decode_w8.hip's arithmetic, pair by pair.
template <int MODE>
LK_DEVICE void g8_epilogue(const GemmW8Args& g, int m, long ra, long rb, long r0, const floatx4 (&a)[2]) {
  float da[4], db[4], va[4], vb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) da[q] = a[0][q] * g.wscale[ra + q], db[q] = a[1][q] * g.wscale[rb + q];
  if constexpr (MODE == 0) {
    g8_store4(g.out + (long)m * g.ldo + ra, da);
    g8_store4(g.out + (long)m * g.ldo + rb, db);
  } else if constexpr (MODE == 1) {
    bf16_t* rr = g.res + (long)m * g.ldr;
    const g8_uint2 oa = *reinterpret_cast<const g8_uint2*>(rr + ra), ob = *reinterpret_cast<const g8_uint2*>(rr + rb);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      va[q] = g8_rbf(g8_rbf(da[q]) + (q & 1 ? g8_hi(oa[q >> 1]) : g8_lo(oa[q >> 1])));
      vb[q] = g8_rbf(g8_rbf(db[q]) + (q & 1 ? g8_hi(ob[q >> 1]) : g8_lo(ob[q >> 1])));
    }
    g8_store4(rr + ra, va);
    g8_store4(rr + rb, vb);
  } else if constexpr (MODE == 2) {
#pragma unroll
    for (int q = 0; q < 4; ++q) va[q] = g8_rbf(g8_silu(g8_rbf(da[q]))) * g8_rbf(db[q]);
    g8_store4(g.out + (long)m * g.ldo + ra, va);  // (gate row = output column)
  } else {
    bf16_t* orow = g.out + (long)m * g.ldo;
    const int head = (int)(r0 / g.D), hd = g.D >> 1;
    const int ca = (int)(ra - (long)head * g.D), cb = (int)(rb - (long)head * g.D);  // columns of the head
    const int slot = g.slots ? g.slots[m] : -1;
    const long blk = slot >= 0 ? slot / g.BS : 0;
    const int off = slot >= 0 ? slot % g.BS : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) va[q] = g8_rbf(da[q]), vb[q] = g8_rbf(db[q]);
    if (head >= g.Hq + g.Hkv) {  // V: copied (into the row and the cache)
      g8_store4(orow + ra, va);
      g8_store4(orow + rb, vb);
      if (g.vc && slot >= 0) {
        bf16_t* vd = g.vc + ((blk * g.Hkv + (head - g.Hq - g.Hkv)) * g.BS + off) * g.D;
        g8_store4(vd + ca, va);
        g8_store4(vd + cb, vb);
      }
      return;
    }
    const float* cs = g.cos_sin + (long)g.positions[m] * g.D;  // [cos(D/2) | sin(D/2)]
    float ya[4], yb[4];                                         // rotated
    if (g.neox) {  // pair q: rows ra + q and rb + q = ra + q + D / 2
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float c = cs[ca + q], s = cs[hd + ca + q];
        ya[q] = va[q] * c - vb[q] * s, yb[q] = vb[q] * c + va[q] * s;
      }
    } else {  // pairs of adjacent rows within each tile
#pragma unroll
      for (int q = 0; q < 4; q += 2) {
        const float c = cs[(ca + q) >> 1], s = cs[hd + ((ca + q) >> 1)];
        ya[q] = va[q] * c - va[q + 1] * s, ya[q + 1] = va[q + 1] * c + va[q] * s;
        const float c2 = cs[(cb + q) >> 1], s2 = cs[hd + ((cb + q) >> 1)];
        yb[q] = vb[q] * c2 - vb[q + 1] * s2, yb[q + 1] = vb[q + 1] * c2 + vb[q] * s2;
      }
    }
    if (head < g.Hq) {
      g8_store4(orow + ra, ya);
      g8_store4(orow + rb, yb);
    } else {  // K: unrotated in the row, rotated in the cache
      g8_store4(orow + ra, va);
      g8_store4(orow + rb, vb);
      if (g.kc && slot >= 0) {
        bf16_t* kd = g.kc + ((blk * g.Hkv + (head - g.Hq)) * g.BS + off) * g.D;
        g8_store4(kd + ca, ya);
        g8_store4(kd + cb, yb);
      }
    }
  }
}

// one register set of the ping-pong: U steps of P units (two tiles, two loads each) and, not NORM,
// the X pieces of the steps ([h][s]: load h, fragment s)
template <bool NORM, int P, int U>
struct G8Set {
  uint4_t w[U][P][2][2];
  g8_bf16x8 x[NORM ? 1 : U][2][2];
};

template <bool NORM, int MODE, int NW, int KW, int P>
__global__ __launch_bounds__(64 * NW) void gemm_w8_kernel(GemmW8Args g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int U = 2 / P;
  const int K = g.K, M = g.M;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 15, grp = lane >> 4;
  const int xrow = r < M ? r : M - 1;
  const int lds_ld = K + 8;                      // LDS row stride of the X image, elements
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);  // NORM: [M][K + 8], then gamma [K]
  // (the partial tiles take gamma's place once the image is normalised)
  floatx4* red = reinterpret_cast<floatx4*>(smem + (NORM ? (size_t)M * lds_ld * 2 : 0));

  if constexpr (NORM) {
    // ---- stage X and gamma by LDS-DMA: instruction gi lands pieces [64 gi, 64 gi + 64) of a row
    bf16_t* gs = xs + M * lds_ld;
    const int nch = K >> 3;  // 16-B pieces of a row (a multiple of 32: the last instruction may be half)
    for (int gi = wv; gi < ((nch + 63) >> 6); gi += NW) {
      const int pc = gi * 64 + lane;
      if (pc < nch) {
        for (int m = 0; m < M; ++m)
          __builtin_amdgcn_global_load_lds((g8_gptr)(g.x + (long)m * g.ldx + pc * 8),
                                           (g8_lptr)(xs + m * lds_ld + gi * 512), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((g8_gptr)(g.gamma + pc * 8), (g8_lptr)(gs + gi * 512), 16, 0, 0);
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) (lgkmcnt / expcnt untouched)
    __syncthreads();
    // RMSNorm with rmsnorm_kernel's rounding, y = bf16(bf16(v * inv) * g), in place; a wave owns
    // whole rows
    for (int m = wv; m < M; m += NW) {
      bf16_t* row = xs + m * lds_ld;
      float ss = 0.f;
      for (int c = lane; c < nch; c += 64) {
        const uint4_t v = *reinterpret_cast<const uint4_t*>(row + c * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) ss += g8_lo(v[j]) * g8_lo(v[j]) + g8_hi(v[j]) * g8_hi(v[j]);
      }
      const float inv = rsqrtf(wave_sum(ss) / (float)K + g.eps);
      for (int c = lane; c < nch; c += 64) {
        const uint4_t v = *reinterpret_cast<const uint4_t*>(row + c * 8);
        const uint4_t gv = *reinterpret_cast<const uint4_t*>(gs + c * 8);
        uint4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = pack_bf2(g8_rbf(g8_lo(v[j]) * inv) * g8_lo(gv[j]), g8_rbf(g8_hi(v[j]) * inv) * g8_hi(gv[j]));
        *reinterpret_cast<uint4_t*>(row + c * 8) = o;
      }
    }
    __syncthreads();
  }

  // ---- stream W.  Slot ps of the workgroup owns P units per round, wave kh of the slot the K
  // steps [sb, se).  The round loop is uniform over the workgroup (its barriers); a unit past the
  // last one streams the last unit again (L2 hits) and drops the sums.
  constexpr int SLOTS = NW / KW, UPW = SLOTS * P;
  const int ps = wv / KW, kh = wv % KW;
  const int ns = K >> 7;
  const int per = ((ns + KW - 1) / KW + U - 1) / U * U;  // (whole register sets per wave)
  const int sb = kh * per, se = sb + per < ns ? sb + per : ns;
  const bf16_t* xg = (NORM ? xs + xrow * lds_ld : g.x + (long)xrow * g.ldx) + 8 * grp * 2;  // this lane's X row and k
  for (int ub = blockIdx.x * UPW; ub < g.nunits; ub += gridDim.x * UPW) {
    const int u0 = ub + ps * P;
    long r0[P], r1[P];
    const unsigned char* wp[P][2];
    floatx4 acc[P][2];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      g8_unit_rows<MODE>(g, u0 + i < g.nunits ? u0 + i : g.nunits - 1, r0[i], r1[i]);
      wp[i][0] = g.w + (r0[i] + r) * (long)K + grp * 16;
      wp[i][1] = g.w + (r1[i] + r) * (long)K + grp * 16;
      acc[i][0] = acc[i][1] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    auto load = [&](G8Set<NORM, P, U>& b, int c0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u;
        if (c >= se) break;  // (wave-uniform)
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h)
              b.w[u][i][t][h] =
                  __builtin_nontemporal_load(reinterpret_cast<const uint4_t*>(wp[i][t] + c * 128 + h * 64));
        if constexpr (!NORM) {
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < 2; ++s)
              b.x[u][h][s] = *reinterpret_cast<const g8_bf16x8*>(xg + c * 128 + h * 64 + 8 * s);
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch issued ahead of the MFMAs below
    };
    auto compute = [&](G8Set<NORM, P, U>& b, int c0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u;
        if (c >= se) break;
        if constexpr (NORM) {
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < 2; ++s)
              b.x[0][h][s] = *reinterpret_cast<const g8_bf16x8*>(xg + c * 128 + h * 64 + 8 * s);
        }
        const int xu = NORM ? 0 : u;
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
              for (int s = 0; s < 2; ++s)
                acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    g8_cvt8(b.w[u][i][t][h][2 * s], b.w[u][i][t][h][2 * s + 1]), b.x[xu][h][s], acc[i][t], 0, 0, 0);
      }
    };
    // ping-pong register sets, no copies: the next set is in flight under this set's MFMAs
    G8Set<NORM, P, U> sa, sc;
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
        if (u0 + i < g.nunits) g8_epilogue<MODE>(g, r, r0[i] + 4 * grp, r1[i] + 4 * grp, r0[i], acc[i]);
    }
  }
}

constexpr int kG8MaxImage = 163840 - 1024;  // the NORM image: M (2 K + 16) + 2 K bytes
constexpr int kG8MaxLds = 163840 - 512;     // dynamic LDS opt-in
int g_plan_nw = 0, g_plan_kw = 0, g_plan_p = 0;  // measurement overrides (0: the plan's own)

struct G8Plan {
  int NW, KW, P;
};

size_t g8_image_bytes(int M, int K) { return (size_t)M * (2 * K + 16) + 2 * (size_t)K; }
size_t g8_red_bytes(const G8Plan& p) { return p.KW > 1 ? (size_t)(p.NW / p.KW) * (p.KW - 1) * p.P * 2 * 1024 : 0; }
// (the partial tiles lie over gamma)
size_t g8_lds_bytes(const G8Plan& p, int M, int K, bool norm) {
  if (!norm) return g8_red_bytes(p);
  const size_t red = g8_red_bytes(p), gam = 2 * (size_t)K;
  return (size_t)M * (2 * K + 16) + (red > gam ? red : gam);
}

// (NW, KW, P) by units, K steps and the X source: docs/decode_fp8_rows.md has the measured arms.
// Eight waves under the prologue (one X image serves eight waves: QKV 12.2 against 16.4 us), four
// without it.  Two units per wave (built without a K split only) where that still leaves a round for
// each of 256 workgroups (the LM head); otherwise the widest K split that keeps the rounds at one
// per CU or fewer (QKV: all 8 waves on one unit, gate_up 2, O and down 4).
G8Plan pick_plan(int M, int nunits, int K, bool norm) {
  const int ns = K / 128;
  G8Plan p;
  p.NW = g_plan_nw ? g_plan_nw : (norm ? 8 : 4);
  p.P = g_plan_p ? g_plan_p : (nunits >= 2 * p.NW * 256 ? 2 : 1);
  if (g_plan_kw) {
    p.KW = g_plan_kw;
  } else {
    p.KW = 1;
    while (p.KW < p.NW && nunits * 2 * p.KW <= p.NW * p.P * 256) p.KW *= 2;
  }
  if (p.KW > p.NW) p.KW = p.NW;
  while (p.KW > 1 && 2 * p.KW > ns) p.KW /= 2;
  if (p.KW > 1) p.P = 1;
  // (the partial tiles share LDS with the NORM image: a narrower K split where they do not fit)
  while (norm && p.KW > 1 && g8_lds_bytes(p, M, K, true) > (size_t)kG8MaxLds) p.KW /= 2;
  return p;
}

template <bool NORM, int MODE>
int launch_plan(const GemmW8Args& a, hipStream_t st) {
  const G8Plan pl = pick_plan(a.M, a.nunits, a.K, NORM);
  const size_t lds = g8_lds_bytes(pl, a.M, a.K, NORM);
  if (lds > (size_t)kG8MaxLds) return -3;
  const int upw = pl.NW / pl.KW * pl.P;
  const int rounds = (a.nunits + upw - 1) / upw;
  // workgroups resident at once: eight waves per CU, fewer where the LDS image allows only one
  // workgroup; every workgroup takes the same number of rounds
  int per_cu = 8 / pl.NW;
  if (NORM && (int)(163840 / (lds + 512)) < per_cu) per_cu = 1;
  const int cap = 256 * per_cu;
  const int rpw = (rounds + cap - 1) / cap;
  const int wgs = (rounds + rpw - 1) / rpw;
#define LK_G8_PLAN(WW, KK, PP)                                                \
  if (pl.NW == WW && pl.KW == KK && pl.P == PP) {                             \
    LK_SET_MAX_LDS((gemm_w8_kernel<NORM, MODE, WW, KK, PP>), kG8MaxLds);      \
    gemm_w8_kernel<NORM, MODE, WW, KK, PP><<<wgs, 64 * WW, lds, st>>>(a);     \
    LK_CHECK_LAUNCH();                                                        \
    return 0;                                                                 \
  }
  LK_G8_PLAN(4, 1, 1) LK_G8_PLAN(4, 1, 2) LK_G8_PLAN(4, 2, 1) LK_G8_PLAN(4, 4, 1)
  LK_G8_PLAN(8, 1, 1) LK_G8_PLAN(8, 1, 2) LK_G8_PLAN(8, 2, 1) LK_G8_PLAN(8, 4, 1) LK_G8_PLAN(8, 8, 1)
#undef LK_G8_PLAN
  return -4;
}

// what the kernel can run
bool shape_ok(int M, int N, int K, int mode, int norm) {
  if (M < 3 || M > 16 || K < 256 || K % 256 || N < 32 || N % 32) return false;
  if (mode < 0 || mode > 3) return false;
  return !norm || g8_image_bytes(M, K) <= (size_t)kG8MaxImage;
}

// The (shape class, row bucket) pairs measured slower than, or within the spread of, the bf16 route
// (benchmarks/gemm_w8_bench.py; the table is in docs/decode_fp8_rows.md): they stay on bf16.
// Buckets are the decode graphs' 4 / 8 / 16.  A shape that was not measured is not routed back.
struct G8RoutedBack {
  int N, K, mlo, mhi;
};
constexpr G8RoutedBack kRoutedBack[] = {
    {6144, 4096, 3, 4},     // Llama-3-8B QKV at bucket 4: 12.3 against 15.0 us, but one slow bf16 round (21.0) widened the spread past the gain
    {6144, 4096, 9, 16},    // QKV at bucket 16: 16.5 against 15.1 us (the 16-row X image per workgroup)
    {4096, 14336, 3, 16},   // down: 26.3 / 28.0 / 32.3 against 26.6 / 25.9 / 26.2 us (128 units fill half the CUs)
};

bool routed(int M, int N, int K) {
  for (const G8RoutedBack& r : kRoutedBack)
    if (r.N == N && r.K == K && M >= r.mlo && M <= r.mhi) return false;
  return true;
}

}  // namespace

int lk_gemm_w8_supported(int M, int N, int K, int mode, int norm) {
  return shape_ok(M, N, K, mode, norm) && routed(M, N, K);
}

void lk_gemm_w8_set_plan(int waves, int kw, int units) {
  g_plan_nw = waves == 4 || waves == 8 ? waves : 0;
  g_plan_kw = kw == 1 || kw == 2 || kw == 4 || kw == 8 ? kw : 0;
  g_plan_p = units == 1 || units == 2 ? units : 0;
}

// Return codes (all before any launch): -1 shape (M, K % 256, N % 32, the NORM image), -5 a null
// pointer, -6 a misaligned pointer or row stride, -7 the mode's own arguments.
int lk_gemm_w8_decode(int mode, const bf16_t* x, long ldx, const bf16_t* gamma, float eps, const unsigned char* wq,
                      const float* wscale, int M, int N, int K, bf16_t* out, long ldo, bf16_t* res, long ldr,
                      const int* positions, const float* cos_sin, int Hq, int Hkv, int D, bf16_t* kc, bf16_t* vc,
                      const int* slots, int BS, int neox, hipStream_t st) {
  if (!shape_ok(M, N, K, mode, gamma != nullptr)) return -1;
  if (!x || !wq || !wscale) return -5;
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(wq) % 16 ||
      reinterpret_cast<uintptr_t>(wscale) % 4 || (gamma && reinterpret_cast<uintptr_t>(gamma) % 16) || ldx % 8 || ldx < K)
    return -6;
  // (every store is 8 B: four consecutive bf16 of a row)
  if ((out && (reinterpret_cast<uintptr_t>(out) % 8 || ldo % 4)) || (res && (reinterpret_cast<uintptr_t>(res) % 8 || ldr % 4)))
    return -6;
  GemmW8Args a;
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
#define LK_G8_MODE(MD) \
  if (mode == MD) return norm ? launch_plan<true, MD>(a, st) : launch_plan<false, MD>(a, st);
  LK_G8_MODE(0) LK_G8_MODE(1) LK_G8_MODE(2) LK_G8_MODE(3)
#undef LK_G8_MODE
  return -1;
}
