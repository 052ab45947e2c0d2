// Maximal-marginal-relevance selection over a query's candidate list (docs/mmr.md): K greedy rounds
//   mmr_i = lam * rel_i - (1 - lam) * m_i,   m_i = max over the already selected s of sim(i, s)
// with sim(i, j) = dot(c_i, c_j) / (cnorm[id_i] * cnorm[id_j] + 1e-9), the form of knn.hip, and the
// pick of a round the present, not yet selected candidate with the largest mmr, ties to the lower
// position: better() of topk.h on (mmr, position).  m_i is 0 in round 0 and is ASSIGNED from the
// first pick (a negative similarity stays negative).  The kernel does not know the query: rel is an
// input.  Candidate i is present iff 0 <= cand_id[i] < N and rel[i] is not NaN; an absent
// candidate's row address is clamped to row 0 and what was computed from it is never used.  When the
// present candidates run out the rest of the row is (-1, -1, -inf, -inf, -inf).  A candidate whose
// mmr is NaN in a round (an infinite rel under lam = 0, say) is not picked in that round.
//
// One 256-thread workgroup per query.  The C x C Gram matrix (C <= 64) is up to four 32x32 tiles of
// v_mfma_f32_32x32x16_bf16: wave 0 and wave 3 the diagonal tiles, wave 1 the tile (rows 0-31, columns
// 32-63), which it also writes mirrored (the matrix is symmetric), wave 2 has no tile.  Both operands
// are corpus rows, so a lane's A and B fragments are 16-byte loads straight from HBM; the MFMA k-order
// is permuted as in knn.hip so that a lane streams 64 contiguous bytes of its row per group of 4
// k-steps (both operands permuted alike), the loads of the next group in flight under the MFMAs of
// this one; the D % 64 tail runs in natural order.  The accumulators are normalised into the LDS
// image S[64][65] (f32, 16.6 KB static) and, after one barrier, wave 0 runs the K rounds with lane =
// candidate: one wave_argmax on (mmr, position), one LDS read of S[lane][pick] to update m.
// No atomics, every sum has one order: the same bits on every run.
//
// Roundings (the build contracts a * b + c, -ffp-contract=fast): the dot is the MFMA's fp32
// accumulation of exact bf16 products; the denominator cn_i * cn_j + 1e-9 is ONE fused
// multiply-add; the quotient is correctly rounded.  mmr_i gets three roundings: lam * rel_i and
// (1 - lam) * m_i are each rounded on their own (pinned to a register, so neither is fused into the
// subtraction), then their difference is rounded; 1 - lam is formed once in fp32 on the host from
// lam as fp32.  ops/reference.py::mmr_select writes the same three operations in fp32.
//
// Nothing the device reads is trusted to index memory: ids outside [0, N) never form an address,
// positions and K are bounded by the host's checks (1 <= K <= C <= 64).
#include "kernels.h"
#include "topk.h"

namespace {

constexpr int MAXC = kLkMmrMaxCand;

__global__ __launch_bounds__(256) void mmr_select_kernel(
    const bf16_t* __restrict__ corpus, const float* __restrict__ cnorm, long N, int D,
    const int* __restrict__ cand_id, const float* __restrict__ rel, int C, float lam, float oml, int K,
    int* __restrict__ out_pos, int* __restrict__ out_id, float* __restrict__ out_rel, float* __restrict__ out_mmr,
    float* __restrict__ out_sim) {
  __shared__ float S[MAXC][MAXC + 1];
  __shared__ float cn_s[MAXC];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int* ids = cand_id + (long)q * C;

  // wave 0: lane = candidate; its norm goes to LDS for the normalisation of every tile
  int my_id = -1;
  float my_rel = 0.f;
  bool avail = false;
  if (w == 0) {
    float cn = 1.f;
    if (lane < C) {
      my_id = ids[lane];
      my_rel = rel[(long)q * C + lane];
      const bool in = my_id >= 0 && (long)my_id < N;
      avail = in && my_rel == my_rel;
      if (in) cn = cnorm[my_id];
    }
    cn_s[lane] = cn;
  }

  const int ti = w >> 1, tj = w & 1;
  const bool active = w != 2 && 32 * ti < C && 32 * tj < C && N > 0;  // the same for a whole wave
  const bool diag = ti == tj;
  floatx16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  if (active) {
    const int ia = 32 * ti + r, ib = 32 * tj + r;
    long ida = ia < C ? (long)ids[ia] : 0, idb = ib < C ? (long)ids[ib] : 0;
    ida = ida >= 0 && ida < N ? ida : 0;
    idb = idb >= 0 && idb < N ? idb : 0;
    const bf16_t* pa = corpus + ida * D;
    const bf16_t* pb = corpus + idb * D;
    const int NG = D / 64;  // groups of 4 k-steps: k-step (4g+u), element j  <->  d = 64g + 32h + 8u + j
    short8 a0[4], b0[4], a1[4], b1[4];
    auto load = [&](int g, short8* a, short8* b) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = *reinterpret_cast<const short8*>(pa + 64 * g + 32 * h + 8 * u);
        b[u] = diag ? a[u] : *reinterpret_cast<const short8*>(pb + 64 * g + 32 * h + 8 * u);
      }
    };
    auto mma = [&](const short8* a, const short8* b) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u], b[u], acc, 0, 0, 0);
    };
    if (NG > 0) load(0, a0, b0);
    int g = 0;
    for (; g + 2 <= NG; g += 2) {
      load(g + 1, a1, b1);
      mma(a0, b0);
      if (g + 2 < NG) load(g + 2, a0, b0);
      mma(a1, b1);
    }
    if (g < NG) mma(a0, b0);
    // tail, natural order: k-step t, element j  <->  d = 64 NG + 16t + 8h + j
    for (int d0 = 64 * NG; d0 < D; d0 += 16) {
      const short8 a = *reinterpret_cast<const short8*>(pa + d0 + 8 * h);
      const short8 b = diag ? a : *reinterpret_cast<const short8*>(pb + d0 + 8 * h);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
  }
  __syncthreads();  // cn_s
  if (active) {
    // acc[i] = G[row (i&3) + 8(i>>2) + 4h of the row tile][column r of the column tile]
    const int col = 32 * tj + r;
    const float cc = cn_s[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 32 * ti + (i & 3) + 8 * (i >> 2) + 4 * h;
      const float s = acc[i] / (cn_s[row] * cc + 1e-9f);
      S[row][col] = s;
      if (!diag) S[col][row] = s;
    }
  }
  __syncthreads();
  if (w != 0) return;

  int* o_pos = out_pos + (long)q * K;
  int* o_id = out_id + (long)q * K;
  float* o_rel = out_rel + (long)q * K;
  float* o_mmr = out_mmr + (long)q * K;
  float* o_sim = out_sim + (long)q * K;
  float lr = lam * my_rel;
  asm volatile("" : "+v"(lr));  // its own rounding, never fused into the subtraction
  float m = 0.f;
  for (int rr = 0; rr < K; ++rr) {
    float pen = oml * m;
    asm volatile("" : "+v"(pen));
    const float v = lr - pen;
    const bool ok = avail && v == v;
    float bs = ok ? v : -INFINITY;
    int bi = ok ? lane : kNoCand;
    wave_argmax(bs, bi);
    if (bi == kNoCand) {  // nobody left (every lane sees the same bi): the rest are pads
      for (int k = rr + lane; k < K; k += 64) {
        o_pos[k] = -1;
        o_id[k] = -1;
        o_rel[k] = -INFINITY;
        o_mmr[k] = -INFINITY;
        o_sim[k] = -INFINITY;
      }
      break;
    }
    if (lane == bi) {
      o_pos[rr] = lane;
      o_id[rr] = my_id;
      o_rel[rr] = my_rel;
      o_mmr[rr] = v;
      o_sim[rr] = m;
      avail = false;
    }
    const float s = S[lane][bi];  // bi < C <= 64
    m = rr == 0 ? s : (s > m ? s : m);
  }
}

}  // namespace

int lk_mmr_supported(long N, int D, int C, int K, float lam) {
  if (C < 1 || C > MAXC) return -1;
  if (K < 1 || K > C) return -2;
  if (D < 16 || D > 1024 || D % 16) return -3;
  if (!(lam >= 0.f && lam <= 1.f)) return -4;
  if (N < 0 || N >= (1L << 31)) return -5;
  return 0;
}

int lk_mmr_select(const bf16_t* corpus, const float* cnorm, long N, int D, const int* cand_id, const float* rel,
                  int nq, int C, float lam, int K, int* pos, int* ids, float* rel_out, float* mmr, float* max_sim,
                  hipStream_t st) {
  const int rc = lk_mmr_supported(N, D, C, K, lam);
  if (rc) return rc;
  if (nq <= 0) return 0;
  mmr_select_kernel<<<nq, 256, 0, st>>>(corpus, cnorm, N, D, cand_id, rel, C, lam, 1.f - lam, K, pos, ids, rel_out,
                                        mmr, max_sim);
  LK_CHECK_LAUNCH();
  return 0;
}
