// The retrieval kernels' one tie rule and the top-k rounds built on it (knn.hip, bm25.hip, mmr.hip).
//
// Order: (score desc, id asc), ids compared as unsigned; NaN is never better than anything, so a NaN
// score is absent.  Pads are (-inf, -1).  Sharded search equals single-GPU search bit for bit only
// because every kernel that selects or merges hits uses this one definition.
#pragma once
#include "common.h"

constexpr int kNoCand = 0x7fffffff;  // the id of "no candidate": loses every tie against a real id

LK_DEVICE bool better(float s1, int i1, float s2, int i2) {
  return s1 > s2 || (s1 == s2 && (unsigned)i1 < (unsigned)i2);
}

// 64-lane argmax: every lane leaves holding the winner
LK_DEVICE void wave_argmax(float& s, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float s2 = __shfl_xor(s, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    if (better(s2, i2, s, i)) {
      s = s2;
      i = i2;
    }
  }
}

// Argmax of a 256-thread workgroup through the LDS slots rs[4] / ri[4]: one barrier, every thread
// folds the four waves' winners and leaves holding the block's.  The caller owns the barrier before
// the slots are written again.
LK_DEVICE void block_argmax(float& s, int& i, float* rs, int* ri) {
  wave_argmax(s, i);
  if ((threadIdx.x & 63) == 0) {
    rs[threadIdx.x >> 6] = s;
    ri[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  s = rs[0];
  i = ri[0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (better(rs[j], ri[j], s, i)) {
      s = rs[j];
      i = ri[j];
    }
}

// The top-K of the 256 * PER scores a 256-thread workgroup holds in registers, written to ps / pi[0, K)
// in order; the workgroup owns ids base + j * 256 + tid, every thread must call, rs[4] / ri[4] are LDS.
// A slot that must not be a hit (row past N, non-positive BM25 score) holds -inf on entry.  Each
// round: the thread's best slot, the block's argmax, thread 0 writes the winner, the winner's slot
// becomes -inf.  Ids are int32 in every output, so they are formed in 32 bits: no 64-bit id
// arithmetic stays live across the rounds.
//
// The rounds stop at the first whose winner is -inf and the workgroup writes the remaining (-inf, -1)
// pads together.  That is bit for bit what running all K rounds writes: a round won with -inf writes
// (-inf, -1) whatever the id is -- a real -inf score, a row out of range and a NaN that never wins
// all read so -- and once the best left is -inf every later round's is too.
//
// knn_partial_kernel's wave-wide rounds (knn.hip) are these without LDS and without the early stop;
// they stay written out there because this routine measured slower in that kernel.
template <int PER>
LK_DEVICE void topk_rounds(float (&v)[PER], long base, int K, float* __restrict__ ps, int* __restrict__ pi,
                           float* rs, int* ri) {
  constexpr int T = 256;
  const int t = threadIdx.x;
  const int id0 = (int)base + t;
  int kk = 0;
  for (; kk < K; ++kk) {
    float bs = -INFINITY;
    int bi = kNoCand;
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (better(v[j], id0 + j * T, bs, bi)) {
        bs = v[j];
        bi = id0 + j * T;
      }
    block_argmax(bs, bi, rs, ri);
    if (bs == -INFINITY) break;  // the same for every thread: no barrier is skipped by some
    if (t == 0) {
      ps[kk] = bs;
      pi[kk] = bi;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (id0 + j * T == bi) v[j] = -INFINITY;
    __syncthreads();  // rs / ri are rewritten by the next round
  }
  for (int r = kk + t; r < K; r += T) {
    ps[r] = -INFINITY;
    pi[r] = -1;
  }
}
