// BM25 posting scan with fused top-k over an inverted index (CSR by term) resident in HBM.
//   score(d) = sum over the query's terms t, ascending, with d in postings(t):  w_t * tf / (tf + kn[d])
// kn[d] = k1 (1 - b + b dl_d / avgdl) and w_t = qtf * idf_t are made on the host (rag/lexical.py).
// Only documents with score > 0 are hits; results are ordered (score desc, id asc), the tie rule
// of knn.hip, and padded with (-inf, -1).
//
// Pass 1 (lk_bm25_partial): one 256-thread workgroup per (chunk of kLkBm25Chunk document ids,
// query).  One lane per query term finds [lo, hi) = the term's postings whose document falls in
// the chunk (two lower-bound searches in post_doc; the second is confined to the kLkBm25Chunk
// postings after lo, since a list is strictly ascending).  A chunk in which no term has a posting
// writes its pads and leaves before it stages anything.  Otherwise kn of the chunk and a zeroed
// score[chunk] go to LDS (32 KB static) and the terms are walked in ascending order: lanes stride
// a term's postings with coalesced loads and each posting adds into its own LDS slot, a workgroup
// barrier between terms.  Inside a term every slot is touched at most once (the lists are
// duplicate-free) and two terms never run concurrently: no atomics, one fixed summation order per
// document, the same bits on every run.  The quotient, the product and the add are each rounded
// once (the product is kept out of an FMA), so the kernel computes what the fp32 reference
// computes.  The chunk's top-k comes out of the block-wide rounds of topk.h (topk_rounds) over
// the slots with score > 0; every other slot enters them as -inf.
// Pass 2: lk_knn_merge (knn.hip) over nchunks * K candidates per query; it skips id < 0.
//
// Nothing the device reads is trusted to index memory: term ids outside [0, V) are empty terms,
// posting ranges are clamped to [0, nnz], a query's terms to kLkBm25MaxTerms, and a posting whose
// document falls outside the chunk is ignored.
#include "kernels.h"
#include "topk.h"

namespace {

constexpr int C = kLkBm25Chunk;
constexpr int MAXT = kLkBm25MaxTerms;
constexpr int PER = C / 256;

// first p in [lo, hi) with post_doc[p] >= key (hi if none)
LK_DEVICE long lower_bound(const int* __restrict__ post_doc, long lo, long hi, long key) {
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if ((long)post_doc[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void bm25_partial_kernel(
    const long* __restrict__ term_ptr, long V, const int* __restrict__ post_doc,
    const unsigned char* __restrict__ post_tf, long nnz, const float* __restrict__ kn, long N,
    const int* __restrict__ q_ptr, const int* __restrict__ q_term, const float* __restrict__ q_w, int K,
    float* __restrict__ part_s, int* __restrict__ part_i, int nchunks) {
  __shared__ float score[C];
  __shared__ float kns[C];
  __shared__ long lo_s[MAXT], hi_s[MAXT];
  __shared__ float w_s[MAXT];
  __shared__ float rs[4];
  __shared__ int ri[4];
  const int q = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const long base = (long)c * C;
  const int q0 = q_ptr[q];
  int nt = q_ptr[q + 1] - q0;
  nt = nt < 0 ? 0 : nt > MAXT ? MAXT : nt;
  float* ps = part_s + ((long)q * nchunks + c) * K;
  int* pi = part_i + ((long)q * nchunks + c) * K;

  int mine = 0;
  if (tid < nt) {
    const long t = q_term[q0 + tid];
    long lo = 0, hi = 0;
    if (t >= 0 && t < V) {
      long beg = term_ptr[t], end = term_ptr[t + 1];
      beg = beg < 0 ? 0 : beg > nnz ? nnz : beg;
      end = end < beg ? beg : end > nnz ? nnz : end;
      lo = lower_bound(post_doc, beg, end, base);
      hi = lower_bound(post_doc, lo, end - lo > C ? lo + C : end, base + C);
    }
    lo_s[tid] = lo;
    hi_s[tid] = hi;
    w_s[tid] = q_w[q0 + tid];
    mine = hi > lo;
  }
  if (!__syncthreads_or(mine)) {  // nothing of this query in the chunk (also publishes lo_s / hi_s / w_s)
    for (int kk = tid; kk < K; kk += 256) {
      ps[kk] = -INFINITY;
      pi[kk] = -1;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const long d = base + j * 256 + tid;
    score[j * 256 + tid] = 0.f;
    kns[j * 256 + tid] = d < N ? kn[d] : 1.f;
  }
  __syncthreads();

  for (int ti = 0; ti < nt; ++ti) {
    const long lo = lo_s[ti], hi = hi_s[ti];
    if (hi <= lo) continue;  // the same for every lane: no barrier is skipped by some
    const float wt = w_s[ti];
    for (long p = lo + tid; p < hi; p += 256) {
      const long d = (long)post_doc[p] - base;
      const float tf = (float)post_tf[p];
      if (d >= 0 && d < C) {
        const float quot = tf / (tf + kns[d]);  // correctly rounded (the build's default division)
        float prod = wt * quot;
        // the build contracts a * b + c into one FMA (-ffp-contract=fast, whatever a pragma says):
        // pinning the product to a register keeps its own rounding, as in the reference
        asm volatile("" : "+v"(prod));
        score[d] += prod;
      }
    }
    __syncthreads();
  }

  float v[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const float s = score[j * 256 + tid];
    v[j] = (s > 0.f && base + j * 256 + tid < N) ? s : -INFINITY;
  }
  topk_rounds(v, base, K, ps, pi, rs, ri);
}

}  // namespace

int lk_bm25_chunks(long N) { return (int)((N + C - 1) / C); }

int lk_bm25_supported(long N, int nq, int max_terms, int K) {
  if (K < 1 || K > 64) return -1;
  if (max_terms > MAXT) return -2;
  if (N >= (1L << 31)) return -3;
  if (nq > 65535) return -4;  // grid.y
  return 0;
}

int lk_bm25_partial(const long* term_ptr, long V, const int* post_doc, const unsigned char* post_tf, long nnz,
                    const float* kn, long N, const int* q_ptr, const int* q_term, const float* q_w, int nq,
                    int max_terms, int K, float* part_s, int* part_i, hipStream_t st) {
  const int rc = lk_bm25_supported(N, nq, max_terms, K);
  if (rc) return rc;
  if (N <= 0 || nq <= 0) return 0;
  const int nc = lk_bm25_chunks(N);
  bm25_partial_kernel<<<dim3(nc, nq), 256, 0, st>>>(term_ptr, V, post_doc, post_tf, nnz, kn, N, q_ptr, q_term, q_w, K,
                                                    part_s, part_i, nc);
  LK_CHECK_LAUNCH();
  return 0;
}
