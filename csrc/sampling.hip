// K13 token selection over the vocabulary: greedy argmax, temperature sampling via
// the Gumbel-max trick (one pass, no sort: argmax(l/T + G), G = -log(-log U)) and
// Ollama/llama.cpp-style repetition penalty.  One workgroup per row, 16-byte logits
// loads, (value, lowest index) wave reductions — argmax ties resolve to the first
// index, like torch.argmax.
#include "common.h"
#include "kernels.h"

namespace {

LK_DEVICE bool gt(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// u = (h + 0.5) * 2^-24 in (0, 1) for the top 24 bits h of a hash.  One FMA rounds the same real number
// as the sum-then-scale it replaces, so every draw keeps its bits -- but for h = 0xFFFFFF the result
// ties to even, 1.0f: the Gumbel noise -log(-log 1) is +inf and the id wins its row whatever its logit
// (and u * kept mass reaches a trailing candidate of mass 0).  The cap moves that one draw to the
// largest float below 1 and changes no other.
LK_DEVICE float u01(unsigned hsh) { return fminf(fmaf((float)(hsh >> 8), 0x1p-24f, 0x1p-25f), 0x1.fffffep-1f); }

LK_DEVICE unsigned hash3(unsigned a, unsigned b, unsigned c) {
  // splitmix-style avalanche over three words
  unsigned long long x = ((unsigned long long)a << 32) ^ ((unsigned long long)b * 0x9E3779B97F4A7C15ull) ^ c;
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (unsigned)(x >> 32);
}

// ALLOWED: grammar-constrained rows consider only their allowed ids (plan = [B flags |
// B+1 row offsets | ids]; flags[row] = 0 -> the whole vocabulary).  Same values, same
// Gumbel noise per (row, step, id) and the same tie order as scanning the row with every
// other id masked to -inf -- without materialising the [B, V] mask (3 full passes over
// the logits) or scanning 128k entries per row.
// KEY: greedy only; instead of the id, write the row's order-preserving int64 (value, id) key
// (ops.argmax_key: vocab-parallel greedy = ONE all-gather of these + a max) to key_out
template <bool BF16, bool SAMPLE, bool ALLOWED = false, bool KEY = false>
__global__ __launch_bounds__(256) void select_kernel(const void* __restrict__ logits, long ls, int V,
                                                     const float* __restrict__ temps,
                                                     unsigned long long seed, int step,
                                                     int* __restrict__ out, const int* __restrict__ plan = nullptr,
                                                     long long* __restrict__ key_out = nullptr, int key_lo = 0) {
  __shared__ float rs[4];
  __shared__ int ri[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float temp = SAMPLE ? temps[row] : 1.f;
  const bool greedy = !SAMPLE || temp <= 0.f;
  const float invt = greedy ? 1.f : 1.f / temp;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  const int nv = V / 8;
  const int B = gridDim.x;
  const bool sparse = ALLOWED && plan[row] != 0;
  auto consider = [&](float x, int idx) {
    if (!greedy) {
      const unsigned hsh = hash3((unsigned)(seed ^ (seed >> 32)) + row, (unsigned)step, (unsigned)idx);
      const float u = u01(hsh);
      x = x * invt - __logf(-__logf(u));
    }
    if (gt(x, idx, best, bi)) {
      best = x;
      bi = idx;
    }
  };
  if (sparse) {
    const int* ids = plan + 2 * B + 1;
    const int a0 = plan[B + row], a1 = plan[B + row + 1];
    for (int j = a0 + tid; j < a1; j += 256) {
      const int id = ids[j];
      if constexpr (BF16) consider(bf2f(reinterpret_cast<const bf16_t*>(logits)[(long)row * ls + id]), id);
      else consider(reinterpret_cast<const float*>(logits)[(long)row * ls + id], id);
    }
  } else if constexpr (BF16) {
    // (not lp_scan_row, the same walk: behind it the updates compile to exec-masked moves instead of
    // selects, measured 3.6 % (Gumbel) and 6 % (greedy) slower: docs/sampling.md)
    const bf16_t* lp = reinterpret_cast<const bf16_t*>(logits) + (long)row * ls;
    for (int c = tid; c < nv; c += 256) {
      float v[8];
      load8(lp + c * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) consider(v[j], c * 8 + j);
    }
    for (int i = nv * 8 + tid; i < V; i += 256) consider(bf2f(lp[i]), i);
  } else {
    const float* lp = reinterpret_cast<const float*>(logits) + (long)row * ls;
    for (int c = tid; c < nv; c += 256) {
      const float4 a = *reinterpret_cast<const float4*>(lp + c * 8);
      const float4 b = *reinterpret_cast<const float4*>(lp + c * 8 + 4);
      consider(a.x, c * 8 + 0); consider(a.y, c * 8 + 1); consider(a.z, c * 8 + 2); consider(a.w, c * 8 + 3);
      consider(b.x, c * 8 + 4); consider(b.y, c * 8 + 5); consider(b.z, c * 8 + 6); consider(b.w, c * 8 + 7);
    }
    for (int i = nv * 8 + tid; i < V; i += 256) consider(lp[i], i);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float b2 = __shfl_xor(best, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    if (gt(b2, i2, best, bi)) {
      best = b2;
      bi = i2;
    }
  }
  if (lane == 0) {
    rs[w] = best;
    ri[w] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int j = 1; j < 4; ++j)
      if (gt(rs[j], ri[j], best, bi)) {
        best = rs[j];
        bi = ri[j];
      }
    if (bi == 0x7fffffff) bi = 0;  // all -inf / NaN row: fall back to token 0
    if constexpr (KEY) {
      // high word: the max's float bits made order-preserving and signed; low word: ~global id
      // (the larger key is the larger value, then the lower id -- torch.argmax's tie order)
      // -0.0 is keyed as +0.0: gt() and torch.argmax hold them equal, so must the shards' keys
      unsigned fb = __float_as_uint(best == best ? best : -INFINITY);
      if (fb == 0x80000000u) fb = 0u;
      const unsigned u = (fb & 0x80000000u) ? ~fb : (fb | 0x80000000u);
      key_out[row] = (long long)(((unsigned long long)(u ^ 0x80000000u) << 32) | (unsigned)(~(unsigned)(bi + key_lo)));
    } else {
      out[row] = bi;
    }
  }
}

// ids[r] = the id of max_w keys[w, r] (the gathered per-rank argmax keys)
__global__ void keys_to_ids_kernel(const long long* __restrict__ keys, int W, int R, int* __restrict__ ids) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  long long k = keys[r];
  for (int w = 1; w < W; ++w) k = max(k, keys[(long)w * R + r]);
  ids[r] = (int)(~(unsigned)(k & 0xFFFFFFFFll));
}

// logits[row, tok] = l > 0 ? l / p : l * p for each UNIQUE token of the row's window
template <bool BF16>
__global__ void repeat_penalty_kernel(void* __restrict__ logits, long ls,
                                      const int* __restrict__ window, int W,
                                      const float* __restrict__ penalty) {
  const int row = blockIdx.x;
  const float p = penalty[row];
  const int* win = window + (long)row * W;
  for (int j = threadIdx.x; j < W; j += blockDim.x) {
    const int tok = win[j];
    if (tok < 0) continue;
    bool dup = false;
    for (int i = 0; i < j; ++i) dup |= (win[i] == tok);
    if (dup) continue;
    if constexpr (BF16) {
      bf16_t* lp = reinterpret_cast<bf16_t*>(logits) + (long)row * ls + tok;
      const float l = bf2f(*lp);
      *lp = f2bf(l > 0.f ? l / p : l * p);
    } else {
      float* lp = reinterpret_cast<float*>(logits) + (long)row * ls + tok;
      const float l = *lp;
      *lp = l > 0.f ? l / p : l * p;
    }
  }
}

}  // namespace

int lk_select_tokens(const void* logits, int is_bf16, long ls, int B, int V, const float* temps,
                     unsigned long long seed, int step, int* out, hipStream_t st) {
  if (B <= 0) return 0;
  if (ls % 8 && is_bf16) return -1;
  if (is_bf16) {
    if (temps) select_kernel<true, true><<<B, 256, 0, st>>>(logits, ls, V, temps, seed, step, out);
    else select_kernel<true, false><<<B, 256, 0, st>>>(logits, ls, V, temps, seed, step, out);
  } else {
    if (temps) select_kernel<false, true><<<B, 256, 0, st>>>(logits, ls, V, temps, seed, step, out);
    else select_kernel<false, false><<<B, 256, 0, st>>>(logits, ls, V, temps, seed, step, out);
  }
  return 0;
}

int lk_argmax_key(const void* logits, int is_bf16, long ls, int B, int V, int vocab_lo, long long* keys, hipStream_t st) {
  if (B <= 0) return 0;
  if (ls % 8 && is_bf16) return -1;
  if (is_bf16) select_kernel<true, false, false, true><<<B, 256, 0, st>>>(logits, ls, V, nullptr, 0, 0, nullptr, nullptr, keys, vocab_lo);
  else select_kernel<false, false, false, true><<<B, 256, 0, st>>>(logits, ls, V, nullptr, 0, 0, nullptr, nullptr, keys, vocab_lo);
  return 0;
}

int lk_keys_to_ids(const long long* keys, int W, int R, int* ids, hipStream_t st) {
  if (R <= 0) return 0;
  if (W < 1) return -1;
  keys_to_ids_kernel<<<(R + 255) / 256, 256, 0, st>>>(keys, W, R, ids);
  return 0;
}

int lk_select_allowed(const void* logits, int is_bf16, long ls, int B, int V, const float* temps,
                      unsigned long long seed, int step, const int* plan, int* out, hipStream_t st) {
  if (B <= 0) return 0;
  if ((ls % 8 && is_bf16) || !plan) return -1;
  if (is_bf16) {
    if (temps) select_kernel<true, true, true><<<B, 256, 0, st>>>(logits, ls, V, temps, seed, step, out, plan);
    else select_kernel<true, false, true><<<B, 256, 0, st>>>(logits, ls, V, temps, seed, step, out, plan);
  } else {
    if (temps) select_kernel<false, true, true><<<B, 256, 0, st>>>(logits, ls, V, temps, seed, step, out, plan);
    else select_kernel<false, false, true><<<B, 256, 0, st>>>(logits, ls, V, temps, seed, step, out, plan);
  }
  return 0;
}

int lk_repeat_penalty(void* logits, int is_bf16, long ls, int B, const int* window, int W,
                      const float* penalty, hipStream_t st) {
  if (B <= 0 || W <= 0) return 0;
  if (is_bf16) repeat_penalty_kernel<true><<<B, 64, 0, st>>>(logits, ls, window, W, penalty);
  else repeat_penalty_kernel<false><<<B, 64, 0, st>>>(logits, ls, window, W, penalty);
  return 0;
}

// ---------------------------------------------------------------------------------------
// Ollama-default sampling on the device (temperature 0.8, top-k 40, top-p 0.9, repeat
// penalty 1.1 over the last 64 generated tokens): two launches per step, no host work
// beyond one per-row parameter row.
//
//   sample_penalty_kernel: per row, the window of the sequence's device history ring
//     (hist[slot][*], the last min(len, last_n) tokens) is de-duplicated and applied to
//     the f32 logits in place (l > 0 ? l / p : l * p).
//   sample_topkp_kernel (1024 threads per row):
//     1. each thread's max over its strided slice of the row;
//     2-3. top_n_sorted (below): the top K finite entries by (value desc, index asc);
//     4. p_i = exp((v_i - v_0) / T), inclusive scan; keep i while the mass before it is
//        <= top_p * total (so the token crossing top_p is kept); draw u from a counter-based
//        hash of (request seed, generated-token position) and pick the first kept i with
//        prefix > u * kept_total;
//     5. the token goes to out[row] and is appended to the ring (len + 1).
//   Greedy rows (T <= 0) take K = 1: the argmax with the lowest index among ties.
// Row parameters (8 x 32-bit): temperature, top_p, repeat_penalty (f32), top_k, last_n,
// slot, reset (1 = new sequence: its ring restarts empty), seed (i32).
// Sampler controls (docs/sampling.md): rows of 12 add [8] min_p, [9] presence, [10] frequency
// penalty (f32), [11] = 0, and an optional CSR operand carries per-row logit biases.  The chain
// is bias -> penalties (l = rp(l) - (c * frequency + presence) per unique window token with c
// occurrences) -> top-k -> temperature softmax -> top-p -> min-p -> draw; greedy rows take
// the argmax after bias and penalties.  8-wide rows without a bias run the code they always did.
// With top_k = 0 the candidate list is the kSampKMax largest.
constexpr int kSampThreads = 1024, kSampKMax = 1024, kCand = 4096;

LK_DEVICE unsigned fkey(float f) {  // order-preserving float -> uint
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// fkey puts -0.0 (kNegZeroKey) one below +0.0, but gt(), torch.argmax and a stable sort hold the two
// equal, and select_kernel's KEY arm keys them alike: a tie between them goes to the lower id.  So
// every key that is sorted, or compared for equality, is zkey(fkey(x)).  The two passes over the whole
// row (per-thread maxima, gather) stay on raw keys -- they are the cost of these kernels -- with a bound
// of +0.0 lowered to -0.0, which gathers both zeros; zkey is applied to the gathered list before it is sorted.
constexpr unsigned kNegZeroKey = 0x7FFFFFFFu, kPosZeroKey = 0x80000000u;
LK_DEVICE unsigned zkey(unsigned k) { return k == kNegZeroKey ? kPosZeroKey : k; }
LK_DEVICE unsigned zbound(unsigned t0) { return t0 == kPosZeroKey ? kNegZeroKey : t0; }
constexpr unsigned kNegInfKey = 0x007FFFFFu;  // fkey(-inf); NaN with the sign bit below it
LK_DEVICE float keyf(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// One workgroup per row.  The window's tokens are de-duplicated through a V-bit "seen" bitmap
// in LDS (one atomicOr per entry; the thread that sets a token's bit penalises it): O(window)
// for any repeat_last_n, including -1 (= the whole ring, sized to max_model_len by the engine).
// EXT (12-wide rows and / or a bias operand): the row's logit bias first (one thread per CSR
// entry, ids unique within a row; complete behind a workgroup barrier before a penalty reads a
// logit), then l = rp(l) - presence by each token's owner, then -- behind a second barrier --
// one fp32 atomic add of -frequency per window entry: c adds of the same value onto the
// owner's result, so the sum does not depend on the order the entries arrive in (the same
// bits run to run), in O(window) and with no memory but the row itself.
template <bool EXT>
__global__ __launch_bounds__(256) void sample_penalty_kernel(float* __restrict__ logits, long ls, int V,
                                                             const int* __restrict__ prm, int pw,
                                                             const int* __restrict__ bias, int bias_n,
                                                             const int* __restrict__ hist,
                                                             const int* __restrict__ hist_len, int W) {
  extern __shared__ unsigned seen[];
  const int row = blockIdx.x;
  const int* p = EXT ? prm + (long)row * pw : prm + row * 8;
  const float pen = __int_as_float(p[2]);
  const int last_n = p[4], slot = p[5], reset = p[6];
  float presence = 0.f, freq = 0.f;
  float* lp = logits + (long)row * ls;
  if constexpr (EXT) {
    if (pw == 12) {
      presence = __int_as_float(p[9]);
      freq = __int_as_float(p[10]);
    }
    if (bias) {  // uniform per workgroup
      const int B = gridDim.x;
      // offsets clamped to the buffer's own n entries: a malformed operand reads nothing outside it
      const int b0 = min(max(bias[row], 0), bias_n), b1 = min(bias[row + 1], bias_n);
      const int* ids = bias + B + 1;
      const int* val = ids + bias_n;
      for (int j = b0 + threadIdx.x; j < b1; j += blockDim.x) {
        const int id = ids[j];
        if (id >= 0 && id < V) lp[id] += __int_as_float(val[j]);  // -inf (a grammar mask) stays -inf
      }
    }
    __syncthreads();  // every thread of the workgroup: the bias is complete before a penalty reads
    if ((pen == 1.f && presence == 0.f && freq == 0.f) || last_n == 0) return;  // uniform per workgroup
  } else {
    if (pen == 1.f || last_n == 0) return;  // uniform per workgroup
  }
  const int hl = reset ? 0 : hist_len[slot];
  const int n = min(min(hl, last_n > 0 ? last_n : W), W);
  if (n == 0) return;
  const int words = (V + 31) >> 5;
  for (int i = threadIdx.x; i < words; i += blockDim.x) seen[i] = 0u;
  __syncthreads();
  const int* h = hist + (long)slot * W;
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    const int tok = h[(hl - 1 - j) % W];
    if (tok < 0 || tok >= V) continue;
    const unsigned bit = 1u << (tok & 31);
    if (atomicOr(&seen[tok >> 5], bit) & bit) continue;  // another entry of the window owns it
    const float l = lp[tok];
    float x = l > 0.f ? l / pen : l * pen;
    if constexpr (EXT) {
      if (presence != 0.f) x -= presence;
    }
    lp[tok] = x;
  }
  if constexpr (EXT) {
    if (freq == 0.f) return;  // uniform per workgroup
    __syncthreads();          // every owner's store is done before the counts land on it
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
      const int tok = h[(hl - 1 - j) % W];
      if (tok < 0 || tok >= V) continue;
      atomicAdd(&lp[tok], -freq);
    }
  }
}

// block-wide inclusive scan (1024 threads = 16 waves): a wave shuffle scan, then the serial sum of the
// earlier waves' totals (for float this association is the one tests/sampler_probes.py models)
template <class T>
LK_DEVICE T block_scan(T v, T* wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  __syncthreads();
  if (lane == 63) wsum[w] = v;
  __syncthreads();
  T add = 0;
  for (int i = 0; i < w; ++i) add += wsum[i];
  return v + add;
}

// bitonic sort of n (power of two <= 4 * 1024) (key desc, idx asc) pairs in LDS
LK_DEVICE bool before(unsigned ka, int ia, unsigned kb, int ib) { return ka > kb || (ka == kb && ia < ib); }
LK_DEVICE void bitonic(unsigned* key, int* idx, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += kSampThreads) {
        const int l = i ^ j;
        if (l > i) {
          const bool up = (i & k) == 0;  // this run sorted "before"-first
          const bool swap = up ? before(key[l], idx[l], key[i], idx[i]) : before(key[i], idx[i], key[l], idx[l]);
          if (swap) {
            const unsigned tk = key[i];
            key[i] = key[l];
            key[l] = tk;
            const int ti = idx[i];
            idx[i] = idx[l];
            idx[l] = ti;
          }
        }
      }
      __syncthreads();
    }
  }
}

// f(value, index) for each element of the row this thread owns: 8-element chunks (16-byte loads) strided
// over the workgroup plus a scalar tail (VEC: 16-byte-aligned rows), or a plain strided scan
template <bool BF16, bool VEC, class F>
LK_DEVICE void lp_scan_row(const void* rowp, int V, F&& f) {
  const int tid = threadIdx.x;
  const int nv = VEC ? V / 8 : 0;
  if constexpr (BF16) {
    const bf16_t* lp = reinterpret_cast<const bf16_t*>(rowp);
    for (int c = tid; c < nv; c += kSampThreads) {
      float v[8];
      load8(lp + c * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) f(v[j], c * 8 + j);
    }
    for (int i = nv * 8 + tid; i < V; i += kSampThreads) f(bf2f(lp[i]), i);
  } else {
    const float* lp = reinterpret_cast<const float*>(rowp);
    for (int c = tid; c < nv; c += kSampThreads) {
      const float4 a = *reinterpret_cast<const float4*>(lp + c * 8);
      const float4 b = *reinterpret_cast<const float4*>(lp + c * 8 + 4);
      f(a.x, c * 8 + 0); f(a.y, c * 8 + 1); f(a.z, c * 8 + 2); f(a.w, c * 8 + 3);
      f(b.x, c * 8 + 4); f(b.y, c * 8 + 5); f(b.z, c * 8 + 6); f(b.w, c * 8 + 7);
    }
    for (int i = nv * 8 + tid; i < V; i += kSampThreads) f(lp[i], i);
  }
}

// The n largest elements of a row, sorted by (value desc, index asc), for one workgroup of kSampThreads:
// shared by sample_topkp_kernel and token_logprobs_kernel.  On entry, behind a barrier, ckey[tid] is
// the largest raw key of thread tid's elements, cidx[tid] = tid and sh.ncand = 0.
//   bound:  the n-th largest of the 1024 thread maxima (bitonic sort in LDS) is a lower bound t0 of
//           the row's n-th largest value (threads without elements hold key 0: a short row gathers whole);
//   gather: every element >= t0 is appended to the CAP-entry candidate list (about n on real logits);
//   radix:  more than CAP of them (a huge tie / plateau at or above t0) -> the exact n-th key by a
//           3-digit MSB radix select over a 2048-bin LDS histogram, then the strictly larger keys
//           (fewer than n) plus the lowest-index ties, chunk by chunk;
//   sort:   -0.0 joins +0.0 (zkey), pad to a power of two, bitonic sort.
// Returns the number of candidates nc, sorted in ckey / cidx; the first min(n, nc) are the answer.
// scan(f) calls f(value, index) for each element this thread owns (lp_scan_row); at(i) is element i.
// FINITE: -inf entries (a grammar mask) are never candidates: with fewer finite entries than n the
// bound would otherwise be -inf and every masked entry would flood the candidate list and the
// histograms (same-bin atomics); nc is then the number of finite entries.  Otherwise -inf takes part.
struct TopNScratch {
  int ncand, thr, above;  // candidate counter; the radix digit's threshold bin and the count above it
  int wsum[16];
};

template <int CAP, bool FINITE, class Scan, class At>
LK_DEVICE int top_n_sorted(unsigned* ckey, int* cidx, TopNScratch& sh, int n, int V, Scan&& scan, At&& at) {
  static_assert(CAP >= kSampThreads && CAP >= 2048, "thread maxima and the radix histogram live in ckey");
  const int tid = threadIdx.x;
  bitonic(ckey, cidx, kSampThreads);
  const unsigned t0 = zbound(FINITE ? max(ckey[n - 1], kNegInfKey + 1u) : ckey[n - 1]);
  __syncthreads();
  scan([&](float x, int i) {
    const unsigned k = fkey(x);
    if (k >= t0) {
      const int p = atomicAdd(&sh.ncand, 1);
      if (p < CAP) {
        ckey[p] = k;
        cidx[p] = i;
      }
    }
  });
  __syncthreads();
  int nc = sh.ncand;
  if (nc > CAP) {
    unsigned* hst = ckey;  // reuse the candidate buffer as a 2048-bin histogram
    unsigned prefix = 0, mask = 0;
    int kr = n;
    const int shifts[3] = {21, 10, 0}, bits[3] = {11, 11, 10};
    for (int d = 0; d < 3; ++d) {
      const int nb = 1 << bits[d];
      for (int b = tid; b < 2048; b += kSampThreads) hst[b] = 0;
      __syncthreads();
      scan([&](float x, int) {
        const unsigned k = zkey(fkey(x));
        if ((!FINITE || k > kNegInfKey) && (k & mask) == prefix) atomicAdd(&hst[(k >> shifts[d]) & (nb - 1)], 1u);
      });
      __syncthreads();
      // thread t owns bins 2047 - 2t and 2046 - 2t: the scan runs from the top bin down
      const int hi = 2047 - 2 * tid;
      const int c_hi = hi < nb ? (int)hst[hi] : 0, c_lo = hi - 1 < nb ? (int)hst[hi - 1] : 0;
      const int incl = block_scan(c_hi + c_lo, sh.wsum);
      const int excl = incl - (c_hi + c_lo);
      if (excl < kr && incl >= kr) {
        const int b = (excl + c_hi >= kr) ? hi : hi - 1;
        sh.thr = b;
        sh.above = excl + (b == hi ? 0 : c_hi);  // elements strictly above bin b
      }
      __syncthreads();
      kr -= sh.above;
      prefix |= (unsigned)sh.thr << shifts[d];
      mask |= (unsigned)(nb - 1) << shifts[d];
      __syncthreads();
    }
    // keys > prefix (n - kr of them, fewer than n), then the first kr ties in index order
    if (tid == 0) sh.ncand = 0;
    __syncthreads();
    scan([&](float x, int i) {
      const unsigned k = zkey(fkey(x));
      if (k > prefix) {
        const int p = atomicAdd(&sh.ncand, 1);
        if (p < CAP) {
          ckey[p] = k;
          cidx[p] = i;
        }
      }
    });
    __syncthreads();
    int base = sh.ncand, need = kr;
    for (int c0 = 0; c0 < V && need > 0; c0 += kSampThreads) {
      const int i = c0 + tid;
      const bool tie = i < V && zkey(fkey(at(i))) == prefix;
      const int pos = block_scan(tie ? 1 : 0, sh.wsum);  // ties up to and including this thread
      if (tie && pos <= need) {
        ckey[base + pos - 1] = prefix;
        cidx[base + pos - 1] = i;
      }
      if (tid == kSampThreads - 1) sh.thr = pos;  // ties in this chunk
      __syncthreads();
      const int taken = min(need, sh.thr);
      base += taken;
      need -= taken;
      __syncthreads();
    }
    nc = base;
  }
  // the gathered keys are raw: -0.0 joins +0.0 here
  for (int i = tid; i < nc; i += kSampThreads) ckey[i] = zkey(ckey[i]);
  int n2 = 1;
  while (n2 < nc) n2 <<= 1;
  for (int i = nc + tid; i < n2; i += kSampThreads) {
    ckey[i] = 0;
    cidx[i] = 0x7fffffff;
  }
  __syncthreads();
  bitonic(ckey, cidx, n2);
  return nc;
}

// WIDE: 12-wide parameter rows; [8] = min_p joins the top-p cut in step 4
template <bool WIDE>
__global__ __launch_bounds__(kSampThreads) void sample_topkp_kernel(const float* __restrict__ logits, long ls, int V,
                                                                   const int* __restrict__ prm,
                                                                   int* __restrict__ hist,
                                                                   int* __restrict__ hist_len, int W,
                                                                   unsigned long long seed, int* __restrict__ out) {
  __shared__ unsigned ckey[kCand];
  __shared__ int cidx[kCand];
  __shared__ float wsum[16];
  __shared__ TopNScratch sh;
  const int row = blockIdx.x, tid = threadIdx.x;
  // (8-wide: the 32-bit offset this kernel always used.  A 64-bit one is an instruction shorter, moves
  // the sort loops 4 bytes and measured 0.5 % slower: docs/sampling.md)
  const int* p = WIDE ? prm + (long)row * 12 : prm + row * 8;
  const float temp = __int_as_float(p[0]), top_p = __int_as_float(p[1]);
  const float min_p = WIDE ? __int_as_float(p[8]) : 0.f;
  const int top_k = p[3], slot = p[5], reset = p[6], rseed = p[7];
  const bool greedy = temp <= 0.f;
  const int K = greedy ? 1 : min(top_k > 0 ? top_k : kSampKMax, min(V, kSampKMax));
  const float* lp = logits + (long)row * ls;

  // 1. per-thread maxima
  unsigned tmax = 0;
  for (int i = tid; i < V; i += kSampThreads) tmax = max(tmax, fkey(lp[i]));
  ckey[tid] = tmax;
  cidx[tid] = tid;
  if (tid == 0) sh.ncand = 0;
  __syncthreads();
  // 2-3. the top K finite entries, sorted (the plain strided scan, as in step 1)
  const int nc = top_n_sorted<kCand, true>(
      ckey, cidx, sh, K, V, [&](auto&& f) { lp_scan_row<false, false>(lp, V, f); }, [&](int i) { return lp[i]; });
  const int k_eff = min(K, nc);  // fewer finite entries than K: all of them
  // 4. temperature softmax over the top K, top-p cut, inverse-CDF draw
  int tok;
  if (greedy || k_eff <= 1) {
    tok = k_eff == 0 ? 0 : cidx[0];  // a fully masked row (all -inf) yields id 0
  } else {
    const float v0 = keyf(ckey[0]);
    const float invt = 1.f / temp;
    const float e = tid < k_eff ? __expf((keyf(ckey[tid]) - v0) * invt) : 0.f;
    const float incl = block_scan(e, wsum);
    __shared__ float tot_s, keep_s;
    __shared__ int nkeep_s;
    if (tid == k_eff - 1) tot_s = incl;
    if (tid == 0) nkeep_s = 0;
    __syncthreads();
    // min-p: p_i >= min_p * p_0, i.e. e_i >= min_p (e_0 = 1); e falls with i, so this is a prefix
    // too and the kept set is the shorter of the two (candidate 0 always stays)
    bool keep = tid < k_eff && (incl - e) <= top_p * tot_s;
    if constexpr (WIDE) keep = keep && (min_p <= 0.f || tid == 0 || e >= min_p);
    if (keep) atomicMax(&nkeep_s, tid + 1);
    __syncthreads();
    if (tid == nkeep_s - 1) keep_s = incl;
    __syncthreads();
    const int hl = reset ? 0 : hist_len[slot];
    // one draw per (request seed, generated-token position): reproducible per request, independent
    // of which batch row or engine step the sequence lands in
    const unsigned hsh = hash3((unsigned)(seed ^ (seed >> 32)), (unsigned)rseed, (unsigned)hl);
    const float u = u01(hsh) * keep_s;  // u01 < 1: a kept candidate of mass 0 at the end of the list is never the pick
    // the first kept i whose inclusive prefix exceeds u
    __shared__ int pick_s;
    if (tid == 0) pick_s = nkeep_s - 1;
    __syncthreads();
    if (tid < nkeep_s && incl > u && (tid == 0 || incl - e <= u)) atomicMin(&pick_s, tid);
    __syncthreads();
    tok = cidx[pick_s];
  }
  // 5. emit + append to the history ring
  if (tid == 0) {
    const int hl = reset ? 0 : hist_len[slot];
    out[row] = tok;
    hist[(long)slot * W + hl % W] = tok;
    hist_len[slot] = hl + 1;
  }
}

int lk_sample(float* logits, long ls, int B, int V, const int* prm, int pw, const int* bias, int bias_n, int* hist,
              int* hist_len, int W, unsigned long long seed, int* out, hipStream_t st) {
  if (B <= 0) return 0;
  if (V < 1 || W < 1 || (pw != 8 && pw != 12) || (bias && bias_n < 0)) return -1;
  const size_t seen_bytes = (size_t)((V + 31) >> 5) * 4;
  if (seen_bytes > 160 * 1024) return -1;  // the LDS "seen" bitmap: V <= 1.3M
  if (pw == 12 || bias) {
    if (seen_bytes > 64 * 1024) {
      LK_SET_MAX_LDS(sample_penalty_kernel<true>, 160 * 1024);
    }
    sample_penalty_kernel<true><<<B, 256, seen_bytes, st>>>(logits, ls, V, prm, pw, bias, bias_n, hist, hist_len, W);
  } else {
    if (seen_bytes > 64 * 1024) {
      LK_SET_MAX_LDS(sample_penalty_kernel<false>, 160 * 1024);
    }
    sample_penalty_kernel<false><<<B, 256, seen_bytes, st>>>(logits, ls, V, prm, 8, nullptr, 0, hist, hist_len, W);
  }
  LK_CHECK_LAUNCH();
  if (pw == 12) sample_topkp_kernel<true><<<B, kSampThreads, 0, st>>>(logits, ls, V, prm, hist, hist_len, W, seed, out);
  else sample_topkp_kernel<false><<<B, kSampThreads, 0, st>>>(logits, ls, V, prm, hist, hist_len, W, seed, out);
  LK_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------
// Token log-probabilities (OpenAI / Ollama `logprobs`, `top_logprobs`): for each requesting
// batch row, log softmax of the row's logits AS THE LM HEAD WROTE THEM at the chosen id and
// at the n <= 20 most likely ids, ordered like the sampler orders (value desc, id asc).
// One workgroup of 1024 threads per requesting row, bf16 rows read as bf16:
//   1. one pass with 16-byte loads: each thread keeps an online (max, sum exp(x - max)) pair
//      and the largest key of its elements; a butterfly + 16-wave combine gives the row
//      maximum and log-sum-exp (exponents are only ever taken of x - a running maximum);
//   2-3. top_n_sorted (above) with a kLpCand-entry candidate list: the top n by the same order, its
//      row passes with 16-byte loads too.  -inf entries take part (logprob -inf, after every
//      finite value).
// Keys are compared on the loaded values themselves; the logits are never written.
constexpr int kLpMaxN = 20, kLpCand = 2048;

// (max, sum exp(x - max)) of two partial rows; an empty part is (-FLT_MAX, 0)
LK_DEVICE void lse_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  m = mn;
}

template <bool BF16, bool VEC>
__global__ __launch_bounds__(kSampThreads) void token_logprobs_kernel(const void* __restrict__ logits, long ls, int B, int V,
                                                                     const int* __restrict__ rows,
                                                                     const int* __restrict__ ids, int n,
                                                                     float* __restrict__ chosen_lp,
                                                                     float* __restrict__ top_lp,
                                                                     int* __restrict__ top_id) {
  __shared__ unsigned ckey[kLpCand];
  __shared__ int cidx[kLpCand];
  __shared__ float wm[16], ws[16];
  __shared__ TopNScratch sh;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row = rows[r];
  if (row < 0 || row >= B) {  // uniform per workgroup: a row outside the batch is never read
    if (tid == 0) chosen_lp[r] = __uint_as_float(0x7FC00000u);
    if (tid < n) {
      top_lp[(long)r * n + tid] = __uint_as_float(0x7FC00000u);
      top_id[(long)r * n + tid] = -1;
    }
    return;
  }
  const void* rowp = BF16 ? (const void*)(reinterpret_cast<const bf16_t*>(logits) + (long)row * ls)
                          : (const void*)(reinterpret_cast<const float*>(logits) + (long)row * ls);
  auto at = [&](int i) -> float {
    if constexpr (BF16) return bf2f(reinterpret_cast<const bf16_t*>(rowp)[i]);
    else return reinterpret_cast<const float*>(rowp)[i];
  };

  // 1. online (max, sum exp) and the thread's largest key
  float m = -3.402823466e+38f, s = 0.f;
  unsigned tmax = 0;
  lp_scan_row<BF16, VEC>(rowp, V, [&](float x, int) {
    const float mn = fmaxf(m, x);
    s = s * __expf(m - mn) + __expf(x - mn);
    m = mn;
    tmax = max(tmax, fkey(x));
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_merge(m, s, m2, s2);
  }
  if (lane == 0) {
    wm[w] = m;
    ws[w] = s;
  }
  ckey[tid] = tmax;
  cidx[tid] = tid;
  if (tid == 0) sh.ncand = 0;
  __syncthreads();
  m = wm[0];
  s = ws[0];
  for (int j = 1; j < 16; ++j) lse_merge(m, s, wm[j], ws[j]);  // the same order in every thread
  const float rowmax = m, logsum = logf(s);
  if (tid == 0) {
    const int id = ids[row];
    chosen_lp[r] = (id >= 0 && id < V) ? (at(id) - rowmax) - logsum : __uint_as_float(0x7FC00000u);
  }
  if (n == 0) return;  // uniform

  // 2-3. the top n, sorted
  const int nc = top_n_sorted<kLpCand, false>(
      ckey, cidx, sh, n, V, [&](auto&& f) { lp_scan_row<BF16, VEC>(rowp, V, f); }, at);
  if (tid < n) {
    const bool ok = tid < nc;  // always: the row has at least n elements
    top_lp[(long)r * n + tid] = ok ? (keyf(ckey[tid]) - rowmax) - logsum : __uint_as_float(0x7FC00000u);
    top_id[(long)r * n + tid] = ok ? cidx[tid] : -1;
  }
}

int lk_token_logprobs(const void* logits, int is_bf16, long ls, int B, int V, const int* rows, int R,
                      const int* ids, int n, float* chosen_lp, float* top_lp, int* top_id, hipStream_t st) {
  if (n < 0 || n > kLpMaxN) return -1;
  if (R <= 0) return 0;
  if (B < 1 || V < 1 || ls < V) return -1;
  if (n > V) n = V;
  // 16-byte loads need 16-byte-aligned rows; any other layout is scanned element by element
  const bool vec = ls % 8 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
  if (is_bf16) {
    if (vec) token_logprobs_kernel<true, true><<<R, kSampThreads, 0, st>>>(logits, ls, B, V, rows, ids, n, chosen_lp, top_lp, top_id);
    else token_logprobs_kernel<true, false><<<R, kSampThreads, 0, st>>>(logits, ls, B, V, rows, ids, n, chosen_lp, top_lp, top_id);
  } else {
    if (vec) token_logprobs_kernel<false, true><<<R, kSampThreads, 0, st>>>(logits, ls, B, V, rows, ids, n, chosen_lp, top_lp, top_id);
    else token_logprobs_kernel<false, false><<<R, kSampThreads, 0, st>>>(logits, ls, B, V, rows, ids, n, chosen_lp, top_lp, top_id);
  }
  LK_CHECK_LAUNCH();
  return 0;
}
