// Token masks for schema-constrained decoding (docs/structured_outputs.md): one launch turns
// the step's logits [B, V] (bf16 or f32) into a private f32 copy in which every id outside its
// row's allowed set is -inf.  The allowed sets live in a device pool of bitmask rows (one per
// grammar state, uploaded once and reused for as long as the state recurs); the step sends only
// one pool-row index per batch row.  Bit v & 31 of word v >> 5 is id v (little-endian: byte
// v >> 3 of a row is np.packbits(bits, bitorder="little")[v >> 3]).
//
// A thread handles 8 consecutive ids: one mask byte, one 16-byte bf16 load (or two 16-byte f32
// loads) and two float4 stores; the grid is (ceil(V / 2048), B) at 256 threads.  Kept values are
// copied bit for bit (bf16 widens exactly; NaN payloads, infinities and -0.0 pass through: no
// arithmetic touches them).  A thread reads its 8 elements before it writes them and no other
// thread touches them, so dst may be src (f32, ld == ls).
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kMaskThreads = 256, kMaskIds = 8;

// VEC: every row start of src and dst is 16-byte aligned
template <bool BF16, bool VEC>
__global__ __launch_bounds__(kMaskThreads) void mask_logits_kernel(const void* src, long ls, float* dst, long ld, int V,
                                                                   const unsigned* __restrict__ pool, int R, int words,
                                                                   const int* __restrict__ mask_row) {
  const int b = blockIdx.y;
  const int v0 = (blockIdx.x * kMaskThreads + threadIdx.x) * kMaskIds;
  if (v0 >= V) return;
  const int mr = mask_row[b];
  // the 8 ids' bits: all kept on an unconstrained row, none on a row index outside the pool (a
  // stale index gives a visibly dead row, never a read outside the pool).  v0 < V, so byte
  // v0 >> 3 lies inside the row's `words` words.
  unsigned bits = 0xFFu;
  if (mr >= R) bits = 0u;
  else if (mr >= 0) bits = reinterpret_cast<const unsigned char*>(pool + (long)mr * words)[v0 >> 3];
  float* d = dst + (long)b * ld + v0;
  const float ninf = -INFINITY;
  if (VEC && v0 + kMaskIds <= V) {
    float x[8];
    if constexpr (BF16) {
      load8(reinterpret_cast<const bf16_t*>(src) + (long)b * ls + v0, x);
    } else {
      const float* s = reinterpret_cast<const float*>(src) + (long)b * ls + v0;
      const float4 a = *reinterpret_cast<const float4*>(s);
      const float4 c = *reinterpret_cast<const float4*>(s + 4);
      x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
      x[4] = c.x; x[5] = c.y; x[6] = c.z; x[7] = c.w;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = (bits >> j) & 1u ? x[j] : ninf;
    *reinterpret_cast<float4*>(d) = make_float4(x[0], x[1], x[2], x[3]);
    *reinterpret_cast<float4*>(d + 4) = make_float4(x[4], x[5], x[6], x[7]);
    return;
  }
  // the V % 8 tail, and rows that are not 16-byte aligned: element by element (ids >= V are
  // neither read nor written, so mask bits beyond V in the last word are ignored)
  const int n = min(kMaskIds, V - v0);
  for (int j = 0; j < n; ++j) {
    float x;
    if constexpr (BF16) x = bf2f(reinterpret_cast<const bf16_t*>(src)[(long)b * ls + v0 + j]);
    else x = reinterpret_cast<const float*>(src)[(long)b * ls + v0 + j];
    d[j] = (bits >> j) & 1u ? x : ninf;
  }
}

}  // namespace

int lk_mask_logits(const void* src, int is_bf16, long ls, float* dst, long ld, int B, int V, const unsigned* pool, int R,
                   int words, const int* mask_row, hipStream_t st) {
  if (B <= 0) return 0;
  if (V < 1 || B > 65535 || ls < V || ld < V || R < 0 || !src || !dst || !mask_row || (R > 0 && !pool)) return -1;
  if (words != (V + 31) / 32) return -1;
  // 16-byte accesses need 16-byte-aligned rows on both sides; any other layout goes element by element
  const bool vec = reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0 &&
                   ls % (is_bf16 ? 8 : 4) == 0 && ld % 4 == 0;
  const dim3 grid((V + kMaskThreads * kMaskIds - 1) / (kMaskThreads * kMaskIds), B);
  if (is_bf16) {
    if (vec) mask_logits_kernel<true, true><<<grid, kMaskThreads, 0, st>>>(src, ls, dst, ld, V, pool, R, words, mask_row);
    else mask_logits_kernel<true, false><<<grid, kMaskThreads, 0, st>>>(src, ls, dst, ld, V, pool, R, words, mask_row);
  } else {
    if (vec) mask_logits_kernel<false, true><<<grid, kMaskThreads, 0, st>>>(src, ls, dst, ld, V, pool, R, words, mask_row);
    else mask_logits_kernel<false, false><<<grid, kMaskThreads, 0, st>>>(src, ls, dst, ld, V, pool, R, words, mask_row);
  }
  LK_CHECK_LAUNCH();
  return 0;
}
