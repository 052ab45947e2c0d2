// Small per-step data movement of the engine's forward, so a steady-state step runs no
// framework (at::native) kernels: the embedding gather from int32 token ids (vocab-parallel
// masked form included), the in-flight decode-id gather of pipelined steps, and the row gather
// of the hidden states that feed the LM head, and the compaction of the rows the last decoder
// layer still computes (residual / attention rows, their sum-of-squares planes and positions).
// Each is one launch of 16-B vector copies.
#include "common.h"
#include "kernels.h"

// token ids outside a whole (non-sharded) table since the last lk_embed_errors() read: a bad id
// must not pass as a silent zero embedding (the engine polls this with the GEMM health check)
__device__ int g_embed_bad_ids = 0;

namespace {

// out[t, :] = table[ids[t] - lo, :] if lo <= ids[t] < lo + n_local else 0   (row of H bf16);
// strict (the whole table, no vocab shard): an id outside it is also counted in g_embed_bad_ids
__global__ __launch_bounds__(256) void embed_rows_kernel(bf16_t* __restrict__ out, const bf16_t* __restrict__ table,
                                                         const int* __restrict__ ids, long T, int H, long lo,
                                                         long n_local, int strict) {
  const int vpr = H >> 3;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= T * vpr) return;
  const long t = i / vpr;
  const int c = (int)(i - t * vpr);
  const long id = (long)ids[t] - lo;
  uint4_t v = {0u, 0u, 0u, 0u};
  if (id >= 0 && id < n_local) v = *reinterpret_cast<const uint4_t*>(table + id * H + c * 8);
  else if (strict && c == 0) atomicAdd(&g_embed_bad_ids, 1);
  *reinterpret_cast<uint4_t*>(out + t * H + c * 8) = v;
}

// ids[dst[i]] = prev[src[i]]
__global__ __launch_bounds__(256) void scatter_ids_kernel(int* __restrict__ ids, const long* __restrict__ dst,
                                                          const int* __restrict__ prev, const long* __restrict__ src,
                                                          int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) ids[dst[i]] = prev[src[i]];
}

// out[r, :] = x[idx[r], :]  (rows of H bf16, x row stride xs)
__global__ __launch_bounds__(256) void gather_rows_kernel(bf16_t* __restrict__ out, const bf16_t* __restrict__ x,
                                                          long xs, const long* __restrict__ idx, long R, int H) {
  const int vpr = H >> 3;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= R * vpr) return;
  const long r = i / vpr;
  const int c = (int)(i - r * vpr);
  *reinterpret_cast<uint4_t*>(out + r * H + c * 8) = *reinterpret_cast<const uint4_t*>(x + idx[r] * xs + c * 8);
}

// The last layer's rows: work item i copies one 16-B vector of an `a` row, then of a `b` row, then
// one plane entry, then one position (four ranges of one flat index; absent parts are empty).
struct GatherStep {
  const long* idx;
  long R, T;
  const bf16_t* a; long a_ld; bf16_t* a_out; int va;  // va = Ha / 8 vectors per row
  const bf16_t* b; long b_ld; bf16_t* b_out; int vb;
  const float* ss; long ss_ld; float* ss_out; long ss_out_ld; int planes;
  const int* pos; int* pos_out;
};

__global__ __launch_bounds__(256) void gather_step_kernel(GatherStep g) {
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long na = g.R * g.va, nb = g.R * g.vb, ns = g.R * g.planes;
  const uint4_t zero = {0u, 0u, 0u, 0u};
  if (i < na) {
    const long r = i / g.va;
    const int c = (int)(i - r * g.va);
    const long s = g.idx[r];
    const bool ok = s >= 0 && s < g.T;
    *reinterpret_cast<uint4_t*>(g.a_out + (r * g.va + c) * 8) =
        ok ? *reinterpret_cast<const uint4_t*>(g.a + s * g.a_ld + c * 8) : zero;
    return;
  }
  i -= na;
  if (i < nb) {
    const long r = i / g.vb;
    const int c = (int)(i - r * g.vb);
    const long s = g.idx[r];
    const bool ok = s >= 0 && s < g.T;
    *reinterpret_cast<uint4_t*>(g.b_out + (r * g.vb + c) * 8) =
        ok ? *reinterpret_cast<const uint4_t*>(g.b + s * g.b_ld + c * 8) : zero;
    return;
  }
  i -= nb;
  if (i < ns) {
    const long p = i / g.R, r = i - p * g.R;
    const long s = g.idx[r];
    g.ss_out[p * g.ss_out_ld + r] = s >= 0 && s < g.T ? g.ss[p * g.ss_ld + s] : 0.f;
    return;
  }
  i -= ns;
  if (i < g.R && g.pos != nullptr) {
    const long s = g.idx[i];
    g.pos_out[i] = s >= 0 && s < g.T ? g.pos[s] : 0;
  }
}

}  // namespace

int lk_embed_rows(bf16_t* out, const bf16_t* table, const int* ids, long T, int H, long lo, long n_local,
                  hipStream_t st, int strict) {
  if (H % 8 || T < 0) return -1;
  if (T == 0) return 0;
  const long n = T * (H / 8);
  embed_rows_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(out, table, ids, T, H, lo, n_local, strict);
  return 0;
}

// ids outside the table counted by strict embed_rows launches on the CURRENT device since the
// last call for that device.  The device counter only grows (no read-then-reset race with a
// kernel incrementing it in between); the host keeps the last value it saw per device.
int lk_embed_errors() {
  static int last[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
  int v = 0;
  if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_embed_bad_ids), sizeof(int)) != hipSuccess) return -1;
  const int d = v - last[dev];  // (wraps only after 2^31 bad ids)
  last[dev] = v;
  return d;
}

int lk_scatter_ids(int* ids, const long* dst, const int* prev, const long* src, int n, hipStream_t st) {
  if (n < 0) return -1;
  if (n == 0) return 0;
  scatter_ids_kernel<<<(n + 255) / 256, 256, 0, st>>>(ids, dst, prev, src, n);
  return 0;
}

int lk_gather_rows(bf16_t* out, const bf16_t* x, long xs, const long* idx, long R, int H, hipStream_t st) {
  if (H % 8 || xs % 8 || R < 0) return -1;
  if (R == 0) return 0;
  const long n = R * (H / 8);
  gather_rows_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(out, x, xs, idx, R, H);
  return 0;
}

int lk_gather_step(const long* idx, long R, long T, const bf16_t* a, long a_ld, bf16_t* a_out, int Ha, const bf16_t* b,
                   long b_ld, bf16_t* b_out, int Hb, const float* ss, long ss_ld, float* ss_out, long ss_out_ld,
                   int planes, const int* pos, int* pos_out, hipStream_t st) {
  if (idx == nullptr || R < 0 || T < 1) return -1;
  if (a == nullptr) Ha = 0;
  if (b == nullptr) Hb = 0;
  if (ss == nullptr) planes = 0;
  if ((a && (!a_out || Ha < 8 || Ha % 8 || a_ld % 8 || a_ld < Ha)) || (b && (!b_out || Hb < 8 || Hb % 8 || b_ld % 8 || b_ld < Hb)))
    return -1;
  if (ss && (!ss_out || planes < 1 || ss_ld < T || ss_out_ld < R)) return -1;
  if (pos && !pos_out) return -1;
  if (R == 0) return 0;
  GatherStep g{idx, R, T, a, a_ld, a_out, Ha / 8, b, b_ld, b_out, Hb / 8, ss, ss_ld, ss_out, ss_out_ld, planes, pos, pos_out};
  const long n = R * (g.va + g.vb + planes + (pos ? 1 : 0));
  if (n == 0) return 0;
  if (n > 0x7FFFFFFFL * 256) return -1;
  gather_step_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(g);
  LK_CHECK_LAUNCH();
  return 0;
}
