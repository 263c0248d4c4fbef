// Top-N alternative log-probabilities over [B, V] logits.
//
// For row r with n = n_per_row[r] (0 <= n <= NMAX): the n largest entries, by value
// descending and lower vocabulary index first among equals (the tie rule of
// sample_kernel's better()), with  lp = x - max - log(sum exp(x - max))  over the
// whole row in fp32 (no temperature: the definition of sample_kernel's out_logprob).
// Entries equal to -inf (masked by top-k / top-p / min-p / a bias of -100) are never
// reported; unused slots hold id = -1, lp = -inf.
//
// One workgroup of 1024 threads per row. Every entry gets the 64-bit image
//   comp = (order-preserving key of the value) << 32 | ~index
// which makes the required order a strict total one: no two entries tie, and the
// answer is the n largest comps.
//   pass 1  running max / sum-exp, and the largest comp of every thread. The 64
//           maxima by lane position come from disjoint parts of the row, so the n-th
//           largest of them, T, is a lower bound of the n-th largest comp of the row.
//   pass 2  entries with comp >= T go to LDS: at least n of them, and ~n for rows whose
//           order does not follow the thread mapping (an all-equal row: ~8n).
//   select  rank of every candidate among the candidates; rank < n is its output slot.
// A row that sends more than CAP candidates (an order that follows the thread mapping)
// takes n rounds of "largest comp below the previous one" over the row instead: slow
// and exact.
//
// prompt_logprobs_kernel (prompt scoring) runs the same passes (row_top) for a row and a given
// target token, and adds the target's log-probability and rank; see there.
#include "llmd_common.h"

using namespace llmd;

namespace {

constexpr int NT = 1024, NW = NT / 64;
constexpr int NMAX = 20;   // OpenAI limit of top_logprobs
constexpr int CAP = 1024;  // candidate slots in LDS
constexpr float NEG_INF = -__builtin_huge_valf();

// order-preserving integer image of a float (sampling.hip fkey)
__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
constexpr uint32_t KEY_NEG_INF = 0x007fffffu;  // fkey(-inf): reportable entries lie above it

__device__ __forceinline__ uint64_t comp_of(uint32_t key, int i) {
  return ((uint64_t)key << 32) | (uint32_t)~(uint32_t)i;
}
__device__ __forceinline__ int comp_index(uint64_t c) { return (int)~(uint32_t)c; }

// f(x, i) for every entry of the row; a thread sees its indices in ascending order
template <bool BF16, typename F>
__device__ __forceinline__ void for_each(const void* row, int V, F&& f) {
  if (BF16) {
    const uint16_t* r = (const uint16_t*)row;
    const int nchunk = V / 8;
    for (int c = threadIdx.x; c < nchunk; c += NT) {
      float x[8];
      unpack8(*reinterpret_cast<const u32x4_t*>(r + c * 8), x);
#pragma unroll
      for (int j = 0; j < 8; ++j) f(x[j], c * 8 + j);
    }
    for (int i = nchunk * 8 + threadIdx.x; i < V; i += NT) f(bf2f(r[i]), i);
  } else {
    const float* r = (const float*)row;
    const int nchunk = V / 4;
    for (int c = threadIdx.x; c < nchunk; c += NT) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(r + c * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) f(v[j], c * 4 + j);
    }
    for (int i = nchunk * 4 + threadIdx.x; i < V; i += NT) f(r[i], i);
  }
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t ov = __shfl_xor((unsigned long long)v, o, 64);
    v = ov > v ? ov : v;
  }
  return v;
}

// One row through pass 1 / pass 2 / select, by the whole workgroup: the n best entries to oid / olp
// (unused slots -1 / -inf). SCORE: pass 1 also counts the entries >= xt (the vLLM rank of a
// target whose stored value is xt), and a row with n == 0 stops after pass 1. logZ and the count
// are returned in every thread.
template <bool BF16, bool SCORE>
__device__ __forceinline__ void row_top(const void* r, int V, int n, float xt, int* __restrict__ oid,
                                        float* __restrict__ olp, float& logZ_out, int& count_out) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  __shared__ uint64_t s_grp[NW][64];
  __shared__ uint64_t s_cand[CAP];
  __shared__ float s_mx[NW], s_se[NW];
  __shared__ unsigned long long s_T, s_best;
  __shared__ uint32_t s_cnt;
  // the per-wave counts of SCORE live in the candidate slots, which nobody writes before pass 2
  int* s_ge = reinterpret_cast<int*>(s_cand);

  // ---- pass 1: max / sum-exp (sample_kernel's guards for masked entries) and the thread's best
  float mx = NEG_INF, se = 0.f;
  uint32_t bk = KEY_NEG_INF;
  int bi = 0, ge = 0;
  for_each<BF16>(r, V, [&](float x, int i) {
    if (x > mx) {
      se = se * __expf(mx - x) + 1.f;
      mx = x;
    } else if (x != NEG_INF) {
      se += __expf(x - mx);
    }
    if (SCORE) ge += x >= xt;
    const uint32_t key = fkey(x);
    if (key > bk) {  // indices ascend: the first of equal keys stays
      bk = key;
      bi = i;
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float omx = __shfl_xor(mx, o, 64), ose = __shfl_xor(se, o, 64);
    const float nm = fmaxf(mx, omx);
    se = (mx == NEG_INF ? 0.f : se * __expf(mx - nm)) + (omx == NEG_INF ? 0.f : ose * __expf(omx - nm));
    mx = nm;
    if (SCORE) ge += __shfl_xor(ge, o, 64);
  }
  if (lane == 0) {
    s_mx[w] = mx;
    s_se[w] = se;
    if (SCORE) s_ge[w] = ge;
  }
  s_grp[w][lane] = bk > KEY_NEG_INF ? comp_of(bk, bi) : 0ull;  // 0: no reportable entry
  if (tid == 0) {
    s_T = 0ull;
    s_cnt = 0u;
  }
  __syncthreads();
  float M = s_mx[0], S = s_se[0];
#pragma unroll
  for (int k = 1; k < NW; ++k) {
    const float nm = fmaxf(M, s_mx[k]);
    S = (M == NEG_INF ? 0.f : S * __expf(M - nm)) + (s_mx[k] == NEG_INF ? 0.f : s_se[k] * __expf(s_mx[k] - nm));
    M = nm;
  }
  const float logZ = M + __logf(S);
  logZ_out = logZ;
  count_out = 0;
  if (SCORE) {
#pragma unroll
    for (int k = 0; k < NW; ++k) count_out += s_ge[k];
    if (n == 0) {  // the same in every thread: the row was read once
      if (tid < NMAX) {
        oid[tid] = -1;
        olp[tid] = NEG_INF;
      }
      return;
    }
  }
  if (w == 0) {
    uint64_t g = 0ull;
#pragma unroll
    for (int k = 0; k < NW; ++k) g = s_grp[k][lane] > g ? s_grp[k][lane] : g;
    int rank = 0;
    for (int j = 0; j < 64; ++j) rank += (uint64_t)__shfl((unsigned long long)g, j, 64) > g;
    // non-zero comps are distinct, so at most one of them has rank n-1; with fewer than
    // n non-zero maxima T stays 0 and every reportable entry is a candidate
    if (rank == n - 1) s_T = g;
  }
  __syncthreads();
  const uint64_t T = s_T;
  const uint32_t Tk = (uint32_t)(T >> 32), Ti = ~(uint32_t)T;
  const uint32_t Tlo = Tk > KEY_NEG_INF ? Tk : KEY_NEG_INF + 1u;

  // ---- pass 2: candidates comp >= T
  for_each<BF16>(r, V, [&](float x, int i) {
    const uint32_t key = fkey(x);
    if (key >= Tlo && (key > Tk || (uint32_t)i <= Ti)) {
      const uint32_t slot = atomicAdd(&s_cnt, 1u);
      if (slot < (uint32_t)CAP) s_cand[slot] = comp_of(key, i);
    }
  });
  __syncthreads();
  const int C = (int)s_cnt;
  int found;
  if (C <= CAP) {
    found = min(n, C);
    for (int c = tid; c < C; c += NT) {
      const uint64_t mine = s_cand[c];
      int rank = 0;
      for (int k = 0; k < C; ++k) rank += s_cand[k] > mine;
      if (rank < n) {
        LLMD_DCHECK(comp_index(mine) >= 0 && comp_index(mine) < V);
        oid[rank] = comp_index(mine);
        olp[rank] = unkey((uint32_t)(mine >> 32)) - logZ;
      }
    }
  } else {
    // ---- more candidates than LDS slots: n rounds of the largest comp below the previous one
    found = n;
    uint64_t prev = ~0ull;
    for (int j = 0; j < n; ++j) {
      uint64_t best = 0ull;
      for_each<BF16>(r, V, [&](float x, int i) {
        const uint32_t key = fkey(x);
        const uint64_t cm = comp_of(key, i);
        if (key > KEY_NEG_INF && cm < prev && cm > best) best = cm;
      });
      best = wave_max_u64(best);
      if (tid == 0) s_best = 0ull;
      __syncthreads();
      if (lane == 0 && best) atomicMax(&s_best, (unsigned long long)best);
      __syncthreads();
      prev = s_best;
      __syncthreads();
      if (prev == 0ull) {  // same in every thread: the row has no further reportable entry
        found = j;
        break;
      }
      if (tid == 0) {
        oid[j] = comp_index(prev);
        olp[j] = unkey((uint32_t)(prev >> 32)) - logZ;
      }
    }
  }
  if (tid >= found && tid < NMAX) {
    oid[tid] = -1;
    olp[tid] = NEG_INF;
  }
}

template <bool BF16>
__device__ __forceinline__ const void* row_ptr(const void* logits, int64_t stride, int row) {
  return BF16 ? (const void*)((const uint16_t*)logits + (int64_t)row * stride)
              : (const void*)((const float*)logits + (int64_t)row * stride);
}

template <bool BF16>
__global__ __launch_bounds__(NT) void top_logprobs_kernel(const void* __restrict__ logits, int64_t stride, int V,
                                                          const int* __restrict__ n_per_row,
                                                          int* __restrict__ out_ids, float* __restrict__ out_lp) {
  const int row = blockIdx.x, tid = threadIdx.x;
  int* oid = out_ids + (int64_t)row * NMAX;
  float* olp = out_lp + (int64_t)row * NMAX;
  const int n = min(max(n_per_row[row], 0), NMAX);
  if (n == 0) {  // nothing asked of this row: its logits are not read
    if (tid < NMAX) {
      oid[tid] = -1;
      olp[tid] = NEG_INF;
    }
    return;
  }
  float logZ;
  int count;
  row_top<BF16, false>(row_ptr<BF16>(logits, stride, row), V, n, 0.f, oid, olp, logZ, count);
}

// Prompt scoring: row r against its target token t = targets[r].
//   lp   = x[t] - logZ, logZ as in top_logprobs_kernel
//   rank = number of entries with x[i] >= x[t] (vLLM: 1 is the best, ties with the target count),
//          counted in pass 1, so a row with n_per_row == 0 is read once
//   top  = what top_logprobs_kernel reports for the row and n_per_row[r] (the same row_top)
// t outside [0, V): lp = -inf, rank = 0, and no entry is read for it. x[t] == -inf: lp = -inf, rank = V.
template <bool BF16>
__global__ __launch_bounds__(NT) void prompt_logprobs_kernel(const void* __restrict__ logits, int64_t stride, int V,
                                                             const int* __restrict__ targets,
                                                             const int* __restrict__ n_per_row,
                                                             float* __restrict__ out_lp, int* __restrict__ out_rank,
                                                             int* __restrict__ out_ids, float* __restrict__ out_tlp) {
  const int row = blockIdx.x;
  const int n = min(max(n_per_row[row], 0), NMAX);
  const void* r = row_ptr<BF16>(logits, stride, row);
  const int t = targets[row];
  const bool in_row = t >= 0 && t < V;
  float xt = 0.f;
  if (in_row) xt = BF16 ? bf2f(((const uint16_t*)r)[t]) : ((const float*)r)[t];
  float logZ;
  int count;
  row_top<BF16, true>(r, V, n, xt, out_ids + (int64_t)row * NMAX, out_tlp + (int64_t)row * NMAX, logZ, count);
  if (threadIdx.x == 0) {
    out_lp[row] = in_row && xt != NEG_INF ? xt - logZ : NEG_INF;
    out_rank[row] = in_row ? count : 0;
  }
}

}  // namespace

extern "C" int llmd_top_logprobs_max() { return NMAX; }

// out_ids / out_lp: [B, NMAX] with NMAX == llmd_top_logprobs_max()
extern "C" void llmd_top_logprobs(const void* logits, int64_t stride, int B, int V, int is_bf16,
                                  const int* n_per_row, int nmax, int* out_ids, float* out_lp, hipStream_t st) {
  if (B == 0 || nmax != NMAX) return;
  if (is_bf16)
    hipLaunchKernelGGL(top_logprobs_kernel<true>, dim3(B), dim3(NT), 0, st, logits, stride, V, n_per_row, out_ids,
                       out_lp);
  else
    hipLaunchKernelGGL(top_logprobs_kernel<false>, dim3(B), dim3(NT), 0, st, logits, stride, V, n_per_row, out_ids,
                       out_lp);
}

// out_lp / out_rank: [R]; out_ids / out_tlp: [R, NMAX] with NMAX == llmd_top_logprobs_max()
extern "C" void llmd_prompt_logprobs(const void* logits, int64_t stride, int R, int V, int is_bf16, const int* targets,
                                     const int* n_per_row, int nmax, float* out_lp, int* out_rank, int* out_ids,
                                     float* out_tlp, hipStream_t st) {
  if (R == 0 || nmax != NMAX) return;
  if (is_bf16)
    hipLaunchKernelGGL(prompt_logprobs_kernel<true>, dim3(R), dim3(NT), 0, st, logits, stride, V, targets, n_per_row,
                       out_lp, out_rank, out_ids, out_tlp);
  else
    hipLaunchKernelGGL(prompt_logprobs_kernel<false>, dim3(R), dim3(NT), 0, st, logits, stride, V, targets, n_per_row,
                       out_lp, out_rank, out_ids, out_tlp);
}
