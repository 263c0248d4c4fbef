// Guided-decoding mask over [B, V] logits: structured outputs (guided choice / regex / JSON schema).
//
// Every constrained row has a byte-level DFA (llmd_amd/guided/compiler.py) and a current state.
// For every token t of the vocabulary the kernel walks the token's bytes through the DFA from
// the row's state and writes -inf where the grammar forbids the token:
//   keep(t)  =  len(t) > 0  and  no byte of t leads to state 0 (dead)
//   keep(e)  =  the row's state is accepting            for the EOS ids e
// Kept entries are not rewritten with another value (their bits stay), entries at index >= V
// and rows with state -1 (unconstrained) are never touched.
//
// DFA arena: trans uint16 [cap, 256] and accept uint8 [cap] hold the grammars one after the
// other; a row's grammar has its n states at arena rows [off, off + n), and the table entries
// are LOCAL state numbers (0 dead, 1 start), so a grammar can sit at any offset.
//
// Grid (B, nsp): a row may be split over nsp workgroups (small batches), each taking a
// contiguous range of 8-token chunks; a thread owns whole chunks (one 16-byte access of bf16
// logits, two of fp32), so no entry is shared between threads. The 1024-thread workgroup
// stages its row's table in LDS when it has at most LDS_STATES states (64 KiB of the CU's
// 160 KiB: two workgroups = 32 waves per CU, full occupancy); larger grammars are read
// through L2, where a step's few hot states stay resident.
//
// Every index is checked before use: a state outside [0, n), a token whose byte range leaves
// the table and a byte walk past MAX_TOKEN_BYTES all count as "forbidden", never as an
// address.
#include "llmd_common.h"

using namespace llmd;

namespace {

constexpr int NT = 1024;
constexpr int LDS_STATES = 128;         // x 256 x 2 B = 64 KiB
constexpr int MAX_EOS = 8;
constexpr int MAX_TOKEN_BYTES = 1024;   // longer tokens are forbidden (real vocabularies: <= 256)

struct EosIds {
  int n;
  int id[MAX_EOS];
};

// true when token t, whose bytes are bytes[b0 .. b1), is kept
template <bool LDS>
__device__ __forceinline__ bool keep_token(int t, const uint16_t* __restrict__ tab, int n_states, int state,
                                           bool accepting, const uint8_t* __restrict__ bytes, int64_t nbytes,
                                           int b0, int b1, const EosIds& eos) {
#pragma unroll
  for (int k = 0; k < MAX_EOS; ++k)
    if (k < eos.n && t == eos.id[k]) return accepting;
  if (b0 < 0 || b1 <= b0 || (int64_t)b1 > nbytes || b1 - b0 > MAX_TOKEN_BYTES) return false;
  int s = state;
  for (int p = b0; p < b1; ++p) {
    s = tab[s * 256 + bytes[p]];
    // LDS holds exactly n_states rows and the global table is read only inside the grammar's rows
    if (s == 0 || s >= n_states) return false;
  }
  return true;
}

template <bool BF16, bool LDS>
__device__ __forceinline__ void mask_range(void* row, int V, int c0, int c1, bool tail, const uint16_t* tab,
                                           int n_states, int state, bool accepting,
                                           const uint8_t* __restrict__ bytes, int64_t nbytes,
                                           const int* __restrict__ tok_off, const EosIds& eos) {
  for (int c = c0 + (int)threadIdx.x; c < c1; c += NT) {
    const int t0 = c * 8;
    int off[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) off[j] = tok_off[t0 + j];  // t0 + 8 <= V: tok_off has V + 1 entries
    // one token after the other: walking the 8 in lockstep (8 load chains in flight) measured 5-24 %
    // slower at 8 waves per SIMD (profiles/guided_mask.txt)
    uint32_t drop = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (!keep_token<LDS>(t0 + j, tab, n_states, state, accepting, bytes, nbytes, off[j], off[j + 1], eos))
        drop |= 1u << j;
    if (drop == 0) continue;
    if (BF16) {
      u32x4_t* p = reinterpret_cast<u32x4_t*>((uint16_t*)row + t0);
      u32x4_t v = *p;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (drop & (1u << j)) v[j >> 1] = (j & 1) ? ((v[j >> 1] & 0x0000ffffu) | 0xff800000u)
                                                  : ((v[j >> 1] & 0xffff0000u) | 0x0000ff80u);
      *p = v;
    } else {
      u32x4_t* p = reinterpret_cast<u32x4_t*>((float*)row + t0);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (((drop >> (4 * h)) & 0xfu) == 0) continue;
        u32x4_t v = p[h];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (drop & (1u << (4 * h + j))) v[j] = 0xff800000u;
        p[h] = v;
      }
    }
  }
  if (tail) {  // the last V % 8 entries, one per thread
    const int t = (V / 8) * 8 + (int)threadIdx.x;
    if (t < V && !keep_token<LDS>(t, tab, n_states, state, accepting, bytes, nbytes, tok_off[t], tok_off[t + 1], eos)) {
      if (BF16)
        ((uint16_t*)row)[t] = 0xff80u;
      else
        ((uint32_t*)row)[t] = 0xff800000u;
    }
  }
}

template <bool BF16>
__global__ __launch_bounds__(NT) void guided_mask_kernel(void* __restrict__ logits, int64_t stride, int V,
                                                         const uint16_t* __restrict__ trans,
                                                         const uint8_t* __restrict__ accept, int cap,
                                                         const int* __restrict__ dfa_off,
                                                         const int* __restrict__ dfa_n,
                                                         const int* __restrict__ states,
                                                         const uint8_t* __restrict__ bytes, int64_t nbytes,
                                                         const int* __restrict__ tok_off, EosIds eos) {
  __shared__ uint16_t s_tab[LDS_STATES * 256];
  const int row = blockIdx.x, nsp = gridDim.y, sp = blockIdx.y;
  const int state = states[row];
  if (state < 0) return;  // unconstrained row (uniform over the workgroup)
  const int off = dfa_off[row], n = dfa_n[row];
  void* r = BF16 ? (void*)((uint16_t*)logits + (int64_t)row * stride) : (void*)((float*)logits + (int64_t)row * stride);
  const int nchunk = V / 8, per = (nchunk + nsp - 1) / nsp;
  const int c0 = min(nchunk, sp * per), c1 = min(nchunk, c0 + per);
  const bool tail = sp == nsp - 1;
  // the host wrapper validated these; a violation masks the whole row instead of reading outside the arena
  const bool ok = off >= 0 && n >= 2 && (int64_t)off + n <= (int64_t)cap && state < n;
  if (!ok) {
    EosIds none;
    none.n = 0;
    mask_range<BF16, false>(r, V, c0, c1, tail, trans, 0, 0, false, bytes, 0, tok_off, none);
    return;
  }
  const bool accepting = accept[off + state] != 0;
  const uint16_t* g = trans + (int64_t)off * 256;
  if (n <= LDS_STATES) {
    const u32x4_t* src = reinterpret_cast<const u32x4_t*>(g);  // arena rows are 512 B: 16-byte aligned
    u32x4_t* dst = reinterpret_cast<u32x4_t*>(s_tab);
    for (int i = threadIdx.x; i < n * 32; i += NT) dst[i] = src[i];
    __syncthreads();
    mask_range<BF16, true>(r, V, c0, c1, tail, s_tab, n, state, accepting, bytes, nbytes, tok_off, eos);
  } else {
    mask_range<BF16, false>(r, V, c0, c1, tail, g, n, state, accepting, bytes, nbytes, tok_off, eos);
  }
}

}  // namespace

extern "C" int llmd_guided_lds_states() { return LDS_STATES; }
extern "C" int llmd_guided_max_eos() { return MAX_EOS; }

// rows split over nsp workgroups each: ~2 workgroups per CU in total, >= 2 chunks of 8 per thread
extern "C" int llmd_guided_splits(int B, int V) {
  if (B <= 0) return 1;
  int nsp = (512 + B - 1) / B;
  const int lim = V / (8 * NT * 2);
  nsp = nsp < lim ? nsp : lim;
  nsp = nsp < 16 ? nsp : 16;
  return nsp > 1 ? nsp : 1;
}

extern "C" void llmd_guided_mask(void* logits, int64_t stride, int B, int V, int is_bf16, const uint16_t* trans,
                                 const uint8_t* accept, int cap, const int* dfa_off, const int* dfa_n,
                                 const int* states, const uint8_t* bytes, int64_t nbytes, const int* tok_off,
                                 const int* eos_ids, int n_eos, hipStream_t st) {
  if (B == 0 || V == 0) return;
  EosIds eos;
  eos.n = n_eos < MAX_EOS ? n_eos : MAX_EOS;
  for (int k = 0; k < MAX_EOS; ++k) eos.id[k] = k < eos.n ? eos_ids[k] : -1;
  const dim3 grid(B, llmd_guided_splits(B, V));
  if (is_bf16)
    hipLaunchKernelGGL(guided_mask_kernel<true>, grid, dim3(NT), 0, st, logits, stride, V, trans, accept, cap,
                       dfa_off, dfa_n, states, bytes, nbytes, tok_off, eos);
  else
    hipLaunchKernelGGL(guided_mask_kernel<false>, grid, dim3(NT), 0, st, logits, stride, V, trans, accept, cap,
                       dfa_off, dfa_n, states, bytes, nbytes, tok_off, eos);
}
