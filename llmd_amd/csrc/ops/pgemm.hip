// Prefill ("large-M") dense bf16 GEMM: C[M, N] = A[M, K] . W[N, K]^T, the
// QKV / O / gate-up / down projections of a prefill chunk (the
// hipBLASLt Cijk_* kernels that take ~68 % of the 70B serving bench).
//
// Three kernels, the ones the dispatch table (ops/pgemm_table.py) names, all on 256 x 256
// output tiles, one workgroup per CU, operands by LDS-DMA:
//   variant 0  pgemm_kernel   8 waves, staggered 4-phase K-step (described here);
//   variant 3  pgemm6_kernel  "PGR2": 4 waves, the K-step's fragments in registers (below);
//   variant 6  pgemm7_kernel  persistent PGR2 (below); its split-K tail is pgemm6_kernel.
// Variants 0 and 3 have the plain epilogue (EPI_NONE) and the fp32 split-K partial (EPI_F32),
// variants 3 and 6 also the fused SiLU-and-mul on the [gate; up] weight (EPI_SILU_STD).
//
// Variant 0 (one 256 x 256 output tile per 512-thread workgroup, 1 per CU):
//   * 8 waves as 2 (M) x 4 (N); a wave owns 128 x 64 of C, as four 64 x 32
//     quadrants of 4 x 2 mfma_f32_16x16x32_bf16 tiles (128 accumulator regs);
//   * K-steps of 64 through TWO LDS buffers of 64 KB (A 256 x 128 B, W 256 x
//     128 B), each split into four 16 KB "halves" by the quadrant that reads
//     them (A: rows of quadrant-row 0 / 1, W: columns of quadrant-col 0 / 1).
//     A half is refilled by LDS-DMA (global_load_lds_dwordx4, no VGPR
//     staging) one phase after its last fragment read, so each K-step's loads
//     are in flight for ~6 phases, across the raw s_barriers, retired by
//     COUNTED vmcnt waits (never 0 inside the loop);
//   * 4 phases per K-step, one quadrant each (16 MFMA), fragment reads
//     front-loaded (12 / 4 / 8 / 0 ds_read_b128): both W halves stay in
//     registers for the whole K-step;
//   * waves 4-7 run one barrier behind waves 0-3 (stagger): on every SIMD one
//     wave's fragment reads + DMA issue overlap its partner's MFMA segment;
//   * 16-B chunks XOR-swizzled by (row & 7) on the DMA source address and on
//     the read (every ds_read_b128 lane group covers 16 distinct bank slots);
//   * XCD-aware tile order (each XCD walks its own contiguous range of tiles,
//     grouped 8 row-tiles deep so concurrently running tiles share A and W
//     panels in that XCD's L2);
//   * epilogue through the (then free) LDS: C is computed transposed (W frags
//     as the MFMA's first operand) so each lane holds 4 consecutive columns,
//     written as 8-B LDS stores, read back as 16-B rows and stored coalesced.
//
// Requirements (checked by the host wrapper): N % 256 == 0, K % 64 == 0,
// 16-B aligned rows; any M (rows past M are clamped on load, not stored).
#include <algorithm>
#include <type_traits>

#include "llmd_common.h"

using namespace llmd;

namespace {

constexpr int BM = 256, BN = 256, BK = 64, NT = 512;
constexpr int HALF = 16384;         // bytes of one half (128 rows x 128 B)
constexpr int BUF = 4 * HALF;       // one K-step: A q0, A q1, W q0, W q1
constexpr int LDS_BYTES = 2 * BUF;  // 128 KB
constexpr int GROUP_M = 8;

// EPI_SILU_STD (variants 3 and 6 only): the fused SiLU-and-mul on the model's own [gate; up]
// weight ([2F, K], F % 128 == 0): tile tn's W rows are gate rows [128 tn, +128) then up rows
// [F + 128 tn, +128), so tile columns [0, 128) are gate, [128, 256) the matching up, and
// silu(g) * u is stored directly as the [M, F] activation (no act kernel, no [M, 2F] round
// trip). The values are the binding's contract (1 was a pre-packed gate/up layout, removed).
enum { EPI_NONE = 0, EPI_F32 = 2, EPI_SILU_STD = 3 };

__device__ __forceinline__ void dma16(const void* src, char* lds) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src,
                                   (void __attribute__((address_space(3)))*)lds, 16, 0, 0);
}

// wait until at most n (wave-uniform, 0..10) VMEM ops of this wave are outstanding
__device__ __forceinline__ void wait_vm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
  }
}

__device__ __forceinline__ void bar() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// logical tile L (XCD-contiguous, GROUP_M-deep grouped order) -> (row tile, column tile)
__device__ __forceinline__ void tile_mn(int L, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int per_group = GROUP_M * tiles_n;
  const int g = L / per_group, first_m = g * GROUP_M;
  const int gm = min(tiles_m - first_m, GROUP_M);
  tm = first_m + (L % per_group) % gm;
  tn = (L % per_group) / gm;
}

// Launch forms (host: llmd_pgemm; pgemm6_kernel takes the same): nsplit == 1 -> tiles [tile0, tile0 + grid)
// over the whole K (data-parallel); nsplit > 1 (EPI_F32) -> the grid covers `tail` tiles from
// tile0 x nsplit K-ranges, each block writing its fp32 partial tile to ws[split][tile][256][256]
// (pgemm_splitk_reduce sums them). The tail split turns a last, mostly idle wave of tiles
// (e.g. 576 tiles = 2.25 waves over 256 CUs at M 4608, N 8192) into one short full wave.
template <int EPI>
__global__ __launch_bounds__(NT, 1) void pgemm_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                      const uint16_t* __restrict__ W, int64_t ldw,
                                                      uint16_t* __restrict__ C, int64_t ldc, int M, int N, int K,
                                                      int tile0, int nsplit, float* __restrict__ ws) {
  __shared__ __attribute__((aligned(1024))) char lds[LDS_BYTES];  // the ONLY LDS object (see moe.hip G3)
  const int tiles_m = (M + BM - 1) / BM, tiles_n = N / BN;
  // XCD-contiguous logical tile id, then GROUP_M-deep grouped order
  const int b = xcd_remap(blockIdx.x, gridDim.x);
  const int tail = gridDim.x / nsplit;
  const int t_local = b % tail, split = b / tail;
  const int nk_all = K / BK;
  const int chunk = (nk_all + nsplit - 1) / nsplit;
  const int kbeg = split * chunk;
  const int nk = min(chunk, nk_all - kbeg);
  int tm, tn;
  tile_mn(tile0 + t_local, tiles_m, tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  A += (int64_t)kbeg * BK;
  W += (int64_t)kbeg * BK;

  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int wr = w >> 2, wc = w & 3;

  // ---- DMA sources: half row i = 8 * (2w + j) + (lane >> 3), LDS chunk slot lane & 7
  // holds source chunk (lane & 7) ^ (i & 7); 32-bit element offsets from A / W
  uint32_t aoff[2][2], woff[2][2];  // [half][j]
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = 8 * (2 * w + j) + (lane >> 3);
      const int c = (lane & 7) ^ (i & 7);
      const int ar = min(m0 + (i >> 6) * 128 + h * 64 + (i & 63), M - 1);
      const int wn = n0 + (i >> 5) * 64 + h * 32 + (i & 31);
      aoff[h][j] = (uint32_t)(ar * lda + c * 8);
      woff[h][j] = (uint32_t)(wn * ldw + c * 8);
    }
  // half kinds in issue order: 0 = A q0, 1 = W q0, 2 = W q1, 3 = A q1; seq = 4 * ktile + kind
  auto issue = [&](int seq) {
    const int kt = seq >> 2, kind = seq & 3;
    char* dst = lds + (kt & 1) * BUF + (2 * w) * 1024;
    const int k0 = kt * BK;
    if (kind == 0 || kind == 3) {
      const int h = kind == 0 ? 0 : 1;
      dst += h * HALF;
      dma16(A + aoff[h][0] + k0, dst);
      dma16(A + aoff[h][1] + k0, dst + 1024);
    } else {
      const int h = kind - 1;
      dst += 2 * HALF + h * HALF;
      dma16(W + woff[h][0] + k0, dst);
      dma16(W + woff[h][1] + k0, dst + 1024);
    }
  };
  const int nseq = 4 * nk;
  int issued = 0;  // halves issued so far (wave-uniform)
  auto issue_upto = [&](int seq) {
    if (seq < nseq) {
      issue(seq);
      issued = seq + 1;
    }
  };
  // wait until half `seq` landed: 2 DMAs per younger half may stay in flight
  auto wait_seq = [&](int seq) { wait_vm(min(5, max(0, issued - seq - 1)) * 2); };

  // ---- fragment read offsets (bytes inside a half): lane row l & 15, chunk 4s + (l >> 4)
  const int fr = lane & 15, fq = lane >> 4;
  int a_rd[4][2], w_rd[2][2];  // [mi][s], [ni][s]
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = wr * 64 + mi * 16 + fr;
      a_rd[mi][s] = i * 128 + (((4 * s + fq) ^ (i & 7)) * 16);
    }
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = wc * 32 + ni * 16 + fr;
      w_rd[ni][s] = i * 128 + (((4 * s + fq) ^ (i & 7)) * 16);
    }

  f32x4_t acc[2][2][4][2];  // [qm][qn][mi][ni]: C^T tiles (row = n, col = m)
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int d = 0; d < 2; ++d) acc[a][b][c][d] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  s16x8_t afr[4][2], wfr[2][2][2];  // [mi][s], [qn][ni][s]
  auto read_a = [&](const char* hb) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int s = 0; s < 2; ++s) afr[mi][s] = *reinterpret_cast<const s16x8_t*>(hb + a_rd[mi][s]);
  };
  auto read_w = [&](const char* hb, int qn) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int s = 0; s < 2; ++s) wfr[qn][ni][s] = *reinterpret_cast<const s16x8_t*>(hb + w_rd[ni][s]);
  };
  auto mfma_q = [&](int qm, int qn) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[qm][qn][mi][ni] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[qn][ni][s], afr[mi][s], acc[qm][qn][mi][ni], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  // one phase: [reads + DMA issue + counted wait] -> lgkmcnt(0) -> barrier -> MFMA -> barrier
  auto seg_end = [&]() {
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0), visible to hipcc's waitcnt pass
    bar();
  };

  // ---- prologue: K-step 0 whole, K-step 1 but its A q1 half
#pragma unroll
  for (int s = 0; s < 7; ++s) issue_upto(s);
  wait_seq(1);
  bar();
  if (__builtin_amdgcn_readfirstlane(wr) == 1) bar();  // stagger: waves 4-7 one segment behind

  // one K-step: 4 phases of [fragment reads + DMA issue + counted wait] -> lgkmcnt(0) ->
  // barrier -> 16 MFMA -> barrier. STEADY (kt + 2 < nk): every refill exists and exactly
  // 5 younger halves (10 DMAs) stay in flight at each wait.
  auto ktile = [&](int kt, auto steady_t) {
    constexpr bool STEADY = decltype(steady_t)::value;
    const char* bufp = lds + (kt & 1) * BUF;
    // phase 1: A q0 + W q0 fragments; refill A q1 of K-step kt+1; W q1 (kt) lands for phase 2
    read_a(bufp);
    read_w(bufp + 2 * HALF, 0);
    if constexpr (STEADY) {
      issue(4 * (kt + 1) + 3);
      wait_vm(10);
    } else {
      issue_upto(4 * (kt + 1) + 3);
      wait_seq(4 * kt + 2);
    }
    seg_end();
    mfma_q(0, 0);
    bar();
    // phase 2: W q1 fragments; refill A q0 of kt+2 (its kt copy was read in phase 1)
    read_w(bufp + 3 * HALF, 1);
    if constexpr (STEADY) {
      issue(4 * (kt + 2) + 0);
      wait_vm(10);
    } else {
      issue_upto(4 * (kt + 2) + 0);
      wait_seq(4 * kt + 3);
    }
    seg_end();
    mfma_q(0, 1);
    bar();
    // phase 3: A q1 fragments; refill W q0 of kt+2
    read_a(bufp + HALF);
    if constexpr (STEADY) issue(4 * (kt + 2) + 1);
    else issue_upto(4 * (kt + 2) + 1);
    seg_end();
    mfma_q(1, 1);
    bar();
    // phase 4: no reads; refill W q1 of kt+2; A q0 + W q0 of kt+1 land for its phase 1
    if constexpr (STEADY) {
      issue(4 * (kt + 2) + 2);
      issued = 4 * (kt + 2) + 3;
      wait_vm(10);
    } else {
      issue_upto(4 * (kt + 2) + 2);
      if (kt + 1 < nk) wait_seq(4 * (kt + 1) + 1);
    }
    seg_end();
    mfma_q(1, 0);
    bar();
  };
  int kt = 0;
  for (; kt + 2 < nk; ++kt) ktile(kt, std::true_type{});
  for (; kt < nk; ++kt) ktile(kt, std::false_type{});
  if (__builtin_amdgcn_readfirstlane(wr) == 0) bar();  // balance the stagger
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (EPI == EPI_F32) {
    float* wt = ws + ((int64_t)split * tail + t_local) * (BM * BN);
#pragma unroll
    for (int qm = 0; qm < 2; ++qm)
#pragma unroll
      for (int qn = 0; qn < 2; ++qn)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const int row = wr * 128 + qm * 64 + mi * 16 + (lane & 15);
            const int col = wc * 64 + qn * 32 + ni * 16 + (lane >> 4) * 4;
            *reinterpret_cast<f32x4_t*>(wt + row * BN + col) = acc[qm][qn][mi][ni];
          }
    return;
  }
  __syncthreads();

  // ---- epilogue: acc[qm][qn][mi][ni][r] = C[m][n] with
  //   m = wr*128 + qm*64 + mi*16 + (lane & 15), n = wc*64 + qn*32 + ni*16 + (lane >> 4)*4 + r
  // wave image in LDS: [128 rows (m)][64 cols (n)] bf16, 16-B chunks XOR-swizzled by row & 7
  char* img = lds + w * 16384;
#pragma unroll
  for (int qm = 0; qm < 2; ++qm)
#pragma unroll
    for (int qn = 0; qn < 2; ++qn)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const int row = qm * 64 + mi * 16 + fr;
          const int col = qn * 32 + ni * 16 + fq * 4;  // 4 consecutive bf16 = 8 B
          const f32x4_t v = acc[qm][qn][mi][ni];
          u32x2_t p;
          p[0] = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
          p[1] = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
          const int chunk = (col >> 3) ^ (row & 7);
          *reinterpret_cast<u32x2_t*>(img + row * 128 + chunk * 16 + (col & 7) * 2) = p;
        }
  __syncthreads();
  // each wave stores its own 128 x 64 block: 8 rows x 128 B per instruction
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const int row = it * 8 + (lane >> 3), c = lane & 7;
    const int m = m0 + wr * 128 + row;
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(img + row * 128 + ((c ^ (row & 7)) * 16));
    if (m < M) *reinterpret_cast<u32x4_t*>(C + (int64_t)m * ldc + n0 + wc * 64 + c * 8) = v;
  }
}

// ---------------------------------------------------------------------------
// Variant 3 ("PGR2"): 4 waves (one per SIMD), each 128 x 128 of C (8 x 8 tiles
// of mfma_f32_16x16x32_bf16: 256 accumulator registers, AGPR-resident), the
// form hipBLASLt's fastest MT256x256x64 kernels take. With one wave per SIMD
// the wave itself must keep its matrix pipe fed, so each 64-deep K-step's
// fragments (both 32-deep halves, 32 ds_read_b128 = 128 VGPR) are read into
// registers BEFORE its LDS buffer is refilled, interleaved with the MFMAs. With the
// whole step register-resident, two 64 KB LDS buffers carry a global prefetch
// two K-steps deep (step kt+2 streams into the buffer step kt was read from),
// so every LDS-DMA piece has ~1.5 K-steps (~3000 cycles) to land.
//
// Per K-step kt (buffer b = kt & 1), 128 MFMA in two halves of 64:
//   half 0 (set 0, k 0..31): MFMA 0-15 each followed by one ds_read of set 1
//     (k 32..63 of step kt, W fragments first); at MFMA 40 lgkmcnt(0) +
//     barrier (every wave has read ALL of buffer b); MFMA 41-63 carry the 8
//     A-tile LDS-DMA pieces of step kt+2 into buffer b, one per 3 MFMA;
//   half 1 (set 1): MFMA 0-35 carry the 8 W-tile pieces (one per 5 MFMA); at
//     MFMA 36 vmcnt(16) (step kt+1's pieces, issued one K-step ago, landed;
//     this step's 16 stay in flight) + barrier; MFMA 37-52 each followed by one
//     ds_read of step kt+1's set 0 from buffer b ^ 1 (11 MFMA of slack before
//     the next step's first MFMA needs them).
// LDS-DMA through buffer_load_dwordx4 ... lds: one scalar buffer descriptor per
// operand, a 32-bit per-lane offset fixed for the whole loop, the K offset in
// soffset and the LDS base in m0 - a handful of scalar instructions per piece,
// no per-piece 64-bit address math, no branch (the step index is clamped; the
// two surplus steps at the end reload the last tile into a buffer nobody reads).
// LDS image per operand: [256 rows][64 k] bf16, each 1 KB DMA piece = 8 rows;
// 16-B chunk c of row r sits at slot c ^ ((r >> 1) & 7) (source-side swizzle,
// conflict-free for the 16 x 16 x 32 operand reads).
constexpr int NT6 = 256;
constexpr int OPB6 = BM * BK * 2;  // 32 KB per operand per K-step
constexpr int BUF6 = 2 * OPB6;     // 64 KB

// The 64 accumulators (256 registers) fill the accumulator file exactly; through the
// builtin, hipcc's register allocator re-homes loop-carried accumulators every
// iteration (~100-450 v_accvgpr moves per 64 MFMAs, with MFMA-result read stalls).
// As an asm statement with the accumulator TIED in an AGPR ("+a") every tile stays
// in place (0 moves). Hazards the compiler cannot see: an MFMA result read by a
// non-MFMA instruction needs 12 wait states (8-pass XDL) -> mfma_drain() before the
// epilogue; the A/B operands come straight from ds_read (lgkmcnt-ordered by hipcc,
// which tracks the asm's "v" inputs), never from a VALU write in the 2 states before.
__device__ __forceinline__ void mfma16_acc(f32x4_t& acc, const s16x8_t& a, const s16x8_t& b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma_drain() { asm volatile("s_nop 7\n\ts_nop 7" ::: "memory"); }

// Same launch forms as pgemm_kernel (tile0 / nsplit / ws).
template <int EPI>
__global__ __launch_bounds__(NT6, 1) void pgemm6_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                        const uint16_t* __restrict__ W, int64_t ldw,
                                                        uint16_t* __restrict__ C, int64_t ldc, int M, int N, int K,
                                                        int tile0, int nsplit, float* __restrict__ ws) {
  // half-1 MFMA index of the first fragment read of the next step (its barrier one before)
  constexpr int RB = 37;
  __shared__ __attribute__((aligned(1024))) char lds[2 * BUF6];  // the ONLY LDS object
  const int tiles_m = (M + BM - 1) / BM, tiles_n = N / BN;
  const int b = xcd_remap(blockIdx.x, gridDim.x);
  const int tail = gridDim.x / nsplit;
  const int t_local = b % tail, split = b / tail;
  const int nk_all = K / BK;
  const int chunk = (nk_all + nsplit - 1) / nsplit;
  const int kbeg = split * chunk;
  const int nk = min(chunk, nk_all - kbeg);
  int tm, tn;
  tile_mn(tile0 + t_local, tiles_m, tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: LDS bases stay scalar
  const int wr = w >> 1, wc = w & 1;

  // buffer descriptors over the K-range of this split (byte offsets must fit 31 bits: host-checked)
  const __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc((void*)(A + (int64_t)kbeg * BK), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc((void*)(W + (int64_t)kbeg * BK), 0, 0x7fffffff, 0x00020000);
  // DMA piece j of this wave: rows 64 w + 8 j + (lane >> 3), LDS slot lane & 7 <- chunk (lane & 7) ^ f(row)
  uint32_t va[8], vw[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = 64 * w + 8 * j + (lane >> 3);
    const int c = (lane & 7) ^ ((row >> 1) & 7);
    va[j] = m0 + row < M ? (uint32_t)(((m0 + row) * lda + c * 8) * 2) : 0x80000000u;  // past M: OOB zeros
    const int wrow = EPI == EPI_SILU_STD ? (row < 128 ? 0 : N / 2 - 128) + tn * 128 + row : n0 + row;
    vw[j] = (uint32_t)((wrow * ldw + c * 8) * 2);
  }
  auto dma = [&](int kt, int j, bool wop) {  // piece j of operand A (wop = false) or W, K-step kt
    const uint32_t so = (uint32_t)(min(kt, nk - 1) * BK * 2);
    char* dst = lds + (kt & 1) * BUF6 + (wop ? OPB6 : 0) + (8 * w + j) * 1024;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(wop ? rw : ra, (__attribute__((address_space(3))) void*)dst, 16,
                                             wop ? vw[j] : va[j], so, 0, 0);
  };

  // fragment reads: row 16 t + (lane & 15), chunk 4 h + (lane >> 4) at slot chunk ^ ((lane >> 1) & 7)
  const int fr = lane & 15, fq = lane >> 4;
  const int rd0 = fr * 128 + ((fq ^ ((fr >> 1) & 7)) * 16);
  const int rd1 = fr * 128 + (((4 + fq) ^ ((fr >> 1) & 7)) * 16);
  const int a_rd = (wr * 128) * 128, w_rd = OPB6 + (wc * 128) * 128;

  f32x4_t acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  s16x8_t fa0[8], fw0[8], fa1[8], fw1[8];

  // prologue: steps 0 and 1 in flight, step 0 landed, its set 0 in registers
#pragma unroll
  for (int j = 0; j < 8; ++j) dma(0, j, false);
#pragma unroll
  for (int j = 0; j < 8; ++j) dma(0, j, true);
#pragma unroll
  for (int j = 0; j < 8; ++j) dma(1, j, false);
#pragma unroll
  for (int j = 0; j < 8; ++j) dma(1, j, true);
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  bar();
  // read order of a set (everywhere): A row 0, the 8 W fragments, A rows 1..7 - MFMA (0, j) then
  // needs only the first j + 2 reads, so the waits before the first MFMA row are progressive
  fa0[0] = *reinterpret_cast<const s16x8_t*>(lds + a_rd + rd0);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    fw0[i] = *reinterpret_cast<const s16x8_t*>(lds + w_rd + i * 2048 + rd0);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = 1; i < 8; ++i) {
    fa0[i] = *reinterpret_cast<const s16x8_t*>(lds + a_rd + i * 2048 + rd0);
    __builtin_amdgcn_sched_barrier(0);
  }
  // nothing pending on the loop's entry edge: hipcc's waitcnt pass then keeps the counted
  // waits of the back edge at the loop head instead of merging to lgkmcnt(0) every K-step
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 4" ::: "memory");  // v_accvgpr_write (zero init) -> MFMA srcC
  __builtin_amdgcn_sched_barrier(0);

  for (int kt = 0; kt < nk; ++kt) {
    const char* cur = lds + (kt & 1) * BUF6;
    const char* nxt = lds + ((kt & 1) ^ 1) * BUF6;
    // ---- half 0: set 0; reads of set 1; barrier; A pieces of step kt + 2
#pragma unroll
    for (int t = 0; t < 64; ++t) {
      const int i = t >> 3, j = t & 7;
      // explicit progressive waits for set 0 (hipcc's own pass waits lgkmcnt(0) at the loop head):
      // MFMA (0, j) needs the first j + 2 of set 0's 16 reads, (i, 0) the first i + 9; the set-1
      // reads issued after MFMA 0 .. t - 1 are younger still
      // (row 1: 7 - 1 + 8 = 14; from row 2 on at least 15 younger reads, nothing to wait for)
      if (t <= 8) __builtin_amdgcn_s_waitcnt(0xC07F | (14 << 8));
      mfma16_acc(acc[i][j], fw0[j], fa0[i]);
      if (t == 0) {
        fa1[0] = *reinterpret_cast<const s16x8_t*>(cur + a_rd + rd1);
      } else if (t < 9) {
        fw1[t - 1] = *reinterpret_cast<const s16x8_t*>(cur + w_rd + (t - 1) * 2048 + rd1);
      } else if (t < 16) {
        fa1[t - 8] = *reinterpret_cast<const s16x8_t*>(cur + a_rd + (t - 8) * 2048 + rd1);
      } else if (t == 40) {
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's reads of buffer b retired
        bar();
      } else if (t > 40 && (t - 41) % 3 == 0) {
        dma(kt + 2, (t - 41) / 3, false);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- half 1: set 1; W pieces of step kt + 2; wait step kt + 1; reads of its set 0
#pragma unroll
    for (int t = 0; t < 64; ++t) {
      const int i = t >> 3, j = t & 7;
      mfma16_acc(acc[i][j], fw1[j], fa1[i]);
      if (t < 36 && t % 5 == 0) {
        dma(kt + 2, t / 5, true);
      } else if (t == RB - 1) {
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");  // step kt+1 landed (this step's 16 in flight)
        bar();
      } else if (t == RB) {
        fa0[0] = *reinterpret_cast<const s16x8_t*>(nxt + a_rd + rd0);
      } else if (t > RB && t < RB + 9) {
        fw0[t - RB - 1] = *reinterpret_cast<const s16x8_t*>(nxt + w_rd + (t - RB - 1) * 2048 + rd0);
      } else if (t >= RB + 9 && t < RB + 16) {
        fa0[t - RB - 8] = *reinterpret_cast<const s16x8_t*>(nxt + a_rd + (t - RB - 8) * 2048 + rd0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  mfma_drain();
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if constexpr (EPI == EPI_F32) {
    float* wt = ws + ((int64_t)split * tail + t_local) * (BM * BN);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = wr * 128 + 16 * i + fr, col = wc * 128 + 16 * j + 4 * fq;
        *reinterpret_cast<f32x4_t*>(wt + row * BN + col) = acc[i][j];
      }
    return;
  }
  __syncthreads();
  // epilogue: acc[i][j][r] = C[m][n], m = wr*128 + 16 i + (lane & 15), n = wc*128 + 16 j + 4 (lane >> 4) + r.
  // wave image: [128 rows][128 cols] bf16 (256-B rows), 16-B chunks XOR-swizzled by row & 15
  char* img = lds + w * 32768;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = 16 * i + fr, col = 16 * j + 4 * fq;
      const f32x4_t v = acc[i][j];
      u32x2_t p;
      p[0] = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
      p[1] = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
      *reinterpret_cast<u32x2_t*>(img + row * 256 + (((col >> 3) ^ (row & 15)) * 16) + (col & 7) * 2) = p;
    }
  __syncthreads();
  if constexpr (EPI == EPI_NONE) {
#pragma unroll 4
    for (int it = 0; it < 32; ++it) {
      const int row = it * 4 + (lane >> 4), c = lane & 15;
      const int m = m0 + wr * 128 + row;
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(img + row * 256 + ((c ^ (row & 15)) * 16));
      if (m < M) *reinterpret_cast<u32x4_t*>(C + (int64_t)m * ldc + n0 + wc * 128 + c * 8) = v;
    }
  } else {
    // EPI_SILU_STD: gate = tile columns [0, 128) (waves wc = 0), up = [128, 256) (wc = 1): both
    // waves of a row half store 64 rows each of silu(g) * u
    const char* gimg = lds + (wr * 2) * 32768;
    const char* uimg = gimg + 32768;
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int row = wc * 64 + it * 4 + (lane >> 4), c = lane & 15;
      const int m = m0 + wr * 128 + row;
      const int off = row * 256 + ((c ^ (row & 15)) * 16);
      float gf[8], uf[8], of[8];
      unpack8(*reinterpret_cast<const u32x4_t*>(gimg + off), gf);
      unpack8(*reinterpret_cast<const u32x4_t*>(uimg + off), uf);
#pragma unroll
      for (int e = 0; e < 8; ++e) of[e] = gf[e] / (1.f + __expf(-gf[e])) * uf[e];
      if (m < M) *reinterpret_cast<u32x4_t*>(C + (int64_t)m * ldc + n0 / 2 + c * 8) = pack8(of);
    }
  }
}

// ---------------------------------------------------------------------------
// Variant 6 ("persistent PGR2"): variant 3's K-loop, but each workgroup walks a
// list of tiles (tile b, b + P, b + 2P, ... of the data-parallel range; P = min(#tiles,
// 256) workgroups) as ONE continuous stream of K-steps: the LDS-DMA of step g + 2
// and the fragment reads of step g + 1 run straight across tile boundaries, so the
// next tile's first two K-steps load while the current tile finishes - no per-tile
// prologue wait (an HBM round trip, ~2-4 % of a 128-step tile). The epilogue stores
// straight from the accumulators (no LDS: both LDS buffers hold the next tile then):
// each lane owns 4 consecutive columns of a row, 8-B stores. EPI_SILU_STD maps
// each wave to 64 gate + the matching 64 up columns (W fragments 0-3 from gate rows,
// 4-7 from up rows), so silu(g) * u is formed in registers.
template <int EPI>
__global__ __launch_bounds__(NT6, 1) void pgemm7_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                        const uint16_t* __restrict__ W, int64_t ldw,
                                                        uint16_t* __restrict__ C, int64_t ldc, int M, int N, int K,
                                                        int ntiles) {
  constexpr int RB = 37;
  __shared__ __attribute__((aligned(1024))) char lds[2 * BUF6];  // the ONLY LDS object
  const int tiles_m = (M + BM - 1) / BM, tiles_n = N / BN;
  const int P = gridDim.x;
  const int b = xcd_remap(blockIdx.x, P);
  const int nt = (ntiles - b + P - 1) / P;  // tiles of this workgroup: b, b + P, ...
  const int nk = K / BK;
  const int S = nt * nk;                    // K-steps of this workgroup, all tiles

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1;
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, 0x7fffffff, 0x00020000);

  // per-lane DMA offsets of the tile being LOADED (advances two K-steps ahead of compute)
  uint32_t va[8], vw[8];
  auto set_dma_tile = [&](int r) {
    int tm, tn;
    tile_mn(b + min(r, nt - 1) * P, tiles_m, tiles_n, tm, tn);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = 64 * w + 8 * j + (lane >> 3);
      const int c = (lane & 7) ^ ((row >> 1) & 7);
      va[j] = tm * BM + row < M ? (uint32_t)(((tm * BM + row) * lda + c * 8) * 2) : 0x80000000u;
      const int wrow = EPI == EPI_SILU_STD ? (row < 128 ? 0 : N / 2 - 128) + tn * 128 + row : tn * BN + row;
      vw[j] = (uint32_t)((wrow * ldw + c * 8) * 2);
    }
  };
  // piece j of operand A or W of global K-step g, whose step within its tile is kt_of_g (the
  // offsets of that tile are set by set_dma_tile)
  auto dma = [&](int g, int kt_of_g, int j, bool wop) {
    const uint32_t so = (uint32_t)(kt_of_g * BK * 2);
    char* dst = lds + (g & 1) * BUF6 + (wop ? OPB6 : 0) + (8 * w + j) * 1024;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(wop ? rw : ra, (__attribute__((address_space(3))) void*)dst, 16,
                                             wop ? vw[j] : va[j], so, 0, 0);
  };

  const int fr = lane & 15, fq = lane >> 4;
  const int rd0 = fr * 128 + ((fq ^ ((fr >> 1) & 7)) * 16);
  const int rd1 = fr * 128 + (((4 + fq) ^ ((fr >> 1) & 7)) * 16);
  const int a_rd = (wr * 128) * 128;
  // W fragment j of this wave: rows wc*128 + 16 j (EPI_NONE); gate rows wc*64 + 16 j (j < 4) and
  // up rows 128 + wc*64 + 16 (j - 4) (EPI_SILU_STD)
  auto w_off = [&](int j) {
    return OPB6 + (EPI == EPI_SILU_STD ? (j < 4 ? wc * 64 + 16 * j : 128 + wc * 64 + 16 * (j - 4))
                                       : wc * 128 + 16 * j) * 128;
  };

  f32x4_t acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  s16x8_t fa0[8], fw0[8], fa1[8], fw1[8];

  set_dma_tile(0);
#pragma unroll
  for (int j = 0; j < 8; ++j) dma(0, 0, j, false);
#pragma unroll
  for (int j = 0; j < 8; ++j) dma(0, 0, j, true);
  if (nk == 1) set_dma_tile(1);
  const int kt1 = nk == 1 ? 0 : 1;
#pragma unroll
  for (int j = 0; j < 8; ++j) dma(1, kt1, j, false);
#pragma unroll
  for (int j = 0; j < 8; ++j) dma(1, kt1, j, true);
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  bar();
  fa0[0] = *reinterpret_cast<const s16x8_t*>(lds + a_rd + rd0);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    fw0[i] = *reinterpret_cast<const s16x8_t*>(lds + w_off(i) + rd0);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = 1; i < 8; ++i) {
    fa0[i] = *reinterpret_cast<const s16x8_t*>(lds + a_rd + i * 2048 + rd0);
    __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 4" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);

  for (int r = 0; r < nt; ++r) {
  for (int kt = 0; kt < nk; ++kt) {
    const int g = r * nk + kt;
    const char* cur = lds + (g & 1) * BUF6;
    const char* nxt = lds + ((g & 1) ^ 1) * BUF6;
    // the DMA of this step loads global step g + 2 = step kt2 of tile r2 (scalar bookkeeping, no
    // division); past the last step it re-loads the last one into a buffer nobody reads
    int kt2 = kt + 2;
    if (nk == 1) {
      kt2 = 0;
      set_dma_tile(r + 2);
    } else if (kt2 >= nk) {
      kt2 -= nk;
      if (kt2 == 0) set_dma_tile(r + 1);
    }
    if (g + 2 >= S) kt2 = nk - 1;
#pragma unroll
    for (int t = 0; t < 64; ++t) {
      const int i = t >> 3, j = t & 7;
      if (t <= 8) __builtin_amdgcn_s_waitcnt(0xC07F | (14 << 8));
      mfma16_acc(acc[i][j], fw0[j], fa0[i]);
      if (t == 0) {
        fa1[0] = *reinterpret_cast<const s16x8_t*>(cur + a_rd + rd1);
      } else if (t < 9) {
        fw1[t - 1] = *reinterpret_cast<const s16x8_t*>(cur + w_off(t - 1) + rd1);
      } else if (t < 16) {
        fa1[t - 8] = *reinterpret_cast<const s16x8_t*>(cur + a_rd + (t - 8) * 2048 + rd1);
      } else if (t == 40) {
        __builtin_amdgcn_s_waitcnt(0xC07F);
        bar();
      } else if (t > 40 && (t - 41) % 3 == 0) {
        dma(g + 2, kt2, (t - 41) / 3, false);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < 64; ++t) {
      const int i = t >> 3, j = t & 7;
      mfma16_acc(acc[i][j], fw1[j], fa1[i]);
      if (t < 36 && t % 5 == 0) {
        dma(g + 2, kt2, t / 5, true);
      } else if (t == RB - 1) {
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        bar();
      } else if (t == RB) {
        fa0[0] = *reinterpret_cast<const s16x8_t*>(nxt + a_rd + rd0);
      } else if (t > RB && t < RB + 9) {
        fw0[t - RB - 1] = *reinterpret_cast<const s16x8_t*>(nxt + w_off(t - RB - 1) + rd0);
      } else if (t >= RB + 9 && t < RB + 16) {
        fa0[t - RB - 8] = *reinterpret_cast<const s16x8_t*>(nxt + a_rd + (t - RB - 8) * 2048 + rd0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
    {
      // tile r done: store it straight from the accumulators, then restart them
      int tm, tn;
      tile_mn(b + r * P, tiles_m, tiles_n, tm, tn);
      mfma_drain();
      __builtin_amdgcn_sched_barrier(0);
      const int mrow = tm * BM + wr * 128 + fr;
      if constexpr (EPI == EPI_NONE) {
        uint16_t* cb = C + (int64_t)tn * BN + wc * 128 + 4 * fq;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int m = mrow + 16 * i;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const f32x4_t v = acc[i][j];
            u32x2_t p;
            p[0] = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
            p[1] = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
            if (m < M) *reinterpret_cast<u32x2_t*>(cb + (int64_t)m * ldc + 16 * j) = p;
          }
        }
      } else {
        uint16_t* cb = C + (int64_t)tn * 128 + wc * 64 + 4 * fq;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int m = mrow + 16 * i;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f32x4_t gv = acc[i][j], uv = acc[i][j + 4];
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = gv[e] / (1.f + __expf(-gv[e])) * uv[e];
            u32x2_t p;
            p[0] = (uint32_t)f2bf(o[0]) | ((uint32_t)f2bf(o[1]) << 16);
            p[1] = (uint32_t)f2bf(o[2]) | ((uint32_t)f2bf(o[3]) << 16);
            if (m < M) *reinterpret_cast<u32x2_t*>(cb + (int64_t)m * ldc + 16 * j) = p;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_nop 4" ::: "memory");  // v_accvgpr_write -> MFMA srcC
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

// ws [nsplit][tail][256][256] fp32 partials -> C tiles tile0 .. tile0 + tail - 1 (bf16, rows < M)
__global__ __launch_bounds__(256) void pgemm_splitk_reduce(const float* __restrict__ ws, int nsplit, int tail,
                                                           int tile0, uint16_t* __restrict__ C, int64_t ldc, int M,
                                                           int N) {
  const int t = blockIdx.x / (BM / 8), rblk = blockIdx.x % (BM / 8);  // 8 rows per block
  int tm, tn;
  tile_mn(tile0 + t, (M + BM - 1) / BM, N / BN, tm, tn);
  const int row = rblk * 8 + (threadIdx.x >> 5), col = (threadIdx.x & 31) * 8;
  const int m = tm * BM + row;
  if (m >= M) return;
  float f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int s = 0; s < nsplit; ++s) {
    const float* p = ws + ((int64_t)s * tail + t) * (BM * BN) + row * BN + col;
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p), b = *reinterpret_cast<const f32x4_t*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f[e] += a[e];
      f[4 + e] += b[e];
    }
  }
  *reinterpret_cast<u32x4_t*>(C + (int64_t)m * ldc + tn * BN + col) = pack8(f);
}

constexpr int PG_CUS = 256;  // MI355X compute units: one 256 x 256 tile per CU per wave

// tail split plan (every variant): (tiles run data-parallel, tail tiles, splits) or splits 1;
// only the plain epilogue splits
__host__ inline void pgemm_plan(int M, int N, int K, int epi, int& full, int& tail, int& nsplit) {
  const int ntiles = ((M + BM - 1) / BM) * (N / BN), nk = K / BK;
  full = ntiles;
  tail = 0;
  nsplit = 1;
  const int t = ntiles % PG_CUS;
  // a last wave at most half full, and K long enough that a quarter of it still pipelines
  if (epi != EPI_NONE || t == 0 || 2 * t > PG_CUS || nk < 32) return;
  int s = PG_CUS / t;
  s = std::min(s, nk / 8);
  if (s < 2) return;
  full = ntiles - t;
  tail = t;
  nsplit = s;
}

// one tile (nsplit == 1) or one K-range of a tail tile per workgroup: (..., tile0, nsplit, ws)
using TileKernel = void (*)(const uint16_t*, int64_t, const uint16_t*, int64_t, uint16_t*, int64_t, int, int, int, int,
                            int, float*);
// min(tiles, CUs) workgroups walking all `ntiles`: (..., ntiles)
using PersistentKernel = void (*)(const uint16_t*, int64_t, const uint16_t*, int64_t, uint16_t*, int64_t, int, int,
                                  int, int);

// The kernels of one variant. Per epilogue the data-parallel kernel is tiled or persistent
// (both null: the variant does not have that epilogue); the split-K tail is always tiled.
struct PgemmKernels {
  int threads;        // block size of every kernel of the set
  bool byte_offsets;  // buffer-descriptor DMA: operand offsets are 31-bit BYTE offsets
  TileKernel none, silu;
  PersistentKernel persistent_none, persistent_silu;
  TileKernel f32;
};

const PgemmKernels* pgemm_kernels(int variant) {
  static const PgemmKernels v0 = {NT, false, pgemm_kernel<EPI_NONE>, nullptr, nullptr, nullptr, pgemm_kernel<EPI_F32>};
  static const PgemmKernels v3 = {
      NT6, true, pgemm6_kernel<EPI_NONE>, pgemm6_kernel<EPI_SILU_STD>, nullptr, nullptr, pgemm6_kernel<EPI_F32>};
  static const PgemmKernels v6 = {
      NT6, true, nullptr, nullptr, pgemm7_kernel<EPI_NONE>, pgemm7_kernel<EPI_SILU_STD>, pgemm6_kernel<EPI_F32>};
  return variant == 0 ? &v0 : variant == 3 ? &v3 : variant == 6 ? &v6 : nullptr;
}

}  // namespace

extern "C" int64_t llmd_pgemm_ws_bytes(int M, int N, int K, int epi) {
  if (M <= 0 || N % BN || K % BK) return 0;
  int full, tail, nsplit;
  pgemm_plan(M, N, K, epi, full, tail, nsplit);
  return nsplit > 1 ? (int64_t)nsplit * tail * BM * BN * 4 : 0;
}

// variant 0: 8-wave staggered 4-phase kernel; 3: PGR2; 6: persistent PGR2. epi: EPI_NONE, or
// EPI_SILU_STD on variants 3 and 6; anything else returns -3 before any launch. With ws given
// (llmd_pgemm_ws_bytes) a last wave of tiles at most half full runs split over K: see pgemm_plan.
extern "C" int llmd_pgemm(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int M, int N,
                          int K, int epi, int variant, void* ws, hipStream_t st) {
  if (M <= 0) return 0;
  if (N % BN || K % BK || lda % 8 || ldw % 8 || ldc % 8) return -1;
  const PgemmKernels* ks = pgemm_kernels(variant);
  if (ks == nullptr || (epi != EPI_NONE && epi != EPI_SILU_STD)) return -3;
  const TileKernel tiled = epi == EPI_NONE ? ks->none : ks->silu;
  const PersistentKernel persistent = epi == EPI_NONE ? ks->persistent_none : ks->persistent_silu;
  if (tiled == nullptr && persistent == nullptr) return -3;
  // 32-bit element offsets of the DMA sources; 31-bit byte offsets of the buffer descriptors
  const int64_t amax = (int64_t)(M - 1) * lda + K, wmax = (int64_t)(N - 1) * ldw + K;
  if (amax > 0x7fffffffLL || wmax > 0x7fffffffLL) return -2;
  if (ks->byte_offsets && (amax * 2 > 0x7fffffffLL || wmax * 2 > 0x7fffffffLL)) return -2;

  int full = ((M + BM - 1) / BM) * (N / BN), tail = 0, nsplit = 1;
  if (ws != nullptr) pgemm_plan(M, N, K, epi, full, tail, nsplit);  // EPI_SILU_STD: no split
  const auto* a = (const uint16_t*)A;
  const auto* w = (const uint16_t*)W;
  auto* c = (uint16_t*)C;
  if (full > 0 && tiled != nullptr)
    hipLaunchKernelGGL(tiled, dim3(full), dim3(ks->threads), 0, st, a, lda, w, ldw, c, ldc, M, N, K, 0, 1, nullptr);
  else if (full > 0)
    hipLaunchKernelGGL(persistent, dim3(std::min(full, PG_CUS)), dim3(ks->threads), 0, st, a, lda, w, ldw, c, ldc, M,
                       N, K, full);
  if (nsplit > 1) {
    hipLaunchKernelGGL(ks->f32, dim3(tail * nsplit), dim3(ks->threads), 0, st, a, lda, w, ldw, c, ldc, M, N, K, full,
                       nsplit, (float*)ws);
    hipLaunchKernelGGL(pgemm_splitk_reduce, dim3(tail * (BM / 8)), dim3(256), 0, st, (const float*)ws, nsplit, tail,
                       full, c, ldc, M, N);
  }
  return (int)hipGetLastError();
}
