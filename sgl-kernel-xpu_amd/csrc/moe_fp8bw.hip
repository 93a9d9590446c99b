// fp8_blockwise_scaled_grouped_mm for gfx950: the block-scaled fp8 GEMM of gemm_8bit.hip over the ragged expert row
// lists of an MoE layer (DeepSeek-V3 / R1 and Qwen3-MoE fp8 checkpoints: e4m3 experts, 1 x 128 activation scales,
// 128 x 128 weight scales). The reference only declares the op (include/sgl_kernel_ops.h:660-678, wrapper
// python/sgl_kernel/moe.py:236-275) and pins its meaning with tests/test_fp8_blockwise_moe.py; there is no reference
// kernel. For every expert e and its rows r in [expert_offsets[e], expert_offsets[e] + problem_sizes[e, 0]):
//   out[r, n] = T( sum_kb sa[r, kb] * sb[e, kb, n / 128] * sum_{k in kb} a[r, k] * b[e, k, n] )
// The fp32 partial of each 128-deep K block comes from the MX MFMA with unit hardware scales and is scaled and added
// on the VALU, as in the dense kernel; one rounding to T at the end.
//
// The row counts and starts are read on the device (find_moe_tile_at of moe_tiles.h): no host sync, no allocation, no
// atomics, a pure function of the inputs, capturable into a graph. The launch is one-dimensional and sized for the
// worst case, its unused indices lie at the end, the real ones are re-ordered per XCD (moe_tiles.h). Rows that belong
// to no expert are neither read into a result nor written.
//
// ONE kernel for every row count. Work unit = (128 rows of one expert, 256 columns), one workgroup per unit - not the
// dense kernel's persistent walk over a static tile list: with row lists known only on the device a workgroup cannot
// know its units without walking every expert in front of them, and the tiles of a short expert would pipeline into
// each other's zero rows. What is kept from the dense kernel (gemm_fp8bw_x32_phase) is its arithmetic: 8 waves as
// 2 (m) x 4 (n), wave tile 64 x 64 as 2 x 2 fragments of the 32 x 32 x 64 MX MFMA, two MFMAs per fragment and K block;
// the m-step is A1 B1 A2 B2 (A, B = the two n-fragments, 1, 2 = the K halves) and the 16 promotion FMAs of a partial
// are written behind the MFMA that follows it (the order is the source's; the compiler's scheduler places them, nothing
// is pinned in assembly); lane (i, h) supplies row i, chunks 4 h + {0, 1} then 4 h + {2, 3} of both operands; LDS rows
// are 128 B with chunk c of row r at c ^ ((r >> 1) & 7) (conflict-free for ds_read_b128); n-fragment row i is LDS row
// 16 (i >> 4) + 8 ((i >> 2) & 1) + 4 ((i >> 3) & 1) + (i & 3), so a lane owns runs of 8 output columns (16-byte
// stores). a rows, b^T rows and the row scales of a K block go global -> LDS by LDS-DMA through buffer resources in a
// THREE-stage ring (16 + 32 + 2 KiB a stage): block kb + 2 is requested behind the barrier of block kb, so a block's
// data has two blocks of MFMAs to land. The resources end at the expert's last row / the last weight row: rows past
// them read as zero, and a block never sees the next expert's rows. Stores are predicated on the row and the column.
// A wave whose 64 rows lie past the expert's last row (a one-row expert) skips its MFMAs and keeps the barriers and
// its share of the DMA.
//
// A second kernel for a few rows per expert - gemm_8bit_skinny_kernel's weight stream (16 weight rows per wave through
// a register ring of 8 K blocks, the v_mfma_scale_f32_16x16x128_f8f6f4 form, work unit = expert x 16 rows x 64 columns) -
// was built, passed the same tests and was measured against this one at the same points: it lost at
// every row count from 4 rows per expert up (172 against 162 us at 4 rows, 285 against 170 us at 32 rows, DeepSeek-V3
// gate/up, 32 experts) and by 2.9x on a skewed list, where an expert's row blocks re-stream its weights. With few rows
// this kernel IS a weight stream - 48 KiB of LDS-DMA in flight per workgroup and nothing but the DMA in the way - so
// the stream kernel and the host-side regime rule were dropped; there is no regime query in the C-ABI. No 64-row form
// either: remainder blocks cost their weight traffic, not their MFMAs.
#include "common.h"
#include "moe_tiles.h"

namespace sglk {
namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int BK = 128;

#define FP8BW_LDS(p) ((__attribute__((address_space(3))) void*)(p))

constexpr int TM = 128, TN = 256;
constexpr int kOffB = TM * BK, kOffS = kOffB + TN * BK, kStg = kOffS + 2048;  // a rows, b^T rows, row scales (8 x 256 B)
constexpr int kNst = 3;
static_assert(kNst * kStg <= 160 * 1024, "LDS");

// buffer resource (raw, 32-bit records) from a wave-uniform pointer and byte count
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, uint32_t nrec) {
  const uint64_t u = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)hi << 32) | lo), 0,
                                           (int)__builtin_amdgcn_readfirstlane(nrec), 0x00020000);
}

template <typename OutT>
__global__ __launch_bounds__(512) void moe_fp8bw_tile_kernel(
    OutT* __restrict__ out, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, const float* __restrict__ sa,
    const float* __restrict__ sb, const int32_t* __restrict__ counts, const int32_t* __restrict__ starts, int E,
    int total_m, int N, int K, int64_t lda, int64_t ldb, int64_t b_se, int64_t ldc, int64_t sa_sm, int64_t sa_sk,
    int64_t sb_se, int64_t sb_sk, int64_t sb_sn) {
  __shared__ __attribute__((aligned(1024))) char smem[kNst * kStg];
  const MoeTile t = find_moe_tile_at(counts, 3, starts, E, total_m, TM, (N + TN - 1) / TN);
  if (t.expert < 0) return;  // (workgroup-uniform)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int nkb = K / BK;
  const int rows_a = t.m_valid < TM ? t.m_valid : TM;
  const int n0 = t.col_block * TN;
  const int rows_b = (N - n0) < TN ? (N - n0) : TN;

  const uint8_t* pa = a + (int64_t)t.m0 * lda;
  const uint8_t* pb = b + (int64_t)t.expert * b_se + (int64_t)n0 * ldb;
  const float* ps = sa + (int64_t)t.m0 * sa_sm;
  const uint32_t nrec_a = (uint32_t)((int64_t)(rows_a - 1) * lda + K);
  const uint32_t nrec_b = (uint32_t)((int64_t)(rows_b - 1) * ldb + K);
  // (row scales: 128 rows = the pieces of waves 0 and 1; the other waves issue theirs out of range, into the stage's spare)
  const uint32_t nrec_s = wave < 2 ? (uint32_t)(((int64_t)(rows_a - 1) * sa_sm + (int64_t)(nkb - 1) * sa_sk + 1) * 4) : 0u;
  int nblk = (n0 + wn * 64) >> 7;
  nblk = nblk < N / 128 - 1 ? nblk : N / 128 - 1;
  const float* sbw = sb + (int64_t)t.expert * sb_se + (int64_t)nblk * sb_sn;

  // DMA piece p of a tile = its rows 8 p .. 8 p + 7 (1 KiB): lane -> row 8 p + lane / 8, source chunk (lane % 8) ^ key(row),
  // key = (row >> 1) & 7 = (4 (p & 1) + lane / 16) & 7; the destination is linear
  uint32_t voff_a[2], voff_b[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const uint32_t ch = (uint32_t)(((lane & 7) ^ ((par * 4 + (lane >> 4)) & 7)) << 4);
    voff_a[par] = (uint32_t)(lane >> 3) * (uint32_t)lda + ch;
    voff_b[par] = (uint32_t)(lane >> 3) * (uint32_t)ldb + ch;
  }
  const uint32_t voff_s = (uint32_t)tid * (uint32_t)sa_sm * 4u;
  // the 7 pieces of this wave for K block kb into stage s (a block past the last one: out of range, zeros, never read)
  auto dma_block = [&](int kb, int s) {
    const bool in = kb < nkb;
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(pa, in ? nrec_a : 0u), rb = make_rsrc(pb, in ? nrec_b : 0u),
                                 rs = make_rsrc(ps, in ? nrec_s : 0u);
    char* base = smem + s * kStg;
    const int kk = in ? kb : 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int piece = wave * 2 + q;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, FP8BW_LDS(base + piece * 1024), 16, voff_a[q], kk * BK + piece * 8 * (int)lda, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int piece = wave * 4 + q;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, FP8BW_LDS(base + kOffB + piece * 1024), 16, voff_b[q & 1],
                                               kk * BK + piece * 8 * (int)ldb, 0, 0);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, FP8BW_LDS(base + kOffS + wave * 256), 4, voff_s, kk * (int)sa_sk * 4, 0, 0);
  };

  // fragment addressing (byte offsets inside a stage)
  const uint32_t lds_base = (uint32_t)(uintptr_t)FP8BW_LDS(smem);
  const int li = lane & 31, lh = lane >> 5;
  const int brow = (li >> 4) * 16 + ((li >> 2) & 1) * 8 + ((li >> 3) & 1) * 4 + (li & 3);
  const int arow = wm * 64 + li, wrow = wn * 64 + brow;
  uint32_t fa[4], fb[4];  // chunk 4 h + q of the lane's a row / b^T row
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    fa[q] = (uint32_t)(arow * 128 + (((4 * lh + q) ^ ((arow >> 1) & 7)) << 4));
    fb[q] = (uint32_t)(kOffB + wrow * 128 + (((4 * lh + q) ^ ((wrow >> 1) & 7)) << 4));
  }
  const uint32_t fs = (uint32_t)(kOffS + arow * 4);
  const bool wave_live = wm * 64 < rows_a && n0 + wn * 64 < N;

#define FP8BW_RD16(dst, addr, imm) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(imm))
#define FP8BW_RD4(dst, addr, imm) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(imm))
#define FP8BW_FRAG(lo, hi) __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7)
#define FP8BW_MFMA(nf, mf, half, c)                                                                               \
  __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(FP8BW_FRAG(nq[nf][half][0], nq[nf][half][1]),                    \
                                                  FP8BW_FRAG(mq[mf][half][0], mq[mf][half][1]), c, 0, 0, 0, 127, 0, 127)

  v16f acc[2][2];  // [m-fragment][n-fragment]
  v16f zero16;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero16[r] = 0.f;
#pragma unroll
  for (int mf = 0; mf < 2; ++mf)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) acc[mf][nf] = zero16;

  dma_block(0, 0);
  dma_block(1, 1);
  int s = 0;
  for (int kb = 0; kb < nkb; ++kb) {
    // vmcnt retires in issue order: all but this wave's 7 pieces of block kb + 1 have landed - block kb is whole once every
    // wave is here; nobody reads stage (kb + 2) % 3 = the stage of block kb - 1 any more
    asm volatile("s_waitcnt vmcnt(7)\n\ts_barrier" ::: "memory");
    const int s2 = s == 0 ? 2 : s - 1;
    dma_block(kb + 2, s2);
    if (wave_live) {
      const float sbv = sbw[(int64_t)kb * sb_sk];
      const uint32_t sbase = lds_base + (uint32_t)(s * kStg);
      v4i nq[2][2][2], mq[2][2][2];  // [fragment][K half][chunk]
      float sar[2];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        FP8BW_RD16(nq[0][half][0], sbase + fb[2 * half], 0);
        FP8BW_RD16(nq[0][half][1], sbase + fb[2 * half + 1], 0);
        FP8BW_RD16(nq[1][half][0], sbase + fb[2 * half], 4096);
        FP8BW_RD16(nq[1][half][1], sbase + fb[2 * half + 1], 4096);
        FP8BW_RD16(mq[0][half][0], sbase + fa[2 * half], 0);
        FP8BW_RD16(mq[0][half][1], sbase + fa[2 * half + 1], 0);
      }
      FP8BW_RD4(sar[0], sbase + fs, 0);
      FP8BW_RD4(sar[1], sbase + fs, 128);
#pragma unroll
      for (int half = 0; half < 2; ++half) {  // the second m-fragment lands under the first m-step
        FP8BW_RD16(mq[1][half][0], sbase + fa[2 * half], 4096);
        FP8BW_RD16(mq[1][half][1], sbase + fa[2 * half + 1], 4096);
      }
      // the 14 reads + 2 scale reads in front of the last four have returned
      asm volatile("s_waitcnt lgkmcnt(4)"
                   : "+v"(nq[0][0][0]), "+v"(nq[0][0][1]), "+v"(nq[0][1][0]), "+v"(nq[0][1][1]), "+v"(nq[1][0][0]),
                     "+v"(nq[1][0][1]), "+v"(nq[1][1][0]), "+v"(nq[1][1][1]), "+v"(mq[0][0][0]), "+v"(mq[0][0][1]),
                     "+v"(mq[0][1][0]), "+v"(mq[0][1][1]), "+v"(sar[0]), "+v"(sar[1]));
      // m-step 0: A1 B1 A2 B2
      v16f c00 = FP8BW_MFMA(0, 0, 0, zero16);
      v16f c01 = FP8BW_MFMA(1, 0, 0, zero16);
      c00 = FP8BW_MFMA(0, 0, 1, c00);
      c01 = FP8BW_MFMA(1, 0, 1, c01);
      __builtin_amdgcn_sched_barrier(0);  // (or the scheduler sinks the four MFMAs behind the wait for the second m-fragment)
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(mq[1][0][0]), "+v"(mq[1][0][1]), "+v"(mq[1][1][0]), "+v"(mq[1][1][1]));
      // m-step 1, the promotion of step 0's partials behind its MFMAs
      const float sc0 = sar[0] * sbv, sc1 = sar[1] * sbv;
      v16f c10 = FP8BW_MFMA(0, 1, 0, zero16);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][0][r] = __builtin_fmaf(c00[r], sc0, acc[0][0][r]);
      v16f c11 = FP8BW_MFMA(1, 1, 0, zero16);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][1][r] = __builtin_fmaf(c01[r], sc0, acc[0][1][r]);
      c10 = FP8BW_MFMA(0, 1, 1, c10);
      c11 = FP8BW_MFMA(1, 1, 1, c11);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[1][0][r] = __builtin_fmaf(c10[r], sc1, acc[1][0][r]);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[1][1][r] = __builtin_fmaf(c11[r], sc1, acc[1][1][r]);
    }
    s = s == 2 ? 0 : s + 1;
  }
#undef FP8BW_MFMA
#undef FP8BW_FRAG
#undef FP8BW_RD4
#undef FP8BW_RD16
  // (the out-of-range pieces of blocks nkb, nkb + 1 still write their zeros: the LDS must stay this workgroup's until they have)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (!wave_live) return;

  // lane (i, h): row wm * 64 + 32 mf + i, columns wn * 64 + 32 nf + 16 hv + 8 h .. + 7 = registers 8 hv .. 8 hv + 7
  const bool vec = (ldc % 8 == 0) && ((uintptr_t)out % 16 == 0);
#pragma unroll
  for (int mf = 0; mf < 2; ++mf) {
    const int row = wm * 64 + mf * 32 + li;
    if (row >= rows_a) continue;
    OutT* orow = out + (int64_t)(t.m0 + row) * ldc + n0 + wn * 64 + lh * 8;
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int hv = 0; hv < 2; ++hv) {
        Vec<OutT, 8> v;
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = (OutT)acc[mf][nf][hv * 8 + c];
        OutT* p = orow + nf * 32 + hv * 16;
        if (vec) {
          store_vec<OutT, 8>(p, v);
        } else {
#pragma unroll
          for (int c = 0; c < 8; ++c) p[c] = v[c];
        }
      }
  }
}

template <typename OutT>
int launch(hipStream_t st, void* out, const void* a, const void* b, const float* sa, const float* sb, const int32_t* counts,
           const int32_t* starts, int64_t total_m, int E, int N, int K, int64_t lda, int64_t ldb, int64_t b_se, int64_t ldc,
           int64_t sa_sm, int64_t sa_sk, int64_t sb_se, int64_t sb_sk, int64_t sb_sn) {
  const int64_t grid = moe_tile_launch_size(total_m, E, TM, (N + TN - 1) / TN);
  moe_fp8bw_tile_kernel<OutT><<<(unsigned)grid, 512, 0, st>>>((OutT*)out, (const uint8_t*)a, (const uint8_t*)b, sa, sb, counts, starts,
                                                              E, (int)total_m, N, K, lda, ldb, b_se, ldc, sa_sm, sa_sk, sb_se, sb_sk,
                                                              sb_sn);
  return check_launch("fp8_blockwise_scaled_grouped_mm");
}

}  // namespace
}  // namespace sglk

extern "C" int sglk_moe_fp8_blockwise_grouped_mm(sglk_stream_t stream, void* out, const void* a, const void* b, const float* sa,
                                                 const float* sb, const int32_t* problem_sizes, const int32_t* expert_offsets,
                                                 int64_t total_m, int64_t n_experts, int64_t N, int64_t K, int64_t lda,
                                                 int64_t ldb, int64_t b_stride_e, int64_t ldc, int64_t sa_stride_m,
                                                 int64_t sa_stride_k, int64_t sb_stride_e, int64_t sb_stride_k,
                                                 int64_t sb_stride_n, int out_dtype) {
  using namespace sglk;
  const char* op = "fp8_blockwise_scaled_grouped_mm";
  SGLK_REQUIRE(total_m >= 0 && n_experts > 0 && N > 0 && K > 0, "%s: bad shape", op);
  if (K % 128 != 0) return fail(SGLK_EUNSUPPORTED, "%s: K = %lld must be a multiple of 128 (one scale per 128-deep block)", op, (long long)K);
  if (N % 128 != 0) return fail(SGLK_EUNSUPPORTED, "%s: N = %lld must be a multiple of 128 (one weight scale per 128 columns)", op, (long long)N);
  SGLK_REQUIRE(out_dtype == SGLK_BF16 || out_dtype == SGLK_F16, "%s: out must be bfloat16 or half", op);
  if (total_m == 0) return SGLK_OK;
  SGLK_REQUIRE(out && a && b && sa && sb && problem_sizes && expert_offsets, "%s: null pointer", op);
  SGLK_REQUIRE((uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0, "%s: a and b must be 16-byte aligned", op);
  SGLK_REQUIRE(lda >= K && ldb >= K && ldc >= N && lda % 16 == 0 && ldb % 16 == 0 && b_stride_e % 16 == 0 && b_stride_e >= 0,
               "%s: lda, ldb >= K and ldc >= N; lda, ldb and the expert stride of b must be multiples of 16", op);
  SGLK_REQUIRE(sa_stride_m >= 0 && sa_stride_k >= 0 && sb_stride_e >= 0 && sb_stride_k >= 0 && sb_stride_n >= 0,
               "%s: negative scale stride", op);
  // what the kernel's buffer resources address with 32-bit offsets: a from the first row of the call (the finder's row
  // numbers are ints), one row block of a, one column block of one expert's b, the scale column of a row block
  SGLK_REQUIRE(total_m < (1ll << 31) && n_experts < (1ll << 24) && N < (1ll << 31) && K < (1ll << 31) &&
                   total_m * lda < (1ll << 40) && 128 * lda + K < (1ll << 31) && 256 * ldb + K < (1ll << 31) &&
                   (128 * sa_stride_m + (K / 128) * sa_stride_k) * 4 < (1ll << 31),
               "%s: a row block of a, a column block of b or their scales do not fit a buffer resource's 2 GiB", op);
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == SGLK_BF16)
    return launch<bf16>(st, out, a, b, sa, sb, problem_sizes, expert_offsets, total_m, (int)n_experts, (int)N, (int)K, lda, ldb,
                        b_stride_e, ldc, sa_stride_m, sa_stride_k, sb_stride_e, sb_stride_k, sb_stride_n);
  return launch<f16>(st, out, a, b, sa, sb, problem_sizes, expert_offsets, total_m, (int)n_experts, (int)N, (int)K, lda, ldb,
                     b_stride_e, ldc, sa_stride_m, sa_stride_k, sb_stride_e, sb_stride_k, sb_stride_n);
}
