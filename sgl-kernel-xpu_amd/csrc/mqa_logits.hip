// fp8_mqa_logits / fp8_paged_mqa_logits for gfx950: the scores of the DeepSeek-V3.2 "lightning indexer" (the reference
// declares them in python/sgl_kernel/nsa.py:112-185 and fp8_paged_mqa_logits.py:82; it has a GEMM plus a reduction, no
// fused kernel):
//   logits[i, j] = k_scale[j] * sum_h weights[i, h] * relu(q[i, h, :] . k[j, :])   inside the query's key window, 0 outside
// q, k e4m3 with D = 128, H <= 64 index heads that share one key vector per token, signed fp32 weights, fp32 output.
//
// THE COMMON CORE. v_mfma_f32_32x32x64_f8f6f4, heads on the M side, keys on the N side: lane (n, h) = (lane % 32,
// lane / 32) supplies head 32 m + n of M-fragment m (A) and key n (B), bytes 32 (h + 2 kh) .. + 31 for K half kh - the
// natural order of the row, so a key row needs no shuffle on its way from memory. The 32 x 32 accumulator gives a lane,
// for ITS key, the heads 32 m + 8 (r / 4) + 4 h + r % 4, r = 0 .. 15: the head sum `p += w[r] * max(s[r], 0)` is
// in-lane against 16 weight registers per fragment, and the two lane halves are joined by one v_permlane32_swap. No
// score goes to LDS or memory; the partial sums stay fp32; scale and window mask once per output. Heads at or past H
// are loaded as zero rows with weight 0, and the second M-fragment is not compiled in for H <= 32 (NM = 1).
// 2 MFMAs (128 cycles) stand against 32 VALU operations (v_max + v_fma, 128 cycles) per fragment: the kernels run two
// (ragged) or three (paged) waves per SIMD so that one wave's head sum runs under another wave's MFMAs, and the source
// order puts a unit's head sum behind the next unit's MFMAs (the compiler's scheduler places them). Built with
// -fno-slp-vectorize: v_pk_fma_f32 beside MFMAs is slower than the two v_fma_f32 it replaces (build.py FILE_FLAGS).
//
// RAGGED (prefill). Workgroup = 16 queries x a chunk of 128-key tiles, 8 waves, 2 queries per wave STATIONARY in
// registers (64 VGPRs of A, 64 of weights); keys stream global -> LDS by LDS-DMA in a three-stage ring of 128-key
// tiles (16 KiB of keys + the tile's scales; moe_fp8bw.hip's layout: 128-byte rows, 16-byte chunk c of row r at
// c ^ ((r >> 1) & 7)). A 32-key B fragment read from LDS (4 ds_read_b128) is used against the wave's two queries, i.e.
// 4 stationary A fragments and 8 MFMAs. Queries, not keys, are stationary because a streamed query costs 8 KiB + 32
// weights per lane against 4 KiB per 32 keys: with keys stationary the LDS reads alone take as long as the MFMAs.
// The swap that joins the lane halves also sorts the two queries: lanes 0..31 end with query 0's 32 keys, lanes
// 32..63 with query 1's - one swap, one add and one store instruction (2 x 128 contiguous bytes) per fragment pair.
// Before any load the block reduces ks / ke over its queries: tiles outside the hull [min ks, max ke) are written as
// zeros and never loaded; a workgroup without visible tiles ends before it loads its queries; inside the hull a wave
// whose two queries do not see a tile skips its MFMAs. Every element of the chunk is written exactly once.
// All stores go through a buffer resource over the block's 16 rows and are predicated by an out-of-range offset, not
// by a branch: every wave issues exactly 4 stores and 3 DMA pieces per tile, which is what the hand-counted vmcnt in
// front of the barrier relies on (vector-memory operations retire in issue order).
//
// PAGED (decode). Workgroup = one sequence x a chunk of keys, 4 waves that take the chunk's 32-key fragments in turn.
// The query's A fragments and weights stay in registers; cache rows go global -> registers directly in B layout (lane
// (n, h) loads segments h and 2 + h of key n with 4-byte-aligned 16-byte loads; rows of D + 4 bytes are only 4-byte
// aligned) through a register ring of 3 fragments: 12 waves a CU x 2 fragments ahead x 4 KiB = 96 KiB in flight, well
// above the ~ 40 KiB that 8 TB/s / 256 CUs x 1.2 us asks for. The page is looked up per key (per lane) - any page size -
// with a shift where the page size is a power of two. Table entries are clamped to [0, num_pages - 1]; entries at or
// past ceil(seq_len / page_size) are never read; positions in [seq_len, max_seq_len) are written as zeros.
#include "common.h"

namespace sglk {
namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef int v4i_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

#define MQA_LDS(p) ((__attribute__((address_space(3))) void*)(p))
#define MQA_FRAG(lo, hi) __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7)
#define MQA_MFMA(a, b, c) __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127)

constexpr int D = 128;
constexpr int QB = 16, KT = 128;  // ragged: queries per workgroup (8 waves x 2), keys per ring stage
constexpr int kOffS = KT * D, kStg = kOffS + 2048, kNst = 3;  // a stage: key rows, then 8 x 256 B of scales (2 pieces live)
constexpr int PW = 4, PCH_MIN = PW * 32;  // paged: waves per workgroup, smallest key chunk

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, uint32_t nrec) {
  const uint64_t u = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)hi << 32) | lo), 0,
                                           (int)__builtin_amdgcn_readfirstlane(nrec), 0x00020000);
}

// One query's operands as lane (n, h) holds them: A fragments [m][K half] and the weights of the lane's 16 heads per fragment.
template <int NM>
struct Query {
  v8i a[NM][2];
  float w[NM][16];
  __device__ __forceinline__ void load(const uint8_t* q, const float* wt, int64_t qi, bool valid, int H, int n, int h) {
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const int head = 32 * m + n;
      const bool in = valid && head < H;
      const uint8_t* row = q + (qi * H + head) * D + 32 * h;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        v4i lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
        if (in) {
          lo = *(const v4i*)(row + 64 * kh);
          hi = *(const v4i*)(row + 64 * kh + 16);
        }
        a[m][kh] = MQA_FRAG(lo, hi);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int hd = 32 * m + 8 * (r >> 2) + 4 * h + (r & 3);
        w[m][r] = (valid && hd < H) ? wt[qi * H + hd] : 0.f;
      }
    }
  }
};

// sum over the lane's heads of fragment m of w * relu(s), on top of p
__device__ __forceinline__ float head_sum(const v16f& c, const float (&w)[16], float p) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    // relu on the bits: a float is negative exactly when its bits are a negative int. One v_max_i32; fmaxf would first
    // canonicalise the MFMA's result (a second v_max_f32 per score), and inline assembly gets no MFMA-hazard nops.
    const float x = c[r];
    const int t = __float_as_int(x);
    p = __builtin_fmaf(__int_as_float(t > 0 ? t : 0), w[r], p);
  }
  return p;
}

__device__ __forceinline__ v16f zero16() {
  v16f z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// ---- ragged ------------------------------------------------------------------------------------------------------

template <int NM>
__global__ __launch_bounds__(512) void mqa_ragged_kernel(float* __restrict__ out, const uint8_t* __restrict__ q,
                                                         const uint8_t* __restrict__ k, const float* __restrict__ k_scale,
                                                         const float* __restrict__ wt, const int32_t* __restrict__ ks,
                                                         const int32_t* __restrict__ ke, int Nq, int Nk, int H, int64_t ld,
                                                         int tiles_per_chunk) {
  __shared__ __attribute__((aligned(1024))) char smem[kNst * kStg];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = blockIdx.y * QB;
  const int ntiles = (Nk + KT - 1) / KT;
  const int t0 = blockIdx.x * tiles_per_chunk;
  const int t1 = t0 + tiles_per_chunk < ntiles ? t0 + tiles_per_chunk : ntiles;

  auto clampk = [&](int v) { return v < 0 ? 0 : (v > Nk ? Nk : v); };
  // the hull of the block's windows (workgroup-uniform), the windows of this wave's two queries, this lane's own
  int lo = Nk, hi = 0, ws[2] = {0, 0}, we[2] = {0, 0};
  for (int i = 0; i < QB; ++i) {
    if (q0 + i >= Nq) break;
    const int s = clampk(ks[q0 + i]), e = clampk(ke[q0 + i]);
    if (e > s) {
      lo = s < lo ? s : lo;
      hi = e > hi ? e : hi;
      if (i == 2 * wave) ws[0] = s, we[0] = e;
      if (i == 2 * wave + 1) ws[1] = s, we[1] = e;
    }
  }
  const int my_s = h ? ws[1] : ws[0], my_e = h ? we[1] : we[0];
  const int wlo = we[0] > ws[0] ? (we[1] > ws[1] ? (ws[0] < ws[1] ? ws[0] : ws[1]) : ws[0]) : ws[1];
  const int whi = we[0] > we[1] ? we[0] : we[1];  // (an empty window is (0, 0): whi <= wlo = nothing visible)
  int v0 = lo / KT > t0 ? lo / KT : t0;
  int v1 = (hi + KT - 1) / KT < t1 ? (hi + KT - 1) / KT : t1;
  if (v1 <= v0) v0 = v1 = t0;

  // stores: row 2 wave + h of the block, predicated by an offset outside the resource
  const int nrows = Nq - q0 < QB ? Nq - q0 : QB;
  const __amdgpu_buffer_rsrc_t rout = make_rsrc(out + (int64_t)q0 * ld, (uint32_t)(nrows * ld * 4));
  const bool row_ok = 2 * wave + h < nrows;
  const uint32_t row_off = (uint32_t)((2 * wave + h) * ld * 4);
  auto store = [&](int key, float v) {
    const uint32_t off = (row_ok && key < Nk) ? row_off + (uint32_t)key * 4u : 0x80000000u;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rout, off, 0, 0);  // (the builtin takes the 32 bits as unsigned)
  };
  // The tiles outside the hull: zeros. Where the rows are 16-byte aligned a wave fills its two rows one after the other, 1 KiB
  // of a row per store instruction (against 4-byte stores, 2 x 128 bytes an instruction: 889 instead of 937 us at 4096 x 32768
  // queries x keys under a causal window).
  const bool vec = (ld & 3) == 0 && (Nk & 3) == 0 && ((uintptr_t)out & 15) == 0;  // (n_k % 4: no store crosses n_k)
  auto zero_fill = [&](int k_lo, int k_hi) {  // k_lo is a multiple of KT
    k_hi = k_hi < Nk ? k_hi : Nk;
    if (!vec) {
      for (int key = k_lo + n; key < k_hi; key += 32) store(key, 0.f);
      return;
    }
    for (int r = 2 * wave; r < 2 * wave + 2; ++r) {
      const uint32_t roff = (uint32_t)(r * ld * 4);
      for (int key = k_lo + 4 * lane; key < k_hi; key += 256) {
        __builtin_amdgcn_raw_buffer_store_b128(v4u{0u, 0u, 0u, 0u}, rout, r < nrows ? roff + (uint32_t)key * 4u : 0x80000000u, 0, 0);
      }
    }
  };
  zero_fill(t0 * KT, v0 * KT);
  zero_fill(v1 * KT, t1 * KT);
  const int ntv = v1 - v0;
  if (ntv == 0) return;  // (workgroup-uniform)

  Query<NM> qa[2];
#pragma unroll
  for (int qq = 0; qq < 2; ++qq) qa[qq].load(q, wt, q0 + 2 * wave + qq, 2 * wave + qq < nrows, H, n, h);

  // DMA piece p of a tile = its rows 8 p .. 8 p + 7 (1 KiB): lane -> row 8 p + lane / 8, source chunk (lane % 8) ^ key(row),
  // key = (row >> 1) & 7 = (4 (p & 1) + lane / 16) & 7; the destination is linear. Wave w: pieces 2 w, 2 w + 1 and, for
  // w < 2, the scales of keys 64 w .. 64 w + 63 (the other waves issue theirs out of range, into the stage's spare).
  uint32_t voff[2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
    voff[par] = (uint32_t)(lane >> 3) * D + (uint32_t)(((lane & 7) ^ ((par * 4 + (lane >> 4)) & 7)) << 4);
  // (rows and scales past n_k - the last tile's, at n_k = 1 or 33 most of it - rely on the raw buffer's range check: voffset +
  // soffset at or past num_records reads as zero, also where soffset alone is past it; the same idiom as moe_fp8bw.hip)
  const uint32_t nrec_k = (uint32_t)Nk * D, nrec_s = wave < 2 ? (uint32_t)Nk * 4u : 0u;
  auto dma_tile = [&](int i, int s) {  // visible tile i of this block into stage s (past the last one: zeros, never read)
    const bool in = i < ntv;
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(k, in ? nrec_k : 0u), rs = make_rsrc(k_scale, in ? nrec_s : 0u);
    char* base = smem + s * kStg;
    const int key0 = in ? (v0 + i) * KT : 0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int piece = wave * 2 + p;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, MQA_LDS(base + piece * 1024), 16, voff[p], (key0 + piece * 8) * D, 0, 0);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, MQA_LDS(base + kOffS + wave * 256), 4, (uint32_t)lane * 4u,
                                             (key0 + (wave & 1) * 64) * 4, 0, 0);
  };

  const uint32_t lds_base = (uint32_t)(uintptr_t)MQA_LDS(smem);
  uint32_t fb[4];  // chunk 2 h + {0, 1} (K half 0), 4 + 2 h + {0, 1} (K half 1) of key row n; fragment f: + 4096 f
#pragma unroll
  for (int c = 0; c < 4; ++c) fb[c] = (uint32_t)(n * D + ((((c >> 1) * 4 + 2 * h + (c & 1)) ^ ((n >> 1) & 7)) << 4));
  const uint32_t fs = (uint32_t)(kOffS + n * 4);

#define MQA_RD16(dst, addr, imm) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(imm))
#define MQA_RD4(dst, addr, imm) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(imm))
#define MQA_READ_FRAG(buf, f)                          \
  MQA_RD16(bq[buf][0], sbase + fb[0], (f) * 4096);     \
  MQA_RD16(bq[buf][1], sbase + fb[1], (f) * 4096);     \
  MQA_RD16(bq[buf][2], sbase + fb[2], (f) * 4096);     \
  MQA_RD16(bq[buf][3], sbase + fb[3], (f) * 4096);     \
  MQA_RD4(bsc[buf], sbase + fs, (f) * 128)
#define MQA_WAIT(cnt, buf)                  \
  asm volatile("s_waitcnt lgkmcnt(" #cnt ")" \
               : "+v"(bq[buf][0]), "+v"(bq[buf][1]), "+v"(bq[buf][2]), "+v"(bq[buf][3]), "+v"(bsc[buf]))

  dma_tile(0, 0);
  dma_tile(1, 1);
  int s = 0;
  for (int i = 0; i < ntv; ++i) {
    // Vector-memory operations retire in issue order, and every wave issues exactly 3 DMA pieces and 4 stores per tile.
    // Behind this wave's pieces of tile i lie: the 4 stores of tile i - 2, the 3 pieces of tile i + 1, the 4 stores of
    // tile i - 1 (i = 0: only the pieces of tile 1; i = 1: the pieces of tile 2 and the stores of tile 0). Tile i is whole
    // once every wave is here, and nobody reads stage (i + 2) % 3 = the stage of tile i - 1 any more.
    if (i == 0) asm volatile("s_waitcnt vmcnt(3)\n\ts_barrier" ::: "memory");
    else if (i == 1) asm volatile("s_waitcnt vmcnt(7)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(11)\n\ts_barrier" ::: "memory");
    dma_tile(i + 2, s == 0 ? 2 : s - 1);
    const int key_t = (v0 + i) * KT;
    const bool live = wlo < key_t + KT && whi > key_t;  // (wave-uniform)
    if (live) {
      const uint32_t sbase = lds_base + (uint32_t)(s * kStg);
      v4i bq[2][4];
      float bsc[2];
      MQA_READ_FRAG(0, 0);
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int cur = f & 1;
        if (f == 0) { MQA_READ_FRAG(1, 1); MQA_WAIT(5, 0); }
        if (f == 1) { MQA_READ_FRAG(0, 2); MQA_WAIT(5, 1); }
        if (f == 2) { MQA_READ_FRAG(1, 3); MQA_WAIT(5, 0); }
        if (f == 3) { MQA_WAIT(0, 1); }
        const v8i b0 = MQA_FRAG(bq[cur][0], bq[cur][1]), b1 = MQA_FRAG(bq[cur][2], bq[cur][3]);
        // units (query, M-fragment); a unit's head sum behind the next unit's MFMAs
        float p[2] = {0.f, 0.f};
        v16f c = MQA_MFMA(qa[0].a[0][0], b0, zero16());
        c = MQA_MFMA(qa[0].a[0][1], b1, c);
#pragma unroll
        for (int u = 1; u < 2 * NM; ++u) {
          const int qq = u / NM, m = u % NM;
          v16f c2 = MQA_MFMA(qa[qq].a[m][0], b0, zero16());
          c2 = MQA_MFMA(qa[qq].a[m][1], b1, c2);
          p[(u - 1) / NM] = head_sum(c, qa[(u - 1) / NM].w[(u - 1) % NM], p[(u - 1) / NM]);
          c = c2;
        }
        p[1] = head_sum(c, qa[1].w[NM - 1], p[1]);
        // lanes 0..31 hold query 0's halves, lanes 32..63 query 1's: the swap hands each lane half its own query's other half
        float c0 = p[0], c1 = p[1];
        asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(c0), "+v"(c1));
        const int key = key_t + 32 * f + n;
        store(key, (key >= my_s && key < my_e) ? (c0 + c1) * bsc[cur] : 0.f);
      }
    } else {
#pragma unroll
      for (int f = 0; f < 4; ++f) store(key_t + 32 * f + n, 0.f);
    }
    s = s == 2 ? 0 : s + 1;
  }
#undef MQA_WAIT
#undef MQA_READ_FRAG
#undef MQA_RD4
#undef MQA_RD16
  // (the out-of-range pieces of tiles ntv, ntv + 1 still write their zeros: the LDS must stay this workgroup's until they have)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- paged -------------------------------------------------------------------------------------------------------

struct KeyFrag {  // 32 keys in B layout: this lane's segments h (d[0], d[1]) and 2 + h (d[2], d[3]) of key n, and the key's scale
  v4i d[4];
  float sc;
};

// (amdgpu_waves_per_eu(2): with at most 256 registers a wave the compiler keeps the MFMA results in VGPRs; with the
// 512 that 256 threads could have it puts them into AGPRs and pays a v_accvgpr_read per score)
template <int NM, bool BLOCK>
__global__ __launch_bounds__(PW * 64) __attribute__((amdgpu_waves_per_eu(2))) void mqa_paged_kernel(float* __restrict__ out, const uint8_t* __restrict__ q,
                                                            const uint8_t* __restrict__ cache, const float* __restrict__ wt,
                                                            const int32_t* __restrict__ seq_lens,
                                                            const int32_t* __restrict__ table, int H, int page_size,
                                                            int page_shift, int num_pages, int64_t table_stride,
                                                            int max_seq_len, int64_t ld, int chunk) {
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y;
  const int c0 = blockIdx.x * chunk;
  const int c1 = c0 + chunk < max_seq_len ? c0 + chunk : max_seq_len;
  int seq = seq_lens[b];
  seq = seq < 0 ? 0 : (seq > max_seq_len ? max_seq_len : seq);
  float* orow = out + (int64_t)b * ld;
  const int j_begin = c0 + 32 * wave;           // this wave's fragments: j_begin, j_begin + 128, ...
  const int live_end = seq < c1 ? seq : c1;     // fragments that start below it are computed, the rest of the chunk is zeros
  int j_zero = j_begin;
  if (j_begin < live_end) j_zero = j_begin + (live_end - j_begin + PW * 32 - 1) / (PW * 32) * (PW * 32);
  if (h == 0)
    for (int j = j_zero + n; j < c1; j += PW * 32) orow[j] = 0.f;
  if (j_begin >= live_end) return;  // (wave-uniform; no barrier in this kernel)

  Query<NM> qa;
  qa.load(q, wt, b, true, H, n, h);
  const int32_t* trow = table + (int64_t)b * table_stride;
  const int64_t page_bytes = (int64_t)page_size * (D + 4);

  auto load_frag = [&](KeyFrag& fr, int j0) {
    const int j = j0 + n;
#pragma unroll
    for (int c = 0; c < 4; ++c) fr.d[c] = v4i{0, 0, 0, 0};
    fr.sc = 0.f;
    if (j < live_end) {
      const int pi = page_shift >= 0 ? j >> page_shift : j / page_size;
      const int t = j - pi * page_size;
      int pg = trow[pi];
      pg = pg < 0 ? 0 : (pg >= num_pages ? num_pages - 1 : pg);
      const uint8_t* pb = cache + (int64_t)pg * page_bytes;
      const uint8_t* row = BLOCK ? pb + t * D : pb + t * (D + 4);
      const uint8_t* psc = BLOCK ? pb + (int64_t)page_size * D + t * 4 : row + D;
      fr.d[0] = *(const v4i_a4*)(row + 32 * h);
      fr.d[1] = *(const v4i_a4*)(row + 32 * h + 16);
      fr.d[2] = *(const v4i_a4*)(row + 64 + 32 * h);
      fr.d[3] = *(const v4i_a4*)(row + 64 + 32 * h + 16);
      fr.sc = *(const float*)psc;
    }
  };
  auto compute = [&](const KeyFrag& fr, int j0) {
    const v8i b0 = MQA_FRAG(fr.d[0], fr.d[1]), b1 = MQA_FRAG(fr.d[2], fr.d[3]);
    v16f c = MQA_MFMA(qa.a[0][0], b0, zero16());
    c = MQA_MFMA(qa.a[0][1], b1, c);
    float p = 0.f;
    if constexpr (NM == 2) {
      v16f c2 = MQA_MFMA(qa.a[1][0], b0, zero16());
      c2 = MQA_MFMA(qa.a[1][1], b1, c2);
      p = head_sum(c, qa.w[0], p);
      c = c2;
    }
    p = head_sum(c, qa.w[NM - 1], p);
    float x0 = p, x1 = p;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x0), "+v"(x1));  // x0 = low half twice, x1 = high half twice
    const int j = j0 + n;
    if (h == 0 && j < c1) orow[j] = j < seq ? (x0 + x1) * fr.sc : 0.f;
  };

  constexpr int ST = PW * 32;
  KeyFrag r0, r1, r2;
  load_frag(r0, j_begin);
  load_frag(r1, j_begin + ST);
  for (int j = j_begin; j < live_end; j += 3 * ST) {
    load_frag(r2, j + 2 * ST);
    compute(r0, j);
    if (j + ST >= live_end) break;
    load_frag(r0, j + 3 * ST);
    compute(r1, j + ST);
    if (j + 2 * ST >= live_end) break;
    load_frag(r1, j + 4 * ST);
    compute(r2, j + 2 * ST);
  }
}

}  // namespace
}  // namespace sglk

extern "C" int sglk_fp8_mqa_logits(sglk_stream_t stream, float* logits, const void* q, const void* k, const float* k_scale,
                                   const float* weights, const int32_t* ks, const int32_t* ke, int64_t n_q, int64_t n_k,
                                   int64_t heads, int64_t head_dim, int64_t ld_logits) {
  using namespace sglk;
  const char* op = "fp8_mqa_logits";
  SGLK_REQUIRE(n_q >= 0 && n_k >= 0 && heads > 0 && head_dim > 0, "%s: bad shape", op);
  if (head_dim != D) return fail(SGLK_EUNSUPPORTED, "%s: head_dim = %lld, only 128 is supported", op, (long long)head_dim);
  if (heads > 64) return fail(SGLK_EUNSUPPORTED, "%s: heads = %lld, at most 64 are supported", op, (long long)heads);
  if (n_q == 0 || n_k == 0) return SGLK_OK;
  SGLK_REQUIRE(logits && q && k && k_scale && weights && ks && ke, "%s: null pointer", op);
  SGLK_REQUIRE((uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0, "%s: q and k must be 16-byte aligned", op);
  SGLK_REQUIRE(ld_logits >= n_k, "%s: ld_logits < n_k", op);
  // what the buffer resources address with 32-bit offsets: all of k, and 16 rows of the output
  SGLK_REQUIRE(n_k < (1ll << 24) && QB * ld_logits * 4 < (1ll << 31) && n_q < (1ll << 31) - QB,
               "%s: n_k must be below 2^24 and 16 rows of logits below 2 GiB", op);
  const int64_t ntiles = cdiv(n_k, KT), qblocks = cdiv(n_q, QB);
  // a chunk of up to 16 tiles amortises the 128 KiB of queries a workgroup loads; shorter where that leaves CUs idle
  int64_t tpc = 16;
  while (tpc > 1 && qblocks * cdiv(ntiles, tpc) < 2 * num_cus()) tpc /= 2;
  SGLK_REQUIRE(qblocks < 65536, "%s: n_q must be below 2^20", op);
  const dim3 grid((unsigned)cdiv(ntiles, tpc), (unsigned)qblocks);
  hipStream_t st = (hipStream_t)stream;
  if (heads <= 32)
    mqa_ragged_kernel<1><<<grid, 512, 0, st>>>(logits, (const uint8_t*)q, (const uint8_t*)k, k_scale, weights, ks, ke, (int)n_q,
                                               (int)n_k, (int)heads, ld_logits, (int)tpc);
  else
    mqa_ragged_kernel<2><<<grid, 512, 0, st>>>(logits, (const uint8_t*)q, (const uint8_t*)k, k_scale, weights, ks, ke, (int)n_q,
                                               (int)n_k, (int)heads, ld_logits, (int)tpc);
  return check_launch(op);
}

extern "C" int sglk_fp8_paged_mqa_logits(sglk_stream_t stream, float* logits, const void* q, const void* kv_cache,
                                         const float* weights, const int32_t* seq_lens, const int32_t* block_tables,
                                         int64_t batch, int64_t heads, int64_t head_dim, int64_t page_size, int64_t num_pages,
                                         int64_t table_stride, int64_t max_seq_len, int64_t ld_logits, int layout) {
  using namespace sglk;
  const char* op = "fp8_paged_mqa_logits";
  SGLK_REQUIRE(batch >= 0 && heads > 0 && head_dim > 0 && max_seq_len >= 0, "%s: bad shape", op);
  if (head_dim != D) return fail(SGLK_EUNSUPPORTED, "%s: head_dim = %lld, only 128 is supported", op, (long long)head_dim);
  if (heads > 64) return fail(SGLK_EUNSUPPORTED, "%s: heads = %lld, at most 64 are supported", op, (long long)heads);
  SGLK_REQUIRE(layout == SGLK_MQA_CACHE_ROWS || layout == SGLK_MQA_CACHE_BLOCKS, "%s: unknown cache layout %d", op, layout);
  if (batch == 0 || max_seq_len == 0) return SGLK_OK;
  SGLK_REQUIRE(logits && q && kv_cache && weights && seq_lens && block_tables, "%s: null pointer", op);
  SGLK_REQUIRE(page_size >= 1 && num_pages >= 1 && page_size < (1ll << 20) && num_pages < (1ll << 31),
               "%s: page_size and num_pages must be at least 1", op);
  SGLK_REQUIRE((uintptr_t)q % 16 == 0 && (uintptr_t)kv_cache % 4 == 0, "%s: q must be 16-byte and kv_cache 4-byte aligned", op);
  SGLK_REQUIRE(ld_logits >= max_seq_len && max_seq_len < (1ll << 31) - 4096 && batch < 65536,
               "%s: ld_logits < max_seq_len, or max_seq_len or batch too large", op);
  SGLK_REQUIRE(table_stride >= cdiv(max_seq_len, page_size), "%s: a block table row is shorter than ceil(max_seq_len / page_size)", op);
  // chunks of up to 2048 keys; shorter while that leaves fewer than 4 workgroups (16 waves) a CU
  int64_t chunk = 2048;
  while (chunk > PCH_MIN && batch * cdiv(max_seq_len, chunk) < 4 * num_cus()) chunk /= 2;
  int shift = -1;
  if ((page_size & (page_size - 1)) == 0) shift = __builtin_ctzll((unsigned long long)page_size);
  const dim3 grid((unsigned)cdiv(max_seq_len, chunk), (unsigned)batch);
  hipStream_t st = (hipStream_t)stream;
#define MQA_LAUNCH(NM, BLOCK)                                                                                              \
  mqa_paged_kernel<NM, BLOCK><<<grid, PW * 64, 0, st>>>(logits, (const uint8_t*)q, (const uint8_t*)kv_cache, weights, seq_lens, \
                                                        block_tables, (int)heads, (int)page_size, shift, (int)num_pages,   \
                                                        table_stride, (int)max_seq_len, ld_logits, (int)chunk)
  const bool blocks = layout == SGLK_MQA_CACHE_BLOCKS;
  if (heads <= 32) {
    if (blocks) MQA_LAUNCH(1, true); else MQA_LAUNCH(1, false);
  } else {
    if (blocks) MQA_LAUNCH(2, true); else MQA_LAUNCH(2, false);
  }
#undef MQA_LAUNCH
  return check_launch(op);
}
