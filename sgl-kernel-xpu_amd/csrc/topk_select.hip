// Exact top-k selection behind the DeepSeek-V3.2 indexer scores (fast_topk_v2, fast_topk_transform_fused,
// fast_topk_transform_ragged_fused, topk_transform_512 / _v2; reference src/sycl/TopKTransform.cpp,
// python/sgl_kernel/top_k.py), gfx950. DESIGN 4.15.
//
// One workgroup of 512 threads per score row; an HBM/L2 stream plus LDS kernel, no matrix instructions. A radix select over
// the order-preserving 32-bit key of a float (bits complemented if negative, sign bit set otherwise), digits 12 + 10 + 10
// bits from the top:
//   * histogram pass: the window is read with 16-byte buffer loads (4 in flight per lane, only 4-byte alignment needed),
//     the digit of every element that matches the prefix found so far is counted in a 4096-bin LDS histogram. Lanes whose
//     digit equals lane 0's are counted with one ballot and ONE atomic (the all-equal / many-zeros rows would otherwise
//     serialise 64 same-address atomics per instruction);
//   * threshold: every thread sums its 8 bins, a shuffle suffix scan over the wave plus 8 wave totals finds the thread
//     that holds the k-th element, that thread walks its 8 bins: 2 barriers, none per bit;
//   * histogram passes over the ROW repeat only while more than CAP = 4096 elements match the prefix (a first digit that
//     holds more than 4096 elements; all-equal rows end with a 32-bit prefix). Windows of at most CAP elements skip them;
//   * compaction pass (the last read of the row, from L2): elements above the prefix go to the result staged in LDS,
//     elements that match it go to the candidate list in LDS (key, index). Positions come from ballots / mbcnt inside a
//     wave and one 8-entry exchange per 8192 elements across waves, so candidates stay in index order and the output is
//     the same bits on every run;
//   * the remaining digits run over the candidate list in LDS with the same two routines; the final pass takes the keys
//     above the k-th key and, of those equal to it, the first `needed` in index order (ties: lowest indices win);
//   * epilogue: the staged indices are mapped (page table / offset / paged) and written with coalesced stores.
// Nothing is ever truncated: a prefix of all 32 bits means every matching element is equal, and the compaction pass then
// takes the lowest indices straight from the row.
//
// Bounds: row_starts is clamped to [0, width], lengths to [0, width - row_start]; the buffer resource ends at the row's
// width as well, and vectors that cross the window's end are read dword by dword, so no byte outside the window is read.
// Every LDS write is bounded by its array, every table index by the table: a row that another stream rewrites between
// the passes gives wrong numbers, never a fault.
#include "common.h"

namespace sglk {
namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));

constexpr int TPB = 512, NW = TPB / 64;
constexpr int KMAX = 2048;             // largest k (the result staging)
constexpr int CAP = 4096;              // candidate list
constexpr int NBIN = 4096, BPT = NBIN / TPB;
constexpr int U = 4;                   // 16-byte vectors a lane keeps in flight
constexpr int WCHUNK = U * 256;        // elements a wave covers per step, contiguous
constexpr int STEP = NW * WCHUNK;

struct Smem {
  uint32_t hist[NBIN];
  uint32_t ckey[CAP];
  int32_t cidx[CAP];
  int32_t res[KMAX];
  uint32_t wsum[NW];
  uint32_t wcnt[2][NW][2];
  uint32_t thr[3];
};

struct TopkArgs {
  int32_t* out;
  int32_t* raw;
  const float* score;
  const int32_t *lengths, *row_starts, *table, *aux;
  int64_t ld_score, ld_out, ld_raw, ld_table;
  int width, k, table_rows, table_cols, page_bits, mode;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, uint32_t nrec) {
  const uint64_t u = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)hi << 32) | lo), 0,
                                           (int)__builtin_amdgcn_readfirstlane(nrec), 0x00020000);
}

__device__ __forceinline__ uint32_t key_of(uint32_t bits) { return bits ^ ((uint32_t)((int32_t)bits >> 31) | 0x80000000u); }
// the top `pbits` bits of a key (0 for pbits == 0)
__device__ __forceinline__ uint32_t top_bits(uint32_t key, int pbits) { return (uint32_t)((uint64_t)key >> (32 - pbits)); }
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Keys of the U vectors of a wave's chunk: lane l holds elements base + u * 256 + 4 * l + {0..3}. Elements at or past n
// come back as key 0 and are masked by position by the callers. LDS: from the candidate list instead of the row.
template <bool LDS>
__device__ __forceinline__ void load_keys(const Smem& sm, __amdgpu_buffer_rsrc_t rs, uint32_t rs0, int base, int lane, int n,
                                          uint32_t (&key)[U][4]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int pos = base + u * 256 + 4 * lane;
    v4u v = {0u, 0u, 0u, 0u};
    if constexpr (LDS) {
      if (pos < n) v = *reinterpret_cast<const v4u*>(&sm.ckey[pos]);  // (n <= CAP, both multiples of 4 apart from n)
#pragma unroll
      for (int j = 0; j < 4; ++j) key[u][j] = v[j];
    } else {
      const uint32_t off = (rs0 + (uint32_t)pos) * 4u;
      if (pos + 4 <= n) {
        v = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (pos + j < n) v[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 4u * j, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) key[u][j] = key_of(v[j]);
    }
  }
}

// hist[d] = number of elements whose top pbits bits equal pval and whose next w bits equal d
template <bool LDS>
__device__ __forceinline__ void hist_pass(Smem& sm, __amdgpu_buffer_rsrc_t rs, uint32_t rs0, int n, int pbits, uint32_t pval,
                                          int w) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int i = 0; i < BPT; ++i) sm.hist[tid + i * TPB] = 0u;
  __syncthreads();
  const int shift = 32 - pbits - w;
  const uint32_t mask = (1u << w) - 1u;
  for (int base = wave * WCHUNK; base < n; base += STEP) {
    uint32_t key[U][4];
    load_keys<LDS>(sm, rs, rs0, base, lane, n, key);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pos = base + u * 256 + 4 * lane + j;
        const bool ok = pos < n && top_bits(key[u][j], pbits) == pval;
        const uint32_t d = ok ? (key[u][j] >> shift) & mask : ~0u;
        const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
        const uint64_t same = __ballot(d == d0);
        if (d == d0) {
          if (lane == 0 && d0 != ~0u) atomicAdd(&sm.hist[d0], (uint32_t)__popcll(same));
        } else if (d != ~0u) {
          atomicAdd(&sm.hist[d], 1u);
        }
      }
  }
  __syncthreads();
}

// The bin t that holds the k_rem-th largest of the counted elements: k_rem loses the elements of the bins above t,
// cnt = hist[t]. Every thread returns the same values.
__device__ __forceinline__ void find_threshold(Smem& sm, uint32_t& k_rem, uint32_t& t, uint32_t& cnt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t h[BPT];
  const v4u h0 = *reinterpret_cast<const v4u*>(&sm.hist[tid * BPT]), h1 = *reinterpret_cast<const v4u*>(&sm.hist[tid * BPT + 4]);
#pragma unroll
  for (int i = 0; i < 4; ++i) h[i] = h0[i], h[4 + i] = h1[i];
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < BPT; ++i) s += h[i];
  uint32_t inc = s;  // -> sum over this lane and the lanes above it
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_down(inc, o, 64);
    if (lane + o < 64) inc += v;
  }
  if (lane == 0) sm.wsum[wave] = inc;
  __syncthreads();
  uint32_t above = inc - s;
  for (int i = wave + 1; i < NW; ++i) above += sm.wsum[i];
  if (above < k_rem && k_rem <= above + s) {  // (exactly one thread)
#pragma unroll
    for (int i = BPT - 1; i >= 0; --i) {
      if (above + h[i] >= k_rem) {
        sm.thr[0] = (uint32_t)(tid * BPT + i), sm.thr[1] = above, sm.thr[2] = h[i];
        break;
      }
      above += h[i];
    }
  }
  __syncthreads();
  t = sm.thr[0], cnt = sm.thr[2];
  k_rem -= sm.thr[1];
}

// One pass over the row (or the candidate list): elements above the prefix go to res[out_above ...]; elements that
// match it go to the candidate list, or - direct - the first k_rem of them go to res[k - k_rem ...]. All in index order.
template <bool LDS>
__device__ __forceinline__ void compact_pass(Smem& sm, __amdgpu_buffer_rsrc_t rs, uint32_t rs0, int n, int pbits, uint32_t pval,
                                             bool direct, uint32_t out_above, uint32_t k_rem, uint32_t k) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t base_a = out_above, base_e = 0u;
  int it = 0;
  for (int base0 = 0; base0 < n; base0 += STEP, it ^= 1) {
    const int base = base0 + wave * WCHUNK;
    uint32_t key[U][4];
    load_keys<LDS>(sm, rs, rs0, base, lane, n, key);
    uint32_t fa[U], fe[U], ra[U], re[U], tot_a = 0u, tot_e = 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      fa[u] = fe[u] = 0u;
      ra[u] = tot_a, re[u] = tot_e;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pos = base + u * 256 + 4 * lane + j;
        const uint32_t hi = top_bits(key[u][j], pbits);
        const bool a = pos < n && hi > pval, e = pos < n && hi == pval;
        const uint64_t ba = __ballot(a), be = __ballot(e);
        fa[u] |= (uint32_t)a << j, fe[u] |= (uint32_t)e << j;
        ra[u] += lanes_below(ba), re[u] += lanes_below(be);
        tot_a += (uint32_t)__popcll(ba), tot_e += (uint32_t)__popcll(be);
      }
    }
    if (lane == 0) sm.wcnt[it][wave][0] = tot_a, sm.wcnt[it][wave][1] = tot_e;
    __syncthreads();  // (two buffers: a wave that writes step i + 2 has passed the barrier of step i + 1)
    uint32_t pre_a = 0u, pre_e = 0u, sum_a = 0u, sum_e = 0u;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const uint32_t ca = sm.wcnt[it][i][0], ce = sm.wcnt[it][i][1];
      if (i < wave) pre_a += ca, pre_e += ce;
      sum_a += ca, sum_e += ce;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint32_t pa = base_a + pre_a + ra[u], pe = base_e + pre_e + re[u];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pos = base + u * 256 + 4 * lane + j;
        if ((fa[u] >> j) & 1u) {
          if (pa < k) sm.res[pa] = LDS ? sm.cidx[pos] : pos;
          ++pa;
        }
        if ((fe[u] >> j) & 1u) {
          if (direct) {
            if (pe < k_rem && k - k_rem + pe < k) sm.res[k - k_rem + pe] = LDS ? sm.cidx[pos] : pos;
          } else if (pe < (uint32_t)CAP) {
            sm.ckey[pe] = key[u][j], sm.cidx[pe] = pos;
          }
          ++pe;
        }
      }
    }
    base_a += sum_a, base_e += sum_e;
  }
  __syncthreads();
}

__global__ __launch_bounds__(TPB) void topk_select_kernel(const TopkArgs a) {
  __shared__ Smem sm;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int k = a.k;
  int rs0 = a.row_starts ? a.row_starts[b] : 0;
  rs0 = min(max(rs0, 0), a.width);
  const int n = min(max(a.lengths[b], 0), a.width - rs0);

  if (n > k) {
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.score + b * a.ld_score, (uint32_t)a.width * 4u);
    int pbits = 0;
    uint32_t pval = 0u, k_rem = (uint32_t)k, m = (uint32_t)n, t;
    while (m > (uint32_t)CAP && pbits < 32) {
      const int w = pbits ? 10 : 12;
      hist_pass<false>(sm, rs, (uint32_t)rs0, n, pbits, pval, w);
      find_threshold(sm, k_rem, t, m);
      pval = (pval << w) | t, pbits += w;
    }
    if (pbits == 32) {  // more than CAP elements equal the k-th value: the lowest indices, straight from the row
      compact_pass<false>(sm, rs, (uint32_t)rs0, n, 32, pval, true, 0u, k_rem, (uint32_t)k);
    } else {
      compact_pass<false>(sm, rs, (uint32_t)rs0, n, pbits, pval, false, 0u, k_rem, (uint32_t)k);
      const uint32_t out_above = (uint32_t)k - k_rem;
      const int nc = (int)min(m, (uint32_t)CAP);
      while (pbits < 32) {
        const int w = pbits ? 10 : 12;
        hist_pass<true>(sm, rs, 0u, nc, pbits, pval, w);
        find_threshold(sm, k_rem, t, m);
        pval = (pval << w) | t, pbits += w;
      }
      compact_pass<true>(sm, rs, 0u, nc, 32, pval, true, out_above, k_rem, (uint32_t)k);
    }
  }

  // ---- epilogue: map the staged window-relative indices and write them ----
  int seq = (int)b;
  if (a.mode == SGLK_TOPK_PAGE_TABLE && a.aux) {  // the sequence with cu_seqlens_q[seq] <= b < cu_seqlens_q[seq + 1]
    int lo = 0, hi = a.table_rows - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((int64_t)a.aux[mid] <= b) lo = mid; else hi = mid - 1;
    }
    seq = lo;
  }
  seq = min(seq, a.table_rows - 1);
  const int32_t* trow = a.table ? a.table + (int64_t)seq * a.ld_table : nullptr;
  const int32_t add = a.mode == SGLK_TOPK_OFFSET ? a.aux[b] : 0;
  const int pmask = (1 << a.page_bits) - 1;
  for (int i = tid; i < k; i += TPB) {
    const int p = n > k ? sm.res[i] : (i < n ? i : -1);
    int32_t v = p;
    if (p >= 0) {
      if (a.mode == SGLK_TOPK_PAGE_TABLE) v = trow[min(p, a.table_cols - 1)];
      else if (a.mode == SGLK_TOPK_OFFSET) v = p + add;
      else if (a.mode == SGLK_TOPK_PAGED) v = (int32_t)(((uint32_t)trow[min(p >> a.page_bits, a.table_cols - 1)] << a.page_bits) | (uint32_t)(p & pmask));
    }
    a.out[b * a.ld_out + i] = v;
    if (a.raw) a.raw[b * a.ld_raw + i] = p;
  }
}

}  // namespace
}  // namespace sglk

extern "C" int sglk_topk_select(sglk_stream_t stream, int32_t* out, int32_t* out_raw, const float* score,
                                const int32_t* lengths, const int32_t* row_starts, const int32_t* table, const int32_t* aux,
                                int64_t rows, int64_t width, int64_t ld_score, int64_t topk, int64_t ld_out, int64_t ld_raw,
                                int64_t table_rows, int64_t table_cols, int64_t ld_table, int64_t page_size, int mode) {
  using namespace sglk;
  const char* op = "topk_select";
  SGLK_REQUIRE(rows >= 0 && width >= 0 && ld_score >= width, "%s: bad shape", op);
  SGLK_REQUIRE(mode >= SGLK_TOPK_RAW && mode <= SGLK_TOPK_PAGED, "%s: unknown mode %d", op, mode);
  if (topk < 1 || topk > KMAX) return fail(SGLK_EUNSUPPORTED, "%s: topk = %lld, 1..%d are supported", op, (long long)topk, KMAX);
  if (rows == 0) return SGLK_OK;
  SGLK_REQUIRE(out && score && lengths, "%s: null pointer", op);
  SGLK_REQUIRE(width < (1ll << 28) && rows < (1ll << 31), "%s: width must be below 2^28 and rows below 2^31", op);
  SGLK_REQUIRE(ld_out >= topk && (!out_raw || ld_raw >= topk), "%s: an output row is shorter than topk", op);
  int bits = 0;
  if (mode == SGLK_TOPK_PAGE_TABLE || mode == SGLK_TOPK_PAGED) {
    SGLK_REQUIRE(table && table_rows >= 1 && table_cols >= 1 && ld_table >= table_cols && table_rows < (1ll << 31) &&
                     table_cols < (1ll << 31), "%s: this mode needs a table with at least one row and one column", op);
    SGLK_REQUIRE(aux || table_rows >= rows, "%s: without cu_seqlens_q the table needs a row per score row", op);
  }
  if (mode == SGLK_TOPK_PAGED) {
    SGLK_REQUIRE(page_size >= 1 && page_size <= (1 << 20) && (page_size & (page_size - 1)) == 0,
                 "%s: page_size must be a power of two, at most 2^20", op);
    bits = __builtin_ctzll((unsigned long long)page_size);
    aux = nullptr;
  }
  if (mode == SGLK_TOPK_OFFSET) SGLK_REQUIRE(aux, "%s: this mode needs the offsets", op);
  TopkArgs a{out, out_raw, score, lengths, row_starts, table, aux, ld_score, ld_out, ld_raw, ld_table,
             (int)width, (int)topk, (int)table_rows, (int)table_cols, bits, mode};
  topk_select_kernel<<<dim3((unsigned)rows), TPB, 0, (hipStream_t)stream>>>(a);
  return check_launch(op);
}
