// flash_mla_sparse_decode for gfx950: DeepSeek-V4 sparse MLA decode over the packed fp8 latent cache. Every query token
// attends to its own list of cache tokens, `topk` of them in a main cache followed by `extra_topk` in an optional
// second cache with its own page size, with invalid entries anywhere in both lists.
//
// Contract (reference python/sgl_kernel/attention.py:250-353, schema src/torch_extension_sycl.cc:371-374, meaning
// tests/test_flash_mla_with_kvcache.py). A cache is [pages, page_size, 1, 584] bytes with `page_bytes` between pages;
// token t of a page at byte P has 448 e4m3 bytes (7 tiles of 64) + 64 bf16 of rope at P + 576 t and 7 UE8M0 scale bytes
// (+ 1 pad) at P + 576 page_size + 8 t. Row = [fp8 * 2^(scale - 127) (448 values), rope (64)]: 512 columns, K and V.
// Slot j of a list is valid iff 0 <= idx < pages * page_size and (no length or j < length[b]); over the valid slots
//   P = sm_scale * q[b, s, h] . row,  lse[b, h, s] = ln sum exp P (+inf without a valid slot; the sink does not change it),
//   out[b, s, h] = sum exp(P - lse') row,  lse' = logaddexp(lse, attn_sink[h]);  exactly 0 without a valid slot.
// A cache token that no valid slot names is never read, neither its data nor its scale bytes.
//
// Design. The compute side is that of mla_sparse_kernel<W, ROPE = false> (mla_sparse.hip; mla_decode.hip documents the
// swizzled [32][1024 B] LDS image and the pi / tau permutations): one workgroup of 8 waves per (query token, block of
// <= 128 heads, slot split), W = 8 / 4 / 2 / 1 waves per 16-head group, tiles of 32 slots, S^T = K . Q^T on 16x16x32
// bf16 MFMA, online softmax, O += P . V through transposed LDS reads. What is new is how a tile arrives: the cache is
// quantised and packed, so LDS-DMA cannot deliver it. One pass instead, HBM -> registers -> LDS, dequantised on the way:
//   - Virtual tiles. The main list is cut into ceil(n_main / 32) tiles and the extra list into ceil(n_extra / 32) tiles
//     that follow them (n = the list length clamped by its topk_length): a tile belongs to ONE cache, so its page
//     size, base and strides are uniform, and the slots past a length cost nothing.
//   - Indices. Lane l of every wave loads the index of slot l & 31 of a tile, one tile ahead of the rows. A ballot gives
//     the tile's 32 validity bits as a scalar (they mask the scores later), a lane shuffle gives each lane the index of
//     the row it fetches. page = idx >> log2(page_size) where the page size is a power of two, idx / page_size otherwise.
//   - Rows. 16 lanes fetch one row (wave w: rows 4w .. 4w + 3): the 576 data bytes are 36 chunks of 16 B, lane c takes
//     chunks c, c + 16 and, for c < 4, c + 32 (chunks 28 .. 35 are the rope), plus the row's 8 scale bytes. An invalid
//     slot loads nothing: its registers are zeros and its score becomes -inf.
//   - Dequantisation in registers with gfx950's scaled conversion (v_cvt_scalef32_pk_bf16_fp8, scale = the UE8M0 byte
//     shifted into an f32 exponent): exact, one instruction per pair. A 16-byte fp8 chunk becomes the two adjacent
//     16-byte bf16 chunks of the image (ds_write_b128 each); a rope chunk is stored as it is.
//   - Pipeline. The raw bytes of tile i + 1 (14 registers a lane) and the indices of tile i + 2 are in flight while
//     tile i is multiplied; the image is double-buffered (2 x 32 KiB instead of the 4 x 36 KiB ring of prefill), one
//     barrier a tile. With the 16 KiB exchange area of W > 1 a workgroup takes 80 KiB, so LDS would let two share a CU;
//     the registers do not (see the launch bounds).
//   - Slot splits. Decode has few tokens and long lists: `splits` workgroups share a token's virtual tiles evenly. With
//     splits > 1 each writes its unnormalised fp32 O and (m, l) to the workspace and a second small launch merges them,
//     applies the sink and writes out / lse; a split without a valid slot carries (-inf, 0) and merges as nothing. With
//     splits == 1 the kernel writes the result itself.
#include <math.h>

#include "common.h"

namespace sglk {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef short v8s __attribute__((ext_vector_type(8)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));

constexpr int kLatent = 512;
constexpr int kTile = 32;                 // slots per tile
constexpr int kStageBytes = kTile * 1024;  // one image: [32 slots][512 bf16], swizzled
constexpr int kStages = 2;
constexpr int kThreads = 512;
constexpr int kHeadBlock = 128;
constexpr int kPartOff = kStages * kStageBytes;  // W > 1: 8 waves x [2 token tiles][64 lanes][16 B]
constexpr int kRowBytes = 576;                   // data bytes of a cache token
constexpr int kCombineThreads = 128;

#define SGLK_LDS(p) ((__attribute__((address_space(3))) void*)(p))

__device__ __forceinline__ v4f mfma(const v8s& a, const v8s& b, const v4f& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
}
__device__ __forceinline__ short cvt_bf16(float x) { return __builtin_bit_cast(short, (bf16)x); }
__device__ __forceinline__ int sw_main(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

struct DecodeCache {
  const char* base;
  int64_t page_bytes;
  int64_t scale_off;  // 576 * page_size: where a page's scale bytes start
  int page_size, shift;  // shift = log2(page_size) or -1
  int ntok;              // pages * page_size
};

struct DecodeParams {
  bf16* out;       // [B, s_q, H, 512]
  float* lse;      // [B, H, s_q]
  float* part_o;   // splits > 1: [tokens, splits, H, 512] unnormalised
  float* part_ml;  //             [tokens, splits, H, 2] = (max raw logit, sum)
  DecodeCache cache[2];
  const int32_t* idx[2];  // [tokens, topk[w]]
  const int32_t* len[2];  // [B] or null
  int topk[2];
  int64_t q_sb, q_ss, q_sh;  // elements
  int H, s_q, splits;
  float scale_log2;
};

// slots of list w in front of its length
__device__ __forceinline__ int live_slots(const DecodeParams& p, int w, int b) {
  int n = p.topk[w];
  if (p.len[w] != nullptr) {
    const int tl = p.len[w][b];
    n = tl < 0 ? 0 : (tl < n ? tl : n);
  }
  return n;
}

// 16 e4m3 bytes times 2^(sbyte - 127) -> 16 bf16 (exact: 4 significant bits into 8)
__device__ __forceinline__ void dequant16(const v4i& x, int sbyte, v4i& lo, v4i& hi) {
  const float sc = __uint_as_float(sbyte ? (uint32_t)sbyte << 23 : 0x00400000u);
  lo[0] = __builtin_bit_cast(int, (v2bf)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[0], sc, false));
  lo[1] = __builtin_bit_cast(int, (v2bf)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[0], sc, true));
  lo[2] = __builtin_bit_cast(int, (v2bf)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[1], sc, false));
  lo[3] = __builtin_bit_cast(int, (v2bf)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[1], sc, true));
  hi[0] = __builtin_bit_cast(int, (v2bf)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[2], sc, false));
  hi[1] = __builtin_bit_cast(int, (v2bf)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[2], sc, true));
  hi[2] = __builtin_bit_cast(int, (v2bf)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[3], sc, false));
  hi[3] = __builtin_bit_cast(int, (v2bf)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[3], sc, true));
}

// the raw bytes a lane holds of one tile: chunks c, c + 16, c + 32 (c < 4) of its row, and the row's scales
struct RawTile {
  v4i a, b, c;
  v2i sc;
};


// q [B, s_q, H, 512] (strides in p), attn_sink [H] or null: read-only for the whole launch.
// Two waves a SIMD (256 registers), one workgroup a CU: at four waves (128 registers, which the 80 KiB of LDS would allow
// for two workgroups) the compiler reloads spilled values inside the tile loop at W = 4 and W = 8.
template <int W>
__global__ __launch_bounds__(kThreads, 2) void mla_sparse_decode_kernel(DecodeParams p,
                                                                                  const bf16* __restrict__ q,
                                                                                  const float* __restrict__ attn_sink) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  constexpr int kNK = 16;      // 32-deep k-steps of QK^T
  constexpr int kNT = 32 / W;  // 16-column output tiles per wave
  constexpr int kKS = kNK / W;  // QK^T k-steps per wave

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hg = wave / W, ww = wave % W;  // head group, position inside the group
  const int tok = blockIdx.x;
  const int b = tok / p.s_q, sq = tok - b * p.s_q;
  const int head0 = blockIdx.y * kHeadBlock;
  const int H = (p.H - head0) < kHeadBlock ? (p.H - head0) : kHeadBlock;  // heads of this block
  const int l15 = lane & 15, g = lane >> 4;
  const bool active = hg * 16 < H;

  // ---- this workgroup's range of virtual tiles: the main list's, then the extra list's
  const int n0 = live_slots(p, 0, b), n1 = live_slots(p, 1, b);
  const int nt0 = (n0 + kTile - 1) / kTile, nt1 = (n1 + kTile - 1) / kTile;
  const int per = (nt0 + nt1 + p.splits - 1) / p.splits;
  const int t_begin = blockIdx.z * per;
  const int t_stop = t_begin + per < nt0 + nt1 ? t_begin + per : nt0 + nt1;
  const int ntiles = t_stop > t_begin ? t_stop - t_begin : 0;
  const int32_t* idx0 = p.idx[0] + (int64_t)tok * p.topk[0];
  const int32_t* idx1 = p.idx[1] + (int64_t)tok * p.topk[1];

  // index of slot lane & 31 of virtual tile t as it stands in the list, -1 past the list's length (the loaded value is
  // not looked at here: a compare would wait for the row loads issued in front of it)
  auto load_idx = [&](int t) {
    const bool ex = t >= nt0;
    const int slot = (ex ? t - nt0 : t) * kTile + (lane & 31);
    int idx = -1;
    if (slot < (ex ? n1 : n0)) idx = (ex ? idx1 : idx0)[slot];
    return idx;
  };
  // row 4 wave + g of the tile, chunks l15 (+ 16, + 32): returns the tile's 32 validity bits
  auto load_rows = [&](int t, int idxv, RawTile& raw) {
    const bool ex = t >= nt0;
    const bool okv = (unsigned)idxv < (unsigned)(ex ? p.cache[1].ntok : p.cache[0].ntok);
    const int mk = (int)(unsigned)__ballot(okv);
    const int idx = __shfl(okv ? idxv : -1, 4 * wave + g, 64);
    const char* base = ex ? p.cache[1].base : p.cache[0].base;
    const int64_t page_bytes = ex ? p.cache[1].page_bytes : p.cache[0].page_bytes;
    const int64_t scale_off = ex ? p.cache[1].scale_off : p.cache[0].scale_off;
    const int page_size = ex ? p.cache[1].page_size : p.cache[0].page_size;
    const int shift = ex ? p.cache[1].shift : p.cache[0].shift;
    const v4i zero = {0, 0, 0, 0};
    raw.a = raw.b = raw.c = zero;
    raw.sc = (v2i){0, 0};
    if (idx >= 0) {
      const int page = shift >= 0 ? idx >> shift : idx / page_size;
      const int off = idx - page * page_size;
      const char* pg = base + (int64_t)page * page_bytes;
      const char* row = pg + (int64_t)off * kRowBytes + 16 * l15;
      raw.a = *reinterpret_cast<const v4i*>(row);
      raw.b = *reinterpret_cast<const v4i*>(row + 256);
      if (l15 < 4) raw.c = *reinterpret_cast<const v4i*>(row + 512);
      raw.sc = *reinterpret_cast<const v2i*>(pg + scale_off + 8 * (int64_t)off);
    }
    return mk;
  };
  // dequantise and store: logical 16-byte chunk lc of column block cb of row r lives at
  // cb * 8192 + (r >> 2) * 1024 + (r & 3) * 256 + ((lc ^ sw_main(r)) << 4)
  auto store_tile = [&](const RawTile& raw, int st) {
    const int r = 4 * wave + g;
    char* rowp = smem + st * kStageBytes + wave * 1024 + g * 256;
    const int sw = sw_main(r);
    const int sh = 8 * (l15 >> 2);  // scale tile of chunk k is k >> 2: byte l15 >> 2 of sc[0] / of sc[1]
    v4i lo, hi;
    // fp8 chunk k -> logical chunks 2 (k & 7) and the next one of block k >> 3: neighbours, in either order
    const int d = (l15 >> 3) * 8192 + (((2 * (l15 & 7)) ^ sw) << 4);
    dequant16(raw.a, (raw.sc[0] >> sh) & 255, lo, hi);
    *reinterpret_cast<v4i*>(rowp + d) = lo;
    *reinterpret_cast<v4i*>(rowp + (d ^ 16)) = hi;
    if (l15 < 12) {  // chunks 16 .. 27: fp8 tiles 4 .. 6
      dequant16(raw.b, (raw.sc[1] >> sh) & 255, lo, hi);
      *reinterpret_cast<v4i*>(rowp + 2 * 8192 + d) = lo;
      *reinterpret_cast<v4i*>(rowp + 2 * 8192 + (d ^ 16)) = hi;
    } else {  // chunks 28 .. 31: rope chunks 0 .. 3 = columns 448 .., logical chunks 8 .. 11 of block 3
      *reinterpret_cast<v4i*>(rowp + 3 * 8192 + (((l15 - 4) ^ sw) << 4)) = raw.b;
    }
    if (l15 < 4) *reinterpret_cast<v4i*>(rowp + 3 * 8192 + (((l15 + 12) ^ sw) << 4)) = raw.c;  // rope chunks 4 .. 7
  };

  // k permutation inside a 32-deep MFMA step: lane group g takes the 8 elements at 8*pi(g)
  const int pig = (0x2130 >> (4 * g)) & 3;  // pi = (0,3,1,2)

  // ---- Q^T fragments (MFMA B operand): lane (head l15, group g) holds q[head][32 ks + 8 pi(g) .. +7]
  // wave ww of a group takes k-steps ww, ww + W, ...
  v8s qf[kKS];
  {
    const int head = hg * 16 + l15;
    const bool ok = active && head < H;
    const bf16* qr = q + (int64_t)b * p.q_sb + (int64_t)sq * p.q_ss + (int64_t)(head0 + (ok ? head : 0)) * p.q_sh + 8 * pig;
    const v8s zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int jk = 0; jk < kKS; ++jk) {
      const v8s v = *reinterpret_cast<const v8s*>(qr + 32 * (ww + jk * W));
      qf[jk] = ok ? v : zero;
    }
  }

  // ---- per-lane LDS read offsets (see mla_decode_kernel)
  const int tau = (l15 & 3) | (((l15 >> 2) & 1) << 3) | (((l15 >> 3) & 1) << 2);
  const int kbase = 256 * tau + 16 * (pig ^ sw_main(tau));  // ^ (k4 << 6): chunk 4 k4 + pi(g)
  int vbase0;
  {
    const int qq = l15 >> 2, pp = l15 & 3;
    const int r = 8 * (g & 1) + 4 * (g >> 1) + qq;
    vbase0 = 256 * r + 16 * ((pp >> 1) ^ sw_main(r)) + 8 * (pp & 1);
  }
  int koff[kKS];
#pragma unroll
  for (int jk = 0; jk < kKS; ++jk) {
    const int kc = ww + jk * W;
    koff[jk] = (kc >> 2) * 8192 + (kbase ^ ((kc & 3) << 6));
  }
  const int g0 = ww * kNT;  // first output tile of this wave
  const int vxor_w = vbase0 ^ ((g0 & 7) << 5), vadd_w = (g0 >> 3) * 8192;

  v4f o[kNT];
#pragma unroll
  for (int nt = 0; nt < kNT; ++nt) o[nt] = (v4f){0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY;  // running max of the raw logits of head l15 (all four lane groups agree)
  float l_run = 0.f;        // running sum over this lane's own slots
  auto head_bcast = [&](float v, int r) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(((lane & 48) | (4 * g + r)) << 2, __builtin_bit_cast(int, v)));
  };
  const uint32_t lds_base = (uint32_t)(uintptr_t)SGLK_LDS(smem);
  // bit (8(g&1) + 4(g>>1) + r) of a tile's word = the slot of s0[r]; 16 higher = that of s1[r]
  const int tb = 8 * (g & 1) + 4 * (g >> 1);

  // ---- prologue: the rows of the first tile and the indices of the second are in flight
  RawTile raw;
  int idx_next = -1, mk_next = 0;
  if (ntiles > 0) {
    idx_next = load_idx(t_begin);
    mk_next = load_rows(t_begin, idx_next, raw);
    if (ntiles > 1) idx_next = load_idx(t_begin + 1);
  }

  int st = 0;
  for (int i = 0; i < ntiles; ++i) {
    const int mk = mk_next;
    store_tile(raw, st);
    if (i + 1 < ntiles) {
      mk_next = load_rows(t_begin + i + 1, idx_next, raw);
      if (i + 2 < ntiles) idx_next = load_idx(t_begin + i + 2);
    }
    // tile i is in LDS for every wave; every wave is done with tile i - 1 (whose image tile i + 1 will overwrite)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const char* base = smem + st * kStageBytes;
    v4f s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (W == 1) {
      if (active) {
        // ---- S^T[slot, head] = K . Q^T for the two 16-slot tiles
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          const v8s a0 = *reinterpret_cast<const v8s*>(base + (ks >> 2) * 8192 + (kbase ^ ((ks & 3) << 6)));
          const v8s a1 = *reinterpret_cast<const v8s*>(base + (ks >> 2) * 8192 + 4096 + (kbase ^ ((ks & 3) << 6)));
          s0 = mfma(a0, qf[ks], s0);
          s1 = mfma(a1, qf[ks], s1);
        }
      }
    } else {
      // ---- this wave's share of S^T, left in LDS for the other waves of the group
      const uint32_t part = lds_base + (uint32_t)kPartOff;
      if (active) {
        v4f p0 = {0.f, 0.f, 0.f, 0.f}, p1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jk = 0; jk < kKS; ++jk) {
          const v8s a0 = *reinterpret_cast<const v8s*>(base + koff[jk]);
          const v8s a1 = *reinterpret_cast<const v8s*>(base + koff[jk] + 4096);
          p0 = mfma(a0, qf[jk], p0);
          p1 = mfma(a1, qf[jk], p1);
        }
        const uint32_t mine = part + (uint32_t)(wave * 2048 + lane * 16);
        // p0 / p1 come straight out of the matrix pipe and this asm reads them from the LDS unit: pad by hand
        asm volatile("s_nop 7\n\ts_nop 7\n\tds_write_b128 %0, %1\n\tds_write_b128 %0, %2 offset:1024" ::"v"(mine), "v"(p0),
                     "v"(p1)
                     : "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (active) {
        const uint32_t grp = part + (uint32_t)(hg * W * 2048 + lane * 16);
        v4f q0[W], q1[W];
#pragma unroll
        for (int u = 0; u < W; ++u) {
          asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4"
                       : "=&v"(q0[u]), "=&v"(q1[u])
                       : "v"(grp), "n"(u * 2048), "n"(u * 2048 + 1024)
                       : "memory");
        }
        // the wait names every register it releases, so that the additions cannot be scheduled above it
        if constexpr (W == 2) {
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(q0[0]), "+v"(q1[0]), "+v"(q0[1]), "+v"(q1[1])::"memory");
        } else if constexpr (W == 4) {
          asm volatile("s_waitcnt lgkmcnt(0)"
                       : "+v"(q0[0]), "+v"(q1[0]), "+v"(q0[1]), "+v"(q1[1]), "+v"(q0[2]), "+v"(q1[2]), "+v"(q0[3]), "+v"(q1[3])
                       :
                       : "memory");
        } else {
          asm volatile("s_waitcnt lgkmcnt(0)"
                       : "+v"(q0[0]), "+v"(q1[0]), "+v"(q0[1]), "+v"(q1[1]), "+v"(q0[2]), "+v"(q1[2]), "+v"(q0[3]), "+v"(q1[3]),
                         "+v"(q0[4]), "+v"(q1[4]), "+v"(q0[5]), "+v"(q1[5]), "+v"(q0[6]), "+v"(q1[6]), "+v"(q0[7]), "+v"(q1[7])
                       :
                       : "memory");
        }
#pragma unroll
        for (int u = 0; u < W; ++u) {
          s0 += q0[u];
          s1 += q1[u];
        }
      }
    }
    if (active) {
      // ---- online softmax for head l15 over this lane's 8 slots (+ the other three lane groups')
      if (mk != -1) {
        const int mkl = mk >> tb;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (!(mkl & (1 << r))) s0[r] = -INFINITY;
          if (!(mkl & (0x10000 << r))) s1[r] = -INFINITY;
        }
      }
      float mt = fmaxf(fmaxf(fmaxf(s0[0], s0[1]), fmaxf(s0[2], s0[3])), fmaxf(fmaxf(s1[0], s1[1]), fmaxf(s1[2], s1[3])));
      mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float m_new = fmaxf(m_run, mt);
      // no valid slot so far: factors against 0 (every p is exp2(-inf) = 0, alpha scales an O and an l that are 0)
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_use) * p.scale_log2);
      const float mneg = -m_use * p.scale_log2;
      float psum = 0.f;
      v8s pf;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[r], p.scale_log2, mneg));
        const float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[r], p.scale_log2, mneg));
        psum += p0 + p1;
        pf[r] = cvt_bf16(p0);
        pf[4 + r] = cvt_bf16(p1);
      }
      l_run = l_run * alpha + psum;
      m_run = m_new;
      // ---- rescale O when any head's maximum moved: O row (head) 4g + r needs alpha of head 4g + r
      if (__any(alpha != 1.0f)) {
        const v4f a4 = {head_bcast(alpha, 0), head_bcast(alpha, 1), head_bcast(alpha, 2), head_bcast(alpha, 3)};
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) {
          o[nt][0] *= a4[0]; o[nt][1] *= a4[1]; o[nt][2] *= a4[2]; o[nt][3] *= a4[3];
        }
      }
      // ---- O[head, dim] += P . V   (A = P from registers, B = V via transposed LDS reads issued from inline asm with
      // hand-counted lgkmcnt, one read per asm statement, see mla_decode_kernel). The wait in front empties the counter
      // of whatever the compiler has in flight (the shuffles above); no other LDS / SMEM traffic of this wave may sit
      // inside.
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      {
        constexpr int kDepth = W == 1 ? 1 : 2, kNB = kDepth + 1;
        const uint32_t vb_t = lds_base + (uint32_t)(st * kStageBytes) + (uint32_t)vadd_w;
        v2i vb[kNB][2];
#define SGLK_TR_ISSUE(I)                                                                          \
  do {                                                                                            \
    const uint32_t a_ = vb_t + (uint32_t)(vxor_w ^ (((I) & 7) << 5));                             \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"                                            \
                 : "=v"(vb[(I) % kNB][0]) : "v"(a_), "i"((((I) >> 3) * 8192)) : "memory");        \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"                                            \
                 : "=v"(vb[(I) % kNB][1]) : "v"(a_), "i"((((I) >> 3) * 8192 + 4096)) : "memory"); \
  } while (0)
#define SGLK_TR_WAIT(N, I) \
  asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(vb[(I) % kNB][0]), "+v"(vb[(I) % kNB][1])::"memory")
#define SGLK_TR_STEP(G)                                                                                         \
  if constexpr ((G) < kNT) {                                                                                    \
    if constexpr ((G) + kDepth < kNT) SGLK_TR_ISSUE((G) + kDepth);                                              \
    constexpr int ahead_ = (G) + kDepth < kNT ? kDepth : kNT - 1 - (G);                                         \
    if constexpr (ahead_ == 2) SGLK_TR_WAIT(4, G);                                                              \
    if constexpr (ahead_ == 1) SGLK_TR_WAIT(2, G);                                                              \
    if constexpr (ahead_ == 0) SGLK_TR_WAIT(0, G);                                                              \
    v8s f_;                                                                                                     \
    const v4s x0_ = __builtin_bit_cast(v4s, vb[(G) % kNB][0]), x1_ = __builtin_bit_cast(v4s, vb[(G) % kNB][1]); \
    f_[0] = x0_[0]; f_[1] = x0_[1]; f_[2] = x0_[2]; f_[3] = x0_[3];                                             \
    f_[4] = x1_[0]; f_[5] = x1_[1]; f_[6] = x1_[2]; f_[7] = x1_[3];                                             \
    o[G] = mfma(pf, f_, o[G]);                                                                                  \
  }
        SGLK_TR_ISSUE(0);
        if constexpr (kDepth > 1) SGLK_TR_ISSUE(1);
        SGLK_TR_STEP(0) SGLK_TR_STEP(1) SGLK_TR_STEP(2) SGLK_TR_STEP(3) SGLK_TR_STEP(4) SGLK_TR_STEP(5)
        SGLK_TR_STEP(6) SGLK_TR_STEP(7) SGLK_TR_STEP(8) SGLK_TR_STEP(9) SGLK_TR_STEP(10) SGLK_TR_STEP(11)
        SGLK_TR_STEP(12) SGLK_TR_STEP(13) SGLK_TR_STEP(14) SGLK_TR_STEP(15) SGLK_TR_STEP(16) SGLK_TR_STEP(17)
        SGLK_TR_STEP(18) SGLK_TR_STEP(19) SGLK_TR_STEP(20) SGLK_TR_STEP(21) SGLK_TR_STEP(22) SGLK_TR_STEP(23)
        SGLK_TR_STEP(24) SGLK_TR_STEP(25) SGLK_TR_STEP(26) SGLK_TR_STEP(27) SGLK_TR_STEP(28) SGLK_TR_STEP(29)
        SGLK_TR_STEP(30) SGLK_TR_STEP(31)
#undef SGLK_TR_STEP
#undef SGLK_TR_WAIT
#undef SGLK_TR_ISSUE
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    st ^= 1;
  }

  if (!active) return;
  // ---- epilogue. O tile nt: lane holds dim 16 (g0 + nt) + l15 of heads 4g + r; m_run / l_tot belong to head l15
  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
  if (p.splits > 1) {
    // unnormalised partial for the merge: (-inf, 0) and a zero O where this split saw no valid slot
    const int64_t row0 = ((int64_t)tok * p.splits + blockIdx.z) * p.H + head0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int head = hg * 16 + 4 * g + r;
      if (head < H) {
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) p.part_o[(row0 + head) * kLatent + (g0 + nt) * 16 + l15] = o[nt][r];
      }
    }
    if (ww == 0 && lane < 16 && hg * 16 + lane < H) {
      p.part_ml[(row0 + hg * 16 + lane) * 2] = m_run;
      p.part_ml[(row0 + hg * 16 + lane) * 2 + 1] = l_tot;
    }
    return;
  }
  bf16* out = p.out + ((int64_t)tok * p.H + head0) * kLatent;
  const bool lonely = m_run == -INFINITY;  // no valid slot: out = 0 whatever the sink says
  float sink_term = 0.f;
  if (attn_sink != nullptr && !lonely) {
    const int head = hg * 16 + l15;
    const float sink = attn_sink[head0 + (head < H ? head : 0)];
    sink_term = __builtin_amdgcn_exp2f(sink * 1.4426950408889634f - m_run * p.scale_log2);  // +inf sink: inf -> out 0
  }
  const float inv_l = lonely ? 0.f : 1.0f / (l_tot + sink_term);
  const v4f i4 = {head_bcast(inv_l, 0), head_bcast(inv_l, 1), head_bcast(inv_l, 2), head_bcast(inv_l, 3)};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int head = hg * 16 + 4 * g + r;
    if (head < H) {
#pragma unroll
      for (int nt = 0; nt < kNT; ++nt) out[(int64_t)head * kLatent + (g0 + nt) * 16 + l15] = (bf16)(o[nt][r] * i4[r]);
    }
  }
  if (ww == 0 && lane < 16 && hg * 16 + lane < H) {
    const int head = head0 + hg * 16 + lane;
    p.lse[((int64_t)b * p.H + head) * p.s_q + sq] =
        lonely ? INFINITY : (m_run * p.scale_log2 + log2f(l_tot)) * 0.6931471805599453f;
  }
}

// Merge of the slot splits: one workgroup per (token, head), 4 output columns a thread.
__global__ __launch_bounds__(kCombineThreads) void mla_sparse_decode_combine_kernel(DecodeParams p,
                                                                                    const float* __restrict__ attn_sink) {
  const int64_t th = blockIdx.x;  // tok * H + head
  const int tok = (int)(th / p.H), head = (int)(th - (int64_t)tok * p.H);
  const int b = tok / p.s_q, sq = tok - b * p.s_q;
  const int64_t row0 = (int64_t)tok * p.splits * p.H + head;  // + z * H
  float m = -INFINITY;
  for (int z = 0; z < p.splits; ++z) m = fmaxf(m, p.part_ml[(row0 + (int64_t)z * p.H) * 2]);
  const int col = threadIdx.x * 4;
  bf16* out = p.out + th * kLatent + col;
  if (m == -INFINITY) {  // no split saw a valid slot
    *reinterpret_cast<v2i*>(out) = (v2i){0, 0};
    if (threadIdx.x == 0) p.lse[((int64_t)b * p.H + head) * p.s_q + sq] = INFINITY;
    return;
  }
  v4f acc = {0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  for (int z = 0; z < p.splits; ++z) {
    const int64_t row = row0 + (int64_t)z * p.H;
    const float w = __builtin_amdgcn_exp2f((p.part_ml[row * 2] - m) * p.scale_log2);  // an empty split: exp2(-inf) = 0
    l += w * p.part_ml[row * 2 + 1];
    const v4f x = *reinterpret_cast<const v4f*>(p.part_o + row * kLatent + col);
    acc += w * x;
  }
  float sink_term = 0.f;
  if (attn_sink != nullptr) sink_term = __builtin_amdgcn_exp2f(attn_sink[head] * 1.4426950408889634f - m * p.scale_log2);
  const float inv_l = 1.0f / (l + sink_term);
  v4s r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = cvt_bf16(acc[i] * inv_l);
  *reinterpret_cast<v4s*>(out) = r;
  if (threadIdx.x == 0)
    p.lse[((int64_t)b * p.H + head) * p.s_q + sq] = (m * p.scale_log2 + log2f(l)) * 0.6931471805599453f;
}

template <int W>
static int launch_w(hipStream_t st, const DecodeParams& p, int64_t tokens, const void* q, const float* attn_sink) {
  static unsigned long long attr_done = 0;
  constexpr int lds = kPartOff + (W == 1 ? 0 : 8 * 2048);
  if (int rc = set_max_dyn_lds(reinterpret_cast<const void*>(&mla_sparse_decode_kernel<W>), lds, &attr_done,
                               "flash_mla_sparse_decode"))
    return rc;
  const dim3 grid((unsigned)tokens, (p.H + kHeadBlock - 1) / kHeadBlock, p.splits);
  mla_sparse_decode_kernel<W><<<grid, kThreads, lds, st>>>(p, (const bf16*)q, attn_sink);
  return check_launch("flash_mla_sparse_decode");
}

static int64_t nominal_tiles(int64_t topk, int64_t extra_topk) { return cdiv(topk, kTile) + cdiv(extra_topk, kTile); }

static int64_t resolve_splits(int64_t num_splits, int64_t tokens, int64_t num_heads, int64_t topk, int64_t extra_topk) {
  int64_t s = num_splits < 1 ? sglk_mla_sparse_decode_auto_splits(tokens, cdiv(num_heads, kHeadBlock), topk + extra_topk)
                             : num_splits;
  const int64_t tiles = nominal_tiles(topk, extra_topk);
  if (s > tiles) s = tiles;
  return s < 1 ? 1 : s;
}

static int log2_or_neg(int64_t v) {
  for (int s = 0; s < 31; ++s)
    if (v == (int64_t)1 << s) return s;
  return -1;
}

}  // namespace
}  // namespace sglk

// One workgroup a CU is what 64 and 128 heads run at (two from 32 heads down): fill the CUs once, but keep at least 4
// tiles (128 slots) a split so that a split's prologue and the merge stay small next to its walk.
extern "C" int64_t sglk_mla_sparse_decode_auto_splits(int64_t tokens, int64_t head_blocks, int64_t slots) {
  const int64_t wgs = (tokens > 0 ? tokens : 1) * (head_blocks > 0 ? head_blocks : 1);
  const int64_t tiles = (slots + 31) / 32;
  int64_t s = 256 / wgs;
  const int64_t cap = tiles / 4;
  if (s > cap) s = cap;
  if (s > 64) s = 64;
  return s < 1 ? 1 : s;
}

extern "C" int64_t sglk_mla_sparse_decode_workspace_size(int64_t tokens, int64_t num_heads, int64_t topk,
                                                         int64_t extra_topk, int64_t num_splits) {
  if (tokens <= 0 || num_heads <= 0 || topk < 0 || extra_topk < 0) return 0;
  const int64_t s = sglk::resolve_splits(num_splits, tokens, num_heads, topk, extra_topk);
  return s == 1 ? 0 : tokens * s * num_heads * (sglk::kLatent + 2) * 4;
}

extern "C" int sglk_flash_mla_sparse_decode(sglk_stream_t stream, void* out, float* lse, const void* q, const void* k_cache,
                                            const int32_t* indices, const int32_t* topk_length, const void* extra_k_cache,
                                            const int32_t* extra_indices, const int32_t* extra_topk_length,
                                            const float* attn_sink, void* workspace, int64_t workspace_bytes,
                                            int64_t batch, int64_t s_q, int64_t num_heads, int64_t topk, int64_t extra_topk,
                                            int64_t q_stride_b, int64_t q_stride_s, int64_t q_stride_h, int64_t num_pages,
                                            int64_t page_size, int64_t page_bytes, int64_t extra_num_pages,
                                            int64_t extra_page_size, int64_t extra_page_bytes, float sm_scale,
                                            int64_t num_splits) {
  using namespace sglk;
  const char* who = "flash_mla_sparse_decode";
  SGLK_REQUIRE(batch >= 0 && s_q >= 1 && batch * s_q < (int64_t)1 << 31, "%s: bad batch %lld or s_q %lld", who,
               (long long)batch, (long long)s_q);
  SGLK_REQUIRE(num_heads > 0 && num_heads <= 128 * 65535 && batch * s_q * num_heads < (int64_t)1 << 31,
               "%s: bad head count %lld", who, (long long)num_heads);
  SGLK_REQUIRE(topk >= 0 && extra_topk >= 0 && topk + extra_topk < (int64_t)1 << 31,
               "%s: topk and extra_topk must be in [0, 2^31), got %lld and %lld", who, (long long)topk, (long long)extra_topk);
  SGLK_REQUIRE(sm_scale > 0.f, "%s: sm_scale must be positive, got %g", who, (double)sm_scale);
  SGLK_REQUIRE(q_stride_b % 8 == 0 && q_stride_s % 8 == 0 && q_stride_h % 8 == 0 && (uintptr_t)q % 16 == 0,
               "%s: q rows must be 16-byte aligned", who);
  SGLK_REQUIRE((extra_k_cache != nullptr) == (extra_indices != nullptr) && (extra_k_cache != nullptr || extra_topk == 0) &&
                   (extra_k_cache != nullptr || extra_topk_length == nullptr),
               "%s: extra_k_cache and extra_indices must be given together", who);
  SGLK_REQUIRE(indices != nullptr || topk == 0, "%s: indices missing", who);
  const bool extra = extra_k_cache != nullptr;
  for (int w = 0; w < (extra ? 2 : 1); ++w) {
    const void* base = w ? extra_k_cache : k_cache;
    const int64_t np = w ? extra_num_pages : num_pages, ps = w ? extra_page_size : page_size,
                  pb = w ? extra_page_bytes : page_bytes;
    SGLK_REQUIRE(base != nullptr && (uintptr_t)base % 16 == 0, "%s: cache %d must be 16-byte aligned", who, w);
    SGLK_REQUIRE(np >= 0 && ps >= 1 && np * ps < (int64_t)1 << 31, "%s: cache %d: bad page count %lld or page size %lld",
                 who, w, (long long)np, (long long)ps);
    SGLK_REQUIRE(pb >= 584 * ps && pb % 16 == 0,
                 "%s: cache %d: a page of %lld tokens needs at least %lld bytes, a multiple of 16; got %lld", who, w,
                 (long long)ps, (long long)(584 * ps), (long long)pb);
  }
  const int64_t tokens = batch * s_q;
  if (tokens == 0) return SGLK_OK;
  const int64_t splits = resolve_splits(num_splits, tokens, num_heads, topk, extra_topk);
  SGLK_REQUIRE(splits <= 65535, "%s: at most 65535 slot splits, got %lld", who, (long long)splits);
  const int64_t part_rows = tokens * splits * num_heads;
  if (splits > 1) {
    SGLK_REQUIRE(workspace != nullptr && (uintptr_t)workspace % 16 == 0 && workspace_bytes >= part_rows * (kLatent + 2) * 4,
                 "%s: %lld splits need a 16-byte aligned workspace of %lld bytes, got %lld", who, (long long)splits,
                 (long long)(part_rows * (kLatent + 2) * 4), (long long)workspace_bytes);
  }
  DecodeParams p;
  p.out = (bf16*)out;
  p.lse = lse;
  p.part_o = (float*)workspace;
  p.part_ml = p.part_o ? p.part_o + part_rows * kLatent : nullptr;
  for (int w = 0; w < 2; ++w) {
    const bool have = w == 0 || extra;
    const int64_t ps = !have ? 1 : w ? extra_page_size : page_size;
    p.cache[w].base = (const char*)(!have ? k_cache : w ? extra_k_cache : k_cache);
    p.cache[w].page_bytes = !have ? 0 : w ? extra_page_bytes : page_bytes;
    p.cache[w].scale_off = kRowBytes * ps;
    p.cache[w].page_size = (int)ps;
    p.cache[w].shift = log2_or_neg(ps);
    p.cache[w].ntok = !have ? 0 : (int)((w ? extra_num_pages : num_pages) * ps);
  }
  p.idx[0] = indices;
  p.idx[1] = extra ? extra_indices : indices;
  p.len[0] = topk_length;
  p.len[1] = extra ? extra_topk_length : nullptr;
  p.topk[0] = (int)topk;
  p.topk[1] = extra ? (int)extra_topk : 0;
  p.q_sb = q_stride_b;
  p.q_ss = q_stride_s;
  p.q_sh = q_stride_h;
  p.H = (int)num_heads;
  p.s_q = (int)s_q;
  p.splits = (int)splits;
  p.scale_log2 = sm_scale * 1.4426950408889634f;
  hipStream_t st = (hipStream_t)stream;
  const int ngroups = (int)((num_heads < kHeadBlock ? num_heads : kHeadBlock) + 15) >> 4;
  int rc;
  if (ngroups <= 1) rc = launch_w<8>(st, p, tokens, q, attn_sink);
  else if (ngroups <= 2) rc = launch_w<4>(st, p, tokens, q, attn_sink);
  else if (ngroups <= 4) rc = launch_w<2>(st, p, tokens, q, attn_sink);
  else rc = launch_w<1>(st, p, tokens, q, attn_sink);
  if (rc != SGLK_OK || splits == 1) return rc;
  mla_sparse_decode_combine_kernel<<<(unsigned)(tokens * num_heads), kCombineThreads, 0, st>>>(p, attn_sink);
  return check_launch("flash_mla_sparse_decode (merge)");
}
