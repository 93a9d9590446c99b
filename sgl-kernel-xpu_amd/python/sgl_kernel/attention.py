"""Multi-head latent attention (DeepSeek MLA) over a paged latent cache: decode and ragged prefill.

Contract (reference python/sgl_kernel/attention.py): the public names and parameters of `flash_mla_decode`
(:54-62), `flash_mla_get_workspace_size` (:128-146), `flash_mla_prefill` (:149-161) and
`flash_mla_prefill_get_workspace_size` (:236-247), `flash_mla_with_kvcache` (:250-353) and `flash_mla_sparse_fwd` (:356-397); latent width 512 + rope width 64, at most 128 heads, 16-bit
dtypes, int32 `seq_lens` / `page_table` (:77-111); a page table whose width covers whole 128-token spans (:101);
output [rows, heads, 512] in the query dtype (:113-119); the op argument order of
src/torch_extension_sycl.cc:364-383.

Deliberate differences: q_nope / q_pe are handed to the kernel with their strides (only a non-unit innermost
stride is copied), the reference's pad-to-128-heads CUDA branch (:86-93) and its 256-row output padding for
prefill (:212-217: its epilogue writes whole tiles, this one writes exactly total_q rows) do not exist here.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

LATENT_DIM = 512
ROPE_DIM = 64
MAX_HEADS = 128
_HALF_TYPES = (torch.float16, torch.bfloat16)

_ops = torch.ops.sgl_kernel  # (patched by the host-logic tests)


@dataclass(frozen=True)
class _MlaShapes:
    rows: int  # batch (decode) or total query tokens (prefill)
    heads: int
    page_size: int


def _check_operands(who, q_nope, q_pe, cache) -> _MlaShapes:
    """Rank / width / dtype rules shared by decode and prefill."""
    for name, t in (("q_nope", q_nope), ("q_pe", q_pe), ("kv_c_and_k_pe_cache", cache)):
        assert t.ndim == 3, f"{who}: {name} must be a 3D tensor, but got {t.ndim}"
    rows, heads, d_nope = q_nope.shape
    assert q_pe.shape[:2] == (rows, heads), f"{who}: q_nope {tuple(q_nope.shape)} and q_pe {tuple(q_pe.shape)} disagree"
    assert d_nope == LATENT_DIM, f"{who}: q_nope last dim must be {LATENT_DIM}, got {d_nope}"
    assert q_pe.shape[2] == ROPE_DIM, f"{who}: q_pe last dim must be {ROPE_DIM}, got {q_pe.shape[2]}"
    assert cache.shape[2] == LATENT_DIM + ROPE_DIM, (
        f"{who}: cache rows must be {LATENT_DIM} + {ROPE_DIM} wide, got {cache.shape[2]}")
    assert heads <= MAX_HEADS, f"{who}: H must be <= {MAX_HEADS}, but got {heads}"
    assert q_nope.dtype in _HALF_TYPES, f"{who}: q_nope.dtype needs to be fp16 or bf16 but got {q_nope.dtype}."
    assert q_nope.dtype == q_pe.dtype == cache.dtype, f"{who}: q_nope, q_pe and the cache must share one dtype"
    return _MlaShapes(rows, heads, cache.shape[1])


def _check_int32(who, **tensors):
    for name, t in tensors.items():
        assert t.dtype == torch.int32, f"{who}: {name}.dtype needs to be int32 but got {t.dtype}."


def _check_positive(who, **values):
    for name, v in values.items():
        assert v > 0, f"{who}: {name} must be greater than 0, got {v}"


def _merge(op_name, v_a, s_a, v_b, s_b, v_merged, s_merged):
    s_a, s_b = s_a.to(torch.float32), s_b.to(torch.float32)
    v_merged = torch.empty_like(v_a) if v_merged is None else v_merged
    s_merged = torch.empty_like(s_a) if s_merged is None else s_merged
    getattr(_ops, op_name).default(v_a, s_a, v_b, s_b, v_merged, s_merged)
    return v_merged, s_merged


def merge_state(v_a: torch.Tensor, s_a: torch.Tensor, v_b: torch.Tensor, s_b: torch.Tensor,
                v_merged: Optional[torch.Tensor] = None,
                s_merged: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge two partial attention states over disjoint key sets: v [tokens, heads, d] normalised outputs, s
    [tokens, heads] log-sum-exp in BASE 2 (the flashinfer convention; reference attention.py:12-28). Outputs are
    allocated unless given."""
    return _merge("merge_state", v_a, s_a, v_b, s_b, v_merged, s_merged)


def merge_state_v2(v_a: torch.Tensor, s_a: torch.Tensor, v_b: torch.Tensor, s_b: torch.Tensor,
                   v_merged: Optional[torch.Tensor] = None,
                   s_merged: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The same merge with natural-log s (what `fwd` returns as softmax_lse; reference attention.py:31-51)."""
    return _merge("merge_state_v2", v_a, s_a, v_b, s_b, v_merged, s_merged)


def _inner_unit_stride(t):
    return t if t.stride(-1) == 1 else t.contiguous()


def flash_mla_decode(q_nope: torch.Tensor, q_pe: torch.Tensor, kv_c_and_k_pe_cache: torch.Tensor,
                     seq_lens: torch.Tensor, page_table: torch.Tensor, workspace: torch.Tensor, sm_scale: float,
                     num_kv_splits: int = 1) -> torch.Tensor:
    """One query token per sequence: out[b, h, :] = softmax(sm_scale * [q_nope, q_pe][b, h] . cache[b]^T) . cache[b][:, :512]
    over the first seq_lens[b] tokens of the pages page_table[b] names. `workspace`: uint8 scratch of
    flash_mla_get_workspace_size(...) bytes (split-KV partials)."""
    who = "flash_mla_decode"
    sh = _check_operands(who, q_nope, q_pe, kv_c_and_k_pe_cache)
    assert page_table.ndim == 2 and page_table.shape[0] == sh.rows, (
        f"{who}: page_table must be [batch={sh.rows}, pages], got {tuple(page_table.shape)}")
    pages = page_table.shape[1]
    assert pages > 0, f"{who}: block num must be greater than 0, got {pages}"
    assert (pages * sh.page_size) % 128 == 0, (
        f"{who}: the page table must cover whole 128-token spans ({pages} pages of {sh.page_size})")
    _check_int32(who, seq_lens=seq_lens, page_table=page_table)

    out = q_nope.new_empty((sh.rows, sh.heads, LATENT_DIM))
    _ops.flash_mla_decode.default(out, _inner_unit_stride(q_nope), _inner_unit_stride(q_pe), kv_c_and_k_pe_cache,
                                  seq_lens, page_table, workspace, sm_scale, num_kv_splits)
    return out


def flash_mla_get_workspace_size(max_seq_len: int, num_batches: int, num_heads: int = 0, page_size: int = 0,
                                 num_kv_splits: int = -1) -> int:
    _check_positive("flash_mla_get_workspace_size", max_seq_len=max_seq_len, num_batches=num_batches)
    return _ops.flash_mla_get_workspace_size.default(max_seq_len, num_batches, num_heads, page_size, num_kv_splits)


def flash_mla_prefill(q_nope: torch.Tensor, q_pe: torch.Tensor, kv_c_and_k_pe_cache: torch.Tensor,
                      cu_seqlens_q: torch.Tensor, seq_lens_k: torch.Tensor, max_seqlen_q: int,
                      page_table: torch.Tensor, workspace: torch.Tensor, sm_scale: float, causal: bool = True,
                      num_kv_splits: int = -1) -> torch.Tensor:
    """Ragged prefill: sequence i owns query rows cu_seqlens_q[i] : cu_seqlens_q[i+1] and the first seq_lens_k[i]
    cached tokens (its new tokens are the LAST ones: the causal mask is aligned bottom-right).
    Returns out [total_q, heads, 512]."""
    who = "flash_mla_prefill"
    sh = _check_operands(who, q_nope, q_pe, kv_c_and_k_pe_cache)
    _check_int32(who, cu_seqlens_q=cu_seqlens_q, seq_lens_k=seq_lens_k, page_table=page_table)
    batch = cu_seqlens_q.shape[0] - 1
    assert seq_lens_k.shape[0] == batch, f"{who}: seq_lens_k must hold one length per sequence ({batch})"

    out = q_nope.new_empty((sh.rows, sh.heads, LATENT_DIM))
    if sh.rows > 0:
        _ops.flash_mla_prefill.default(out, q_nope, q_pe, kv_c_and_k_pe_cache, cu_seqlens_q, seq_lens_k.contiguous(),
                                       max_seqlen_q, page_table, workspace, sm_scale, causal, num_kv_splits)
    return out


def flash_mla_prefill_get_workspace_size(max_seq_len: int, num_batches: int, num_heads: int = 0, page_size: int = 0,
                                         num_kv_splits: int = -1) -> int:
    """This library's prefill keeps everything on chip: the answer is 0 (the op is still asked, as the reference does)."""
    _check_positive("flash_mla_prefill_get_workspace_size", max_seq_len=max_seq_len, num_batches=num_batches)
    return _ops.flash_mla_prefill_get_workspace_size.default(max_seq_len, num_batches, num_heads, page_size, num_kv_splits)


def flash_mla_sparse_fwd(q: torch.Tensor, kv: torch.Tensor, indices: torch.Tensor, sm_scale: float, d_v: int = 512,
                         attn_sink: Optional[torch.Tensor] = None,
                         topk_length: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Sparse MLA prefill: token t attends to the kv rows indices[t, 0, :] names (reference attention.py:356-397).

    q [s_q, h_q, d_qk] and kv [s_kv, 1, d_qk] bf16 with d_qk 512 or 576, indices [s_q, 1, topk] int32. Slot j of token t
    is valid iff 0 <= indices[t, 0, j] < s_kv and (topk_length is None or j < topk_length[t]). Over the valid slots
    P = sm_scale * q[t, h] . kv[idx]; returns (out [s_q, h_q, 512] bf16, max_logits [s_q, h_q] f32 = max P, lse [s_q, h_q]
    f32 = ln sum exp P) with out = sum exp(P - lse') kv[idx][:512], lse' = logaddexp(lse, attn_sink[h]) where attn_sink
    (f32 [h_q]) is given (it changes neither lse nor max_logits). A token without a valid slot gets out = 0, lse = +inf,
    max_logits = -inf. Unlike the reference, kv rows that no valid slot names are never read."""
    who = "flash_mla_sparse_fwd"
    assert q.ndim == 3 and kv.ndim == 3 and indices.ndim == 3, f"{who}: q, kv and indices must be 3D tensors"
    s_q, h_q, d_qk = q.shape
    assert d_qk in (LATENT_DIM, LATENT_DIM + ROPE_DIM), f"{who}: d_qk must be 512 or 576, got {d_qk}"
    assert d_v == LATENT_DIM, f"{who}: d_v can only be {LATENT_DIM}, got {d_v}"
    assert kv.shape[1:] == (1, d_qk), f"{who}: kv must be [s_kv, 1, {d_qk}], got {tuple(kv.shape)}"
    assert indices.shape[:2] == (s_q, 1), f"{who}: indices must be [s_q={s_q}, 1, topk], got {tuple(indices.shape)}"
    assert q.dtype == kv.dtype == torch.bfloat16, f"{who}: q and kv must be bf16, got {q.dtype} and {kv.dtype}"
    _check_int32(who, indices=indices)
    if attn_sink is not None:
        assert attn_sink.dtype == torch.float32 and attn_sink.shape == (h_q,), f"{who}: attn_sink must be float32 [{h_q}]"
    if topk_length is not None:
        _check_int32(who, topk_length=topk_length)
        assert topk_length.shape == (s_q,), f"{who}: topk_length must be [{s_q}], got {tuple(topk_length.shape)}"

    out = q.new_empty((s_q, h_q, d_v))
    max_logits = q.new_empty((s_q, h_q), dtype=torch.float32)
    lse = q.new_empty((s_q, h_q), dtype=torch.float32)
    if s_q > 0:
        _ops.flash_mla_sparse_prefill.default(
            out, max_logits, lse, _inner_unit_stride(q), _inner_unit_stride(kv), _inner_unit_stride(indices), sm_scale, d_v,
            None if attn_sink is None else attn_sink.contiguous(), None if topk_length is None else topk_length.contiguous())
    return out, max_logits, lse


def flash_mla_with_kvcache(q: torch.Tensor, k_cache: torch.Tensor, block_table: Optional[torch.Tensor] = None,
                           cache_seqlens: Optional[torch.Tensor] = None, head_dim_v: int = 512,
                           tile_scheduler_metadata: Optional[torch.Tensor] = None,
                           num_splits: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None,
                           causal: bool = False, is_fp8_kvcache: bool = False, indices: Optional[torch.Tensor] = None,
                           attn_sink: Optional[torch.Tensor] = None, extra_k_cache: Optional[torch.Tensor] = None,
                           extra_indices_in_kvcache: Optional[torch.Tensor] = None,
                           topk_length: Optional[torch.Tensor] = None,
                           extra_topk_length: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Sparse MLA decode over the DeepSeek-V4 packed fp8 cache (reference attention.py:250-353).

    q [B, s_q, H, 512] bf16; indices [B, s_q, topk] and extra_indices_in_kvcache [B, s_q, extra_topk] int32; topk_length /
    extra_topk_length int32 [B] (per batch element); attn_sink f32 [H]. k_cache / extra_k_cache are
    [pages, page_size, 1, 584] float8_e4m3fn with stride(3) == 1 and stride(0) = the page size in bytes: token t of a page
    holds 448 e4m3 bytes (7 tiles of 64) + 64 bf16 of rope at byte 576 t and 7 UE8M0 scale bytes (+ 1 pad) at
    576 page_size + 8 t; its row is [e4m3 * 2^(scale - 127), rope], 512 columns, K and V at once. Token index i is slot
    i % page_size of page i // page_size; the two caches may differ in page size.

    The slot list of query (b, s) is indices[b, s] followed by extra_indices_in_kvcache[b, s]; a slot is valid iff its
    index lies inside its cache and in front of its list's length. Over the valid slots P = softmax_scale * q . row;
    returns (out [B, s_q, H, 512] bf16, lse [B, H, s_q] f32 = ln sum exp P) with out = sum exp(P - lse') row and
    lse' = logaddexp(lse, attn_sink[h]). A query without a valid slot gets out = 0 and lse = +inf: the value the
    reference's kernel writes and flash_mla_sparse_fwd returns (the reference's Python fallback leaves -inf there and
    never checks it). Cache tokens that no valid slot names are never read.

    Only this path exists: is_fp8_kvcache must be True, block_table raises NotImplementedError (the reference returns
    uninitialised memory there), tile_scheduler_metadata / num_splits / causal are refused as in the reference."""
    who = "flash_mla_with_kvcache"
    assert tile_scheduler_metadata is None, f"{who}: tile_scheduler_metadata is not supported"
    assert num_splits is None, f"{who}: num_splits is not supported"
    assert not causal, f"{who}: causal attention is not supported"
    if block_table is not None:
        raise NotImplementedError(f"{who}: the dense block_table path is not implemented; pass indices")
    assert is_fp8_kvcache, f"{who}: only the packed fp8 cache is implemented (is_fp8_kvcache must be True)"
    assert q.ndim == 4, f"{who}: q must be 4D [B, s_q, H, D_qk], got {q.ndim}D"
    assert k_cache.ndim == 4, f"{who}: k_cache must be 4D [num_pages, P, 1, D], got {k_cache.ndim}D"
    B, s_q, H, d_qk = q.shape
    assert q.dtype == torch.bfloat16, f"{who}: q.dtype must be bf16, got {q.dtype}"
    assert d_qk == LATENT_DIM and head_dim_v == LATENT_DIM, f"{who}: D_qk and head_dim_v must be {LATENT_DIM}"
    assert indices is not None, f"{who}: indices must be provided for the sparse decode path"
    if (extra_k_cache is None) != (extra_indices_in_kvcache is None):
        raise AssertionError(f"{who}: extra_k_cache and extra_indices_in_kvcache must be provided together")
    lists = {"indices": indices}
    if extra_indices_in_kvcache is not None:
        lists["extra_indices_in_kvcache"] = extra_indices_in_kvcache
    _check_int32(who, **lists)
    for name, t in lists.items():
        assert t.ndim == 3 and t.shape[:2] == (B, s_q), f"{who}: {name} must be [B={B}, s_q={s_q}, topk]"
    for name, t in (("topk_length", topk_length), ("extra_topk_length", extra_topk_length)):
        assert t is None or (t.dtype == torch.int32 and t.shape == (B,)), f"{who}: {name} must be int32 [{B}]"
    assert attn_sink is None or (attn_sink.dtype == torch.float32 and attn_sink.shape == (H,)), (
        f"{who}: attn_sink must be float32 [{H}]")
    if softmax_scale is None:
        softmax_scale = d_qk ** (-0.5)

    out = q.new_empty((B, s_q, H, head_dim_v))
    lse = q.new_empty((B, H, s_q), dtype=torch.float32)
    cont = lambda t: None if t is None else t.contiguous()
    _ops.flash_mla_sparse_decode.default(out, lse, _inner_unit_stride(q), k_cache, indices.contiguous(), cont(topk_length),
                                         extra_k_cache, cont(extra_indices_in_kvcache), cont(extra_topk_length),
                                         cont(attn_sink), softmax_scale, head_dim_v, is_fp8_kvcache)
    return out, lse
