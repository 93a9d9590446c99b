"""Indexer scores of DeepSeek-V3.2's sparse attention (same signatures as reference python/sgl_kernel/nsa.py:112-185 and
fp8_paged_mqa_logits.py:82):

    logits[i, j] = k_scale[j] * sum_h weights[i, h] * relu(q[i, h, :] . k[j, :])   inside the query's key window, 0 outside

Both forms run one fused HIP kernel (csrc/mqa_logits.hip). The result is always written in full, with zeros (not -inf)
outside the window, so `clean_logits` and `schedule_metadata` are accepted and ignored.
"""
from typing import Any, Optional, Tuple

import torch

_FP8 = (torch.uint8, torch.float8_e4m3fn)


def _bytes(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype not in _FP8:
        raise TypeError(f"{name} must be uint8 or float8_e4m3fn, got {t.dtype}")
    return t.contiguous()


def fp8_mqa_logits(
    q_fp8: torch.Tensor,
    kv_fp8: Tuple[torch.Tensor, torch.Tensor],
    weights: torch.Tensor,
    ks: torch.Tensor,
    ke: torch.Tensor,
    clean_logits: bool = False,
) -> torch.Tensor:
    """Ragged (prefill / extend) form. q_fp8 (Nq, H, 128) e4m3; kv_fp8 = (k_fp8 (Nk, 128) e4m3, k_scale (Nk,) float32);
    weights (Nq, H) float32; query i sees the keys [ks[i], ke[i]) (int32). Returns (Nq, Nk) float32."""
    k_fp8, k_scale = kv_fp8
    return torch.ops.sgl_kernel.fp8_mqa_logits.default(
        _bytes(q_fp8, "q_fp8"), _bytes(k_fp8, "k_fp8"), k_scale.reshape(-1).contiguous(), weights.contiguous(),
        ks.contiguous(), ke.contiguous())


def _paged(q_fp8, kv_cache, weights, seq_lens, block_tables, max_seq_len, block_layout):
    if not kv_cache.is_contiguous():  # (never copied: a cache is gigabytes, and this runs every decode step)
        raise ValueError("kv_cache must be contiguous")
    q_fp8 = _bytes(q_fp8, "q_fp8")
    if q_fp8.dim() == 3:
        q_fp8 = q_fp8.unsqueeze(1)
    if q_fp8.dim() != 4 or q_fp8.shape[1] != 1:
        raise ValueError(f"q_fp8 must be (B, H, D) or (B, 1, H, D), got {tuple(q_fp8.shape)}")
    if seq_lens.dim() > 1:
        seq_lens = seq_lens.reshape(-1)
    return torch.ops.sgl_kernel.fp8_paged_mqa_logits.default(
        q_fp8, _bytes(kv_cache, "kv_cache"), weights.contiguous(), seq_lens.contiguous(), block_tables, None,
        int(max_seq_len), False, block_layout)


def fp8_paged_mqa_logits(
    q_fp8: torch.Tensor,
    kv_cache: torch.Tensor,
    weights: torch.Tensor,
    seq_lens: torch.Tensor,
    block_tables: torch.Tensor,
    schedule_metadata: Optional[torch.Tensor],
    max_seq_len: int,
    clean_logits: bool = False,
) -> torch.Tensor:
    """Paged (decode) form over the ROW layout: token t of page p is the (D + 4)-byte row p * page_size + t of kv_cache
    (num_pages, page_size, 1, D + 4), 128 key bytes followed by its float32 scale. q_fp8 (B, 1, H, D) or (B, H, D);
    weights (B, H) float32; seq_lens (B,) or (B, 1) int32; block_tables (B, max_blocks) int32. Returns
    (B, max_seq_len) float32."""
    return _paged(q_fp8, kv_cache, weights, seq_lens, block_tables, max_seq_len, False)


def fp8_paged_mqa_logits_triton(
    q_fp8: torch.Tensor,
    kvcache_fp8: torch.Tensor,
    weight: torch.Tensor,
    seq_lens: torch.Tensor,
    page_table: torch.Tensor,
    deep_gemm_metadata: Any,
    max_seq_len: int,
    clean_logits: bool = False,
) -> torch.Tensor:
    """The same over the BLOCK layout of SGLang's V3.2 cache: inside a page of page_size * (D + 4) bytes all
    page_size * D key bytes come first, then page_size float32 scales. A HIP kernel here, whatever the name says."""
    return _paged(q_fp8, kvcache_fp8, weight, seq_lens, page_table, max_seq_len, True)
