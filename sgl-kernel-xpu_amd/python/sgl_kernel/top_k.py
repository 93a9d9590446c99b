"""Top-k selection behind the DeepSeek-V3.2 indexer scores (same signatures as reference python/sgl_kernel/top_k.py).

For score row b the window is score[b, rs : rs + len] with rs = row_starts[b] (0 without row_starts) and len = lengths[b];
the `topk` largest elements are selected EXACTLY (ties at the k-th value: lowest indices), their window-relative indices
p are mapped and written in an unspecified but reproducible order. len <= topk: slot i < len maps i, later slots are -1.
All five run one HIP kernel (csrc/topk_select.hip); the scores behind it carry zeros, not -inf, outside the window
(sgl_kernel.nsa), which is why the window is given by position.
"""
from typing import Optional

import torch

_TOPK = 2048


def _prepare(name: str, score: torch.Tensor, lengths: torch.Tensor, topk: int):
    if topk != _TOPK:
        raise ValueError(f"{name} only supports topk={_TOPK}, got {topk}")
    if score.dim() != 2:
        raise ValueError(f"{name}: score must be 2-D, got {tuple(score.shape)}")
    return score.new_empty((score.shape[0], topk), dtype=torch.int32), lengths.reshape(-1)


def fast_topk_v2(
    score: torch.Tensor, lengths: torch.Tensor, topk: int, row_starts: Optional[torch.Tensor] = None
) -> torch.Tensor:
    """score (B, L) float32, lengths (B,) int32, row_starts (B,) int32 or None -> (B, topk) int32: p."""
    out, lengths = _prepare("fast_topk_v2", score, lengths, topk)
    torch.ops.sgl_kernel.fast_topk.default(score, out, lengths, row_starts)
    return out


def fast_topk_transform_fused(
    score: torch.Tensor,
    lengths: torch.Tensor,
    page_table_size_1: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    topk: int,
    row_starts: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """-> page_table_size_1[s, p] (a page table of page size 1). Decode form (row_starts None and a table row per score
    row): s = b. Otherwise s is the sequence with cu_seqlens_q[s] <= b < cu_seqlens_q[s + 1] (int32, table rows + 1)."""
    out, lengths = _prepare("fast_topk_transform_fused", score, lengths, topk)
    torch.ops.sgl_kernel.fast_topk_transform_fused.default(score, lengths, out, page_table_size_1, cu_seqlens_q, row_starts)
    return out


def fast_topk_transform_ragged_fused(
    score: torch.Tensor,
    lengths: torch.Tensor,
    topk_indices_offset: torch.Tensor,
    topk: int,
    row_starts: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """-> p + topk_indices_offset[b]: indices into a ragged (unpaged) key / value buffer."""
    out, lengths = _prepare("fast_topk_transform_ragged_fused", score, lengths, topk)
    torch.ops.sgl_kernel.fast_topk_transform_ragged_fused.default(score, lengths, out, topk_indices_offset, row_starts)
    return out


def topk_transform_512(
    scores: torch.Tensor,
    seq_lens: torch.Tensor,
    page_tables: torch.Tensor,
    out_page_indices: torch.Tensor,
    page_size: int,
    out_raw_indices: Optional[torch.Tensor] = None,
) -> None:
    """Window [0, seq_lens[b]); topk = out_page_indices.shape[1] (1..2048); page_size a power of two. Writes
    (page_tables[b, p // page_size] * page_size) | (p % page_size) to out_page_indices and p to out_raw_indices."""
    torch.ops.sgl_kernel.topk_transform_512.default(
        scores, seq_lens.reshape(-1), page_tables, out_page_indices, page_size, out_raw_indices)


def topk_transform_512_v2(
    scores: torch.Tensor,
    seq_lens: torch.Tensor,
    page_tables: torch.Tensor,
    out_page_indices: torch.Tensor,
    page_size: int,
    metadata: torch.Tensor,
    out_raw_indices: Optional[torch.Tensor] = None,
) -> None:
    """topk_transform_512 with the reference's scheduling `metadata`, which this kernel does not need."""
    torch.ops.sgl_kernel.topk_transform_512_v2.default(
        scores, seq_lens.reshape(-1), page_tables, out_page_indices, page_size, metadata, out_raw_indices)
