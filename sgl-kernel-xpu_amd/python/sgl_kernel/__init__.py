"""sgl_kernel for AMD Instinct MI355X (gfx950).

Same module and function names as reference python/sgl_kernel/__init__.py:14-184
for the hot path; every op dispatches through torch.ops.sgl_kernel.* (registered
by the `common_ops` extension at import) into hand-written HIP kernels behind
the C-ABI of include/sglk.h. There is no CPU or eager fallback: if the
extension is missing the import fails.
"""
import os as _os

import torch as _torch  # noqa: F401  (loads the HIP runtime the extension binds to)

_here = _os.path.dirname(_os.path.abspath(__file__))
if not any(f.startswith("common_ops") and f.endswith(".so") for f in _os.listdir(_here)):
    raise ImportError(
        "sgl_kernel: the HIP extension common_ops*.so is not built; run "
        "`python sgl-kernel-xpu_amd/build.py` (or __graft_entry__.build())."
    )

from sgl_kernel import common_ops  # noqa: E402,F401  (TORCH_LIBRARY registration happens at dlopen)
from sgl_kernel.attention import (  # noqa: E402
    flash_mla_decode,
    flash_mla_get_workspace_size,
    flash_mla_prefill,
    flash_mla_prefill_get_workspace_size,
    flash_mla_sparse_fwd,
    flash_mla_with_kvcache,
    merge_state,
    merge_state_v2,
)
from sgl_kernel.elementwise import (  # noqa: E402
    fused_add_rmsnorm,
    fused_inplace_qknorm_rope,
    fused_qk_norm_rope,
    gelu_and_mul,
    gelu_tanh_and_mul,
    gemma_fused_add_rmsnorm,
    gemma_rmsnorm,
    rmsnorm,
    rotary_embedding,
    silu_and_mul,
    silu_and_mul_clamp,
    store_cache,
    store_cache_xpu,
)
from sgl_kernel.flash_attn import flash_attn_varlen_func, flash_attn_with_kvcache, is_fa3_supported  # noqa: E402
from sgl_kernel.gemm import (  # noqa: E402
    awq_dequantize,
    sgl_per_tensor_quant_fp8,
    sgl_per_token_quant_fp8,
    fp8_blockwise_scaled_mm,
    fp8_scaled_mm,
    int8_scaled_mm,
    qserve_w4a8_per_chn_gemm,
    qserve_w4a8_per_group_gemm,
    sgl_per_token_group_quant_8bit,
    sgl_per_token_group_quant_fp8,
    sgl_per_token_group_quant_int8,
)
from sgl_kernel.moe import (  # noqa: E402
    apply_shuffle_mul_sum,
    biased_topk,
    fp8_blockwise_scaled_grouped_mm,
    fused_experts,
    swiglu_gpt_oss_sigmoid_alpha,
    moe_align_block_size,
    moe_fused_gate,
    prepare_moe_input,
    scatter_tokens_to_experts,
    topk_sigmoid,
    topk_softmax,
)
from sgl_kernel.nsa import fp8_mqa_logits, fp8_paged_mqa_logits, fp8_paged_mqa_logits_triton  # noqa: E402
from sgl_kernel.sampling import (  # noqa: E402
    min_p_sampling_from_probs,
    top_k_renorm_prob,
    top_k_renorm_probs,
    top_k_top_p_sampling_from_probs,
    top_p_renorm_prob,
    top_p_renorm_probs,
    top_p_sampling_from_probs,
)
from sgl_kernel.top_k import (  # noqa: E402
    fast_topk_transform_fused,
    fast_topk_transform_ragged_fused,
    fast_topk_v2,
    topk_transform_512,
    topk_transform_512_v2,
)
from sgl_kernel.utils import get_device_capability, is_gfx950_arch, is_xe2_arch  # noqa: E402
from sgl_kernel.version import __version__  # noqa: E402

# Public names of the reference package (python/sgl_kernel/__init__.py:14-184) that are outside the MI355X hot path
# (SURVEY.md section 2.3 / 8(b)(3)): every one of them imports and resolves lazily to a stub that raises on call, so
# `from sgl_kernel import X` keeps working for callers that never use X. The list is the reference's export list minus
# what this package implements; tests/test_reference_exports.py diffs it against the reference (and against the committed
# copy of that list, tests/golden/reference_exports.txt, where the reference tree is absent).
_OUT_OF_SCOPE = frozenset(
    """
    apply_rope_with_cos_sin_cache_inplace apply_token_bitmask_inplace_cuda bmm_fp8
    build_tree_kernel_efficient causal_conv1d causal_conv1d_fn_xpu causal_conv1d_update_xpu
    compile_inkling_attn_prologue compress_norm_rope_store convert_vertical_slash_indexes
    convert_vertical_slash_indexes_mergehead cutlass_fp4_group_mm cutlass_scaled_fp4_mm
    embedding_lora_a_fwd
    flash_compress128_decode flash_compress128_prefill flash_compress4_decode
    flash_compress4_prefill
    fused_causal_conv1d_update_decode fused_decode_sconv_metadata
    fused_draft_extend_sconv_cache fused_extend_sconv_metadata
    fused_gather_scatter_to_sconv_cache fused_k_norm_rope_flashmla
    fused_q_indexer_rope_hadamard_quant fused_q_norm_rope fused_qk_rope
    fused_qk_rope_with_cos_sin_cache_inplace gdn_attention hadamard_transform hash_topk hc_post
    hc_pre_big_fuse hc_pre_gemm_sqr_sum hc_split_sinkhorn inkling_attn_prologue_decode
    inkling_attn_prologue_extend inkling_attn_prologue_verify lightning_attention_decode mhc_pre
    moe_sum moe_sum_reduce multimodal_rotary_embedding plan_compress_decode
    plan_compress_decode_legacy plan_compress_prefill plan_compress_prefill_legacy
    precompute_helion_decode_metadata precompute_helion_extend_metadata qkv_lora_b_fwd
    save_intermediate_conv_windows scaled_fp4_experts_quant scaled_fp4_quant segment_packbits
    sgemm_lora_a_fwd sgemm_lora_b_fwd sgl_per_token_group_quant_fp4 sparse_attn_func
    sparse_attn_varlen_func track_conv_indices
    transfer_kv_all_layer transfer_kv_all_layer_direct_lf_pf transfer_kv_all_layer_lf_pf
    transfer_kv_all_layer_lf_ph transfer_kv_all_layer_mla transfer_kv_all_layer_mla_lf_pf
    transfer_kv_direct transfer_kv_per_layer transfer_kv_per_layer_direct_pf_lf
    transfer_kv_per_layer_mla transfer_kv_per_layer_mla_pf_lf transfer_kv_per_layer_pf_lf
    transfer_kv_per_layer_ph_lf tree_speculative_sampling_target_only update_sconv_cache
    verify_tree_greedy weak_ref_tensor
    """.split()
)


def __getattr__(name):
    if name in _OUT_OF_SCOPE:

        def _stub(*args, **kwargs):
            raise NotImplementedError(
                f"sgl_kernel.{name} is outside the MI355X hot path of this build (see DESIGN.md)"
            )

        _stub.__name__ = name
        return _stub
    raise AttributeError(f"module 'sgl_kernel' has no attribute {name!r}")
