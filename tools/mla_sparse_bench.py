"""flash_mla_sparse_fwd timing at the DeepSeek-V3.2 prefill shape (4096 query tokens, each over 2048 rows picked from a
16384-row latent buffer, d_qk = 576) for 16 / 64 / 128 heads, next to the dense yardstick: flash_mla_prefill, non-causal,
the same tokens and heads over 2048 page-contiguous keys per sequence. The two are timed interleaved; each figure is the
median of 5 device-event timings after 3 warm-up calls, and the whole comparison is repeated 3 times."""
import os, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "sgl-kernel-xpu_amd", "python"))
import sgl_kernel

dev = "cuda"
S_Q, S_KV, TOPK, PAGE = 4096, 16384, 2048, 64


def median_ms(f):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[2]


def case(H):
    g = torch.Generator(device=dev).manual_seed(H)
    q = torch.randn(S_Q, H, 576, device=dev, dtype=torch.bfloat16, generator=g)
    kv = torch.randn(S_KV, 1, 576, device=dev, dtype=torch.bfloat16, generator=g)
    # distinct random rows per token, as a top-k selection gives
    indices = torch.rand(S_Q, S_KV, device=dev, generator=g).topk(TOPK, dim=1).indices.int().view(S_Q, 1, TOPK).contiguous()
    sparse = lambda: sgl_kernel.flash_mla_sparse_fwd(q, kv, indices, 576 ** -0.5)
    # dense: 8 sequences of 512 tokens, each over its own 2048 cached keys
    nb = 8
    cache = kv.view(S_KV // PAGE, PAGE, 576)
    table = torch.arange(nb * TOPK // PAGE, device=dev, dtype=torch.int32).view(nb, TOPK // PAGE)
    qn, qp = q[..., :512], q[..., 512:].contiguous()
    cu = torch.arange(nb + 1, device=dev, dtype=torch.int32) * (S_Q // nb)
    sl = torch.full((nb,), TOPK, device=dev, dtype=torch.int32)
    ws = torch.empty(1, device=dev, dtype=torch.uint8)
    dense = lambda: sgl_kernel.flash_mla_prefill(qn, qp, cache, cu, sl, S_Q // nb, table, ws, 576 ** -0.5, False)
    flop = 2.0 * S_Q * H * (576 + 512) * TOPK
    for rnd in range(3):
        ms_s, ms_d = median_ms(sparse), median_ms(dense)
        print(f"H={H}: sparse {ms_s:.4f} ms ({flop / ms_s / 1e9:.1f} TFLOP/s)  dense {ms_d:.4f} ms "
              f"({flop / ms_d / 1e9:.1f} TFLOP/s)  ratio {ms_s / ms_d:.3f}", flush=True)


for H in (16, 64, 128):
    case(H)
