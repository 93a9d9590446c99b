"""flash_mla_with_kvcache timing at DeepSeek-V4 decode shapes: 64 heads, one query token per sequence, 128 slots of the main
fp8 cache (page size 256) plus 512 or 8256 slots of the extra cache (page size 64), batch 1 / 8 / 128 / 512. Next to it
the two-stage composition the package could already run: a torch gather + dequantisation of the named tokens to bf16 in
HBM, then flash_mla_sparse_fwd at d_qk 512 over the gathered rows. The two are timed interleaved; each figure is the
median of 5 device-event timings after 3 warm-up calls. GB/s counts the 584 cache bytes of every slot once."""
import os, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "sgl-kernel-xpu_amd", "python"))
import sgl_kernel

dev = "cuda"
H, TOPK = 64, 128
MAIN, EXTRA = (64, 256), (2048, 64)  # (pages, page size)


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


def make_cache(pages, ps, g):
    """random e4m3 bytes below 2.0, rope in [-1, 1), scale bytes 124..130, production page size in bytes"""
    pb = 576 * ps + -(-8 * ps // 576) * 576
    buf = torch.zeros(pages, pb, dtype=torch.uint8, device=dev)
    data = buf[:, :576 * ps].unflatten(1, (ps, 576))
    data[..., :448] = torch.randint(0, 0x40, (pages, ps, 448), device=dev, generator=g, dtype=torch.uint8)
    data[..., 448:] = (torch.rand(pages, ps, 64, device=dev, generator=g) * 2 - 1).to(torch.bfloat16).view(torch.uint8)
    buf[:, 576 * ps:584 * ps].unflatten(1, (ps, 8))[..., :7] = torch.randint(124, 131, (pages, ps, 7), device=dev, generator=g,
                                                                             dtype=torch.uint8)
    return buf


def gather_dequant(buf, ps, idx):
    """bf16 [n, 512]: the rows of the tokens idx (int64 [n]) names"""
    data = buf[:, :576 * ps].unflatten(1, (ps, 576))[idx // ps, idx % ps]
    scale = (buf[:, 576 * ps:584 * ps].unflatten(1, (ps, 8))[idx // ps, idx % ps][:, :7].int() << 23).view(torch.float32)
    nope = data[:, :448].contiguous().view(torch.float8_e4m3fn).float().view(-1, 7, 64) * scale[..., None]
    return torch.cat([nope.view(-1, 448).to(torch.bfloat16), data[:, 448:].contiguous().view(torch.bfloat16)], 1)


def case(B, extra_topk):
    g = torch.Generator(device=dev).manual_seed(B + extra_topk)
    q = torch.randn(B, 1, H, 512, device=dev, dtype=torch.bfloat16, generator=g)
    bufs = [make_cache(*MAIN, g), make_cache(*EXTRA, g)]
    view = lambda buf, ps: buf.view(torch.float8_e4m3fn).as_strided((buf.shape[0], ps, 1, 584), (buf.shape[1], 576, 576, 1))
    idx = torch.randint(0, MAIN[0] * MAIN[1], (B, 1, TOPK), device=dev, generator=g, dtype=torch.int32)
    eidx = torch.randint(0, EXTRA[0] * EXTRA[1], (B, 1, extra_topk), device=dev, generator=g, dtype=torch.int32)
    slots = TOPK + extra_topk
    fused = lambda: sgl_kernel.flash_mla_with_kvcache(q, view(bufs[0], MAIN[1]), softmax_scale=0.09, is_fp8_kvcache=True,
                                                      indices=idx, extra_k_cache=view(bufs[1], EXTRA[1]),
                                                      extra_indices_in_kvcache=eidx)
    where = torch.arange(B * slots, device=dev, dtype=torch.int32).view(B, 1, slots)

    def two_stage():
        kv = torch.cat([gather_dequant(bufs[0], MAIN[1], idx.view(B, TOPK).long().flatten()).view(B, TOPK, 512),
                        gather_dequant(bufs[1], EXTRA[1], eidx.view(B, extra_topk).long().flatten()).view(B, extra_topk, 512)], 1)
        return sgl_kernel.flash_mla_sparse_fwd(q.view(B, H, 512), kv.view(B * slots, 1, 512), where, 0.09)

    a, b = fused()[0], two_stage()[0].view(B, 1, H, 512)
    err = (a.float() - b.float()).abs().max().item()
    ms_f, ms_t = median_ms(fused), median_ms(two_stage)
    gb = B * slots * 584 / 1e6
    print(f"B={B} extra_topk={extra_topk}: fused {ms_f * 1e3:.1f} us ({gb / ms_f:.0f} GB/s)  two-stage {ms_t * 1e3:.1f} us "
          f"({gb / ms_t:.0f} GB/s)  ratio {ms_f / ms_t:.3f}  max |diff| {err:.3g}", flush=True)


for extra_topk in (512, 8256):
    for B in (1, 8, 128, 512):
        case(B, extra_topk)
