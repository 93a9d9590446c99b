"""fp8_mqa_logits / fp8_paged_mqa_logits against the torch composition a user has without them: a bf16 matmul over all
heads (e4m3 is exact in bf16; the scores come back rounded to bf16, hence the loose sanity check), relu, weight, head sum, scale and mask - for the paged form
behind a gather of the cache rows. Graph-timed as tools/moe_fp8_sweep.py (warm-up, median of three replays), op and
composition alternating in one process; prints microseconds, the FLOP rate as a fraction of 5 PFLOP/s, for the paged
form the cache bytes over the time as a fraction of 8 TB/s, and the ratio composition / op. A graph replays the same
cache: a paged point whose cache is below 512 MB (twice the 256 MB of infinity cache) is marked `*` - its bytes come from
cache, its figure is no HBM figure.

  python tools/mqa_logits_sweep.py [--only ragged|paged]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "sgl-kernel-xpu_amd", "python"))
import sgl_kernel  # noqa: E402

dev = "cuda"
FP8 = torch.float8_e4m3fn
H, D = 64, 128


def timeit(f, it):
    for _ in range(2): f()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for _ in range(it): f()
    torch.cuda.current_stream().wait_stream(side)
    g.replay(); torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record(); g.replay(); en.record(); torch.cuda.synchronize()
        ts.append(st.elapsed_time(en) / it * 1e3)
    return sorted(ts)[1]


def fp8_rand(*shape):
    return (torch.randn(*shape, device=dev, dtype=torch.bfloat16) * 100).clamp_(-448, 448).to(FP8)


def compose(q, k, k_scale, w, ks, ke):
    """(Nq, H, D) x (Nk, D): the whole (Nq * H, Nk) score tensor, then five passes over it"""
    Nq, Nk = q.shape[0], k.shape[0]
    s = (q.view(Nq * H, D).to(torch.bfloat16) @ k.to(torch.bfloat16).t()).float().view(Nq, H, Nk)
    out = (s.relu_() * w[:, :, None]).sum(1) * k_scale[None]
    j = torch.arange(Nk, device=dev, dtype=torch.int32)[None]
    return out * ((j >= ks[:, None]) & (j < ke[:, None]))


def ragged_point(Nq, Nk, causal):
    q, k = fp8_rand(Nq, H, D), fp8_rand(Nk, D)
    k_scale, w = torch.rand(Nk, device=dev) + 0.5, torch.randn(Nq, H, device=dev)
    ks = torch.zeros(Nq, dtype=torch.int32, device=dev)
    ke = (torch.arange(1, Nq + 1, device=dev) * Nk // Nq).to(torch.int32) if causal else torch.full_like(ks, Nk)
    op = lambda: sgl_kernel.fp8_mqa_logits(q, (k, k_scale), w, ks, ke)  # noqa: E731
    ref = lambda: compose(q, k, k_scale, w, ks, ke)  # noqa: E731
    torch.testing.assert_close(op(), ref(), rtol=2e-2, atol=2e-2 * float(ref().abs().max()))
    it = max(2, min(20, int(2e11 / (Nq * Nk * H))))
    t_op, t_ref = [], []
    for _ in range(2):
        t_op.append(timeit(op, it)); t_ref.append(timeit(ref, it))
    us, cu = min(t_op), min(t_ref)
    flop = 2.0 * H * D * float(ke.sum())
    return us, cu, flop / (us * 1e-6) / 5e15


def paged_point(B, seq, block, page=64):
    pages = B * seq // page
    cache = torch.empty(pages, page, 1, D + 4, dtype=torch.uint8, device=dev)
    keys, scales = fp8_rand(pages, page, D).view(torch.uint8), (torch.rand(pages, page, 1, device=dev) + 0.5)
    if block:
        flat = cache.view(pages, page * (D + 4))
        flat[:, :page * D] = keys.view(pages, page * D)
        flat[:, page * D:] = scales.view(pages, page).contiguous().view(torch.uint8).view(pages, page * 4)
    else:
        cache.view(pages, page, D + 4)[:, :, :D] = keys
        cache.view(pages, page, D + 4)[:, :, D:] = scales.view(torch.uint8).view(pages, page, 4)
    q, w = fp8_rand(B, 1, H, D), torch.randn(B, H, device=dev)
    table = torch.randperm(pages, device=dev).view(B, seq // page).to(torch.int32)
    seq_lens = torch.full((B,), seq, dtype=torch.int32, device=dev)
    fn = sgl_kernel.fp8_paged_mqa_logits_triton if block else sgl_kernel.fp8_paged_mqa_logits
    op = lambda: fn(q, cache, w, seq_lens, table, None, seq)  # noqa: E731

    def ref():
        g = cache.view(pages, page * (D + 4))[table.long()]  # (B, pages per sequence, page bytes): the gather
        if block:
            kk, sc = g[:, :, :page * D].reshape(B, seq, D), g[:, :, page * D:].reshape(B, seq, 4)
        else:
            g = g.view(B, seq, D + 4)
            kk, sc = g[:, :, :D], g[:, :, D:]
        sc = sc.contiguous().view(torch.float32).view(B, seq)
        s = torch.bmm(q.view(B, H, D).to(torch.bfloat16), kk.contiguous().view(FP8).to(torch.bfloat16).transpose(1, 2)).float()
        return (s.relu_() * w[:, :, None]).sum(1) * sc

    torch.testing.assert_close(op(), ref(), rtol=2e-2, atol=2e-2 * float(ref().abs().max()))
    it = max(2, min(20, int(3e9 / (B * seq * H))))
    t_op, t_ref = [], []
    for _ in range(2):
        t_op.append(timeit(op, it)); t_ref.append(timeit(ref, it))
    us, cu = min(t_op), min(t_ref)
    return us, cu, 2.0 * H * D * B * seq / (us * 1e-6) / 5e15, B * seq * (D + 4) / (us * 1e-6) / 8e12


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    if args.only != "paged":
        print("%-7s %5s %6s %-7s %10s %10s %7s %6s" % ("form", "Nq", "Nk", "window", "op us", "torch us", "of 5PF", "ratio"))
        for Nq in (128, 1024, 4096):
            for Nk in (4096, 32768):
                for causal in (True, False):
                    us, cu, fl = ragged_point(Nq, Nk, causal)
                    print("%-7s %5d %6d %-7s %10.1f %10.1f %7.3f %6.2f" % ("ragged", Nq, Nk, "causal" if causal else "full", us, cu, fl, cu / us), flush=True)
    if args.only != "ragged":
        print("%-7s %5s %6s %-7s %10s %10s %7s %8s %6s" % ("form", "B", "seq", "layout", "op us", "torch us", "of 5PF", "of 8TB/s", "ratio"))
        for B in (1, 16, 128):
            for seq in (4096, 65536):
                for block in (False, True):
                    us, cu, fl, bw = paged_point(B, seq, block)
                    mark = "*" if B * seq * (D + 4) < 512e6 else " "
                    print("%-7s %5d %6d %-7s %10.1f %10.1f %7.3f %7.3f%s %6.2f" % ("paged", B, seq, "block" if block else "row", us, cu, fl, bw, mark, cu / us), flush=True)
