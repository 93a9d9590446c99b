"""The indexer top-k (csrc/topk_select.hip) against the torch composition a user has without it: mask the scores to the
window, torch.topk(k = 2048, sorted=False), map the indices. Graph-timed as tools/mqa_logits_sweep.py (warm-up, median of
three replays, op and composition alternating in one process, the better of two rounds); prints microseconds, the bytes of
ONE pass over the windows over the op's whole time as a fraction of 8 TB/s (the op reads a long row twice, the second time
from cache, so this understates the first pass), and the ratio composition / op.

  python tools/topk_sweep.py [--only grid|epilogues|indexer]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "sgl-kernel-xpu_amd", "python"))
import sgl_kernel  # noqa: E402

dev = "cuda"
K = 2048


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


def compose_raw(score, lengths):
    j = torch.arange(score.shape[1], device=dev, dtype=torch.int32)[None]
    return torch.topk(score.masked_fill(j >= lengths[:, None], float("-inf")), K, dim=1, sorted=False).indices


def measure(op, ref, elems):
    it = max(2, min(50, int(3e8 / elems)))
    t_op, t_ref = [], []
    for _ in range(2):
        t_op.append(timeit(op, it)); t_ref.append(timeit(ref, max(2, it // 8)))
    return min(t_op), min(t_ref)


def same_values(score, a, b):
    va, vb = torch.gather(score, 1, a.long()).sort(dim=1).values, torch.gather(score, 1, b.long()).sort(dim=1).values
    assert torch.equal(va, vb), "the op and torch.topk select different values"


def line(name, B, L, us, cu):
    print("%-26s %5d %7d %10.1f %10.1f %8.3f %7.1f" % (name, B, L, us, cu, B * L * 4 / (us * 1e-6) / 8e12, cu / us), flush=True)


def grid():
    for B in (1, 32, 128, 4096):
        for L in (4096, 16384, 32768, 131072):
            if B == 4096 and L > 32768:
                continue
            score = torch.randn(B, L, device=dev)
            lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
            op = lambda: sgl_kernel.fast_topk_v2(score, lengths, K)  # noqa: E731
            ref = lambda: compose_raw(score, lengths)  # noqa: E731
            same_values(score, op(), ref())
            line("fast_topk_v2", B, L, *measure(op, ref, B * L))


def epilogues(B=128, L=32768, page=64):
    score = torch.randn(B, L, device=dev)
    lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
    table1 = torch.stack([torch.randperm(L, device=dev) for _ in range(B)]).to(torch.int32)
    cu = torch.arange(B + 1, dtype=torch.int32, device=dev)
    off = torch.arange(B, dtype=torch.int32, device=dev) * L
    pages = torch.randperm(B * L // page, device=dev).view(B, L // page).to(torch.int32)
    out = torch.empty(B, K, dtype=torch.int32, device=dev)
    cases = {
        "fast_topk_v2": (lambda: sgl_kernel.fast_topk_v2(score, lengths, K), lambda: compose_raw(score, lengths)),
        "transform_fused": (lambda: sgl_kernel.fast_topk_transform_fused(score, lengths, table1, cu, K),
                            lambda: torch.gather(table1, 1, compose_raw(score, lengths))),
        "transform_ragged_fused": (lambda: sgl_kernel.fast_topk_transform_ragged_fused(score, lengths, off, K),
                                   lambda: compose_raw(score, lengths).to(torch.int32) + off[:, None]),
        "topk_transform_512": (lambda: sgl_kernel.topk_transform_512(score, lengths, pages, out, page),
                               lambda: torch.gather(pages, 1, compose_raw(score, lengths) // page) * page
                               + compose_raw(score, lengths) % page),
    }
    for name, (op, ref) in cases.items():
        line(name, B, L, *measure(op, ref, B * L))


def indexer(Nq=1024, Nk=32768, H=64, D=128):
    FP8 = torch.float8_e4m3fn
    q = (torch.randn(Nq, H, D, device=dev, dtype=torch.bfloat16) * 100).clamp_(-448, 448).to(FP8)
    k = (torch.randn(Nk, D, device=dev, dtype=torch.bfloat16) * 100).clamp_(-448, 448).to(FP8)
    k_scale, w = torch.rand(Nk, device=dev) + 0.5, torch.randn(Nq, H, device=dev).abs()
    ks = torch.zeros(Nq, dtype=torch.int32, device=dev)
    lengths = torch.full((Nq,), Nk, dtype=torch.int32, device=dev)
    off = torch.zeros(Nq, dtype=torch.int32, device=dev)
    real = sgl_kernel.fp8_mqa_logits(q, (k, k_scale), w, ks, lengths)
    for name, score in (("indexer scores", real), ("random normal", torch.randn(Nq, Nk, device=dev))):
        op = lambda: sgl_kernel.fast_topk_transform_ragged_fused(score, lengths, off, K, ks)  # noqa: E731
        ref = lambda: compose_raw(score, lengths).to(torch.int32) + off[:, None]  # noqa: E731
        same_values(score, op(), ref())
        line(name, Nq, Nk, *measure(op, ref, Nq * Nk))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    print("%-26s %5s %7s %10s %10s %8s %7s" % ("case", "B", "len", "op us", "torch us", "of 8TB/s", "ratio"))
    for part in (grid, epilogues, indexer):
        if args.only in ("", part.__name__):
            part()
