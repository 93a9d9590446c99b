"""fp8_blockwise_scaled_grouped_mm against the only thing the package could do before it: a Python loop of E dense
fp8_blockwise_scaled_mm calls on host-known row counts. Graph-timed as tools/row_sweep.py (warm-up, median of three replays
of 20 calls), the two alternating in one process; prints microseconds, the weight stream as a fraction of 8 TB/s, the FLOP
rate as a fraction of 5 PFLOP/s and the ratio loop / op per point.

  python tools/moe_fp8_sweep.py [--shapes ds,qwen] [--rows 1,4,16,...]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "sgl-kernel-xpu_amd", "python"))
import sgl_kernel  # noqa: E402

dev = "cuda"
FP8 = torch.float8_e4m3fn
SHAPES = {"ds": (32, [(4096, 7168), (7168, 2048)]), "qwen": (16, [(3072, 4096), (4096, 1536)])}


def timeit(f, it=20):
    for _ in range(3): f()
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
    return (torch.randn(*shape, device=dev, dtype=torch.bfloat16) * 100).to(FP8)


def point(E, N, K, rows, w, sw):
    total = sum(rows)
    offsets = [sum(rows[:e]) for e in range(E)]
    a = fp8_rand(max(total, 1), K)[:total]
    sa = (torch.rand(K // 128, total, device=dev) * 1e-3).t()  # column-major, as the group quant emits it
    out = torch.empty(total, N, dtype=torch.bfloat16, device=dev)
    ps = torch.tensor([[r, N, K] for r in rows], dtype=torch.int32, device=dev)
    eo = torch.tensor(offsets, dtype=torch.int32, device=dev)
    scratch = torch.empty(E, dtype=torch.int64, device=dev)
    b, sb = w.transpose(1, 2), sw.transpose(1, 2)

    def op():
        sgl_kernel.fp8_blockwise_scaled_grouped_mm(out, scratch, scratch, scratch, scratch, scratch, a, b, sa, sb, scratch, scratch,
                                                   scratch, scratch, scratch, ps, eo, scratch)

    def loop():
        for e in range(E):
            if rows[e]:
                o = offsets[e]
                sgl_kernel.fp8_blockwise_scaled_mm(a[o:o + rows[e]], b[e], sa[o:o + rows[e]], sb[e], torch.bfloat16)

    t_op, t_loop = [], []
    for _ in range(2):
        t_op.append(timeit(op))
        t_loop.append(timeit(loop))
    us, lp = min(t_op), min(t_loop)
    live = sum(1 for r in rows if r)
    return us, lp, live * N * K / (us * 1e-6) / 8e12, 2.0 * sum(rows) * N * K / (us * 1e-6) / 5e15


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ds,qwen")
    ap.add_argument("--rows", default="1,4,16,32,64,128,256,512")
    args = ap.parse_args()
    print("%-5s %5s %5s %3s %-8s %9s %9s %8s %7s %6s" % ("model", "N", "K", "E", "rows", "op us", "loop us", "of 8TB/s", "of 5PF", "ratio"))
    for name in args.shapes.split(","):
        E, nks = SHAPES[name]
        for N, K in nks:
            w = torch.cat([fp8_rand(1, N, K) for _ in range(E)])
            sw = torch.rand(E, N // 128, K // 128, device=dev) * 1e-3
            lists = [(str(r), [r] * E) for r in map(int, args.rows.split(","))]
            lists.append(("skew32", [64 if e % 2 else 0 for e in range(E)]))  # half the experts empty, the rest twice the average
            for label, rows in lists:
                us, lp, bw, fl = point(E, N, K, rows, w, sw)
                print("%-5s %5d %5d %3d %-8s %9.1f %9.1f %8.3f %7.3f %6.2f" % (name, N, K, E, label, us, lp, bw, fl, lp / us), flush=True)
