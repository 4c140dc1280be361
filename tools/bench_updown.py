#!/usr/bin/env python3
"""A/B of engine.FUSE_UPDOWN on the LSUN-Churches LDM-8 UNet bench.py --model churches measures, in one process:

  eval   ms per UNet evaluation under HIP-graph replay at the benchmark's batch, knob off / on alternated, three windows a side;
  heads  GPU time of what stands between an `updown` block's input and its first convolution (conv1's int8 rows and the
         resampled skip rows), per block at the shapes the evaluation hands it, default route vs the one-launch producer; the
         stream is parked behind a spin kernel while the host enqueues, so the event interval is kernel time, not launch latency.
         Both sides compute their own statistics pass (no producer partial sums), and the default side of an up block includes
         the copy that replicates the codes, which the fused route leaves to the convolution's gather.

Prints plain lines; profiles/updown_fused.txt holds one run's."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "q-diffusion_amd"))
import bench  # noqa: E402
from qdiff import engine, quant_block as qb  # noqa: E402


def gpu_us(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    torch.cuda._sleep(int(2e8))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def head_default(p, x):
    """The lines of quant_block._res_forward_int between the block's input and conv1 / the residual, knob off."""
    B, C, H, W = x.shape
    rows = qb._nhwc_rows(x)
    conv1 = p.conv1
    if p.mode == 1:
        y = engine.groupnorm_silu_quant(rows, B, H * W, C, p.norm1, True, want_float=True)[1]
        hp = qb._nhwc_rows(p.block.h_upd(qb._rows_to_nchw(y, B, H, W)))
        xq = engine.quantize_rows(hp, conv1.conv_plan(), 1, C, B * H * W // 4, (0, 1, hp.stride(0)))
    else:
        xq = qb._rep2x(qb._gn_silu_to(conv1, rows, B, H * W, C, p.norm1), B, H, W)
    return xq, qb._nhwc_rows(p.block.x_upd(x))


def head_fused(p, x):
    B, C, H, W = x.shape
    return engine.groupnorm_resample_quant(qb._nhwc_rows(x), B, H, W, C, p.norm1, p.conv1.conv_plan(), p.mode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--evals", type=int, default=40, help="evaluations per timed window")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    qnn, _ = bench.build_quantised_unet("churches", dev)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(a.batch, 4, 32, 32, device=dev, generator=g)
    t = torch.full((a.batch,), 500, device=dev, dtype=torch.long)
    seen = {}
    blocks = [m for m in qnn.modules() if isinstance(m, qb.QuantResBlock) and m.updown]
    hooks = [b.register_forward_pre_hook(lambda m, args: seen.__setitem__(m, args[0].clone())) for b in blocks]
    outs = {}
    with torch.no_grad():
        qnn.enable_hip_graphs(False)
        qnn(x, t)                                 # the inputs of the updown blocks, for the heads below
        for h in hooks:
            h.remove()
        for on in (False, True):
            engine.set_fused_updown(on)
            before = dict(engine.UPDOWN_FUSED)
            outs[on] = qnn(x, t).clone()
            print(f"knob {'on ' if on else 'off'}: producer launches in one evaluation {[engine.UPDOWN_FUSED[k] - before[k] for k in ('down', 'up')]}"
                  f" of {len(blocks)} updown blocks")
        d = (outs[True] - outs[False]).abs().max().item()
        print(f"output on vs off: max|diff| {d:.3e} = {d / outs[False].abs().max().item():.2e} of range")
        # ---- whole evaluation, graph replay -------------------------------------------------------------------------------
        qnn.enable_hip_graphs(True)
        for on in (False, True):
            engine.set_fused_updown(on)
            for _ in range(4):                    # second sight captures; then replays
                qnn(x, t)
        torch.cuda.synchronize()
        win = {False: [], True: []}
        for w in range(3):
            for on in (False, True):
                engine.set_fused_updown(on)
                qnn(x, t)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.evals):
                    qnn(x, t)
                e1.record()
                torch.cuda.synchronize()
                win[on].append(e0.elapsed_time(e1) / a.evals)
                print(f"eval window {w} knob {'on ' if on else 'off'}: {win[on][-1]:.4f} ms per evaluation (batch {a.batch}, graph replay, {len(qnn._graphs)} graphs)")
        for on in (False, True):
            print(f"eval knob {'on ' if on else 'off'}: best {min(win[on]):.4f} ms, spread {max(win[on]) - min(win[on]):.4f} ms")
        # ---- heads alone --------------------------------------------------------------------------------------------------
        qnn.enable_hip_graphs(False)
        engine.set_fused_updown(False)
        tot = {False: 0.0, True: 0.0}
        for b in blocks:
            xin = seen[b]
            mode = 1 if hasattr(b.h_upd, "op") else 2
            p = qb._parts_of(b, b.in_layers[-1], b.out_layers[-1], mode)
            us = {False: gpu_us(lambda: head_default(p, xin)), True: gpu_us(lambda: head_fused(p, xin))}
            tot[False] += us[False]
            tot[True] += us[True]
            print(f"head {'down' if mode == 1 else 'up  '} {tuple(xin.shape)}: default {us[False]:7.1f} us, fused {us[True]:7.1f} us")
        print(f"heads total: default {tot[False]:.1f} us, fused {tot[True]:.1f} us per evaluation")


if __name__ == "__main__":
    main()
