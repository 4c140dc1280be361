#!/usr/bin/env python3
"""One weight-phase iteration of calibration (unit forward, ReconstructionObjective, backward, Adam step: the body of the loop
of qdiff/recon._reconstruct) with engine.FUSED_ADAROUND off and on, on SD-shaped units with random-init weights:

    res1280   a 1280-channel residual block at 16 x 16          (2 x 14.7 M weights + the embedding Linear)
    tran1280  a 1280-wide transformer block at 256 tokens, 77 context tokens of 768
    res320    a 320-channel residual block at 64 x 64

Batch 8 (the reference scripts' calibration batch).  The knob is alternated off / on three times in ONE process; per side the
best window and the spread of the three are printed, with the peak device memory of the side.  The objective is placed past its
warm-up (call 5000 of 20000: the regulariser is on, as in 80 % of the iterations).  GPU box:

    python tools/bench_adaround.py [--iters 100] [--units res1280,tran1280,res320]

--rehearse runs two knob-off iterations of tiny units on the CPU (shapes and plumbing only: it prints no time)."""
import argparse
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-diffusion_amd"))
import qdiff  # noqa: E402
from qdiff import engine, recon, synthetic  # noqa: E402
from qdiff.arch import ldm_unet  # noqa: E402

BATCH = 8


class _Holder(nn.Module):
    """What QuantModel wraps: one block (QuantModel turns it into its Quant* counterpart)."""

    def __init__(self, block, in_channels):
        super().__init__()
        self.block, self.in_channels = block, in_channels

    def forward(self, *args):
        return self.block(*args)


def make_unit(name, dev, tiny):
    """(QuantModel, unit, inputs) of one named unit; weights from qdiff.synthetic, inputs seeded."""
    g = torch.Generator().manual_seed(7)
    if name.startswith("res"):
        C, S = (1280, 16) if name == "res1280" else (320, 64)
        E = 1280
        if tiny:
            C, S, E = 32, 8, 64
        block = ldm_unet.ResBlock(C, E, 0, out_channels=C)
        args = [torch.randn(BATCH, C, S, S, generator=g), torch.randn(BATCH, E, generator=g)]
    elif name == "tran1280":
        C, H, T, ctx = (1280, 8, 256, 768) if not tiny else (64, 2, 16, 24)
        block = ldm_unet.BasicTransformerBlock(C, H, C // H, context_dim=ctx)
        args = [torch.randn(BATCH, T, C, generator=g), torch.randn(BATCH, 77 if not tiny else 5, ctx, generator=g)]
    else:
        raise SystemExit(f"unknown unit {name!r}")
    holder = _Holder(block, C)
    synthetic.load_synthetic_weights(holder, seed=3)
    wq = dict(n_bits=4, channel_wise=True, scale_method="max")
    aq = dict(n_bits=8, channel_wise=False, scale_method="max", leaf_param=True)
    qnn = qdiff.QuantModel(holder.to(dev).eval(), wq, aq, sm_abit=16).to(dev).eval()
    return qnn, qnn.model.block, [a.to(dev) for a in args]


def prepare(qnn, unit, args):
    """The state _reconstruct leaves before its loop: fp target, weight quantisers initialised, AdaRound with soft targets."""
    with torch.no_grad(), engine.simulation():
        qnn.set_quant_state(False, False)
        tgt = unit(*args)
        qnn.set_quant_state(True, False)
        unit(*args)
    mods = recon._quant_modules(unit)
    for m in mods:
        recon.to_adaround(m, layer_unit=False)
    params = []
    for m in mods:
        params.append(m.weight_quantizer.alpha)
        if m.split != 0:
            params.append(m.weight_quantizer_0.alpha)
    return tgt, params


def iterations(unit, args, tgt, params, n, fused):
    """n iterations of the weight phase from a fresh optimiser and objective; returns the last loss (a device tensor)."""
    engine.set_fused_adaround(fused)
    opt = torch.optim.Adam(params)
    obj = recon.ReconstructionObjective(unit, 20000, weight=0.01, b_range=(20, 2), warmup=0.2)
    obj.calls = 5000
    try:
        with engine.simulation():
            for _ in range(n):
                opt.zero_grad()
                if fused:
                    obj.arm()
                try:
                    err = obj(unit(*args), tgt)
                finally:
                    if fused:
                        obj.disarm()
                err.backward()
                opt.step()
    finally:
        engine.set_fused_adaround(False)
    return err.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--units", default="res1280,tran1280,res320")
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        for name in a.units.split(","):
            qnn, unit, args = make_unit(name, torch.device("cpu"), tiny=True)
            tgt, params = prepare(qnn, unit, args)
            loss = iterations(unit, args, tgt, params, 2, fused=False)
            print(f"{name}: rehearsal, {sum(p.numel() for p in params)} rounding variables in {len(params)} quantisers, loss {float(loss):.4f} (no timing on the CPU)")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_adaround.py measures on the GPU: no device visible")
    dev = torch.device("cuda:0")
    print(f"# weight-phase iteration (forward, objective, backward, Adam), batch {BATCH}, {a.iters} iterations per window after {a.warmup} "
          f"warm-up, knob alternated off/on x3 in one process; device events; {torch.cuda.get_device_name(0)}")
    for name in a.units.split(","):
        qnn, unit, args = make_unit(name, dev, tiny=False)
        tgt, params = prepare(qnn, unit, args)
        init = [p.detach().clone() for p in params]
        nw = sum(p.numel() for p in params)
        ms, peak, loss = {False: [], True: []}, {False: 0, True: 0}, {}
        for rep in range(3):
            for fused in (False, True):
                with torch.no_grad():
                    for p, p0 in zip(params, init):
                        p.copy_(p0)
                        p.grad = None
                iterations(unit, args, tgt, params, a.warmup, fused)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                n0 = engine.ADAROUND_LAUNCHES[0]
                e0.record()
                loss[fused] = iterations(unit, args, tgt, params, a.iters, fused)
                e1.record()
                torch.cuda.synchronize()
                ms[fused].append(e0.elapsed_time(e1) / a.iters)
                peak[fused] = max(peak[fused], torch.cuda.max_memory_allocated())
                launches = (engine.ADAROUND_LAUNCHES[0] - n0) / a.iters
        off, on = ms[False], ms[True]
        print(f"{name}: {nw / 1e6:.1f} M rounding variables in {len(params)} quantisers")
        print(f"  off: best {min(off):8.3f} ms  (three windows {', '.join(f'{v:.3f}' for v in off)}; spread {max(off) - min(off):.3f})  "
              f"peak {peak[False] / 2**20:8.0f} MiB  loss {float(loss[False]):.6f}")
        print(f"  on : best {min(on):8.3f} ms  (three windows {', '.join(f'{v:.3f}' for v in on)}; spread {max(on) - min(on):.3f})  "
              f"peak {peak[True] / 2**20:8.0f} MiB  loss {float(loss[True]):.6f}  adaround launches / iteration {launches:.0f}")
        print(f"  off / on = {min(off) / min(on):.3f}x, difference {min(off) - min(on):+.3f} ms against an off-side spread of {max(off) - min(off):.3f} ms")
        del qnn, unit, args, tgt, params, init
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
