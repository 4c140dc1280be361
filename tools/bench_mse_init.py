#!/usr/bin/env python3
"""One 'mse' initialisation of a quantiser (UniformAffineQuantizer.init_quantization_scale, the LAPQ-style range search) with
engine.FUSED_MSE_INIT off and on, on SD-sized tensors:

    weights      (320, 320, 3, 3)   (1280, 2560, 3, 3)   (10240, 1280)         channel-wise, 4 bit
    activations  (16, 320, 64, 64)  (16, 1280, 8, 8)                           whole tensor, 8 bit
    softmax      (128, 4096, 77)                                               whole tensor, 16 bit, always_zero

The knob is alternated off / on three times in ONE process after a warm-up of each side; a window is `--iters` searches between
two device events (the scalar composition synchronises 80 times per search by itself: that is part of what it costs).  Per side
the best window and the spread of the three are printed, then the ATen operator calls of one search on each side (counted by a
dispatch mode: every one of the composition's is at least one launch; the fused side's are allocations and views, its kernel
launches are the library's: 1 in the row form, 3 in the spread form) and whether both sides returned the same
(delta, zero_point).  --accuracy then prints the score errors and pick differences that the judge of
tests/mse_init_cases.py measures on the test cases.  GPU box:

    python tools/bench_mse_init.py [--iters 3] [--accuracy]

--rehearse runs the composition once on tiny tensors on the CPU (shapes and plumbing only: it prints no time)."""
import argparse
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-diffusion_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from qdiff import engine, hip  # noqa: E402
from qdiff.quant_layer import UniformAffineQuantizer  # noqa: E402

# (name, kind, shape, bits, always_zero, tiny shape)
SHAPES = [("w320x320x3x3", "weight", (320, 320, 3, 3), 4, False, (8, 8, 3, 3)),
          ("w1280x2560x3x3", "weight", (1280, 2560, 3, 3), 4, False, (4, 16, 3, 3)),
          ("w10240x1280", "weight", (10240, 1280), 4, False, (32, 24)),
          ("a16x320x64x64", "act", (16, 320, 64, 64), 8, False, (2, 8, 8, 8)),
          ("a16x1280x8x8", "act", (16, 1280, 8, 8), 8, False, (2, 16, 4, 4)),
          ("softmax128x4096x77", "softmax", (128, 4096, 77), 16, True, (2, 16, 7))]


class _Count(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def make(kind, shape, dev):
    g = torch.Generator().manual_seed(17)
    if kind == "weight":
        x = torch.randn(shape, generator=g) * torch.rand(shape[0], *([1] * (len(shape) - 1)), generator=g)
    elif kind == "act":
        x = torch.randn(shape, generator=g)
        x = torch.where(torch.rand(shape, generator=g) < 1e-3, x * 20, x)
    else:
        x = torch.softmax(torch.randn(shape, generator=g) * 3, dim=-1)
    return x.to(dev)


def search(x, kind, bits, always_zero, fused):
    q = UniformAffineQuantizer(n_bits=bits, channel_wise=kind == "weight", scale_method="mse", always_zero=always_zero)
    engine.set_fused_mse_init(fused)
    try:
        return q.init_quantization_scale(x, q.channel_wise)
    finally:
        engine.set_fused_mse_init(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    chosen = [s for s in SHAPES if s[0] in a.shapes.split(",")]
    if a.rehearse:
        for name, kind, _, bits, az, tiny in chosen:
            d, z = search(make(kind, tiny, torch.device("cpu")), kind, bits, az, fused=False)
            print(f"{name}: rehearsal at {tiny}, delta {tuple(d.shape)} (no timing on the CPU)")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_mse_init.py measures on the GPU: no device visible")
    dev = torch.device("cuda:0")
    print(f"# one 'mse' quantiser initialisation, {a.iters} searches per window after one warm-up search per side, knob alternated "
          f"off/on x3 in one process; device events; {torch.cuda.get_device_name(0)}")
    for name, kind, shape, bits, az, _ in chosen:
        x = make(kind, shape, dev)
        res, ops = {}, {}
        for fused in (False, True):
            res[fused] = search(x, kind, bits, az, fused)                   # warm-up of the side, and its result
            with _Count() as c:
                search(x, kind, bits, az, fused)
            ops[fused] = c.n
        ms = {False: [], True: []}
        for rep in range(3):
            for fused in (False, True):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    search(x, kind, bits, az, fused)
                e1.record()
                torch.cuda.synchronize()
                ms[fused].append(e0.elapsed_time(e1) / a.iters)
        rows, cols, _ = hip.adaround_rows(x)
        form = hip.mse_search_form(rows, cols, kind == "weight")
        same_d = (res[True][0] == res[False][0]).flatten()
        z_on, z_off = res[True][1], res[False][1]
        same_z = (z_on == z_off).flatten() if torch.is_tensor(z_on) else torch.tensor([z_on == z_off])
        off, on = ms[False], ms[True]
        print(f"{name}: {x.numel() / 1e6:.2f} M elements, {bits} bit, {'per row' if kind == 'weight' else 'whole tensor'}, "
              f"launch form {('row/wave', 'row/block', 'spread')[form]} = {3 if form == hip.MSE_FORM_SPREAD else 1} kernel launch(es)")
        print(f"  off: best {min(off):10.3f} ms  (three windows {', '.join(f'{v:.3f}' for v in off)}; spread {max(off) - min(off):.3f})  "
              f"ATen operator calls / search {ops[False]}")
        print(f"  on : best {min(on):10.3f} ms  (three windows {', '.join(f'{v:.3f}' for v in on)}; spread {max(on) - min(on):.3f})  "
              f"ATen operator calls / search {ops[True]}")
        print(f"  off / on = {min(off) / min(on):.1f}x;  same delta on {int(same_d.sum())} of {same_d.numel()} groups, "
              f"same zero point on {int(same_z.sum())} of {same_z.numel()}")
        del x, res
        torch.cuda.empty_cache()
    if a.accuracy:
        import mse_init_cases as mc
        print("# score error against fp64 and picks against the composition on the test cases (tests/mse_init_cases.py judge)")
        worst = dict(f=0.0, c=0.0, d=0)
        for case in mc.CASES:
            fig = mc.judge(case[1](dev), *case[2:], label=case[0])
            worst = dict(f=max(worst["f"], fig["err_fused"]), c=max(worst["c"], fig["err_composition"]), d=worst["d"] + fig["picks_differ"])
        print(f"# worst over the cases: fused {worst['f']:.3e}, composition {worst['c']:.3e}; picks differing from the composition: {worst['d']}")


if __name__ == "__main__":
    main()
