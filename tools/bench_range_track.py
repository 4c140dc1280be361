#!/usr/bin/env python3
"""One no-grad forward of an initialised activation quantiser (UniformAffineQuantizer.forward) with engine.FUSED_RANGE_TRACK off
and on, tracking its range (running_stat: act_momentum_update + the simulation) and plain (the simulation alone), on SD-sized
tensors:

    softmax128x4096x77      the cross-attention map of `--rs_sm_only`, 16 bit, always_zero
    a16x320x64x64           an activation, 8 bit
    a16x160of320x64x64      its channel slice x[:, :160], read in place as 16 strided rows
    selfattn128x4096x4096   the 2^31-element self-attention map, 16 bit, always_zero: ONE call per window

The knob is alternated off / on three times in ONE process after a warm-up of each side; a window is `--iters` forwards between
two device events.  Per side the best window and the spread of the three are printed, then whether both sides returned the
same y and the same state bit for bit — at the 2^31 elements that is the only check of the 64-bit indexing at full size.  GPU box:

    python tools/bench_range_track.py [--iters 10] [--shapes a,b]

--rehearse runs the composition once on tiny tensors on the CPU (shapes and plumbing only: it prints no time)."""
import argparse
import copy
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-diffusion_amd"))
from qdiff import engine  # noqa: E402
from qdiff.quant_layer import UniformAffineQuantizer  # noqa: E402

# (name, shape, channel slice or None, bits, always_zero, calls per window or None = --iters, tiny shape)
SHAPES = [("softmax128x4096x77", (128, 4096, 77), None, 16, True, None, (2, 16, 7)),
          ("a16x320x64x64", (16, 320, 64, 64), None, 8, False, None, (2, 8, 4, 4)),
          ("a16x160of320x64x64", (16, 320, 64, 64), 160, 8, False, None, (2, 8, 4, 4)),
          ("selfattn128x4096x4096", (128, 4096, 4096), None, 16, True, 1, (2, 8, 8))]


def make(shape, cut, softmax, dev):
    g = torch.Generator(device=dev).manual_seed(17)
    x = torch.rand(shape, generator=g, device=dev)
    x = torch.softmax(x.mul_(6), dim=-1) if softmax else x.mul_(8).sub_(3)
    return x if cut is None else x[:, :cut]


def quantizer(x, bits, always_zero):
    q = UniformAffineQuantizer(n_bits=bits, scale_method='max', leaf_param=True, always_zero=always_zero)
    with torch.no_grad():
        q(x[:1])                                                    # initialise from a part: the range then moves
    return q


def forward(q, x, fused):
    engine.set_fused_range_track(fused)
    try:
        with torch.no_grad():
            return q(x)
    finally:
        engine.set_fused_range_track(False)


def same_bits(a, b):
    if not torch.is_tensor(a):
        return type(a) is type(b) and a == b
    return torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    chosen = [s for s in SHAPES if s[0] in a.shapes.split(",")]
    if a.rehearse:
        for name, _, cut, bits, az, _, tiny in chosen:
            x = make(tiny, None if cut is None else tiny[1] // 2, az, torch.device("cpu"))
            q = quantizer(x, bits, az)
            q.running_stat = True
            print(f"{name}: rehearsal at {tuple(x.shape)}, y {tuple(forward(q, x, False).shape)} (no timing on the CPU)")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_range_track.py measures on the GPU: no device visible")
    dev = torch.device("cuda:0")
    print(f"# one no-grad quantiser forward, knob alternated off/on x3 in one process after one warm-up forward per side; "
          f"device events; {torch.cuda.get_device_name(0)}")
    for name, shape, cut, bits, az, calls, _ in chosen:
        x = make(shape, cut, az, dev)
        calls = calls or a.iters
        print(f"{name}: {x.numel() / 1e6:.2f} M elements, {bits} bit{', always_zero' if az else ''}, {calls} forward(s) per window")
        for tracking in (True, False):
            qs = {}
            for fused in (False, True):                             # the equality check doubles as the warm-up of each side
                qs[fused] = quantizer(x, bits, az)
                qs[fused].running_stat = tracking
            y_off = forward(qs[False], x, False)
            y_on = forward(qs[True], x, True)
            same = same_bits(y_on, y_off) and all(same_bits(getattr(qs[True], n), getattr(qs[False], n))
                                                  for n in ("x_min", "x_max", "delta", "zero_point"))
            del y_off, y_on
            ms = {False: [], True: []}
            for rep in range(3):
                for fused in (False, True):
                    q = copy.deepcopy(qs[fused])
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        forward(q, x, fused)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[fused].append(e0.elapsed_time(e1) / calls)
            off, on = ms[False], ms[True]
            gbs = x.numel() * (12 if tracking else 8) / min(on) / 1e6
            print(f"  {'tracking' if tracking else 'plain   '}  off: best {min(off):9.3f} ms (spread {max(off) - min(off):.3f})   "
                  f"on: best {min(on):9.3f} ms (spread {max(on) - min(on):.3f})   off / on = {min(off) / min(on):.2f}x   "
                  f"on side: {gbs:.0f} GB/s of the {12 if tracking else 8} B/element it must move   bit-identical y and state: {same}")
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
